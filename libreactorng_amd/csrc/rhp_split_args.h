/*
 * rhp_split_args.h -- the argument rules of rhp_split_sessions (rhp.h), one
 * statement of them for the kernels' launcher (rhp_split.hip) and the host
 * twin (rhp_host.cpp rhp_cpu_split_sessions).
 */
#ifndef RHP_SPLIT_ARGS_H
#define RHP_SPLIT_ARGS_H

#include <stdint.h>
#include "rhp.h"

#define RHP_SPLIT_LF 10u
#define RHP_SPLIT_CR 13u

/* 0: split; -22: refused */
static inline int rhp_split_sessions_check(const uint8_t *bytes, uint64_t bytes_end, const uint64_t *sess_off,
                                           uint32_t n_sessions, const rhp_split_out_t *o)
{
  if (!sess_off || !o) return -22;
  if (!o->n_pieces || !o->offsets || !o->work) return -22;
  if (n_sessions && !o->sessions) return -22;
  if (bytes_end && (!bytes || ((uintptr_t) bytes & 15u))) return -22;
  /* positions and piece indices are u32 on the device */
  if (bytes_end >= (1ull << 32) || bytes_end + n_sessions >= (1ull << 32)) return -22;
  return 0;
}

#endif
