/*
 * rhp_chunked_args.h -- the argument rules of rhp_decode_chunked (rhp.h), one
 * statement of them for the kernel's launcher (rhp_chunked.hip) and the host
 * twin (rhp_host.cpp rhp_cpu_decode_chunked), and the test for a corrupt
 * decoder.
 */
#ifndef RHP_CHUNKED_ARGS_H
#define RHP_CHUNKED_ARGS_H

#include <stdint.h>
#include "rhp.h"

/* 0: decode the batch; 1: nothing to do (n == 0); -22: refused.  device_pointers
 * adds the launcher's own rules (decoders and results are whole 16-byte loads
 * and stores, the moves' 16-byte stores are counted from bytes), which host
 * callers, who pass any memory, leave out. */
static inline int rhp_chunked_batch_check(const rhp_chunked_batch_t *b, int device_pointers)
{
  if (!b) return -22;
  if (b->reserved != 0) return -22;
  if (b->n == 0) return 1;
  if (!b->bytes || !b->offsets || !b->decoders || !b->results) return -22;
  if (device_pointers && ((((uintptr_t) b->bytes | (uintptr_t) b->decoders | (uintptr_t) b->results) & 15u) != 0)) return -22;
  return 0;
}

/* a state or a digit count the reference cannot have left (rhp.h: ret -1, size 0, nothing touched) */
#define RHP_CHUNKED_CORRUPT(state, hex_count) ((state) > RHP_CHUNKED_IN_TRAILERS_LINE_MIDDLE || (hex_count) > 16u)

#endif
