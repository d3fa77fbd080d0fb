/*
 * rhp_msg_args.h -- the argument rules of rhp_parse_messages (rhp.h), one
 * statement of them for the kernel's launcher (rhp_messages.hip) and the host
 * twin (rhp_host.cpp rhp_cpu_parse_messages).  They are rhp_batch_check's
 * (rhp_records.h) for the fields the two batches share.
 */
#ifndef RHP_MSG_ARGS_H
#define RHP_MSG_ARGS_H

#include <stdint.h>
#include "rhp.h"

/* 0: parse the batch; 1: nothing to do (n == 0); -22: refused.  device_pointers
 * adds the launcher's own rules (the reader's lines are aligned 16-byte loads,
 * the records leave as whole 16- and 8-byte stores), which host callers, who
 * pass any memory, leave out. */
static inline int rhp_msg_batch_check(const rhp_msg_batch_t *b, int device_pointers)
{
  if (!b) return -22;
  if (b->kind != RHP_MSG_RESPONSE && b->kind != RHP_MSG_HEADERS) return -22;
  if (b->layout != RHP_LAYOUT_REQUEST_MAJOR && b->layout != RHP_LAYOUT_HEADER_MAJOR) return -22;
  if (b->max_headers > RHP_MAX_HEADERS) return -22;
  if ((uint64_t) b->n * b->max_headers > 0xffffffffull) return -22;   /* record indices are 32-bit */
  if (b->n == 0) return 1;
  if (!b->bytes || !b->offsets || !b->msgs) return -22;
  if (b->max_headers > 0 && !b->hdrs) return -22;
  if (b->bytes_size < RHP_PAD) return -22;   /* bytes_size >= offsets[n] + RHP_PAD */
  if (device_pointers && ((((uintptr_t) b->bytes | (uintptr_t) b->msgs) & 15u) != 0 || ((uintptr_t) b->hdrs & 7u) != 0)) return -22;
  return 0;
}

#endif
