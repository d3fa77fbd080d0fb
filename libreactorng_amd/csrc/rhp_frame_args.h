/*
 * rhp_frame_args.h -- the argument rules of rhp_frame_messages (rhp.h), one
 * statement of them for the kernel's launcher (rhp_classify.hip) and the host
 * twin (rhp_host.cpp rhp_cpu_frame_messages).  The batch's are
 * rhp_parse_messages' (rhp_msg_args.h), the names' rhp_classify_batch's.
 */
#ifndef RHP_FRAME_ARGS_H
#define RHP_FRAME_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_msg_args.h"

/* 0: frame the batch; 1: nothing to do (n == 0); -22: refused.  Framing only
 * reads the batch, and never last_len.  device_pointers adds the launcher's own
 * rules (a frame and an armed decoder leave as whole 16-byte stores), which host
 * callers, who pass any memory, leave out. */
static inline int rhp_frame_check(const rhp_msg_batch_t *b, const rhp_frame_args_t *f, int device_pointers)
{
  if (!b || !f) return -22;
  if (f->reserved != 0 || f->consume_trailer > 1u) return -22;
  if (f->n_names > RHP_CLASSIFY_MAX_NAMES) return -22;
  if (f->n_names && (!f->text || !f->names || !f->fields)) return -22;
  for (uint32_t j = 0; j < f->n_names; j++)
    if (f->names[j].len == 0 || f->names[j].len > RHP_CLASSIFY_NAME_MAX) return -22;
  rhp_msg_batch_t q = *b;
  q.last_len = NULL;
  const int rc = rhp_msg_batch_check(&q, device_pointers);
  if (rc != 0) return rc;
  if (!f->frames) return -22;
  if (device_pointers && ((((uintptr_t) f->frames | (uintptr_t) f->decoders) & 15u) != 0)) return -22;
  return 0;
}

/* where a message has to end for it to be read: bytes_size rounded down to whole
 * dwords (the bytes are read as the aligned dwords that hold them) */
static inline uint64_t rhp_frame_readable(const rhp_msg_batch_t *b) { return b->bytes_size & ~(uint64_t) 3; }

#endif
