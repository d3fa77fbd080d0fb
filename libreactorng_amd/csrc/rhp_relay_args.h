/*
 * rhp_relay_args.h -- the argument rules of rhp_relay_walked (rhp.h) and the
 * rule that decides which slot of a walk is relayed and how large its reply
 * is, one statement of them for the kernels and their launcher
 * (rhp_classify.hip) and the host twin (rhp_host.cpp rhp_cpu_relay_walked).
 * The batch's rules are rhp_walk_responses' (rhp_walk_args.h); the owner, the
 * in-use, the head and the inside tests are rhp_lookup_walked's
 * (rhp_lookup_args.h).
 */
#ifndef RHP_RELAY_ARGS_H
#define RHP_RELAY_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_walk_args.h"
#include "rhp_lookup_args.h"
#include "rhp_digits.h"

#define RHP_RELAY_HD RHP_LOOKUP_HD

/* 0: relay the slots; 1: out_off[0] = 0 and nothing else (no slot, or no
 * session to own one); -22: refused.  device_pointers adds the launcher's own
 * rules (rhp_walk_check's alignments; out_off and the plan in work are 8-byte
 * accesses, why a 4-byte store), which host callers, who pass any memory, leave
 * out. */
static inline int rhp_relay_check(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, int device_pointers)
{
  const int rc = rhp_walk_check(w, device_pointers);
  if (rc < 0) return rc;
  if (!r) return -22;
  if (!r->out_off || !r->why || !r->date || !r->work) return -22;
  if (r->date_len != RHP_DATE_LEN) return -22;
  if (r->n_names > RHP_RELAY_MAX_NAMES) return -22;
  if (r->n_names > 0 && (!r->text || !r->names)) return -22;
  for (uint32_t j = 0; j < r->n_names; j++)
    if (r->names[j].len == 0 || r->names[j].len > RHP_CLASSIFY_NAME_MAX) return -22;
  if (!r->out && r->out_size != 0) return -22;
  if (device_pointers && ((((uintptr_t) r->out_off | (uintptr_t) r->work) & 7u) != 0 || ((uintptr_t) r->why & 3u) != 0)) return -22;
  return rc == 1 || w->n_slots_total == 0 ? 1 : 0;
}

/* the three names that are always dropped; Content-Type's first value is the type */
#define RHP_RELAY_TYPE_NAME   "Content-Type"
#define RHP_RELAY_LENGTH_NAME "Content-Length"
#define RHP_RELAY_TE_NAME     "Transfer-Encoding"

/* where a body has to end: the readable end the walk clamps its sessions to, a
 * multiple of 16, so a body end rounded up to 4 is below it when the end is */
static inline uint64_t rhp_relay_readable(uint64_t bytes_size) { return rhp_walk_readable(bytes_size); }

/* The tests that need no header record, in rhp.h's order: 0, or the code of the
 * first that failed.  in_use false: nothing else was loaded and every other
 * argument is ignored.  k = i - slot_off[s], the slot's place in its session. */
RHP_RELAY_HD uint32_t rhp_relay_why_head(int in_use, int32_t slot_result, int32_t ret, uint64_t st, uint64_t a, uint64_t e,
                                         uint64_t head_readable, uint32_t status, uint32_t k, uint32_t n_slots, uint32_t stop)
{
  if (!in_use) return RHP_RELAY_UNUSED;
  if (!rhp_lookup_is_head(slot_result, ret)) return RHP_RELAY_NOT_HEAD;
  if (!rhp_lookup_inside(st, ret, a, e, head_readable)) return RHP_RELAY_OUTSIDE;
  if (status >= 100u && status <= 199u) return RHP_RELAY_INTERIM;
  if (k + 1u == n_slots && (stop == RHP_WALK_BODY || stop == RHP_WALK_CLOSE)) return RHP_RELAY_PARTIAL;
  return RHP_RELAY_OK;
}

/* a phrase, name or value [off, off + len) inside [0, ret), ret > 0 */
RHP_RELAY_HD int rhp_relay_span_inside(uint32_t off, uint32_t len, int32_t ret) { return off + len <= (uint32_t) ret; }

/* The tests behind the header records, for a head that passed the ones above
 * (so st + ret <= e): fold: a record with name_off == RHP_NAME_NULL was seen;
 * span_bad: a span that is not inside [0, ret) was */
RHP_RELAY_HD uint32_t rhp_relay_why_body(int fold, int span_bad, uint32_t body_kind, uint64_t body_len, uint64_t wire_len,
                                         uint32_t flags, uint64_t st, int32_t ret, uint64_t e, uint64_t readable)
{
  if (fold) return RHP_RELAY_FOLD;
  if (span_bad) return RHP_RELAY_SPAN;
  const int named = (body_len == 0 && wire_len == 0) || (body_kind == RHP_FRAME_LENGTH && wire_len == body_len) ||
                    (body_kind == RHP_FRAME_CHUNKED && (flags & RHP_WALK_DEFRAME) != 0);
  if (!named) return RHP_RELAY_FRAMING;
  if (body_len > 0xffffffffull) return RHP_RELAY_LONG;
  const uint64_t b = st + (uint64_t) (uint32_t) ret;   /* <= e */
  if (body_len > e - b || b > readable || body_len > readable - b) return RHP_RELAY_BODY_OUTSIDE;
  return RHP_RELAY_OK;
}

/* the status text: three digits and, with a phrase, one SP and the phrase */
RHP_RELAY_HD uint32_t rhp_relay_status_len(uint32_t msg_len) { return 3u + (msg_len ? 1u + msg_len : 0u); }

/* every byte of a reply except its variable parts: 9 + 2 + 11 + 37 + 16 + 18 +
 * 2 (http.c:244), then the variable parts but the fields */
RHP_RELAY_HD uint64_t rhp_relay_size_head(uint32_t msg_len, uint32_t type_len, uint32_t body_len)
{
  return 95u + (uint64_t) rhp_relay_status_len(msg_len) + type_len + rhp_u32_len(body_len) + body_len;
}

/* one kept field: name ": " value CRLF (http.c:272) */
RHP_RELAY_HD uint64_t rhp_relay_size_field(uint32_t name_len, uint32_t value_len) { return (uint64_t) name_len + 2u + value_len + 2u; }

#endif
