/*
 * rhp_forward_args.h -- the argument rules of rhp_forward_sessions (rhp.h) and
 * the rule that decides which record slot of a round is forwarded and how large
 * its request is, one statement of them for the kernels and their launcher
 * (rhp_forward.hip) and the host twin (rhp_host.cpp rhp_cpu_forward_sessions).
 * The batch's rules are rhp_classify_sessions' (rhp_classify_args.h).
 */
#ifndef RHP_FORWARD_ARGS_H
#define RHP_FORWARD_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_records.h"
#include "rhp_digits.h"

#if defined(__HIPCC__)
#define RHP_FORWARD_HD __host__ __device__ __forceinline__
#else
#define RHP_FORWARD_HD static inline
#endif

/* 0: forward the slots; 1: out_off[0] = 0, fwd_off[0, n_sessions] = 0 and
 * nothing else (no slot, or no session to own one); -22: refused.
 * device_pointers adds the launcher's own rules (out_off, the counts and the
 * plan in work are 8-byte accesses; why, fwd_off and head_bits 4-byte ones),
 * which host callers, who pass any memory, leave out. */
static inline int rhp_forward_check(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                    const rhp_session_result_t *results, const uint64_t *req_start, const uint16_t *route,
                                    const rhp_forward_t *f, int device_pointers)
{
  if (!b || !route || !f) return -22;
  if (!f->out_off || !f->why || !f->fwd_off || !f->head_bits || !f->work) return -22;
  if (!f->out && f->out_size != 0) return -22;
  if (f->n_routes == 0 || f->n_routes > RHP_CLASSIFY_MAX_ROUTES) return -22;
  if (f->n_names > RHP_FORWARD_MAX_NAMES) return -22;
  if (f->n_names > 0 && (!f->text || !f->names)) return -22;
  for (uint32_t j = 0; j < f->n_names; j++)
    if (f->names[j].len == 0 || f->names[j].len > RHP_CLASSIFY_NAME_MAX) return -22;
  if (f->extra_len > RHP_FORWARD_EXTRA_MAX) return -22;
  if (f->extra_len > 0 && (!f->extra || f->extra_len < 2u || f->extra[f->extra_len - 2u] != '\r' || f->extra[f->extra_len - 1u] != '\n')) return -22;
  if (b->mode != RHP_MODE_HTTP || b->flags != RHP_BATCH_SPECULATIVE) return -22;
  if (n_sessions && (!sessions || !results || !req_start)) return -22;
  if (device_pointers && ((((uintptr_t) f->out_off | (uintptr_t) f->work) & 7u) != 0 ||
                          (((uintptr_t) f->why | (uintptr_t) f->fwd_off | (uintptr_t) f->head_bits) & 3u) != 0)) return -22;
  rhp_batch_t q = *b;   /* forwarding only reads, and never last_len (rhp_classify_args.h) */
  if (!q.bytes_rw) q.bytes_rw = (uint8_t *) q.bytes;
  q.last_len = NULL;
  const int rc = rhp_batch_check(&q, 1);
  if (rc < 0) return rc;
  return rc == 1 || n_sessions == 0 ? 1 : 0;
}

/* the two names that are always dropped: the framing is written anew */
#define RHP_FORWARD_LENGTH_NAME "Content-Length"
#define RHP_FORWARD_TE_NAME     "Transfer-Encoding"

/* where a request and its body have to end: names, values and bodies are read
 * as the aligned dwords that hold them, and an end at or below a multiple of 4
 * stays there when it is rounded up to 4 */
RHP_FORWARD_HD uint64_t rhp_forward_readable(uint64_t bytes_size) { return bytes_size & ~(uint64_t) 3u; }

/* In use: rhp_classify_sessions' test, the one that lets a load of slot i's
 * records through: session (lo, hi, n_slots) of a batch of n slots wrote slot i */
RHP_FORWARD_HD int rhp_forward_in_use(uint32_t i, uint32_t lo, uint32_t hi, uint32_t n_slots, uint32_t n)
{
  return lo <= i && i - lo < n_slots && lo <= hi && hi <= n;
}

/* the slot whose result says where an in-use slot's session stopped, or n when
 * the session's n_slots runs past the batch (no such record: not closed) */
RHP_FORWARD_HD uint32_t rhp_forward_last_slot(uint32_t lo, uint32_t n_slots, uint32_t n)
{
  const uint64_t last = (uint64_t) lo + n_slots - 1u;   /* (in use: n_slots >= 1) */
  return last < n ? (uint32_t) last : n;
}

/* The request [rs, rs + ret), ret > 0, inside the session's input [a, e) and the readable bytes */
RHP_FORWARD_HD int rhp_forward_inside(uint64_t rs, int32_t ret, uint64_t a, uint64_t e, uint64_t readable)
{
  const uint64_t r = (uint64_t) (uint32_t) ret;
  return rs >= a && rs <= e && r <= e - rs && rs <= readable && r <= readable - rs;
}

/* a method, path, name or value [off, off + len) inside [0, ret), ret > 0 */
RHP_FORWARD_HD int rhp_forward_span_inside(uint32_t off, uint32_t len, int32_t ret) { return off + len <= (uint32_t) ret; }

/* whether route r goes upstream */
RHP_FORWARD_HD int rhp_forward_route(uint32_t r, uint32_t n_routes, uint32_t forward_mask)
{
  return r < n_routes && ((forward_mask >> r) & 1u);
}

/* The tests behind the header records, for a request that passed the ones
 * before them (so rs + ret <= e and <= readable): fold: a record with name_off
 * == RHP_NAME_NULL was seen; span_bad: a span that is not inside [0, ret) was */
RHP_FORWARD_HD uint32_t rhp_forward_why_body(int fold, int span_bad, uint32_t body_kind, uint64_t body_len, uint64_t rs, int32_t ret,
                                             uint64_t e, uint64_t readable)
{
  if (fold) return RHP_FORWARD_FOLD;
  if (span_bad) return RHP_FORWARD_SPAN;
  if (body_kind > 1u) return RHP_FORWARD_BODY;
  if (body_kind == 1u) {
    if (body_len > 0xffffffffull) return RHP_FORWARD_LONG;
    const uint64_t b = rs + (uint64_t) (uint32_t) ret;   /* <= e, <= readable */
    if (body_len > e - b || body_len > readable - b) return RHP_FORWARD_BODY_OUTSIDE;
  }
  return RHP_FORWARD_OK;
}

/* every byte of a forwarded request except its kept fields: method SP path
 * " HTTP/1.1\r\n", the Content-Length line of a request with a body, extra,
 * the empty line, the body */
RHP_FORWARD_HD uint64_t rhp_forward_size_head(uint32_t method_len, uint32_t path_len, uint32_t body_kind, uint32_t body_len, uint32_t extra_len)
{
  return (uint64_t) method_len + 1u + path_len + 11u + (body_kind == 1u ? 16u + rhp_u32_len(body_len) + 2u + (uint64_t) body_len : 0u) + extra_len + 2u;
}

/* one kept field: name ": " value CRLF (http.c:63-71) */
RHP_FORWARD_HD uint64_t rhp_forward_size_field(uint32_t name_len, uint32_t value_len) { return (uint64_t) name_len + 2u + value_len + 2u; }

#endif
