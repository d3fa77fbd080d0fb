/*
 * rhp_gather_args.h -- the argument rules of rhp_gather_wide (rhp.h), one
 * statement of them for the kernels' launcher (rhp_gather.hip) and the host
 * twin (rhp_host.cpp rhp_cpu_gather_wide).
 */
#ifndef RHP_GATHER_ARGS_H
#define RHP_GATHER_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_records.h"

/* 0: gather; 1: no slot to look at (n == 0 or no session: zero totals); -22: refused.
 * The batch is held to what rhp_classify_sessions holds it to (rhp_classify_args.h:
 * the speculative http batch, bytes_rw may be NULL) and to rhp_pack_dense's layout */
static inline int rhp_gather_wide_check(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                        const rhp_session_result_t *results, const uint64_t *req_start,
                                        const rhp_req_dense_t *dreq, const rhp_http_compact_t *hc, const rhp_wide_out_t *o)
{
  if (!b || !dreq || !hc || !o) return -22;
  if (!o->totals || !o->work) return -22;
  if ((!o->slots && o->cap_slots) || (!o->hdrs && o->cap_hdrs) || (!o->body && o->cap_body)) return -22;
  if (((uintptr_t) o->slots & 15u) || ((uintptr_t) o->hdrs & 7u)) return -22;
  if (b->mode != RHP_MODE_HTTP || b->flags != RHP_BATCH_SPECULATIVE || b->layout != RHP_LAYOUT_REQUEST_MAJOR) return -22;
  if (n_sessions && (!sessions || !results || !req_start)) return -22;
  rhp_batch_t q = *b;
  if (!q.bytes_rw) q.bytes_rw = (uint8_t *) q.bytes;
  q.last_len = NULL;
  const int rc = rhp_batch_check(&q, 1);
  if (rc < 0) return rc;
  return rc == 1 || n_sessions == 0 ? 1 : 0;
}

#endif
