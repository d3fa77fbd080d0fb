/*
 * rhp_reply_args.h -- the argument rules of rhp_reply_sessions (rhp.h), one
 * statement of them for the kernels' launcher (rhp_reply.hip) and the host
 * twin (rhp_host.cpp rhp_cpu_reply_sessions).
 */
#ifndef RHP_REPLY_ARGS_H
#define RHP_REPLY_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_records.h"

/* 0: answer the sessions; 1: no slot to look at (n == 0: every count is 0); -22: refused.
 * The batch is held to what rhp_classify_sessions holds it to (rhp_classify_args.h):
 * the speculative http batch in one of the two rhp_hdr_t layouts, bytes_rw may be
 * NULL.  host_tables: image_off is host memory (the twin), so that a NULL images
 * can be held to "every image is empty"; the launcher cannot read it (rhp.h) */
static inline int rhp_reply_sessions_check(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                           const rhp_session_result_t *results, const uint16_t *route,
                                           const rhp_reply_table_t *t, const rhp_reply_out_t *o, int host_tables)
{
  if (!b || !route || !t || !o) return -22;
  if (!t->image_off || t->n_routes == 0 || t->n_routes > RHP_CLASSIFY_MAX_ROUTES) return -22;
  if (!o->replies || !o->total || !o->work) return -22;
  if (!o->out && o->out_size != 0) return -22;
  if (b->mode != RHP_MODE_HTTP || b->flags != RHP_BATCH_SPECULATIVE) return -22;
  if (n_sessions && (!sessions || !results)) return -22;
  rhp_batch_t q = *b;
  if (!q.bytes_rw) q.bytes_rw = (uint8_t *) q.bytes;
  q.last_len = NULL;
  const int rc = rhp_batch_check(&q, 1);
  if (rc < 0) return rc;
  if (!t->images && host_tables && t->image_off[t->n_routes] != t->image_off[0]) return -22;
  return rc;
}

#endif
