/*
 * rhp_classify_args.h -- the argument rules of rhp_classify_batch and
 * rhp_classify_sessions (rhp.h), one statement of them for the kernels'
 * launchers (rhp_classify.hip) and their host twins (rhp_host.cpp
 * rhp_cpu_classify_batch, rhp_cpu_classify_sessions).
 */
#ifndef RHP_CLASSIFY_ARGS_H
#define RHP_CLASSIFY_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_records.h"

/* the lookup tables, the same for both entry points: 0 or -22 */
static inline int rhp_classify_tables_check(const rhp_classify_t *c)
{
  if (c->n_names > RHP_CLASSIFY_MAX_NAMES || c->n_routes > RHP_CLASSIFY_MAX_ROUTES) return -22;
  if (c->n_names == 0 && c->n_routes == 0) return -22;
  if (!c->text) return -22;
  if (c->n_names && !c->names) return -22;
  if (c->n_routes && !c->routes) return -22;
  for (uint32_t j = 0; j < c->n_names; j++)
    if (c->names[j].len == 0 || c->names[j].len > RHP_CLASSIFY_NAME_MAX) return -22;
  uint64_t text = 0;
  for (uint32_t r = 0; r < c->n_routes; r++) text += (uint64_t) c->routes[r].method.len + c->routes[r].target.len;
  if (text > RHP_CLASSIFY_TEXT_MAX) return -22;
  return 0;
}

/* the batch: what rhp_parse_batch accepts (rhp_records.h), with the flags the
 * caller has looked at.  Classifying only reads, and never last_len: bytes_rw
 * may be NULL (the request's bytes are then read through `bytes`) and last_len
 * is not looked at.  Then the outputs.  0, 1 (n == 0) or -22 */
static inline int rhp_classify_batch_and_outputs_check(const rhp_batch_t *b, const rhp_classify_t *c)
{
  rhp_batch_t q = *b;
  if (!q.bytes_rw) q.bytes_rw = (uint8_t *) q.bytes;
  q.last_len = NULL;
  const int rc = rhp_batch_check(&q, 1);
  if (rc != 0) return rc;
  if (c->n_names && !c->fields) return -22;
  if (c->n_routes && !c->route) return -22;
  return 0;
}

/* 0: classify the batch; 1: nothing to do (n == 0); -22: refused */
static inline int rhp_classify_check(const rhp_batch_t *b, const rhp_classify_t *c)
{
  if (!b || !c) return -22;
  const int rc = rhp_classify_tables_check(c);
  if (rc != 0) return rc;
  if (b->flags) return -22;   /* a speculative batch: rhp_classify_sessions */
  return rhp_classify_batch_and_outputs_check(b, c);
}

/* rhp_classify_sessions: the same codes.  The batch is the speculative http
 * batch rhp_fixup_sessions has walked, which rhp_batch_check holds to the two
 * rhp_hdr_t layouts (request-major and header-major) */
static inline int rhp_classify_sessions_check(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                              const rhp_session_result_t *results, const uint64_t *req_start,
                                              const rhp_classify_t *c)
{
  if (!b || !c) return -22;
  const int rc = rhp_classify_tables_check(c);
  if (rc != 0) return rc;
  if (b->mode != RHP_MODE_HTTP || b->flags != RHP_BATCH_SPECULATIVE) return -22;
  if (n_sessions && (!sessions || !results || !req_start)) return -22;
  return rhp_classify_batch_and_outputs_check(b, c);
}

#endif
