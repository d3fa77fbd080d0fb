/*
 * rhp_classify_args.h -- the argument rules of rhp_classify_batch (rhp.h), one
 * statement of them for the kernel's launcher (rhp_classify.hip) and its host
 * twin (rhp_host.cpp rhp_cpu_classify_batch).
 */
#ifndef RHP_CLASSIFY_ARGS_H
#define RHP_CLASSIFY_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_records.h"

/* 0: classify the batch; 1: nothing to do (n == 0); -22: refused */
static inline int rhp_classify_check(const rhp_batch_t *b, const rhp_classify_t *c)
{
  if (!b || !c) return -22;
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
  /* the batch: what rhp_parse_batch accepts (rhp_records.h), without flags.
   * Classifying only reads, and never last_len: bytes_rw may be NULL (the
   * request's bytes are then read through `bytes`) and last_len is not looked at */
  if (b->flags) return -22;
  rhp_batch_t q = *b;
  if (!q.bytes_rw) q.bytes_rw = (uint8_t *) q.bytes;
  q.last_len = NULL;
  const int rc = rhp_batch_check(&q, 1);
  if (rc != 0) return rc;
  if (c->n_names && !c->fields) return -22;
  if (c->n_routes && !c->route) return -22;
  return 0;
}

#endif
