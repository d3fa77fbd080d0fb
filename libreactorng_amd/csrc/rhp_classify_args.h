/*
 * rhp_classify_args.h -- the argument rules of rhp_classify_batch (rhp.h), one
 * statement of them for the kernel's launcher (rhp_classify.hip) and its host
 * twin (rhp_emu.cpp rhp_cpu_classify_batch).
 */
#ifndef RHP_CLASSIFY_ARGS_H
#define RHP_CLASSIFY_ARGS_H

#include <stdint.h>
#include "rhp.h"

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
  /* the batch: what rhp_parse_batch accepts, without the speculative flag */
  if (b->flags) return -22;
  if (b->mode != RHP_MODE_PHR && b->mode != RHP_MODE_HTTP) return -22;
  if (b->layout > RHP_LAYOUT_DENSE_RM) return -22;
  if (b->layout == RHP_LAYOUT_DENSE_RM && b->mode != RHP_MODE_PHR) return -22;
  if (b->max_headers > RHP_MAX_HEADERS) return -22;
  if ((uint64_t) b->n * b->max_headers > 0xffffffffull) return -22;
  if (b->n == 0) return 1;
  if (!b->bytes || !b->offsets || !b->reqs) return -22;
  if (((uintptr_t) b->bytes & 15u) != 0) return -22;
  if (b->max_headers > 0 && !b->hdrs) return -22;
  if (b->mode == RHP_MODE_HTTP && !b->http) return -22;
  if (c->n_names && !c->fields) return -22;
  if (c->n_routes && !c->route) return -22;
  return 0;
}

#endif
