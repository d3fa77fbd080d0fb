/*
 * rhp_walk_args.h -- the argument rules of rhp_walk_responses,
 * rhp_walk_resume and rhp_walk_answers (rhp.h), one statement of them for the
 * kernels' launchers (rhp_walk.hip) and the host twins (rhp_host.cpp
 * rhp_cpu_walk_responses, rhp_cpu_walk_resume, rhp_cpu_walk_answers), with the
 * clamps all apply to whatever sess_off, slot_off and req_off hold.
 */
#ifndef RHP_WALK_ARGS_H
#define RHP_WALK_ARGS_H

#include <stdint.h>
#include "rhp.h"

#define RHP_WALK_FLAGS (RHP_WALK_TRAILERS | RHP_WALK_DEFRAME | RHP_WALK_NONE_EMPTY)

/* 0: walk the sessions; 1: nothing to do (n_sessions == 0); -22: refused.
 * device_pointers adds the launcher's own rules (the reader's lines are aligned
 * 16-byte loads, the records leave as whole 16- and 8-byte stores), which host
 * callers, who pass any memory, leave out. */
static inline int rhp_walk_check(const rhp_walk_batch_t *w, int device_pointers)
{
  if (!w) return -22;
  if (w->max_headers > RHP_MAX_HEADERS) return -22;
  if (w->flags & ~RHP_WALK_FLAGS) return -22;
  if ((uint64_t) w->n_slots_total * w->max_headers > 0xffffffffull) return -22;   /* record indices are 32-bit */
  if ((w->flags & RHP_WALK_DEFRAME) && (!w->bytes_rw || w->bytes_rw != w->bytes)) return -22;   /* the same bytes, writable */
  if (w->n_sessions == 0) return 1;
  if (!w->bytes || !w->sess_off || !w->slot_off || !w->results) return -22;
  if (w->n_slots_total > 0 && (!w->msgs || !w->slots)) return -22;
  if (w->n_slots_total > 0 && w->max_headers > 0 && !w->hdrs) return -22;
  if (w->bytes_size < RHP_PAD) return -22;   /* bytes_size >= sess_off[n_sessions] + RHP_PAD */
  if (device_pointers &&
      ((((uintptr_t) w->bytes | (uintptr_t) w->msgs | (uintptr_t) w->slots | (uintptr_t) w->results) & 15u) != 0 ||
       ((uintptr_t) w->hdrs & 7u) != 0))
    return -22;
  return 0;
}

/* rhp_walk_resume (rhp.h): rhp_walk_check's answers, and its own two rules
 * about the states, for its launcher (rhp_walk.hip) and its host twin
 * (rhp_host.cpp rhp_cpu_walk_resume); a state is two whole 16-byte accesses */
static inline int rhp_walk_resume_check(const rhp_walk_batch_t *w, const rhp_walk_state_t *states, int device_pointers)
{
  const int rc = rhp_walk_check(w, device_pointers);
  if (rc != 0) return rc;
  if (!states) return -22;
  if (device_pointers && ((uintptr_t) states & 15u) != 0) return -22;
  return 0;
}

/* rhp_walk_answers (rhp.h): the answers of the walk it runs -- rhp_walk_check
 * with states == NULL, rhp_walk_resume_check with states -- and its own rules
 * about the queue, for its launcher (rhp_walk.hip) and its host twin
 * (rhp_host.cpp rhp_cpu_walk_answers); the four arrays are 4-byte accesses */
static inline int rhp_walk_answers_check(const rhp_walk_batch_t *w, const rhp_walk_state_t *states, const rhp_walk_asked_t *x,
                                         int device_pointers)
{
  const int rc = states ? rhp_walk_resume_check(w, states, device_pointers) : rhp_walk_check(w, device_pointers);
  if (rc < 0) return rc;
  if (!x || x->reserved != 0) return -22;
  if (rc != 0) return rc;
  if (!x->req_off || !x->answered) return -22;
  if (x->n_req_total > 0 && !x->head_bits) return -22;
  if (device_pointers &&
      (((uintptr_t) x->req_off | (uintptr_t) x->head_bits | (uintptr_t) x->answered | (uintptr_t) x->slot_req) & 3u) != 0)
    return -22;
  return 0;
}

/* the queue session s owns, from its req_off pair: the requests [*q0, *q0 +
 * nq), nq returned; a pair that is not ordered or reaches beyond n_req_total
 * owns no request, so no bit at or beyond n_req_total is ever looked at */
#if defined(__HIPCC__)
#define RHP_WALK_HD __host__ __device__ __forceinline__
#else
#define RHP_WALK_HD static inline
#endif
RHP_WALK_HD uint32_t rhp_walk_queue(uint32_t lo, uint32_t hi, uint32_t n_req_total, uint32_t *q0)
{
  if (lo > hi || hi > n_req_total) hi = lo = 0;
  *q0 = lo;
  return hi - lo;
}

/* where a session has to end, and where the reader's zeros begin: bytes_size
 * rounded down to whole 16-byte lines, less one line -- the de-framing move
 * loads the aligned line behind the one that holds its last source byte.  A
 * batch that keeps RHP_PAD has no session beyond it (RHP_PAD >= 31). */
static inline uint64_t rhp_walk_readable(uint64_t bytes_size) { return (bytes_size & ~(uint64_t) 15) - 16u; }

#endif
