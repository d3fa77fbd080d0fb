/*
 * rhp_lookup_args.h -- the argument rules of rhp_lookup_walked (rhp.h) and the
 * rules that decide which slot of a walk is looked up, one statement of them
 * for the kernel and its launcher (rhp_classify.hip) and the host twin
 * (rhp_host.cpp rhp_cpu_lookup_walked).  The batch's rules are
 * rhp_walk_responses' (rhp_walk_args.h), the names' rhp_classify_batch's.
 */
#ifndef RHP_LOOKUP_ARGS_H
#define RHP_LOOKUP_ARGS_H

#include <stdint.h>
#include "rhp.h"
#include "rhp_walk_args.h"

#if defined(__HIPCC__)
#define RHP_LOOKUP_HD __host__ __device__ __forceinline__
#else
#define RHP_LOOKUP_HD static inline
#endif

/* 0: look the slots up; 1: nothing to do (no slot, or no session to own one);
 * -22: refused.  device_pointers adds the launcher's own rules (rhp_walk_check's
 * alignments: the records are read as whole 16- and 8-byte loads; a field
 * leaves as one 4-byte store), which host callers, who pass any memory, leave
 * out. */
static inline int rhp_lookup_walked_check(const rhp_walk_batch_t *w, const rhp_walk_lookup_t *l, int device_pointers)
{
  const int rc = rhp_walk_check(w, device_pointers);
  if (rc < 0) return rc;
  if (!l) return -22;
  if (l->reserved != 0) return -22;
  if (l->n_names == 0 || l->n_names > RHP_CLASSIFY_MAX_NAMES) return -22;
  if (!l->text || !l->names || !l->fields) return -22;
  for (uint32_t j = 0; j < l->n_names; j++)
    if (l->names[j].len == 0 || l->names[j].len > RHP_CLASSIFY_NAME_MAX) return -22;
  if (device_pointers && ((uintptr_t) l->fields & 3u) != 0) return -22;
  return rc == 1 || w->n_slots_total == 0 ? 1 : 0;
}

/* where a head has to end for it to be looked up: bytes_size rounded down to
 * whole dwords (names are read as the aligned dwords that hold them), as
 * rhp_frame_readable */
static inline uint64_t rhp_lookup_readable(uint64_t bytes_size) { return bytes_size & ~(uint64_t) 3; }

/* Owner: the number of sessions s < n_sessions with slot_off[s] <= i
 * (bisection; slot_off is non-decreasing, rhp.h: the owner of slot i is the
 * last of them).  Reads slot_off[0, n_sessions) only. */
RHP_LOOKUP_HD uint32_t rhp_lookup_sessions_upto(const uint64_t *slot_off, uint32_t n_sessions, uint32_t i)
{
  uint32_t above = 0;
  for (uint32_t hi = n_sessions; above < hi;) {
    const uint32_t mid = above + ((hi - above) >> 1);
    if (slot_off[mid] <= i) above = mid + 1u; else hi = mid;
  }
  return above;
}

/* In use: the one test that lets a load of slot i's records through, whatever
 * the search returned: the session's slot range [lo, hi) holds in a batch of
 * n_slots_total slots, contains i, and the walk wrote the slot */
RHP_LOOKUP_HD int rhp_lookup_in_use(uint32_t i, uint64_t lo, uint64_t hi, uint32_t n_slots, uint32_t n_slots_total)
{
  return lo <= i && i < hi && hi <= n_slots_total && i - lo < n_slots;
}

/* Head: a slot with a parsed head (a continuation slot has ret == 0, a HEAD or
 * BAD stop slot result != 1, RHP_RET_TOOLONG is negative) */
RHP_LOOKUP_HD int rhp_lookup_is_head(int32_t slot_result, int32_t ret) { return slot_result == 1 && ret > 0; }

/* Inside: the head [st, st + ret), ret > 0, lies inside its session's bytes
 * [a, e] and below the readable end */
RHP_LOOKUP_HD int rhp_lookup_inside(uint64_t st, int32_t ret, uint64_t a, uint64_t e, uint64_t readable)
{
  return a <= st && st <= e && (uint64_t) (uint32_t) ret <= e - st && st <= readable && (uint64_t) (uint32_t) ret <= readable - st;
}

#endif
