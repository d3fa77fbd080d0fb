/*
 * rhp_classify.hip -- rhp_classify_batch (rhp.h): http_field_lookup
 * (src/reactor/http.c:167-175) for up to 16 names and the string_equal route
 * dispatch of the reference's users (http.c:198, test/server.c:75-82) over a
 * parsed batch whose bytes and records are in HBM.  gfx950.
 *
 * One request per lane.  The lane decodes its request record (any of the five
 * layouts, rhp.h), walks its header records k < num_headers -- in the
 * header-major layouts lens[k * n + i] is one coalesced load per wave and k, in
 * the compact and dense ones the offsets are the running sum carried in
 * registers -- and compares in two stages: name_len against the lengths of the
 * names still looked for (records only, a 65-entry mask table in LDS), and only
 * for a length match the name's bytes, read as the aligned dwords that hold
 * them, funnel-shifted, folded four at a time (SWAR a..z -> A..Z) and compared
 * with the names the host folded once.  The lookup tables (rhp_tables.h, shared
 * with rhp_forward.hip) travel by value in
 * the kernel argument (3.5 KiB) and the block copies them to LDS at its start:
 * no allocation, no copy, the caller's tables are free when the call returns.
 *
 * Nothing of a request that is not ready, and no record k >= num_headers, is
 * used: those are unspecified (rhp.h) and may hold anything.
 *
 * rhp_classify_sessions (rhp.h) is the same lookup over the record slots
 * rhp_fixup_sessions leaves in a speculative batch: one slot per lane, the
 * slot's session by binary search over sessions[].piece_lo (sessions_upto,
 * rhp_device.h, shared with rhp_reply.hip and rhp_gather.hip), the request's
 * first byte from req_start[i].  Its kernel writes out the first one's table
 * load, compare, absent fill and route match again: the forms of stating them
 * once that were tried, and why none is here, are in DESIGN 3.5.  The launchers
 * share fill_params.
 *
 * rhp_frame_messages (rhp.h) is the lookup over the rhp_msg_t / rhp_hdr_t
 * records rhp_parse_messages leaves, with the framing of http.c:204-233 decided
 * in the same walk: its kernel stands here because it shares fold4, same_text,
 * CTables and pack_tables.
 *
 * rhp_lookup_walked (rhp.h) is rhp_classify_sessions' lookup over the slots a
 * response walk (rhp_walk.hip) left: one slot per lane, the slot's session by
 * binary search over slot_off[], the head's first byte from slots[i].start,
 * the rules that let a slot through in rhp_lookup_args.h.
 *
 * rhp_relay_walked (rhp.h) re-writes the walked responses for the client side:
 * http_write_response (src/reactor/http.c:236-297) for every slot that holds a
 * whole response.  Its sizes step stands here because it is the lookup above
 * with sixteen drop names in the same tables; its copy step is
 * rhp_writer.hip's plan over the walked records, built from rhp_device.h's
 * stage writers, and the scan between them is rhp_device.h's.  The rule is
 * rhp_relay_args.h's.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rhp.h"
#include "rhp_classify_args.h"
#define RHP_DEVICE_SCAN_KERNELS   /* this file launches rhp_device.h's two scan kernels */
#include "rhp_device.h"
#include "rhp_frame_args.h"
#include "rhp_lookup_args.h"
#include "rhp_relay_args.h"
#include "rhp_scalar.h"
#include "rhp_tables.h"

namespace {

struct CParams {
  CTables         t;          /* first: the kernels read it from the start of their argument segment */
  const uint8_t  *bytes;
  const uint64_t *offsets;
  const uint8_t  *reqs, *hdrs, *http;
  uint32_t       *fields;
  uint16_t       *route;
  uint32_t        n, m, layout, n_names, n_routes;
};
static_assert(offsetof(CParams, t) == 0, "the tables lead the argument");
static_assert(sizeof(CParams) <= 4096, "a kernel argument holds 4 KiB");

__global__ __launch_bounds__(256) void rhp_classify_kernel(CParams p)
{
  __shared__ uint32_t tab[kTabDwords];
  __shared__ uint16_t lenmask[RHP_CLASSIFY_NAME_MAX + 1u];
  {
    /* the tables lead the argument segment: read them from there (indexing
     * the by-value struct would make a private copy per lane) */
#if defined(__HIP_DEVICE_COMPILE__)   /* (the host pass only checks the body) */
    const ka32 *ka = (const ka32 *) __builtin_amdgcn_kernarg_segment_ptr();
#else
    const ka32 *ka = nullptr;
#endif
    for (uint32_t t = threadIdx.x; t < kTabDwords; t += blockDim.x) tab[t] = ka[t];
    if (threadIdx.x <= RHP_CLASSIFY_NAME_MAX) {
      const ka32 *nl = ka + offsetof(CTables, name_len) / 4u;
      uint32_t mk = 0;
      for (uint32_t j = 0; j < p.n_names; j++) mk |= (((nl[j >> 2] >> (8u * (j & 3u))) & 0xffu) == threadIdx.x ? 1u : 0u) << j;
      lenmask[threadIdx.x] = (uint16_t) mk;
    }
  }
  __syncthreads();
  const uint32_t *names = tab + offsetof(CTables, name) / 4u, *text = tab + offsetof(CTables, text) / 4u;
  const uint16_t *r_moff = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_moff) / 4u);
  const uint16_t *r_mlen = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_mlen) / 4u);
  const uint16_t *r_toff = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_toff) / 4u);
  const uint16_t *r_tlen = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_tlen) / 4u);

  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = p.n, m = p.m;
  if (i >= n) return;
  const bool dense = p.layout == RHP_LAYOUT_DENSE || p.layout == RHP_LAYOUT_DENSE_RM;
  const bool lengths = dense || p.layout == RHP_LAYOUT_COMPACT;   /* running-sum records, rhp_hdr_t ones in a wide area */
  const bool chttp = p.layout == RHP_LAYOUT_COMPACT || p.layout == RHP_LAYOUT_DENSE;   /* rhp_http_compact_t */

  /* ---- the request record: ready? path, method, num_headers, wide? ---- */
  int32_t ret = 0;
  uint32_t method_off = 0, method_len = 0, path_off = 0, path_len = 0, nh = 0;
  bool wide = false;
  {
    bool full = !dense;   /* an rhp_req_t holds this request */
    const uint8_t *rq = p.reqs;
    if (dense) {
      const uint2 d = reinterpret_cast<const uint2 *>(p.reqs)[i];
      const uint32_t fl = d.y >> 24;
      if (fl & RHP_DENSE_WIDE) {
        full = true;
        rq = p.reqs + RHP_DENSE_REQ_WIDE_OFF(n);
      } else if (!(fl & RHP_DENSE_BAD)) {
        ret = (int32_t) (d.x & 0xffffu);
        path_len = d.x >> 16;
        method_len = d.y & 0xffu;
        path_off = method_len + 1u;
        nh = (d.y >> 8) & 0xffu;
      }
    }
    if (full) {
      const uint4 q = reinterpret_cast<const uint4 *>(rq)[i];
      ret = (int32_t) q.x;
      method_len = q.y & 0xffffu;
      path_off = q.y >> 16;
      path_len = q.z & 0xffffu;
      method_off = (q.z >> 16) & 0xffu;
      nh = q.w & 0xffffu;
      wide = lengths && (dense || ((q.w >> 16) & RHP_F_WIDE));
    }
  }
  bool ready = ret > 0;   /* RHP_RET_TOOLONG is negative */
  if (p.http) {           /* RHP_MODE_HTTP: result == 1 */
    int32_t result;
    if (chttp) {
      const uint2 c = reinterpret_cast<const uint2 *>(p.http)[i];
      if ((c.x >> 16) & RHP_HTTP_WIDE)
        result = *reinterpret_cast<const int32_t *>(p.http + RHP_COMPACT_HTTP_WIDE_OFF(n) + (size_t) i * sizeof(rhp_http_t));
      else
        result = (int8_t) (c.x & 0xffu);
    } else {
      result = *reinterpret_cast<const int32_t *>(p.http + (size_t) i * sizeof(rhp_http_t));
    }
    ready = ready && result == 1;
  }
  if (!ready) nh = 0;
  if (nh > m) nh = m;   /* never more records than the batch holds */
  const uint64_t at0 = ready ? p.offsets[i] : 0u;   /* the request's first byte */

  /* ---- header lookup ---- */
  const uint32_t all = (1u << p.n_names) - 1u;
  uint32_t found = 0;
  if (p.n_names) {
    /* rhp_hdr_t records: index i * s_req + k * s_hdr of recs */
    const uint8_t *recs = p.hdrs;
    uint64_t s_req = m, s_hdr = 1;
    if (p.layout == RHP_LAYOUT_HEADER_MAJOR) {
      s_req = 1;
      s_hdr = n;
    }
    if (lengths) recs = p.hdrs + (dense ? RHP_DENSE_WIDE_OFF(n, m) : RHP_COMPACT_WIDE_OFF(n, m));
    const bool drm = p.layout == RHP_LAYOUT_DENSE_RM;
    const uint16_t *lens16 = reinterpret_cast<const uint16_t *>(p.hdrs);
    const uint32_t *lens32 = reinterpret_cast<const uint32_t *>(p.hdrs);
    const uint32_t *ovf32 = reinterpret_cast<const uint32_t *>(p.hdrs + RHP_DENSE_OVF_OFF(n, m));
    uint32_t at = path_off + path_len + 11u;   /* the first header line (rhp.h) */
    for (uint32_t k = 0; k < nh && found != all; k++) {
      uint32_t noff, nl, voff, vl;
      if (!lengths || wide) {
        const uint2 h = reinterpret_cast<const uint2 *>(recs)[(uint64_t) i * s_req + (uint64_t) k * s_hdr];
        noff = h.x & 0xffffu;
        nl = h.x >> 16;
        voff = h.y & 0xffffu;
        vl = h.y >> 16;
        if (noff == RHP_NAME_NULL) continue;   /* name == NULL: an obs-fold line */
      } else {
        uint32_t l;
        if (dense) {
          const uint64_t idx = drm ? (uint64_t) i * m + k : (uint64_t) k * n + i;
          l = lens16[idx];
          l = l == RHP_DENSE_OVERFLOW ? ovf32[idx] : (l & 63u) | (l >> 6) << 16;
        } else {
          l = lens32[(uint64_t) k * n + i];
        }
        nl = l & 0xffffu;
        vl = l >> 16;
        noff = at;
        voff = (at + nl + 2u) & 0xffffu;
        at += nl + vl + 4u;
      }
      uint32_t cand = nl <= RHP_CLASSIFY_NAME_MAX ? (uint32_t) lenmask[nl] & ~found : 0u;
      if (cand == 0) continue;
      if (noff + nl > (uint32_t) ret) continue;   /* (a parsed name lies inside its header section) */
      cand = same_text<true>(p.bytes + at0 + noff, nl, cand, names, [](uint32_t j) { return j * kNameDwords; });
      for (uint32_t c = cand; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = voff | vl << 16;
      found |= cand;
    }
    for (uint32_t c = all & ~found; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = RHP_NAME_NULL;
  }

  /* ---- route match: lengths first, then the path's and the method's bytes ---- */
  if (p.route) {
    uint32_t rt = RHP_ROUTE_NONE;
    if (ready && p.n_routes) {
      uint32_t cand = 0, with_method = 0;
      for (uint32_t r = 0; r < p.n_routes; r++) {
        const uint32_t ml = r_mlen[r];
        if (r_tlen[r] == path_len && (ml == 0 || ml == method_len)) cand |= 1u << r;
        if (ml) with_method |= 1u << r;
      }
      if (path_off + path_len > (uint32_t) ret || method_off + method_len > (uint32_t) ret) cand = 0;   /* (as the names) */
      if (cand) cand = same_text<false>(p.bytes + at0 + path_off, path_len, cand, text, [&](uint32_t r) { return (uint32_t) r_toff[r]; });
      if (cand & with_method) {
        const uint32_t ok = same_text<false>(p.bytes + at0 + method_off, method_len, cand & with_method, text,
                                             [&](uint32_t r) { return (uint32_t) r_moff[r]; });
        cand = (cand & ~with_method) | ok;
      }
      if (cand) rt = (uint32_t) __builtin_ctz(cand);
    }
    p.route[i] = (uint16_t) rt;
  }
}

/* rhp_classify_sessions_kernel's argument: CParams' members under their names
 * (fill_params fills either), with what the session search needs among them */
struct SParams {
  CTables         t;
  const uint8_t  *bytes;
  const uint64_t *offsets;
  const uint8_t  *reqs, *hdrs, *http;
  uint32_t       *fields;
  uint16_t       *route;
  const rhp_session_t        *sessions;
  const rhp_session_result_t *results;
  const uint64_t *req_start;
  uint32_t        n, m, layout, n_names, n_routes, n_sessions;
};
static_assert(offsetof(SParams, t) == 0, "the tables lead the argument");
static_assert(sizeof(SParams) <= 4096, "a kernel argument holds 4 KiB");

/* One record slot per lane.  The lane finds the last session whose piece_lo is
 * at or below its slot (sessions ascend by piece_lo, rhp.h) and tests that the
 * slot is one the fix-up filled for that session; only then are req_start[i]
 * and the slot's records loaded -- a slot the walk did not use holds a stale
 * speculative record or nothing.  Whatever the search returns, it is the test
 * that lets a load through, so sessions in any order read nothing outside the
 * batch's buffers (a slot may then be reported absent).  rhp_hdr_t records
 * only, request-major or header-major: the layouts of a speculative batch. */
__global__ __launch_bounds__(256) void rhp_classify_sessions_kernel(SParams p)
{
  __shared__ uint32_t tab[kTabDwords];
  __shared__ uint16_t lenmask[RHP_CLASSIFY_NAME_MAX + 1u];
  {
#if defined(__HIP_DEVICE_COMPILE__)   /* (as rhp_classify_kernel) */
    const ka32 *ka = (const ka32 *) __builtin_amdgcn_kernarg_segment_ptr();
#else
    const ka32 *ka = nullptr;
#endif
    for (uint32_t t = threadIdx.x; t < kTabDwords; t += blockDim.x) tab[t] = ka[t];
    if (threadIdx.x <= RHP_CLASSIFY_NAME_MAX) {
      const ka32 *nl = ka + offsetof(CTables, name_len) / 4u;
      uint32_t mk = 0;
      for (uint32_t j = 0; j < p.n_names; j++) mk |= (((nl[j >> 2] >> (8u * (j & 3u))) & 0xffu) == threadIdx.x ? 1u : 0u) << j;
      lenmask[threadIdx.x] = (uint16_t) mk;
    }
  }
  __syncthreads();
  const uint32_t *names = tab + offsetof(CTables, name) / 4u, *text = tab + offsetof(CTables, text) / 4u;
  const uint16_t *r_moff = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_moff) / 4u);
  const uint16_t *r_mlen = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_mlen) / 4u);
  const uint16_t *r_toff = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_toff) / 4u);
  const uint16_t *r_tlen = reinterpret_cast<const uint16_t *>(tab + offsetof(CTables, r_tlen) / 4u);

  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = p.n, m = p.m;
  if (i >= n) return;

  /* ---- the slot's session: the sessions before `above` have piece_lo <= i ---- */
  const uint32_t above = rhp_device::sessions_upto(p.sessions, p.n_sessions, i);

  /* ---- in use?  ready?  then the request record and the request's first byte ---- */
  int32_t ret = 0;
  uint32_t method_off = 0, method_len = 0, path_off = 0, path_len = 0, nh = 0;
  uint64_t at0 = 0;
  bool ready = false;
  if (above) {
    const uint2 se = reinterpret_cast<const uint2 *>(p.sessions)[above - 1u];   /* piece_lo, piece_hi */
    const uint32_t n_slots = p.results[above - 1u].n_slots;
    /* (se.y <= n: offsets[piece_hi] is an entry of offsets).  Not rhp_device.h's
     * in_use(): this test asks se.x <= se.y where that one asks se.x + n_slots <=
     * se.y, so a session whose n_slots passes piece_hi is classified here and not
     * answered or gathered there.  The difference is known; this test and the host
     * twin's define what rhp_classify_sessions returns, and it stays as it is */
    if (se.x <= i && i - se.x < n_slots && se.x <= se.y && se.y <= n &&
        *reinterpret_cast<const int32_t *>(p.http + (size_t) i * sizeof(rhp_http_t)) == 1) {
      const uint4 q = reinterpret_cast<const uint4 *>(p.reqs)[i];
      ret = (int32_t) q.x;
      if (ret > 0) {   /* RHP_RET_TOOLONG is negative */
        /* the request lies inside its session's input */
        const uint64_t rs = p.req_start[i], b_lo = p.offsets[se.x], b_hi = p.offsets[se.y];
        ready = rs >= b_lo && rs <= b_hi && (uint64_t) (uint32_t) ret <= b_hi - rs;
        at0 = rs;
      }
      if (ready) {
        method_len = q.y & 0xffffu;
        path_off = q.y >> 16;
        path_len = q.z & 0xffffu;
        method_off = (q.z >> 16) & 0xffu;
        nh = q.w & 0xffffu;
      }
    }
  }
  if (nh > m) nh = m;   /* never more records than the batch holds */

  /* ---- header lookup over rhp_hdr_t records ---- */
  const uint32_t all = (1u << p.n_names) - 1u;
  uint32_t found = 0;
  if (p.n_names) {
    uint64_t s_req = m, s_hdr = 1;   /* record k of slot i: index i * s_req + k * s_hdr */
    if (p.layout == RHP_LAYOUT_HEADER_MAJOR) {
      s_req = 1;
      s_hdr = n;
    }
    for (uint32_t k = 0; k < nh && found != all; k++) {
      const uint2 h = reinterpret_cast<const uint2 *>(p.hdrs)[(uint64_t) i * s_req + (uint64_t) k * s_hdr];
      const uint32_t noff = h.x & 0xffffu, nl = h.x >> 16, voff = h.y & 0xffffu, vl = h.y >> 16;
      if (noff == RHP_NAME_NULL) continue;   /* name == NULL: an obs-fold line */
      uint32_t cand = nl <= RHP_CLASSIFY_NAME_MAX ? (uint32_t) lenmask[nl] & ~found : 0u;
      if (cand == 0) continue;
      if (noff + nl > (uint32_t) ret) continue;   /* (a parsed name lies inside its header section) */
      cand = same_text<true>(p.bytes + at0 + noff, nl, cand, names, [](uint32_t j) { return j * kNameDwords; });
      for (uint32_t c = cand; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = voff | vl << 16;
      found |= cand;
    }
    for (uint32_t c = all & ~found; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = RHP_NAME_NULL;
  }

  /* ---- route match: lengths first, then the path's and the method's bytes ---- */
  if (p.route) {
    uint32_t rt = RHP_ROUTE_NONE;
    if (ready && p.n_routes) {
      uint32_t cand = 0, with_method = 0;
      for (uint32_t r = 0; r < p.n_routes; r++) {
        const uint32_t ml = r_mlen[r];
        if (r_tlen[r] == path_len && (ml == 0 || ml == method_len)) cand |= 1u << r;
        if (ml) with_method |= 1u << r;
      }
      if (path_off + path_len > (uint32_t) ret || method_off + method_len > (uint32_t) ret) cand = 0;   /* (as the names) */
      if (cand) cand = same_text<false>(p.bytes + at0 + path_off, path_len, cand, text, [&](uint32_t r) { return (uint32_t) r_toff[r]; });
      if (cand & with_method) {
        const uint32_t ok = same_text<false>(p.bytes + at0 + method_off, method_len, cand & with_method, text,
                                             [&](uint32_t r) { return (uint32_t) r_moff[r]; });
        cand = (cand & ~with_method) | ok;
      }
      if (cand) rt = (uint32_t) __builtin_ctz(cand);
    }
    p.route[i] = (uint16_t) rt;
  }
}

/* what CParams and SParams share; which bytes and whether http is the caller's */
template <class P>
void fill_params(P &p, const rhp_batch_t *b, const rhp_classify_t *c, const uint8_t *bytes, const rhp_http_t *http)
{
  pack_tables(c, p.t);
  p.bytes = bytes;
  p.offsets = b->offsets;
  p.reqs = reinterpret_cast<const uint8_t *>(b->reqs);
  p.hdrs = reinterpret_cast<const uint8_t *>(b->hdrs);
  p.http = reinterpret_cast<const uint8_t *>(http);
  p.fields = reinterpret_cast<uint32_t *>(c->fields);
  p.route = c->route;
  p.n = b->n;
  p.m = b->max_headers;
  p.layout = b->layout;
  p.n_names = c->n_names;
  p.n_routes = c->n_routes;
}

/* ---- rhp_frame_messages ---- */

/* the framing names and `chunked`, folded, lie in the tables' route text (a
 * frame call has no routes), each at a dword; they take the mask bits above the
 * caller's names */
constexpr uint32_t kTeBit = 1u << RHP_CLASSIFY_MAX_NAMES, kClBit = kTeBit << 1;
constexpr uint32_t kTeLen = 17u, kClLen = 14u, kChunkedLen = 7u;
constexpr uint32_t kTextAt = offsetof(CTables, text) / 4u;                   /* dword index into the tables */
constexpr uint32_t kTeAt = kTextAt, kClAt = kTextAt + 8u, kChunkedAt = kTextAt + 16u;
static_assert(kTeLen <= 32u && kClLen <= 32u && kChunkedLen <= 32u && kTextDwords >= 24u, "eight dwords each");
static_assert(offsetof(CTables, name) == 0 && kTeLen <= RHP_CLASSIFY_NAME_MAX && kClLen <= RHP_CLASSIFY_NAME_MAX, "");

struct FParams {
  CTables         t;          /* first, as CParams */
  const uint8_t  *bytes;
  const uint64_t *offsets;
  uint64_t        readable;   /* rhp_frame_readable */
  const uint4    *msgs;
  const uint2    *hdrs;
  uint32_t       *fields;
  uint4          *frames, *decoders;
  uint32_t        n, m, n_names, consume_trailer;
  uint32_t        s_req, s_hdr;   /* record k of message i: hdrs[i * s_req + k * s_hdr] */
};
static_assert(offsetof(FParams, t) == 0, "the tables lead the argument");
static_assert(sizeof(FParams) <= 4096, "a kernel argument holds 4 KiB");
static_assert(sizeof(rhp_msg_t) == 16 && sizeof(rhp_frame_t) == 16 && sizeof(rhp_chunked_t) == 16 &&
              offsetof(rhp_msg_t, num_headers) == 12 && offsetof(rhp_frame_t, body_len) == 8 &&
              offsetof(rhp_chunked_t, consume_trailer) == 8, "records as 16-byte accesses");

/* strtoull10 (rhp_scalar.h) over the len >= 1 bytes at src, read as the aligned
 * dwords that hold them: those of the first 24 bytes up front (independent
 * loads), then, only while digits go on, a dependent byte at a time.  The same
 * num_step over the same bytes, zeros behind the value's end. */
__device__ __forceinline__ uint64_t value_number(const uint8_t *src, uint32_t len)
{
  constexpr uint32_t kWin = 24u;   /* strtoull10's kNumWindow */
  const uintptr_t a = (uintptr_t) src;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t) 3);
  const uint32_t sh = (uint32_t) a & 3u, nd = (sh + len + 3u) >> 2;
  uint32_t d[kWin / 4u + 1u];
#pragma unroll
  for (uint32_t q = 0; q <= kWin / 4u; q++) d[q] = q < nd ? w[q] : 0u;
  uint32_t st = 0;
  bool neg = false, ovf = false;
  uint64_t v = 0;
#pragma unroll
  for (uint32_t q = 0; q < kWin / 4u; q++) {
    const uint32_t x = __builtin_amdgcn_alignbyte(d[q + 1u], d[q], sh);
#pragma unroll
    for (uint32_t e = 0; e < 4u; e++) rhp::num_step(4u * q + e < len ? (x >> (8u * e)) & 0xffu : 0u, st, neg, ovf, v);
  }
  for (uint32_t j = kWin; st != 2u && j < len; j++) {
    const uint32_t at = sh + j;
    rhp::num_step((w[at >> 2] >> (8u * (at & 3u))) & 0xffu, st, neg, ovf, v);
  }
  return ovf ? ~0ull : neg ? 0 - v : v;
}

/* One message per lane, rhp_classify_kernel's mapping: the lane loads its
 * rhp_msg_t as one 16-byte load and walks its rhp_hdr_t records k < num_headers
 * once (header-major: consecutive lanes read consecutive records) for the two
 * framing names and the caller's together -- name_len against one length mask,
 * the name's bytes only on a length match -- until all of them are settled;
 * then the one value the decision needs.  Nothing of a message that is not
 * ready, and no record k >= num_headers, is read; a message is ready only when
 * [offsets[i], offsets[i] + ret) lies below `readable`, and every name and
 * value read lies inside [0, ret). */
__global__ __launch_bounds__(256) void rhp_frame_messages_kernel(FParams p)
{
  __shared__ uint32_t tab[kTabDwords];
  __shared__ uint32_t lenmask[RHP_CLASSIFY_NAME_MAX + 1u];
  {
#if defined(__HIP_DEVICE_COMPILE__)   /* (as rhp_classify_kernel) */
    const ka32 *ka = (const ka32 *) __builtin_amdgcn_kernarg_segment_ptr();
#else
    const ka32 *ka = nullptr;
#endif
    for (uint32_t t = threadIdx.x; t < kTabDwords; t += blockDim.x) tab[t] = ka[t];
    if (threadIdx.x <= RHP_CLASSIFY_NAME_MAX) {
      const ka32 *nl = ka + offsetof(CTables, name_len) / 4u;
      uint32_t mk = (threadIdx.x == kTeLen ? kTeBit : 0u) | (threadIdx.x == kClLen ? kClBit : 0u);
      for (uint32_t j = 0; j < p.n_names; j++) mk |= (((nl[j >> 2] >> (8u * (j & 3u))) & 0xffu) == threadIdx.x ? 1u : 0u) << j;
      lenmask[threadIdx.x] = mk;
    }
  }
  __syncthreads();

  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = p.n;
  if (i >= n) return;

  /* ---- the message record: ready?  num_headers ---- */
  const uint4 q = p.msgs[i];
  const int32_t ret = (int32_t) q.x;
  uint64_t at0 = 0;
  bool ready = ret > 0;   /* RHP_RET_TOOLONG is negative */
  if (ready) {
    at0 = p.offsets[i];
    ready = at0 <= p.readable && (uint64_t) (uint32_t) ret <= p.readable - at0;
  }
  uint32_t nh = ready ? q.w & 0xffffu : 0u;
  if (nh > p.m) nh = p.m;   /* never more records than the batch holds */

  /* ---- one walk: the framing names and the caller's ---- */
  const uint32_t callers = (1u << p.n_names) - 1u, all = callers | kTeBit | kClBit;
  const auto text_at = [](uint32_t j) { return j < RHP_CLASSIFY_MAX_NAMES ? j * kNameDwords : j == RHP_CLASSIFY_MAX_NAMES ? kTeAt : kClAt; };
  uint32_t found = 0, te = 0, cl = 0;   /* te, cl: value_off | value_len << 16 of the first match */
  for (uint32_t k = 0; k < nh && found != all; k++) {
    const uint2 h = p.hdrs[(uint64_t) i * p.s_req + (uint64_t) k * p.s_hdr];
    const uint32_t noff = h.x & 0xffffu, nl = h.x >> 16, voff = h.y & 0xffffu, vl = h.y >> 16;
    if (noff == RHP_NAME_NULL) continue;   /* name == NULL: an obs-fold line */
    uint32_t cand = nl <= RHP_CLASSIFY_NAME_MAX ? lenmask[nl] & ~found : 0u;
    if (voff + vl > (uint32_t) ret) cand &= callers;   /* (a parsed value lies inside its header section) */
    if (cand == 0) continue;
    if (noff + nl > (uint32_t) ret) continue;          /* (and so does a parsed name) */
    cand = same_text<true>(p.bytes + at0 + noff, nl, cand, tab, text_at);
    for (uint32_t c = cand & callers; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = h.y;
    if (cand & kTeBit) te = h.y;
    if (cand & kClBit) cl = h.y;
    found |= cand;
  }
  for (uint32_t c = callers & ~found; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = RHP_NAME_NULL;

  /* ---- the decision (rhp_scalar.h frame_of_values) and the one value it reads ---- */
  int32_t result = rhp::http_result_of(ret);   /* ret <= 0, or a message that does not lie inside the batch's bytes: 0 */
  uint32_t kind = RHP_FRAME_NONE;
  uint64_t body_len = 0;
  if (ready) {
    const uint32_t te_len = te >> 16, cl_len = cl >> 16;
    bool chunked = false;
    uint64_t number = 0;
    if (cl_len) {
      if (!te_len) number = value_number(p.bytes + at0 + (cl & 0xffffu), cl_len);
    } else if (te_len == kChunkedLen) {
      chunked = same_text<true>(p.bytes + at0 + (te & 0xffffu), kChunkedLen, 1u, tab, [](uint32_t) { return kChunkedAt; }) != 0;
    }
    result = rhp::frame_of_values(te_len, cl_len, chunked, number, &kind, &body_len);
  }
  p.frames[i] = uint4{(uint32_t) result, kind, (uint32_t) body_len, (uint32_t) (body_len >> 32)};
  if (p.decoders && kind == RHP_FRAME_CHUNKED) p.decoders[i] = uint4{0u, 0u, p.consume_trailer, 0u};
}

/* ---- rhp_lookup_walked ---- */

struct WParams {
  CTables         t;          /* first, as CParams */
  const uint8_t  *bytes;
  const uint64_t *sess_off, *slot_off;
  uint64_t        readable;   /* rhp_lookup_readable */
  const uint4    *msgs;
  const uint2    *hdrs;
  const uint4    *slots;      /* two per slot */
  const uint4    *results;
  uint32_t       *fields;
  uint32_t        n, m, n_names, n_sessions;
};
static_assert(offsetof(WParams, t) == 0, "the tables lead the argument");
static_assert(sizeof(WParams) <= 4096, "a kernel argument holds 4 KiB");
static_assert(sizeof(rhp_walk_slot_t) == 32 && offsetof(rhp_walk_slot_t, start) == 0 && offsetof(rhp_walk_slot_t, result) == 24 &&
              sizeof(rhp_walk_result_t) == 16 && offsetof(rhp_walk_result_t, n_slots) == 0, "records as 16-byte accesses");

/* One slot of the walk per lane, rhp_classify_sessions_kernel's mapping over
 * the records rhp_walk_responses / rhp_walk_resume left: the lane finds the
 * last session whose slot_off is at or below its slot and tests that the slot
 * is one that session's walk wrote (rhp_lookup_args.h: the test that lets a
 * load through, whatever the search returned); only then it loads msgs[i] as
 * one 16-byte load and the slot's start and result from its two halves, and,
 * for a head that lies inside its session's bytes, walks the rhp_hdr_t records
 * k < num_headers (request-major, 8-byte loads) -- name_len against the length
 * mask, the name's bytes only on a length match -- until every name is found.
 * A slot the walk did not write holds stale records or nothing and is never
 * read. */
__global__ __launch_bounds__(256) void rhp_lookup_walked_kernel(WParams p)
{
  __shared__ uint32_t tab[kTabDwords];
  __shared__ uint16_t lenmask[RHP_CLASSIFY_NAME_MAX + 1u];
  {
#if defined(__HIP_DEVICE_COMPILE__)   /* (as rhp_classify_kernel) */
    const ka32 *ka = (const ka32 *) __builtin_amdgcn_kernarg_segment_ptr();
#else
    const ka32 *ka = nullptr;
#endif
    for (uint32_t t = threadIdx.x; t < kTabDwords; t += blockDim.x) tab[t] = ka[t];
    if (threadIdx.x <= RHP_CLASSIFY_NAME_MAX) {
      const ka32 *nl = ka + offsetof(CTables, name_len) / 4u;
      uint32_t mk = 0;
      for (uint32_t j = 0; j < p.n_names; j++) mk |= (((nl[j >> 2] >> (8u * (j & 3u))) & 0xffu) == threadIdx.x ? 1u : 0u) << j;
      lenmask[threadIdx.x] = (uint16_t) mk;
    }
  }
  __syncthreads();
  const uint32_t *names = tab + offsetof(CTables, name) / 4u;

  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, n = p.n, m = p.m;
  if (i >= n) return;

  /* ---- the slot's session: the sessions before `above` have slot_off <= i ---- */
  const uint32_t above = rhp_lookup_sessions_upto(p.slot_off, p.n_sessions, i);

  /* ---- in use?  a head?  inside its session?  then its first byte and its records ---- */
  int32_t ret = 0;
  uint32_t nh = 0;
  uint64_t at0 = 0;
  if (above) {
    const uint32_t s = above - 1u;
    const uint64_t lo = p.slot_off[s], hi = p.slot_off[s + 1u];
    const uint32_t n_slots = p.results[s].x;
    if (rhp_lookup_in_use(i, lo, hi, n_slots, n)) {
      const uint4 q = p.msgs[i], s0 = p.slots[2u * (uint64_t) i], s1 = p.slots[2u * (uint64_t) i + 1u];
      const uint64_t st = (uint64_t) s0.x | (uint64_t) s0.y << 32;
      if (rhp_lookup_is_head((int32_t) s1.z, (int32_t) q.x) &&
          rhp_lookup_inside(st, (int32_t) q.x, p.sess_off[s], p.sess_off[s + 1u], p.readable)) {
        ret = (int32_t) q.x;
        at0 = st;
        nh = q.w & 0xffffu;
      }
    }
  }
  if (nh > m) nh = m;   /* never more records than the batch holds */

  /* ---- header lookup over rhp_hdr_t records ---- */
  const uint32_t all = (1u << p.n_names) - 1u;
  uint32_t found = 0;
  for (uint32_t k = 0; k < nh && found != all; k++) {
    const uint2 h = p.hdrs[(uint64_t) i * m + k];
    const uint32_t noff = h.x & 0xffffu, nl = h.x >> 16;
    if (noff == RHP_NAME_NULL) continue;   /* name == NULL: an obs-fold line */
    uint32_t cand = nl <= RHP_CLASSIFY_NAME_MAX ? (uint32_t) lenmask[nl] & ~found : 0u;
    if (cand == 0) continue;
    if (noff + nl > (uint32_t) ret) continue;   /* (a parsed name lies inside its header section) */
    cand = same_text<true>(p.bytes + at0 + noff, nl, cand, names, [](uint32_t j) { return j * kNameDwords; });
    for (uint32_t c = cand; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = h.y;
    found |= cand;
  }
  for (uint32_t c = all & ~found; c; c &= c - 1u) p.fields[(uint64_t) __builtin_ctz(c) * n + i] = RHP_NAME_NULL;
}

/* ---- rhp_relay_walked ---- */

/* the three names that are always dropped take the tables' last three rows and
 * mask bits, the caller's the first RHP_RELAY_MAX_NAMES */
constexpr uint32_t kTypeRow = RHP_RELAY_MAX_NAMES, kLengthRow = kTypeRow + 1u, kTeRow = kTypeRow + 2u;
static_assert(kTeRow + 1u == RHP_CLASSIFY_MAX_NAMES, "sixteen rows, sixteen mask bits");

struct RParams {
  CTables         t;          /* first, as CParams */
  const uint8_t  *bytes;
  const uint64_t *sess_off, *slot_off;
  uint64_t        head_readable, readable;   /* rhp_lookup_readable, rhp_relay_readable */
  const uint4    *msgs;
  const uint2    *hdrs;
  const uint4    *slots;      /* two per slot */
  const uint4    *results;
  uint64_t       *out_off, *tile_sum, *plan;   /* plan: two words per slot */
  uint32_t       *why;
  uint32_t        n, m, flags, n_sessions;
};
static_assert(offsetof(RParams, t) == 0, "the tables lead the argument");
static_assert(sizeof(RParams) <= 4096, "a kernel argument holds 4 KiB");
static_assert(offsetof(rhp_walk_slot_t, body_len) == 8 && offsetof(rhp_walk_slot_t, wire_len) == 16 && offsetof(rhp_walk_slot_t, body_kind) == 28 &&
              offsetof(rhp_walk_result_t, stop) == 4 && offsetof(rhp_msg_t, status) == 4 && offsetof(rhp_msg_t, msg_off) == 6 &&
              offsetof(rhp_msg_t, msg_len) == 8, "records as 16-byte accesses");

/* The sizes step: a tile of kTile slots per workgroup (the scan's tiles,
 * rhp_device.h), a slot per lane and round.  rhp_lookup_walked_kernel's way to
 * a head -- owner, in use, head, inside, and only then the records -- then the
 * rule of rhp_relay_args.h: one pass over the head's rhp_hdr_t records that
 * looks for an obs-fold line and a stray span and compares each name, by
 * length first, with the sixteen rows.  It leaves why[i], the size in
 * out_off[i + 1], the tile's sum, and for a relayed slot the plan the copy step
 * reads: the kept records as a bit mask and the type's value. */
__global__ __launch_bounds__(1024) void rhp_relay_sizes_kernel(RParams p)
{
  __shared__ uint32_t tab[kTabDwords];
  __shared__ uint16_t lenmask[RHP_CLASSIFY_NAME_MAX + 1u];
  __shared__ unsigned long long part[16];
  {
#if defined(__HIP_DEVICE_COMPILE__)   /* (as rhp_classify_kernel) */
    const ka32 *ka = (const ka32 *) __builtin_amdgcn_kernarg_segment_ptr();
#else
    const ka32 *ka = nullptr;
#endif
    for (uint32_t t = threadIdx.x; t < kTabDwords; t += blockDim.x) tab[t] = ka[t];
    if (threadIdx.x <= RHP_CLASSIFY_NAME_MAX) {
      const ka32 *nl = ka + offsetof(CTables, name_len) / 4u;
      uint32_t mk = 0;
      for (uint32_t j = 0; j < RHP_CLASSIFY_MAX_NAMES; j++) {   /* (a row not in use has length 0) */
        const uint32_t len = (nl[j >> 2] >> (8u * (j & 3u))) & 0xffu;
        mk |= (len != 0u && len == threadIdx.x ? 1u : 0u) << j;
      }
      lenmask[threadIdx.x] = (uint16_t) mk;
    }
  }
  __syncthreads();
  const uint32_t *names = tab + offsetof(CTables, name) / 4u;
  const uint32_t n = p.n, m = p.m;

  unsigned long long sum = 0;
  const uint64_t lo_i = (uint64_t) blockIdx.x * rhp_device::kTile, hi_i = min(lo_i + rhp_device::kTile, (uint64_t) n);
  for (uint64_t i64 = lo_i + threadIdx.x; i64 < hi_i; i64 += 1024) {
    const uint32_t i = (uint32_t) i64;
    const uint32_t above = rhp_lookup_sessions_upto(p.slot_off, p.n_sessions, i);
    uint32_t why = RHP_RELAY_UNUSED;
    uint64_t size = 0;
    if (above) {
      const uint32_t s = above - 1u;
      const uint64_t lo = p.slot_off[s], hi = p.slot_off[s + 1u];
      const uint4 res = p.results[s];
      if (rhp_lookup_in_use(i, lo, hi, res.x, n)) {
        const uint4 q = p.msgs[i], s0 = p.slots[2u * (uint64_t) i], s1 = p.slots[2u * (uint64_t) i + 1u];
        const uint64_t st = (uint64_t) s0.x | (uint64_t) s0.y << 32, e = p.sess_off[s + 1u];
        const int32_t ret = (int32_t) q.x;
        why = rhp_relay_why_head(1, (int32_t) s1.z, ret, st, p.sess_off[s], e, p.head_readable, q.y & 0xffffu, (uint32_t) (i - lo), res.x, res.y);
        if (why == RHP_RELAY_OK) {
          const uint32_t msg_off = q.y >> 16, msg_len = q.z & 0xffffu;
          uint32_t nh = q.w & 0xffffu;
          if (nh > m) nh = m;   /* never more records than the batch holds */
          bool fold = false, span_bad = msg_len != 0u && !rhp_relay_span_inside(msg_off, msg_len, ret), typed = false;
          uint64_t keep = 0, fields = 0;
          uint32_t type = 0;
          for (uint32_t k = 0; k < nh; k++) {
            const uint2 h = p.hdrs[(uint64_t) i * m + k];
            const uint32_t noff = h.x & 0xffffu, nl = h.x >> 16, voff = h.y & 0xffffu, vl = h.y >> 16;
            if (noff == RHP_NAME_NULL) { fold = true; continue; }   /* name == NULL: an obs-fold line */
            if (!rhp_relay_span_inside(noff, nl, ret) || !rhp_relay_span_inside(voff, vl, ret)) { span_bad = true; continue; }
            if (fold || span_bad) continue;
            uint32_t cand = nl <= RHP_CLASSIFY_NAME_MAX ? (uint32_t) lenmask[nl] : 0u;
            if (cand) cand = same_text<true>(p.bytes + st + noff, nl, cand, names, [](uint32_t j) { return j * kNameDwords; });
            if ((cand >> kTypeRow & 1u) && !typed) {
              typed = true;
              type = h.y;
            }
            if (cand) continue;   /* dropped: every match, not only the first */
            keep |= 1ull << k;
            fields += rhp_relay_size_field(nl, vl);
          }
          const uint64_t body_len = (uint64_t) s0.z | (uint64_t) s0.w << 32, wire_len = (uint64_t) s1.x | (uint64_t) s1.y << 32;
          why = rhp_relay_why_body(fold, span_bad, s1.w, body_len, wire_len, p.flags, st, ret, e, p.readable);
          if (why == RHP_RELAY_OK) {
            size = rhp_relay_size_head(msg_len, type >> 16, (uint32_t) body_len) + fields;
            p.plan[2u * (uint64_t) i] = keep;
            p.plan[2u * (uint64_t) i + 1u] = type;
          }
        }
      }
    }
    p.why[i] = why;
    p.out_off[i64 + 1u] = size;
    sum += size;
  }
  rhp_device::block_sum_to(sum, part, &p.tile_sum[blockIdx.x]);
}

struct RWParams {
  const uint8_t  *bytes;
  const uint4    *msgs;
  const uint2    *hdrs;
  const uint4    *slots;
  const uint64_t *out_off, *plan;
  uint8_t        *out;
  uint64_t        out_size;
  uint32_t        n, m;
  uint32_t        date[8];   /* the 29 date bytes, little-endian in dwords */
};

/* what the copy step needs of a relayed slot (one with a size): every span is
 * inside the batch's bytes, the sizes step has seen to that */
struct RelaySlot {
  const uint8_t *head;
  uint32_t ret, status, msg_off, msg_len, nh, type, body_len;
  uint64_t keep;
};
__device__ __forceinline__ RelaySlot relay_slot(const RWParams &p, uint32_t i)
{
  const uint4 q = p.msgs[i], s0 = p.slots[2u * (uint64_t) i];
  RelaySlot r;
  r.head = p.bytes + ((uint64_t) s0.x | (uint64_t) s0.y << 32);
  r.ret = q.x;
  r.status = q.y & 0xffffu;
  r.msg_off = q.y >> 16;
  r.msg_len = q.z & 0xffffu;
  r.nh = min(q.w & 0xffffu, p.m);
  r.body_len = s0.z;   /* below 2^32 */
  r.keep = p.plan[2u * (uint64_t) i];
  r.type = (uint32_t) p.plan[2u * (uint64_t) i + 1u];
  return r;
}

/* one reply, wave-cooperatively (the path for groups larger than the stage):
 * rhp_writer.hip's write_one over a walked slot */
__device__ void relay_one(const RWParams &p, uint32_t i, uint32_t lane)
{
  using rhp_device::put;
  using rhp_device::put_const;
  uint64_t o = p.out_off[i];
  if (p.out_off[i + 1u] == o) return;   /* not relayed */
  uint8_t *dst = p.out;
  const RelaySlot r = relay_slot(p, i);
  const auto span = [&](uint32_t off, uint32_t len) {
    put(dst + o, r.head + off, len, lane);
    o += len;
  };
  put_const(dst, o, "HTTP/1.1 ", lane);
  if (lane < 3) dst[o + lane] = (uint8_t) ('0' + (lane == 0 ? r.status / 100u : lane == 1 ? r.status / 10u : r.status) % 10u);
  o += 3;
  if (r.msg_len) {
    if (lane == 0) dst[o] = ' ';
    o += 1;
    span(r.msg_off, r.msg_len);
  }
  put_const(dst, o, "\r\nServer: *\r\nDate: ", lane);
  if (lane < RHP_DATE_LEN) dst[o + lane] = (uint8_t) (p.date[lane >> 2] >> (8u * (lane & 3u)));
  o += RHP_DATE_LEN;
  put_const(dst, o, "\r\nContent-Type: ", lane);
  span(r.type & 0xffffu, r.type >> 16);
  put_const(dst, o, "\r\nContent-Length: ", lane);
  const uint32_t D = rhp_u32_len(r.body_len);   /* http_u32_sprint: most significant first */
  if (lane < D) {
    uint32_t x = r.body_len;
    for (uint32_t q = D - 1u; q > lane; q--) x /= 10u;
    dst[o + lane] = (uint8_t) ('0' + x % 10u);
  }
  o += D;
  put_const(dst, o, "\r\n", lane);
  for (uint64_t c = r.keep; c; c &= c - 1u) {   /* http_push_field (http.c:61-69) */
    const uint32_t k = (uint32_t) __builtin_ctzll(c);
    if (k >= r.nh) break;
    const uint2 h = p.hdrs[(uint64_t) i * p.m + k];
    span(h.x & 0xffffu, h.x >> 16);
    put_const(dst, o, ": ", lane);
    span(h.y & 0xffffu, h.y >> 16);
    put_const(dst, o, "\r\n", lane);
  }
  put_const(dst, o, "\r\n", lane);   /* the empty line */
  span(r.ret, r.body_len);
}

constexpr uint32_t kRelayStage = 16384;   /* LDS bytes per wave, as rhp_writer.hip's: groups up to 16 KiB - 16 */

/* The copy step, rhp_resp_write_kernel's plan over the walked slots: a wave per
 * 64 consecutive slots; each lane assembles its slot's reply, if it has one, in
 * the wave's LDS stage in the reference's push order, then the wave stores the
 * group's contiguous output with 16-byte stores (flush_stage, rhp_device.h).  A
 * group larger than the stage is written reply by reply, the wave's 64 lanes
 * copying each segment. */
__global__ __launch_bounds__(256) void rhp_relay_write_kernel(RWParams p)
{
  using namespace rhp_device;
  __shared__ __attribute__((aligned(16))) uint8_t stage_all[4 * kRelayStage];
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  if (p.out_off[p.n] > p.out_size) return;   /* does not fit: sizes only (rhp.h) */
  lds8 *L = (lds8 *) (stage_all + wv * kRelayStage);
  const uint32_t groups = (p.n + 63u) / 64u;
  for (uint32_t g = wave; g < groups; g += nwaves) {
    const uint32_t i0 = g * 64u, i1 = min(i0 + 64u, p.n);
    const uint64_t G0 = p.out_off[i0], G1 = p.out_off[i1];
    if (G0 == G1) continue;   /* no slot of the group is relayed */
    const uint32_t shift = (uint32_t) (uintptr_t) (p.out + G0) & 15u;   /* LDS and HBM agree modulo 16 */
    if (G1 - G0 + shift > kRelayStage) {   /* big replies: the cooperative path */
      for (uint32_t i = i0; i < i1; i++) relay_one(p, i, lane);
      continue;
    }
    const uint32_t i = i0 + lane;
    if (i < i1) {
      const uint64_t at = p.out_off[i];
      if (p.out_off[i + 1u] != at) {
        const RelaySlot r = relay_slot(p, i);
        uint32_t o = shift + (uint32_t) (at - G0);
        st_const(L, o, "HTTP/1.1 ");
        L[o] = (uint8_t) ('0' + r.status / 100u % 10u);
        L[o + 1] = (uint8_t) ('0' + r.status / 10u % 10u);
        L[o + 2] = (uint8_t) ('0' + r.status % 10u);
        o += 3;
        if (r.msg_len) {
          L[o++] = ' ';
          st_span(L, o, r.head + r.msg_off, r.msg_len);
        }
        st_const(L, o, "\r\nServer: *\r\nDate: ");
#pragma unroll
        for (uint32_t j = 0; j < RHP_DATE_LEN; j++) L[o + j] = (uint8_t) (p.date[j >> 2] >> (8u * (j & 3u)));
        o += RHP_DATE_LEN;
        st_const(L, o, "\r\nContent-Type: ");
        st_span(L, o, r.head + (r.type & 0xffffu), r.type >> 16);
        st_const(L, o, "\r\nContent-Length: ");
        const uint32_t D = rhp_u32_len(r.body_len);   /* http_u32_sprint: most significant first */
        for (uint32_t j = D, x = r.body_len; j-- > 0; x /= 10u) L[o + j] = (uint8_t) ('0' + x % 10u);
        o += D;
        st_const(L, o, "\r\n");
        for (uint64_t c = r.keep; c; c &= c - 1u) {   /* http_push_field (http.c:61-69) */
          const uint32_t k = (uint32_t) __builtin_ctzll(c);
          if (k >= r.nh) break;
          const uint2 h = p.hdrs[(uint64_t) i * p.m + k];
          st_span(L, o, r.head + (h.x & 0xffffu), h.x >> 16);
          st_const(L, o, ": ");
          st_span(L, o, r.head + (h.y & 0xffffu), h.y >> 16);
          st_const(L, o, "\r\n");
        }
        st_const(L, o, "\r\n");   /* the empty line */
        st_span(L, o, r.head + r.ret, r.body_len);
      }
    }
    flush_stage(L, shift, p.out, G0, G1, lane);
  }
}

}  // namespace

/* the call; ev: NULL, or four events recorded before the sizes step, behind it,
 * behind the two scan kernels and behind the copy step (rhp_relay_walked_steps) */
static int relay_launch(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, hipStream_t s, hipEvent_t *ev)
{
  const int rc = rhp_relay_check(w, r, 1);
  if (rc < 0) return rc;
  if (rc != 0) {   /* no slot: out_off[0] = 0, one 8-byte memset node and no kernel */
    if (ev) return -22;
    return (int) hipMemsetAsync(r->out_off, 0, sizeof(uint64_t), s);
  }
  const uint32_t n = w->n_slots_total, tiles = (n + rhp_device::kTile - 1u) / rhp_device::kTile;
  RParams p;
  const rhp_classify_t names = {r->text, r->names, nullptr, r->n_names, 0, nullptr, nullptr};
  pack_tables(&names, p.t);
  const char *const builtin[3] = {RHP_RELAY_TYPE_NAME, RHP_RELAY_LENGTH_NAME, RHP_RELAY_TE_NAME};   /* rows kTypeRow.. */
  for (uint32_t j = 0; j < 3u; j++) pack_name(p.t, kTypeRow + j, (const uint8_t *) builtin[j], (uint32_t) strlen(builtin[j]));
  p.bytes = w->bytes;
  p.sess_off = w->sess_off;
  p.slot_off = w->slot_off;
  p.head_readable = rhp_lookup_readable(w->bytes_size);
  p.readable = rhp_relay_readable(w->bytes_size);
  p.msgs = reinterpret_cast<const uint4 *>(w->msgs);
  p.hdrs = reinterpret_cast<const uint2 *>(w->hdrs);
  p.slots = reinterpret_cast<const uint4 *>(w->slots);
  p.results = reinterpret_cast<const uint4 *>(w->results);
  p.out_off = r->out_off;
  p.tile_sum = r->work;
  p.plan = r->work + tiles + 1u;
  p.why = r->why;
  p.n = n;
  p.m = w->max_headers;
  p.flags = w->flags;
  p.n_sessions = w->n_sessions;
  RWParams q;
  q.bytes = w->bytes;
  q.msgs = p.msgs;
  q.hdrs = p.hdrs;
  q.slots = p.slots;
  q.out_off = r->out_off;
  q.plan = p.plan;
  q.out = r->out;
  q.out_size = r->out_size;
  q.n = n;
  q.m = w->max_headers;
  memset(q.date, 0, sizeof q.date);
  memcpy(q.date, r->date, RHP_DATE_LEN);
  if (ev) (void) hipEventRecord(ev[0], s);
  hipLaunchKernelGGL(rhp_relay_sizes_kernel, dim3(tiles), dim3(1024), 0, s, p);
  if (ev) (void) hipEventRecord(ev[1], s);
  hipLaunchKernelGGL(rhp_device::rhp_resp_top_scan_kernel, dim3(1), dim3(1024), 0, s, r->work, tiles);
  hipLaunchKernelGGL(rhp_device::rhp_resp_tile_scan_kernel, dim3(tiles), dim3(1024), 0, s, r->out_off, n, (const uint64_t *) r->work);
  if (ev) (void) hipEventRecord(ev[2], s);
  /* 4 waves per workgroup, a wave per 64 slots */
  hipLaunchKernelGGL(rhp_relay_write_kernel, dim3((uint32_t) (((uint64_t) n + 255u) / 256u)), dim3(256), 0, s, q);
  if (ev) (void) hipEventRecord(ev[3], s);
  return (int) hipGetLastError();
}

extern "C" int rhp_relay_walked(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, void *stream)
{
  return relay_launch(w, r, reinterpret_cast<hipStream_t>(stream), nullptr);
}

/* the call with a HIP event between its steps, for measuring (rhp.h): it
 * creates and destroys its events and waits for the stream */
extern "C" int rhp_relay_walked_steps(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, void *stream, float us[3])
{
  if (!us) return -22;
  int rc = rhp_relay_check(w, r, 1);   /* (the refusals come before anything is created) */
  if (rc != 0) return -22;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int k = 0; k < 4 && rc == 0; k++) rc = (int) hipEventCreate(&ev[k]);
  if (rc == 0) rc = relay_launch(w, r, reinterpret_cast<hipStream_t>(stream), ev);
  if (rc == 0) rc = (int) hipEventSynchronize(ev[3]);
  for (int k = 0; k < 3 && rc == 0; k++) {
    float ms = 0;
    rc = (int) hipEventElapsedTime(&ms, ev[k], ev[k + 1]);
    us[k] = ms * 1e3f;
  }
  for (int k = 0; k < 4; k++)
    if (ev[k]) (void) hipEventDestroy(ev[k]);
  return rc;
}

extern "C" int rhp_classify_batch(const rhp_batch_t *b, const rhp_classify_t *c, void *stream)
{
  const int rc = rhp_classify_check(b, c);
  if (rc != 0) return rc < 0 ? rc : 0;
  const bool http_mode = b->mode == RHP_MODE_HTTP;
  CParams p;
  fill_params(p, b, c, http_mode && b->bytes_rw ? b->bytes_rw : b->bytes, http_mode ? b->http : nullptr);
  hipLaunchKernelGGL(rhp_classify_kernel, dim3((b->n + 255u) / 256u), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  return (int) hipGetLastError();
}

extern "C" int rhp_classify_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                     const rhp_session_result_t *results, const uint64_t *req_start,
                                     const rhp_classify_t *c, void *stream)
{
  const int rc = rhp_classify_sessions_check(b, sessions, n_sessions, results, req_start, c);
  if (rc != 0) return rc < 0 ? rc : 0;
  SParams p;
  fill_params(p, b, c, b->bytes_rw ? b->bytes_rw : b->bytes, b->http);   /* (a speculative batch is an http one) */
  p.sessions = sessions;
  p.results = results;
  p.req_start = req_start;
  p.n_sessions = n_sessions;
  hipLaunchKernelGGL(rhp_classify_sessions_kernel, dim3((b->n + 255u) / 256u), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  return (int) hipGetLastError();
}

extern "C" int rhp_frame_messages(const rhp_msg_batch_t *b, const rhp_frame_args_t *f, void *stream)
{
  const int rc = rhp_frame_check(b, f, 1);
  if (rc != 0) return rc < 0 ? rc : 0;
  const bool hmajor = b->layout == RHP_LAYOUT_HEADER_MAJOR;
  FParams p;
  const rhp_classify_t names = {f->text, f->names, nullptr, f->n_names, 0, nullptr, nullptr};
  pack_tables(&names, p.t);
  uint8_t *text = reinterpret_cast<uint8_t *>(p.t.text);
  memcpy(text + 4u * (kTeAt - kTextAt), "TRANSFER-ENCODING", kTeLen);
  memcpy(text + 4u * (kClAt - kTextAt), "CONTENT-LENGTH", kClLen);
  memcpy(text + 4u * (kChunkedAt - kTextAt), "CHUNKED", kChunkedLen);
  p.bytes = b->bytes;
  p.offsets = b->offsets;
  p.readable = rhp_frame_readable(b);
  p.msgs = reinterpret_cast<const uint4 *>(b->msgs);
  p.hdrs = reinterpret_cast<const uint2 *>(b->hdrs);
  p.fields = reinterpret_cast<uint32_t *>(f->fields);
  p.frames = reinterpret_cast<uint4 *>(f->frames);
  p.decoders = reinterpret_cast<uint4 *>(f->decoders);
  p.n = b->n;
  p.m = b->max_headers;
  p.n_names = f->n_names;
  p.consume_trailer = f->consume_trailer;
  p.s_req = hmajor ? 1u : b->max_headers;
  p.s_hdr = hmajor ? b->n : 1u;
  hipLaunchKernelGGL(rhp_frame_messages_kernel, dim3((uint32_t) (((uint64_t) b->n + 255u) / 256u)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  return (int) hipGetLastError();
}

extern "C" int rhp_lookup_walked(const rhp_walk_batch_t *w, const rhp_walk_lookup_t *l, void *stream)
{
  const int rc = rhp_lookup_walked_check(w, l, 1);
  if (rc != 0) return rc < 0 ? rc : 0;
  WParams p;
  const rhp_classify_t names = {l->text, l->names, nullptr, l->n_names, 0, nullptr, nullptr};
  pack_tables(&names, p.t);
  p.bytes = w->bytes;
  p.sess_off = w->sess_off;
  p.slot_off = w->slot_off;
  p.readable = rhp_lookup_readable(w->bytes_size);
  p.msgs = reinterpret_cast<const uint4 *>(w->msgs);
  p.hdrs = reinterpret_cast<const uint2 *>(w->hdrs);
  p.slots = reinterpret_cast<const uint4 *>(w->slots);
  p.results = reinterpret_cast<const uint4 *>(w->results);
  p.fields = reinterpret_cast<uint32_t *>(l->fields);
  p.n = w->n_slots_total;
  p.m = w->max_headers;
  p.n_names = l->n_names;
  p.n_sessions = w->n_sessions;
  hipLaunchKernelGGL(rhp_lookup_walked_kernel, dim3((uint32_t) (((uint64_t) w->n_slots_total + 255u) / 256u)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  return (int) hipGetLastError();
}
