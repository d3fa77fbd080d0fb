/*
 * rhp_gather.hip -- rhp_gather_wide (rhp.h): the records of a round's wide slots
 * and the chunked bodies the fix-up de-framed, gathered into three small
 * contiguous areas of HBM, so that the round's one D2H carries them.  gfx950.
 *
 * One record slot per lane, a wave per 64 consecutive slots.  The common round
 * has few or no wide slots, so the cost is the scan over the n slots: a wave
 * reads its slots' hc and dreq (16 B per slot, coalesced) and only when one of
 * them carries a wide mark looks for the sessions that own its slots.  Three
 * launches, reduce-then-scan over the triple (wide slots, header records, body
 * bytes), which is plain addition:
 *
 *   rhp_gather_sums_kernel  per wave: the marks, the owning sessions of the
 *                           marked slots, the wave's three sums and two masks
 *                           (wide; wide with a body to gather) into work[]
 *   rhp_gather_top_kernel   one workgroup: the exclusive prefix of the waves'
 *                           sums in place, *totals.  A thread takes a run of
 *                           consecutive waves, the 1024 runs are scanned in LDS
 *                           (a round of more than kTopSlots slots gives a
 *                           thread more than one wave's sums)
 *   rhp_gather_copy_kernel  per wave with a wide slot, when the totals fit the
 *                           caps: a wide lane's offsets by a scan inside the
 *                           wave, its 64-byte record as four 16-byte stores,
 *                           then the wave copies each wide slot's header
 *                           records (a lane per record) and each body (put():
 *                           16 bytes per lane, bytes at the two edges)
 *
 * The session search is rhp_classify_sessions_kernel's bisection
 * (sessions_upto, rhp_device.h), per marked lane; the session's fields as
 * loaded must contain the slot before anything of the slot's records is read
 * (in_use(), rhp_device.h).  A search once per wave
 * (a 64-way search for the wave's first slot, 64 sessions from there in LDS, a
 * bisection in LDS per lane) was built and measured: it was no faster at any
 * round size and 3 % slower with 65536 sessions, so it is not here.
 *
 * With the sessions out of order the sums may count anything; every offset is
 * still a prefix sum of the lengths that are copied, the copy runs only when
 * the totals fit the caps, and the copy kernel takes its lengths from the same
 * records and masks as the sums: nothing is written outside [0, cap) of an
 * area.  put() is rhp_device.h's too, shared with rhp_reply.hip and
 * rhp_writer.hip.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rhp.h"
#include "rhp_device.h"
#include "rhp_gather_args.h"

namespace {

using namespace rhp_device;

struct GParams {
  const uint8_t              *bytes;     /* bytes_rw when set */
  const uint64_t             *offsets;
  const rhp_req_t            *reqs;
  const rhp_hdr_t            *hdrs;
  const rhp_http_t           *http;
  const rhp_session_t        *sessions;
  const rhp_session_result_t *results;
  const uint64_t             *req_start;
  const uint2                *dreq, *hc;
  rhp_wide_totals_t          *totals;
  rhp_wide_slot_t            *slots;
  rhp_hdr_t                  *out_hdrs;
  uint8_t                    *body;
  uint64_t                    cap_body;
  uint64_t *agg;     /* work: [3 * groups] a wave's wide slots, header records, body bytes; after the top scan their exclusive prefix */
  uint64_t *wmask;   /* work: [groups] bit l: slot 64 g + l is wide */
  uint64_t *bmask;   /* work: [groups] bit l: it has a body to gather */
  uint32_t  n, n_sessions, max_headers, groups, cap_slots, cap_hdrs;
};

constexpr uint32_t kTopThreads = 1024;
constexpr uint32_t kTopSlots = kTopThreads * 64u;   /* above it rhp_gather_top_kernel gives a thread more than one wave's sums */

struct Owner {
  bool     ok;
  uint32_t lo, hi;   /* piece_lo, piece_hi */
};

/* the session that owns slot i: the last whose piece_lo <= i, when its fields contain i */
__device__ __forceinline__ Owner owner_of(const GParams &p, uint32_t i)
{
  const uint32_t above = sessions_upto(p.sessions, p.n_sessions, i);
  if (!above) return Owner{false, 0, 0};
  const uint2 se = reinterpret_cast<const uint2 *>(p.sessions)[above - 1u];
  return Owner{in_use(i, se.x, se.y, p.results[above - 1u].n_slots, p.n), se.x, se.y};
}

/* the wide marks of slot i < n (rhp.h): hc.flags & RHP_HTTP_WIDE, or hc.result == 1 and dreq.flags & RHP_DENSE_WIDE */
__device__ __forceinline__ bool marked(const GParams &p, uint32_t i)
{
  const uint2 c = p.hc[i], d = p.dreq[i];
  const bool hw = (c.x >> 16) & RHP_HTTP_WIDE;
  return hw || ((c.x & 0xffu) == 1u && ((d.y >> 24) & RHP_DENSE_WIDE));
}

__device__ __forceinline__ uint32_t n_hdrs(const GParams &p, const rhp_req_t &r, const rhp_http_t &x)
{
  return x.result == 1 && r.ret > 0 && r.num_headers <= p.max_headers ? r.num_headers : 0u;
}

__global__ __launch_bounds__(256) void rhp_gather_sums_kernel(GParams p)
{
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + wv);   /* (the same in the whole wave) */
  if (g >= p.groups) return;
  const uint64_t i64 = (uint64_t) g * 64u + lane;
  const bool mark = i64 < p.n && marked(p, (uint32_t) i64);
  unsigned long long cw = 0, ch = 0, cb = 0, wm = 0, bm = 0;
  if (__ballot(mark)) {
    const uint32_t i = g * 64u + lane;   /* (a marked slot is below n: no wrap) */
    const Owner w = mark ? owner_of(p, i) : Owner{false, 0, 0};
    bool has_body = false;
    if (w.ok) {
      const rhp_req_t r = p.reqs[i];
      const rhp_http_t x = p.http[i];
      ch = n_hdrs(p, r, x);
      if (x.result == 1 && x.body_kind == 1u && x.consumed != (uint64_t) (int64_t) r.ret + x.body_len) {
        const uint64_t at = p.req_start[i] + (uint64_t) (int64_t) r.ret, s0 = p.offsets[w.lo], s1 = p.offsets[w.hi];
        has_body = s0 <= at && at <= s1 && x.body_len <= s1 - at;
      }
      if (has_body) cb = x.body_len;
    }
    wm = __ballot(w.ok);
    bm = __ballot(has_body);
    cw = __popcll(wm);
    for (int o = 32; o > 0; o >>= 1) {
      ch += __shfl_xor(ch, o);
      cb += __shfl_xor(cb, o);
    }
  }
  if (lane == 0) {
    p.agg[3u * (uint64_t) g] = cw;
    p.agg[3u * (uint64_t) g + 1u] = ch;
    p.agg[3u * (uint64_t) g + 2u] = cb;
    p.wmask[g] = wm;
    p.bmask[g] = bm;
  }
}

/* one workgroup: every wave's exclusive prefix in place, *totals */
__global__ __launch_bounds__(kTopThreads) void rhp_gather_top_kernel(GParams p)
{
  __shared__ unsigned long long sW[kTopThreads], sH[kTopThreads], sB[kTopThreads];
  const uint32_t t = threadIdx.x;
  const uint64_t groups = p.groups, chunk = (groups + kTopThreads - 1u) / kTopThreads;
  const uint64_t lo = min((uint64_t) t * chunk, groups), hi = min(lo + chunk, groups);
  unsigned long long w = 0, h = 0, b = 0;
  for (uint64_t k = lo; k < hi; k++) w += p.agg[3u * k], h += p.agg[3u * k + 1u], b += p.agg[3u * k + 2u];
  sW[t] = w, sH[t] = h, sB[t] = b;
  __syncthreads();
  for (uint32_t o = 1; o < kTopThreads; o <<= 1) {
    const unsigned long long uw = t >= o ? sW[t - o] : 0, uh = t >= o ? sH[t - o] : 0, ub = t >= o ? sB[t - o] : 0;
    __syncthreads();
    sW[t] += uw, sH[t] += uh, sB[t] += ub;
    __syncthreads();
  }
  w = t ? sW[t - 1u] : 0, h = t ? sH[t - 1u] : 0, b = t ? sB[t - 1u] : 0;
  for (uint64_t k = lo; k < hi; k++) {
    const unsigned long long aw = p.agg[3u * k], ah = p.agg[3u * k + 1u], ab = p.agg[3u * k + 2u];
    p.agg[3u * k] = w, p.agg[3u * k + 1u] = h, p.agg[3u * k + 2u] = b;
    w += aw, h += ah, b += ab;
  }
  if (t == kTopThreads - 1u) {
    /* (in order: n_wide <= n and n_hdrs <= n * max_headers < 2^32; out of order they saturate, and then fit no cap the kernel uses) */
    uint2 c;
    c.x = (uint32_t) min(sW[t], 0xffffffffull);
    c.y = (uint32_t) min(sH[t], 0xffffffffull);
    *reinterpret_cast<uint2 *>(p.totals) = c;
    p.totals->body_bytes = sB[t];
  }
}

__global__ __launch_bounds__(256) void rhp_gather_copy_kernel(GParams p)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
  if (g >= p.groups) return;
  const uint64_t wm = p.wmask[g];
  if (!wm) return;
  const uint2 tot = *reinterpret_cast<const uint2 *>(p.totals);
  const uint64_t tot_body = p.totals->body_bytes;
  if (tot.x > p.cap_slots || tot.y > p.cap_hdrs || tot_body > p.cap_body) return;   /* does not fit: totals only (rhp.h) */
  const uint64_t bm = p.bmask[g] & wm;
  const uint32_t i = g * 64u + lane;   /* (used by wide lanes only: below n) */
  const bool wide = (wm >> lane) & 1u, has_body = (bm >> lane) & 1u;
  rhp_req_t r{};
  rhp_http_t x{};
  uint64_t start = 0;
  if (wide) {
    r = p.reqs[i];
    x = p.http[i];
    start = p.req_start[i];
  }
  const uint32_t nh = wide ? n_hdrs(p, r, x) : 0u;
  const unsigned long long bl = has_body ? x.body_len : 0;
  /* (two sums in one loop: as two calls of wave_incl_scan the call measured 0.7 % slower at 65536 slots) */
  uint32_t hinc = nh;
  unsigned long long binc = bl;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t uh = __shfl_up(hinc, o);
    const unsigned long long ub = __shfl_up(binc, o);
    if ((int) lane >= o) hinc += uh, binc += ub;
  }
  /* the wave's prefix; every offset is held to the totals again, so that a copy stays inside its cap whatever the records say */
  const uint64_t at_slot = p.agg[3u * (uint64_t) g] + __popcll(wm & ((1ull << lane) - 1ull));
  const uint64_t at_hdr = p.agg[3u * (uint64_t) g + 1u] + hinc - nh;
  const uint64_t at_body = p.agg[3u * (uint64_t) g + 2u] + binc - bl;
  const bool fits = wide && at_slot < tot.x && at_hdr + nh <= tot.y && bl <= tot_body && at_body <= tot_body - bl;
  if (fits) {
    rhp_wide_slot_t rec;
    rec.slot = i;
    rec.hdr_first = (uint32_t) at_hdr;
    rec.req = r;
    rec.http = x;
    rec.req_start = start;
    rec.body_off = has_body ? at_body : RHP_WIDE_NO_BODY;
    static_assert(sizeof rec == 64, "one sector per wide slot");
    u32x4 q[4];
    __builtin_memcpy(q, &rec, sizeof rec);
    u32x4 *dst = reinterpret_cast<u32x4 *>(p.slots + at_slot);
    dst[0] = q[0], dst[1] = q[1], dst[2] = q[2], dst[3] = q[3];
  }
  /* the header records: the wave takes its wide slots one after the other, a lane per record */
  const uint64_t hm = __ballot(fits && nh != 0u);
  for (uint64_t m = hm; m; m &= m - 1u) {
    const int j = __builtin_ctzll(m);
    const uint32_t nh_j = __shfl(nh, j);
    const uint64_t to = __shfl((unsigned long long) at_hdr, j);
    if (lane < nh_j) {   /* (nh_j <= max_headers <= 64) */
      const uint2 *src = reinterpret_cast<const uint2 *>(p.hdrs + (uint64_t) (g * 64u + (uint32_t) j) * p.max_headers);
      reinterpret_cast<uint2 *>(p.out_hdrs + to)[lane] = src[lane];
    }
  }
  /* the bodies, each across the wave */
  const uint64_t cm = __ballot(fits && has_body && bl != 0);
  for (uint64_t m = cm; m; m &= m - 1u) {
    const int j = __builtin_ctzll(m);
    const uint64_t to = __shfl((unsigned long long) at_body, j), len = __shfl(bl, j);
    const uint64_t from = __shfl((unsigned long long) (start + (uint64_t) (int64_t) r.ret), j);
    put(p.body + to, p.bytes + from, len, lane);
  }
}

}  // namespace

extern "C" int rhp_gather_wide(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                               const rhp_session_result_t *results, const uint64_t *req_start,
                               const rhp_req_dense_t *dreq, const rhp_http_compact_t *hc, const rhp_wide_out_t *o, void *stream)
{
  const int rc = rhp_gather_wide_check(b, sessions, n_sessions, results, req_start, dreq, hc, o);
  if (rc < 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  GParams p;
  p.bytes = b->bytes_rw ? b->bytes_rw : b->bytes;
  p.offsets = b->offsets;
  p.reqs = b->reqs;
  p.hdrs = b->hdrs;
  p.http = b->http;
  p.sessions = sessions;
  p.results = results;
  p.req_start = req_start;
  p.dreq = reinterpret_cast<const uint2 *>(dreq);
  p.hc = reinterpret_cast<const uint2 *>(hc);
  p.totals = o->totals;
  p.slots = o->slots;
  p.out_hdrs = o->hdrs;
  p.body = o->body;
  p.cap_body = o->cap_body;
  p.n = rc == 1 ? 0u : b->n;   /* no session: no slot is looked at */
  p.n_sessions = n_sessions;
  p.max_headers = b->max_headers;
  p.groups = (uint32_t) (((uint64_t) p.n + 63u) / 64u);
  p.cap_slots = o->cap_slots;
  p.cap_hdrs = o->cap_hdrs;
  p.agg = o->work;
  p.wmask = p.agg + 3u * (uint64_t) p.groups;
  p.bmask = p.wmask + p.groups;
  const uint32_t blocks = (p.groups + 3u) / 4u;
  if (blocks) hipLaunchKernelGGL(rhp_gather_sums_kernel, dim3(blocks), dim3(256), 0, s, p);
  hipLaunchKernelGGL(rhp_gather_top_kernel, dim3(1), dim3(kTopThreads), 0, s, p);
  if (blocks) hipLaunchKernelGGL(rhp_gather_copy_kernel, dim3(blocks), dim3(256), 0, s, p);
  return (int) hipGetLastError();
}
