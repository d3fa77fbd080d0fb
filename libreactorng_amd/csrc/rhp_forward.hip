/*
 * rhp_forward.hip -- rhp_forward_sessions (rhp.h): the requests of a proxied
 * route re-written for the upstream, from the record slots the parse and the
 * fix-up left and rhp_classify_sessions' route[] to request bytes in HBM, and
 * the queue rhp_walk_answers wants of them (fwd_off, head_bits).  gfx950.  The
 * request side's rhp_relay_walked (rhp_classify.hip), in its shape; the rule
 * is rhp_forward_args.h's.
 *
 *   rhp_forward_sizes_kernel  a tile of kTile slots per workgroup, a slot per
 *                             lane and round: rhp_classify_sessions_kernel's
 *                             way to a request (owner, in use, and only then the
 *                             records), the tests in rhp.h's order, one pass
 *                             over the header records against the drop names in
 *                             LDS (rhp_tables.h).  Leaves why[i], the size in
 *                             out_off[i + 1], 0 / 1 in cnt[i + 1], the two tile
 *                             sums, the kept records as a bit mask in plan[i]
 *                             and a wave's HEAD flags in headmask[i / 64]
 *   rhp_device.h's two scan kernels, over the sizes and again over the counts
 *   rhp_forward_queue_kernel  fwd_off[s] from the scanned counts; the words of
 *                             head_bits below (total + 31) / 32 zeroed
 *   rhp_forward_write_kernel  a wave per 64 consecutive slots: the HEAD bits of
 *                             its forwarded slots (atomicOr: a word is shared
 *                             by the waves whose ordinals fall into it), then
 *                             each lane assembles its request in the wave's
 *                             LDS stage and the wave stores the group's
 *                             contiguous output with 16-byte stores; a group
 *                             larger than the stage is written request by
 *                             request, the 64 lanes copying each segment
 *
 * Whatever the searches return, an offset is a prefix sum of the sizes that are
 * written and a size is computed from spans the sizes step has tested, so
 * sessions in any order write nothing outside out[0, out_off[n]).
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rhp.h"
#define RHP_DEVICE_SCAN_KERNELS   /* this file launches rhp_device.h's two scan kernels */
#include "rhp_device.h"
#include "rhp_forward_args.h"
#include "rhp_tables.h"

namespace {

using namespace rhp_device;

/* the two names that are always dropped take the tables' last two rows, the
 * caller's the first RHP_FORWARD_MAX_NAMES */
constexpr uint32_t kLengthRow = RHP_FORWARD_MAX_NAMES, kTeRow = kLengthRow + 1u;
static_assert(kTeRow + 1u == RHP_CLASSIFY_MAX_NAMES, "sixteen rows, sixteen mask bits");

struct FSParams {
  CTables         t;          /* first: the kernel reads it from the start of its argument segment */
  const uint8_t  *bytes;
  const uint64_t *offsets;
  const uint4    *reqs;
  const uint2    *hdrs;
  const uint8_t  *http;
  const rhp_session_t        *sessions;
  const rhp_session_result_t *results;
  const uint64_t *req_start;
  const uint16_t *route;
  uint64_t        readable;   /* rhp_forward_readable */
  uint64_t        s_req, s_hdr;   /* record k of slot i: hdrs[i * s_req + k * s_hdr] */
  uint64_t       *out_off, *tile_sum, *cnt, *cnt_sum, *plan, *headmask;
  uint32_t       *why;
  uint32_t        n, m, n_sessions, n_routes, forward_mask, extra_len;
};
static_assert(offsetof(FSParams, t) == 0, "the tables lead the argument");
static_assert(sizeof(FSParams) <= 4096, "a kernel argument holds 4 KiB");
static_assert(sizeof(rhp_req_t) == 16 && sizeof(rhp_hdr_t) == 8 && sizeof(rhp_http_t) == 24 && offsetof(rhp_http_t, body_kind) == 4 &&
              offsetof(rhp_http_t, body_len) == 16 && offsetof(rhp_req_t, method_len) == 4 && offsetof(rhp_req_t, path_len) == 8 &&
              offsetof(rhp_req_t, num_headers) == 12, "records as 16-, 8- and 8-byte accesses");

/* the four bytes at src, which lie inside a tested span: the aligned dword that
 * holds the first and, only when the four reach it, the next */
__device__ __forceinline__ uint32_t load4(const uint8_t *src)
{
  const uintptr_t a = (uintptr_t) src;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t) 3);
  const uint32_t sh = (uint32_t) a & 3u;
  const uint32_t lo = w[0], hi = sh ? w[1] : 0u;
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
}
constexpr uint32_t kHEAD = 0x44414548u;   /* "HEAD", little-endian */

__global__ __launch_bounds__(1024) void rhp_forward_sizes_kernel(FSParams p)
{
  __shared__ uint32_t tab[kTabDwords];
  __shared__ uint16_t lenmask[RHP_CLASSIFY_NAME_MAX + 1u];
  __shared__ unsigned long long part[16], part2[16];
  {
#if defined(__HIP_DEVICE_COMPILE__)   /* (the host pass only checks the body) */
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
  const uint32_t n = p.n, m = p.m, lane = threadIdx.x & 63u;

  unsigned long long sum = 0, count = 0;
  const uint64_t lo_i = (uint64_t) blockIdx.x * kTile, hi_i = min(lo_i + kTile, (uint64_t) n);
  for (uint64_t i64 = lo_i + threadIdx.x; i64 < hi_i; i64 += 1024) {
    const uint32_t i = (uint32_t) i64;
    const uint32_t above = sessions_upto(p.sessions, p.n_sessions, i);
    uint32_t why = RHP_FORWARD_UNUSED;
    uint64_t size = 0;
    bool head = false;
    if (above) {
      const uint2 se = reinterpret_cast<const uint2 *>(p.sessions)[above - 1u];   /* piece_lo, piece_hi */
      const uint32_t ns = p.results[above - 1u].n_slots;
      if (rhp_forward_in_use(i, se.x, se.y, ns, n)) {
        const uint2 x0 = *reinterpret_cast<const uint2 *>(p.http + (size_t) i * sizeof(rhp_http_t));   /* result, body_kind */
        const uint4 q = p.reqs[i];
        const int32_t ret = (int32_t) q.x;
        why = RHP_FORWARD_NOT_READY;
        if ((int32_t) x0.x == 1 && ret > 0) {
          const uint64_t rs = p.req_start[i], e = p.offsets[se.y];
          why = RHP_FORWARD_OUTSIDE;
          if (rhp_forward_inside(rs, ret, p.offsets[se.x], e, p.readable)) {
            const uint32_t last = rhp_forward_last_slot(se.x, ns, n);
            why = RHP_FORWARD_CLOSED;
            if (!(last < n && *reinterpret_cast<const int32_t *>(p.http + (size_t) last * sizeof(rhp_http_t)) == -1)) {
              why = RHP_FORWARD_ROUTE;
              if (rhp_forward_route(p.route[i], p.n_routes, p.forward_mask)) {
                const uint32_t method_len = q.y & 0xffffu, path_off = q.y >> 16, path_len = q.z & 0xffffu, method_off = (q.z >> 16) & 0xffu;
                uint32_t nh = q.w & 0xffffu;
                if (nh > m) nh = m;   /* never more records than the batch holds */
                bool fold = false, span_bad = !rhp_forward_span_inside(method_off, method_len, ret) || !rhp_forward_span_inside(path_off, path_len, ret);
                uint64_t keep = 0, fields = 0;
                for (uint32_t k = 0; k < nh; k++) {
                  const uint2 h = p.hdrs[(uint64_t) i * p.s_req + (uint64_t) k * p.s_hdr];
                  const uint32_t noff = h.x & 0xffffu, nl = h.x >> 16, voff = h.y & 0xffffu, vl = h.y >> 16;
                  if (noff == RHP_NAME_NULL) { fold = true; continue; }   /* name == NULL: an obs-fold line */
                  if (!rhp_forward_span_inside(noff, nl, ret) || !rhp_forward_span_inside(voff, vl, ret)) { span_bad = true; continue; }
                  if (fold || span_bad) continue;
                  uint32_t cand = nl <= RHP_CLASSIFY_NAME_MAX ? (uint32_t) lenmask[nl] : 0u;
                  if (cand) cand = same_text<true>(p.bytes + rs + noff, nl, cand, names, [](uint32_t j) { return j * kNameDwords; });
                  if (cand) continue;   /* dropped: every match, not only the first */
                  keep |= 1ull << k;
                  fields += rhp_forward_size_field(nl, vl);
                }
                const uint2 x1 = *reinterpret_cast<const uint2 *>(p.http + (size_t) i * sizeof(rhp_http_t) + 16u);   /* body_len */
                const uint64_t body_len = (uint64_t) x1.x | (uint64_t) x1.y << 32;
                why = rhp_forward_why_body(fold, span_bad, x0.y, body_len, rs, ret, e, p.readable);
                if (why == RHP_FORWARD_OK) {
                  size = rhp_forward_size_head(method_len, path_len, x0.y, (uint32_t) body_len, p.extra_len) + fields;
                  head = method_len == 4u && load4(p.bytes + rs + method_off) == kHEAD;
                  p.plan[i] = keep;
                }
              }
            }
          }
        }
      }
    }
    p.why[i] = why;
    p.out_off[i64 + 1u] = size;
    p.cnt[i64 + 1u] = why == RHP_FORWARD_OK ? 1u : 0u;
    sum += size;
    count += why == RHP_FORWARD_OK ? 1u : 0u;
    /* (the wave's lanes that are in the loop hold consecutive slots from a multiple of 64; lane 0 is one of them) */
    const uint64_t hm = __ballot(head);
    if (lane == 0) p.headmask[i >> 6] = hm;
  }
  block_sum_to(sum, part, &p.tile_sum[blockIdx.x]);
  block_sum_to(count, part2, &p.cnt_sum[blockIdx.x]);
}

struct FQParams {
  const rhp_session_t *sessions;
  const uint64_t *cnt;
  uint32_t *fwd_off, *head_bits;
  uint32_t n, n_sessions;
};

/* fwd_off[s]: the forwarded slots below the session's first slot; the words of
 * head_bits the copy step sets bits in, zeroed */
__global__ __launch_bounds__(256) void rhp_forward_queue_kernel(FQParams p)
{
  const uint64_t gid = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t) gridDim.x * blockDim.x;
  const uint64_t total = p.cnt[p.n];   /* <= n */
  for (uint64_t s = gid; s <= p.n_sessions; s += nthreads)
    p.fwd_off[s] = (uint32_t) (s < p.n_sessions ? p.cnt[min(p.sessions[s].piece_lo, p.n)] : total);
  for (uint64_t w = gid; w < (total + 31u) / 32u; w += nthreads) p.head_bits[w] = 0u;
}

struct FWParams {
  uint32_t        extra[RHP_FORWARD_EXTRA_MAX / 4u];   /* first: read from the start of the argument segment; little-endian in dwords */
  const uint8_t  *bytes;
  const uint4    *reqs;
  const uint2    *hdrs;
  const uint8_t  *http;
  const uint64_t *req_start;
  const uint64_t *out_off, *cnt, *plan, *headmask;
  uint8_t        *out;
  uint64_t        out_size;
  uint32_t       *head_bits;
  uint64_t        s_req, s_hdr;
  uint32_t        n, m, extra_len;
};
static_assert(offsetof(FWParams, extra) == 0, "extra leads the argument");

/* what the copy step needs of a forwarded slot (one with a size): every span is
 * inside the batch's bytes, the sizes step has seen to that */
struct ForwardSlot {
  const uint8_t *req;
  uint32_t ret, method_off, method_len, path_off, path_len, nh, body_kind, body_len;
  uint64_t keep;
};
__device__ __forceinline__ ForwardSlot forward_slot(const FWParams &p, uint32_t i)
{
  const uint4 q = p.reqs[i];
  const uint8_t *x = p.http + (size_t) i * sizeof(rhp_http_t);
  ForwardSlot r;
  r.req = p.bytes + p.req_start[i];
  r.ret = q.x;
  r.method_len = q.y & 0xffffu;
  r.path_off = q.y >> 16;
  r.path_len = q.z & 0xffffu;
  r.method_off = (q.z >> 16) & 0xffu;
  r.nh = min(q.w & 0xffffu, p.m);
  r.body_kind = *reinterpret_cast<const uint32_t *>(x + 4u);
  r.body_len = r.body_kind == 1u ? *reinterpret_cast<const uint32_t *>(x + 16u) : 0u;   /* below 2^32 */
  r.keep = p.plan[i];
  return r;
}

/* one request, wave-cooperatively (the path for groups larger than the stage) */
__device__ void forward_one(const FWParams &p, const lds8 *extra, uint32_t i, uint32_t lane)
{
  uint64_t o = p.out_off[i];
  if (p.out_off[i + 1u] == o) return;   /* not forwarded */
  uint8_t *dst = p.out;
  const ForwardSlot r = forward_slot(p, i);
  const auto span = [&](uint32_t off, uint32_t len) {
    put(dst + o, r.req + off, len, lane);
    o += len;
  };
  span(r.method_off, r.method_len);
  put_const(dst, o, " ", lane);
  span(r.path_off, r.path_len);
  put_const(dst, o, " HTTP/1.1\r\n", lane);
  for (uint64_t c = r.keep; c; c &= c - 1u) {   /* http_push_field's form (http.c:63-71) */
    const uint32_t k = (uint32_t) __builtin_ctzll(c);
    if (k >= r.nh) break;
    const uint2 h = p.hdrs[(uint64_t) i * p.s_req + (uint64_t) k * p.s_hdr];
    span(h.x & 0xffffu, h.x >> 16);
    put_const(dst, o, ": ", lane);
    span(h.y & 0xffffu, h.y >> 16);
    put_const(dst, o, "\r\n", lane);
  }
  if (r.body_kind == 1u) {
    put_const(dst, o, "Content-Length: ", lane);
    const uint32_t D = rhp_u32_len(r.body_len);   /* most significant first */
    if (lane < D) {
      uint32_t x = r.body_len;
      for (uint32_t q = D - 1u; q > lane; q--) x /= 10u;
      dst[o + lane] = (uint8_t) ('0' + x % 10u);
    }
    o += D;
    put_const(dst, o, "\r\n", lane);
  }
  for (uint32_t j = lane; j < p.extra_len; j += 64u) dst[o + j] = extra[j];
  o += p.extra_len;
  put_const(dst, o, "\r\n", lane);   /* the empty line */
  span(r.ret, r.body_len);
}

/* LDS bytes per wave: with the 128 bytes of `extra` the workgroup's four stages fill 64 KiB */
constexpr uint32_t kForwardStage = 16384u - RHP_FORWARD_EXTRA_MAX / 4u;
static_assert(kForwardStage % 16u == 0, "a stage starts at a 16-byte line");

__global__ __launch_bounds__(256) void rhp_forward_write_kernel(FWParams p)
{
  __shared__ __attribute__((aligned(16))) uint8_t stage_all[4 * kForwardStage];
  __shared__ uint32_t extra_w[RHP_FORWARD_EXTRA_MAX / 4u];
  {
#if defined(__HIP_DEVICE_COMPILE__)   /* (the host pass only checks the body) */
    const ka32 *ka = (const ka32 *) __builtin_amdgcn_kernarg_segment_ptr();
#else
    const ka32 *ka = nullptr;
#endif
    if (threadIdx.x < RHP_FORWARD_EXTRA_MAX / 4u) extra_w[threadIdx.x] = ka[threadIdx.x];
  }
  __syncthreads();
  const lds8 *extra = (const lds8 *) extra_w;
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  const bool fits = p.out_off[p.n] <= p.out_size;   /* does not fit: sizes and the queue only (rhp.h) */
  lds8 *L = (lds8 *) (stage_all + wv * kForwardStage);
  const uint32_t groups = (uint32_t) (((uint64_t) p.n + 63u) / 64u);
  for (uint32_t g = wave; g < groups; g += nwaves) {
    const uint32_t i0 = g * 64u, i1 = (uint32_t) min((uint64_t) i0 + 64u, (uint64_t) p.n);
    const uint64_t G0 = p.out_off[i0], G1 = p.out_off[i1];
    if (G0 == G1) continue;   /* no slot of the group is forwarded */
    const uint32_t i = i0 + lane;
    uint64_t at = 0;
    bool fwd = false;
    if (i < i1) {
      at = p.out_off[i];
      fwd = p.out_off[i + 1u] != at;
    }
    /* ---- the queue: this lane's request is the q-th forwarded one ---- */
    const uint64_t fm = __ballot(fwd), hm = p.headmask[g];
    if (fwd && ((hm >> lane) & 1u)) {
      const uint64_t q = p.cnt[i0] + (uint32_t) __popcll(fm & ((1ull << lane) - 1u));
      atomicOr(&p.head_bits[q >> 5], 1u << (q & 31u));
    }
    if (!fits) continue;
    /* ---- the bytes ---- */
    const uint32_t shift = (uint32_t) (uintptr_t) (p.out + G0) & 15u;   /* LDS and HBM agree modulo 16 */
    if (G1 - G0 + shift > kForwardStage) {   /* big requests: the cooperative path */
      for (uint32_t j = i0; j < i1; j++) forward_one(p, extra, j, lane);
      continue;
    }
    if (fwd) {
      const ForwardSlot r = forward_slot(p, i);
      uint32_t o = shift + (uint32_t) (at - G0);
      st_span(L, o, r.req + r.method_off, r.method_len);
      L[o++] = ' ';
      st_span(L, o, r.req + r.path_off, r.path_len);
      st_const(L, o, " HTTP/1.1\r\n");
      for (uint64_t c = r.keep; c; c &= c - 1u) {   /* http_push_field's form (http.c:63-71) */
        const uint32_t k = (uint32_t) __builtin_ctzll(c);
        if (k >= r.nh) break;
        const uint2 h = p.hdrs[(uint64_t) i * p.s_req + (uint64_t) k * p.s_hdr];
        st_span(L, o, r.req + (h.x & 0xffffu), h.x >> 16);
        st_const(L, o, ": ");
        st_span(L, o, r.req + (h.y & 0xffffu), h.y >> 16);
        st_const(L, o, "\r\n");
      }
      if (r.body_kind == 1u) {
        st_const(L, o, "Content-Length: ");
        const uint32_t D = rhp_u32_len(r.body_len);   /* most significant first */
        for (uint32_t j = D, x = r.body_len; j-- > 0; x /= 10u) L[o + j] = (uint8_t) ('0' + x % 10u);
        o += D;
        st_const(L, o, "\r\n");
      }
      for (uint32_t j = 0; j < p.extra_len; j++) L[o + j] = extra[j];
      o += p.extra_len;
      st_const(L, o, "\r\n");   /* the empty line */
      st_span(L, o, r.req + r.ret, r.body_len);
    }
    flush_stage(L, shift, p.out, G0, G1, lane);
  }
}

}  // namespace

extern "C" int rhp_forward_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                    const rhp_session_result_t *results, const uint64_t *req_start,
                                    const uint16_t *route, const rhp_forward_t *f, void *stream)
{
  const int rc = rhp_forward_check(b, sessions, n_sessions, results, req_start, route, f, 1);
  if (rc < 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (rc != 0) {   /* no slot, or no session: two memset nodes and no kernel */
    const int e = (int) hipMemsetAsync(f->out_off, 0, sizeof(uint64_t), s);
    if (e != 0) return e;
    return (int) hipMemsetAsync(f->fwd_off, 0, sizeof(uint32_t) * ((size_t) n_sessions + 1u), s);
  }
  const uint32_t n = b->n, tiles = (uint32_t) (((uint64_t) n + kTile - 1u) / kTile);
  const bool hmajor = b->layout == RHP_LAYOUT_HEADER_MAJOR;
  FSParams p;
  const rhp_classify_t names = {f->text, f->names, nullptr, f->n_names, 0, nullptr, nullptr};
  pack_tables(&names, p.t);
  const char *const builtin[2] = {RHP_FORWARD_LENGTH_NAME, RHP_FORWARD_TE_NAME};   /* rows kLengthRow.. */
  for (uint32_t j = 0; j < 2u; j++) pack_name(p.t, kLengthRow + j, (const uint8_t *) builtin[j], (uint32_t) strlen(builtin[j]));
  p.bytes = b->bytes_rw ? b->bytes_rw : b->bytes;
  p.offsets = b->offsets;
  p.reqs = reinterpret_cast<const uint4 *>(b->reqs);
  p.hdrs = reinterpret_cast<const uint2 *>(b->hdrs);
  p.http = reinterpret_cast<const uint8_t *>(b->http);
  p.sessions = sessions;
  p.results = results;
  p.req_start = req_start;
  p.route = route;
  p.readable = rhp_forward_readable(b->bytes_size);
  p.s_req = hmajor ? 1u : b->max_headers;
  p.s_hdr = hmajor ? n : 1u;
  p.out_off = f->out_off;
  p.tile_sum = f->work;
  p.cnt_sum = p.tile_sum + tiles + 1u;
  p.cnt = p.cnt_sum + tiles + 1u;
  p.plan = p.cnt + (uint64_t) n + 1u;
  p.headmask = p.plan + n;
  p.why = f->why;
  p.n = n;
  p.m = b->max_headers;
  p.n_sessions = n_sessions;
  p.n_routes = f->n_routes;
  p.forward_mask = f->forward_mask;
  p.extra_len = f->extra_len;
  FQParams q;
  q.sessions = sessions;
  q.cnt = p.cnt;
  q.fwd_off = f->fwd_off;
  q.head_bits = f->head_bits;
  q.n = n;
  q.n_sessions = n_sessions;
  FWParams w;
  memset(w.extra, 0, sizeof w.extra);
  if (f->extra_len) memcpy(w.extra, f->extra, f->extra_len);
  w.bytes = p.bytes;
  w.reqs = p.reqs;
  w.hdrs = p.hdrs;
  w.http = p.http;
  w.req_start = req_start;
  w.out_off = f->out_off;
  w.cnt = p.cnt;
  w.plan = p.plan;
  w.headmask = p.headmask;
  w.out = f->out;
  w.out_size = f->out_size;
  w.head_bits = f->head_bits;
  w.s_req = p.s_req;
  w.s_hdr = p.s_hdr;
  w.n = n;
  w.m = b->max_headers;
  w.extra_len = f->extra_len;
  hipLaunchKernelGGL(rhp_forward_sizes_kernel, dim3(tiles), dim3(1024), 0, s, p);
  hipLaunchKernelGGL(rhp_resp_top_scan_kernel, dim3(1), dim3(1024), 0, s, p.tile_sum, tiles);
  hipLaunchKernelGGL(rhp_resp_tile_scan_kernel, dim3(tiles), dim3(1024), 0, s, f->out_off, n, (const uint64_t *) p.tile_sum);
  hipLaunchKernelGGL(rhp_resp_top_scan_kernel, dim3(1), dim3(1024), 0, s, p.cnt_sum, tiles);
  hipLaunchKernelGGL(rhp_resp_tile_scan_kernel, dim3(tiles), dim3(1024), 0, s, p.cnt, n, (const uint64_t *) p.cnt_sum);
  /* a thread per session and per 32 slots at the most; the kernel's loops stride over the rest */
  uint64_t qthreads = (uint64_t) n_sessions + 1u;
  if (((uint64_t) n + 31u) / 32u > qthreads) qthreads = ((uint64_t) n + 31u) / 32u;
  uint64_t qblocks = (qthreads + 255u) / 256u;
  if (qblocks > (1u << 20)) qblocks = 1u << 20;
  hipLaunchKernelGGL(rhp_forward_queue_kernel, dim3((uint32_t) qblocks), dim3(256), 0, s, q);
  /* 4 waves per workgroup, a wave per 64 slots */
  hipLaunchKernelGGL(rhp_forward_write_kernel, dim3((uint32_t) (((uint64_t) n + 255u) / 256u)), dim3(256), 0, s, w);
  return (int) hipGetLastError();
}
