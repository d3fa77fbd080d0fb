/*
 * rhp_reply.hip -- rhp_reply_sessions (rhp.h): the replies of static routes,
 * from route[] and the fix-up's session results to each session's reply bytes
 * in HBM.  gfx950.  The reply of a static route is a byte string the caller
 * serialized once (rhp_write_responses), so nothing is assembled here: the
 * kernels decide which record slots are answered, sum their image lengths and
 * copy images.
 *
 * One record slot per lane.  A slot is live when it is in use by a session
 * whose fields hold and whose walk did not stop on -1, and its route is
 * static; its session comes from the search rhp_classify_sessions_kernel does
 * (sessions_upto, rhp_device.h).
 * A slot is answered when every slot from its session's piece_lo up to it is
 * live.  Inside a wave that is bit arithmetic on the ballot of the live flags;
 * only a run that began before the wave's first slot depends on what came
 * before: whether the slot just before the wave was answered.  So a range of
 * slots is a function of that one bit x -- the bit after the range is x itself
 * (P) or a constant (c), the bytes the range adds are S + x * H -- and such
 * functions compose (combine()).  Reduce-then-scan over them, four launches:
 *
 *   rhp_reply_tile_kernel  every slot's session and live flag (kept in work[]
 *                          for the third launch), a wave's function, the
 *                          function of a tile of 256 slots into work[]
 *   rhp_reply_top_kernel   one workgroup composes the tiles' functions from the
 *                          left: each tile's incoming bit and offset; *total
 *   rhp_reply_scan_kernel  every slot's offset into `out` (work[]: n + 1
 *                          offsets, as rhp_write_responses' out_off) and a bit
 *                          per slot: answered
 *   rhp_reply_copy_kernel  a thread per session writes replies[s] (the
 *                          answered slots are a prefix of the session's: a
 *                          bisection over the bits); a wave per 64 slots copies
 *                          their images: each lane its own into the wave's LDS
 *                          stage, shifted so that LDS and HBM agree modulo 16,
 *                          aligned dwords funnel-shifted from the aligned
 *                          dwords of the image, then the wave stores its
 *                          contiguous run of `out` 16 bytes per lane, bytes
 *                          only at the run's two unaligned edges.  A run larger
 *                          than the stage is copied image by image across the
 *                          wave.
 *
 * Whatever the searches return, an offset is a prefix sum of the lengths that
 * are copied and *total bounds them all, so sessions in any order write nothing
 * outside out[0, total).  The session search and the in-use test, the wave's
 * scan, put() and the stage's flush are rhp_device.h's, shared with
 * rhp_classify.hip, rhp_gather.hip and rhp_writer.hip.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rhp.h"
#include "rhp_device.h"
#include "rhp_reply_args.h"

namespace {

using namespace rhp_device;

struct RParams {
  const uint8_t              *http;
  const rhp_session_t        *sessions;
  const rhp_session_result_t *results;
  const uint16_t             *route;
  const uint8_t              *images;
  const uint64_t             *image_off;
  rhp_session_reply_t        *replies;
  uint64_t                   *total;
  uint8_t                    *out;
  uint64_t                    out_size;
  uint64_t *agg;    /* work: [3 * tiles] a tile's H, S, flags; after the top scan -, its incoming offset, incoming bit */
  uint64_t *pos;    /* work: [n + 1] a slot's info word (kLive | route << 32 | piece_lo), then its offset into out */
  uint64_t *mask;   /* work: [(n + 63) / 64] bit i & 63 of word i / 64: slot i is answered */
  uint32_t  n, n_sessions, n_routes, static_mask, tiles;
};

constexpr uint32_t kTileSlots = 256;   /* a workgroup of four waves; RHP_REPLY_WORK_WORDS counts these */
constexpr uint64_t kLive = 1ull << 63;

/* a range of slots as a function of x, "the slot before the range is answered":
 * the bit after it is x (kPass) or the constant kAlive holds; it adds S + x * H bytes */
struct Agg {
  uint64_t H, S;
  uint32_t f;
};
constexpr uint32_t kPass = 1u, kAlive = 2u;

__device__ __forceinline__ Agg agg_identity() { return Agg{0, 0, kPass}; }
__device__ __forceinline__ uint32_t agg_bit(uint32_t f, uint32_t x) { return (f & kPass) ? x : (f & kAlive) ? 1u : 0u; }
/* a, then b */
__device__ __forceinline__ Agg combine(const Agg &a, const Agg &b)
{
  Agg r;
  const bool pass = a.f & kPass, alive = a.f & kAlive;
  r.H = a.H + (pass ? b.H : 0);
  r.S = a.S + b.S + (!pass && alive ? b.H : 0);
  r.f = (a.f & b.f & kPass) | ((b.f & kPass) ? (a.f & kAlive) : (b.f & kAlive));
  return r;
}

/* slot i < n: kLive | route << 32 | piece_lo when it is live, else 0 */
__device__ __forceinline__ uint64_t slot_info(const RParams &p, uint32_t i)
{
  const uint32_t above = sessions_upto(p.sessions, p.n_sessions, i);
  if (!above) return 0;
  const uint2 se = reinterpret_cast<const uint2 *>(p.sessions)[above - 1u];   /* piece_lo, piece_hi */
  const uint32_t ns = p.results[above - 1u].n_slots;
  if (!in_use(i, se.x, se.y, ns, p.n)) return 0;
  /* the walk's last slot (piece_lo + n_slots - 1 < piece_hi <= n): stopped on -1? */
  if (*reinterpret_cast<const int32_t *>(p.http + (size_t) (se.x + ns - 1u) * sizeof(rhp_http_t)) == -1) return 0;
  const uint32_t r = p.route[i];
  if (r >= p.n_routes || !((p.static_mask >> r) & 1u)) return 0;
  return kLive | (uint64_t) r << 32 | se.x;
}

struct WaveSlots {
  bool     ok;     /* live, and every slot from max(piece_lo, the wave's first) up to this one is */
  bool     cond;   /* ok, and the run began before the wave: answered iff the slot before the wave is */
  uint64_t len;    /* the image's length (ok) */
  Agg      agg;    /* the wave's 64 slots */
};

/* all 64 lanes call it */
__device__ __forceinline__ WaveSlots wave_slots(const RParams &p, uint64_t info, uint32_t wave_base, uint32_t lane)
{
  WaveSlots w;
  const bool live = info >> 63;
  const uint32_t lo = (uint32_t) info, r = (uint32_t) (info >> 32) & 0xffffu;
  const uint64_t livemask = __ballot(live);
  const uint32_t a = lo > wave_base ? lo - wave_base : 0u;   /* (live: piece_lo <= wave_base + lane) */
  const uint64_t range = (~0ull >> (63u - lane)) & (~0ull << (a & 63u));   /* bits a .. lane */
  w.ok = live && (~livemask & range) == 0;
  w.cond = w.ok && lo < wave_base;
  w.len = w.ok ? p.image_off[r + 1u] - p.image_off[r] : 0;
  unsigned long long h = w.cond ? w.len : 0, s = w.ok && !w.cond ? w.len : 0;
  for (int o = 32; o > 0; o >>= 1) {
    h += __shfl_xor(h, o);
    s += __shfl_xor(s, o);
  }
  const uint64_t condmask = __ballot(w.cond), okmask = __ballot(w.ok);
  w.agg = Agg{h, s, ((condmask >> 63) & 1u ? kPass : 0u) | (((okmask & ~condmask) >> 63) & 1u ? kAlive : 0u)};
  return w;
}

__global__ __launch_bounds__(256) void rhp_reply_tile_kernel(RParams p)
{
  __shared__ unsigned long long wH[4], wS[4];
  __shared__ uint32_t wF[4];
  const uint32_t i = blockIdx.x * kTileSlots + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t info = i < p.n ? slot_info(p, i) : 0;
  if (i < p.n) p.pos[i] = info;
  const WaveSlots w = wave_slots(p, info, i - lane, lane);
  if (lane == 0) {
    wH[wv] = w.agg.H;
    wS[wv] = w.agg.S;
    wF[wv] = w.agg.f;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    Agg t = agg_identity();
    for (uint32_t q = 0; q < 4; q++) t = combine(t, Agg{wH[q], wS[q], wF[q]});
    p.agg[3u * (uint64_t) blockIdx.x] = t.H;
    p.agg[3u * (uint64_t) blockIdx.x + 1u] = t.S;
    p.agg[3u * (uint64_t) blockIdx.x + 2u] = t.f;
  }
}

/* one workgroup: every tile's incoming bit and offset (the tiles before it composed
 * and given x = 0), in place; *total, and the offset past the last slot.  A thread
 * takes a run of consecutive tiles, the 1024 runs are scanned in LDS */
__global__ __launch_bounds__(1024) void rhp_reply_top_kernel(RParams p)
{
  __shared__ unsigned long long sH[1024], sS[1024];
  __shared__ uint32_t sF[1024];
  const uint32_t t = threadIdx.x;
  const uint64_t tiles = p.tiles, chunk = (tiles + 1023u) / 1024u;
  const uint64_t lo = min((uint64_t) t * chunk, tiles), hi = min(lo + chunk, tiles);
  Agg a = agg_identity();
  for (uint64_t k = lo; k < hi; k++) a = combine(a, Agg{p.agg[3u * k], p.agg[3u * k + 1u], (uint32_t) p.agg[3u * k + 2u]});
  sH[t] = a.H, sS[t] = a.S, sF[t] = a.f;
  __syncthreads();
  for (uint32_t o = 1; o < 1024u; o <<= 1) {
    const Agg u = t >= o ? Agg{sH[t - o], sS[t - o], sF[t - o]} : agg_identity(), v = Agg{sH[t], sS[t], sF[t]};
    __syncthreads();
    const Agg r = combine(u, v);
    sH[t] = r.H, sS[t] = r.S, sF[t] = r.f;
    __syncthreads();
  }
  uint32_t x = t ? agg_bit(sF[t - 1u], 0u) : 0u;
  uint64_t off = t ? sS[t - 1u] : 0u;
  for (uint64_t k = lo; k < hi; k++) {
    const Agg g = Agg{p.agg[3u * k], p.agg[3u * k + 1u], (uint32_t) p.agg[3u * k + 2u]};
    p.agg[3u * k + 1u] = off;
    p.agg[3u * k + 2u] = x;
    off += g.S + (x ? g.H : 0);
    x = agg_bit(g.f, x);
  }
  if (t == 1023u) {
    *p.total = sS[1023];
    p.pos[p.n] = sS[1023];
  }
}

__global__ __launch_bounds__(256) void rhp_reply_scan_kernel(RParams p)
{
  __shared__ unsigned long long wH[4], wS[4];
  __shared__ uint32_t wF[4];
  const uint32_t i = blockIdx.x * kTileSlots + threadIdx.x, lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint64_t info = i < p.n ? p.pos[i] : 0;
  const WaveSlots w = wave_slots(p, info, i - lane, lane);
  if (lane == 0) {
    wH[wv] = w.agg.H;
    wS[wv] = w.agg.S;
    wF[wv] = w.agg.f;
  }
  __syncthreads();
  uint64_t off = p.agg[3u * (uint64_t) blockIdx.x + 1u];
  uint32_t x = (uint32_t) p.agg[3u * (uint64_t) blockIdx.x + 2u];
  for (uint32_t q = 0; q < wv; q++) {   /* the waves before this one */
    off += wS[q] + (x ? wH[q] : 0);
    x = agg_bit(wF[q], x);
  }
  const bool answered = w.ok && (!w.cond || x);
  const unsigned long long v = answered ? w.len : 0;
  const unsigned long long inc = wave_incl_scan(v, lane);
  const uint64_t m = __ballot(answered);
  if (i < p.n) p.pos[i] = off + inc - v;
  if (lane == 0 && i < p.n) p.mask[i >> 6] = m;
}

/* one image by one lane into its wave's stage at byte o: aligned LDS dwords,
 * funnel-shifted from the aligned dwords that hold the image; bytes at the two
 * unaligned edges */
__device__ __forceinline__ void lds_put(lds8 *L, uint32_t o, const uint8_t *src, uint32_t len)
{
  if (len == 0) return;
  const uintptr_t sa = (uintptr_t) src;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(sa & ~(uintptr_t) 3);
  const uint32_t s0 = (uint32_t) sa & 3u, nd = (s0 + len + 3u) >> 2;   /* the dwords that hold the image */
  /* the four bytes from src + k, k < len: dword (s0 + k) / 4 holds the first, the next one only if the image reaches it */
  auto get4 = [&](uint32_t k) {
    const uint32_t a = s0 + k, q = a >> 2;
    const uint32_t lo = w[q], hi = q + 1u < nd ? w[q + 1u] : 0u;
    return __builtin_amdgcn_alignbyte(hi, lo, a & 3u);
  };
  const uint32_t head = min(len, (4u - (o & 3u)) & 3u);
  uint32_t k = 0;
  if (head) {
    const uint32_t x = get4(0);
    for (; k < head; k++) L[o + k] = (uint8_t) (x >> (8u * k));
  }
  for (; k + 4u <= len; k += 4u) *reinterpret_cast<lds32 *>(L + o + k) = get4(k);
  if (k < len) {
    const uint32_t x = get4(k);
    for (uint32_t j = 0; k + j < len; j++) L[o + k + j] = (uint8_t) (x >> (8u * j));
  }
}

constexpr uint32_t kStage = 10240;   /* LDS bytes per wave: 64 plaintext replies and the shift; four workgroups per CU */

__global__ __launch_bounds__(256) void rhp_reply_copy_kernel(RParams p)
{
  __shared__ __attribute__((aligned(16))) uint8_t stage_all[4 * kStage];
  const uint32_t gid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;

  /* ---- replies[s]: the answered slots of a session are a prefix of its slots ---- */
  for (uint64_t s = gid; s < p.n_sessions; s += nthreads) {
    const uint2 se = reinterpret_cast<const uint2 *>(p.sessions)[s];
    const uint32_t ns = p.results[s].n_slots, lo = min(se.x, p.n);
    uint32_t count = 0;
    if ((uint64_t) se.x + ns <= se.y && se.y <= p.n) {   /* (then every slot looked at is below n) */
      for (uint32_t hi = ns; count < hi;) {
        const uint32_t mid = count + ((hi - count) >> 1), j = lo + mid;
        if ((p.mask[j >> 6] >> (j & 63u)) & 1u) count = mid + 1u; else hi = mid;
      }
    }
    const uint64_t at = p.pos[lo];
    uint64_t *r = reinterpret_cast<uint64_t *>(p.replies + s);
    r[0] = count;   /* count, reserved = 0 */
    r[1] = at;
    r[2] = p.pos[lo + count] - at;
  }

  /* ---- the images ---- */
  if (p.pos[p.n] > p.out_size || !p.images) return;   /* does not fit: sizes only (rhp.h) */
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t wave = gid >> 6, nwaves = nthreads >> 6;
  lds8 *L = (lds8 *) (stage_all + wv * kStage);
  const uint32_t groups = (uint32_t) (((uint64_t) p.n + 63u) / 64u);
  for (uint32_t g = wave; g < groups; g += nwaves) {
    const uint64_t i0 = (uint64_t) g * 64u, i1 = min(i0 + 64u, (uint64_t) p.n);
    const uint64_t G0 = p.pos[i0], G1 = p.pos[i1];
    if (G1 == G0) continue;   /* nothing to copy (empty images at the most) */
    const uint64_t am = p.mask[g];
    /* this lane's image: the route again, held to the table, and to the room the scan gave it */
    const uint64_t i = i0 + lane;
    uint64_t at = 0, len = 0, from = 0;
    if ((am >> lane) & 1u) {   /* (answered: i < n) */
      const uint32_t r = p.route[i];
      if (r < p.n_routes) {
        at = p.pos[i];
        from = p.image_off[r];
        len = min(p.pos[i + 1u] - at, p.image_off[r + 1u] - from);
      }
    }
    const uint32_t shift = (uint32_t) (uintptr_t) (p.out + G0) & 15u;   /* LDS and HBM agree modulo 16 */
    if (G1 - G0 + shift > kStage) {   /* big images: one after the other, across the wave */
      for (uint32_t j = 0; j < 64u; j++) {
        if (!((am >> j) & 1u)) continue;   /* (the same word in every lane) */
        const uint64_t at_j = __shfl((unsigned long long) at, (int) j), len_j = __shfl((unsigned long long) len, (int) j),
                       from_j = __shfl((unsigned long long) from, (int) j);
        put(p.out + at_j, p.images + from_j, len_j, lane);
      }
      continue;
    }
    lds_put(L, shift + (uint32_t) (at - G0), p.images + from, (uint32_t) len);
    flush_stage(L, shift, p.out, G0, G1, lane);
  }
}

}  // namespace

extern "C" int rhp_reply_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                  const rhp_session_result_t *results, const uint16_t *route,
                                  const rhp_reply_table_t *t, const rhp_reply_out_t *o, void *stream)
{
  const int rc = rhp_reply_sessions_check(b, sessions, n_sessions, results, route, t, o, 0);
  if (rc < 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  /* no session: no slot is looked at, *total = 0 */
  const uint32_t n = rc == 1 || n_sessions == 0 ? 0u : b->n;
  RParams p;
  p.http = reinterpret_cast<const uint8_t *>(b->http);
  p.sessions = sessions;
  p.results = results;
  p.route = route;
  p.images = t->images;
  p.image_off = t->image_off;
  p.replies = o->replies;
  p.total = o->total;
  p.out = o->out;
  p.out_size = o->out_size;
  p.n = n;
  p.n_sessions = n_sessions;
  p.n_routes = t->n_routes;
  p.static_mask = t->static_mask;
  p.tiles = (uint32_t) (((uint64_t) n + kTileSlots - 1u) / kTileSlots);
  p.agg = o->work;
  p.pos = p.agg + 3u * (uint64_t) p.tiles;
  p.mask = p.pos + (uint64_t) n + 1u;
  if (p.tiles) hipLaunchKernelGGL(rhp_reply_tile_kernel, dim3(p.tiles), dim3(256), 0, s, p);
  hipLaunchKernelGGL(rhp_reply_top_kernel, dim3(1), dim3(1024), 0, s, p);
  if (n_sessions == 0) return (int) hipGetLastError();
  if (p.tiles) hipLaunchKernelGGL(rhp_reply_scan_kernel, dim3(p.tiles), dim3(256), 0, s, p);
  uint64_t blocks = ((uint64_t) (n > n_sessions ? n : n_sessions) + 255u) / 256u;
  if (blocks > (1u << 20)) blocks = 1u << 20;   /* (the kernel's loops stride over the rest) */
  hipLaunchKernelGGL(rhp_reply_copy_kernel, dim3((uint32_t) blocks), dim3(256), 0, s, p);
  return (int) hipGetLastError();
}
