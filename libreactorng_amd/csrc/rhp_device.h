/*
 * rhp_device.h -- the device helpers that more than one of rhp_writer.hip,
 * rhp_classify.hip, rhp_reply.hip, rhp_gather.hip, rhp_chunked.hip, rhp_messages.hip,
 * rhp_walk.hip and rhp_kernel.hip use, stated once: the
 * inclusive scan of a wave, the wave's copy of a byte range, the flush of a
 * wave's LDS stage, the search and the test that give a record slot its
 * session, the bounded 16-byte line reader and the record stores of the message
 * parse (rhp_messages.hip, rhp_walk.hip), and one thread's move down in place
 * (rhp_kernel.hip's http_dechunk, rhp_walk.hip's de-framing).  Device code
 * only; every function is inlined into its caller.
 */
#ifndef RHP_DEVICE_H
#define RHP_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rhp.h"

namespace rhp_device {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) uint8_t lds8;
typedef __attribute__((address_space(3))) uint32_t lds32;

/* inclusive sum over the wave's 64 lanes (unsigned long long or uint32_t) */
template <class T>
__device__ __forceinline__ T wave_incl_scan(T v, uint32_t lane)
{
  for (int o = 1; o < 64; o <<= 1) {
    const T u = __shfl_up(v, o);
    if ((int) lane >= o) v += u;
  }
  return v;
}

/* out_off[1..n] sizes -> out_off[0..n] offsets, reduce-then-scan over tiles of
 * kTile sizes: tile sums into work[], one workgroup scans work[] (exclusive),
 * then every tile is scanned in place with its carry.  Loads and stores are
 * coalesced; within a workgroup a thread scans 4 consecutive sizes, a wave its
 * 64 threads through shuffles, the workgroup its 16 waves through LDS.
 * (rhp_writer.hip and rhp_classify.hip's relay: each writes the sizes and the
 * tile sums in a kernel of its own and launches the two kernels below.) */
constexpr uint32_t kTile = 4096;   /* 1024 threads x 4 */

/* inclusive scan of one value per thread over a 1024-thread workgroup */
__device__ __forceinline__ unsigned long long block_incl_scan(unsigned long long v, unsigned long long *part)
{
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  v = wave_incl_scan(v, lane);
  if (lane == 63) part[w] = v;
  __syncthreads();
  if (w == 0) {
    unsigned long long x = lane < 16 ? part[lane] : 0;
    x = wave_incl_scan(x, lane);
    if (lane < 16) part[lane] = x;
  }
  __syncthreads();
  return v + (w ? part[w - 1] : 0);
}

/* a tile's sum from one partial sum per thread of a 1024-thread workgroup */
__device__ __forceinline__ void block_sum_to(unsigned long long s, unsigned long long *part, uint64_t *to)
{
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if ((threadIdx.x & 63u) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned long long t = 0;
    for (int w = 0; w < 16; w++) t += part[w];
    *to = t;
  }
}

/* The two scan kernels, only in a file that defines RHP_DEVICE_SCAN_KERNELS before
 * it includes this header (rhp_writer.hip, rhp_classify.hip, rhp_forward.hip): every other file
 * would emit and register kernels it never launches. */
#if defined(RHP_DEVICE_SCAN_KERNELS)
/* work[0..tiles) -> exclusive offsets (one workgroup, 1024 per round) */
static __global__ __launch_bounds__(1024) void rhp_resp_top_scan_kernel(uint64_t *work, uint32_t tiles)
{
  __shared__ unsigned long long part[16];
  unsigned long long carry = 0;
  for (uint32_t b = 0; b < tiles; b += 1024) {
    const uint32_t k = b + threadIdx.x;
    const unsigned long long v = k < tiles ? work[k] : 0;
    const unsigned long long inc = block_incl_scan(v, part);
    if (k < tiles) work[k] = carry + inc - v;
    carry += part[15];   /* the round's total */
    __syncthreads();
  }
}

static __global__ __launch_bounds__(1024) void rhp_resp_tile_scan_kernel(uint64_t *a, uint32_t n, const uint64_t *work)
{
  __shared__ unsigned long long part[16];
  const uint64_t base = 1 + (uint64_t) blockIdx.x * kTile + 4u * threadIdx.x, end = (uint64_t) n + 1;
  unsigned long long x[4], s = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    x[q] = base + q < end ? a[base + q] : 0;
    s += x[q];
    x[q] = s;   /* thread-local inclusive */
  }
  const unsigned long long before = block_incl_scan(s, part) - s + work[blockIdx.x];
#pragma unroll
  for (int q = 0; q < 4; q++)
    if (base + q < end) a[base + q] = before + x[q];
  if (blockIdx.x == 0 && threadIdx.x == 0) a[0] = 0;
}

#endif

/* ---- the lane-per-reply stage writers (LDS byte o of the wave's stage) ---- */
/* a compile-time constant string */
template <uint32_t N>
__device__ __forceinline__ void st_const(lds8 *L, uint32_t &o, const char (&s)[N])
{
#pragma unroll
  for (uint32_t j = 0; j + 1 < N; j++) L[o + j] = (uint8_t) s[j];
  o += N - 1;
}
/* len bytes from global memory at src: the aligned dwords that hold them (no
 * byte outside [src & ~3, src + len + 3) is read), funnel-shifted */
__device__ __forceinline__ void st_span(lds8 *L, uint32_t &o, const uint8_t *src, uint32_t len)
{
  const uintptr_t a = (uintptr_t) src;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t) 3);
  const uint32_t sh = (uint32_t) a & 3u, nd = (sh + len + 3u) >> 2;
  uint32_t lo = len ? w[0] : 0;
  for (uint32_t j = 0; j < len; j += 4) {
    const uint32_t k = (j >> 2) + 1u;
    const uint32_t hi = k < nd ? w[k] : 0u;
    const uint32_t d = __builtin_amdgcn_alignbyte(hi, lo, sh);
    L[o + j] = (uint8_t) d;
    if (j + 1 < len) L[o + j + 1] = (uint8_t) (d >> 8);
    if (j + 2 < len) L[o + j + 2] = (uint8_t) (d >> 16);
    if (j + 3 < len) L[o + j + 3] = (uint8_t) (d >> 24);
    lo = hi;
  }
  o += len;
}

/* a compile-time constant string across the wave (shorter than 64 bytes), o
 * advancing past it: the cooperative twin of st_const */
template <uint32_t N>
__device__ __forceinline__ void put_const(uint8_t *dst, uint64_t &o, const char (&s)[N], uint32_t lane)
{
  static_assert(N - 1 <= 64, "a byte per lane");
  if (lane < N - 1) dst[o + lane] = (uint8_t) s[lane];
  o += N - 1;
}

/* d[0, len) <- src[0, len) across the wave, all 64 lanes calling: bytes up to
 * the first 16-aligned destination, then 16 bytes per lane (1 KiB per store
 * instruction) from funnel-shifted aligned source dwords, then the tail bytes;
 * below 128 bytes a byte per lane.  The read contract: no byte outside the
 * aligned dwords that hold [src, src + len) is read -- the dword past the
 * last one a 16-byte step needs is loaded only if the range reaches it.
 * Overlap: safe for d <= src (a move down in place, rhp_chunked.hip), by the
 * order of its steps -- the head bytes, then the body 1 KiB at a time, then the
 * tail bytes (below 128 bytes: 64 bytes at a time); step t covers bytes
 * [a_t, b_t) of the range, ascending and back to back.  With g = src - d, the
 * stores of step t land on src + [a_t - g, b_t - g), and the source bytes step
 * u uses are src + [a_u, b_u) (a dword's bytes outside that range are loaded
 * and shifted out by alignbyte), so a store of step t can reach a source byte
 * of step u only for u <= t.  Those are loaded already: d and src may alias as
 * far as the compiler knows, so it keeps a lane's loads and stores in program
 * order; the wave issues every instruction for all its lanes at once; and a
 * step's store waits (vmcnt) for that step's loads, which return for the whole
 * wave.  DESIGN.md 3.10 */
__device__ __forceinline__ void put(uint8_t *d, const uint8_t *src, uint64_t len, uint32_t lane)
{
  if (len < 128) {
    for (uint32_t j = lane; j < len; j += 64) d[j] = src[j];
    return;
  }
  const uint32_t head = (uint32_t) ((16u - ((uintptr_t) d & 15u)) & 15u);
  if (lane < head) d[lane] = src[lane];
  const uint8_t *s = src + head;
  const uint64_t body = (len - head) & ~(uint64_t) 15u;
  const uintptr_t sa = (uintptr_t) s;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(sa & ~(uintptr_t) 3);
  const uint32_t sh = (uint32_t) sa & 3u;
  const uint64_t nd = (sh + (len - head) + 3u) >> 2;
  for (uint64_t j = 16u * lane; j < body; j += 1024u) {
    const uint64_t k = j >> 2;
    const uint32_t w0 = w[k], w1 = w[k + 1], w2 = w[k + 2], w3 = w[k + 3], w4 = k + 4 < nd ? w[k + 4] : 0u;
    *reinterpret_cast<u32x4 *>(d + head + j) = u32x4{__builtin_amdgcn_alignbyte(w1, w0, sh), __builtin_amdgcn_alignbyte(w2, w1, sh),
                                                     __builtin_amdgcn_alignbyte(w3, w2, sh), __builtin_amdgcn_alignbyte(w4, w3, sh)};
  }
  for (uint64_t j = head + body + lane; j < len; j += 64) d[j] = src[j];
}

/* out[G0, G1) <- stage[shift, shift + G1 - G0), the wave's LDS stage L that its
 * lanes have just written, shift = (out + G0) & 15 so that LDS and HBM agree
 * modulo 16: 16-byte stores between the first and the last 16-aligned
 * addresses, byte stores outside.  All 64 lanes call it; the stage may be
 * written again when it returns */
__device__ __forceinline__ void flush_stage(const lds8 *L, uint32_t shift, uint8_t *out, uint64_t G0, uint64_t G1, uint32_t lane)
{
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_s_waitcnt(0xc07f);   /* lgkmcnt(0): the stage is written (wave-local) */
  __builtin_amdgcn_wave_barrier();
  const uint64_t A0 = G0 + ((16u - shift) & 15u), A1 = G1 - (((uint32_t) (uintptr_t) (out + G1)) & 15u);
  if (A0 < A1) {
    for (uint64_t a = A0 + 16u * lane; a < A1; a += 1024u) {
      const uint32_t so = (uint32_t) (a - G0) + shift;
      const u32x4 d = *reinterpret_cast<const __attribute__((address_space(3))) u32x4 *>(L + so);
      *reinterpret_cast<u32x4 *>(out + a) = d;
    }
    if (lane < A0 - G0) out[G0 + lane] = L[shift + lane];
    if (lane < G1 - A1) out[A1 + lane] = L[shift + (uint32_t) (A1 - G0) + lane];
  } else {   /* the whole range within one 16-byte line (or two) */
    for (uint32_t j = lane; j < G1 - G0; j += 64) out[G0 + j] = L[shift + j];
  }
  __builtin_amdgcn_wave_barrier();
}

/* the number of sessions whose piece_lo <= i (bisection; sessions ascend by
 * piece_lo, rhp.h: the owner of slot i is the last of them) */
__device__ __forceinline__ uint32_t sessions_upto(const rhp_session_t *sessions, uint32_t n_sessions, uint32_t i)
{
  uint32_t above = 0;
  for (uint32_t hi = n_sessions; above < hi;) {
    const uint32_t mid = above + ((hi - above) >> 1);
    if (sessions[mid].piece_lo <= i) above = mid + 1u; else hi = mid;
  }
  return above;
}

/* the one test that lets a load of slot i's records through, whatever the
 * search returned: the session's fields (piece_lo, piece_hi, n_slots) hold in
 * a batch of n slots and contain i.  (n by reference: the callers pass a member
 * of their kernel argument, read where the test comes to it, which keeps
 * rhp_gather.hip's kernels the instruction streams they were) */
__device__ __forceinline__ bool in_use(uint32_t i, uint32_t lo, uint32_t hi, uint32_t ns, const uint32_t &n)
{
  return lo <= i && i - lo < ns && (uint64_t) lo + ns <= hi && hi <= n;
}

/* byte p of the message that starts at byte `at` of the batch (bytes is
 * 16-byte aligned: a line is an aligned 16-byte load) */
struct BoundedLineBytes {
  const uint8_t *bytes;
  uint64_t at, size, line;   /* size: a multiple of 16 */
  u32x4 c;
  __device__ uint32_t operator()(uint64_t p)
  {
    const uint64_t a = at + p;
    const uint64_t l = a & ~(uint64_t) 15;
    if (l != line) {
      c = u32x4{0, 0, 0, 0};
      if (l < size) c = *reinterpret_cast<const __attribute__((address_space(1))) u32x4 *>((uintptr_t) (bytes + l));
      line = l;
    }
    const uint32_t q = (uint32_t) (a >> 2) & 3u;
    const uint32_t d = q == 0 ? c[0] : q == 1 ? c[1] : q == 2 ? c[2] : c[3];
    return (d >> (8u * ((uint32_t) a & 3u))) & 0xffu;
  }
};

/* OutMsg's Store on the device: whole records, one store each */
struct DevMsgStore {
  rhp_msg_t *m;
  rhp_hdr_t *h;
  uint64_t hs;
  __device__ void msg(const rhp_msg_t &v) const
  {
    static_assert(sizeof(rhp_msg_t) == 16, "a message record is one 16-byte store");
    u32x4 w;
    __builtin_memcpy(&w, &v, 16);
    *reinterpret_cast<u32x4 *>(m) = w;
  }
  __device__ void hdr(uint32_t k, const rhp_hdr_t &v) const
  {
    static_assert(sizeof(rhp_hdr_t) == 8, "a header record is one 8-byte store");
    uint2 w;
    __builtin_memcpy(&w, &v, 8);
    *reinterpret_cast<uint2 *>(h + k * hs) = w;
  }
};

/* n body bytes from src to dst (dst <= src, offsets from `in`), forward: the
 * in-place move of http_dechunk (http.c:155) for one thread.  Destination
 * blocks are whole aligned 16-byte stores built from aligned 16-byte source
 * lines (funnel-shifted by the constant src - dst), four blocks per memory
 * round trip; the partial first and last blocks are byte stores, so no byte
 * outside [dst, dst + n) -- another request's -- is written.  Loads read only
 * source bytes no earlier store has reached (each block's source lies past its
 * destination), apart from unused bytes of shared lines. */
struct DevMove {
  uint8_t *in;
  __device__ void operator()(uint64_t dst, uint64_t src, uint64_t n) const
  {
    typedef __attribute__((address_space(1))) const u32x4 gq;
    typedef __attribute__((address_space(1))) u32x4 gw;
    if (n == 0 || dst == src) return;
    const uintptr_t da = (uintptr_t) (in + dst), de = da + n, delta = (uintptr_t) (src - dst);
    const uint32_t q = (uint32_t) (delta >> 2) & 3u, r = (uint32_t) delta & 3u;
    /* block at destination A: source bytes [A + delta, A + delta + 16) from the
     * lines at (A + delta) & ~15 and the one after it */
    auto ld = [](uintptr_t a) -> u32x4 { return *reinterpret_cast<gq *>(a); };
    auto block = [&](const u32x4 &l0, const u32x4 &l1) {
      const uint32_t w[8] = {l0[0], l0[1], l0[2], l0[3], l1[0], l1[1], l1[2], l1[3]};
      u32x4 o;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const uint32_t lo = q == 0 ? w[j] : q == 1 ? w[j + 1] : q == 2 ? w[j + 2] : w[j + 3];
        const uint32_t hi = q == 0 ? w[j + 1] : q == 1 ? w[j + 2] : q == 2 ? w[j + 3] : w[j + 4];
        o[j] = __builtin_amdgcn_alignbyte(hi, lo, r);
      }
      return o;
    };
    auto partial = [&](uintptr_t A) {   /* bytes of block A inside [da, de): whole dwords, then bytes */
      typedef __attribute__((address_space(1))) uint32_t gw1;
      typedef __attribute__((address_space(1))) uint8_t gb1;
      const uintptr_t s0 = (A + delta) & ~(uintptr_t) 15;
      const u32x4 o = block(ld(s0), ld(s0 + 16));
#pragma unroll
      for (uint32_t j = 0; j < 4; j++) {
        const uintptr_t w = A + 4 * j;
        if (w >= da && w + 4 <= de) {
          *reinterpret_cast<gw1 *>(w) = o[j];
        } else if (w + 4 > da && w < de) {
#pragma unroll
          for (uint32_t k = 0; k < 4; k++)
            if (w + k >= da && w + k < de) *reinterpret_cast<gb1 *>(w + k) = (uint8_t) (o[j] >> (8 * k));
        }
      }
    };
    uintptr_t A = da & ~(uintptr_t) 15;
    if (A != da || A + 16 > de) {   /* a partial first block */
      partial(A);
      A += 16;
    }
    constexpr int U = 4;   /* destination blocks per memory round trip */
    while (A + 16 * U <= de) {
      const uintptr_t s0 = (A + delta) & ~(uintptr_t) 15;
      u32x4 l[U + 1];
#pragma unroll
      for (int u = 0; u <= U; u++) l[u] = ld(s0 + 16 * u);
#pragma unroll
      for (int u = 0; u < U; u++) *reinterpret_cast<gw *>(A + 16 * u) = block(l[u], l[u + 1]);
      A += 16 * U;
    }
    while (A + 16 <= de) {
      const uintptr_t s0 = (A + delta) & ~(uintptr_t) 15;
      *reinterpret_cast<gw *>(A) = block(ld(s0), ld(s0 + 16));
      A += 16;
    }
    if (A < de) partial(A);
  }
};

}  // namespace rhp_device

#endif
