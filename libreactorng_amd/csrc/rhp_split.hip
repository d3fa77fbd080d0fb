/*
 * rhp_split.hip -- rhp_split_sessions (rhp.h): the packed input of a round's
 * sessions cut at every empty line, on the device: offsets[] and
 * rhp_session_t[] for rhp_parse_batch and rhp_fixup_sessions.  gfx950.
 *
 * A cut is a predicate on the three bytes before a position, and a piece index
 * is a position's rank among the cuts plus its session's index: a mark, a scan
 * and a scatter.  Three launches:
 *
 *   rhp_split_mark_kernel   a wave per step of RHP_SPLIT_STEP_BYTES: a lane
 *                           loads one aligned 16-byte group (one dwordx4) and
 *                           turns it into 16-bit LF and CR masks; the three
 *                           bytes before the group come from the lane below
 *                           (lane 0: one dword load in front of the step).  The
 *                           session starts inside the step are found by one
 *                           wave-uniform bisection over sess_off and leave
 *                           their kill bits in LDS: positions a and a + 1 cut
 *                           nothing, a + 2 cuts only on LF LF (the look-back
 *                           stays inside the session).  Out: a u64 cut mask
 *                           per 64 bytes, the count of the step's cuts before
 *                           each mask, the step's count
 *   rhp_split_scan_kernel   one workgroup: the steps' counts to their
 *                           exclusive prefix in place (wave_incl_scan), the
 *                           total, *n_pieces
 *   rhp_split_write_kernel  when the pieces fit cap_pieces: a thread per 16
 *                           bytes scatters its cuts, offsets[session + rank +
 *                           1] = position (the session by bisection, per cut);
 *                           a thread per session writes piece_lo, piece_hi and
 *                           offsets[piece_lo] from the rank at its start; a
 *                           thread per tail index fills offsets(n_pieces,
 *                           cap_pieces]
 *
 * Traffic: the input once, 200 bytes of work per 1024 bytes of input written
 * and read once (12.5 per 64), sess_off, the outputs.
 *
 * Whatever sess_off holds: a byte group is loaded only below bytes_end, the
 * masks are indexed by the step and lane alone, a rank is clamped to the total
 * and every index into offsets is held below n_pieces <= cap_pieces again.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rhp.h"
#include "rhp_device.h"
#include "rhp_split_args.h"

namespace {

using namespace rhp_device;

constexpr uint32_t kStep = RHP_SPLIT_STEP_BYTES;
static_assert(kStep == 64u * 16u, "a wave marks 16 bytes per lane");
constexpr uint32_t kScanThreads = 1024;

struct SParams {
  const uint8_t  *bytes;
  const uint64_t *sess_off;
  uint64_t       *n_pieces, *offsets;
  rhp_session_t  *sessions;
  uint64_t *mask;      /* work: [16 * steps] bit b of word w: position 64 w + b is a cut */
  uint32_t *inword;    /* work: [16 * steps] the cuts of the word's step at positions before the word */
  uint64_t *stepsum;   /* work: [steps + 1] a step's cuts; after the scan the cuts before the step, [steps] the total */
  uint32_t  bytes_end, n_sessions, steps, cap;
};

/* bit k: byte k of w equals c (exact: no carry between the bytes) */
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t c)
{
  const uint32_t x = w ^ (c * 0x01010101u);
  const uint32_t z = ~(((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu);   /* 0x80 in every zero byte of x */
  return ((z >> 7) * 0x01020408u) >> 24;
}

__device__ __forceinline__ uint32_t eq16(const u32x4 &d, uint32_t c)
{
  return eq4(d.x, c) | eq4(d.y, c) << 4 | eq4(d.z, c) << 8 | eq4(d.w, c) << 12;
}

__global__ __launch_bounds__(256) void rhp_split_mark_kernel(SParams p)
{
  __shared__ uint32_t kill[4][2][32];   /* per wave, a bit per position of its step: [0] a and a + 1, [1] a + 2 */
  const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
  const uint32_t step = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + wv);
  const bool live = step < p.steps;   /* (the same in the whole wave) */
  const uint64_t base = (uint64_t) step * kStep;
  kill[wv][lane >> 5][lane & 31u] = 0u;
  __syncthreads();
  if (live) {
    /* the first of sess_off[0 .. n_sessions] that is at or after base - 2; the last one, the input's end, kills as a start does */
    uint32_t i0 = 0;
    for (uint32_t hi = p.n_sessions + 1u; i0 < hi;) {
      const uint32_t mid = i0 + ((hi - i0) >> 1);
      if (p.sess_off[mid] + 2u < base) i0 = mid + 1u; else hi = mid;
    }
    for (uint64_t k = i0; k <= p.n_sessions; k += 64u) {
      const uint64_t idx = k + lane;
      const uint64_t v = idx <= p.n_sessions ? p.sess_off[idx] : 0u;
      const bool in = idx <= p.n_sessions && v + 2u >= base && v < base + kStep;
      if (in) {
        const int32_t r = (int32_t) (int64_t) (v - base);   /* -2 .. kStep - 1 */
        if (r >= 0) atomicOr(&kill[wv][0][r >> 5], 1u << (r & 31));
        if (r + 1 >= 0 && r + 1 < (int32_t) kStep) atomicOr(&kill[wv][0][(r + 1) >> 5], 1u << ((r + 1) & 31));
        if (r + 2 < (int32_t) kStep) atomicOr(&kill[wv][1][(r + 2) >> 5], 1u << ((r + 2) & 31));
      }
      if (__ballot(in) != ~0ull) break;   /* (ascending: nothing further starts in this step) */
    }
  }
  __syncthreads();
  if (!live) return;
  const uint64_t S0 = p.sess_off[0], S1 = min(p.sess_off[p.n_sessions], (uint64_t) p.bytes_end);
  const uint64_t g = base + 16u * lane;
  /* rhp.h: only the groups that hold [S0, S1) are read */
  u32x4 d = {0u, 0u, 0u, 0u};
  if (g < S1 && g + 16u > S0) d = *reinterpret_cast<const u32x4 *>(p.bytes + g);
  const uint32_t lf = eq16(d, RHP_SPLIT_LF), cr = eq16(d, RHP_SPLIT_CR);
  uint32_t plf = __shfl_up(lf, 1), pcr = __shfl_up(cr, 1);
  if (lane == 0u) {
    plf = pcr = 0u;
    if (base >= 16u && base - 16u < S1 && base > S0) {
      const uint32_t w = *reinterpret_cast<const uint32_t *>(p.bytes + base - 4u);
      plf = eq4(w, RHP_SPLIT_LF) << 12, pcr = eq4(w, RHP_SPLIT_CR) << 12;
    }
  }
  /* bit 16 + j of lf32: the group's byte j; L1, L2, L3: LF one, two, three bytes before position j */
  const uint32_t lf32 = lf << 16 | plf, cr32 = cr << 16 | pcr;
  const uint32_t L1 = lf32 >> 15, L2 = lf32 >> 14, L3 = lf32 >> 13, C2 = cr32 >> 14;
  const uint32_t sh = 16u * (lane & 1u);
  const uint32_t k01 = kill[wv][0][lane >> 1] >> sh, k2 = kill[wv][1][lane >> 1] >> sh;
  const uint32_t lo = S0 > g ? (uint32_t) min(S0 - g, (uint64_t) 16u) : 0u, hi = S1 > g ? (uint32_t) min(S1 - g, (uint64_t) 16u) : 0u;
  const uint32_t range = ((1u << hi) - 1u) & ~((1u << lo) - 1u);
  const uint32_t cut = L1 & (L2 | (C2 & L3 & ~k2)) & ~k01 & range & 0xffffu;
  unsigned long long word = (unsigned long long) cut << (16u * (lane & 3u));
  word |= __shfl_xor(word, 1);
  word |= __shfl_xor(word, 2);
  const uint32_t c = __popc(cut), inc = wave_incl_scan(c, lane);
  if ((lane & 3u) == 0u) {
    p.mask[16u * (uint64_t) step + (lane >> 2)] = word;
    p.inword[16u * (uint64_t) step + (lane >> 2)] = inc - c;
  }
  if (lane == 63u) p.stepsum[step] = inc;
}

/* one workgroup: every step's exclusive prefix in place, the total, *n_pieces */
__global__ __launch_bounds__(kScanThreads) void rhp_split_scan_kernel(SParams p)
{
  __shared__ unsigned long long sW[kScanThreads / 64u];
  const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
  const uint64_t steps = p.steps, chunk = (steps + kScanThreads - 1u) / kScanThreads;
  const uint64_t lo = min((uint64_t) t * chunk, steps), hi = min(lo + chunk, steps);
  unsigned long long sum = 0;
  for (uint64_t k = lo; k < hi; k++) sum += p.stepsum[k];
  const unsigned long long inc = wave_incl_scan(sum, lane);
  if (lane == 63u) sW[w] = inc;
  __syncthreads();
  unsigned long long before = 0, total = 0;
  for (uint32_t i = 0; i < kScanThreads / 64u; i++) {
    if (i < w) before += sW[i];
    total += sW[i];
  }
  unsigned long long run = before + inc - sum;
  for (uint64_t k = lo; k < hi; k++) {
    const unsigned long long c = p.stepsum[k];
    p.stepsum[k] = run;
    run += c;
  }
  if (t == 0u) {
    p.stepsum[steps] = total;
    *p.n_pieces = (uint64_t) p.n_sessions + total;
  }
}

/* the cuts at positions below a */
__device__ __forceinline__ uint64_t rank_below(const SParams &p, uint64_t total, uint64_t a)
{
  if (a >= (uint64_t) p.steps * kStep) return total;
  const uint64_t w = a >> 6;
  return p.stepsum[a >> 10] + p.inword[w] + (uint64_t) __popcll(p.mask[w] & ((1ull << (a & 63u)) - 1ull));
}

__global__ __launch_bounds__(256) void rhp_split_write_kernel(SParams p)
{
  const uint64_t total = p.stepsum[p.steps], np = (uint64_t) p.n_sessions + total;
  if (np > p.cap) return;   /* does not fit: *n_pieces only (rhp.h) */
  const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
  if (t <= p.n_sessions) {   /* a session's first piece; t == n_sessions: offsets[n_pieces], the input's end */
    const uint64_t a = p.sess_off[t];
    const uint64_t r = t + rank_below(p, total, a);   /* (<= np, the rank being at most the total) */
    p.offsets[r] = a;
    if (t < p.n_sessions) p.sessions[t].piece_lo = (uint32_t) r;
    if (t) p.sessions[t - 1u].piece_hi = (uint32_t) r;
  }
  if (t > np && t <= p.cap) p.offsets[t] = p.sess_off[p.n_sessions];
  if (t < (uint64_t) p.steps * 64u) {   /* the 16 positions from 16 t */
    const uint64_t w = t >> 2, m = p.mask[w];
    const uint32_t sh = 16u * ((uint32_t) t & 3u);
    uint32_t cut = (uint32_t) (m >> sh) & 0xffffu;
    if (!cut) return;
    uint64_t j = p.stepsum[t >> 6] + p.inword[w] + (uint64_t) __popcll(m & ((1ull << sh) - 1ull));
    for (; cut; cut &= cut - 1u, j++) {
      const uint64_t pos = 16u * t + (uint32_t) __builtin_ctz(cut);
      /* the sessions that start at or before pos: the cut lies in the last of them */
      uint32_t above = 0;
      for (uint32_t hi = p.n_sessions; above < hi;) {
        const uint32_t mid = above + ((hi - above) >> 1);
        if (p.sess_off[mid] <= pos) above = mid + 1u; else hi = mid;
      }
      const uint64_t at = (uint64_t) above + j;   /* (above - 1) + j + 1 */
      if (above && at < np) p.offsets[at] = pos;
    }
  }
}

}  // namespace

extern "C" int rhp_split_sessions(const uint8_t *bytes, uint64_t bytes_end, const uint64_t *sess_off, uint32_t n_sessions,
                                  const rhp_split_out_t *o, void *stream)
{
  const int rc = rhp_split_sessions_check(bytes, bytes_end, sess_off, n_sessions, o);
  if (rc < 0) return rc;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  SParams p;
  p.bytes = bytes;
  p.sess_off = sess_off;
  p.n_pieces = o->n_pieces;
  p.offsets = o->offsets;
  p.sessions = o->sessions;
  p.bytes_end = (uint32_t) bytes_end;
  p.n_sessions = n_sessions;
  p.steps = (uint32_t) ((bytes_end + kStep - 1u) / kStep);
  p.cap = o->cap_pieces;
  p.mask = o->work;
  p.inword = reinterpret_cast<uint32_t *>(p.mask + 16u * (uint64_t) p.steps);
  p.stepsum = p.mask + 24u * (uint64_t) p.steps;
  uint64_t threads = (uint64_t) p.steps * 64u;
  if (threads < (uint64_t) n_sessions + 1u) threads = (uint64_t) n_sessions + 1u;
  if (threads < (uint64_t) p.cap + 1u) threads = (uint64_t) p.cap + 1u;
  if (p.steps) hipLaunchKernelGGL(rhp_split_mark_kernel, dim3((p.steps + 3u) / 4u), dim3(256), 0, s, p);
  hipLaunchKernelGGL(rhp_split_scan_kernel, dim3(1), dim3(kScanThreads), 0, s, p);
  hipLaunchKernelGGL(rhp_split_write_kernel, dim3((uint32_t) ((threads + 255u) / 256u)), dim3(256), 0, s, p);
  return (int) hipGetLastError();
}
