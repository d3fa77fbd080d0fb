/*
 * rhp_chunked.hip -- rhp_decode_chunked (rhp.h): phr_decode_chunked over a
 * batch of streams whose new bytes lie in HBM.  gfx950.
 *
 * One wave per stream, four streams per workgroup, one launch; everything but
 * the bytes themselves is wave-uniform (the stream's index is read from the
 * first lane, the decoder and the offsets are uniform loads, every decision
 * comes from a ballot), so the walk is scalar code around two vector
 * operations:
 *   the window   lane l holds byte wb + l of the piece (zero at and beyond its
 *                end).  A state that scans (rhp_scalar.h decode_chunked_t is
 *                the byte-wise statement) is settled from the window's ballots,
 *                shifted down to src: the first non-hex byte, the first LF, the
 *                first non-CR byte.  The digits' values are read from the lanes
 *                below the first non-hex one.  A window is loaded again only
 *                when src has left it, so a short size line, the CR LF in front
 *                of it and the LF behind it cost one memory round trip; a line
 *                longer than the window (extensions, trailer lines) advances a
 *                window per step.
 *   the moves    a chunk's data is not scanned: it goes down by src - dst bytes
 *                through rhp_device::put, whose order is safe for a destination
 *                below the source (rhp_device.h), and is skipped by its length.
 *                The reference's closing memmove (:632-633) is the same move.
 * put stores bytes up to the first 16-aligned destination and behind the last,
 * 16-byte lines between them: nothing outside [dst, dst + n), which lies inside
 * the piece.  A window's and a move's loads stay inside the aligned dwords that
 * hold the piece.  decoders[i] is one 16-byte load and one 16-byte store,
 * results[i] one 16-byte store.  No LDS, no scratch.
 *
 * Whatever offsets[] holds: a piece's start and end are clamped to bytes_size,
 * as rhp_messages_kernel does.
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rhp.h"
#include "rhp_chunked_args.h"
#include "rhp_device.h"

namespace {

using rhp_device::put;
using rhp_device::u32x4;

struct CParams {
  uint8_t              *bytes;
  const uint64_t       *offsets;
  uint64_t              size;
  rhp_chunked_t        *decoders;
  rhp_chunked_result_t *results;
  uint32_t              n;
};

__device__ __forceinline__ bool is_hex(uint32_t c) { return c - '0' < 10u || (c | 0x20u) - 'a' < 6u; }

__global__ __launch_bounds__(256) void rhp_chunked_kernel(CParams p)
{
  static_assert(sizeof(rhp_chunked_t) == 16 && sizeof(rhp_chunked_result_t) == 16, "a decoder and a result are one 16-byte access each");
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t t = (uint64_t) blockIdx.x * 4u + (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x >> 6));
  if (t >= p.n) return;
  const uint32_t i = (uint32_t) t;
  uint64_t off = p.offsets[i], end = p.offsets[i + 1];
  off = off < p.size ? off : p.size;
  end = end < off ? off : end < p.size ? end : p.size;
  uint8_t *buf = p.bytes + off;
  const uint64_t len = end - off;

  const u32x4 dv = *reinterpret_cast<const u32x4 *>(p.decoders + i);
  uint64_t left = (uint64_t) dv[0] | (uint64_t) dv[1] << 32;
  const bool trailer = (dv[2] & 0xffu) != 0;
  uint32_t hex = (dv[2] >> 8) & 0xffu, st = (dv[2] >> 16) & 0xffu;
  int64_t ret = -2;
  uint64_t src = 0, dst = 0;
  if (RHP_CHUNKED_CORRUPT(st, hex)) {
    if (lane == 0) *reinterpret_cast<u32x4 *>(p.results + i) = u32x4{~0u, ~0u, 0u, 0u};
    return;
  }

  uint64_t wb = 0;                                        /* the window: bytes [wb, wb + 64) of the piece */
  uint32_t c = lane < len ? (uint32_t) buf[lane] : 0u;
  for (;;) {
    if (st == RHP_CHUNKED_IN_CHUNK_DATA) {
      const uint64_t avail = len - src, n = avail < left ? avail : left;
      if (dst != src && n) put(buf + dst, buf + src, n, lane);
      src += n;
      dst += n;
      left -= n;
      if (left) break;
      st = RHP_CHUNKED_IN_CHUNK_CRLF;
    }
    if (src == len) break;
    if (src - wb >= 64u) {
      wb = src;
      c = wb + lane < len ? (uint32_t) buf[wb + lane] : 0u;
    }
    const uint32_t k = (uint32_t) (src - wb);             /* the window's lane that holds byte src */
    const uint64_t rest = len - src;
    const uint32_t nw = rest < 64u - k ? (uint32_t) rest : 64u - k;   /* 1..64 bytes of the piece from src on */
    const uint64_t valid = nw == 64u ? ~0ull : (1ull << nw) - 1u;
    const uint64_t lf = (__ballot(c == '\n') >> k) & valid;
    if (st == RHP_CHUNKED_IN_CHUNK_SIZE) {
      const uint64_t nh = ((__ballot(!is_hex(c)) >> k) & valid) | ~valid;
      const uint32_t f = nh ? (uint32_t) __builtin_ctzll(nh) : 64u;   /* hex digits from src on: <= nw */
      const uint32_t room = 16u - hex, take = f < room ? f : room;
      const uint32_t v = c - '0' < 10u ? c - '0' : (c | 0x20u) - 'a' + 10u;
      for (uint32_t j = 0; j < take; j++) left = (left << 4) | (uint32_t) __builtin_amdgcn_readlane((int) v, (int) (k + j));
      hex += take;
      src += take;
      if (take < f) {   /* a 17th digit */
        ret = -1;
        break;
      }
      if (f == nw) continue;   /* digits up to the window's or the piece's end */
      if (hex == 0) {
        ret = -1;
        break;
      }
      hex = 0;
      st = RHP_CHUNKED_IN_CHUNK_EXT;
    } else if (st == RHP_CHUNKED_IN_CHUNK_EXT || st == RHP_CHUNKED_IN_TRAILERS_LINE_MIDDLE) {
      if (!lf) {
        src += nw;
        continue;
      }
      src += (uint32_t) __builtin_ctzll(lf) + 1u;
      if (st == RHP_CHUNKED_IN_TRAILERS_LINE_MIDDLE || (left == 0 && trailer)) st = RHP_CHUNKED_IN_TRAILERS_LINE_HEAD;
      else if (left != 0) st = RHP_CHUNKED_IN_CHUNK_DATA;
      else {
        ret = (int64_t) (len - src);
        break;
      }
    } else {   /* IN_CHUNK_CRLF, IN_TRAILERS_LINE_HEAD */
      const uint64_t ncr = (__ballot(c != '\r') >> k) & valid;
      if (!ncr) {
        src += nw;
        continue;
      }
      const uint32_t j = (uint32_t) __builtin_ctzll(ncr);
      const bool is_lf = ((lf >> j) & 1u) != 0;
      src += j;
      if (st == RHP_CHUNKED_IN_CHUNK_CRLF) {
        if (!is_lf) {
          ret = -1;
          break;
        }
        src++;
        st = RHP_CHUNKED_IN_CHUNK_SIZE;
      } else {
        src++;
        if (is_lf) {
          ret = (int64_t) (len - src);
          break;
        }
        st = RHP_CHUNKED_IN_TRAILERS_LINE_MIDDLE;
      }
    }
  }
  if (dst != src && src < len) put(buf + dst, buf + src, len - src, lane);
  if (lane == 0) {
    *reinterpret_cast<u32x4 *>(p.results + i) = u32x4{(uint32_t) (uint64_t) ret, (uint32_t) ((uint64_t) ret >> 32), (uint32_t) dst, (uint32_t) (dst >> 32)};
    *reinterpret_cast<u32x4 *>(p.decoders + i) = u32x4{(uint32_t) left, (uint32_t) (left >> 32), (dv[2] & 0xff0000ffu) | hex << 8 | st << 16, dv[3]};
  }
}

}  // namespace

extern "C" int rhp_decode_chunked(const rhp_chunked_batch_t *b, void *stream)
{
  const int rc = rhp_chunked_batch_check(b, 1);
  if (rc != 0) return rc < 0 ? rc : 0;
  CParams p;
  p.bytes = b->bytes;
  p.offsets = b->offsets;
  p.size = b->bytes_size;
  p.decoders = b->decoders;
  p.results = b->results;
  p.n = b->n;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((uint32_t) (((uint64_t) b->n + 3u) / 4u));
  hipLaunchKernelGGL(rhp_chunked_kernel, grid, dim3(256), 0, s, p);
  return (int) hipGetLastError();
}
