/*
 * rhp_messages.hip -- rhp_parse_messages (rhp.h): phr_parse_response and
 * phr_parse_headers over a batch of messages in HBM.  gfx950.
 *
 * One message per lane, one launch: the lane runs the exact scalar statement
 * of its kind (rhp_scalar.h scalar_response_t / scalar_headers_t, behind
 * is_complete when last_len says so) -- the code the host twin runs over
 * PlainBytes -- through the 16-byte line cache of the exact request path
 * (rhp_kernel.hip LineBytes), here with an end: only whole lines below
 * bytes + bytes_size are loaded, anything behind them reads as zeros (what the
 * last line of the pad holds anyway: a message ends RHP_PAD bytes before
 * bytes_size).  The records leave whole: a header
 * record as one 8-byte store at its RHP_HDR() position when its line ends, the
 * message record as one 16-byte store when the parse returns.
 *
 * Whatever offsets[] holds: a message's start and end are clamped to
 * bytes_size, so every scan ends; record k of message i is written only for
 * k < max_headers and i < n.
 *
 * A pair-DFA kernel for responses, built like rhp_dfa_kernel, is the follow-up
 * (DESIGN.md 10).
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rhp.h"
#include "rhp_device.h"
#include "rhp_msg_args.h"
#include "rhp_scalar.h"

namespace {

using namespace rhp;
using rhp_device::BoundedLineBytes;
using rhp_device::DevMsgStore;

struct MParams {
  const uint8_t  *bytes;
  const uint64_t *offsets, *last_len;
  uint64_t        size;             /* bytes_size rounded down to whole 16-byte lines */
  rhp_msg_t      *msgs;
  rhp_hdr_t      *hdrs;
  uint32_t        n, max_headers;
  uint32_t        hs_req, hs_hdr;   /* record k of message i at hdrs[i * hs_req + k * hs_hdr] */
};

template <uint32_t KIND>
__global__ __launch_bounds__(256) void rhp_messages_kernel(MParams p)
{
  const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
  if (t >= p.n) return;
  const uint32_t i = (uint32_t) t;
  uint64_t off = p.offsets[i], end = p.offsets[i + 1];
  off = off < p.size ? off : p.size;
  end = end < off ? off : end < p.size ? end : p.size;
  const uint64_t ll = p.last_len ? p.last_len[i] : 0;
  BoundedLineBytes B{p.bytes, off, p.size, ~0ull, {0, 0, 0, 0}};
  OutMsg<DevMsgStore> out{{p.msgs + i, p.hdrs + (uint64_t) i * p.hs_req, p.hs_hdr}};
  scalar_message_t<KIND>(B, end - off, ll, p.max_headers, out);
}

}  // namespace

extern "C" int rhp_parse_messages(const rhp_msg_batch_t *b, void *stream)
{
  const int rc = rhp_msg_batch_check(b, 1);
  if (rc != 0) return rc < 0 ? rc : 0;
  const bool hmajor = b->layout == RHP_LAYOUT_HEADER_MAJOR;
  MParams p;
  p.bytes = b->bytes;
  p.offsets = b->offsets;
  p.last_len = b->last_len;
  p.size = b->bytes_size & ~(uint64_t) 15;
  p.msgs = b->msgs;
  p.hdrs = b->hdrs;
  p.n = b->n;
  p.max_headers = b->max_headers;
  p.hs_req = hmajor ? 1u : b->max_headers;
  p.hs_hdr = hmajor ? b->n : 1u;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((uint32_t) (((uint64_t) b->n + 255u) / 256u));
  if (b->kind == RHP_MSG_RESPONSE)
    hipLaunchKernelGGL(rhp_messages_kernel<RHP_MSG_RESPONSE>, grid, dim3(256), 0, s, p);
  else
    hipLaunchKernelGGL(rhp_messages_kernel<RHP_MSG_HEADERS>, grid, dim3(256), 0, s, p);
  return (int) hipGetLastError();
}
