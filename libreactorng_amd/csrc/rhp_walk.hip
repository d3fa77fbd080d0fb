/*
 * rhp_walk.hip -- rhp_walk_responses (rhp.h): the pipelined responses of a
 * batch of upstream connections walked in HBM, rhp_walk_resume, the same
 * walk carried from round to round by a 32-byte state per session, and
 * rhp_walk_answers, either of them told which requests were HEAD.  gfx950.
 *
 * One session per lane, one launch: the lane runs the walk's one statement
 * (rhp_scalar.h walk_session_t) -- the code the host twin runs over plain
 * memory -- which is phr_parse_response, the framing decision and the chunked
 * decoder of rhp_parse_messages, rhp_frame_messages and rhp_decode_chunked,
 * message after message.  Bytes come through the bounded 16-byte line cache of
 * rhp_messages.hip (rhp_device.h BoundedLineBytes): one dependent aligned
 * 16-byte load per 16 bytes scanned, nothing loaded at or behind the readable
 * end (rhp_walk_args.h), where the reader sees zeros.  Records leave whole: a
 * header record as one 8-byte store, a message record and a session's result
 * as one 16-byte store, a slot as two.  The header records are read back as
 * the 8-byte words they were stored as, and of name and value bytes only those
 * inside [pos, pos + ret) of a parsed message, which lie below the session's
 * clamped end.  A completed chunked body is de-framed by the one-thread move of
 * the request path (rhp_device.h DevMove), which stores only inside
 * [dst, dst + n).
 *
 * Whatever sess_off and slot_off hold: a session's ends are clamped to the
 * readable end, so every scan ends and every address read lies below
 * bytes_size; a slot index becomes an address only inside the session's own
 * range, which is empty unless it lies inside [0, n_slots_total).
 *
 * Lane-per-session leaves a wave's other lanes idle while one long session is
 * walked; whether few long sessions want another shape is not measured
 * (DESIGN.md 3.12).
 */
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "rhp.h"
#include "rhp_device.h"
#include "rhp_walk_args.h"
#include "rhp_scalar.h"

namespace {

using namespace rhp;
using rhp_device::BoundedLineBytes;
using rhp_device::DevMove;
using rhp_device::DevMsgStore;
using rhp_device::u32x4;

struct WParams {
  const uint8_t     *bytes;
  uint8_t           *bytes_rw;
  const uint64_t    *sess_off, *slot_off;
  uint64_t           lim;            /* rhp_walk_readable(bytes_size) */
  rhp_msg_t         *msgs;
  rhp_hdr_t         *hdrs;
  rhp_walk_slot_t   *slots;
  rhp_walk_result_t *results;
  uint32_t           n_sessions, n_slots_total, max_headers, flags;
};

/* HdrsRec (rhp_scalar.h) over records DevMsgStore has just stored: each is
 * loaded as the 8-byte word it left as */
struct DevHdrs {
  const uint8_t *b;
  const rhp_hdr_t *h;
  __device__ rhp_hdr_t at(uint32_t i) const
  {
    const uint2 w = *reinterpret_cast<const uint2 *>(h + i);
    rhp_hdr_t r;
    __builtin_memcpy(&r, &w, 8);
    return r;
  }
  __device__ bool null(uint32_t i) const { return at(i).name_off == RHP_NAME_NULL; }
  __device__ const uint8_t *name(uint32_t i) const { return b + at(i).name_off; }
  __device__ uint64_t name_len(uint32_t i) const { return at(i).name_len; }
  __device__ const uint8_t *value(uint32_t i) const { return b + at(i).value_off; }
  __device__ uint64_t value_len(uint32_t i) const { return at(i).value_len; }
};

/* walk_session_t's io over the batch in HBM */
struct DevWalkIO {
  const WParams &p;
  __device__ BoundedLineBytes bytes(uint64_t at) const { return BoundedLineBytes{p.bytes, at, p.lim, ~0ull, {0, 0, 0, 0}}; }
  __device__ DevMsgStore store(uint32_t slot) const
  {
    return DevMsgStore{p.msgs + slot, p.hdrs + (uint64_t) slot * p.max_headers, 1};
  }
  __device__ DevHdrs hdrs(uint32_t slot, uint64_t at) const
  {
    return DevHdrs{p.bytes + at, p.hdrs + (uint64_t) slot * p.max_headers};
  }
  __device__ DevMove move(uint64_t at) const { return DevMove{p.bytes_rw + at}; }
  __device__ void slot(uint32_t slot, const rhp_walk_slot_t &x) const
  {
    static_assert(sizeof(rhp_walk_slot_t) == 32, "a slot is two 16-byte stores");
    u32x4 w[2];
    __builtin_memcpy(w, &x, 32);
    u32x4 *d = reinterpret_cast<u32x4 *>(p.slots + slot);
    d[0] = w[0];
    d[1] = w[1];
  }
};

__global__ __launch_bounds__(256) void rhp_walk_kernel(WParams p)
{
  const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
  if (t >= p.n_sessions) return;
  const uint32_t s = (uint32_t) t;
  uint64_t a = p.sess_off[s], e = p.sess_off[s + 1];
  a = a < p.lim ? a : p.lim;
  e = e < a ? a : e < p.lim ? e : p.lim;
  uint64_t lo = p.slot_off[s], hi = p.slot_off[s + 1];
  if (lo > hi || hi > p.n_slots_total) hi = lo = 0;   /* owns no slot */
  DevWalkIO io{p};
  rhp_walk_result_t r;
  NobodyAsked nobody;
  walk_session_t(io, a, e, (uint32_t) lo, (uint32_t) hi, p.max_headers, p.flags, &r, nobody);
  static_assert(sizeof(rhp_walk_result_t) == 16, "a result is one 16-byte store");
  u32x4 w;
  __builtin_memcpy(&w, &r, 16);
  *reinterpret_cast<u32x4 *>(p.results + s) = w;
}

/* rhp_walk_resume: the same lane per session over walk_resume_t, from
 * states[s] (two 16-byte loads) to states[s] (two 16-byte stores, none where
 * the statement keeps the state as it lies).  A continuation reads and moves
 * from the session's first byte on, with the reader and the move of the walk
 * above: nothing loaded at or behind the readable end, nothing stored outside
 * [a, e). */
struct RParams {
  WParams w;
  rhp_walk_state_t *states;
};

__global__ __launch_bounds__(256) void rhp_walk_resume_kernel(RParams q)
{
  const WParams &p = q.w;
  const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
  if (t >= p.n_sessions) return;
  const uint32_t s = (uint32_t) t;
  uint64_t a = p.sess_off[s], e = p.sess_off[s + 1];
  a = a < p.lim ? a : p.lim;
  e = e < a ? a : e < p.lim ? e : p.lim;
  uint64_t lo = p.slot_off[s], hi = p.slot_off[s + 1];
  if (lo > hi || hi > p.n_slots_total) hi = lo = 0;   /* owns no slot */
  static_assert(sizeof(rhp_walk_state_t) == 32, "a state is two 16-byte accesses");
  u32x4 *sp = reinterpret_cast<u32x4 *>(q.states + s);
  u32x4 sw[2] = {sp[0], sp[1]};
  rhp_walk_state_t st;
  __builtin_memcpy(&st, sw, 32);
  DevWalkIO io{p};
  rhp_walk_result_t r;
  NobodyAsked nobody;
  if (walk_resume_t(io, a, e, (uint32_t) lo, (uint32_t) hi, p.max_headers, p.flags, &st, &r, nobody)) {
    __builtin_memcpy(sw, &st, 32);
    sp[0] = sw[0];
    sp[1] = sw[1];
  }
  u32x4 w;
  __builtin_memcpy(&w, &r, 16);
  *reinterpret_cast<u32x4 *>(p.results + s) = w;
}

/* rhp_walk_answers: either walk above with the Asked policy (rhp_scalar.h)
 * over the session's queue, RESUME choosing which -- two kernels, the same lane
 * per session.  The lane reads its req_off pair, keeps the current head_bits
 * word in a register (one 4-byte load per 32 requests of its queue, none
 * outside the clamped queue) and stores answered[s] and the slot_req entries of
 * the slots it wrote as plain 4-byte stores. */
struct AParams {
  WParams w;
  rhp_walk_state_t *states;   /* RESUME */
  const uint32_t *req_off, *head_bits;
  uint32_t *answered, *slot_req;
  uint32_t n_req_total;
};

template <bool RESUME>
__global__ __launch_bounds__(256) void rhp_walk_answers_kernel(AParams q)
{
  const WParams &p = q.w;
  const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
  if (t >= p.n_sessions) return;
  const uint32_t s = (uint32_t) t;
  uint64_t a = p.sess_off[s], e = p.sess_off[s + 1];
  a = a < p.lim ? a : p.lim;
  e = e < a ? a : e < p.lim ? e : p.lim;
  uint64_t lo = p.slot_off[s], hi = p.slot_off[s + 1];
  if (lo > hi || hi > p.n_slots_total) hi = lo = 0;   /* owns no slot */
  Asked ask;
  ask.head_bits = q.head_bits;
  ask.slot_req = q.slot_req;
  ask.nq = rhp_walk_queue(q.req_off[s], q.req_off[s + 1], q.n_req_total, &ask.q0);
  ask.k = 0;
  ask.have = ~0u;
  ask.word = 0;
  DevWalkIO io{p};
  rhp_walk_result_t r;
  if (RESUME) {
    u32x4 *sp = reinterpret_cast<u32x4 *>(q.states + s);
    u32x4 sw[2] = {sp[0], sp[1]};
    rhp_walk_state_t st;
    __builtin_memcpy(&st, sw, 32);
    if (walk_resume_t(io, a, e, (uint32_t) lo, (uint32_t) hi, p.max_headers, p.flags, &st, &r, ask)) {
      __builtin_memcpy(sw, &st, 32);
      sp[0] = sw[0];
      sp[1] = sw[1];
    }
  } else {
    walk_session_t(io, a, e, (uint32_t) lo, (uint32_t) hi, p.max_headers, p.flags, &r, ask);
  }
  u32x4 w;
  __builtin_memcpy(&w, &r, 16);
  *reinterpret_cast<u32x4 *>(p.results + s) = w;
  q.answered[s] = ask.k;
}

}  // namespace

static WParams walk_params(const rhp_walk_batch_t *b)
{
  WParams p;
  p.bytes = b->bytes;
  p.bytes_rw = b->bytes_rw;
  p.sess_off = b->sess_off;
  p.slot_off = b->slot_off;
  p.lim = rhp_walk_readable(b->bytes_size);
  p.msgs = b->msgs;
  p.hdrs = b->hdrs;
  p.slots = b->slots;
  p.results = b->results;
  p.n_sessions = b->n_sessions;
  p.n_slots_total = b->n_slots_total;
  p.max_headers = b->max_headers;
  p.flags = b->flags;
  return p;
}

extern "C" int rhp_walk_responses(const rhp_walk_batch_t *b, void *stream)
{
  const int rc = rhp_walk_check(b, 1);
  if (rc != 0) return rc < 0 ? rc : 0;
  const WParams p = walk_params(b);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((uint32_t) (((uint64_t) b->n_sessions + 255u) / 256u));
  hipLaunchKernelGGL(rhp_walk_kernel, grid, dim3(256), 0, s, p);
  return (int) hipGetLastError();
}

extern "C" int rhp_walk_resume(const rhp_walk_batch_t *b, rhp_walk_state_t *states, void *stream)
{
  const int rc = rhp_walk_resume_check(b, states, 1);
  if (rc != 0) return rc < 0 ? rc : 0;
  const RParams q = {walk_params(b), states};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((uint32_t) (((uint64_t) b->n_sessions + 255u) / 256u));
  hipLaunchKernelGGL(rhp_walk_resume_kernel, grid, dim3(256), 0, s, q);
  return (int) hipGetLastError();
}

extern "C" int rhp_walk_answers(const rhp_walk_batch_t *b, rhp_walk_state_t *states, const rhp_walk_asked_t *x, void *stream)
{
  const int rc = rhp_walk_answers_check(b, states, x, 1);
  if (rc != 0) return rc < 0 ? rc : 0;
  const AParams q = {walk_params(b), states, x->req_off, x->head_bits, x->answered, x->slot_req, x->n_req_total};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((uint32_t) (((uint64_t) b->n_sessions + 255u) / 256u));
  if (states) hipLaunchKernelGGL(rhp_walk_answers_kernel<true>, grid, dim3(256), 0, s, q);
  else hipLaunchKernelGGL(rhp_walk_answers_kernel<false>, grid, dim3(256), 0, s, q);
  return (int) hipGetLastError();
}
