/*
 * rhp_host.cpp -- the product's host entry points (rhp_host.h): the exact
 * scalar parser over a batch in host memory, the session fix-up, the dense
 * pack and the three expansions, the host classify, reply, gather and split, the
 * message parse (responses, header blocks), their framing, the chunked decoder, the response walk, its lookup and its relay, the forward, and the pointer-based
 * rhp_phr_parse_request / _response / _headers, rhp_phr_decode_chunked and rhp_http_read_cpu.  libreactor.so links them.  The
 * parser is rhp_scalar.h's (the code the kernel's rare paths run); where the
 * records sit and how they are encoded is rhp_records.h's.
 */
#include <stdint.h>
#include <string.h>
#include <vector>

#include "rhp.h"
#include "rhp_host.h"
#include "rhp_records.h"
#include "rhp_scalar.h"
#include "rhp_classify_args.h"
#include "rhp_reply_args.h"
#include "rhp_gather_args.h"
#include "rhp_split_args.h"
#include "rhp_msg_args.h"
#include "rhp_chunked_args.h"
#include "rhp_frame_args.h"
#include "rhp_walk_args.h"
#include "rhp_lookup_args.h"
#include "rhp_relay_args.h"
#include "rhp_forward_args.h"
#include "rhp_host_exact.h"

using namespace rhp;

void rhp::host_put_http(const rhp_view_t &v, uint32_t i, const rhp_http_t &x, bool wide)
{
  if (!v.hc) {
    v.http[i] = x;
    return;
  }
  if (wide) v.http[i] = x;
  v.hc[i] = rhp_http_compact_encode(&x, wide);
}

void rhp::host_exact(const rhp_batch_t *b, const rhp_view_t &v, uint32_t i, uint64_t off, uint64_t len)
{
  rhp_req_t r;
  /* a length layout: the exact path's records are the wide ones */
  r.flags = RHP_F_EXACT | (rhp_layout_lens(b->layout) ? RHP_F_WIDE : 0u);
  rhp_hdr_t *h = v.hdrs + i * v.hs_req;
  if (b->mode == RHP_MODE_HTTP) {
    PlainBytes B{b->bytes_rw + off};
    rhp_http_t x;
    scalar_http_t(B, b->bytes_rw + off, len, b->max_headers, &r, h, v.hs_hdr, &x, !(b->flags & RHP_BATCH_SPECULATIVE));
    host_put_http(v, i, x, true);
  }
  else {
    const uint64_t ll = b->last_len ? b->last_len[i] : 0;
    const int pre = ll ? is_complete(b->bytes + off, len, ll) : 0;   /* picohttpparser.c:399-401 */
    if (pre != 0) {
      const uint16_t flags = r.flags;
      memset(&r, 0, sizeof r);
      r.ret = pre;
      r.minor_version = -1;
      r.flags = flags;
    } else {
      scalar_phr(b->bytes + off, len, b->max_headers, &r, h, v.hs_hdr);
    }
  }
  v.reqs[i] = r;
  if (v.dreq) v.dreq[i] = rhp_req_dense_mark(RHP_DENSE_WIDE);
}

/* The exact scalar path alone, on the host (the product's CPU parser): in a
 * length layout every record is a wide one. */
extern "C" int rhp_cpu_parse_batch(const rhp_batch_t *b)
{
  if (rhp_batch_check(b, 0) < 0) return -22;
  const rhp_view_t v = rhp_batch_view(b);
  for (uint32_t i = 0; i < b->n; i++) host_exact(b, v, i, b->offsets[i], b->offsets[i + 1] - b->offsets[i]);
  return 0;
}

/* rhp_fixup_sessions (rhp.h) on the host: the same walk (rhp_scalar.h
 * fixup_session_t) over a speculative batch parsed by rhp_cpu_parse_batch or
 * rhp_emu_parse_batch. */
extern "C" int rhp_cpu_fixup_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                      rhp_session_result_t *results, uint64_t *req_start)
{
  if (!b || b->mode != RHP_MODE_HTTP || !(b->flags & RHP_BATCH_SPECULATIVE)) return -22;
  const rhp_view_t v = rhp_batch_view(b);
  const FixupIO io{b->bytes_rw, b->offsets, v.reqs, v.hdrs, v.http, v.hs_req, v.hs_hdr, b->max_headers};
  for (uint32_t k = 0; k < n_sessions; k++)
    fixup_session_t(io, sessions[k].piece_lo, sessions[k].piece_hi, req_start, &results[k],
                    [&](uint64_t at) { return PlainBytes{b->bytes_rw + at}; });
  return 0;
}

extern "C" int rhp_expand_reqs(const rhp_batch_t *b, const void *reqs, rhp_req_t *out)
{
  if (!b || !reqs || !out) return -22;
  const rhp_view_t v = rhp_view(reqs, nullptr, nullptr, b->n, b->max_headers, b->mode, b->layout);
  if (!v.dreq) {
    memcpy(out, reqs, sizeof(rhp_req_t) * b->n);
    return 0;
  }
  for (uint32_t i = 0; i < b->n; i++) out[i] = rhp_req_dense_decode(v.dreq[i], &v.reqs[i]);
  return 0;
}

extern "C" int rhp_expand_records(const rhp_batch_t *b, const rhp_req_t *reqs, const void *hdrs, rhp_hdr_t *out)
{
  if (!b || !reqs || !out || (b->max_headers && !hdrs)) return -22;
  if (b->layout > RHP_LAYOUT_DENSE_RM) return -22;
  const uint32_t n = b->n, m = b->max_headers;
  const rhp_view_t v = rhp_view(nullptr, hdrs, nullptr, n, m, b->mode, b->layout);
  const bool lens = rhp_layout_lens(b->layout);
  for (uint32_t i = 0; i < n; i++) {
    rhp_hdr_t *o = out + (uint64_t) i * m;
    memset(o, 0, sizeof(rhp_hdr_t) * m);
    const rhp_req_t &r = reqs[i];
    if (r.ret <= 0) continue;
    const uint32_t nh = r.num_headers < m ? r.num_headers : m;
    if (lens && !(r.flags & RHP_F_WIDE)) {
      uint32_t at = rhp_hdr_first(&r);
      for (uint32_t k = 0; k < nh; k++) o[k] = rhp_hdr_next(&at, rhp_view_len32(&v, i, k));
    } else {
      for (uint32_t k = 0; k < nh; k++) o[k] = v.hdrs[i * v.hs_req + k * v.hs_hdr];
    }
  }
  return 0;
}

extern "C" int rhp_expand_http(const rhp_batch_t *b, const rhp_req_t *reqs, const void *http, rhp_http_t *out)
{
  if (!b || !reqs || !http || !out) return -22;
  /* the http records are what the layout says in RHP_MODE_HTTP, whatever mode `b` names */
  const rhp_view_t v = rhp_view(nullptr, nullptr, http, b->n, b->max_headers, RHP_MODE_HTTP, b->layout);
  if (!v.hc) {
    memcpy(out, http, sizeof(rhp_http_t) * b->n);
    return 0;
  }
  for (uint32_t i = 0; i < b->n; i++) out[i] = rhp_http_compact_decode(v.hc[i], reqs[i].ret, &v.http[i]);
  return 0;
}

/* rhp_pack_dense (rhp.h) on the host: rhp_pack_dense_one per record slot, as
 * the kernel (rhp_kernel.hip rhp_pack_dense_kernel), for the reactor's
 * host-async parser */
extern "C" int rhp_cpu_pack_dense(const rhp_batch_t *b, rhp_req_dense_t *dreq, rhp_http_compact_t *hc, uint16_t *lens16)
{
  if (!b || b->mode != RHP_MODE_HTTP || b->layout != RHP_LAYOUT_REQUEST_MAJOR || b->max_headers > RHP_MAX_HEADERS) return -22;
  const uint32_t n = b->n, m = b->max_headers;
  for (uint32_t i = 0; i < n; i++)
    dreq[i] = rhp_pack_dense_one(&b->reqs[i], &b->http[i], b->hdrs + (uint64_t) i * m, m, lens16 + i, n, &hc[i]);
  return 0;
}

namespace {

/* slot i of the classification as an absent request has it */
void classify_absent(const rhp_classify_t *c, uint32_t n, uint32_t i)
{
  for (uint32_t j = 0; j < c->n_names; j++) c->fields[(size_t) j * n + i] = rhp_fieldref_t{RHP_NAME_NULL, 0};
  if (c->route) c->route[i] = RHP_ROUTE_NONE;
}

/* Slot i of the classification, absent on entry (classify_absent), for one
 * ready request (r.ret > 0) whose first byte is req[0] and whose header record
 * k < min(r.num_headers, m) is hdr(k):
 * http_field_lookup (src/reactor/http.c:167-175: the first field whose name is
 * string_equal_case, src/reactor/data.c:11-28) per name and the first route
 * whose target and method are string_equal, one byte at a time.  Both host
 * twins classify here.  As in the kernels (rhp_classify.hip),
 * no byte outside [req, req + ret) is read: a name that ends
 * past ret matches nothing, and a path or method that does takes no route.
 * No parsed record is like that; rhp_cpu_classify_batch used to read such
 * offsets as they stood, where its kernel did not. */
template <class Hdr>
void classify_one(const rhp_classify_t *c, uint32_t n, uint32_t m, uint32_t i, const uint8_t *req, const rhp_req_t &r, Hdr hdr)
{
  const uint64_t ret = (uint64_t) r.ret;
  const uint32_t nh = r.num_headers < m ? r.num_headers : m;
  const auto upper = [](uint8_t x) { return x >= 'a' && x <= 'z' ? (uint8_t) (x - ('a' - 'A')) : x; };   /* C-locale toupper */
  const auto same = [&](const uint8_t *s, uint32_t len, rhp_span_t t) {
    return len == t.len && (len == 0 || memcmp(s, c->text + t.off, len) == 0);
  };
  for (uint32_t j = 0; j < c->n_names; j++) {
    const uint8_t *name = c->text + c->names[j].off;
    const uint32_t len = c->names[j].len;
    for (uint32_t k = 0; k < nh; k++) {
      const rhp_hdr_t &h = hdr(k);
      if (h.name_off == RHP_NAME_NULL || h.name_len != len) continue;
      if ((uint64_t) h.name_off + len > ret) continue;   /* (a parsed name lies inside its header section) */
      uint32_t q = 0;
      while (q < len && upper(req[h.name_off + q]) == upper(name[q])) q++;
      if (q == len) {
        c->fields[(size_t) j * n + i] = rhp_fieldref_t{h.value_off, h.value_len};
        break;
      }
    }
  }
  if (!c->route) return;
  if ((uint64_t) r.path_off + r.path_len > ret || (uint64_t) r.method_off + r.method_len > ret) return;
  for (uint32_t k = 0; k < c->n_routes; k++) {
    const rhp_route_t &t = c->routes[k];
    if (same(req + r.path_off, r.path_len, t.target) && (t.method.len == 0 || same(req + r.method_off, r.method_len, t.method))) {
      c->route[i] = (uint16_t) k;
      break;
    }
  }
}

}  // namespace

/* rhp_classify_batch (rhp.h) on the host, over a parsed batch in host memory:
 * classify_one per ready request, over the records as rhp_expand_reqs /
 * rhp_expand_records / rhp_expand_http give them -- a decode of the layouts
 * that shares nothing with the kernel's (rhp_classify.hip). */
extern "C" int rhp_cpu_classify_batch(const rhp_batch_t *b, const rhp_classify_t *c)
{
  const int rc = rhp_classify_check(b, c);
  if (rc != 0) return rc < 0 ? rc : 0;
  const uint32_t n = b->n, m = b->max_headers;
  const bool http_mode = b->mode == RHP_MODE_HTTP;
  std::vector<rhp_req_t> reqs(n);
  std::vector<rhp_hdr_t> hdrs((size_t) n * m);
  std::vector<rhp_http_t> http(http_mode ? n : 0);
  if (rhp_expand_reqs(b, b->reqs, reqs.data()) != 0) return -22;
  if (m && rhp_expand_records(b, reqs.data(), b->hdrs, hdrs.data()) != 0) return -22;
  if (http_mode && rhp_expand_http(b, reqs.data(), b->http, http.data()) != 0) return -22;
  const uint8_t *bytes = http_mode && b->bytes_rw ? b->bytes_rw : b->bytes;
  for (uint32_t i = 0; i < n; i++) {
    classify_absent(c, n, i);
    if (reqs[i].ret > 0 && (!http_mode || http[i].result == 1))
      classify_one(c, n, m, i, bytes + b->offsets[i], reqs[i], [&](uint32_t k) -> const rhp_hdr_t & { return hdrs[(size_t) i * m + k]; });
  }
  return 0;
}

/* rhp_classify_sessions (rhp.h) on the host, over the speculative batch
 * rhp_cpu_parse_batch / rhp_emu_parse_batch and a host fix-up left in host
 * memory.  Every slot is absent first; then the sessions are walked one after
 * the other and the slots each one filled, piece_lo .. piece_lo + n_slots, are
 * classified (classify_one) from req_start[slot] -- no search, so the walk
 * takes the sessions in any order.  That a request lies inside its session's
 * input is tested here, before classify_one reads a byte of it.  rhp_hdr_t
 * records only (a speculative batch has no other kind). */
extern "C" int rhp_cpu_classify_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                         const rhp_session_result_t *results, const uint64_t *req_start,
                                         const rhp_classify_t *c)
{
  const int rc = rhp_classify_sessions_check(b, sessions, n_sessions, results, req_start, c);
  if (rc != 0) return rc < 0 ? rc : 0;
  const uint32_t n = b->n, m = b->max_headers;
  const uint8_t *bytes = b->bytes_rw ? b->bytes_rw : b->bytes;
  for (uint32_t i = 0; i < n; i++) classify_absent(c, n, i);
  for (uint32_t s = 0; s < n_sessions; s++) {
    const uint32_t lo = sessions[s].piece_lo, hi = sessions[s].piece_hi;
    if (lo > hi || hi > n) continue;   /* not a session of this batch */
    for (uint32_t q = 0; q < results[s].n_slots && q < n - lo; q++) {
      const uint32_t i = lo + q;
      const rhp_req_t &r = b->reqs[i];
      if (b->http[i].result != 1 || r.ret <= 0) continue;
      /* the request lies inside its session's input */
      const uint64_t at = req_start[i];
      if (at < b->offsets[lo] || at > b->offsets[hi] || (uint64_t) r.ret > b->offsets[hi] - at) continue;
      classify_one(c, n, m, i, bytes + at, r, [&](uint32_t k) -> const rhp_hdr_t & { return RHP_HDR(b->hdrs, b->layout, n, m, i, k); });
    }
  }
  return 0;
}

/* rhp_reply_sessions (rhp.h) on the host, every pointer in host memory: a plain
 * walk, session by session and slot by slot -- the leading run of static slots
 * of a session whose fields hold and whose walk did not stop on -1, its sizes
 * summed on the way; then, when the total fits, the images copied in the same
 * order.  It shares the argument check with the kernels' launcher
 * (rhp_reply_args.h) and nothing else. */
extern "C" int rhp_cpu_reply_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                      const rhp_session_result_t *results, const uint16_t *route,
                                      const rhp_reply_table_t *t, const rhp_reply_out_t *o)
{
  const int rc = rhp_reply_sessions_check(b, sessions, n_sessions, results, route, t, o, 1);
  if (rc < 0) return rc;
  const uint32_t n = rc == 1 ? 0 : b->n;
  const auto is_static = [&](uint32_t r) { return r < t->n_routes && ((t->static_mask >> r) & 1u); };
  uint64_t total = 0;
  for (uint32_t s = 0; s < n_sessions; s++) {
    const uint32_t lo = sessions[s].piece_lo, hi = sessions[s].piece_hi, ns = results[s].n_slots;
    uint32_t count = 0;
    uint64_t len = 0;
    if ((uint64_t) lo + ns <= hi && hi <= n && ns >= 1 && b->http[lo + ns - 1u].result != -1)
      for (; count < ns && is_static(route[lo + count]); count++) {
        const uint32_t r = route[lo + count];
        len += t->image_off[r + 1u] - t->image_off[r];
      }
    o->replies[s] = rhp_session_reply_t{count, 0, total, len};
    total += len;
  }
  *o->total = total;
  if (total > o->out_size) return 0;   /* sizes only */
  for (uint32_t s = 0; s < n_sessions; s++) {
    uint64_t at = o->replies[s].out_off;
    for (uint32_t q = 0; q < o->replies[s].count; q++) {
      const uint32_t r = route[sessions[s].piece_lo + q];
      const uint64_t len = t->image_off[r + 1u] - t->image_off[r];
      if (len) memcpy(o->out + at, t->images + t->image_off[r], len);
      at += len;
    }
  }
  return 0;
}

/* rhp_gather_wide (rhp.h) on the host, every pointer in host memory: a plain
 * walk, session by session and slot by slot, twice -- the totals first, then,
 * when they fit the caps, the records, header records and bodies in the same
 * order.  With the sessions in order that is ascending slot order.  It shares
 * the argument check with the kernels' launcher (rhp_gather_args.h) and
 * nothing else. */
extern "C" int rhp_cpu_gather_wide(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                   const rhp_session_result_t *results, const uint64_t *req_start,
                                   const rhp_req_dense_t *dreq, const rhp_http_compact_t *hc, const rhp_wide_out_t *o)
{
  const int rc = rhp_gather_wide_check(b, sessions, n_sessions, results, req_start, dreq, hc, o);
  if (rc < 0) return rc;
  rhp_wide_totals_t tot = {0, 0, 0};
  if (rc == 1) {
    *o->totals = tot;
    return 0;
  }
  const uint32_t n = b->n, m = b->max_headers;
  const uint8_t *bytes = b->bytes_rw ? b->bytes_rw : b->bytes;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t at_slot = 0, at_hdr = 0, at_body = 0;
    for (uint32_t s = 0; s < n_sessions; s++) {
      const uint32_t lo = sessions[s].piece_lo, hi = sessions[s].piece_hi, ns = results[s].n_slots;
      if (!((uint64_t) lo + ns <= hi && hi <= n)) continue;   /* owns nothing */
      for (uint32_t i = lo; i < lo + ns; i++) {
        const bool hw = hc[i].flags & RHP_HTTP_WIDE;
        if (!hw && !(hc[i].result == 1 && (dreq[i].flags & RHP_DENSE_WIDE))) continue;
        const rhp_req_t &r = b->reqs[i];
        const rhp_http_t &x = b->http[i];
        const uint32_t nh = x.result == 1 && r.ret > 0 && r.num_headers <= m ? r.num_headers : 0u;
        const uint64_t from = req_start[i] + (uint64_t) (int64_t) r.ret;
        bool body = x.result == 1 && x.body_kind == 1u && x.consumed != (uint64_t) (int64_t) r.ret + x.body_len;
        body = body && b->offsets[lo] <= from && from <= b->offsets[hi] && x.body_len <= b->offsets[hi] - from;
        if (pass) {
          rhp_wide_slot_t w;
          w.slot = i;
          w.hdr_first = (uint32_t) at_hdr;
          w.req = r;
          w.http = x;
          w.req_start = req_start[i];
          w.body_off = body ? at_body : RHP_WIDE_NO_BODY;
          o->slots[at_slot] = w;
          if (nh) memcpy(o->hdrs + at_hdr, b->hdrs + (uint64_t) i * m, sizeof(rhp_hdr_t) * nh);
          if (body && x.body_len) memcpy(o->body + at_body, bytes + from, x.body_len);
        }
        at_slot++;
        at_hdr += nh;
        if (body) at_body += x.body_len;
      }
    }
    if (pass) break;
    tot.n_wide = (uint32_t) (at_slot < 0xffffffffull ? at_slot : 0xffffffffull);
    tot.n_hdrs = (uint32_t) (at_hdr < 0xffffffffull ? at_hdr : 0xffffffffull);
    tot.body_bytes = at_body;
    *o->totals = tot;
    /* (sessions that overlap, against the contract, may count a slot twice: the saturated counts fit no area) */
    if (at_slot > o->cap_slots || at_hdr > o->cap_hdrs || at_body > o->cap_body) break;   /* totals only */
  }
  return 0;
}

/* rhp_split_sessions (rhp.h) on the host, every pointer in host memory: a plain
 * walk over each session's bytes with the cut rule as rhp.h words it, twice --
 * the count first, then, when the pieces fit cap_pieces, the offsets and the
 * sessions in the same order, and the tail.  It shares the argument check with
 * the kernels' launcher (rhp_split_args.h) and nothing else. */
extern "C" int rhp_cpu_split_sessions(const uint8_t *bytes, uint64_t bytes_end, const uint64_t *sess_off, uint32_t n_sessions,
                                      const rhp_split_out_t *o)
{
  const int rc = rhp_split_sessions_check(bytes, bytes_end, sess_off, n_sessions, o);
  if (rc < 0) return rc;
  for (int pass = 0; pass < 2; pass++) {
    uint64_t k = 0;
    for (uint32_t s = 0; s < n_sessions; s++) {
      const uint64_t a = sess_off[s], e = sess_off[s + 1u] < bytes_end ? sess_off[s + 1u] : bytes_end;
      if (pass) {
        o->sessions[s].piece_lo = (uint32_t) k;
        o->offsets[k] = a;
      }
      k++;
      for (uint64_t p = a + 2u; p < e; p++) {
        if (bytes[p - 1u] != RHP_SPLIT_LF) continue;
        if (bytes[p - 2u] == RHP_SPLIT_LF || (p - a >= 3u && bytes[p - 2u] == RHP_SPLIT_CR && bytes[p - 3u] == RHP_SPLIT_LF)) {
          if (pass) o->offsets[k] = p;
          k++;
        }
      }
      if (pass) o->sessions[s].piece_hi = (uint32_t) k;
    }
    if (pass) {
      for (; k <= o->cap_pieces; k++) o->offsets[k] = sess_off[n_sessions];
      break;
    }
    *o->n_pieces = k;
    if (k > o->cap_pieces) break;   /* *n_pieces only */
  }
  return 0;
}

/* rhp_parse_messages (rhp.h) on the host, every pointer in host memory: the
 * kernel's templates (rhp_scalar.h) over PlainBytes, message by message.  It
 * shares the argument check with the launcher (rhp_msg_args.h).  As the
 * reference, it may read the bytes after a message (rhp.h). */
extern "C" int rhp_cpu_parse_messages(const rhp_msg_batch_t *b)
{
  const int rc = rhp_msg_batch_check(b, 0);
  if (rc != 0) return rc < 0 ? rc : 0;
  const bool hmajor = b->layout == RHP_LAYOUT_HEADER_MAJOR;
  const uint64_t hs_req = hmajor ? 1u : b->max_headers, hs_hdr = hmajor ? b->n : 1u;
  for (uint32_t i = 0; i < b->n; i++) {
    const uint64_t off = b->offsets[i], len = b->offsets[i + 1] - off;
    const uint64_t ll = b->last_len ? b->last_len[i] : 0;
    PlainBytes B{b->bytes + off};
    OutMsg<PlainMsgStore> out{{b->msgs + i, b->hdrs ? b->hdrs + i * hs_req : nullptr, hs_hdr}};
    if (b->kind == RHP_MSG_RESPONSE) scalar_message_t<RHP_MSG_RESPONSE>(B, len, ll, b->max_headers, out);
    else scalar_message_t<RHP_MSG_HEADERS>(B, len, ll, b->max_headers, out);
  }
  return 0;
}

/* rhp_frame_messages (rhp.h) on the host, every pointer in host memory: per
 * ready message the framing statement of rhp_scalar.h (frame_of_records_t) over
 * a view of its records that hides what the kernel skips -- an obs-fold line, a
 * record whose name or value does not lie inside [0, ret) -- and classify_one,
 * the lookup both classify twins run, for the caller's names.  It shares the
 * argument check with the launcher (rhp_frame_args.h). */
namespace {

/* HdrsRec (rhp_scalar.h) over records at any stride, inside [0, ret) */
struct FrameHdrs {
  const uint8_t *b;
  const rhp_hdr_t *h;
  uint64_t hs, ret;
  const rhp_hdr_t &at(uint32_t i) const { return h[i * hs]; }
  bool null(uint32_t i) const
  {
    const rhp_hdr_t &r = at(i);
    return r.name_off == RHP_NAME_NULL || (uint64_t) r.name_off + r.name_len > ret || (uint64_t) r.value_off + r.value_len > ret;
  }
  const uint8_t *name(uint32_t i) const { return b + at(i).name_off; }
  uint64_t name_len(uint32_t i) const { return at(i).name_len; }
  const uint8_t *value(uint32_t i) const { return b + at(i).value_off; }
  uint64_t value_len(uint32_t i) const { return at(i).value_len; }
};

}  // namespace

extern "C" int rhp_cpu_frame_messages(const rhp_msg_batch_t *b, const rhp_frame_args_t *f)
{
  const int rc = rhp_frame_check(b, f, 0);
  if (rc != 0) return rc < 0 ? rc : 0;
  const uint32_t n = b->n, m = b->max_headers;
  const bool hmajor = b->layout == RHP_LAYOUT_HEADER_MAJOR;
  const uint64_t hs_req = hmajor ? 1u : m, hs_hdr = hmajor ? n : 1u, readable = rhp_frame_readable(b);
  const rhp_classify_t c = {f->text, f->names, nullptr, f->n_names, 0, f->fields, nullptr};
  for (uint32_t i = 0; i < n; i++) {
    const int32_t ret = b->msgs[i].ret;
    rhp_frame_t x = {http_result_of(ret), RHP_FRAME_NONE, 0};   /* (a ret > 0 that is not ready: 0) */
    classify_absent(&c, n, i);
    if (ret > 0 && b->offsets[i] <= readable && (uint64_t) ret <= readable - b->offsets[i]) {
      const uint8_t *msg = b->bytes + b->offsets[i];
      const rhp_hdr_t *h = b->hdrs ? b->hdrs + i * hs_req : nullptr;   /* (max_headers 0) */
      const uint32_t nh = b->msgs[i].num_headers < m ? b->msgs[i].num_headers : m;
      x.result = frame_of_records_t(FrameHdrs{msg, h, hs_hdr, (uint64_t) ret}, nh, &x.body_kind, &x.body_len);
      rhp_req_t r = {};
      r.ret = ret;
      r.num_headers = (uint16_t) nh;
      classify_one(&c, n, m, i, msg, r, [&](uint32_t k) -> const rhp_hdr_t & { return h[k * hs_hdr]; });
      if (f->decoders && x.body_kind == RHP_FRAME_CHUNKED) {
        rhp_chunked_t d = {};
        d.consume_trailer = (uint8_t) f->consume_trailer;
        f->decoders[i] = d;
      }
    }
    f->frames[i] = x;
  }
  return 0;
}

/* rhp_decode_chunked (rhp.h) on the host, every pointer in host memory: the
 * scalar statement (rhp_scalar.h decode_chunked_t) over PlainBytes and the
 * byte-wise forward move, stream by stream, with the launcher's argument check
 * (rhp_chunked_args.h) and the kernel's clamp of a piece's ends. */
namespace {

int64_t decode_chunked_piece(rhp_chunked_t *d, uint8_t *buf, uint64_t len, uint64_t *size)
{
  if (RHP_CHUNKED_CORRUPT(d->state, d->hex_count)) {
    *size = 0;
    return kBad;
  }
  PlainBytes B{buf};
  PlainMove M{buf};
  uint64_t left = d->bytes_left_in_chunk;
  uint32_t hex = d->hex_count, st = d->state;
  const int64_t ret = decode_chunked_t(B, M, len, d->consume_trailer != 0, left, hex, st, size);
  d->bytes_left_in_chunk = left;
  d->hex_count = (uint8_t) hex;
  d->state = (uint8_t) st;
  return ret;
}

}  // namespace

extern "C" int rhp_cpu_decode_chunked(const rhp_chunked_batch_t *b)
{
  const int rc = rhp_chunked_batch_check(b, 0);
  if (rc != 0) return rc < 0 ? rc : 0;
  for (uint32_t i = 0; i < b->n; i++) {
    uint64_t off = b->offsets[i], end = b->offsets[i + 1];
    off = off < b->bytes_size ? off : b->bytes_size;
    end = end < off ? off : end < b->bytes_size ? end : b->bytes_size;
    uint64_t size = 0;
    const int64_t ret = decode_chunked_piece(&b->decoders[i], b->bytes + off, end - off, &size);
    b->results[i].ret = ret;
    b->results[i].size = size;
  }
  return 0;
}

extern "C" ssize_t rhp_phr_decode_chunked(rhp_chunked_t *decoder, char *buf, size_t *bufsz)
{
  uint64_t size = 0;
  const int64_t ret = decode_chunked_piece(decoder, (uint8_t *) buf, *bufsz, &size);
  *bufsz = (size_t) size;
  return (ssize_t) ret;
}

extern "C" int rhp_phr_decode_chunked_is_in_data(rhp_chunked_t *decoder)
{
  return decoder->state == RHP_CHUNKED_IN_CHUNK_DATA;   /* picohttpparser.c:638-641 */
}

/* rhp_walk_responses (rhp.h) on the host, every pointer in host memory: the
 * kernel's statement (rhp_scalar.h walk_session_t) session by session, with the
 * launcher's argument check and the kernel's two clamps (rhp_walk_args.h).  The
 * reader is bounded as the kernel's is: zeros from the readable end on. */
namespace {

struct BoundedPlainBytes {
  const uint8_t *bytes;
  uint64_t at, size;
  uint32_t operator()(uint64_t p) const { return at + p < size ? bytes[at + p] : 0u; }
};

struct HostWalkIO {
  const rhp_walk_batch_t *w;
  uint64_t lim;
  BoundedPlainBytes bytes(uint64_t at) const { return BoundedPlainBytes{w->bytes, at, lim}; }
  PlainMsgStore store(uint32_t slot) const
  {
    return PlainMsgStore{w->msgs + slot, w->hdrs ? w->hdrs + (uint64_t) slot * w->max_headers : nullptr, 1};
  }
  HdrsRec hdrs(uint32_t slot, uint64_t at) const
  {
    return HdrsRec{w->bytes + at, w->hdrs ? w->hdrs + (uint64_t) slot * w->max_headers : nullptr, 1};
  }
  PlainMove move(uint64_t at) const { return PlainMove{w->bytes_rw + at}; }
  void slot(uint32_t slot, const rhp_walk_slot_t &x) const { w->slots[slot] = x; }
};

}  // namespace

extern "C" int rhp_cpu_walk_responses(const rhp_walk_batch_t *w)
{
  const int rc = rhp_walk_check(w, 0);
  if (rc != 0) return rc < 0 ? rc : 0;
  HostWalkIO io{w, rhp_walk_readable(w->bytes_size)};
  for (uint32_t s = 0; s < w->n_sessions; s++) {
    uint64_t a = w->sess_off[s], e = w->sess_off[s + 1];
    a = a < io.lim ? a : io.lim;
    e = e < a ? a : e < io.lim ? e : io.lim;
    uint64_t lo = w->slot_off[s], hi = w->slot_off[s + 1];
    if (lo > hi || hi > w->n_slots_total) hi = lo = 0;   /* owns no slot */
    rhp_walk_result_t r;
    NobodyAsked nobody;
    walk_session_t(io, a, e, (uint32_t) lo, (uint32_t) hi, w->max_headers, w->flags, &r, nobody);
    w->results[s] = r;
  }
  return 0;
}

/* rhp_walk_resume (rhp.h) on the host: walk_resume_t over the same io, with
 * the launcher's argument check and the kernel's clamps */
extern "C" int rhp_cpu_walk_resume(const rhp_walk_batch_t *w, rhp_walk_state_t *states)
{
  const int rc = rhp_walk_resume_check(w, states, 0);
  if (rc != 0) return rc < 0 ? rc : 0;
  HostWalkIO io{w, rhp_walk_readable(w->bytes_size)};
  for (uint32_t s = 0; s < w->n_sessions; s++) {
    uint64_t a = w->sess_off[s], e = w->sess_off[s + 1];
    a = a < io.lim ? a : io.lim;
    e = e < a ? a : e < io.lim ? e : io.lim;
    uint64_t lo = w->slot_off[s], hi = w->slot_off[s + 1];
    if (lo > hi || hi > w->n_slots_total) hi = lo = 0;   /* owns no slot */
    rhp_walk_state_t st;
    memcpy(&st, &states[s], sizeof st);   /* (any alignment) */
    rhp_walk_result_t r;
    NobodyAsked nobody;
    if (walk_resume_t(io, a, e, (uint32_t) lo, (uint32_t) hi, w->max_headers, w->flags, &st, &r, nobody)) memcpy(&states[s], &st, sizeof st);
    w->results[s] = r;
  }
  return 0;
}

/* rhp_walk_answers (rhp.h) on the host: either walk above with the kernels'
 * policy (rhp_scalar.h Asked) over the session's queue, clamped as the kernels
 * clamp it (rhp_walk_args.h rhp_walk_queue), with the launcher's argument check */
extern "C" int rhp_cpu_walk_answers(const rhp_walk_batch_t *w, rhp_walk_state_t *states, const rhp_walk_asked_t *x)
{
  const int rc = rhp_walk_answers_check(w, states, x, 0);
  if (rc != 0) return rc < 0 ? rc : 0;
  HostWalkIO io{w, rhp_walk_readable(w->bytes_size)};
  for (uint32_t s = 0; s < w->n_sessions; s++) {
    uint64_t a = w->sess_off[s], e = w->sess_off[s + 1];
    a = a < io.lim ? a : io.lim;
    e = e < a ? a : e < io.lim ? e : io.lim;
    uint64_t lo = w->slot_off[s], hi = w->slot_off[s + 1];
    if (lo > hi || hi > w->n_slots_total) hi = lo = 0;   /* owns no slot */
    Asked ask = {x->head_bits, x->slot_req, 0, 0, 0, ~0u, 0};
    ask.nq = rhp_walk_queue(x->req_off[s], x->req_off[s + 1], x->n_req_total, &ask.q0);
    rhp_walk_result_t r;
    if (states) {
      rhp_walk_state_t st;
      memcpy(&st, &states[s], sizeof st);   /* (any alignment) */
      if (walk_resume_t(io, a, e, (uint32_t) lo, (uint32_t) hi, w->max_headers, w->flags, &st, &r, ask)) memcpy(&states[s], &st, sizeof st);
    } else {
      walk_session_t(io, a, e, (uint32_t) lo, (uint32_t) hi, w->max_headers, w->flags, &r, ask);
    }
    w->results[s] = r;
    x->answered[s] = ask.k;
  }
  return 0;
}

/* rhp_lookup_walked (rhp.h) on the host, every pointer in host memory: slot by
 * slot the kernel's own rules (rhp_lookup_args.h: the owner by the same
 * bisection, in use, head, inside) and then classify_one, the lookup every
 * classify twin and rhp_cpu_frame_messages run, from slots[i].start.  Every
 * slot is absent first.  It shares the argument check with the launcher. */
extern "C" int rhp_cpu_lookup_walked(const rhp_walk_batch_t *w, const rhp_walk_lookup_t *l)
{
  const int rc = rhp_lookup_walked_check(w, l, 0);
  if (rc != 0) return rc < 0 ? rc : 0;
  const uint32_t n = w->n_slots_total, m = w->max_headers;
  const uint64_t readable = rhp_lookup_readable(w->bytes_size);
  const rhp_classify_t c = {l->text, l->names, nullptr, l->n_names, 0, l->fields, nullptr};
  for (uint32_t i = 0; i < n; i++) {
    classify_absent(&c, n, i);
    const uint32_t above = rhp_lookup_sessions_upto(w->slot_off, w->n_sessions, i);
    if (!above) continue;
    const uint32_t s = above - 1u;
    if (!rhp_lookup_in_use(i, w->slot_off[s], w->slot_off[s + 1], w->results[s].n_slots, n)) continue;
    const int32_t ret = w->msgs[i].ret;
    const uint64_t st = w->slots[i].start;
    if (!rhp_lookup_is_head(w->slots[i].result, ret) || !rhp_lookup_inside(st, ret, w->sess_off[s], w->sess_off[s + 1], readable)) continue;
    rhp_req_t r = {};
    r.ret = ret;
    r.num_headers = w->msgs[i].num_headers;
    classify_one(&c, n, m, i, w->bytes + st, r, [&](uint32_t k) -> const rhp_hdr_t & { return w->hdrs[(size_t) i * m + k]; });
  }
  return 0;
}

/* rhp_relay_walked (rhp.h) on the host, every pointer in host memory: slot by
 * slot the rule of rhp_relay_args.h (the kernels' own: the owner by the same
 * bisection, the tests in rhp.h's order, the sizes), then, when everything
 * fits, every relayed slot's reply in http_write_response's push order, a byte
 * at a time.  It shares the argument check with the launcher. */
namespace {

struct RelayPlan {
  uint32_t why;
  uint64_t size, keep;      /* keep: bit k set: header record k is a field of the reply */
  uint32_t type_off, type_len;
};

bool relay_same_name(const uint8_t *s, uint32_t len, const uint8_t *name, uint32_t name_len)
{
  const auto upper = [](uint8_t x) { return x >= 'a' && x <= 'z' ? (uint8_t) (x - ('a' - 'A')) : x; };   /* C-locale toupper */
  if (len != name_len) return false;
  for (uint32_t q = 0; q < len; q++)
    if (upper(s[q]) != upper(name[q])) return false;
  return true;
}

RelayPlan relay_plan(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, uint32_t i, uint64_t head_readable, uint64_t readable)
{
  RelayPlan p = {RHP_RELAY_UNUSED, 0, 0, 0, 0};
  const uint32_t n = w->n_slots_total, m = w->max_headers;
  const uint32_t above = rhp_lookup_sessions_upto(w->slot_off, w->n_sessions, i);
  if (!above) return p;
  const uint32_t s = above - 1u;
  const uint64_t lo = w->slot_off[s];
  if (!rhp_lookup_in_use(i, lo, w->slot_off[s + 1], w->results[s].n_slots, n)) return p;
  const rhp_msg_t &g = w->msgs[i];
  const rhp_walk_slot_t &t = w->slots[i];
  const uint64_t e = w->sess_off[s + 1];
  p.why = rhp_relay_why_head(1, t.result, g.ret, t.start, w->sess_off[s], e, head_readable, g.status, (uint32_t) (i - lo),
                             w->results[s].n_slots, w->results[s].stop);
  if (p.why != RHP_RELAY_OK) return p;
  const uint8_t *head = w->bytes + t.start;
  const uint32_t nh = g.num_headers < m ? g.num_headers : m;
  bool fold = false, span_bad = g.msg_len > 0 && !rhp_relay_span_inside(g.msg_off, g.msg_len, g.ret), typed = false;
  uint64_t fields = 0;
  for (uint32_t k = 0; k < nh; k++) {
    const rhp_hdr_t &h = w->hdrs[(size_t) i * m + k];
    if (h.name_off == RHP_NAME_NULL) { fold = true; continue; }
    if (!rhp_relay_span_inside(h.name_off, h.name_len, g.ret) || !rhp_relay_span_inside(h.value_off, h.value_len, g.ret)) { span_bad = true; continue; }
    if (fold || span_bad) continue;
    const uint8_t *name = head + h.name_off;
    bool drop = false;
    if (relay_same_name(name, h.name_len, (const uint8_t *) RHP_RELAY_TYPE_NAME, sizeof RHP_RELAY_TYPE_NAME - 1)) {
      drop = true;
      if (!typed) { typed = true; p.type_off = h.value_off; p.type_len = h.value_len; }
    }
    drop = drop || relay_same_name(name, h.name_len, (const uint8_t *) RHP_RELAY_LENGTH_NAME, sizeof RHP_RELAY_LENGTH_NAME - 1) ||
           relay_same_name(name, h.name_len, (const uint8_t *) RHP_RELAY_TE_NAME, sizeof RHP_RELAY_TE_NAME - 1);
    for (uint32_t j = 0; j < r->n_names && !drop; j++) drop = relay_same_name(name, h.name_len, r->text + r->names[j].off, r->names[j].len);
    if (drop) continue;
    p.keep |= 1ull << k;
    fields += rhp_relay_size_field(h.name_len, h.value_len);
  }
  p.why = rhp_relay_why_body(fold, span_bad, t.body_kind, t.body_len, t.wire_len, w->flags, t.start, g.ret, e, readable);
  if (p.why == RHP_RELAY_OK) p.size = rhp_relay_size_head(g.msg_len, p.type_len, (uint32_t) t.body_len) + fields;
  return p;
}

/* http_write_response's pushes (http.c:236-284) for slot i at d; returns the end */
uint8_t *relay_write(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, uint32_t i, const RelayPlan &p, uint8_t *d)
{
  const rhp_msg_t &g = w->msgs[i];
  const rhp_walk_slot_t &t = w->slots[i];
  const uint8_t *head = w->bytes + t.start;
  const auto text = [&](const char *s) { const size_t l = strlen(s); memcpy(d, s, l); d += l; };
  const auto span = [&](const uint8_t *s, size_t l) { if (l) memcpy(d, s, l); d += l; };
  text("HTTP/1.1 ");
  *d++ = (uint8_t) ('0' + g.status / 100u % 10u); *d++ = (uint8_t) ('0' + g.status / 10u % 10u); *d++ = (uint8_t) ('0' + g.status % 10u);
  if (g.msg_len) { *d++ = ' '; span(head + g.msg_off, g.msg_len); }
  text("\r\nServer: *\r\nDate: ");
  span((const uint8_t *) r->date, RHP_DATE_LEN);
  text("\r\nContent-Type: ");
  span(head + p.type_off, p.type_len);
  text("\r\nContent-Length: ");
  const uint32_t v = (uint32_t) t.body_len, L = rhp_u32_len(v);
  for (uint32_t q = 0, x = v; q < L; q++, x /= 10u) d[L - 1u - q] = (uint8_t) ('0' + x % 10u);   /* http_u32_sprint */
  d += L;
  text("\r\n");
  const uint32_t m = w->max_headers, nh = g.num_headers < m ? g.num_headers : m;
  for (uint32_t k = 0; k < nh; k++) {
    if (!(p.keep >> k & 1u)) continue;
    const rhp_hdr_t &h = w->hdrs[(size_t) i * m + k];
    span(head + h.name_off, h.name_len); text(": "); span(head + h.value_off, h.value_len); text("\r\n");
  }
  text("\r\n");
  span(head + (uint32_t) g.ret, (size_t) t.body_len);
  return d;
}

}  // namespace

extern "C" int rhp_cpu_relay_walked(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r)
{
  const int rc = rhp_relay_check(w, r, 0);
  if (rc < 0) return rc;
  uint64_t zero = 0;
  memcpy(r->out_off, &zero, sizeof zero);   /* (any alignment) */
  if (rc != 0) return 0;
  const uint32_t n = w->n_slots_total;
  const uint64_t head_readable = rhp_lookup_readable(w->bytes_size), readable = rhp_relay_readable(w->bytes_size);
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    const RelayPlan p = relay_plan(w, r, i, head_readable, readable);
    total += p.size;
    memcpy((uint8_t *) r->why + 4u * (size_t) i, &p.why, 4);
    memcpy((uint8_t *) r->out_off + 8u * ((size_t) i + 1u), &total, 8);
  }
  if (total > r->out_size) return 0;
  uint8_t *d = r->out;
  for (uint32_t i = 0; i < n; i++) {
    const RelayPlan p = relay_plan(w, r, i, head_readable, readable);
    if (p.why == RHP_RELAY_OK) d = relay_write(w, r, i, p, d);
  }
  return 0;
}

/* rhp_forward_sessions (rhp.h) on the host, every pointer in host memory: slot
 * by slot the rule of rhp_forward_args.h (the kernels' own: the owner by
 * bisection over piece_lo, the tests in rhp.h's order, the sizes), then, when
 * everything fits, every forwarded slot's request in rhp.h's order, a byte at a
 * time.  It shares the argument check with the launcher. */
namespace {

struct ForwardPlan {
  uint32_t why;
  uint64_t size, keep;   /* keep: bit k set: header record k is written */
  bool     head;         /* the method is "HEAD" */
};

struct ForwardHost {
  const rhp_batch_t *b;
  const rhp_session_t *sessions;
  uint32_t n_sessions;
  const rhp_session_result_t *results;
  const uint64_t *req_start;
  const uint16_t *route;
  const rhp_forward_t *f;
  const uint8_t *bytes;
  uint64_t readable;
};

ForwardPlan forward_plan(const ForwardHost &a, uint32_t i)
{
  ForwardPlan p = {RHP_FORWARD_UNUSED, 0, 0, false};
  const rhp_batch_t *b = a.b;
  const uint32_t n = b->n, m = b->max_headers;
  uint32_t above = 0;   /* the sessions before it have piece_lo <= i */
  for (uint32_t hi = a.n_sessions; above < hi;) {
    const uint32_t mid = above + ((hi - above) >> 1);
    if (a.sessions[mid].piece_lo <= i) above = mid + 1u; else hi = mid;
  }
  if (!above) return p;
  const uint32_t lo = a.sessions[above - 1u].piece_lo, hi = a.sessions[above - 1u].piece_hi, ns = a.results[above - 1u].n_slots;
  if (!rhp_forward_in_use(i, lo, hi, ns, n)) return p;
  const rhp_req_t &r = b->reqs[i];
  const rhp_http_t &x = b->http[i];
  p.why = RHP_FORWARD_NOT_READY;
  if (x.result != 1 || r.ret <= 0) return p;
  const uint64_t rs = a.req_start[i], e = b->offsets[hi];
  p.why = RHP_FORWARD_OUTSIDE;
  if (!rhp_forward_inside(rs, r.ret, b->offsets[lo], e, a.readable)) return p;
  const uint32_t last = rhp_forward_last_slot(lo, ns, n);
  p.why = RHP_FORWARD_CLOSED;
  if (last < n && b->http[last].result == -1) return p;
  p.why = RHP_FORWARD_ROUTE;
  if (!rhp_forward_route(a.route[i], a.f->n_routes, a.f->forward_mask)) return p;
  const uint8_t *req = a.bytes + rs;
  const uint32_t nh = r.num_headers < m ? r.num_headers : m;
  bool fold = false, span_bad = !rhp_forward_span_inside(r.method_off, r.method_len, r.ret) || !rhp_forward_span_inside(r.path_off, r.path_len, r.ret);
  uint64_t fields = 0;
  for (uint32_t k = 0; k < nh; k++) {
    const rhp_hdr_t &h = RHP_HDR(b->hdrs, b->layout, n, m, i, k);
    if (h.name_off == RHP_NAME_NULL) { fold = true; continue; }
    if (!rhp_forward_span_inside(h.name_off, h.name_len, r.ret) || !rhp_forward_span_inside(h.value_off, h.value_len, r.ret)) { span_bad = true; continue; }
    if (fold || span_bad) continue;
    const uint8_t *name = req + h.name_off;
    bool drop = relay_same_name(name, h.name_len, (const uint8_t *) RHP_FORWARD_LENGTH_NAME, sizeof RHP_FORWARD_LENGTH_NAME - 1) ||
                relay_same_name(name, h.name_len, (const uint8_t *) RHP_FORWARD_TE_NAME, sizeof RHP_FORWARD_TE_NAME - 1);
    for (uint32_t j = 0; j < a.f->n_names && !drop; j++) drop = relay_same_name(name, h.name_len, a.f->text + a.f->names[j].off, a.f->names[j].len);
    if (drop) continue;
    p.keep |= 1ull << k;
    fields += rhp_forward_size_field(h.name_len, h.value_len);
  }
  p.why = rhp_forward_why_body(fold, span_bad, x.body_kind, x.body_len, rs, r.ret, e, a.readable);
  if (p.why != RHP_FORWARD_OK) return p;
  p.size = rhp_forward_size_head(r.method_len, r.path_len, x.body_kind, (uint32_t) x.body_len, a.f->extra_len) + fields;
  p.head = r.method_len == 4u && memcmp(req + r.method_off, "HEAD", 4) == 0;
  return p;
}

/* slot i's request at d; returns the end */
uint8_t *forward_write(const ForwardHost &a, uint32_t i, const ForwardPlan &p, uint8_t *d)
{
  const rhp_batch_t *b = a.b;
  const rhp_req_t &r = b->reqs[i];
  const rhp_http_t &x = b->http[i];
  const uint8_t *req = a.bytes + a.req_start[i];
  const auto text = [&](const char *s) { const size_t l = strlen(s); memcpy(d, s, l); d += l; };
  const auto span = [&](const uint8_t *s, size_t l) { if (l) memcpy(d, s, l); d += l; };
  span(req + r.method_off, r.method_len);
  text(" ");
  span(req + r.path_off, r.path_len);
  text(" HTTP/1.1\r\n");
  const uint32_t n = b->n, m = b->max_headers, nh = r.num_headers < m ? r.num_headers : m;
  for (uint32_t k = 0; k < nh; k++) {
    if (!(p.keep >> k & 1u)) continue;
    const rhp_hdr_t &h = RHP_HDR(b->hdrs, b->layout, n, m, i, k);
    span(req + h.name_off, h.name_len); text(": "); span(req + h.value_off, h.value_len); text("\r\n");
  }
  if (x.body_kind == 1u) {
    text("Content-Length: ");
    const uint32_t v = (uint32_t) x.body_len, L = rhp_u32_len(v);
    for (uint32_t q = 0, y = v; q < L; q++, y /= 10u) d[L - 1u - q] = (uint8_t) ('0' + y % 10u);
    d += L;
    text("\r\n");
  }
  span(a.f->extra, a.f->extra_len);
  text("\r\n");
  if (x.body_kind == 1u) span(req + (uint32_t) r.ret, (size_t) x.body_len);
  return d;
}

}  // namespace

extern "C" int rhp_cpu_forward_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                        const rhp_session_result_t *results, const uint64_t *req_start,
                                        const uint16_t *route, const rhp_forward_t *f)
{
  const int rc = rhp_forward_check(b, sessions, n_sessions, results, req_start, route, f, 0);
  if (rc < 0) return rc;
  const auto put32 = [](uint32_t *at, size_t k, uint32_t v) { memcpy((uint8_t *) at + 4u * k, &v, 4); };   /* (any alignment) */
  const auto put64 = [](uint64_t *at, size_t k, uint64_t v) { memcpy((uint8_t *) at + 8u * k, &v, 8); };
  put64(f->out_off, 0, 0);
  if (rc != 0) {
    for (uint32_t s = 0; s <= n_sessions; s++) put32(f->fwd_off, s, 0);
    return 0;
  }
  const uint32_t n = b->n;
  const ForwardHost a = {b, sessions, n_sessions, results, req_start, route, f, b->bytes_rw ? b->bytes_rw : b->bytes,
                         rhp_forward_readable(b->bytes_size)};
  std::vector<uint32_t> count((size_t) n + 1u);   /* the forwarded slots below i */
  uint64_t total = 0;
  uint32_t q = 0, word = 0;
  for (uint32_t i = 0; i < n; i++) {
    const ForwardPlan p = forward_plan(a, i);
    count[i] = q;
    total += p.size;
    put32(f->why, i, p.why);
    put64(f->out_off, (size_t) i + 1u, total);
    if (p.why != RHP_FORWARD_OK) continue;
    if (p.head) word |= 1u << (q & 31u);
    if ((++q & 31u) == 0) {
      put32(f->head_bits, (q >> 5) - 1u, word);
      word = 0;
    }
  }
  count[n] = q;
  if (q & 31u) put32(f->head_bits, q >> 5, word);
  for (uint32_t s = 0; s < n_sessions; s++) put32(f->fwd_off, s, count[sessions[s].piece_lo < n ? sessions[s].piece_lo : n]);
  put32(f->fwd_off, n_sessions, q);
  if (total > f->out_size) return 0;
  uint8_t *d = f->out;
  for (uint32_t i = 0; i < n; i++) {
    const ForwardPlan p = forward_plan(a, i);
    if (p.why == RHP_FORWARD_OK) d = forward_write(a, i, p, d);
  }
  return 0;
}

/* ---- the pointer-based host parser: phr_parse_request's own outputs ---- */

namespace {

/* rhp_scalar.h output policy writing phr_parse_request's outputs (pointers
 * into buf, size_t lengths): no length limit */
struct OutPhr {
  const uint8_t *base;
  const char **method;
  size_t *method_len;
  const char **path;
  size_t *path_len;
  int *minor_version;
  rhp_phr_header_t *h;
  size_t *num_headers;
  void begin()
  {
    *method = nullptr; *method_len = 0; *path = nullptr; *path_len = 0;   /* picohttpparser.c:390-395 */
    *minor_version = -1; *num_headers = 0;
  }
  int fail(int code) { return code; }
  void header(uint32_t n, bool fold, uint64_t name, uint64_t name_len, uint64_t vs, uint64_t vlen)
  {
    h[n].name = fold ? nullptr : (const char *) base + name;
    h[n].name_len = (size_t) name_len;
    h[n].value = (const char *) base + vs;
    h[n].value_len = (size_t) vlen;
  }
  int done(uint64_t p, const uint64_t (&tok)[2][2], int minor, uint32_t n)
  {
    *method = (const char *) base + tok[0][0];
    *method_len = (size_t) (tok[0][1] - tok[0][0]);
    *path = (const char *) base + tok[1][0];
    *path_len = (size_t) (tok[1][1] - tok[1][0]);
    *minor_version = minor;
    *num_headers = n;
    return (int) p;
  }
};

/* rhp_scalar.h header view over phr_header records */
struct HdrsPhr {
  const rhp_phr_header_t *h;
  bool null(uint32_t i) const { return h[i].name == nullptr; }
  const uint8_t *name(uint32_t i) const { return (const uint8_t *) h[i].name; }
  uint64_t name_len(uint32_t i) const { return h[i].name_len; }
  const uint8_t *value(uint32_t i) const { return (const uint8_t *) h[i].value; }
  uint64_t value_len(uint32_t i) const { return h[i].value_len; }
};

}  // namespace

extern "C" int rhp_phr_parse_request(const char *buf, size_t len, const char **method, size_t *method_len,
                                     const char **path, size_t *path_len, int *minor_version,
                                     rhp_phr_header_t *headers, size_t *num_headers, size_t last_len)
{
  const uint8_t *b = (const uint8_t *) buf;
  const size_t max = *num_headers;
  OutPhr o{b, method, method_len, path, path_len, minor_version, headers, num_headers};
  if (last_len != 0) {   /* picohttpparser.c:399-401 */
    o.begin();
    const int r = is_complete(b, len, last_len);
    if (r != 0) return r;
  }
  PlainBytes B{b};
  return scalar_phr_t(B, len, (uint32_t) (max < 0xffffffffu ? max : 0xffffffffu), o);
}

namespace {

/* rhp_scalar.h output policy writing phr_parse_response's / phr_parse_headers'
 * outputs (picohttpparser.c:461-465, 486); a NULL status: the header block's */
struct OutPhrMsg {
  const uint8_t *base;
  int *minor_version, *status;
  const char **msg;
  size_t *msg_len;
  rhp_phr_header_t *h;
  size_t *num_headers;
  void begin()
  {
    if (status) { *minor_version = -1; *status = 0; *msg = nullptr; *msg_len = 0; }
    *num_headers = 0;
  }
  int fail(int code) { return code; }
  void header(uint32_t n, bool fold, uint64_t name, uint64_t name_len, uint64_t vs, uint64_t vlen)
  {
    h[n].name = fold ? nullptr : (const char *) base + name;
    h[n].name_len = (size_t) name_len;
    h[n].value = (const char *) base + vs;
    h[n].value_len = (size_t) vlen;
  }
  int done(uint64_t p, int minor, uint32_t st, uint64_t m, uint64_t m_len, uint32_t n)
  {
    if (status) { *minor_version = minor; *status = (int) st; *msg = (const char *) base + m; *msg_len = (size_t) m_len; }
    *num_headers = n;
    return (int) p;
  }
};

template <uint32_t KIND>
int phr_message(OutPhrMsg &o, const char *buf, size_t len, size_t last_len)
{
  const size_t max = *o.num_headers;
  PlainBytes B{(const uint8_t *) buf};
  return scalar_message_t<KIND>(B, len, last_len, (uint32_t) (max < 0xffffffffu ? max : 0xffffffffu), o);
}

}  // namespace

extern "C" int rhp_phr_parse_response(const char *buf, size_t len, int *minor_version, int *status, const char **msg,
                                      size_t *msg_len, rhp_phr_header_t *headers, size_t *num_headers, size_t last_len)
{
  OutPhrMsg o{(const uint8_t *) buf, minor_version, status, msg, msg_len, headers, num_headers};
  return phr_message<RHP_MSG_RESPONSE>(o, buf, len, last_len);
}

extern "C" int rhp_phr_parse_headers(const char *buf, size_t len, rhp_phr_header_t *headers, size_t *num_headers,
                                     size_t last_len)
{
  OutPhrMsg o{(const uint8_t *) buf, nullptr, nullptr, nullptr, nullptr, headers, num_headers};
  return phr_message<RHP_MSG_HEADERS>(o, buf, len, last_len);
}

extern "C" int rhp_http_read_cpu(uint8_t *buf, size_t len, rhp_http_req_t *req, rhp_phr_header_t *fields,
                                 size_t *fields_count)
{
  if (len == 0) return 0;                               /* http.c:184-186 */
  const int n = rhp_phr_parse_request((const char *) buf, len, &req->method, &req->method_len, &req->target,
                                      &req->target_len, &req->minor_version, fields, fields_count, 0);
  if (n <= 0) return n == kBad ? -1 : 0;                /* http.c:194-195 */
  const bool get = req->method_len == 3 && memcmp(req->method, "GET", 3) == 0;
  rhp_http_t x;
  http_frame_t(buf, len, n, get, HdrsPhr{fields}, (uint32_t) *fields_count, &x);
  req->body = x.body_kind ? buf + n : nullptr;
  req->body_len = x.body_kind ? (size_t) x.body_len : 0;
  req->consumed = x.consumed;
  return x.result;
}
