/*
 * rhp_records.h -- the record layouts of rhp.h, stated once: which layout has
 * which records, where each area of a batch's buffers sits, how a dense
 * request, a compact http record and a 16-bit length pair are encoded, and
 * which batches rhp_parse_batch refuses.  C11, C++17 and HIP (host and device);
 * nothing here allocates or keeps state.
 *
 * Used by the launchers (rhp_kernel.hip, rhp_classify.hip through
 * rhp_classify_args.h), rhp_pack_dense_kernel, the host library (rhp_host.cpp),
 * the emulator (rhp_emu.cpp) and the reactor (reactor/batch.c).  Two decodes are
 * deliberately their own: rhp_dfa_kernel's stores (a shared helper moves its
 * register allocation) and the word-level decode of rhp_classify_kernel and
 * rhp_classify_sessions_kernel (the host classify, written over this header,
 * is what their tests compare them with).
 */
#ifndef RHP_RECORDS_H
#define RHP_RECORDS_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rhp.h"

#ifdef __HIPCC__
#define RHP_REC __host__ __device__ static inline
#else
#define RHP_REC static inline
#endif

/* ---- which layout has which records ---- */

RHP_REC int rhp_layout_dense(uint32_t layout) { return layout == RHP_LAYOUT_DENSE || layout == RHP_LAYOUT_DENSE_RM; }
/* header records as lengths (the running sum), the exact path's in a wide area */
RHP_REC int rhp_layout_lens(uint32_t layout) { return layout == RHP_LAYOUT_COMPACT || rhp_layout_dense(layout); }
/* http records as rhp_http_compact_t, the other ones in a wide area */
RHP_REC int rhp_layout_compact_http(uint32_t mode, uint32_t layout)
{
  return mode == RHP_MODE_HTTP && (layout == RHP_LAYOUT_COMPACT || layout == RHP_LAYOUT_DENSE);
}

/* ---- where a batch's records are ---- */

typedef struct rhp_view {
  rhp_req_dense_t *dreq;   /* the dense request records, NULL in any other layout */
  rhp_req_t *reqs;         /* the rhp_req_t records: the batch's, or a dense batch's wide area */
  /* the rhp_hdr_t records the exact path writes (a length layout: the wide
   * area, request-major): record k of request i is hdrs[i * hs_req + k * hs_hdr] */
  rhp_hdr_t *hdrs;
  uint64_t hs_req, hs_hdr;
  /* a length layout: header k of request i at index i * rec_req + k * rec_hdr of
   * lens (compact), or of lens16 and the overflow area ovf32 (dense); any other
   * layout: NULL, and rec_* are hs_* */
  uint32_t *lens;
  uint16_t *lens16;
  uint32_t *ovf32;
  uint64_t rec_req, rec_hdr;
  rhp_http_compact_t *hc;  /* the compact http records, NULL when the batch has none */
  rhp_http_t *http;        /* the rhp_http_t records: the batch's, or the wide area behind hc */
} rhp_view_t;

/* Address arithmetic only: nothing is read, so a caller that holds const
 * buffers reads through the view and writes nothing; a buffer the caller does
 * not have (NULL) stays NULL in every place. */
RHP_REC uint8_t *rhp_view_at(const void *p, size_t off) { return p ? (uint8_t *) p + off : NULL; }
RHP_REC rhp_view_t rhp_view(const void *reqs, const void *hdrs, const void *http, uint32_t n, uint32_t m, uint32_t mode,
                            uint32_t layout)
{
  const int dense = rhp_layout_dense(layout), compact = layout == RHP_LAYOUT_COMPACT, hmajor = layout == RHP_LAYOUT_HEADER_MAJOR;
  const int ch = rhp_layout_compact_http(mode, layout);
  rhp_view_t v;
  v.dreq = (rhp_req_dense_t *) (dense ? rhp_view_at(reqs, 0) : NULL);
  v.reqs = (rhp_req_t *) rhp_view_at(reqs, dense ? RHP_DENSE_REQ_WIDE_OFF(n) : 0);
  v.hdrs = (rhp_hdr_t *) rhp_view_at(hdrs, dense ? RHP_DENSE_WIDE_OFF(n, m) : compact ? RHP_COMPACT_WIDE_OFF(n, m) : 0);
  v.hs_req = hmajor ? 1u : m;
  v.hs_hdr = hmajor ? n : 1u;
  v.lens = (uint32_t *) (compact ? rhp_view_at(hdrs, 0) : NULL);
  v.lens16 = (uint16_t *) (dense ? rhp_view_at(hdrs, 0) : NULL);
  v.ovf32 = (uint32_t *) (dense ? rhp_view_at(hdrs, RHP_DENSE_OVF_OFF(n, m)) : NULL);
  /* the lengths: header-major, but for RHP_LAYOUT_DENSE_RM */
  v.rec_req = (dense || compact) && layout != RHP_LAYOUT_DENSE_RM ? 1u : v.hs_req;
  v.rec_hdr = (dense || compact) && layout != RHP_LAYOUT_DENSE_RM ? n : v.hs_hdr;
  v.hc = (rhp_http_compact_t *) (ch ? rhp_view_at(http, 0) : NULL);
  v.http = (rhp_http_t *) rhp_view_at(http, ch ? RHP_COMPACT_HTTP_WIDE_OFF(n) : 0);
  return v;
}

RHP_REC rhp_view_t rhp_batch_view(const rhp_batch_t *b)
{
  return rhp_view(b->reqs, b->hdrs, b->http, b->n, b->max_headers, b->mode, b->layout);
}

/* ---- the header lengths ---- */

/* name_len | value_len << 16: a compact record, a dense overflow record */
RHP_REC uint32_t rhp_len32(uint32_t nl, uint32_t vl) { return nl | vl << 16; }
RHP_REC int rhp_len16_fits(uint32_t nl, uint32_t vl) { return nl <= RHP_DENSE_NAME_MAX && vl <= RHP_DENSE_VALUE_MAX; }
/* name_len | value_len << 6 (a name of 63 is RHP_DENSE_OVERFLOW's: never a fitting pair's) */
RHP_REC uint16_t rhp_len16_pack(uint32_t nl, uint32_t vl) { return (uint16_t) (nl | vl << 6); }
RHP_REC uint32_t rhp_len16_unpack(uint32_t l) { return (l & 63u) | (l >> 6) << 16; }

/* header k of request i of a length layout, as rhp_len32 */
RHP_REC uint32_t rhp_view_len32(const rhp_view_t *v, uint64_t i, uint64_t k)
{
  const uint64_t at = i * v->rec_req + k * v->rec_hdr;
  if (v->lens) return v->lens[at];
  const uint32_t l = v->lens16[at];
  return l == RHP_DENSE_OVERFLOW ? v->ovf32[at] : rhp_len16_unpack(l);
}
RHP_REC void rhp_view_put_len(const rhp_view_t *v, uint64_t i, uint64_t k, uint32_t nl, uint32_t vl)
{
  const uint64_t at = i * v->rec_req + k * v->rec_hdr;
  if (v->lens) {
    v->lens[at] = rhp_len32(nl, vl);
  } else if (rhp_len16_fits(nl, vl)) {
    v->lens16[at] = rhp_len16_pack(nl, vl);
  } else {
    v->lens16[at] = RHP_DENSE_OVERFLOW;
    v->ovf32[at] = rhp_len32(nl, vl);
  }
}

/* The running sum: the first header line starts behind `SP "HTTP/1." digit
 * CRLF`, each next one behind `name ": " value CRLF`. */
RHP_REC uint32_t rhp_hdr_first(const rhp_req_t *r) { return (uint32_t) r->path_off + r->path_len + 11u; }
RHP_REC rhp_hdr_t rhp_hdr_next(uint32_t *at, uint32_t len32)
{
  const uint32_t nl = len32 & 0xffffu, vl = len32 >> 16;
  rhp_hdr_t h;
  h.name_off = (uint16_t) *at;
  h.name_len = (uint16_t) nl;
  h.value_off = (uint16_t) (*at + nl + 2u);
  h.value_len = (uint16_t) vl;
  *at += nl + vl + 4u;
  return h;
}

/* ---- dense request <-> rhp_req_t ---- */

RHP_REC rhp_req_dense_t rhp_req_dense_mark(uint32_t flag)   /* RHP_DENSE_WIDE, RHP_DENSE_BAD */
{
  rhp_req_dense_t d;
  memset(&d, 0, sizeof d);
  d.flags = (uint8_t) flag;
  return d;
}
/* whether the dense record holds r: the DFA's regular form (rhp.h) */
RHP_REC int rhp_req_dense_fits(const rhp_req_t *r)
{
  return r->ret > 0 && r->ret <= (int32_t) RHP_MAX_LEN && r->method_off == 0 && r->method_len <= 255u &&
         r->path_off == r->method_len + 1u && r->num_headers <= 255u;
}
RHP_REC rhp_req_dense_t rhp_req_dense_encode(const rhp_req_t *r)
{
  rhp_req_dense_t d;
  d.ret = (uint16_t) r->ret;
  d.path_len = r->path_len;
  d.method_len = (uint8_t) r->method_len;
  d.num_headers = (uint8_t) r->num_headers;
  d.minor_version = (uint8_t) r->minor_version;
  d.flags = 0;
  return d;
}
/* `wide` is the request's record in the wide area; a reader that does not hold
 * it passes NULL and gets a wide request as all zero (ret 0: no answer here) */
RHP_REC rhp_req_t rhp_req_dense_decode(rhp_req_dense_t d, const rhp_req_t *wide)
{
  rhp_req_t r;
  memset(&r, 0, sizeof r);
  if (d.flags & RHP_DENSE_WIDE) {
    if (wide) r = *wide;
  } else if (d.flags & RHP_DENSE_BAD) {
    r.ret = -1;
    r.minor_version = -1;
  } else {
    r.ret = d.ret;
    r.method_len = d.method_len;
    r.path_off = (uint16_t) (d.method_len + 1u);
    r.path_len = d.path_len;
    r.minor_version = (int8_t) d.minor_version;
    r.num_headers = d.num_headers;
  }
  return r;
}

/* ---- compact http <-> rhp_http_t ---- */

/* the consumed a compact record stands for, from its request's ret */
RHP_REC uint64_t rhp_http_consumed(int32_t ret, int32_t result, uint32_t body_kind, uint64_t body_len)
{
  return result == 1 ? (uint64_t) (uint32_t) ret + (body_kind == 1 ? body_len : 0u) : 0u;
}
/* whether the compact record holds x: its consumed follows, its body_len fits 32 bits */
RHP_REC int rhp_http_compact_fits(int32_t ret, const rhp_http_t *x)
{
  return x->consumed == rhp_http_consumed(ret, x->result, x->body_kind, x->body_len) && !(x->body_len >> 32);
}
RHP_REC rhp_http_compact_t rhp_http_compact_encode(const rhp_http_t *x, int wide)
{
  rhp_http_compact_t c;
  memset(&c, 0, sizeof c);
  if (wide) {
    c.flags = RHP_HTTP_WIDE;
  } else {
    c.result = (int8_t) x->result;
    c.body_kind = (uint8_t) x->body_kind;
    c.body_len = (uint32_t) x->body_len;
  }
  return c;
}
RHP_REC rhp_http_t rhp_http_compact_decode(rhp_http_compact_t c, int32_t ret, const rhp_http_t *wide)
{
  if (c.flags & RHP_HTTP_WIDE) return *wide;
  rhp_http_t x;
  x.result = c.result;
  x.body_kind = c.body_kind;
  x.body_len = c.body_len;
  x.consumed = rhp_http_consumed(ret, x.result, x.body_kind, x.body_len);
  return x;
}

/* ---- rhp_pack_dense (rhp.h), one record slot ----
 * From a request-major http batch's records of one slot (h: its m header
 * records): the compact http record into *hc, the dense request returned, the
 * length rows the request uses written to lens16[k * stride].  A slot of a
 * speculative batch may hold anything, so beyond the two fit tests above the
 * http record must be a final one (body_kind 0 or 1, ret > 0 with result 1)
 * and the header records must follow the running sum. */
RHP_REC rhp_req_dense_t rhp_pack_dense_one(const rhp_req_t *r, const rhp_http_t *x, const rhp_hdr_t *h, uint32_t m,
                                           uint16_t *lens16, uint64_t stride, rhp_http_compact_t *hc)
{
  const int hok = rhp_http_compact_fits(r->ret, x) && x->body_kind <= 1u && (x->result != 1 || r->ret > 0);
  *hc = rhp_http_compact_encode(x, !hok);
  /* the request: dense when the DFA's regular form holds it and the http
   * record is compact (a de-framed chunked body moves its request's bytes:
   * the wide records' offsets are the moved ones) */
  int reg = hok && x->result == 1 && rhp_req_dense_fits(r) && r->num_headers <= m;
  uint32_t at = rhp_hdr_first(r);
  const uint32_t nh = reg ? r->num_headers : 0u;
  for (uint32_t k = 0; k < nh; k++) {
    const rhp_hdr_t g = h[k];
    reg = reg && g.name_off == at && g.value_off == at + g.name_len + 2u && rhp_len16_fits(g.name_len, g.value_len);
    at += (uint32_t) g.name_len + g.value_len + 4u;
    lens16[k * stride] = rhp_len16_pack(g.name_len, g.value_len);
  }
  return reg ? rhp_req_dense_encode(r) : rhp_req_dense_mark(RHP_DENSE_WIDE);
}

/* ---- what rhp_parse_batch refuses ----
 * 0: parse the batch; 1: nothing to do (n == 0); -22: refused.  Every rule the
 * device launcher applies before it looks at the device; device_pointers adds
 * the launcher's own (bytes 16-byte aligned: windows and exact-path lines are
 * aligned loads), which host callers, who pass any memory, leave out. */
RHP_REC int rhp_batch_check(const rhp_batch_t *b, int device_pointers)
{
  if (!b) return -22;
  if (b->mode != RHP_MODE_PHR && b->mode != RHP_MODE_HTTP) return -22;
  if (b->layout > RHP_LAYOUT_DENSE_RM) return -22;
  if (b->flags & ~RHP_BATCH_SPECULATIVE) return -22;
  if (b->flags & RHP_BATCH_SPECULATIVE) {   /* pieces of pipelined http input, in rhp_hdr_t records */
    if (b->mode != RHP_MODE_HTTP || rhp_layout_lens(b->layout)) return -22;
  }
  if (b->layout == RHP_LAYOUT_DENSE_RM && b->mode != RHP_MODE_PHR) return -22;   /* dense http: header-major */
  if (b->max_headers > RHP_MAX_HEADERS) return -22;
  if ((uint64_t) b->n * b->max_headers > 0xffffffffull) return -22;   /* record indices are 32-bit */
  if (b->last_len && b->mode != RHP_MODE_PHR) return -22;   /* http_read_request passes last_len 0 */
  if (b->n == 0) return 1;
  if (!b->bytes || !b->offsets || !b->reqs) return -22;
  if (b->max_headers > 0 && !b->hdrs) return -22;
  if (b->mode == RHP_MODE_HTTP && (!b->http || !b->bytes_rw)) return -22;
  if (device_pointers && ((uintptr_t) b->bytes & 15u) != 0) return -22;
  return 0;
}

#endif
