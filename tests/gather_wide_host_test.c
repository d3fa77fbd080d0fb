/*
 * gather_wide_host_test.c -- rhp_cpu_gather_wide (include/rhp_host.h) under
 * ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and rhp_gen.c
 * (the `gather-wide-asan` rule of libreactorng_amd/csrc/Makefile builds and runs
 * it).
 *
 * A small hand-built round of sessions -- requests the dense copies cannot hold
 * (a leading CRLF, `Host:x`, chunked bodies) between dense ones, a malformed
 * request with wide requests before and behind it, a partial tail, a session
 * without a piece -- is cut at its empty lines, parsed speculatively, fixed up
 * and packed on the host; every slot no session owns is then filled with 0xEE
 * (garbage records that carry a wide mark) and packed again.  The gather runs
 * into buffers of exactly the documented sizes, each holding 0xFF first.  With
 * the sessions in order the answer is held to the batch's own records slot by
 * slot, and every gathered body to the plain loop over rhp_http_read_cpu from
 * the front of each session.  Further runs plant num_headers above max_headers
 * and a body length that runs past the session's input in an in-use wide slot
 * (no header record, no body), take each cap one short (exact totals, no byte
 * of any area written), and hand the sessions over in reverse order: then the
 * answers are held only to their bounds, and the sanitizer sees any access
 * outside a buffer.  Exits non-zero on the first mismatch.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rhp.h"
#include "rhp_host.h"

enum { M = 8, MAX_PIECES = 128 };

#define PLAIN "GET /plaintext HTTP/1.1\r\nHost: tfb\r\n\r\n"
#define CRLF "\r\nGET /crlf HTTP/1.1\r\nHost: a\r\nB: c\r\n\r\n"
#define NOSPACE "GET /nospace HTTP/1.1\r\nHost:x\r\n\r\n"
#define CHUNKED "POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n"
#define CHUNKED2 "POST /c2 HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n3\r\na\n\n\r\n0\r\n\r\n"
#define POSTCL "POST /cl HTTP/1.1\r\nContent-Length: 6\r\n\r\nhe\n\nlo"
#define BAD "GET /x HTTP/1.1\r\nBad Header\r\n\r\n"
static const char *SESSIONS[] = {
  PLAIN CRLF POSTCL CHUNKED PLAIN NOSPACE,
  NOSPACE CHUNKED2 BAD NOSPACE NOSPACE PLAIN,   /* ends on -1: the slots behind it are nobody's */
  "",
  CHUNKED CHUNKED2 CRLF "GET /last HTTP/1.1\r\nHost:",
  PLAIN PLAIN PLAIN,
};
enum { N_SESSIONS = sizeof SESSIONS / sizeof SESSIONS[0] };

/* a cut after every empty line (LF LF or LF CR LF) and at the end: the server's split */
static uint32_t split(const char *d, size_t n, uint64_t at, uint64_t *off, uint32_t k)
{
  size_t from = 0;
  for (size_t p = 0; p < n; p++) {
    if (d[p] != '\n') continue;
    size_t cut = 0;
    if (p + 1 < n && d[p + 1] == '\n') cut = p + 2;
    else if (p + 2 < n && d[p + 1] == '\r' && d[p + 2] == '\n') cut = p + 3;
    if (cut > from && cut < n) {
      off[k++] = at + from;
      from = cut;
    }
  }
  off[k++] = at + from;
  return k;
}

static void *xmalloc(size_t n)
{
  void *p = malloc(n ? n : 1);
  if (!p) abort();
  return p;
}

typedef struct round {
  rhp_batch_t b;
  rhp_session_t ss[N_SESSIONS];
  rhp_session_result_t sr[N_SESSIONS];
  uint64_t *start;
  rhp_req_dense_t *dreq;
  rhp_http_compact_t *hc;
  uint16_t *lens;
  uint8_t *in_use;
  uint8_t *pristine;   /* the input before any de-framing */
  uint64_t size;
} round_t;

static int is_marked(const round_t *R, uint32_t i)
{
  return (R->hc[i].flags & RHP_HTTP_WIDE) || (R->hc[i].result == 1 && (R->dreq[i].flags & RHP_DENSE_WIDE));
}

typedef struct areas {
  rhp_wide_totals_t tot;
  rhp_wide_slot_t *slots;
  rhp_hdr_t *hdrs;
  uint8_t *body;
  uint32_t cs, ch;
  uint64_t cb;
} areas_t;

/* one call into areas of exactly the caps' sizes, all 0xFF first */
static int gather(const round_t *R, const rhp_session_t *ss, const rhp_session_result_t *sr, uint32_t cs, uint32_t ch, uint64_t cb,
                  areas_t *A)
{
  uint64_t *work = xmalloc(8 * RHP_WIDE_WORK_WORDS(R->b.n));
  A->cs = cs, A->ch = ch, A->cb = cb;
  A->slots = xmalloc(sizeof(rhp_wide_slot_t) * cs);
  A->hdrs = xmalloc(sizeof(rhp_hdr_t) * ch);
  A->body = xmalloc(cb);
  memset(A->slots, 0xFF, sizeof(rhp_wide_slot_t) * cs);
  memset(A->hdrs, 0xFF, sizeof(rhp_hdr_t) * ch);
  memset(A->body, 0xFF, cb);
  memset(&A->tot, 0xFF, sizeof A->tot);
  const rhp_wide_out_t o = {&A->tot, cs ? A->slots : NULL, cs, ch ? A->hdrs : NULL, ch, cb ? A->body : NULL, cb, work};
  const int rc = rhp_cpu_gather_wide(&R->b, ss, N_SESSIONS, sr, R->start, R->dreq, R->hc, &o);
  free(work);
  return rc;
}

static void release(areas_t *A)
{
  free(A->slots);
  free(A->hdrs);
  free(A->body);
}

static int all_ff(const void *p, size_t n)
{
  for (size_t k = 0; k < n; k++)
    if (((const uint8_t *) p)[k] != 0xFF) return 0;
  return 1;
}

#define FAIL(...) do { printf("gather_wide_host_test: " __VA_ARGS__); printf("\n"); return 1; } while (0)

/* sessions in order: the areas against the batch's records and the plain loop's bodies */
static int check_in_order(const round_t *R, const areas_t *A, int planted_hdr_slot, int planted_body_slot)
{
  const uint32_t n = R->b.n;
  uint32_t want = 0, at = 0, hdr_at = 0;
  uint64_t body_at = 0;
  for (uint32_t i = 0; i < n; i++) want += R->in_use[i] && is_marked(R, i);
  if (A->tot.n_wide != want) FAIL("n_wide %u, want %u", A->tot.n_wide, want);
  for (uint32_t i = 0; i < n; i++) {
    if (!(R->in_use[i] && is_marked(R, i))) continue;
    const rhp_wide_slot_t *w = &A->slots[at++];
    if (w->slot != i) FAIL("slot %u at position %u, want %u", w->slot, at - 1, i);
    if (memcmp(&w->req, &R->b.reqs[i], sizeof w->req) || memcmp(&w->http, &R->b.http[i], sizeof w->http) || w->req_start != R->start[i])
      FAIL("slot %u: records differ from the batch's", i);
    uint32_t nh = w->http.result == 1 && w->req.ret > 0 ? w->req.num_headers : 0;
    if ((int) i == planted_hdr_slot) nh = 0;
    if (w->hdr_first != hdr_at) FAIL("slot %u: hdr_first %u, want %u", i, w->hdr_first, hdr_at);
    if (nh && memcmp(A->hdrs + hdr_at, R->b.hdrs + (size_t) i * M, sizeof(rhp_hdr_t) * nh)) FAIL("slot %u: header records", i);
    hdr_at += nh;
    /* the plain loop: the request from its start over a fresh copy of the input */
    const int chunked = w->http.result == 1 && w->http.body_kind == 1 && w->http.consumed != (uint64_t) w->req.ret + w->http.body_len;
    if (chunked && (int) i != planted_body_slot) {
      rhp_http_req_t q;
      rhp_phr_header_t h[M];
      size_t nf = M;
      uint8_t *rw = xmalloc(R->size);
      memcpy(rw, R->pristine, R->size);
      uint32_t s = 0;
      while (!(R->ss[s].piece_lo <= i && i < R->ss[s].piece_hi)) s++;
      const uint64_t end = R->b.offsets[R->ss[s].piece_hi];
      const int res = rhp_http_read_cpu(rw + w->req_start, end - w->req_start, &q, h, &nf);
      const int same = res == 1 && q.body && q.body_len == w->http.body_len && w->body_off == body_at &&
                       memcmp(A->body + body_at, q.body, q.body_len) == 0;
      free(rw);
      if (!same) FAIL("slot %u: the gathered body is not http_read_request's", i);
      body_at += w->http.body_len;
    } else if (w->body_off != RHP_WIDE_NO_BODY) {
      FAIL("slot %u: a body where there is none to gather", i);
    }
  }
  if (A->tot.n_hdrs != hdr_at || A->tot.body_bytes != body_at) FAIL("totals: %u header records, %llu body bytes", A->tot.n_hdrs, (unsigned long long) A->tot.body_bytes);
  return 0;
}

int main(void)
{
  round_t R;
  memset(&R, 0, sizeof R);
  uint64_t off[MAX_PIECES + 1], at = 0;
  uint32_t n = 0;
  for (uint32_t s = 0; s < N_SESSIONS; s++) {
    const size_t len = strlen(SESSIONS[s]);
    R.ss[s].piece_lo = n;
    if (len) n = split(SESSIONS[s], len, at, off, n);
    R.ss[s].piece_hi = n;
    at += len;
  }
  off[n] = at;
  R.size = at + RHP_PAD;
  uint8_t *bytes = xmalloc(R.size);
  memset(bytes, 0, R.size);
  at = 0;
  for (uint32_t s = 0; s < N_SESSIONS; s++) {
    memcpy(bytes + at, SESSIONS[s], strlen(SESSIONS[s]));
    at += strlen(SESSIONS[s]);
  }
  R.pristine = xmalloc(R.size);
  memcpy(R.pristine, bytes, R.size);
  rhp_req_t *reqs = xmalloc(sizeof(rhp_req_t) * n);
  rhp_hdr_t *hdrs = xmalloc(sizeof(rhp_hdr_t) * n * M);
  rhp_http_t *http = xmalloc(sizeof(rhp_http_t) * n);
  R.start = xmalloc(8 * n);
  R.dreq = xmalloc(sizeof(rhp_req_dense_t) * n);
  R.hc = xmalloc(sizeof(rhp_http_compact_t) * n);
  R.lens = xmalloc(2 * n * M);
  R.in_use = xmalloc(n);
  memset(reqs, 0, sizeof(rhp_req_t) * n);
  memset(hdrs, 0, sizeof(rhp_hdr_t) * n * M);
  memset(http, 0, sizeof(rhp_http_t) * n);
  memset(R.start, 0, 8 * n);
  memset(R.lens, 0, 2 * n * M);
  const rhp_batch_t b = {bytes, bytes, off, R.size, n, M, RHP_MODE_HTTP, RHP_LAYOUT_REQUEST_MAJOR, reqs, hdrs, http, NULL,
                         RHP_BATCH_SPECULATIVE, 0, NULL};
  R.b = b;
  if (rhp_cpu_parse_batch(&R.b) != 0 || rhp_cpu_fixup_sessions(&R.b, R.ss, N_SESSIONS, R.sr, R.start) != 0) FAIL("host parse");
  /* garbage records with a wide mark in every slot nobody owns */
  memset(R.in_use, 0, n);
  for (uint32_t s = 0; s < N_SESSIONS; s++)
    for (uint32_t q = 0; q < R.sr[s].n_slots; q++) R.in_use[R.ss[s].piece_lo + q] = 1;
  uint32_t unused = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (R.in_use[i]) continue;
    memset(&reqs[i], 0xEE, sizeof reqs[i]);
    memset(&http[i], 0xEE, sizeof http[i]);
    memset(hdrs + (size_t) i * M, 0xEE, sizeof(rhp_hdr_t) * M);
    R.start[i] = 0xEEEEEEEEEEEEEEEEull;
    unused++;
  }
  if (rhp_cpu_pack_dense(&R.b, R.dreq, R.hc, R.lens) != 0) FAIL("host pack");
  for (uint32_t i = 0; i < n; i++)
    if (!R.in_use[i] && !is_marked(&R, i)) FAIL("unused slot %u carries no wide mark", i);
  if (unused < 4) FAIL("only %u unused slots", unused);

  areas_t T, A;
  if (gather(&R, R.ss, R.sr, 0, 0, 0, &T) != 0) FAIL("totals-only call");
  release(&T);
  const uint32_t cs = T.tot.n_wide, ch = T.tot.n_hdrs;
  const uint64_t cb = T.tot.body_bytes;
  if (cs < 8 || ch < 8 || cb < 20) FAIL("the round holds too little: %u %u %llu", cs, ch, (unsigned long long) cb);

  /* in order, exact caps */
  if (gather(&R, R.ss, R.sr, cs, ch, cb, &A) != 0 || check_in_order(&R, &A, -1, -1)) FAIL("in order");
  int chunked_slot = -1, hdr_slot = -1;
  for (uint32_t k = 0; k < cs; k++) {
    if (A.slots[k].body_off != RHP_WIDE_NO_BODY && chunked_slot < 0) chunked_slot = (int) A.slots[k].slot;
    else if (A.slots[k].http.result == 1 && A.slots[k].req.num_headers && hdr_slot < 0) hdr_slot = (int) A.slots[k].slot;
  }
  release(&A);
  if (chunked_slot < 0 || hdr_slot < 0) FAIL("no slot to plant in");

  /* each cap one short: exact totals, nothing written */
  for (int k = 0; k < 3; k++) {
    if (gather(&R, R.ss, R.sr, cs - (k == 0), ch - (k == 1), cb - (k == 2), &A) != 0) FAIL("cap %d one short", k);
    if (A.tot.n_wide != cs || A.tot.n_hdrs != ch || A.tot.body_bytes != cb) FAIL("cap %d one short: totals", k);
    if (!all_ff(A.slots, sizeof(rhp_wide_slot_t) * A.cs) || !all_ff(A.hdrs, sizeof(rhp_hdr_t) * A.ch) || !all_ff(A.body, A.cb))
      FAIL("cap %d one short: an area was written", k);
    release(&A);
  }

  /* sessions reversed: bounds only */
  rhp_session_t rs[N_SESSIONS];
  rhp_session_result_t rr[N_SESSIONS];
  for (uint32_t s = 0; s < N_SESSIONS; s++) rs[s] = R.ss[N_SESSIONS - 1 - s], rr[s] = R.sr[N_SESSIONS - 1 - s];
  if (gather(&R, rs, rr, cs, ch, cb, &A) != 0 || A.tot.n_wide > n) FAIL("reversed");
  release(&A);
  if (gather(&R, rs, rr, cs - 1, ch, cb, &A) != 0) FAIL("reversed, one short");
  release(&A);

  /* num_headers above max_headers in an in-use wide slot: no header record of it */
  const rhp_req_t kept = reqs[hdr_slot];
  reqs[hdr_slot].num_headers = M + 1;
  if (gather(&R, R.ss, R.sr, cs, ch, cb, &A) != 0 || A.tot.n_hdrs != ch - kept.num_headers || check_in_order(&R, &A, hdr_slot, -1))
    FAIL("num_headers above max_headers");
  release(&A);
  reqs[hdr_slot] = kept;

  /* a body that runs past the session's input: not gathered */
  const rhp_http_t keptx = http[chunked_slot];
  http[chunked_slot].body_len = R.size;
  if (gather(&R, R.ss, R.sr, cs, ch, cb, &A) != 0 || A.tot.body_bytes != cb - keptx.body_len || check_in_order(&R, &A, -1, chunked_slot))
    FAIL("a body past the session's input");
  release(&A);
  http[chunked_slot].body_len = ~(uint64_t) 0 - 3;   /* (wraps the range's end) */
  if (gather(&R, R.ss, R.sr, cs, ch, cb, &A) != 0 || A.tot.body_bytes != cb - keptx.body_len) FAIL("a body length that wraps");
  release(&A);
  http[chunked_slot] = keptx;

  free(bytes), free(R.pristine), free(reqs), free(hdrs), free(http), free(R.start), free(R.dreq), free(R.hc), free(R.lens), free(R.in_use);
  printf("gather_wide_host_test OK: %u slots, %u wide, %u header records, %llu body bytes, %u unused slots with marks\n", n, cs, ch,
         (unsigned long long) cb, unused);
  return 0;
}
