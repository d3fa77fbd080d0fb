/*
 * forward_sessions_host_test.c -- rhp_cpu_forward_sessions (include/rhp_host.h)
 * under ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and
 * rhp_gen.c (the `forward-sessions-asan` rule of libreactorng_amd/csrc/Makefile
 * builds and runs it).
 *
 * A small hand-built round of sessions -- forwarded GETs, POSTs with a body, a
 * chunked POST, HEADs, requests for the device's and the host's routes and for
 * none, a session that ends on -1, a partial tail, a session without a piece --
 * is cut at its empty lines, parsed speculatively, fixed up and classified on
 * the host, then forwarded into buffers of exactly the documented sizes: `out`
 * first absent, then exactly out_off[n], then one byte short; head_bits first
 * at (n + 31) / 32 words, then at exactly (total + 31) / 32.  The records of the
 * slots no session owns hold 0xFF.  Every forwarded request must read back
 * through rhp_http_read_cpu with result 1, consumed == its size and the method
 * and target it was written from.  Then hand-built records, one per why code,
 * the sessions reversed, and the refusals.  Exits non-zero on the first
 * mismatch.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <strings.h>

#include "rhp.h"
#include "rhp_host.h"

static const char *ROUTES[][2] = {{"", "/up"}, {"", "/static"}, {"", "/host"}};
enum { N_ROUTES = 3, FORWARD_MASK = 0x1, M = 8, MAX_PIECES = 96 };

#define GET "GET /up HTTP/1.1\r\nHost: u\r\nConnection: keep-alive\r\n\r\n"
#define HEAD "HEAD /up HTTP/1.1\r\nHost: u\r\n\r\n"
#define POST "POST /up HTTP/1.1\r\ncontent-length: 6\r\nKeep-Alive: 5\r\n\r\nhe\n\nlo"
#define CHUNKED "POST /up HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n0\r\n\r\n"
#define STATIC "GET /static HTTP/1.1\r\nHost: s\r\n\r\n"
#define HOST "PUT /host HTTP/1.1\r\nHost: h\r\n\r\n"
static const char *SESSIONS[] = {
  GET POST HEAD STATIC GET,                                    /* 4 forwarded around a static one */
  GET GET "GET /up HTTP/1.1\r\nBad Header\r\n\r\n" GET,       /* ends on -1: CLOSED */
  "",
  CHUNKED HOST "GET /nowhere HTTP/1.1\r\nHost: n\r\n\r\n" HEAD,   /* 2 forwarded */
  POST POST GET "GET /up HTTP/1.1\r\nHost:",                 /* 3 forwarded, a partial tail */
};
enum { N_SESSIONS = sizeof SESSIONS / sizeof SESSIONS[0] };
static const uint32_t WANT_FWD[N_SESSIONS + 1] = {0, 4, 4, 4, 6, 9};
static const uint32_t WANT_HEAD_BITS = (1u << 2) | (1u << 5);
static const char EXTRA[] = "Via: 1.1 rhp\r\n";

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

typedef struct round {
  uint8_t *rw;
  uint64_t size;
  const uint64_t *off;
  uint32_t n;
  rhp_req_t *reqs;
  rhp_hdr_t *hdrs;
  rhp_http_t *http;
  uint64_t *starts;
  rhp_session_result_t *results;
  rhp_session_t *order;
  uint16_t *route;
  rhp_batch_t b;
} round_t;

static void *need(size_t n)
{
  void *p = malloc(n ? n : 1);
  if (!p) abort();
  return p;
}

/* parse, fix up and classify; every buffer at its exact size, 0xFF where nothing is written */
static int make_round(round_t *r, const uint8_t *bytes, uint64_t size, const uint64_t *off, uint32_t n, const rhp_session_t *ss,
                      uint32_t layout, int reversed)
{
  uint8_t text[64];
  rhp_route_t routes[N_ROUTES];
  uint32_t at = 0;
  for (int k = 0; k < N_ROUTES; k++)
    for (int q = 0; q < 2; q++) {
      const rhp_span_t s = {at, (uint32_t) strlen(ROUTES[k][q])};
      memcpy(text + at, ROUTES[k][q], s.len);
      at += s.len;
      if (q) routes[k].target = s; else routes[k].method = s;
    }
  r->size = size, r->off = off, r->n = n;
  r->rw = aligned_alloc(16, (size + 15u) & ~(uint64_t) 15u);
  if (!r->rw) abort();
  r->reqs = need(n * sizeof *r->reqs), r->hdrs = need((size_t) n * M * sizeof *r->hdrs), r->http = need(n * sizeof *r->http);
  r->starts = need(n * sizeof *r->starts), r->results = need(N_SESSIONS * sizeof *r->results);
  r->order = need(N_SESSIONS * sizeof *r->order), r->route = need(n * sizeof *r->route);
  memcpy(r->rw, bytes, size);
  memset(r->reqs, 0xFF, n * sizeof *r->reqs), memset(r->hdrs, 0xFF, (size_t) n * M * sizeof *r->hdrs), memset(r->http, 0xFF, n * sizeof *r->http);
  memset(r->starts, 0xFF, n * sizeof *r->starts), memset(r->results, 0xFF, N_SESSIONS * sizeof *r->results);
  for (int s = 0; s < N_SESSIONS; s++) r->order[s] = ss[reversed ? N_SESSIONS - 1 - s : s];
  const rhp_batch_t b = {.bytes = r->rw, .bytes_rw = r->rw, .offsets = off, .bytes_size = size, .n = n, .max_headers = M,
                         .mode = RHP_MODE_HTTP, .layout = layout, .reqs = r->reqs, .hdrs = r->hdrs, .http = r->http,
                         .flags = RHP_BATCH_SPECULATIVE};
  r->b = b;
  rhp_classify_t c = {.text = text, .routes = routes, .n_routes = N_ROUTES, .route = r->route};
  int rc = rhp_cpu_parse_batch(&r->b);
  if (rc == 0) rc = rhp_cpu_fixup_sessions(&r->b, r->order, N_SESSIONS, r->results, r->starts);
  if (rc == 0) rc = rhp_cpu_classify_sessions(&r->b, r->order, N_SESSIONS, r->results, r->starts, &c);
  /* the slots no session's walk wrote: poisoned again behind the speculative parse */
  for (uint32_t i = 0; i < n && rc == 0; i++) {
    int used = 0;
    for (int s = 0; s < N_SESSIONS; s++) used |= i >= r->order[s].piece_lo && i - r->order[s].piece_lo < r->results[s].n_slots;
    if (!used) {
      memset(&r->reqs[i], 0xFF, sizeof r->reqs[i]), memset(&r->http[i], 0xFF, sizeof r->http[i]), memset(&r->starts[i], 0xFF, 8);
      for (uint32_t k = 0; k < M; k++) memset(&RHP_HDR(r->hdrs, layout, n, M, i, k), 0xFF, sizeof(rhp_hdr_t));
    }
  }
  return rc;
}

static void free_round(round_t *r)
{
  free(r->rw), free(r->reqs), free(r->hdrs), free(r->http), free(r->starts), free(r->results), free(r->order), free(r->route);
}

typedef struct answer {
  uint64_t *out_off;
  uint32_t *why, *fwd_off, *head_bits;
  uint8_t *out;
  uint64_t out_size;
} answer_t;

/* one call; out_size bytes of out, bits_words words of head_bits, everything else at its documented size */
static int forward(round_t *r, answer_t *a, uint64_t out_size, uint32_t bits_words)
{
  static const char *NAMES[] = {"Connection", "Keep-Alive"};
  uint8_t text[32];
  rhp_span_t names[2];
  uint32_t at = 0;
  for (int j = 0; j < 2; j++) {
    names[j].off = at, names[j].len = (uint32_t) strlen(NAMES[j]);
    memcpy(text + at, NAMES[j], names[j].len);
    at += names[j].len;
  }
  const uint32_t n = r->n;
  a->out_off = need((n + 1) * sizeof *a->out_off), a->why = need(n * sizeof *a->why);
  a->fwd_off = need((N_SESSIONS + 1) * sizeof *a->fwd_off), a->head_bits = need(bits_words * sizeof *a->head_bits);
  a->out = need(out_size), a->out_size = out_size;
  uint64_t *work = need(RHP_FORWARD_WORK_WORDS(n, N_SESSIONS) * sizeof *work);
  memset(a->out, 0xC3, out_size ? out_size : 1);
  memset(a->head_bits, 0xC3, bits_words ? bits_words * 4u : 1);
  const rhp_forward_t f = {.n_routes = N_ROUTES, .forward_mask = FORWARD_MASK, .text = text, .names = names, .n_names = 2,
                           .extra_len = sizeof EXTRA - 1, .extra = (const uint8_t *) EXTRA, .out_off = a->out_off, .why = a->why,
                           .out = out_size ? a->out : NULL, .out_size = out_size, .fwd_off = a->fwd_off, .head_bits = a->head_bits,
                           .work = work};
  const int rc = rhp_cpu_forward_sessions(&r->b, r->order, N_SESSIONS, r->results, r->starts, r->route, &f);
  free(work);
  return rc;
}

static void free_answer(answer_t *a) { free(a->out_off), free(a->why), free(a->fwd_off), free(a->head_bits), free(a->out); }

/* every forwarded request reads back: result 1, consumed == size, the slot's method and target */
static int reads_back(const round_t *r, const answer_t *a)
{
  int bad = 0;
  for (uint32_t i = 0; i < r->n && !bad; i++) {
    const uint64_t at = a->out_off[i], len = a->out_off[i + 1] - at;
    if ((a->why[i] == RHP_FORWARD_OK) != (len != 0)) bad = 1;
    if (!len || bad) continue;
    uint8_t *copy = need(len);
    memcpy(copy, a->out + at, len);
    rhp_http_req_t q;
    rhp_phr_header_t h[M + 2];
    size_t nh = M + 2;
    const rhp_req_t *g = &r->reqs[i];
    const uint8_t *req = r->rw + r->starts[i];
    if (rhp_http_read_cpu(copy, len, &q, h, &nh) != 1 || q.consumed != len || q.method_len != g->method_len ||
        memcmp(q.method, req + g->method_off, g->method_len) != 0 || q.target_len != g->path_len ||
        memcmp(q.target, req + g->path_off, g->path_len) != 0 || nh < 1 || h[nh - 1].name_len != 3 || memcmp(h[nh - 1].name, "Via", 3) != 0)
      bad = 1;
    for (size_t k = 0; k < nh && !bad; k++)
      if ((h[k].name_len == 10 && strncasecmp(h[k].name, "Connection", 10) == 0) || (h[k].name_len == 17 && strncasecmp(h[k].name, "Transfer-Encoding", 17) == 0))
        bad = 1;
    if (bad) fprintf(stderr, "slot %u does not read back: %.*s\n", i, (int) len, (const char *) a->out + at);
    free(copy);
  }
  return bad;
}

static int run(const char *label, const uint8_t *bytes, uint64_t size, const uint64_t *off, uint32_t n, const rhp_session_t *ss, uint32_t layout)
{
  round_t r;
  int bad = make_round(&r, bytes, size, off, n, ss, layout, 0) != 0;
  answer_t sizes, exact, tight;
  bad |= forward(&r, &sizes, 0, (n + 31u) / 32u) != 0;
  const uint64_t total = sizes.out_off[n];
  const uint32_t fwd = sizes.fwd_off[N_SESSIONS];
  for (int s = 0; s <= N_SESSIONS; s++) bad |= sizes.fwd_off[s] != WANT_FWD[s];
  bad |= forward(&r, &exact, total, (fwd + 31u) / 32u) != 0;
  bad |= exact.out_off[n] != total || memcmp(exact.out_off, sizes.out_off, (n + 1) * 8u) != 0 || memcmp(exact.why, sizes.why, n * 4u) != 0;
  bad |= exact.head_bits[0] != WANT_HEAD_BITS;
  if (!bad) bad |= reads_back(&r, &exact);
  bad |= forward(&r, &tight, total - 1, (fwd + 31u) / 32u) != 0;
  for (uint64_t k = 0; k + 1 < total; k++) bad |= tight.out[k] != 0xC3;   /* one byte short: out stays as it was */
  bad |= tight.out_off[n] != total || tight.head_bits[0] != WANT_HEAD_BITS;
  printf("%s: %u slots, %u forwarded, %llu bytes: %s\n", label, n, fwd, (unsigned long long) total, bad ? "MISMATCH" : "ok");
  free_answer(&sizes), free_answer(&exact), free_answer(&tight), free_round(&r);
  return bad;
}

/* one record crafted per why code, in slot 1 of the first session (a POST with a body); the session's last slot for CLOSED */
static int crafted(const uint8_t *bytes, uint64_t size, const uint64_t *off, uint32_t n, const rhp_session_t *ss, uint32_t layout, int reversed)
{
  int bad = 0;
  for (uint32_t code = RHP_FORWARD_UNUSED; code <= RHP_FORWARD_BODY_OUTSIDE; code++) {
    round_t r;
    if (make_round(&r, bytes, size, off, n, ss, layout, reversed) != 0) return 1;
    const int s0 = reversed ? N_SESSIONS - 1 : 0;
    const uint32_t i = ss[0].piece_lo + 1u, last = ss[0].piece_lo + r.results[s0].n_slots - 1u;
    switch (code) {
    case RHP_FORWARD_UNUSED: r.results[s0].n_slots = 1; break;
    case RHP_FORWARD_NOT_READY: r.reqs[i].ret = RHP_RET_TOOLONG; break;
    case RHP_FORWARD_OUTSIDE: r.starts[i] = ~(uint64_t) 0 - 3u; break;
    case RHP_FORWARD_CLOSED: r.http[last].result = -1; break;
    case RHP_FORWARD_ROUTE: r.route[i] = N_ROUTES; break;
    case RHP_FORWARD_FOLD: RHP_HDR(r.hdrs, layout, n, M, i, 1).name_off = RHP_NAME_NULL; break;
    case RHP_FORWARD_SPAN: RHP_HDR(r.hdrs, layout, n, M, i, 0).value_len = 0xFFFFu; break;
    case RHP_FORWARD_BODY: r.http[i].body_kind = RHP_BODY_CHUNKED_PENDING; break;
    case RHP_FORWARD_LONG: r.http[i].body_len = (uint64_t) 1 << 32; break;
    default: r.http[i].body_len = 0xFFFFFFF0u; break;
    }
    answer_t a;
    bad |= forward(&r, &a, 0, (n + 31u) / 32u) != 0;
    const int ordered = !reversed;   /* out of order a slot may be UNUSED instead; the sanitizer is the check */
    if (ordered && a.why[i] != code) {
      fprintf(stderr, "crafted code %u: why %u\n", code, a.why[i]);
      bad = 1;
    }
    for (uint32_t k = 0; k < n; k++) bad |= a.why[k] > RHP_FORWARD_BODY_OUTSIDE || a.out_off[k + 1] < a.out_off[k];
    free_answer(&a), free_round(&r);
  }
  printf("crafted records, layout %u%s: %s\n", layout, reversed ? ", sessions reversed" : "", bad ? "MISMATCH" : "ok");
  return bad;
}

int main(void)
{
  uint64_t off[MAX_PIECES + 1];
  rhp_session_t ss[N_SESSIONS];
  uint32_t k = 0;
  uint64_t at = 0;
  for (int s = 0; s < N_SESSIONS; s++) {
    const size_t len = strlen(SESSIONS[s]);
    ss[s].piece_lo = k;
    if (len) k = split(SESSIONS[s], len, at, off, k);   /* (the empty session has no piece) */
    ss[s].piece_hi = k;
    at += len;
    if (k >= MAX_PIECES) return 2;
  }
  off[k] = at;
  const uint32_t n = k;
  const uint64_t size = at + RHP_PAD;
  uint8_t *bytes = calloc(size, 1);
  if (!bytes) abort();
  at = 0;
  for (int s = 0; s < N_SESSIONS; s++) {
    memcpy(bytes + at, SESSIONS[s], strlen(SESSIONS[s]));
    at += strlen(SESSIONS[s]);
  }
  int bad = 0;
  for (uint32_t layout = RHP_LAYOUT_REQUEST_MAJOR; layout <= RHP_LAYOUT_HEADER_MAJOR; layout++) {
    char label[64];
    snprintf(label, sizeof label, "layout %u", layout);
    bad |= run(label, bytes, size, off, n, ss, layout);
    bad |= crafted(bytes, size, off, n, ss, layout, 0);
    bad |= crafted(bytes, size, off, n, ss, layout, 1);
  }

  /* refused arguments read and write nothing; the empty calls write two things */
  uint64_t out_off[2] = {77, 77}, work[16];
  uint32_t why[1], fwd_off[2] = {77, 77}, bits[1] = {77};
  uint16_t rt[4] = {0};
  rhp_batch_t b = {.n = 4, .mode = RHP_MODE_HTTP, .flags = 0};
  rhp_forward_t f = {.n_routes = 1, .forward_mask = 1, .out_off = out_off, .why = why, .fwd_off = fwd_off, .head_bits = bits, .work = work};
  if (rhp_cpu_forward_sessions(&b, NULL, 0, NULL, NULL, rt, &f) != -22) bad = 1;   /* not a speculative batch */
  b.flags = RHP_BATCH_SPECULATIVE;
  if (rhp_cpu_forward_sessions(&b, NULL, 1, NULL, NULL, rt, &f) != -22) bad = 1;   /* sessions without their arrays */
  f.n_routes = 0;
  if (rhp_cpu_forward_sessions(&b, NULL, 0, NULL, NULL, rt, &f) != -22) bad = 1;
  f.n_routes = 1, f.extra = (const uint8_t *) "Via: x\r", f.extra_len = 7;
  if (rhp_cpu_forward_sessions(&b, NULL, 0, NULL, NULL, rt, &f) != -22) bad = 1;   /* extra does not end in CRLF */
  f.extra = NULL, f.extra_len = 0, f.head_bits = NULL;
  if (rhp_cpu_forward_sessions(&b, NULL, 0, NULL, NULL, rt, &f) != -22) bad = 1;
  f.head_bits = bits;
  if (out_off[0] != 77 || fwd_off[0] != 77 || bits[0] != 77) bad = 1;
  b.n = 0;
  if (rhp_cpu_forward_sessions(&b, NULL, 0, NULL, NULL, rt, &f) != 0 || out_off[0] != 0 || out_off[1] != 77 || fwd_off[0] != 0 ||
      fwd_off[1] != 77 || bits[0] != 77)
    bad = 1;
  free(bytes);
  printf("%s\n", bad ? "FAILED" : "all ok");
  return bad;
}
