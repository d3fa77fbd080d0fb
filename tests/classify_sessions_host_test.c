/*
 * classify_sessions_host_test.c -- rhp_cpu_classify_sessions (include/rhp_host.h)
 * under ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and
 * rhp_gen.c (the `classify-sessions-asan` rule of libreactorng_amd/csrc/Makefile
 * builds and runs it).
 *
 * A small hand-built round of sessions -- a Content-Length body and a chunked
 * body that each hold a whole fake request, a malformed request in the middle
 * of a session with well-formed ones behind it, a session without a piece, a
 * partial tail -- is cut at its empty lines, parsed speculatively, fixed up
 * and classified, by the exact host parser and by the DFA emulation with the
 * fix-up's prefix twin, in both rhp_hdr_t layouts.  Before the classify every
 * record slot the fix-up did not use is overwritten with a lie: the records
 * and the start of its session's first request, which would classify as
 * present if they were read.  The answers must equal the plain loop over
 * rhp_http_read_cpu (the pointer-based parser) from the front of each session.
 * A second run hands the sessions over in reverse order: every answer must
 * then be the right one or absent.  Exits non-zero on the first mismatch.
 */
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rhp.h"
#include "rhp_host.h"

static const char *NAMES[] = {"Host", "connection", "Content-Length", "TRANSFER-ENCODING", "X-Absent"};
static const char *ROUTES[][2] = {{"GET", "/plaintext"}, {"", "/c"}, {"POST", "/cl"}, {"GET", "/inside-a-body"}};
enum { N_NAMES = sizeof NAMES / sizeof NAMES[0], N_ROUTES = sizeof ROUTES / sizeof ROUTES[0], M = 8, MAX_PIECES = 64 };

#define FAKE "GET /inside-a-body HTTP/1.1\r\nHost: fake\r\n\r\n"
#define PLAIN "GET /plaintext HTTP/1.1\r\nHost: tfb\r\nConnection: keep-alive\r\n\r\n"
/* (the Content-Length is the length of `line one CRLF CRLF FAKE LF LF tail`) */
#define CL_BODY "line one\r\n\r\n" FAKE "\n\ntail"
static const char *SESSIONS[] = {
  PLAIN "POST /cl HTTP/1.1\r\nhost: outer\r\nContent-Length: 61\r\n\r\n" CL_BODY
        "PUT /c HTTP/1.1\r\nhOST: b\r\n folded\r\nConnection:\r\nHost: second\r\n\r\n",
  PLAIN "GET /x HTTP/1.1\r\nBad Header\r\n\r\n" PLAIN PLAIN,
  "",
  "POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n31\r\nab\r\n\r\n" FAKE "\r\n0\r\n\r\n"
  "GET /plaintext HTTP/1.1\nHost: lf\n\n" "GET /last HTTP/1.1\r\nHost:",
  PLAIN,
};
enum { N_SESSIONS = sizeof SESSIONS / sizeof SESSIONS[0] };

static void *xcalloc(size_t n, size_t size)
{
  void *p = calloc(n ? n : 1, size);
  if (!p) abort();
  return p;
}

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

typedef struct {
  rhp_fieldref_t f[N_NAMES];
  uint16_t route;
} answer_t;

static void absent(answer_t *a)
{
  for (int j = 0; j < N_NAMES; j++) a->f[j] = (rhp_fieldref_t) {RHP_NAME_NULL, 0};
  a->route = RHP_ROUTE_NONE;
}

/* the plain loop: http_read_request from the front of each session, slot piece_lo + m */
static void expect(const uint8_t *bytes, uint64_t size, const uint64_t *off, const rhp_session_t *ss, answer_t *want, uint32_t n)
{
  uint8_t *rw = xcalloc(size, 1);
  memcpy(rw, bytes, size);
  for (uint32_t i = 0; i < n; i++) absent(&want[i]);
  for (uint32_t s = 0; s < N_SESSIONS; s++) {
    uint64_t pos = off[ss[s].piece_lo];
    const uint64_t end = off[ss[s].piece_hi];
    for (uint32_t slot = ss[s].piece_lo; pos < end && slot < ss[s].piece_hi; slot++) {
      rhp_http_req_t q;
      rhp_phr_header_t h[M];
      size_t nh = M;
      uint8_t *req = rw + pos;
      if (rhp_http_read_cpu(req, end - pos, &q, h, &nh) != 1) break;
      answer_t *a = &want[slot];
      for (int j = 0; j < N_NAMES; j++) {
        const size_t len = strlen(NAMES[j]);
        for (size_t k = 0; k < nh; k++) {
          if (!h[k].name || h[k].name_len != len) continue;
          size_t x = 0;
          while (x < len && toupper((unsigned char) h[k].name[x]) == toupper((unsigned char) NAMES[j][x])) x++;
          if (x == len) {
            a->f[j] = (rhp_fieldref_t) {(uint16_t) ((const uint8_t *) h[k].value - req), (uint16_t) h[k].value_len};
            break;
          }
        }
      }
      for (int r = 0; r < N_ROUTES; r++) {
        const size_t ml = strlen(ROUTES[r][0]), tl = strlen(ROUTES[r][1]);
        if (q.target_len == tl && memcmp(q.target, ROUTES[r][1], tl) == 0 &&
            (ml == 0 || (q.method_len == ml && memcmp(q.method, ROUTES[r][0], ml) == 0))) {
          a->route = (uint16_t) r;
          break;
        }
      }
      pos += q.consumed;
    }
  }
  free(rw);
}

static int run(const char *label, const uint8_t *bytes, uint64_t size, const uint64_t *off, uint32_t n, const rhp_session_t *ss,
               const answer_t *want, uint32_t layout, int emulate, int reversed)
{
  uint8_t text[256];
  rhp_span_t names[N_NAMES];
  rhp_route_t routes[N_ROUTES];
  uint32_t at = 0;
  for (int j = 0; j < N_NAMES; j++) {
    names[j] = (rhp_span_t) {at, (uint32_t) strlen(NAMES[j])};
    memcpy(text + at, NAMES[j], names[j].len);
    at += names[j].len;
  }
  for (int r = 0; r < N_ROUTES; r++)
    for (int q = 0; q < 2; q++) {
      const rhp_span_t s = {at, (uint32_t) strlen(ROUTES[r][q])};
      memcpy(text + at, ROUTES[r][q], s.len);
      at += s.len;
      if (q) routes[r].target = s; else routes[r].method = s;
    }

  /* exact sizes: the sanitizer sees a read past a buffer */
  uint8_t *rw = aligned_alloc(16, (size + 15u) & ~(uint64_t) 15u);
  rhp_req_t *reqs = malloc(n * sizeof *reqs);
  rhp_hdr_t *hdrs = malloc((size_t) n * M * sizeof *hdrs);
  rhp_http_t *http = malloc(n * sizeof *http);
  uint64_t *starts = malloc(n * sizeof *starts);
  rhp_session_result_t *results = malloc(N_SESSIONS * sizeof *results);
  rhp_session_t *order = malloc(N_SESSIONS * sizeof *order);
  rhp_fieldref_t *got_f = malloc((size_t) N_NAMES * n * sizeof *got_f);
  uint16_t *got_r = malloc(n * sizeof *got_r);
  uint8_t *used = xcalloc(n, 1);
  if (!rw || !reqs || !hdrs || !http || !starts || !results || !order || !got_f || !got_r) abort();
  memcpy(rw, bytes, size);
  memset(reqs, 0xFF, n * sizeof *reqs), memset(hdrs, 0xFF, (size_t) n * M * sizeof *hdrs), memset(http, 0xFF, n * sizeof *http);
  memset(starts, 0xFF, n * sizeof *starts), memset(results, 0xFF, N_SESSIONS * sizeof *results);
  memset(got_f, 0xA5, (size_t) N_NAMES * n * sizeof *got_f), memset(got_r, 0xA5, n * sizeof *got_r);
  for (int s = 0; s < N_SESSIONS; s++) order[s] = ss[reversed ? N_SESSIONS - 1 - s : s];

  rhp_batch_t b = {.bytes = rw, .bytes_rw = rw, .offsets = off, .bytes_size = size, .n = n, .max_headers = M,
                   .mode = RHP_MODE_HTTP, .layout = layout, .reqs = reqs, .hdrs = hdrs, .http = http,
                   .flags = RHP_BATCH_SPECULATIVE};
  rhp_classify_t c = {.text = text, .names = names, .routes = routes, .n_names = N_NAMES, .n_routes = N_ROUTES,
                      .fields = got_f, .route = got_r};
  int rc = emulate ? rhp_emu_parse_batch(&b, NULL) : rhp_cpu_parse_batch(&b);
  if (rc == 0)
    rc = emulate ? rhp_emu_fixup_sessions(&b, order, N_SESSIONS, results, starts)
                 : rhp_cpu_fixup_sessions(&b, order, N_SESSIONS, results, starts);
  /* the lie in every slot the fix-up did not use: its session's first request, where that one is ready */
  uint32_t lies = 0;
  for (int s = 0; s < N_SESSIONS && rc == 0; s++)
    for (uint32_t q = 0; q < results[s].n_slots; q++) used[order[s].piece_lo + q] = 1;
  for (int s = 0; s < N_SESSIONS && rc == 0; s++) {
    const uint32_t lo = order[s].piece_lo;
    if (results[s].n_slots == 0 || http[lo].result != 1) continue;
    for (uint32_t i = lo + 1; i < order[s].piece_hi; i++) {
      if (used[i]) continue;
      reqs[i] = reqs[lo];
      http[i] = http[lo];
      starts[i] = starts[lo];
      for (uint32_t k = 0; k < M; k++) RHP_HDR(hdrs, layout, n, M, i, k) = RHP_HDR(hdrs, layout, n, M, lo, k);
      lies++;
    }
  }
  if (rc == 0) rc = rhp_cpu_classify_sessions(&b, order, N_SESSIONS, results, starts, &c);
  int bad = rc != 0;
  if (bad) fprintf(stderr, "%s: rc %d\n", label, rc);
  uint32_t right = 0, present = 0;
  for (uint32_t i = 0; i < n && !bad; i++) {
    int same = got_r[i] == want[i].route, none = got_r[i] == RHP_ROUTE_NONE;
    for (int j = 0; j < N_NAMES; j++) {
      const rhp_fieldref_t g = got_f[(size_t) j * n + i], w = want[i].f[j];
      same = same && g.value_off == w.value_off && g.value_len == w.value_len;
      none = none && g.value_off == RHP_NAME_NULL && g.value_len == 0;
      present += w.value_off != RHP_NAME_NULL;
    }
    right += same;
    if (!(same || (reversed && none))) {
      fprintf(stderr, "%s slot %u: route %u want %u; Host (%u, %u) want (%u, %u)\n", label, i, got_r[i], want[i].route,
              got_f[i].value_off, got_f[i].value_len, want[i].f[0].value_off, want[i].f[0].value_len);
      bad = 1;
    }
  }
  if (!bad && lies < 4) {
    fprintf(stderr, "%s: only %u unused slots held a lie\n", label, lies);
    bad = 1;
  }
  printf("%s: %u slots, %u right, %u fields present, %u unused slots with a ready request's records: %s\n", label, n, right,
         present, lies, bad ? "MISMATCH" : "ok");
  free(rw), free(reqs), free(hdrs), free(http), free(starts), free(results), free(order), free(got_f), free(got_r), free(used);
  return bad;
}

int main(void)
{
  if (strlen(CL_BODY) != 61) return 2;
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
  uint8_t *bytes = xcalloc(size, 1);
  at = 0;
  for (int s = 0; s < N_SESSIONS; s++) {
    memcpy(bytes + at, SESSIONS[s], strlen(SESSIONS[s]));
    at += strlen(SESSIONS[s]);
  }
  answer_t *want = xcalloc(n, sizeof *want);
  expect(bytes, size, off, ss, want, n);
  uint32_t routed = 0;
  for (uint32_t i = 0; i < n; i++) routed += want[i].route != RHP_ROUTE_NONE;
  if (routed != 7) {   /* 3 + 1 + 0 + 2 + 1: every ready request of SESSIONS matches a route */
    fprintf(stderr, "the plain loop routed %u requests\n", routed);
    return 2;
  }
  int bad = 0;
  for (uint32_t layout = RHP_LAYOUT_REQUEST_MAJOR; layout <= RHP_LAYOUT_HEADER_MAJOR; layout++)
    for (int emulate = 0; emulate < 2; emulate++)
      for (int reversed = 0; reversed < 2; reversed++) {
        char label[96];
        snprintf(label, sizeof label, "layout %u %s%s", layout, emulate ? "dfa emulation, prefix twin" : "exact parser",
                 reversed ? ", sessions reversed" : "");
        bad |= run(label, bytes, size, off, n, ss, want, layout, emulate, reversed);
      }

  /* refused arguments read nothing */
  rhp_batch_t b = {.n = 4, .mode = RHP_MODE_HTTP, .flags = 0};
  const uint8_t t[1] = {'x'};
  const rhp_span_t nm = {0, 1};
  rhp_classify_t c = {.text = t, .names = &nm, .n_names = 1};
  if (rhp_cpu_classify_sessions(&b, NULL, 0, NULL, NULL, &c) != -22) bad = 1;
  b.flags = RHP_BATCH_SPECULATIVE;
  if (rhp_cpu_classify_sessions(&b, NULL, 1, NULL, NULL, &c) != -22) bad = 1;
  b.n = 0;
  if (rhp_cpu_classify_sessions(&b, NULL, 0, NULL, NULL, &c) != 0) bad = 1;
  free(bytes), free(want);
  printf("%s\n", bad ? "FAILED" : "all ok");
  return bad;
}
