/*
 * reply_sessions_host_test.c -- rhp_cpu_reply_sessions (include/rhp_host.h) under
 * ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and rhp_gen.c
 * (the `reply-sessions-asan` rule of libreactorng_amd/csrc/Makefile builds and
 * runs it).
 *
 * A small hand-built round of sessions -- static runs stopped by a request for
 * the host's route, by a request with no route, by a malformed request with
 * static requests before and behind it, by a partial tail and by the end of the
 * input; a session without a piece -- is cut at its empty lines, parsed
 * speculatively, fixed up and classified on the host, then answered into buffers
 * of exactly the documented sizes.  The answer must equal the plain loop over
 * rhp_http_read_cpu from the front of each session with the images appended in
 * request order.  Further runs plant route values at and above n_routes in the
 * middle of a run (it stops there, image_off is not indexed), hand the sessions
 * over in reverse order, and claim n_slots beyond piece_hi: then the answers are
 * held only to their bounds (count <= n_slots, the replies inside out[0, total),
 * total <= out_size), and the sanitizer sees any access outside a buffer.
 * Exits non-zero on the first mismatch.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rhp.h"
#include "rhp_host.h"

static const char *ROUTES[][2] = {{"GET", "/plaintext"}, {"", "/c"}, {"POST", "/cl"}, {"GET", "/big"}};
static const char *IMAGES[] = {"<reply to GET /plaintext>", "<the host's>", "", "<big:0123456789abcdef0123456789abcdef>"};
enum { N_ROUTES = 4, STATIC_MASK = 0xD, M = 8, MAX_PIECES = 96 };

#define PLAIN "GET /plaintext HTTP/1.1\r\nHost: tfb\r\n\r\n"
#define POSTCL "POST /cl HTTP/1.1\r\nContent-Length: 6\r\n\r\nhe\n\nlo"
#define BIG "GET /big HTTP/1.1\r\nHost: b\r\n\r\n"
static const char *SESSIONS[] = {
  PLAIN POSTCL BIG "PUT /c HTTP/1.1\r\nHost: h\r\n\r\n" PLAIN PLAIN,   /* 3 answered, the host's, 2 not answered */
  PLAIN PLAIN "GET /x HTTP/1.1\r\nBad Header\r\n\r\n" PLAIN,          /* ends on -1: nothing answered */
  "",
  BIG "GET /nowhere HTTP/1.1\r\nHost: n\r\n\r\n" PLAIN,                /* 1 answered, no route */
  POSTCL PLAIN "GET /last HTTP/1.1\r\nHost:",                         /* 2 answered, a partial tail */
  PLAIN PLAIN PLAIN PLAIN PLAIN,                                      /* 5 answered, the end of the input */
};
enum { N_SESSIONS = sizeof SESSIONS / sizeof SESSIONS[0] };
static const uint32_t WANT_COUNT[N_SESSIONS] = {3, 0, 0, 1, 2, 5};

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

static uint16_t route_of(const rhp_http_req_t *q)
{
  for (int r = 0; r < N_ROUTES; r++) {
    const size_t ml = strlen(ROUTES[r][0]), tl = strlen(ROUTES[r][1]);
    if (q->target_len == tl && memcmp(q->target, ROUTES[r][1], tl) == 0 &&
        (ml == 0 || (q->method_len == ml && memcmp(q->method, ROUTES[r][0], ml) == 0)))
      return (uint16_t) r;
  }
  return RHP_ROUTE_NONE;
}

/* the plain loop: the replies of every session's leading static requests; a session that stops on -1 drops its own */
static size_t expect(const uint8_t *bytes, uint64_t size, const uint64_t *off, const rhp_session_t *ss, char *out, uint32_t *count)
{
  uint8_t *rw = malloc(size);
  if (!rw) abort();
  memcpy(rw, bytes, size);
  size_t total = 0;
  for (uint32_t s = 0; s < N_SESSIONS; s++) {
    uint64_t pos = off[ss[s].piece_lo];
    const uint64_t end = off[ss[s].piece_hi];
    const size_t before = total;
    int open = 1, res = 0;
    count[s] = 0;
    while (pos < end) {
      rhp_http_req_t q;
      rhp_phr_header_t h[M];
      size_t nh = M;
      res = rhp_http_read_cpu(rw + pos, end - pos, &q, h, &nh);
      if (res != 1) break;
      const uint16_t r = route_of(&q);
      if (r == RHP_ROUTE_NONE || !((STATIC_MASK >> r) & 1)) open = 0;
      if (open) {
        memcpy(out + total, IMAGES[r], strlen(IMAGES[r]));
        total += strlen(IMAGES[r]);
        count[s]++;
      }
      pos += q.consumed;
    }
    if (res == -1) {
      total = before;
      count[s] = 0;
    }
  }
  free(rw);
  return total;
}

enum { EXACT = 0, BOUNDS = 1 };

static int run(const char *label, const uint8_t *bytes, uint64_t size, const uint64_t *off, uint32_t n, const rhp_session_t *ss,
               const char *want, size_t want_total, const uint32_t *want_count, uint32_t layout, int emulate, int reversed,
               int plant, int overclaim)
{
  uint8_t text[64];
  rhp_route_t routes[N_ROUTES];
  uint32_t at = 0;
  for (int r = 0; r < N_ROUTES; r++)
    for (int q = 0; q < 2; q++) {
      const rhp_span_t s = {at, (uint32_t) strlen(ROUTES[r][q])};
      memcpy(text + at, ROUTES[r][q], s.len);
      at += s.len;
      if (q) routes[r].target = s; else routes[r].method = s;
    }
  uint64_t image_off[N_ROUTES + 1] = {0};
  for (int r = 0; r < N_ROUTES; r++) image_off[r + 1] = image_off[r] + strlen(IMAGES[r]);
  uint8_t *images = malloc(image_off[N_ROUTES]);

  /* exact sizes: the sanitizer sees an access past a buffer */
  uint8_t *rw = aligned_alloc(16, (size + 15u) & ~(uint64_t) 15u);
  rhp_req_t *reqs = malloc(n * sizeof *reqs);
  rhp_hdr_t *hdrs = malloc((size_t) n * M * sizeof *hdrs);
  rhp_http_t *http = malloc(n * sizeof *http);
  uint64_t *starts = malloc(n * sizeof *starts);
  rhp_session_result_t *results = malloc(N_SESSIONS * sizeof *results);
  rhp_session_t *order = malloc(N_SESSIONS * sizeof *order);
  uint16_t *route = malloc(n * sizeof *route);
  rhp_session_reply_t *replies = malloc(N_SESSIONS * sizeof *replies);
  uint64_t *total = malloc(sizeof *total);
  uint64_t *work = malloc(RHP_REPLY_WORK_WORDS(n, N_SESSIONS) * sizeof *work);
  const uint64_t out_size = want_total;
  uint8_t *out = malloc(out_size ? out_size : 1);
  if (!images || !rw || !reqs || !hdrs || !http || !starts || !results || !order || !route || !replies || !total || !work || !out) abort();
  for (int r = 0; r < N_ROUTES; r++) memcpy(images + image_off[r], IMAGES[r], strlen(IMAGES[r]));
  memcpy(rw, bytes, size);
  memset(reqs, 0xFF, n * sizeof *reqs), memset(hdrs, 0xFF, (size_t) n * M * sizeof *hdrs), memset(http, 0xFF, n * sizeof *http);
  memset(starts, 0xFF, n * sizeof *starts), memset(results, 0xFF, N_SESSIONS * sizeof *results);
  memset(route, 0xA5, n * sizeof *route), memset(replies, 0xFF, N_SESSIONS * sizeof *replies);
  memset(total, 0xFF, sizeof *total), memset(out, 0xFF, out_size ? out_size : 1);
  for (int s = 0; s < N_SESSIONS; s++) order[s] = ss[reversed ? N_SESSIONS - 1 - s : s];

  rhp_batch_t b = {.bytes = rw, .bytes_rw = rw, .offsets = off, .bytes_size = size, .n = n, .max_headers = M,
                   .mode = RHP_MODE_HTTP, .layout = layout, .reqs = reqs, .hdrs = hdrs, .http = http,
                   .flags = RHP_BATCH_SPECULATIVE};
  rhp_classify_t c = {.text = text, .routes = routes, .n_routes = N_ROUTES, .route = route};
  rhp_reply_table_t t = {.images = images, .image_off = image_off, .n_routes = N_ROUTES, .static_mask = STATIC_MASK};
  rhp_reply_out_t o = {.replies = replies, .total = total, .out = out_size ? out : NULL, .out_size = out_size, .work = work};
  int rc = emulate ? rhp_emu_parse_batch(&b, NULL) : rhp_cpu_parse_batch(&b);
  if (rc == 0)
    rc = emulate ? rhp_emu_fixup_sessions(&b, order, N_SESSIONS, results, starts)
                 : rhp_cpu_fixup_sessions(&b, order, N_SESSIONS, results, starts);
  if (rc == 0) rc = rhp_cpu_classify_sessions(&b, order, N_SESSIONS, results, starts, &c);
  /* a route value at or above n_routes in the middle of the first session's run: the run stops at its second slot */
  static const uint16_t PLANTS[] = {0, N_ROUTES, 0xFFFE, RHP_ROUTE_NONE};
  if (plant && rc == 0) route[ss[0].piece_lo + 1] = PLANTS[plant];
  if (overclaim && rc == 0) results[reversed ? N_SESSIONS - 1 : 0].n_slots = n + 7;   /* beyond piece_hi, and beyond n */
  if (rc == 0) rc = rhp_cpu_reply_sessions(&b, order, N_SESSIONS, results, route, &t, &o);
  int bad = rc != 0;
  if (bad) fprintf(stderr, "%s: rc %d\n", label, rc);
  const int mode = reversed || overclaim ? BOUNDS : EXACT;
  uint32_t answered = 0;
  for (int s = 0; s < N_SESSIONS && !bad; s++) {
    const int ws = reversed ? N_SESSIONS - 1 - s : s;
    const rhp_session_reply_t r = replies[s];
    answered += r.count;
    if (r.reserved != 0 || r.count > results[s].n_slots || r.out_off > *total || r.out_len > *total - r.out_off) bad = 1;
    if (mode == EXACT) {
      uint32_t wc = want_count[ws];
      if (plant && ws == 0) wc = 1;
      if (r.count != wc) bad = 1;
    }
    if (overclaim && ws == 0 && r.count != 0) bad = 1;   /* a session whose fields do not hold answers nothing */
    if (bad) fprintf(stderr, "%s session %d: count %u off %llu len %llu of total %llu\n", label, s, r.count,
                     (unsigned long long) r.out_off, (unsigned long long) r.out_len, (unsigned long long) *total);
  }
  if (!bad && *total > out_size && mode == EXACT && !plant) bad = 1;
  if (!bad && mode == EXACT && !plant && (*total != want_total || memcmp(out, want, want_total) != 0)) {
    fprintf(stderr, "%s: total %llu want %zu, or the bytes differ\n", label, (unsigned long long) *total, want_total);
    bad = 1;
  }
  printf("%s: %u slots, %u requests answered, %llu bytes: %s\n", label, n, answered, (unsigned long long) *total, bad ? "MISMATCH" : "ok");
  free(images), free(rw), free(reqs), free(hdrs), free(http), free(starts), free(results), free(order), free(route);
  free(replies), free(total), free(work), free(out);
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
  char *want = calloc(4096, 1);
  if (!bytes || !want) abort();
  at = 0;
  for (int s = 0; s < N_SESSIONS; s++) {
    memcpy(bytes + at, SESSIONS[s], strlen(SESSIONS[s]));
    at += strlen(SESSIONS[s]);
  }
  uint32_t count[N_SESSIONS];
  const size_t want_total = expect(bytes, size, off, ss, want, count);
  for (int s = 0; s < N_SESSIONS; s++)
    if (count[s] != WANT_COUNT[s]) {
      fprintf(stderr, "the plain loop answers %u requests of session %d\n", count[s], s);
      return 2;
    }
  int bad = 0;
  for (uint32_t layout = RHP_LAYOUT_REQUEST_MAJOR; layout <= RHP_LAYOUT_HEADER_MAJOR; layout++)
    for (int emulate = 0; emulate < 2; emulate++)
      for (int reversed = 0; reversed < 2; reversed++)
        for (int overclaim = 0; overclaim < 2; overclaim++)
          for (int plant = 0; plant < (reversed || overclaim ? 1 : 4); plant++) {
            char label[128];
            snprintf(label, sizeof label, "layout %u %s%s%s plant %d", layout, emulate ? "dfa emulation, prefix twin" : "exact parser",
                     reversed ? ", sessions reversed" : "", overclaim ? ", n_slots beyond piece_hi" : "", plant);
            bad |= run(label, bytes, size, off, n, ss, want, want_total, count, layout, emulate, reversed, plant, overclaim);
          }

  /* refused arguments read and write nothing */
  rhp_batch_t b = {.n = 4, .mode = RHP_MODE_HTTP, .flags = 0};
  uint64_t io[2] = {0, 0}, tot = 77, w[16];
  uint16_t rt[4] = {0};
  rhp_session_reply_t rp;
  rhp_reply_table_t t = {.images = NULL, .image_off = io, .n_routes = 1, .static_mask = 1};
  rhp_reply_out_t o = {.replies = &rp, .total = &tot, .out = NULL, .out_size = 0, .work = w};
  if (rhp_cpu_reply_sessions(&b, NULL, 0, NULL, rt, &t, &o) != -22) bad = 1;   /* not a speculative batch */
  b.flags = RHP_BATCH_SPECULATIVE;
  if (rhp_cpu_reply_sessions(&b, NULL, 1, NULL, rt, &t, &o) != -22) bad = 1;   /* sessions without their arrays */
  t.n_routes = 0;
  if (rhp_cpu_reply_sessions(&b, NULL, 0, NULL, rt, &t, &o) != -22) bad = 1;
  t.n_routes = 1;
  b.n = 0;
  if (tot != 77) bad = 1;
  if (rhp_cpu_reply_sessions(&b, NULL, 0, NULL, rt, &t, &o) != 0 || tot != 0) bad = 1;   /* no session: *total = 0 */
  free(bytes), free(want);
  printf("%s\n", bad ? "FAILED" : "all ok");
  return bad;
}
