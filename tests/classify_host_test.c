/*
 * classify_host_test.c -- rhp_cpu_classify_batch (include/rhp_host.h) under
 * ASan/UBSan: a stand-alone program over rhp_emu.cpp and rhp_gen.c (the
 * `classify-asan` rule of libreactorng_amd/csrc/Makefile builds and runs it).
 *
 * A hand-built batch and two fuzz batches are parsed by the DFA emulation in
 * every record layout; the classification of each must equal a plain loop per
 * request over the request-major records of the exact host parser: toupper
 * (C locale) byte by byte for the names, length and memcmp for the routes.
 * Exits non-zero on the first mismatch.
 */
#include <ctype.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rhp.h"
#include "rhp_gen.h"
#include "rhp_host.h"

static const char *NAMES[] = {"Content-Length", "transfer-encoding", "HOST", "Content-Lengt", "a^_`|", "A~_`|", "a^_@|",
                              "Via", "x"};
static const char *ROUTES[][2] = {{"GET", "/exact"}, {"", "/any"}, {"PUT", "/exact"}, {"GET", "/"}, {"GET", "/exact/long"}};
enum { N_NAMES = sizeof NAMES / sizeof NAMES[0], N_ROUTES = sizeof ROUTES / sizeof ROUTES[0] };

static const char *HAND[] = {
  "GET /exact HTTP/1.1\r\nhost: a\r\nA^_`|: caret\r\nVia:\r\n\r\n",
  "PUT /exact HTTP/1.1\r\nA~_`|: tilde\r\n folded\r\na^_`|: after\r\nHOST: one\r\nHost: two\r\n\r\n",
  "POST /exact HTTP/1.1\r\nContent-Lengt: 1\r\nContent-Length: 2\r\nX: y\r\n\r\nhi",
  "\r\nDELETE /any HTTP/1.1\r\nTransfer-Encoding: chunked\r\nx: \r\n\r\n0\r\n\r\n",
  "GET /exact/ HTTP/1.1\r\nHosu: u\r\n\r\n",
  "GET /exac HTTP/1.1\r\nHost : bad\r\n\r\n",
  "GET /exact HTTP/1.1\r\nHost: partial\r\n",
  "GET / HTTP/1.0\r\n\r\n",
};

static void *xcalloc(size_t n, size_t size)
{
  void *p = calloc(n ? n : 1, size);
  if (!p) abort();
  return p;
}

/* the straightforward loop: expected fields and route of request i */
static void expect(const uint8_t *req, const rhp_req_t *r, const rhp_hdr_t *h, int ready, rhp_fieldref_t *f, uint16_t *route)
{
  for (uint32_t j = 0; j < N_NAMES; j++) {
    const size_t len = strlen(NAMES[j]);
    f[j] = (rhp_fieldref_t) {RHP_NAME_NULL, 0};
    for (uint32_t k = 0; ready && k < r->num_headers; k++) {
      if (h[k].name_off == RHP_NAME_NULL || h[k].name_len != len) continue;
      size_t q = 0;
      while (q < len && toupper(req[h[k].name_off + q]) == toupper((unsigned char) NAMES[j][q])) q++;
      if (q == len) {
        f[j] = (rhp_fieldref_t) {h[k].value_off, h[k].value_len};
        break;
      }
    }
  }
  *route = RHP_ROUTE_NONE;
  for (uint32_t k = 0; ready && k < N_ROUTES; k++) {
    const size_t ml = strlen(ROUTES[k][0]), tl = strlen(ROUTES[k][1]);
    if (r->path_len == tl && memcmp(req + r->path_off, ROUTES[k][1], tl) == 0 &&
        (ml == 0 || (r->method_len == ml && memcmp(req + r->method_off, ROUTES[k][0], ml) == 0))) {
      *route = (uint16_t) k;
      break;
    }
  }
}

static int run(const char *label, const uint8_t *bytes, const uint64_t *off, uint32_t n, uint32_t m, uint32_t mode)
{
  /* the tables */
  uint8_t text[1024];
  rhp_span_t names[N_NAMES];
  rhp_route_t routes[N_ROUTES];
  uint32_t at = 0;
  for (uint32_t j = 0; j < N_NAMES; j++) {
    names[j] = (rhp_span_t) {at, (uint32_t) strlen(NAMES[j])};
    memcpy(text + at, NAMES[j], names[j].len);
    at += names[j].len;
  }
  for (uint32_t k = 0; k < N_ROUTES; k++)
    for (int q = 0; q < 2; q++) {
      rhp_span_t s = {at, (uint32_t) strlen(ROUTES[k][q])};
      memcpy(text + at, ROUTES[k][q], s.len);
      at += s.len;
      if (q) routes[k].target = s; else routes[k].method = s;
    }
  const uint64_t size = off[n] + RHP_PAD;

  /* expected: the exact parser's request-major records, the plain loop */
  rhp_fieldref_t *want_f = xcalloc((size_t) N_NAMES * n, sizeof *want_f);
  uint16_t *want_r = xcalloc(n, sizeof *want_r);
  {
    uint8_t *rw = xcalloc(size, 1);
    memcpy(rw, bytes, size);
    rhp_req_t *reqs = xcalloc(n, sizeof *reqs);
    rhp_hdr_t *hdrs = xcalloc((size_t) n * m, sizeof *hdrs);
    rhp_http_t *http = xcalloc(n, sizeof *http);
    rhp_batch_t b = {.bytes = rw, .bytes_rw = rw, .offsets = off, .bytes_size = size, .n = n, .max_headers = m, .mode = mode,
                     .layout = RHP_LAYOUT_REQUEST_MAJOR, .reqs = reqs, .hdrs = hdrs, .http = http};
    if (rhp_cpu_parse_batch(&b) != 0) return 1;
    for (uint32_t i = 0; i < n; i++) {
      rhp_fieldref_t f[N_NAMES];
      const int ready = reqs[i].ret > 0 && (mode == RHP_MODE_PHR || http[i].result == 1);
      expect(rw + off[i], &reqs[i], hdrs + (size_t) i * m, ready, f, &want_r[i]);
      for (uint32_t j = 0; j < N_NAMES; j++) want_f[(size_t) j * n + i] = f[j];
    }
    free(rw), free(reqs), free(hdrs), free(http);
  }

  int bad = 0;
  for (uint32_t layout = RHP_LAYOUT_REQUEST_MAJOR; layout <= RHP_LAYOUT_DENSE_RM && !bad; layout++) {
    if (layout == RHP_LAYOUT_DENSE_RM && mode == RHP_MODE_HTTP) continue;   /* refused by the parser */
    const int dense = layout == RHP_LAYOUT_DENSE || layout == RHP_LAYOUT_DENSE_RM;
    uint8_t *rw = xcalloc(size, 1);
    memcpy(rw, bytes, size);
    /* exact sizes, filled with 0xFF: the sanitizer sees a read past a buffer, the
     * comparison one of a record the parse did not write */
    const size_t reqs_size = dense ? RHP_DENSE_REQS_BYTES(n) : (size_t) n * sizeof(rhp_req_t);
    const size_t hdrs_size = layout == RHP_LAYOUT_COMPACT ? RHP_COMPACT_HDRS_BYTES(n, m)
                             : dense                      ? RHP_DENSE_HDRS_BYTES(n, m)
                                                          : (size_t) n * m * sizeof(rhp_hdr_t);
    const size_t http_size = layout == RHP_LAYOUT_COMPACT || layout == RHP_LAYOUT_DENSE ? RHP_COMPACT_HTTP_BYTES(n)
                                                                                         : (size_t) n * sizeof(rhp_http_t);
    void *reqs = malloc(reqs_size ? reqs_size : 1), *hdrs = malloc(hdrs_size ? hdrs_size : 1), *http = malloc(http_size ? http_size : 1);
    if (!reqs || !hdrs || !http) abort();
    memset(reqs, 0xFF, reqs_size), memset(hdrs, 0xFF, hdrs_size), memset(http, 0xFF, http_size);
    rhp_batch_t b = {.bytes = rw, .bytes_rw = rw, .offsets = off, .bytes_size = size, .n = n, .max_headers = m, .mode = mode,
                     .layout = layout, .reqs = reqs, .hdrs = hdrs, .http = http};
    rhp_fieldref_t *got_f = malloc((size_t) N_NAMES * (n ? n : 1) * sizeof *got_f);
    uint16_t *got_r = malloc((n ? n : 1) * sizeof *got_r);
    rhp_classify_t c = {.text = text, .names = names, .routes = routes, .n_names = N_NAMES, .n_routes = N_ROUTES,
                        .fields = got_f, .route = got_r};
    int rc = rhp_emu_parse_batch(&b, NULL);
    if (rc == 0) rc = rhp_cpu_classify_batch(&b, &c);
    if (rc != 0) {
      fprintf(stderr, "%s layout %u: rc %d\n", label, layout, rc);
      bad = 1;
    }
    for (uint32_t i = 0; i < n && !bad; i++) {
      for (uint32_t j = 0; j < N_NAMES && !bad; j++) {
        const rhp_fieldref_t g = got_f[(size_t) j * n + i], w = want_f[(size_t) j * n + i];
        if (g.value_off != w.value_off || g.value_len != w.value_len) {
          fprintf(stderr, "%s layout %u request %u name %s: got (%u, %u) want (%u, %u)\n", label, layout, i, NAMES[j],
                  g.value_off, g.value_len, w.value_off, w.value_len);
          bad = 1;
        }
      }
      if (!bad && got_r[i] != want_r[i]) {
        fprintf(stderr, "%s layout %u request %u: route %u want %u\n", label, layout, i, got_r[i], want_r[i]);
        bad = 1;
      }
    }
    free(rw), free(reqs), free(hdrs), free(http), free(got_f), free(got_r);
  }
  uint32_t present = 0, routed = 0;
  for (size_t q = 0; q < (size_t) N_NAMES * n; q++) present += want_f[q].value_off != RHP_NAME_NULL;
  for (uint32_t i = 0; i < n; i++) routed += want_r[i] != RHP_ROUTE_NONE;
  printf("%s: %u requests, max_headers %u, mode %u: %u fields present, %u routed: %s\n", label, n, m, mode, present, routed,
         bad ? "MISMATCH" : "ok");
  free(want_f), free(want_r);
  return bad;
}

int main(void)
{
  int bad = 0;
  {
    enum { N = sizeof HAND / sizeof HAND[0] };
    uint64_t off[N + 1] = {0};
    for (int i = 0; i < N; i++) off[i + 1] = off[i] + strlen(HAND[i]);
    uint8_t *bytes = xcalloc(off[N] + RHP_PAD + 16, 1);
    for (int i = 0; i < N; i++) memcpy(bytes + off[i], HAND[i], strlen(HAND[i]));
    bad |= run("hand phr", bytes, off, N, 8, RHP_MODE_PHR);
    bad |= run("hand http", bytes, off, N, 8, RHP_MODE_HTTP);
    free(bytes);
  }
  const int cfg[2] = {RHP_GEN_FUZZ, RHP_GEN_FUZZ_HTTP};
  for (int q = 0; q < 2; q++) {
    const uint32_t n = 3000;
    const uint64_t size = rhp_gen_size(cfg[q], 0, n, 77);
    uint8_t *bytes = xcalloc(size + RHP_PAD + 16, 1);
    uint64_t *off = xcalloc(n + 1, sizeof *off);
    if (rhp_gen_fill(cfg[q], 0, n, 77, bytes, off) != 0) return 2;
    bad |= run(q ? "fuzz http" : "fuzz phr", bytes, off, n, 16, q ? RHP_MODE_HTTP : RHP_MODE_PHR);
    free(bytes), free(off);
  }
  return bad;
}
