/*
 * reactor_record_test.c -- reactor_batch_record (reactor/batch.c) against the
 * records it was packed from and against rhp_expand_* (include/rhp_host.h),
 * under ASan/UBSan: a stand-alone program over the reactor and host parser
 * sources (the `record-asan` rule of libreactorng_amd/csrc/Makefile builds and
 * runs it; no GPU, no Python).
 *
 * The batch is tests/batches.py http_field_limits' at the ends of the u16
 * header record (names of 62 and 63, values of 1007 and 1008 bytes; per pair:
 * no body, a Content-Length body, the same two bytes short, a chunked POST, a
 * POST whose Content-Length stands before the long field) and a malformed
 * request (-1).  It is parsed request-major by the exact host parser and packed
 * by rhp_cpu_pack_dense.  Every slot read through reactor_batch_record must
 * give the http record it was packed from and, for result 1, the request and
 * header records field for field, the wide slots included; and the same
 * records must come out of rhp_expand_reqs / _records / _http over the packed
 * copies laid out as an RHP_LAYOUT_DENSE batch.  Exits non-zero on a mismatch.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "reactor.h"
#include "rhp.h"
#include "rhp_host.h"
#include "../libreactorng_amd/csrc/reactor/reactor_batch.h"

enum { M = REACTOR_BATCH_HEADERS, MAX_REQ = 4096 };

static uint8_t *bytes;
static uint64_t off[64];
static uint32_t n;
static size_t total;

static void add(const char *head, const char *field, const char *tail)
{
  const size_t a = strlen(head), b = strlen(field), c = strlen(tail);
  memcpy(bytes + total, head, a);
  memcpy(bytes + total + a, field, b);
  memcpy(bytes + total + a + b, tail, c);
  off[n++] = total;
  total += a + b + c;
}

static void *xcalloc(size_t k, size_t size)
{
  void *p = calloc(k ? k : 1, size);
  if (!p) abort();
  return p;
}

static int fails;
#define CHECK(cond, ...) do { if (!(cond)) { fails++; printf("slot %u: ", i); printf(__VA_ARGS__); printf("\n"); } } while (0)

static void same_req(uint32_t i, const char *what, const rhp_req_t *got, const rhp_req_t *want)
{
  CHECK(got->ret == want->ret && got->method_len == want->method_len && got->path_off == want->path_off &&
        got->path_len == want->path_len && got->method_off == want->method_off &&
        got->minor_version == want->minor_version && got->num_headers == want->num_headers,
        "%s: request differs (ret %d / %d, method_len %u / %u, path %u+%u / %u+%u, minor %d / %d, headers %u / %u)", what,
        got->ret, want->ret, got->method_len, want->method_len, got->path_off, got->path_len, want->path_off,
        want->path_len, got->minor_version, want->minor_version, got->num_headers, want->num_headers);
}

static void same_hdrs(uint32_t i, const char *what, const rhp_hdr_t *got, const rhp_hdr_t *want, uint32_t nh)
{
  for (uint32_t k = 0; k < nh; k++)
    CHECK(got[k].name_off == want[k].name_off && got[k].name_len == want[k].name_len &&
          got[k].value_off == want[k].value_off && got[k].value_len == want[k].value_len,
          "%s: header %u differs (%u+%u %u+%u / %u+%u %u+%u)", what, k, got[k].name_off, got[k].name_len, got[k].value_off,
          got[k].value_len, want[k].name_off, want[k].name_len, want[k].value_off, want[k].value_len);
}

static void same_http(uint32_t i, const char *what, const rhp_http_t *got, const rhp_http_t *want)
{
  CHECK(got->result == want->result, "%s: result %d / %d", what, got->result, want->result);
  if (want->result == 1)
    CHECK(got->body_kind == want->body_kind && got->consumed == want->consumed && got->body_len == want->body_len,
          "%s: http differs (kind %u / %u, consumed %llu / %llu, body_len %llu / %llu)", what, got->body_kind,
          want->body_kind, (unsigned long long) got->consumed, (unsigned long long) want->consumed,
          (unsigned long long) got->body_len, (unsigned long long) want->body_len);
}

int main(void)
{
  bytes = xcalloc(64 * MAX_REQ + RHP_PAD, 1);
  static const uint32_t names[] = {RHP_DENSE_NAME_MAX, RHP_DENSE_NAME_MAX + 1u};
  static const uint32_t values[] = {RHP_DENSE_VALUE_MAX, RHP_DENSE_VALUE_MAX + 1u};
  for (int a = 0; a < 2; a++)
    for (int b = 0; b < 2; b++) {
      char field[2048];
      memset(field, 'N', names[a]);
      memcpy(field + names[a], ": ", 2);
      memset(field + names[a] + 2, 'v', values[b]);
      strcpy(field + names[a] + 2 + values[b], "\r\n");
      add("GET /p HTTP/1.1\r\n", field, "\r\n");
      add("PUT /p HTTP/1.1\r\n", field, "Content-Length: 5\r\n\r\nhello");
      add("PUT /p HTTP/1.1\r\n", field, "Content-Length: 5\r\n\r\nhel");
      add("POST /p HTTP/1.1\r\n", field, "Transfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n3\r\nabc\r\n0\r\n\r\n");
      add("POST /p HTTP/1.1\r\nContent-Length: 5\r\n", field, "\r\nhello");
    }
  add("GET /x HTTP/1.1\r\n", "Host : bad\r\n", "\r\n");
  off[n] = total;

  rhp_req_t *reqs = xcalloc(n, sizeof *reqs);
  rhp_hdr_t *hdrs = xcalloc((size_t) n * M, sizeof *hdrs);
  rhp_http_t *http = xcalloc(n, sizeof *http);
  rhp_batch_t bt = {.bytes = bytes, .bytes_rw = bytes, .offsets = off, .bytes_size = total + RHP_PAD, .n = n,
                    .max_headers = M, .mode = RHP_MODE_HTTP, .layout = RHP_LAYOUT_REQUEST_MAJOR, .reqs = reqs,
                    .hdrs = hdrs, .http = http};
  if (rhp_cpu_parse_batch(&bt) != 0) return 2;

  /* the packed copies, in place in the buffers of an RHP_LAYOUT_DENSE batch
   * (rhp.h): the dense records first, then the wide areas = the batch's own */
  uint8_t *dq = xcalloc(RHP_DENSE_REQS_BYTES(n), 1), *dh = xcalloc(RHP_DENSE_HDRS_BYTES(n, M), 1);
  uint8_t *dx = xcalloc(RHP_COMPACT_HTTP_BYTES(n), 1);
  rhp_req_dense_t *dreq = (rhp_req_dense_t *) dq;
  rhp_http_compact_t *hc = (rhp_http_compact_t *) dx;
  uint16_t *lens16 = (uint16_t *) dh;
  if (rhp_cpu_pack_dense(&bt, dreq, hc, lens16) != 0) return 2;
  rhp_req_t *wide_req = (rhp_req_t *) (dq + RHP_DENSE_REQ_WIDE_OFF(n));
  memcpy(wide_req, reqs, n * sizeof *reqs);
  for (uint32_t i = 0; i < n; i++) wide_req[i].flags |= RHP_F_WIDE;   /* as a dense parse marks the wide area's */
  memcpy(dh + RHP_DENSE_WIDE_OFF(n, M), hdrs, (size_t) n * M * sizeof *hdrs);
  memcpy(dx + RHP_COMPACT_HTTP_WIDE_OFF(n), http, n * sizeof *http);

  rhp_batch_t bd = bt;
  bd.layout = RHP_LAYOUT_DENSE;
  rhp_req_t *ereq = xcalloc(n, sizeof *ereq);
  rhp_hdr_t *ehdr = xcalloc((size_t) n * M, sizeof *ehdr);
  rhp_http_t *ehttp = xcalloc(n, sizeof *ehttp);
  if (rhp_expand_reqs(&bd, dq, ereq) != 0 || rhp_expand_records(&bd, ereq, dh, ehdr) != 0 ||
      rhp_expand_http(&bd, ereq, dx, ehttp) != 0)
    return 2;

  const reactor_batch_result_t res = {.bytes = bytes, .offsets = off, .reqs = reqs, .hdrs = hdrs, .n = n, .http = http,
                                      .dense = 1, .dreq = dreq, .hc = hc, .lens16 = lens16};
  uint32_t ready = 0, dense = 0, wide_ready = 0, wide_http = 0, partial = 0, bad = 0;
  for (uint32_t i = 0; i < n; i++) {
    rhp_req_t req;
    rhp_http_t x;
    rhp_hdr_t h[M];
    const rhp_hdr_t *hp = NULL;
    reactor_batch_record(&res, i, &req, &x, h, &hp);
    same_http(i, "record / packed from", &x, &http[i]);
    same_http(i, "record / rhp_expand_http", &x, &ehttp[i]);
    partial += http[i].result == 0;
    bad += http[i].result == -1;
    wide_http += (hc[i].flags & RHP_HTTP_WIDE) != 0;
    if (http[i].result != 1) continue;
    ready++;
    dense += !(dreq[i].flags & RHP_DENSE_WIDE);
    wide_ready += (dreq[i].flags & RHP_DENSE_WIDE) != 0;
    same_req(i, "record / packed from", &req, &reqs[i]);
    same_req(i, "record / rhp_expand_reqs", &req, &ereq[i]);
    same_hdrs(i, "record / packed from", hp, hdrs + (size_t) i * M, reqs[i].num_headers);
    same_hdrs(i, "record / rhp_expand_records", hp, ehdr + (size_t) i * M, reqs[i].num_headers);
  }
  /* per length pair: GET, PUT and the late-field POST are ready and dense only
   * for 62 / 1007; the chunked POST is ready with a wide http record */
  if (ready != 16 || dense != 3 || wide_ready != 13 || wide_http != 4 || partial != 4 || bad != 1) {
    printf("unexpected batch: ready %u dense %u wide ready %u wide http %u partial %u bad %u\n", ready, dense,
           wide_ready, wide_http, partial, bad);
    fails++;
  }
  free(ereq); free(ehdr); free(ehttp); free(dq); free(dh); free(dx); free(reqs); free(hdrs); free(http); free(bytes);
  printf("reactor_record_test: %u slots, %u ready (%u dense, %u wide): %s\n", n, ready, dense, wide_ready,
         fails ? "FAILED" : "OK");
  return fails ? 1 : 0;
}
