/*
 * decode_chunked_host_test.c -- rhp_cpu_decode_chunked and
 * rhp_phr_decode_chunked (include/rhp_host.h) under ASan/UBSan: a stand-alone
 * program over rhp_host.cpp, rhp_emu.cpp and rhp_gen.c (the
 * `decode-chunked-asan` rule of libreactorng_amd/csrc/Makefile builds and runs
 * it).
 *
 * It reads tests/golden/decode_chunked.npz (argv[1], or the path from csrc/):
 * the calls of tests/decode_chunked_sets.py with the compiled reference's
 * answers, written flat and uncompressed by
 * tests/golden/make_golden_decode_chunked.py, whose header names the arrays.
 * Every set runs through the batch twin as one batch, its pieces packed back to
 * back from the set's start on in an allocation of exactly that size, with
 * offsets[n + 1], decoders[n] and results[n] at theirs; every record runs
 * through the pointer-based function on a piece allocated at exactly its size
 * (an empty piece: one byte that is never touched).  The sanitizer sees any
 * access outside a buffer.  ret, size, the 16 bytes of the decoder and every
 * byte of the piece are compared.  Then the refusals and the corrupt decoders.
 * Exits non-zero on the first mismatch.
 */
#include "rhp_host.h"

#define HOST_TEST_NAME "decode_chunked_host_test"
#include "host_test.h"

static int refusals(void)
{
  static const char body[] = "3\r\nabc\r\n0\r\nXY";
  enum { LEN = sizeof body - 1 };
  uint8_t bytes[LEN];
  uint64_t off[2] = {0, LEN};
  memcpy(bytes, body, LEN);
  rhp_chunked_t d, d0;
  rhp_chunked_result_t r;
  memset(&d, 0, sizeof d);
  memset(&r, 0x77, sizeof r);
  rhp_chunked_batch_t ok = {bytes, off, LEN, 1, 0, &d, &r}, b;
  if (rhp_cpu_decode_chunked(NULL) != -22) FAIL("a NULL batch is refused");
#define REFUSED(change, what) do { b = ok; change; if (rhp_cpu_decode_chunked(&b) != -22) FAIL("refusal: %s", what); } while (0)
  REFUSED(b.bytes = NULL, "NULL bytes");
  REFUSED(b.offsets = NULL, "NULL offsets");
  REFUSED(b.decoders = NULL, "NULL decoders");
  REFUSED(b.results = NULL, "NULL results");
  REFUSED(b.reserved = 1, "reserved");
  REFUSED((b.n = 0, b.reserved = 7), "the rules come before the empty batch");
  if (r.ret != 0x7777777777777777ll || bytes[0] != '3' || d.state != 0) FAIL("a refused call writes nothing");
  b = ok;
  b.n = 0;
  b.bytes = NULL;
  b.offsets = NULL;
  b.decoders = NULL;
  b.results = NULL;
  if (rhp_cpu_decode_chunked(&b) != 0 || r.ret != 0x7777777777777777ll) FAIL("an empty batch succeeds and writes nothing");
  /* corrupt decoders: -1, size 0, nothing touched */
  const uint8_t bad[3][2] = {{6, 0}, {255, 0}, {0, 17}};
  for (int k = 0; k < 3; k++) {
    memset(&d, 0x5a, sizeof d);
    d.state = bad[k][0];
    d.hex_count = bad[k][1];
    d0 = d;
    memset(&r, 0x77, sizeof r);
    if (rhp_cpu_decode_chunked(&ok) != 0 || r.ret != -1 || r.size != 0 || memcmp(&d, &d0, sizeof d) != 0 ||
        memcmp(bytes, body, LEN) != 0)
      FAIL("corrupt decoder %d: the batch twin", k);
    size_t sz = LEN;
    if (rhp_phr_decode_chunked(&d, (char *) bytes, &sz) != -1 || sz != 0 || memcmp(&d, &d0, sizeof d) != 0 ||
        memcmp(bytes, body, LEN) != 0)
      FAIL("corrupt decoder %d: the pointer-based function", k);
  }
  /* offsets beyond bytes_size are clamped */
  memset(&d, 0, sizeof d);
  off[0] = 8;   /* "0 CR LF XY": the body's end, two bytes behind it */
  off[1] = ~(uint64_t) 0;
  if (rhp_cpu_decode_chunked(&ok) != 0 || r.ret != 2 || r.size != 0 || memcmp(bytes + 8, "XY", 2) != 0) FAIL("a piece clamped to bytes_size");
  off[0] = ~(uint64_t) 0;
  off[1] = 5;
  if (rhp_cpu_decode_chunked(&ok) != 0 || r.ret != -2 || r.size != 0) FAIL("a piece that starts beyond bytes_size is empty");
  return 0;
}

int main(int argc, char **argv)
{
  const char *path = argc > 1 ? argv[1] : "../../tests/golden/decode_chunked.npz";
  if (npz_open(path)) return 1;

  LOAD(set_start, uint64_t, "'<u8'");
  LOAD(set_lo, uint32_t, "'<u4'");
  LOAD(item_rec, uint32_t, "'<u4'");
  LOAD(rec_lo, uint64_t, "'<u8'");
  LOAD(before, uint8_t, "'|u1'");
  LOAD(after, uint8_t, "'|u1'");
  LOAD(dec_before, uint8_t, "'|u1'");
  LOAD(dec_after, uint8_t, "'|u1'");
  LOAD(ret, int64_t, "'<i8'");
  LOAD(size, uint64_t, "'<u8'");
  const size_t S = n_set_start, R = n_ret, I = n_item_rec;
  if (!S || !R || n_set_lo != S + 1 || set_lo[S] != I || n_rec_lo != R + 1 || rec_lo[R] != n_before || n_after != n_before ||
      n_dec_before != 16 * R || n_dec_after != 16 * R || n_size != R)
    FAIL("%s: the arrays' sizes do not fit each other", path);
  for (size_t k = 0; k < I; k++)
    if (item_rec[k] >= R) FAIL("%s: a call's record index", path);

  for (size_t s = 0; s < S; s++) {   /* the batch twin: a set as one batch */
    const uint32_t lo = set_lo[s], n = set_lo[s + 1] - lo;
    size_t total = (size_t) set_start[s];
    for (uint32_t i = 0; i < n; i++) total += (size_t) (rec_lo[item_rec[lo + i] + 1] - rec_lo[item_rec[lo + i]]);
    uint8_t *buf = (uint8_t *) malloc(total ? total : 1), *want = (uint8_t *) malloc(total ? total : 1);
    uint64_t *off = (uint64_t *) malloc(sizeof(uint64_t) * (n + 1u));
    rhp_chunked_t *dec = (rhp_chunked_t *) malloc(sizeof(rhp_chunked_t) * n);
    rhp_chunked_result_t *res = (rhp_chunked_result_t *) malloc(sizeof(rhp_chunked_result_t) * n);
    memset(buf, 0xEE, (size_t) set_start[s]);
    memset(want, 0xEE, (size_t) set_start[s]);
    memset(res, 0xC3, sizeof(rhp_chunked_result_t) * n);
    size_t at = (size_t) set_start[s];
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t r = item_rec[lo + i];
      const size_t len = (size_t) (rec_lo[r + 1] - rec_lo[r]);
      off[i] = at;
      if (len) memcpy(buf + at, before + rec_lo[r], len);
      if (len) memcpy(want + at, after + rec_lo[r], len);
      memcpy(&dec[i], dec_before + 16u * r, 16);
      at += len;
    }
    off[n] = at;
    const rhp_chunked_batch_t b = {buf, off, total, n, 0, dec, res};
    if (rhp_cpu_decode_chunked(&b) != 0) FAIL("set %zu: refused", s);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t r = item_rec[lo + i];
      if (res[i].ret != ret[r] || res[i].size != size[r])
        FAIL("set %zu piece %u: ret %lld size %llu, the reference's %lld %llu", s, i, (long long) res[i].ret,
             (unsigned long long) res[i].size, (long long) ret[r], (unsigned long long) size[r]);
      if (memcmp(&dec[i], dec_after + 16u * r, 16) != 0) FAIL("set %zu piece %u: the decoder differs from the reference's", s, i);
    }
    if (total && memcmp(buf, want, total) != 0) FAIL("set %zu: the bytes differ from the reference's", s);
    free(buf); free(want); free(off); free(dec); free(res);
  }

  for (size_t r = 0; r < R; r++) {   /* the pointer-based function: every record */
    const size_t len = (size_t) (rec_lo[r + 1] - rec_lo[r]);
    char *piece = (char *) malloc(len ? len : 1);
    rhp_chunked_t d;
    if (len) memcpy(piece, before + rec_lo[r], len);
    memcpy(&d, dec_before + 16u * r, 16);
    size_t sz = len;
    const ssize_t got = rhp_phr_decode_chunked(&d, piece, &sz);
    if (got != ret[r] || sz != size[r]) FAIL("record %zu: the pointer-based function's ret or size", r);
    if (memcmp(&d, dec_after + 16u * r, 16) != 0) FAIL("record %zu: the pointer-based function's decoder", r);
    if (len && memcmp(piece, after + rec_lo[r], len) != 0) FAIL("record %zu: the pointer-based function's bytes", r);
    if (rhp_phr_decode_chunked_is_in_data(&d) != (d.state == RHP_CHUNKED_IN_CHUNK_DATA)) FAIL("record %zu: is_in_data", r);
    free(piece);
  }
  if (refusals()) return 1;
  free(set_start); free(set_lo); free(item_rec); free(rec_lo); free(before); free(after); free(dec_before); free(dec_after);
  free(ret); free(size); free(g_file);
  printf("decode_chunked_host_test OK: %zu sets, %zu calls, %zu records\n", S, I, R);
  return 0;
}
