/*
 * frame_messages_host_test.c -- rhp_cpu_frame_messages (include/rhp_host.h)
 * under ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and
 * rhp_gen.c (the `frame-messages-asan` rule of libreactorng_amd/csrc/Makefile
 * builds and runs it).
 *
 * It reads tests/golden/frame_messages.npz (argv[1], or the path from csrc/):
 * the sets of tests/frame_sets.py with the compiled reference's answers, written
 * flat and uncompressed by tests/golden/make_golden_frame_messages.py, whose
 * header names the arrays.  Every set is parsed with rhp_cpu_parse_messages and
 * framed with rhp_cpu_frame_messages in both layouts.  Every buffer is
 * allocated at exactly its documented size -- the set's bytes with their
 * RHP_PAD, offsets[n + 1], msgs[n], hdrs[n * max_headers], frames[n],
 * fields[n_names * n], decoders[n], the names' text -- and the outputs hold
 * 0xC3 first; the sanitizer sees any access outside a buffer.  Then records
 * that point past their message and past the batch's bytes, and the refusals.
 * Exits non-zero on the first mismatch.
 */
#include "rhp_host.h"

#define HOST_TEST_NAME "frame_messages_host_test"
#include "host_test.h"

static const char kMsg[] = "HTTP/1.1 200 OK\r\nContent-Length: 25\r\nConnection: close\r\n\r\n";   /* 58 bytes */

/* records no parse leaves, every buffer at its exact size: a ret past
 * bytes_size, a value and a name past ret, num_headers above max_headers, a
 * message that ends past bytes_size */
static int crafted(uint32_t layout)
{
  enum { N = 5, M = 4, LEN = sizeof kMsg - 1 };
  const uint64_t size = RHP_PAD;   /* four messages lie inside it, the last one ends past it */
  uint8_t *buf = (uint8_t *) calloc(1, (size_t) size);
  uint64_t *off = (uint64_t *) malloc(sizeof(uint64_t) * (N + 1));
  rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * N);
  rhp_hdr_t *hdrs = (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * N * M);
  rhp_frame_t *frames = (rhp_frame_t *) malloc(sizeof(rhp_frame_t) * N);
  rhp_fieldref_t *fields = (rhp_fieldref_t *) malloc(sizeof(rhp_fieldref_t) * N);
  uint8_t *text = (uint8_t *) malloc(10);
  rhp_span_t *names = (rhp_span_t *) malloc(sizeof(rhp_span_t));
  memcpy(text, "connection", 10);
  names[0].off = 0;
  names[0].len = 10;
  for (uint32_t i = 0; i <= N; i++) off[i] = (uint64_t) i * LEN;
  for (uint32_t i = 0; i + 1 < N; i++) memcpy(buf + off[i], kMsg, LEN);
  /* parse four whole messages in a roomy copy, then lay the records out for five */
  {
    uint8_t *room = (uint8_t *) calloc(1, (size_t) N * LEN + RHP_PAD);
    rhp_msg_t *pm = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * N);
    rhp_hdr_t *ph = (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * N * M);
    for (uint32_t i = 0; i < N; i++) memcpy(room + off[i], kMsg, LEN);
    const rhp_msg_batch_t pb = {room, off, (uint64_t) N * LEN + RHP_PAD, N, M, RHP_MSG_RESPONSE, layout, pm, ph, NULL};
    if (rhp_cpu_parse_messages(&pb) != 0) FAIL("crafted: the parse is refused");
    memcpy(msgs, pm, sizeof(rhp_msg_t) * N);
    memcpy(hdrs, ph, sizeof(rhp_hdr_t) * N * M);
    free(room); free(pm); free(ph);
  }
  if (msgs[0].ret != LEN || msgs[0].num_headers != 2) FAIL("crafted: the message does not parse as meant");
#define H(i, k) RHP_HDR(hdrs, layout, N, M, i, k)
  msgs[1].ret = 0x7fffffff;
  H(2, 0).value_len = 0xffff;
  H(2, 1).name_off = 0xff00;
  msgs[3].num_headers = 0xffff;
  memset(&H(3, 2), 0xff, sizeof(rhp_hdr_t));   /* name_off RHP_NAME_NULL */
  H(3, 3).name_off = 0xfff0;
  H(3, 3).name_len = 10;
  memset(frames, 0xC3, sizeof(rhp_frame_t) * N);
  memset(fields, 0xC3, sizeof(rhp_fieldref_t) * N);
  const rhp_msg_batch_t b = {buf, off, size, N, M, RHP_MSG_RESPONSE, layout, msgs, hdrs, NULL};
  const rhp_frame_args_t f = {text, names, 1, 0, fields, frames, NULL, 0};
  if (rhp_cpu_frame_messages(&b, &f) != 0) FAIL("crafted: refused");
  const rhp_frame_t want[N] = {{1, RHP_FRAME_LENGTH, 25}, {0, 0, 0}, {1, 0, 0}, {1, RHP_FRAME_LENGTH, 25}, {0, 0, 0}};
  const int present[N] = {1, 0, 0, 1, 0};
  for (uint32_t i = 0; i < N; i++) {
    if (frames[i].result != want[i].result || frames[i].body_kind != want[i].body_kind || frames[i].body_len != want[i].body_len)
      FAIL("crafted layout %u message %u: frame (%d, %u, %llu)", layout, i, frames[i].result, frames[i].body_kind,
           (unsigned long long) frames[i].body_len);
    if ((fields[i].value_off != RHP_NAME_NULL) != present[i] || fields[i].value_len != (present[i] ? 5 : 0))
      FAIL("crafted layout %u message %u: field (%u, %u)", layout, i, fields[i].value_off, fields[i].value_len);
  }
#undef H
  free(buf); free(off); free(msgs); free(hdrs); free(frames); free(fields); free(text); free(names);
  return 0;
}

static int refusals(void)
{
  uint8_t *bytes = (uint8_t *) calloc(1, 512);
  uint64_t off[2] = {0, 0};
  rhp_msg_t m;
  rhp_hdr_t h[4];
  rhp_frame_t fr;
  rhp_fieldref_t fl;
  rhp_chunked_t d;
  const uint8_t text[] = "Host";
  rhp_span_t names[1] = {{0, 4}};
  memset(&m, 0, sizeof m);
  m.ret = -2;
  memset(&fr, 0x77, sizeof fr);
  memset(&fl, 0x77, sizeof fl);
  memset(&d, 0x77, sizeof d);
  const rhp_msg_batch_t okb = {bytes, off, 512, 1, 4, RHP_MSG_RESPONSE, RHP_LAYOUT_REQUEST_MAJOR, &m, h, NULL};
  const rhp_frame_args_t okf = {text, names, 1, 1, &fl, &fr, &d, 0};
  rhp_msg_batch_t b;
  rhp_frame_args_t f;
  if (rhp_cpu_frame_messages(NULL, &okf) != -22 || rhp_cpu_frame_messages(&okb, NULL) != -22) FAIL("a NULL batch or f is refused");
#define REFUSED(change, what) do { b = okb; f = okf; change; if (rhp_cpu_frame_messages(&b, &f) != -22) FAIL("refusal: %s", what); } while (0)
  REFUSED(b.bytes = NULL, "NULL bytes");
  REFUSED(b.offsets = NULL, "NULL offsets");
  REFUSED(b.msgs = NULL, "NULL msgs");
  REFUSED(b.hdrs = NULL, "NULL hdrs with max_headers > 0");
  REFUSED(b.kind = 2, "kind");
  REFUSED(b.layout = RHP_LAYOUT_COMPACT, "layout");
  REFUSED(b.max_headers = RHP_MAX_HEADERS + 1, "max_headers");
  REFUSED((b.n = 0xffffffffu, b.max_headers = 2), "n * max_headers >= 2^32");
  REFUSED(b.bytes_size = RHP_PAD - 1, "bytes_size below RHP_PAD");
  REFUSED((b.n = 0, b.kind = 9), "the rules come before the empty batch");
  REFUSED(f.n_names = RHP_CLASSIFY_MAX_NAMES + 1, "n_names");
  REFUSED(f.text = NULL, "NULL text");
  REFUSED(f.names = NULL, "NULL names");
  REFUSED(f.fields = NULL, "NULL fields");
  REFUSED(names[0].len = 0, "an empty name");
  REFUSED(names[0].len = RHP_CLASSIFY_NAME_MAX + 1, "a long name");
  names[0].len = 4;
  REFUSED(f.frames = NULL, "NULL frames");
  REFUSED(f.consume_trailer = 2, "consume_trailer");
  REFUSED(f.reserved = 1, "reserved");
  if (fr.result != 0x77777777 || fl.value_off != 0x7777 || d.state != 0x77) FAIL("a refused call writes nothing");
  b = okb;
  b.n = 0;
  b.bytes = NULL;
  b.offsets = NULL;
  b.msgs = NULL;
  b.hdrs = NULL;
  if (rhp_cpu_frame_messages(&b, &okf) != 0 || fr.result != 0x77777777) FAIL("an empty batch succeeds and writes nothing");
  if (rhp_cpu_frame_messages(&okb, &okf) != 0 || fr.result != 0 || fr.body_kind != 0 || fr.body_len != 0 ||
      fl.value_off != RHP_NAME_NULL || fl.value_len != 0 || d.state != 0x77)
    FAIL("a message that is not ready: result 0, no field, the decoder untouched");
  free(bytes);
  return 0;
}

int main(int argc, char **argv)
{
  const char *path = argc > 1 ? argv[1] : "../../tests/golden/frame_messages.npz";
  if (npz_open(path)) return 1;

  LOAD(set_kind, uint32_t, "'<u4'");
  LOAD(set_maxh, uint32_t, "'<u4'");
  LOAD(set_msg, uint32_t, "'<u4'");
  LOAD(set_byte, uint64_t, "'<u8'");
  LOAD(bytes, uint8_t, "'|u1'");
  LOAD(offsets, uint64_t, "'<u8'");
  LOAD(set_names, uint32_t, "'<u4'");
  LOAD(name_span, uint32_t, "'<u4'");
  LOAD(name_text, uint8_t, "'|u1'");
  LOAD(result, int32_t, "'<i4'");
  LOAD(body_kind, uint32_t, "'<u4'");
  LOAD(body_len, uint64_t, "'<u8'");
  LOAD(set_field, uint32_t, "'<u4'");
  LOAD(field, uint16_t, "'<u2'");
  const size_t S = n_set_kind, N = n_result;
  if (!S || n_set_maxh != S || n_set_msg != S + 1 || n_set_byte != S + 1 || set_msg[S] != N || set_byte[S] != n_bytes ||
      n_offsets != N + S || n_set_names != S + 1 || n_name_span != 2u * set_names[S] || n_body_kind != N || n_body_len != N ||
      n_set_field != S + 1 || n_field != 2u * set_field[S])
    FAIL("%s: the arrays' sizes do not fit each other", path);

  size_t framed = 0, calls = 0, armed = 0;
  for (size_t s = 0; s < S; s++) {
    const uint32_t lo = set_msg[s], n = set_msg[s + 1] - lo, maxh = set_maxh[s], kind = set_kind[s];
    const uint32_t nn = set_names[s + 1] - set_names[s];
    const size_t blen = (size_t) (set_byte[s + 1] - set_byte[s]);
    if (set_field[s + 1] - set_field[s] != nn * n) FAIL("set %zu: the file's field count", s);
    size_t tlen = 0;
    for (uint32_t j = 0; j < nn; j++) tlen += name_span[2u * (set_names[s] + j) + 1u];
    uint8_t *buf = (uint8_t *) malloc(blen);
    uint64_t *off = (uint64_t *) malloc(sizeof(uint64_t) * (n + 1u));
    rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * n);
    rhp_hdr_t *hdrs = maxh ? (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * n * maxh) : NULL;
    rhp_frame_t *frames = (rhp_frame_t *) malloc(sizeof(rhp_frame_t) * n);
    rhp_fieldref_t *fields = nn ? (rhp_fieldref_t *) malloc(sizeof(rhp_fieldref_t) * nn * n) : NULL;
    rhp_chunked_t *dec = (rhp_chunked_t *) malloc(sizeof(rhp_chunked_t) * n);
    uint8_t *text = nn ? (uint8_t *) malloc(tlen) : NULL;
    rhp_span_t *names = nn ? (rhp_span_t *) malloc(sizeof(rhp_span_t) * nn) : NULL;
    memcpy(buf, bytes + set_byte[s], blen);
    memcpy(off, offsets + lo + s, sizeof(uint64_t) * (n + 1u));
    for (uint32_t j = 0, at = 0; j < nn; j++) {
      const uint32_t *sp = name_span + 2u * (set_names[s] + j);
      memcpy(text + at, name_text + sp[0], sp[1]);
      names[j].off = at;
      names[j].len = sp[1];
      at += sp[1];
    }
    if (off[n] + RHP_PAD > blen) FAIL("set %zu: no pad behind the messages", s);

    for (uint32_t layout = RHP_LAYOUT_REQUEST_MAJOR; layout <= RHP_LAYOUT_HEADER_MAJOR; layout++) {
      const uint32_t ct = (uint32_t) (s + layout) & 1u;
      memset(msgs, 0xC3, sizeof(rhp_msg_t) * n);
      if (hdrs) memset(hdrs, 0xC3, sizeof(rhp_hdr_t) * n * maxh);
      memset(frames, 0xC3, sizeof(rhp_frame_t) * n);
      if (fields) memset(fields, 0xC3, sizeof(rhp_fieldref_t) * nn * n);
      memset(dec, 0xC3, sizeof(rhp_chunked_t) * n);
      const rhp_msg_batch_t b = {buf, off, blen, n, maxh, kind, layout, msgs, hdrs, NULL};
      const rhp_frame_args_t f = {text, names, nn, ct, fields, frames, dec, 0};
      if (rhp_cpu_parse_messages(&b) != 0) FAIL("set %zu layout %u: the parse is refused", s, layout);
      if (rhp_cpu_frame_messages(&b, &f) != 0) FAIL("set %zu layout %u: refused", s, layout);
      for (uint32_t i = 0; i < n; i++) {
        const size_t g = lo + i;
        if (frames[i].result != result[g] || frames[i].body_kind != body_kind[g] || frames[i].body_len != body_len[g])
          FAIL("set %zu layout %u message %u: frame (%d, %u, %llu), the reference's (%d, %u, %llu)", s, layout, i, frames[i].result,
               frames[i].body_kind, (unsigned long long) frames[i].body_len, result[g], body_kind[g], (unsigned long long) body_len[g]);
        for (uint32_t j = 0; j < nn; j++) {
          const uint16_t *e = field + 2u * (set_field[s] + (size_t) j * n + i);
          const rhp_fieldref_t r = fields[(size_t) j * n + i];
          if (r.value_off != e[0] || r.value_len != e[1]) FAIL("set %zu layout %u message %u name %u: the field differs", s, layout, i, j);
        }
        const uint8_t *d = (const uint8_t *) &dec[i];
        for (uint32_t q = 0; q < 16; q++) {
          const uint8_t want = body_kind[g] == RHP_FRAME_CHUNKED ? (q == 8 ? (uint8_t) ct : 0) : 0xC3;
          if (d[q] != want) FAIL("set %zu layout %u message %u: decoder byte %u is %u", s, layout, i, q, d[q]);
        }
        armed += body_kind[g] == RHP_FRAME_CHUNKED;
        framed++;
      }
      calls++;
    }
    free(buf); free(off); free(msgs); free(hdrs); free(frames); free(fields); free(dec); free(text); free(names);
  }
  if (crafted(RHP_LAYOUT_REQUEST_MAJOR) || crafted(RHP_LAYOUT_HEADER_MAJOR)) return 1;
  if (refusals()) return 1;
  free(set_kind); free(set_maxh); free(set_msg); free(set_byte); free(bytes); free(offsets); free(set_names); free(name_span);
  free(name_text); free(result); free(body_kind); free(body_len); free(set_field); free(field); free(g_file);
  printf("frame_messages_host_test OK: %zu sets, %zu messages, %zu batch calls, %zu frames compared, %zu decoders armed\n", S, N,
         calls, framed, armed);
  return 0;
}
