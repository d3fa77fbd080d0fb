/*
 * walk_relay_host_test.c -- rhp_cpu_relay_walked (include/rhp_host.h) under
 * ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and
 * rhp_gen.c (the `walk-relay-asan` rule of libreactorng_amd/csrc/Makefile
 * builds and runs it).
 *
 * Sessions built here are walked by the host twin (rhp_cpu_walk_responses, with
 * and without RHP_WALK_DEFRAME) and then relayed.  Every buffer is allocated at
 * exactly its documented size -- out_off n + 1 words, why n words, work
 * RHP_RELAY_WORK_WORDS(n) words, out first 0 bytes (NULL) and then exactly
 * out_off[n] -- and the records of the slots the walk did not write are
 * poisoned for the sanitizer while the relay runs: it sees any access outside a
 * buffer and any read of a slot that is not in use.  The replies are compared
 * with the text written out below, why with the codes.  Then records built by
 * hand whose spans and bodies point outside, an out one byte short, and the
 * refusals.  Exits non-zero on the first mismatch.
 */
#include "rhp_host.h"

#define HOST_TEST_NAME "walk_relay_host_test"
#include "host_test.h"

#define DATE "Wed, 16 Aug 2023 10:29:23 GMT"
#define HEAD(status, type, len) "HTTP/1.1 " status "\r\nServer: *\r\nDate: " DATE "\r\nContent-Type: " type "\r\nContent-Length: " len "\r\n"

enum { NS = 4, CAP = 4, NT = NS * CAP, MAXH = 6 };

static const char *const SESSION[NS] = {
  /* a typed reply with dropped and kept fields, a chunked one, a 204 */
  "HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\nconnection: close\r\nX-Kept: 1\r\nContent-Length: 5\r\n\r\nhello"
  "HTTP/1.1 404    Not  Found\r\nTransfer-Encoding: chunked\r\nSERVER: up\r\n\r\n3\r\nabc\r\n2\r\nde\r\n0\r\n\r\n"
  "HTTP/1.0 204\r\n\r\n",
  /* an interim head, an obs-fold head, the last slot of a BODY round */
  "HTTP/1.1 100 Continue\r\n\r\n"
  "HTTP/1.1 200 OK\r\nX-A: 1\r\n folded\r\nContent-Length: 0\r\n\r\n"
  "HTTP/1.1 200 OK\r\nContent-Length: 9\r\n\r\n12345678",
  "",
  /* a reply, then a head that is not complete */
  "HTTP/1.1 099 Odd\r\nContent-Length: 1\r\nContent-Type:\r\ncontent-type: second\r\n\r\nzHTTP/1.1 200 OK\r\nContent-Len",
};

static const char *const REPLY_DEFRAMED =
  HEAD("200 OK", "text/plain", "5") "X-Kept: 1\r\n\r\nhello"
  HEAD("404 Not  Found", "", "5") "\r\nabcde"
  HEAD("204", "", "0") "\r\n"
  HEAD("099 Odd", "", "1") "\r\nz";
static const char *const REPLY_FRAMED =
  HEAD("200 OK", "text/plain", "5") "X-Kept: 1\r\n\r\nhello"
  HEAD("204", "", "0") "\r\n"
  HEAD("099 Odd", "", "1") "\r\nz";

static const uint32_t WHY[NT] = {
  RHP_RELAY_OK, RHP_RELAY_OK /* FRAMING without the de-framing */, RHP_RELAY_OK, RHP_RELAY_UNUSED,
  RHP_RELAY_INTERIM, RHP_RELAY_FOLD, RHP_RELAY_PARTIAL, RHP_RELAY_UNUSED,
  RHP_RELAY_UNUSED, RHP_RELAY_UNUSED, RHP_RELAY_UNUSED, RHP_RELAY_UNUSED,
  RHP_RELAY_OK, RHP_RELAY_NOT_HEAD, RHP_RELAY_UNUSED, RHP_RELAY_UNUSED,
};

typedef struct {
  uint8_t *bytes;
  uint64_t size, *sess_off, *slot_off;
  rhp_msg_t *msgs;
  rhp_hdr_t *hdrs;
  rhp_walk_slot_t *slots;
  rhp_walk_result_t *results;
  rhp_walk_batch_t w;
} walked_t;

static int walk(walked_t *x, uint32_t flags)
{
  uint64_t total = 0;
  for (int s = 0; s < NS; s++) total += strlen(SESSION[s]);
  x->size = total + RHP_PAD;
  x->bytes = calloc(1, x->size);
  x->sess_off = malloc((NS + 1) * sizeof(uint64_t));
  x->slot_off = malloc((NS + 1) * sizeof(uint64_t));
  x->msgs = malloc(NT * sizeof(rhp_msg_t));
  x->hdrs = malloc((size_t) NT * MAXH * sizeof(rhp_hdr_t));
  x->slots = malloc(NT * sizeof(rhp_walk_slot_t));
  x->results = malloc(NS * sizeof(rhp_walk_result_t));
  memset(x->msgs, 0xC3, NT * sizeof(rhp_msg_t));
  memset(x->hdrs, 0xC3, (size_t) NT * MAXH * sizeof(rhp_hdr_t));
  memset(x->slots, 0xC3, NT * sizeof(rhp_walk_slot_t));
  uint64_t at = 0;
  for (int s = 0; s < NS; s++) {
    x->sess_off[s] = at;
    x->slot_off[s] = (uint64_t) s * CAP;
    memcpy(x->bytes + at, SESSION[s], strlen(SESSION[s]));
    at += strlen(SESSION[s]);
  }
  x->sess_off[NS] = at;
  x->slot_off[NS] = NT;
  const rhp_walk_batch_t w = {x->bytes, x->bytes, x->size, x->sess_off, x->slot_off, NS, NT, MAXH, flags,
                              x->msgs, x->hdrs, x->slots, x->results};
  x->w = w;
  return rhp_cpu_walk_responses(&x->w);
}

static void unwritten(const walked_t *x, int poison)
{
  for (int s = 0; s < NS; s++)
    for (uint32_t k = x->results[s].n_slots; k < CAP; k++) {
      const size_t i = (size_t) s * CAP + k;
      if (poison) {
        POISON(&x->msgs[i], sizeof(rhp_msg_t)); POISON(&x->hdrs[i * MAXH], MAXH * sizeof(rhp_hdr_t)); POISON(&x->slots[i], sizeof(rhp_walk_slot_t));
      } else {
        UNPOISON(&x->msgs[i], sizeof(rhp_msg_t)); UNPOISON(&x->hdrs[i * MAXH], MAXH * sizeof(rhp_hdr_t)); UNPOISON(&x->slots[i], sizeof(rhp_walk_slot_t));
      }
    }
}

static void release(walked_t *x)
{
  free(x->bytes); free(x->sess_off); free(x->slot_off); free(x->msgs); free(x->hdrs); free(x->slots); free(x->results);
}

/* the relay over x with every output at its exact size: sizes first (out NULL), then the replies; *out and *total
 * are the caller's to free and read.  short_by: the second call's out is that many bytes short and must stay 0xC3 */
static int relay(const walked_t *x, const rhp_span_t *names, uint32_t n_names, const char *text, uint32_t *why, uint8_t **out,
                 uint64_t *total, uint64_t short_by)
{
  uint64_t *off = malloc((NT + 1) * sizeof(uint64_t)), *work = malloc(RHP_RELAY_WORK_WORDS(NT) * sizeof(uint64_t));
  memset(off, 0xC3, (NT + 1) * sizeof(uint64_t));
  rhp_walk_relay_t r = {(const uint8_t *) text, names, n_names, RHP_DATE_LEN, DATE, off, why, NULL, 0, work};
  int rc = rhp_cpu_relay_walked(&x->w, &r);
  if (rc == 0) {
    *total = off[NT];
    for (int i = 0; i < NT && rc == 0; i++)
      if (off[i] > off[i + 1] || (off[i] == off[i + 1]) != (why[i] != RHP_RELAY_OK)) rc = 1000 + i;
    const uint64_t size = *total - short_by;
    *out = malloc(size ? size : 1);
    memset(*out, 0xC3, size ? size : 1);
    r.out = size ? *out : NULL;
    r.out_size = size;
    if (rc == 0) rc = rhp_cpu_relay_walked(&x->w, &r);
    if (rc == 0 && off[NT] != *total) rc = 2000;
    for (uint64_t q = 0; short_by && q < size && rc == 0; q++)
      if ((*out)[q] != 0xC3) rc = 3000;
  }
  free(off); free(work);
  return rc;
}

int main(void)
{
  static const char text[] = "ConnectionServer";
  static const rhp_span_t names[2] = {{0, 10}, {10, 6}};
  for (int pass = 0; pass < 2; pass++) {
    const uint32_t flags = RHP_WALK_TRAILERS | (pass ? RHP_WALK_DEFRAME : 0u);
    walked_t x;
    if (walk(&x, flags) != 0) FAIL("the walk failed");
    uint32_t why[NT];
    uint8_t *out = NULL;
    uint64_t total = 0;
    unwritten(&x, 1);
    int rc = relay(&x, names, 2, text, why, &out, &total, 0);
    if (rc != 0) FAIL("pass %d: relay %d", pass, rc);
    const char *want = pass ? REPLY_DEFRAMED : REPLY_FRAMED;
    for (int i = 0; i < NT; i++) {
      const uint32_t w = !pass && i == 1 ? RHP_RELAY_FRAMING : WHY[i];
      if (why[i] != w) FAIL("pass %d: why[%d] is %u, not %u", pass, i, why[i], w);
    }
    if (total != strlen(want) || memcmp(out, want, total) != 0) FAIL("pass %d: %llu reply bytes differ from the %zu expected", pass, (unsigned long long) total, strlen(want));
    free(out);
    /* an out one byte short: the sizes are exact and nothing is written */
    if ((rc = relay(&x, names, 2, text, why, &out, &total, 1)) != 0) FAIL("pass %d: one byte short: %d", pass, rc);
    free(out);
    /* no caller's name: the two fields stay */
    if ((rc = relay(&x, NULL, 0, NULL, why, &out, &total, 0)) != 0) FAIL("pass %d: no names: %d", pass, rc);
    if (total != strlen(want) + strlen("connection: close\r\n") + strlen("SERVER: up\r\n") * (pass ? 1 : 0)) FAIL("pass %d: no names: %llu bytes", pass, (unsigned long long) total);
    free(out);
    /* records built by hand: spans and bodies that point outside are never read through */
    const rhp_msg_t m0 = x.msgs[0];
    const rhp_hdr_t h0 = x.hdrs[0];
    const rhp_walk_slot_t s0 = x.slots[0];
    struct { int what; uint32_t code; } crafted[] = {{0, RHP_RELAY_SPAN}, {1, RHP_RELAY_SPAN}, {2, RHP_RELAY_SPAN}, {3, RHP_RELAY_LONG},
                                                     {4, RHP_RELAY_BODY_OUTSIDE}, {5, RHP_RELAY_OUTSIDE}, {6, RHP_RELAY_FRAMING}, {7, RHP_RELAY_OK}};
    for (size_t c = 0; c < sizeof crafted / sizeof crafted[0]; c++) {
      x.msgs[0] = m0; x.hdrs[0] = h0; x.slots[0] = s0;
      switch (crafted[c].what) {
        case 0: x.msgs[0].msg_off = 0xFFF0; break;
        case 1: x.hdrs[0].name_off = (uint16_t) (m0.ret - 2); break;
        case 2: x.hdrs[0].value_len = 0xFFFF; break;
        case 3: x.slots[0].body_len = x.slots[0].wire_len = 1ull << 32; break;
        case 4: x.slots[0].body_len = x.slots[0].wire_len = 0x7fffffff; break;
        case 5: x.slots[0].start = ~0ull - 3; break;
        case 6: x.slots[0].wire_len = 6; break;
        case 7: x.msgs[0].num_headers = 0xFFFF; break;   /* capped at max_headers... */
      }
      if (crafted[c].what == 7) { x.hdrs[4] = x.hdrs[0]; x.hdrs[5] = x.hdrs[2]; }         /* ... whose records are there */
      if ((rc = relay(&x, names, 2, text, why, &out, &total, 0)) != 0) FAIL("pass %d: crafted %zu: %d", pass, c, rc);
      if (why[0] != crafted[c].code) FAIL("pass %d: crafted %zu: why[0] is %u, not %u", pass, c, why[0], crafted[c].code);
      free(out);
    }
    x.msgs[0] = m0; x.hdrs[0] = h0; x.slots[0] = s0;
    /* the refusals */
    uint64_t off[NT + 1], work[RHP_RELAY_WORK_WORDS(NT)];
    uint8_t o1[1];
    const rhp_walk_relay_t good = {(const uint8_t *) text, names, 2, RHP_DATE_LEN, DATE, off, why, NULL, 0, work};
    rhp_walk_relay_t r = good;
    if (rhp_cpu_relay_walked(&x.w, &good) != 0 || rhp_cpu_relay_walked(NULL, &good) != -22 || rhp_cpu_relay_walked(&x.w, NULL) != -22) FAIL("NULL arguments");
    r = good; r.out_off = NULL; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("out_off NULL");
    r = good; r.why = NULL; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("why NULL");
    r = good; r.date = NULL; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("date NULL");
    r = good; r.work = NULL; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("work NULL");
    r = good; r.date_len = 28; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("date_len");
    r = good; r.n_names = RHP_RELAY_MAX_NAMES + 1; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("n_names");
    r = good; r.names = NULL; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("names NULL");
    r = good; r.out_size = 1; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("out NULL with a size");
    const rhp_span_t empty[2] = {{0, 10}, {10, 0}}, longer[1] = {{0, RHP_CLASSIFY_NAME_MAX + 1}};
    r = good; r.names = empty; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("an empty name");
    r = good; r.names = longer; r.n_names = 1; if (rhp_cpu_relay_walked(&x.w, &r) != -22) FAIL("a name too long");
    rhp_walk_batch_t w = x.w;
    w.results = NULL; if (rhp_cpu_relay_walked(&w, &good) != -22) FAIL("results NULL");
    w = x.w; w.n_slots_total = 0; off[0] = 7; r = good; r.out = o1; r.out_size = 1; o1[0] = 0xC3;
    if (rhp_cpu_relay_walked(&w, &r) != 0 || off[0] != 0 || o1[0] != 0xC3) FAIL("no slot: out_off[0] = 0 and nothing else");
    w = x.w; w.n_sessions = 0; off[0] = 7;
    if (rhp_cpu_relay_walked(&w, &good) != 0 || off[0] != 0) FAIL("no session: out_off[0] = 0 and nothing else");
    unwritten(&x, 0);
    release(&x);
  }
  printf("walk_relay_host_test OK\n");
  return 0;
}
