/*
 * walk_lookup_host_test.c -- rhp_cpu_lookup_walked (include/rhp_host.h) under
 * ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and
 * rhp_gen.c (the `walk-lookup-asan` rule of libreactorng_amd/csrc/Makefile
 * builds and runs it).
 *
 * It reads tests/golden/walk_lookup.npz (argv[1], or the path from csrc/): the
 * calls of the sets of tests/walk_lookup_sets.py with the reference's
 * http_field_lookup over every head slot, written flat and uncompressed by
 * tests/golden/make_golden_walk_lookup.py, whose header names the arrays.
 * Every set's calls are walked by the host twin (rhp_cpu_walk_responses, or
 * rhp_cpu_walk_resume as a chain with the states carried) and then looked up.
 * Every buffer is allocated at exactly its documented size, fields holds 0xC3
 * first, and the records of the slots the walk did not write are poisoned for
 * the sanitizer while the lookup runs: it sees any access outside a buffer and
 * any read of a slot that is not in use.  Every field of every slot is
 * compared.  Then records built by hand that each gate of rhp.h has to stop,
 * the bytes at exactly bytes_size, and the refusals.  Exits non-zero on the
 * first mismatch.
 */
#include "rhp_host.h"

#define HOST_TEST_NAME "walk_lookup_host_test"
#include "host_test.h"

static int is_absent(const rhp_fieldref_t *f) { return f->value_off == RHP_NAME_NULL && f->value_len == 0; }

/* records built by hand: two sessions, three slots each, one head written per
 * session; every buffer at its exact size, the bytes at exactly bytes_size */
static int crafted(void)
{
  static const char kHead[] = "HTTP/1.1 200 OK\r\nConnection: close\r\nContent-Length: 0\r\n\r\n";
  enum { RET = sizeof kHead - 1, AT1 = 250, NS = 2, NT = 6, M = 2, SIZE = AT1 + RET + RHP_PAD };   /* session 1 starts at AT1 */
  static const char kText[] = "connectionCONTENT-LENGTHX-Sixty-Four-nnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnnn";
  _Static_assert(sizeof kText - 1 == 10 + 14 + 64, "three names");
  const rhp_span_t names[3] = {{0, 10}, {10, 14}, {24, 64}};
  int cases = 0;
  for (int c = 0; c < 12; c++) {
    uint64_t size = SIZE;
    if (c == 5) size = AT1 + RET - 1;   /* the second head ends past bytes_size & ~3, the first does not */
    uint8_t *buf = (uint8_t *) calloc(1, (size_t) size);
    memcpy(buf, kHead, RET);
    memcpy(buf + AT1, kHead, c == 5 ? RET - 1 : RET);
    uint64_t *so = (uint64_t *) malloc(8 * (NS + 1)), *sl = (uint64_t *) malloc(8 * (NS + 1));
    so[0] = 0; so[1] = AT1; so[2] = AT1 + RET;
    sl[0] = 0; sl[1] = 3; sl[2] = 6;
    rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * NT);
    rhp_hdr_t *hdrs = (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * NT * M);
    rhp_walk_slot_t *slots = (rhp_walk_slot_t *) malloc(sizeof(rhp_walk_slot_t) * NT);
    rhp_walk_result_t *res = (rhp_walk_result_t *) malloc(sizeof(rhp_walk_result_t) * NS);
    rhp_fieldref_t *fields = (rhp_fieldref_t *) malloc(sizeof(rhp_fieldref_t) * 3 * NT);
    memset(msgs, 0xC3, sizeof(rhp_msg_t) * NT);
    memset(hdrs, 0xC3, sizeof(rhp_hdr_t) * NT * M);
    memset(slots, 0xC3, sizeof(rhp_walk_slot_t) * NT);
    memset(fields, 0xC3, sizeof(rhp_fieldref_t) * 3 * NT);
    for (int s = 0; s < NS; s++) {
      const int i = 3 * s;
      res[s].n_slots = 1; res[s].stop = RHP_WALK_END; res[s].consumed = so[s + 1] - so[s];
      memset(&msgs[i], 0, sizeof msgs[i]);
      msgs[i].ret = RET; msgs[i].status = 200; msgs[i].num_headers = 2;
      hdrs[i * M + 0] = (rhp_hdr_t){17, 10, 29, 5};
      hdrs[i * M + 1] = (rhp_hdr_t){36, 14, 52, 1};
      memset(&slots[i], 0, sizeof slots[i]);
      slots[i].start = (uint64_t) s * AT1; slots[i].result = 1; slots[i].body_kind = RHP_FRAME_LENGTH;
    }
    /* what each case does to slot 3 (session 1's head), and whether slot 3 keeps its two fields */
    int keep = 0;
    uint32_t nt = NT;
    switch (c) {
      case 0: keep = 1; break;                                             /* sound */
      case 1: sl[2] = 7; break;                                            /* slot_off[s+1] above n_slots_total */
      case 2: slots[3].start = so[1] - 1; break;                           /* start below sess_off[s] */
      case 3: slots[3].start = so[1] + 1; break;                           /* start + ret past sess_off[s+1] */
      case 4: slots[3].start = ~(uint64_t) 0; break;
      case 5: break;                                                       /* start + ret past bytes_size & ~3 */
      case 6: msgs[3].ret = 0; break;                                      /* a continuation slot */
      case 7: slots[3].result = -1; break;                                 /* a BAD stop slot */
      case 8: msgs[3].ret = RHP_RET_TOOLONG; break;
      case 9: res[1].n_slots = 0; break;                                   /* not written */
      case 10: msgs[3].num_headers = 0xFFFF; keep = 1; break;              /* num_headers above max_headers: two records scanned */
      case 11: hdrs[3 * M] = (rhp_hdr_t){RET - 5, 64, 29, 5}; hdrs[3 * M + 1] = (rhp_hdr_t){0xFFF0, 14, 52, 1}; break;   /* names past ret */
    }
    for (uint32_t i = 0; i < NT; i++) {   /* the slots not in use: never read */
      const uint32_t s = i / 3;
      if (i % 3 < res[s].n_slots && !(c == 1 && s == 1)) continue;
      POISON(&msgs[i], sizeof msgs[i]); POISON(&slots[i], sizeof slots[i]); POISON(&hdrs[i * M], sizeof(rhp_hdr_t) * M);
    }
    const rhp_walk_batch_t w = {buf, buf, size, so, sl, NS, nt, M, 0, msgs, hdrs, slots, res};
    const rhp_walk_lookup_t l = {(const uint8_t *) kText, names, 3, 0, fields};
    if (rhp_cpu_lookup_walked(&w, &l) != 0) FAIL("crafted case %d: refused", c);
    UNPOISON(msgs, sizeof(rhp_msg_t) * NT); UNPOISON(slots, sizeof(rhp_walk_slot_t) * NT); UNPOISON(hdrs, sizeof(rhp_hdr_t) * NT * M);
    for (uint32_t j = 0; j < 3; j++)
      for (uint32_t i = 0; i < NT; i++) {
        const rhp_fieldref_t *f = &fields[j * NT + i];
        const int present = j < 2 && (i == 0 || (i == 3 && keep));
        if (!present && !is_absent(f)) FAIL("crafted case %d: name %u of slot %u is {%u, %u}, not absent", c, j, i, f->value_off, f->value_len);
        if (present && (f->value_off != (j ? 52u : 29u) || f->value_len != (j ? 1u : 5u)))
          FAIL("crafted case %d: name %u of slot %u is {%u, %u}", c, j, i, f->value_off, f->value_len);
      }
    free(buf); free(so); free(sl); free(msgs); free(hdrs); free(slots); free(res); free(fields);
    cases++;
  }
  return cases == 12 ? 0 : 1;
}

static int refusals(void)
{
  uint8_t *bytes = (uint8_t *) calloc(1, 512);
  uint64_t so[2] = {0, 0}, sl[2] = {0, 1};
  rhp_msg_t m;
  rhp_hdr_t h[4];
  rhp_walk_slot_t x;
  rhp_walk_result_t r = {0, 0, 0};
  rhp_fieldref_t f[2];
  const rhp_span_t names[2] = {{0, 1}, {1, 2}};
  const uint8_t text[3] = {'a', 'b', 'c'};
  const rhp_walk_batch_t ok = {bytes, bytes, 512, so, sl, 1, 1, 4, 0, &m, h, &x, &r};
  const rhp_walk_lookup_t lk = {text, names, 2, 0, f};
  memset(f, 0xC3, sizeof f);
  if (rhp_cpu_lookup_walked(&ok, &lk) != 0 || !is_absent(&f[0]) || !is_absent(&f[1])) FAIL("a sound call was refused, or its unwritten slot is not absent");
  if (rhp_cpu_lookup_walked(&ok, NULL) != -22 || rhp_cpu_lookup_walked(NULL, &lk) != -22) FAIL("a NULL argument accepted");
  rhp_walk_batch_t b = ok;
  b.flags = 8;
  if (rhp_cpu_lookup_walked(&b, &lk) != -22) FAIL("an unknown flag accepted");
  b = ok;
  b.results = NULL;
  if (rhp_cpu_lookup_walked(&b, &lk) != -22) FAIL("NULL results accepted");
  rhp_walk_lookup_t q = lk;
  q.reserved = 1;
  if (rhp_cpu_lookup_walked(&ok, &q) != -22) FAIL("reserved accepted");
  q = lk; q.n_names = 0;
  if (rhp_cpu_lookup_walked(&ok, &q) != -22) FAIL("no name accepted");
  q = lk; q.n_names = RHP_CLASSIFY_MAX_NAMES + 1;
  if (rhp_cpu_lookup_walked(&ok, &q) != -22) FAIL("17 names accepted");
  q = lk; q.fields = NULL;
  if (rhp_cpu_lookup_walked(&ok, &q) != -22) FAIL("NULL fields accepted");
  const rhp_span_t bad[2] = {{0, 0}, {0, 65}};
  q = lk; q.names = bad; q.n_names = 1;
  if (rhp_cpu_lookup_walked(&ok, &q) != -22) FAIL("an empty name accepted");
  q.names = bad + 1;
  if (rhp_cpu_lookup_walked(&ok, &q) != -22) FAIL("a 65-byte name accepted");
  memset(f, 0xC3, sizeof f);
  b = ok;
  b.n_sessions = 0;
  if (rhp_cpu_lookup_walked(&b, &lk) != 0 || f[0].value_off != 0xC3C3) FAIL("no session: succeeds, fields untouched");
  free(bytes);
  return 0;
}

int main(int argc, char **argv)
{
  const char *path = argc > 1 ? argv[1] : "../../tests/golden/walk_lookup.npz";
  if (npz_open(path)) return 1;
  LOAD(set_maxh, uint32_t, "<u4"); LOAD(set_flags, uint32_t, "<u4"); LOAD(set_nsess, uint32_t, "<u4"); LOAD(set_resume, uint8_t, "|u1");
  LOAD(set_call, uint32_t, "<u4"); LOAD(set_first, uint32_t, "<u4"); LOAD(states_in, uint8_t, "|u1"); LOAD(set_names, uint32_t, "<u4");
  LOAD(name_span, uint32_t, "<u4"); LOAD(name_text, uint8_t, "|u1");
  LOAD(call_q, uint32_t, "<u4"); LOAD(call_f, uint32_t, "<u4"); LOAD(call_byte, uint64_t, "<u8"); LOAD(bytes, uint8_t, "|u1");
  LOAD(len, uint32_t, "<u4"); LOAD(cap, uint8_t, "|u1"); LOAD(n_slots, uint8_t, "|u1");
  LOAD(f_slot, uint32_t, "<u4"); LOAD(f_name, uint8_t, "|u1"); LOAD(f_off, uint16_t, "<u2"); LOAD(f_len, uint16_t, "<u2");
  const size_t S = n_set_maxh;
  if (n_set_call != S + 1 || n_set_first != S + 1 || n_set_names != S + 1 || n_len != n_cap || n_f_slot != n_f_len || n_name_span % 2) FAIL("%s: sizes", path);
  size_t calls_run = 0, present = 0;
  for (size_t s = 0; s < S; s++) {
    const uint32_t n = set_nsess[s], maxh = set_maxh[s], nn = set_names[s + 1] - set_names[s];
    const rhp_span_t *names = (const rhp_span_t *) (name_span + 2 * (size_t) set_names[s]);
    for (int deframe = 0; deframe < 2; deframe++) {
      rhp_walk_state_t *st = (rhp_walk_state_t *) calloc(n ? n : 1, sizeof(rhp_walk_state_t));
      if (set_first[s + 1] > set_first[s]) memcpy(st, states_in + 32 * (size_t) set_first[s], 32 * (size_t) n);
      for (uint32_t c = set_call[s]; c < set_call[s + 1]; c++) {
        const size_t q0 = call_q[c], nb = (size_t) (call_byte[c + 1] - call_byte[c]);
        if (call_q[c + 1] - q0 != n) FAIL("set %zu call %u: sessions", s, c);
        uint8_t *buf = (uint8_t *) calloc(1, nb + RHP_PAD);
        memcpy(buf, bytes + call_byte[c], nb);
        uint64_t *so = (uint64_t *) calloc(n + 1, 8), *sl = (uint64_t *) calloc(n + 1, 8);
        for (uint32_t i = 0; i < n; i++) {
          so[i + 1] = so[i] + len[q0 + i];
          sl[i + 1] = sl[i] + cap[q0 + i];
        }
        const uint32_t nt = (uint32_t) sl[n];
        rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * (nt ? nt : 1));
        rhp_hdr_t *hdrs = (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * (size_t) nt * maxh + 1);
        rhp_walk_slot_t *slots = (rhp_walk_slot_t *) malloc(sizeof(rhp_walk_slot_t) * (nt ? nt : 1));
        rhp_walk_result_t *res = (rhp_walk_result_t *) malloc(sizeof(rhp_walk_result_t) * n);
        rhp_fieldref_t *fields = (rhp_fieldref_t *) malloc(sizeof(rhp_fieldref_t) * (size_t) nn * nt + 1);
        memset(msgs, 0xC3, sizeof(rhp_msg_t) * nt);
        memset(hdrs, 0xC3, sizeof(rhp_hdr_t) * (size_t) nt * maxh);
        memset(slots, 0xC3, sizeof(rhp_walk_slot_t) * nt);
        memset(fields, 0xC3, sizeof(rhp_fieldref_t) * (size_t) nn * nt);
        const rhp_walk_batch_t w = {buf, buf, nb + RHP_PAD, so, sl, n, nt, maxh, set_flags[s] | (deframe ? RHP_WALK_DEFRAME : 0u),
                                    msgs, hdrs, slots, res};
        if ((set_resume[s] ? rhp_cpu_walk_resume(&w, st) : rhp_cpu_walk_responses(&w)) != 0) FAIL("set %zu call %u: the walk was refused", s, c);
        for (uint32_t i = 0; i < n; i++) {
          if (res[i].n_slots != n_slots[q0 + i]) FAIL("set %zu call %u session %u: n_slots %u, the file's %u", s, c, i, res[i].n_slots, n_slots[q0 + i]);
          for (uint32_t k = res[i].n_slots; k < cap[q0 + i]; k++) {   /* not written: never read */
            const size_t at = (size_t) sl[i] + k;
            POISON(&msgs[at], sizeof msgs[at]); POISON(&slots[at], sizeof slots[at]); POISON(hdrs + at * maxh, sizeof(rhp_hdr_t) * maxh);
          }
        }
        const rhp_walk_lookup_t l = {name_text, names, nn, 0, fields};
        if (rhp_cpu_lookup_walked(&w, &l) != 0) FAIL("set %zu call %u: the lookup was refused", s, c);
        UNPOISON(msgs, sizeof(rhp_msg_t) * nt); UNPOISON(slots, sizeof(rhp_walk_slot_t) * nt); UNPOISON(hdrs, sizeof(rhp_hdr_t) * (size_t) nt * maxh);
        /* the file's present fields, then every other one absent */
        uint8_t *seen = (uint8_t *) calloc((size_t) nn * nt + 1, 1);
        for (uint32_t h = call_f[c]; h < call_f[c + 1]; h++) {
          if (f_name[h] >= nn || f_slot[h] >= nt) FAIL("set %zu call %u: field %u of the file", s, c, h);
          const size_t at = (size_t) f_name[h] * nt + f_slot[h];
          if (fields[at].value_off != f_off[h] || fields[at].value_len != f_len[h])
            FAIL("set %zu call %u (deframe %d): name %u of slot %u is {%u, %u}, the reference's {%u, %u}", s, c, deframe, f_name[h], f_slot[h],
                 fields[at].value_off, fields[at].value_len, f_off[h], f_len[h]);
          seen[at] = 1;
          present++;
        }
        for (size_t at = 0; at < (size_t) nn * nt; at++)
          if (!seen[at] && !is_absent(&fields[at]))
            FAIL("set %zu call %u (deframe %d): name %zu of slot %zu is {%u, %u}, the reference's absent", s, c, deframe, at / nt, at % nt,
                 fields[at].value_off, fields[at].value_len);
        free(seen); free(buf); free(so); free(sl); free(msgs); free(hdrs); free(slots); free(res); free(fields);
        calls_run++;
      }
      free(st);
    }
  }
  if (crafted() || refusals()) return 1;
  printf("walk_lookup_host_test OK: %zu sets, %zu calls run, %zu fields present, 12 crafted cases\n", S, calls_run, present);
  void *loaded[] = {set_maxh, set_flags, set_nsess, set_resume, set_call, set_first, states_in, set_names, name_span, name_text, call_q,
                    call_f, call_byte, bytes, len, cap, n_slots, f_slot, f_name, f_off, f_len, g_file};
  for (size_t i = 0; i < sizeof loaded / sizeof loaded[0]; i++) free(loaded[i]);
  return 0;
}
