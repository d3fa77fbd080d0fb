/*
 * walk_responses_host_test.c -- rhp_cpu_walk_responses (include/rhp_host.h)
 * under ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and
 * rhp_gen.c (the `walk-responses-asan` rule of libreactorng_amd/csrc/Makefile
 * builds and runs it).
 *
 * It reads tests/golden/walk_responses.npz (argv[1], or the path from csrc/):
 * the sets of tests/walk_sets.py with the walk's answers over the compiled
 * reference, written flat and uncompressed by tests/golden/make_golden_walk.py,
 * whose header names the arrays.  Every set is walked with and without
 * RHP_WALK_DEFRAME.  Every buffer is allocated at exactly its documented size
 * -- the set's bytes with their RHP_PAD, sess_off and slot_off [n_sessions + 1],
 * msgs, slots [n_slots_total], hdrs [n_slots_total * max_headers], results
 * [n_sessions] -- and the outputs hold 0xC3 first; the sanitizer sees any access
 * outside a buffer.  Then sess_off and slot_off rows that hold anything, and
 * the refusals.  Exits non-zero on the first mismatch.
 */
#include "rhp_host.h"

#define HOST_TEST_NAME "walk_responses_host_test"
#include "host_test.h"

#include "walk_edges_host.h"

/* sess_off and slot_off rows that hold anything, every buffer at its exact size */
static int garbage(void)
{
  static const char kTwo[] = "HTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n3\r\nabc\r\n0\r\n\r\nHTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\nok";
  enum { NS = 6, NT = 8, M = 2, LEN = sizeof kTwo - 1 };
  const uint64_t size = 2 * LEN + RHP_PAD;
  static const uint64_t vals[] = {0, 1, LEN, 2 * LEN, 2 * LEN + RHP_PAD, 2 * LEN + RHP_PAD - 1, ~(uint64_t) 0, (uint64_t) 1 << 63, 5, 77};
  static const uint64_t svals[] = {0, 1, NT, NT + 1, ~(uint64_t) 0, (uint64_t) 1 << 32, 4, 7};
  uint64_t seed = 12345;
  for (int trial = 0; trial < 200; trial++) {
    uint8_t *buf = (uint8_t *) calloc(1, (size_t) size);
    uint64_t *so = (uint64_t *) malloc(sizeof(uint64_t) * (NS + 1)), *sl = (uint64_t *) malloc(sizeof(uint64_t) * (NS + 1));
    rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * NT);
    rhp_hdr_t *hdrs = (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * NT * M);
    rhp_walk_slot_t *slots = (rhp_walk_slot_t *) malloc(sizeof(rhp_walk_slot_t) * NT);
    rhp_walk_result_t *res = (rhp_walk_result_t *) malloc(sizeof(rhp_walk_result_t) * NS);
    memcpy(buf, kTwo, LEN);
    memcpy(buf + LEN, kTwo, LEN);
    for (int i = 0; i <= NS; i++) {
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      so[i] = vals[(seed >> 33) % (sizeof vals / sizeof vals[0])];
      sl[i] = svals[(seed >> 45) % (sizeof svals / sizeof svals[0])];
    }
    const rhp_walk_batch_t w = {buf, buf, size, so, sl, NS, NT, M, (uint32_t) (trial & 7), msgs, hdrs, slots, res};
    if (rhp_cpu_walk_responses(&w) != 0) FAIL("garbage trial %d: refused", trial);
    for (int s = 0; s < NS; s++) {
      const int owns = sl[s] <= sl[s + 1] && sl[s + 1] <= NT;
      if (res[s].stop > RHP_WALK_MORE || res[s].n_slots > (owns ? sl[s + 1] - sl[s] : 0))
        FAIL("garbage trial %d session %d: n_slots %u stop %u", trial, s, res[s].n_slots, res[s].stop);
    }
    free(buf); free(so); free(sl); free(msgs); free(hdrs); free(slots); free(res);
  }
  return 0;
}

static int refusals(void)
{
  uint8_t *bytes = (uint8_t *) calloc(1, 512);
  uint64_t so[2] = {0, 0}, sl[2] = {0, 1};
  rhp_msg_t m;
  rhp_hdr_t h[4];
  rhp_walk_slot_t x;
  rhp_walk_result_t r;
  memset(&m, 0x77, sizeof m);
  memset(&x, 0x77, sizeof x);
  memset(&r, 0x77, sizeof r);
  const rhp_walk_batch_t ok = {bytes, bytes, 512, so, sl, 1, 1, 4, RHP_WALK_DEFRAME, &m, h, &x, &r};
  rhp_walk_batch_t w;
  if (rhp_cpu_walk_responses(NULL) != -22) FAIL("a NULL batch is refused");
#define REFUSED(change, what) do { w = ok; change; if (rhp_cpu_walk_responses(&w) != -22) FAIL("refusal: %s", what); } while (0)
  REFUSED(w.bytes = NULL, "NULL bytes");
  REFUSED(w.bytes_rw = NULL, "RHP_WALK_DEFRAME without bytes_rw");
  REFUSED(w.bytes_rw = bytes + 1, "bytes_rw that is not bytes");
  REFUSED(w.sess_off = NULL, "NULL sess_off");
  REFUSED(w.slot_off = NULL, "NULL slot_off");
  REFUSED(w.results = NULL, "NULL results");
  REFUSED(w.msgs = NULL, "NULL msgs");
  REFUSED(w.slots = NULL, "NULL slots");
  REFUSED(w.hdrs = NULL, "NULL hdrs with max_headers > 0");
  REFUSED(w.max_headers = RHP_MAX_HEADERS + 1, "max_headers");
  REFUSED(w.flags = 8, "an unknown flag");
  REFUSED(w.bytes_size = RHP_PAD - 1, "bytes_size below RHP_PAD");
  REFUSED((w.n_slots_total = 0xffffffffu, w.max_headers = 2), "n_slots_total * max_headers >= 2^32");
  REFUSED((w.n_sessions = 0, w.flags = 16), "the rules come before the empty call");
  if (m.ret != 0x77777777 || x.result != 0x77777777 || r.stop != 0x77777777u) FAIL("a refused call writes nothing");
  w = ok;
  w.n_sessions = 0;
  w.sess_off = NULL;
  if (rhp_cpu_walk_responses(&w) != 0 || r.stop != 0x77777777u) FAIL("no session succeeds and writes nothing");
  if (rhp_cpu_walk_responses(&ok) != 0 || r.n_slots != 0 || r.stop != RHP_WALK_END || r.consumed != 0 || x.result != 0x77777777)
    FAIL("an empty session: no slot, RHP_WALK_END");
  free(bytes);
  return 0;
}

int main(int argc, char **argv)
{
  const char *path = argc > 1 ? argv[1] : "../../tests/golden/walk_responses.npz";
  if (npz_open(path)) return 1;

  LOAD(set_maxh, uint32_t, "'<u4'");
  LOAD(set_flags, uint32_t, "'<u4'");
  LOAD(set_sess, uint32_t, "'<u4'");
  LOAD(set_slot, uint32_t, "'<u4'");
  LOAD(set_byte, uint64_t, "'<u8'");
  LOAD(bytes, uint8_t, "'|u1'");
  LOAD(deframed, uint8_t, "'|u1'");
  LOAD(sess_off, uint64_t, "'<u8'");
  LOAD(slot_off, uint64_t, "'<u8'");
  LOAD(n_slots, uint32_t, "'<u4'");
  LOAD(stop, uint32_t, "'<u4'");
  LOAD(consumed, uint64_t, "'<u8'");
  LOAD(written, uint8_t, "'|u1'");
  LOAD(start, uint64_t, "'<u8'");
  LOAD(body_len, uint64_t, "'<u8'");
  LOAD(wire_len, uint64_t, "'<u8'");
  LOAD(result, int32_t, "'<i4'");
  LOAD(body_kind, uint32_t, "'<u4'");
  LOAD(ret, int32_t, "'<i4'");
  LOAD(status, int32_t, "'<i4'");
  LOAD(num_headers, int32_t, "'<i4'");
  LOAD(hdr_lo, uint32_t, "'<u4'");
  LOAD(hdr, uint16_t, "'<u2'");
  const size_t S = n_set_maxh, NS = n_n_slots, NT = n_written;
  if (!S || n_set_flags != S || n_set_sess != S + 1 || n_set_slot != S + 1 || n_set_byte != S + 1 || set_sess[S] != NS ||
      set_slot[S] != NT || set_byte[S] != n_bytes || n_deframed != n_bytes || n_sess_off != NS + S || n_slot_off != NS + S ||
      n_stop != NS || n_consumed != NS || n_start != NT || n_body_len != NT || n_wire_len != NT || n_result != NT ||
      n_body_kind != NT || n_ret != NT || n_status != NT || n_num_headers != NT || n_hdr_lo != NT + 1 || n_hdr != 4u * hdr_lo[NT])
    FAIL("%s: the arrays' sizes do not fit each other", path);

  size_t calls = 0, compared = 0, moved = 0;
  for (size_t s = 0; s < S; s++) {
    const uint32_t lo = set_sess[s], ns = set_sess[s + 1] - lo, tl = set_slot[s], nt = set_slot[s + 1] - tl, maxh = set_maxh[s];
    const size_t blen = (size_t) (set_byte[s + 1] - set_byte[s]);
    for (uint32_t deframe = 0; deframe <= RHP_WALK_DEFRAME; deframe += RHP_WALK_DEFRAME) {
      uint8_t *buf = (uint8_t *) malloc(blen);
      uint64_t *so = (uint64_t *) malloc(sizeof(uint64_t) * (ns + 1u)), *sl = (uint64_t *) malloc(sizeof(uint64_t) * (ns + 1u));
      rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * nt);
      rhp_hdr_t *hdrs = maxh ? (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * nt * maxh) : NULL;
      rhp_walk_slot_t *slots = (rhp_walk_slot_t *) malloc(sizeof(rhp_walk_slot_t) * nt);
      rhp_walk_result_t *res = (rhp_walk_result_t *) malloc(sizeof(rhp_walk_result_t) * ns);
      memcpy(buf, bytes + set_byte[s], blen);
      memcpy(so, sess_off + lo + s, sizeof(uint64_t) * (ns + 1u));
      memcpy(sl, slot_off + lo + s, sizeof(uint64_t) * (ns + 1u));
      if (so[ns] + RHP_PAD > blen || sl[ns] != nt) FAIL("set %zu: no pad behind the sessions, or another slot count", s);
      memset(msgs, 0xC3, sizeof(rhp_msg_t) * nt);
      if (hdrs) memset(hdrs, 0xC3, sizeof(rhp_hdr_t) * nt * maxh);
      memset(slots, 0xC3, sizeof(rhp_walk_slot_t) * nt);
      memset(res, 0xC3, sizeof(rhp_walk_result_t) * ns);
      const rhp_walk_batch_t w = {buf, deframe ? buf : NULL, blen, so, sl, ns, nt, maxh, set_flags[s] | deframe, msgs, hdrs, slots, res};
      if (rhp_cpu_walk_responses(&w) != 0) FAIL("set %zu: refused", s);
      for (uint32_t i = 0; i < ns; i++)
        if (res[i].n_slots != n_slots[lo + i] || res[i].stop != stop[lo + i] || res[i].consumed != consumed[lo + i])
          FAIL("set %zu session %u: result (%u, %u, %llu), the reference's (%u, %u, %llu)", s, i, res[i].n_slots, res[i].stop,
               (unsigned long long) res[i].consumed, n_slots[lo + i], stop[lo + i], (unsigned long long) consumed[lo + i]);
      for (uint32_t k = 0; k < nt; k++) {
        const size_t g = tl + k;
        if (!written[g]) {
          if (!all_poison(&slots[k], sizeof slots[k]) || !all_poison(&msgs[k], sizeof msgs[k]) ||
              (hdrs && !all_poison(hdrs + (size_t) k * maxh, sizeof(rhp_hdr_t) * maxh)))
            FAIL("set %zu slot %u: written past n_slots", s, k);
          continue;
        }
        if (slots[k].start != start[g] || slots[k].body_len != body_len[g] || slots[k].wire_len != wire_len[g] ||
            slots[k].result != result[g] || slots[k].body_kind != body_kind[g] || msgs[k].ret != ret[g])
          FAIL("set %zu slot %u: (%llu, %llu, %llu, %d, %u; ret %d) differs from the reference's", s, k, (unsigned long long) slots[k].start,
               (unsigned long long) slots[k].body_len, (unsigned long long) slots[k].wire_len, slots[k].result, slots[k].body_kind, msgs[k].ret);
        if (ret[g] > 0) {
          if (msgs[k].status != status[g] || msgs[k].num_headers != num_headers[g] || hdr_lo[g + 1] - hdr_lo[g] != (uint32_t) num_headers[g])
            FAIL("set %zu slot %u: the message record differs", s, k);
          for (uint32_t j = 0; j < (uint32_t) num_headers[g]; j++) {
            const uint16_t *e = hdr + 4u * (hdr_lo[g] + j);
            const rhp_hdr_t r = hdrs[(size_t) k * maxh + j];
            if (r.name_off != e[0] || r.name_len != e[1] || r.value_off != e[2] || r.value_len != e[3])
              FAIL("set %zu slot %u header %u: the record differs", s, k, j);
          }
        }
        compared++;
      }
      const uint8_t *want = (deframe ? deframed : bytes) + set_byte[s];
      for (size_t q = 0; q < blen; q++) {
        if (buf[q] != want[q]) FAIL("set %zu deframe %u: byte %zu is %u, not %u", s, deframe, q, buf[q], want[q]);
        moved += deframe && buf[q] != bytes[set_byte[s] + q];
      }
      calls++;
      free(buf); free(so); free(sl); free(msgs); free(hdrs); free(slots); free(res);
    }
  }
  size_t edge_cases = 0;
  if (garbage() || refusals() || walk_edges(argc > 2 ? argv[2] : "../../tests/golden/walk_edges.npz", 0, &edge_cases)) return 1;
  free(set_maxh); free(set_flags); free(set_sess); free(set_slot); free(set_byte); free(bytes); free(deframed); free(sess_off);
  free(slot_off); free(n_slots); free(stop); free(consumed); free(written); free(start); free(body_len); free(wire_len); free(result);
  free(body_kind); free(ret); free(status); free(num_headers); free(hdr_lo); free(hdr); free(g_file);
  printf("walk_responses_host_test OK: %zu sets, %zu sessions, %zu calls, %zu slots compared, %zu bytes moved by the de-framing, "
         "%zu cases at the readable end\n", S, NS, calls, compared, moved, edge_cases);
  return 0;
}
