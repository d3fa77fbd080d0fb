/*
 * walk_resume_host_test.c -- rhp_cpu_walk_resume (include/rhp_host.h) under
 * ASan/UBSan: a stand-alone program over rhp_host.cpp, rhp_emu.cpp and
 * rhp_gen.c (the `walk-resume-asan` rule of libreactorng_amd/csrc/Makefile
 * builds and runs it).
 *
 * It reads tests/golden/walk_resume.npz (argv[1], or the path from csrc/): the
 * rounds of the sets of tests/walk_resume_sets.py with the answers over the
 * compiled reference, written flat and uncompressed by
 * tests/golden/make_golden_walk_resume.py, whose header names the arrays.
 * Every set's rounds are run as a chain, the states carried from round to
 * round, with and without RHP_WALK_DEFRAME.  Every buffer is allocated at
 * exactly its documented size -- the round's bytes with their RHP_PAD, sess_off
 * and slot_off [n_sessions + 1], msgs, slots [n_slots_total], hdrs
 * [n_slots_total * max_headers], results and states [n_sessions] -- and the
 * outputs hold 0xC3 first; the sanitizer sees any access outside a buffer.
 * Then states of every kind over sess_off rows that hold anything, the
 * refusals, and the rhp_walk_resume cases of tests/golden/walk_edges.npz
 * (argv[2], or the path from csrc/), each in a block of lim + 16 <= bytes_size bytes
 * (walk_edges_host.h).  Exits non-zero on the first mismatch.
 */
#include "rhp_host.h"

#define HOST_TEST_NAME "walk_resume_host_test"
#include "host_test.h"

#include "walk_edges_host.h"

/* states of every kind over sess_off rows that hold anything, every buffer at its exact size */
static int garbage(void)
{
  static const char kTwo[] = "3\r\nabc\r\n0\r\n\r\nHTTP/1.1 200 OK\r\nTransfer-Encoding: chunked\r\n\r\n3\r\nabc\r\n0\r\n\r\nHTTP/1.1 200 OK\r\nContent-Length: 20\r\n\r\nok";
  enum { NS = 6, NT = 8, M = 2, LEN = sizeof kTwo - 1 };
  const uint64_t size = 2 * LEN + RHP_PAD;
  static const uint64_t vals[] = {0, 1, LEN, 2 * LEN, 2 * LEN + RHP_PAD, 2 * LEN + RHP_PAD - 1, ~(uint64_t) 0, (uint64_t) 1 << 63, 5, 77};
  static const uint64_t svals[] = {0, 1, NT, NT + 1, ~(uint64_t) 0, (uint64_t) 1 << 32, 4, 7};
  uint64_t seed = 12345;
  for (int trial = 0; trial < 300; trial++) {
    uint8_t *buf = (uint8_t *) calloc(1, (size_t) size);
    uint64_t *so = (uint64_t *) malloc(sizeof(uint64_t) * (NS + 1)), *sl = (uint64_t *) malloc(sizeof(uint64_t) * (NS + 1));
    rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * NT);
    rhp_hdr_t *hdrs = (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * NT * M);
    rhp_walk_slot_t *slots = (rhp_walk_slot_t *) malloc(sizeof(rhp_walk_slot_t) * NT);
    rhp_walk_result_t *res = (rhp_walk_result_t *) malloc(sizeof(rhp_walk_result_t) * NS);
    rhp_walk_state_t *st = (rhp_walk_state_t *) calloc(NS, sizeof(rhp_walk_state_t));
    memcpy(buf, kTwo, LEN);
    memcpy(buf + LEN, kTwo, LEN);
    for (int i = 0; i <= NS; i++) {
      seed = seed * 6364136223846793005ull + 1442695040888963407ull;
      so[i] = vals[(seed >> 33) % (sizeof vals / sizeof vals[0])];
      sl[i] = svals[(seed >> 45) % (sizeof svals / sizeof svals[0])];
      if (i < NS) {
        st[i].phase = (uint32_t) ((seed >> 20) % 7);
        st[i].left = vals[(seed >> 12) % (sizeof vals / sizeof vals[0])];
        st[i].decoder.state = (uint8_t) ((seed >> 8) % 7);
        st[i].decoder.hex_count = (uint8_t) ((seed >> 4) % 18);
        st[i].decoder.consume_trailer = (uint8_t) (seed & 1);
        st[i].decoder.bytes_left_in_chunk = vals[(seed >> 16) % (sizeof vals / sizeof vals[0])];
      }
    }
    const rhp_walk_batch_t w = {buf, buf, size, so, sl, NS, NT, M, (uint32_t) (trial & 7), msgs, hdrs, slots, res};
    for (int round = 0; round < 2; round++) {
      if (rhp_cpu_walk_resume(&w, st) != 0) FAIL("garbage trial %d: refused", trial);
      for (int s = 0; s < NS; s++) {
        const int owns = sl[s] <= sl[s + 1] && sl[s + 1] <= NT;
        if (res[s].stop > RHP_WALK_MORE || res[s].n_slots > (owns ? sl[s + 1] - sl[s] : 0))
          FAIL("garbage trial %d session %d: n_slots %u stop %u", trial, s, res[s].n_slots, res[s].stop);
      }
    }
    free(buf); free(so); free(sl); free(msgs); free(hdrs); free(slots); free(res); free(st);
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
  rhp_walk_state_t st;
  memset(&st, 0, sizeof st);
  const rhp_walk_batch_t ok = {bytes, bytes, 512, so, sl, 1, 1, 4, 0, &m, h, &x, &r};
  if (rhp_cpu_walk_resume(&ok, &st) != 0) FAIL("a sound call was refused");
  if (rhp_cpu_walk_resume(&ok, NULL) != -22) FAIL("NULL states accepted");
  if (rhp_cpu_walk_resume(NULL, &st) != -22) FAIL("NULL batch accepted");
  rhp_walk_batch_t b = ok;
  b.flags = 8;
  if (rhp_cpu_walk_resume(&b, &st) != -22) FAIL("an unknown flag accepted");
  b = ok;
  b.results = NULL;
  if (rhp_cpu_walk_resume(&b, &st) != -22) FAIL("NULL results accepted");
  b = ok;
  b.n_sessions = 0;
  if (rhp_cpu_walk_resume(&b, NULL) != 0) FAIL("an empty call needs no states");
  free(bytes);
  return 0;
}

int main(int argc, char **argv)
{
  const char *path = argc > 1 ? argv[1] : "../../tests/golden/walk_resume.npz";
  if (npz_open(path)) return 1;
  LOAD(set_maxh, uint32_t, "<u4"); LOAD(set_flags, uint32_t, "<u4"); LOAD(set_nsess, uint32_t, "<u4");
  LOAD(set_round, uint32_t, "<u4"); LOAD(set_first, uint32_t, "<u4"); LOAD(states_in, uint8_t, "|u1");
  LOAD(round_q, uint32_t, "<u4"); LOAD(round_slot, uint32_t, "<u4"); LOAD(round_byte, uint64_t, "<u8");
  LOAD(bytes, uint8_t, "|u1"); LOAD(defr_idx, uint32_t, "<u4"); LOAD(defr_val, uint8_t, "|u1");
  LOAD(len, uint32_t, "<u4"); LOAD(cap, uint8_t, "|u1"); LOAD(n_slots, uint8_t, "|u1"); LOAD(stop, uint8_t, "|u1");
  LOAD(consumed, uint32_t, "<u4"); LOAD(kept, uint8_t, "|u1"); LOAD(st_phase, uint8_t, "|u1"); LOAD(st_ct, uint8_t, "|u1");
  LOAD(st_hex, uint8_t, "|u1"); LOAD(st_state, uint8_t, "|u1"); LOAD(st_left, uint64_t, "<u8");
  LOAD(start, uint32_t, "<u4"); LOAD(body_len, uint64_t, "<u8"); LOAD(wire_len, uint32_t, "<u4"); LOAD(result, int8_t, "|i1");
  LOAD(body_kind, uint8_t, "|u1"); LOAD(ret, int32_t, "<i4");
  const size_t S = n_set_maxh;
  if (n_set_round != S + 1 || n_set_first != S + 1 || n_len != n_stop || n_start != n_ret || n_defr_idx != n_defr_val) FAIL("%s: sizes", path);
  uint8_t *deframed = (uint8_t *) malloc(n_bytes ? n_bytes : 1);
  memcpy(deframed, bytes, n_bytes);
  for (size_t i = 0; i < n_defr_idx; i++) deframed[defr_idx[i]] = defr_val[i];
  size_t rounds_run = 0;
  for (size_t s = 0; s < S; s++) {
    const uint32_t n = set_nsess[s], maxh = set_maxh[s];
    for (int deframe = 0; deframe < 2; deframe++) {
      rhp_walk_state_t *st = (rhp_walk_state_t *) calloc(n ? n : 1, sizeof(rhp_walk_state_t));
      rhp_walk_state_t *in = (rhp_walk_state_t *) calloc(n ? n : 1, sizeof(rhp_walk_state_t));
      if (set_first[s + 1] > set_first[s]) memcpy(st, states_in + 32 * (size_t) set_first[s], 32 * (size_t) n);
      for (uint32_t r = set_round[s]; r < set_round[s + 1]; r++) {
        const size_t q0 = round_q[r], nb = (size_t) (round_byte[r + 1] - round_byte[r]);
        if (round_q[r + 1] - q0 != n) FAIL("set %zu round %u: sessions", s, r);
        uint8_t *buf = (uint8_t *) calloc(1, nb + RHP_PAD);
        memcpy(buf, bytes + round_byte[r], nb);
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
        memset(msgs, 0xC3, sizeof(rhp_msg_t) * nt);
        memset(hdrs, 0xC3, sizeof(rhp_hdr_t) * (size_t) nt * maxh);
        memset(slots, 0xC3, sizeof(rhp_walk_slot_t) * nt);
        memset(res, 0xC3, sizeof(rhp_walk_result_t) * n);
        memcpy(in, st, sizeof(rhp_walk_state_t) * n);
        const rhp_walk_batch_t w = {buf, buf, nb + RHP_PAD, so, sl, n, nt, maxh, set_flags[s] | (deframe ? RHP_WALK_DEFRAME : 0u),
                                    msgs, hdrs, slots, res};
        if (rhp_cpu_walk_resume(&w, st) != 0) FAIL("set %zu round %u: refused", s, r);
        size_t t = round_slot[r];
        for (uint32_t i = 0; i < n; i++) {
          const size_t q = q0 + i;
          if (res[i].n_slots != n_slots[q] || res[i].stop != stop[q] || res[i].consumed != consumed[q])
            FAIL("set %zu round %u session %u: result (%u, %u, %llu), the reference's (%u, %u, %u)", s, r, i, res[i].n_slots, res[i].stop,
                 (unsigned long long) res[i].consumed, n_slots[q], stop[q], consumed[q]);
          for (uint32_t k = 0; k < cap[q]; k++) {
            const size_t at = (size_t) sl[i] + k;
            if (k >= n_slots[q]) {
              if (!all_poison(&slots[at], sizeof slots[at]) || !all_poison(&msgs[at], sizeof msgs[at]) || !all_poison(hdrs + at * maxh, sizeof(rhp_hdr_t) * maxh))
                FAIL("set %zu round %u session %u: a record past n_slots was written", s, r, i);
              continue;
            }
            const rhp_walk_slot_t *x = &slots[at];
            if (x->start != start[t] || x->body_len != body_len[t] || x->wire_len != wire_len[t] || x->result != result[t] ||
                x->body_kind != body_kind[t] || msgs[at].ret != ret[t])
              FAIL("set %zu round %u session %u slot %u differs from the reference's", s, r, i, k);
            t++;
          }
          const rhp_walk_state_t want = state_of(kept, st_phase, st_ct, st_hex, st_state, st_left, q, in[i]);
          if (memcmp(&st[i], &want, sizeof want) != 0) FAIL("set %zu round %u session %u: the state differs from the reference's", s, r, i);
        }
        if (t != round_slot[r + 1]) FAIL("set %zu round %u: slots", s, r);
        if (memcmp(buf, (deframe ? deframed : bytes) + round_byte[r], nb) != 0) FAIL("set %zu round %u (deframe %d): the bytes differ", s, r, deframe);
        for (size_t i = nb; i < nb + RHP_PAD; i++) if (buf[i]) FAIL("set %zu round %u: the pad was written", s, r);
        free(buf); free(so); free(sl); free(msgs); free(hdrs); free(slots); free(res);
        rounds_run++;
      }
      free(st); free(in);
    }
  }
  size_t edge_cases = 0;
  if (garbage() || refusals() || walk_edges(argc > 2 ? argv[2] : "../../tests/golden/walk_edges.npz", 1, &edge_cases)) return 1;
  printf("walk_resume_host_test OK: %zu sets, %zu rounds run, %zu cases at the readable end\n", S, rounds_run, edge_cases);
  free(deframed);
  void *loaded[] = {set_maxh, set_flags, set_nsess, set_round, set_first, states_in, round_q, round_slot, round_byte, bytes, defr_idx, defr_val,
                    len, cap, n_slots, stop, consumed, kept, st_phase, st_ct, st_hex, st_state, st_left, start, body_len, wire_len, result,
                    body_kind, ret, g_file};
  for (size_t i = 0; i < sizeof loaded / sizeof loaded[0]; i++) free(loaded[i]);
  return 0;
}
