/*
 * walk_edges_host.h -- the cases of tests/golden/walk_edges.npz for the two
 * stand-alone host programs (walk_responses_host_test.c, walk_resume_host_test.c),
 * which include it behind host_test.h (npz_open, LOAD, FAIL and all_poison).
 *
 * The file (tests/golden/make_golden_walk_edges.py names its arrays) holds calls
 * whose bytes_size puts the readable end at every byte of a session's last
 * message, with walkable text lying beyond.  Here every case of one call runs
 * with its bytes copied into a heap block of lim + 16 bytes, lim the readable
 * end (rhp_walk_args.h) -- never more than bytes_size, which the call states as
 * the file has it -- so a read at or beyond bytes + lim + 16, and so any at or
 * beyond bytes + bytes_size, is a sanitizer report: the twin's reader has to
 * see zeros from lim on without looking.  The answers do not depend on what
 * lies beyond, so the file's expectations hold as they are: results, slots,
 * message and header records, states and bytes.
 * With and without RHP_WALK_DEFRAME; every other buffer at its exact size, the
 * outputs 0xC3 first.
 */
static int walk_edges(const char *path, int which, size_t *cases_run)   /* which: 0 rhp_cpu_walk_responses, 1 rhp_cpu_walk_resume */
{
  uint8_t *const old_file = g_file;
  const size_t old_size = g_size;
  if (npz_open(path)) return 1;   /* a second file: the program's own is put back at the end */
  LOAD(kind_state, uint8_t, "|u1"); LOAD(max_headers, uint32_t, "<u4"); LOAD(flags, uint32_t, "<u4"); LOAD(slot_off, uint64_t, "<u8");
  LOAD(lead, uint8_t, "|u1"); LOAD(tail, uint8_t, "|u1"); LOAD(tail_sess, uint32_t, "<u4"); LOAD(buf_kind, uint8_t, "|u1");
  LOAD(buf_byte, uint32_t, "<u4"); LOAD(buf_a, uint16_t, "<u2"); LOAD(mid, uint8_t, "|u1");
  LOAD(call, uint8_t, "|u1"); LOAD(case_buf, uint16_t, "<u2"); LOAD(lim, uint32_t, "<u4"); LOAD(size, uint32_t, "<u4");
  LOAD(case_slot, uint32_t, "<u4"); LOAD(case_defr, uint32_t, "<u4"); LOAD(defr_idx, uint16_t, "<u2"); LOAD(defr_val, uint8_t, "|u1");
  LOAD(n_slots, uint8_t, "|u1"); LOAD(stop, uint8_t, "|u1"); LOAD(consumed, uint16_t, "<u2"); LOAD(kept, uint8_t, "|u1");
  LOAD(st_phase, uint8_t, "|u1"); LOAD(st_ct, uint8_t, "|u1"); LOAD(st_hex, uint8_t, "|u1"); LOAD(st_state, uint8_t, "|u1");
  LOAD(st_left, uint32_t, "<u4");
  LOAD(start, uint16_t, "<u2"); LOAD(body_len, uint32_t, "<u4"); LOAD(wire_len, uint16_t, "<u2"); LOAD(result, int8_t, "|i1");
  LOAD(body_kind, uint8_t, "|u1"); LOAD(ret, int16_t, "<i2"); LOAD(status, uint16_t, "<u2"); LOAD(msg_off, uint16_t, "<u2");
  LOAD(msg_len, uint16_t, "<u2"); LOAD(minor, int8_t, "|i1"); LOAD(num_headers, uint8_t, "|u1"); LOAD(hdr, uint16_t, "<u2");
  enum { NS = 4 };
  const size_t N = n_call, B = n_buf_kind;
  if (n_slot_off != NS + 1 || n_tail_sess != 2 || n_buf_byte != B + 1 || n_buf_a != B || n_case_buf != N || n_lim != N || n_size != N ||
      n_case_slot != N + 1 || n_case_defr != N + 1 || n_n_slots != NS * N || n_stop != NS * N || n_consumed != NS * N || n_kept != NS * N ||
      n_st_left != NS * N || n_start != case_slot[N] || n_ret != n_start || n_defr_idx != case_defr[N] || n_defr_val != n_defr_idx ||
      n_status != n_start || n_msg_off != n_start || n_msg_len != n_start || n_minor != n_start || n_num_headers != n_start ||
      n_max_headers != 1 || n_flags != 1 || max_headers[0] == 0)
    FAIL("%s: the arrays' sizes do not fit each other", path);
  const uint32_t nt = (uint32_t) slot_off[NS], maxh = max_headers[0];
  uint32_t *hdr_lo = (uint32_t *) calloc(n_start + 1, sizeof(uint32_t));   /* slot t's header records: hdr[hdr_lo[t], hdr_lo[t + 1]) */
  for (size_t t = 0; t < n_start; t++) hdr_lo[t + 1] = hdr_lo[t] + (ret[t] > 0 ? num_headers[t] : 0u);
  if (n_hdr != 4u * (size_t) hdr_lo[n_start]) FAIL("%s: the header records do not fit the slots", path);
  *cases_run = 0;
  for (size_t i = 0; i < N; i++) {
    if (call[i] != which) continue;
    const size_t b = case_buf[i], ml = buf_byte[b + 1] - buf_byte[b], full = n_lead + ml + n_tail + RHP_PAD;
    if (b >= B || size[i] > full || size[i] < RHP_PAD || lim[i] != (size[i] & ~15u) - 16u) FAIL("%s case %zu: sizes", path, i);
    uint8_t *whole = (uint8_t *) calloc(1, full), *after = (uint8_t *) malloc(full);
    memcpy(whole, lead, n_lead);
    memcpy(whole + n_lead, mid + buf_byte[b], ml);
    memcpy(whole + n_lead + ml, tail, n_tail);
    memcpy(after, whole, full);
    for (size_t d = case_defr[i]; d < case_defr[i + 1]; d++) {
      if (defr_idx[d] >= lim[i]) FAIL("%s case %zu: a byte at or behind the readable end is de-framed", path, i);
      after[defr_idx[d]] = defr_val[d];
    }
    uint64_t so[NS + 1] = {n_lead + buf_a[b], n_lead + buf_a[b], n_lead + ml, n_lead + ml + tail_sess[0], n_lead + ml + tail_sess[0] + tail_sess[1]};
    for (uint32_t deframe = 0; deframe <= RHP_WALK_DEFRAME; deframe += RHP_WALK_DEFRAME) {
      const size_t block = (size_t) lim[i] + 16;    /* <= bytes_size: the text beyond is not there */
      uint8_t *buf = (uint8_t *) malloc(block);
      uint64_t *sop = (uint64_t *) malloc(sizeof so), *sl = (uint64_t *) malloc(sizeof(uint64_t) * (NS + 1));
      rhp_msg_t *msgs = (rhp_msg_t *) malloc(sizeof(rhp_msg_t) * nt);
      rhp_hdr_t *hdrs = (rhp_hdr_t *) malloc(sizeof(rhp_hdr_t) * (size_t) nt * maxh);
      rhp_walk_slot_t *slots = (rhp_walk_slot_t *) malloc(sizeof(rhp_walk_slot_t) * nt);
      rhp_walk_result_t *res = (rhp_walk_result_t *) malloc(sizeof(rhp_walk_result_t) * NS);
      rhp_walk_state_t *st = (rhp_walk_state_t *) calloc(NS, sizeof(rhp_walk_state_t)), in[NS];
      memcpy(buf, whole, block);
      memcpy(sop, so, sizeof so);
      memcpy(sl, slot_off, sizeof(uint64_t) * (NS + 1));
      memset(msgs, 0xC3, sizeof(rhp_msg_t) * nt);
      memset(hdrs, 0xC3, sizeof(rhp_hdr_t) * (size_t) nt * maxh);
      memset(slots, 0xC3, sizeof(rhp_walk_slot_t) * nt);
      memset(res, 0xC3, sizeof(rhp_walk_result_t) * NS);
      if (call[i] == 1) memcpy(&st[1], kind_state + 32 * (size_t) buf_kind[b], 32);
      memcpy(in, st, sizeof in);
      const rhp_walk_batch_t w = {buf, buf, size[i], sop, sl, NS, nt, maxh, flags[0] | deframe, msgs, hdrs, slots, res};
      if ((call[i] == 1 ? rhp_cpu_walk_resume(&w, st) : rhp_cpu_walk_responses(&w)) != 0) FAIL("%s case %zu: refused", path, i);
      size_t t = case_slot[i];
      for (uint32_t s = 0; s < NS; s++) {
        const size_t q = NS * i + s;
        if (res[s].n_slots != n_slots[q] || res[s].stop != stop[q] || res[s].consumed != consumed[q])
          FAIL("%s case %zu session %u: result (%u, %u, %llu), the reference's (%u, %u, %u)", path, i, s, res[s].n_slots, res[s].stop,
               (unsigned long long) res[s].consumed, n_slots[q], stop[q], consumed[q]);
        for (uint64_t k = sl[s]; k < sl[s + 1]; k++) {
          if (k - sl[s] >= n_slots[q]) {
            if (!all_poison(&slots[k], sizeof slots[k]) || !all_poison(&msgs[k], sizeof msgs[k]) || !all_poison(hdrs + k * maxh, sizeof(rhp_hdr_t) * maxh))
              FAIL("%s case %zu session %u: a record past n_slots was written", path, i, s);
            continue;
          }
          const rhp_walk_slot_t *x = &slots[k];
          if (x->start != start[t] || x->body_len != body_len[t] || x->wire_len != wire_len[t] || x->result != result[t] ||
              x->body_kind != body_kind[t] || msgs[k].ret != ret[t])
            FAIL("%s case %zu session %u slot %llu differs from the reference's", path, i, s, (unsigned long long) (k - sl[s]));
          if (ret[t] > 0) {
            const rhp_msg_t *m = &msgs[k];
            if (m->status != status[t] || m->msg_off != msg_off[t] || m->msg_len != msg_len[t] || m->minor_version != minor[t] ||
                m->num_headers != num_headers[t] || m->reserved != 0 || m->flags != 0)
              FAIL("%s case %zu session %u slot %llu: the message record differs", path, i, s, (unsigned long long) (k - sl[s]));
            for (uint32_t j = 0; j < num_headers[t]; j++) {
              const uint16_t *e = hdr + 4u * (hdr_lo[t] + j);
              const rhp_hdr_t r = hdrs[k * maxh + j];
              if (r.name_off != e[0] || r.name_len != e[1] || r.value_off != e[2] || r.value_len != e[3])
                FAIL("%s case %zu session %u slot %llu header %u: the record differs", path, i, s, (unsigned long long) (k - sl[s]), j);
            }
          } else if (ret[t] == 0 && result[t] == 1) {   /* a continuation: sixteen zero bytes, no header record */
            static const uint8_t zero[sizeof(rhp_msg_t)];
            if (memcmp(&msgs[k], zero, sizeof zero) != 0 || !all_poison(hdrs + k * maxh, sizeof(rhp_hdr_t) * maxh))
              FAIL("%s case %zu session %u slot %llu: the continuation's records", path, i, s, (unsigned long long) (k - sl[s]));
          }
          t++;
        }
        if (call[i] == 1) {
          rhp_walk_state_t want = in[s];
          if (!kept[q]) {
            memset(&want, 0, sizeof want);
            want.phase = st_phase[q];
            if (want.phase == RHP_WALK_IN_LENGTH) want.left = st_left[q];
            if (want.phase == RHP_WALK_IN_CHUNKED) want.decoder.bytes_left_in_chunk = st_left[q];
            want.decoder.consume_trailer = st_ct[q];
            want.decoder.hex_count = st_hex[q];
            want.decoder.state = st_state[q];
          }
          if (memcmp(&st[s], &want, sizeof want) != 0) FAIL("%s case %zu session %u: the state differs from the reference's", path, i, s);
        }
      }
      if (t != case_slot[i + 1]) FAIL("%s case %zu: slots", path, i);
      if (memcmp(buf, deframe ? after : whole, lim[i]) != 0) FAIL("%s case %zu (deframe %u): the bytes below the readable end differ", path, i, deframe);
      if (memcmp(buf + lim[i], whole + lim[i], block - lim[i]) != 0) FAIL("%s case %zu: a byte at or behind the readable end was written", path, i);
      free(buf); free(sop); free(sl); free(msgs); free(hdrs); free(slots); free(res); free(st);
    }
    free(whole); free(after);
    ++*cases_run;
  }
  void *loaded[] = {kind_state, max_headers, flags, slot_off, lead, tail, tail_sess, buf_kind, buf_byte, buf_a, mid, call, case_buf, lim, size,
                    case_slot, case_defr, defr_idx, defr_val, n_slots, stop, consumed, kept, st_phase, st_ct, st_hex, st_state, st_left,
                    start, body_len, wire_len, result, body_kind, ret, status, msg_off, msg_len, minor, num_headers, hdr, hdr_lo, g_file};
  for (size_t i = 0; i < sizeof loaded / sizeof loaded[0]; i++) free(loaded[i]);
  g_file = old_file;
  g_size = old_size;
  return *cases_run ? 0 : 1;
}
