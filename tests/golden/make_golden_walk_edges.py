#!/usr/bin/env python3
"""Writes tests/golden/walk_edges.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every case of tests/walk_edge_sets.py -- a call of rhp_walk_responses or
rhp_walk_resume whose bytes_size puts the readable end, lim, at every byte of
a session's last message -- the expected answers are what rhp.h says such a
call is: the plain walk over the clamped view.  The clamped view is the case's
buffer with zeros from lim on and the offsets min(sess_off, lim), and the walk
over it is make_golden_walk.walker / make_golden_walk_resume.round_walker, the
walks in plain Python whose every parse, lookup, number and chunked decode is
the compiled reference's.  The view is as long as the buffer, so the reference
reads zeros, never anything outside it, behind lim.

The file is flat, so that the stand-alone C tests (tests/walk_responses_host_test.c,
tests/walk_resume_host_test.c) read it as well: np.savez, not compressed, narrow
columns.  K kinds, B buffers, N cases, NT written slots (only the slots a session
wrote are held, case after case in session order).
  kind_name str [K]      kind_state u8 [K * 32]: the rhp_walk_state_t of the session under test before a resume case
  max_headers, flags u32 [1]   slot_off u64 [5]: the same in every case
  lead u8: the bytes every buffer starts with     tail u8: the bytes every buffer ends with, before RHP_PAD zero bytes
  tail_sess u32 [2]: the lengths of the two planted sessions at the tail's start
  buf_kind, buf_pad u8 [B]   buf_byte u32 [B + 1]: buffer b is lead + mid[buf_byte[b], buf_byte[b + 1]) + tail + the pad
  buf_a u16 [B]: the session under test is the last bytes of that piece, from its byte buf_a[b] on (before it: what
                 closes the lead); sess_off = len(lead) + (buf_a, buf_a, piece length, + tail_sess[0], + tail_sess[1])
  mid u8
  per case: call u8 (0 rhp_walk_responses, 1 rhp_walk_resume), case_buf u16, c i16, lim u32, size u32 (bytes_size)
            case_slot u32 [N + 1]: its written slots     case_defr u32 [N + 1]: the bytes a call with RHP_WALK_DEFRAME
            leaves different, defr_idx u16 (offset in the buffer), defr_val u8 -- all inside the session under test
            and below lim: [a, min(e, lim)); every other byte of a case comes back as it went in
  per case and session (4 per case): n_slots, stop u8, consumed u16     (rhp_walk_result_t)
            kept u8 (1: the state is left as it lay), st_phase, st_ct, st_hex, st_state u8, st_left u32: the state at
            exit as in walk_resume.npz (resume cases; zero in the others)
  per slot: start u16 (offset in the buffer), body_len u32, wire_len u16, result i8, body_kind u8   (rhp_walk_slot_t)
            ret i16, status, msg_off, msg_len u16, minor i8, num_headers u8   (rhp_msg_t; ret 0 with result 1: a continuation)
  hdr u16 [H, 4]  name_off (RHP_NAME_NULL: name == NULL), name_len, value_off, value_len: num_headers records of
                  every slot with ret > 0, one slot after the other
Behind them the sess_off rows that hold anything (walk_edge_sets.stray_cases) over one small batch per call, the
n65 set of walk_responses.npz and round 1 of three_rounds of walk_resume.npz as those files hold them: P cases, each
sess_off rows [off_lo, off_hi] at off_value, bytes_size all of the buffer.  The sessions off_lo - 1 .. min(off_hi,
n_sessions - 1) are the only ones whose clamped [a, e) changes; the reference walk over them is stored, every other
session is the clean run's, which the two older files hold.
  off_call u8, off_lo, off_hi u16, off_value u64, off_deframe u8 (1: the case is run with RHP_WALK_DEFRAME too) [P]
  off_sess u32 [P + 1]: the changed sessions of a case, in order, with off_n_slots, off_stop u8, off_consumed u32,
            off_kept, off_st_phase, off_st_ct, off_st_hex, off_st_state u8, off_st_left u64 as above
  off_slot u32 [P + 1]: their written slots, with off_start u32, off_body_len u64, off_wire_len u32, off_result i8,
            off_body_kind u8, off_ret i32, off_status, off_msg_off, off_msg_len u16, off_minor i8, off_num_headers u8
  off_hdr u16 [H', 4]    off_defr u32 [P + 1], off_defr_idx u32, off_defr_val u8: what RHP_WALK_DEFRAME leaves different
            from the input at and behind the first changed session's start (off_deframe cases)
usage: python tests/golden/make_golden_walk_edges.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import libreactorng_amd as rhp  # noqa: E402
import walk_edge_sets as we  # noqa: E402
import walk_resume_sets as wr  # noqa: E402
import make_golden_decode_chunked as mdc  # noqa: E402
from make_golden_messages import reference  # noqa: E402
from make_golden_walk import walker  # noqa: E402
from make_golden_walk_resume import round_walker, state_tuples  # noqa: E402

GOLDEN = os.path.join(HERE, "walk_edges.npz")
LIMIT = 357137   # the largest walk fixture: the file stays below it


def walkers():
    ref, ref_chunked = reference(), mdc.reference()
    return walker(ref, ref_chunked), round_walker(ref, ref_chunked)


def expected(walks, call, kind, pad, lim):
    """the reference walk of one case over its clamped view: ([(result, rows, state after or None)] per session, the
    view as RHP_WALK_DEFRAME leaves it)"""
    walk, rwalk = walks
    buf, sess_off = we.buffer(kind, pad)
    view = buf.copy()
    view[lim:] = 0
    out = view.copy()
    off = np.minimum(sess_off, np.uint64(lim))
    zero = state_tuples([wr.state()])[0]
    answers = []
    for s, cap in enumerate(we.SLOTS):
        a, e = int(off[s]), int(off[s + 1])
        if call == we.RESPONSES:
            res, rows = walk(view, out, a, e, cap, we.MAXH, we.FLAGS)
            nxt = None
        else:
            st = state_tuples([we.state_in(kind)])[0] if s == 1 else zero
            res, rows, nxt = rwalk(view, out, a, e, cap, we.MAXH, we.FLAGS, st)
        answers.append((res, rows, nxt))
    assert (view[:lim] == buf[:lim]).all() and not view[lim:].any(), "the reference moves nothing in the bytes it reads"
    return answers, out


def stray_expected(walks, call, lo, hi, value):
    """the reference walk over the changed sessions of one stray-offset case: ([(session, result, rows, state after
    or None)], the bytes from the first changed session's start on as RHP_WALK_DEFRAME leaves them, that start)"""
    walk, rwalk = walks
    b = we.small_batch(call)
    buf, ns = b["buf"], len(b["sess_off"]) - 1
    lim = we.readable(buf.size)
    view = buf.copy()
    view[lim:] = 0
    out = view.copy()
    so = we.stray_offsets(b["sess_off"], lo, hi, value)
    sts = state_tuples(b["states"]) if b["states"] is not None else None
    answers = []
    for s in range(max(lo - 1, 0), min(hi, ns - 1) + 1):
        a, e = we.clamped(so, s, lim)
        cap = int(b["slot_off"][s + 1] - b["slot_off"][s])
        if call == we.RESPONSES:
            res, rows = walk(view, out, a, e, cap, b["maxh"], b["flags"])
            nxt = None
        else:
            res, rows, nxt = rwalk(view, out, a, e, cap, b["maxh"], b["flags"], sts[s])
        answers.append((s, res, rows, nxt))
    first = we.clamped(so, max(lo - 1, 0), lim)[0]
    assert (out[:first] == buf[:first]).all()
    return answers, out, first


def stray(walks):
    """the off_* arrays"""
    P = {k: [] for k in ("off_call", "off_lo", "off_hi", "off_value", "off_deframe")}
    Q = {"off_" + k: [] for k in ("n_slots", "stop", "consumed", "kept", "st_phase", "st_ct", "st_hex", "st_state", "st_left")}
    T = {"off_" + k: [] for k in ("start", "body_len", "wire_len", "result", "body_kind", "ret", "status", "msg_off", "msg_len", "minor", "num_headers")}
    off_sess, off_slot, off_defr, defr_idx, defr_val, hdr = [0], [0], [0], [], [], []
    for call in (we.RESPONSES, we.RESUME):
        stops = []
        for lo, hi, value, deframe in we.stray_cases(call):
            answers, out, first = stray_expected(walks, call, lo, hi, value)
            buf = we.small_batch(call)["buf"]
            for k, v in zip(P, (call, lo, hi, value, deframe)):
                P[k].append(v)
            for s, res, rows, nxt in answers:
                phase, left, dec, _ = nxt if nxt is not None else (0, 0, bytes(16), 0)
                for k, v in zip(Q, res + (int(nxt is None and call == we.RESUME), phase, dec[8], dec[9], dec[10],
                                          left if phase == wr.IN_LENGTH else int.from_bytes(dec[:8], "little"))):
                    Q[k].append(v)
                for row in rows:
                    msg = row[5] if row[5][0] > 0 else (row[5][0], 0, 0, 0, 0, 0)
                    for k, v in zip(T, row[:5] + msg):
                        T[k].append(v)
                    hdr.extend(row[6])
            stops.append(answers[0][1][1])
            off_sess.append(len(Q["off_stop"]))
            off_slot.append(len(T["off_start"]))
            if deframe:
                d = np.flatnonzero(out != buf)
                defr_idx.extend(d.tolist())
                defr_val.extend(out[d].tolist())
            off_defr.append(len(defr_idx))
        print(f"{we.CALL_NAMES[call]} stray sess_off: {len(stops)} cases, stops of the session that runs on {sorted(set(stops))}")
    arr = lambda a, dt: np.array(a, dtype=dt)
    types = dict(off_lo=np.uint16, off_hi=np.uint16, off_value=np.uint64, off_consumed=np.uint32, off_st_left=np.uint64, off_start=np.uint32,
                 off_body_len=np.uint64, off_wire_len=np.uint32, off_result=np.int8, off_ret=np.int32, off_status=np.uint16,
                 off_msg_off=np.uint16, off_msg_len=np.uint16, off_minor=np.int8)
    out = dict(off_sess=arr(off_sess, np.uint32), off_slot=arr(off_slot, np.uint32), off_defr=arr(off_defr, np.uint32),
               off_defr_idx=arr(defr_idx, np.uint32), off_defr_val=arr(defr_val, np.uint8), off_hdr=arr(hdr, np.uint16).reshape(-1, 4))
    for cols in (P, Q, T):
        for k, v in cols.items():
            out[k] = arr(v, types.get(k, np.uint8))
            assert [int(x) for x in out[k]] == [int(x) for x in v], f"{k} fits its column"
    return out


def main():
    walks = walkers()
    lead, tail = we.LEAD, we.PLANTED + we.PLANTED + we.BEHIND
    bufs, mids, buf_a = [], [], []
    for kind in we.KINDS:
        for pad in range(we.PADS):
            ld, session, _, _ = we.parts(kind, pad)
            assert ld[: len(lead)] == lead and bytes(we.buffer(kind, pad)[0]) == ld + session + tail + bytes(we.RHP_PAD)
            bufs.append((we.KINDS.index(kind), pad))
            mids.append(ld[len(lead):] + session)
            buf_a.append(len(ld) - len(lead))
    C = {k: [] for k in ("call", "case_buf", "c", "lim", "size")}
    Q = {k: [] for k in ("n_slots", "stop", "consumed", "kept", "st_phase", "st_ct", "st_hex", "st_state", "st_left")}
    T = {k: [] for k in ("start", "body_len", "wire_len", "result", "body_kind", "ret", "status", "msg_off", "msg_len", "minor", "num_headers")}
    case_slot, case_defr, defr_idx, defr_val, hdr = [0], [0], [], [], []
    stops = {}
    for call, kind, pad, c, lim, size in we.all_cases():
        answers, out = expected(walks, call, kind, pad, lim)
        buf, off = we.buffer(kind, pad)
        for k, v in zip(C, (call, bufs.index((we.KINDS.index(kind), pad)), c, lim, size)):
            C[k].append(v)
        for s, (res, rows, nxt) in enumerate(answers):
            phase, left, dec, _ = nxt if nxt is not None else (0, 0, bytes(16), 0)
            assert dec[11:] == bytes(5)
            for k, v in zip(Q, res + (int(nxt is None and call == we.RESUME), phase, dec[8], dec[9], dec[10],
                                      left if phase == wr.IN_LENGTH else int.from_bytes(dec[:8], "little"))):
                Q[k].append(v)
            for row in rows:
                msg = row[5] if row[5][0] > 0 else (row[5][0], 0, 0, 0, 0, 0)   # (but for ret meaningful for ret > 0)
                for k, v in zip(T, row[:5] + msg):
                    T[k].append(v)
                hdr.extend(row[6])
        stops.setdefault((call, kind), set()).add(answers[1][0][1])
        case_slot.append(len(T["start"]))
        d = np.flatnonzero(out[:lim] != buf[:lim])
        assert not len(d) or (d[0] >= int(off[1]) and d[-1] < min(int(off[2]), lim)), "only the session under test is de-framed"
        defr_idx.extend(d.tolist())
        defr_val.extend(out[d].tolist())
        case_defr.append(len(defr_idx))
    for (call, kind), v in stops.items():
        print(f"{we.CALL_NAMES[call]} {kind}: {len(we.cases(kind))} cases, stops of the session under test {sorted(v)}")
    arr = lambda a, dt: np.array(a, dtype=dt)
    states = np.array([we.state_in(k) for k in we.KINDS], dtype=wr.STATE_DTYPE)
    out = dict(kind_name=np.array(we.KINDS), kind_state=states.view(np.uint8).reshape(-1).copy(),
               max_headers=arr([we.MAXH], np.uint32), flags=arr([we.FLAGS], np.uint32), slot_off=we.slot_off(),
               lead=np.frombuffer(lead, dtype=np.uint8), tail=np.frombuffer(tail, dtype=np.uint8),
               tail_sess=arr([len(we.PLANTED)] * 2, np.uint32), buf_kind=arr([b[0] for b in bufs], np.uint8),
               buf_pad=arr([b[1] for b in bufs], np.uint8), buf_byte=arr(np.concatenate([[0], np.cumsum([len(m) for m in mids])]), np.uint32),
               buf_a=arr(buf_a, np.uint16), mid=np.frombuffer(b"".join(mids), dtype=np.uint8),
               case_slot=arr(case_slot, np.uint32), case_defr=arr(case_defr, np.uint32), defr_idx=arr(defr_idx, np.uint16),
               defr_val=arr(defr_val, np.uint8), hdr=arr(hdr, np.uint16).reshape(-1, 4))
    ct = dict(call=np.uint8, case_buf=np.uint16, c=np.int16, lim=np.uint32, size=np.uint32)
    qt = dict(consumed=np.uint16, st_left=np.uint32)
    tt = dict(start=np.uint16, body_len=np.uint32, wire_len=np.uint16, result=np.int8, body_kind=np.uint8, ret=np.int16,
              status=np.uint16, msg_off=np.uint16, msg_len=np.uint16, minor=np.int8, num_headers=np.uint8)
    for cols, types in ((C, ct), (Q, qt), (T, tt)):
        for k, v in cols.items():
            out[k] = arr(v, types.get(k, np.uint8))
            assert (out[k].astype(np.int64) == np.array(v, dtype=np.int64)).all(), f"{k} fits its column"
    out.update(stray(walks))
    np.savez(GOLDEN, **out)
    size = os.path.getsize(GOLDEN)
    print(f"{GOLDEN}: {len(bufs)} buffers, {len(C['call'])} cases, {len(T['start'])} slots, {len(hdr)} header records, "
          f"{len(defr_idx)} bytes moved by the de-framing, {size} bytes")
    assert size < LIMIT, f"the file stays below {LIMIT} bytes"


if __name__ == "__main__":
    main()
