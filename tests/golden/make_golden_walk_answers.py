#!/usr/bin/env python3
"""Writes tests/golden/walk_answers.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every set of tests/walk_answer_sets.py the rounds of rhp.h
(rhp_walk_answers) are written out here in plain Python, session by session and
round by round, and every value a round steps by is the compiled reference's,
taken as the other walk generators take it:
  parse    phr_parse_response in place on the round's packed buffer
           (make_golden_messages.reference_message)
  framing  http_field_lookup, data_equal_case, libc strtoull
           (make_golden_frame_messages.composer)
  body     phr_decode_chunked on a private copy of the piece
           (make_golden_decode_chunked.reference_call)
What is not the reference's is stated as rhp.h states it: a status of 100..199,
204 or 304 has no body; the phases, the arming and the corrupt-state rules of
the resumed walk; and this call's own rules -- the queue and its clamp, interim
and final heads, the reply to a HEAD, answered and slot_req.  The reference has
no response walker and no rule for any of these.

The file is flat, so that the stand-alone C test
(tests/walk_answers_host_test.c) reads it as well: np.savez, not compressed,
narrow columns.  It holds what walk_resume.npz holds, under the same names (see
make_golden_walk_resume.py; header records are not held: the heads are parsed
as in the other walks, whose files hold theirs), and
  set_mode u32 [S]        0: states == NULL, one round; 1: the resumed walk
  req_off u32             a round's req_off [n + 1], round r's at round_q[r] + r
  round_word u32 [R + 1]  head_words u32: a round's head_bits words [lo, hi)
  round_nreq u32 [R]      n_req_total as the call is given it
  per session-round: answered u8
  per slot: slot_req i16 (-1: RHP_WALK_REQ_NONE)
usage: python tests/golden/make_golden_walk_answers.py
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
import walk_answer_sets as wa  # noqa: E402
import walk_resume_sets as wr  # noqa: E402
import make_golden_decode_chunked as mdc  # noqa: E402
from make_golden_frame_messages import composer  # noqa: E402
from make_golden_messages import reference, reference_message  # noqa: E402
from make_golden_walk_resume import state_array, state_tuples  # noqa: E402

GOLDEN = os.path.join(HERE, "walk_answers.npz")
NO_BODY = lambda status: 100 <= status <= 199 or status in (204, 304)   # RFC 9112 6.3: the walk's first invented rule
INTERIM = lambda status: 100 <= status <= 199
ZERO_DECODER = lambda trailers: bytes(8) + bytes([int(trailers)]) + bytes(7)
NONE = -1   # RHP_WALK_REQ_NONE in the file


def queue_of(req_off, head_bits, n_req_total, s):
    """session s's queue as rhp.h clamps it: one truth value per request it owns"""
    lo, hi = int(req_off[s]), int(req_off[s + 1])
    if lo > hi or hi > n_req_total:
        return []
    return [bool(int(head_bits[q >> 5]) >> (q & 31) & 1) for q in range(lo, hi)]


def answer_walker(ref, ref_chunked):
    """walk(buf, out, a, e, cap, maxh, flags, st, queue) -> ((n_slots, stop, consumed), rows, state after or None
    (kept), answered, [slot_req]); st None: the one-shot walk (a started body is not taken and not de-framed), else a
    state (phase, left, sixteen decoder bytes, reserved); rows as make_golden_walk's"""
    compose = composer(ref)
    decode = lambda dec, piece: mdc.reference_call(ref_chunked, dec, piece)

    def chunked_piece(buf, out, at, e, dec, partial):
        """the decoder over [at, e): (ret, size, wire_len, decoder after); `out` gets the de-framed bytes of a completed
        body and, with `partial`, of one that is not complete"""
        piece = bytes(buf[at: e])
        ret, size, after_dec, after = decode(dec, piece)
        if ret == -1:
            return ret, 0, 0, dec
        wire = len(piece) if ret == -2 else len(piece) - ret
        if ret >= 0:
            r2, size2, _, after = decode(dec, piece[:wire])
            assert (r2, size2) == (0, size), "the body's own wire span decodes to the same body"
        if ret >= 0 or partial:
            out[at: at + wire] = np.frombuffer(after, dtype=np.uint8)[:wire]
        return ret, size, wire, after_dec

    def walk(buf, out, a, e, cap, maxh, flags, st, queue):
        take = st is not None
        phase, left, dec, reserved = st if take else (wr.AT_HEAD, 0, bytes(16), 0)
        trailers = bool(flags & wa.TRAILERS)
        if phase >= wr.DEAD or reserved != 0 or (phase == wr.IN_CHUNKED and (dec[10] > 5 or dec[9] > 16)):
            return (0, rhp.WALK_BAD, 0), [], None, 0, []
        if take and a == e:
            return (0, {wr.AT_HEAD: rhp.WALK_END, wr.IN_CLOSE: rhp.WALK_CLOSE}.get(phase, rhp.WALK_BODY), 0), [], None, 0, []
        pos, rows, stop = a, [], rhp.WALK_END
        k, slot_req = 0, []                      # the queue starts at the first unanswered request: k = 0 every round
        nxt = (wr.AT_HEAD, 0, bytes(16), 0)
        none = (0, 0, 0, 0, 0, 0)
        if phase != wr.AT_HEAD:
            if cap == 0:
                return (0, rhp.WALK_MORE, 0), [], None, 0, []
            avail = e - a
            if phase == wr.IN_LENGTH:
                wire = min(left, avail)
                rows.append((a, left, wire, 1, rhp.FRAME_LENGTH, none, []))
                if left - wire:
                    stop, nxt = rhp.WALK_BODY, (wr.IN_LENGTH, left - wire, bytes(16), 0)
            elif phase == wr.IN_CHUNKED:
                ret, size, wire, after_dec = chunked_piece(buf, out, a, e, dec, True)
                if ret == -1:
                    rows.append((a, 0, 0, -1, rhp.FRAME_NONE, none, []))
                    stop = rhp.WALK_BAD
                else:
                    rows.append((a, size, wire, 1, rhp.FRAME_CHUNKED, none, []))
                    if ret == -2:
                        stop, nxt = rhp.WALK_BODY, (wr.IN_CHUNKED, 0, after_dec, 0)
            else:
                rows.append((a, 0, avail, 1, rhp.FRAME_NONE, none, []))
                stop, nxt = rhp.WALK_CLOSE, (wr.IN_CLOSE, 0, bytes(16), 0)
            pos = a + rows[0][2]
            slot_req.append(NONE)                # a continuation slot is no response
        while stop == rhp.WALK_END and pos < e:
            if len(rows) == cap:
                stop = rhp.WALK_MORE
                break
            ret, status, mo, ml, minor, recs = reference_message(ref, rhp.MSG_RESPONSE, buf, pos, e - pos, maxh, 0)
            assert ret <= rhp.RHP_MAX_LEN, "no set holds a head the records cannot encode"
            msg = (ret, status, mo, ml, minor, len(recs))
            body_len = wire_len = 0
            kind = rhp.FRAME_NONE
            if ret <= 0:
                result = -1 if ret == -1 else 0
                stop = rhp.WALK_HEAD if ret == -2 else rhp.WALK_BAD
            else:
                ret2, result, kind, body_len, _ = compose(rhp.MSG_RESPONSE, buf, pos, e - pos, maxh, [])
                assert ret2 == ret
                body, avail = pos + ret, e - (pos + ret)
                if result != 1:
                    stop = rhp.WALK_BAD          # a bad Content-Length is bad whoever asked
                elif NO_BODY(status):
                    body_len = 0
                elif k < len(queue) and queue[k]:
                    body_len = 0                 # the reply to a HEAD: the second invented rule (RFC 9112 6.3 item 1)
                elif kind == rhp.FRAME_LENGTH:
                    wire_len = min(body_len, avail)
                    if body_len > avail:
                        stop, nxt = rhp.WALK_BODY, (wr.IN_LENGTH, body_len - avail, bytes(16), 0)
                elif kind == rhp.FRAME_CHUNKED:
                    r, size, wire, after_dec = chunked_piece(buf, out, body, e, ZERO_DECODER(trailers), take)
                    if r == -1:
                        result, kind, stop = -1, rhp.FRAME_NONE, rhp.WALK_BAD
                    else:
                        body_len, wire_len = size, wire
                        if r == -2:
                            stop, nxt = rhp.WALK_BODY, (wr.IN_CHUNKED, 0, after_dec, 0)
                elif not flags & wa.NONE_EMPTY:
                    wire_len, stop, nxt = avail, rhp.WALK_CLOSE, (wr.IN_CLOSE, 0, bytes(16), 0)
            rows.append((pos, body_len, wire_len, result, kind, msg, recs if ret > 0 else []))
            if ret > 0 and result == 1:
                slot_req.append(k)               # an interim head names the request it precedes
                if not INTERIM(status):
                    k += 1
            else:
                slot_req.append(NONE)
            if stop == rhp.WALK_END:
                pos += ret + wire_len
            elif take and stop in (rhp.WALK_BODY, rhp.WALK_CLOSE):
                pos = e          # the bytes of a started body are taken
        if stop == rhp.WALK_BAD:
            nxt = (wr.DEAD, 0, bytes(16), 0)
        return (len(rows), stop, pos - a), rows, nxt, k, slot_req

    return walk


def reference_round(walk, mode, maxh, flags, buf, off, sl, states, req_off, head_bits, n_req_total):
    """one round of every session over the reference: (out bytes, [result], [rows], [state after], [kept], [answered],
    [[slot_req]])"""
    n = len(off) - 1
    sts = (state_tuples(states) if states is not None else [(wr.AT_HEAD, 0, bytes(16), 0)] * n) if mode else [None] * n
    out = buf.copy()
    res, rows_all, after, kept, answered, sreq = [], [], [], [], [], []
    for s in range(n):
        r, rows, nxt, k, sr = walk(buf, out, int(off[s]), int(off[s + 1]), int(sl[s + 1] - sl[s]), maxh, flags, sts[s],
                                   queue_of(req_off, head_bits, n_req_total, s))
        res.append(r); rows_all.append(rows); answered.append(k); sreq.append(sr)
        kept.append(nxt is None)
        after.append((sts[s] if nxt is None else nxt) if mode else (wr.AT_HEAD, 0, bytes(16), 0))
    return out, res, rows_all, after, kept, answered, sreq


def main():
    walk = answer_walker(reference(), mdc.reference())
    S = dict(name=[], maxh=[], flags=[], nsess=[], mode=[], round=[0], first=[0])
    states_in, chunks, defr_idx, defr_val, req_offs, words = [], [], [], [], [], []
    round_q, round_slot, round_byte, round_word, round_nreq = [0], [0], [0], [0], []
    Q = {k: [] for k in ("len", "cap", "n_slots", "stop", "consumed", "kept", "st_phase", "st_ct", "st_hex", "st_state", "st_left", "answered")}
    T = {k: [] for k in ("start", "body_len", "wire_len", "result", "body_kind", "ret", "status", "msg_off", "msg_len", "minor", "num_headers",
                         "slot_req")}
    for s in wa.all_sets():
        n = len(s["deliveries"][0])
        if s["states"] is not None:
            states_in.append(s["states"].view(np.uint8).reshape(-1).copy())

        def step(buf, off, sl, sts, req_off, head_bits, total, s=s):
            out, res, rows_all, after, kept, answered, sreq = reference_round(walk, s["mode"], s["maxh"], s["flags"], buf, off, sl, sts,
                                                                              req_off, head_bits, total)
            nbytes, base = int(off[-1]), round_byte[-1]
            chunks.append(buf[:nbytes].copy())
            assert (buf[nbytes:] == out[nbytes:]).all()
            d = np.flatnonzero(buf[:nbytes] != out[:nbytes])
            defr_idx.extend((d + base).tolist())
            defr_val.extend(out[d].tolist())
            req_offs.extend(int(v) for v in req_off)
            words.extend(int(v) for v in head_bits)
            round_word.append(len(words))
            round_nreq.append(total)
            for i in range(len(res)):
                phase, left, dec, _ = after[i]
                r = res[i]
                Q["len"].append(int(off[i + 1] - off[i])); Q["cap"].append(int(sl[i + 1] - sl[i]))
                Q["n_slots"].append(r[0]); Q["stop"].append(r[1]); Q["consumed"].append(r[2]); Q["kept"].append(int(kept[i]))
                Q["st_phase"].append(phase & 0xff); Q["st_ct"].append(dec[8]); Q["st_hex"].append(dec[9]); Q["st_state"].append(dec[10])
                Q["st_left"].append(left if phase == wr.IN_LENGTH else int.from_bytes(dec[:8], "little"))
                Q["answered"].append(answered[i])
                for row, sr in zip(rows_all[i], sreq[i]):
                    for f, v in zip(("start", "body_len", "wire_len", "result", "body_kind"), row[:5]):
                        T[f].append(v)
                    for f, v in zip(("ret", "status", "msg_off", "msg_len", "minor", "num_headers"), row[5]):
                        T[f].append(v)
                    T["slot_req"].append(sr)
            round_q.append(round_q[-1] + len(res))
            round_slot.append(len(T["start"]))
            round_byte.append(base + nbytes)
            results = np.array(res, dtype=rhp.WALK_RESULT_DTYPE)
            return dict(results=results, states=state_array(after), answered=answered)

        rounds = wa.answer_rounds(step, s)
        S["name"].append(s["name"]); S["maxh"].append(s["maxh"]); S["flags"].append(s["flags"]); S["nsess"].append(n); S["mode"].append(s["mode"])
        S["round"].append(S["round"][-1] + len(rounds)); S["first"].append(S["first"][-1] + (n if s["states"] is not None else 0))
        q0 = round_q[S["round"][-2]]
        print(f"{s['name']}: {n} sessions, {len(rounds)} rounds, mode {s['mode']}: stops {Q['stop'][q0:]}, answered {Q['answered'][q0:]}")
    arr = lambda a, dt: np.array(a, dtype=dt)
    out = dict(set_name=np.array(S["name"]), set_maxh=arr(S["maxh"], np.uint32), set_flags=arr(S["flags"], np.uint32),
               set_nsess=arr(S["nsess"], np.uint32), set_mode=arr(S["mode"], np.uint32), set_round=arr(S["round"], np.uint32),
               set_first=arr(S["first"], np.uint32), states_in=np.concatenate(states_in), round_q=arr(round_q, np.uint32),
               round_slot=arr(round_slot, np.uint32), round_byte=arr(round_byte, np.uint64), round_word=arr(round_word, np.uint32),
               round_nreq=arr(round_nreq, np.uint32), req_off=arr(req_offs, np.uint32), head_words=arr(words, np.uint32),
               bytes=np.concatenate(chunks), defr_idx=arr(defr_idx, np.uint32), defr_val=arr(defr_val, np.uint8))
    qt = dict(len=np.uint32, consumed=np.uint32, st_left=np.uint64)
    for k, v in Q.items():
        out[k] = arr(v, qt.get(k, np.uint8))
    tt = dict(start=np.uint32, body_len=np.uint64, wire_len=np.uint32, result=np.int8, body_kind=np.uint8, ret=np.int32,
              status=np.uint16, msg_off=np.uint16, msg_len=np.uint16, minor=np.int8, num_headers=np.uint16, slot_req=np.int16)
    for k, v in T.items():
        out[k] = arr(v, tt[k])
    np.savez(GOLDEN, **out)
    size, limit = os.path.getsize(GOLDEN), os.path.getsize(os.path.join(HERE, "walk_resume.npz"))
    print(f"{GOLDEN}: {len(S['name'])} sets, {len(round_q) - 1} rounds, {len(Q['stop'])} session-rounds, {len(T['start'])} slots, "
          f"{len(defr_idx)} bytes moved by the de-framing, {size} bytes")
    assert size <= limit, f"the file is no larger than walk_resume.npz ({limit} bytes)"


if __name__ == "__main__":
    main()
