#!/usr/bin/env python3
"""Writes tests/golden/walk_resume.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every set of tests/walk_resume_sets.py the rounds of rhp.h (rhp_walk_resume)
are written out here in plain Python, session by session and round by round,
and every value a round steps by is the compiled reference's:
  parse    phr_parse_response, called in place on the round's packed buffer, so
           that what it reads past the session's end is the next session's bytes
           and then the pad (make_golden_messages.reference_message)
  framing  http_field_lookup, data_equal_case, libc strtoull
           (make_golden_frame_messages.composer)
  body     phr_decode_chunked on a private copy of the piece
           (make_golden_decode_chunked.reference_call): from a zero decoder behind
           a head, from the sixteen decoder bytes the reference itself left in the
           round before in a continuation; for the de-framed bytes a second call
           on a copy of the body's own wire span from the same decoder
What is not the reference's is stated as rhp.h states it: a status of 100..199,
204 or 304 has no body; the phases, the arming and the corrupt-state rules.
A round's input is made by walk_resume_sets.walk_rounds from the round before.

The file is flat, so that the stand-alone C test (tests/walk_resume_host_test.c)
reads it as well: np.savez, not compressed, narrow columns.  S sets, R rounds,
Q session-rounds, NT written slots (only the slots a session wrote are held, in
session order), NF first-round sessions.
  set_name str [S]   set_maxh, set_flags, set_nsess u32 [S]   set_round u32 [S + 1]: its rounds [lo, hi)
  set_first u32 [S + 1]   states_in u8 [NF * 32]: the rhp_walk_state_t of its sessions before its first round
                          (an empty range: all zero); a later round's states are what the round before left
  round_q, round_slot u32 [R + 1], round_byte u64 [R + 1]: the round's session-rounds, slots and bytes
  bytes u8: a round's sessions back to back, no pad (RHP_PAD zero bytes follow in the call)
  defr_idx u32, defr_val u8: the bytes a call with RHP_WALK_DEFRAME leaves different: bytes[defr_idx] = defr_val
  per session-round: len u32, cap u8 (slots owned), n_slots u8, stop u8, consumed u32     (rhp_walk_result_t)
                     kept u8 (1: the state is left as it lay), st_phase, st_ct, st_hex, st_state u8 and st_left u64:
                     the state at exit -- phase; decoder.consume_trailer, hex_count, state; left when IN_LENGTH,
                     decoder.bytes_left_in_chunk when IN_CHUNKED; every other byte of it zero
  per slot: start u32 (from the round's first byte), body_len u64, wire_len u32, result i8, body_kind u8   (rhp_walk_slot_t)
            ret i32, status, msg_off, msg_len u16, minor i8, num_headers u16   (rhp_msg_t; ret 0 with result 1: a continuation)
  hdr u16 [H, 4]  name_off (RHP_NAME_NULL: name == NULL), name_len, value_off, value_len: num_headers records of
                  every slot with ret > 0, one slot after the other
usage: python tests/golden/make_golden_walk_resume.py
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
import walk_resume_sets as wr  # noqa: E402
import make_golden_decode_chunked as mdc  # noqa: E402
from make_golden_frame_messages import composer  # noqa: E402
from make_golden_messages import reference, reference_message  # noqa: E402

GOLDEN = os.path.join(HERE, "walk_resume.npz")
NO_BODY = lambda status: 100 <= status <= 199 or status in (204, 304)   # RFC 9112 6.3: the walk's one invented rule
ZERO_DECODER = lambda trailers: bytes(8) + bytes([int(trailers)]) + bytes(7)


def round_walker(ref, ref_chunked):
    """walk(buf, out, a, e, cap, maxh, flags, st) -> ((n_slots, stop, consumed), rows, state after or None (kept));
    a state is (phase, left, sixteen decoder bytes, reserved); rows as make_golden_walk's"""
    compose = composer(ref)
    decode = lambda dec, piece: mdc.reference_call(ref_chunked, dec, piece)

    def chunked_piece(buf, out, at, e, dec):
        """the decoder over [at, e): (ret, size, wire_len, decoder after); on ret != -1 `out` gets the de-framed bytes"""
        piece = bytes(buf[at: e])
        ret, size, after_dec, after = decode(dec, piece)
        if ret == -1:
            return ret, 0, 0, dec
        wire = len(piece) if ret == -2 else len(piece) - ret
        if ret >= 0:   # the body's own wire span from the same decoder: what the de-framing leaves
            r2, size2, _, after = decode(dec, piece[:wire])
            assert (r2, size2) == (0, size), "the body's own wire span decodes to the same body"
        out[at: at + wire] = np.frombuffer(after, dtype=np.uint8)[:wire]
        return ret, size, wire, after_dec

    def walk(buf, out, a, e, cap, maxh, flags, st):
        phase, left, dec, reserved = st
        trailers = bool(flags & wr.TRAILERS)
        if phase >= wr.DEAD or reserved != 0 or (phase == wr.IN_CHUNKED and (dec[10] > 5 or dec[9] > 16)):
            return (0, rhp.WALK_BAD, 0), [], None
        if a == e:
            return (0, {wr.AT_HEAD: rhp.WALK_END, wr.IN_CLOSE: rhp.WALK_CLOSE}.get(phase, rhp.WALK_BODY), 0), [], None
        pos, rows, stop = a, [], rhp.WALK_END
        nxt = (wr.AT_HEAD, 0, bytes(16), 0)
        none = (0, 0, 0, 0, 0, 0)
        if phase != wr.AT_HEAD:
            if cap == 0:
                return (0, rhp.WALK_MORE, 0), [], None
            avail = e - a
            if phase == wr.IN_LENGTH:
                wire = min(left, avail)
                rows.append((a, left, wire, 1, rhp.FRAME_LENGTH, none, []))
                if left - wire:
                    stop, nxt = rhp.WALK_BODY, (wr.IN_LENGTH, left - wire, bytes(16), 0)
            elif phase == wr.IN_CHUNKED:
                ret, size, wire, after_dec = chunked_piece(buf, out, a, e, dec)
                if ret == -1:
                    rows.append((a, 0, 0, -1, rhp.FRAME_NONE, none, []))
                    stop = rhp.WALK_BAD
                else:
                    rows.append((a, size, wire, 1, rhp.FRAME_CHUNKED, none, []))
                    if ret == -2:
                        stop, nxt = rhp.WALK_BODY, (wr.IN_CHUNKED, 0, after_dec, 0)
            else:
                wire = avail
                rows.append((a, 0, wire, 1, rhp.FRAME_NONE, none, []))
                stop, nxt = rhp.WALK_CLOSE, (wr.IN_CLOSE, 0, bytes(16), 0)
            pos = a + rows[0][2]
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
                    stop = rhp.WALK_BAD
                elif NO_BODY(status):
                    body_len = 0
                elif kind == rhp.FRAME_LENGTH:
                    wire_len = min(body_len, avail)
                    if body_len > avail:
                        stop, nxt = rhp.WALK_BODY, (wr.IN_LENGTH, body_len - avail, bytes(16), 0)
                elif kind == rhp.FRAME_CHUNKED:
                    r, size, wire, after_dec = chunked_piece(buf, out, body, e, ZERO_DECODER(trailers))
                    if r == -1:
                        result, kind, stop = -1, rhp.FRAME_NONE, rhp.WALK_BAD
                    else:
                        body_len, wire_len = size, wire
                        if r == -2:
                            stop, nxt = rhp.WALK_BODY, (wr.IN_CHUNKED, 0, after_dec, 0)
                elif not flags & wr.NONE_EMPTY:
                    wire_len, stop, nxt = avail, rhp.WALK_CLOSE, (wr.IN_CLOSE, 0, bytes(16), 0)
            rows.append((pos, body_len, wire_len, result, kind, msg, recs if ret > 0 else []))
            if stop == rhp.WALK_END:
                pos += ret + wire_len
            elif stop in (rhp.WALK_BODY, rhp.WALK_CLOSE):
                pos = e          # the bytes of a started body are taken
        if stop == rhp.WALK_BAD:
            nxt = (wr.DEAD, 0, bytes(16), 0)
        return (len(rows), stop, pos - a), rows, nxt

    return walk


def state_tuples(states):
    return [(int(s["phase"]), int(s["left"]), s["decoder"].tobytes(), int(s["reserved"])) for s in states]


def state_array(tuples):
    out = np.zeros(len(tuples), dtype=wr.STATE_DTYPE)
    for k, (phase, left, dec, reserved) in enumerate(tuples):
        out[k]["phase"], out[k]["left"], out[k]["reserved"] = phase, left, reserved
        out[k: k + 1].view(np.uint8)[:16] = np.frombuffer(dec, dtype=np.uint8)
    return out


def reference_step(walk, record):
    """walk_rounds' step over the reference: a round of every session, recorded"""
    def step(buf, off, sl, states, maxh, flags):
        n = len(off) - 1
        sts = state_tuples(states) if states is not None else [(wr.AT_HEAD, 0, bytes(16), 0)] * n
        out = buf.copy()
        res, rows_all, after, kept = [], [], [], []
        for s in range(n):
            r, rows, nxt = walk(buf, out, int(off[s]), int(off[s + 1]), int(sl[s + 1] - sl[s]), maxh, flags, sts[s])
            res.append(r)
            rows_all.append(rows)
            kept.append(nxt is None)
            after.append(sts[s] if nxt is None else nxt)
        record(buf, out, off, sl, res, rows_all, after, kept)
        results = np.array(res, dtype=rhp.WALK_RESULT_DTYPE)
        return results, None, None, None, out, state_array(after)
    return step


def main():
    walk = round_walker(reference(), mdc.reference())
    S = dict(name=[], maxh=[], flags=[], nsess=[], round=[0], first=[0])
    states_in, chunks, defr_idx, defr_val = [], [], [], []
    round_q, round_slot, round_byte = [0], [0], [0]
    Q = {k: [] for k in ("len", "cap", "n_slots", "stop", "consumed", "kept", "st_phase", "st_ct", "st_hex", "st_state", "st_left")}
    T = {k: [] for k in ("start", "body_len", "wire_len", "result", "body_kind", "ret", "status", "msg_off", "msg_len", "minor", "num_headers")}
    hdr_lo, hdr = [0], []
    seen = dict(entry=set(), exit=set(), cont_stop=set(), head_stop=set(), cut_state=set(), moved=0, after_cont=set())

    def record(buf, out, off, sl, res, rows_all, after, kept):
        nbytes = int(off[-1])
        base = round_byte[-1]
        chunks.append(buf[:nbytes].copy())
        assert (buf[nbytes:] == out[nbytes:]).all()
        d = np.flatnonzero(buf[:nbytes] != out[:nbytes])
        defr_idx.extend((d + base).tolist())
        defr_val.extend(out[d].tolist())
        seen["moved"] += len(d)
        for s, (r, rows) in enumerate(zip(res, rows_all)):
            phase, left, dec, _ = after[s]
            assert dec[11:] == bytes(5) and (kept[s] or phase <= wr.DEAD)
            Q["len"].append(int(off[s + 1] - off[s])); Q["cap"].append(int(sl[s + 1] - sl[s]))
            Q["n_slots"].append(r[0]); Q["stop"].append(r[1]); Q["consumed"].append(r[2]); Q["kept"].append(int(kept[s]))
            Q["st_phase"].append(phase & 0xff); Q["st_ct"].append(dec[8]); Q["st_hex"].append(dec[9]); Q["st_state"].append(dec[10])
            Q["st_left"].append(left if phase == wr.IN_LENGTH else int.from_bytes(dec[:8], "little"))
            if not kept[s]:
                seen["exit"].add(phase)
                if phase == wr.IN_CHUNKED:
                    seen["cut_state"].add(dec[10])
            for k, row in enumerate(rows):
                for f, v in zip(("start", "body_len", "wire_len", "result", "body_kind"), row[:5]):
                    T[f].append(v - int(off[0]) if f == "start" else v)
                for f, v in zip(("ret", "status", "msg_off", "msg_len", "minor", "num_headers"), row[5]):
                    T[f].append(v)
                hdr.extend(row[6])
                hdr_lo.append(len(hdr))
            if rows:
                first_is_cont = _entry_phase[s] != wr.AT_HEAD   # (a round that writes a slot from an IN_* phase starts with it)
                (seen["cont_stop"] if first_is_cont and len(rows) == 1 else seen["head_stop"]).add(r[1])
                if first_is_cont:
                    seen["after_cont"].add(r[1])
        round_q.append(round_q[-1] + len(res))
        round_slot.append(len(T["start"]))
        round_byte.append(base + nbytes)

    _entry_phase = []
    for name, maxh, flags, deliveries, caps, states in wr.all_sets():
        n = len(deliveries[0])
        st0 = states if states is not None else np.zeros(n, dtype=wr.STATE_DTYPE)
        if states is not None:
            states_in.append(st0.view(np.uint8).reshape(-1).copy())
        q0 = len(Q["stop"])

        def step(buf, off, sl, sts, maxh_, flags_, inner=reference_step(walk, record)):
            _entry_phase[:] = [int(p) for p in sts["phase"]]
            for k in range(n):
                if off[k + 1] > off[k] or sts["phase"][k] >= wr.DEAD:
                    seen["entry"].add(min(int(sts["phase"][k]), wr.DEAD))
            return inner(buf, off, sl, sts, maxh_, flags_)

        rounds = wr.walk_rounds(step, deliveries, caps, maxh, flags, st0)
        S["name"].append(name); S["maxh"].append(maxh); S["flags"].append(flags); S["nsess"].append(n)
        S["round"].append(S["round"][-1] + len(rounds)); S["first"].append(S["first"][-1] + (n if states is not None else 0))
        stops = Q["stop"][q0:]
        print(f"{name}: {n} sessions, {len(rounds)} rounds, max_headers {maxh}, flags {flags}: stops "
              + ", ".join(f"{c} x {stops.count(c)}" for c in sorted(set(stops))))
    # what the sets are for (tests/test_walk_resume.py asserts the same from the file)
    assert seen["entry"] == set(range(5)) and seen["exit"] == set(range(5)), (seen["entry"], seen["exit"])
    assert seen["cont_stop"] == {rhp.WALK_END, rhp.WALK_BAD, rhp.WALK_BODY, rhp.WALK_CLOSE, rhp.WALK_MORE}, seen["cont_stop"]
    assert seen["head_stop"] == set(range(6)) and seen["after_cont"] == set(range(6)), (seen["head_stop"], seen["after_cont"])
    assert seen["cut_state"] == set(range(6)), seen["cut_state"]
    assert seen["moved"] > 0
    arr = lambda a, dt: np.array(a, dtype=dt)
    out = dict(set_name=np.array(S["name"]), set_maxh=arr(S["maxh"], np.uint32), set_flags=arr(S["flags"], np.uint32),
               set_nsess=arr(S["nsess"], np.uint32), set_round=arr(S["round"], np.uint32), set_first=arr(S["first"], np.uint32),
               states_in=np.concatenate(states_in), round_q=arr(round_q, np.uint32), round_slot=arr(round_slot, np.uint32),
               round_byte=arr(round_byte, np.uint64), bytes=np.concatenate(chunks), defr_idx=arr(defr_idx, np.uint32),
               defr_val=arr(defr_val, np.uint8), hdr=arr(hdr, np.uint16).reshape(-1, 4))
    qt = dict(len=np.uint32, consumed=np.uint32, st_left=np.uint64)
    for k, v in Q.items():
        out[k] = arr(v, qt.get(k, np.uint8))
    tt = dict(start=np.uint32, body_len=np.uint64, wire_len=np.uint32, result=np.int8, body_kind=np.uint8, ret=np.int32,
              status=np.uint16, msg_off=np.uint16, msg_len=np.uint16, minor=np.int8, num_headers=np.uint16)
    for k, v in T.items():
        out[k] = arr(v, tt[k])
    np.savez(GOLDEN, **out)
    size, limit = os.path.getsize(GOLDEN), os.path.getsize(os.path.join(HERE, "walk_responses.npz"))
    print(f"{GOLDEN}: {len(S['name'])} sets, {len(round_q) - 1} rounds, {len(Q['stop'])} session-rounds, {len(T['start'])} slots, "
          f"{len(hdr)} header records, {seen['moved']} bytes moved by the de-framing, {size} bytes")
    assert size <= limit, f"the file is no larger than walk_responses.npz ({limit} bytes)"


if __name__ == "__main__":
    main()
