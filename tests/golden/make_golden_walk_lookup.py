#!/usr/bin/env python3
"""Writes tests/golden/walk_lookup.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every set of tests/walk_lookup_sets.py the walk is the plain-Python one of
make_golden_walk.py (rhp_walk_responses) or, call by call, of
make_golden_walk_resume.py (rhp_walk_resume), every value they step by the
compiled reference's.  For every head slot -- result 1, ret > 0 -- the fields are
the reference's http_field_lookup, called for each of the set's names on the
header array its phr_parse_response returned for that head
(make_golden_frame_messages.composer).  Every other slot is absent, as rhp.h
(rhp_lookup_walked) says.

The file is flat, so that the stand-alone C test (tests/walk_lookup_host_test.c)
reads it as well: np.savez, not compressed, narrow columns.  S sets, C calls
(a set's rounds), Q session-calls, W written slots, F present fields.
  set_name str [S]   set_maxh, set_flags, set_nsess u32 [S]   set_resume u8 [S]: 1: its calls are rhp_walk_resume rounds
  set_call u32 [S + 1]: its calls [lo, hi)
  set_first u32 [S + 1]   states_in u8 [NF * 32]: the rhp_walk_state_t of its sessions before its first call (an empty
                          range: all zero), as walk_resume.npz
  set_names u32 [S + 1]: its names are name_span[lo, hi)   name_span u32 [T, 2]: (off, len) into name_text u8
  call_q, call_w, call_f u32 [C + 1], call_byte u64 [C + 1]: the call's session-calls, written slots, present fields, bytes
  bytes u8: a call's sessions back to back, no pad (RHP_PAD zero bytes follow in the call)
  per session-call: len u32, cap u8 (slots owned), n_slots u8, stop u8     (what the walk answers)
  per written slot, in session order: start u32 (from the call's first byte), ret i32, result i8, num_headers u16
  hdr u16 [H, 4]: name_off (RHP_NAME_NULL: name == NULL), name_len, value_off, value_len: num_headers records of every
                  written slot with ret > 0, one slot after the other
  per present field: f_slot u32 (the slot's index in the call, 0 .. n_slots_total), f_name u8 (the name's index in the
                  set's list), f_off, f_len u16.  Every other field of the call is {RHP_NAME_NULL, 0}.
usage: python tests/golden/make_golden_walk_lookup.py
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
import walk_lookup_sets as wl  # noqa: E402
import walk_resume_sets as wr  # noqa: E402
import make_golden_decode_chunked as mdc  # noqa: E402
from make_golden_frame_messages import composer  # noqa: E402
from make_golden_messages import reference  # noqa: E402
from make_golden_walk import walker  # noqa: E402
from make_golden_walk_resume import round_walker, state_array, state_tuples  # noqa: E402

GOLDEN = os.path.join(HERE, "walk_lookup.npz")


def main():
    ref, ref_chunked = reference(), mdc.reference()
    walk_once, walk_round, compose = walker(ref, ref_chunked), round_walker(ref, ref_chunked), composer(ref)
    S = dict(name=[], maxh=[], flags=[], nsess=[], resume=[], call=[0], first=[0], names=[0])
    spans, text, states_in, chunks = [], b"", [], []
    call_q, call_w, call_f, call_byte = [0], [0], [0], [0]
    Q = {k: [] for k in ("len", "cap", "n_slots", "stop")}
    W = {k: [] for k in ("start", "ret", "result", "num_headers")}
    F = {k: [] for k in ("f_slot", "f_name", "f_off", "f_len")}
    hdr = []

    def record(buf, off, sl, maxh, names, res, rows_all):
        """one call: what the walk answered, and the reference's lookup over every head slot"""
        nbytes = int(off[-1])
        chunks.append(buf[:nbytes].copy())
        for s, (r, rows) in enumerate(zip(res, rows_all)):
            Q["len"].append(int(off[s + 1] - off[s])); Q["cap"].append(int(sl[s + 1] - sl[s]))
            Q["n_slots"].append(r[0]); Q["stop"].append(r[1])
            for k, (start, _, _, result, _, msg, recs) in enumerate(rows):
                W["start"].append(start); W["ret"].append(msg[0]); W["result"].append(result); W["num_headers"].append(msg[5] if msg[0] > 0 else 0)
                hdr.extend(recs)
                if result != 1 or msg[0] <= 0:
                    continue
                ret, _, _, _, fields = compose(rhp.MSG_RESPONSE, buf, start, int(off[s + 1]) - start, maxh, names)
                assert ret == msg[0]
                for j, (vo, vl) in enumerate(fields):
                    if vo != rhp.RHP_NAME_NULL:
                        F["f_slot"].append(int(sl[s]) + k); F["f_name"].append(j); F["f_off"].append(vo); F["f_len"].append(vl)
        call_q.append(len(Q["len"])); call_w.append(len(W["ret"])); call_f.append(len(F["f_slot"]))
        call_byte.append(call_byte[-1] + nbytes)

    for name, maxh, flags, resume, deliveries, caps, states, names in wl.all_sets():
        n = len(deliveries[0])
        f0 = len(F["f_slot"])
        if not resume:
            buf, off = wl.ws.pack(deliveries[0])
            sl = wl.ws.slot_offsets(caps[0])
            out = buf.copy()
            got = [walk_once(buf, out, int(off[s]), int(off[s + 1]), caps[0][s], maxh, flags) for s in range(n)]
            record(buf, off, sl, maxh, names, [g[0] for g in got], [g[1] for g in got])
        else:
            if states is not None:
                states_in.append(states.view(np.uint8).reshape(-1).copy())

            def step(buf, off, sl, sts, maxh_, flags_):
                out = buf.copy()
                tup = state_tuples(sts)
                got = [walk_round(buf, out, int(off[s]), int(off[s + 1]), int(sl[s + 1] - sl[s]), maxh_, flags_, tup[s]) for s in range(n)]
                record(buf, off, sl, maxh_, names, [g[0] for g in got], [g[1] for g in got])
                after = [tup[s] if g[2] is None else g[2] for s, g in enumerate(got)]
                return np.array([g[0] for g in got], dtype=rhp.WALK_RESULT_DTYPE), None, None, None, out, state_array(after)

            wr.walk_rounds(step, deliveries, caps, maxh, flags, states if states is not None else np.zeros(n, dtype=wr.STATE_DTYPE))
        S["name"].append(name); S["maxh"].append(maxh); S["flags"].append(flags); S["nsess"].append(n); S["resume"].append(int(resume))
        S["call"].append(len(call_q) - 1); S["first"].append(S["first"][-1] + (n if states is not None else 0))
        for x in names:
            spans.append((len(text), len(x)))
            text += bytes(x)
        S["names"].append(len(spans))
        print(f"{name}: {n} sessions, {len(deliveries)} calls, max_headers {maxh}, flags {flags}, {len(names)} names: "
              f"{len(F['f_slot']) - f0} fields present")
    arr = lambda a, dt: np.array(a, dtype=dt)
    out = dict(set_name=np.array(S["name"]), set_maxh=arr(S["maxh"], np.uint32), set_flags=arr(S["flags"], np.uint32),
               set_nsess=arr(S["nsess"], np.uint32), set_resume=arr(S["resume"], np.uint8), set_call=arr(S["call"], np.uint32),
               set_first=arr(S["first"], np.uint32), states_in=np.concatenate(states_in), set_names=arr(S["names"], np.uint32),
               name_span=arr(spans, np.uint32).reshape(-1, 2), name_text=np.frombuffer(text, dtype=np.uint8),
               call_q=arr(call_q, np.uint32), call_w=arr(call_w, np.uint32), call_f=arr(call_f, np.uint32),
               call_byte=arr(call_byte, np.uint64), bytes=np.concatenate(chunks), hdr=arr(hdr, np.uint16).reshape(-1, 4))
    types = dict(len=np.uint32, cap=np.uint8, n_slots=np.uint8, stop=np.uint8, start=np.uint32, ret=np.int32, result=np.int8,
                 num_headers=np.uint16, f_slot=np.uint32, f_name=np.uint8, f_off=np.uint16, f_len=np.uint16)
    for T in (Q, W, F):
        for k, v in T.items():
            out[k] = arr(v, types[k])
    np.savez(GOLDEN, **out)
    size, limit = os.path.getsize(GOLDEN), os.path.getsize(os.path.join(HERE, "walk_responses.npz"))
    print(f"{GOLDEN}: {len(S['name'])} sets, {len(call_q) - 1} calls, {len(Q['len'])} session-calls, {len(W['ret'])} written slots, "
          f"{len(hdr)} header records, {len(F['f_slot'])} fields present, {size} bytes")
    assert size <= limit, f"the file is no larger than walk_responses.npz ({limit} bytes)"


if __name__ == "__main__":
    main()
