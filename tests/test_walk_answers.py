"""rhp_walk_answers (include/rhp.h): the response walk told which of the session's outstanding requests were HEAD --
a HEAD's reply has the framing headers of the GET's reply and no body -- and telling which request each slot answers.

The expected answers are in tests/golden/walk_answers.npz, written by tests/golden/make_golden_walk_answers.py: the
rounds stated in plain Python with the call's own rules, every parse, lookup, number and chunked decode in them the
compiled reference's, for every round of every set of tests/walk_answer_sets.py.  Held to them, value for value:
  CPU  the host twin rhp_cpu_walk_answers on every round alone and on every chain through the driver
       (walk_answer_sets.answer_rounds), with and without RHP_WALK_DEFRAME; the live reference where
       oracle/_ref/libref.so is built; with every bit clear the files of the two walks it runs and the cases at the
       readable end; the HEAD rule stated here in plain Python over hand-built inputs; the refusals of
       rhp_walk_args.h; rhp_lookup_walked over a HEAD reply; a sanitizer build of the twin as a stand-alone program
  GPU  the kernels on every round of every set and on every chain with the states left on the device, outputs
       poisoned first and guard bytes on both sides of every buffer; n_sessions 1, 255, 256, 257; slot_req == NULL;
       the kernel against the twin on a seeded mix of 512 sessions over three rounds; the equivalence again
Compared: every field of results; every field of the slots a session wrote and their ret; slots past n_slots keep
their poison, in slot_req too; answered; slot_req; the states, byte for byte; the bytes.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import walk_answer_sets as wa
import walk_resume_sets as wr
import walk_sets as ws

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "walk_answers.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
GUARD = 256
SLOT_FIELDS = ("start", "body_len", "wire_len", "result", "body_kind")
Q_FIELDS = ("len", "cap", "n_slots", "stop", "consumed", "kept", "st_phase", "st_ct", "st_hex", "st_state", "st_left", "answered")
POISON32 = int.from_bytes(bytes([rhp.WALK_POISON]) * 4, "little")
E, H, B, Y, C, M = range(6)   # enum rhp_walk_stop


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    g["deframed"] = g["bytes"].copy()
    g["deframed"][g["defr_idx"]] = g["defr_val"]
    return g


SET_NAMES = [str(x) for x in golden()["set_name"]]
state_bytes = lambda states: np.ascontiguousarray(states).view(np.uint8).reshape(len(states), 32)


@functools.lru_cache(maxsize=None)
def golden_set(name):
    """(max_headers, flags, mode, [round]); a round: dict of buf and deframed (u8, RHP_PAD zero bytes behind the
    sessions), sess_off, slot_off, req_off, head_bits, n_req_total, states_in, states_out and the expected columns,
    the per-slot ones spread over the slots the sessions own (written: 1 where the session wrote the slot)"""
    g = golden()
    s = SET_NAMES.index(name)
    n = int(g["set_nsess"][s])
    f0, f1 = int(g["set_first"][s]), int(g["set_first"][s + 1])
    states = (g["states_in"][32 * f0: 32 * f1].copy().view(rhp.WALK_STATE_DTYPE) if f1 > f0 else np.zeros(n, dtype=rhp.WALK_STATE_DTYPE))
    rounds = []
    for r in range(int(g["set_round"][s]), int(g["set_round"][s + 1])):
        q0, q1 = int(g["round_q"][r]), int(g["round_q"][r + 1])
        t0, b0, b1 = int(g["round_slot"][r]), int(g["round_byte"][r]), int(g["round_byte"][r + 1])
        assert q1 - q0 == n
        x = {k: g[k][q0:q1].copy() for k in Q_FIELDS}
        pad = np.zeros(ws.RHP_PAD, dtype=np.uint8)
        x["buf"], x["deframed"] = np.concatenate([g["bytes"][b0:b1], pad]), np.concatenate([g["deframed"][b0:b1], pad])
        x["sess_off"] = np.concatenate([[0], np.cumsum(x["len"].astype(np.uint64))]).astype(np.uint64)
        x["slot_off"] = ws.slot_offsets(x["cap"].astype(np.uint64))
        x["req_off"] = g["req_off"][q0 + r: q0 + r + n + 1].copy()
        x["head_bits"] = g["head_words"][int(g["round_word"][r]): int(g["round_word"][r + 1])].copy()
        x["n_req_total"] = int(g["round_nreq"][r])
        nt = int(x["slot_off"][-1])
        where = np.concatenate([int(x["slot_off"][i]) + np.arange(int(x["n_slots"][i])) for i in range(n)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        x["written"] = np.zeros(nt, dtype=np.uint8)
        x["written"][where] = 1
        for k in SLOT_FIELDS + ("ret", "status", "slot_req"):
            col = np.zeros(nt, dtype=np.uint64 if k in ("start", "body_len", "wire_len") else np.int64)
            col[where] = g[k][t0: t0 + len(where)]
            x[k] = col
        x["slot_req"] = np.where(x["slot_req"] < 0, wa.REQ_NONE, x["slot_req"])
        out = np.zeros(n, dtype=rhp.WALK_STATE_DTYPE)
        out["phase"] = x["st_phase"]
        out["left"] = np.where(x["st_phase"] == wr.IN_LENGTH, x["st_left"], 0)
        out["decoder"]["bytes_left_in_chunk"] = np.where(x["st_phase"] == wr.IN_CHUNKED, x["st_left"], 0)
        for col, f in (("st_ct", "consume_trailer"), ("st_hex", "hex_count"), ("st_state", "state")):
            out["decoder"][f] = x[col]
        kept = x["kept"] == 1
        out[kept] = states[kept]
        x["states_in"], x["states_out"] = states, out
        for a in x.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        rounds.append(x)
        states = out
    return int(g["set_maxh"][s]), int(g["set_flags"][s]), int(g["set_mode"][s]), rounds


def named(out, mode):
    """what rhp.walk_answers_cpu / _gpu returned, by name"""
    d = dict(zip(("results", "slots", "msgs", "hdrs", "bytes"), out[:5]))
    rest = list(out[5:])
    if mode:
        d["states"] = rest.pop(0)
    d["answered"], d["slot_req"] = rest[0], rest[1]
    if len(rest) > 2:
        d["carry"] = rest[2]
    return d


def call(fn, x, maxh, flags, mode, states="file", **kw):
    st = x["states_in"] if states == "file" else states
    return named(fn(x["buf"], x["sess_off"], x["slot_off"], x["req_off"], x["head_bits"], st if mode else None, bool(mode), maxh, flags,
                    n_req_total=x["n_req_total"], **kw), mode)


def check(name, r, d, what, deframe, slot_req=True):
    """what one round returned against round r of the set in the golden file"""
    _, _, mode, rounds = golden_set(name)
    x = rounds[r]
    what = f"{what} {name} round {r}"
    results, slots, msgs = d["results"], d["slots"], d["msgs"]
    assert len(results) == len(x["len"]) and len(slots) == len(msgs) == int(x["slot_off"][-1])
    for f in ("n_slots", "stop", "consumed"):
        bad = np.flatnonzero(results[f] != x[f])
        assert not len(bad), f"{what}: {f} of session {int(bad[0])} is {int(results[f][bad[0]])}, the reference's {int(x[f][bad[0]])} ({len(bad)} differ)"
    bad = np.flatnonzero(d["answered"] != x["answered"])
    assert not len(bad), f"{what}: answered of session {int(bad[0])} is {int(d['answered'][bad[0]])}, the reference's {int(x['answered'][bad[0]])}"
    w = x["written"] == 1
    for f in SLOT_FIELDS:
        bad = np.flatnonzero(w & (slots[f].astype(x[f].dtype) != x[f]))
        assert not len(bad), f"{what}: {f} of slot {int(bad[0])} is {int(slots[f][bad[0]])}, the reference's {int(x[f][bad[0]])} ({len(bad)} differ)"
    bad = np.flatnonzero(w & (msgs["ret"] != x["ret"]))
    assert not len(bad), f"{what}: ret of slot {int(bad[0])} is {int(msgs['ret'][bad[0]])}, the reference's {int(x['ret'][bad[0]])}"
    ok = w & (x["ret"] > 0)
    assert (msgs["status"][ok] == x["status"][ok]).all()
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    for a, label in ((slots, "slot"), (msgs, "message record"), (d["hdrs"], "header records")):
        if a.size:
            assert (raw(a)[~w] == rhp.WALK_POISON).all(), f"{what}: a {label} past n_slots was written"
    if slot_req:
        sr = d["slot_req"]
        bad = np.flatnonzero(w & (sr != x["slot_req"]))
        assert not len(bad), f"{what}: slot_req of slot {int(bad[0])} is {int(sr[bad[0]])}, the reference's {int(x['slot_req'][bad[0]])}"
        assert (sr[~w] == POISON32).all(), f"{what}: a slot_req entry past n_slots was written"
    else:
        assert d["slot_req"] is None
    if mode:
        bad = np.flatnonzero((state_bytes(d["states"]) != state_bytes(x["states_out"])).any(axis=1))
        assert not len(bad), (f"{what}: the state of session {int(bad[0])} is {d['states'][bad[0]]}, the reference's "
                              f"{x['states_out'][bad[0]]} ({len(bad)} differ)")
    want = x["deframed"] if deframe else x["buf"]
    bad = np.flatnonzero(d["bytes"] != want)
    assert not len(bad), f"{what}: byte {int(bad[0])} is {int(d['bytes'][bad[0]])}, not {int(want[bad[0]])} ({len(bad)} differ)"


def set_plan(name):
    return next(s for s in wa.all_sets() if s["name"] == name)


def chain(fn, s, deframe, **kw):
    """the set's rounds through the driver over fn (rhp.walk_answers_cpu / _gpu)"""
    def step(buf, off, sl, states, req_off, head_bits, total):
        return named(fn(buf, off, sl, req_off, head_bits, states if s["mode"] else None, bool(s["mode"]), s["maxh"], s["flags"] | deframe,
                        n_req_total=total, **kw), s["mode"])
    return wa.answer_rounds(step, s)


def slot_rows(x, s):
    """(stop, answered, [(result, body_kind, body_len, wire_len, slot_req)] of the written slots) of session s of a round"""
    lo = int(x["slot_off"][s])
    rows = [(int(x["result"][k]), int(x["body_kind"][k]), int(x["body_len"][k]), int(x["wire_len"][k]), int(x["slot_req"][k]))
            for k in range(lo, lo + int(x["n_slots"][s]))]
    return int(x["stop"][s]), int(x["answered"][s]), rows


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_sets():
    """the file's sets, bytes, offsets, capacities, queues and first states are what tests/walk_answer_sets.py builds,
    the rounds made by the driver from the file's own consumed and answered counts; it is no larger than walk_resume.npz"""
    sets = wa.all_sets()
    assert [s["name"] for s in sets] == SET_NAMES
    for s in sets:
        gm, gf, mode, rounds = golden_set(s["name"])
        assert (gm, gf, mode, len(rounds)) == (s["maxh"], s["flags"], s["mode"], len(s["deliveries"])), s["name"]
        it = iter(rounds)

        def step(buf, off, sl, st, req_off, head_bits, total):
            x = next(it)
            assert (buf == x["buf"]).all() and (off == x["sess_off"]).all() and (sl == x["slot_off"]).all(), s["name"]
            assert (req_off == x["req_off"]).all() and (head_bits == x["head_bits"]).all() and total == x["n_req_total"], s["name"]
            assert st is None or (state_bytes(st) == state_bytes(x["states_in"])).all(), s["name"]
            res = np.zeros(len(off) - 1, dtype=rhp.WALK_RESULT_DTYPE)
            res["consumed"] = x["consumed"]
            return dict(results=res, states=x["states_out"], answered=x["answered"])

        wa.answer_rounds(step, s)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "walk_resume.npz"))


def test_golden_covers():
    """each situation the sets exist for is in the file"""
    L, CH, NO, NONE = rhp.FRAME_LENGTH, rhp.FRAME_CHUNKED, rhp.FRAME_NONE, wa.REQ_NONE
    one = lambda name: golden_set(name)[3][0]
    # 1: a HEAD reply with Content-Length 5: no body, the GET reply behind it is walked
    x = one("head_length")
    assert slot_rows(x, 0) == (E, 2, [(1, L, 0, 0, 0), (1, L, 5, 5, 1)])
    assert slot_rows(x, 2) == (E, 3, [(1, L, 0, 0, 0), (1, L, 0, 0, 1), (1, L, 5, 5, 2)])
    # 2: ... with Transfer-Encoding: chunked; the de-framing moves bytes only in the session whose body is there
    x = one("head_chunked")
    assert slot_rows(x, 0) == (E, 2, [(1, CH, 0, 0, 0), (1, L, 5, 5, 1)])
    moved = np.flatnonzero(x["buf"] != x["deframed"])
    assert len(moved) and (moved >= int(x["sess_off"][1])).all() and slot_rows(x, 2)[2][2] == (1, CH, 0, 0, 2)
    # 3: ... with neither header, RHP_WALK_NONE_EMPTY clear; without the bit the same bytes stop with CLOSE
    x = one("head_bare")
    assert golden_set("head_bare")[1] & ws.NONE_EMPTY == 0
    assert slot_rows(x, 0) == (E, 2, [(1, NO, 0, 0, 0), (1, L, 5, 5, 1)]) and slot_rows(x, 1)[:2] == (C, 1)
    # 4: interim responses take a slot, answer nothing and name the request they precede
    x = one("interim")
    assert slot_rows(x, 0) == (E, 1, [(1, NO, 0, 0, 0), (1, L, 0, 0, 0)]), "100 Continue, then the HEAD's final reply"
    assert slot_rows(x, 1) == (E, 1, [(1, NO, 0, 0, 0), (1, NO, 0, 0, 0), (1, L, 5, 5, 0)]), "two 103s, then a final reply"
    assert slot_rows(x, 2) == (E, 1, [(1, NO, 0, 0, 0), (1, L, 5, 5, 0)]) and int(x["status"][int(x["slot_off"][2])]) == 101
    assert [r[4] for r in slot_rows(x, 3)[2]] == [0, 0, 1, 1] and slot_rows(x, 4) == (E, 0, [(1, NO, 0, 0, 0)])
    # 5: a HEAD bit on a 204 and a 304: the same slots as without it, and k advances
    x = one("head_no_body_status")
    assert slot_rows(x, 0) == slot_rows(x, 1) and slot_rows(x, 0)[1] == 2
    assert [int(x["status"][int(x["slot_off"][s])]) for s in (0, 2)] == [204, 304]
    assert slot_rows(x, 2) == slot_rows(x, 3) == (E, 3, [(1, L, 0, 0, 0), (1, L, 0, 0, 1), (1, L, 5, 5, 2)])
    # 6: bit addressing
    x = one("bits_from_30")
    assert x["req_off"].tolist() == [30, 33, 36, 69, 70, 71] and len(x["head_bits"]) == 3
    assert [[r[2] for r in slot_rows(x, s)[2]] for s in (0, 1)] == [[5, 0, 0], [0, 5, 5]], "a queue across the word's end; opposite bits beside it"
    assert [r[2] for r in slot_rows(x, 2)[2]] == [5] * 32 + [0] and slot_rows(x, 2)[1] == 33, "33 requests, only the last a HEAD"
    assert [slot_rows(x, s)[2][0][2] for s in (3, 4)] == [0, 5]
    x = one("bits_from_32")
    assert int(x["req_off"][0]) == 32 and [[r[2] for r in slot_rows(x, s)[2]] for s in range(3)] == [[0, 5], [5, 0], [0, 0, 5]]
    # 7: more final responses than requests; no request; a pair out of order; a pair beyond n_req_total
    x = one("unasked")
    assert slot_rows(x, 0) == (E, 3, [(1, L, 0, 0, 0), (1, L, 5, 5, 1), (1, L, 5, 5, 2)]) and x["req_off"][1] - x["req_off"][0] == 1
    assert slot_rows(x, 1)[:2] == (E, 1) and x["req_off"][2] == x["req_off"][1] and slot_rows(x, 2) == (E, 0, [])
    assert x["req_off"][4] < x["req_off"][3] and slot_rows(x, 3) == (E, 2, [(1, L, 5, 5, 0), (1, L, 5, 5, 1)])
    x = one("unasked_beyond")
    assert x["req_off"][2] > x["n_req_total"] and slot_rows(x, 1) == (E, 2, [(1, L, 5, 5, 0), (1, L, 5, 5, 1)])
    assert (x["head_bits"] >> 1 & 1).all() and slot_rows(x, 0)[2][0][2] == 0
    # 8: a HEAD reply whose Content-Length exceeds the rest of the session: END, not BODY
    x = one("head_length_exceeds")
    assert slot_rows(x, 0) == (E, 1, [(1, L, 0, 0, 0)]) and slot_rows(x, 1) == (E, 2, [(1, L, 0, 0, 0), (1, L, 5, 5, 1)])
    assert slot_rows(x, 2) == (Y, 1, [(1, L, 500, 0, 0)])
    # 9: a HEAD reply the framing answers -1 to is still BAD and answers nothing
    x = one("head_bad_length")
    assert slot_rows(x, 0) == (B, 0, [(-1, NO, 0, 0, NONE)]) and slot_rows(x, 2) == (B, 0, [(-1, NO, 0, 0, NONE)])
    assert slot_rows(x, 1) == (B, 1, [(1, L, 0, 0, 0), (-1, NO, 0, 0, NONE)])
    # 10: the slots run out after the first of three replies
    x = one("more")
    assert slot_rows(x, 0) == (M, 1, [(1, L, 0, 0, 0)]) and slot_rows(x, 1)[:2] == (M, 2) and slot_rows(x, 2) == (M, 0, [(1, NO, 0, 0, 0)])
    # 11: the resumed walk
    r0, r1, r2 = golden_set("resume_chains")[3]
    assert slot_rows(r0, 0) == (H, 0, [(0, NO, 0, 0, NONE)]) and slot_rows(r1, 0) == (E, 2, [(1, L, 0, 0, 0), (1, L, 5, 5, 1)])
    assert r0["head_bits"][0] & 1 and r1["head_bits"][0] & 1, "the same bit is used again"
    assert slot_rows(r0, 1) == (Y, 1, [(1, L, 10, 5, 0)]), "a GET reply is counted at its head"
    assert slot_rows(r1, 1) == (E, 2, [(1, L, 5, 5, NONE), (1, L, 0, 0, 0), (1, L, 5, 5, 1)]), "the continuation answers nothing; bit 0 of the new queue"
    for s in (2, 3):
        assert slot_rows(r0, s) == (B, 0, []) and r0["kept"][s] == 1, "a dead and a corrupt state"
    assert slot_rows(r0, 4) == (Y, 0, []) and r0["kept"][4] == 1 and slot_rows(r1, 4) == (E, 1, [(1, L, 5, 5, NONE), (1, L, 0, 0, 0)])
    assert slot_rows(r1, 5) == (M, 0, []) and r1["kept"][5] == 1 and int(r1["states_out"]["phase"][5]) == wr.IN_LENGTH
    assert slot_rows(r2, 5) == (E, 1, [(1, L, 5, 5, NONE), (1, L, 0, 0, 0)])
    for s in (6, 7, 8):
        assert slot_rows(r0, s)[:2] == (E, 1) and int(r0["states_out"]["phase"][s]) == wr.AT_HEAD, "no state is armed"
        assert slot_rows(r1, s) == (E, 1, [(1, L, 5, 5, 0)])
    assert slot_rows(r0, 9) == (E, 0, [(1, NO, 0, 0, 0)]) and slot_rows(r1, 9)[:2] == (H, 1)
    assert slot_rows(r0, 10)[:2] == (Y, 1) and [r[4] for r in slot_rows(r1, 10)[2]] == [NONE, 0, 1]
    x = golden_set("resume_one_round")[3][0]
    assert [slot_rows(x, s)[0] for s in range(5)] == [E, E, E, E, Y] and int(x["states_out"]["phase"][4]) == wr.IN_LENGTH
    assert {int(m) for m in golden()["set_mode"]} == {0, 1}


DEFRAMES = [0, ws.DEFRAME]


@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_twin_equals_golden(name, deframe):
    """every round alone, from the file's bytes, queues and states"""
    maxh, flags, mode, rounds = golden_set(name)
    for r, x in enumerate(rounds):
        check(name, r, call(rhp.walk_answers_cpu, x, maxh, flags | deframe, mode), "rhp_cpu_walk_answers", deframe)
    check(name, 0, call(rhp.walk_answers_cpu, rounds[0], maxh, flags | deframe, mode, slot_req=False), "rhp_cpu_walk_answers (no slot_req)",
          deframe, slot_req=False)


@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_chain_equals_golden(name, deframe):
    """the chain through the driver, every round fed from the twin's own answers"""
    for r, rnd in enumerate(chain(rhp.walk_answers_cpu, set_plan(name), deframe)):
        check(name, r, rnd[6], "rhp_cpu_walk_answers (chained)", deframe)


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
def test_golden_equals_live_reference():
    """the maker's rounds over the compiled reference, run now, against the file"""
    from golden import make_golden_decode_chunked as mdc
    from golden.make_golden_messages import reference
    from golden.make_golden_walk_answers import answer_walker, reference_round
    from golden.make_golden_walk_resume import state_array
    walk = answer_walker(reference(), mdc.reference())
    for name in SET_NAMES:
        maxh, flags, mode, rounds = golden_set(name)
        for r, x in enumerate(rounds):
            out, res, rows_all, after, kept, answered, sreq = reference_round(walk, mode, maxh, flags, x["buf"].copy(), x["sess_off"], x["slot_off"],
                                                                              x["states_in"], x["req_off"], x["head_bits"], x["n_req_total"])
            assert (out == x["deframed"]).all() and answered == x["answered"].tolist(), (name, r)
            for s in range(len(res)):
                lo = int(x["slot_off"][s])
                assert res[s] == (int(x["n_slots"][s]), int(x["stop"][s]), int(x["consumed"][s])), (name, r, s)
                for k, (row, sr) in enumerate(zip(rows_all[s], sreq[s])):
                    assert row[:5] == tuple(int(x[f][lo + k]) for f in SLOT_FIELDS) and row[5][0] == int(x["ret"][lo + k]), (name, r, s, k)
                    assert (wa.REQ_NONE if sr < 0 else sr) == int(x["slot_req"][lo + k]), (name, r, s, k)
            if mode:
                assert kept == [bool(v) for v in x["kept"]] and (state_bytes(state_array(after)) == state_bytes(x["states_out"])).all(), (name, r)


def clear_queues(n, rng=None):
    """queues with every bit clear: req_off of seeded lengths (or none), the words zero"""
    lens = rng.integers(0, 5, size=n) if rng is not None else np.zeros(n, dtype=np.int64)
    req_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    return req_off, np.zeros((int(req_off[-1]) + 31) // 32 + 1, dtype=np.uint32)


def same_as_old(new, old, mode, what):
    """every output the old call has, byte for byte"""
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    for k in range(6 if mode else 5):
        assert (raw(new[k]) == raw(old[k])).all(), f"{what}: output {k} differs from the walk's with every bit clear"


def equivalence(part, fn_new, fn_old_one, fn_old_resume, **kw):
    """with every bit clear, and with every nq == 0, the call leaves what rhp_walk_responses / rhp_walk_resume leave:
    over walk_responses.npz, walk_resume.npz and the cases of walk_edges.npz (part: which of them)"""
    import test_walk_responses as t1
    import test_walk_resume as t2
    import test_walk_edges as t3
    rng = np.random.default_rng(5)
    if part == "responses":
        for name in t1.SET_NAMES:
            maxh, flags, buf, _, sess_off, slot_off, _ = t1.golden_set(name)
            for deframe in DEFRAMES:
                old = fn_old_one(buf, sess_off, slot_off, maxh, flags | deframe, **kw)
                for q in (clear_queues(len(sess_off) - 1, rng), clear_queues(len(sess_off) - 1)):
                    new = fn_new(buf, sess_off, slot_off, q[0], q[1], None, False, maxh, flags | deframe, **kw)
                    same_as_old(new, old, 0, f"walk_responses.npz {name}")
    elif part == "resume":
        for name in t2.SET_NAMES:
            maxh, flags, rounds = t2.golden_set(name)
            for x in rounds:
                old = fn_old_resume(x["buf"], x["sess_off"], x["slot_off"], x["states_in"], maxh, flags | ws.DEFRAME, **kw)
                q = clear_queues(len(x["len"]), rng)
                new = fn_new(x["buf"], x["sess_off"], x["slot_off"], q[0], q[1], x["states_in"], True, maxh, flags | ws.DEFRAME, **kw)
                same_as_old(new, old, 1, f"walk_resume.npz {name}")
    else:
        g3 = t3.golden()
        for i in t3.cases_of(*part):
            c = t3.golden_case(i)
            a = (c["buf"], c["sess_off"], c["slot_off"])
            o = dict(max_headers=int(g3["max_headers"][0]), flags=int(g3["flags"][0]) | ws.DEFRAME, bytes_size=c["size"], **kw)
            q = clear_queues(t3.NSESS, rng)
            what = f"walk_edges.npz case {i} ({c['kind']})"
            if c["call"] == t3.we.RESUME:
                same_as_old(fn_new(*a, q[0], q[1], c["states_in"], True, **o), fn_old_resume(*a, c["states_in"], **o), 1, what)
            else:
                same_as_old(fn_new(*a, q[0], q[1], None, False, **o), fn_old_one(*a, **o), 0, what)


def equivalence_parts():
    import test_walk_edges as t3
    return ["responses", "resume"] + list(t3.CALL_KINDS), ["walk_responses.npz", "walk_resume.npz"] + [f"walk_edges.npz-{i}" for i in t3.IDS]


@pytest.mark.parametrize("part", equivalence_parts()[0], ids=equivalence_parts()[1])
def test_cpu_equivalence_with_every_bit_clear(part):
    equivalence(part, rhp.walk_answers_cpu, rhp.walk_responses_cpu, rhp.walk_resume_cpu)


def head_rule(status, kind, body_len, avail, is_head, none_empty):
    """the body step of a final or interim head, in plain Python: (body_len, wire_len, stop)"""
    if 100 <= status <= 199 or status in (204, 304) or is_head:
        return 0, 0, E
    if kind == rhp.FRAME_LENGTH:
        return body_len, min(body_len, avail), Y if body_len > avail else E
    assert kind == rhp.FRAME_NONE
    return (0, 0, E) if none_empty else (0, avail, C)


@pytest.mark.parametrize("none_empty", [0, ws.NONE_EMPTY])
def test_cpu_head_rule_on_hand_built_inputs(none_empty):
    """one session per (status, framing, tail, HEAD or not), the queue one request each: the slot is the rule's"""
    cases = [(st, cl, tail, h) for st in (200, 404, 100, 204, 304, 199, 205) for cl in (None, 0, 3, 40) for tail in (b"", b"abc", b"abcdefgh")
             for h in (0, 1)]
    sessions = [ws.resp([b"Content-Length: %d" % cl] if cl is not None else [], tail, status=b"HTTP/1.1 %d X" % st) for st, cl, tail, _ in cases]
    buf, off = ws.pack(sessions)
    req_off, head_bits, total = wa.pack_queues([[h] for *_, h in cases])
    d = named(rhp.walk_answers_cpu(buf, off, ws.slot_offsets([1] * len(cases)), req_off, head_bits, None, False, 4, none_empty), 0)
    for i, (st, cl, tail, h) in enumerate(cases):
        kind = rhp.FRAME_NONE if cl is None else rhp.FRAME_LENGTH
        body_len, wire_len, stop = head_rule(st, kind, cl or 0, len(tail), h, none_empty)
        if stop == E and wire_len < len(tail):
            stop = M          # the one slot is used and bytes are left
        x = d["slots"][i]
        assert (int(x["result"]), int(x["body_kind"]), int(x["body_len"]), int(x["wire_len"]), int(d["results"]["stop"][i])) == \
            (1, kind, body_len, wire_len, stop), (st, cl, tail, h)
        assert int(d["slot_req"][i]) == 0 and int(d["answered"][i]) == (0 if 100 <= st <= 199 else 1), (st, cl, tail, h)


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU): what the walk refuses, a NULL
    x, reserved != 0, a NULL req_off or answered, a NULL head_bits with requests, and on the device any of the four
    not 4-byte aligned.  Only refused calls and n_sessions == 0 go to the GPU library here"""
    gpu = which == "gpu-library"
    fn = ((lambda w, st, x: rhp.lib().rhp_walk_answers(w, st, x, None)) if gpu else (lambda w, st, x: rhp.host().rhp_cpu_walk_answers(w, st, x)))
    al = lambda nbytes, fill: (lambda r: r[(-r.ctypes.data) % 16:][:nbytes])(np.full(nbytes + 16, fill, dtype=np.uint8))
    buf = al(512, 0)
    buf[: len(wa.HEAD5)] = np.frombuffer(wa.HEAD5, dtype=np.uint8)
    so = np.array([0, len(wa.HEAD5), len(wa.HEAD5)], dtype=np.uint64)
    sl = np.array([0, 2, 4], dtype=np.uint64)
    msgs, hdrs, slots, results, states = al(64, 0x77), al(4 * 4 * 8, 0x77), al(128, 0x77), al(32, 0x77), al(64, 0)
    req_off, head_bits, answered, slot_req = al(12, 0), al(4, 0), al(8, 0x77), al(16, 0x77)
    req_off.view(np.uint32)[:] = [0, 1, 1]
    head_bits.view(np.uint32)[:] = [1]
    p = lambda a: a.ctypes.data
    STATES = object()

    def go(states_=None, x_=True, **kw):
        a = dict(bytes=p(buf), bytes_rw=p(buf), bytes_size=512, sess_off=p(so), slot_off=p(sl), n_sessions=2, n_slots_total=4,
                 max_headers=4, flags=0, msgs=p(msgs), hdrs=p(hdrs), slots=p(slots), results=p(results))
        b = dict(req_off=p(req_off), head_bits=p(head_bits), n_req_total=1, reserved=0, answered=p(answered), slot_req=p(slot_req))
        a.update({k: v for k, v in kw.items() if k in a})
        b.update({k: v for k, v in kw.items() if k in b})
        x = rhp.WalkAsked(*(b[k] for k, _ in rhp.WalkAsked._fields_))
        return fn(ctypes.byref(rhp.WalkBatch(*(a[k] for k, _ in rhp.WalkBatch._fields_))), p(states) if states_ is STATES else states_,
                  ctypes.byref(x) if x_ else None)

    EINVAL = -22
    x_ok = rhp.WalkAsked(p(req_off), p(head_bits), 1, 0, p(answered), p(slot_req))
    assert fn(None, None, ctypes.byref(x_ok)) == EINVAL and go(x_=False) == EINVAL and go(STATES, x_=False) == EINVAL
    for k in ("bytes", "sess_off", "slot_off", "results", "msgs", "slots", "hdrs"):   # whatever the underlying walk refuses
        assert go(**{k: None}) == EINVAL and go(STATES, **{k: None}) == EINVAL, k
    assert go(flags=8) == EINVAL and go(bytes_size=rhp.RHP_PAD - 1) == EINVAL and go(max_headers=rhp.RHP_MAX_HEADERS + 1) == EINVAL
    assert go(flags=ws.DEFRAME, bytes_rw=None) == EINVAL
    assert go(reserved=1) == EINVAL and go(STATES, reserved=1 << 31) == EINVAL
    assert go(req_off=None) == EINVAL and go(answered=None) == EINVAL and go(head_bits=None) == EINVAL
    assert go(n_sessions=0, reserved=1) == EINVAL and go(n_sessions=0, x_=False) == EINVAL and go(n_sessions=0, flags=8) == EINVAL, \
        "the rules come before the empty call"
    if gpu:
        for k, a in (("req_off", req_off), ("head_bits", head_bits), ("answered", answered), ("slot_req", slot_req)):
            assert go(**{k: p(a) + 2}) == EINVAL and go(STATES, **{k: p(a) + 1}) == EINVAL, k
        assert go(p(states) + 8) == EINVAL and go(results=p(results) + 8) == EINVAL
    untouched = lambda: all((a == 0x77).all() for a in (msgs, hdrs, slots, results, answered, slot_req)) and not states.any()
    assert untouched(), "a refused call writes nothing"
    # accepted: no session asks no pointer and launches nothing
    assert go(n_sessions=0) == 0 and go(STATES, n_sessions=0) == 0
    assert go(n_sessions=0, req_off=None, head_bits=None, answered=None, slot_req=None, n_req_total=0, bytes=None, bytes_rw=None,
              sess_off=None, slot_off=None, msgs=None, hdrs=None, slots=None, results=None, bytes_size=0, n_slots_total=0) == 0
    assert untouched()
    if gpu:
        return
    # accepted by the host twin: a NULL head_bits with no request, a NULL slot_req
    assert go(head_bits=None, n_req_total=0, slot_req=None) == 0
    assert answered.view(np.uint32).tolist() == [1, 0] and (slot_req == 0x77).all()
    assert slots[:32].view(rhp.WALK_SLOT_DTYPE).tolist() == [(0, 5, 0, 1, rhp.FRAME_LENGTH)], "n_req_total 0: nobody asked, a body is awaited"
    assert go(STATES) == 0 and answered.view(np.uint32).tolist() == [1, 0] and slot_req.view(np.uint32).tolist()[:2] == [0, 0x77777777]
    assert slots[:32].view(rhp.WALK_SLOT_DTYPE).tolist() == [(0, 0, 0, 1, rhp.FRAME_LENGTH)] and not states.any()


def test_cpu_lookup_over_a_head_reply():
    """rhp_lookup_walked over the slots of a walk that met a HEAD reply returns its Content-Length field"""
    maxh, flags, mode, rounds = golden_set("head_length")
    x = rounds[0]
    out = rhp.walk_answers_cpu(x["buf"], x["sess_off"], x["slot_off"], x["req_off"], x["head_bits"], None, False, maxh, flags)
    fields = rhp.lookup_walked_cpu(out[:4], x["buf"], x["sess_off"], x["slot_off"], [b"Content-Length"], maxh, flags)
    lo = int(x["slot_off"][0])
    for k, want in ((lo, b"5"), (lo + 1, b"5")):
        f, st = fields[0, k], int(out[1]["start"][k])
        assert bytes(x["buf"][st + int(f["value_off"]): st + int(f["value_off"]) + int(f["value_len"])]) == want
    assert int(out[1]["body_len"][lo]) == 0 and int(fields[0, lo]["value_len"]) == 1, "the field says 5, the walk took no body"


def test_host_twin_asan_ubsan_clean():
    """`make walk-answers-asan`: a stand-alone program over the host sources (tests/walk_answers_host_test.c) that
    runs the rounds of the golden file with the host twin"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    probe = subprocess.run("echo 'int main(void){return 0;}' | gcc -fsanitize=address,undefined -x c - -o /dev/null", shell=True,
                           capture_output=True)
    if probe.returncode != 0:
        pytest.skip("the compiler lacks the sanitizer runtime")
    out = subprocess.run(["make", "-s", "-C", csrc, "walk-answers-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "walk_answers_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernels against the golden file and against the twin


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_equals_golden(name, deframe):
    """every round alone: outputs poisoned first, guard bytes beside every buffer, the queue's among them"""
    maxh, flags, mode, rounds = golden_set(name)
    for r, x in enumerate(rounds):
        check(name, r, call(rhp.walk_answers_gpu, x, maxh, flags | deframe, mode, guard=GUARD), "rhp_walk_answers", deframe)


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", [n for n in SET_NAMES if len(golden_set(n)[3]) > 1])
def test_gpu_chain_equals_golden(name, deframe):
    """the chain through the driver with the states left on the device between rounds"""
    for r, rnd in enumerate(chain(rhp.walk_answers_gpu, set_plan(name), deframe, guard=GUARD)):
        assert "carry" in rnd[6]
        check(name, r, rnd[6], "rhp_walk_answers (chained)", deframe)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["head_chunked", "bits_from_30", "resume_chains"])
def test_gpu_without_slot_req(name):
    """slot_req == NULL: everything else as the file has it"""
    maxh, flags, mode, rounds = golden_set(name)
    for r, x in enumerate(rounds):
        check(name, r, call(rhp.walk_answers_gpu, x, maxh, flags | ws.DEFRAME, mode, guard=GUARD, slot_req=False), "rhp_walk_answers (no slot_req)",
              ws.DEFRAME, slot_req=False)


@functools.lru_cache(maxsize=None)
def twin_mix():
    s = wa.random_mix(512, 20261020)
    return s, chain(rhp.walk_answers_cpu, s, ws.DEFRAME)


def test_cpu_mix_is_a_mix():
    """the seeded mix holds what it is for: HEAD replies of every shape taken without a body, about a quarter of the
    requests HEAD, words of head_bits shared between sessions, every stop code"""
    s, rounds = twin_mix()
    heads = [h for q in s["heads"] for h in q]
    assert 0.15 < sum(heads) / len(heads) < 0.35
    req_off = rounds[0][3]
    assert len(set((req_off[:-1] >> 5).tolist())) < len(req_off) // 4, "many sessions to a word"
    stops = set()
    for *_, out in rounds:
        stops |= set(out["results"]["stop"].tolist())
    assert stops == set(range(6))
    assert sum(int(out["answered"].sum()) for *_, out in rounds) > 800


@pytest.mark.gpu
def test_gpu_equals_twin_on_a_random_mix():
    s, want = twin_mix()
    got = chain(rhp.walk_answers_gpu, s, ws.DEFRAME, guard=GUARD)
    for r, (w, g) in enumerate(zip(want, got)):
        for k, label in ((0, "bytes"), (1, "sess_off"), (3, "req_off"), (4, "head_bits")):
            assert (w[k] == g[k]).all(), f"round {r}: the inputs ({label}) differ, so a round before did"
        wo, go = w[6], g[6]
        for label in ("results", "slots", "bytes", "answered", "slot_req"):
            assert (go[label] == wo[label]).all(), f"round {r}: {label} differ between the kernel and the host twin"
        assert (state_bytes(go["states"]) == state_bytes(wo["states"])).all(), f"round {r}: the states differ"
        assert (go["msgs"]["ret"] == wo["msgs"]["ret"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", wa.GEOMETRY)
def test_gpu_geometry(n):
    """the first n sessions of the mix's first two rounds as batches of their own: the twin's answers"""
    s, want = twin_mix()
    for r in (0, 1):
        buf, off, sl, req_off, head_bits, total, wo = want[r]
        e, t = int(off[n]), int(sl[n])
        b = np.concatenate([buf[:e], np.zeros(ws.RHP_PAD, dtype=np.uint8)])
        st = want[r - 1][6]["states"][:n] if r else None
        d = named(rhp.walk_answers_gpu(b, off[: n + 1], sl[: n + 1], req_off[: n + 1], head_bits, st, True, s["maxh"], s["flags"] | ws.DEFRAME,
                                       guard=GUARD, n_req_total=total), 1)
        assert (d["results"] == wo["results"][:n]).all() and (d["answered"] == wo["answered"][:n]).all(), (n, r)
        assert (d["slots"] == wo["slots"][:t]).all() and (d["slot_req"] == wo["slot_req"][:t]).all(), (n, r)
        assert (state_bytes(d["states"]) == state_bytes(wo["states"][:n])).all() and (d["bytes"][:e] == wo["bytes"][:e]).all(), (n, r)


@pytest.mark.gpu
@pytest.mark.parametrize("part", equivalence_parts()[0], ids=equivalence_parts()[1])
def test_gpu_equivalence_with_every_bit_clear(part):
    equivalence(part, rhp.walk_answers_gpu, rhp.walk_responses_gpu, rhp.walk_resume_gpu, guard=GUARD)


@pytest.mark.gpu
def test_gpu_lookup_over_a_head_reply():
    """walk and lookup on one stream: the HEAD reply's Content-Length field is found where the record lies"""
    import torch
    maxh, flags, mode, rounds = golden_set("head_length")
    x = rounds[0]
    ns, nt = len(x["len"]), int(x["slot_off"][-1])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    db, dso, dsl, dq, dh = dev(x["buf"]), dev(x["sess_off"]), dev(x["slot_off"]), dev(x["req_off"]), dev(x["head_bits"])
    z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    gm, gh, gs, gr, ga, gl, gf = z(16 * nt), z(8 * nt * maxh), z(32 * nt), z(16 * ns), z(4 * ns), z(4 * nt), z(4 * nt)
    rhp.walk_answers_device(db, x["buf"].size, dso, dsl, ns, nt, maxh, flags, gm, gh, gs, gr, None, dq, dh, x["n_req_total"], ga, gl)
    rhp.lookup_walked_device(db, x["buf"].size, dso, dsl, ns, nt, maxh, flags, gm, gh, gs, gr, [b"Content-Length"], gf)
    torch.cuda.synchronize()
    fields = gf.cpu().numpy().view(rhp.FIELDREF_DTYPE)
    starts = gs.cpu().numpy().view(rhp.WALK_SLOT_DTYPE)["start"]
    lo = int(x["slot_off"][0])
    at = int(starts[lo]) + int(fields[lo]["value_off"])
    assert bytes(x["buf"][at: at + int(fields[lo]["value_len"])]) == b"5" and ga.cpu().numpy().view(np.uint32).tolist() == x["answered"].tolist()
