"""rhp_walk_resume (include/rhp.h): the response walk carried across rounds by a 32-byte state per session -- a
round ends inside a Content-Length body, a chunk, a size line or a head, and the next round goes on from there.

The expected answers are in tests/golden/walk_resume.npz, written by tests/golden/make_golden_walk_resume.py: the
rounds stated in plain Python, every parse, lookup, number and chunked decode in them the compiled reference's own
(the chunked decoder's sixteen bytes carried from round to round as the reference left them), for every round of
every set of tests/walk_resume_sets.py.  Held to them, value for value:
  CPU  the host twin rhp_cpu_walk_resume on every round alone and on every chain through the driver
       (walk_resume_sets.walk_rounds), with and without RHP_WALK_DEFRAME; split invariance against
       rhp_cpu_walk_responses over the whole stream; the live reference where oracle/_ref/libref.so is built; the
       refusals of rhp_walk_args.h; sess_off and slot_off rows that hold anything, between guard bytes; a sanitizer
       build of the twin as a stand-alone program
  GPU  the kernel on every round of every set and on every chain with the states left on the device, outputs
       poisoned first and guard bytes on both sides of every buffer; n_sessions 1, 63, 64, 65, 257; the kernel
       against the twin on a seeded mix of 512 sessions over three rounds; rhp_walk_responses as it was
Compared: every field of results; every field of the slots a session wrote; of their message records ret always
and the rest where ret > 0 (a continuation's record: sixteen zero bytes); their header records k < num_headers;
slots past n_slots keep their poison; the states, byte for byte; the bytes.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import walk_resume_sets as wr
import walk_sets as ws

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "walk_resume.npz")
OLD_GOLDEN = os.path.join(HERE, "golden", "walk_responses.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
GUARD = 256
SLOT_FIELDS = ("start", "body_len", "wire_len", "result", "body_kind")
MSG_FIELDS = ("status", "msg_off", "msg_len", "minor", "num_headers")
MSG_COLUMN = {"minor": "minor_version"}
Q_FIELDS = ("len", "cap", "n_slots", "stop", "consumed", "kept", "st_phase", "st_ct", "st_hex", "st_state", "st_left")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    nh = np.where(g["ret"] > 0, g["num_headers"], 0).astype(np.int64)
    g["hdr_lo"] = np.concatenate([[0], np.cumsum(nh)])
    assert g["hdr_lo"][-1] == len(g["hdr"])
    g["deframed"] = g["bytes"].copy()
    g["deframed"][g["defr_idx"]] = g["defr_val"]
    return g


SET_NAMES = [str(x) for x in golden()["set_name"]]


def state_bytes(states):
    return np.ascontiguousarray(states).view(np.uint8).reshape(len(states), 32)


@functools.lru_cache(maxsize=None)
def golden_set(name):
    """(max_headers, flags, [round]); a round: dict of buf and deframed (u8, RHP_PAD zero bytes behind the sessions),
    sess_off, slot_off (u64 [n + 1]), states_in, states_out (WALK_STATE_DTYPE [n]) and the expected columns, the
    per-slot ones spread over the slots the sessions own (written: 1 where the session wrote the slot)"""
    g = golden()
    s = SET_NAMES.index(name)
    n = int(g["set_nsess"][s])
    f0, f1 = int(g["set_first"][s]), int(g["set_first"][s + 1])
    states = (g["states_in"][32 * f0: 32 * f1].copy().view(rhp.WALK_STATE_DTYPE) if f1 > f0 else np.zeros(n, dtype=rhp.WALK_STATE_DTYPE))
    assert len(states) == n
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
        nt = int(x["slot_off"][-1])
        where = np.concatenate([int(x["slot_off"][i]) + np.arange(int(x["n_slots"][i])) for i in range(n)] + [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        x["written"] = np.zeros(nt, dtype=np.uint8)
        x["written"][where] = 1
        for k in SLOT_FIELDS + ("ret",) + MSG_FIELDS:
            col = np.zeros(nt, dtype=np.uint64 if k in ("start", "body_len", "wire_len") else np.int64)
            col[where] = g[k][t0: t0 + len(where)]
            x[k] = col
        x["hdrs"] = [np.zeros((0, 4), dtype=np.uint16)] * nt
        for j, i in enumerate(where):
            x["hdrs"][int(i)] = g["hdr"][int(g["hdr_lo"][t0 + j]): int(g["hdr_lo"][t0 + j + 1])]
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
    return int(g["set_maxh"][s]), int(g["set_flags"][s]), rounds


def check(name, r, out, what, deframe):
    """what one round returned (rhp.walk_resume_cpu / _gpu) against round r of the set in the golden file"""
    x = golden_set(name)[2][r]
    results, slots, msgs, hdrs, bytes_out, states = out[:6]
    what = f"{what} {name} round {r}"
    assert len(results) == len(x["len"]) and len(slots) == len(msgs) == len(hdrs) == int(x["slot_off"][-1])
    for f in ("n_slots", "stop", "consumed"):
        bad = np.flatnonzero(results[f] != x[f])
        assert not len(bad), f"{what}: {f} of session {int(bad[0])} is {int(results[f][bad[0]])}, the reference's {int(x[f][bad[0]])} ({len(bad)} differ)"
    w = x["written"] == 1
    for f in SLOT_FIELDS:
        bad = np.flatnonzero(w & (slots[f].astype(x[f].dtype) != x[f]))
        assert not len(bad), f"{what}: {f} of slot {int(bad[0])} is {int(slots[f][bad[0]])}, the reference's {int(x[f][bad[0]])} ({len(bad)} differ)"
    bad = np.flatnonzero(w & (msgs["ret"] != x["ret"]))
    assert not len(bad), f"{what}: ret of slot {int(bad[0])} is {int(msgs['ret'][bad[0]])}, the reference's {int(x['ret'][bad[0]])}"
    ok = w & (x["ret"] > 0)
    for f in MSG_FIELDS:
        bad = np.flatnonzero(ok & (msgs[MSG_COLUMN.get(f, f)] != x[f]))
        assert not len(bad), f"{what}: {f} of slot {int(bad[0])} is {int(msgs[MSG_COLUMN.get(f, f)][bad[0]])}, the reference's {int(x[f][bad[0]])}"
    assert (msgs["reserved"][ok] == 0).all() and (msgs["flags"][ok] == 0).all()
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    cont = w & (x["ret"] == 0) & (x["result"] != 0)   # continuation slots: sixteen zero bytes, no header record written
    if cont.any():
        assert not raw(msgs)[cont].any(), f"{what}: a continuation's message record is not sixteen zero bytes"
        assert (raw(hdrs)[cont] == rhp.WALK_POISON).all(), f"{what}: a continuation wrote a header record"
    for i in np.flatnonzero(ok):
        got = hdrs[i, : int(x["num_headers"][i])]
        want = np.ascontiguousarray(x["hdrs"][i]).view(rhp.HDR_DTYPE).reshape(-1)
        assert (got == want).all(), f"{what}: the header records of slot {int(i)} are {got}, the reference's {want}"
    for a, label in ((slots, "slot"), (msgs, "message record"), (hdrs, "header records")):
        if a.size:
            assert (raw(a)[~w] == rhp.WALK_POISON).all(), f"{what}: a {label} past n_slots was written"
    bad = np.flatnonzero((state_bytes(states) != state_bytes(x["states_out"])).any(axis=1))
    assert not len(bad), (f"{what}: the state of session {int(bad[0])} is {states[bad[0]]}, the reference's "
                          f"{x['states_out'][bad[0]]} (at entry {x['states_in'][bad[0]]}; {len(bad)} differ)")
    want = x["deframed"] if deframe else x["buf"]
    bad = np.flatnonzero(bytes_out != want)
    assert not len(bad), f"{what}: byte {int(bad[0])} is {int(bytes_out[bad[0]])}, not {int(want[bad[0]])} ({len(bad)} differ)"


def set_plan(name):
    return next(s for s in wr.all_sets() if s[0] == name)


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_sets():
    """the file's sets, bytes, offsets, capacities and first states are what tests/walk_resume_sets.py builds, the
    rounds made by the driver from the file's own consumed counts; it is no larger than walk_responses.npz"""
    sets = wr.all_sets()
    assert [s[0] for s in sets] == SET_NAMES
    assert wr.STATE_DTYPE == rhp.WALK_STATE_DTYPE
    for name, maxh, flags, deliveries, caps, states in sets:
        gm, gf, rounds = golden_set(name)
        assert (gm, gf, len(rounds)) == (maxh, flags, len(deliveries)), name
        it = iter(rounds)

        def step(buf, off, sl, st, maxh_, flags_):
            x = next(it)
            assert (buf == x["buf"]).all() and (off == x["sess_off"]).all() and (sl == x["slot_off"]).all(), name
            assert st is None or (state_bytes(st) == state_bytes(x["states_in"])).all(), name
            res = np.zeros(len(off) - 1, dtype=rhp.WALK_RESULT_DTYPE)
            res["consumed"] = x["consumed"]
            return res, None, None, None, None, x["states_out"]

        wr.walk_rounds(step, deliveries, caps, maxh, flags, states)
        assert all(len(b"".join(d[s] for d in deliveries)) <= 450 for s in range(len(deliveries[0]))), "streams stay small"
    assert os.path.getsize(GOLDEN) <= os.path.getsize(OLD_GOLDEN)


def test_golden_covers_what_the_sets_are_for():
    """each situation the sets exist for is in the file"""
    entry, exit_, cont_stop, head_stop, after_cont, cut_state, moved_partial = set(), set(), set(), set(), set(), set(), 0
    for name in SET_NAMES:
        for x in golden_set(name)[2]:
            for s in range(len(x["len"])):
                pin, pout = int(x["states_in"]["phase"][s]), int(x["states_out"]["phase"][s])
                if x["len"][s] or pin >= wr.DEAD:
                    entry.add(min(pin, wr.DEAD))
                if x["kept"][s]:
                    continue
                exit_.add(pout)
                if pout == wr.IN_CHUNKED:
                    cut_state.add(int(x["states_out"]["decoder"]["state"][s]))
                n, stop = int(x["n_slots"][s]), int(x["stop"][s])
                if n:
                    first_cont = pin != wr.AT_HEAD
                    (cont_stop if first_cont and n == 1 else head_stop).add(stop)
                    if first_cont:
                        after_cont.add(stop)
                    last = int(x["slot_off"][s]) + n - 1
                    if stop == rhp.WALK_BODY and x["body_kind"][last] == rhp.FRAME_CHUNKED:
                        a = int(x["start"][last]) + int(x["ret"][last])
                        moved_partial += int((x["buf"][a: a + int(x["wire_len"][last])] != x["deframed"][a: a + int(x["wire_len"][last])]).sum())
    assert entry == set(range(5)) and exit_ == set(range(5)), "every phase at entry and at exit"
    assert cont_stop == {rhp.WALK_END, rhp.WALK_BAD, rhp.WALK_BODY, rhp.WALK_CLOSE, rhp.WALK_MORE}, "every stop a continuation slot can be the last slot of"
    assert head_stop == set(range(6)) and after_cont == set(range(6)), "every stop from a head slot, and in a round that began with a continuation"
    assert cut_state == set(range(6)), "a cut in each of the six decoder states"
    assert moved_partial > 0, "bytes moved by a partial de-frame"
    # the cut plans
    _, _, (r0, r1) = golden_set("cut_everywhere")
    L = len(wr.CUT_STREAM)
    assert r0["len"].tolist() == list(range(1, L)), "a cut at every byte"
    assert (r1["stop"] == rhp.WALK_END).all() and (r1["states_out"]["phase"] == wr.AT_HEAD).all(), "every split ends where the whole stream ends"
    exact = (r0["states_out"]["phase"] == wr.IN_LENGTH) & (r0["states_out"]["left"] == r1["len"])
    assert exact.any() and (r0["states_out"]["left"] == 4).any(), "left == avail exactly; one byte into a body"
    hexes = r0["states_out"]["decoder"]["hex_count"]
    assert (hexes == 1).any(), "a cut between two hex digits"
    _, _, drip = golden_set("drip")
    assert len(drip) == len(wr.DRIP_STREAM) and all(x["len"][0] >= 1 for x in drip) and int(drip[-1]["stop"][0]) == rhp.WALK_END
    assert {int(x["states_out"]["phase"][0]) for x in drip} == {wr.AT_HEAD, wr.IN_LENGTH, wr.IN_CHUNKED}
    assert len(golden_set("drip65")[2][0]["len"]) == 65 and len(golden_set("three_rounds")[2][0]["len"]) == 257
    assert {int(v) % 16 for x in golden_set("three_rounds")[2] for v in x["sess_off"][:-1]} == set(range(16)), "a session start at every residue mod 16"
    assert {int(golden()["set_flags"][SET_NAMES.index(n)]) & 1 for n in SET_NAMES} == {0, 1}, "both values of RHP_WALK_TRAILERS"
    # the stops set, session by session: (stop per round)
    stops = [[int(x["stop"][s]) for x in golden_set("stops")[2]] for s in range(19)]
    E, H, B, Y, C, M = range(6)
    assert stops[:9] == [[Y, Y, Y], [Y, Y, E], [C, C, C], [Y, B, B], [Y, M, E], [M, E, E], [H, E, E], [Y, E, E], [Y, Y, Y]]
    assert stops[9:] == [[Y, B, B], [Y, C, C], [Y, H, E], [Y, E, E], [Y, Y, E], [Y, M, E], [B, B, B], [Y, M, E], [Y, Y, E], [Y, E, E]]
    x1 = golden_set("stops")[2][1]
    assert int(x1["consumed"][4]) == 0 and x1["kept"][4] == 1 and int(x1["n_slots"][4]) == 0, "MORE with no slot keeps the state"
    x0 = golden_set("stops")[2][0]
    assert int(x0["wire_len"][int(x0["slot_off"][7])]) == 0 and int(x0["states_out"]["phase"][7]) == wr.IN_CHUNKED and not state_bytes(x0["states_out"])[7, :8].any() \
        and int(x0["states_out"]["decoder"]["consume_trailer"][7]) == 1, "a head that ends exactly at e arms a zero decoder"
    assert int(x0["states_out"]["left"][8]) == 2 ** 64 - 1 - 3 and int(x1["body_len"][int(x1["slot_off"][8])]) == 2 ** 64 - 4
    c = golden_set("corrupt")[2][0]
    assert c["stop"].tolist() == [E, B, B, B, B, E, B, B, E, B, B, E] and c["kept"].tolist() == [0, 1, 1, 1, 1, 0, 1, 1, 0, 0, 1, 0]
    e = golden_set("empty_rounds")[2][0]
    assert e["stop"].tolist() == [E, E, Y, Y, C, B, E, E] and e["kept"].tolist() == [1, 0, 1, 1, 1, 1, 0, 1]
    sp = golden_set("sp_run_into_moving_body")[2][0]
    assert sp["stop"].tolist() == [H, E, H, E, H] and [int(sp["ret"][int(sp["slot_off"][s]) + int(sp["n_slots"][s]) - 1]) for s in (0, 2, 4)] == [-2] * 3
    b = int(sp["sess_off"][1])
    assert bytes(sp["buf"][b: b + 4]) == b"    " and bytes(sp["deframed"][b: b + 4]) == b"wxyz", "the neighbour's spaces are moved over"


DEFRAMES = [0, ws.DEFRAME]


@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_twin_equals_golden(name, deframe):
    """every round alone, from the file's bytes and states"""
    maxh, flags, rounds = golden_set(name)
    for r, x in enumerate(rounds):
        check(name, r, rhp.walk_resume_cpu(x["buf"], x["sess_off"], x["slot_off"], x["states_in"], maxh, flags | deframe),
              "rhp_cpu_walk_resume", deframe)


@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_chain_equals_golden(name, deframe):
    """the chain through the driver, every round fed from the twin's own answers"""
    _, maxh, flags, deliveries, caps, states = set_plan(name)
    rounds = wr.walk_rounds(lambda *a: rhp.walk_resume_cpu(*a[:5], a[5] | deframe), deliveries, caps, maxh, flags, states)
    for r, (_, _, _, out) in enumerate(rounds):
        check(name, r, out, "rhp_cpu_walk_resume (chained)", deframe)


def messages_of_rounds(rounds, n):
    """per session the messages of its rounds: [[msg record, header records, result, body_kind, head's body_len,
    summed wire_len, summed decoded length, decoded bytes]]; a head slot opens a message, a continuation slot adds
    to the last; slots with result 0 (an incomplete head, parsed again in the next round) are left out"""
    per = [[] for _ in range(n)]
    for _, off, sl, out in rounds:
        results, slots, msgs, hdrs, after = out[:5]
        for s in range(n):
            for k in range(int(sl[s]), int(sl[s]) + int(results["n_slots"][s])):
                x, m = slots[k], msgs[k]
                if x["result"] == 0:
                    continue
                chunked = x["body_kind"] == rhp.FRAME_CHUNKED
                if m["ret"] == 0 and x["result"] == 1:
                    body = int(x["start"])
                    msg = per[s][-1]
                elif m["ret"] == 0:   # a continuation that went bad: the message ends malformed
                    per[s][-1][2] = -1
                    continue
                else:
                    body = int(x["start"]) + max(int(m["ret"]), 0)
                    rec = m.tolist() if m["ret"] > 0 else int(m["ret"])
                    msg = [rec, hdrs[k, : int(m["num_headers"])].tolist() if m["ret"] > 0 else [], int(x["result"]), int(x["body_kind"]),
                           int(x["body_len"]) if not chunked else 0, 0, 0, b""]
                    per[s].append(msg)
                msg[5] += int(x["wire_len"])
                if chunked:
                    msg[6] += int(x["body_len"])
                    msg[7] += bytes(after[body: body + int(x["body_len"])])
    return per


@pytest.mark.parametrize("name", ["cut_everywhere", "three_rounds", "three_rounds_f0", "three_rounds_f5"])
def test_cpu_split_invariance(name):
    """however a stream is cut into rounds, its head slots, each message's summed wire_len and, de-framed, its
    decoded bytes are what rhp_cpu_walk_responses gives over the whole stream"""
    _, maxh, flags, deliveries, caps, _ = set_plan(name)
    n = len(deliveries[0])
    rounds = wr.walk_rounds(lambda *a: rhp.walk_resume_cpu(*a[:5], a[5] | ws.DEFRAME), deliveries, caps, maxh, flags)
    got = messages_of_rounds(rounds, n)
    streams = [b"".join(d[s] for d in deliveries) for s in range(n)]
    buf, off = ws.pack(streams)
    sl = ws.slot_offsets([16] * n)
    whole = rhp.walk_responses_cpu(buf, off, sl, maxh, flags)
    want = messages_of_rounds([(buf, off, sl, whole)], n)
    chunked_bodies = 0
    for s in range(n):
        for msg in want[s]:   # the whole walk de-frames nothing here: the decoded bytes are rhp_cpu_decode_chunked's
            if msg[3] == rhp.FRAME_CHUNKED and msg[2] == 1 and msg[5]:
                k = next(k for k in range(int(sl[s]), int(sl[s + 1])) if whole[2][k].tolist() == msg[0])
                a = int(whole[1]["start"][k]) + int(whole[2]["ret"][k])
                piece = buf[a: a + msg[5]]
                dec = np.zeros(1, dtype=rhp.CHUNKED_DTYPE)
                dec["consume_trailer"] = flags & ws.TRAILERS
                res, _, left = rhp.decode_chunked_cpu(piece, np.array([0, piece.size], dtype=np.uint64), dec)
                assert int(res["size"][0]) == msg[6]
                msg[7] = bytes(left[: msg[6]])
                chunked_bodies += 1
        assert got[s] == want[s], f"{name} session {s}: cut into rounds {got[s]}, whole {want[s]}"
    assert chunked_bodies >= 3


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
@pytest.mark.parametrize("name", ["cut_everywhere", "drip", "three_rounds_f0", "stops", "corrupt", "sp_run_into_moving_body"])
def test_golden_equals_live_reference(name):
    """the maker's rounds over the compiled reference, run now, against the file"""
    from golden import make_golden_decode_chunked as mdc
    from golden.make_golden_messages import reference
    from golden.make_golden_walk_resume import round_walker, state_tuples, state_array
    maxh, flags, rounds = golden_set(name)
    walk = round_walker(reference(), mdc.reference())
    for r, x in enumerate(rounds):
        live, out = x["buf"].copy(), x["buf"].copy()
        sts = state_tuples(x["states_in"])
        after = []
        for s in range(len(sts)):
            lo = int(x["slot_off"][s])
            res, rows, nxt = walk(live, out, int(x["sess_off"][s]), int(x["sess_off"][s + 1]), int(x["cap"][s]), maxh, flags, sts[s])
            assert res == (int(x["n_slots"][s]), int(x["stop"][s]), int(x["consumed"][s])), (name, r, s)
            assert (nxt is None) == bool(x["kept"][s]), (name, r, s)
            after.append(sts[s] if nxt is None else nxt)
            for k, row in enumerate(rows):
                assert row[:5] == tuple(int(x[f][lo + k]) for f in SLOT_FIELDS), (name, r, s, k)
                assert row[5][0] == int(x["ret"][lo + k]), (name, r, s, k)
        assert (state_bytes(state_array(after)) == state_bytes(x["states_out"])).all(), (name, r)
        assert (out == x["deframed"]).all() and (live == x["buf"]).all()


def test_cpu_offsets_that_hold_anything_stay_inside():
    """sess_off and slot_off rows of poison and states of every phase, every buffer between guard bytes: nothing
    outside is written, every stop is a stop code and every phase left is a phase"""
    maxh, flags, rounds = golden_set("three_rounds")
    x = rounds[1]
    buf, sess_off, slot_off = x["buf"], x["sess_off"], x["slot_off"]
    ns, nt = len(sess_off) - 1, int(slot_off[-1])
    rng = np.random.default_rng(7)
    guarded = lambda nbytes: np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8)
    for trial in range(6):
        so, sl = sess_off.copy(), slot_off.copy()
        rows = rng.integers(0, ns + 1, size=12)
        so[rows[:6]] = rng.choice(np.array([0, 1, 2 ** 63, 2 ** 64 - 1, buf.size, buf.size - 1, buf.size + 17, 77], dtype=np.uint64), 6)
        if trial & 1:
            sl[rows[6:]] = rng.choice(np.array([0, nt, nt + 1, 2 ** 32, 2 ** 64 - 1, 3], dtype=np.uint64), 6)
        g = {k: guarded(n) for k, n in (("msgs", 16 * nt), ("hdrs", 8 * nt * maxh), ("slots", 32 * nt), ("results", 16 * ns), ("states", 32 * ns))}
        st = x["states_in"].copy()
        st["phase"][rng.integers(0, ns, size=40)] = rng.integers(0, 5, size=40)
        st["left"][rng.integers(0, ns, size=10)] = rng.choice(np.array([0, 1, 2 ** 64 - 1, 50], dtype=np.uint64), 10)
        g["states"][GUARD:-GUARD] = st.view(np.uint8)
        rw = np.concatenate([np.full(GUARD, 0xA5, dtype=np.uint8), buf, np.full(GUARD, 0xA5, dtype=np.uint8)])
        p = lambda a: a.ctypes.data + GUARD
        w = rhp.WalkBatch(p(rw), p(rw), buf.size, so.ctypes.data, sl.ctypes.data, ns, nt, maxh, flags | ws.DEFRAME,
                          p(g["msgs"]), p(g["hdrs"]), p(g["slots"]), p(g["results"]))
        assert rhp.host().rhp_cpu_walk_resume(ctypes.byref(w), p(g["states"])) == 0
        for k, a in list(g.items()) + [("bytes", rw)]:
            assert (a[:GUARD] == 0xA5).all() and (a[-GUARD:] == 0xA5).all(), f"trial {trial}: the guard bytes of {k} were written"
        res = g["results"][GUARD:-GUARD].view(rhp.WALK_RESULT_DTYPE)
        after = g["states"][GUARD:-GUARD].view(rhp.WALK_STATE_DTYPE)
        assert (res["stop"] <= rhp.WALK_MORE).all() and (res["n_slots"] <= nt).all() and (after["phase"] <= rhp.WALK_DEAD).all()
        assert (after["reserved"] == 0).all()
        for s in range(ns):
            if sl[s] > sl[s + 1] or sl[s + 1] > nt:
                assert res["n_slots"][s] == 0, (trial, s)
            else:
                assert res["n_slots"][s] <= sl[s + 1] - sl[s], (trial, s)


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU): everything
    rhp_walk_responses refuses, a NULL states and, on the device, states that are not 16-byte aligned.  Only refused
    calls and n_sessions == 0 go to the GPU library here"""
    gpu = which == "gpu-library"
    fn = ((lambda w, st: rhp.lib().rhp_walk_resume(w, st, None)) if gpu else (lambda w, st: rhp.host().rhp_cpu_walk_resume(w, st)))
    al = lambda nbytes, fill: (lambda r: r[(-r.ctypes.data) % 16:][:nbytes])(np.full(nbytes + 16, fill, dtype=np.uint8))
    buf = al(512, 0)
    buf[: len(ws.HELLO)] = np.frombuffer(ws.HELLO, dtype=np.uint8)
    so = np.array([0, len(ws.HELLO), len(ws.HELLO)], dtype=np.uint64)
    sl = np.array([0, 2, 4], dtype=np.uint64)
    msgs, hdrs, slots, results, states = al(64, 0x77), al(4 * 4 * 8, 0x77), al(128, 0x77), al(32, 0x77), al(64, 0)
    p = lambda a: a.ctypes.data
    STATES = object()

    def call(states_=STATES, **kw):
        a = dict(bytes=p(buf), bytes_rw=p(buf), bytes_size=512, sess_off=p(so), slot_off=p(sl), n_sessions=2, n_slots_total=4,
                 max_headers=4, flags=0, msgs=p(msgs), hdrs=p(hdrs), slots=p(slots), results=p(results))
        a.update(kw)
        return fn(ctypes.byref(rhp.WalkBatch(*(a[k] for k, _ in rhp.WalkBatch._fields_))), p(states) if states_ is STATES else states_)

    E = -22
    assert fn(None, p(states)) == E and call(states_=None) == E
    for k in ("bytes", "sess_off", "slot_off", "results", "msgs", "slots", "hdrs"):
        assert call(**{k: None}) == E, k
    assert call(max_headers=rhp.RHP_MAX_HEADERS + 1) == E and call(n_slots_total=2 ** 32 - 1, max_headers=2) == E
    assert call(flags=8) == E and call(flags=1 << 31) == E and call(bytes_size=rhp.RHP_PAD - 1) == E
    assert call(flags=ws.DEFRAME, bytes_rw=None) == E and call(flags=ws.DEFRAME, bytes_rw=p(buf) + 16) == E
    assert call(n_sessions=0, flags=8) == E and call(n_sessions=0, max_headers=65) == E, "the rules come before the empty call"
    if gpu:   # the device's alone: the whole-line loads and whole-record accesses
        for k, a in (("bytes", buf), ("msgs", msgs), ("slots", slots), ("results", results)):
            assert call(**{k: p(a) + 8}) == E, k
        assert call(hdrs=p(hdrs) + 4) == E and call(states_=p(states) + 8) == E
    untouched = lambda: all((a == 0x77).all() for a in (msgs, hdrs, slots, results)) and not states.any()
    assert untouched(), "a refused call writes nothing"
    # accepted: no session asks no pointer, states among them, and launches nothing
    assert call(n_sessions=0) == 0 and call(states_=None, n_sessions=0, bytes=None, bytes_rw=None, sess_off=None, slot_off=None,
                                            msgs=None, hdrs=None, slots=None, results=None, bytes_size=0, n_slots_total=0) == 0
    assert untouched()
    if gpu:
        return
    # accepted by the host twin: any alignment, of the states too
    odd, odd_st = np.full(33, 0x77, dtype=np.uint8), np.zeros(65, dtype=np.uint8)
    assert call(states_=p(odd_st) + 1, results=p(odd) + 1, bytes_rw=None) == 0 and odd[0] == 0x77
    assert odd[1:].copy().view(rhp.WALK_RESULT_DTYPE).tolist() == [(1, rhp.WALK_END, len(ws.HELLO)), (0, rhp.WALK_END, 0)]
    assert slots[:32].view(rhp.WALK_SLOT_DTYPE).tolist() == [(0, 12, 12, 1, rhp.FRAME_LENGTH)] and (slots[32:] == 0x77).all()
    assert not odd_st.any()


def test_host_twin_asan_ubsan_clean():
    """`make walk-resume-asan`: a stand-alone program over the host sources (tests/walk_resume_host_test.c) that
    runs the rounds of the golden file with the host twin"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "walk-resume-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "walk_resume_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernel against the golden file and against the twin


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_equals_golden(name, deframe):
    """every round alone: outputs poisoned first, guard bytes beside bytes, msgs, hdrs, slots, results and states;
    the states of dead and corrupt sessions keep their value"""
    maxh, flags, rounds = golden_set(name)
    for r, x in enumerate(rounds):
        check(name, r, rhp.walk_resume_gpu(x["buf"], x["sess_off"], x["slot_off"], x["states_in"], maxh, flags | deframe, guard=GUARD),
              "rhp_walk_resume", deframe)


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", [n for n in SET_NAMES if len(golden_set(n)[2]) > 1])
def test_gpu_chain_equals_golden(name, deframe):
    """the chain through the driver with the states left on the device between rounds"""
    _, maxh, flags, deliveries, caps, states = set_plan(name)
    rounds = wr.walk_rounds(lambda *a: rhp.walk_resume_gpu(*a[:5], a[5] | deframe, guard=GUARD), deliveries, caps, maxh, flags, states)
    for r, (_, _, _, out) in enumerate(rounds):
        check(name, r, out, "rhp_walk_resume (chained)", deframe)


@pytest.mark.gpu
@pytest.mark.parametrize("n", wr.GEOMETRY)
def test_gpu_geometry(n):
    """the first n sessions of three_rounds as a batch of their own: a session's answers do not depend on its
    neighbours, so they are the file's"""
    maxh, flags, rounds = golden_set("three_rounds")
    for r, x in enumerate(rounds):
        e, t = int(x["sess_off"][n]), int(x["slot_off"][n])
        buf = np.concatenate([x["buf"][:e], np.zeros(ws.RHP_PAD, dtype=np.uint8)])
        res, slots, msgs, hdrs, after, states, _ = rhp.walk_resume_gpu(buf, x["sess_off"][: n + 1], x["slot_off"][: n + 1], x["states_in"][:n],
                                                                       maxh, flags | ws.DEFRAME, guard=GUARD)
        for f in ("n_slots", "stop", "consumed"):
            assert (res[f] == x[f][:n]).all(), (n, r, f)
        w = x["written"][:t] == 1
        for f in SLOT_FIELDS:
            assert (slots[f].astype(x[f].dtype)[w] == x[f][:t][w]).all(), (n, r, f)
        assert (msgs["ret"][w] == x["ret"][:t][w]).all() and (after[:e] == x["deframed"][:e]).all()
        assert (state_bytes(states) == state_bytes(x["states_out"][:n])).all(), (n, r)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [ws.TRAILERS, ws.TRAILERS | ws.DEFRAME | ws.NONE_EMPTY, ws.DEFRAME])
def test_gpu_equals_twin_on_a_random_mix(flags):
    deliveries, caps = wr.random_mix(512, 20261020)
    want = wr.walk_rounds(lambda *a: rhp.walk_resume_cpu(*a), deliveries, caps, 8, flags)
    got = wr.walk_rounds(lambda *a: rhp.walk_resume_gpu(*a, guard=GUARD), deliveries, caps, 8, flags)
    stops, phases = set(), set()
    for r, ((wb, wo, wl, w), (gb, go, gl, g)) in enumerate(zip(want, got)):
        assert (wb == gb).all() and (wo == go).all(), f"round {r}: the inputs differ, so a round before did"
        stops |= set(w[0]["stop"].tolist())
        phases |= set(w[5]["phase"].tolist())
        for k, label in ((0, "results"), (1, "slots"), (4, "bytes")):
            assert (g[k] == w[k]).all(), f"round {r}: {label} differ between the kernel and the host twin"
        assert (state_bytes(g[5]) == state_bytes(w[5])).all(), f"round {r}: the states differ between the kernel and the host twin"
        gs, gm, gh, wm, wh = g[1], g[2], g[3], w[2], w[3]
        written = gs["start"] != np.frombuffer(bytes([rhp.WALK_POISON]) * 8, dtype=np.uint64)[0]
        assert (gm["ret"] == wm["ret"]).all()
        ok = written & (wm["ret"] > 0)
        assert (gm[ok] == wm[ok]).all()
        k = np.arange(gh.shape[1])[None, :] < np.where(ok, wm["num_headers"], 0)[:, None]
        assert (gh[k] == wh[k]).all()
    every = set(range(6)) - ({rhp.WALK_CLOSE} if flags & ws.NONE_EMPTY else set())
    assert stops == every and phases >= set(range(5)) - ({wr.IN_CLOSE} if flags & ws.NONE_EMPTY else set()), "the mix holds every stop code and phase"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["kinds_f1", "n65"])
def test_gpu_walk_responses_is_as_it_was(name):
    """rhp_walk_responses, whose statement now shares its loop with rhp_walk_resume, still equals its own file"""
    import test_walk_responses as old
    maxh, flags, buf, _, sess_off, slot_off, _ = old.golden_set(name)
    for deframe in DEFRAMES:
        old.check(name, rhp.walk_responses_gpu(buf, sess_off, slot_off, maxh, flags | deframe, guard=GUARD), "rhp_walk_responses", deframe)
