"""rhp_walk_responses (include/rhp.h): the pipelined responses of a batch of upstream connections walked message
after message -- phr_parse_response, the framing rule of rhp_frame_messages, phr_decode_chunked from a zero
decoder -- one session per lane.

The expected answers are in tests/golden/walk_responses.npz, written by tests/golden/make_golden_walk.py: the walk
stated in plain Python, every parse, lookup, number and chunked decode in it the compiled reference's own, for
every session of every set of tests/walk_sets.py.  Held to them, value for value:
  CPU  the host twin rhp_cpu_walk_responses, with and without RHP_WALK_DEFRAME; the live reference where
       oracle/_ref/libref.so is built; the refusals of rhp_walk_args.h; sess_off and slot_off rows that hold
       anything, between guard bytes; the de-framed bytes against decode_chunked_cpu; a sanitizer build of the
       twin as a stand-alone program
  GPU  the kernel on every set (n_sessions 1, 63, 64, 65, 257 among them; a session start at every residue mod
       16), outputs poisoned first and guard bytes on both sides of every buffer, with and without
       RHP_WALK_DEFRAME; the kernel against the twin on a seeded mix of 512 sessions
Compared: every field of results; every field of the slots a session wrote; of their message records ret always
and the rest where ret > 0; their header records k < num_headers; slots past n_slots keep their poison; the bytes.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import walk_sets as ws

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "walk_responses.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
GUARD = 256
MSG_FIELDS = ("status", "msg_off", "msg_len", "minor", "num_headers")
MSG_COLUMN = {"minor": "minor_version"}


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


SET_NAMES = [str(x) for x in golden()["set_name"]]


@functools.lru_cache(maxsize=None)
def golden_set(name):
    """(max_headers, flags, buf u8, deframed u8, sess_off u64 [n + 1], slot_off u64 [n + 1], expected) of one set;
    expected: the per-session and per-slot arrays of the file, and hdrs: a list of u16 [num_headers, 4] per slot"""
    g = golden()
    s = SET_NAMES.index(name)
    lo, hi = int(g["set_sess"][s]), int(g["set_sess"][s + 1])
    tl, th = int(g["set_slot"][s]), int(g["set_slot"][s + 1])
    bl, bh = int(g["set_byte"][s]), int(g["set_byte"][s + 1])
    exp = {k: g[k][lo:hi].copy() for k in ("n_slots", "stop", "consumed")}
    exp.update({k: g[k][tl:th].copy() for k in ("written", "start", "body_len", "wire_len", "result", "body_kind", "ret") + MSG_FIELDS})
    exp["hdrs"] = [g["hdr"][int(g["hdr_lo"][i]): int(g["hdr_lo"][i + 1])] for i in range(tl, th)]
    arrays = (g["bytes"][bl:bh].copy(), g["deframed"][bl:bh].copy(), g["sess_off"][lo + s: hi + s + 1].copy(),
              g["slot_off"][lo + s: hi + s + 1].copy())
    for a in arrays + tuple(v for v in exp.values() if isinstance(v, np.ndarray)):
        a.setflags(write=False)
    return (int(g["set_maxh"][s]), int(g["set_flags"][s])) + arrays + (exp,)


def check(name, out, what, deframe):
    """what a walk of one set returned (rhp.walk_responses_cpu / _gpu) against the golden file"""
    maxh, _, buf, deframed, sess_off, slot_off, exp = golden_set(name)
    results, slots, msgs, hdrs, bytes_out = out
    assert len(results) == len(sess_off) - 1 and len(slots) == len(msgs) == len(hdrs) == int(slot_off[-1])
    for f in ("n_slots", "stop", "consumed"):
        bad = np.flatnonzero(results[f] != exp[f])
        assert not len(bad), (f"{what} {name}: {f} of session {int(bad[0])} is {int(results[f][bad[0]])}, the reference's "
                              f"{int(exp[f][bad[0]])} ({len(bad)} differ)")
    w = exp["written"] == 1
    for f in ("start", "body_len", "wire_len", "result", "body_kind"):
        bad = np.flatnonzero(w & (slots[f] != exp[f]))
        assert not len(bad), (f"{what} {name}: {f} of slot {int(bad[0])} is {int(slots[f][bad[0]])}, the reference's "
                              f"{int(exp[f][bad[0]])} ({len(bad)} differ)")
    bad = np.flatnonzero(w & (msgs["ret"] != exp["ret"]))
    assert not len(bad), f"{what} {name}: ret of slot {int(bad[0])} is {int(msgs['ret'][bad[0]])}, the reference's {int(exp['ret'][bad[0]])}"
    ok = w & (exp["ret"] > 0)
    for f in MSG_FIELDS:
        bad = np.flatnonzero(ok & (msgs[MSG_COLUMN.get(f, f)] != exp[f]))
        assert not len(bad), f"{what} {name}: {f} of slot {int(bad[0])} is {int(msgs[MSG_COLUMN.get(f, f)][bad[0]])}, the reference's {int(exp[f][bad[0]])}"
    assert (msgs["reserved"][ok] == 0).all() and (msgs["flags"][ok] == 0).all()
    for i in np.flatnonzero(ok):
        got = hdrs[i, : int(exp["num_headers"][i])]
        want = np.ascontiguousarray(exp["hdrs"][i]).view(rhp.HDR_DTYPE).reshape(-1)
        assert (got == want).all(), f"{what} {name}: the header records of slot {int(i)} are {got}, the reference's {want}"
    raw = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1)
    for a, label in ((slots, "slot"), (msgs, "message record"), (hdrs, "header records")):
        if a.size:
            assert (raw(a)[~w] == rhp.WALK_POISON).all(), f"{what} {name}: a {label} past n_slots was written"
    want = deframed if deframe else buf
    bad = np.flatnonzero(bytes_out != want)
    assert not len(bad), f"{what} {name}: byte {int(bad[0])} is {int(bytes_out[bad[0]])}, not {int(want[bad[0]])} ({len(bad)} differ)"


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_sets():
    """the golden file's bytes, offsets, capacities and flags are what tests/walk_sets.py builds"""
    sets = ws.all_sets()
    assert [s[0] for s in sets] == SET_NAMES
    for name, maxh, flags, sessions, nslots in sets:
        gm, gf, buf, _, sess_off, slot_off, _ = golden_set(name)
        b, o = ws.pack(sessions)
        assert (gm, gf) == (maxh, flags) and (o == sess_off).all() and (ws.slot_offsets(nslots) == slot_off).all(), name
        assert (buf[: b.size] == b).all() and not buf[b.size:].any(), name
        assert all(len(s) - s.rfind(b"\r\n\r\n") <= 220 for s in sessions if b"\r\n\r\n" in s), "bodies stay small"


def test_golden_covers_what_the_sets_are_for():
    """the answers that the sets exist to produce are in the file"""
    M = 2 ** 64 - 1
    e = lambda name: golden_set(name)[6]

    def session(name, s):
        """(n_slots, stop, [(result, body_kind, body_len, wire_len) per written slot]) of session s"""
        x, lo = e(name), int(golden_set(name)[5][s])
        n = int(x["n_slots"][s])
        return n, int(x["stop"][s]), [tuple(int(x[f][lo + k]) for f in ("result", "body_kind", "body_len", "wire_len")) for k in range(n)]

    L, C, N = rhp.FRAME_LENGTH, rhp.FRAME_CHUNKED, rhp.FRAME_NONE
    assert [int(v) for v in e("stops")["stop"]] == [rhp.WALK_END, rhp.WALK_HEAD, rhp.WALK_END, rhp.WALK_BAD, rhp.WALK_BODY,
                                                   rhp.WALK_CLOSE, rhp.WALK_MORE, rhp.WALK_MORE, rhp.WALK_END]
    assert [int(v) for v in e("stops")["n_slots"]] == [3, 2, 0, 2, 2, 2, 2, 0, 2]
    assert session("stops", 4)[2][1] == (1, L, 10, 9) and session("stops", 5)[2][1] == (1, N, 0, 16)
    assert int(e("stops")["consumed"][4]) == len(ws.SHORT) and int(e("stops")["consumed"][0]) == len(ws.HELLO + ws.CHUNKS_T + ws.SHORT)
    # the kinds in one session, under both values of both flags
    for flags in (1, 5):
        n, stop, rows = session(f"kinds_f{flags}", 0)
        assert (n, stop) == (6, rhp.WALK_END) and [r[1] for r in rows] == [L, C, N, C, N, L] and rows[1][2] == 52 and rows[3][2] == 45
        assert session(f"kinds_f{flags}", 1) == (3, rhp.WALK_END, [(1, N, 0, 0), rows[3], rows[0]])
    assert session("kinds_f0", 0)[:2] == (3, rhp.WALK_BAD), "without RHP_WALK_TRAILERS the trailer lines are the next head"
    assert session("kinds_f1", 3)[:2] == (2, rhp.WALK_CLOSE) and session("kinds_f5", 3)[:2] == (3, rhp.WALK_END)
    assert session("kinds_f1", 5) == (2, rhp.WALK_BODY, [(1, L, 7, 7), (1, L, 10, 9)])
    assert session("kinds_f1", 8)[1] == rhp.WALK_BODY and session("kinds_f1", 8)[2][0][1] == C
    # framing
    f = lambda s: session("framing", s)
    assert f(0) == (2, rhp.WALK_END, [(1, L, 0, 0), (1, L, 12, 12)]), "304 with a Content-Length has no body"
    assert f(1)[2][0] == (1, C, 0, 0) and f(2)[2][0] == (1, L, 0, 0) and f(3)[1] == rhp.WALK_BAD and f(4)[:2] == (2, rhp.WALK_END)
    for s in (5, 6, 7, 8, 15):
        assert f(s)[1] == rhp.WALK_BAD and f(s)[2][-1] == (-1, N, 0, 0), s
    assert f(9)[:2] == (2, rhp.WALK_END), "16 hex digits are a size"
    assert f(10) == (2, rhp.WALK_BODY, [(1, L, 0, 0), (1, L, M, 3)]), "Content-Length: -1 negates: a BODY stop"
    assert f(11) == (1, rhp.WALK_BODY, [(1, L, M, 3)]) and f(12) == (1, rhp.WALK_CLOSE, [(1, N, 0, 3)])
    assert f(13)[:2] == (2, rhp.WALK_END) and f(14)[2][0] == (1, C, 1, 11) and f(16)[:2] == (2, rhp.WALK_END)
    assert (e("split")["stop"] == rhp.WALK_HEAD).all() and (e("split")["n_slots"] == 2).all()
    assert [session("heads", s)[1] for s in range(9)] == [0, 0, rhp.WALK_CLOSE, 0, 0, rhp.WALK_BAD, rhp.WALK_BAD, rhp.WALK_BAD, rhp.WALK_BAD]
    assert session("heads", 1)[2][0] == (1, L, 5, 5) and int(e("heads")["num_headers"][4]) == 4, "obs-fold lines are records"
    for name in ("max0", "max2"):
        assert [session(name, s)[:2] for s in range(3)] == [(3, rhp.WALK_BAD), (3, rhp.WALK_END), (1, rhp.WALK_CLOSE)], name
    assert [int(v) for v in e("sp_run")["stop"]] == [1, 2, 1, 2, 1, 0, 1, 1], "the SP run reads the next session's bytes, then the pad"
    assert sorted(int(v) % 16 for v in golden_set("residues")[4][:16]) == list(range(16)), "a session start at every residue mod 16"
    for n in ws.GEOMETRY:
        assert len(e(f"n{n}")["stop"]) == n
    assert set(e("n257")["stop"].tolist()) | set(e("n64")["stop"].tolist()) == set(range(6)), "every stop code"


DEFRAMES = [0, ws.DEFRAME]


@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_twin_equals_golden(name, deframe):
    maxh, flags, buf, _, sess_off, slot_off, _ = golden_set(name)
    check(name, rhp.walk_responses_cpu(buf, sess_off, slot_off, maxh, flags | deframe), "rhp_cpu_walk_responses", deframe)


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
@pytest.mark.parametrize("name", ["stops", "kinds_f0", "kinds_f5", "framing", "sp_run", "n65"])
def test_golden_equals_live_reference(name):
    """the maker's walk over the compiled reference, run now, against the file"""
    from golden import make_golden_decode_chunked as mdc
    from golden.make_golden_messages import reference
    from golden.make_golden_walk import walker
    maxh, flags, buf, deframed, sess_off, slot_off, exp = golden_set(name)
    walk = walker(reference(), mdc.reference())
    live, out = buf.copy(), buf.copy()
    for s in range(len(sess_off) - 1):
        lo, cap = int(slot_off[s]), int(slot_off[s + 1] - slot_off[s])
        res, rows = walk(live, out, int(sess_off[s]), int(sess_off[s + 1]), cap, maxh, flags)
        assert res == (int(exp["n_slots"][s]), int(exp["stop"][s]), int(exp["consumed"][s])), (name, s)
        for k, r in enumerate(rows):
            assert r[:5] == tuple(int(exp[f][lo + k]) for f in ("start", "body_len", "wire_len", "result", "body_kind")), (name, s, k)
            assert r[5][0] == int(exp["ret"][lo + k]), (name, s, k)
    assert (out == deframed).all() and (live == buf).all()


@pytest.mark.parametrize("name", ["kinds_f1", "kinds_f0", "residues", "n65"])
def test_cpu_deframed_bytes_equal_decode_chunked_cpu(name):
    """with RHP_WALK_DEFRAME the wire span of every completed chunked body is what rhp_cpu_decode_chunked leaves of
    that piece, and no other byte differs"""
    maxh, flags, buf, _, sess_off, slot_off, exp = golden_set(name)
    results, slots, msgs, _, after = rhp.walk_responses_cpu(buf, sess_off, slot_off, maxh, flags | ws.DEFRAME)
    want, spans = buf.copy(), 0
    for s in range(len(results)):
        lo, n, stop = int(slot_off[s]), int(results["n_slots"][s]), int(results["stop"][s])
        for k in range(lo, lo + n):
            done = k < lo + n - 1 or stop in (rhp.WALK_END, rhp.WALK_MORE)
            if slots["body_kind"][k] == rhp.FRAME_CHUNKED and slots["result"][k] == 1 and done and slots["wire_len"][k]:
                a = int(slots["start"][k]) + int(msgs["ret"][k])
                piece = buf[a: a + int(slots["wire_len"][k])]
                dec = np.zeros(1, dtype=rhp.CHUNKED_DTYPE)
                dec["consume_trailer"] = flags & ws.TRAILERS
                res, _, left = rhp.decode_chunked_cpu(piece, np.array([0, piece.size], dtype=np.uint64), dec)
                assert (int(res["ret"][0]), int(res["size"][0])) == (0, int(slots["body_len"][k])), (name, s, k)
                want[a: a + piece.size] = left
                spans += 1
    assert spans >= 3 and (after == want).all(), name


def test_cpu_offsets_that_hold_anything_stay_inside():
    """sess_off and slot_off rows of poison, every buffer between guard bytes: nothing outside is written, every
    stop is a stop code, and a session whose slot range is not ordered or reaches past n_slots_total owns no slot"""
    maxh, flags, buf, _, sess_off, slot_off, _ = golden_set("n65")
    ns, nt = len(sess_off) - 1, int(slot_off[-1])
    rng = np.random.default_rng(7)
    guarded = lambda nbytes: np.full(nbytes + 2 * GUARD, 0xA5, dtype=np.uint8)
    for trial in range(6):
        so, sl = sess_off.copy(), slot_off.copy()
        rows = rng.integers(0, ns + 1, size=12)
        so[rows[:6]] = rng.choice(np.array([0, 1, 2 ** 63, 2 ** 64 - 1, buf.size, buf.size - 1, buf.size + 17, 77], dtype=np.uint64), 6)
        if trial & 1:
            sl[rows[6:]] = rng.choice(np.array([0, nt, nt + 1, 2 ** 32, 2 ** 64 - 1, 3], dtype=np.uint64), 6)
        g = {k: guarded(n) for k, n in (("msgs", 16 * nt), ("hdrs", 8 * nt * maxh), ("slots", 32 * nt), ("results", 16 * ns))}
        rw = np.concatenate([np.full(GUARD, 0xA5, dtype=np.uint8), buf, np.full(GUARD, 0xA5, dtype=np.uint8)])
        p = lambda a: a.ctypes.data + GUARD
        w = rhp.WalkBatch(p(rw), p(rw), buf.size, so.ctypes.data, sl.ctypes.data, ns, nt, maxh, flags | ws.DEFRAME,
                          p(g["msgs"]), p(g["hdrs"]), p(g["slots"]), p(g["results"]))
        assert rhp.host().rhp_cpu_walk_responses(ctypes.byref(w)) == 0
        for k, a in list(g.items()) + [("bytes", rw)]:
            assert (a[:GUARD] == 0xA5).all() and (a[-GUARD:] == 0xA5).all(), f"trial {trial}: the guard bytes of {k} were written"
        res = g["results"][GUARD:-GUARD].view(rhp.WALK_RESULT_DTYPE)
        assert (res["stop"] <= rhp.WALK_MORE).all() and (res["n_slots"] <= nt).all()
        for s in range(ns):
            if sl[s] > sl[s + 1] or sl[s + 1] > nt:
                assert res["n_slots"][s] == 0 and res["stop"][s] in (rhp.WALK_END, rhp.WALK_MORE), (trial, s)
            else:
                assert res["n_slots"][s] <= sl[s + 1] - sl[s], (trial, s)


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls and
    n_sessions == 0 go to the GPU library here: any other accepted one would launch a kernel over host memory"""
    gpu = which == "gpu-library"
    fn = ((lambda w: rhp.lib().rhp_walk_responses(w, None)) if gpu else (lambda w: rhp.host().rhp_cpu_walk_responses(w)))
    al = lambda nbytes, fill: (lambda r: r[(-r.ctypes.data) % 16:][:nbytes])(np.full(nbytes + 16, fill, dtype=np.uint8))
    buf = al(512, 0)
    buf[: len(ws.HELLO)] = np.frombuffer(ws.HELLO, dtype=np.uint8)
    so = np.array([0, len(ws.HELLO), len(ws.HELLO)], dtype=np.uint64)
    sl = np.array([0, 2, 4], dtype=np.uint64)
    msgs, hdrs, slots, results = al(64, 0x77), al(4 * 4 * 8, 0x77), al(128, 0x77), al(32, 0x77)
    p = lambda a: a.ctypes.data

    def call(**kw):
        a = dict(bytes=p(buf), bytes_rw=p(buf), bytes_size=512, sess_off=p(so), slot_off=p(sl), n_sessions=2, n_slots_total=4,
                 max_headers=4, flags=0, msgs=p(msgs), hdrs=p(hdrs), slots=p(slots), results=p(results))
        a.update(kw)
        return fn(ctypes.byref(rhp.WalkBatch(*(a[k] for k, _ in rhp.WalkBatch._fields_))))

    E = -22
    assert fn(None) == E
    for k in ("bytes", "sess_off", "slot_off", "results", "msgs", "slots", "hdrs"):
        assert call(**{k: None}) == E, k
    assert call(max_headers=rhp.RHP_MAX_HEADERS + 1) == E and call(n_slots_total=2 ** 32 - 1, max_headers=2) == E
    assert call(flags=8) == E and call(flags=1 << 31) == E and call(bytes_size=rhp.RHP_PAD - 1) == E
    assert call(flags=ws.DEFRAME, bytes_rw=None) == E and call(flags=ws.DEFRAME, bytes_rw=p(buf) + 16) == E
    assert call(n_sessions=0, flags=8) == E and call(n_sessions=0, max_headers=65) == E, "the rules come before the empty call"
    if gpu:   # the device's alone: the whole-line loads and whole-record stores
        for k, a in (("bytes", buf), ("msgs", msgs), ("slots", slots), ("results", results)):
            assert call(**{k: p(a) + 8}) == E, k
        assert call(hdrs=p(hdrs) + 4) == E
    untouched = lambda: all((a == 0x77).all() for a in (msgs, hdrs, slots, results))
    assert untouched(), "a refused call writes nothing"
    # accepted: no session asks no pointer and launches nothing
    assert call(n_sessions=0) == 0 and call(n_sessions=0, bytes=None, bytes_rw=None, sess_off=None, slot_off=None, msgs=None,
                                            hdrs=None, slots=None, results=None, bytes_size=0, n_slots_total=0) == 0
    assert untouched()
    if gpu:
        return
    # accepted by the host twin: any alignment; no records at all when no session owns a slot; no bytes_rw
    odd = np.full(33, 0x77, dtype=np.uint8)
    assert call(results=p(odd) + 1, bytes_rw=None) == 0 and odd[0] == 0x77
    assert odd[1:].copy().view(rhp.WALK_RESULT_DTYPE).tolist() == [(1, rhp.WALK_END, len(ws.HELLO)), (0, rhp.WALK_END, 0)]
    assert slots[:32].view(rhp.WALK_SLOT_DTYPE).tolist() == [(0, 12, 12, 1, rhp.FRAME_LENGTH)] and (slots[32:] == 0x77).all()
    zero = np.zeros(3, dtype=np.uint64)
    assert call(slot_off=p(zero), n_slots_total=0, msgs=None, hdrs=None, slots=None) == 0
    assert results.view(rhp.WALK_RESULT_DTYPE).tolist() == [(0, rhp.WALK_MORE, 0), (0, rhp.WALK_END, 0)]


def test_host_twin_asan_ubsan_clean():
    """`make walk-responses-asan`: a stand-alone program over the host sources (tests/walk_responses_host_test.c)
    that walks the golden file's sets with the host twin"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "walk-responses-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "walk_responses_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernel against the golden file and against the twin


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_equals_golden(name, deframe):
    """outputs poisoned first, guard bytes beside bytes, msgs, hdrs, slots and results; without RHP_WALK_DEFRAME
    the bytes are unchanged bit for bit, with it only the wire spans of completed chunked bodies differ"""
    maxh, flags, buf, _, sess_off, slot_off, _ = golden_set(name)
    check(name, rhp.walk_responses_gpu(buf, sess_off, slot_off, maxh, flags | deframe, guard=GUARD), "rhp_walk_responses", deframe)


def random_mix(n, seed):
    """n sessions drawn from walk_sets' pool and the residue sessions, with slot counts of their own"""
    rng = np.random.default_rng(seed)
    p = ws.pool() + list(zip(*ws._residues()))
    pick = rng.integers(0, len(p), size=n)
    sessions = [p[i][0] for i in pick]
    nslots = [int(rng.integers(0, 7)) for _ in pick]
    buf, off = ws.pack(sessions)
    return buf, off, ws.slot_offsets(nslots)


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [ws.TRAILERS, ws.TRAILERS | ws.DEFRAME | ws.NONE_EMPTY, ws.DEFRAME])
def test_gpu_equals_twin_on_a_random_mix(flags):
    buf, off, sl = random_mix(512, 20261020)
    want = rhp.walk_responses_cpu(buf, off, sl, 8, flags)
    got = rhp.walk_responses_gpu(buf, off, sl, 8, flags, guard=GUARD)
    every = set(range(6)) - ({rhp.WALK_CLOSE} if flags & ws.NONE_EMPTY else set())   # (no CLOSE with RHP_WALK_NONE_EMPTY)
    assert set(want[0]["stop"].tolist()) == every, "the mix holds every stop code"
    for a, b, label in zip(got, want, ("results", "slots", "msgs", "hdrs", "bytes")):
        if label in ("msgs", "hdrs"):   # unspecified where ret <= 0 / k >= num_headers: compared through the slots' view
            continue
        assert (a == b).all(), f"{label} differ between the kernel and the host twin"
    (_, gs, gm, gh, _), (_, _, wm, wh, _) = got, want
    written = gs["start"] != np.frombuffer(bytes([rhp.WALK_POISON]) * 8, dtype=np.uint64)[0]
    assert (gm["ret"] == wm["ret"]).all()
    ok = written & (wm["ret"] > 0)
    assert (gm[ok] == wm[ok]).all()
    k = np.arange(gh.shape[1])[None, :] < np.where(ok, wm["num_headers"], 0)[:, None]
    assert (gh[k] == wh[k]).all()
