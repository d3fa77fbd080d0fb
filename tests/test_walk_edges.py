"""rhp_walk_responses and rhp_walk_resume (include/rhp.h) at the readable end: calls whose bytes_size puts
rhp_walk_readable(bytes_size) -- lim -- at every byte of a session's last message, from 8 bytes before it to 8 bytes
behind it, at every start residue mod 16, with walkable text lying from lim on; and sess_off, slot_off and
n_slots_total values that hold anything.

By rhp.h a call with a short bytes_size is the plain walk over the clamped view: the same bytes with zeros from lim
on, offsets min(off, lim).  The expected answers are in tests/golden/walk_edges.npz, written by
tests/golden/make_golden_walk_edges.py: the plain-Python walks of make_golden_walk.py and make_golden_walk_resume.py
over the compiled reference, run over that view, for every case of tests/walk_edge_sets.py.  Held to them, value
for value, with and without RHP_WALK_DEFRAME:
  CPU  the host twins with bytes_size=; the live reference where oracle/_ref/libref.so is built
  GPU  the kernels with bytes_size=, the device buffer the whole buffer (the planted text behind bytes_size is
       there), outputs poisoned first, guard bytes beside bytes, msgs, hdrs, slots, results and states
Compared as tests/test_walk_responses.py and tests/test_walk_resume.py compare: every field of results; every field
of the written slots; of their message records ret always and the rest where ret > 0; header records k < num_headers;
unwritten slots keep their poison; the states byte for byte; bytes below lim are the expected bytes, bytes from lim
on the input's.

One-shot, c < 0 cuts the body of the HELLO before the last message, so RHP_WALK_BODY occurs for the `head` and `sp`
kinds too, and test_golden_covers_the_edge asserts END, HEAD and BODY for them.  A header record exists
only for a head that parsed, whose closing CRLF CRLF lie below the clamped end, so the value nearest to lim ends at
lim - 5 with those four bytes up to lim - 1: that is the case the fixture is held to contain.

Offsets that hold anything (GPU): single sess_off rows at 2^64 - 1, 2^63, bytes_size, bytes_size - 1, lim, lim + 1
and lim - 1 without RHP_WALK_DEFRAME (the kernel only reads, so sessions that overlap do not race); slot_off rows
that leave both neighbours without slots; a stale n_slots_total; with RHP_WALK_DEFRAME the last three sess_off rows
at a value from lim on.  A slot_off value that makes two sessions share slots, and a sess_off row that makes
sessions overlap under RHP_WALK_DEFRAME, are races by construction and are not run.  The expected answers of the
sessions a stray sess_off changes are the reference walk over the clamped view, stored in the file; those of the
sessions left without slots are what rhp.h's rules give; every other session is the clean run's in the two older
golden files.  The host twins are held to the same answers on the CPU.

That the reader sees zeros from lim on, not from bytes_size on, cannot show in the twins' answers (with e clamped
the one read past e is the SP run, and a run that reaches e gives -2 whatever lies beyond): the device tests hold
it through the planted text, and the stand-alone sanitizer programs by giving the twin a block of lim + 16 bytes.
"""
from __future__ import annotations

import functools
import os
import time

import numpy as np
import pytest

import libreactorng_amd as rhp
import walk_edge_sets as we
import walk_resume_sets as wr
import walk_sets as ws

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "walk_edges.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
GUARD = 256
SLOT_FIELDS = ("start", "body_len", "wire_len", "result", "body_kind")
MSG_FIELDS = ("status", "msg_off", "msg_len", "minor", "num_headers")
MSG_COLUMN = {"minor": "minor_version"}
NSESS = len(we.SLOTS)
E, H, Y, B, C, M = range(6)   # enum rhp_walk_stop: END, HEAD, BAD, BODY, CLOSE, MORE


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    nh = np.where(g["ret"] > 0, g["num_headers"], 0).astype(np.int64)
    g["hdr_lo"] = np.concatenate([[0], np.cumsum(nh)])
    assert g["hdr_lo"][-1] == len(g["hdr"])
    return g


KINDS = [str(k) for k in golden()["kind_name"]]
CALL_KINDS = [(call, kind) for call in (we.RESPONSES, we.RESUME) for kind in we.KINDS_OF[call]]
IDS = [f"{we.CALL_NAMES[call]}-{kind}" for call, kind in CALL_KINDS]


@functools.lru_cache(maxsize=None)
def golden_buffer(b):
    """(kind, pad, bytes u8, sess_off u64 [5]) of buffer b, put together from the file alone"""
    g = golden()
    piece = g["mid"][int(g["buf_byte"][b]): int(g["buf_byte"][b + 1])]
    buf = np.concatenate([g["lead"], piece, g["tail"], np.zeros(ws.RHP_PAD, dtype=np.uint8)])
    a = len(g["lead"]) + int(g["buf_a"][b])
    e = len(g["lead"]) + len(piece)
    off = np.array([a, a, e, e + int(g["tail_sess"][0]), e + int(g["tail_sess"][0]) + int(g["tail_sess"][1])], dtype=np.uint64)
    buf.setflags(write=False)
    off.setflags(write=False)
    return KINDS[int(g["buf_kind"][b])], int(g["buf_pad"][b]), buf, off


@functools.lru_cache(maxsize=None)
def golden_case(i):
    """case i of the file: dict of call, kind, pad, c, lim, size, buf, deframed, sess_off, slot_off, states_in,
    states_out, the per-session columns and the per-slot ones spread over the slots the sessions own"""
    g = golden()
    kind, pad, buf, off = golden_buffer(int(g["case_buf"][i]))
    x = dict(call=int(g["call"][i]), kind=kind, pad=pad, c=int(g["c"][i]), lim=int(g["lim"][i]), size=int(g["size"][i]),
             buf=buf, sess_off=off, slot_off=g["slot_off"])
    q = slice(NSESS * i, NSESS * (i + 1))
    for k in ("n_slots", "stop", "consumed", "kept", "st_phase", "st_ct", "st_hex", "st_state", "st_left"):
        x[k] = g[k][q]
    d = slice(int(g["case_defr"][i]), int(g["case_defr"][i + 1]))
    x["deframed"] = buf.copy()
    x["deframed"][g["defr_idx"][d]] = g["defr_val"][d]
    nt, t0 = int(g["slot_off"][-1]), int(g["case_slot"][i])
    where = np.concatenate([int(g["slot_off"][s]) + np.arange(int(x["n_slots"][s])) for s in range(NSESS)]).astype(np.int64)
    assert t0 + len(where) == int(g["case_slot"][i + 1])
    x["written"] = np.zeros(nt, dtype=bool)
    x["written"][where] = True
    for k in SLOT_FIELDS + ("ret",) + MSG_FIELDS:
        col = np.zeros(nt, dtype=np.uint64 if k in ("start", "body_len", "wire_len") else np.int64)
        col[where] = g[k][t0: t0 + len(where)]
        x[k] = col
    x["hdrs"] = [np.zeros((0, 4), dtype=np.uint16)] * nt
    for j, s in enumerate(where):
        x["hdrs"][int(s)] = g["hdr"][int(g["hdr_lo"][t0 + j]): int(g["hdr_lo"][t0 + j + 1])]
    st = np.zeros(NSESS, dtype=rhp.WALK_STATE_DTYPE)
    if x["call"] == we.RESUME:
        st[1:2].view(np.uint8)[:] = g["kind_state"][32 * KINDS.index(kind): 32 * KINDS.index(kind) + 32]
    out = np.zeros(NSESS, dtype=rhp.WALK_STATE_DTYPE)
    out["phase"] = x["st_phase"]
    out["left"] = np.where(x["st_phase"] == wr.IN_LENGTH, x["st_left"], 0)
    out["decoder"]["bytes_left_in_chunk"] = np.where(x["st_phase"] == wr.IN_CHUNKED, x["st_left"], 0)
    for col, f in (("st_ct", "consume_trailer"), ("st_hex", "hex_count"), ("st_state", "state")):
        out["decoder"][f] = x[col]
    kept = x["kept"] == 1
    out[kept] = st[kept]
    x["states_in"], x["states_out"] = st, out
    return x


def cases_of(call, kind):
    g = golden()
    return [i for i in range(len(g["call"])) if g["call"][i] == call and g["buf_kind"][g["case_buf"][i]] == KINDS.index(kind)]


def state_bytes(states):
    return np.ascontiguousarray(states).view(np.uint8).reshape(len(states), 32)


def check(i, out, what, deframe):
    """what one call returned (rhp.walk_responses_* / rhp.walk_resume_*) against case i of the golden file"""
    x = golden_case(i)
    results, slots, msgs, hdrs, bytes_out = out[:5]
    what = f"{what} {x['kind']} pad {x['pad']} c {x['c']} (lim {x['lim']}, bytes_size {x['size']}, deframe {deframe})"
    assert len(results) == NSESS and len(slots) == len(msgs) == len(hdrs) == int(x["slot_off"][-1])
    for f in ("n_slots", "stop", "consumed"):
        bad = np.flatnonzero(results[f] != x[f])
        assert not len(bad), f"{what}: {f} of session {int(bad[0])} is {int(results[f][bad[0]])}, the reference's {int(x[f][bad[0]])}"
    w = x["written"]
    for f in SLOT_FIELDS:
        bad = np.flatnonzero(w & (slots[f].astype(x[f].dtype) != x[f]))
        assert not len(bad), f"{what}: {f} of slot {int(bad[0])} is {int(slots[f][bad[0]])}, the reference's {int(x[f][bad[0]])}"
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
    for k in np.flatnonzero(ok):
        got = hdrs[k, : int(x["num_headers"][k])]
        want = np.ascontiguousarray(x["hdrs"][k]).view(rhp.HDR_DTYPE).reshape(-1)
        assert (got == want).all(), f"{what}: the header records of slot {int(k)} are {got}, the reference's {want}"
    for a, label in ((slots, "slot"), (msgs, "message record"), (hdrs, "header records")):
        assert (raw(a)[~w] == rhp.WALK_POISON).all(), f"{what}: a {label} past n_slots was written"
    if x["call"] == we.RESUME:
        bad = np.flatnonzero((state_bytes(out[5]) != state_bytes(x["states_out"])).any(axis=1))
        assert not len(bad), f"{what}: the state of session {int(bad[0])} is {out[5][bad[0]]}, the reference's {x['states_out'][bad[0]]}"
    want = x["deframed"] if deframe else x["buf"]
    lim = x["lim"]
    bad = np.flatnonzero(bytes_out[:lim] != want[:lim])
    assert not len(bad), f"{what}: byte {int(bad[0])} is {int(bytes_out[bad[0]])}, not {int(want[bad[0]])} ({len(bad)} differ)"
    bad = np.flatnonzero(bytes_out[lim:] != x["buf"][lim:])
    assert not len(bad), f"{what}: byte {lim + int(bad[0])}, at or behind the readable end, was written"


def run(i, deframe, gpu):
    x = golden_case(i)
    kw = dict(max_headers=int(golden()["max_headers"][0]), flags=int(golden()["flags"][0]) | deframe, bytes_size=x["size"])
    if gpu:
        kw["guard"] = GUARD
    if x["call"] == we.RESPONSES:
        return (rhp.walk_responses_gpu if gpu else rhp.walk_responses_cpu)(x["buf"], x["sess_off"], x["slot_off"], **kw)
    return (rhp.walk_resume_gpu if gpu else rhp.walk_resume_cpu)(x["buf"], x["sess_off"], x["slot_off"], x["states_in"], **kw)


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_cases():
    """the file's bytes, offsets, sizes, flags and states are what tests/walk_edge_sets.py builds; it stays below
    the largest walk fixture; what the de-framing moves lies inside the session under test, below lim"""
    g = golden()
    assert KINDS == list(we.KINDS) and (int(g["max_headers"][0]), int(g["flags"][0])) == (we.MAXH, we.FLAGS)
    assert (g["slot_off"] == we.slot_off()).all()
    cases = we.all_cases()
    assert len(cases) == len(g["call"])
    for i, (call, kind, pad, c, lim, size) in enumerate(cases):
        x = golden_case(i)
        buf, off = we.buffer(kind, pad)
        assert (x["call"], x["kind"], x["pad"], x["c"], x["lim"], x["size"]) == (call, kind, pad, c, lim, size), i
        assert x["buf"].size == buf.size and (x["buf"] == buf).all() and (x["sess_off"] == off).all(), i
        assert lim == (size & ~15) - 16 and size >= ws.RHP_PAD and size <= buf.size - ws.RHP_PAD, i
        want = we.state_in(kind) if call == we.RESUME else wr.state()
        assert state_bytes(x["states_in"])[1].tobytes() == want.tobytes() and not state_bytes(x["states_in"])[[0, 2, 3]].any(), i
        d = np.flatnonzero(x["deframed"] != buf)
        assert not len(d) or (int(off[1]) <= d[0] and d[-1] < min(int(off[2]), lim)), i
        assert bytes(buf[lim: lim + 4]) != bytes(4) and int(off[1]) >= ws.RHP_PAD, "text lies at the readable end"
    assert os.path.getsize(GOLDEN) < 357137


def test_golden_covers_the_edge():
    """conditions on the fixture, checked from the file alone"""
    g = golden()
    stops, residues = {}, {}
    deframed_last_line = partial_to_lim = value_to_lim = 0
    partial = {"chunked": 0, "in_chunked": 0}
    for call, kind in CALL_KINDS:
        ids = cases_of(call, kind)
        xs = [golden_case(i) for i in ids]
        span = we.parts(kind, 0)[3]
        assert sorted(x["c"] for x in xs) == list(range(-8, span + 9)), f"every c of {kind}"
        assert {x["size"] % 16 for x in xs} == set(range(16)), kind
        stops[call, kind] = {int(x["stop"][1]) for x in xs}
        for x in xs:
            assert x["lim"] % 16 == 0 and x["size"] - x["lim"] - 16 in range(16)
            lo, n = int(x["slot_off"][1]), int(x["n_slots"][1])
            if not n:
                continue
            last = lo + n - 1
            body = int(x["start"][last]) + max(int(x["ret"][last]), 0)
            end = body + int(x["wire_len"][last])
            moved = int((x["buf"][body: end] != x["deframed"][body: end]).sum())
            if kind == "chunked" and call == we.RESPONSES and x["stop"][1] == E:
                deframed_last_line += x["body_kind"][last] == rhp.FRAME_CHUNKED and end > x["lim"] - 16 and moved > 0
            if call == we.RESUME and kind in partial and x["stop"][1] == B and x["body_kind"][last] == rhp.FRAME_CHUNKED:
                partial[kind] += end == x["lim"] and x["body_len"][last] > 0 and moved > 0
            if kind == "head":
                for k in range(lo, lo + n):
                    if x["ret"][k] > 0:
                        value_to_lim += any(int(x["start"][k]) + int(h[2]) + int(h[3]) + 4 == x["lim"] for h in x["hdrs"][k])
    for kind in ("length", "chunked"):
        assert stops[we.RESPONSES, kind] == {E, H, B} and stops[we.RESUME, kind] == {E, H, B}, kind
    for kind in ("head", "sp"):   # (and BODY where c < 0 cuts the body of the HELLO before the last message)
        assert stops[we.RESPONSES, kind] == {E, H, B} and stops[we.RESUME, kind] == {E, H, B}, kind
    assert stops[we.RESUME, "close"] == {E, H, B, C}
    assert stops[we.RESUME, "in_length"] == {E, H, B} and stops[we.RESUME, "in_chunked"] == {E, H, B}
    assert stops[we.RESUME, "in_close"] == {C}
    assert deframed_last_line >= 1, "a completed chunked body whose wire span ends in the last line below lim, bytes moved"
    assert partial["chunked"] >= 1 and partial["in_chunked"] >= 1, "chunk data that runs to the clamped end, bytes moved"
    assert value_to_lim >= 1, "a header value that ends as close to lim as a parsed head's can: its CRLF CRLF end at lim - 1"
    for i in range(len(g["call"])):   # lim - c: where the last message (the continuation's session) starts
        residues.setdefault(int(g["buf_kind"][g["case_buf"][i]]), set()).add((int(g["lim"][i]) - int(g["c"][i])) % 16)
    assert len(residues) == len(KINDS) and all(v == set(range(16)) for v in residues.values()), "a start at every residue mod 16"


@pytest.mark.parametrize("deframe", [0, ws.DEFRAME])
@pytest.mark.parametrize("call,kind", CALL_KINDS, ids=IDS)
def test_cpu_twin_equals_golden(call, kind, deframe):
    """rhp_cpu_walk_responses / rhp_cpu_walk_resume with bytes_size= on every case of the kind"""
    for i in cases_of(call, kind):
        check(i, run(i, deframe, gpu=False), "rhp_cpu_walk_" + we.CALL_NAMES[call], deframe)


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
@pytest.mark.parametrize("call,kind", [(we.RESPONSES, "chunked"), (we.RESPONSES, "sp"), (we.RESUME, "head"), (we.RESUME, "in_chunked")])
def test_golden_equals_live_reference(call, kind):
    """the maker's walk over the compiled reference, run now over the clamped view, against the file"""
    from golden.make_golden_walk_edges import expected, walkers
    from golden.make_golden_walk_resume import state_array
    walks = walkers()
    for i in cases_of(call, kind):
        x = golden_case(i)
        answers, out = expected(walks, call, kind, x["pad"], x["lim"])
        for s, (res, rows, nxt) in enumerate(answers):
            lo = int(x["slot_off"][s])
            assert res == (int(x["n_slots"][s]), int(x["stop"][s]), int(x["consumed"][s])), (kind, x["c"], s)
            assert (nxt is None) == (x["kept"][s] == 1 or call == we.RESPONSES), (kind, x["c"], s)
            for k, row in enumerate(rows):
                assert row[:5] == tuple(int(x[f][lo + k]) for f in SLOT_FIELDS), (kind, x["c"], s, k)
                assert row[5][0] == int(x["ret"][lo + k]), (kind, x["c"], s, k)
                if row[5][0] > 0:
                    assert row[5][1:] == tuple(int(x[f][lo + k]) for f in MSG_FIELDS), (kind, x["c"], s, k)
                    assert [tuple(int(v) for v in h) for h in row[6]] == [tuple(int(v) for v in h) for h in x["hdrs"][lo + k]], (kind, x["c"], s, k)
            if call == we.RESUME and nxt is not None:
                assert state_bytes(state_array([nxt]))[0].tobytes() == state_bytes(x["states_out"])[s].tobytes(), (kind, x["c"], s)
        assert (out[: x["lim"]] == x["deframed"][: x["lim"]]).all(), (kind, x["c"])


# ---------------------------------------------------------------------------
# GPU: the kernels at the readable end


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", [0, ws.DEFRAME])
@pytest.mark.parametrize("call,kind", CALL_KINDS, ids=IDS)
def test_gpu_equals_golden(call, kind, deframe):
    """every case of the kind, one launch each: the device buffer is the whole buffer, bytes_size the case's;
    outputs poisoned first, guard bytes beside bytes, msgs, hdrs, slots, results and states"""
    t0 = time.perf_counter()
    ids = cases_of(call, kind)
    for i in ids:
        check(i, run(i, deframe, gpu=True), "rhp_walk_" + we.CALL_NAMES[call], deframe)
    print(f"{we.CALL_NAMES[call]}-{kind} deframe {deframe}: {len(ids)} launches, {time.perf_counter() - t0:.2f} s")


# ---------------------------------------------------------------------------
# slot_off and n_slots_total values that hold anything: one small batch per call, the n65 set of
# walk_responses.npz and round 1 of three_rounds of walk_resume.npz


@functools.lru_cache(maxsize=None)
def small_batch(call, deframe):
    """(args, base): the batch's arguments and its clean answers, which are the golden files' (checked here by the
    two files' own comparisons, so `base` is the reference's walk); args: dict of buf, sess_off, slot_off, states,
    maxh, flags"""
    b = we.small_batch(call)
    a = dict(b, flags=b["flags"] | deframe)
    if call == we.RESPONSES:
        import test_walk_responses as t
        base = rhp.walk_responses_cpu(a["buf"], a["sess_off"], a["slot_off"], a["maxh"], a["flags"])
        t.check("n65", base, "rhp_cpu_walk_responses", deframe)
    else:
        import test_walk_resume as t
        base = rhp.walk_resume_cpu(a["buf"], a["sess_off"], a["slot_off"], a["states"], a["maxh"], a["flags"])
        t.check("three_rounds", 1, base, "rhp_cpu_walk_resume", deframe)
    return a, base


def call_small(call, a, gpu, slot_off=None, n_slots_total=None):
    kw = dict(max_headers=a["maxh"], flags=a["flags"], n_slots_total=n_slots_total)
    if gpu:
        kw["guard"] = GUARD
    sl = a["slot_off"] if slot_off is None else slot_off
    if call == we.RESPONSES:
        return (rhp.walk_responses_gpu if gpu else rhp.walk_responses_cpu)(a["buf"], a["sess_off"], sl, **kw)
    return (rhp.walk_resume_gpu if gpu else rhp.walk_resume_cpu)(a["buf"], a["sess_off"], sl, a["states"], **kw)


def check_slotless(call, a, base, out, slot_off, nt, what):
    """`out` of a call whose slot_off / n_slots_total leave some sessions without slots, against the clean answers:
    such a session has n_slots 0, consumed 0, its state kept bit for bit and, by rhp.h's order of rules, stop BAD on
    a dead or corrupt state, the empty round's stop where a == e, RHP_WALK_MORE otherwise; nothing of it is
    de-framed; every slot no session owns keeps its poison; every other session is the clean run's"""
    so, sl0 = a["sess_off"], a["slot_off"]
    ns = len(so) - 1
    results, slots, msgs, hdrs, bytes_out = out[:5]
    assert len(slots) == len(msgs) == len(hdrs) == nt
    owns = np.array([slot_off[s] <= slot_off[s + 1] and slot_off[s + 1] <= nt for s in range(ns)])
    assert (~owns).any() and owns.any(), what
    st_in = a["states"] if a["states"] is not None else np.zeros(ns, dtype=rhp.WALK_STATE_DTYPE)
    touched = np.zeros(nt, dtype=bool)
    want_bytes = base[4].copy()
    raw = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1)
    for s in range(ns):
        got = tuple(int(results[f][s]) for f in ("n_slots", "stop", "consumed"))
        if owns[s]:
            assert (slot_off[s], slot_off[s + 1]) == (sl0[s], sl0[s + 1]), "an owning session keeps its own range"
            assert got == tuple(int(base[0][f][s]) for f in ("n_slots", "stop", "consumed")), f"{what}: session {s} is {got}"
            for k in range(int(sl0[s]), int(sl0[s]) + got[0]):
                touched[k] = True
                assert slots[k] == base[1][k] and msgs["ret"][k] == base[2]["ret"][k], f"{what}: slot {k} of session {s}"
                if base[2]["ret"][k] > 0:
                    n = int(base[2]["num_headers"][k])
                    assert msgs[k] == base[2][k] and (hdrs[k, :n] == base[3][k, :n]).all(), f"{what}: the records of slot {k}"
            continue
        ph, empty = int(st_in["phase"][s]), so[s] == so[s + 1]
        dec = st_in["decoder"][s]
        dead = ph >= wr.DEAD or st_in["reserved"][s] != 0 or (ph == wr.IN_CHUNKED and (dec["state"] > 5 or dec["hex_count"] > 16))
        stop = Y if dead else ({wr.AT_HEAD: E, wr.IN_CLOSE: C}.get(ph, B) if empty else M)
        assert got == (0, stop, 0), f"{what}: session {s}, which owns no slot, is {got}, not (0, {stop}, 0)"
        want_bytes[int(so[s]): int(so[s + 1])] = a["buf"][int(so[s]): int(so[s + 1])]
    for x, label in ((slots, "slot"), (msgs, "message record"), (hdrs, "header records")):
        assert (raw(x)[~touched] == rhp.WALK_POISON).all(), f"{what}: a {label} that no session owns was written"
    if call == we.RESUME:
        want = np.where(owns[:, None], state_bytes(base[5]), state_bytes(st_in))
        assert (state_bytes(out[5]) == want).all(), f"{what}: a state differs"
    assert (bytes_out == want_bytes).all(), f"{what}: the bytes differ"


def slot_cases(sl0, nt):
    """[(label, slot_off)]: rows 0, 9, a middle one and the last set to a value that leaves both neighbours without
    slots; 2^32 + the row's own value is what a 32-bit truncation before the compare would accept"""
    ns = len(sl0) - 1
    rows = [0, 9, ns // 2, ns]
    out = []
    for label, f in (("n_slots_total + 1", lambda v: nt + 1), ("2^32", lambda v: 2 ** 32), ("2^32 + own", lambda v: 2 ** 32 + int(v)),
                     ("2^64 - 1", lambda v: 2 ** 64 - 1)):
        sl = sl0.copy()
        for r in rows:
            sl[r] = f(sl0[r])
        out.append((label, sl))
    return out


def slotless(call, deframe, gpu):
    a, base = small_batch(call, deframe)
    nt = int(a["slot_off"][-1])
    name = ("rhp_walk_" if gpu else "rhp_cpu_walk_") + we.CALL_NAMES[call]
    for label, sl in slot_cases(a["slot_off"], nt):
        # (slot_off[-1] itself may be the changed row: the host's copy, n_slots_total, stays what it was)
        check_slotless(call, a, base, call_small(call, a, gpu, slot_off=sl, n_slots_total=nt), sl, nt, f"{name} slot_off rows at {label}")
    half = nt // 2
    check_slotless(call, a, base, call_small(call, a, gpu, n_slots_total=half), a["slot_off"], half, f"{name} n_slots_total {half} of {nt}")


@pytest.mark.parametrize("deframe", [0, ws.DEFRAME])
@pytest.mark.parametrize("call", [we.RESPONSES, we.RESUME], ids=we.CALL_NAMES)
def test_cpu_slot_offsets_that_hold_anything(call, deframe):
    """the host twins: slot_off rows beyond n_slots_total, at and beyond 2^32, and a stale n_slots_total"""
    slotless(call, deframe, gpu=False)


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", [0, ws.DEFRAME])
@pytest.mark.parametrize("call", [we.RESPONSES, we.RESUME], ids=we.CALL_NAMES)
def test_gpu_slot_offsets_that_hold_anything(call, deframe):
    """the kernels: the same values; the record buffers of the stale n_slots_total are sized for it, between guard
    bytes.  Values that make two sessions share slots are a race by construction and are not run"""
    slotless(call, deframe, gpu=True)


# ---------------------------------------------------------------------------
# sess_off rows that hold anything, over the same small batches: the changed sessions against the reference walk the
# maker stored, every other session against the clean run


@functools.lru_cache(maxsize=None)
def stray_case(p):
    """case p of the file's off_* arrays: (call, lo, hi, value, deframe, {session: expected}, defr_idx, defr_val);
    expected: dict of res (n_slots, stop, consumed), state (32 bytes at exit, or None: kept) and rows, a list of
    (the five slot fields, ret, the five message fields, header records u16 [n, 4])"""
    g = golden()
    call, lo, hi = int(g["off_call"][p]), int(g["off_lo"][p]), int(g["off_hi"][p])
    t, h = int(g["off_slot"][p]), int(np.where(g["off_ret"][: int(g["off_slot"][p])] > 0, g["off_num_headers"][: int(g["off_slot"][p])], 0).sum())
    changed = {}
    for j, q in enumerate(range(int(g["off_sess"][p]), int(g["off_sess"][p + 1]))):
        rows = []
        for _ in range(int(g["off_n_slots"][q])):
            n = int(g["off_num_headers"][t]) if g["off_ret"][t] > 0 else 0
            rows.append((tuple(int(g["off_" + f][t]) for f in SLOT_FIELDS), int(g["off_ret"][t]),
                         tuple(int(g["off_" + f][t]) for f in MSG_FIELDS), g["off_hdr"][h: h + n]))
            t, h = t + 1, h + n
        st = None
        if call == we.RESUME and not g["off_kept"][q]:
            st = np.zeros(1, dtype=rhp.WALK_STATE_DTYPE)
            ph = int(g["off_st_phase"][q])
            st["phase"] = ph
            st["left"] = g["off_st_left"][q] if ph == wr.IN_LENGTH else 0
            st["decoder"]["bytes_left_in_chunk"] = g["off_st_left"][q] if ph == wr.IN_CHUNKED else 0
            for col, f in (("st_ct", "consume_trailer"), ("st_hex", "hex_count"), ("st_state", "state")):
                st["decoder"][f] = g["off_" + col][q]
        changed[max(lo - 1, 0) + j] = dict(res=tuple(int(g["off_" + f][q]) for f in ("n_slots", "stop", "consumed")), state=st, rows=rows)
    assert t == int(g["off_slot"][p + 1])
    d = slice(int(g["off_defr"][p]), int(g["off_defr"][p + 1]))
    return call, lo, hi, int(g["off_value"][p]), int(g["off_deframe"][p]), changed, g["off_defr_idx"][d], g["off_defr_val"][d]


def check_stray(p, deframe, out, what):
    call, lo, hi, value, _, changed, didx, dval = stray_case(p)
    a, base = small_batch(call, deframe)
    so0, sl = a["sess_off"], a["slot_off"]
    ns, nt = len(so0) - 1, int(sl[-1])
    what = f"{what}: sess_off rows [{lo}, {hi}] at {value} (deframe {deframe})"
    results, slots, msgs, hdrs, bytes_out = out[:5]
    assert sorted(changed) == list(range(max(lo - 1, 0), min(hi, ns - 1) + 1)), what
    st_in = a["states"] if a["states"] is not None else np.zeros(ns, dtype=rhp.WALK_STATE_DTYPE)
    want_states = state_bytes(base[5]).copy() if call == we.RESUME else None
    touched = np.zeros(nt, dtype=bool)
    raw = lambda x: np.ascontiguousarray(x).view(np.uint8).reshape(len(x), -1)
    for s in range(ns):
        got = tuple(int(results[f][s]) for f in ("n_slots", "stop", "consumed"))
        k0 = int(sl[s])
        if s not in changed:
            assert got == tuple(int(base[0][f][s]) for f in ("n_slots", "stop", "consumed")), f"{what}: session {s} is {got}"
            for k in range(k0, k0 + got[0]):
                touched[k] = True
                assert slots[k] == base[1][k] and msgs["ret"][k] == base[2]["ret"][k], f"{what}: slot {k} of session {s}"
                if base[2]["ret"][k] > 0:
                    n = int(base[2]["num_headers"][k])
                    assert msgs[k] == base[2][k] and (hdrs[k, :n] == base[3][k, :n]).all(), f"{what}: the records of slot {k}"
            continue
        x = changed[s]
        assert got == x["res"], f"{what}: session {s} is {got}, the reference's {x['res']}"
        for k, (fields, ret, msg, hdr) in zip(range(k0, k0 + got[0]), x["rows"]):
            touched[k] = True
            assert tuple(int(slots[f][k]) for f in SLOT_FIELDS) == fields and int(msgs["ret"][k]) == ret, f"{what}: slot {k} of session {s}"
            if ret > 0:
                assert tuple(int(msgs[MSG_COLUMN.get(f, f)][k]) for f in MSG_FIELDS) == msg, f"{what}: the message record of slot {k}"
                assert msgs["reserved"][k] == 0 and msgs["flags"][k] == 0
                want = np.ascontiguousarray(hdr).view(rhp.HDR_DTYPE).reshape(-1)
                assert (hdrs[k, : len(want)] == want).all(), f"{what}: the header records of slot {k}"
            elif ret == 0 and fields[3] == 1:
                assert not raw(msgs)[k].any() and (raw(hdrs)[k] == rhp.WALK_POISON).all(), f"{what}: the continuation slot {k}"
        if call == we.RESUME:
            want_states[s] = state_bytes(st_in)[s] if x["state"] is None else state_bytes(x["state"])[0]
    for x, label in ((slots, "slot"), (msgs, "message record"), (hdrs, "header records")):
        assert (raw(x)[~touched] == rhp.WALK_POISON).all(), f"{what}: a {label} past n_slots was written"
    if call == we.RESUME:
        bad = np.flatnonzero((state_bytes(out[5]) != want_states).any(axis=1))
        assert not len(bad), f"{what}: the state of session {int(bad[0])} differs"
    want_bytes = base[4].copy()
    if deframe:   # from the first changed session's start on: the input, but for what the file says is moved
        first = min(int(so0[max(lo - 1, 0)]), we.readable(a["buf"].size))
        want_bytes[first:] = a["buf"][first:]
        want_bytes[didx] = dval
    assert (bytes_out == want_bytes).all(), f"{what}: the bytes differ"


def stray(call, deframe, gpu):
    g = golden()
    a, _ = small_batch(call, deframe)
    name = ("rhp_walk_" if gpu else "rhp_cpu_walk_") + we.CALL_NAMES[call]
    cases = we.stray_cases(call)
    ps = [p for p in range(len(g["off_call"])) if g["off_call"][p] == call]
    assert [(int(g["off_lo"][p]), int(g["off_hi"][p]), int(g["off_value"][p]), int(g["off_deframe"][p])) for p in ps] == cases
    ran = 0
    for p in ps:
        if deframe and not g["off_deframe"][p]:   # overlapping sessions that move bytes race: not run
            continue
        so = we.stray_offsets(a["sess_off"], *cases[ps.index(p)][:3])
        kw = dict(max_headers=a["maxh"], flags=a["flags"], **({"guard": GUARD} if gpu else {}))
        if call == we.RESPONSES:
            out = (rhp.walk_responses_gpu if gpu else rhp.walk_responses_cpu)(a["buf"], so, a["slot_off"], **kw)
        else:
            out = (rhp.walk_resume_gpu if gpu else rhp.walk_resume_cpu)(a["buf"], so, a["slot_off"], a["states"], **kw)
        check_stray(p, deframe, out, name)
        ran += 1
    assert ran == (5 if deframe else len(cases))


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
@pytest.mark.parametrize("call", [we.RESPONSES, we.RESUME], ids=we.CALL_NAMES)
def test_stray_golden_equals_live_reference(call):
    """the maker's walk over the changed sessions of every stray sess_off case, run now, against the file"""
    from golden.make_golden_walk_edges import stray_expected, walkers
    from golden.make_golden_walk_resume import state_array
    walks = walkers()
    buf = we.small_batch(call)["buf"]
    for p in range(len(golden()["off_call"])):
        if golden()["off_call"][p] != call:
            continue
        _, lo, hi, value, deframe, changed, didx, dval = stray_case(p)
        answers, out, _ = stray_expected(walks, call, lo, hi, value)
        assert [a[0] for a in answers] == sorted(changed), p
        for s, res, rows, nxt in answers:
            x = changed[s]
            assert res == x["res"] and len(rows) == len(x["rows"]), (p, s)
            for row, (fields, ret, msg, hdr) in zip(rows, x["rows"]):
                assert row[:5] == fields and row[5][0] == ret, (p, s)
                if ret > 0:
                    assert row[5][1:] == msg and [tuple(int(v) for v in h) for h in row[6]] == [tuple(int(v) for v in h) for h in hdr], (p, s)
            assert (nxt is None) == (x["state"] is None), (p, s)
            if nxt is not None:
                assert state_bytes(state_array([nxt])).tobytes() == state_bytes(x["state"]).tobytes(), (p, s)
        if deframe:
            d = np.flatnonzero(out != buf)
            assert (d == didx).all() and (out[d] == dval).all(), p


@pytest.mark.parametrize("deframe", [0, ws.DEFRAME])
@pytest.mark.parametrize("call", [we.RESPONSES, we.RESUME], ids=we.CALL_NAMES)
def test_cpu_sess_offsets_that_hold_anything(call, deframe):
    """the host twins against the stored reference walk: single sess_off rows at 2^64 - 1, 2^63, bytes_size,
    bytes_size - 1, lim, lim + 1 and lim - 1 (row s: session s - 1 runs to lim through its neighbours, session s is
    empty); with RHP_WALK_DEFRAME only the last three rows at a value from lim on"""
    stray(call, deframe, gpu=False)


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", [0, ws.DEFRAME])
@pytest.mark.parametrize("call", [we.RESPONSES, we.RESUME], ids=we.CALL_NAMES)
def test_gpu_sess_offsets_that_hold_anything(call, deframe):
    """the kernels against the same stored answers, which the twins equal too (the test above): the two clamp
    lines keep these values from becoming addresses; guard bytes beside every buffer.  sess_off rows that make
    sessions overlap under RHP_WALK_DEFRAME are a race by construction and are not run"""
    stray(call, deframe, gpu=True)
