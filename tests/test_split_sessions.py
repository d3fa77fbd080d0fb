"""rhp_split_sessions (include/rhp.h): the packed input of a round's sessions cut
at every empty line on the device -- offsets[] and rhp_session_t[] for the parse
and the fix-up.

The yardstick is statement(): the cut rule of rhp.h in numpy, position by
position over the whole buffer at once, with the piece indices by rhp.h's two
formulas.  It shares no code with the host twin (rhp_cpu_split_sessions, a walk
over each session's bytes) or with the kernels (masks per 16 bytes, a scan, a
scatter), and is pinned once, session by session, against rhp.split_pieces and
rhp.pack_sessions, which look forward from every LF.

Every output holds 0xFF before a call; on the GPU every output is a Guarded
buffer, and n_pieces, offsets, sessions and work must leave the bytes around
them untouched."""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import gather_sets
import session_sets
import split_sets as ss

GUARD = 4096
POISON = rhp.SPLIT_POISON
POISON64 = np.uint64(0xFFFFFFFFFFFFFFFF)
STEP = rhp.SPLIT_STEP_BYTES
CAPS = ("exact", "roomy", "short")


def statement(buf, sess_off):
    """(n_pieces, offsets u64 [n_pieces + 1], sessions SESSION_DTYPE) by rhp.h's rule: position p, a < p < e, is
    a cut when bytes[p-1] is LF and bytes[p-2] is LF (p-2 >= a) or bytes[p-2] is CR and bytes[p-3] is LF (p-3 >= a)"""
    so = np.asarray(sess_off, dtype=np.int64)
    ns, begin, end = len(so) - 1, int(so[0]), int(so[-1])
    b = np.asarray(buf, dtype=np.uint8)
    sessions = np.zeros(ns, dtype=rhp.SESSION_DTYPE)
    if ns == 0:
        return 0, np.array([begin], dtype=np.uint64), sessions
    p = np.arange(begin, end, dtype=np.int64)
    starts = so[:-1]
    a = starts[np.searchsorted(starts, p, side="right") - 1]   # the start of the session that holds p (p < its e)
    is_at = lambda q, c: (q >= a) & (b[np.maximum(q, 0)] == c)   # bytes[q] == c, and q not before the session's start
    cut = (p > a) & is_at(p - 1, 10) & (is_at(p - 2, 10) | (is_at(p - 2, 13) & is_at(p - 3, 10)))
    cuts = p[cut]
    n_pieces = ns + len(cuts)
    offsets = np.full(n_pieces + 1, POISON64, dtype=np.uint64)
    lo = np.arange(ns) + np.searchsorted(cuts, starts, side="left")          # s + the cuts at positions < a
    in_session = np.searchsorted(starts, cuts, side="right") - 1
    offsets[lo] = starts.astype(np.uint64)
    offsets[in_session + np.arange(len(cuts)) + 1] = cuts.astype(np.uint64)   # the j-th cut, in session s: s + j + 1
    offsets[n_pieces] = end
    sessions["piece_lo"] = lo
    sessions["piece_hi"] = lo + 1 + np.bincount(in_session, minlength=ns)
    assert not (offsets == POISON64).any(), "the two formulas fill every index once"
    return n_pieces, offsets, sessions


def caps_of(n_pieces):
    """rhp.h's three cases; no cap is one short of no piece at all"""
    return {"exact": n_pieces, "roomy": n_pieces + 37, "short": n_pieces - 1 if n_pieces else None}


def expected(stated, cap, end):
    """what a call with `cap` leaves in buffers that held POISON: (n_pieces, offsets [cap + 1], sessions)"""
    n_pieces, offsets, sessions = stated
    if cap < n_pieces:
        return n_pieces, np.full(cap + 1, POISON64, dtype=np.uint64), np.full(len(sessions), POISON, dtype=np.uint8).repeat(8).view(rhp.SESSION_DTYPE)
    return n_pieces, np.concatenate([offsets, np.full(cap - n_pieces, end, dtype=np.uint64)]), sessions


def check(got, want, label):
    assert got[0] == want[0], f"{label}: n_pieces {got[0]}, want {want[0]}"
    assert len(got[1]) == len(want[1]) and len(got[2]) == len(want[2]), label
    bad = np.flatnonzero(got[1] != want[1])
    assert not len(bad), f"{label}: offsets[{bad[0]}] = {got[1][bad[0]]}, want {want[1][bad[0]]} ({len(bad)} differ)"
    bad = np.flatnonzero(got[2] != want[2])
    assert not len(bad), f"{label}: sessions[{bad[0]}] = {got[2][bad[0]]}, want {want[2][bad[0]]} ({len(bad)} differ)"


@functools.lru_cache(maxsize=None)
def stated(name):
    """statement() of a set, computed once and only read"""
    return statement(*ss.inputs(name))


# ---------------------------------------------------------------------------
# no GPU: the yardstick, the host twin, the refusals

SESSION_LISTS = {"shapes": lambda: [s[-2] for s in session_sets.shapes()],
                 "causes": lambda: [d for d, _ in gather_sets.causes_sessions()]}


@pytest.mark.parametrize("name", ss.NAMES)
def test_statement_is_split_pieces_per_session(name):
    """the pin: each session on its own, cut by rhp.split_pieces, numbered by rhp.pack_sessions"""
    data, first = ss.sessions(name)
    n_pieces, offsets, sessions = stated(name)
    _, off, sess, starts = rhp.pack_sessions(data)
    assert n_pieces == len(off) - 1 == sum(len(rhp.split_pieces(d)) for d in data)
    assert (offsets == off + np.uint64(first)).all() and (sessions == sess).all()
    assert (offsets[sessions["piece_lo"]] == starts + np.uint64(first)).all()


def test_sets_hold_what_they_are_for():
    n = {k: stated(k)[0] for k in ss.NAMES}
    assert n["tiny"] == 4 and n["tiny_only_1"] == n["tiny_only_2"] == 1 and n["tiny_only_3"] == 2
    assert n["end_lf_start_lf"] == 5 and n["end_lfcr_start_lf"] == 5   # no cut across a start; "\n\nxy" has its own
    assert n["end_lf_start_crlf"] == 5                                 # "\r\n\r\nxy": one, at 4
    assert n["all_lf_three_steps"] == 1 + 3 * STEP - 2 and n["no_lf"] == 1 and n["cr_only"] == 2
    assert n["no_session"] == n["no_session_at_5"] == 0 and n["empty_only"] == 1
    so = ss.inputs("many_in_one_step")[1]
    assert int(np.sum((so[:-1] >= STEP) & (so[:-1] < 2 * STEP))) >= 300
    for d in ss.DELTAS:   # every pattern cuts at every boundary it was laid around
        cuts = set(stated(f"edges_end_{d}")[1].tolist())
        assert all(b + d in cuts for i in range(len(ss.PATTERNS)) for b in ss.edge_boundaries(i)), d
    assert [int(ss.inputs(k)[1][0]) for k in ("first_0", "first_5", "first_16")] == [0, 5, 16]
    assert int(ss.inputs("past_the_scan_edge")[1][-1]) > ss.SCAN_STEPS * STEP


@pytest.mark.parametrize("name", ss.NAMES)
def test_cpu_twin_is_the_statement(name):
    buf, so = ss.inputs(name)
    for which, cap in caps_of(stated(name)[0]).items():
        if cap is not None:
            check(rhp.split_sessions_cpu(buf, so, cap), expected(stated(name), cap, int(so[-1])), f"{name} cap {which}")
    assert rhp.split_sessions_cpu(buf, so)[0] == stated(name)[0]


@pytest.mark.parametrize("which", list(SESSION_LISTS))
@pytest.mark.parametrize("first", [0, 5])
def test_cpu_twin_equals_pack_sessions(which, first):
    data = SESSION_LISTS[which]()
    _, off, sess, _ = rhp.pack_sessions(data, split=True)
    buf, so = rhp.pack_raw(data, first)
    n_pieces, offsets, sessions = rhp.split_sessions_cpu(buf, so)
    assert n_pieces == len(off) - 1
    assert (offsets == off + np.uint64(first)).all() and (sessions == sess).all()
    check((n_pieces, offsets, sessions), statement(buf, so), which)


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls go
    to the GPU library here: an accepted one would launch kernels over host memory"""
    gpu = which == "gpu-library"
    if gpu:
        fn = lambda b, e, so, ns, o: rhp.lib().rhp_split_sessions(b, e, so, ns, o, None)
    else:
        fn = lambda b, e, so, ns, o: rhp.host().rhp_cpu_split_sessions(b, e, so, ns, o)
    raw = np.full(64 + 16, ord("x"), dtype=np.uint8)
    b = raw[(-raw.ctypes.data) % 16:][:64]
    so = np.array([0, 40, 64], dtype=np.uint64)
    n_pieces, offsets = np.full(1, 77, dtype=np.uint64), np.full(5, 77, dtype=np.uint64)
    sessions = np.full(2, 77, dtype=np.uint64)
    work = np.zeros(rhp.split_work_words(64, 2), dtype=np.uint64)
    p = lambda a: a.ctypes.data

    def call(bytes_p=p(b), end=64, so_p=p(so), ns=2, patch=None):
        o = rhp.SplitOut(p(n_pieces), p(offsets), 4, p(sessions), p(work))
        if patch:
            patch(o)
        return fn(bytes_p, end, so_p, ns, ctypes.byref(o))

    E = -22
    assert fn(None, 0, None, 0, None) == E
    assert call(so_p=None) == E
    assert fn(p(b), 64, p(so), 2, None) == E
    for f in ("n_pieces", "offsets", "work", "sessions"):
        assert call(patch=lambda o: setattr(o, f, None)) == E, f
    assert call(bytes_p=None) == E
    assert call(bytes_p=p(b) + 4, end=60) == E and call(bytes_p=p(b) + 8, end=56) == E
    assert call(end=2 ** 32 - 2) == E and call(end=2 ** 32 - 1, ns=1) == E and call(end=2 ** 32, ns=0) == E
    assert call(end=1, ns=2 ** 32 - 1) == E and call(end=2 ** 64 - 1) == E
    assert n_pieces[0] == 77 and (offsets == 77).all() and (sessions == 77).all(), "a refused call writes nothing"
    if gpu:
        return
    # accepted by the host twin: no session without `sessions`, no byte without `bytes`
    assert call(ns=0, patch=lambda o: setattr(o, "sessions", None)) == 0
    assert n_pieces[0] == 0 and (offsets == 0).all()
    so0 = np.array([0, 0], dtype=np.uint64)
    assert call(bytes_p=None, end=0, so_p=p(so0), ns=1) == 0
    assert n_pieces[0] == 1 and (offsets == 0).all() and sessions.view(np.uint32).tolist() == [0, 1] + [77, 0]


def test_work_words():
    assert rhp.split_work_words(0, 9) == 1 and rhp.split_work_words(1) == 26
    assert rhp.split_work_words(STEP) == 26 and rhp.split_work_words(STEP + 1) == 51


def test_host_twin_asan_ubsan_clean():
    """`make split-sessions-asan`: a stand-alone program over the host sources (tests/split_sessions_host_test.c)"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "split-sessions-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "split_sessions_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernels against the statement and, byte for byte, the twin


@functools.lru_cache(maxsize=None)
def device_inputs(name):
    """a set's bytes (Guarded) and sess_off on the device, uploaded once"""
    import torch
    buf, so = ss.inputs(name)
    return rhp.Guarded("bytes", buf.size, GUARD, data=buf), torch.from_numpy(so.view(np.int64).copy()).to("cuda")


def gpu_split(name, cap):
    buf, so = ss.inputs(name)
    db, dso = device_inputs(name)
    got = rhp.split_sessions_device(db.view, int(so[-1]), dso, len(so) - 1, cap, GUARD)[1]()
    db.check()
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("which", CAPS)
@pytest.mark.parametrize("name", ss.NAMES)
def test_gpu_sets(name, which):
    buf, so = ss.inputs(name)
    cap = caps_of(stated(name)[0])[which]
    if cap is None:
        assert stated(name)[0] == 0 and which == "short"   # (no piece: there is no cap one short)
        return
    got = gpu_split(name, cap)
    label = f"{name} cap {which} ({cap})"
    check(got, expected(stated(name), cap, int(so[-1])), label + ": kernels against the statement")
    cpu = rhp.split_sessions_cpu(buf, so, cap)
    assert got[0] == cpu[0] and got[1].tobytes() == cpu[1].tobytes() and got[2].tobytes() == cpu[2].tobytes(), \
        label + ": kernels against the twin"


@pytest.mark.gpu
def test_gpu_split_sessions_gpu_counts_first():
    """the glue's own path: a count-only call (cap 0), then the exact cap"""
    data, first = ss.sessions("first_5")
    check(rhp.split_sessions_gpu(data, first=first, guard=GUARD), stated("first_5"), "split_sessions_gpu")


ROUND_SESSIONS = 65   # session_sets.shapes(): every lead and stopper once, the two empty sessions


@functools.lru_cache(maxsize=None)
def round_inputs():
    data = [s[-2] for s in session_sets.shapes()[:ROUND_SESSIONS]]
    buf, off, sess, _ = rhp.pack_sessions(data, split=True)
    return data, buf, off, sess


@pytest.mark.gpu
def test_gpu_round_from_raw_input():
    """split -> parse (n = cap) -> fix-up with no host step, against the fix-up over the host-split input and
    against the reference's loop"""
    from test_sessions import assert_same_fixup, check as check_sessions, oracle_sessions, used_slots
    data, buf, off, sess = round_inputs()
    n = len(off) - 1
    cap = n + 64
    res, results, starts, n_pieces, offsets, sessions = rhp.fixup_raw_gpu(data, cap, guard=GUARD)
    assert n_pieces == n and (offsets[: n + 1] == off).all() and (offsets[n:] == off[-1]).all() and (sessions == sess).all()
    want = rhp.fixup_gpu(buf, off, sess, guard=GUARD)
    # the session results, and req_start, the records and the de-framed bytes of every slot in use (header rows
    # past num_headers are unspecified, rhp.h)
    assert_same_fixup((res, results, starts), want, sess, int(off[-1]), "raw round against the host-split round", every_row=False)
    used = used_slots(sessions, results)
    assert len(used) and used.max() < n and (sessions["piece_hi"] <= n).all(), "a slot of an empty tail piece is in use"
    assert (res.http["result"][n:cap] == 0).all(), "an empty tail piece parses to 0"
    check_sessions(res, results, starts, buf, off, sess, "raw round against the reference's loop",
                   want=oracle_sessions(buf, off, [(int(a), int(b)) for a, b in sess]))
