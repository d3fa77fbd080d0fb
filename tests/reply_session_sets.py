"""Input sets of the rhp_reply_sessions tests (tests/test_reply_sessions.py) and
of their golden fixture (tests/golden/reply_sessions.npz, written by
tests/golden/make_golden_reply_sessions.py from the compiled reference: its
request boundaries and results, its http_field_lookup-side route match, its
http_write_response over the answered requests in session order).

The sets of classify_session_sets (mixed, shapes, the geometry sets) under its
NAMES and ROUTES, and one more:

  runs      every session is a static run of L requests -- TFB GETs (route 0) and
            a POST /cl with a body (route 2) in turn -- followed by one stopper;
            every (L, stopper) pair of RUN_LENGTHS x STOPPERS once, shuffled by a
            fixed seed so that long and short sessions alternate.  RUN_LENGTHS
            lie around the scan's wave (64 slots) and tile (256 slots) edges.

Routes 0, 2 and 3 are static (STATIC_MASK); route 1 (/c, any method) is the
host's.  The reply images are one response per route (responses()).
"""
from __future__ import annotations

import functools
import hashlib
import os

import numpy as np

import libreactorng_amd as rhp
import classify_session_sets as css
import session_sets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reply_sessions.npz")

MAX_HEADERS = css.MAX_HEADERS
ROUTES = css.ROUTES
STATIC_MASK = 0b1101
BIG_BODY = 20000   # route 3's body: a wave's run of it exceeds any LDS stage

TFB = session_sets.TFB
POST_CL = session_sets.WHOLE[3]   # POST /cl with a body that holds an empty line
RUN_LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257, 1025)
HOST_REQ = b"PUT /c HTTP/1.1\r\nHost: the-host-answers\r\n\r\n"
STOPPERS = {
    "host": HOST_REQ + TFB + POST_CL + TFB,                       # a /c request, static requests behind it
    "noroute": b"GET /nowhere HTTP/1.1\r\nHost: x\r\n\r\n" + TFB,  # a ready request that matches no route
    "bad": session_sets.BAD + TFB,                                # malformed: the session ends on -1
    "partial": session_sets.PARTIAL,                              # a partial tail: result 0
    "end": b"",                                                   # the end of the input
}
AFTER_STOP = {"host": 3, "noroute": 1}   # static requests behind the stop, which must not be answered


@functools.lru_cache(maxsize=None)
def runs():
    """[(L, stopper, bytes)] in the set's order"""
    out = [(L, st, b"".join(TFB if q % 2 == 0 else POST_CL for q in range(L)) + tail)
           for L in RUN_LENGTHS for st, tail in STOPPERS.items()]
    order = np.random.default_rng(20261020).permutation(len(out))
    out = [out[int(k)] for k in order]
    assert {(L, st) for L, st, _ in out} == {(L, st) for L in RUN_LENGTHS for st in STOPPERS} and \
        len(out) == len(RUN_LENGTHS) * len(STOPPERS), "every (L, stopper) pair once"
    assert any(st in AFTER_STOP for _, st, _ in out), "a session with static requests after its stop"
    return tuple(out)


def _runs():
    buf, off, sess, _ = rhp.pack_sessions([data for _, _, data in runs()])
    return buf, off, sess


SETS = dict(css.SETS)
SETS["runs"] = _runs
GEOMETRY = css.GEOMETRY


@functools.lru_cache(maxsize=None)
def responses():
    """(arena, resps, fields): one response per route of ROUTES, the reply images"""
    parts, pos = [], 0

    def add(b):
        nonlocal pos
        parts.append(b)
        pos += len(b)
        return [pos - len(b), len(b)]

    ok, plain, js = add(b"200 OK"), add(b"text/plain"), add(b"application/json")
    hello, one, empty = add(b"Hello, World!"), add(b"x"), [pos, 0]
    big = add(np.random.default_rng(3).integers(0x20, 0x7F, size=BIG_BODY, dtype=np.uint8).tobytes())
    fields = np.array([add(b"Cache-Control") + add(b"no-store"), add(b"X-Request-Id") + add(b"cl-0001")], dtype=np.uint32)
    resps = np.array([ok + plain + hello + [0, 0],    # route 0: the TFB plaintext reply
                      ok + plain + one + [0, 0],      # route 1: in the table, masked out
                      ok + js + empty + [0, 2],       # route 2: an empty body, two extra fields
                      ok + plain + big + [0, 0]],     # route 3
                     dtype=np.uint32)
    assert len(resps) == len(ROUTES)
    return np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), resps, fields


def digest(buf, off, sess):
    d = hashlib.sha256()
    for a in (buf, off, sess) + responses():
        d.update(np.ascontiguousarray(a).tobytes())
    d.update(bytes([STATIC_MASK]) + rhp.DEFAULT_DATE)
    return d.hexdigest()


_golden = None
_inputs = {}


def golden():
    global _golden
    if _golden is None and os.path.exists(GOLDEN):
        _golden = dict(np.load(GOLDEN))
    return _golden


def inputs(name):
    """(buf, off, sessions) of a set, built once and checked against the fixture's
    sha256; the tests only read them (the parsers work on copies)"""
    if name not in _inputs:
        buf, off, sess = SETS[name]()
        g = golden()
        if g is not None:
            assert digest(buf, off, sess) == str(g[name + "/sha256"]), f"{name}: input drifted"
        _inputs[name] = (buf, off, sess)
    return _inputs[name]


def expected(name):
    """(count u32 [n_sessions], out_len u64 [n_sessions], total, sha256 of out, out bytes or None), from the
    compiled reference"""
    g = golden()
    assert g is not None, f"{GOLDEN} is missing (tests/golden/make_golden_reply_sessions.py writes it)"
    out = g.get(name + "/out")
    want = g[name + "/count"], g[name + "/out_len"], int(g[name + "/total"]), str(g[name + "/out_sha256"]), out
    if name == "runs":   # what the set is for, held against the reference's answer
        for (L, st, _), count in zip(runs(), want[0]):
            assert count == (0 if st == "bad" else L), f"runs: session ({L}, {st}) answers {count}"
    return want
