"""Input sets of the rhp_classify_sessions tests (tests/test_classify_sessions.py)
and of their golden fixture (tests/golden/classify_sessions.npz, written by
tests/golden/make_golden_classify_sessions.py from the compiled reference's
http_field_lookup at the request boundaries of the reference's session loop).
Every set is rebuilt from seeds or by hand here; the fixture holds only the
sha256 of its inputs and the expected (fields, route) arrays by record slot,
which do not depend on the record layout or on which parser made the records.

  mixed     60 seeded sessions of 1-40 requests: the request pool of
            test_sessions.py and requests made for the lookup (EXTRA), some
            sessions with a malformed request in the middle and well-formed
            GET /plaintext requests behind it, all with a tail.  The speculative
            parse leaves result-1 records that match a route in slots the fix-up
            does not use: pieces that began inside a body, pieces behind a -1.
  shapes    session_sets.packed_shapes(9): the fix-up's wave-prefix leads, a
            session with no piece and a session of one empty piece.
  geom_*    TFB GETs only, n record slots around the kernel's wave and block
            edges: n sessions of one piece each (the search runs over n entries)
            and one session that holds all n; and no session at all over 65 slots.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

import libreactorng_amd as rhp
import session_sets
from test_sessions import request_pool

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classify_sessions.npz")

MAX_HEADERS = 16
N64 = b"X-Sixty-Four-Bytes-" + b"n" * 44 + b"z"   # the longest lookup name
assert len(N64) == rhp.CLASSIFY_NAME_MAX
NAMES = (b"Host", b"Connection", b"Content-Length", b"Transfer-Encoding", N64)
ROUTES = ((b"GET", b"/plaintext"), (None, b"/c"), (b"POST", b"/cl"), (b"GET", b"/inside-a-body"))

TFB = session_sets.TFB
FAKE = b"GET /inside-a-body HTTP/1.1\r\nHost: fake\r\n\r\n"   # a whole request inside a body
_CL_BODY = b"line one\r\n\r\n" + FAKE + b"\n\ntail"        # empty lines around it: a piece starts at FAKE
_CHUNK = b"ab\r\n\r\n" + FAKE + b"cd"
EXTRA = (
    b"GET /plaintext HTTP/1.1\r\nhOsT: MiXed\r\ncONNECTION: Close\r\ncontent-LENGTH: 0\r\n\r\n",   # names in mixed case
    b"GET /plaintext HTTP/1.1\r\nHost: first\r\nX: y\r\nhost: second\r\nHOST: third\r\n\r\n",       # the first wins
    b"GET /c HTTP/1.1\r\nHost: a\r\n folded\r\nConnection: after-fold\r\n\r\n",                      # obs-fold
    b"PUT /c HTTP/1.1\r\nConnection: x\r\n\tfolded: Host\r\nHost: b\r\n\r\n",
    b"GET /plaintext HTTP/1.1\r\n" + b"".join(b"H%d: v\r\n" % k for k in range(15)) +
    N64.swapcase() + b": sixteenth\r\n\r\n",                                                         # the 16th of 16
    b"GET /plaintext HTTP/1.1\nHost: lf-only\nConnection: keep-alive\n\n",                           # LF-only line ends
    b"GET /c HTTP/1.1\r\nHost:\r\nConnection: \r\n\r\n",                                             # empty values
    b"POST /cl HTTP/1.1\r\nHost: outer\r\nContent-Length: %d\r\n\r\n" % len(_CL_BODY) + _CL_BODY,
    b"POST /c HTTP/1.1\r\nHost: outer\r\nTransfer-Encoding: chunked\r\n\r\n%x\r\n" % len(_CHUNK) + _CHUNK + b"\r\n0\r\n\r\n",
    b"DELETE /plaintext HTTP/1.1\r\nHost: wrong-method\r\n\r\n",                                     # a route's target, not its method
    b"GET /plaintext/ HTTP/1.1\r\nHosts: near\r\nConnectio: near\r\n\r\n",                           # near misses
)
GEOMETRY_SIZES = (1, 63, 64, 65, 255, 256, 257, 1025)
NO_SESSION_SLOTS = 65


def mixed_sessions(n_sessions=60, seed=20261019):
    rng = np.random.default_rng(seed)
    pool, bad, tails = request_pool(rng)
    pool = list(pool) + list(EXTRA) * 2   # (the lookup's requests as often as the pool's)
    out = []
    for s in range(n_sessions):
        k = int(rng.integers(1, 41))
        parts = [pool[int(rng.integers(len(pool)))] for _ in range(k)]
        if s % 4 == 1:   # a malformed request in the middle, well-formed requests behind it
            at = int(rng.integers(len(parts) + 1))
            parts[at:at] = [bad[int(rng.integers(len(bad)))]] + [TFB] * 3
        parts.append(tails[int(rng.integers(len(tails)))])
        out.append(b"".join(parts))
    return out


def _mixed():
    buf, off, sess, _ = rhp.pack_sessions(mixed_sessions())
    return buf, off, sess


def _geometry(n, split):
    """n TFB GETs: as n sessions of one piece, or as one session of n pieces"""
    buf, off, sess, _ = rhp.pack_sessions([TFB] * n if split else [TFB * n])
    assert len(off) - 1 == n and len(sess) == (n if split else 1)
    return buf, off, sess


def _no_session():
    buf, off, _ = _geometry(NO_SESSION_SLOTS, False)
    return buf, off, np.zeros(0, dtype=rhp.SESSION_DTYPE)


# name -> inputs() -> (buf, piece offsets, rhp_session_t array); every set at MAX_HEADERS with NAMES and ROUTES
SETS = {"mixed": _mixed, "shapes": lambda: session_sets.packed_shapes(9)}
for _n in GEOMETRY_SIZES:
    SETS[f"geom_split_{_n}"] = lambda n=_n: _geometry(n, True)
    SETS[f"geom_one_{_n}"] = lambda n=_n: _geometry(n, False)
SETS[f"geom_none_{NO_SESSION_SLOTS}"] = _no_session
GEOMETRY = tuple(k for k in SETS if k.startswith("geom_"))

_golden = None
_inputs = {}


def digest(buf, off, sess):
    d = hashlib.sha256()
    for a in (buf, off, sess):
        d.update(np.ascontiguousarray(a).tobytes())
    return d.hexdigest()


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
    """(fields FIELDREF_DTYPE [n_names, n], route u16 [n]) by record slot, from the compiled reference"""
    g = golden()
    assert g is not None, f"{GOLDEN} is missing (tests/golden/make_golden_classify_sessions.py writes it)"
    f = g[name + "/fields"]
    out = np.zeros(f.shape[:2], dtype=rhp.FIELDREF_DTYPE)
    out["value_off"], out["value_len"] = f[..., 0], f[..., 1]
    return out, g[name + "/route"]
