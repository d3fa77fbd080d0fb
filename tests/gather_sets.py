"""Input sets of the rhp_gather_wide tests (tests/test_gather_wide.py), built by
hand from the generators of classify_session_sets.py and session_sets.py and
the requests of test_reactor_records.stream_wide.

  causes   for every cause that keeps a slot out of the dense copies (CAUSES)
           REPEAT sessions that hold the wide request, a dense request just
           inside the limit next to it and TFB GETs around them; sessions whose
           walk stops on -1, 0 and RHP_RET_TOOLONG with wide requests before
           the stop and, behind a -1, requests whose stale speculative records
           carry wide marks in slots nobody owns; a session of one piece with
           three requests (`more`); stream_wide() as one session
  mixed    classify_session_sets' 60 seeded sessions (chunked bodies, pieces
           inside bodies, requests behind a -1)
  shapes   session_sets.packed_shapes(): the fix-up's wave-prefix leads
  geom_*   TFB GETs, n slots around the kernels' wave and workgroup edges, as n
           sessions of one piece or one session of n; no slot wide, every slot
           wide (a leading CRLF on each request) or only the last one
  bodies_* chunked POSTs whose de-framed bodies give every destination and
           source alignment of the copy, the sizes around 4096, a 100 KB body
"""
from __future__ import annotations

import functools

import numpy as np

import libreactorng_amd as rhp
import classify_session_sets as css
import session_sets
from test_reactor_records import stream_wide

MAX_HEADERS = 16
TFB = session_sets.TFB
REPEAT = 6


def chunked(path: bytes, body: bytes, chunk: int = 0) -> bytes:
    """a chunked POST whose de-framed body is `body`, in chunks of `chunk` bytes (0: one chunk)"""
    step = chunk or max(len(body), 1)
    parts = [b"%x\r\n" % len(body[a: a + step]) + body[a: a + step] + b"\r\n" for a in range(0, len(body), step)]
    return b"POST " + path + b" HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n" + b"".join(parts) + b"0\r\n\r\n"


# cause -> (the wide request, the dense request just inside the limit); the targets name them
CAUSES = {
    "crlf": (b"\r\nGET /w-crlf HTTP/1.1\r\nHost: a\r\n\r\n", b"GET /d-crlf HTTP/1.1\r\nHost: a\r\n\r\n"),
    "nospace": (b"GET /w-nospace HTTP/1.1\r\nHost:x\r\n\r\n", b"GET /d-nospace HTTP/1.1\r\nHost: x\r\n\r\n"),
    "ows": (b"GET /w-ows HTTP/1.1\r\nHost: a \t \r\nB: c\r\n\r\n", b"GET /d-ows HTTP/1.1\r\nHost: a\r\nB: c\r\n\r\n"),
    "fold": (b"GET /w-fold HTTP/1.1\r\nA: b\r\n \tfolded\r\nHost: a\r\n\r\n", b"GET /d-fold HTTP/1.1\r\nA: b\r\nHost: a\r\n\r\n"),
    "lf": (b"GET /w-lf HTTP/1.1\nX: y\nZ: w\n\n", b"GET /d-lf HTTP/1.1\r\nX: y\r\nZ: w\r\n\r\n"),
    "name63": (b"GET /w-name63 HTTP/1.1\r\n" + b"N" * 63 + b": v\r\nHost: a\r\n\r\n",
               b"GET /d-name63 HTTP/1.1\r\n" + b"N" * 62 + b": v\r\nHost: a\r\n\r\n"),
    "value1008": (b"GET /w-value1008 HTTP/1.1\r\nHost: a\r\nX: " + b"v" * 1008 + b"\r\n\r\n",
                  b"GET /d-value1008 HTTP/1.1\r\nHost: a\r\nX: " + b"v" * 1007 + b"\r\n\r\n"),
    "method256": (b"M" * 256 + b" /w-method256 HTTP/1.1\r\nHost: a\r\n\r\n", b"M" * 255 + b" /d-method256 HTTP/1.1\r\nHost: a\r\n\r\n"),
    "chunked": (chunked(b"/w-chunked", b"hello world"), b"POST /d-chunked HTTP/1.1\r\nContent-Length: 11\r\n\r\nhello world"),
}
BAD = session_sets.BAD
PARTIAL = session_sets.PARTIAL
TOOLONG = b"GET /toolong HTTP/1.1\r\nX: " + b"v" * 66000 + b"\r\n\r\n"
STOPS = {"bad": (BAD, -1), "partial": (PARTIAL, 0), "toolong": (TOOLONG, rhp.RHP_RET_TOOLONG)}
STOP_SESSIONS = 3
W_CRLF, W_CHUNKED = CAUSES["crlf"][0], CAUSES["chunked"][0]
# behind a -1: slots nobody owns, wide marks in their stale speculative records (requests that are whole pieces)
BEHIND = [CAUSES[k][0] for k in ("nospace", "ows", "fold", "lf", "name63", "value1008", "method256", "nospace")]
MORE = W_CRLF + TFB + W_CHUNKED       # one piece, three requests


def causes_sessions():
    """[(bytes, one piece?)]"""
    out = []
    for k in range(REPEAT):
        for wide, dense in CAUSES.values():
            out.append((b"".join([TFB] * (k % 3) + [wide, dense, TFB] + [dense, wide] * (k % 2)), False))
    for stop, _ in STOPS.values():
        for k in range(STOP_SESSIONS):
            behind = b"".join(BEHIND) if stop is BAD else b""
            out.append((b"".join([W_CRLF, TFB] * k + [W_CRLF, W_CHUNKED, stop]) + behind, False))
    out.append((MORE, True))
    out.append((stream_wide(), False))
    return out


def _causes():
    ss = causes_sessions()
    one = iter([o for _, o in ss])
    buf, off, sess, _ = rhp.pack_sessions([d for d, _ in ss], split=lambda data: [len(data)] if next(one) else rhp.split_pieces(data))
    return buf, off, sess


GEOMETRY_SIZES = css.GEOMETRY_SIZES
TOP_EDGE = 1024 * 64   # rhp_gather.hip kTopSlots: above it the top scan gives a thread more than one wave's sums
WIDE_TFB = b"\r\n" + TFB


def _geometry(n, split, which):
    """n TFB GETs as n sessions or one; which: "none", "all" (a leading CRLF on each) or "last" """
    reqs = [WIDE_TFB if which == "all" or (which == "last" and q == n - 1) else TFB for q in range(n)]
    if split:
        buf, off, sess, _ = rhp.pack_sessions(reqs)
    else:   # cut at the requests' ends (the empty-line split would leave a leading CRLF with the piece before)
        buf, off, sess, _ = rhp.pack_sessions([b"".join(reqs)], split=lambda data: [len(r) for r in reqs])
    assert len(off) - 1 == n and len(sess) == (n if split else 1)
    return buf, off, sess


def _top_edge():
    """TOP_EDGE + 65 slots in sessions of 1..300 requests, every 97th request wide, a chunked POST every 5000th"""
    n, reqs = TOP_EDGE + 65, []
    for q in range(n):
        reqs.append(chunked(b"/c%d" % q, b"b" * (q % 50)) if q % 5000 == 77 else WIDE_TFB if q % 97 == 0 else TFB)
    sizes, at = [], 0
    while at < n:
        sizes.append(min((1, 300, 64, 5, 129)[len(sizes) % 5], n - at))
        at += sizes[-1]
    lo = np.cumsum([0] + sizes[:-1])
    datas = [b"".join(reqs[a: a + k]) for a, k in zip(lo, sizes)]
    cuts = iter([[len(r) for r in reqs[a: a + k]] for a, k in zip(lo, sizes)])
    buf, off, sess, _ = rhp.pack_sessions(datas, split=lambda data: next(cuts))
    assert len(off) - 1 == n
    return buf, off, sess


BODY_LENS = tuple(range(34))        # back to back: every destination alignment
PATH_LENS = tuple(range(1, 17))     # every source alignment
BIG_BODIES = (4095, 4096, 4097)
HUGE_BODY = 100 * 1024


def _body(length, seed):
    return np.random.default_rng(seed).integers(0, 256, size=length, dtype=np.uint8).tobytes()


def _bodies(path_len):
    reqs = [chunked(b"/" + b"p" * (path_len - 1), _body(k, k)) for k in BODY_LENS]
    buf, off, sess, _ = rhp.pack_sessions([b"".join(reqs)])
    return buf, off, sess


def _bodies_big():
    reqs = [chunked(b"/big%d" % k, _body(k, k), 1500) for k in BIG_BODIES] + [TFB, chunked(b"/huge", _body(HUGE_BODY, 5), 1024)]
    buf, off, sess, _ = rhp.pack_sessions([b"".join(reqs[:3]), b"".join(reqs[3:])])
    return buf, off, sess


def _css(name):
    return css.SETS[name]()


SETS = {"causes": _causes, "mixed": lambda: _css("mixed"), "shapes": lambda: session_sets.packed_shapes(),
        "top_edge": _top_edge, "bodies_big": _bodies_big}
GEOMETRY = []
for _n in GEOMETRY_SIZES:
    for _split in (True, False):
        for _which in ("none", "all", "last"):
            _name = f"geom_{'split' if _split else 'one'}_{_n}_{_which}"
            SETS[_name] = lambda n=_n, split=_split, which=_which: _geometry(n, split, which)
            GEOMETRY.append(_name)
BODIES = [f"bodies_path{_k}" for _k in PATH_LENS]
for _k in PATH_LENS:
    SETS[f"bodies_path{_k}"] = lambda k=_k: _bodies(k)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(buf, piece offsets, rhp_session_t array) of a set, built once; the tests only read them"""
    return SETS[name]()
