"""Input cases of the rhp_forward_sessions tests (tests/test_forward_sessions.py)
and of their golden fixture (tests/golden/forward_sessions.npz, written by
tests/golden/make_golden_forward.py).

A case is a handful of sessions of pipelined input, split at every empty line
as the server splits them, with the drop names, the extra lines and max_headers
it is forwarded with.  Every case is classified over ROUTES and forwarded with
FORWARD_MASK: /up and /plaintext go upstream, /static is the device's own reply
and /host the host's; any other path matches no route.
"""
from __future__ import annotations

import functools
import os

import numpy as np

import libreactorng_amd as rhp
import session_sets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_sessions.npz")

ROUTES = ((b"", b"/up"), (b"", b"/static"), (b"", b"/plaintext"), (b"", b"/host"))
FORWARD_MASK = 0b0101
DROP = (b"Connection", b"Keep-Alive", b"Proxy-Connection", b"TE", b"Upgrade")
VIA = b"Via: 1.1 rhp\r\n"
_EXTRA = b"Via: 1.1 rhp\r\nX-Forwarded-For: 192.0.2.33\r\nX-Forwarded-Proto: https\r\nX-Request-Id: "
EXTRA_128 = _EXTRA + bytes(0x30 + k % 10 for k in range(rhp.FORWARD_EXTRA_MAX - len(_EXTRA) - 2)) + b"\r\n"
assert len(EXTRA_128) == rhp.FORWARD_EXTRA_MAX
LAYOUTS = (rhp.LAYOUT_REQUEST_MAJOR, rhp.LAYOUT_HEADER_MAJOR)

TFB = session_sets.TFB   # GET /plaintext, four headers, one of them Connection
GET = b"GET /up HTTP/1.1\r\nHost: upstream\r\nAccept: */*\r\n\r\n"
STATIC = b"GET /static HTTP/1.1\r\nHost: s\r\n\r\n"
HOST = b"PUT /host HTTP/1.1\r\nHost: h\r\n\r\n"
NOWHERE = b"GET /nowhere HTTP/1.1\r\nHost: x\r\n\r\n"
PARTIAL = b"GET /up HTTP/1.1\r\nHost:"
BAD = b"GET /up HTTP/1.1\r\nBad Header\r\n\r\n"
FOLD = b"GET /up HTTP/1.1\r\nHost: a\r\nX-Long: one\r\n two\r\n\r\n"


def post(n: int, path: bytes = b"/up", more: bytes = b"") -> bytes:
    """a Content-Length POST whose body holds no empty line"""
    body = bytes(0x61 + k % 26 for k in range(n))
    return b"POST " + path + b" HTTP/1.1\r\nHost: upstream\r\n" + more + b"Content-Length: %d\r\n\r\n" % n + body


CHUNKED = b"POST /up HTTP/1.1\r\nHost: c\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n"
CHUNKED_EMPTY = b"POST /up HTTP/1.1\r\nTransfer-Encoding: chunked\r\nTrailer-Less: 1\r\n\r\n0\r\n\r\n"
NO_FRAMING = b"POST /up HTTP/1.1\r\nHost: neither\r\n\r\n"
HEAD = b"HEAD /up HTTP/1.1\r\nHost: upstream\r\n\r\n"
LOWER_HEAD = b"head /up HTTP/1.1\r\nHost: upstream\r\n\r\n"
DROPS = (b"POST /up HTTP/1.1\r\nconnection: close\r\nHost: d\r\nKEEP-ALIVE: timeout=5\r\nUser-Agent: ten-letters\r\n"
         b"Connection: again\r\nX-Custom-Hdr: as long as Content-Type\r\nproxy-connection: keep-alive\r\nte: trailers\r\n"
         b"X-Empty:\r\nUpgrade: h2c\r\nCONTENT-LENGTH: 3\r\nAccept: */*\r\n\r\nabc")
BODY_WITH_EMPTY_LINES = b"one\r\n\r\nGET /up HTTP/1.1\r\nHost: inside-a-body\r\n\r\n\n\ntail"
CL_SPLIT = b"POST /up HTTP/1.1\r\nContent-Length: %d\r\n\r\n" % len(BODY_WITH_EMPTY_LINES) + BODY_WITH_EMPTY_LINES
TOOLONG = b"GET /up HTTP/1.1\r\nX-Big: " + b"v" * 66000 + b"\r\n\r\n"
FOUR = b"GET /up HTTP/1.1\r\nA: 1\r\nB: 2\r\nC: 3\r\nD: 4\r\n\r\n"   # max_headers 4: full
FIVE = b"GET /up HTTP/1.1\r\nA: 1\r\nB: 2\r\nC: 3\r\nD: 4\r\nE: 5\r\n\r\n"   # one too many: -1


def case(name, sessions, names=DROP, extra=VIA, maxh=16):
    return {"name": name, "sessions": tuple(sessions), "names": tuple(names), "extra": extra, "maxh": maxh}


@functools.lru_cache(maxsize=None)
def all_cases():
    return (
        case("gets", [GET, GET * 3, TFB * 5 + GET]),
        case("posts", [post(0), post(1) + post(300), post(300) + GET + post(0) + post(1)]),
        case("chunked", [CHUNKED, GET + CHUNKED + GET, CHUNKED_EMPTY + NO_FRAMING + CHUNKED]),
        case("heads", [HEAD, GET + HEAD + LOWER_HEAD + HEAD, LOWER_HEAD, GET, HEAD + HEAD]),
        case("drops", [DROPS, DROPS + GET + DROPS]),
        case("no_names", [DROPS + TFB], names=()),
        case("full", [TFB * 2 + FOUR, TFB + FIVE + TFB, FOUR + TFB], maxh=4),
        case("stops", [GET * 2 + PARTIAL, GET + post(5) + BAD + GET, GET + TOOLONG + GET, BAD, PARTIAL, b""]),
        case("mixed", [GET + STATIC + NOWHERE + GET + HOST + post(7) + FOLD + GET, STATIC, HOST + GET]),
        case("unused", [CL_SPLIT + GET, GET, CL_SPLIT * 2, GET * 2]),
        case("extra_empty", [GET + post(2), HEAD], extra=b""),
        case("extra_128", [GET + post(2), HEAD + post(300)], extra=EXTRA_128),
    )


CASE_NAMES = tuple(c["name"] for c in all_cases())


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


@functools.lru_cache(maxsize=None)
def packed(name):
    """(buf, off, sessions) of a case, built once; the tests only read them"""
    buf, off, sess, _ = rhp.pack_sessions(list(by_name(name)["sessions"]))
    return buf, off, sess


@functools.lru_cache(maxsize=None)
def host_round(name, layout=rhp.LAYOUT_REQUEST_MAJOR):
    """the case parsed, fixed up and classified on the host: (Result, session results, req_start, route), shared
    between the tests, which only read them"""
    return host_round_of(*packed(name), by_name(name)["maxh"], layout)


def host_round_of(buf, off, sess, maxh, layout=rhp.LAYOUT_REQUEST_MAJOR):
    res, results, starts = rhp.fixup_cpu(buf, off, sess, maxh, layout=layout)
    _, route = rhp.classify_sessions_cpu(res, sess, results, starts, (), ROUTES)
    return res, results, starts, route


def forward_cpu(name, layout=rhp.LAYOUT_REQUEST_MAJOR, out_size=None):
    c = by_name(name)
    res, results, starts, route = host_round(name, layout)
    return rhp.forward_sessions_cpu(res, packed(name)[2], results, starts, route, len(ROUTES), FORWARD_MASK, c["names"], c["extra"],
                                    out_size=out_size)


def forward_gpu(name, layout=rhp.LAYOUT_REQUEST_MAJOR, **kw):
    c = by_name(name)
    buf, off, sess = packed(name)
    return rhp.forward_sessions_gpu(buf, off, sess, ROUTES, FORWARD_MASK, c["names"], c["extra"], c["maxh"], layout=layout, **kw)


_golden = None


def golden():
    global _golden
    if _golden is None:
        assert os.path.exists(GOLDEN), f"{GOLDEN} is missing (tests/golden/make_golden_forward.py writes it)"
        _golden = dict(np.load(GOLDEN))
    return _golden


def expected(name):
    """(why u8 [n], size u32 [n], out u8, fwd_off u32 [n_sessions + 1], head_bits u32) of a case, from the file"""
    g = golden()
    k = list(g["case_name"]).index(name)
    s0, s1 = (int(v) for v in g["case_slot"][k: k + 2])
    b0, b1 = (int(v) for v in g["case_byte"][k: k + 2])
    f0, f1 = (int(v) for v in g["case_sess"][k: k + 2])
    w0, w1 = (int(v) for v in g["case_word"][k: k + 2])
    return g["why"][s0:s1], g["size"][s0:s1], g["out"][b0:b1], g["fwd_off"][f0:f1], g["head_bits"][w0:w1]


def same_as_expected(got, want, label):
    """a forward_sessions_* result against expected()"""
    out_off, why, out, fwd_off, head_bits = got
    w_why, w_size, w_out, w_fwd, w_bits = want
    assert (why == w_why).all(), f"{label}: why {why.tolist()} != {w_why.tolist()}"
    assert (np.diff(out_off) == w_size).all() and int(out_off[0]) == 0, f"{label}: sizes {np.diff(out_off).tolist()} != {w_size.tolist()}"
    assert out is not None and bytes(out) == bytes(w_out), f"{label}: the forwarded bytes differ"
    assert (fwd_off == w_fwd).all(), f"{label}: fwd_off {fwd_off.tolist()} != {w_fwd.tolist()}"
    assert (head_bits == w_bits).all(), f"{label}: head_bits {head_bits.tolist()} != {w_bits.tolist()}"
