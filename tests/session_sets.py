"""The "session shapes" set of the fix-up tests (tests/test_sessions.py): sessions
built by hand around the steps of rhp_fixup_kernel's wave-parallel prefix (64
pieces per step, rhp_scalar.h kFixupStep) and the hand-over to lane 0's walk.

A session is LEAD whole pieces, one STOPPER at piece LEAD, and TAIL more whole
pieces.  A whole piece is one the prefix takes as it is: a request that ends
exactly at its piece's end with no chunked body to de-frame; the four kinds of
WHOLE cycle, starting at another kind in every session.  The sessions are cut
at true request boundaries where a kind says so (a Content-Length body stays
in its request's piece), which the server's empty-line split would not do:
pack() hands rhp.pack_sessions the piece lengths."""
from __future__ import annotations

import functools

import libreactorng_amd as rhp

TFB = (b"GET /plaintext HTTP/1.1\r\nHost: tfb-server:8080\r\nAccept: text/plain\r\n"
       b"Connection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n\r\n")   # exactly 4 headers
TFB_HEADERS = 4
WHOLE = (TFB,
         b"GET /lf HTTP/1.1\nX: y\n\n",
         b"PUT /zero HTTP/1.1\r\nContent-Length: 0\r\n\r\n",
         b"POST /cl HTTP/1.1\r\nContent-Length: 6\r\n\r\nhe\n\nlo")   # one piece: cut at the request's true end

# around one, two and three steps of the prefix, and a fourth step's middle
LEADS = (64, 63, 65, 0, 1, 127, 128, 129, 200)
TAILS = (1, 0, 70)

CHUNKED = b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n"
_BODY = b"line one\r\n\r\nGET /inside-a-body HTTP/1.1\r\nHost: x\r\n\r\n\n\ntail"
CL_SPLIT = b"POST /cl-empty-lines HTTP/1.1\r\nContent-Length: %d\r\n\r\n" % len(_BODY) + _BODY
PARTIAL = b"GET /last HTTP/1.1\r\nHost:"
BAD = b"GET /x HTTP/1.1\r\nBad Header\r\n\r\n"
TWO = TFB + b"GET / HTTP/1.1\r\nHost: a\r\n\r\n"

# name -> the stopper's pieces, as (bytes, piece lengths)
STOPPERS = {
    "none": (b"", []),                                   # the session ends: the prefix takes it whole
    "chunked": (CHUNKED, [len(CHUNKED)]),                # result 1, RHP_BODY_CHUNKED_PENDING: lane 0 de-frames it
    "cl_split": (CL_SPLIT, rhp.split_pieces(CL_SPLIT)),  # cut at its empty lines: the body runs into the next pieces
    "partial": (PARTIAL, [len(PARTIAL)]),                # result 0
    "bad": (BAD, [len(BAD)]),                            # result -1
    "two": (TWO, [len(TWO), 0]),                         # two requests in one piece (consumed < piece length), and
    #                                                      an empty piece, so that the session has a slot per request
    "empty_piece": (b"", [0]),                           # a zero-length piece between two requests
}


def session(lead, stopper, tail, phase=0):
    """(bytes, piece lengths) of one session"""
    data, lens = [], []
    for i in range(lead):
        w = WHOLE[(phase + i) % len(WHOLE)]
        data.append(w)
        lens.append(len(w))
    sd, sl = STOPPERS[stopper]
    data.append(sd)
    lens += sl
    for i in range(tail):
        w = WHOLE[(phase + lead + 1 + i) % len(WHOLE)]
        data.append(w)
        lens.append(len(w))
    return b"".join(data), lens


@functools.lru_cache(maxsize=None)
def shapes():
    """[(lead, stopper, tail, bytes, piece lengths)]: TAILS x LEADS x STOPPERS,
    the stopper changing fastest (the four sessions of a workgroup take
    different paths), plus an empty session (no piece: lead None, third) and a
    session that is one empty piece (lead None, sixth).  The first session is
    taken whole in two steps."""
    out = []
    for tail in TAILS:
        for lead in LEADS:
            for stopper in STOPPERS:
                out.append((lead, stopper, tail) + session(lead, stopper, tail, phase=len(out)))
    out.insert(2, (None, "no_piece", 0, b"", []))
    out.insert(5, (None, "one_empty_piece", 0, b"", [0]))
    return tuple(out)


def pack(sessions):
    """rhp.pack_sessions of (.., bytes, piece lengths) sessions at their own cuts"""
    lens = iter([s[-1] for s in sessions])
    return rhp.pack_sessions([s[-2] for s in sessions], split=lambda data: list(next(lens)))


@functools.lru_cache(maxsize=None)
def packed_shapes(first=None):
    """(buf, off, sessions) of shapes(), or of its first `first` sessions (the
    bytes end after their last piece, padded as every batch).  Shared between
    the tests, which only read them (the parsers work on copies)."""
    buf, off, sess, _ = pack(shapes()[:first])
    return buf, off, sess
