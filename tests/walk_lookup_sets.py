"""The inputs of the rhp_lookup_walked tests (tests/test_walk_lookup.py): every set of tests/walk_sets.py and every
chain of tests/walk_resume_sets.py looked up with one fixed list of sixteen names, and sets of this module's own whose
header lines sit where the lookup can go wrong, each with names of its own.  tests/golden/make_golden_walk_lookup.py
walks them over the compiled reference, looks every head up with its http_field_lookup and writes
tests/golden/walk_lookup.npz, which holds the bytes and the names too: the tests read that file, and one CPU test
holds it to what this module builds.

A set is a chain of calls over the same sessions:
  (name, max_headers, flags, resume, deliveries, caps, states, names)
  resume       False: one rhp_walk_responses call (deliveries and caps hold one round); True: rhp_walk_resume rounds,
               as walk_resume_sets
  names        the lookup names, bytes each
"""
import walk_resume_sets as wr
import walk_sets as ws
from walk_sets import TRAILERS, resp, SHORT, HELLO

NAME64 = b"X-Sixty-Four-" + b"n" * 51          # the longest name a call takes
NAME65 = b"X-Sixty-Five-" + b"m" * 52          # one byte longer: no call can name it
assert len(NAME64) == 64 and len(NAME65) == 65

# the names every set of walk_sets.py and walk_resume_sets.py is looked up with, all sixteen at once
FIXED_NAMES = (b"Content-Length", b"Transfer-Encoding", b"Connection", b"X-No-Message-Has-This", NAME64, b"server", b"ETAG",
               b"Upgrade", b"X-Pad", b"X-Long", b"X-A", b"H0", b"h1", b"T", b"cOnTeNt-LeNgTh", b"X-Checksum")
assert len(FIXED_NAMES) == 16


def _dup():
    s = [resp([b"Set-Cookie: a=1", b"Set-Cookie: b=2", b"Content-Length: 0"]) +
         resp([b"X-Empty:", b"X-Empty: later", b"set-cookie: c=3", b"Content-Length: 0"]),
         resp([b"X-Empty:   \t ", b"Content-Length: 0", b"X-EMPTY: again"])]   # only OWS: empty too
    return s, [3, 2], (b"Set-Cookie", b"X-Empty", b"Content-Length")


def _fold():
    """an obs-fold line (a record with name == NULL) between the matches: skipped, and never a match itself"""
    s = [resp([b"X-A: 1", b" X-B: folded", b"X-B: 2", b"\tX-A: folded", b"X-A: 3", b"Content-Length: 0"]) + SHORT,
         resp([b"X-B: first", b"  ", b"X-A: behind", b"Content-Length: 0"])]
    return s, [3, 2], (b"X-B", b"X-A", b"Content-Length", b" X-B")


def _fold_edges():
    """names of equal length that differ from a header's only in a byte beside the fold's range: a..z and A..Z are
    the same, no other pair is -- ^ and ~ (and >), _ and DEL, ` and @, | and backslash, and a letter with bit 7 set"""
    heads = [b"X~Edge: tilde", b"X_Edge: under", b"X`Edge: tick", b"XaEdge: letter", b"X|Edge: bar"]
    s = [resp(heads + [b"Content-Length: 0"]) + resp([b"X^Edge: caret", b"xZeDGE: zed", b"Content-Length: 0"]),
         resp([b"XzEdge: zed", b"Content-Length: 0"])]
    names = (b"X^Edge", b"X\x7fEdge", b"X@Edge", b"X\xe1Edge", b"X\xc1Edge", b"X\\Edge", b"X>Edge", b"x~edge", b"x_EDGE",
             b"x`edge", b"xAedge", b"X|EDGE", b"X^EDGE", b"XZEDGE", b"X\xfaEdge", b"X\x1aEdge")
    assert len(names) == 16 and all(len(x) == 6 for x in names)
    return s, [3, 2], names


def _len64():
    s = [resp([NAME64 + b": sixty-four", NAME65 + b": sixty-five", b"Content-Length: 0"]) +
         resp([NAME65 + b": sixty-five", NAME64.upper() + b": again", b"Content-Length: 0"])]
    return s, [3], (NAME64.lower(), NAME65[:64], NAME65[1:], NAME64[:63] + b"N", NAME64[:63] + b"x")


def _starts():
    """one session of 33 responses of 1 mod 16 bytes: the heads start at every residue mod 16, twice, and the
    names' first bytes land on every residue mod 4"""
    one = lambda k: resp([b"X-Pad: " + b"p" * pad, b"Content-Length: 0", b"X-K: %d" % k])
    out = b""
    for k in range(33):
        pad = 0
        m = one(k)
        pad = (1 - len(m)) % 16
        m = one(k)
        assert len(m) % 16 == 1
        out += m
    return [out, SHORT], [34, 1], (b"X-K", b"X-Pad", b"Content-Length")


def _more():
    """a session whose slots ran out, sessions that left slots unwritten behind it, one with no slot at all"""
    s = [SHORT * 5, HELLO, SHORT * 2, b"", HELLO + SHORT[:9], SHORT]
    return s, [2, 4, 0, 3, 4, 1], (b"Content-Length", b"Connection")


def _continuation():
    """round 1 starts inside a Content-Length body: a continuation slot, then heads"""
    L10 = resp([b"Connection: keep-alive", b"Content-Length: 10"])
    close = resp([b"Connection: close", b"Content-Length: 0"])
    te = resp([b"Transfer-Encoding: chunked", b"Connection: Upgrade"])
    rows = [((L10 + b"01234", b"56789" + close + SHORT), (3, 3)),
            ((te + b"3\r\nab", b"c\r\n0\r\n\r\n" + close), (3, 2)),
            ((close, close), (2, 2)),
            ((L10 + b"01234", b"567"), (1, 1))]                      # still inside: the round's only slot is a continuation
    deliveries = [[r[0][k] for r in rows] for k in range(2)]
    caps = [[r[1][k] for r in rows] for k in range(2)]
    return deliveries, caps, (b"Connection", b"Content-Length", b"Transfer-Encoding")


def all_sets():
    sets = []
    for name, maxh, flags, sessions, nslots in ws.all_sets():
        sets.append((name, maxh, flags, False, [sessions], [nslots], None, FIXED_NAMES))
    for name, maxh, flags, deliveries, caps, states in wr.all_sets():
        sets.append(("resume_" + name, maxh, flags, True, deliveries, caps, states, FIXED_NAMES))
    for name, f in (("dup", _dup), ("fold", _fold), ("fold_edges", _fold_edges), ("len64", _len64), ("starts", _starts), ("more", _more)):
        sessions, nslots, names = f()
        sets.append((name, 8, TRAILERS, False, [sessions], [nslots], None, names))
    d, c, names = _continuation()
    sets.append(("continuation", 8, TRAILERS, True, d, c, None, names))
    return sets
