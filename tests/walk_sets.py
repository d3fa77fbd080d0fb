"""The inputs of the rhp_walk_responses tests (tests/test_walk_responses.py): sessions of pipelined responses
whose heads, framing headers and bodies sit where the walk can go wrong, built here from fixed text.
tests/golden/make_golden_walk.py runs the compiled reference over them, message after message, and writes
tests/golden/walk_responses.npz, which holds the bytes too: the tests read that file, and one CPU test holds it to
what this module builds.

A set is one call: (name, max_headers, flags, [session bytes], [slots per session]).  Its buffer is the sessions
back to back and RHP_PAD zero bytes: what lies behind a session is its neighbour, as rhp.h says.
"""
import numpy as np

RHP_PAD = 256
TRAILERS, DEFRAME, NONE_EMPTY = 1, 2, 4   # RHP_WALK_* (rhp.h)
GEOMETRY = (1, 63, 64, 65, 257)           # n_sessions: the wave's and the block's edges


def resp(lines=(), body=b"", status=b"HTTP/1.1 200 OK", eol=b"\r\n"):
    """a response: the status line, the header lines `lines` (no line end), the empty line and `body`"""
    return status + eol + b"".join(x + eol for x in lines) + eol + body


def chunked(parts, trailers=(), ext=b"", eol=b"\r\n"):
    """a chunked body: one chunk per part, the last chunk, the trailer lines, the empty line"""
    return (b"".join(b"%x" % len(p) + ext + eol + p + eol for p in parts) + b"0" + eol +
            b"".join(t + eol for t in trailers) + eol)


def length(body, extra=()):
    return resp([b"Content-Length: %d" % len(body)] + list(extra), body)


def te(parts, trailers=(), **kw):
    return resp([b"Transfer-Encoding: chunked"], chunked(parts, trailers, **kw))


HELLO = length(b"hello, world")
CHUNKS = te([b"first chunk", b"x" * 33, b"y"])
CHUNKS_T = te([b"0123456789abcdef" * 3, b"tail"], [b"X-Checksum: 77", b"X-More: yes"])
NO_CONTENT = resp(status=b"HTTP/1.1 204 No Content")
NOT_MODIFIED = resp([b"ETag: \"v1\""], status=b"HTTP/1.1 304 Not Modified")
SWITCHING = resp([b"Upgrade: websocket", b"Connection: Upgrade"], status=b"HTTP/1.1 101 Switching Protocols")
BARE = resp([b"Server: bare"])   # a 200 with no framing header
SHORT = resp([b"Content-Length: 0"])


def pack(sessions):
    """(bytes u8 with RHP_PAD zero bytes behind the last session, sess_off u64 [n + 1])"""
    off = np.zeros(len(sessions) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in sessions])
    buf = np.zeros(int(off[-1]) + RHP_PAD, dtype=np.uint8)
    buf[: int(off[-1])] = np.frombuffer(b"".join(sessions), dtype=np.uint8)
    return buf, off


def slot_offsets(slots):
    off = np.zeros(len(slots) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(slots)
    return off


def _stops():
    """one session per stop code, an empty one between full ones, one whose slots run out"""
    s = [HELLO + CHUNKS_T + SHORT,                        # END
         HELLO + SHORT[:20],                              # HEAD
         b"",                                             # empty: END, no slot
         HELLO + b"HTTP/2.0 200 OK\r\n\r\n" + HELLO,      # BAD: the third message is never looked at
         SHORT + length(b"0123456789")[:-1],              # BODY: one byte short
         SHORT + BARE + b"whatever follows",              # CLOSE
         HELLO + SHORT + NO_CONTENT,                      # MORE: two slots for three messages
         HELLO,                                           # MORE with no slot at all
         SHORT + SHORT]                                   # END with slots to spare
    return s, [6, 6, 3, 6, 6, 6, 2, 0, 5]


def _kinds():
    """the body kinds mixed in one session; the same sessions run under every value of the two walk flags"""
    s = [HELLO + CHUNKS_T + NO_CONTENT + CHUNKS + NOT_MODIFIED + HELLO,
         SWITCHING + CHUNKS + HELLO,
         CHUNKS_T + SHORT,
         HELLO + BARE + HELLO,                            # NONE on 200 in the middle: CLOSE, or empty with NONE_EMPTY
         NO_CONTENT + BARE,                               # ... at the end
         length(b"exactly") + length(b"0123456789")[:-1],   # LENGTH exact, then one byte short
         te([b"abc"], eol=b"\n") + SHORT,                 # bare-LF chunk lines
         te([b"abc", b"de"], ext=b";name=value") + SHORT,   # chunk extensions
         te([b"partial chunk data"])[:-9],                # a chunked body that has not arrived in full
         te([b"z" * 200], [b"T: 1"])]
    return s, [6] * len(s)


def _framing():
    bad_size = resp([b"Transfer-Encoding: chunked"], b"zz\r\nabc\r\n0\r\n\r\n")
    hex17 = resp([b"Transfer-Encoding: chunked"], b"00000000000000003\r\nabc\r\n0\r\n\r\n")
    hex16 = resp([b"Transfer-Encoding: chunked"], b"0000000000000003\r\nabc\r\n0\r\n\r\n")
    s = [resp([b"Content-Length: 5"], status=b"HTTP/1.1 304 Not Modified") + HELLO,   # 304 with a Content-Length: no body
         resp([b"Transfer-Encoding: chunked"], status=b"HTTP/1.1 204 No Content") + SHORT,
         resp([b"Content-Length: 3"], status=b"HTTP/1.1 100 Continue") + HELLO,
         resp([b"Content-Length: 3"], b"abc", status=b"HTTP/1.1 199 Odd") + HELLO,       # (the body bytes are the next head: BAD)
         resp([b"Content-Length: 3"], b"abc", status=b"HTTP/1.1 205 Reset Content") + HELLO,   # 205 is not in the rule
         SHORT + resp([b"Content-Length: 3", b"Transfer-Encoding: chunked"], b"abc") + HELLO,   # CL + TE
         SHORT + resp([b"Transfer-Encoding: gzip"], b"abc") + HELLO,                    # TE that is not chunked
         SHORT + bad_size + HELLO,
         SHORT + hex17 + HELLO,
         hex16 + HELLO,
         SHORT + resp([b"Content-Length: -1"], b"abc"),                                 # strtoull: 2^64 - 1, a BODY stop
         resp([b"Content-Length: 18446744073709551616"], b"abc"),
         resp([b"Content-Length:", b"Content-Length: 3"], b"abc"),                      # first match only: absent, CLOSE
         resp([b"content-length: 3", b"Content-Length: 1"], b"abc") + SHORT,
         resp([b"TRANSFER-ENCODING: CHUNKED"], chunked([b"q"])) + SHORT,
         resp([b"Transfer-Encoding: chunked"], b"3\r\nabcXX0\r\n\r\n") + SHORT,         # no CRLF behind the chunk data
         resp([b"Transfer-Encoding: chunked"], b"3\r\nabc\r\r\r\n0\r\n\r\n") + SHORT]   # a run of CRs before the LF
    return s, [4] * len(s)


def _split():
    """a head cut at every byte of a short message, behind a whole one"""
    s = [SHORT + SHORT[:k] for k in range(1, len(SHORT))]
    return s, [2] * len(s)


def _heads():
    fold = resp([b"Content-Length: 5", b"X-Long: a", b" folded", b"\tagain"], b"hello")
    fold_cl = resp([b"X-A: b", b" Content-Length: 5"], b"hello")   # the name inside an obs-fold line: no header
    s = [resp([b"Content-Length: 5"], b"hello", eol=b"\n") + resp([b"Server: x"], status=b"HTTP/1.0 204 Gone", eol=b"\n") + HELLO,
         fold + fold + SHORT,
         fold_cl + SHORT,
         resp([b"Content-Length: 2"], b"ok", status=b"HTTP/1.1    200    fine  ") + SHORT,
         resp([b"Content-Length: 2"], b"ok", status=b"HTTP/1.1 200") + SHORT,
         b"\r\n" + SHORT,                                 # a leading CRLF is not skipped
         SHORT + b"\r\n" + SHORT,
         SHORT + resp([b"Bad Name: x"]) + SHORT,
         SHORT + resp([b"A: b"], status=b"HTTP/1.1 20") + SHORT]
    return s, [4] * len(s)


def _capacity(maxh):
    """exactly max_headers lines fit; one more is BAD.  The framing header is the last that fits."""
    fill = [b"H%d: v%d" % (i, i) for i in range(maxh)]
    full = resp(fill[:-1] + [b"Content-Length: 2"], b"ok") if maxh else NO_CONTENT
    s = [full + full + resp(fill + [b"Content-Length: 2"], b"ok") + full,
         full + resp(fill, status=b"HTTP/1.1 204 No Content") + full,
         resp(fill) + full]                               # no framing header: CLOSE
    return s, [5] * len(s)


def _sp_run():
    """the SP run behind the version has no end test: it reads the next session's bytes, and the pad"""
    s = [SHORT + b"HTTP/1.1 ", b"   200 OK\r\n\r\n",
         SHORT + b"HTTP/1.1  ", b" 204 No\r\nA: b\r\n\r\n",
         b"HTTP/1.1 ", b"", b"  ",
         SHORT + b"HTTP/1.1   "]                          # into the pad
    return s, [3] * len(s)


def _residues():
    """17 sessions of 1 mod 16 bytes: the session starts go through every residue mod 16"""
    out = []
    for k in range(17):
        base = HELLO + te([b"r%02d" % k, b"w" * (k + 1)], [b"T: %d" % k]) + NO_CONTENT
        head = lambda pad: resp([b"X-Pad: " + b"p" * pad], status=b"HTTP/1.1 204 No Content")
        out.append(head((1 - len(base) - len(head(0))) % 16) + base)
        assert len(out[-1]) % 16 == 1
    return out, [5] * len(out)


def pool():
    """the sessions the geometry sets and the random mix cycle through: every answer, short"""
    s = []
    for f in (_stops, _kinds, _framing, _heads):
        s += [(a, b) for a, b in zip(*f())]
    return s


def geometry(n):
    p = pool()
    pick = [p[(i * 7 + i // 11) % len(p)] for i in range(n)]
    return [a for a, _ in pick], [b for _, b in pick]


def all_sets():
    sets = []
    add = lambda name, maxh, flags, sb: sets.append((name, maxh, flags, list(sb[0]), list(sb[1])))
    add("stops", 8, TRAILERS, _stops())
    for flags in (0, TRAILERS, NONE_EMPTY, TRAILERS | NONE_EMPTY):
        add(f"kinds_f{flags}", 8, flags, _kinds())
    add("framing", 8, TRAILERS, _framing())
    add("framing_f0", 8, 0, _framing())
    add("split", 4, TRAILERS, _split())
    add("heads", 8, TRAILERS, _heads())
    add("max0", 0, TRAILERS, _capacity(0))
    add("max2", 2, TRAILERS, _capacity(2))
    add("sp_run", 4, TRAILERS, _sp_run())
    add("residues", 4, TRAILERS, _residues())
    for n in GEOMETRY:
        add(f"n{n}", 8, TRAILERS | (NONE_EMPTY if n & 1 else 0), geometry(n))
    return sets
