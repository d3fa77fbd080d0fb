"""The inputs of the rhp_frame_messages tests (tests/test_frame_messages.py): batches of responses and of bare
header blocks whose framing headers sit where the lookup, the number parse and the `chunked` compare can go
wrong, built here from fixed text and a fixed seed.  tests/golden/make_golden_frame_messages.py runs the compiled
reference over them and writes tests/golden/frame_messages.npz, which holds the bytes and the lookup names too:
the tests read that file, and one CPU test holds it to what this module builds.

A set is one batch: (name, kind, max_headers, [message bytes], [lookup names]).  A message may carry body bytes
behind its header section; its buffer is message_sets.pack's (back to back, RHP_PAD zero bytes behind).
"""
import numpy as np

import message_sets as ms
from message_sets import HEADERS, RESPONSE, RHP_MAX_LEN, STATUS, pack  # noqa: F401  (pack: the tests' packer)

NAMES = [b"Content-Type", b"Connection"]   # the lookup names of most sets
CL, TE = b"Content-Length", b"Transfer-Encoding"
BATCH_SIZES = (1, 63, 64, 65, 255, 256, 257)
CAPACITIES = (0, 1, 16, 64)

CL_VALUES = [b"0", b"1", b"18446744073709551615", b"18446744073709551616", b"-1", b"+5", b"12abc", b"abc",
             b"0" * 40 + b"7",                       # crosses the 24-byte window
             b"0" * 23 + b"9", b"0" * 24 + b"9",     # the window's last byte and the first behind it
             b"1" * 24 + b"x9", b"99999999999999999999999999", b"-18446744073709551615", b"-", b"+", b"-0", b"4294967296",
             b"5 6", b"7\t", b"08"]
TE_VALUES = [b"chunked", b"Chunked", b"CHUNKED", b"cHuNkEd", b"chunke", b"chunkedx", b"gzip, chunked", b"identity",
             b"chunkeD", b"xhunked", b"chunke\xc4", b"CHUNKE\x64", b"c", b"chunked, gzip"]


def msg(kind, lines, eol=b"\r\n", body=b""):
    """a message of `kind` with the header lines `lines` (no line end), the empty line and `body` behind it"""
    return (STATUS if kind == RESPONSE else b"") + b"".join(x + eol for x in lines) + eol + body


def _shapes(kind):
    """one message per answer: the pool the geometry sets cycle through"""
    ct = b"Content-Type: text/plain"
    return [msg(kind, [ct, CL + b": 5"], body=b"hello"),
            msg(kind, [TE + b": chunked", b"Connection: close"], body=b"5\r\nhello\r\n0\r\n\r\n"),
            msg(kind, [b"Server: x"]),
            b"",                                                             # -2
            msg(kind, [b"connection: keep-alive", b"content-length: 300"]),  # the body has not arrived
            msg(kind, [CL + b": 3", TE + b": chunked"]),                     # both: -1
            msg(kind, [b"Bad Name: x"]),                                     # ret -1
            msg(kind, [b"TRANSFER-ENCODING: gzip", ct]),                     # not chunked: -1
            msg(kind, [b"X-A: 1", b"X-B: 2", b"X-C: 3", b"CONTENT-TYPE: a", b"CONNECTION: b", b"transfer-encoding: CHUNKED"], b"\n"),
            msg(kind, [CL + b": 12"])[:-3]]                                  # -2


def _placement(kind):
    out = []
    for name, value in ((CL, b"17"), (TE, b"chunked")):
        other = [b"H%d: v%d" % (i, i) for i in range(4)]
        for spell in (name, name.lower(), name.upper(), name.swapcase(), name[:5].upper() + name[5:].lower()):
            out.append(msg(kind, [spell + b": " + value] + other))           # record 0
            out.append(msg(kind, other + [spell + b": " + value]))           # the last record
        for shift in range(4):   # the name's first byte at each alignment; the next message's start moves with it
            out.append(msg(kind, [b"P: " + b"p" * shift, name + b": " + value]))
            out.append(msg(kind, [b"P: " + b"p" * shift, name + b":" + b" " * shift + value, b"Connection: x"]))
        out.append(msg(kind, [name + b":", name + b": " + value]))           # first empty, then set: absent
        out.append(msg(kind, [name + b":   \t", name + b": " + value]))      # (a value of OWS only is empty)
        out.append(msg(kind, [name + b": " + value, name + b": 99"]))        # first set, then another
        out.append(msg(kind, [name + b": " + value, name + b":"]))
        out.append(msg(kind, [name + b": " + value, b" folded", b"\tagain"]))   # obs-fold lines behind it
        out.append(msg(kind, [b"A: b", b" " + name + b": " + value]))        # the name inside an obs-fold line: no header
    return out


PLACEMENT_PER_NAME, PLACEMENT_ABSENT = 24, (18, 19, 23)   # per framing name: the messages, and those whose header is absent


def _near(kind):
    out = []
    for name, value in ((CL, b"5"), (TE, b"chunked")):
        for k in range(len(name)):   # equal length, one byte different
            if name[k:k + 1].isalpha():
                out.append(msg(kind, [name[:k] + b"x" + name[k + 1:] + b": " + value]))
        out.append(msg(kind, [name.replace(b"-", b"_") + b": " + value]))
        out.append(msg(kind, [name.replace(b"-", b"^") + b": " + value]))
    for nm in (b"Content-Lengt", b"Content-Lengthh", b"Content-Lengthhh", b"Content-Length-X-", b"Transfer-Encodin",
               b"Transfer-Encodingg", b"ransfer-Encoding", b"Transfer-Encod", b"Content-Length-Tr"):   # 13 .. 18 bytes
        out.append(msg(kind, [nm + b": 5"]))
    # the 0x20 pairs no toupper joins, against NEAR_NAMES: what a header spells / what is looked up
    for nm in NEAR_PAIRS:
        out.append(msg(kind, [nm + b": v", CL + b": 1"]))
    return out


NEAR_PAIRS = (b"A~B", b"A^B", b"A`B", b"A_B", b"a~b", b"A|B")   # header names ('@', DEL and '\\' are no token bytes)
NEAR_NAMES = [b"A^B", b"A~B", b"A@B", b"A`B", b"A\x7fB", b"A_B", b"a|b", b"A\x5cB", b"Content-Length", b"transfer-encoding",
              b"Content-Lengtx", b"Transfer-Encodinx"]


def _values(kind):
    out = [msg(kind, [CL + b": " + v]) for v in CL_VALUES]
    out += [msg(kind, [CL + b": " + v], b"\n") for v in CL_VALUES[:9]]
    for shift in range(4):   # a value at each alignment, short and past the window
        out.append(msg(kind, [b"P:" + b"p" * shift, CL + b": 1234567"]))
        out.append(msg(kind, [b"P:" + b"p" * shift, CL + b": " + b"0" * 30 + b"12345678901234567890123"]))
    out += [msg(kind, [CL + b": 5"], body=b"hello"), msg(kind, [CL + b": 5"], body=b"hell"),
            msg(kind, [CL + b": 5"], body=b"hello, world"), msg(kind, [CL + b": -1"], body=b"x")]
    out += [msg(kind, [TE + b": " + v]) for v in TE_VALUES]
    for shift in range(4):
        out.append(msg(kind, [b"P:" + b"p" * shift, TE + b": chunked"]))
        out.append(msg(kind, [b"P:" + b"p" * shift, TE + b": chunkex"]))
    out += [msg(kind, [TE + b": chunked", CL + b": 5"]), msg(kind, [CL + b": 5", TE + b": chunked"]),
            msg(kind, [CL + b": 5", TE + b": gzip"]), msg(kind, [CL + b": abc", TE + b": identity"]),
            msg(kind, [TE + b":", CL + b": 5"]), msg(kind, [CL + b": 5", TE + b":"]),   # empty Transfer-Encoding: absent
            msg(kind, [CL + b":", TE + b": chunked"]), msg(kind, [TE + b": chunked", CL + b":"]),   # empty Content-Length
            msg(kind, [CL + b":", TE + b": gzip"]), msg(kind, [CL + b":", TE + b":"])]
    return out


def _capacity(kind, maxh):
    """exactly max_headers lines with the framing header last and first, and one line more (ret -1)"""
    fill = lambda k: [b"H%d: v%d" % (i, i) for i in range(k)]
    out = []
    for extra in (0, 1):
        k = maxh + extra
        out.append(msg(kind, fill(k)))
        if k:
            out += [msg(kind, fill(k - 1) + [CL + b": 42"]), msg(kind, [TE + b": chunked"] + fill(k - 1)),
                    msg(kind, fill(k - 1) + [b"Connection: close"], b"\n")]
    return out


def _not_ready(kind):
    head = (STATUS if kind == RESPONSE else b"") + CL + b": 7\r\nX-Pad: "
    long_ = lambda ret: head + b"a" * (ret - len(head) - 4) + b"\r\n\r\n"
    tail = (STATUS if kind == RESPONSE else b"") + b"X-Pad: " + b"a" * (RHP_MAX_LEN - 60 - len(STATUS) * (kind == RESPONSE))
    tail += b"\r\n" + CL + b": "
    at_end = tail + b"1" * (RHP_MAX_LEN - len(tail) - 4) + b"\r\n\r\n"   # the value's last byte: the last before the line end
    assert len(long_(RHP_MAX_LEN)) == RHP_MAX_LEN and len(at_end) == RHP_MAX_LEN
    longs = [long_(RHP_MAX_LEN + 1), at_end] if kind == RESPONSE else []   # (once: they are most of the file)
    return [msg(kind, [CL + b": 5"]), msg(kind, [b"Bad Name: x", CL + b": 5"]), msg(kind, [CL + b": 5"])[:-1], b""] + longs + [
            msg(kind, [CL + b"\x01: 5"]), msg(kind, [TE + b": chunked"])[:9], b"\r", b"\n"]


FUZZ_LINES = ([CL + b": " + v for v in CL_VALUES[:12]] + [TE + b": " + v for v in TE_VALUES[:8]] +
              [CL.lower() + b": 10", TE.upper() + b": CHUNKED", CL + b":", TE + b":", b"Content-Lengtx: 5",
               b"Transfer-Encodinx: chunked", b"Content-Type: t", b"connection: c", CL + b" : 5", b" " + CL + b": 5"])


def _fuzz(kind, seed, n):
    """message_sets' fuzz messages with up to three framing lines spliced in behind line ends"""
    rng = np.random.default_rng(seed)
    out = []
    for m in ms._fuzz(kind, seed, n):
        for _ in range(int(rng.integers(0, 4))):
            ends = [i + 1 for i, c in enumerate(m) if c == 10]
            at = ends[int(rng.integers(0, len(ends)))] if ends and rng.integers(0, 8) else int(rng.integers(0, len(m) + 1))
            m = m[:at] + FUZZ_LINES[int(rng.integers(0, len(FUZZ_LINES)))] + (b"\r\n" if rng.integers(0, 4) else b"\n") + m[at:]
        out.append(m)
    return out


def all_sets():
    sets = []
    add = lambda name, kind, maxh, msgs, names=NAMES: sets.append((name, kind, maxh, list(msgs), list(names)))
    for kind, kn in ((RESPONSE, "response"), (HEADERS, "headers")):
        shapes = _shapes(kind)
        for n in BATCH_SIZES:   # launch geometry; the message lengths move every start through the alignments
            add(f"{kn}_n{n}", kind, 16, [shapes[(i * 7 + i // 10) % len(shapes)] for i in range(n)])
        for maxh in CAPACITIES:
            add(f"{kn}_max{maxh}", kind, maxh, _capacity(kind, maxh))
        add(f"{kn}_placement", kind, 16, _placement(kind))
        add(f"{kn}_near", kind, 16, _near(kind), NEAR_NAMES)
        add(f"{kn}_values", kind, 16, _values(kind))
        add(f"{kn}_values_no_names", kind, 4, _values(kind)[:40], [])
        add(f"{kn}_sixteen_names", kind, 16, _placement(kind)[:24],
            [b"H%d" % i for i in range(4)] + [b"P", CL, TE, b"Connection"] + [b"n" * k for k in (1, 13, 14, 15, 16, 17, 18, 64)])
        add(f"{kn}_not_ready", kind, 4, _not_ready(kind))
        add(f"{kn}_fuzz", kind, 8, _fuzz(kind, 20261020 + kind, 1500))
    return sets
