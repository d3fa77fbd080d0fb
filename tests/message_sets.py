"""The inputs of the rhp_parse_messages tests (tests/test_messages.py): batches of responses
(phr_parse_response) and of bare header blocks (phr_parse_headers), built here from fixed text and a fixed
seed.  tests/golden/make_golden_messages.py runs the compiled reference over them and writes
tests/golden/messages.npz, which holds the bytes too: the tests read that file, and one CPU test holds it to
what this module builds.

A set is one batch: (name, kind, max_headers, [message bytes], [last_len] or None).  Its buffer is the messages
back to back and RHP_PAD zero bytes: what lies behind a message is its neighbour, as rhp.h says.
"""
import numpy as np

RESPONSE, HEADERS = 0, 1   # enum rhp_msg_kind
RHP_PAD = 256
RHP_MAX_LEN = 65535

STATUS = b"HTTP/1.1 200 OK\r\n"
VALID = {  # a valid message per kind and line end: every proper prefix of it is -2
    (RESPONSE, "crlf"): b"HTTP/1.1 200 OK\r\nHost: example.com\r\nContent-Length: 12\r\nX-Empty:\r\n folded\r\n\r\n",
    (RESPONSE, "lf"): b"HTTP/1.0 404 Not Found\nServer: x\nA: b \t\n\n",
    (HEADERS, "crlf"): b"Host: example.com\r\nContent-Length: 12\r\nX-Empty:\r\n folded\r\n\r\n",
    (HEADERS, "lf"): b"Server: x\nA: b \t\n\n",
}

STATUS_LINES = [   # RESPONSE only; the answers are the reference's (golden), the comments what rhp.h says
    b"HTTP/1.1 200 OK\r\nA: b\r\n\r\n",
    b"HTTP/1.1 200 OK\nA: b\n\n",                 # bare LF
    b"HTTP/1.1 200\r\n\r\n",                      # no reason phrase
    b"HTTP/1.1 200\n\n",
    b"HTTP/1.1 200   \r\n\r\n",                   # a reason of spaces only
    b"HTTP/1.1    200    OK  go \r\nA: b\r\n\r\n",  # several spaces before the status and the reason
    b"HTTP/1.1 200X\r\n\r\n",                     # -1
    b"HTTP/1.1 20\r\n\r\n",                       # a two-digit status: -1
    b"HTTP/1.1 2\xb00 OK\r\n\r\n",                # a byte above 0x7f where a digit belongs: -1
    b"HTTP/1.0 200 OK\r\n\r\n",
    b"HTTP/1.9 999 OK\r\n\r\n",
    b"HTTP/2.0 200 OK\r\n\r\n",                   # -1
    b"HTTP/1.x 200 OK\r\n\r\n",                   # -1
    b"http/1.1 200 OK\r\n\r\n",                   # -1
    b"HTTP/1.1200 OK\r\n\r\n",                    # no space after the version: -1
    b"HTTP/1.1\t200 OK\r\n\r\n",                  # -1
    b"HTTP/1.1 200 O\x01K\r\n\r\n",               # a control byte in the reason: -1
    b"HTTP/1.1 200 O\x7fK\r\n\r\n",               # DEL: -1
    b"HTTP/1.1 200 O\x00K\r\n\r\n",               # -1
    b"HTTP/1.1 200 O\tK\r\n\r\n",                 # HT is accepted
    b"HTTP/1.1 200 \xc3\xa9t\xe9\r\n\r\n",        # bytes above 0x7f are accepted
    b"HTTP/1.1 200\tOK\r\n\r\n",                  # a reason that does not start with a space: -1
    b"HTTP/1.1 200 OK\r\r\n\r\n",                 # CR not followed by LF: -1
    b"\r\nHTTP/1.1 200 OK\r\n\r\n",               # a leading CRLF is not skipped: -1
    b"\nHTTP/1.1 200 OK\r\n\r\n",
    b"HTTP/1.1 200 OK\r\n\r\nHTTP/1.1 500 Next\r\n\r\n",   # ret stops behind the first message
]


def header_lines(k: int, eol: bytes = b"\r\n") -> bytes:
    return b"".join(b"H%d: v%d" % (i, i) + eol for i in range(k)) + eol


HEADER_SHAPES = [   # header blocks; a RESPONSE set puts STATUS in front
    b"A: b\r\nB: c\r\n\r\n",
    b"A: b\r\n folded line\r\nC: d\r\n\r\n",      # obs-fold on line 2
    b"A: b\r\n\tfolded with HT\r\n\r\n",
    b" A: b\r\n\r\n",                             # OWS at the start of the first line: -1
    b"\tA: b\r\n\r\n",
    b": b\r\n\r\n",                               # an empty name: -1
    b"A: b\r\n: c\r\n\r\n",
    b"A B: c\r\n\r\n",                            # a non-token byte in a name: -1
    b"A(: c\r\n\r\n",
    b"A\x80: c\r\n\r\n",
    b"A\r\n\r\n",                                 # no colon: -1
    b"A: value \t \r\n\r\n",                      # trailing OWS is trimmed
    b"A:    \r\n\r\n",                            # a value of OWS only
    b"A:\r\n\r\n",                                # an empty value
    b"A:\n\n",
    b"A:b\r\nB:\tc\r\n\r\n",                      # no OWS, HT before the value
    b"A: b\x01\r\n\r\n",                          # a control byte in a value: -1
    b"A: b\x7f\r\n\r\n",
    b"A: b\tc\xff\r\n\r\n",
    b"A: b\rX\r\n\r\n",                           # CR not followed by LF: -1
    b"!#$%&'*+-.^_`|~09az: ok\r\n\r\n",           # every kind of token byte
    b"\r\n",                                      # no header at all
    b"\n",
    b"\r\nA: b\r\n\r\n",                          # the empty line comes first
]


def _mutate(rng, m: bytes) -> bytes:
    """a few byte edits of a valid message: the bytes the parser branches on, cuts, doubled and dropped bytes"""
    hot = b" \t\r\n:\x00\x01\x7f\x80\xffHTP/1.209aZ(,"
    b = bytearray(m)
    for _ in range(int(rng.integers(0, 3))):
        op, at = int(rng.integers(0, 8)) % 5, int(rng.integers(0, max(len(b), 1)))   # (a cut is the rarest edit)
        if op == 0 and b:
            b[at] = hot[int(rng.integers(0, len(hot)))]
        elif op == 1:
            b.insert(at, hot[int(rng.integers(0, len(hot)))])
        elif op == 2 and b:
            del b[at]
        elif op == 3:
            del b[at:]
        elif b:
            b[at] = int(rng.integers(0, 256))
    return bytes(b)


def _fuzz(kind: int, seed: int, n: int):
    rng = np.random.default_rng(seed)
    front = [STATUS, b"HTTP/1.0 404  Not Found\n", b"HTTP/1.1 204\r\n"] if kind == RESPONSE else [b""]
    pool = [VALID[(kind, "crlf")], VALID[(kind, "lf")]] + [
        f + header_lines(k, e) for f in front for k in (0, 1, 3, 8) for e in (b"\r\n", b"\n")] + [
        f + b"A: b\r\n folded\r\nLong-Name-Header:   padded value \t\r\n\r\n" for f in front]
    return [_mutate(rng, pool[int(rng.integers(0, len(pool)))]) for _ in range(n)]


def _long(kind: int, ret: int) -> bytes:
    """a message whose header section is exactly `ret` bytes"""
    head = (STATUS if kind == RESPONSE else b"") + b"A: b\r\nX-Pad: "
    return head + b"a" * (ret - len(head) - 4) + b"\r\n\r\n"


def all_sets():
    sets = []
    add = lambda name, kind, maxh, msgs, ll=None: sets.append((name, kind, maxh, list(msgs), ll))
    kinds = ((RESPONSE, "response"), (HEADERS, "headers"))
    add("status_lines", RESPONSE, 4, STATUS_LINES)
    # a message that ends inside the space run, its neighbour starting with spaces and digits: the read past
    # len is defined by the neighbour
    add("space_run", RESPONSE, 4, [b"HTTP/1.1  ", b"  200 OK\r\n\r\n", b"HTTP/1.1 ", b"204 No Content\r\n\r\n",
                                   b"HTTP/1.1 ", b" 20", b"HTTP/1.1 200 OK\r\n\r\n", b"HTTP/1.1 "])
    for kind, kn in kinds:
        front = STATUS if kind == RESPONSE else b""
        for eol in ("crlf", "lf"):
            m = VALID[(kind, eol)]
            add(f"{kn}_prefixes_{eol}", kind, 16, [m[:k] for k in range(len(m))] + [m])
        for maxh in (0, 1, 16):
            shapes = [front + header_lines(k, e) for k in (maxh, maxh + 1) for e in (b"\r\n", b"\n")]
            add(f"{kn}_headers_max{maxh}", kind, maxh, shapes + [front + h for h in HEADER_SHAPES])
        # last_len 1, 2, 3, len - 1 and len on a complete message, an incomplete one, and one whose is_complete
        # answer is -1 (a CR that no LF follows); the same bytes once per value
        whole = VALID[(kind, "crlf")]
        part = whole[:-2]
        bad = front + b"A: b\r\n\rX\r\n\r\n"
        msgs, ll = [], []
        for m in (whole, part, bad, VALID[(kind, "lf")], VALID[(kind, "lf")][:-1]):
            for v in (1, 2, 3, len(m) - 1, len(m), 0):
                msgs.append(m)
                ll.append(v)
        add(f"{kn}_last_len", kind, 16, msgs, ll)
        # ret exactly RHP_MAX_LEN fits, one more is RHP_RET_TOOLONG; both in one wave with 62 short messages
        short = [front + header_lines(i % 4) for i in range(64)]
        short[7], short[40] = _long(kind, RHP_MAX_LEN), _long(kind, RHP_MAX_LEN + 1)
        add(f"{kn}_long", kind, 4, short)
        for n in (1, 63, 64, 65, 257):   # launch geometry; every seventh message is empty (-2)
            add(f"{kn}_n{n}", kind, 4, [b"" if i % 7 == 3 else front + header_lines(i % 5, b"\n" if i % 3 == 0 else b"\r\n")
                                         for i in range(n)])
        fz = _fuzz(kind, 20261020 + kind, 300)
        add(f"{kn}_fuzz", kind, 8, fz)
        rng = np.random.default_rng(77 + kind)
        add(f"{kn}_fuzz_last_len", kind, 8, fz[:150], [int(rng.integers(0, len(m) + 1)) for m in fz[:150]])
    return sets


def pack(msgs):
    """(buf u8 with RHP_PAD zero bytes behind the messages, off u64 [n + 1])"""
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    if msgs:
        off[1:] = np.cumsum([len(m) for m in msgs], dtype=np.uint64)
    buf = np.zeros(int(off[-1]) + RHP_PAD, dtype=np.uint8)
    buf[: int(off[-1])] = np.frombuffer(b"".join(msgs), dtype=np.uint8)
    return buf, off
