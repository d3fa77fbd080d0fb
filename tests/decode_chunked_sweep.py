"""Two sweeps for rhp_decode_chunked (include/rhp.h) whose expected values follow from how the pieces are made, built
without any library; tests/test_decode_chunked_sweep.py holds the host twins, the live reference and the kernel to
them.  They are not in tests/golden/decode_chunked.npz: the move sweep alone is tens of MB.

A Piece is one call.  It is put together from parts the builder knows -- (FRAME, bytes) that the decoder consumes,
(RUN, bytes) chunk data, (REST, bytes) what the call leaves unread, always last -- and carries the decoder before
the call, the expected ret and the decoder after it.  Everything else is derived (Piece.__post_init__): with `orig`
the parts joined, D the data runs joined and src = len(orig) - len(rest),
    size   len(D)
    after  ret == -2:            D + orig[len(D):]
           ret >= 0, ret == -1:  D + orig[src:] + orig[len(D) + len(orig) - src:]
which is picohttpparser's closing move with everything behind it untouched.  consume_trailer and the five reserved
bytes are consumed by no call and go through as they came; some streams give them non-zero values.  A stream is a
list of Pieces, the decoder before a later one the decoder after the one in front of it; a sweep is a list of
streams whose pieces, in order, are one batch packed back to back.  Data bytes are slices of one seeded pool of
random bytes (periodic in no gap: a byte read after it was overwritten differs from the right one).

move_sweep()    one piece per (g, o, n): a size line of exactly g bytes, one chunk of n data bytes, CR LF 0 CR LF and
                five leftover bytes, the piece starting at o mod 16 of a 16-aligned batch (a filler piece 'z' * f in
                front where needed: -1 at once, nothing moved).  The first move is n bytes down by g onto a
                destination at o mod 16; the closing move follows.  g = 1 is a decoder left in IN_CHUNK_EXT with n
                bytes to come and a piece that starts with the LF; a line shorter than its digits plus LF has the
                first digits carried in the decoder; longer lines are padded with a chunk extension.
                The form kept is the full one, every n at every g and o (60 016 pieces, 71 MB): built and compared
                in a second or two on the host, a fraction of a second on the device, so nothing is thinned.
window_sweep()  for each of the five scanning states, each lane k of the 64-byte window at which the state is entered
                and each distance d from there to the byte that decides the scan (distances(k), digit_counts(k)):
                complete (the deciding byte is there and the body goes on to its end with leftover bytes), cut (the
                piece ends just before the deciding byte: -2 with the state carried mid-token; a second piece
                finishes it), and wrong where the state has such a byte (-1 and the closing move).  entry(state, k)
                says how lane k is reached.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

SIZE, EXT, DATA, CRLF, TRAILER_HEAD, TRAILER_MIDDLE = range(6)   # RHP_CHUNKED_IN_* (rhp.h)
SCANNING = (SIZE, EXT, CRLF, TRAILER_HEAD, TRAILER_MIDDLE)
STATE_NAMES = ("IN_CHUNK_SIZE", "IN_CHUNK_EXT", "IN_CHUNK_DATA", "IN_CHUNK_CRLF", "IN_TRAILERS_LINE_HEAD", "IN_TRAILERS_LINE_MIDDLE")
FRAME, RUN, REST = "frame", "data", "rest"
WINDOW = 64

POOL = random.Random(3101).randbytes(1 << 16)
NOT_LF = POOL.translate(bytes(11 if c == 10 else c for c in range(256)))   # what an extension or a trailer line may hold
_at = [0]


def _slice(pool: bytes, n: int) -> bytes:
    """the next n bytes of the pool, from a start that no two neighbours share"""
    a = _at[0] % (len(pool) - n)
    _at[0] += n + 7919
    return pool[a: a + n]


def data(n: int) -> bytes:
    return _slice(POOL, n)


def line_bytes(n: int) -> bytes:
    """n bytes without an LF (CRs and hex digits among them)"""
    return _slice(NOT_LF, n)


def decoder(left: int, hexc: int, state: int, trailer: int = 0, reserved: bytes = bytes(5)) -> bytes:
    """the 16 bytes of rhp_chunked_t"""
    return left.to_bytes(8, "little") + bytes([trailer, hexc, state]) + reserved


@dataclass
class Piece:
    key: tuple           # ("move", g, o, n), ("filler", f) or (state, k, d, form, shape, call)
    parts: tuple         # ((FRAME | RUN | REST, bytes), ...)
    dec_before: bytes
    ret: int
    dec_after: bytes
    before: bytes = field(init=False)
    size: int = field(init=False)
    after: bytes = field(init=False)

    def __post_init__(self):
        kinds = [k for k, _ in self.parts]
        assert REST not in kinds[:-1] and len(self.dec_before) == 16 and len(self.dec_after) == 16
        assert self.dec_before[8] == self.dec_after[8] and self.dec_before[11:] == self.dec_after[11:], "consumed by no call"
        orig = b"".join(b for _, b in self.parts)
        D = b"".join(b for k, b in self.parts if k == RUN)
        rest = b"".join(b for k, b in self.parts if k == REST)
        src = len(orig) - len(rest)
        assert self.ret == (len(rest) if self.ret >= 0 else self.ret) and (self.ret != -2 or not rest)
        self.before, self.size = orig, len(D)
        self.after = D + orig[len(D):] if self.ret == -2 else D + orig[src:] + orig[len(D) + len(orig) - src:]
        assert len(self.after) == len(orig)


def stream(key, trailer, reserved, calls):
    """calls: [(parts, (left, hex_count, state) before or None for the one the call in front left, ret, (left,
    hex_count, state) after)] -> [Piece]"""
    out, prev = [], None
    for c, (parts, before, ret, after) in enumerate(calls):
        b = decoder(*before, trailer, reserved) if before is not None else prev
        prev = decoder(*after, trailer, reserved)
        out.append(Piece(key if isinstance(key[0], str) else key + (c,), tuple(parts), b, ret, prev))
    return out


# ---------------------------------------------------------------------------
# the move sweep

MOVE_GAPS = tuple(range(1, 25)) + (31, 32, 33, 40, 63, 64, 65)
MOVE_OFFSETS = tuple(range(16))
MOVE_LENGTHS = tuple(range(120, 151)) + tuple(range(1016, 1061)) + tuple(range(2040, 2085))   # the 128-byte threshold, the first
#                                                                        and the second 1 KiB step edge, for every head and tail 0..15
RESERVED = (bytes(5), b"\x11\x22\x33\x44\x55", b"\xff\x00\x80\x0a\x0d")


def move_triples():
    return [(g, o, n) for g in MOVE_GAPS for o in MOVE_OFFSETS for n in MOVE_LENGTHS]


def size_line(g: int, n: int):
    """((left, hex_count, state) before, the g bytes in front of the n data bytes)"""
    H = b"%x" % n
    h = len(H)
    if g == 1:
        return (n, 0, EXT), b"\n"
    if g <= h:   # the first h + 1 - g digits came in an earlier call
        return (int(H[: h + 1 - g], 16), h + 1 - g, SIZE), H[h + 1 - g:] + b"\n"
    if g == h + 1:
        return (0, 0, SIZE), H + b"\n"
    pad = g - h - 2
    return (0, 0, SIZE), H + (b";" + line_bytes(pad - 1) if pad else b"") + b"\r\n"


def move_sweep():
    """[[Piece]]: a filler stream in front of a triple's wherever the batch is not at o mod 16 by itself"""
    out, pos = [], 0
    _at[0] = 0
    for g, o, n in move_triples():
        f = (o - pos) % 16
        if f:
            out.append(stream(("filler", f), 0, bytes(5), [([(REST, b"z" * f)], (0, 0, SIZE), -1, (0, 0, SIZE))]))
        before, line = size_line(g, n)
        assert len(line) == g
        parts = [(FRAME, line), (RUN, data(n)), (FRAME, b"\r\n0\r\n"), (REST, data(5))]
        out.append(stream(("move", g, o, n), 0, RESERVED[(g + o + n) % 3], [(parts, before, 5, (0, 0, EXT))]))
        pos += f + g + n + 10
    return out


# ---------------------------------------------------------------------------
# the window sweep


def distances(k: int):
    """from lane k to the deciding byte: the scan ends in the entry window, at its last lane, at the next window's
    first lanes, and one whole window further on"""
    return sorted(d for d in {0, 1} | set(range(62 - k, 67 - k)) | set(range(126 - k, 131 - k)) if d >= 0)


def digit_counts(k: int):
    """the same for IN_CHUNK_SIZE, d the number of digits: 0 (a non-hex first byte), 1, 16, 17 (the 17th: -1), and
    those of distances(k) that are at most 17.  A line of digits cannot run further: digits cross the window's end
    only from lanes 47 on"""
    return sorted(d for d in {0, 1, 16, 17} | set(range(62 - k, 67 - k)) if 0 <= d <= 17)


def window_distances(state: int, k: int):
    return digit_counts(k) if state == SIZE else distances(k)


HEXDIGITS = b"0123456789abcdefABCDEF"


def digits(d: int, shape: str, r: random.Random) -> bytes:
    """sig: d significant digits, the first 16 of them distinct in value; zeros: leading zeros and three distinct
    digits (at most 0x3ff); either case of a letter"""
    cased = lambda v: (b"0123456789abcdef", b"0123456789ABCDEF")[r.randrange(2)][v: v + 1]
    if shape == "zeros":
        a = r.randrange(1, 4)
        b, c = r.sample([v for v in range(16) if v != a], 2)
        return b"0" * (d - 3) + cased(a) + cased(b) + cased(c)
    if d <= 3:
        vals = [r.randrange(1, 4)]
        vals += r.sample([v for v in range(16) if v != vals[0]], d - 1)
    else:
        vals = r.sample(range(16), 16)
        if vals[0] == 0:
            vals[0], vals[1] = vals[1], vals[0]
        vals = (vals + [r.randrange(16)])[:d]
    return b"".join(cased(v) for v in vals)


def entry(state: int, k: int):
    """How the state is entered at lane k of a piece's first window: ((left, hex_count, state) of the decoder a call
    before left, consume_trailer or None where no call reads it, the parts that consume k bytes without a window
    reload, bytes_left_in_chunk on entry)"""
    if state == SIZE:       # behind the CR LF of a chunk: k - 1 CRs and the LF
        return ((0, 0, SIZE), 0, [], 0) if k == 0 else ((0, 0, CRLF), 0, [(FRAME, b"\r" * (k - 1) + b"\n")], 0)
    if state == EXT:        # carried; behind k digits of a fresh size line; behind CRs, the LF and one digit
        if k == 0:
            return (11, 0, EXT), 0, [], 11
        if k <= 16:
            return (0, 0, SIZE), 0, [(FRAME, b"0" * (k - 1) + b"d")], 13
        return (0, 0, CRLF), 0, [(FRAME, b"\r" * (k - 2) + b"\n9")], 9
    if state == CRLF:       # behind the last k bytes of a chunk's data
        return ((0, 0, CRLF), 0, [], 0) if k == 0 else ((k, 0, DATA), 0, [(RUN, data(k))], 0)
    if state == TRAILER_HEAD:   # carried; behind a trailer line's end; behind the last chunk's size line's end
        if k == 0:
            return (0, 0, TRAILER_HEAD), None, [], 0
        if k & 1:
            return (0, 0, TRAILER_MIDDLE), None, [(FRAME, line_bytes(k - 1) + b"\n")], 0
        return (0, 0, EXT), (1, 0x80)[(k >> 1) & 1], [(FRAME, line_bytes(k - 1) + b"\n")], 0
    assert state == TRAILER_MIDDLE   # behind CRs and a line's first byte
    return ((0, 0, TRAILER_MIDDLE), None, [], 0) if k == 0 else ((0, 0, TRAILER_HEAD), None, [(FRAME, b"\r" * (k - 1) + b"X")], 0)


def window_streams(state: int, k: int, d: int, r: random.Random):
    """the streams of one (state, k, d): {form or (form, shape): [Piece]}"""
    before, trailer, prefix, left = entry(state, k)
    if trailer is None:
        trailer = (0, 1, 0xff)[(k + d) % 3]
    reserved = RESERVED[(k + 2 * d) % 3]
    out = {}

    def add(form, shape, calls):
        out[(form, shape)] = stream((state, k, d, form, shape), trailer, reserved, calls)

    if state == SIZE:
        if d == 0:
            bad = [(REST, bytes([b"x;\r\n g\x00\xff"[(k + d) % 8]]) + b" unread")]
            add("wrong", "", [(prefix + bad, before, -1, (0, 0, SIZE))])
            add("cut", "", [(prefix, before, -2, (0, 0, SIZE)), (bad, None, -1, (0, 0, SIZE))])
            return out
        for shape in ("sig", "zeros") if d >= 4 else ("sig",):
            dg = digits(d, shape, r)
            if d == 17:   # the 17th digit decides
                v, bad = int(dg[:16], 16), [(REST, dg[16:] + b"\r\nab")]
                add("complete", shape, [(prefix + [(FRAME, dg[:16])] + bad, before, -1, (v, 16, SIZE))])
                add("cut", shape, [(prefix + [(FRAME, dg[:16])], before, -2, (v, 16, SIZE)), (bad, None, -1, (v, 16, SIZE))])
                continue
            v = int(dg, 16)
            if v < 4096:
                body, ret, after = [(RUN, data(v)), (FRAME, b"\r\n0\r\n"), (REST, data(3))], 3, (0, 0, EXT)
            else:   # fewer bytes behind it than it says: -2 and the whole 64-bit value, minus what arrived
                body, ret, after = [(RUN, data(40))], -2, (v - 40, 0, DATA)
            add("complete", shape, [(prefix + [(FRAME, dg + b"\r\n")] + body, before, ret, after)])
            add("cut", shape, [(prefix + [(FRAME, dg)], before, -2, (v, d, SIZE)), ([(FRAME, b"\r\n")] + body, None, ret, after)])
    elif state == EXT:
        ext = (b";" + line_bytes(d - 1)) if d else b""     # behind digits: its first byte is no digit
        body = [(RUN, data(left)), (FRAME, b"\r\n0\r\n"), (REST, data(4))]
        mid = (left, 0, EXT) if d or not k else (left, min(k, 16) if k <= 16 else 1, SIZE)   # d = 0 behind digits: still in them
        add("complete", "", [(prefix + [(FRAME, ext + b"\n")] + body, before, 4, (0, 0, EXT))])
        add("cut", "", [(prefix + [(FRAME, ext)], before, -2, mid), ([(FRAME, b"\n")] + body, None, 4, (0, 0, EXT))])
    elif state == CRLF:
        body = [(FRAME, b"4\r\n"), (RUN, data(4)), (FRAME, b"\r\n0\r\n"), (REST, data(2))]
        bad = [(REST, bytes([b"x0\x00\xff;"[(k + d) % 5]]) + b"\n unread")]
        crs = [(FRAME, b"\r" * d)]
        add("complete", "", [(prefix + [(FRAME, b"\r" * d + b"\n")] + body, before, 2, (0, 0, EXT))])
        add("cut", "", [(prefix + crs, before, -2, (0, 0, CRLF)), ([(FRAME, b"\n")] + body, None, 2, (0, 0, EXT))])
        add("wrong", "", [(prefix + crs + bad, before, -1, (0, 0, CRLF))])
    elif state == TRAILER_HEAD:
        rest = [(REST, data(6))]
        crs = [(FRAME, b"\r" * d)]
        add("complete", "", [(prefix + [(FRAME, b"\r" * d + b"\n")] + rest, before, 6, (0, 0, TRAILER_HEAD))])
        add("line", "", [(prefix + [(FRAME, b"\r" * d + b"T: v\r\n\r\n")] + rest, before, 6, (0, 0, TRAILER_HEAD))])
        add("cut", "", [(prefix + crs, before, -2, (0, 0, TRAILER_HEAD)), ([(FRAME, b"\n")] + rest, None, 6, (0, 0, TRAILER_HEAD))])
    else:
        rest = [(REST, data(7))]
        line = line_bytes(d)
        add("complete", "", [(prefix + [(FRAME, line + b"\n\r\n")] + rest, before, 7, (0, 0, TRAILER_HEAD))])
        add("cut", "", [(prefix + [(FRAME, line)], before, -2, (0, 0, TRAILER_MIDDLE)),
                        ([(FRAME, b"\n\r\n")] + rest, None, 7, (0, 0, TRAILER_HEAD))])
    return out


def window_sweep():
    """[[Piece]]"""
    r = random.Random(4211)
    _at[0] = 0
    return [s for state in SCANNING for k in range(WINDOW) for d in window_distances(state, k)
            for s in window_streams(state, k, d, r).values()]


def name(key) -> str:
    """a piece's key in words, for a failure's message"""
    if key[0] == "move":
        return f"move gap {key[1]}, destination offset {key[2]} mod 16, length {key[3]}"
    if key[0] == "filler":
        return f"filler of {key[1]} bytes"
    state, k, d, form, shape, call = key
    return f"{STATE_NAMES[state]} entered at lane {k}, distance {d}, {form}{' ' + shape if shape else ''}, call {call}"
