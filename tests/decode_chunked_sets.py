"""The test sets of rhp_decode_chunked (include/rhp.h), built without any library: what
tests/golden/make_golden_decode_chunked.py feeds to the compiled reference and what tests/test_decode_chunked.py
holds the golden file to.

A Stream is one chunked body as it arrives: `pieces`, one per call, the decoder zero-filled before the first call
but for consume_trailer (`trailer`) and the five reserved bytes; `initial` = (bytes_left_in_chunk, hex_count,
state) starts it from a decoder no earlier call of the set left.  A set is (name, start, [Stream]): its calls, in
order, are the pieces of one batch, packed back to back from byte `start` on.
"""
from __future__ import annotations

import random
from dataclasses import dataclass

SIZE, EXT, DATA, CRLF, TRAILER_HEAD, TRAILER_MIDDLE = range(6)   # RHP_CHUNKED_IN_* (rhp.h)


@dataclass
class Stream:
    pieces: list
    trailer: int = 0
    reserved: bytes = bytes(5)
    initial: tuple = (0, 0, SIZE)


def data(n: int, seed: int = 0) -> bytes:
    """n bytes of every value, CR, LF and hex digits among them: chunk data is never looked at"""
    return bytes((i * 37 + seed * 101 + (i >> 7) * 13 + 10) & 0xff for i in range(n))


def chunk(d: bytes, ext: bytes = b"", eol: bytes = b"\r\n", after: bytes = b"\r\n", digits: bytes | None = None) -> bytes:
    return (digits if digits is not None else b"%x" % len(d)) + ext + eol + d + after


def one(body: bytes, trailer: int = 0, **kw) -> Stream:
    return Stream([body], trailer, **kw)


SIZES = (1, 15, 16, 17, 127, 128, 129, 1023, 1024, 1025, 5000)
EXT_SHORT = b";name=value"
EXT_100 = b";e=" + b"x" * 97                 # longer than a window of 64
EXT_1500 = b" ; q=\"" + b"y" * 1493 + b"\""    # longer than 1024
TRAILERS = b"Trailer-One: v1\r\nX-Long: " + b"t" * 100 + b"\r\n\r\rY: z\n"   # the third line behind two CRs, ended by a bare LF


def set_whole():
    """whole bodies in one call"""
    s = []
    for k, n in enumerate(SIZES):
        s.append(one(chunk(data(n, k)) + b"0\r\n\r\n", trailer=k & 1))      # without consume_trailer: ret 2, the CR LF left over
    s.append(one(b"".join(chunk(data(n, 20 + k)) for k, n in enumerate(SIZES)) + b"0\r\n\r\n", 1))   # every move by another amount
    s.append(one(chunk(data(70000, 3)) + b"0\r\n"))
    s.append(one(b"0\r\n"))                                                  # the end alone
    s.append(one(b"0\r\n\r\n", 1, reserved=b"\x11\x22\x33\x44\x55"))         # an empty trailer section; the reserved bytes stay
    s.append(one(chunk(data(0xab, 4), digits=b"00Ab") + chunk(data(0xab, 5), digits=b"aB") + chunk(data(0xcd, 6), digits=b"0cD") + b"000\r\n"))
    s.append(one(chunk(data(10, 7), digits=b"000000000000000a") + b"0\r\n"))      # exactly 16 digits
    s.append(one(chunk(data(10, 7), digits=b"0000000000000000a") + b"0\r\n"))     # a 17th: -1
    s.append(one(b"1ffffffffffffffff\r\nab"))                                     # a 17th, all significant
    s.append(one(b"ffffffffffffffff\r\n" + data(40, 8)))                          # 2^64 - 1 bytes to come
    s.append(one(chunk(data(30, 9), EXT_SHORT) + chunk(data(200, 10), EXT_100) + chunk(data(130, 11), EXT_1500) + b"0" + EXT_100 + b"\r\n"))
    s.append(one(chunk(data(77, 12), ext=EXT_1500, eol=b"\n") + b"0" + EXT_1500 + b"\n", 1))   # (ends in the trailers: -2)
    s.append(one(chunk(data(5, 13), eol=b"\n", after=b"\n") + chunk(data(300, 14), eol=b"\n") + b"0\n"))   # bare LFs
    s.append(one(chunk(data(64, 15), after=b"\r\r\r\n") + chunk(data(1, 16), after=b"\r" * 70 + b"\n") + b"0\r\n"))   # CR runs, one longer than a window
    for t in (0, 1):
        s.append(one(chunk(data(100, 17)) + b"0\r\n" + TRAILERS + b"\r\n" + data(33, 18), t))
    for left in (0, 1, 300):
        s.append(one(chunk(data(50, 19 + left)) + chunk(data(500, 20 + left)) + b"0\r\n\r\n" + data(left, 21), 1))
    return s


def set_overlap():
    """a first size line of 2, 3, 4 and 19 bytes (the shortest two by way of digits that came in an earlier call),
    3000 data bytes, and a second such chunk that moves by another amount -- each at every start offset mod 16,
    reached with a filler piece in front ('z' * g: -1 at once, nothing moved)"""
    second = b"bb8\r\n" + data(3000, 31) + b"\r\n"
    shapes = [([b"bb"], b"8\n"), ([b"bb"], b"8\r\n"), ([], b"bb8\n"), ([], b"bb8;ext=abcdefghi\r\n")]
    assert [len(l) for _, l in shapes] == [2, 3, 4, 19]
    s, pos = [], 0
    for o in range(16):
        for k, (first, line) in enumerate(shapes):
            g = (o - pos - sum(map(len, first))) % 16
            big = line + data(3000, 30 + k) + b"\r\n" + second
            s += [one(b"z" * g), Stream(first + [big])]
            pos += g + sum(map(len, first)) + len(big)
    return s


CUT_BODY = (chunk(data(61, 40), ext=b";ext=\"q\"", after=b"\r\r\r\n", digits=b"3d") + chunk(data(10, 41), eol=b"\n", digits=b"00a") +
            b"0;last\r\n" + b"Trailer-One: v1\r\n\r\rX: y\n" + b"\r\n" + b"LEFTOVER")


def set_cuts2():
    return [Stream([CUT_BODY[:c], CUT_BODY[c:]], 1) for c in range(1, len(CUT_BODY))]


def set_cuts3():
    r = random.Random(1523)
    out = []
    for _ in range(200):
        a, b = sorted(r.sample(range(1, len(CUT_BODY)), 2))
        out.append(Stream([CUT_BODY[:a], CUT_BODY[a:b], CUT_BODY[b:]], 1))
    return out


def set_prefixes():
    return [one(CUT_BODY[:c], 1) for c in range(len(CUT_BODY) + 1)]


def set_big_chunk():
    """a chunk larger than the piece: bytes_left_in_chunk carried across three calls"""
    d = data(1000, 50)
    return [Stream([b"3e8\r\n" + d[:300], d[300:700], d[700:] + b"\r\n0\r\n"])]


def set_errors():
    """each -1 with unread bytes behind it and decoded bytes in front, so that the closing move is seen"""
    return [one(b"xyz unread"),                                               # a non-hex first byte (nothing decoded: no move)
            one(b"2\r\nab\r\nzzz the rest stays unread"),                     # the same at the second size line
            one(b"3\r\nabcx\r\n0\r\n unread bytes behind"),                   # x where the LF after data belongs
            one(b"3\r\nabc\r\rx\n"),                                          # ... behind CRs
            Stream([b"1\r\na\r\n000000000000000", b"12\r\nunread bytes behind"]),   # the 17th digit arrives in a second call
            Stream([b"0000000000000001", b"2\r\nunread"]),                    # ... as its first byte
            Stream([b"\r\n5\r\nhello\r\n"], initial=(0, 0, DATA)),            # decoders no call leaves, which the reference still takes:
            Stream([b";x\r\nabc\r\n0\r\n"], initial=(3, 7, EXT))]             # no data left in IN_CHUNK_DATA; a digit count outside the digits


FAMILY = [chunk(data(5 + 7 * k, 60 + k), ext=EXT_SHORT if k % 3 == 0 else b"") + (chunk(data(3 * k + 1, 80 + k)) if k & 1 else b"") + b"0\r\n" +
          data(k % 4, 90 + k) for k in range(13)]


def batch_of(n):
    """n whole bodies, every 7th piece empty; 13 different bodies in turn, so neighbours differ"""
    return [one(b"" if j % 7 == 3 else FAMILY[j % 13]) for j in range(n)]


BATCH_SIZES = (1, 3, 4, 5, 63, 64, 65, 257)


def set_fuzz():
    """300 mutated bodies (byte flips, cuts, duplicated lines) at random cuts"""
    r = random.Random(977)
    base = [chunk(data(20, 70), ext=b";a=b") + chunk(data(9, 71), after=b"\r\r\n") + b"0\r\n" + b"T: v\r\n\r\n" + b"left",
            chunk(data(33, 72), eol=b"\n") + b"000\r\nAb: c\n\r\n"]
    out = []
    for _ in range(300):
        b = bytearray(r.choice(base))
        for _ in range(r.randrange(4)):
            kind = r.randrange(3)
            if kind == 0 and b:
                b[r.randrange(len(b))] = r.choice(b"\r\n0aF;x \xff\x00") if r.random() < 0.7 else r.randrange(256)
            elif kind == 1 and len(b) > 2:
                a = r.randrange(len(b))
                del b[a: a + r.randrange(1, 6)]
            else:
                lines = bytes(b).split(b"\n")
                k = r.randrange(len(lines))
                lines.insert(k, lines[k])
                b = bytearray(b"\n".join(lines))
        b = bytes(b)
        cuts = sorted(r.sample(range(len(b) + 1), r.randrange(3))) if b else []
        out.append(Stream([b[x:y] for x, y in zip([0] + cuts, cuts + [len(b)])], r.randrange(2)))
    return out


def all_sets():
    sets = [("whole", 0, set_whole()), ("overlap", 0, set_overlap()), ("cuts2", 16, set_cuts2()), ("cuts3", 5, set_cuts3()),
            ("prefixes", 0, set_prefixes()), ("big_chunk", 3, set_big_chunk()), ("errors", 0, set_errors())]
    sets += [(f"n{n}", 0, batch_of(n)) for n in BATCH_SIZES]
    sets.append(("fuzz", 1, set_fuzz()))
    return sets


def fresh_decoder(s: Stream) -> bytes:
    """the 16 bytes of rhp_chunked_t before the stream's first call"""
    left, hexc, state = s.initial
    return left.to_bytes(8, "little") + bytes([s.trailer, hexc, state]) + s.reserved
