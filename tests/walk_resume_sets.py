"""The inputs of the rhp_walk_resume tests (tests/test_walk_resume.py): streams of responses and the plans that cut
them into rounds, built here from fixed text and seeded cuts, and walk_rounds, the driver that feeds a round from the
round before it as rhp.h says.  tests/golden/make_golden_walk_resume.py runs the rounds over the compiled reference
and writes tests/golden/walk_resume.npz, which holds every round's packed bytes too: the tests read that file, and
one CPU test holds it to what this module builds.

A set is a chain of rounds over the same sessions:
  (name, max_headers, flags, deliveries, caps, states)
  deliveries[r][s]  the bytes that arrive for session s in round r (b"": nothing new)
  caps[r][s]        the slots session s owns in round r
  states            None (all zero: every connection's first round) or WALK_STATE_DTYPE [n_sessions] before round 0
A round's input for session s is what the round before left unconsumed of its input, [consumed, len), and
deliveries[r][s] behind it; the sessions lie back to back with RHP_PAD zero bytes behind the last.
"""
import numpy as np

import walk_sets as ws
from walk_sets import RHP_PAD, TRAILERS, DEFRAME, NONE_EMPTY, resp, chunked, length, te, HELLO, SHORT, BARE, NO_CONTENT  # noqa: F401

AT_HEAD, IN_LENGTH, IN_CHUNKED, IN_CLOSE, DEAD = range(5)   # enum rhp_walk_phase (rhp.h)
GEOMETRY = (1, 63, 64, 65, 257)
# rhp_walk_state_t (rhp.h), as libreactorng_amd.WALK_STATE_DTYPE
STATE_DTYPE = np.dtype([("decoder", [("bytes_left_in_chunk", "<u8"), ("consume_trailer", "u1"), ("hex_count", "u1"),
                                     ("state", "u1"), ("reserved", "u1", (5,))]),
                        ("left", "<u8"), ("phase", "<u4"), ("reserved", "<u4")])


def state(phase=AT_HEAD, left=0, reserved=0, chunk_left=0, consume_trailer=0, hex_count=0, dstate=0):
    s = np.zeros(1, dtype=STATE_DTYPE)
    s["phase"], s["left"], s["reserved"] = phase, left, reserved
    d = s["decoder"]
    d["bytes_left_in_chunk"], d["consume_trailer"], d["hex_count"], d["state"] = chunk_left, consume_trailer, hex_count, dstate
    return s[0]


def walk_rounds(step, deliveries, caps, max_headers, flags, states=None):
    """The rounds of one set through `step`, one call per round:
      step(buf, sess_off, slot_off, states, max_headers, flags) -> (results, slots, msgs, hdrs, bytes, states[, carry])
    as libreactorng_amd.walk_resume_cpu / walk_resume_gpu return.  Round r + 1's input is round r's unconsumed bytes,
    [consumed, len) of each session as round r found them, and the new bytes behind them; its states are what round r
    left -- `carry` where step returns one (the states as they lie on the device), the returned states otherwise.
    Returns [(buf, sess_off, slot_off, out)] per round, buf as it went in."""
    n = len(deliveries[0])
    pending = [b""] * n
    rounds = []
    for new, cap in zip(deliveries, caps):
        sessions = [pending[s] + new[s] for s in range(n)]
        buf, off = ws.pack(sessions)
        sl = ws.slot_offsets(cap)
        out = step(buf, off, sl, states, max_headers, flags)
        states = out[6] if len(out) > 6 else out[5]
        consumed = out[0]["consumed"]
        pending = [sessions[s][int(consumed[s]):] for s in range(n)]
        rounds.append((buf, off, sl, out))
    return rounds


# ---------------------------------------------------------------------------
# the streams

CUT_STREAM = (length(b"hello") +
              resp([b"Transfer-Encoding: chunked"],
                   b"5;x=y\r\nabcde\r\r\n" + b"10\r\n0123456789abcdef\r\n" + b"0\r\n" + b"T: 1\r\n" + b"\r\n") +
              NO_CONTENT + length(b"world"))
DRIP_STREAM = (length(b"abc") + resp([b"Transfer-Encoding: chunked"], b"2\r\nhi\r\n0\r\nT: 1\r\n\r\n") +
               resp(status=b"HTTP/1.1 204 No") + resp([b"Content-Length: 0"]))


def cut_plan(streams, cuts, cap):
    """deliveries and caps of streams cut at cuts[s] (ascending offsets): len(cuts[s]) + 1 rounds"""
    r = len(cuts[0]) + 1
    edges = [[0] + list(c) + [len(x)] for x, c in zip(streams, cuts)]
    deliveries = [[x[e[k]: e[k + 1]] for x, e in zip(streams, edges)] for k in range(r)]
    return deliveries, [[cap] * len(streams) for _ in range(r)]


def _cut_everywhere():
    """session k gets CUT_STREAM[:k] in round 0 and the rest in round 1, for every k in 1 .. L - 1"""
    L = len(CUT_STREAM)
    return cut_plan([CUT_STREAM] * (L - 1), [[k] for k in range(1, L)], 6)


def _drip(n):
    """DRIP_STREAM one byte per round.  n == 1: the whole stream, a round per byte.  n > 1: the sessions stand at
    staggered offsets: session j gets the first (7 j) mod 120 bytes in round 0, then a byte per round for 10 rounds,
    then the rest, so every launch holds lanes in every phase and every byte of the stream is some session's drip"""
    L = len(DRIP_STREAM)
    if n == 1:
        return cut_plan([DRIP_STREAM], [list(range(1, L))], 4)
    cuts = [[(7 * j) % 120 + k for k in range(11)] for j in range(n)]
    return cut_plan([DRIP_STREAM] * n, cuts, 4)


def kinds_streams():
    """the sessions of walk_sets' kinds that are no longer than 160 bytes (the file stays small)"""
    return [x for x in ws._kinds()[0] if len(x) <= 160]


def _three_rounds(n, seed):
    """n sessions over the streams of walk_sets' kinds, two seeded cuts each"""
    rng = np.random.default_rng(seed)
    pool = kinds_streams()
    streams = [pool[i % len(pool)] for i in range(n)]
    cuts = [sorted(int(c) for c in rng.integers(0, len(x) + 1, size=2)) for x in streams]
    return cut_plan(streams, cuts, 7)


def _stops():
    """every stop reached from a continuation and from a head; three rounds; (deliveries, cap) per session"""
    L30 = resp([b"Content-Length: 30"])
    TE = resp([b"Transfer-Encoding: chunked"])
    L10 = resp([b"Content-Length: 10"])
    huge = resp([b"Content-Length: -1"])
    s = [((L30 + b"01234", b"56789", b"abcde"), (3, 3, 3)),                        # BODY, BODY, BODY: twice from a continuation
         ((TE + b"a\r\n012", b"345", b"6789\r\n0\r\n\r\n"), (3, 3, 3)),            # the same inside a chunk, then END
         ((BARE + b"abc", b"def", b""), (3, 3, 3)),                                 # CLOSE, CLOSE, CLOSE on an empty round
         ((TE + b"3\r\nab", b"cXX", b"more"), (3, 3, 3)),                           # BAD inside a resumed chunk, then DEAD
         ((L10 + b"01234", b"56789" + SHORT, b""), (2, 0, 2)),                      # MORE on a continuation with no slot, then a slot
         ((SHORT + SHORT + SHORT, b"", b""), (2, 2, 2)),                            # MORE in the head loop
         ((HELLO[:20], HELLO[20:], b""), (3, 3, 3)),                                # HEAD, then the head completed
         ((TE, b"3\r\nabc\r\n0\r\n\r\n", b""), (3, 3, 3)),                          # a chunked head that ends exactly at e
         ((huge + b"abc", b"defg", b""), (3, 3, 3)),                                # Content-Length 2^64 - 1
         ((L10 + b"01234", b"56789" + b"HTTP/2.0 200 OK\r\n\r\n", b"x"), (3, 3, 3)),   # BAD at a head behind a continuation
         ((L10 + b"01234", b"56789" + BARE + b"xy", b"z"), (3, 3, 3)),              # CLOSE at a head behind a continuation
         ((TE + b"3\r\na", b"bc\r\n0\r\n\r\n" + SHORT[:10], SHORT[10:]), (3, 3, 3)),   # HEAD behind a continuation
         ((L10 + b"01234", b"56789", b""), (3, 3, 3)),                              # left == avail exactly: END from a continuation
         ((L10 + b"01234", b"56789" + L10 + b"ab", b"cdefghij"), (3, 3, 3)),        # BODY at a head behind a continuation
         ((L10 + b"01234", b"56789" + SHORT + SHORT, b""), (2, 2, 2)),              # MORE in the head loop behind a continuation
         ((b"HTTP/2.0 200 OK\r\n\r\n", b"", b"abc"), (3, 3, 3)),                    # BAD at the first head; DEAD on an empty round
         ((L10 + b"01234", b"56789" + SHORT, b""), (1, 1, 1)),                      # MORE right behind a continuation slot
         ((TE + b"3\r\nabc", b"\r", b"\r\r\n0\r\n\r\n"), (3, 3, 3)),                # a cut inside the CR run, twice
         ((L10, b"0123456789", b""), (3, 3, 3))]                                    # a Content-Length head that ends exactly at e
    deliveries = [[x[0][r] for x in s] for r in range(3)]
    caps = [[x[1][r] for x in s] for r in range(3)]
    return deliveries, caps


def _corrupt():
    """one round: a session for each corrupt-state rule, sound states between them"""
    body = b"3\r\nabc\r\n0\r\n\r\n"
    rows = [(HELLO, state()),
            (HELLO, state(DEAD)),
            (HELLO, state(DEAD + 1)),
            (HELLO, state(0xFFFFFFFF)),
            (HELLO, state(AT_HEAD, reserved=1)),
            (b"abc" + SHORT, state(IN_LENGTH, left=3)),
            (body, state(IN_CHUNKED, dstate=6)),
            (body, state(IN_CHUNKED, hex_count=17)),
            (b"\r\n" + SHORT, state(IN_CHUNKED, consume_trailer=1, dstate=5)),          # state 5 is sound: a trailer line's rest
            (b"a\r\n0123456789\r\n0\r\n", state(IN_CHUNKED, hex_count=16)),               # hex_count 16 is sound; a 17th digit is -1
            (HELLO, state(IN_LENGTH, left=3, reserved=0x80000000)),
            (HELLO, state(AT_HEAD, dstate=9, hex_count=99))]                              # the decoder is not looked at outside IN_CHUNKED
    return [[r[0] for r in rows]], [[3] * len(rows)], np.array([r[1] for r in rows], dtype=STATE_DTYPE)


def _empty_rounds():
    """a == e at each phase, between sessions that have bytes"""
    rows = [(b"", state(AT_HEAD)), (HELLO, state()), (b"", state(IN_LENGTH, left=5)),
            (b"", state(IN_CHUNKED, consume_trailer=1, chunk_left=4, dstate=2)), (b"", state(IN_CLOSE)), (b"", state(DEAD)),
            (b"abcde", state(IN_LENGTH, left=5)), (b"", state(AT_HEAD))]
    return [[r[0] for r in rows]], [[2] * len(rows)], np.array([r[1] for r in rows], dtype=STATE_DTYPE)


def _sp_run_into_moving_body():
    """A ends in the version and spaces up to e; its neighbour B is a continuation inside a size line's rest whose
    first bytes are spaces, which the de-framing overwrites with the chunk's data.  The mirror: A's run ends one byte
    before e.  The last A runs into the pad."""
    moving = b"      \r\nwxyz\r\n2\r\nuv\r\n0\r\n\r\n" + SHORT
    ext = state(IN_CHUNKED, consume_trailer=1, chunk_left=4, dstate=1)
    rows = [(SHORT + b"HTTP/1.1    ", state()), (moving, ext),
            (SHORT + b"HTTP/1.1   2", state()), (moving, ext),
            (b"HTTP/1.1  ", state())]
    return [[r[0] for r in rows]], [[3] * len(rows)], np.array([r[1] for r in rows], dtype=STATE_DTYPE)


def all_sets():
    sets = []
    add = lambda name, maxh, flags, plan, states=None: sets.append((name, maxh, flags, plan[0], plan[1], states))
    add("cut_everywhere", 8, TRAILERS, _cut_everywhere())
    add("drip", 8, TRAILERS, _drip(1))
    add("drip65", 8, TRAILERS, _drip(65))
    add("three_rounds", 8, TRAILERS, _three_rounds(257, 20261020))
    add("three_rounds_f0", 8, 0, _three_rounds(21, 7))
    add("three_rounds_f5", 4, TRAILERS | NONE_EMPTY, _three_rounds(21, 11))
    add("stops", 8, TRAILERS, _stops())
    add("stops_f0", 8, 0, _stops())
    for name, f in (("corrupt", _corrupt), ("empty_rounds", _empty_rounds), ("sp_run_into_moving_body", _sp_run_into_moving_body)):
        d, c, st = f()
        add(name, 8, TRAILERS, (d, c), st)
    return sets


def random_mix(n, seed):
    """n sessions over walk_sets' pool, the residue sessions and this module's streams, two seeded cuts and slot
    counts of their own: (deliveries, caps) of three rounds"""
    rng = np.random.default_rng(seed)
    pool = [a for a, _ in ws.pool()] + ws._residues()[0] + [CUT_STREAM, DRIP_STREAM]
    streams = [pool[i] for i in rng.integers(0, len(pool), size=n)]
    cuts = [sorted(int(c) for c in rng.integers(0, len(x) + 1, size=2)) for x in streams]
    deliveries, _ = cut_plan(streams, cuts, 0)
    caps = [[int(c) for c in rng.integers(0, 7, size=n)] for _ in range(3)]
    return deliveries, caps
