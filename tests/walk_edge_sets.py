"""The inputs of the walk tests at the readable end (tests/test_walk_edges.py): calls of rhp_walk_responses and
rhp_walk_resume whose bytes_size puts the readable end -- rhp_walk_args.h rhp_walk_readable(bytes_size), `lim` here --
at, inside and just behind the last message of a session, with walkable text lying beyond it.
tests/golden/make_golden_walk_edges.py runs the compiled reference over the clamped view of every case (the same
bytes with zeros from lim on, offsets min(off, lim)) and writes tests/golden/walk_edges.npz; the tests read that
file, and one CPU test holds it to what this module builds.

A buffer, one per (kind, pad):
  LEAD           whole responses, not a session: what is under test starts behind byte RHP_PAD
  (an empty session)
  the session under test
  PLANTED, PLANTED   two sessions of complete, valid responses
  BEHIND         more responses behind the last sess_off entry
  RHP_PAD zero bytes
so every byte from lim on, inside and beyond bytes_size, is walkable text: a reader that does not stop at lim gives
other answers.  The head kinds' session is a 204 head with an X-Pad header of `pad` bytes, HELLO, and the kind's
last message; the continuation kinds' session is raw body bytes and HELLO, walked from a state, and the 204 head
with the pad closes the lead.  The pad moves what is under test through every start residue mod 16.

A case is one call: (call, kind, pad, c, lim, bytes_size) with c = lim - (the last message's start; for a
continuation kind the session's start), every integer from -8 to that message's (session's) length + 8, each
realised by the one pad that puts lim on a line start; bytes_size = lim + 16 + r, r cycling through 0..15 over a
kind's cases.  Four sessions (the empty one, the one under test, the planted two) own SLOTS slots; max_headers 8;
flags RHP_WALK_TRAILERS, and the tests add RHP_WALK_DEFRAME.
"""
import functools

import numpy as np

import walk_resume_sets as wr
from walk_sets import RHP_PAD, TRAILERS, HELLO, CHUNKS, CHUNKS_T, SHORT, NO_CONTENT, resp, length, te, chunked

MAXH = 8
FLAGS = TRAILERS
SLOTS = (1, 5, 3, 3)
LEAD = HELLO + CHUNKS_T + SHORT + NO_CONTENT
PLANTED = HELLO + CHUNKS + HELLO
BEHIND = SHORT + CHUNKS + HELLO
assert len(LEAD) >= RHP_PAD
PADS = 16
RESPONSES, RESUME = 0, 1
CALL_NAMES = ("responses", "resume")

BODY40 = b"0123456789abcdefghijklmnopqrstuvwxyzABCD"
BODY37 = b"abcdefghijklmnopqrstuvwxyz0123456789+"
LAST = {"length": length(BODY40),
        "chunked": te([BODY40, BODY37, b"final"], [b"X-Sum: 9"]),
        "head": resp([b"X-First: one", b"ETag: \"v2\""], status=b"HTTP/1.1 204 No Content"),
        "sp": SHORT + b"HTTP/1.1 " + b" " * 30,
        "close": resp(body=BODY40)}
CONT = {"in_length": (b"L" * 50 + HELLO, wr.state(wr.IN_LENGTH, left=50)),
        "in_chunked": (b"1234567\r\n" + chunked([BODY37], [b"X-Sum: 9"]) + HELLO,
                       wr.state(wr.IN_CHUNKED, chunk_left=7, consume_trailer=1, dstate=2)),   # 2: in chunk data
        "in_close": (BODY40 + HELLO, wr.state(wr.IN_CLOSE))}
KINDS = ("length", "chunked", "head", "sp", "close", "in_length", "in_chunked", "in_close")
KINDS_OF = {RESPONSES: KINDS[:4], RESUME: KINDS}


def head(pad):
    return resp([b"X-Pad: " + b"p" * pad], status=b"HTTP/1.1 204 No Content")


def state_in(kind):
    """the state of the session under test before a rhp_walk_resume case (every other session's: all zero)"""
    return CONT[kind][1] if kind in CONT else wr.state()


def parts(kind, pad):
    """(lead, the session under test, the offset inside the buffer that c counts from, the length c runs over)"""
    if kind in CONT:
        lead, session = LEAD + head(pad), CONT[kind][0]
        return lead, session, len(lead), len(session)
    session = head(pad) + HELLO + LAST[kind]
    return LEAD, session, len(LEAD) + len(head(pad) + HELLO), len(LAST[kind])


@functools.lru_cache(maxsize=None)
def buffer(kind, pad):
    """(bytes u8, sess_off u64 [5]) of one buffer, read-only"""
    lead, session, _, _ = parts(kind, pad)
    text = lead + session + PLANTED + PLANTED + BEHIND
    buf = np.zeros(len(text) + RHP_PAD, dtype=np.uint8)
    buf[: len(text)] = np.frombuffer(text, dtype=np.uint8)
    off = np.cumsum([len(lead), 0, len(session), len(PLANTED), len(PLANTED)]).astype(np.uint64)
    buf.setflags(write=False)
    off.setflags(write=False)
    return buf, off


def slot_off():
    return np.concatenate([[0], np.cumsum(SLOTS)]).astype(np.uint64)


def cases(kind):
    """[(pad, c, lim, bytes_size)] of one kind, the same for both calls"""
    _, _, m0, n = parts(kind, 0)
    out = []
    for i, c in enumerate(range(-8, n + 9)):
        pad = -(m0 + c) % PADS
        lim = m0 + pad + c
        assert lim % 16 == 0 and lim + 31 <= buffer(kind, pad)[0].size and lim + 16 >= RHP_PAD
        out.append((pad, c, lim, lim + 16 + i % 16))
    return out


def all_cases():
    """[(call, kind, pad, c, lim, bytes_size)], the file's order"""
    return [(call, kind) + x for call in (RESPONSES, RESUME) for kind in KINDS_OF[call] for x in cases(kind)]


# ---------------------------------------------------------------------------
# sess_off rows that hold anything, over one small batch per call: the n65 set of walk_responses.npz and round 1 of
# three_rounds of walk_resume.npz, with bytes_size all of the buffer


def readable(bytes_size):
    """rhp_walk_args.h rhp_walk_readable"""
    return (bytes_size & ~15) - 16


@functools.lru_cache(maxsize=None)
def small_batch(call):
    """dict of buf, sess_off, slot_off, states (None: all zero), maxh, flags: the batch as the two golden files hold it"""
    if call == RESPONSES:
        import test_walk_responses as t
        maxh, flags, buf, _, sess_off, slot_off, _ = t.golden_set("n65")
        return dict(buf=buf, sess_off=sess_off, slot_off=slot_off, states=None, maxh=maxh, flags=flags)
    import test_walk_resume as t
    maxh, flags, rounds = t.golden_set("three_rounds")
    x = rounds[1]
    return dict(buf=x["buf"], sess_off=x["sess_off"], slot_off=x["slot_off"], states=x["states_in"], maxh=maxh, flags=flags)


def stray_cases(call):
    """[(lo, hi, value, deframe)]: sess_off rows [lo, hi] hold `value`.  A single row s: session s - 1 runs on to
    lim through its neighbours, session s is empty; without RHP_WALK_DEFRAME only, since the sessions overlap.  The
    last three rows at a value from lim on: the trailing sessions are empty and the one before them runs over bytes
    that are nobody else's, so these run with RHP_WALK_DEFRAME too (deframe 1)"""
    b = small_batch(call)
    ns, size = len(b["sess_off"]) - 1, b["buf"].size
    lim = readable(size)
    out = [(s, s, v, 0) for s in (1, ns // 2, ns) for v in (2 ** 64 - 1, 2 ** 63, size, size - 1, lim, lim + 1, lim - 1)]
    return out + [(ns - 2, ns, v, 1) for v in (2 ** 64 - 1, 2 ** 63, size, lim, lim + 1)]


def stray_offsets(sess_off, lo, hi, value):
    so = np.array(sess_off, dtype=np.uint64)
    so[lo: hi + 1] = np.uint64(value)
    return so


def clamped(so, s, lim):
    """the [a, e) rhp.h gives session s of sess_off `so`"""
    a, e = min(int(so[s]), lim), int(so[s + 1])
    return a, a if e < a else min(e, lim)
