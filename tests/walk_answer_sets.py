"""The inputs of the rhp_walk_answers tests (tests/test_walk_answers.py): streams of responses, the queues of
outstanding requests they answer, and answer_rounds, the driver that feeds a round from the round before it and pops
the answered requests as rhp.h says.  tests/golden/make_golden_walk_answers.py runs the rounds over the compiled
reference and writes tests/golden/walk_answers.npz, which holds every round's packed bytes and queues too: the tests
read that file, and one CPU test holds it to what this module builds.

A set is a chain of rounds over the same sessions, a dict:
  name, maxh, flags
  mode              0: states == NULL (rhp_walk_responses' walk, one round); 1: rhp_walk_resume's walk
  deliveries[r][s]  the bytes that arrive for session s in round r (b"": nothing new)
  caps[r][s]        the slots session s owns in round r
  states            None (all zero) or WALK_STATE_DTYPE [n_sessions] before round 0 (mode 1)
  heads[s]          one truth value per outstanding request of session s, oldest first: it was a HEAD
  lead              request bits that belong to nobody in front of session 0's queue (all set)
  warp              None, or what the last session's req_off pair is: "unordered" (req_off[n] = 0) or "beyond"
                    (n_req_total one short of req_off[n]); the bits it would own are all set
A round's queue for session s is heads[s] less the requests the rounds before answered.
"""
import numpy as np

import walk_resume_sets as wr
import walk_sets as ws
from walk_sets import TRAILERS, DEFRAME, NONE_EMPTY, resp, length, te, BARE, SHORT, NO_CONTENT, SWITCHING, HELLO  # noqa: F401
from walk_resume_sets import AT_HEAD, IN_LENGTH, IN_CHUNKED, IN_CLOSE, DEAD, STATE_DTYPE, state  # noqa: F401

REQ_NONE = 0xFFFFFFFF            # RHP_WALK_REQ_NONE (rhp.h)
GEOMETRY = (1, 255, 256, 257)    # n_sessions: the block's edges

GET5 = length(b"hello")                                  # the reply to a GET: the body is there
HEAD5 = resp([b"Content-Length: 5"])                     # the reply to a HEAD for the same resource: no body
HEAD_TE = resp([b"Transfer-Encoding: chunked"])
HEAD_BARE = BARE                                         # neither framing header
CONTINUE = resp(status=b"HTTP/1.1 100 Continue")
HINTS = resp([b"Link: </style.css>; rel=preload"], status=b"HTTP/1.1 103 Early Hints")
NOT_MODIFIED5 = resp([b"Content-Length: 5"], status=b"HTTP/1.1 304 Not Modified")
HEAD_500 = resp([b"Content-Length: 500"])
# The framing's -1 (rhp_frame_messages): a Content-Length beside a Transfer-Encoding, a Transfer-Encoding that is not
# chunked.  The number itself is libc strtoull's, which refuses nothing: "5x" is 5 and 2^64 is 2^64 - 1.
HEAD_BADLEN = resp([b"Content-Length: 5", b"Transfer-Encoding: chunked"])
HEAD_BADTE = resp([b"Transfer-Encoding: gzip"])
HEAD_ODDLEN = resp([b"Content-Length: 5x"])
L10 = resp([b"Content-Length: 10"])


def pack_queues(queues, lead=0, warp=None):
    """(req_off u32 [n + 1], head_bits u32 words, n_req_total) for the sessions' queues (lists of truth values) packed
    back to back behind `lead` set bits; every bit that belongs to no session's clamped queue is set"""
    n = len(queues)
    req_off = np.zeros(n + 1, dtype=np.uint32)
    req_off[0] = lead
    req_off[1:] = lead + np.cumsum([len(q) for q in queues])
    bits = [True] * lead + [bool(b) for q in queues for b in q]
    total = len(bits)
    if warp is not None:
        own = int(req_off[n] - req_off[n - 1])
        assert own > 0 and req_off[n - 1] > 0
        bits[total - own:] = [True] * own
        if warp == "unordered":
            req_off[n] = 0
        else:
            assert warp == "beyond"
            total -= 1
    words = (total + 31) // 32
    bits = (bits + [True] * 32)[: 32 * words] if words else []
    head_bits = np.zeros(max(words, 1), dtype=np.uint32)
    for q, b in enumerate(bits):
        if b:
            head_bits[q >> 5] |= np.uint32(1 << (q & 31))
    return req_off, head_bits, total


def answer_rounds(step, s):
    """The rounds of set `s` through `step`, one call per round:
      step(buf, sess_off, slot_off, states, req_off, head_bits, n_req_total) -> dict with results, answered and,
      in mode 1, states (and `carry`: the states as they lie on the device, handed to the next round as they are)
    Round r + 1's input is round r's unconsumed bytes and the new bytes behind them, its states what round r left,
    its queues round r's less the answered requests.  Returns [(buf, sess_off, slot_off, req_off, head_bits,
    n_req_total, out)] per round, the inputs as they went in."""
    n = len(s["deliveries"][0])
    pending = [b""] * n
    queues = [list(h) for h in s["heads"]]
    states = s["states"]
    rounds = []
    for new, cap in zip(s["deliveries"], s["caps"]):
        sessions = [pending[k] + new[k] for k in range(n)]
        buf, off = ws.pack(sessions)
        sl = ws.slot_offsets(cap)
        req_off, head_bits, total = pack_queues(queues, s["lead"], s["warp"])
        out = step(buf, off, sl, states, req_off, head_bits, total)
        if s["mode"]:
            states = out.get("carry", out["states"])
        pending = [sessions[k][int(out["results"]["consumed"][k]):] for k in range(n)]
        queues = [q[int(a):] for q, a in zip(queues, out["answered"])]
        rounds.append((buf, off, sl, req_off, head_bits, total, out))
    return rounds


def replies(heads, get=GET5, head=HEAD5):
    """the stream that answers a queue: a HEAD's reply where the request was one"""
    return b"".join(head if h else get for h in heads)


def _one(name, sessions, heads, cap=6, flags=TRAILERS, mode=0, lead=0, warp=None, maxh=4, states=None):
    caps = cap if isinstance(cap, list) else [cap] * len(sessions)
    return dict(name=name, maxh=maxh, flags=flags, mode=mode, deliveries=[list(sessions)], caps=[caps], states=states,
                heads=[list(h) for h in heads], lead=lead, warp=warp)


def _resume_chains():
    """three rounds, one session per situation; (deliveries, caps, state before round 0, heads)"""
    z = state()
    rows = [((HEAD5[:10], HEAD5[10:] + GET5, b""), (3, 3, 3), z, [1, 0]),                # a round ends inside a HEAD reply's head
            ((L10 + b"01234", b"56789" + HEAD5 + GET5, b""), (3, 3, 3), z, [0, 1, 0]),  # ... inside a GET reply's body
            ((HELLO, b"", b""), (3, 3, 3), state(DEAD), [1]),                              # a dead state
            ((HELLO, b"", b""), (3, 3, 3), state(AT_HEAD, reserved=1), [1]),               # a corrupt state
            ((b"", b"abcde" + HEAD5, b""), (3, 3, 3), state(IN_LENGTH, left=5), [1]),      # an empty round, then the body's rest
            ((L10 + b"01234", b"56789" + HEAD5, b""), (2, 0, 2), z, [0, 1]),              # a continuation with no slot
            ((HEAD_500, GET5, b""), (3, 3, 3), z, [1, 0]),                                 # no state is armed by a HEAD reply
            ((HEAD_TE, GET5, b""), (3, 3, 3), z, [1, 0]),
            ((HEAD_BARE, GET5, b""), (3, 3, 3), z, [1, 0]),
            ((CONTINUE, HEAD5 + GET5[:12], GET5[12:]), (3, 3, 3), z, [1, 0]),              # an interim reply alone in its round
            ((HEAD_TE + b"3\r\nab", b"c\r\n0\r\n\r\n" + HEAD_TE + GET5, b""), (3, 3, 3), z, [0, 1, 0])]   # a chunked body cut, a HEAD behind it
    deliveries = [[x[0][r] for x in rows] for r in range(3)]
    caps = [[x[1][r] for x in rows] for r in range(3)]
    return dict(name="resume_chains", maxh=4, flags=TRAILERS, mode=1, deliveries=deliveries, caps=caps,
                states=np.array([x[2] for x in rows], dtype=STATE_DTYPE), heads=[list(x[3]) for x in rows], lead=0, warp=None)


def all_sets():
    only_last = [0] * 32 + [1]
    return [
        # 1-3: the three shapes the walk went wrong on, each beside the same bytes asked for with GET
        _one("head_length", [HEAD5 + GET5, GET5 + GET5, HEAD5 + HEAD5 + GET5], [[1, 0], [0, 0], [1, 1, 0]]),
        _one("head_chunked", [HEAD_TE + GET5, te([b"abc", b"de"]) + SHORT, HEAD_TE + te([b"xyz"]) + HEAD_TE], [[1, 0], [0, 0], [1, 0, 1]]),
        _one("head_bare", [HEAD_BARE + GET5, HEAD_BARE + GET5], [[1, 0], [0, 0]], flags=0),
        # 4: interim responses
        _one("interim", [CONTINUE + HEAD5, HINTS + HINTS + GET5, SWITCHING + GET5, CONTINUE + HEAD5 + HINTS + GET5, CONTINUE],
             [[1], [0], [0], [1, 0], [1]]),
        # 5: a HEAD bit on a 204 and a 304, beside the same bytes without the bit
        _one("head_no_body_status", [NO_CONTENT + GET5, NO_CONTENT + GET5, NOT_MODIFIED5 + HEAD5 + GET5, NOT_MODIFIED5 + HEAD5 + GET5],
             [[1, 0], [0, 0], [1, 1, 0], [0, 1, 0]]),
        # 6: bit addressing
        _one("bits_from_30", [replies([0, 1, 1]), replies([1, 0, 0]), replies(only_last), replies([1]), replies([0])],
             [[0, 1, 1], [1, 0, 0], only_last, [1], [0]], cap=[4, 4, 34, 2, 2], lead=30),
        _one("bits_from_32", [replies([1, 0]), replies([0, 1]), replies([1, 1, 0])], [[1, 0], [0, 1], [1, 1, 0]], lead=32),
        # 7: more final responses than requests; no request; a pair out of order; a pair beyond n_req_total
        _one("unasked", [HEAD5 + GET5 + GET5, GET5, b"", GET5 + GET5], [[1], [], [1], [1, 1]], warp="unordered"),
        _one("unasked_beyond", [replies([1, 0]), GET5 + GET5], [[1, 0], [1, 1]], lead=31, warp="beyond"),
        # 8, 9: Content-Length beyond the session's end; a Content-Length the framing answers -1 to
        _one("head_length_exceeds", [HEAD_500, HEAD_500 + GET5, HEAD_500], [[1], [1, 0], [0]]),
        _one("head_bad_length", [HEAD_BADLEN + GET5, SHORT + HEAD_BADLEN, HEAD_BADTE + GET5, HEAD_ODDLEN + GET5],
             [[1, 0], [0, 1], [1, 0], [1, 0]]),
        # 10: the slots run out
        _one("more", [HEAD5 + GET5 + GET5, HEAD5 + GET5 + GET5, CONTINUE + HEAD5], [[1, 0, 0], [1, 0, 0], [1]], cap=[1, 2, 1]),
        # 11: the resumed walk
        _resume_chains(),
        _one("resume_one_round", [HEAD5 + GET5, HEAD_TE + GET5, HEAD_BARE + GET5, HEAD_500, GET5[:-2]],
             [[1, 0], [1, 0], [1, 0], [1], [0]], mode=1, flags=0),
    ]


# ---------------------------------------------------------------------------
# a seeded mix for the kernel against the twin

def random_mix(n, seed):
    """n sessions of the resumed walk over three rounds: streams of replies drawn from GET and HEAD shapes (about a
    quarter of the requests HEAD), interim responses between them, two seeded cuts each, slot counts of their own,
    the queues packed back to back so that sessions share words of head_bits"""
    rng = np.random.default_rng(seed)
    gets = [GET5, te([b"abc", b"de"]), SHORT, NO_CONTENT, length(b"0123456789abcdef" * 3), te([b"z" * 40], [b"T: 1"])]
    heads_ = [HEAD5, HEAD_TE, HEAD_BARE, HEAD_500, NOT_MODIFIED5]
    streams, heads = [], []
    for _ in range(n):
        x, h = b"", []
        for _ in range(int(rng.integers(0, 7))):
            if rng.integers(0, 8) == 0:
                x += (CONTINUE, HINTS)[int(rng.integers(0, 2))]
            is_head = bool(rng.integers(0, 4) == 0)
            pool = heads_ if is_head else gets
            x += pool[int(rng.integers(0, len(pool)))]
            h.append(is_head)
        if rng.integers(0, 24) == 0:   # a reply the framing refuses ends a few sessions with BAD
            x += HEAD_BADTE + GET5
            h += [bool(rng.integers(0, 2)), False]
        # some queues are shorter or longer than the replies that arrive
        drift = int(rng.integers(-1, 3))
        h = h[: max(len(h) - 1, 0)] if drift < 0 else h + [bool(rng.integers(0, 2))] * (drift == 2)
        streams.append(x)
        heads.append(h)
    cuts = [sorted(int(c) for c in rng.integers(0, len(x) + 1, size=2)) for x in streams]
    deliveries, _ = wr.cut_plan(streams, cuts, 0)
    caps = [[int(c) for c in rng.integers(0, 7, size=n)] for _ in range(3)]
    return dict(name="mix", maxh=4, flags=TRAILERS, mode=1, deliveries=deliveries, caps=caps, states=None, heads=heads,
                lead=0, warp=None)
