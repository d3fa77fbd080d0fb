"""The inputs of the rhp_relay_walked tests (tests/test_walk_relay.py).  A case is one call of a walk and of the relay
behind it:
  dict(name, kind, maxh, flags, buf, sess_off, slot_off, states, asked, names)
  kind     "once": rhp_walk_responses; "resume": one round of rhp_walk_resume from `states` (WALK_STATE_DTYPE
           [n_sessions]); "answers": rhp_walk_answers over asked = (req_off, head_bits, n_req_total), a round of the
           resumed walk when `states` is not None
  names    the caller's drop names, bytes each
Every case runs with and without RHP_WALK_DEFRAME.  The cases are every set of tests/golden/walk_responses.npz, every
round of every set of walk_resume.npz and of walk_answers.npz (their inputs as those files hold them, read through
the loaders of their tests), and sets of this module's own whose heads, status lines, bodies and sizes sit where the
relay can go wrong.  tests/golden/make_golden_walk_relay.py states rhp.h's rule over their walked records in plain
Python, has the compiled reference's http_write_response write every relayed slot and keeps why, sizes and bytes in
tests/golden/walk_relay.npz.
"""
import functools

import numpy as np

import walk_answer_sets as wa
import walk_resume_sets as wr
import walk_sets as ws
from walk_sets import TRAILERS, NONE_EMPTY, resp, length, te, SHORT, HELLO, BARE

STAGE = 16384                                              # the copy kernel's LDS stage per wave (rhp_classify.hip)
DROP = (b"connection", b"Keep-Alive", b"SERVER", b"Date")   # a proxy's hop-by-hop names, in mixed case
FIXED = 95                                                 # every byte of a reply except its variable parts (http.c:244)


def reply_size(status_text, type_, body_len, fields=()):
    """the size http_write_response allocates (http.c:244-246, 270-272)"""
    return FIXED + len(status_text) + len(type_) + len(str(body_len)) + body_len + sum(len(n) + len(v) + 4 for n, v in fields)


def _case(name, sessions, caps, names=DROP, kind="once", maxh=8, flags=TRAILERS, states=None, heads=None):
    buf, off = ws.pack(sessions)
    asked = wa.pack_queues(heads) if heads is not None else None
    return dict(name=name, kind=kind, maxh=maxh, flags=flags, buf=buf, sess_off=off, slot_off=ws.slot_offsets(caps), states=states,
                asked=asked, names=tuple(names))


def _names():
    typed = lambda *ct: resp(list(ct) + [b"Connection: keep-alive", b"X-Kept: yes", b"server: upstream/1", b"KEEP-ALIVE: timeout=5",
                                         b"date: Tue, 15 Nov 1994 08:12:31 GMT", b"Content-Length: 2"], b"ok")
    s = [typed(b"Content-Type: text/plain", b"content-type: text/second") + typed(b"Content-Type:") + typed() +
         typed(b"X-First: 1", b"CONTENT-TYPE: application/octet-stream"),
         resp(status=b"HTTP/1.1 204 No Content") + resp() + SHORT,                        # heads with no header at all
         resp([b"X-A: 1", b" folded", b"Content-Length: 2"], b"ok") + SHORT,               # an obs-fold line: not relayed
         te([b"chunked ", b"body"]) + resp([b"Transfer-Encoding: chunked", b"Content-Type: a/b"], ws.chunked([b"x" * 40], [b"T: 1"])) + SHORT]
    return _case("names", s, [6, 4, 3, 4], flags=TRAILERS | NONE_EMPTY)


def _full(drop):
    fill = [b"H%d: v%d" % (i, i) for i in range(8)]
    s = [resp(fill) + resp(fill[:7] + [b"Content-Length: 1"], b"z"), SHORT]
    return _case("full_dropped" if drop else "full_kept", s, [3, 2], names=[b"h%d" % i for i in range(8)] if drop else DROP,
                 flags=TRAILERS | NONE_EMPTY)


def _status():
    L2 = [b"Content-Length: 2"]
    s = [resp(L2, b"ok", status=b"HTTP/1.1 200") + resp(L2, b"ok", status=b"HTTP/1.1 200   fine  ") +
         resp(L2, b"ok", status=b"HTTP/1.1 099 Odd") + resp(status=b"HTTP/1.1 100 Continue") +
         resp([b"Content-Length: 3"], status=b"HTTP/1.1 199 Odd") + resp(L2, b"ok", status=b"HTTP/1.0 200 OK") +
         resp(L2, b"ok", status=b"HTTP/1.1 007") + resp(L2, b"ok", status=b"HTTP/1.1 999 \tTab and more")]
    return _case("status", s, [10])


def _stops():
    """the last slot of a BODY and of a CLOSE round, HEAD, BAD and MORE stops, a continuation slot in front of heads"""
    s = [SHORT + length(b"0123456789")[:-1], SHORT + BARE + b"until close", HELLO + SHORT[:20],
         HELLO + b"HTTP/2.0 200 OK\r\n\r\n" + HELLO, HELLO + SHORT + HELLO, b"56789" + HELLO + SHORT, b"567"]
    states = np.array([wr.state()] * 5 + [wr.state(wr.IN_LENGTH, left=5), wr.state(wr.IN_LENGTH, left=5)], dtype=wr.STATE_DTYPE)
    return _case("stops", s, [4, 4, 4, 4, 2, 4, 2], kind="resume", states=states)


def _head_reply():
    """a reply to a HEAD with Content-Length: 5 is relayed with 0; the same reply to a GET carries its five bytes"""
    head, get = resp([b"Content-Length: 5", b"Content-Type: t/x"]), resp([b"Content-Length: 5", b"Content-Type: t/x"], b"hello")
    s = [head + get + head, get + resp([b"Transfer-Encoding: chunked"]) + SHORT]
    return _case("head_reply", s, [4, 4], kind="answers", heads=[[1, 0, 1], [0, 1, 0]])


def _bodies():
    """the body lengths at which the digit count switches, and bodies that start at every residue mod 16"""
    s = [b"".join(length(bytes([65 + k % 26]) * n, [b"Content-Type: b/%d" % n]) for k, n in enumerate((0, 1, 9, 10, 99, 100, 999, 1000)))]
    run = b""
    for k in range(17):
        one = lambda pad: resp([b"X-Pad: " + b"p" * pad, b"Content-Length: 5"], b"b%04d" % k)
        run += one((1 - len(one(0))) % 16)
        assert len(run) % 16 == (k + 1) % 16
    return _case("bodies", s + [run], [9, 18])


def _big_body():
    """one 20 KiB body among 63 small replies: the group leaves the stage and is written reply by reply"""
    small = [length(b"r%02d" % k, [b"Content-Type: s/%d" % k]) for k in range(63)]
    big = length(bytes(range(256)) * 80, [b"Content-Type: big/20k", b"X-Kept: behind the stage"])
    return _case("big_body", [b"".join(small[:31]) + big + b"".join(small[31:])], [64])


def _stage(total):
    """64 replies in one group whose bytes are exactly `total`: the last body is as long as that takes"""
    small = [length(b"s%02d" % k) for k in range(63)]
    used = 63 * reply_size(b"200 OK", b"", 3)
    fit = [n for n in range(total) if used + reply_size(b"200 OK", b"", n) == total]
    assert len(fit) == 1, total
    return _case(f"stage_{total}", [b"".join(small) + length(b"q" * fit[0])], [64])


def own_cases():
    return [_names(), _full(False), _full(True), _status(), _stops(), _head_reply(), _bodies(), _big_body(),
            _stage(STAGE - 16), _stage(STAGE - 15), _stage(STAGE)]


def file_cases():
    """the inputs of the three walk files, one case per call"""
    import test_walk_answers as ta
    import test_walk_responses as t1
    import test_walk_resume as tr
    cases = []
    for name in t1.SET_NAMES:
        maxh, flags, buf, _, sess_off, slot_off, _ = t1.golden_set(name)
        cases.append(dict(name=f"walk_{name}", kind="once", maxh=maxh, flags=flags, buf=buf, sess_off=sess_off, slot_off=slot_off,
                          states=None, asked=None, names=DROP))
    for name in tr.SET_NAMES:
        maxh, flags, rounds = tr.golden_set(name)
        for r, x in enumerate(rounds):
            cases.append(dict(name=f"resume_{name}_r{r}", kind="resume", maxh=maxh, flags=flags, buf=x["buf"], sess_off=x["sess_off"],
                              slot_off=x["slot_off"], states=x["states_in"], asked=None, names=DROP))
    for name in ta.SET_NAMES:
        maxh, flags, mode, rounds = ta.golden_set(name)
        for r, x in enumerate(rounds):
            cases.append(dict(name=f"answers_{name}_r{r}", kind="answers", maxh=maxh, flags=flags, buf=x["buf"], sess_off=x["sess_off"],
                              slot_off=x["slot_off"], states=x["states_in"] if mode else None,
                              asked=(x["req_off"], x["head_bits"], x["n_req_total"]), names=DROP))
    return cases


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = file_cases() + own_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def walk_cpu(rhp, c, deframe):
    """the case's walk on the host twin: (results, slots, msgs, hdrs, bytes, ...)"""
    flags = c["flags"] | deframe
    if c["kind"] == "answers":
        return rhp.walk_answers_cpu(c["buf"], c["sess_off"], c["slot_off"], c["asked"][0], c["asked"][1], c["states"], c["states"] is not None,
                                    c["maxh"], flags, n_req_total=c["asked"][2], slot_req=False)
    if c["kind"] == "resume":
        return rhp.walk_resume_cpu(c["buf"], c["sess_off"], c["slot_off"], c["states"], c["maxh"], flags)
    return rhp.walk_responses_cpu(c["buf"], c["sess_off"], c["slot_off"], c["maxh"], flags)


def random_mix(n, seed):
    """three resumed rounds over n sessions with about a quarter of the bodies chunked: (deliveries, caps) as
    walk_resume_sets.walk_rounds takes them"""
    rng = np.random.default_rng(seed)
    def message():
        body = bytes(rng.integers(97, 123, size=int(rng.integers(0, 300)), dtype=np.uint8))
        lines = [b"Content-Type: mix/%d" % len(body), b"Connection: keep-alive", b"X-Trace: %d" % int(rng.integers(1 << 30))][: int(rng.integers(0, 4))]
        if rng.integers(4) == 0:
            cut = int(rng.integers(0, len(body) + 1))
            return resp(lines + [b"Transfer-Encoding: chunked"], ws.chunked([p for p in (body[:cut], body[cut:]) if p]))
        return length(body, lines)
    streams = [b"".join(message() for _ in range(int(rng.integers(1, 6)))) for _ in range(n)]
    cuts = [sorted(int(c) for c in rng.integers(0, len(x) + 1, size=2)) for x in streams]
    deliveries, _ = wr.cut_plan(streams, cuts, 0)
    caps = [[int(c) for c in rng.integers(1, 8, size=n)] for _ in range(3)]
    return deliveries, caps
