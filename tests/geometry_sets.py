"""Batches chosen for how rhp_parse_batch is launched, not for what a request
holds (tests/test_gpu_geometry.py; their claims are checked on the CPU in
tests/test_geometry_sets.py).

launch_dfa (rhp_kernel.hip) runs grid = min(CUs, ceil(n / 1024)) workgroups;
workgroup g owns requests [g * span, min((g + 1) * span, n)), span =
ceil(n / grid).  What a range does changes with its length: `ranges` restates
that formula, `cycle` is a batch for any n, `span_batch` / `deferred_batch`
give every range a chosen length and a chosen kind.

Every batch is assembled from a few request templates by index (numpy), so a
batch of two million requests costs a fraction of a second."""
from __future__ import annotations

import numpy as np

import libreactorng_amd as rhp

WG_REQUESTS = 1024     # 64 lanes x 16 waves: both modes' workgroups (rhp_kernel.hip RHP_PHR_WAVES, kHttpWaves)
DEFER_CAP = 480        # rhp_kernel.hip kDeferCap
SLOW_CAP = 6080        # rhp_kernel.hip kSlowCap with 16 waves: (kLdsTable 26624 - 16 * kChunkTabWave 144) / 4
ORDER_SPAN = 8192      # rhp_kernel.hip kOrderSpan


def assemble(templates, which, align_shift=0):
    """(buf, off) of the batch whose request i is templates[which[i]] (as
    batches.pack: RHP_PAD zero bytes behind, align_shift zero bytes before)"""
    which = np.asarray(which, dtype=np.int64)
    lens = np.array([len(t) for t in templates], dtype=np.int64)
    off = np.zeros(len(which) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens[which])
    off += np.uint64(align_shift)
    buf = np.zeros(int(off[-1]) + rhp.RHP_PAD, dtype=np.uint8)
    starts = off[:-1].astype(np.int64)
    for t, tpl in enumerate(templates):
        if len(tpl):
            at = starts[which == t]
            buf[at[:, None] + np.arange(len(tpl))[None, :]] = np.frombuffer(tpl, dtype=np.uint8)
    return buf, off


def _get(path, *fields):
    return b"GET " + path + b" HTTP/1.1\r\n" + b"".join(n + b": " + v + b"\r\n" for n, v in fields) + b"\r\n"


# the kinds every cycle holds, by name (test_geometry_sets.py finds each outcome in the oracle's records)
_ONE_WINDOW = [_get(b"/"), _get(b"/a", (b"Host", b"x")), _get(b"/plaintext", (b"Host", b"tfb"), (b"Accept", b"*/*")),
               b"POST /p HTTP/1.0\r\nA: b\r\n\r\n", _get(b"/" + b"q" * 40, (b"H", b"v"))]
_MANY_WINDOWS = [_get(b"/two-long-values", (b"X-A", b"a" * 150), (b"X-B", b"b" * 160)),                    # 3 windows, 2 headers
                 _get(b"/" + b"p" * 200, (b"Host", b"h" * 90), (b"C", b"c" * 200)),                        # 5 windows
                 _get(b"/eight", *[(b"X-H%d" % k, b"v" * (30 + k)) for k in range(8)]),                     # 8 headers
                 _get(b"/fourteen", *[(b"X-Header-%02d" % k, b"w" * (40 + k)) for k in range(14)])]         # ~1 KiB
_EXACT = [b"\r\nGET /crlf HTTP/1.1\r\nHost: a\r\n\r\n",                    # leading CRLF
          b"GET /fold HTTP/1.1\r\nA: b\r\n \tfolded  \r\n\r\n",            # obs-fold
          b"GET /lf HTTP/1.0\nX: y\n\n"]                                   # bare LF
_BAD = [b"GET / HTTP/1.1\r\nBad Header\r\n\r\n", b"GET / HTTP/2.0\r\n\r\n", b"GET /ctl HTTP/1.1\r\nA: a\x01b\r\n\r\n"]
_PARTIAL = [b"GET / HTTP/1.1\r\nA: b\r", b"GET /part", b"G"]
_EMPTY = [b""]
_HTTP_ONLY = [b"POST /cl HTTP/1.1\r\nContent-Length: 5\r\n\r\nhello",                                               # a body
              b"POST /short HTTP/1.1\r\nContent-Length: 9\r\n\r\nhel",                                              # result 0
              b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n",      # chunked
              b"POST /c HTTP/1.1\r\nHost: h\r\nTransfer-Encoding: Chunked\r\n\r\n" +
              b"".join(b"%x\r\n%s\r\n" % (k, b"d" * k) for k in (1, 15, 16, 200)) + b"0\r\n\r\n",
              b"POST /m HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\nzz\r\nhello\r\n0\r\n\r\n",                    # malformed
              b"PUT /z HTTP/1.1\r\nContent-Length: 0\r\n\r\n"]
_PHR_ONLY = [_get(b"/k%d" % k, (b"K", b"v" * (7 * k))) for k in range(6)]


def _interleave(*groups):
    """round-robin over the groups, so that neighbours in the cycle are of different kinds"""
    out, k = [], 0
    while any(k < len(g) for g in groups):
        out += [g[k] for g in groups if k < len(g)]
        k += 1
    return out


def cycle_templates(mode):
    """the cycle's 37 requests (a prime: with 64 lanes a wave, a lane's kind
    changes from wave to wave and from refill to refill); none above 1 KiB"""
    own = _HTTP_ONLY if mode == rhp.MODE_HTTP else _PHR_ONLY
    common = _ONE_WINDOW + _MANY_WINDOWS + _EXACT + _BAD + _PARTIAL + _EMPTY
    more = [_get(b"/r%d" % k, (b"Host", b"r" * k)) for k in range(37 - len(common) - len(own))]
    t = _interleave(_ONE_WINDOW + more, _MANY_WINDOWS, _EXACT + _EMPTY, _BAD, _PARTIAL, own)
    assert len(t) == 37 and max(len(x) for x in t) <= 1024
    return t


def cycle(n, mode, align_shift=0):
    """the first n requests of the fixed 37-request cycle: every outcome (plain
    GETs of one and of three or more windows; leading CRLF, obs-fold and bare LF,
    which the emulator sends to the exact path; -1; -2; an empty request; in http
    mode a Content-Length body, a short body, chunked bodies, a malformed
    chunked body)"""
    return assemble(cycle_templates(mode), np.arange(n) % 37, align_shift)


def ranges(n, cus):
    """the (lo, hi) request ranges launch_dfa gives its workgroups for a batch of n on `cus` CUs"""
    grid = max(min(cus, -(-n // WG_REQUESTS)), 1)
    span = -(-n // grid)
    return [(min(g * span, n), min((g + 1) * span, n)) for g in range(grid)]


# 18 .. 40 bytes; 61 of them in turn (a prime, coprime to every range length the tests use)
SHORT = [b"GET /" + b"s" * (k % 23) + b" HTTP/1.1\r\n\r\n" if k % 3 else
         b"GET /" + b"t" * (k % 17) + b" HTTP/1.0\r\nH: v\r\n\r\n" for k in range(61)]
LONG = _get(b"/" + b"L" * 100, *[(b"X-Long-%d" % k, b"l" * 60) for k in range(4)])    # >= 400 bytes, 4 headers
PLAIN18 = b"GET / HTTP/1.1\r\n\r\n"
DEFER_HTTP = b"POST / HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n3\r\nabc\r\n0\r\n\r\n"   # framed in the replay
DEFER_PHR = b"\r\nGET / HTTP/1.1\r\n\r\n"                                                    # the exact path
assert all(18 <= len(s) <= 40 for s in SHORT) and len(LONG) >= 400 and len(PLAIN18) == 18


def span_n(S, cus, short_last=False):
    """the batch size that gives `cus` ranges of S requests; short_last: the
    smallest n with span S (cus * (S - 1) + 1: its last range has S - cus + 1)"""
    return cus * (S - 1) + 1 if short_last else cus * S


def _span_which(n, kind):
    i = np.arange(n)
    which = i % len(SHORT)
    if kind == "even":
        return which
    long_at = i % 16 == 0
    if kind == "mixed":
        long_at &= i >= n // 2
    elif kind != "uneven":
        raise ValueError(kind)
    return np.where(long_at, len(SHORT), which)


def span_batch(S, cus, kind, n=None):
    """n = cus * S requests (or the caller's n) of 18 to 40 bytes.  kind "even":
    no request is longer than twice its range's mean (the write-through path of
    the header-major, compact and dense layouts); "uneven": a request of 400
    bytes or more at every 16th index, so that len * span_n > 2 * range_bytes
    holds for one of every range's first 64 requests (the kernel's test);
    "mixed": the batch's first half even, its second half uneven."""
    n = span_n(S, cus) if n is None else n
    return assemble(SHORT + [LONG], _span_which(n, kind))


def deferred_batch(S, cus, per_range, mode, n=None, plain18=False):
    """span_batch(S, cus, "even") with per_range requests of every range replaced
    by ones the loop defers to the replay: chunked bodies in http mode, requests
    of the exact path (a leading CRLF) in phr mode.  They stand past the range's
    first 64 requests where the range has room (the kernel's evenness test reads
    those), evenly spread.  per_range: 480 (kDeferCap: the replay's list just
    holds them), 481 (it overflows: the replay scans the range, http mode frames
    directly), or kSlowCap + 1 = 6081 (phr mode: the slow list overflows too and
    the exact path runs inline).  plain18: every other request is the 18-byte
    plain GET."""
    n = span_n(S, cus) if n is None else n
    which = np.zeros(n, dtype=np.int64) if plain18 else np.arange(n) % len(SHORT)
    templates = ([PLAIN18] if plain18 else SHORT) + [DEFER_HTTP if mode == rhp.MODE_HTTP else DEFER_PHR]
    for lo, hi in ranges(n, cus):
        ln = hi - lo
        k = min(per_range, ln)
        first = 64 if ln - 64 >= k else 0
        at = lo + first + (np.arange(k) * (ln - first)) // max(k, 1)
        which[at] = len(templates) - 1
    return assemble(templates, which)


# ---- the properties the names claim, by the kernel's own tests ----

def range_is_uneven(off, lo, hi):
    """rhp_dfa_kernel's test (`uneven`): one of the range's first 64 requests has
    len * span_n > 2 * range_bytes"""
    o = off[lo:hi + 1].astype(np.int64)
    ln = np.diff(o)[:64]
    return bool((ln * (hi - lo) > 2 * (o[-1] - o[0])).any())


def range_has_no_long_request(off, lo, hi):
    """no request of the range is longer than twice its mean"""
    o = off[lo:hi + 1].astype(np.int64)
    return bool((np.diff(o) * (hi - lo) <= 2 * (o[-1] - o[0])).all())


def is_chunked(reqs, http):
    """the oracle's records of requests whose chunked body was de-framed: a body
    whose framing was consumed with it"""
    return (http["result"] == 1) & (http["body_kind"] == 1) & \
           (http["consumed"] != reqs["ret"].astype(np.uint64) + http["body_len"])


def deferred_per_range(off, cus, deferred):
    """how many requests of each range are deferred (a bool per request)"""
    c = np.concatenate([[0], np.cumsum(deferred)])
    return [int(c[hi] - c[lo]) for lo, hi in ranges(len(off) - 1, cus)]


# ---- what a fill shows ----

def fill_word(fill, dtype="<i4"):
    return np.frombuffer(bytes([fill]) * np.dtype(dtype).itemsize, dtype=dtype)[0]


def assert_no_slot_left(res, mode, fill, want):
    """After a parse into request-major buffers that held `fill`: no reqs[i].ret,
    and in http mode no http[i].result, still reads as the fill.  Where the
    fill's word is a value the parser can give (0xFF: -1), the slots the oracle
    (want: canonical records) gives that value are left out; a fill such as 0x5A,
    whose word no answer has, leaves none out."""
    word = fill_word(fill)
    for name, got, exp in (("reqs[i].ret", res.reqs["ret"], want[0]["ret"]),
                           ("http[i].result", res.http["result"] if mode == rhp.MODE_HTTP else None,
                            want[2]["result"] if mode == rhp.MODE_HTTP else None)):
        if got is None:
            continue
        left = (got == word) & (exp != word)
        if left.any():
            raise AssertionError(f"{name} still holds the fill 0x{fill:02x} in {int(left.sum())} slots, first #"
                                 f"{int(np.flatnonzero(left)[0])}")
