"""rhp_forward_sessions (include/rhp.h): the requests of a proxied route re-written
for the upstream, and the queue rhp_walk_answers wants of them.

tests/golden/forward_sessions.npz holds why, size, bytes, fwd_off and head_bits
of every case of tests/forward_sets.py; tests/golden/make_golden_forward.py
wrote it from rhp.h's rule in plain Python and held every forwarded slot's bytes
to the compiled reference's http_read_request (the round trip).  Here the host
twin and the kernels are held to the file, to each other on larger rounds, and to
the rule on hand-built records, one per why code and in rhp.h's order.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import forward_sets as fs
from golden.make_golden_forward import expected as rule_expected

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, H = fs.LAYOUTS
LAYOUT_IDS = {R: "request-major", H: "header-major"}
CASES = [(name, layout) for name in fs.CASE_NAMES for layout in fs.LAYOUTS]
CASE_IDS = [f"{name}-{LAYOUT_IDS[layout]}" for name, layout in CASES]


# ---- the file ----

def test_golden_holds_the_cases_and_is_small():
    g = fs.golden()
    assert tuple(str(x) for x in g["case_name"]) == fs.CASE_NAMES
    assert os.path.getsize(fs.GOLDEN) <= 64 * 1024


def test_golden_covers():
    """what the cases are for, held against the file's answers"""
    whys = np.concatenate([fs.expected(name)[0] for name in fs.CASE_NAMES])
    for code in (rhp.FORWARD_OK, rhp.FORWARD_UNUSED, rhp.FORWARD_NOT_READY, rhp.FORWARD_CLOSED, rhp.FORWARD_ROUTE, rhp.FORWARD_FOLD):
        assert (whys == code).any(), f"no slot with why {code}"
    why, size, out, fwd_off, bits = fs.expected("heads")
    assert (why == 0).all() and bits.tolist() == [0b110010101], "HEAD in upper case alone sets a bit"
    assert b"Content-Length: 11\r\n" in bytes(fs.expected("chunked")[2]) and b"chunked" not in bytes(fs.expected("chunked")[2])
    drops = bytes(fs.expected("drops")[2])
    assert b"onnection" not in drops and b"User-Agent: ten-letters\r\n" in drops and b"X-Custom-Hdr: " in drops and b"X-Empty: \r\n" in drops
    assert b"Content-Length: 3\r\n" in drops and b"CONTENT-LENGTH" not in drops
    assert b"Connection: keep-alive\r\n" in bytes(fs.expected("no_names")[2])
    assert b"\r\nD: 4\r\nVia: 1.1 rhp\r\n\r\n" in bytes(fs.expected("full")[2])
    assert bytes(fs.expected("extra_128")[2]).count(fs.EXTRA_128) == 4 and b"Via" not in bytes(fs.expected("extra_empty")[2])
    assert b"Content-Length: 0\r\n" in bytes(fs.expected("posts")[2]) and b"Content-Length: 300\r\n" in bytes(fs.expected("posts")[2])
    why = fs.expected("mixed")[0]
    assert (why[1:3] == rhp.FORWARD_ROUTE).all() and why[0] == why[3] == 0, "a forwarded request behind ones that are not"


def test_rule_equals_file():
    """the generator's rule over today's host records gives the file (no reference needed)"""
    for name in fs.CASE_NAMES:
        got, want = rule_expected(fs, name), fs.expected(name)
        assert all(len(a) == len(b) and (np.asarray(a) == np.asarray(b)).all() for a, b in zip(got, want)), name


# ---- the host twin ----

@pytest.mark.parametrize("name,layout", CASES, ids=CASE_IDS)
def test_cpu_twin_equals_golden(name, layout):
    fs.same_as_expected(fs.forward_cpu(name, layout), fs.expected(name), f"{name} (host)")


def test_cpu_out_one_byte_short():
    for name in ("posts", "heads"):
        want = fs.expected(name)
        total = int(want[1].sum())
        out_off, why, out, fwd_off, bits = fs.forward_cpu(name, out_size=total - 1)
        assert out is None and int(out_off[-1]) == total and (np.diff(out_off) == want[1]).all() and (why == want[0]).all()
        assert (fwd_off == want[3]).all() and (bits == want[4]).all(), "the queue is complete when out is too small"


def _raw_forward_cpu(b, sess, results, starts, route, size, n_routes=len(fs.ROUTES), mask=fs.FORWARD_MASK):
    """one host call over an `out` of `size` poison bytes: (rc, out)"""
    n, ns = b.n, len(sess)
    off = np.zeros(n + 1, dtype=np.uint64)
    why = np.zeros(max(n, 1), dtype=np.uint32)
    out = np.full(max(size, 1), rhp.FORWARD_POISON, dtype=np.uint8)
    fo = np.zeros(ns + 1, dtype=np.uint32)
    hb = np.zeros((n + 31) // 32 + 1, dtype=np.uint32)
    work = np.zeros(rhp.forward_work_words(n, ns), dtype=np.uint64)
    *_keep, f = rhp._forward_desc(n_routes, mask, fs.DROP, fs.VIA, rhp._ptr(off), rhp._ptr(why), rhp._ptr(out) if size else None, size,
                                  rhp._ptr(fo), rhp._ptr(hb), rhp._ptr(work))
    rc = rhp.host().rhp_cpu_forward_sessions(ctypes.byref(b), rhp._ptr(sess), ns, rhp._ptr(results), rhp._ptr(starts), rhp._ptr(route),
                                             ctypes.byref(f))
    return rc, out


def test_cpu_out_untouched_when_short():
    res, results, starts, route = fs.host_round("posts")
    total = int(fs.expected("posts")[1].sum())
    rc, out = _raw_forward_cpu(res.batch, fs.packed("posts")[2], results, starts, route, total - 1)
    assert rc == 0 and (out == rhp.FORWARD_POISON).all(), "out one byte short stays untouched"


# ---- hand-built records: one per why code, and the order of the tests ----

CRAFT_SESSIONS = (fs.post(40) + fs.post(40) + fs.post(40), fs.GET)
CODES = tuple(range(rhp.FORWARD_UNUSED, rhp.FORWARD_BODY_OUTSIDE + 1))
CODE_IDS = ("UNUSED", "NOT_READY", "OUTSIDE", "CLOSED", "ROUTE", "FOLD", "SPAN", "BODY", "LONG", "BODY_OUTSIDE")


@functools.lru_cache(maxsize=None)
def _craft_base(layout):
    buf, off, sess, _ = rhp.pack_sessions(list(CRAFT_SESSIONS))
    return (buf, off, sess) + fs.host_round_of(buf, off, sess, 16, layout)


def crafted(layout, codes):
    """the base round (three POSTs with a body, then a session of one GET) with slot 1 made to fail every test of
    `codes`; applied from the last code to the first, so that an earlier test's craft stands.  Returns (buf, off, sess,
    Batch over copies, raw reqs, raw hdrs, raw http, results, starts, route)"""
    buf, off, sess, res, results, starts, route = _craft_base(layout)
    n, m = len(off) - 1, 16
    raw_reqs, raw_hdrs, raw_http = res.raw_reqs.copy(), res.raw_hdrs.copy(), res.raw_http.copy()
    results, starts, route = results.copy(), starts.copy(), route.copy()
    reqs = raw_reqs[: n * rhp.REQ_DTYPE.itemsize].view(rhp.REQ_DTYPE)
    hdrs = rhp.hdr_view(raw_hdrs.view(rhp.HDR_DTYPE), n, m, layout)
    http = raw_http[: n * rhp.HTTP_DTYPE.itemsize].view(rhp.HTTP_DTYPE)
    i, last = 1, 2
    for code in sorted(codes, reverse=True):
        if code == rhp.FORWARD_UNUSED:
            results["n_slots"][0] = 1
        elif code == rhp.FORWARD_NOT_READY:
            http["result"][i] = 0
        elif code == rhp.FORWARD_OUTSIDE:
            starts[i] = off[sess["piece_hi"][0]]   # the request would end behind its session
        elif code == rhp.FORWARD_CLOSED:
            http["result"][last] = -1
        elif code == rhp.FORWARD_ROUTE:
            route[i] = rhp.ROUTE_NONE
        elif code == rhp.FORWARD_FOLD:
            hdrs["name_off"][i, 0] = rhp.RHP_NAME_NULL
        elif code == rhp.FORWARD_SPAN:
            hdrs["value_len"][i, 1] = 0xFFFF
        elif code == rhp.FORWARD_BODY:
            http["body_kind"][i] = rhp.BODY_CHUNKED_PENDING
        elif code == rhp.FORWARD_LONG:
            http["body_kind"][i], http["body_len"][i] = 1, 2 ** 32
        elif code == rhp.FORWARD_BODY_OUTSIDE and rhp.FORWARD_LONG not in codes:
            http["body_kind"][i], http["body_len"][i] = 1, 0xFFFFFFF0
    rw = res.bytes_out.copy()
    b = rhp.Batch(rhp._ptr(rw), rhp._ptr(rw), rhp._ptr(off), rw.size, n, m, rhp.MODE_HTTP, layout, rhp._ptr(raw_reqs), rhp._ptr(raw_hdrs),
                  rhp._ptr(raw_http), None, rhp.BATCH_SPECULATIVE, 0, None)
    return buf, off, sess, b, raw_reqs, raw_hdrs, raw_http, results, starts, route, rw


def check_crafted(why, out_off, code, label, codes=()):
    """slot 1 answers `code` and has no bytes; slot 0 is forwarded unless the session is made CLOSED; the other session's GET always is"""
    assert int(why[1]) == code and int(out_off[2]) == int(out_off[1]), f"{label}: why {why.tolist()}"
    closed = rhp.FORWARD_CLOSED in codes and rhp.FORWARD_UNUSED not in codes   # (with n_slots 1 the walk's last slot is slot 0)
    assert int(why[0]) == (rhp.FORWARD_CLOSED if closed else 0), f"{label}: why {why.tolist()}"
    assert int(why[-1]) == 0 and int(why[-2]) == rhp.FORWARD_UNUSED, "the slot behind the three POSTs is no session's; the GET is forwarded"


@pytest.mark.parametrize("layout", fs.LAYOUTS, ids=LAYOUT_IDS.values())
@pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
def test_cpu_why_codes_in_order(code, layout):
    for codes in ((code,), tuple(c for c in CODES if c >= code)):   # alone, and with every later test failing too
        _, off, sess, b, *_recs, results, starts, route, rw = crafted(layout, codes)
        out_off, why, out, fwd_off, bits = rhp.forward_sessions_cpu(b, sess, results, starts, route, len(fs.ROUTES), fs.FORWARD_MASK,
                                                                  fs.DROP, fs.VIA)
        check_crafted(why, out_off, code, f"{CODE_IDS[code - 1]} of {codes}", codes)
        assert int(fwd_off[-1]) == int((why == 0).sum()) and out is not None


def test_cpu_body_outside_the_readable_bytes():
    """a body inside its session that ends above bytes_size rounded down to 4"""
    _, off, sess, b, *_recs, results, starts, route, rw = crafted(R, ())
    end = int(starts[2])   # the second POST's body ends where the third request starts
    for size in range(end - 4, end + 5):   # (the request's head ends 40 bytes lower: it stays inside)
        b.bytes_size = size
        why = rhp.forward_sessions_cpu(b, sess, results, starts, route, len(fs.ROUTES), fs.FORWARD_MASK, fs.DROP, fs.VIA)[1]
        assert int(why[1]) == (0 if (size & ~3) >= end else rhp.FORWARD_BODY_OUTSIDE), (size, end, why.tolist())


# ---- refusals and the empty calls ----

def _refusals():
    """(label, change(batch, forward desc fields, call args))"""
    def setf(**kw):
        return lambda b, f, a: [setattr(f, k, v) for k, v in kw.items()]

    def setb(**kw):
        return lambda b, f, a: [setattr(b, k, v) for k, v in kw.items()]

    def seta(k, v):
        return lambda b, f, a: a.__setitem__(k, v)

    return [("phr mode", setb(mode=rhp.MODE_PHR)), ("no flags", setb(flags=0)), ("a length layout", setb(layout=rhp.LAYOUT_COMPACT)),
            ("max_headers", setb(max_headers=65)), ("no reqs", setb(reqs=None)), ("no offsets", setb(offsets=None)),
            ("no sessions", seta("sessions", None)), ("no results", seta("results", None)), ("no req_start", seta("starts", None)),
            ("no route", seta("route", None)), ("no f", seta("f", None)),
            ("no out_off", setf(out_off=None)), ("no why", setf(why=None)), ("no fwd_off", setf(fwd_off=None)),
            ("no head_bits", setf(head_bits=None)), ("no work", setf(work=None)), ("no out", setf(out=None)),
            ("n_routes 0", setf(n_routes=0)), ("n_routes 33", setf(n_routes=33)), ("15 names", setf(n_names=15)),
            ("no names", setf(names=None)), ("no text", setf(text=None)), ("extra 129", setf(extra_len=129)),
            ("no extra", setf(extra=None)), ("extra without CRLF", setf(extra=b"Via: 1.1 rhp\r\r")),
            ("extra of one byte", setf(extra=b"\n", extra_len=1))]


REFUSALS = _refusals()


def _call_with(change, which, misalign=None):
    _, off, sess, b, *_recs, results, starts, route, rw = crafted(R, ())
    n, ns = b.n, len(sess)
    bufs = {k: np.zeros(v + 1, dtype=np.uint64) for k, v in (("out_off", n + 1), ("why", n), ("fwd_off", ns + 1), ("head_bits", n),
                                                             ("work", rhp.forward_work_words(n, ns)), ("out", 512))}
    keep = rhp._forward_desc(len(fs.ROUTES), fs.FORWARD_MASK, fs.DROP, fs.VIA, *(rhp._ptr(bufs[k]) for k in ("out_off", "why", "out")), 4096,
                             *(rhp._ptr(bufs[k]) for k in ("fwd_off", "head_bits", "work")))
    f = keep[-1]
    if misalign:
        setattr(f, misalign[0], getattr(f, misalign[0]) + misalign[1])
    a = {"sessions": rhp._ptr(sess), "results": rhp._ptr(results), "starts": rhp._ptr(starts), "route": rhp._ptr(route), "f": ctypes.byref(f)}
    if change:
        change(b, f, a)
    args = [ctypes.byref(b), a["sessions"], ns, a["results"], a["starts"], a["route"], a["f"]]
    if which == "host":
        return rhp.host().rhp_cpu_forward_sessions(*args)
    return rhp.lib().rhp_forward_sessions(*args, None)


@pytest.mark.parametrize("label,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refused_arguments(label, change):
    """-EINVAL from the host twin and, before anything is launched, from the device entry (host pointers are never
    read there: the check comes first)"""
    assert _call_with(None, "host") == 0
    assert _call_with(change, "host") == -22, label
    assert _call_with(change, "device") == -22, label


@pytest.mark.parametrize("field,by", [("out_off", 4), ("work", 4), ("why", 2), ("fwd_off", 2), ("head_bits", 1)])
def test_refused_alignment(field, by):
    """the device entry's own rules; the host twin takes any alignment"""
    assert _call_with(None, "device", (field, by)) == -22
    assert _call_with(None, "host", (field, by)) == 0


def test_cpu_empty_calls():
    buf, off, sess = fs.packed("gets")
    res, results, starts, route = fs.host_round("gets")
    none = np.zeros(0, dtype=rhp.SESSION_DTYPE)
    out_off, why, out, fwd_off, bits = rhp.forward_sessions_cpu(res, none, results[:0], starts, route, len(fs.ROUTES), fs.FORWARD_MASK)
    assert out_off.tolist() == [0] and fwd_off.tolist() == [0] and len(bits) == 0 and len(why) == 0
    eb, eoff, _, _ = rhp.pack_sessions([])
    eres, er, es = rhp.fixup_cpu(eb, eoff, sess[:0], 16)
    zero = np.zeros(3, dtype=rhp.SESSION_DTYPE)
    out_off, why, out, fwd_off, bits = rhp.forward_sessions_cpu(eres, zero, np.zeros(3, dtype=rhp.SESSION_RESULT_DTYPE), es,
                                                              np.zeros(1, dtype=np.uint16), len(fs.ROUTES), fs.FORWARD_MASK)
    assert out_off.tolist() == [0] and fwd_off.tolist() == [0, 0, 0, 0] and len(bits) == 0


# ---- the hand-over to the upstream walk ----

REPLY = b"HTTP/1.1 200 OK\r\nContent-Type: text/plain\r\nContent-Length: 5\r\n\r\n"


def upstream_replies(name, got):
    """what an upstream answers to the forwarded requests of a case, one connection per client session: a reply with
    Content-Length: 5 to each, its five body bytes only when the request was no HEAD.  (sess_off, slot_off, bytes,
    replies per session)"""
    out_off, why, out, fwd_off, bits = got
    sess = fs.packed(name)[2]
    data, counts = [], []
    for s in range(len(sess)):
        replies = b""
        for i in range(int(sess["piece_lo"][s]), int(sess["piece_hi"][s])):
            if why[i] == 0:
                req = bytes(out[int(out_off[i]): int(out_off[i + 1])])
                replies += REPLY + (b"" if req.startswith(b"HEAD ") else b"hello")
        data.append(replies)
        counts.append(int(fwd_off[s + 1] - fwd_off[s]))
    sess_off = np.concatenate([[0], np.cumsum([len(d) for d in data])]).astype(np.uint64)
    slot_off = np.concatenate([[0], np.cumsum([c + 1 for c in counts])]).astype(np.uint64)
    buf = np.frombuffer(b"".join(data) + b"\0" * rhp.RHP_PAD, dtype=np.uint8).copy()
    return sess_off, slot_off, buf, counts


def check_hand_over(name, got, walk):
    sess_off, slot_off, buf, counts = upstream_replies(name, got)
    out = walk(buf, sess_off, slot_off, got[3], got[4])
    results, slots, answered = out[0], out[1], out[-2]
    assert answered.tolist() == counts, f"{name}: answered {answered.tolist()} of {counts}"
    assert results["n_slots"].tolist() == counts and (results["consumed"] == np.diff(sess_off)).all(), \
        f"{name}: every reply is taken whole, the HEAD replies without a body"
    heads = sum(bin(int(w)).count("1") for w in got[4])
    assert int((slots["body_len"][[int(slot_off[s]) + k for s in range(len(counts)) for k in range(counts[s])]] == 0).sum()) == heads


def test_cpu_queue_feeds_walk_answers():
    """fwd_off and head_bits, as they stand, are rhp_walk_asked_t's req_off and head_bits"""
    for name in ("heads", "extra_128", "mixed"):
        check_hand_over(name, fs.forward_cpu(name), rhp.walk_answers_cpu)
    got = fs.forward_cpu("heads")
    sess_off, slot_off, buf, counts = upstream_replies("heads", got)
    none = rhp.walk_answers_cpu(buf, sess_off, slot_off, got[3], np.zeros_like(got[4]))
    assert (none[0]["consumed"] != np.diff(sess_off)).any(), "without the HEAD bits the walk waits for bodies that never come"


def test_host_twin_asan_ubsan_clean():
    """`make forward-sessions-asan`: a stand-alone program over the host sources (tests/forward_sessions_host_test.c)"""
    csrc = os.path.join(ROOT, "libreactorng_amd", "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "forward-sessions-asan"], capture_output=True, text=True)
    assert out.returncode == 0 and "all ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- the kernels ----

@pytest.mark.gpu
@pytest.mark.parametrize("name,layout", CASES, ids=CASE_IDS)
def test_gpu_equals_golden(name, layout):
    fs.same_as_expected(fs.forward_gpu(name, layout, guard=4096), fs.expected(name), f"{name} (gpu)")


@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(16))
def test_gpu_out_at_every_residue(shift):
    fs.same_as_expected(fs.forward_gpu("posts", guard=512, out_shift=shift), fs.expected("posts"), f"posts, out at +{shift}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["posts", "heads", "extra_128"])
def test_gpu_out_one_byte_short(name):
    want = fs.expected(name)
    total = int(want[1].sum())
    out_off, why, out, fwd_off, bits = fs.forward_gpu(name, guard=512, out_size=total - 1)   # (asserts that out stays untouched)
    assert out is None and int(out_off[-1]) == total and (np.diff(out_off) == want[1]).all() and (why == want[0]).all()
    assert (fwd_off == want[3]).all() and (bits == want[4]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", fs.LAYOUTS, ids=LAYOUT_IDS.values())
@pytest.mark.parametrize("code", CODES, ids=CODE_IDS)
def test_gpu_why_codes_in_order(code, layout):
    for codes in ((code,), tuple(c for c in CODES if c >= code)):
        buf, off, sess, b, raw_reqs, raw_hdrs, raw_http, results, starts, route, rw = crafted(layout, codes)
        got = rhp.forward_sessions_gpu(rw, off, sess, fs.ROUTES, fs.FORWARD_MASK, fs.DROP, fs.VIA, 16, layout=layout, guard=512,
                                       records=(raw_reqs, raw_hdrs, raw_http, results, starts, route))
        want = rhp.forward_sessions_cpu(b, sess, results, starts, route, len(fs.ROUTES), fs.FORWARD_MASK, fs.DROP, fs.VIA)
        check_crafted(got[1], got[0], code, f"{CODE_IDS[code - 1]} of {codes}", codes)
        same(got, want, f"crafted {codes}")


def same(got, want, label):
    for a, b, what in zip(got, want, ("out_off", "why", "out", "fwd_off", "head_bits")):
        assert a is not None and b is not None and len(a) == len(b) and (np.asarray(a) == np.asarray(b)).all(), f"{label}: {what} differs"


def gpu_equals_twin(sessions, label, names=fs.DROP, extra=fs.VIA, maxh=16, layout=R, guard=512):
    """one round on the GPU and on the host; returns the GPU's answer"""
    buf, off, sess, _ = rhp.pack_sessions(list(sessions))
    got = rhp.forward_sessions_gpu(buf, off, sess, fs.ROUTES, fs.FORWARD_MASK, names, extra, maxh, layout=layout, guard=guard)
    res, results, starts, route = fs.host_round_of(buf, off, sess, maxh, layout)
    same(got, rhp.forward_sessions_cpu(res, sess, results, starts, route, len(fs.ROUTES), fs.FORWARD_MASK, names, extra), label)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4097])
def test_gpu_slot_counts(n):
    """n slots: sessions of up to five requests, every seventh request for the host (4097 crosses a scan tile of 4096)"""
    reqs = [fs.HOST if k % 7 == 3 else fs.HEAD if k % 5 == 2 else fs.post(k % 9) if k % 3 == 0 else fs.GET for k in range(n)]
    # (a body at a session's end would be a piece of its own: a session ends on a request without one)
    chunks = [reqs[k: k + 5] for k in range(0, n, 5)]
    sessions = [b"".join(c[:-1] + [fs.GET if c[-1].startswith(b"POST") else c[-1]]) for c in chunks]
    got = gpu_equals_twin(sessions, f"{n} slots", layout=H if n % 2 else R)
    assert len(got[1]) == n and int(got[3][-1]) == n - len([k for k in range(n) if k % 7 == 3])


@pytest.mark.gpu
@pytest.mark.parametrize("counts", [(33,), (32,), (64,), (20, 12), (40, 24), (50, 30, 60, 3, 70), (31, 1, 31, 2, 63, 65)],
                         ids=lambda c: "-".join(str(x) for x in c))
def test_gpu_forwarded_ordinals_across_word_edges(counts):
    """sessions of `counts` forwarded requests, HEADs among them, a host request between the sessions' runs: ordinals
    that cross a 32-bit word inside a session, words shared by two waves, totals of exactly 32 and 64"""
    sessions = [b"".join(fs.HEAD if (k * 7 + s) % 3 == 0 else fs.GET for k in range(c)) + fs.HOST for s, c in enumerate(counts)]
    got = gpu_equals_twin(sessions, f"counts {counts}")
    assert np.diff(got[3]).tolist() == list(counts) and len(got[4]) == (sum(counts) + 31) // 32
    want_bits = [q for q, h in enumerate(h for s, c in enumerate(counts) for h in ((k * 7 + s) % 3 == 0 for k in range(c))) if h]
    assert [q for q in range(sum(counts)) if (int(got[4][q >> 5]) >> (q & 31)) & 1] == want_bits


@pytest.mark.gpu
def test_gpu_group_larger_than_the_stage():
    """one 20 KiB body in a group of 64 slots: the cooperative path, small requests before and behind it"""
    sessions = [fs.GET * 3 + fs.post(20 * 1024) + fs.HEAD + fs.post(100), fs.GET * 70]
    got = gpu_equals_twin(sessions, "a 20 KiB body")
    assert int(np.diff(got[0]).max()) > 20 * 1024
    gpu_equals_twin(sessions, "a 20 KiB body, 128 extra bytes", extra=fs.EXTRA_128, layout=H)


@pytest.mark.gpu
def test_gpu_equals_twin_on_a_random_mix():
    """512 sessions drawn from the cases' requests by a fixed seed"""
    rng = np.random.default_rng(20261021)
    pool = (fs.GET, fs.TFB, fs.post(0), fs.post(1), fs.post(300), fs.CHUNKED, fs.CHUNKED_EMPTY, fs.NO_FRAMING, fs.HEAD, fs.LOWER_HEAD,
            fs.DROPS, fs.STATIC, fs.HOST, fs.NOWHERE, fs.FOLD, fs.CL_SPLIT)
    tails = (b"", b"", b"", fs.PARTIAL, fs.BAD)
    sessions = [b"".join(pool[int(k)] for k in rng.integers(0, len(pool), size=int(rng.integers(0, 9)))) + tails[int(rng.integers(0, len(tails)))]
                for _ in range(512)]
    for layout in fs.LAYOUTS:
        got = gpu_equals_twin(sessions, f"mix, {LAYOUT_IDS[layout]}", layout=layout)
        assert len(set(got[1].tolist())) >= 6, "the mix reaches six why codes at least"


@pytest.mark.gpu
def test_gpu_empty_calls():
    eb, eoff, es, _ = rhp.pack_sessions([])
    out_off, why, out, fwd_off, bits = rhp.forward_sessions_gpu(eb, eoff, es, fs.ROUTES, fs.FORWARD_MASK, guard=512)
    assert out_off.tolist() == [0] and fwd_off.tolist() == [0] and len(bits) == 0
    buf, off, sess = fs.packed("gets")
    out_off, why, out, fwd_off, bits = rhp.forward_sessions_gpu(buf, off, sess[:0], fs.ROUTES, fs.FORWARD_MASK, guard=512)
    assert out_off.tolist() == [0] and fwd_off.tolist() == [0] and len(bits) == 0


@pytest.mark.gpu
def test_gpu_queue_feeds_walk_answers():
    for name in ("heads", "mixed"):
        check_hand_over(name, fs.forward_gpu(name), rhp.walk_answers_gpu)


@pytest.mark.gpu
def test_gpu_details_are_the_round_as_the_gpu_left_it():
    """details=True: behind the five outputs (Result, session results, req_start, route), against the host's round.
    The smallest input with every kind of session: two pipelined complete requests, one incomplete request, no bytes"""
    buf, off, sess, _ = rhp.pack_sessions([fs.post(3) + fs.GET, fs.PARTIAL, b""])
    n = len(off) - 1
    got = rhp.forward_sessions_gpu(buf, off, sess, fs.ROUTES, fs.FORWARD_MASK, fs.DROP, fs.VIA, 4, guard=64, details=True)
    assert len(got) == 9
    wres, wresults, wstarts, wroute = fs.host_round_of(buf, off, sess, 4)
    same(got[:5], rhp.forward_sessions_cpu(wres, sess, wresults, wstarts, wroute, len(fs.ROUTES), fs.FORWARD_MASK, fs.DROP, fs.VIA), "details")
    res, results, starts, route = got[5:]
    assert results.tolist() == wresults.tolist() and results["n_slots"].tolist() == [2, 1, 0]
    assert len(starts) == len(route) == n
    ready = np.flatnonzero(wres.http["result"] == 1)   # (of a slot that is not ready only the http result means anything)
    assert ready.tolist() == [0, 1] and (res.http["result"] == wres.http["result"]).all()
    assert (starts[ready] == wstarts[ready]).all() and (route[ready] == wroute[ready]).all() and route[ready].tolist() == [0, 0]
    assert (res.http[ready] == wres.http[ready]).all()
    for f in ("ret", "method_len", "path_off", "path_len", "method_off", "minor_version", "num_headers"):
        assert (res.reqs[f][ready] == wres.reqs[f][ready]).all(), f
