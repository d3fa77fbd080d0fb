"""rhp_reply_sessions (include/rhp.h): the replies of static routes made on the
device from route[] and the fix-up's session results.

The yardstick is tests/golden/reply_sessions.npz: the compiled reference's
boundaries, results and routes, the leading-run and -1 rules in Python, and the
reference's own http_write_response over the answered requests in session order
(tests/golden/make_golden_reply_sessions.py).  CPU tests hold the host twin
(rhp_cpu_reply_sessions, a sequential walk) to it over the records of the exact
parser and of the DFA emulation, with both fix-up walks, in both layouts; GPU
tests hold the kernels (a scan over the slots) to it and to the twin, with
replies, total, out and work holding 0xFF first and guarded on both sides.
Hand-built route arrays and image tables (expected: a Python concatenation)
cover what the sets cannot: images larger than the LDS stage, every alignment
of the images and of `out`, route values outside the table, and a batch past
the edge of the top scan's runs of tiles."""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import libreactorng_amd as rhp
import reply_session_sets as rss
from oracle_util import oracle_write_responses

LAYOUTS = (rhp.LAYOUT_REQUEST_MAJOR, rhp.LAYOUT_HEADER_MAJOR)
MAXH = rss.MAX_HEADERS
GUARD = 4096
POISON = rhp.REPLY_POISON


@functools.lru_cache(maxsize=None)
def images():
    """(images u8, image_off u64 [n_routes + 1]) of rss.responses(), by the oracle's http_write_response"""
    out, off = oracle_write_responses(*rss.responses())
    return out, off


def check(got, name, label):
    """(replies, total, out) against the fixture; out may be longer than total: the rest holds the poison"""
    replies, total, out = got
    count, out_len, want_total, sha, want_out = rss.expected(name)
    assert len(replies) == len(count), label
    assert (replies["count"] == count).all(), f"{label}: count, first at session {int(np.flatnonzero(replies['count'] != count)[0])}"
    assert (replies["out_len"] == out_len).all(), f"{label}: out_len"
    assert (replies["out_off"] == np.cumsum(out_len) - out_len).all(), f"{label}: out_off"
    assert (replies["reserved"] == 0).all(), label
    assert total == want_total, f"{label}: total {total}, want {want_total}"
    if want_out is not None:
        assert bytes(out[:total]) == bytes(want_out), f"{label}: bytes"
    assert hashlib.sha256(out[:total].tobytes()).hexdigest() == sha, f"{label}: the bytes of out"
    assert (out[total:] == POISON).all(), f"{label}: bytes written past total"


def cpu_round(name, emulate_dfa=False, prefix=False, layout=rhp.LAYOUT_REQUEST_MAJOR):
    """(Result, sessions, results, route) of a set parsed, fixed up and classified on the host"""
    buf, off, sess = rss.inputs(name)
    res, results, starts = rhp.fixup_cpu(buf, off, sess, MAXH, emulate_dfa, layout, prefix)
    _, route = rhp.classify_sessions_cpu(res, sess, results, starts, (), rss.ROUTES)
    return res, sess, results, route


@functools.lru_cache(maxsize=None)
def cpu_round_once(name):
    return cpu_round(name, True, True, rhp.LAYOUT_HEADER_MAJOR)


def twin(rnd, **kw):
    res, sess, results, route = rnd
    return rhp.reply_sessions_cpu(res, sess, results, route, *images(), rss.STATIC_MASK, **kw)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("emulate_dfa", [False, True])
@pytest.mark.parametrize("name", ["mixed", "shapes", "runs"])
def test_cpu_matches_reference(name, emulate_dfa, prefix, layout):
    check(twin(cpu_round(name, emulate_dfa, prefix, layout)), name, f"{name} dfa {emulate_dfa} prefix {prefix} layout {layout}")


@pytest.mark.parametrize("name", rss.GEOMETRY)
def test_cpu_geometry(name):
    check(twin(cpu_round_once(name)), name, name)


def test_sets_stop_for_every_cause():
    """what the sets are for (the issue's table): runs stopped by a host route, by a request with no route and by
    -1, some of the latter with static requests before"""
    res, sess, results, route = cpu_round_once("mixed")
    count = rss.expected("mixed")[0]
    assert len(sess) == 60 and int(count.sum()) == 25 and int(count.max()) == 4
    stop = [int(lo) + int(c) for (lo, _), c in zip(sess, count)]
    live = [(s, c) for s, c, k in zip(stop, count, results["n_slots"]) if c < k]
    last = np.array([int(lo) + int(k) - 1 for (lo, _), k in zip(sess, results["n_slots"])])
    minus1 = res.http["result"][last] == -1
    assert sum(route[s] == 1 for s, _ in live) >= 10 and minus1.sum() >= 10
    assert sum(route[int(lo)] in (0, 2) for (lo, _), m in zip(sess, minus1) if m) >= 3, "-1 sessions with static requests before"
    assert int(rss.expected("shapes")[0].sum()) == 3
    c_runs = rss.expected("runs")[0]   # (asserts count == L, or 0 behind a malformed stopper)
    assert any(st in rss.AFTER_STOP and L for (L, st, _), c in zip(rss.runs(), c_runs))


def test_cpu_out_one_byte_short():
    rnd = cpu_round_once("mixed")
    total = rss.expected("mixed")[2]
    replies, got_total, out = twin(rnd, out_size=total - 1)
    assert got_total == total and (out == POISON).all() and len(out) == total - 1
    full = twin(rnd)
    assert (replies == full[0]).all()


# ---------------------------------------------------------------------------
# hand-built route arrays and image tables; the expected answer is concat()


def concat(sess, n_slots, route, imgs, image_off, static_mask):
    """(count, out_len, out bytes): the leading run of static slots of every session, their images back to back.
    For sessions that did not end on -1 (the geometry sets: TFB GETs only)."""
    nr = len(image_off) - 1
    img = [bytes(imgs[int(image_off[r]): int(image_off[r + 1])]) for r in range(nr)]
    count, lens, parts = [], [], []
    for (lo, _), k in zip(sess, n_slots):
        c = 0
        while c < k and route[lo + c] < nr and (static_mask >> int(route[lo + c])) & 1:
            c += 1
        mine = [img[route[lo + q]] for q in range(c)]
        count.append(c)
        lens.append(sum(map(len, mine)))
        parts += mine
    return np.array(count), np.array(lens, dtype=np.uint64), b"".join(parts)


def check_concat(got, want, label):
    replies, total, out = got
    count, lens, data = want
    assert (replies["count"] == count).all(), f"{label}: count"
    assert (replies["out_len"] == lens).all() and (replies["out_off"] == np.cumsum(lens) - lens).all(), f"{label}: out_len / out_off"
    assert (replies["reserved"] == 0).all() and total == len(data), f"{label}: total {total}, want {len(data)}"
    assert bytes(out[:total]) == data, f"{label}: bytes"
    assert (out[total:] == POISON).all(), f"{label}: bytes written past total"


def big_routes(name):
    n = len(rss.inputs(name)[1]) - 1
    if name == "geom_one_257":   # the big image among the small ones, in a run across two tiles
        return np.array([3 if q % 5 == 0 else 2 if q % 3 == 0 else 0 for q in range(n)], dtype=np.uint16)
    return np.full(n, 3, dtype=np.uint16)


BIG_CASES = ("geom_one_1", "geom_one_64", "geom_one_65", "geom_split_65", "geom_one_257")


@pytest.mark.parametrize("name", BIG_CASES)
def test_cpu_big_image(name):
    """route 3's 20 000-byte image in runs of 1, 64 and 65: a wave's run exceeds any LDS stage"""
    res, sess, results, _ = cpu_round_once(name)
    route = big_routes(name)
    got = rhp.reply_sessions_cpu(res, sess, results, route, *images(), rss.STATIC_MASK)
    check_concat(got, concat(sess, results["n_slots"], route, *images(), rss.STATIC_MASK), name)


ALIGN_LENS = (0, 1, 3, 15, 16, 17, 126)
ALIGN_SET = "geom_one_257"


@functools.lru_cache(maxsize=None)
def align_table(a):
    """hand-made images of ALIGN_LENS, the first one at byte `a` of the buffer; a route per slot of ALIGN_SET"""
    rng = np.random.default_rng(99)
    off = a + np.cumsum((0,) + ALIGN_LENS).astype(np.uint64)
    imgs = rng.integers(1, 255, size=int(off[-1]) + 5, dtype=np.uint8)
    n = len(rss.inputs(ALIGN_SET)[1]) - 1
    route = rng.integers(0, len(ALIGN_LENS), size=n).astype(np.uint16)
    return imgs, off, route


def test_cpu_alignments():
    res, sess, results, _ = cpu_round_once(ALIGN_SET)
    mask = (1 << len(ALIGN_LENS)) - 1
    for a in range(16):
        imgs, off, route = align_table(a)
        want = concat(sess, results["n_slots"], route, imgs, off, mask)
        for shift in range(16):
            got = rhp.reply_sessions_cpu(res, sess, results, route, imgs, off, mask, out_shift=shift)
            check_concat(got, want, f"images at {a}, out at {shift}")


ODD_ROUTES = (len(rss.ROUTES), 0xFFFE, rhp.ROUTE_NONE, 1)   # (1: in the table, not in the mask)


def odd_routes(n, value):
    route = np.zeros(n, dtype=np.uint16)
    route[10::7] = value
    return route


@pytest.mark.parametrize("value", ODD_ROUTES)
@pytest.mark.parametrize("name", ["geom_one_65", "geom_split_65"])
def test_cpu_routes_outside_the_table(name, value):
    """a route value at or above n_routes in the middle of a run stops it and never indexes image_off"""
    res, sess, results, _ = cpu_round_once(name)
    route = odd_routes(len(rss.inputs(name)[1]) - 1, value)
    got = rhp.reply_sessions_cpu(res, sess, results, route, *images(), rss.STATIC_MASK)
    want = concat(sess, results["n_slots"], route, *images(), rss.STATIC_MASK)
    assert want[0].sum() == (10 if name == "geom_one_65" else 65 - 8)
    check_concat(got, want, f"{name} route {value:#x}")


# a batch past the edge of the top scan's runs of tiles (1024 tiles of 256 slots): records made by hand
WIDE_N = 1024 * 256 + 257
WIDE_LENS = (0, 1, 3, 17)
WIDE_MASK = 0b1011


@functools.lru_cache(maxsize=None)
def wide():
    """(http records, sessions, results, route, images, image_off, expected): sessions of 1 to 70 000 slots in
    turn, half of the slots static, the session across slot 262 144 answered whole, a 70 000-slot one ended on -1"""
    rng = np.random.default_rng(7)
    sizes, at = [], 0
    while at < WIDE_N:
        k = min((1, 300, 70000, 64, 5)[len(sizes) % 5], WIDE_N - at)
        sizes.append(k)
        at += k
    lo = np.cumsum([0] + sizes[:-1])
    sess = np.zeros(len(sizes), dtype=rhp.SESSION_DTYPE)
    sess["piece_lo"], sess["piece_hi"] = lo, lo + sizes
    results = np.zeros(len(sizes), dtype=rhp.SESSION_RESULT_DTYPE)
    results["n_slots"] = sizes
    route = rng.choice(np.array([0, 1, 3, 2, rhp.ROUTE_NONE], dtype=np.uint16), size=WIDE_N, p=[0.5, 0.3, 0.1997, 0.0002, 0.0001])
    across = int(np.flatnonzero((lo <= 262144) & (lo + sizes > 262144))[0])
    route[lo[across]: lo[across] + sizes[across]] = 0
    http = np.zeros(WIDE_N, dtype=rhp.HTTP_DTYPE)
    http["result"] = 1
    dead = across - 5   # a 70 000-slot session
    http["result"][lo[dead] + sizes[dead] - 1] = -1
    off = np.cumsum((0,) + WIDE_LENS).astype(np.uint64)
    imgs = rng.integers(1, 255, size=int(off[-1]), dtype=np.uint8)
    n_slots = results["n_slots"].copy()
    n_slots[dead] = 0   # (concat: it answers nothing)
    want = concat(sess, n_slots, route, imgs, off, WIDE_MASK)
    assert want[0][across] == sizes[across] > 40000 and sizes[dead] == 70000 and want[0][dead] == 0 and 0 < want[0].sum() < WIDE_N // 2
    return http, sess, results, route, imgs, off, want


def test_cpu_past_the_top_scan_edge():
    http, sess, results, route, imgs, off, want = wide()
    dummy = np.zeros(32, dtype=np.uint8)
    at = dummy.ctypes.data + (-dummy.ctypes.data) % 16
    b = rhp.Batch(at, at, at, 16, WIDE_N, 0, rhp.MODE_HTTP, rhp.LAYOUT_REQUEST_MAJOR, at, None, http.ctypes.data, None,
                  rhp.BATCH_SPECULATIVE, 0, None)
    check_concat(rhp.reply_sessions_cpu(b, sess, results, route, imgs, off, WIDE_MASK), want, "wide")


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls go to
    the GPU library here: an accepted one would launch kernels over host memory"""
    gpu = which == "gpu-library"
    if gpu:
        fn = lambda b, s, k, r, q, t, o: rhp.lib().rhp_reply_sessions(b, s, k, r, q, t, o, None)
    else:
        fn = lambda b, s, k, r, q, t, o: rhp.host().rhp_cpu_reply_sessions(b, s, k, r, q, t, o)
    buf, off, sess = rss.inputs("shapes")
    n = len(off) - 1
    b0, res = rhp._host_batch(buf, off, MAXH, rhp.MODE_HTTP, rhp.LAYOUT_REQUEST_MAJOR, None, rhp.BATCH_SPECULATIVE)
    results = np.zeros(len(sess), dtype=rhp.SESSION_RESULT_DTYPE)
    route = np.full(n, rhp.ROUTE_NONE, dtype=np.uint16)
    imgs, ioff = images()
    replies = np.zeros(len(sess), dtype=rhp.SESSION_REPLY_DTYPE)
    total = np.full(1, 77, dtype=np.uint64)
    out = np.zeros(64, dtype=np.uint8)
    work = np.zeros(rhp.reply_work_words(n, len(sess)), dtype=np.uint64)
    p = lambda a: a.ctypes.data

    def call(patch_b=None, patch_t=None, patch_o=None, n_sessions=len(sess), sessions=p(sess), res_p=p(results),
             route_p=p(route), accepted=False):
        assert not (gpu and accepted)
        b = rhp.Batch.from_buffer_copy(b0)
        t = rhp.ReplyTable(p(imgs), p(ioff), len(ioff) - 1, rss.STATIC_MASK)
        o = rhp.ReplyOut(p(replies), p(total), p(out), out.size, p(work))
        for patch, x in ((patch_b, b), (patch_t, t), (patch_o, o)):
            if patch:
                patch(x)
        return fn(ctypes.byref(b), sessions, n_sessions, res_p, route_p, ctypes.byref(t), ctypes.byref(o))

    E = -22
    zero = lambda b: setattr(b, "n", 0)
    assert fn(None, None, 0, None, None, None, None) == E
    # what rhp_classify_sessions refuses about the batch, the sessions and the results
    assert call(patch_b=lambda b: setattr(b, "mode", rhp.MODE_PHR)) == E
    assert call(patch_b=lambda b: setattr(b, "flags", 0)) == E
    assert call(patch_b=lambda b: (zero(b), setattr(b, "flags", 0))) == E
    assert call(patch_b=lambda b: setattr(b, "flags", rhp.BATCH_SPECULATIVE | 2)) == E
    for layout in (rhp.LAYOUT_DENSE, rhp.LAYOUT_COMPACT, rhp.LAYOUT_DENSE_RM, 5):
        assert call(patch_b=lambda b: setattr(b, "layout", layout)) == E
        assert call(patch_b=lambda b: (zero(b), setattr(b, "layout", layout))) == E
    assert call(res_p=None) == E
    assert call(sessions=None) == E
    assert call(patch_b=lambda b: setattr(b, "max_headers", rhp.RHP_MAX_HEADERS + 1)) == E
    assert call(patch_b=lambda b: setattr(b, "reqs", None)) == E
    assert call(patch_b=lambda b: setattr(b, "http", None)) == E
    # the call's own
    assert call(route_p=None) == E
    assert call(patch_t=lambda t: setattr(t, "image_off", None)) == E
    assert call(patch_t=lambda t: setattr(t, "n_routes", 0)) == E
    assert call(patch_t=lambda t: setattr(t, "n_routes", rhp.CLASSIFY_MAX_ROUTES + 1)) == E
    for f in ("replies", "total", "work", "out"):
        assert call(patch_o=lambda o: setattr(o, f, None)) == E, f
    b = rhp.Batch.from_buffer_copy(b0)
    t = rhp.ReplyTable(p(imgs), p(ioff), len(ioff) - 1, rss.STATIC_MASK)
    o = rhp.ReplyOut(p(replies), p(total), p(out), out.size, p(work))
    assert fn(ctypes.byref(b), p(sess), len(sess), p(results), p(route), None, ctypes.byref(o)) == E
    assert fn(ctypes.byref(b), p(sess), len(sess), p(results), p(route), ctypes.byref(t), None) == E
    assert total[0] == 77 and not replies["count"].any(), "a refused call writes nothing"
    if gpu:
        return
    # the host twin: images may be NULL only when every image is empty; accepted calls
    assert call(patch_t=lambda t: setattr(t, "images", None)) == E
    empty = np.full(len(ioff), 5, dtype=np.uint64)
    assert call(patch_t=lambda t: (setattr(t, "images", None), setattr(t, "image_off", p(empty))), accepted=True) == 0
    assert call(patch_o=lambda o: (setattr(o, "out", None), setattr(o, "out_size", 0)), accepted=True) == 0
    assert call(patch_b=lambda b: setattr(b, "bytes_rw", None), accepted=True) == 0
    total[0] = 77
    assert call(n_sessions=0, sessions=None, res_p=None, accepted=True) == 0 and total[0] == 0   # *total = 0, nothing else
    replies[:] = (9, 9, 9, 9)
    assert call(patch_b=zero, accepted=True) == 0   # n == 0 with sessions: every count 0
    assert not replies["count"].any() and not replies["out_len"].any() and not replies["out_off"].any() and total[0] == 0


# ---------------------------------------------------------------------------
# GPU: one round per case -- parse, fix-up, classify, the images, the replies, one stream


def gpu_case(name, impl=rhp.IMPL_DFA, layout=rhp.LAYOUT_REQUEST_MAJOR, against_twin=False, **kw):
    buf, off, sess = rss.inputs(name)
    total = rss.expected(name)[2]
    label = f"{name} impl{impl} layout {layout} {kw}"
    got = rhp.reply_sessions_gpu(buf, off, sess, (), rss.ROUTES, rss.responses(), rss.STATIC_MASK, MAXH, impl, layout,
                                 guard=GUARD, out_size=kw.pop("out_size", total), details=against_twin, **kw)
    check(got[:3], name, label + ": kernels against the reference")
    if against_twin:   # the twin over the records, session results and routes the GPU left
        res, results, route = got[3:]
        cpu = rhp.reply_sessions_cpu(res, sess, results, route, *images(), rss.STATIC_MASK)
        assert (cpu[0] == got[0]).all() and cpu[1] == got[1] and bytes(cpu[2]) == bytes(got[2][: got[1]]), label + ": kernels against the twin"


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
def test_gpu_mixed(impl, layout):
    gpu_case("mixed", impl, layout, out_shift=(impl * 7 + layout * 3) % 16)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_shapes(layout):
    gpu_case("shapes", layout=layout, out_shift=5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", rss.GEOMETRY)
def test_gpu_geometry(name):
    gpu_case(name, layout=rhp.LAYOUT_HEADER_MAJOR)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
def test_gpu_runs_kernel_is_twin(impl):
    gpu_case("runs", impl, against_twin=True, out_shift=9)


@pytest.mark.gpu
def test_gpu_out_one_byte_short():
    buf, off, sess = rss.inputs("mixed")
    count, out_len, total, *_ = rss.expected("mixed")
    replies, got_total, out = rhp.reply_sessions_gpu(buf, off, sess, (), rss.ROUTES, rss.responses(), rss.STATIC_MASK, MAXH,
                                                     guard=GUARD, out_size=total - 1)
    assert got_total == total and (out == POISON).all() and len(out) == total - 1
    assert (replies["count"] == count).all() and (replies["out_len"] == out_len).all()
    assert (replies["out_off"] == np.cumsum(out_len) - out_len).all()


@functools.lru_cache(maxsize=None)
def gpu_round(name):
    """a geometry set parsed and fixed up on the GPU: (batch descriptor, sessions, results) on the device, kept"""
    import torch
    buf, off, sess = rss.inputs(name)
    res, results, starts, db = rhp.fixup_gpu(buf, off, sess, MAXH, with_batch=True)
    ds = torch.from_numpy(np.ascontiguousarray(sess).view(np.uint8).copy()).to("cuda")
    dres = torch.from_numpy(np.ascontiguousarray(results).view(np.uint8).copy()).to("cuda")
    return db.desc(), ds, dres, sess, results, db


def gpu_hand(name, route, imgs, off, mask, out_size, shift=0):
    import torch
    d, ds, dres, sess, results, _ = gpu_round(name)
    padded = np.zeros((len(imgs) + 3) & ~3, dtype=np.uint8)   # readable to the next 4-byte boundary (rhp.h)
    padded[: len(imgs)] = imgs
    finish = rhp.reply_sessions_device(d, ds, len(sess), dres, torch.from_numpy(route.view(np.int16)).to("cuda"),
                                       torch.from_numpy(padded).to("cuda"),
                                       torch.from_numpy(np.ascontiguousarray(off).view(np.int64)).to("cuda"), mask, out_size,
                                       GUARD, shift)
    return finish()


@pytest.mark.gpu
@pytest.mark.parametrize("name", BIG_CASES)
def test_gpu_big_image(name):
    d, ds, dres, sess, results, _ = gpu_round(name)
    route = big_routes(name)
    want = concat(sess, results["n_slots"], route, *images(), rss.STATIC_MASK)
    check_concat(gpu_hand(name, route, *images(), rss.STATIC_MASK, len(want[2]), shift=3), want, name)


@pytest.mark.gpu
def test_gpu_alignments():
    d, ds, dres, sess, results, _ = gpu_round(ALIGN_SET)
    mask = (1 << len(ALIGN_LENS)) - 1
    for a in range(16):
        imgs, off, route = align_table(a)
        want = concat(sess, results["n_slots"], route, imgs, off, mask)
        for shift in range(16):
            check_concat(gpu_hand(ALIGN_SET, route, imgs, off, mask, len(want[2]), shift), want, f"images at {a}, out at {shift}")


@pytest.mark.gpu
@pytest.mark.parametrize("value", ODD_ROUTES)
@pytest.mark.parametrize("name", ["geom_one_65", "geom_split_65"])
def test_gpu_routes_outside_the_table(name, value):
    d, ds, dres, sess, results, _ = gpu_round(name)
    route = odd_routes(len(rss.inputs(name)[1]) - 1, value)
    want = concat(sess, results["n_slots"], route, *images(), rss.STATIC_MASK)
    check_concat(gpu_hand(name, route, *images(), rss.STATIC_MASK, len(want[2])), want, f"{name} route {value:#x}")


@pytest.mark.gpu
def test_gpu_past_the_top_scan_edge():
    import torch
    http, sess, results, route, imgs, off, want = wide()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    dhttp, dummy = dev(http), torch.zeros(512, dtype=torch.uint8, device="cuda")
    at = dummy.data_ptr()
    d = rhp.Batch(at, at, at, 16, WIDE_N, 0, rhp.MODE_HTTP, rhp.LAYOUT_REQUEST_MAJOR, at, None, dhttp.data_ptr(), None,
                  rhp.BATCH_SPECULATIVE, 0, None)
    padded = np.zeros((len(imgs) + 3) & ~3, dtype=np.uint8)
    padded[: len(imgs)] = imgs
    finish = rhp.reply_sessions_device(d, dev(sess), len(sess), dev(results), dev(route), dev(padded),
                                       torch.from_numpy(off.view(np.int64)).to("cuda"), WIDE_MASK,
                                       len(want[2]), GUARD, 11)
    check_concat(finish(), want, "wide")
