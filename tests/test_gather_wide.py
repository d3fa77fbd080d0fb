"""rhp_gather_wide (include/rhp.h): the records of a round's wide slots and its
de-framed chunked bodies in three contiguous areas.

The yardstick is statement(): the selection, header, body and order rules of
rhp.h written in numpy over the Result of a fix-up and the output of
pack_dense_cpu -- neither the host twin (rhp_cpu_gather_wide, a sequential walk)
nor the kernels (a scan over the slots).  On top of it the consumer's property:
rhp.rebuild_records, which sees only the dense copies, the session results and
the three areas, gives the batch's own request-major records for every in-use
slot (tests/test_sessions.py holds those to the reference's loop), and every
gathered body is the body the oracle's sequential http_read_request loop
returns for that request.  CPU tests run the twin over the exact parser's and
the DFA emulation's records with both fix-up walks; GPU tests run the kernels
over the GPU's own records, every output holding 0xFF first and guarded."""
import ctypes
import functools

import numpy as np
import pytest

import libreactorng_amd as rhp
import gather_sets as gs
from test_sessions import oracle_sessions

MAXH = gs.MAX_HEADERS
GUARD = 4096
POISON = rhp.WIDE_POISON
NO_BODY = rhp.WIDE_NO_BODY
REQ_FIELDS = ("ret", "method_len", "path_off", "path_len", "method_off", "minor_version", "num_headers")


def statement(res, off, sess, results, starts, dreq, hc, m=MAXH):
    """rhp.h's rules: (totals (n_wide, n_hdrs, body_bytes), slots WIDE_SLOT_DTYPE, hdrs HDR_DTYPE, body u8)"""
    n = len(off) - 1
    dq = np.ascontiguousarray(dreq).view(np.uint8)[: 8 * n].view(rhp.REQ_DENSE_DTYPE)
    c = np.ascontiguousarray(hc).view(np.uint8)[: 8 * n].view(rhp.HTTP_COMPACT_DTYPE)
    owner = np.full(n, -1, dtype=np.int64)
    for s, ((lo, hi), k) in enumerate(zip(sess.tolist(), results["n_slots"].tolist())):
        if lo <= lo + k <= hi <= n:
            owner[lo: lo + k] = s
    mark = ((c["flags"] & rhp.HTTP_WIDE) != 0) | ((c["result"] == 1) & ((dq["flags"] & rhp.DENSE_WIDE) != 0))
    wide = np.flatnonzero((owner >= 0) & mark)
    r, x = res.reqs[wide], res.http[wide]
    nh = np.where((x["result"] == 1) & (r["ret"] > 0) & (r["num_headers"] <= m), r["num_headers"], 0).astype(np.int64)
    ret64 = r["ret"].astype(np.int64).view(np.uint64)
    off = np.asarray(off, dtype=np.uint64)
    with np.errstate(over="ignore"):
        a = starts[wide].astype(np.uint64) + ret64
        s0, s1 = off[sess["piece_lo"][owner[wide]]], off[sess["piece_hi"][owner[wide]]]
        has = ((x["result"] == 1) & (x["body_kind"] == 1) & (x["consumed"] != ret64 + x["body_len"]) &
               (s0 <= a) & (a <= s1) & (x["body_len"] <= s1 - a))
    bl = np.where(has, x["body_len"], 0).astype(np.uint64)
    slots = np.zeros(len(wide), dtype=rhp.WIDE_SLOT_DTYPE)
    slots["slot"], slots["req"], slots["http"], slots["req_start"] = wide, r, x, starts[wide]
    slots["hdr_first"] = np.cumsum(nh) - nh
    slots["body_off"] = np.where(has, np.cumsum(bl) - bl, np.uint64(NO_BODY))
    hdrs = [res.hdrs[i, :k] for i, k in zip(wide.tolist(), nh.tolist()) if k]
    hdrs = np.concatenate(hdrs) if hdrs else np.zeros(0, dtype=rhp.HDR_DTYPE)
    body = [res.bytes_out[int(p): int(p) + int(k)] for p, k, h in zip(a.tolist(), bl.tolist(), has.tolist()) if h]
    body = np.concatenate(body) if body else np.zeros(0, dtype=np.uint8)
    return (len(wide), int(nh.sum()), int(bl.sum())), slots, hdrs, body


def check(got, want, label, caps=None):
    """the four outputs against statement(); beyond the used part an area still holds the poison"""
    totals, slots, hdrs, body = got
    (nw, nhd, nb), wslots, whdrs, wbody = want
    assert (int(totals["n_wide"]), int(totals["n_hdrs"]), int(totals["body_bytes"])) == (nw, nhd, nb), f"{label}: totals"
    bad = np.flatnonzero(slots[:nw] != wslots)
    assert not len(bad), f"{label}: slot record {int(bad[0])}: got {slots[bad[0]]}, want {wslots[bad[0]]}"
    assert (hdrs[:nhd] == whdrs).all(), f"{label}: header records"
    assert bytes(body[:nb]) == bytes(wbody), f"{label}: body bytes"
    for name, a, used in (("slots", slots, nw), ("hdrs", hdrs, nhd), ("body", body, nb)):
        assert (a[used:].view(np.uint8) == POISON).all(), f"{label}: {name} written past its total"


def untouched(got, label):
    for name, a in zip(("slots", "hdrs", "body"), got[1:]):
        assert (a.view(np.uint8) == POISON).all(), f"{label}: {name} written though the totals do not fit"


@functools.lru_cache(maxsize=None)
def cpu_round(name, emulate_dfa=False, prefix=False):
    """(Result, results, starts, dreq, hc, lens16) of a set parsed, fixed up and packed on the host"""
    buf, off, sess = gs.inputs(name)
    res, results, starts = rhp.fixup_cpu(buf, off, sess, MAXH, emulate_dfa, rhp.LAYOUT_REQUEST_MAJOR, prefix)
    return (res, results, starts) + rhp.pack_dense_cpu(res, len(off) - 1, MAXH)


@functools.lru_cache(maxsize=None)
def oracle_bodies(name):
    """{slot: body} of the requests the oracle's sequential loop returns, with their Transfer-Encoding fields"""
    buf, off, sess = gs.inputs(name)
    want, _ = oracle_sessions(buf, off, [(int(a), int(b)) for a, b in sess], MAXH)
    out = {}
    for (lo, _), seq in zip(sess.tolist(), want):
        for q, rec in enumerate(seq):
            if rec[0] == 1:
                out[lo + q] = (rec[6], any(nm.upper() == b"TRANSFER-ENCODING" for nm, _ in rec[5]))
    return out


def check_consumer(name, got, rnd, label):
    """rebuild_records over the dense copies and the gathered areas alone: the batch's records, the oracle's bodies"""
    buf, off, sess = gs.inputs(name)
    res, results, starts, dreq, hc, lens = rnd
    n = len(off) - 1
    rb = rhp.rebuild_records(n, MAXH, sess, results, dreq, hc, lens, *got)
    use = np.flatnonzero(rb["in_use"])
    assert (rb["http"]["result"][use] == res.http["result"][use]).all(), f"{label}: http results"
    ready = use[res.http["result"][use] == 1]
    for f in REQ_FIELDS:
        assert (rb["reqs"][f][ready] == res.reqs[f][ready]).all(), f"{label}: req.{f}"
    assert (rb["http"][ready] == res.http[ready]).all(), f"{label}: http records"
    valid = np.arange(MAXH)[None, :] < res.reqs["num_headers"][ready][:, None]
    assert (rb["hdrs"][ready][valid] == res.hdrs[ready][valid]).all(), f"{label}: header records"
    for i, at in rb["req_start"].items():
        assert at == int(starts[i]), f"{label}: req_start of slot {i}"
    want = oracle_bodies(name)
    owned = {lo + q for (lo, _), k in zip(sess.tolist(), results["n_slots"].tolist()) for q in range(k)}
    for i, b in rb["bodies"].items():
        assert i in want and b == want[i][0], f"{label}: body of slot {i}"
    for i, (b, te) in want.items():
        if te and i in owned:
            assert i in rb["bodies"], f"{label}: the chunked body of slot {i} was not gathered"
    return rb


# ---------------------------------------------------------------------------
# CPU


def test_sets_hold_what_they_are_for():
    buf, off, sess = gs.inputs("causes")
    res, results, starts, dreq, hc, _ = cpu_round("causes")
    n = len(off) - 1
    (nw, _, _), slots, _, _ = statement(res, off, sess, results, starts, dreq, hc)
    wide = set(slots["slot"].tolist())
    used = np.zeros(n, dtype=bool)
    for (lo, _), k in zip(sess.tolist(), results["n_slots"].tolist()):
        used[lo: lo + k] = True
    target = {}
    for i in np.flatnonzero(used & (res.http["result"] == 1)).tolist():
        a = int(starts[i]) + int(res.reqs["path_off"][i])
        target.setdefault(bytes(buf[a: a + int(res.reqs["path_len"][i])]), []).append(i)
    for cause in gs.CAUSES:
        w, d = target[b"/w-" + cause.encode()], target[b"/d-" + cause.encode()]
        assert len(w) >= 5 and all(i in wide for i in w), f"{cause}: wide slots {len(w)}"
        assert len(d) >= 5 and not any(i in wide for i in d), f"{cause}: the request just inside the limit is dense"
    dq, c = dreq.view(rhp.REQ_DENSE_DTYPE), hc.view(rhp.HTTP_COMPACT_DTYPE)
    mark = ((c["flags"] & rhp.HTTP_WIDE) != 0) | ((c["result"] == 1) & ((dq["flags"] & rhp.DENSE_WIDE) != 0))
    assert int((mark & ~used).sum()) >= 20, "unused slots with a wide mark"
    last = [int(lo) + int(k) - 1 for (lo, _), k in zip(sess.tolist(), results["n_slots"].tolist()) if k]
    for _, code in gs.STOPS.values():
        stopped = [i for i in last if res.http["result"][i] == code and i - 1 in wide and i - 2 in wide]
        assert len(stopped) >= gs.STOP_SESSIONS, f"sessions that stop on {code} behind wide slots"
    assert int(results["more"].sum()) >= 1
    assert int((slots["body_off"] != NO_BODY).sum()) >= 10


@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("emulate_dfa", [False, True])
@pytest.mark.parametrize("name", ["causes", "mixed", "shapes"])
def test_cpu_twin_is_the_statement(name, emulate_dfa, prefix):
    buf, off, sess = gs.inputs(name)
    rnd = cpu_round(name, emulate_dfa, prefix)
    res, results, starts, dreq, hc, _ = rnd
    label = f"{name} dfa {emulate_dfa} prefix {prefix}"
    got = rhp.gather_wide_cpu(res, sess, results, starts, dreq, hc, body_shift=3)
    check(got, statement(res, off, sess, results, starts, dreq, hc), label)
    check_consumer(name, got, rnd, label)


@pytest.mark.parametrize("name", ["geom_split_65_all", "geom_one_257_last", "geom_one_64_none", "bodies_path3", "bodies_big"])
def test_cpu_geometry_and_bodies(name):
    buf, off, sess = gs.inputs(name)
    rnd = cpu_round(name, True, True)
    res, results, starts, dreq, hc, _ = rnd
    got = rhp.gather_wide_cpu(res, sess, results, starts, dreq, hc)
    check(got, statement(res, off, sess, results, starts, dreq, hc), name)
    check_consumer(name, got, rnd, name)


def test_cpu_caps():
    """each cap one short: totals exact, every area still all 0xFF; the exact caps; generous caps"""
    buf, off, sess = gs.inputs("causes")
    res, results, starts, dreq, hc, _ = cpu_round("causes")
    want = statement(res, off, sess, results, starts, dreq, hc)
    exact = want[0]
    assert all(exact)
    for k in range(3):
        caps = tuple(c - (q == k) for q, c in enumerate(exact))
        got = rhp.gather_wide_cpu(res, sess, results, starts, dreq, hc, caps=caps)
        assert (int(got[0]["n_wide"]), int(got[0]["n_hdrs"]), int(got[0]["body_bytes"])) == exact
        untouched(got, f"cap {k} one short")
    check(rhp.gather_wide_cpu(res, sess, results, starts, dreq, hc, caps=exact), want, "exact caps")
    check(rhp.gather_wide_cpu(res, sess, results, starts, dreq, hc, caps=(exact[0] + 3, exact[1] + 9, exact[2] + 17)), want, "roomy")


def _arguments(name="shapes"):
    buf, off, sess = gs.inputs(name)
    n = len(off) - 1
    b0, _ = rhp._host_batch(buf, off, MAXH, rhp.MODE_HTTP, rhp.LAYOUT_REQUEST_MAJOR, None, rhp.BATCH_SPECULATIVE)
    return b0, sess, n


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls go to
    the GPU library here: an accepted one would launch kernels over host memory"""
    gpu = which == "gpu-library"
    if gpu:
        fn = lambda b, s, k, r, st, dq, c, o: rhp.lib().rhp_gather_wide(b, s, k, r, st, dq, c, o, None)
    else:
        fn = lambda b, s, k, r, st, dq, c, o: rhp.host().rhp_cpu_gather_wide(b, s, k, r, st, dq, c, o)
    b0, sess, n = _arguments()
    results = np.zeros(len(sess), dtype=rhp.SESSION_RESULT_DTYPE)
    starts = np.zeros(n, dtype=np.uint64)
    dreq, hc = np.zeros(8 * n, dtype=np.uint8), np.zeros(8 * n, dtype=np.uint8)
    totals = np.full(2, 77, dtype=np.uint64)
    raw = np.full(64 * 8 + 32, POISON, dtype=np.uint8)
    slots = raw[(-raw.ctypes.data) % 16:][: 64 * 8]
    hdrs, body = np.full(8 * 8, POISON, dtype=np.uint8), np.full(64, POISON, dtype=np.uint8)
    work = np.zeros(rhp.wide_work_words(n), dtype=np.uint64)
    p = lambda a: a.ctypes.data

    def call(patch_b=None, patch_o=None, n_sessions=len(sess), sessions=p(sess), res_p=p(results), st_p=p(starts),
             dq_p=p(dreq), hc_p=p(hc), accepted=False):
        assert not (gpu and accepted)
        b = rhp.Batch.from_buffer_copy(b0)
        o = rhp.WideOut(p(totals), p(slots), 8, p(hdrs), 8, p(body), 64, p(work))
        for patch, x in ((patch_b, b), (patch_o, o)):
            if patch:
                patch(x)
        return fn(ctypes.byref(b), sessions, n_sessions, res_p, st_p, dq_p, hc_p, ctypes.byref(o))

    E = -22
    zero = lambda b: setattr(b, "n", 0)
    assert fn(None, None, 0, None, None, None, None, None) == E
    # what rhp_classify_sessions and rhp_pack_dense refuse about the batch, the sessions and the results
    assert call(patch_b=lambda b: setattr(b, "mode", rhp.MODE_PHR)) == E
    assert call(patch_b=lambda b: setattr(b, "flags", 0)) == E
    assert call(patch_b=lambda b: setattr(b, "flags", rhp.BATCH_SPECULATIVE | 2)) == E
    for layout in (rhp.LAYOUT_HEADER_MAJOR, rhp.LAYOUT_DENSE, rhp.LAYOUT_COMPACT, rhp.LAYOUT_DENSE_RM, 5):
        assert call(patch_b=lambda b: setattr(b, "layout", layout)) == E
        assert call(patch_b=lambda b: (zero(b), setattr(b, "layout", layout))) == E
    assert call(res_p=None) == E
    assert call(sessions=None) == E
    assert call(st_p=None) == E
    assert call(patch_b=lambda b: setattr(b, "max_headers", rhp.RHP_MAX_HEADERS + 1)) == E
    for f in ("reqs", "http", "hdrs", "offsets", "bytes"):
        assert call(patch_b=lambda b: setattr(b, f, None)) == E, f
    # the call's own
    assert call(dq_p=None) == E and call(hc_p=None) == E
    for f in ("totals", "work", "slots", "hdrs", "body"):
        assert call(patch_o=lambda o: setattr(o, f, None)) == E, f
    assert call(patch_o=lambda o: setattr(o, "slots", p(slots) + 8)) == E
    assert call(patch_o=lambda o: setattr(o, "hdrs", p(hdrs) + 4)) == E
    b = rhp.Batch.from_buffer_copy(b0)
    assert fn(ctypes.byref(b), p(sess), len(sess), p(results), p(starts), p(dreq), p(hc), None) == E
    assert totals[0] == 77 and (slots == POISON).all(), "a refused call writes nothing"
    if gpu:
        return
    # accepted by the host twin: NULL areas with cap 0, no bytes_rw, no session, no slot
    none = lambda o: [setattr(o, f, None) for f in ("slots", "hdrs", "body")] + [setattr(o, f, 0) for f in ("cap_slots", "cap_hdrs", "cap_body")]
    assert call(patch_o=none, accepted=True) == 0 and totals[0] == 0 and totals[1] == 0
    assert call(patch_b=lambda b: setattr(b, "bytes_rw", None), accepted=True) == 0
    totals[:] = 77
    assert call(n_sessions=0, sessions=None, res_p=None, st_p=None, accepted=True) == 0 and not totals.any()
    totals[:] = 77
    assert call(patch_b=zero, accepted=True) == 0 and not totals.any()
    assert (slots == POISON).all() and (hdrs == POISON).all() and (body == POISON).all()


# ---------------------------------------------------------------------------
# GPU: one round per case -- parse, fix-up, pack, gather, one stream


@functools.lru_cache(maxsize=None)
def gpu_round(name, impl=rhp.IMPL_DFA):
    """a set parsed, fixed up and packed on the GPU, kept there: (descriptor, device sessions, results, starts,
    dreq, hc, the host copies (Result, results, starts, dreq, hc, lens16), keep-alive)"""
    import torch
    buf, off, sess = gs.inputs(name)
    res, results, starts, db = rhp.fixup_gpu(buf, off, sess, MAXH, impl, with_batch=True, guard=GUARD)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    packed = rhp.pack_dense_device(db, GUARD)
    torch.cuda.synchronize()
    n = db.n
    dreq, hc, lens = (x.view.cpu().numpy() for x in packed)
    host = (res, results, starts, dreq[: 8 * n], hc[: 8 * n], lens.view(np.uint16)[: MAXH * n])
    return db.desc(), dev(sess), dev(results), dev(starts), packed[0].view, packed[1].view, host, (db, packed)


def gpu_gather(name, impl=rhp.IMPL_DFA, caps=None, body_shift=0, sess_t=None):
    d, ds, dres, dst, ddq, dhc, host, keep = gpu_round(name, impl)
    ns = len(gs.inputs(name)[2])
    if caps is None:
        caps = statement(host[0], gs.inputs(name)[1], gs.inputs(name)[2], *host[1:5])[0]
    got = rhp.gather_wide_device(d, ds if sess_t is None else sess_t[0], ns, dres if sess_t is None else sess_t[1], dst,
                                 ddq, dhc, caps, GUARD, body_shift)()
    keep[0].check_guards()
    for x in keep[1]:
        x.check()
    return got, host


def gpu_case(name, impl=rhp.IMPL_DFA, twin=False, consumer=True, **kw):
    buf, off, sess = gs.inputs(name)
    got, host = gpu_gather(name, impl, **kw)
    res, results, starts, dreq, hc, _ = host
    label = f"{name} impl{impl} {kw}"
    check(got, statement(res, off, sess, results, starts, dreq, hc), label + ": kernels against the statement")
    if twin:
        cpu = rhp.gather_wide_cpu(res, sess, results, starts, dreq, hc)
        assert got[0] == cpu[0] and (got[1] == cpu[1]).all() and (got[2] == cpu[2]).all() and (got[3] == cpu[3]).all(), \
            label + ": kernels against the twin"
    if consumer:
        check_consumer(name, got, host, label)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
@pytest.mark.parametrize("name", ["causes", "mixed", "shapes"])
def test_gpu_sets(name, impl):
    gpu_case(name, impl, twin=True, body_shift=5 + impl)


@pytest.mark.gpu
@pytest.mark.parametrize("name", gs.GEOMETRY)
def test_gpu_geometry(name):
    gpu_case(name, consumer=name.endswith("_65_all") or name.endswith("_257_last"))


@pytest.mark.gpu
def test_gpu_past_the_top_scan_edge():
    """gs.TOP_EDGE + 65 slots: rhp_gather_top_kernel gives a thread two waves' sums"""
    gpu_case("top_edge", consumer=False)


@pytest.mark.gpu
@pytest.mark.parametrize("name", gs.BODIES)
def test_gpu_bodies_every_alignment(name):
    """de-framed lengths 0..33 back to back (every destination alignment) behind paths of 1..16 bytes (every source one)"""
    gpu_case(name, twin=True)


@pytest.mark.gpu
def test_gpu_big_bodies():
    """4095, 4096, 4097 bytes and 100 KB of 1 KiB chunks, `body` at every alignment: the 16-byte path of the copy
    (it stages nothing in LDS)"""
    gpu_case("bodies_big", twin=True)
    buf, off, sess = gs.inputs("bodies_big")
    for shift in range(1, 16):
        got, host = gpu_gather("bodies_big", body_shift=shift)
        check(got, statement(host[0], off, sess, *host[1:5]), f"body at {shift}")


@pytest.mark.gpu
def test_gpu_caps():
    buf, off, sess = gs.inputs("causes")
    _, host = gpu_gather("causes")
    want = statement(host[0], off, sess, *host[1:5])
    exact = want[0]
    for k in range(3):
        caps = tuple(c - (q == k) for q, c in enumerate(exact))
        got, _ = gpu_gather("causes", caps=caps)
        assert (int(got[0]["n_wide"]), int(got[0]["n_hdrs"]), int(got[0]["body_bytes"])) == exact
        untouched(got, f"cap {k} one short")
    got, _ = gpu_gather("causes", caps=(0, 0, 0))   # NULL areas: the totals-only call
    assert (int(got[0]["n_wide"]), int(got[0]["n_hdrs"]), int(got[0]["body_bytes"])) == exact


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["causes", "mixed", "geom_split_257_all"])
def test_gpu_sessions_reversed(name):
    """against the contract: only the guards and n_wide <= n are checked"""
    import torch
    buf, off, sess = gs.inputs(name)
    d, ds, dres, dst, ddq, dhc, host, keep = gpu_round(name)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    rev = (dev(sess[::-1]), dev(host[1][::-1]))
    n = len(off) - 1
    for caps in ((n, n * MAXH, int(off[-1])), statement(host[0], off, sess, *host[1:5])[0]):
        got, _ = gpu_gather(name, caps=caps, sess_t=rev)
        assert int(got[0]["n_wide"]) <= n


@pytest.mark.gpu
def test_gpu_no_session_and_no_slot():
    import torch
    d, ds, dres, dst, ddq, dhc, host, keep = gpu_round("geom_one_65_all")
    got = rhp.gather_wide_device(d, None, 0, None, None, ddq, dhc, (4, 4, 4), GUARD)()
    assert not any(int(got[0][f]) for f in got[0].dtype.names)
    untouched(got, "no session")
    d0 = rhp.Batch.from_buffer_copy(d)
    d0.n = 0
    got = rhp.gather_wide_device(d0, ds, 1, dres, dst, ddq, dhc, (4, 4, 4), GUARD)()
    assert not any(int(got[0][f]) for f in got[0].dtype.names)
    untouched(got, "no slot")


@pytest.mark.gpu
def test_gpu_whole_round_in_one_call():
    """rhp.gather_wide_gpu with details, the round's buffers left on the device between the fix-up and the gather:
    the four outputs against the twin over the records the call returns, the session results against the host's
    fix-up.  The smallest input with every kind of session: two pipelined complete requests (the first one chunked,
    so a slot is wide and a body gathered), one incomplete request, no bytes"""
    chunked = b"POST /c HTTP/1.1\r\nHost: c\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n0\r\n\r\n"
    buf, off, sess, _ = rhp.pack_sessions([chunked + b"GET /a HTTP/1.1\r\nHost: a\r\n\r\n", b"GET /b HTTP/1.1\r\nHost:", b""])
    n = len(off) - 1
    got = rhp.gather_wide_gpu(buf, off, sess, 4, guard=64, details=True)
    assert len(got) == 10
    res, results, starts, dreq, hc, lens = got[4:]
    assert len(dreq) == len(hc) == 8 * n and len(lens) == 4 * n and lens.dtype == np.uint16
    want_results = rhp.fixup_cpu(buf, off, sess, 4)[1]
    assert results.tolist() == want_results.tolist() and results["n_slots"].tolist() == [2, 1, 0]
    cpu = rhp.gather_wide_cpu(res, sess, results, starts, dreq, hc)
    assert got[0] == cpu[0] and (got[1] == cpu[1]).all() and (got[2] == cpu[2]).all() and (got[3] == cpu[3]).all()
    assert int(got[0]["n_wide"]) >= 1 and bytes(got[3]) == b"hello"
    check(got[:4], statement(res, off, sess, results, starts, dreq, hc, 4), "one call")
    short = rhp.gather_wide_gpu(buf, off, sess, 4, guard=64)
    assert len(short) == 4 and short[0] == got[0] and all((a == b).all() for a, b in zip(short[1:], got[1:4]))
