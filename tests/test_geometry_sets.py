"""The batches of tests/geometry_sets.py are what their names claim, for every
CU count the launch formula may meet (256: MI355X; 128 and 304 beside it):
conditions computed from the offsets with the kernel's own inequality, from the
emulator's F_EXACT flags and from the oracle's records.  And the harness
(DeviceBatch fill / guard, Guarded) catches what it is for, shown on host
memory.  No GPU."""
import numpy as np
import pytest

import libreactorng_amd as rhp
import geometry_sets as gs
from oracle_util import run_oracle, to_rhp

CUS = (256, 128, 304)
PHR, HTTP = rhp.MODE_PHR, rhp.MODE_HTTP
# (S, short last range) of test_gpu_geometry.py's range-size cases
SPANS = [(1025, False), (4096, False), (4097, False), (4097, True), (8192, False), (8193, False), (8193, True)]
# (S, per_range, mode) of its replay cases
DEFERRED = [(4096, 480, HTTP), (4096, 481, HTTP), (4096, 481, PHR), (gs.SLOW_CAP + 1, gs.SLOW_CAP + 1, PHR)]


def test_ranges_hand_computed():
    assert gs.ranges(1, 256) == [(0, 1)]
    assert gs.ranges(1024, 256) == [(0, 1024)]
    assert gs.ranges(1025, 256) == [(0, 513), (513, 1025)]
    assert gs.ranges(3073, 256) == [(0, 769), (769, 1538), (1538, 2307), (2307, 3073)]
    for cus in CUS:
        r = gs.ranges(1024 * cus + 1, cus)
        assert len(r) == cus and r[0] == (0, 1025) and r[1] == (1025, 2050)     # span 1025
        assert r[-1] == (1025 * (cus - 1), 1024 * cus + 1)                      # the last range: what is left
        r = gs.ranges(1024 * cus, cus)
        assert len(r) == cus and all(hi - lo == 1024 for lo, hi in r)
        r = gs.ranges(1024 * cus - 1, cus)
        assert len(r) == cus and r[0] == (0, 1024) and r[-1][1] - r[-1][0] == 1023


@pytest.mark.parametrize("cus", CUS)
def test_span_n_gives_the_span(cus):
    for S, short in SPANS:
        r = gs.ranges(gs.span_n(S, cus, short), cus)
        assert len(r) == cus and all(hi - lo == S for lo, hi in r[:-1])
        # the smallest n with span S leaves the last range S - cus + 1 requests: none of
        # these S is below cus + 64, so it still has the 64 requests the evenness test reads
        assert r[-1][1] - r[-1][0] == (S - cus + 1 if short else S) >= 64


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("kind", ["even", "uneven", "mixed"])
def test_span_batches_are_what_they_claim(cus, kind):
    for S, short in SPANS:
        n = gs.span_n(S, cus, short)
        buf, off = gs.span_batch(S, cus, kind, n)
        assert len(off) - 1 == n
        ln = np.diff(off.astype(np.int64))
        assert ln.min() >= 18 and ((ln <= 40) | (ln >= 400)).all()
        seen = set()
        for lo, hi in gs.ranges(n, cus):
            want = kind if kind != "mixed" else "even" if hi <= n // 2 else "uneven" if lo >= n // 2 else None
            if want == "even":
                assert gs.range_has_no_long_request(off, lo, hi) and not gs.range_is_uneven(off, lo, hi), (S, lo, hi)
            elif want == "uneven":
                assert gs.range_is_uneven(off, lo, hi), (S, lo, hi)
            seen.add(want)
        assert seen >= ({"even", "uneven"} if kind == "mixed" else {kind})


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("S,per_range,mode", DEFERRED)
def test_deferred_batches_defer_what_they_claim(cus, S, per_range, mode):
    """every range defers exactly per_range requests: by the emulator's F_EXACT
    flags in phr mode; in http mode the chunked bodies of the oracle's records
    and, beside them, whatever the emulator sends to the exact path (nothing).
    The records come from one period of the batch (a request's records depend
    only on its own bytes and the bytes after it) spread over the batch by the
    template index, and from the whole batch where that is small."""
    buf, off = gs.deferred_batch(S, cus, per_range, mode)
    n = len(off) - 1
    assert n == cus * S
    m = min(n, 3 * S)   # three ranges: every position a replaced request can have in a range
    sb, so = buf[: int(off[m]) + rhp.RHP_PAD].copy(), off[: m + 1]
    sb[int(off[m]):] = 0
    emu, _ = rhp.emulate(sb, so, 4, mode)
    deferred = (emu.reqs["flags"] & rhp.F_EXACT) != 0
    if mode == HTTP:
        reqs, _, http, _ = run_oracle(sb, so, 4, mode)
        assert not deferred.any()
        deferred = gs.is_chunked(reqs, http)
    # the ranges repeat: a request is deferred exactly when its bytes are the deferred template's
    tpl = gs.DEFER_HTTP if mode == HTTP else gs.DEFER_PHR
    ln = np.diff(off.astype(np.int64))
    is_tpl = (ln == len(tpl)) & (buf[off[:-1].astype(np.int64)] == tpl[0])
    assert not any(s[0] == tpl[0] for s in gs.SHORT)
    assert np.array_equal(deferred, is_tpl[:m])
    counts = gs.deferred_per_range(off, cus, is_tpl)
    assert counts == [per_range] * cus
    for lo, hi in gs.ranges(n, cus):
        assert not gs.range_is_uneven(off, lo, hi)


@pytest.mark.parametrize("mode", [PHR, HTTP])
def test_cycle_holds_every_outcome(mode):
    buf, off = gs.cycle(64, mode)
    t = gs.cycle_templates(mode)
    assert len(off) - 1 == 64 and len(set(t)) == 37 and max(len(x) for x in t) <= 1024
    ln = np.diff(off.astype(np.int64))
    reqs, hdrs, http, _ = run_oracle(buf, off, 16, mode)
    emu, _ = rhp.emulate(buf, off, 16, mode)
    exact = (emu.reqs["flags"] & rhp.F_EXACT) != 0
    ret = reqs["ret"]
    plain = (ret > 0) & ~exact & (ret == ln)
    assert (plain & (ret <= 128)).sum() >= 5 and (plain & (ret > 256)).sum() >= 3     # one window; three or more
    first = buf[off[:-1].astype(np.int64)]
    text = [bytes(buf[int(off[i]):int(off[i + 1])]) for i in range(64)]
    assert (exact & (ret > 0) & (first == 13)).any()                                   # leading CRLF
    assert any(exact[i] and ret[i] > 0 and b"\r\n \t" in text[i] for i in range(64))    # obs-fold
    assert any(exact[i] and ret[i] > 0 and b"\r" not in text[i] for i in range(64))     # bare LF
    assert (ret == -1).sum() >= 3 and ((ret == -2) & (ln > 0)).sum() >= 3 and ((ret == -2) & (ln == 0)).sum() >= 1
    if mode == HTTP:
        res = http["result"]
        chunked = gs.is_chunked(reqs, http)
        assert ((res == 1) & (http["body_kind"] == 1) & ~chunked & (http["body_len"] > 0)).any()   # Content-Length
        assert ((res == 0) & (ret > 0)).any()                                                      # short body
        assert chunked.sum() >= 2
        assert any(res[i] == -1 and ret[i] > 0 and b"chunked" in text[i] for i in range(64))       # malformed chunked


def test_fill_word():
    assert gs.fill_word(0xFF) == -1 and gs.fill_word(0x5A) == 0x5A5A5A5A


# ---- the harness catches what it is for ----

def _parsed_into(fill):
    """an http batch parsed on the host into request-major buffers, laid into
    Guarded host slices that held `fill` first: what DeviceBatch(fill=, guard=)
    downloads, without a device"""
    buf, off = gs.cycle(64, HTTP)
    res = rhp.parse_cpu_exact(buf, off, 4, HTTP)
    want = to_rhp(*run_oracle(buf, off, 4, HTTP)[:3], HTTP)
    areas = {name: rhp.Guarded(name, raw.size, guard=64, fill=fill, device="cpu", data=raw)
             for name, raw in (("reqs", res.raw_reqs), ("hdrs", res.raw_hdrs), ("http", res.raw_http))}
    return res, want, areas


def _as_result(areas, n):
    reqs = areas["reqs"].view.numpy()[: n * 16].view(rhp.REQ_DTYPE)
    http = areas["http"].view.numpy()[: n * 24].view(rhp.HTTP_DTYPE)
    return rhp.Result(reqs, None, http)


@pytest.mark.parametrize("fill", [0xFF, 0x5A, rhp.GUARD_BYTE])
def test_guards_and_fill_catch_a_stray_and_a_missed_store(fill):
    res, want, areas = _parsed_into(fill)
    n = len(res.reqs)
    for g in areas.values():
        assert g.pattern != fill and g.front % rhp.Guarded.ALIGN == 0
        g.check()
    gs.assert_no_slot_left(_as_result(areas, n), HTTP, fill, want)
    # one byte directly behind hdrs, one directly before http
    g = areas["hdrs"]
    g.buf[g.front + g.size] = fill
    with pytest.raises(rhp.GuardError, match=r"hdrs: 1 guard bytes after the buffer.*offset 0 from its end"):
        g.check()
    g = areas["http"]
    g.buf[g.front - 1] ^= 1
    with pytest.raises(rhp.GuardError, match=r"http: 1 guard bytes before the buffer.*offset -1 from its start"):
        g.check()
    areas["reqs"].check()
    # one http record, then one request record, back to the fill: a store that never happened
    i = int(np.flatnonzero(want[2]["result"] == 1)[0])
    areas["http"].view[24 * i: 24 * i + 24] = fill
    with pytest.raises(AssertionError, match=rf"http\[i\].result still holds the fill.*first #{i}\b"):
        gs.assert_no_slot_left(_as_result(areas, n), HTTP, fill, want)
    areas["http"].view[24 * i: 24 * i + 24].copy_(areas["http"].view.new_tensor(res.raw_http[24 * i: 24 * i + 24]))
    areas["reqs"].view[16 * i: 16 * i + 16] = fill
    with pytest.raises(AssertionError, match=rf"reqs\[i\].ret still holds the fill.*first #{i}\b"):
        gs.assert_no_slot_left(_as_result(areas, n), HTTP, fill, want)


def test_guarded_shift_and_plain_allocation():
    g = rhp.Guarded("bytes", 100, guard=0, device="cpu", shift=48, data=np.arange(100, dtype=np.uint8))
    assert g.front == 48 and (g.view.numpy() == np.arange(100)).all() and (g.buf[:48] == g.pattern).all()
    g.check()
    g = rhp.Guarded("bytes", 100, guard=32, device="cpu", shift=16)
    assert g.front == rhp.Guarded.ALIGN + 16 and len(g.buf) == g.front + 100 + 32 and (g.view == 0).all()
    g = rhp.Guarded("reqs", 64, device="cpu")
    assert g.buf is g.view and (g.view == 0).all()       # no guard, no shift: the plain allocation
    g = rhp.Guarded("reqs", 64, fill=0xFF, device="cpu")
    assert g.buf is g.view and (g.view == 0xFF).all()


def test_canonical_records_do_not_depend_on_the_fill():
    """expand_reqs / expand_records / expand_http / canonical read nothing the
    layout leaves unspecified: the emulator's records laid over buffers of 0xFF
    and of 0x5A in every area the layout leaves unspecified (_refilled) give the
    same canonical records as over zeroed ones, in every layout."""
    for mode, layouts in ((PHR, range(5)), (HTTP, range(4))):
        buf, off = gs.cycle(200, mode)
        n = len(off) - 1
        for layout in layouts:
            for maxh in (0, 3, 16):
                base, _ = rhp.emulate(buf, off, maxh, mode, layout)
                want = rhp.canonical(base, mode)
                for fill in (0xFF, 0x5A):
                    raw = [None if a is None else np.full_like(a, fill)
                           for a in (base.raw_reqs, base.raw_hdrs, base.raw_http)]
                    reqs = rhp.expand_reqs(base.raw_reqs, n, layout)
                    got_reqs = rhp.expand_reqs(_refilled(base.raw_reqs, raw[0], layout, n, "reqs"), n, layout)
                    hd = _refilled(base.raw_hdrs, raw[1], layout, n, "hdrs", maxh, reqs)
                    hdrs = (rhp.expand_records(got_reqs, hd, n, maxh, layout) if layout in rhp.LENGTH_LAYOUTS
                            else rhp.hdr_view(hd.view(rhp.HDR_DTYPE), n, maxh, layout))
                    http = None
                    if mode == HTTP:
                        http = rhp.expand_http(got_reqs, _refilled(base.raw_http, raw[2], layout, n, "http", 0, reqs),
                                               n, layout)
                    got = rhp.canonical(rhp.Result(got_reqs, hdrs, http), mode)
                    for a, b in zip(got, want):
                        assert (a is None and b is None) or np.array_equal(a, b), (mode, layout, maxh, fill)


def _refilled(zeroed, filled, layout, n, what, maxh=0, reqs=None):
    """`zeroed` (the emulator's buffer over zeros) with the areas the layout
    leaves unspecified taken from `filled`: the wide slots of requests that are
    not wide, header records and lengths past num_headers or of ret <= 0"""
    out = zeroed.copy()
    dense, lens = layout in rhp.DENSE_LAYOUTS, layout in rhp.LENGTH_LAYOUTS
    if what == "reqs":
        if dense:
            wide = (zeroed[: 8 * n].reshape(n, 8)[:, 7] & rhp.DENSE_WIDE) != 0
            at = (8 * n + 15) & ~15
            w = out[at: at + 16 * n].reshape(n, 16)
            w[~wide] = filled[at: at + 16 * n].reshape(n, 16)[~wide]
        return out
    if what == "http":
        if layout in (rhp.LAYOUT_COMPACT, rhp.LAYOUT_DENSE):
            wide = (zeroed[: 8 * n].reshape(n, 8)[:, 2] & rhp.HTTP_WIDE) != 0
            at = (8 * n + 15) & ~15
            w = out[at: at + 24 * n].reshape(n, 24)
            w[~wide] = filled[at: at + 24 * n].reshape(n, 24)[~wide]
        return out
    if maxh == 0:
        return out
    nh = np.where(reqs["ret"] > 0, np.minimum(reqs["num_headers"], maxh), 0)
    unused = np.arange(maxh)[None, :] >= nh[:, None]                 # [n, maxh]
    is_wide = (reqs["flags"] & rhp.F_WIDE) != 0 if lens else np.ones(n, dtype=bool)
    if lens:
        # lengths (header-major but for dense-rm): unused rows, and every row of a wide request
        width = 2 if dense else 4
        a = out[: n * maxh * width].reshape((n, maxh, width) if layout == rhp.LAYOUT_DENSE_RM else (maxh, n, width))
        f = filled[: n * maxh * width].reshape(a.shape)
        m = unused | is_wide[:, None]
        m = m if layout == rhp.LAYOUT_DENSE_RM else m.T
        a[m] = f[m]
        at = rhp.hdrs_bytes(n, maxh, layout) - n * maxh * 8
    else:
        at = 0
    # the rhp_hdr_t records (the wide area of a length layout: request-major)
    shape = (maxh, n, 8) if layout == rhp.LAYOUT_HEADER_MAJOR else (n, maxh, 8)
    a = out[at: at + n * maxh * 8].reshape(shape)
    f = filled[at: at + n * maxh * 8].reshape(shape)
    m = unused | ~is_wide[:, None]
    m = m.T if layout == rhp.LAYOUT_HEADER_MAJOR else m
    a[m] = f[m]
    return out
