"""How rhp_parse_batch is launched and where its results land (the batches of
tests/geometry_sets.py): batch sizes around every threshold of the launch
formula and of rhp_dfa_kernel's ranges, record buffers that hold 0xFF (or 0x5A)
instead of zeros, guards beside every buffer the library writes, bytes at an
address that is 16-byte aligned and no more, two parses in flight.

Expected records: the oracle's (run_oracle -> to_rhp), compared with
assert_same; in http mode the bytes too.  Every DeviceBatch here has guards
(GUARD bytes on both sides of reqs, hdrs, http and bytes; result() checks
them) and a fill.

range length           what changes (rhp_kernel.hip)                          covered by
< 64 .. 1024           lanes / waves with no first request                    test_gpu_batch_size_sweep (n 1 .. 1024)
1024 -> 1025           first refill; may_order                                ... (n 1025 .. 3073, 1024 CUs + 1), range S 1025
4096 -> 4097           order in two waves' staging                            test_gpu_range_size_thresholds
8192 -> 8193           order_on false                                         test_gpu_range_size_thresholds
> 480 deferred         use_list false; http: direct                           test_gpu_replay_thresholds (480 | 481)
> kSlowCap exact       slow list full: finish_slow inline                     test_gpu_replay_thresholds (6081, phr)
65536 -> 65537         use_list false whatever was deferred                   not covered
n > 2048 CUs           rhp_exact_kernel's second stride iteration             test_gpu_exact_kernel_second_stride
"""
import functools

import numpy as np
import pytest

import libreactorng_amd as rhp
import geometry_sets as gs
from oracle_util import assert_same, canon, run_oracle, to_rhp

pytestmark = pytest.mark.gpu

PHR, HTTP = rhp.MODE_PHR, rhp.MODE_HTTP
RM, HM, CO, DE, DRM = (rhp.LAYOUT_REQUEST_MAJOR, rhp.LAYOUT_HEADER_MAJOR, rhp.LAYOUT_COMPACT, rhp.LAYOUT_DENSE,
                       rhp.LAYOUT_DENSE_RM)
LAYOUTS = {PHR: (RM, HM, CO, DE, DRM), HTTP: (RM, HM, CO, DE)}
IMPLS = {PHR: (rhp.IMPL_DFA, rhp.IMPL_DFA_LATE), HTTP: (rhp.IMPL_DFA,)}
GUARD = 4096
FLAGS = rhp.F_EXACT | rhp.F_WIDE


@functools.lru_cache(maxsize=None)
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def resolve(n):
    """a batch size: a number, or one stated in CUs ("1024cus+1")"""
    if isinstance(n, int):
        return n
    mult, _, rest = n.partition("cus")
    return int(mult) * cus() + int(rest or 0)


@functools.lru_cache(maxsize=3)
def batch(key):
    """(buf, off) by name, shared and never written: ("cycle", n, mode, shift),
    ("span", S, short_last, kind), ("short", n), ("deferred", S, per_range, mode), ("lead",)"""
    kind = key[0]
    if kind == "cycle":
        buf, off = gs.cycle(key[1], key[2], key[3])
    elif kind == "span":
        buf, off = gs.span_batch(key[1], cus(), key[3], gs.span_n(key[1], cus(), key[2]))
    elif kind == "short":
        buf, off = gs.span_batch(None, cus(), "even", key[1])
    elif kind == "deferred":
        buf, off = gs.deferred_batch(key[1], cus(), key[2], key[3])
    else:
        from test_line_windows import lead_batch
        buf, off = lead_batch()
    buf.flags.writeable = off.flags.writeable = False
    return buf, off


@functools.lru_cache(maxsize=6)
def expected(key, maxh, mode):
    """(the oracle's canonical records, its rewritten bytes) of batch(key); shared, never written"""
    buf, off = batch(key)
    rq, hd, ht, out = run_oracle(buf, off, maxh, mode)
    return to_rhp(rq, hd, ht, mode), (out if mode == HTTP else None)


@functools.lru_cache(maxsize=12)
def emulated_flags(key, maxh, mode, layout):
    buf, off = batch(key)
    emu, _ = rhp.emulate(buf, off, maxh, mode, layout)
    return (emu.reqs["flags"] & FLAGS).copy()


def run(key, maxh, mode, impl, layout, fill, label, flags=True, **kw):
    """one guarded, filled parse of batch(key) against the oracle; the parsed Result"""
    buf, off = batch(key)
    want, out = expected(key, maxh, mode)
    res = rhp.parse_batch(buf, off, maxh, mode, impl=impl, layout=layout, fill=fill, guard=GUARD, **kw)
    label = f"{label} {key} maxh{maxh} mode{mode} impl{impl} layout{layout} fill{fill:#x}"
    assert_same(canon(res, mode), want, buf, off, label)
    if mode == HTTP:
        assert np.array_equal(res.bytes_out, out), f"{label}: {int((res.bytes_out != out).sum())} rewritten bytes differ"
    if layout == RM:   # no slot's specified field is left holding the fill
        gs.assert_no_slot_left(res, mode, fill, want)
    if flags and impl != rhp.IMPL_EXACT:   # the kernel takes the exact path where the emulator of its algorithm does
        assert np.array_equal(res.reqs["flags"] & FLAGS, emulated_flags(key, maxh, mode, layout)), label
    return res


# ---- 1. batch sizes ----

SWEEP_N = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 2047, 2048, 2049, 3073, "1024cus-1", "1024cus", "1024cus+1")
SWEEP = [pytest.param(mode, n, layout, id=f"mode{mode}-n{n}-layout{layout}")
         for mode in (PHR, HTTP) for n in SWEEP_N for layout in LAYOUTS[mode]]


@pytest.mark.parametrize("fill", [0xFF, 0x5A])
@pytest.mark.parametrize("mode,n,layout", SWEEP)
def test_gpu_batch_size_sweep(mode, n, layout, fill):
    """cycle(n, mode) at the sizes where a range's prologue changes: ranges
    with fewer requests than lanes, than waves, than threads; the first refill
    (1025 is two ranges of 513 and 512, 2049 three, 3073 four); one workgroup
    per CU with ranges of 1023, 1024 and (1024 CUs + 1: span 1025) the first
    range that refills on a full grid."""
    n = resolve(n)
    for shift in (0, 1):
        for maxh in (0, 3, 16):
            for impl in IMPLS[mode]:
                run(("cycle", n, mode, shift), maxh, mode, impl, layout, fill, "size sweep")


EXACT_SMALL = [pytest.param(mode, n, layout, id=f"mode{mode}-n{n}-layout{layout}")
               for mode in (PHR, HTTP) for n in (1, 255, 256, 257) for layout in LAYOUTS[mode]]


@pytest.mark.parametrize("fill", [0xFF, 0x5A])
@pytest.mark.parametrize("mode,n,layout", EXACT_SMALL)
def test_gpu_exact_kernel_sizes(mode, n, layout, fill):
    """rhp_exact_kernel (256 threads a block) around one block"""
    for shift in (0, 1):
        for maxh in (0, 3, 16):
            run(("cycle", n, mode, shift), maxh, mode, rhp.IMPL_EXACT, layout, fill, "exact sizes")


@pytest.mark.parametrize("fill", [0xFF, 0x5A])
@pytest.mark.parametrize("layout", [RM, DE])
@pytest.mark.parametrize("mode", [PHR, HTTP])
@pytest.mark.parametrize("n", ["2048cus", "2048cus+1"])
def test_gpu_exact_kernel_second_stride(n, mode, layout, fill):
    """rhp_exact_kernel's grid is at most 8 blocks a CU: above 2048 requests a
    CU a thread takes a second request (short requests: the bytes stay small)"""
    run(("short", resolve(n)), 3, mode, rhp.IMPL_EXACT, layout, fill, "exact stride")


# ---- 2. range sizes ----

SPANS = [(1025, False), (4096, False), (4097, False), (4097, True), (8192, False), (8193, False), (8193, True)]
SPAN_CASES = [(PHR, rhp.IMPL_DFA, HM), (PHR, rhp.IMPL_DFA, DE), (PHR, rhp.IMPL_DFA_LATE, HM), (PHR, rhp.IMPL_DFA_LATE, DE),
              (HTTP, rhp.IMPL_DFA, RM), (HTTP, rhp.IMPL_DFA, CO)]


@pytest.mark.parametrize("S,short_last,mode,impl,layout",
                         [pytest.param(S, short, *c, id=f"S{S}{'-shortlast' if short else ''}-mode{c[0]}-impl{c[1]}-layout{c[2]}")
                          for S, short in SPANS for c in SPAN_CASES])
def test_gpu_range_size_thresholds(S, short_last, mode, impl, layout):
    """one range of S requests per CU, the batch's first half even, its second
    half uneven (span_batch "mixed"): the refill and may_order (1025), the order
    in one wave's staging and in two (4096 | 4097), the longest-first order on
    and off (8192 | 8193).  short_last: n = CUs * (S - 1) + 1, the smallest batch
    with span S; its last range has S - CUs + 1 requests, so at 8193 it alone
    still orders."""
    run(("span", S, short_last, "mixed"), 4, mode, impl, layout, 0xFF, "range size")


# ---- 3. the replay's lists ----

REPLAY = [(4096, 480, HTTP, rhp.IMPL_DFA, RM), (4096, 480, HTTP, rhp.IMPL_DFA, CO),
          (4096, 481, HTTP, rhp.IMPL_DFA, RM), (4096, 481, HTTP, rhp.IMPL_DFA, CO),
          (4096, 481, PHR, rhp.IMPL_DFA, RM), (4096, 481, PHR, rhp.IMPL_DFA_LATE, DE),
          (gs.SLOW_CAP + 1, gs.SLOW_CAP + 1, PHR, rhp.IMPL_DFA, RM), (gs.SLOW_CAP + 1, gs.SLOW_CAP + 1, PHR, rhp.IMPL_DFA, DE)]


@pytest.mark.parametrize("S,per_range,mode,impl,layout", REPLAY)
def test_gpu_replay_thresholds(S, per_range, mode, impl, layout):
    """every range defers per_range requests: 480 fill the replay's list
    (kDeferCap), 481 overflow it (the replay scans the range; http mode frames
    in its second pass), kSlowCap + 1 = 6081 exact-path requests in a range of as
    many (the smallest that holds them) overflow the slow list too."""
    res = run(("deferred", S, per_range, mode), 4, mode, impl, layout, 0xFF, "replay")
    if mode == PHR:
        deferred = (res.reqs["flags"] & rhp.F_EXACT) != 0
        assert gs.deferred_per_range(batch(("deferred", S, per_range, mode))[1], cus(), deferred) == [per_range] * cus()


# ---- 4. the pointer contract ----

@pytest.mark.parametrize("layout", [RM, DE])
@pytest.mark.parametrize("which", ["cycle", "lead"])
@pytest.mark.parametrize("mode", [PHR, HTTP])
@pytest.mark.parametrize("bytes_shift", [16, 48, 112])
def test_gpu_bytes_16_byte_aligned_only(bytes_shift, mode, which, layout):
    """rhp.h asks for `bytes` 16-byte aligned: the records are the oracle's at
    any such address, and the choice between the DFA and the exact path is the
    one at a 512-byte aligned address (windows are counted from p.bytes)."""
    key = ("cycle", 1025, mode, 0) if which == "cycle" else ("lead",)
    for maxh in (2, 16):
        base = run(key, maxh, mode, rhp.IMPL_DFA, layout, 0xFF, "bytes_shift 0")
        res = run(key, maxh, mode, rhp.IMPL_DFA, layout, 0xFF, f"bytes_shift {bytes_shift}", bytes_shift=bytes_shift)
        assert np.array_equal(res.reqs["flags"] & FLAGS, base.reqs["flags"] & FLAGS)


# ---- 6. rhp_pack_dense and rhp_fixup_sessions outputs ----

@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_gpu_pack_dense_outputs_guarded(n):
    from test_dense import gpu_pack_equals_cpu_pack
    buf, off = batch(("cycle", n, HTTP, 0))
    for maxh in (3, 16):
        db = rhp.DeviceBatch(buf, off, maxh, HTTP, layout=RM, fill=0xFF, guard=GUARD)
        db.launch()
        res, _, _, _ = gpu_pack_equals_cpu_pack(db, n, maxh, guard=GUARD, fill=0xFF)
        assert_same(canon(res, HTTP), expected(("cycle", n, HTTP, 0), maxh, HTTP)[0], buf, off, f"pack n{n}")


@pytest.mark.parametrize("first", [1, 5])
@pytest.mark.parametrize("layout", [RM, HM])
def test_gpu_fixup_outputs_guarded(first, layout):
    """the session shapes set's smallest cases with guards beside `results` and
    `req_start` (and the batch's buffers), against the reference loop and the
    host twin"""
    import test_sessions
    test_sessions.gpu_shapes(first, 16, rhp.IMPL_DFA, layout, guard=GUARD)


# ---- 7. two parses in flight ----

def test_gpu_two_parses_in_flight():
    """the benchmark's launch pattern: two batches on two streams, launched in
    turn for three rounds with no synchronize between; each round refills its
    records with 0xFF and (http: de-framed in place) uploads its bytes again, on
    its own stream"""
    import torch
    ka, kb = ("span", 1025, False, "mixed"), ("cycle", 3073, HTTP, 0)
    (ba, oa), (bb, ob) = batch(ka), batch(kb)
    a = rhp.DeviceBatch(ba, oa, 4, PHR, layout=HM, fill=0xFF, guard=GUARD)
    b = rhp.DeviceBatch(bb, ob, 16, HTTP, layout=RM, fill=0xFF, guard=GUARD)
    fresh = torch.from_numpy(bb.copy()).pin_memory()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    for _ in range(3):
        with torch.cuda.stream(sa):
            a.fill_records()
            a.launch(sa)
        with torch.cuda.stream(sb):
            b.fill_records()
            b.bytes.copy_(fresh, non_blocking=True)
            b.launch(sb)
    torch.cuda.synchronize()
    ra, rb = a.result(), b.result()
    assert_same(canon(ra, PHR), expected(ka, 4, PHR)[0], ba, oa, "in flight: phr header-major")
    want, out = expected(kb, 16, HTTP)
    assert_same(canon(rb, HTTP), want, bb, ob, "in flight: http request-major")
    assert np.array_equal(rb.bytes_out, out)
    gs.assert_no_slot_left(rb, HTTP, 0xFF, want)
