"""Dense records (RHP_LAYOUT_DENSE / RHP_LAYOUT_DENSE_RM, include/rhp.h; round
6): 8-byte request records and 2-byte header lengths (header- or request-major)
for what the DFA parses, the wide rhp_req_t / rhp_hdr_t records for everything
else.  Expanded (rhp_expand_reqs, rhp_expand_records), the records equal the
reference's (golden fixtures, the oracle, full-size digests) whichever path
parsed a request.

CPU: the kernel's emulator and the product's exact parser in the dense layouts;
a method over 255 bytes sends a request to the exact path, a header name of 63+
or a value of 1008+ bytes overflows into the u32 area; the same limits in http
mode (batches.http_field_limits) in the dense, compact and request-major
layouts and through rhp_cpu_pack_dense.
GPU (-m gpu): that http batch by every kernel at every alignment; the DFA kernel (both loop forms) and the exact kernel in the dense
layout, against the golden sets, fuzz at every max_headers, the full-size
digests of configs 2/3/4, edge cases at every alignment, last_len; the
DFA/exact choice equals the emulator's."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

import libreactorng_amd as rhp
from golden_sets import inputs, record_digest
from oracle_util import assert_same, canon, run_oracle, to_rhp
from batches import EDGE, HTTP_LIMIT_NAMES, HTTP_LIMIT_VALUES, http_field_limits, pack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SETS = json.load(open(os.path.join(GOLDEN, "manifest.json")))["sets"]
FULL = json.load(open(os.path.join(GOLDEN, "full_digests.json")))["sets"]
PHR_SETS = sorted(k for k, v in SETS.items() if v["mode"] == rhp.MODE_PHR)
HTTP_SETS = sorted(k for k, v in SETS.items() if v["mode"] == rhp.MODE_HTTP)
D = rhp.LAYOUT_DENSE
LAYS = [rhp.LAYOUT_DENSE, rhp.LAYOUT_DENSE_RM]


def golden(name):
    spec = SETS[name]
    buf, off = inputs(spec)
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    return spec, buf, off, (z["reqs"], z["hdrs"], z["http"] if "http" in z.files else None)


def dense_fields(res, n):
    """(flags, ret) of the raw rhp_req_dense_t records"""
    raw = res.raw_reqs[: 8 * n].reshape(n, 8)
    return raw[:, 7], raw[:, 0].astype(np.uint32) | raw[:, 1].astype(np.uint32) << 8


def long_fields():
    """requests whose DFA records the dense fields cannot hold, beside ones they can"""
    return [b"GET / HTTP/1.1\r\nHost: a\r\n\r\n",
            b"M" * 256 + b" / HTTP/1.1\r\nHost: a\r\n\r\n",                     # method 256 B
            b"M" * 255 + b" / HTTP/1.1\r\nHost: a\r\n\r\n",                     # method 255 B: dense
            b"GET / HTTP/1.1\r\n" + b"N" * 63 + b": v\r\n\r\n",                 # name 63 B
            b"GET / HTTP/1.1\r\n" + b"N" * 62 + b": v\r\n\r\n",                 # name 62 B: dense
            b"GET / HTTP/1.1\r\nX: " + b"v" * 1008 + b"\r\n\r\n",               # value 1008 B
            b"GET / HTTP/1.1\r\nX: " + b"v" * 1007 + b"\r\n\r\n",               # value 1007 B: dense
            b"GET /" + b"p" * 60000 + b" HTTP/1.0\r\nA: b\r\n\r\n",             # long path: dense
            b"GET / HTTP/1.1\r\nBad Header\r\n\r\n",                            # -1
            b"GET / HTTP/1.1\r\nA: b\r\n"]                                      # -2: exact


@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", PHR_SETS)
def test_emulation_dense_matches_golden(name, lay):
    spec, buf, off, want = golden(name)
    res, _ = rhp.emulate(buf, off, spec["max_headers"], spec["mode"], lay)
    assert_same(canon(res, spec["mode"]), want, buf, off, f"emulation (dense {lay}) vs golden {name}")
    res = rhp.parse_cpu_exact(buf, off, spec["max_headers"], spec["mode"], lay)
    assert_same(canon(res, spec["mode"]), want, buf, off, f"CPU exact (dense) vs golden {name}")
    flags, _ = dense_fields(res, len(off) - 1)
    assert (flags & rhp.DENSE_WIDE).all()   # the exact parser's records are all wide


@pytest.mark.parametrize("lay", LAYS)
def test_dense_field_limits(lay):
    buf, off = pack(long_fields())
    want = to_rhp(*run_oracle(buf, off, 16, rhp.MODE_PHR)[:3], rhp.MODE_PHR)
    res, _ = rhp.emulate(buf, off, 16, rhp.MODE_PHR, lay)
    assert_same(canon(res, rhp.MODE_PHR), want, buf, off, "dense limits (emulation)")
    flags, _ = dense_fields(res, len(off) - 1)
    wide = (flags & rhp.DENSE_WIDE) != 0
    # a long method takes the exact path; long names and values overflow into the u32 area
    assert list(wide) == [False, True, False, False, False, False, False, False, False, True]
    assert flags[8] & rhp.DENSE_BAD
    n = len(off) - 1
    l16 = res.raw_hdrs[: 2 * n * 16].view(np.uint16)
    k0 = (np.arange(n) * 16) if lay == rhp.LAYOUT_DENSE_RM else np.arange(n)   # header 0 of each request
    assert list(l16[k0] == 0xFFFF) == [False, False, False, True, False, True, False, False, False, False]


def test_dense_request_major_rejected_in_http_mode():
    buf, off = pack([b"GET / HTTP/1.1\r\n\r\n"])
    with pytest.raises(RuntimeError):
        rhp.emulate(buf, off, 16, rhp.MODE_HTTP, rhp.LAYOUT_DENSE_RM)
    with pytest.raises(RuntimeError):
        rhp.parse_cpu_exact(buf, off, 16, rhp.MODE_HTTP, rhp.LAYOUT_DENSE_RM)


@pytest.mark.parametrize("name", HTTP_SETS)
def test_emulation_dense_http_matches_golden(name):
    """http mode (round 6): dense request and header records beside the compact
    http records; de-framed bytes as the reference's"""
    spec, buf, off, want = golden(name)
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    for res in (rhp.emulate(buf, off, spec["max_headers"], spec["mode"], D)[0],
                rhp.parse_cpu_exact(buf, off, spec["max_headers"], spec["mode"], D)):
        assert_same(canon(res, spec["mode"]), want, buf, off, f"dense http vs golden {name}")
        if "bytes_out_sha256" in z.files:
            assert hashlib.sha256(res.bytes_out.tobytes()).digest() == z["bytes_out_sha256"].tobytes()


HTTP_LAYS = [rhp.LAYOUT_DENSE, rhp.LAYOUT_COMPACT, rhp.LAYOUT_REQUEST_MAJOR]
LIMIT_SHIFTS, LIMIT_MAXH = (0, 1, 2, 3), (1, 2, 16)


@functools.lru_cache(maxsize=None)
def http_limits(shift, maxh, times=1):
    """(buf, off, the oracle's canonical records, its de-framed bytes) of
    batches.http_field_limits(); shared, never written"""
    buf, off = pack(http_field_limits() * times, align_shift=shift)
    rq, hd, ht, out = run_oracle(buf, off, maxh, rhp.MODE_HTTP)
    for a in (buf, off, out):
        a.flags.writeable = False
    return buf, off, to_rhp(rq, hd, ht, rhp.MODE_HTTP), out


def check_http_limits(res, shift, maxh, times, label):
    buf, off, want, out = http_limits(shift, maxh, times)
    assert_same(canon(res, rhp.MODE_HTTP), want, buf, off, label)
    assert (res.bytes_out == out).all(), f"{label}: de-framed bytes differ from the oracle's"


@pytest.mark.parametrize("maxh", LIMIT_MAXH)
@pytest.mark.parametrize("shift", LIMIT_SHIFTS)
def test_dense_http_field_limits(shift, maxh):
    """http mode at the limits of the dense encodings (method 255/256, name
    62/63/64, value 1007/1008/1023/1024 bytes): the emulator in the layouts the
    product ships and the exact parser equal the oracle, the de-framed bytes
    included; rhp_cpu_pack_dense rebuilds the records of the requests it calls
    dense, and calls some but not all of them dense."""
    buf, off, want, _ = http_limits(shift, maxh)
    n = len(off) - 1
    assert n == 300
    for lay in HTTP_LAYS:
        res, _ = rhp.emulate(buf, off, maxh, rhp.MODE_HTTP, lay)
        check_http_limits(res, shift, maxh, 1, f"http limits (emulation, layout {lay}) shift{shift} maxh{maxh}")
        if lay == D:
            flags, _ = dense_fields(res, n)
            wide = (flags & rhp.DENSE_WIDE) != 0
            assert wide.any() and not wide.all()
            m256 = np.array([r.startswith(b"M" * 256) for r in http_field_limits()])
            assert wide[m256 & (want[2]["result"] == 1)].all()   # a method the u8 cannot hold: the exact path
        res = rhp.parse_cpu_exact(buf, off, maxh, rhp.MODE_HTTP, lay)
        check_http_limits(res, shift, maxh, 1, f"http limits (CPU exact, layout {lay}) shift{shift} maxh{maxh}")
    res = rhp.parse_cpu_exact(buf, off, maxh, rhp.MODE_HTTP)
    assert 0 < check_pack(res, n, maxh) < n
    # parsed with room for its fields, each length is where the encodings say
    if maxh == 16:
        ok = want[2]["result"] == 1
        assert ok.sum() == 240
        assert set(want[0]["method_len"][ok]) == {3, 4, 255, 256}
        assert set(HTTP_LIMIT_NAMES) <= set(want[1]["name_len"][ok].ravel())
        assert set(HTTP_LIMIT_VALUES) <= set(want[1]["value_len"][ok].ravel())


def test_dense_sizes():
    assert rhp.reqs_bytes(1000, D) == 8000 + 16000
    assert rhp.hdrs_bytes(1000, 16, D) == 32000 + 64000 + 128000
    assert rhp.hdrs_bytes(3, 3, D) == 32 + 48 + 72   # the areas 16-byte aligned


# ------------------------------------------------------------------ GPU

IMPLS = [rhp.IMPL_DFA, rhp.IMPL_DFA_LATE, rhp.IMPL_EXACT]


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("name", PHR_SETS)
def test_gpu_dense_matches_reference_golden(name, impl, lay):
    spec, buf, off, want = golden(name)
    res = rhp.parse_batch(buf, off, spec["max_headers"], spec["mode"], impl=impl, layout=lay)
    assert_same(canon(res, spec["mode"]), want, buf, off, f"GPU dense impl{impl} vs golden {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("maxh", [0, 1, 3, 16, 32, 64])
def test_gpu_dense_fuzz_vs_oracle(maxh, lay):
    for impl, seed in ((rhp.IMPL_DFA, 9600 + maxh), (rhp.IMPL_DFA_LATE, 9700 + maxh)):
        buf, off = rhp.generate(rhp.GEN_FUZZ, 60000, seed)
        res = rhp.parse_batch(buf, off, maxh, rhp.MODE_PHR, impl=impl, layout=lay)
        want = to_rhp(*run_oracle(buf, off, maxh, rhp.MODE_PHR)[:3], rhp.MODE_PHR)
        assert_same(canon(res, rhp.MODE_PHR), want, buf, off, f"GPU dense fuzz impl{impl} maxh{maxh}")
        emu, _ = rhp.emulate(buf, off, maxh, rhp.MODE_PHR, lay)
        assert np.array_equal(res.reqs["flags"] & (rhp.F_EXACT | rhp.F_WIDE), emu.reqs["flags"] & (rhp.F_EXACT | rhp.F_WIDE))


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYS)
def test_gpu_dense_field_limits(lay):
    buf, off = pack(long_fields() * 40)
    want = to_rhp(*run_oracle(buf, off, 16, rhp.MODE_PHR)[:3], rhp.MODE_PHR)
    for impl in IMPLS:
        res = rhp.parse_batch(buf, off, 16, rhp.MODE_PHR, impl=impl, layout=lay)
        assert_same(canon(res, rhp.MODE_PHR), want, buf, off, f"GPU dense limits impl{impl}")
    emu, _ = rhp.emulate(buf, off, 16, rhp.MODE_PHR, lay)
    res = rhp.parse_batch(buf, off, 16, rhp.MODE_PHR, layout=lay)
    assert np.array_equal(dense_fields(res, len(off) - 1)[0], dense_fields(emu, len(off) - 1)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("name", ["config2_get256_h16", "config3_zipf_h32", "config4_get256_shard5of8",
                                  "config4_get256_shard7of8"])
def test_gpu_dense_full_size_matches_reference_digest(name, lay):
    spec = FULL[name]
    buf, off = inputs(spec)
    res = rhp.parse_batch(buf, off, spec["max_headers"], spec["mode"], layout=lay)
    got = canon(res, spec["mode"])
    if record_digest(*got) != spec["records_sha256"]:
        want = to_rhp(*run_oracle(buf, off, spec["max_headers"], spec["mode"])[:3], spec["mode"])
        assert_same(got, want, buf, off, name)
        raise AssertionError(f"{name}: dense digest differs from the reference but matches the oracle")


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYS)
@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_gpu_dense_edge_cases(shift, lay):
    buf, off = pack(EDGE * 3, align_shift=shift)
    for maxh in (0, 1, 16):
        want = to_rhp(*run_oracle(buf, off, maxh, rhp.MODE_PHR)[:3], rhp.MODE_PHR)
        res = rhp.parse_batch(buf, off, maxh, rhp.MODE_PHR, layout=lay)
        assert_same(canon(res, rhp.MODE_PHR), want, buf, off, f"GPU dense edge shift{shift} maxh{maxh}")


@pytest.mark.gpu
@pytest.mark.parametrize("lay", LAYS)
def test_gpu_dense_last_len_matches_reference_golden(lay):
    top = json.load(open(os.path.join(GOLDEN, "manifest.json")))
    buf, off = inputs(top["phr_last_len"])
    z = np.load(os.path.join(GOLDEN, "phr_last_len.npz"))
    for impl in IMPLS:
        res = rhp.parse_batch(buf, off, 16, rhp.MODE_PHR, impl=impl, layout=lay, last_len=z["last_len"])
        assert_same(canon(res, rhp.MODE_PHR), (z["reqs"], z["hdrs"], None), buf, off, f"GPU dense impl{impl} last_len")


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
@pytest.mark.parametrize("name", HTTP_SETS)
def test_gpu_dense_http_matches_reference_golden(name, impl):
    spec, buf, off, want = golden(name)
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    res = rhp.parse_batch(buf, off, spec["max_headers"], spec["mode"], impl=impl, layout=D)
    assert_same(canon(res, spec["mode"]), want, buf, off, f"GPU dense http impl{impl} vs golden {name}")
    if "bytes_out_sha256" in z.files:
        assert hashlib.sha256(res.bytes_out.tobytes()).digest() == z["bytes_out_sha256"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("maxh", [0, 1, 3, 16, 32, 64])
def test_gpu_dense_http_fuzz_vs_oracle(maxh):
    buf, off = rhp.generate(rhp.GEN_FUZZ_HTTP, 60000, 9800 + maxh)
    res = rhp.parse_batch(buf, off, maxh, rhp.MODE_HTTP, layout=D)
    rq, hd, ht, out = run_oracle(buf, off, maxh, rhp.MODE_HTTP)
    assert_same(canon(res, rhp.MODE_HTTP), to_rhp(rq, hd, ht, rhp.MODE_HTTP), buf, off, f"GPU dense http fuzz maxh{maxh}")
    assert (res.bytes_out == out).all()
    emu, _ = rhp.emulate(buf, off, maxh, rhp.MODE_HTTP, D)
    assert np.array_equal(res.reqs["flags"] & (rhp.F_EXACT | rhp.F_WIDE), emu.reqs["flags"] & (rhp.F_EXACT | rhp.F_WIDE))


@functools.lru_cache(maxsize=None)
def http_limits_emulated_flags(shift, maxh, lay, times):
    """(F_EXACT | F_WIDE of the expanded records, the raw dense flag bytes) of the emulator"""
    buf, off, _, _ = http_limits(shift, maxh, times)
    emu, _ = rhp.emulate(buf, off, maxh, rhp.MODE_HTTP, lay)
    return emu.reqs["flags"] & (rhp.F_EXACT | rhp.F_WIDE), dense_fields(emu, len(off) - 1)[0].copy()


@pytest.mark.gpu
@pytest.mark.parametrize("lay", HTTP_LAYS)
@pytest.mark.parametrize("impl", IMPLS)
@pytest.mark.parametrize("maxh", LIMIT_MAXH)
@pytest.mark.parametrize("shift", LIMIT_SHIFTS)
def test_gpu_dense_http_field_limits(shift, maxh, impl, lay):
    """batches.http_field_limits() x 20 (6000 requests, several workgroups) in
    http mode: records and de-framed bytes equal the oracle's in the layouts the
    product ships (dense: config 5; compact; request-major: the reactor, packed
    by rhp_pack_dense), by every kernel; the DFA kernel's choice of path (and in
    the dense layout its flag bytes) equals the emulator's."""
    buf, off, _, _ = http_limits(shift, maxh, 20)
    res = rhp.parse_batch(buf, off, maxh, rhp.MODE_HTTP, impl=impl, layout=lay)
    check_http_limits(res, shift, maxh, 20, f"GPU http limits impl{impl} layout{lay} shift{shift} maxh{maxh}")
    if impl != rhp.IMPL_EXACT:
        want_flags, want_dense = http_limits_emulated_flags(shift, maxh, lay, 20)
        assert np.array_equal(res.reqs["flags"] & (rhp.F_EXACT | rhp.F_WIDE), want_flags)
        if lay == D:
            assert np.array_equal(dense_fields(res, len(off) - 1)[0], want_dense)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["config5_post1k_http_h16", "chunked_post_http_h16"])
def test_gpu_dense_http_full_size_matches_reference_digest(name):
    spec = FULL[name]
    buf, off = inputs(spec)
    res = rhp.parse_batch(buf, off, spec["max_headers"], spec["mode"], layout=D)
    got = canon(res, spec["mode"])
    if record_digest(*got) != spec["records_sha256"]:
        want = to_rhp(*run_oracle(buf, off, spec["max_headers"], spec["mode"])[:3], spec["mode"])
        assert_same(got, want, buf, off, name)
        raise AssertionError(f"{name}: dense digest differs from the reference but matches the oracle")
    if "bytes_out_sha256" in spec:
        assert hashlib.sha256(res.bytes_out.tobytes()).hexdigest() == spec["bytes_out_sha256"]


# ---------------------------------------------------------------------------
# rhp_pack_dense (include/rhp.h): the dense copies of a request-major http
# batch's records, what the reactor copies back (reactor/batch.c)

def check_pack(res, n, maxh):
    """the packed copies of `res` (rhp_cpu_pack_dense) rebuild its records where
    they claim to; returns how many requests were dense"""
    dreq, hc, lens = rhp.pack_dense_cpu(res, n, maxh)
    d = dreq.reshape(n, 8)
    c = hc.reshape(n, 8)
    lens = lens.reshape(maxh, n) if maxh else lens[:0].reshape(0, n)
    dense = 0
    for i in range(n):
        r, x = res.reqs[i], res.http[i]
        cons = int(r["ret"]) + (int(x["body_len"]) if x["body_kind"] == 1 else 0) if x["result"] == 1 else 0
        compact = (int(x["consumed"]) == cons and x["body_kind"] <= 1 and int(x["body_len"]) < 1 << 32
                   and (x["result"] != 1 or r["ret"] > 0))
        if c[i, 2] & rhp.HTTP_WIDE:
            assert not compact, i
        else:
            assert compact, i
            assert int(np.int8(c[i, 0])) == x["result"] and c[i, 1] == x["body_kind"], i
            assert int(c[i, 4:8].view(np.uint32)[0]) == x["body_len"], i
        if d[i, 7] & rhp.DENSE_WIDE:
            continue
        dense += 1
        assert compact and x["result"] == 1, i
        ret, plen = int(d[i, 0:2].view(np.uint16)[0]), int(d[i, 2:4].view(np.uint16)[0])
        assert (ret, plen, d[i, 4], d[i, 5], d[i, 6]) == (r["ret"], r["path_len"], r["method_len"],
                                                         r["num_headers"], r["minor_version"]), i
        assert r["method_off"] == 0 and r["path_off"] == r["method_len"] + 1, i
        at = int(r["path_off"]) + plen + 11
        for k in range(int(d[i, 5])):
            h = res.hdrs[i, k]
            nl, vl = int(lens[k, i]) & 63, int(lens[k, i]) >> 6
            assert (h["name_off"], h["name_len"], h["value_off"], h["value_len"]) == (at, nl, at + nl + 2, vl), (i, k)
            at += nl + vl + 4
    return dense


@pytest.mark.parametrize("name", HTTP_SETS + ["limits"])
def test_pack_dense_cpu_rebuilds_records(name):
    if name == "limits":   # batches.http_field_limits(): names and values on both sides of what lens16 holds
        buf, off, _, _ = http_limits(0, 16)
        n, maxh = len(off) - 1, 16
    else:
        spec, buf, off, _ = golden(name)
        n, maxh = len(off) - 1, spec["max_headers"]
    res = rhp.parse_cpu_exact(buf, off, maxh, rhp.MODE_HTTP)
    dense = check_pack(res, n, maxh)
    if name == "limits":
        assert 0 < dense < n   # (all wide would rebuild nothing)
    assert dense > 0 or "chunked" in name   # (every chunked body de-framed: all wide)


def test_pack_dense_cpu_fixup_chunked_stays_wide():
    """a chunked body de-framed by the fix-up moves its request's bytes: its
    request and http records stay wide"""
    streams = [b"GET /a HTTP/1.1\r\nHost: x\r\n\r\n"
               b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n"
               b"POST /l HTTP/1.1\r\nContent-Length: 3\r\n\r\nabcGET /z HTTP/1.0\r\n\r\n"]
    buf, off, sess, _ = rhp.pack_sessions(streams)
    res, sres, _ = rhp.fixup_cpu(buf, off, sess, 16)
    n = len(off) - 1
    dreq, hc, _ = rhp.pack_dense_cpu(res, n, 16)
    check_pack(res, n, 16)
    slots = range(int(sess[0]["piece_lo"]), int(sess[0]["piece_lo"]) + int(sres[0]["n_slots"]))
    kinds = [(int(res.http[i]["body_kind"]), bool(dreq[8 * i + 7] & rhp.DENSE_WIDE),
              bool(hc[8 * i + 2] & rhp.HTTP_WIDE)) for i in slots]
    assert kinds == [(0, False, False), (1, True, True), (1, False, False), (0, False, False)], kinds


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["golden", "post", "chunked", "fuzz", "limits"])
def test_gpu_pack_dense_equals_cpu_pack(case):
    """rhp_pack_dense on the device's records, byte for byte the CPU pack of
    the same records (their parity with the oracle is the other tests')"""
    if case == "golden":
        spec, buf, off, _ = golden([s for s in HTTP_SETS if "chunked" not in s][0])
        maxh = spec["max_headers"]
    elif case == "limits":
        buf, off, _, _ = http_limits(1, 16, 20)
        maxh = 16
    else:
        gen = {"post": rhp.GEN_POST1K, "chunked": rhp.GEN_CHUNKED, "fuzz": rhp.GEN_FUZZ_HTTP}[case]
        buf, off = rhp.generate(gen, 20000, 77, lo=1000 if case != "fuzz" else 0)
        maxh = 16
    n = len(off) - 1
    db = rhp.DeviceBatch(buf, off, maxh, rhp.MODE_HTTP, layout=rhp.LAYOUT_REQUEST_MAJOR)
    db.launch()
    _, _, _, dense = gpu_pack_equals_cpu_pack(db, n, maxh)
    assert dense > 0 if case != "chunked" else dense == 0   # (de-framed chunked bodies: all wide)
    if case == "limits":
        assert 0 < dense < n   # (all wide would compare nothing)


def gpu_pack_equals_cpu_pack(db, n, maxh, guard=0, fill=None):
    """rhp_pack_dense over the device records of `db` as they are now, compared
    with the CPU pack of the same records fetched; (Result, dreq [n, 8], hc
    [n, 8], how many requests check_pack found dense).  guard, fill: the three
    outputs are rhp.Guarded slices that hold `fill` first, their guards checked."""
    import ctypes
    import torch
    outs = [rhp.Guarded(name, size, guard, fill) for name, size in
            (("dreq", 8 * n), ("hc", 8 * n), ("lens16", 2 * max(maxh * n, 1)))]
    dd, dh, dl = (g.view for g in outs)
    d = db.desc()
    rc = rhp.lib().rhp_pack_dense(ctypes.byref(d), dd.data_ptr(), dh.data_ptr(), dl.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    res = db.result()
    for g in outs:
        g.check()
    want_d, want_h, want_l = rhp.pack_dense_cpu(res, n, maxh)
    got_l = dl.cpu().numpy().view(np.uint16)[: maxh * n]
    assert (dd.cpu().numpy() == want_d).all()
    assert (dh.cpu().numpy() == want_h).all()
    # rows past a request's num_headers are unspecified: compare the used ones
    nh = np.where((want_d.reshape(n, 8)[:, 7] & rhp.DENSE_WIDE) == 0, want_d.reshape(n, 8)[:, 5], 0)
    used = np.arange(maxh)[:, None] < nh[None, :]
    assert (got_l.reshape(maxh, n)[used] == want_l.reshape(maxh, n)[used]).all()
    return res, want_d.reshape(n, 8), want_h.reshape(n, 8), check_pack(res, n, maxh)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["shapes", "mixed"])
def test_gpu_fixup_then_pack_dense(case):
    """a reactor round on the device: speculative parse, rhp_fixup_sessions,
    rhp_pack_dense over the records the fix-up left.  The fix-up's answers are
    the reference loop's; the packed copies are the CPU pack of those records;
    a chunked body de-framed by the fix-up keeps its slot wide in both."""
    import session_sets
    import test_sessions
    if case == "shapes":
        buf, off, sess = session_sets.packed_shapes()
        want = test_sessions.shapes_oracle()
    else:
        buf, off, sess, _ = rhp.pack_sessions(test_sessions.make_sessions(200, 9))
        want = test_sessions.oracle_sessions(buf, off, [(int(a), int(b)) for a, b in sess])
    n = len(off) - 1
    _, results, starts, db = rhp.fixup_gpu(buf, off, sess, 16, with_batch=True)
    res, dreq, hc, dense = gpu_pack_equals_cpu_pack(db, n, 16)
    test_sessions.check(res, results, starts, buf, off, sess, f"gpu fix-up then pack {case}", want=want)
    used = test_sessions.used_slots(sess, results)
    assert 0 < dense < n
    assert 0 < int(((dreq[used, 7] & rhp.DENSE_WIDE) == 0).sum()) < len(used)
    # the slots whose chunked body the fix-up de-framed: the oracle's requests with
    # Transfer-Encoding set, in session order
    chunked = [int(lo) + m for (lo, _), seq in zip(sess, want[0]) for m, q in enumerate(seq)
               if q[0] == 1 and any(name.upper() == b"TRANSFER-ENCODING" and value for name, value in q[5])]
    assert len(chunked) > 10
    assert (res.http["body_kind"][chunked] == 1).all()
    assert (dreq[chunked, 7] & rhp.DENSE_WIDE).all() and (hc[chunked, 2] & rhp.HTTP_WIDE).all()
