"""rhp_decode_chunked (include/rhp.h): batched, resumable phr_decode_chunked.

The expected values are the compiled reference's own, recorded in tests/golden/decode_chunked.npz by
tests/golden/make_golden_decode_chunked.py (phr_decode_chunked called piece after piece on every stream of every
set of tests/decode_chunked_sets.py).  A record is one call; held to it, value for value -- ret, size, the whole
decoder and every byte of the piece:
  CPU  the host twin rhp_cpu_decode_chunked (a set as one batch, packed as the device gets it), the pointer-based
       rhp_phr_decode_chunked, the live reference where oracle/_ref/libref.so is built; the refusals of
       rhp_chunked_args.h; corrupt decoders; a sanitizer build of the twins as a stand-alone program; a
       lane-by-lane model of the wave's overlapping move against memmove
  GPU  the kernel on every set as one launch, results poisoned first and guard bytes on both sides of bytes,
       decoders and results; the multi-call streams chained on the device; all single-call records in one launch
       behind a non-zero offsets[0]; offsets that run past bytes_size
tests/test_decode_chunked_sweep.py holds twins, live reference and kernel to two sweeps whose expected values follow
from how their pieces are built (tests/decode_chunked_sweep.py), not from the golden file: the overlapping move at
every (gap, destination offset mod 16, length) around the 128-byte threshold and the 1 KiB step edges, gaps 1, 8 and
13..17 among them, and every scanning state entered at every lane of the 64-byte window, its token ending in that
window, at its end and in the ones behind it -- complete, cut into two calls, and wrong.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import decode_chunked_sets as ds
import decode_chunked_sweep as sw

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "decode_chunked.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
GUARD = 256
FILLER = 0xEE   # what a batch holds in front of its first piece


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for a in g.values():
        a.setflags(write=False)
    return g


SET_NAMES = [str(x) for x in golden()["set_name"]]


def record(r):
    """(piece before, decoder before [1], piece after, ret, size, decoder after [1]) of record r"""
    g = golden()
    lo, hi = int(g["rec_lo"][r]), int(g["rec_lo"][r + 1])
    dec = lambda k: g[k][16 * r: 16 * r + 16].view(rhp.CHUNKED_DTYPE)
    return g["before"][lo:hi], dec("dec_before"), g["after"][lo:hi], int(g["ret"][r]), int(g["size"][r]), dec("dec_after")


def pack(recs, start):
    """the records as one batch, pieces back to back from byte `start` on: (bytes, offsets, decoders) before, and
    (bytes, results, decoders) as the reference leaves them"""
    rs = [record(r) for r in recs]
    front = np.full(start, FILLER, dtype=np.uint8)
    off = (start + np.cumsum([0] + [len(x[0]) for x in rs])).astype(np.uint64)
    cat = lambda k, dt: np.concatenate([x[k] for x in rs]) if rs else np.zeros(0, dtype=dt)
    res = np.array([(x[3], x[4]) for x in rs], dtype=rhp.CHUNKED_RESULT_DTYPE)
    return ((np.concatenate([front, cat(0, np.uint8)]), off, cat(1, rhp.CHUNKED_DTYPE)),
            (np.concatenate([front, cat(2, np.uint8)]), res, cat(5, rhp.CHUNKED_DTYPE)))


@functools.lru_cache(maxsize=None)
def golden_set(name):
    """(record indices, first-call flags, start, the batch before, the batch after) of one set"""
    g = golden()
    s = SET_NAMES.index(name)
    lo, hi = int(g["set_lo"][s]), int(g["set_lo"][s + 1])
    recs, start = g["item_rec"][lo:hi], int(g["set_start"][s])
    return (recs, g["item_first"][lo:hi], start) + pack(recs, start)


def same(what, got, want, off=None):
    """results, decoders and bytes of a batch against the reference's"""
    (res, dec, by), (wby, wres, wdec) = got, want
    for f in ("ret", "size"):
        bad = np.flatnonzero(res[f] != wres[f])
        assert not len(bad), f"{what}: {f} of piece {int(bad[0])} is {int(res[f][bad[0]])}, the reference's {int(wres[f][bad[0]])} ({len(bad)} differ)"
    bad = np.flatnonzero(dec.view(np.uint8).reshape(-1, 16) != wdec.view(np.uint8).reshape(-1, 16))
    assert not len(bad), f"{what}: the decoder of piece {int(bad[0]) // 16} is {dec[int(bad[0]) // 16]}, the reference's {wdec[int(bad[0]) // 16]}"
    bad = np.flatnonzero(by != wby)
    if len(bad):
        at = int(bad[0])
        i = int(np.searchsorted(off, at, side="right")) - 1 if off is not None else -1
        raise AssertionError(f"{what}: byte {at} (piece {i}, its byte {at - int(off[i]) if i >= 0 else at}) is {int(by[at])}, "
                             f"the reference's {int(wby[at])} ({len(bad)} differ)")


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_sets():
    """the golden file's pieces, decoders-before, starts and call order are what tests/decode_chunked_sets.py
    builds; the decoder before a later call is the reference's after the call before it"""
    sets = ds.all_sets()
    assert [s[0] for s in sets] == SET_NAMES
    for name, start, streams in sets:
        recs, first, gstart, _, _ = golden_set(name)
        calls = [(s, r) for s in streams for r in range(len(s.pieces))]
        assert gstart == start and len(calls) == len(recs), name
        prev = None
        for (s, r), rec, f in zip(calls, recs, first):
            before, dbefore, _, _, _, dafter = record(int(rec))
            assert bytes(before) == s.pieces[r] and int(f) == (r == 0), name
            assert dbefore.tobytes() == (ds.fresh_decoder(s) if r == 0 else prev), name
            prev = dafter.tobytes()


def test_golden_covers_what_the_sets_are_for():
    """the reference's answers that the sets exist to produce are in the file"""
    g = golden()
    ret, size = g["ret"], g["size"]
    state = g["dec_after"].view(rhp.CHUNKED_DTYPE)["state"]
    hexc = g["dec_after"].view(rhp.CHUNKED_DTYPE)["hex_count"]
    plen = np.diff(g["rec_lo"]).astype(np.int64)
    changed = np.array([not np.array_equal(g["before"][a:b], g["after"][a:b]) for a, b in zip(g["rec_lo"][:-1], g["rec_lo"][1:])])
    for st in range(6):
        assert ((state == st) & (ret == -2)).any(), f"state {st} carried across a call"
    assert ((ret == -2) & (state == ds.SIZE) & (hexc > 0) & (hexc < 16)).any(), "hex_count in the middle of the digits"
    assert ((ret >= 0) & (state == ds.EXT)).any() and ((ret >= 0) & (state == ds.TRAILER_HEAD)).any(), "both ends of a body"
    assert {0, 1, 300} <= set(ret[ret >= 0].tolist())
    assert ((ret == -1) & (state == ds.SIZE) & (hexc == 16)).any(), "a 17th digit"
    assert ((ret == -1) & (state == ds.SIZE) & (hexc == 0)).any() and ((ret == -1) & (state == ds.CRLF)).any()
    assert ((ret == -1) & changed & (size > 0)).any(), "the closing move after -1"
    assert ((ret > 0) & changed).any() and ((ret == -2) & (plen == 0)).any()
    assert (size[ret == -2] <= plen[ret == -2]).all() and size.max() >= 70000
    left = g["dec_after"].view(rhp.CHUNKED_DTYPE)["bytes_left_in_chunk"]
    assert ((state == ds.DATA) & (left > 0) & (ret == -2)).sum() >= 3 and left.max() == 2 ** 64 - 1 - 40
    recs, first, _, _, (_, wres, _) = golden_set("prefixes")
    end = len(ds.CUT_BODY) - len(b"LEFTOVER")
    assert (wres["ret"][:end] == -2).all() and wres["ret"][end:].tolist() == list(range(9)), "every proper prefix of the body is -2"
    for n in ds.BATCH_SIZES:
        recs, _, _, _, (_, wres, _) = golden_set(f"n{n}")
        assert len(recs) == n and all(wres["ret"][j] == -2 and wres["size"][j] == 0 for j in range(3, n, 7))
    recs, first, _, ((_, off, _)), _ = golden_set("overlap")
    big = [j for j in range(len(recs)) if off[j + 1] - off[j] > 6000]
    assert len(big) == 64 and sorted({(int(off[j]) % 16) for j in big}) == list(range(16))
    assert all(golden()["size"][recs[j]] == 6000 for j in big)
    f = golden_set("fuzz")[4][1]["ret"]
    assert (f >= 0).sum() > 50 and (f == -1).sum() > 50 and (f == -2).sum() > 50


@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_twin_equals_golden(name):
    _, _, _, (buf, off, dec), want = golden_set(name)
    same(f"rhp_cpu_decode_chunked {name}", rhp.decode_chunked_cpu(buf, off, dec), want, off)


def every_record(call, what):
    for r in range(len(golden()["ret"])):
        before, dbefore, after, ret, size, dafter = record(r)
        piece, dec = before.copy(), dbefore.copy()
        got = call(dec, piece)
        assert got == (ret, size), f"{what}: record {r}: (ret, size) {got}, the reference's {(ret, size)}"
        assert dec.tobytes() == dafter.tobytes(), f"{what}: record {r}: the decoder is {dec}, the reference's {dafter}"
        assert np.array_equal(piece, after), f"{what}: record {r}: the piece's bytes differ from the reference's"


def test_pointer_twin_equals_golden():
    every_record(rhp.phr_decode_chunked_cpu, "rhp_phr_decode_chunked")
    h = rhp.host()
    for st in range(6):
        d = np.zeros(1, dtype=rhp.CHUNKED_DTYPE)
        d["state"] = st
        assert h.rhp_phr_decode_chunked_is_in_data(d.ctypes.data) == (st == ds.DATA)


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
def test_live_reference_equals_golden():
    """the compiled reference, called now, against the file"""
    from golden.make_golden_decode_chunked import reference
    ref = reference()

    def call(dec, piece):
        sz = ctypes.c_size_t(piece.size)
        ret = ref.phr_decode_chunked(dec.ctypes.data, piece.ctypes.data, ctypes.byref(sz))
        return int(ret), int(sz.value)
    every_record(call, "the live reference")


# corrupt decoders (rhp.h): their expected values are the contract's, not the reference's (it asserts on the
# first and cannot leave the second): ret -1, size 0, the piece and the decoder untouched
CORRUPT = [dict(state=6), dict(state=255), dict(hex_count=17), dict(state=3, hex_count=255)]


def corrupt_batch():
    """a good piece on either side of each corrupt one"""
    body = np.frombuffer(b"3\r\nabc\r\n0\r\nrest", dtype=np.uint8)
    n = 2 * len(CORRUPT) + 1
    dec = np.zeros(n, dtype=rhp.CHUNKED_DTYPE)
    dec["reserved"] = [9, 8, 7, 6, 5]
    for k, c in enumerate(CORRUPT):
        for f, v in c.items():
            dec[2 * k + 1][f] = v
        dec[2 * k + 1]["bytes_left_in_chunk"] = 0x1122334455667788
    off = (len(body) * np.arange(n + 1)).astype(np.uint64)
    buf = np.tile(body, n)
    wres = np.array([(4, 3), (-1, 0)] * len(CORRUPT) + [(4, 3)], dtype=rhp.CHUNKED_RESULT_DTYPE)
    wdec = dec.copy()
    wdec["state"][0::2] = ds.EXT
    wby = buf.reshape(n, -1).copy()
    wby[0::2, :7] = np.frombuffer(b"abcrest", dtype=np.uint8)
    return (buf, off, dec), (wby.reshape(-1), wres, wdec)


def test_corrupt_decoders_cpu():
    (buf, off, dec), want = corrupt_batch()
    same("rhp_cpu_decode_chunked, corrupt decoders", rhp.decode_chunked_cpu(buf, off, dec), want, off)
    for k in range(len(CORRUPT)):
        piece, d = buf[: int(off[1])].copy(), dec[2 * k + 1: 2 * k + 2].copy()
        assert rhp.phr_decode_chunked_cpu(d, piece) == (-1, 0)
        assert d.tobytes() == dec[2 * k + 1: 2 * k + 2].tobytes() and np.array_equal(piece, buf[: int(off[1])])


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls and
    n == 0 go to the GPU library here: any other accepted one would launch a kernel over host memory"""
    gpu = which == "gpu-library"
    fn = (lambda b: rhp.lib().rhp_decode_chunked(b, None)) if gpu else (lambda b: rhp.host().rhp_cpu_decode_chunked(b))
    aligned = lambda size, fill: (lambda raw: raw[(-raw.ctypes.data) % 16:][:size])(np.full(size + 16, fill, dtype=np.uint8))
    buf = aligned(64, 0)
    buf[:11] = np.frombuffer(b"3\r\nabc\r\n0\r\n", dtype=np.uint8)
    off = np.array([0, 11, 11], dtype=np.uint64)
    dec, res = aligned(32, 0), aligned(32, 0x77)
    p = lambda a: a.ctypes.data

    def call(**kw):
        f = dict(bytes=p(buf), offsets=p(off), bytes_size=buf.size, n=2, reserved=0, decoders=p(dec), results=p(res))
        f.update(kw)
        return fn(ctypes.byref(rhp.ChunkedBatch(*(f[k] for k, _ in rhp.ChunkedBatch._fields_))))

    E = -22
    assert fn(None) == E
    for f in ("bytes", "offsets", "decoders", "results"):
        assert call(**{f: None}) == E, f
    assert call(reserved=1) == E and call(reserved=0x80000000) == E and call(n=0, reserved=1) == E
    if gpu:   # the device's alone: whole 16-byte records and lines counted from bytes
        for f, a in (("bytes", buf), ("decoders", dec), ("results", res)):
            assert call(**{f: p(a) + 8}) == E and call(**{f: p(a) + 1}) == E, f
    assert (res == 0x77).all() and not dec.any() and buf[0] == ord("3"), "a refused call writes nothing"
    # accepted: an empty batch asks no pointer and launches nothing
    assert call(n=0) == 0 and call(n=0, bytes=None, offsets=None, decoders=None, results=None, bytes_size=0) == 0
    assert (res == 0x77).all() and not dec.any()
    if gpu:
        return
    # accepted by the host twin: any alignment
    ubuf = np.concatenate([np.zeros(1, dtype=np.uint8), buf[:11]])
    udec, ures = np.zeros(33, dtype=np.uint8), np.zeros(33, dtype=np.uint8)
    assert call(bytes=p(ubuf) + 1, bytes_size=11, decoders=p(udec) + 1, results=p(ures) + 1) == 0
    got = ures[1:].view(rhp.CHUNKED_RESULT_DTYPE)
    assert got["ret"].tolist() == [0, -2] and got["size"].tolist() == [3, 0] and bytes(ubuf[1:4]) == b"abc"


def test_host_twins_asan_ubsan_clean():
    """`make decode-chunked-asan`: a stand-alone program over the host sources (tests/decode_chunked_host_test.c)
    that runs the batch twin and the pointer-based function over the golden file"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "decode-chunked-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "decode_chunked_host_test OK" in out.stdout


def wave_move(mem, d, s, n, log):
    """rhp_device::put (csrc/rhp_device.h) as the wave runs it, the schedule the kernel's moves have: mem[d, d + n)
    <- mem[s, s + n), lane by lane (a row per lane), step by step in ascending order; in every step all lanes'
    loads (gathers) come before any lane's store (one scatter).  Steps: below 128 bytes a byte per lane, 64 bytes a
    step.  Otherwise the bytes up to the first 16-aligned destination (lane l < head: byte l); then 1 KiB steps,
    lane l of step t storing the 16 bytes at head + 1024 t + 16 l, aligned, put together from the five aligned
    source dwords around them (the fifth is loaded only where the source's dwords reach it, else it is zero;
    alignbyte drops the bytes outside the lane's 16); then the tail bytes.
    log: [lowest load, highest load + 1, lowest store, highest store + 1]."""
    lanes = np.arange(64)

    def loaded(idx):
        if idx.size:
            log[0], log[1] = min(log[0], int(idx.min())), max(log[1], int(idx.max()) + 1)
        return mem[idx]

    def store(idx, v):
        log[2], log[3] = min(log[2], int(idx.min())), max(log[3], int(idx.max()) + 1)
        mem[idx] = v

    def byte_steps(lo, hi):
        for j in range(lo, hi, 64):
            k = j + lanes[lanes < hi - j]
            v = loaded(s + k)
            store(d + k, v)

    if n < 128:
        return byte_steps(0, n)
    head = (16 - d % 16) % 16
    byte_steps(0, head)
    body = (n - head) & ~15
    sa = s + head
    base, sh = sa & ~3, sa & 3
    nd = (sh + (n - head) + 3) >> 2
    for t in range(0, body, 1024):
        j = t + 16 * lanes
        j = j[j < body]
        k = j >> 2
        idx = base + 4 * k[:, None] + np.arange(20)[None, :]
        fifth = k + 4 < nd
        w = np.zeros((len(k), 20), dtype=np.uint8)
        w[:, :16] = loaded(idx[:, :16])
        w[fifth, 16:] = loaded(idx[fifth, 16:])
        store(d + head + j[:, None] + np.arange(16)[None, :], w[:, sh: sh + 16])
    byte_steps(head + body, n)


def test_wave_move_model_equals_memmove():
    """the overlap argument of DESIGN.md 3.10 run as a model: for every gap 1..40, every destination offset mod 16
    and lengths 0..200, 1000..1100 and 2040..2060 the wave's move leaves what memmove leaves, no store leaves
    [dst, dst + len) and no load leaves the aligned dwords that hold the source.  The lengths of the move sweep
    (tests/decode_chunked_sweep.py, up to 2084) are run here too; test_gpu_move_sweep runs that sweep's gaps, offsets
    and lengths through the compiled put on the device."""
    lengths = sorted(set(range(0, 201)) | set(range(1000, 1101)) | set(range(2040, 2061)) | set(sw.MOVE_LENGTHS))
    rng = np.random.default_rng(5)
    orig = rng.integers(0, 256, 64 + 16 + 40 + max(lengths) + 64, dtype=np.uint8)
    for gap in range(1, 41):
        for o in range(16):
            d = 64 + o
            s = d + gap
            for n in lengths:
                mem = orig.copy()
                log = [1 << 30, 0, 1 << 30, 0]
                wave_move(mem, d, s, n, log)
                want = orig.copy()
                want[d: d + n] = orig[s: s + n]
                assert np.array_equal(mem, want), (gap, o, n)
                if n:
                    assert d <= log[2] and log[3] <= d + n, ("a store outside the destination", gap, o, n, log)
                    assert (s & ~3) <= log[0] and log[1] <= ((s + n + 3) & ~3), ("a load outside the source's dwords", gap, o, n, log)


# ---------------------------------------------------------------------------
# GPU: the kernel against the golden file


@pytest.mark.gpu
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_equals_golden(name):
    """one launch per set with the golden decoders-before; results poisoned first (an unwritten ret is no answer's
    value), guard bytes beside bytes, decoders and results; the bytes in front of the first piece stay too"""
    _, _, _, (buf, off, dec), want = golden_set(name)
    same(f"rhp_decode_chunked {name}", rhp.decode_chunked_gpu(buf, off, dec, guard=GUARD), want, off)


@pytest.mark.gpu
def test_gpu_chains_streams_on_the_device():
    """the multi-call streams of every set, round after round: round r holds call r of every stream that has one,
    and its decoders are the device's own from round r - 1 (they never leave HBM)"""
    import torch
    g = golden()
    streams = []
    for name in SET_NAMES:
        recs, first, _, _, _ = golden_set(name)
        starts = list(np.flatnonzero(first)) + [len(recs)]
        streams += [recs[a:b] for a, b in zip(starts[:-1], starts[1:]) if b - a > 1]
    assert len(streams) > 400 and max(map(len, streams)) == 3
    n = len(streams)
    dec0 = np.concatenate([record(int(s[0]))[1] for s in streams])
    ddec = torch.from_numpy(dec0.view(np.uint8).copy()).to("cuda")
    for r in range(3):
        live = [k for k, s in enumerate(streams) if len(s) > r]
        empty = np.zeros(0, dtype=np.uint8)
        pieces = [record(int(s[r])) if len(s) > r else None for s in streams]
        off = np.cumsum([0] + [len(p[0]) if p else 0 for p in pieces]).astype(np.uint64)
        buf = np.concatenate([p[0] if p else empty for p in pieces])
        dbuf = torch.from_numpy(buf.copy()).to("cuda")
        doff = torch.from_numpy(off.view(np.int64).copy()).to("cuda")
        dres = torch.full((16 * n,), rhp.CHUNKED_POISON, dtype=torch.uint8, device="cuda")
        before = ddec.cpu().numpy().view(rhp.CHUNKED_DTYPE).copy()
        rhp.decode_chunked_device(dbuf, buf.size, doff, n, ddec, dres)
        torch.cuda.synchronize()
        res, dec, by = dres.cpu().numpy().view(rhp.CHUNKED_RESULT_DTYPE), ddec.cpu().numpy().view(rhp.CHUNKED_DTYPE), dbuf.cpu().numpy()
        assert np.array_equal(by, np.concatenate([p[2] if p else empty for p in pieces])), f"round {r}: the bytes"
        for k in live:
            assert (int(res["ret"][k]), int(res["size"][k])) == pieces[k][3:5], (r, k)
            assert dec[k: k + 1].tobytes() == pieces[k][5].tobytes(), (r, k)
        done = [k for k in range(n) if k not in set(live)]   # a finished stream's empty piece: -2, the decoder as it was
        assert (res["ret"][done] == -2).all() and (res["size"][done] == 0).all() and dec[done].tobytes() == before[done].tobytes()


@pytest.mark.gpu
def test_gpu_all_single_calls_in_one_launch():
    """every record once, as one batch whose first piece starts at byte 37"""
    recs = np.arange(len(golden()["ret"]))
    (buf, off, dec), want = pack(recs, 37)
    same("rhp_decode_chunked, every record", rhp.decode_chunked_gpu(buf, off, dec, guard=GUARD), want, off)


@pytest.mark.gpu
def test_gpu_offsets_past_bytes_size():
    """offsets that run past bytes_size are clamped (a piece's start and end to bytes_size, the end to at least the
    start): the piece that straddles the end is decoded as far as bytes_size, the ones behind it are empty, and the
    bytes at and beyond bytes_size -- decodable chunks -- are neither moved nor read as input.  The host twin
    gives the same."""
    body = b"5\r\nhello\r\n3\r\nabc\r\n0\r\n"
    L = len(body)
    buf = np.frombuffer(body * 4, dtype=np.uint8)
    size = 2 * L + 6                                             # inside the third body: "5\r\nhel"
    off = np.array([0, L, 2 * L, 3 * L, 4 * L, 2 ** 64 - 1, 2 ** 63, 7], dtype=np.uint64)
    dec = np.zeros(len(off) - 1, dtype=rhp.CHUNKED_DTYPE)
    res, gdec, by = rhp.decode_chunked_gpu(buf, off, dec, guard=GUARD, bytes_size=size)
    assert res["ret"].tolist() == [0, 0, -2, -2, -2, -2, -2] and res["size"].tolist() == [8, 8, 3, 0, 0, 0, 0]
    assert gdec["state"].tolist() == [ds.EXT, ds.EXT, ds.DATA, 0, 0, 0, 0] and gdec["bytes_left_in_chunk"].tolist() == [0, 0, 2, 0, 0, 0, 0]
    want = bytearray(body * 4)
    want[0:8] = want[L: L + 8] = b"helloabc"
    want[2 * L: 2 * L + 3] = b"hel"
    assert bytes(by) == bytes(want)
    tbuf, tdec, tres = buf.copy(), dec.copy(), np.zeros(len(dec), dtype=rhp.CHUNKED_RESULT_DTYPE)
    b = rhp.ChunkedBatch(tbuf.ctypes.data, off.ctypes.data, size, len(dec), 0, tdec.ctypes.data, tres.ctypes.data)
    assert rhp.host().rhp_cpu_decode_chunked(ctypes.byref(b)) == 0
    assert np.array_equal(res, tres) and gdec.tobytes() == tdec.tobytes() and np.array_equal(by, tbuf)


@pytest.mark.gpu
def test_gpu_corrupt_decoders():
    (buf, off, dec), want = corrupt_batch()
    same("rhp_decode_chunked, corrupt decoders", rhp.decode_chunked_gpu(buf, off, dec, guard=GUARD), want, off)
