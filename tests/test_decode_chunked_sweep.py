"""rhp_decode_chunked on the two sweeps of tests/decode_chunked_sweep.py: the wave's move down onto its own source
(rhp_device::put) at every (gap, destination offset mod 16, length) around the 128-byte threshold and the first two
1 KiB step edges, and every scanning state entered at every lane of the 64-byte window with its token ending
inside the window, at its last lane, in the next window and a whole window further on.

The expected values are the builder's: they follow from how a piece is put together (its module docstring has the
rule).  What pins the rule is the pointer twin, itself held to the compiled reference by the golden file
(tests/test_decode_chunked.py), and the live reference where it is built.
  CPU  what the sweeps hold, from the builder's metadata; the pointer twin and the live reference piece by piece,
       the batch twin on each sweep packed as the device gets it
  GPU  each sweep as one launch, results poisoned first and guard bytes beside bytes, decoders and results; the cut
       streams' second pieces in a second launch behind the device's own decoders
"""
from __future__ import annotations

import collections
import ctypes
import functools
import os

import numpy as np
import pytest

import libreactorng_amd as rhp
import decode_chunked_sweep as sw
from test_decode_chunked import FILLER, GUARD, LIBREF, same

START = {"move": 0, "window": 7}   # where a sweep's first piece starts in its batch (the move sweep: 16-aligned)


@functools.lru_cache(maxsize=None)
def sweep(which):
    """the sweep as one batch: keys, first-call flags, pieces, offsets, (bytes, offsets, decoders) before and (bytes,
    results, decoders) as the construction says the call leaves them; built once, read-only"""
    streams = sw.move_sweep() if which == "move" else sw.window_sweep()
    pieces = [p for s in streams for p in s]
    first = np.array([c == 0 for s in streams for c in range(len(s))])
    front = bytes([FILLER]) * START[which]
    off = (len(front) + np.cumsum([0] + [len(p.before) for p in pieces])).astype(np.uint64)
    arr = lambda b, dt=np.uint8: np.frombuffer(b, dtype=dt)
    before = arr(front + b"".join(p.before for p in pieces))
    after = arr(front + b"".join(p.after for p in pieces))
    dec = arr(b"".join(p.dec_before for p in pieces), rhp.CHUNKED_DTYPE)
    wdec = arr(b"".join(p.dec_after for p in pieces), rhp.CHUNKED_DTYPE)
    wres = np.array([(p.ret, p.size) for p in pieces], dtype=rhp.CHUNKED_RESULT_DTYPE)
    for a in (first, off, wres):
        a.setflags(write=False)
    S = collections.namedtuple("S", "keys first pieces off batch want")
    return S([p.key for p in pieces], first, pieces, off, (before, off, dec), (after, wres, wdec))


def first_differing(got, want, off):
    (res, dec, by), (wby, wres, wdec) = got, want
    rows = lambda a: a.view(np.uint8).reshape(-1, 16)
    bad = (res["ret"] != wres["ret"]) | (res["size"] != wres["size"]) | (rows(dec) != rows(wdec)).any(axis=1)
    cand = np.flatnonzero(bad)[:1].tolist()
    b = np.flatnonzero(by != wby)
    if len(b):
        cand.append(max(int(np.searchsorted(off, b[0], side="right")) - 1, 0))
    return min(cand)


def same_named(what, got, want, off, keys):
    """same() of tests/test_decode_chunked.py, its message followed by what the first differing piece is for"""
    try:
        same(what, got, want, off)
    except AssertionError as e:
        i = first_differing(got, want, off)
        raise AssertionError(f"{e}\n  the first differing piece, {i}: {sw.name(keys[i])}") from None


# ---------------------------------------------------------------------------
# CPU


def test_sweeps_hold_what_they_are_for():
    """from the builder's metadata alone (keys and parts), against ranges stated here: a range cut from the builder
    fails this test.
    move: every (gap, offset, length) exactly once, the first framing part of its piece g bytes,
    the data run behind it n bytes, the piece at o mod 16 of the batch -- so gaps 1, 8 and 13..17, which the golden
    sets never move by with 128 bytes or more, at every length from 128 on.
    window: for every state, lane k and distance d a complete and a cut stream (and a wrong one where the state has
    one), the token where the key says: the entry at byte k, the deciding byte at k + d, the cut piece k + d bytes
    long and its decoder after in the state (mid-token).  Crossing cases (k + d >= 64) at all 64 lanes of the four
    states whose token has no bound; IN_CHUNK_SIZE takes at most 16 digits and -1 at the 17th, so its digits cross
    only from lanes 47 on, and do at each of them.  The three digit shapes with digits on both sides of lane 63."""
    m = sweep("move")
    gaps = list(range(1, 25)) + [31, 32, 33, 40, 63, 64, 65]
    lengths = list(range(120, 151)) + list(range(1016, 1061)) + list(range(2040, 2085))
    want = collections.Counter((g, o, n) for g in gaps for o in range(16) for n in lengths)
    have = collections.Counter(k[1:] for k in m.keys if k[0] == "move")
    assert have == want and set(have.values()) == {1}
    for g in (1, 8, 13, 14, 15, 16, 17):
        assert all((g, o, n) in have for o in range(16) for n in (128, 129, 1024 + (-o % 16), 2048 + (-o % 16)))
    for i, (key, p) in enumerate(zip(m.keys, m.pieces)):
        if key[0] != "move":
            assert key[0] == "filler" and p.ret == -1 and p.after == p.before
            continue
        _, g, o, n = key
        (k0, line), (k1, run) = p.parts[:2]
        assert (k0, len(line), k1, len(run), int(m.off[i]) % 16) == (sw.FRAME, g, sw.RUN, n, o), key
        assert p.ret == 5 and p.size == n and p.after[:n] == run and p.after[n: n + 5] == p.before[-5:], key
    assert any(p.dec_before[11:] != bytes(5) for p in m.pieces)

    w = sweep("window")
    at = {k: p for k, p in zip(w.keys, w.pieces)}
    forms = collections.defaultdict(set)
    for state, k, d, form, shape, call in w.keys:
        forms[state, k, d].add((form, call))
    hexd = set(b"0123456789abcdefABCDEF")
    for state in (sw.SIZE, sw.EXT, sw.CRLF, sw.TRAILER_HEAD, sw.TRAILER_MIDDLE):
        for k in range(64):
            ds_ = {0, 1} | set(range(62 - k, 67 - k)) | set(range(126 - k, 131 - k))
            if state == sw.SIZE:
                ds_ = {d for d in ds_ | {16, 17} if d <= 17}
            ds_ = sorted(d for d in ds_ if d >= 0)
            assert sorted(d for (s, kk, d) in forms if (s, kk) == (state, k)) == ds_, (state, k)
            for d in ds_:
                need = {("cut", 0), ("cut", 1), ("wrong", 0) if state == sw.SIZE and d == 0 else ("complete", 0)}
                if state == sw.CRLF:
                    need.add(("wrong", 0))
                assert need <= forms[state, k, d], (state, k, d)
            crossing = [d for d in ds_ if k + d >= 64]
            assert crossing or (state == sw.SIZE and k + 17 < 64), (state, k)
    for (state, k, d, form, shape, call), p in at.items():
        if call:
            assert form == "cut", (state, k, d)
            continue
        b, tok = p.before, p.before[k: k + d]
        if form == "cut":
            mid = state if not (state == sw.EXT and d == 0 and k) else sw.SIZE   # no byte of the extension yet: still in the digits
            assert len(b) == k + min(d, 16 if state == sw.SIZE else d) and p.ret == -2 and p.dec_after[10] == mid, (state, k, d)
            continue
        assert len(b) > k + d
        if state == sw.SIZE:
            assert set(tok) <= hexd and (d == 17 or b[k + d] not in hexd) and (d != 17 or p.ret == -1), (k, d)
            assert (form == "wrong") == (d == 0) and (d != 0 or p.ret == -1)
        elif state in (sw.EXT, sw.TRAILER_MIDDLE):
            assert 10 not in tok and b[k + d] == 10, (state, k, d)
        else:
            assert set(tok) <= {13} and b[k + d] != 13, (state, k, d)
            assert (b[k + d] == 10) == (form == "complete") and (form != "wrong" or p.ret == -1), (state, k, d, form)
    straddle = lambda sel: any(k <= 63 < k + d - 1 for (s, k, d, form, shape, call) in w.keys
                               if s == sw.SIZE and form == "complete" and sel(d, shape))
    assert straddle(lambda d, shape: d == 16 and shape == "sig") and straddle(lambda d, shape: d < 17 and shape == "zeros")
    assert straddle(lambda d, shape: d == 17)
    sig16 = [(k, p) for (s, k, d, form, shape, call), p in at.items() if s == sw.SIZE and d == 16 and shape == "sig" and form == "complete"]
    assert all(len(set(p.before[k: k + 16].lower())) == 16 and p.ret == -2 for k, p in sig16)
    left = np.frombuffer(b"".join(p.dec_after for _, p in sig16), dtype=rhp.CHUNKED_DTYPE)["bytes_left_in_chunk"]
    assert (left >= 1 << 60).all(), "the whole 64-bit value, minus what arrived"
    assert any(p.dec_before[8] for p in w.pieces) and any(p.dec_before[11:] != bytes(5) for p in w.pieces)


def every_piece(which, call, what):
    """call(decoder [1], piece) -> (ret, size), both changed in place, on every piece in stream order; a later call's
    decoder is the one the call in front of it left"""
    s = sweep(which)
    before, off, dec = s.batch
    after, wres, wdec = s.want
    d = None
    for i, key in enumerate(s.keys):
        lo, hi = int(off[i]), int(off[i + 1])
        piece = before[lo:hi].copy()
        d = dec[i: i + 1].copy() if s.first[i] else d
        assert d.tobytes() == dec[i: i + 1].tobytes()
        got = call(d, piece)
        where = f"{what}: piece {i}, {sw.name(key)}"
        assert got == (int(wres["ret"][i]), int(wres["size"][i])), f"{where}: (ret, size) {got}, constructed {wres[i]}"
        assert d.tobytes() == wdec[i: i + 1].tobytes(), f"{where}: the decoder is {d}, constructed {wdec[i]}"
        assert piece.tobytes() == after[lo:hi].tobytes(), f"{where}: the piece's bytes differ from the constructed ones"


@pytest.mark.parametrize("which", ["move", "window"])
def test_pointer_twin_equals_construction(which):
    every_piece(which, rhp.phr_decode_chunked_cpu, "rhp_phr_decode_chunked")


@pytest.mark.parametrize("which", ["move", "window"])
def test_batch_twin_equals_construction(which):
    s = sweep(which)
    same_named(f"rhp_cpu_decode_chunked, {which} sweep", rhp.decode_chunked_cpu(*s.batch), s.want, s.off, s.keys)


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
@pytest.mark.parametrize("which", ["move", "window"])
def test_live_reference_equals_construction(which):
    from golden.make_golden_decode_chunked import reference
    ref = reference()

    def call(dec, piece):
        sz = ctypes.c_size_t(piece.size)
        ret = ref.phr_decode_chunked(dec.ctypes.data, piece.ctypes.data, ctypes.byref(sz))
        return int(ret), int(sz.value)
    every_piece(which, call, "the live reference")


# ---------------------------------------------------------------------------
# GPU


@pytest.mark.gpu
def test_gpu_move_sweep():
    """one launch: every triple's move down onto its own source, and the closing move behind it"""
    s = sweep("move")
    same_named("rhp_decode_chunked, move sweep", rhp.decode_chunked_gpu(*s.batch, guard=GUARD), s.want, s.off, s.keys)


@pytest.mark.gpu
def test_gpu_window_sweep():
    """one launch: every piece of every stream behind its constructed decoder"""
    s = sweep("window")
    same_named("rhp_decode_chunked, window sweep", rhp.decode_chunked_gpu(*s.batch, guard=GUARD), s.want, s.off, s.keys)


@pytest.mark.gpu
def test_gpu_window_sweep_chained():
    """two launches over one decoder per stream that never leaves HBM: every stream's first piece, then the cut
    streams' second pieces (an empty piece for the others: -2, the decoder as it was)"""
    import torch
    s = sweep("window")
    before, off, dec = s.batch
    after, wres, wdec = s.want
    heads = np.flatnonzero(s.first)
    n = len(heads)
    ddec = torch.from_numpy(dec[heads].view(np.uint8).copy()).to("cuda")
    carried = None
    for r in (0, 1):
        idx = [int(h) + r if h + r < len(s.keys) and (r == 0 or not s.first[h + r]) else -1 for h in heads]
        assert r == 0 or sum(i >= 0 for i in idx) == sum(k[3] == "cut" and k[5] == 0 for k in s.keys)
        span = lambda a, i: a[int(off[i]): int(off[i + 1])] if i >= 0 else a[:0]
        roff = np.cumsum([0] + [len(span(before, i)) for i in idx]).astype(np.uint64)
        buf = np.concatenate([span(before, i) for i in idx])
        wby = np.concatenate([span(after, i) for i in idx])
        live = np.array([i >= 0 for i in idx])
        pick = np.array([max(i, 0) for i in idx])
        want_res, want_dec = wres[pick].copy(), wdec[pick].copy()
        want_res[~live] = (-2, 0)
        if r:
            want_dec[~live] = carried[~live]
        dbuf = torch.from_numpy(buf.copy()).to("cuda")
        doff = torch.from_numpy(roff.view(np.int64).copy()).to("cuda")
        dres = torch.full((16 * n,), rhp.CHUNKED_POISON, dtype=torch.uint8, device="cuda")
        rhp.decode_chunked_device(dbuf, buf.size, doff, n, ddec, dres)
        torch.cuda.synchronize()
        got = (dres.cpu().numpy().view(rhp.CHUNKED_RESULT_DTYPE), ddec.cpu().numpy().view(rhp.CHUNKED_DTYPE), dbuf.cpu().numpy())
        keys = [s.keys[i] if i >= 0 else s.keys[int(h)][:5] + ("no second call",) for i, h in zip(idx, heads)]
        same_named(f"rhp_decode_chunked, window sweep, launch {r}", got, (wby, want_res, want_dec), roff, keys)
        carried = want_dec
