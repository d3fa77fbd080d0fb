"""rhp_write_responses (rhp_writer.hip) at the shapes where its branches switch.

The response batches of tests/test_responses.py have short statuses, types and
fields and allocator-aligned pointers.  Here: make_responses "edge" and
"edge-coop" (span lengths around every step of the copy loops, every source
alignment, empty spans at the arena's end), `out` and `arena` at every
alignment, a group of 64 on either side of the stage threshold, groups of one
to three responses, every digit count of Content-Length, more than 1024 scan
tiles with offsets past 2^32, an output one byte too small, and another date.

CPU: the oracle (oracle/rhp_oracle.c orc_write_responses) against the compiled
reference on the new kinds where /root/reference is present (everywhere:
tests/golden/responses.json pins both kinds to the reference's digests,
tests/test_responses.py), and a numpy restatement of the size the reference
allocates (http.c:244-246, 270-272) against the oracle's offsets.
GPU (-m gpu): offsets and bytes equal the oracle's (the size function's where
the output is too large to allocate); every run that writes has guard bytes on
both sides of `out` and finds them untouched.
"""
import functools
import os

import numpy as np
import pytest

import libreactorng_amd as rhp
from oracle_util import oracle_write_responses, reference, reference_write_responses

GUARD = 64
EDGE_NS = (1, 63, 64, 65, 127, 4095, 4096, 4097)
COOP_NS = (64, 1000)
KSTAGE = 16384   # rhp_writer.hip kStage: a group goes through LDS when its bytes + (out + G0) % 16 <= kStage


def response_sizes(resps, fields):
    """u64[n]: the bytes http_write_response allocates for each response,
    9 + 2 + 11 + 37 + 16 + 18 + 2 = 95 and the status, type, body and the
    digits of the body's length (http.c:244-246), and name + 2 + value + 2 for
    every extra field (http.c:270-272)"""
    resps = np.asarray(resps).reshape(-1, 8)
    body = resps[:, 5].astype(np.uint64)
    digits = np.ones(len(resps), dtype=np.uint64)
    for k in range(1, 10):
        digits += body >= np.uint64(10 ** k)
    fl = np.asarray(fields).reshape(-1, 4)
    run = np.zeros(len(fl) + 1, dtype=np.uint64)
    run[1:] = np.cumsum(fl[:, 1].astype(np.uint64) + fl[:, 3].astype(np.uint64) + np.uint64(4))
    first, count = resps[:, 6].astype(np.int64), resps[:, 7].astype(np.int64)
    first = np.where(count > 0, first, 0)
    extra = run[first + count] - run[first]
    return np.uint64(95) + resps[:, 1].astype(np.uint64) + resps[:, 3].astype(np.uint64) + body + digits + extra


def size_offsets(resps, fields):
    off = np.zeros(len(resps) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(response_sizes(resps, fields))
    return off


@functools.lru_cache(maxsize=None)
def edge(kind, n, date=rhp.DEFAULT_DATE):
    """(arena, resps, fields, oracle bytes, oracle offsets) of one seeded batch; shared, never written"""
    arena, resps, fields = rhp.make_responses(n, 7000 + n, kind)
    want, woff = oracle_write_responses(arena, resps, fields, date)
    for a in (arena, resps, fields, want, woff):
        a.flags.writeable = False
    return arena, resps, fields, want, woff


def gpu_write(arena, resps, fields, **kw):
    """one rhp_write_responses with guards around `out`: (bytes, offsets), the guards checked"""
    d = rhp.DeviceResponses(arena, resps, fields, guard=GUARD, **kw)
    d.launch()
    got, off, before, after = d.result()
    assert len(before) == GUARD and len(after) == GUARD
    assert (before == d.GUARD_BYTE).all(), "bytes before `out` were written"
    assert (after == d.GUARD_BYTE).all(), "bytes after out + out_size were written"
    return got, off


def check_gpu(arena, resps, fields, want, woff, label="", **kw):
    got, off = gpu_write(arena, resps, fields, **kw)
    assert np.array_equal(off, woff), f"{label}: offsets differ"
    assert len(got) == len(want), label
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(np.searchsorted(woff, bad[0], side="right")) - 1
        raise AssertionError(f"{label}: {len(bad)} bytes differ, the first at {int(bad[0])}, "
                             f"{int(bad[0]) - int(woff[i])} into response {i} {resps[i]}")


# ------------------------------------------------------------------ CPU


@pytest.mark.parametrize("kind", ["edge", "edge-coop"])
def test_edge_generator_shape(kind):
    """what the "edge" kinds promise (make_responses): the length sets, every
    source alignment, empty spans at the arena's end, the field counts"""
    arena, resps, fields = rhp.make_responses(4097, 11, kind)
    spans = np.concatenate([resps[:, 0:2], resps[:, 2:4], fields[:, 0:2], fields[:, 2:4]])
    assert set(spans[:, 1]) == set(rhp.EDGE_SPAN_LENS)
    body = resps[:, 5]
    if kind == "edge-coop":
        assert (body[::64] == rhp.EDGE_COOP_BODY).all()
        body = np.delete(body, np.arange(0, len(body), 64))
    assert set(body) == set(rhp.EDGE_SPAN_LENS) | set(rhp.EDGE_BODY_LENS)
    every = np.concatenate([spans, resps[:, 4:6]]).astype(np.int64)
    assert (every[:, 0] + every[:, 1] <= len(arena)).all()
    for ln in (1, 17, 129, 1025):   # every source alignment at short, odd and long lengths
        assert set(spans[spans[:, 1] == ln][:, 0] & 3) == {0, 1, 2, 3}
    empty = every[every[:, 1] == 0]
    assert 0 < (empty[:, 0] == len(arena)).sum() < len(empty)
    assert set(resps[:, 7]) == set(rhp.EDGE_FIELD_COUNTS)
    assert np.array_equal(resps[:, 6], np.cumsum(resps[:, 7]) - resps[:, 7]) and resps[:, 7].sum() == len(fields)
    again = rhp.make_responses(4097, 11, kind)
    assert all(np.array_equal(a, b) for a, b in zip((arena, resps, fields), again))


def test_unknown_response_kind_is_an_error():
    with pytest.raises(ValueError):
        rhp.make_responses(4, 1, "edgy")


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="needs /root/reference (dev container)")
def test_oracle_matches_reference_on_edge_kinds():
    assert reference() is not None
    date2 = bytes(range(65, 94))
    for kind, ns in (("edge", EDGE_NS), ("edge-coop", COOP_NS)):
        for n in ns:
            arena, resps, fields, want, woff = edge(kind, n)
            out, off = reference_write_responses(arena, resps, fields)
            assert np.array_equal(off, woff) and np.array_equal(out, want), (kind, n)
    for kind, n in (("edge", 200), ("edge-coop", 130)):
        arena, resps, fields, want, woff = edge(kind, n, date2)
        out, off = reference_write_responses(arena, resps, fields, date2)
        assert np.array_equal(off, woff) and np.array_equal(out, want), (kind, n)
    for batch in (digits_batch(), one_line_batch(3)) + tuple(threshold_batch(w, KSTAGE) for w in WHERE):
        o1, f1 = oracle_write_responses(*batch)
        o2, f2 = reference_write_responses(*batch)
        assert np.array_equal(f1, f2) and np.array_equal(o1, o2)


def test_size_function_matches_oracle_offsets():
    for kind, ns in (("edge", EDGE_NS), ("edge-coop", COOP_NS)):
        for n in ns:
            arena, resps, fields, _, woff = edge(kind, n)
            assert np.array_equal(size_offsets(resps, fields), woff), (kind, n)
    arena, resps, fields = digits_batch()
    assert np.array_equal(size_offsets(resps, fields), oracle_write_responses(arena, resps, fields)[1])
    # the digit counts the oracle's output is too large for: by hand (95 + 6 + 10 = 111 and the body and its digits)
    arena, resps, fields = digits_batch(SIZE_ONLY_BODIES)
    assert list(response_sizes(resps, fields)) == [111 + v + len(str(v)) for v in SIZE_ONLY_BODIES]


# ------------------------------------------------------------------ batches built by hand


def span_pool(size, seed):
    return np.random.default_rng(seed).integers(0x20, 0x7F, size=size, dtype=np.uint8)


WHERE = ("body", "status", "type", "value")
LONG_AT, LONG_OFF = 37, 5   # the long response's place in its group; its span's arena offset (source alignment 1)


def threshold_batch(where, total):
    """A group of 64 responses of `total` bytes in all, 63 of them minimal (96
    bytes: no status, type, fields or body) and one with a long body, status,
    type or field value, then a group of 10 ordinary responses."""
    arena = span_pool(20000, 41)
    resps = np.zeros((74, 8), dtype=np.uint32)
    fields = [[0, 0, 0, 0]]   # (record 0 is the long response's)
    rest = total - 63 * 96
    if where == "body":
        ln = rest - 95 - 5
        assert 10000 <= ln <= 99999   # five digits
        resps[LONG_AT, 4:6] = (LONG_OFF, ln)
    elif where == "value":
        fields[0] = [3, 3, LONG_OFF, rest - 96 - 3 - 4]
        resps[LONG_AT, 6:8] = (0, 1)
    else:
        col = {"status": 0, "type": 2}[where]
        resps[LONG_AT, col:col + 2] = (LONG_OFF, rest - 96)
    rng = np.random.default_rng(42)
    for i in range(64, 74):
        nf = int(rng.integers(0, 3))
        resps[i] = [rng.integers(0, 1000), rng.integers(0, 30), rng.integers(0, 1000), rng.integers(0, 30),
                    rng.integers(0, 1000), rng.integers(0, 300), len(fields), nf]
        fields += [[rng.integers(0, 1000), rng.integers(0, 20), rng.integers(0, 1000), rng.integers(0, 50)]
                   for _ in range(nf)]
    return arena, resps, np.array(fields, dtype=np.uint32)


def one_line_batch(n):
    """1 to 3 responses, the first two minimal (96 bytes), the third with a
    1-byte status, a 2-byte type and a 3-byte body"""
    arena = np.frombuffer(b"?abcdefg", dtype=np.uint8).copy()
    resps = np.zeros((n, 8), dtype=np.uint32)
    if n == 3:
        resps[2, :6] = (1, 1, 2, 2, 4, 3)
    return arena, resps, np.zeros((0, 4), dtype=np.uint32)


WRITTEN_BODIES = (0, 1) + tuple(v for k in range(1, 8) for v in (10 ** k - 1, 10 ** k))
SIZE_ONLY_BODIES = (10 ** 8 - 1, 10 ** 8, 10 ** 9 - 1, 10 ** 9, 2 ** 32 - 1)
DIGITS_ARENA = 10 ** 7


@functools.lru_cache(maxsize=None)
def digits_batch(bodies=WRITTEN_BODIES):
    """one response per body length; the bodies alias one 10 MB arena span (at
    every source alignment where they leave room for it)"""
    arena = np.concatenate([span_pool(DIGITS_ARENA, 43), np.frombuffer(b"200 OKtext/plain", dtype=np.uint8)])
    arena.flags.writeable = False
    resps = np.zeros((len(bodies), 8), dtype=np.uint32)
    for i, v in enumerate(bodies):
        resps[i, :6] = (DIGITS_ARENA, 6, DIGITS_ARENA + 6, 10, i % 4 if v + 3 <= DIGITS_ARENA else 0, v)
    return arena, resps, np.zeros((0, 4), dtype=np.uint32)


def clipped_edge(clip):
    """the "edge" batch of 1000 with every span cut to `clip` bytes (the starts
    stay), so that groups of 64 fit the stage"""
    arena, resps, fields, _, _ = edge("edge", 1000)
    resps, fields = resps.copy(), fields.copy()
    for a, cols in ((resps, (1, 3, 5)), (fields, (1, 3))):
        for c in cols:
            a[:, c] = np.minimum(a[:, c], clip)
    return arena, resps, fields


# ------------------------------------------------------------------ GPU


@pytest.mark.gpu
@pytest.mark.parametrize("kind,n", [("edge", n) for n in EDGE_NS] + [("edge-coop", n) for n in COOP_NS])
def test_gpu_writer_edge_lengths(kind, n):
    arena, resps, fields, want, woff = edge(kind, n)
    if kind == "edge-coop":   # every group is larger than the stage at any alignment
        assert (woff[np.minimum(np.arange(64, n + 64, 64), n)] - woff[np.arange(0, n, 64)] > KSTAGE).all()
    check_gpu(arena, resps, fields, want, woff, f"{kind} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [5, 17, 33])
def test_gpu_writer_staged_short_spans(clip):
    """The "edge" spans cut short, so that groups of 64 go through the LDS stage:
    st_span at every source alignment, at lengths 0-5 (and 15-17, 31-33) that
    are no multiples of 4, empty spans at the arena's end.  clip 5 also puts a
    body of 9 ... 1000 bytes into every group (Content-Length of 1-4 digits
    printed by the stage path; 5 digits: test_gpu_writer_stage_threshold)."""
    arena, resps, fields = clipped_edge(clip)
    if clip == 5:
        resps[7::64, 5] = np.resize((9, 10, 99, 100, 999, 1000), len(resps[7::64]))
    want, woff = oracle_write_responses(arena, resps, fields)
    group = woff[np.minimum(np.arange(64, 1064, 64), 1000)] - woff[np.arange(0, 1000, 64)]
    staged = group + 15 <= KSTAGE
    assert staged.sum() >= (14 if clip < 33 else 1), group
    for out_shift, arena_shift in ((0, 0), (9, 1), (3, 2), (14, 3)):
        check_gpu(arena, resps, fields, want, woff, f"clip {clip} out+{out_shift} arena+{arena_shift}",
                  out_shift=out_shift, arena_shift=arena_shift)


@pytest.mark.gpu
@pytest.mark.parametrize("arena_shift", [0, 1, 2, 3])
@pytest.mark.parametrize("out_shift", [1, 7, 8, 15])
def test_gpu_writer_misaligned_pointers(out_shift, arena_shift):
    """`out` and `arena` off their allocations' alignment (the arena's bytes
    moved with it: the expected output is the same)"""
    for kind, n in (("edge", 300), ("edge-coop", 130)):
        arena, resps, fields, want, woff = edge(kind, n)
        check_gpu(arena, resps, fields, want, woff, f"{kind} out+{out_shift} arena+{arena_shift}",
                  out_shift=out_shift, arena_shift=arena_shift)


@pytest.mark.gpu
@pytest.mark.parametrize("where", WHERE)
def test_gpu_writer_stage_threshold(where):
    """A group whose bytes + (out + G0) % 16 are kStage - 1 and kStage (staged
    through LDS) and kStage + 1 (written response by response), at four
    alignments of `out`, the long part a body, a status, a type or a field value
    (st_span below the threshold, put() >= 128 B above it); a second group after
    it, whose first bytes a store past the group's end would hit."""
    for s in (0, 1, 8, 15):
        for total in (KSTAGE - s - 1, KSTAGE - s, KSTAGE - s + 1):
            arena, resps, fields = threshold_batch(where, total)
            want, woff = oracle_write_responses(arena, resps, fields)
            assert int(woff[64]) == total
            check_gpu(arena, resps, fields, want, woff, f"{where} shift {s} group of {total} B", out_shift=s)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3])
def test_gpu_writer_one_line_group(n):
    """The smallest groups (96, 192 and 294 bytes) at all 16 alignments of
    `out`: 0-15 head and tail bytes around a store window A0..A1 of 5 to 18
    lines.  (No group is shorter than 96 bytes, so A0 < A1 always holds: the
    kernel's byte-only branch for a group within one line cannot be reached
    through rhp_write_responses.)"""
    arena, resps, fields = one_line_batch(n)
    want, woff = oracle_write_responses(arena, resps, fields)
    assert int(woff[-1]) == (96, 192, 294)[n - 1]
    for s in range(16):
        check_gpu(arena, resps, fields, want, woff, f"n={n} out+{s}", out_shift=s)


@pytest.mark.gpu
def test_gpu_writer_content_length_digits():
    """Content-Length of 1 to 8 digits written (bodies of 0, 1, 9, 10, 99, 100,
    ... 9 999 999, 10 000 000 bytes, about 22 MB of output) and compared with
    the oracle; 8 to 10 digits (10^8 - 1, 10^8, 10^9 - 1, 10^9, 2^32 - 1) as
    sizes only (out NULL, out_size 0) against response_sizes.  Written output
    for 9- and 10-digit lengths is out of scope: it takes 1 GB or more."""
    arena, resps, fields = digits_batch()
    want, woff = oracle_write_responses(arena, resps, fields)
    assert len(want) > 22_000_000
    check_gpu(arena, resps, fields, want, woff, "digits")
    arena, resps, fields = digits_batch(SIZE_ONLY_BODIES)
    d = rhp.DeviceResponses(arena, resps, fields, out_size=0)
    assert d.desc().out is None
    d.launch()
    off = d.out_off.cpu().numpy().view(np.uint64)
    assert np.array_equal(off, size_offsets(resps, fields))


@pytest.mark.gpu
def test_gpu_writer_scan_many_tiles():
    """1024 * 4096 + 4097 responses: 1026 scan tiles, so the top scan's second
    round and its carry, a last tile of one response, and offsets past 2^32.
    Sizes only (out NULL, out_size 0) against response_sizes."""
    n = 1024 * 4096 + 4097
    rng = np.random.default_rng(44)
    arena = span_pool(64, 45)
    fields = np.zeros((8, 4), dtype=np.uint32)
    fields[:, 1], fields[:, 3] = rng.integers(0, 13, 8), rng.integers(0, 48, 8)
    resps = np.zeros((n, 8), dtype=np.uint32)
    resps[:, 1] = rng.integers(0, 41, n, dtype=np.uint32)
    resps[:, 3] = 10
    resps[:, 5] = rng.integers(0, 4001, n, dtype=np.uint32)
    resps[:, 7] = rng.integers(0, 3, n, dtype=np.uint32)
    resps[:, 6] = rng.integers(0, 7, n, dtype=np.uint32)   # first + count <= 8
    want = size_offsets(resps, fields)
    assert int(want[-1]) > 2 ** 32
    d = rhp.DeviceResponses(arena, resps, fields, out_size=0)
    d.launch()
    off = d.out_off.cpu().numpy().view(np.uint64)
    assert int(off[n]) > 2 ** 32
    assert np.array_equal(off, want), f"first difference at {int(np.flatnonzero(off != want)[0])}"


@pytest.mark.gpu
def test_gpu_writer_out_size_one_short():
    """out_size one byte less than the total: the offsets are complete and
    nothing is written (out_size == total is every other test here)"""
    for kind, n in (("edge", 200), ("edge-coop", 130)):
        arena, resps, fields, want, woff = edge(kind, n)
        d = rhp.DeviceResponses(arena, resps, fields, out_size=len(want) - 1, guard=GUARD, out_shift=3)
        d.launch()
        _, off, before, after = d.result()
        assert np.array_equal(off, woff)
        assert not d.out.cpu().numpy().any()
        assert (before == d.GUARD_BYTE).all() and (after == d.GUARD_BYTE).all()


@pytest.mark.gpu
def test_gpu_writer_date_bytes():
    date = bytes(range(65, 94))
    assert len(date) == rhp.RHP_DATE_LEN
    for kind, n in (("edge", 200), ("edge-coop", 130)):
        arena, resps, fields, want, woff = edge(kind, n, date)
        assert b"\r\nDate: " + date + b"\r\n" in bytes(want[: int(woff[1])])
        check_gpu(arena, resps, fields, want, woff, f"{kind} date", date=date)
    arena, resps, fields = clipped_edge(5)   # the stage path's date bytes
    want, woff = oracle_write_responses(arena, resps, fields, date)
    check_gpu(arena, resps, fields, want, woff, "clipped date", date=date, out_shift=5)
