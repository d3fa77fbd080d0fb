"""Pipelined input in one batch: every session's input is
split at its empty lines, the pieces are parsed as one speculative batch, and
rhp_fixup_sessions walks each session in order.  The result must equal the
reference's server_session_read loop (server.c:37-65): http_read_request
(http.c:177-234) from the front of the input, advancing by what it consumed,
until it returns 0 or -1 -- here the oracle restatement called per request at
the true boundaries of the same batch buffer (so the bytes after a session are
the same in both), de-framing chunked bodies in place as the reference does.

Streams mix GETs, Content-Length bodies (some holding empty lines and whole
fake requests), chunked bodies (also with empty lines inside), LF-only line
ends, malformed requests and incomplete tails.  CPU: the product's exact host
parser and the kernel's DFA emulation; GPU (-m gpu): the MI355X kernels.

The "session shapes" set (session_sets.py) is built by hand around the
kernel's wave-parallel prefix, which takes a session's leading whole pieces 64
per step before lane 0 walks the rest: 0, 1, 63, 64, 65, 127, 128, 129 or 200
whole pieces (TFB GET, LF-only GET, PUT with Content-Length 0, a POST cut at
its body's end), then nothing, a complete chunked POST, a POST whose body runs
into the next pieces, a partial request, a malformed one, a piece holding two
requests or an empty piece, then 0, 1 or 70 more whole pieces; a session
without pieces and one that is a single empty piece.  On it the fix-up is
held to the reference loop in both rhp_hdr_t layouts (request-major and
header-major: the walk copies header records between slots by the layout's
strides), at header capacities below, at and above what its requests need, on
the host with and without the prefix (rhp_emu_fixup_sessions, the host twin of
rhp_fixup_kernel's prefix, must equal the plain walk record for record), and
on the device, for 1, 3, 4, 5 and 9 sessions too (four sessions per workgroup)."""
import ctypes
import functools

import numpy as np
import pytest

import libreactorng_amd as rhp
import session_sets
from oracle_util import ORC_HDR, ORC_HTTP, ORC_REQ, oracle

LAYOUTS = (rhp.LAYOUT_REQUEST_MAJOR, rhp.LAYOUT_HEADER_MAJOR)
RM, HM = LAYOUTS

TFB = (b"GET /plaintext HTTP/1.1\r\nHost: tfb-server:8080\r\nAccept: text/plain\r\n"
       b"Connection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n\r\n")


def request_pool(rng):
    fake = b"GET /inside-a-body HTTP/1.1\r\nHost: x\r\n\r\n"
    body = b"line one\r\n\r\n" + fake + b"\n\ntail"
    chunk_data = b"ab\r\n\r\ncd"
    pool = [
        TFB,
        b"GET / HTTP/1.1\r\nHost: a\r\n\r\n",
        b"GET /lf HTTP/1.1\nX: y\n\n",
        b"GET /mix HTTP/1.0\r\nA: b\n\r\n",
        b"POST /cl HTTP/1.1\r\nContent-Length: 5\r\n\r\nhello",
        b"POST /cl-empty-lines HTTP/1.1\r\nContent-Length: %d\r\n\r\n" % len(body) + body,
        b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n",
        b"POST /c2 HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n%x\r\n" % len(chunk_data) + chunk_data +
        b"\r\n0\r\n\r\n",
        b"PUT /zero HTTP/1.1\r\nContent-Length: 0\r\n\r\n",
        b"GET /h HTTP/1.1\r\n" + b"".join(b"H%d: v\r\n" % i for i in range(16)) + b"\r\n",
    ]
    bad = [b"GET /x HTTP/1.1\r\nBad Header\r\n\r\n", b"POST /b HTTP/1.1\r\nContent-Length: 3\r\n"
           b"Transfer-Encoding: chunked\r\n\r\nabc", b"GET / HTTP/2.0\r\n\r\n",
           b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\nzz\r\n"]
    tails = [b"GET /last HTTP/1.1\r\nHost:", b"POST /p HTTP/1.1\r\nContent-Length: 100\r\n\r\nonly-part",
             b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhel", b""]
    return pool, bad, tails


def make_sessions(n_sessions, seed):
    rng = np.random.default_rng(seed)
    pool, bad, tails = request_pool(rng)
    out = []
    for _ in range(n_sessions):
        k = int(rng.integers(1, 40))
        parts = [pool[int(rng.integers(len(pool)))] for _ in range(k)]
        if rng.random() < 0.1:
            parts.insert(int(rng.integers(len(parts) + 1)), bad[int(rng.integers(len(bad)))])
        parts.append(tails[int(rng.integers(len(tails)))])
        out.append(b"".join(parts))
    return out


def oracle_sessions(buf, off, sessions, max_headers=16):
    """Per session: [(result, start, consumed, method, path, fields, body)] of the
    reference's loop, and the batch bytes after it (chunked bodies de-framed)."""
    o = oracle()
    rw = buf.copy()
    reqs = np.zeros(1, dtype=ORC_REQ)
    hdrs = np.zeros((1, max_headers), dtype=ORC_HDR)
    http = np.zeros(1, dtype=ORC_HTTP)
    one = np.zeros(2, dtype=np.uint64)
    out = []
    for lo, hi in sessions:
        pos, end, seq = int(off[lo]), int(off[hi]), []
        while pos < end:
            one[0], one[1] = pos, end
            o.orc_http_batch(rw.ctypes.data, one.ctypes.data, 1, max_headers, reqs.ctypes.data, hdrs.ctypes.data,
                             http.ctypes.data)
            res = int(http["result"][0])
            r = reqs[0]
            if res == 1 and r["ret"] > rhp.RHP_MAX_LEN:
                res = rhp.RHP_RET_TOOLONG
            if res != 1:
                seq.append((res, pos, 0, None, None, None, None))
                break
            b = bytes(rw[pos:end])
            fields = [(b"" if no < 0 else b[no:no + nl], b[vo:vo + vl])
                      for no, nl, vo, vl in hdrs[0][: int(r["num_headers"])].tolist()]
            body = b""
            if http["body_kind"][0]:
                bo = int(http["body_off"][0])
                body = b[bo:bo + int(http["body_len"][0])]
            c = int(http["consumed"][0])
            seq.append((1, pos, c, b[r["method_off"]:r["method_off"] + r["method_len"]],
                        b[r["path_off"]:r["path_off"] + r["path_len"]], fields, body))
            pos += c
        out.append(seq)
    return out, rw


def product_sessions(res, results, starts, off, sessions, allow_more=False):
    """The same view of rhp_fixup_sessions' output."""
    out = []
    rw = res.bytes_out.tobytes()
    # (plain Python values: field access on numpy records is most of this function's time)
    http = {f: res.http[f].tolist() for f in res.http.dtype.names}
    reqs = {f: res.reqs[f].tolist() for f in res.reqs.dtype.names}
    for (lo, hi), sr in zip(sessions, results):
        end, seq = int(off[hi]), []
        for m in range(int(sr["n_slots"])):
            i = lo + m
            pos = int(starts[i])
            if http["result"][i] != 1:
                seq.append((http["result"][i], pos, 0, None, None, None, None))
                break
            b = rw[pos:end]
            fields = [(b"" if no == rhp.RHP_NAME_NULL else b[no:no + nl], b[vo:vo + vl])
                      for no, nl, vo, vl in res.hdrs[i][: reqs["num_headers"][i]].tolist()]
            ret = reqs["ret"][i]
            body = b[ret:ret + http["body_len"][i]] if http["body_kind"][i] else b""
            mo, po = reqs["method_off"][i], reqs["path_off"][i]
            seq.append((1, pos, http["consumed"][i], b[mo:mo + reqs["method_len"][i]], b[po:po + reqs["path_len"][i]],
                        fields, body))
        assert allow_more or not sr["more"]
        out.append(seq)
    return out


def check(res, results, starts, buf, off, sess, label, allow_more=False, max_headers=16, want=None):
    """`want`: oracle_sessions(buf, off, sessions, max_headers) where a caller shares it"""
    sessions = [(int(a), int(b)) for a, b in sess]
    want, want_bytes = want if want is not None else oracle_sessions(buf, off, sessions, max_headers)
    got = product_sessions(res, results, starts, off, sessions, allow_more)
    if allow_more:   # a session that ran out of pieces: its first n_slots requests, the rest in a later batch
        want = [w[: len(g)] if sr["more"] else w for g, w, sr in zip(got, want, results)]
        want_bytes = None
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{label}: session {k}: first difference at request " \
                       f"{next(i for i in range(min(len(g), len(w)) + 1) if i >= min(len(g), len(w)) or g[i] != w[i])}"
    n = int(off[-1])
    if want_bytes is not None:
        assert bytes(res.bytes_out[:n]) == bytes(want_bytes[:n]), f"{label}: de-framed bytes differ"
    return sum(len(w) for w in want)


def test_split_pieces():
    assert rhp.split_pieces(b"GET / HTTP/1.1\r\n\r\nGET / HTTP/1.1\n\nX") == [18, 16, 1]
    assert rhp.split_pieces(b"") == [0]
    assert rhp.split_pieces(b"abc") == [3]
    assert rhp.split_pieces(b"A\n\r\n") == [4]


def cpu_matches_reference_loop(seed, emulate_dfa, layout):
    data = make_sessions(60, seed)
    buf, off, sess, _ = rhp.pack_sessions(data)
    res, results, starts = rhp.fixup_cpu(buf, off, sess, 16, emulate_dfa, layout)
    total = check(res, results, starts, buf, off, sess, f"cpu seed {seed} layout {layout}")
    assert total > 60


@pytest.mark.parametrize("emulate_dfa", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fixup_cpu_matches_reference_loop(seed, emulate_dfa):
    cpu_matches_reference_loop(seed, emulate_dfa, RM)


@pytest.mark.parametrize("emulate_dfa", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fixup_cpu_matches_reference_loop_header_major(seed, emulate_dfa):
    cpu_matches_reference_loop(seed, emulate_dfa, HM)


def test_fixup_cpu_unsplit_sessions():
    """One piece per session: the first request of each is the piece's own
    speculative result (chunked bodies validated, then de-framed by the
    fix-up: RHP_BODY_CHUNKED_PENDING), the rest runs out of pieces (more)."""
    data = make_sessions(80, 9)
    buf, off, sess, _ = rhp.pack_sessions(data, split=False)
    res, results, starts = rhp.fixup_cpu(buf, off, sess)
    assert results["more"].sum() > 0
    check(res, results, starts, buf, off, sess, "unsplit", allow_more=True)


def merged_split(seed):
    """A split coarser than the server's: runs of 1-3 consecutive server pieces
    merged, so a piece may hold several requests and the walk meets request
    boundaries inside pieces whose records an earlier request overwrote."""
    rng = np.random.default_rng(seed)

    def split(data):
        p, out = rhp.split_pieces(data), []
        while p:
            k = int(rng.integers(1, 4))
            out.append(sum(p[:k]))
            p = p[k:]
        return out
    return split


def cpu_partly_merged_split(emulate_dfa, layout):
    data = make_sessions(80, 11)
    buf, off, sess, _ = rhp.pack_sessions(data, split=merged_split(11))
    res, results, starts = rhp.fixup_cpu(buf, off, sess, 16, emulate_dfa, layout)
    check(res, results, starts, buf, off, sess, f"merged layout {layout}", allow_more=True)


@pytest.mark.parametrize("emulate_dfa", [False, True])
def test_fixup_cpu_partly_merged_split(emulate_dfa):
    """Pieces that each hold up to three requests: requests past a
    piece's first are parsed again from their true boundary, never read from
    record slots the walk has already overwritten; sessions that run out of
    pieces report `more`."""
    cpu_partly_merged_split(emulate_dfa, RM)


@pytest.mark.parametrize("emulate_dfa", [False, True])
def test_fixup_cpu_partly_merged_split_header_major(emulate_dfa):
    cpu_partly_merged_split(emulate_dfa, HM)


def cpu_every_chunking_of_one_stream(layout):
    rng = np.random.default_rng(5)
    pool, _, _ = request_pool(rng)
    stream = b"".join(pool)
    data = [stream[:k] for k in range(0, len(stream) + 1, 7)]
    buf, off, sess, _ = rhp.pack_sessions(data)
    res, results, starts = rhp.fixup_cpu(buf, off, sess, layout=layout)
    check(res, results, starts, buf, off, sess, f"prefixes layout {layout}")


def test_fixup_cpu_every_chunking_of_one_stream():
    """One pipelined stream cut at every position into (delivered, rest): the
    delivered part as one session, as a server round sees a partial recv."""
    cpu_every_chunking_of_one_stream(RM)


def test_fixup_cpu_every_chunking_of_one_stream_header_major():
    cpu_every_chunking_of_one_stream(HM)


# ---------------------------------------------------------------------------
# The session shapes set (session_sets.py)

@functools.lru_cache(maxsize=None)
def _shapes_oracle(max_headers, first):
    buf, off, sess = session_sets.packed_shapes(first)
    return oracle_sessions(buf, off, [(int(a), int(b)) for a, b in sess], max_headers)


def shapes_oracle(max_headers=16, first=None):
    """oracle_sessions of session_sets.packed_shapes(first), computed once per
    capacity; check() reads it and leaves it as it is"""
    return _shapes_oracle(max_headers, first)


def used_slots(sess, results):
    """the record slots a fix-up filled: piece_lo .. piece_lo + n_slots of every session"""
    return np.concatenate([np.arange(int(lo), int(lo) + int(k)) for (lo, _), k in zip(sess, results["n_slots"])] +
                          [np.zeros(0, dtype=np.int64)]).astype(np.int64)


def assert_same_fixup(a, b, sess, n, label, every_row=True):
    """two fix-ups of one batch, (Result, session results, req_start) each,
    agree exactly: the rhp_session_result_t array, req_start of the used slots,
    their reqs / http / hdrs records and the de-framed bytes.  every_row=False
    (two different parsers of the pieces): header rows below num_headers of
    requests with ret > 0 only -- what a parser leaves in the rows past a
    request's headers is unspecified (rhp.h)."""
    (ra, sa, ta), (rb, sb, tb) = a, b
    assert np.array_equal(sa, sb), f"{label}: session results differ at {np.flatnonzero(sa != sb)[:5]}"
    u = used_slots(sess, sa)
    assert np.array_equal(ta[u], tb[u]), f"{label}: req_start differs"
    assert np.array_equal(ra.http[u], rb.http[u]), f"{label}: http records differ at {u[ra.http[u] != rb.http[u]][:5]}"
    assert np.array_equal(ra.reqs[u], rb.reqs[u]), f"{label}: request records differ at {u[ra.reqs[u] != rb.reqs[u]][:5]}"
    ha, hb = np.ascontiguousarray(ra.hdrs[u]), np.ascontiguousarray(rb.hdrs[u])
    if not every_row:
        nh = np.where(ra.reqs["ret"][u] > 0, ra.reqs["num_headers"][u], 0)
        rows = np.arange(ha.shape[1])[None, :] < nh[:, None]
        ha, hb = ha[rows], hb[rows]
    assert np.array_equal(ha, hb), f"{label}: header records differ"
    assert np.array_equal(ra.bytes_out[:n], rb.bytes_out[:n]), f"{label}: de-framed bytes differ"


def test_session_shapes_cover_every_step_and_stopper():
    """the set is what its description says, measured on the speculative parse
    by the kernel's own predicate (rhp_scalar.h fixup_piece_whole)"""
    shapes = session_sets.shapes()
    buf, off, sess = session_sets.packed_shapes()
    b, res = rhp.speculative_cpu(buf, off, 16)
    whole = rhp.whole_pieces(b)
    x = res.raw_http.view(rhp.HTTP_DTYPE)[: b.n].copy()   # the speculative records, before the fix-up rewrites them
    _, results, _ = rhp.fixup_host(b, res, sess)
    lead = []
    for lo, hi in sess:
        k = 0
        while lo + k < hi and whole[lo + k]:
            k += 1
        lead.append(k)
    assert set(session_sets.LEADS) >= {0, 1, 63, 64, 65, 127, 128, 129, 200}
    assert set(session_sets.LEADS) <= set(lead), sorted(set(lead))
    # every session's leading run is its LEAD (with no stopper, the tail too)
    for (ld, stopper, tail, _, lens), k, (lo, hi) in zip(shapes, lead, sess):
        assert hi - lo == len(lens)
        if ld is not None:
            assert k == (ld + tail if stopper == "none" else ld), (ld, stopper, tail, k)
    assert {s[1] for s in shapes} == set(session_sets.STOPPERS) | {"no_piece", "one_empty_piece"}
    # the stoppers are what their names say, on the piece after a lead of 64
    at = {s[1]: int(sess[i]["piece_lo"]) + 64 for i, s in enumerate(shapes) if s[0] == 64 and s[2] == 1}
    plen = off[1:] - off[:-1]
    assert x["result"][at["chunked"]] == 1 and x["body_kind"][at["chunked"]] == rhp.BODY_CHUNKED_PENDING
    assert x["result"][at["cl_split"]] == 0 and plen[at["cl_split"]] > 0
    assert x["result"][at["partial"]] == 0 and x["result"][at["bad"]] == -1
    assert x["result"][at["two"]] == 1 and 0 < x["consumed"][at["two"]] < plen[at["two"]] and plen[at["two"] + 1] == 0
    assert plen[at["empty_piece"]] == 0 and whole[at["empty_piece"] + 1]
    # taken whole by the prefix alone, in more than one step
    assert any(hi > lo and k == hi - lo >= 64 for k, (lo, hi) in zip(lead, sess))
    assert any(hi == lo for lo, hi in sess) and any(hi == lo + 1 and off[hi] == off[lo] for lo, hi in sess)
    assert not results["more"].any()
    # a workgroup's four sessions take different paths
    assert all(len({s[1] for s in shapes[i:i + 4]}) == 4 for i in range(0, len(shapes) - 3, 4))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("emulate_dfa", [False, True])
@pytest.mark.parametrize("prefix", [False, True])
def test_fixup_cpu_shapes_match_reference_loop(prefix, emulate_dfa, layout):
    buf, off, sess = session_sets.packed_shapes()
    res, results, starts = rhp.fixup_cpu(buf, off, sess, 16, emulate_dfa, layout, prefix)
    total = check(res, results, starts, buf, off, sess, f"shapes prefix {prefix} dfa {emulate_dfa} layout {layout}",
                  want=shapes_oracle())
    assert total > 20000


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("emulate_dfa", [False, True])
def test_fixup_cpu_prefix_equals_plain_walk(emulate_dfa, layout):
    """rhp_emu_fixup_sessions (the kernel's prefix, then the walk from where it
    stopped) leaves what the walk from every session's first piece leaves"""
    buf, off, sess = session_sets.packed_shapes()
    plain = rhp.fixup_cpu(buf, off, sess, 16, emulate_dfa, layout, prefix=False)
    twin = rhp.fixup_cpu(buf, off, sess, 16, emulate_dfa, layout, prefix=True)
    assert_same_fixup(twin, plain, sess, int(off[-1]), f"prefix vs plain dfa {emulate_dfa} layout {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fixup_cpu_prefix_leaves_a_request_past_its_piece_to_the_walk(layout):
    """records written by hand: a result-1 record whose consumed is larger than
    its piece (no parser of a piece gives one; the walk's own test is consumed
    <= piece length) is not a whole piece -- the prefix stops there, and the
    twin equals the plain walk, which parses from that boundary again"""
    data = [session_sets.TFB * 70 + b"GET /last HTTP/1.1\r\nHost:", session_sets.TFB * 3]
    buf, off, sess, _ = rhp.pack_sessions(data)
    out = []
    for prefix in (False, True):
        b, res = rhp.speculative_cpu(buf, off, 16, False, layout)
        http = res.raw_http.view(rhp.HTTP_DTYPE)
        assert http["result"][66] == 1 and http["consumed"][66] == len(session_sets.TFB)
        http["consumed"][66] += len(session_sets.TFB)
        assert not rhp.whole_pieces(b)[66] and rhp.whole_pieces(b)[:66].all()
        out.append(rhp.fixup_host(b, res, sess, prefix))
    assert_same_fixup(out[1], out[0], sess, int(off[-1]), f"overlong consumed layout {layout}")
    check(*out[1], buf, off, sess, f"overlong consumed layout {layout}")


CAPACITIES = (0, 3, 4, 16, 64)


def capacity_case(which):
    """(buf, off, sess, the oracle's answer at capacity m) of a capacity sweep's input"""
    if which == "shapes":
        return session_sets.packed_shapes() + (shapes_oracle,)
    buf, off, sess, _ = rhp.pack_sessions(make_sessions(60, which))
    return buf, off, sess, lambda m: None


def check_tfb_capacity(res, results, sess, maxh, label):
    """the TFB GET has exactly 4 headers: a session that starts with it stops
    with -1 in its first slot at a capacity of 3, and goes on at 4"""
    first = [i for i, s in enumerate(session_sets.shapes()) if s[3].startswith(session_sets.TFB)]
    assert len(first) > 10 and session_sets.TFB_HEADERS == 4
    for i in first:
        lo = int(sess[i]["piece_lo"])
        if maxh < 4:
            assert results["n_slots"][i] == 1 and res.http["result"][lo] == -1, f"{label}: session {i}"
        else:
            assert res.http["result"][lo] == 1 and res.reqs["num_headers"][lo] == 4, f"{label}: session {i}"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("maxh", CAPACITIES)
@pytest.mark.parametrize("which", ["shapes", 21])
def test_fixup_cpu_header_capacity(which, maxh, layout):
    """a request with more headers than the records hold stops its session with
    -1 exactly where the reference's loop does, called at the same capacity"""
    buf, off, sess, want = capacity_case(which)
    label = f"cpu {which} max_headers {maxh} layout {layout}"
    plain = rhp.fixup_cpu(buf, off, sess, maxh, False, layout, prefix=False)
    twin = rhp.fixup_cpu(buf, off, sess, maxh, True, layout, prefix=True)   # (the DFA emulation, and the prefix)
    check(*plain, buf, off, sess, label, max_headers=maxh, want=want(maxh))
    check(*twin, buf, off, sess, label + " twin", max_headers=maxh, want=want(maxh))
    if which == "shapes":
        check_tfb_capacity(plain[0], plain[1], sess, maxh, label)
        check_tfb_capacity(twin[0], twin[1], sess, maxh, label + " twin")


# ---------------------------------------------------------------------------
# GPU

def gpu_matches_reference_loop(seed, impl, layout):
    data = make_sessions(400, seed)
    buf, off, sess, _ = rhp.pack_sessions(data)
    res, results, starts = rhp.fixup_gpu(buf, off, sess, 16, impl, layout)
    total = check(res, results, starts, buf, off, sess, f"gpu impl{impl} seed {seed} layout {layout}")
    assert total > 400


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fixup_gpu_matches_reference_loop(seed, impl):
    gpu_matches_reference_loop(seed, impl, RM)


@pytest.mark.gpu
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_fixup_gpu_matches_reference_loop_header_major(seed, impl):
    gpu_matches_reference_loop(seed, impl, HM)


def gpu_unsplit_sessions(layout):
    data = make_sessions(200, 9)
    buf, off, sess, _ = rhp.pack_sessions(data, split=False)
    res, results, starts = rhp.fixup_gpu(buf, off, sess, layout=layout)
    assert results["more"].sum() > 0
    check(res, results, starts, buf, off, sess, f"gpu unsplit layout {layout}", allow_more=True)


@pytest.mark.gpu
def test_fixup_gpu_unsplit_sessions():
    gpu_unsplit_sessions(RM)


@pytest.mark.gpu
def test_fixup_gpu_unsplit_sessions_header_major():
    gpu_unsplit_sessions(HM)


def gpu_partly_merged_split(layout):
    data = make_sessions(300, 12)
    buf, off, sess, _ = rhp.pack_sessions(data, split=merged_split(12))
    res, results, starts = rhp.fixup_gpu(buf, off, sess, layout=layout)
    check(res, results, starts, buf, off, sess, f"gpu merged layout {layout}", allow_more=True)


@pytest.mark.gpu
def test_fixup_gpu_partly_merged_split():
    gpu_partly_merged_split(RM)


@pytest.mark.gpu
def test_fixup_gpu_partly_merged_split_header_major():
    gpu_partly_merged_split(HM)


def gpu_prefixes(layout):
    rng = np.random.default_rng(5)
    pool, _, _ = request_pool(rng)
    stream = b"".join(pool) * 3
    data = [stream[:k] for k in range(0, len(stream) + 1, 3)]
    buf, off, sess, _ = rhp.pack_sessions(data)
    res, results, starts = rhp.fixup_gpu(buf, off, sess, layout=layout)
    check(res, results, starts, buf, off, sess, f"gpu prefixes layout {layout}")


@pytest.mark.gpu
def test_fixup_gpu_prefixes():
    gpu_prefixes(RM)


@pytest.mark.gpu
def test_fixup_gpu_prefixes_header_major():
    gpu_prefixes(HM)


def gpu_shapes(first, maxh, impl, layout, guard=0):
    """the shapes set (or its first sessions) on the device: the reference loop's
    answers, and record for record what the host twin of the kernel leaves
    (guard: rhp.fixup_gpu's, guards beside every buffer the two kernels write)"""
    buf, off, sess = session_sets.packed_shapes(first)
    label = f"gpu shapes first {first} max_headers {maxh} impl{impl} layout {layout}"
    got = rhp.fixup_gpu(buf, off, sess, maxh, impl, layout, guard=guard)
    check(*got, buf, off, sess, label, max_headers=maxh, want=shapes_oracle(maxh, first))
    twin = rhp.fixup_cpu(buf, off, sess, maxh, impl == rhp.IMPL_DFA, layout, prefix=True)
    assert_same_fixup(got, twin, sess, int(off[-1]), label + " vs host twin", every_row=False)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
def test_fixup_gpu_shapes_match_reference_loop_and_host_twin(impl, layout):
    gpu_shapes(None, 16, impl, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("first", [1, 3, 4, 5, 9])
def test_fixup_gpu_session_counts(first, layout):
    """four sessions (waves) per workgroup: a workgroup's waves past the last
    session, one session, a full workgroup, one more; the third session has no
    piece and the sixth is one empty piece"""
    res, results, _ = gpu_shapes(first, 16, rhp.IMPL_DFA, layout)
    assert len(results) == first and results["n_slots"][0] == 65
    if first >= 3:
        assert results["n_slots"][2] == 0 and results["consumed"][2] == 0
    if first >= 9:
        assert results["n_slots"][5] == 0 and results["consumed"][5] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("maxh", [0, 3, 4, 64])
def test_fixup_gpu_header_capacity(maxh, layout):
    res, results, _ = gpu_shapes(None, maxh, rhp.IMPL_DFA, layout)
    buf, off, sess = session_sets.packed_shapes()
    check_tfb_capacity(res, results, sess, maxh, f"gpu max_headers {maxh} layout {layout}")


