"""rhp_classify_sessions (include/rhp.h): header lookup and route match over the
record slots rhp_fixup_sessions leaves in a speculative batch.

The yardstick is tests/golden/classify_sessions.npz: the compiled reference's
own http_field_lookup at the request boundaries of the reference's session
loop, scattered to record slot piece_lo + m, every other slot absent
(tests/golden/make_golden_classify_sessions.py).  CPU tests hold the host twin
(rhp_cpu_classify_sessions, a linear walk over the sessions) to it over the
records of the host exact parser and of the DFA emulation, with and without
the fix-up's prefix twin, in both layouts; GPU tests hold the kernel (a binary
search per slot) to it and to the host twin run over the records the GPU left,
with the record buffers, req_start and the session results poisoned too."""
import ctypes

import numpy as np
import pytest

import libreactorng_amd as rhp
import classify_session_sets as css
from test_classify import same

LAYOUTS = (rhp.LAYOUT_REQUEST_MAJOR, rhp.LAYOUT_HEADER_MAJOR)
MAXH = css.MAX_HEADERS


def in_use(sess, results, n):
    """bool [n]: the record slots of piece_lo .. piece_lo + n_slots of every session"""
    used = np.zeros(n, dtype=bool)
    for (lo, _), k in zip(sess, results["n_slots"]):
        used[int(lo): int(lo) + int(k)] = True
    return used


def test_mixed_set_leaves_matching_records_in_unused_slots():
    """what the set is for: the speculative parse leaves result-1 records in slots
    the fix-up does not use -- pieces that began inside a body, pieces behind a
    -1 -- and some of them match a route; the in-use slots have matches too"""
    buf, off, sess = css.inputs("mixed")
    n = len(off) - 1
    assert 50 <= len(sess) <= 70
    b, res = rhp.speculative_cpu(buf, off, MAXH)
    spec_one = res.raw_http.view(rhp.HTTP_DTYPE)[:n]["result"] == 1   # before the fix-up rewrites the records
    # the speculative records classified one by one, as a non-speculative batch of the pieces
    plain = rhp.Batch.from_buffer_copy(b)
    plain.flags = 0
    _, spec_route = rhp.classify_cpu(plain, css.NAMES, css.ROUTES)
    _, results, _ = rhp.fixup_host(b, res, sess)
    used = in_use(sess, results, n)
    stale = spec_one & ~used
    assert stale.sum() >= 20, int(stale.sum())
    assert (spec_route[stale] == 0).any(), "no unused slot whose stale record is GET /plaintext (behind a -1)"
    assert (spec_route[stale] == 3).any(), "no unused slot whose stale record is GET /inside-a-body"
    wf, wr = css.expected("mixed")
    assert (wr[~used] == rhp.ROUTE_NONE).all() and (wf["value_off"][:, ~used] == rhp.RHP_NAME_NULL).all()
    assert set(wr[used].tolist()) >= {0, 1, 2, rhp.ROUTE_NONE}, "in-use route matches"
    assert not (wr == 3).any(), "GET /inside-a-body is never a request"
    assert ((wf["value_off"] != rhp.RHP_NAME_NULL).sum(axis=1) > 20).all(), "every name is found somewhere"
    assert ((wf["value_off"] != rhp.RHP_NAME_NULL) & (wf["value_len"] == 0)).any(), "an empty value"
    assert not results["more"].any()
    last = np.array([int(lo) + int(k) - 1 for (lo, _), k in zip(sess, results["n_slots"]) if k])
    assert {0, -1} <= set(res.http["result"][last].tolist()), "sessions that stop on 0 and on -1"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("prefix", [False, True])
@pytest.mark.parametrize("emulate_dfa", [False, True])
@pytest.mark.parametrize("name", ["mixed", "shapes"])
def test_cpu_matches_reference(name, emulate_dfa, prefix, layout):
    buf, off, sess = css.inputs(name)
    res, results, starts = rhp.fixup_cpu(buf, off, sess, MAXH, emulate_dfa, layout, prefix)
    got = rhp.classify_sessions_cpu(res, sess, results, starts, css.NAMES, css.ROUTES)
    same(got, css.expected(name), f"{name} dfa {emulate_dfa} prefix {prefix} layout {layout}")


@pytest.mark.parametrize("name", css.GEOMETRY)
def test_cpu_geometry(name):
    buf, off, sess = css.inputs(name)
    res, results, starts = rhp.fixup_cpu(buf, off, sess, MAXH, True, rhp.LAYOUT_HEADER_MAJOR, True)
    got = rhp.classify_sessions_cpu(res, sess, results, starts, css.NAMES, css.ROUTES)
    want = css.expected(name)
    same(got, want, name)
    assert (want[1] == (rhp.ROUTE_NONE if len(sess) == 0 else 0)).all()


def poisoned_fixup_cpu(buf, off, sess, layout):
    """fixup_cpu into record buffers, req_start and session results that held 0xFF"""
    b, res = rhp._host_batch(buf, off, MAXH, rhp.MODE_HTTP, layout, None, rhp.BATCH_SPECULATIVE)
    for a in res.keep[2:5]:
        a[:] = 0xFF
    assert rhp.host().rhp_emu_parse_batch(ctypes.byref(b), None) == 0
    results = np.full(len(sess), 0xFF, dtype=np.uint8).repeat(rhp.SESSION_RESULT_DTYPE.itemsize).view(rhp.SESSION_RESULT_DTYPE)
    starts = np.full(max(b.n, 1), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    rc = rhp.host().rhp_emu_fixup_sessions(ctypes.byref(b), sess.ctypes.data, len(sess), results.ctypes.data,
                                           starts.ctypes.data)
    assert rc == 0
    return b, res, results, starts


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["mixed", "shapes"])
def test_cpu_poisoned_buffers(name, layout):
    """nothing of a slot that is not in use is read: req_start holds ~0 there"""
    buf, off, sess = css.inputs(name)
    b, res, results, starts = poisoned_fixup_cpu(buf, off, sess, layout)
    assert (starts[~in_use(sess, results, b.n)] == 0xFFFFFFFFFFFFFFFF).all()
    got = rhp.classify_sessions_cpu(b, sess, results, starts, css.NAMES, css.ROUTES)
    same(got, css.expected(name), f"{name} poisoned layout {layout}")


def test_cpu_names_only_and_routes_only():
    buf, off, sess = css.inputs("mixed")
    wf, wr = css.expected("mixed")
    res, results, starts = rhp.fixup_cpu(buf, off, sess, MAXH)
    got = rhp.classify_sessions_cpu(res, sess, results, starts, css.NAMES, ())
    same(got, (wf, np.full(len(wr), rhp.ROUTE_NONE, dtype=np.uint16)), "names only")
    got = rhp.classify_sessions_cpu(res, sess, results, starts, (), css.ROUTES)
    same(got, (wf[:0], wr), "routes only")


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU)"""
    if which == "gpu-library":
        fn = lambda b, s, k, r, q, c: rhp.lib().rhp_classify_sessions(b, s, k, r, q, c, None)
    else:
        fn = lambda b, s, k, r, q, c: rhp.host().rhp_cpu_classify_sessions(b, s, k, r, q, c)
    buf, off, sess = css.inputs("shapes")
    n = len(off) - 1
    b0, res = rhp._host_batch(buf, off, MAXH, rhp.MODE_HTTP, rhp.LAYOUT_REQUEST_MAJOR, None, rhp.BATCH_SPECULATIVE)
    results = np.zeros(len(sess), dtype=rhp.SESSION_RESULT_DTYPE)
    starts = np.zeros(n, dtype=np.uint64)

    def call(names=(b"Host",), routes=((b"GET", b"/"),), patch_b=None, patch_c=None, n_sessions=len(sess),
             sessions=sess.ctypes.data, res_p=results.ctypes.data, starts_p=starts.ctypes.data):
        text, nm, rt = rhp.classify_tables(names, routes)
        fields = np.zeros((max(len(nm), 1), n), dtype=rhp.FIELDREF_DTYPE)
        route = np.zeros(n, dtype=np.uint16)
        c = rhp.Classify(text.ctypes.data, nm.ctypes.data if len(nm) else None, rt.ctypes.data if len(rt) else None,
                         len(nm), len(rt), fields.ctypes.data, route.ctypes.data)
        b = rhp.Batch.from_buffer_copy(b0)
        if patch_b:
            patch_b(b)
        if patch_c:
            patch_c(c)
        return fn(ctypes.byref(b), sessions, n_sessions, res_p, starts_p, ctypes.byref(c))

    E = -22
    zero = lambda b: setattr(b, "n", 0)
    assert fn(None, None, 0, None, None, None) == E
    assert call(patch_b=zero) == 0                                           # n == 0: nothing to do (and as a base line)
    assert call(patch_b=lambda b: setattr(b, "mode", rhp.MODE_PHR)) == E     # not http mode
    assert call(patch_b=lambda b: (zero(b), setattr(b, "mode", rhp.MODE_PHR))) == E
    assert call(patch_b=lambda b: setattr(b, "flags", 0)) == E               # not a speculative batch
    assert call(patch_b=lambda b: (zero(b), setattr(b, "flags", 0))) == E
    assert call(patch_b=lambda b: setattr(b, "flags", rhp.BATCH_SPECULATIVE | 2)) == E
    for layout in (rhp.LAYOUT_DENSE, rhp.LAYOUT_COMPACT, rhp.LAYOUT_DENSE_RM, 5):
        assert call(patch_b=lambda b: setattr(b, "layout", layout)) == E
        assert call(patch_b=lambda b: (zero(b), setattr(b, "layout", layout))) == E
    assert call(res_p=None) == E                                             # n_sessions > 0 without its arrays
    assert call(starts_p=None) == E
    assert call(sessions=None) == E
    assert call(patch_b=lambda b: setattr(b, "max_headers", rhp.RHP_MAX_HEADERS + 1)) == E
    assert call(patch_b=lambda b: setattr(b, "reqs", None)) == E
    assert call(patch_b=lambda b: setattr(b, "http", None)) == E
    # the table and output rules of rhp_classify_batch
    assert call(names=(b"",)) == E
    assert call(names=(b"x" * (rhp.CLASSIFY_NAME_MAX + 1),)) == E
    assert call(names=(b"x",) * (rhp.CLASSIFY_MAX_NAMES + 1)) == E
    assert call(routes=((b"GET", b"/"),) * (rhp.CLASSIFY_MAX_ROUTES + 1)) == E
    assert call(routes=((b"G" * 1024, b"/" * 1025),)) == E
    assert call(names=(), routes=()) == E
    assert call(patch_c=lambda c: setattr(c, "fields", None)) == E
    assert call(patch_c=lambda c: setattr(c, "route", None)) == E
    assert call(patch_c=lambda c: setattr(c, "names", None)) == E
    assert call(patch_c=lambda c: setattr(c, "text", None)) == E
    # limits that are met exactly are accepted; so are no sessions without their arrays, and bytes_rw == NULL
    assert call(names=(b"x" * rhp.CLASSIFY_NAME_MAX,) * rhp.CLASSIFY_MAX_NAMES,
                routes=((b"G" * 32, b"/" * 32),) * rhp.CLASSIFY_MAX_ROUTES, patch_b=zero) == 0
    assert call(patch_b=zero, n_sessions=0, sessions=None, res_p=None, starts_p=None) == 0
    assert call(patch_b=lambda b: (zero(b), setattr(b, "bytes_rw", None))) == 0


def test_host_twin_without_sessions_and_without_bytes_rw():
    """n_sessions == 0 with NULL arrays: every slot absent, the outputs fully
    written; bytes_rw == NULL: the bytes are read through `bytes`"""
    buf, off, sess = css.inputs("geom_none_65")
    b, res = rhp.speculative_cpu(buf, off, MAXH)
    text, nm, rt = rhp.classify_tables(css.NAMES, css.ROUTES)
    fields = np.full((len(nm), b.n), 0xA5A5, dtype=np.uint16).repeat(2, axis=1).view(rhp.FIELDREF_DTYPE)
    route = np.full(b.n, 0xA5A5, dtype=np.uint16)
    c = rhp.Classify(text.ctypes.data, nm.ctypes.data, rt.ctypes.data, len(nm), len(rt), fields.ctypes.data,
                     route.ctypes.data)
    assert rhp.host().rhp_cpu_classify_sessions(ctypes.byref(b), None, 0, None, None, ctypes.byref(c)) == 0
    same((fields, route), css.expected("geom_none_65"), "no sessions")
    buf, off, sess = css.inputs("geom_one_65")
    res, results, starts = rhp.fixup_cpu(buf, off, sess, MAXH)
    res.batch.bytes_rw = None
    same(rhp.classify_sessions_cpu(res, sess, results, starts, css.NAMES, css.ROUTES), css.expected("geom_one_65"),
         "bytes_rw NULL")


# ---------------------------------------------------------------------------
# GPU: one parse, one fix-up and one classify per case


def gpu_case(name, impl, layout, fill=None):
    """the kernel against the fixture, and against the host twin run over the
    records, session results and req_start the GPU left"""
    buf, off, sess = css.inputs(name)
    f, r, res, results, starts = rhp.classify_sessions_gpu(buf, off, sess, css.NAMES, css.ROUTES, MAXH, impl, layout,
                                                           fill=fill)
    label = f"{name} impl{impl} layout {layout} fill {fill}"
    same((f, r), css.expected(name), label + ": kernel against the reference")
    cpu = rhp.classify_sessions_cpu(res, sess, results, starts, css.NAMES, css.ROUTES)
    same((f, r), cpu, label + ": kernel against the host twin")
    return res, results, starts


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("impl", [rhp.IMPL_DFA, rhp.IMPL_EXACT])
def test_gpu_mixed(impl, layout):
    gpu_case("mixed", impl, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_shapes(layout):
    gpu_case("shapes", rhp.IMPL_DFA, layout)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["mixed", "shapes"])
def test_gpu_poisoned_buffers(name, layout):
    """record buffers, req_start and session results held 0xFF before the first
    launch: a slot the fix-up never wrote reads back as poison, and is absent"""
    buf, off, sess = css.inputs(name)
    res, results, starts = gpu_case(name, rhp.IMPL_DFA, layout, fill=0xFF)
    unused = ~in_use(sess, results, len(off) - 1)
    assert unused.any() and (starts[: len(unused)][unused] == 0xFFFFFFFFFFFFFFFF).all()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", css.GEOMETRY)
def test_gpu_geometry(name, layout):
    gpu_case(name, rhp.IMPL_DFA, layout, fill=0xFF)


@pytest.mark.gpu
@pytest.mark.parametrize("part", ["names-only", "routes-only"])
def test_gpu_names_only_and_routes_only(part):
    buf, off, sess = css.inputs("mixed")
    wf, wr = css.expected("mixed")
    names, routes = css.NAMES, css.ROUTES
    if part == "names-only":   # an empty route table, route == NULL
        routes, want = (), (wf, np.full(len(wr), rhp.ROUTE_NONE, dtype=np.uint16))
    else:
        names, want = (), (wf[:0], wr)
    f, r, *_ = rhp.classify_sessions_gpu(buf, off, sess, names, routes, MAXH)
    same((f, r), want, part)
