"""rhp_relay_walked (include/rhp.h): the walked responses re-written for the client side -- http_write_response for
every slot of a walk that holds a whole response, from the records where the walk left them.

The expected answers are in tests/golden/walk_relay.npz, written by tests/golden/make_golden_walk_relay.py: rhp.h's
rule in plain Python over the walked records of every case of tests/walk_relay_sets.py (every set of
walk_responses.npz, every round of walk_resume.npz and walk_answers.npz, and sets of its own), without and with
RHP_WALK_DEFRAME, every reply byte the compiled reference's http_write_response.  Held to the file: why, the size and
the bytes of every slot.
  CPU  the host twin rhp_cpu_relay_walked behind the host walks on every case; the plain-Python rule and the twin on
       records built by hand, one why code each; the refusals of rhp_relay_args.h; a sanitizer build of the twin as a
       stand-alone program; the live reference where oracle/_ref/libref.so is built
  GPU  the kernels behind the walk kernels on one stream, out_off, why and out poisoned first and guard bytes on both
       sides of every buffer; an out one byte short; out at every residue mod 16; the hand-built records; the kernels
       against the twin on a seeded mix of 512 sessions over three resumed rounds; n_slots_total 1, 63, 64, 65, 257
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import walk_relay_sets as wy
import walk_resume_sets as wr
import walk_sets as ws
from golden.make_golden_walk_relay import expected, rule
from oracle_util import oracle_write_responses

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "walk_relay.npz")
EDGES_GOLDEN = os.path.join(HERE, "golden", "walk_edges.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
GUARD = 256
DEFRAMES = (0, ws.DEFRAME)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


CASE_NAMES = [str(x) for x in golden()["case_name"]]


def case(name):
    return next(c for c in wy.all_cases() if c["name"] == name)


def want_of(name, deframe):
    """(why u8, size u32, out u8) of one call of the file"""
    g = golden()
    c = CASE_NAMES.index(name)
    k = 2 * c + (1 if deframe and not g["same"][c] else 0)
    s0, s1, b0, b1 = int(g["call_slot"][k]), int(g["call_slot"][k + 1]), int(g["call_byte"][k]), int(g["call_byte"][k + 1])
    return g["why"][s0:s1], g["size"][s0:s1], g["out"][b0:b1]


def same_relay(got, want, what):
    """why, the size and the bytes of every slot; out None: the replies were not written"""
    off, why, out = got
    w_why, w_size, w_out = want
    assert len(why) == len(w_why) and len(off) == len(w_why) + 1, what
    bad = np.flatnonzero(why != w_why)
    assert not len(bad), f"{what}: why of slot {int(bad[0])} is {int(why[bad[0]])}, not {int(w_why[bad[0]])} ({len(bad)} differ)"
    w_off = np.concatenate([[0], np.cumsum(w_size.astype(np.uint64))]).astype(np.uint64)
    bad = np.flatnonzero(off != w_off)
    assert not len(bad), f"{what}: out_off[{int(bad[0])}] is {int(off[bad[0]])}, not {int(w_off[bad[0]])} ({len(bad)} differ)"
    if out is None:
        return
    assert len(out) == len(w_out), what
    bad = np.flatnonzero(out != w_out)
    if len(bad):
        i = int(np.searchsorted(w_off, bad[0], side="right")) - 1
        raise AssertionError(f"{what}: byte {int(bad[0])} (slot {i}) differs ({len(bad)} do): got "
                             f"{bytes(out[int(w_off[i]): int(w_off[i + 1])])[:200]!r}, want {bytes(w_out[int(w_off[i]): int(w_off[i + 1])])[:200]!r}")


def cpu_relay(c, deframe, **kw):
    out = wy.walk_cpu(rhp, c, deframe)
    return rhp.relay_walked_cpu(out, out[4], c["sess_off"], c["slot_off"], c["names"], c["maxh"], c["flags"] | deframe, **kw), out


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_cases_and_is_small():
    assert [c["name"] for c in wy.all_cases()] == CASE_NAMES
    assert os.path.getsize(GOLDEN) <= os.path.getsize(EDGES_GOLDEN)
    g = golden()
    for c in wy.all_cases():
        assert len(want_of(c["name"], 0)[0]) == int(c["slot_off"][-1]), c["name"]
    assert g["call_slot"][-1] == len(g["why"]) == len(g["size"]) and g["call_byte"][-1] == len(g["out"]) == int(g["size"].sum())
    assert ((g["why"] == 0) == (g["size"] > 0)).all()


def test_golden_covers():
    """each situation the sets exist for is in the file: a thinned fixture cannot pass silently"""
    g = golden()
    assert set(int(x) for x in g["why"]) >= {rhp.RELAY_OK, rhp.RELAY_UNUSED, rhp.RELAY_NOT_HEAD, rhp.RELAY_INTERIM, rhp.RELAY_PARTIAL,
                                             rhp.RELAY_FOLD, rhp.RELAY_FRAMING}
    text = lambda name, d: bytes(want_of(name, d)[2])
    names = text("names", ws.DEFRAME)
    assert names.count(b"Content-Type: text/plain\r\n") == 1 and b"text/second" not in names and names.count(b"Content-Type: \r\n") >= 3
    assert b"Content-Type: application/octet-stream\r\n" in names and b"X-First: 1\r\n" in names and b"X-Kept: yes\r\n" in names
    for gone in (b"onnection:", b"erver: upstream", b"timeout=5", b"Nov 1994", b"folded", b"ransfer-"):
        assert gone not in names, gone
    assert b"Content-Length: 12\r\n\r\nchunked body" in names and b"chunked body" not in text("names", 0)
    assert (want_of("names", 0)[0] == rhp.RELAY_FRAMING).sum() == 2 and (want_of("names", 0)[0] == rhp.RELAY_FOLD).sum() == 1
    assert text("full_kept", 0).count(b"\r\nH7: v7\r\n") == 1 and b"H0" not in text("full_dropped", 0) and b"H7" not in text("full_dropped", 0)
    status = text("status", 0)
    for line in (b"HTTP/1.1 200\r\n", b"HTTP/1.1 200 fine  \r\n", b"HTTP/1.1 099 Odd\r\n", b"HTTP/1.1 200 OK\r\n", b"HTTP/1.1 007\r\n",
                 b"HTTP/1.1 999 \tTab and more\r\n"):
        assert line in status, line
    assert list(want_of("status", 0)[0][:8]) == [0, 0, 0, rhp.RELAY_INTERIM, rhp.RELAY_INTERIM, 0, 0, 0]
    why = want_of("stops", 0)[0].reshape(-1)
    assert list(why[:2]) == [0, rhp.RELAY_PARTIAL] and list(why[4:6]) == [0, rhp.RELAY_PARTIAL] and list(why[8:10]) == [0, rhp.RELAY_NOT_HEAD]
    assert list(why[12:14]) == [0, rhp.RELAY_NOT_HEAD] and list(why[16:18]) == [0, 0] and list(why[18:22]) == [rhp.RELAY_NOT_HEAD, 0, 0, rhp.RELAY_UNUSED]
    assert why[22] == rhp.RELAY_NOT_HEAD
    head = text("head_reply", 0)
    assert head.count(b"Content-Type: t/x\r\nContent-Length: 0\r\n\r\nHTTP") == 2 and head.count(b"Content-Length: 5\r\n\r\nhello") == 2
    bodies = text("bodies", 0)
    for n in (0, 1, 9, 10, 99, 100, 999, 1000):
        assert b"Content-Type: b/%d\r\nContent-Length: %d\r\n\r\n" % (n, n) in bodies
    c = case("bodies")
    out = wy.walk_cpu(rhp, c, 0)
    assert {(int(s) + int(r)) % 16 for s, r in zip(out[1]["start"][9:26], out[2]["ret"][9:26])} == set(range(16))
    assert int(want_of("big_body", 0)[1].max()) > 20480 > wy.STAGE and (want_of("big_body", 0)[0] == 0).all()
    for total in (wy.STAGE - 16, wy.STAGE - 15, wy.STAGE):
        assert int(want_of(f"stage_{total}", 0)[1].sum()) == total


@pytest.mark.parametrize("name", CASE_NAMES)
def test_cpu_twin_equals_golden(name):
    for deframe in DEFRAMES:
        got, _ = cpu_relay(case(name), deframe)
        same_relay(got, want_of(name, deframe), f"rhp_cpu_relay_walked {name} deframe {deframe}")


def test_cpu_out_one_byte_short():
    c = case("names")
    want = want_of("names", ws.DEFRAME)
    (off, why, out), _ = cpu_relay(c, ws.DEFRAME, out_size=int(want[1].sum()) - 1)
    assert out is None
    same_relay((off, why, None), want, "one byte short")


def crafted():
    """Records built by hand, each against one test of rhp.h: [(label, kw of the call, records, flags, {slot: why})].
    The base is a walk of the twin's: three sessions of two heads in three slots; the slots not in use hold poison."""
    a = ws.resp([b"Content-Type: a/a", b"Connection: close", b"Content-Length: 3", b"X-Four: 4"], b"abc")   # max_headers records
    b = ws.resp([b"X-Next: 1", b"Content-Length: 0"])
    sessions = [a + b, b + a, a + a]
    buf, off = ws.pack(sessions)
    sl = ws.slot_offsets([3, 3, 3])
    maxh = 4
    base = tuple(x.copy() for x in rhp.walk_responses_cpu(buf, off, sl, maxh, ws.TRAILERS)[:4])
    ret = int(base[2]["ret"][0])
    kw = dict(buf=buf, sess_off=off, slot_off=sl, nt=9, bytes_size=buf.size, maxh=maxh)
    unused = {2: rhp.RELAY_UNUSED, 5: rhp.RELAY_UNUSED, 8: rhp.RELAY_UNUSED}
    cases = [("base", kw, base, ws.TRAILERS, {**unused, **{i: 0 for i in (0, 1, 3, 4, 6, 7)}})]

    def add(label, expect, flags=ws.TRAILERS, **change):
        r = tuple(x.copy() for x in base)
        k = dict(kw)
        for key, f in change.items():
            if key in k:
                k[key] = f(k[key].copy() if isinstance(k[key], np.ndarray) else k[key])
            else:
                f(dict(results=r[0], slots=r[1], msgs=r[2], hdrs=r[3])[key])
        cases.append((label, k, r, flags, {**unused, **expect}))

    def put(field, at, value):
        def f(x):
            x[field][at] = value
        return f

    both = lambda *fs: (lambda x: [f(x) for f in fs])
    add("not in use: slot_off[s+1] above n_slots_total", {6: rhp.RELAY_UNUSED, 7: rhp.RELAY_UNUSED}, slot_off=lambda x: (x.__setitem__(3, 10), x)[1])
    add("not a head", {0: rhp.RELAY_NOT_HEAD, 3: rhp.RELAY_NOT_HEAD, 6: rhp.RELAY_NOT_HEAD}, msgs=put("ret", 0, 0),
        slots=both(put("result", 3, 0), put("result", 6, -1)))
    add("head outside", {3: rhp.RELAY_OUTSIDE, 0: rhp.RELAY_OUTSIDE}, slots=both(put("start", 3, int(off[1]) - 1), put("start", 0, 2 ** 64 - 1)))
    add("head past bytes_size & ~3", {7: rhp.RELAY_OUTSIDE}, bytes_size=lambda _: int(base[1]["start"][7]) + int(base[2]["ret"][7]) - 1)
    add("interim", {0: rhp.RELAY_INTERIM, 1: rhp.RELAY_INTERIM, 3: 0, 4: 0}, msgs=both(put("status", 0, 100), put("status", 1, 199), put("status", 3, 99),
                                                                                        put("status", 4, 200)))
    add("a status above 999 prints its last three digits", {0: 0, 1: rhp.RELAY_INTERIM, 3: 0}, msgs=both(put("status", 0, 1200), put("status", 1, 100),
                                                                                                       put("status", 3, 65535)))
    add("last slot of a BODY and of a CLOSE round", {1: rhp.RELAY_PARTIAL, 4: rhp.RELAY_PARTIAL, 0: 0}, results=both(put("stop", 0, rhp.WALK_BODY),
                                                                                                                      put("stop", 1, rhp.WALK_CLOSE)))
    add("an obs-fold record", {0: rhp.RELAY_FOLD}, hdrs=lambda x: x.__setitem__((0, 1), (rhp.RHP_NAME_NULL, 0, 40, 2)))
    add("a name past ret", {0: rhp.RELAY_SPAN}, hdrs=lambda x: x.__setitem__((0, 0), (ret - 2, 12, 5, 1)))
    add("a value far past ret", {0: rhp.RELAY_SPAN}, hdrs=lambda x: x.__setitem__((0, 2), (20, 4, 0xFFF0, 0xFFFF)))
    add("a phrase past ret", {0: rhp.RELAY_SPAN}, msgs=put("msg_off", 0, ret - 1))
    add("a fold comes before a span", {0: rhp.RELAY_FOLD}, hdrs=lambda x: (x.__setitem__((0, 0), (ret - 2, 12, 5, 1)),
                                                                          x.__setitem__((0, 2), (rhp.RHP_NAME_NULL, 0, 40, 2))))
    add("a length body whose wire span is shorter", {0: rhp.RELAY_FRAMING}, slots=put("wire_len", 0, 2))
    add("a chunked body without the de-framing", {0: rhp.RELAY_FRAMING}, slots=put("body_kind", 0, rhp.FRAME_CHUNKED))
    add("a chunked body with it", {0: 0}, flags=ws.TRAILERS | ws.DEFRAME, slots=both(put("body_kind", 0, rhp.FRAME_CHUNKED), put("wire_len", 0, 20)))
    add("no framing, bytes on the wire", {0: rhp.RELAY_FRAMING}, slots=both(put("body_kind", 0, rhp.FRAME_NONE), put("body_len", 0, 0)))
    add("any kind with both lengths 0", {0: 0, 7: 0}, slots=both(put("body_len", 0, 0), put("wire_len", 0, 0), put("body_kind", 7, 9),
                                                                 put("body_len", 7, 0), put("wire_len", 7, 0)))
    add("body_len 2^32", {0: rhp.RELAY_LONG, 3: rhp.RELAY_LONG}, slots=both(put("body_len", 0, 2 ** 32), put("wire_len", 0, 2 ** 32),
                                                                           put("body_len", 3, 2 ** 64 - 1), put("wire_len", 3, 2 ** 64 - 1)))
    add("a body past its session", {0: rhp.RELAY_BODY_OUTSIDE, 7: rhp.RELAY_BODY_OUTSIDE},
        slots=both(put("body_len", 0, int(off[1]) - ret + 1), put("wire_len", 0, int(off[1]) - ret + 1), put("body_len", 7, 2 ** 32 - 1),
                   put("wire_len", 7, 2 ** 32 - 1)))
    add("a body past the readable end", {7: rhp.RELAY_BODY_OUTSIDE, 6: 0}, bytes_size=lambda _: int(off[3]) + 15)   # the readable end lies below the last body's end
    add("num_headers above max_headers", {0: 0, 7: 0}, msgs=both(put("num_headers", 0, 60), put("num_headers", 7, 0xFFFF)))
    return cases


CRAFTED = crafted()
CRAFTED_IDS = [c[0].replace(" ", "_").replace(":", "").replace("^", "") for c in CRAFTED]
CRAFTED_NAMES = (b"connection",)


def crafted_want(kw, records, flags, expect, label):
    """rhp.h's rule in plain Python, the bytes through the restatement's writer (built everywhere); the codes the
    case is for are the rule's"""
    why, size, out = expected(oracle_write_responses, records, kw["buf"], kw["bytes_size"], kw["sess_off"], kw["slot_off"], kw["nt"], kw["maxh"],
                              flags, CRAFTED_NAMES)
    for i, code in expect.items():
        assert why[i] == code, (label, i, int(why[i]), code)
    return why, size, out


@pytest.mark.parametrize("case_", CRAFTED, ids=CRAFTED_IDS)
def test_cpu_crafted_records(case_):
    label, kw, records, flags, expect = case_
    got = rhp.relay_walked_cpu(records, kw["buf"], kw["sess_off"], kw["slot_off"], CRAFTED_NAMES, kw["maxh"], flags,
                               bytes_size=kw["bytes_size"], n_slots_total=kw["nt"])
    same_relay(got, crafted_want(kw, records, flags, expect, label), f"rhp_cpu_relay_walked, {label}")


def test_rule_equals_file_through_the_restatement():
    """the plain-Python rule and the restatement's writer over the twin's records give the file: the file is what
    the maker's rule says, wherever the compiled reference is not built"""
    for name in ("names", "status", "stops", "head_reply", "walk_kinds_f1", "walk_heads"):
        c = case(name)
        for deframe in DEFRAMES:
            out = wy.walk_cpu(rhp, c, deframe)
            why, size, text = expected(oracle_write_responses, out[:4], out[4], out[4].size, c["sess_off"], c["slot_off"], int(c["slot_off"][-1]),
                                       c["maxh"], c["flags"] | deframe, c["names"])
            w_why, w_size, w_out = want_of(name, deframe)
            assert (why == w_why).all() and (size == w_size).all() and (text == w_out).all(), (name, deframe)


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
def test_golden_equals_live_reference():
    """the reference's http_write_response, run now over every relayed slot of every case, against the file"""
    from oracle_util import reference_write_responses
    relayed = 0
    for c in wy.all_cases():
        for deframe in DEFRAMES:
            out = wy.walk_cpu(rhp, c, deframe)
            why, size, text = expected(reference_write_responses, out[:4], out[4], out[4].size, c["sess_off"], c["slot_off"], int(c["slot_off"][-1]),
                                       c["maxh"], c["flags"] | deframe, c["names"])
            w_why, w_size, w_out = want_of(c["name"], deframe)
            assert (why == w_why).all() and (size == w_size).all() and (text == w_out).all(), (c["name"], deframe)
            relayed += int((why == 0).sum())
    assert relayed > 4000


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls go to
    the GPU library here"""
    gpu = which == "gpu-library"
    fn = ((lambda w, r: rhp.lib().rhp_relay_walked(w, r, None)) if gpu else (lambda w, r: rhp.host().rhp_cpu_relay_walked(w, r)))
    al = lambda nbytes, fill: (lambda r: r[(-r.ctypes.data) % 16:][:nbytes])(np.full(nbytes + 16, fill, dtype=np.uint8))
    buf = al(512, 0)
    buf[: len(ws.HELLO)] = np.frombuffer(ws.HELLO, dtype=np.uint8)
    so = np.array([0, len(ws.HELLO), len(ws.HELLO)], dtype=np.uint64)
    sl = np.array([0, 2, 4], dtype=np.uint64)
    msgs, hdrs, slots, results = al(64, 0x77), al(4 * 4 * 8, 0x77), al(128, 0x77), al(32, 0x77)
    out_off, why, out, work = al(8 * 5, 0x77), al(4 * 4, 0x77), al(64, 0x77), al(8 * rhp.relay_work_words(4), 0x77)
    results[:] = 0   # n_slots 0: no slot is in use
    text, nm, _ = rhp.classify_tables([b"Connection", b"x" * 64])
    p = lambda a: a.ctypes.data
    KEEP = object()

    def call(r=KEEP, rk=None, **kw):
        a = dict(bytes=p(buf), bytes_rw=p(buf), bytes_size=512, sess_off=p(so), slot_off=p(sl), n_sessions=2, n_slots_total=4,
                 max_headers=4, flags=0, msgs=p(msgs), hdrs=p(hdrs), slots=p(slots), results=p(results))
        a.update(kw)
        b = dict(text=p(text), names=p(nm), n_names=2, date_len=29, date=rhp.DEFAULT_DATE, out_off=p(out_off), why=p(why), out=p(out),
                 out_size=64, work=p(work))
        b.update(rk or {})
        relay = rhp.WalkRelay(*(b[k] for k, _ in rhp.WalkRelay._fields_))
        return fn(ctypes.byref(rhp.WalkBatch(*(a[k] for k, _ in rhp.WalkBatch._fields_))), ctypes.byref(relay) if r is KEEP else r)

    E = -22
    good = rhp.WalkRelay(p(text), p(nm), 2, 29, rhp.DEFAULT_DATE, p(out_off), p(why), p(out), 64, p(work))
    assert fn(None, ctypes.byref(good)) == E and call(r=None) == E
    for k in ("bytes", "sess_off", "slot_off", "results", "msgs", "slots", "hdrs"):
        assert call(**{k: None}) == E, k
    assert call(max_headers=rhp.RHP_MAX_HEADERS + 1) == E and call(n_slots_total=2 ** 32 - 1, max_headers=2) == E
    assert call(flags=8) == E and call(bytes_size=rhp.RHP_PAD - 1) == E
    assert call(flags=ws.DEFRAME, bytes_rw=None) == E and call(flags=ws.DEFRAME, bytes_rw=p(buf) + 16) == E
    for k in ("out_off", "why", "date", "work", "text", "names"):
        assert call(rk={k: None}) == E, k
    assert call(rk=dict(date_len=28)) == E and call(rk=dict(date_len=30)) == E and call(rk=dict(n_names=rhp.RELAY_MAX_NAMES + 1)) == E
    assert call(rk=dict(out=None)) == E, "a NULL out with a size"
    for bad in ([b""], [b"a", b""], [b"y" * 65]):
        t2, n2, _ = rhp.classify_tables(bad)
        assert call(rk=dict(text=p(t2), names=p(n2), n_names=len(bad))) == E, bad
    assert call(n_sessions=0, flags=8) == E and call(n_slots_total=0, rk=dict(date_len=0)) == E, "the rules come before the empty call"
    if gpu:   # the device's alone: whole-record loads, whole-word stores
        for k, a in (("bytes", buf), ("msgs", msgs), ("slots", slots), ("results", results)):
            assert call(**{k: p(a) + 8}) == E, k
        assert call(hdrs=p(hdrs) + 4) == E and call(rk=dict(out_off=p(out_off) + 4)) == E and call(rk=dict(why=p(why) + 2)) == E
        assert call(rk=dict(work=p(work) + 4)) == E
    if gpu:   # the measuring call: the same refusals, and no times for a call that launches no kernel
        us = (ctypes.c_float * 3)()
        w4 = rhp.WalkBatch(p(buf), p(buf), 512, p(so), p(sl), 2, 4, 4, 0, p(msgs), p(hdrs), p(slots), p(results))
        w0 = rhp.WalkBatch(p(buf), p(buf), 512, p(so), p(sl), 2, 0, 4, 0, None, None, None, p(results))
        steps = rhp.lib().rhp_relay_walked_steps
        assert steps(ctypes.byref(w4), ctypes.byref(good), None, None) == E and steps(None, ctypes.byref(good), None, ctypes.byref(us)) == E
        assert steps(ctypes.byref(w0), ctypes.byref(good), None, ctypes.byref(us)) == E
        assert rhp.lib().rhp_write_responses_steps(None, None, ctypes.byref(us)) == E
    for a in (out_off, why, out, work):
        assert (a == 0x77).all(), "a refused call writes nothing"
    if gpu:
        return
    # accepted by the host twin: no slot, or no session to own one: out_off[0] = 0 and nothing else
    for kw in (dict(n_slots_total=0, msgs=None, hdrs=None, slots=None), dict(n_sessions=0)):
        out_off[:] = 0x77
        assert call(**kw) == 0
        assert not out_off[:8].any() and (out_off[8:] == 0x77).all() and (why == 0x77).all() and (out == 0x77).all(), kw
    # any alignment, no names, an absent out: every slot not in use
    odd_off, odd_why = np.full(8 * 5 + 1, 0x77, dtype=np.uint8), np.full(4 * 4 + 1, 0x77, dtype=np.uint8)
    assert call(rk=dict(out_off=p(odd_off) + 1, why=p(odd_why) + 1, out=None, out_size=0, n_names=0, text=None, names=None), bytes_rw=None) == 0
    assert odd_off[0] == 0x77 and odd_why[0] == 0x77 and not odd_off[1:].any()
    assert (odd_why[1:].copy().view(np.uint32) == rhp.RELAY_UNUSED).all()


def test_host_twin_asan_ubsan_clean():
    """`make walk-relay-asan`: a stand-alone program over the host sources (tests/walk_relay_host_test.c)"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "walk-relay-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "walk_relay_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernels behind the walk kernels, against the golden file and against the twin


def gpu_relay(c, deframe, **kw):
    return rhp.relay_walked_gpu(c["buf"], c["sess_off"], c["slot_off"], c["names"], c["maxh"], c["flags"] | deframe, guard=GUARD,
                                states=c["states"], resume=c["kind"] == "resume" or (c["kind"] == "answers" and c["states"] is not None),
                                asked=c["asked"], **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gpu_equals_golden(name):
    """the walk and the relay on one stream, the records left on the device; out_off, why and out poisoned first,
    guard bytes beside every buffer, out at exactly out_off[n_slots_total] bytes"""
    for deframe in DEFRAMES:
        got, _ = gpu_relay(case(name), deframe)
        same_relay(got, want_of(name, deframe), f"rhp_relay_walked {name} deframe {deframe}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["names", "big_body", f"stage_{wy.STAGE}"])
def test_gpu_out_one_byte_short(name):
    """out is left untouched (the poison and the guard bytes hold), out_off and why are exact"""
    want = want_of(name, ws.DEFRAME)
    total = int(want[1].sum())
    (off, why, out), _ = gpu_relay(case(name), ws.DEFRAME, out_size=total - 1)   # (checks that out still holds the poison)
    assert out is None
    same_relay((off, why, None), want, f"{name}, one byte short")


@pytest.mark.gpu
@pytest.mark.parametrize("shift", range(16))
def test_gpu_out_at_every_residue(shift):
    for name in ("bodies", f"stage_{wy.STAGE - 15}"):
        got, _ = gpu_relay(case(name), ws.DEFRAME, out_shift=shift)
        same_relay(got, want_of(name, ws.DEFRAME), f"rhp_relay_walked {name}, out at {shift} mod 16")


@pytest.mark.gpu
@pytest.mark.parametrize("case_", CRAFTED, ids=CRAFTED_IDS)
def test_gpu_crafted_records(case_):
    """the hand-built records copied to the device, every slot not in use and what lies behind them 0xC3"""
    label, kw, records, flags, expect = case_
    got, _ = rhp.relay_walked_gpu(kw["buf"], kw["sess_off"], kw["slot_off"], CRAFTED_NAMES, kw["maxh"], flags, guard=GUARD, records=records,
                                  bytes_size=kw["bytes_size"], n_slots_total=kw["nt"])
    same_relay(got, crafted_want(kw, records, flags, expect, label), f"rhp_relay_walked, {label}")


@pytest.mark.gpu
def test_gpu_equals_twin_on_a_random_mix():
    """512 sessions over three resumed rounds, a quarter of the bodies chunked, de-framed"""
    deliveries, caps = wy.random_mix(512, 20261021)
    flags = ws.TRAILERS | ws.DEFRAME
    want, got = [], []

    def cpu_round(buf, off, sl, st, maxh, fl):
        out = rhp.walk_resume_cpu(buf, off, sl, st, maxh, fl)
        want.append(rhp.relay_walked_cpu(out, out[4], off, sl, wy.DROP, maxh, fl))
        return out

    def gpu_round(buf, off, sl, st, maxh, fl):
        r, out = rhp.relay_walked_gpu(buf, off, sl, wy.DROP, maxh, fl, guard=GUARD, states=st, resume=True)
        got.append(r)
        return out

    wr.walk_rounds(cpu_round, deliveries, caps, 8, flags)
    wr.walk_rounds(gpu_round, deliveries, caps, 8, flags)
    assert len(want) == len(got) == 3
    relayed = 0
    for r, (w, g) in enumerate(zip(want, got)):
        same_relay(g, (w[1], np.diff(w[0]).astype(np.uint32), w[2]), f"the kernels against the host twin, round {r}")
        relayed += int((w[1] == 0).sum())
    assert relayed > 500 and sum(bytes(w[2]).count(b"chunked") for w in want) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 63, 64, 65, 257])
def test_gpu_slot_counts(nt):
    """n_slots_total at the wave's and the block's edges: nt sessions of one slot each, every one a reply"""
    sessions = [ws.length(b"n%03d" % k * (k % 5), [b"Content-Type: n/%d" % k, b"Connection: close"]) for k in range(nt)]
    buf, off = ws.pack(sessions)
    sl = ws.slot_offsets([1] * nt)
    out = rhp.walk_responses_cpu(buf, off, sl, 4, ws.TRAILERS)
    want = rhp.relay_walked_cpu(out, out[4], off, sl, wy.DROP, 4, ws.TRAILERS)
    assert (want[1] == 0).all()
    got, _ = rhp.relay_walked_gpu(buf, off, sl, wy.DROP, 4, ws.TRAILERS, guard=GUARD)
    same_relay(got, (want[1], np.diff(want[0]).astype(np.uint32), want[2]), f"the kernels against the host twin, {nt} slots")


@pytest.mark.gpu
def test_gpu_measuring_call_leaves_the_same():
    """rhp_relay_walked_steps: the same kernels with an event between them -- the file's answers"""
    for name in ("names", "big_body"):
        got, _ = gpu_relay(case(name), ws.DEFRAME, steps=True)
        same_relay(got, want_of(name, ws.DEFRAME), f"rhp_relay_walked_steps {name}")
