"""rhp_parse_messages (include/rhp.h): batched phr_parse_response and phr_parse_headers.

The expected answers are the compiled reference's own, recorded in tests/golden/messages.npz by
tests/golden/make_golden_messages.py (phr_parse_response / phr_parse_headers called in place on every message
of every set of tests/message_sets.py).  Held to them, value for value:
  CPU  the host twin rhp_cpu_parse_messages (the kernel's templates over plain memory), both layouts; the
       pointer-based rhp_phr_parse_response / rhp_phr_parse_headers; the live reference where
       oracle/_ref/libref.so is built; the refusals of rhp_msg_args.h; the header loop's second statement
       against the request parser's; a sanitizer build of the twins as a stand-alone program
  GPU  the kernel on every set in both layouts, records poisoned first and guard bytes on both sides of
       bytes, msgs and hdrs
A record is compared as rhp.h defines it: ret always; the other fields only for ret > 0; header records
only below num_headers.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import message_sets as ms

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "messages.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
LAYOUTS = [rhp.LAYOUT_REQUEST_MAJOR, rhp.LAYOUT_HEADER_MAJOR]
GUARD = 256


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


SET_NAMES = [str(x) for x in golden()["set_name"]]


@functools.lru_cache(maxsize=None)
def golden_set(name):
    """(kind, max_headers, buf u8, off u64 [n + 1], last_len u64 [n] | None, expected) of one set; expected:
    ret (RHP_RET_TOOLONG where the reference's exceeds RHP_MAX_LEN), status, msg_off, msg_len, minor,
    num_headers (int arrays [n]) and hdrs, a list of [num_headers, 4] u16 arrays"""
    g = golden()
    s = SET_NAMES.index(name)
    lo, hi = int(g["set_msg"][s]), int(g["set_msg"][s + 1])
    buf = g["bytes"][int(g["set_byte"][s]): int(g["set_byte"][s + 1])].copy()
    off = g["offsets"][lo + s: hi + s + 1].copy()
    ll = g["last_len"][lo:hi].copy() if g["set_has_ll"][s] else None
    exp = {k: g[k][lo:hi].astype(np.int64) for k in ("ret", "status", "msg_off", "msg_len", "minor", "num_headers")}
    exp["ret"] = np.where(exp["ret"] > rhp.RHP_MAX_LEN, rhp.RHP_RET_TOOLONG, exp["ret"])
    exp["hdrs"] = [g["hdr"][int(g["hdr_lo"][i]): int(g["hdr_lo"][i + 1])] for i in range(lo, hi)]
    for a in (buf, off) + tuple(exp[k] for k in exp if k != "hdrs"):
        a.setflags(write=False)
    return int(g["set_kind"][s]), int(g["set_maxh"][s]), buf, off, ll, exp


def check(name, msgs, hdrs, what):
    """the records of one set against the golden file"""
    kind, maxh, buf, off, ll, exp = golden_set(name)
    n = len(off) - 1
    assert len(msgs) == n and hdrs.shape == (n, maxh)
    ret = msgs["ret"].astype(np.int64)
    bad = np.flatnonzero(ret != exp["ret"])
    assert not len(bad), (f"{what} {name}: ret of message {int(bad[0])} is {int(ret[bad[0]])}, the reference's "
                          f"{int(exp['ret'][bad[0]])} ({len(bad)} differ): {bytes(buf[int(off[bad[0]]): int(off[bad[0] + 1])][:80])!r}")
    ok = ret > 0
    for f, e in (("status", "status"), ("msg_off", "msg_off"), ("msg_len", "msg_len"), ("minor_version", "minor"),
                 ("num_headers", "num_headers")):
        got = msgs[f].astype(np.int64)
        bad = np.flatnonzero(ok & (got != exp[e]))
        assert not len(bad), f"{what} {name}: {f} of message {int(bad[0])} is {int(got[bad[0]])}, the reference's {int(exp[e][bad[0]])}"
    assert (msgs["reserved"][ok] == 0).all() and (msgs["flags"][ok] == 0).all(), f"{what} {name}: reserved / flags are written 0"
    for i in np.flatnonzero(ok):
        got = hdrs[i, : int(exp["num_headers"][i])]
        got = np.stack([got[f] for f in ("name_off", "name_len", "value_off", "value_len")], axis=1) if len(got) else np.zeros((0, 4), np.uint16)
        assert (got == exp["hdrs"][i]).all(), f"{what} {name}: header records of message {int(i)}: {got.tolist()}, the reference's {exp['hdrs'][i].tolist()}"


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_sets():
    """the golden file's bytes, offsets, kinds, capacities and last_len are what tests/message_sets.py builds"""
    sets = ms.all_sets()
    assert [s[0] for s in sets] == SET_NAMES
    for name, kind, maxh, msgs, ll in sets:
        gk, gm, buf, off, gll, _ = golden_set(name)
        b, o = ms.pack(msgs)
        assert (gk, gm) == (kind, maxh) and (o == off).all() and (buf[: b.size] == b).all() and not buf[b.size:].any(), name
        assert (ll is None) == (gll is None) and (ll is None or list(gll) == ll), name


def test_golden_covers_what_the_sets_are_for():
    """the reference's answers that the sets exist to produce are in the file"""
    ret = lambda name: golden_set(name)[5]["ret"]
    for kn in ("response", "headers"):
        for eol in ("crlf", "lf"):
            r = ret(f"{kn}_prefixes_{eol}")
            assert (r[:-1] == -2).all() and r[-1] > 0, "every proper prefix is -2"
        r = ret(f"{kn}_long")
        assert r[7] == rhp.RHP_MAX_LEN and r[40] == rhp.RHP_RET_TOOLONG and (np.delete(r, [7, 40]) > 0).all()
        assert set(ret(f"{kn}_last_len").tolist()) >= {-1, -2} and (ret(f"{kn}_last_len") > 0).any()
        for n in (1, 63, 64, 65, 257):
            r = ret(f"{kn}_n{n}")
            assert len(r) == n and all(r[i] == -2 for i in range(3, n, 7)), "empty messages are -2"
        for maxh in (0, 1, 16):
            _, _, _, _, _, exp = golden_set(f"{kn}_headers_max{maxh}")
            assert exp["ret"][0] > 0 and exp["ret"][1] > 0 and exp["num_headers"][0] == maxh, "exactly max_headers lines fit"
            assert exp["ret"][2] == -1 and exp["ret"][3] == -1, "one more line is -1"
        e = golden_set(f"{kn}_headers_max16")[5]
        assert any((h[:, 0] == rhp.RHP_NAME_NULL).any() for h in e["hdrs"]), "an obs-fold record"
        assert (ret(f"{kn}_fuzz") > 0).sum() > 50 and (ret(f"{kn}_fuzz") == -1).sum() > 50 and (ret(f"{kn}_fuzz") == -2).sum() > 10
    sl = golden_set("status_lines")[5]
    assert sl["ret"][2] > 0 and sl["msg_len"][2] == 0 and sl["msg_off"][2] == 12, "no reason phrase: msg at the line end"
    assert sl["ret"][4] > 0 and sl["msg_len"][4] == 0 and sl["msg_off"][4] == 15, "a reason of spaces only"
    assert sl["ret"][23] == -1 and sl["ret"][24] == -1, "a leading empty line is not skipped"
    assert sl["status"][10] == 999 and sl["minor"][10] == 9


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_twin_equals_golden(name, layout):
    kind, maxh, buf, off, ll, _ = golden_set(name)
    check(name, *rhp.parse_messages_cpu(buf, off, kind, maxh, layout, ll), "rhp_cpu_parse_messages")


def pointer_records(kind, maxh, buf, off, ll, parse):
    """one pointer-based call per message -> (msgs, hdrs) as parse_messages_cpu, ret beyond RHP_MAX_LEN as RHP_RET_TOOLONG"""
    n = len(off) - 1
    msgs, hdrs = np.zeros(n, dtype=rhp.MSG_DTYPE), np.zeros((n, maxh), dtype=rhp.HDR_DTYPE)
    for i in range(n):
        ret, minor, status, (mo, ml), hs = parse(kind, buf, int(off[i]), int(off[i + 1] - off[i]), maxh,
                                                 0 if ll is None else int(ll[i]))
        if ret > rhp.RHP_MAX_LEN:
            msgs[i]["ret"] = rhp.RHP_RET_TOOLONG
            continue
        msgs[i] = (ret, status, mo, ml, minor, 0, len(hs), 0)
        for k, (no, nl, vo, vl) in enumerate(hs):
            hdrs[i, k] = (rhp.RHP_NAME_NULL if no < 0 else no, nl, vo, vl)
    return msgs, hdrs


@pytest.mark.parametrize("name", SET_NAMES)
def test_pointer_twins_equal_golden(name):
    kind, maxh, buf, off, ll, exp = golden_set(name)
    check(name, *pointer_records(kind, maxh, buf, off, ll, rhp.phr_parse_message_cpu), "rhp_phr_parse_response / _headers")


def test_pointer_twins_have_no_length_limit():
    """the message the batch answers with RHP_RET_TOOLONG: the pointer-based twins return its length"""
    for kn, kind in (("response", rhp.MSG_RESPONSE), ("headers", rhp.MSG_HEADERS)):
        _, maxh, buf, off, _, exp = golden_set(f"{kn}_long")
        assert exp["ret"][40] == rhp.RHP_RET_TOOLONG
        ret, _, _, _, hs = rhp.phr_parse_message_cpu(kind, buf, int(off[40]), int(off[41] - off[40]), maxh)
        assert ret == rhp.RHP_MAX_LEN + 1 and len(hs) == 2 and hs[1][3] > 65000


def reference_parse(ref):
    from golden.make_golden_messages import reference_message

    def parse(kind, buf, start, length, maxh, last_len):
        ret, status, mo, ml, minor, recs = reference_message(ref, kind, buf, start, length, maxh, last_len)
        return ret, minor, status, (mo, ml), [(-1 if no == rhp.RHP_NAME_NULL else no, nl, vo, vl) for no, nl, vo, vl in recs]
    return parse


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
@pytest.mark.parametrize("name", [n for n in SET_NAMES if "fuzz" in n])
def test_twins_equal_live_reference_on_fuzz(name):
    """the compiled reference, called now, against the file and against the host twin"""
    from golden.make_golden_messages import reference
    kind, maxh, buf, off, ll, _ = golden_set(name)
    live = pointer_records(kind, maxh, buf.copy(), off, ll, reference_parse(reference()))
    check(name, *live, "the live reference")
    twin = rhp.parse_messages_cpu(buf, off, kind, maxh, rhp.LAYOUT_REQUEST_MAJOR, ll)
    assert (twin[0]["ret"] == live[0]["ret"]).all()


@pytest.mark.parametrize("name", ["headers_fuzz", "headers_headers_max16", "headers_headers_max1", "headers_headers_max0",
                                  "headers_prefixes_crlf", "headers_prefixes_lf"])
def test_header_loop_statements_agree(name):
    """rhp_scalar.h states the header loop twice (scalar_phr_t's own, scalar_header_lines_t for the messages):
    a header block parsed as such, and as the header section of a request behind a 16-byte request line, gives
    the same status and the same records, shifted by the line"""
    line = b"GET / HTTP/1.1\r\n"
    kind, maxh, buf, off, _, _ = golden_set(name)
    msgs, hdrs = rhp.parse_messages_cpu(buf, off, kind, maxh)
    for i in range(len(off) - 1):
        m = bytes(buf[int(off[i]): int(off[i + 1])])
        req = np.frombuffer(line + m + bytes(rhp.RHP_PAD), dtype=np.uint8).copy()
        ret, _, _, _, hs = rhp.phr_parse_request_cpu(req, 0, len(line) + len(m), maxh)
        want = int(msgs["ret"][i])
        assert ret == (want + len(line) if want > 0 else want), (name, i, m)
        if ret > 0:
            got = [(int(h["name_off"]), int(h["name_len"]), int(h["value_off"]), int(h["value_len"])) for h in hdrs[i, : len(hs)]]
            assert len(hs) == int(msgs["num_headers"][i])
            assert got == [(rhp.RHP_NAME_NULL if no < 0 else no - len(line), nl, vo - len(line), vl) for no, nl, vo, vl in hs], (name, i, m)


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls and
    n == 0 go to the GPU library here: any other accepted one would launch a kernel over host memory"""
    gpu = which == "gpu-library"
    fn = (lambda b: rhp.lib().rhp_parse_messages(b, None)) if gpu else (lambda b: rhp.host().rhp_cpu_parse_messages(b))
    raw = np.zeros(512 + 16, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:][:512]
    buf[:19] = np.frombuffer(b"HTTP/1.1 200 OK\r\n\r\n", dtype=np.uint8)
    off = np.array([0, 19, 19], dtype=np.uint64)
    rawm = np.full(2 * 16 + 16, 0x77, dtype=np.uint8)
    msgs = rawm[(-rawm.ctypes.data) % 16:][:32]
    hdrs = np.full(2 * 4 * 8, 0x77, dtype=np.uint8)
    p = lambda a: a.ctypes.data

    def call(**kw):
        f = dict(bytes=p(buf), offsets=p(off), bytes_size=buf.size, n=2, max_headers=4, kind=rhp.MSG_RESPONSE,
                 layout=rhp.LAYOUT_REQUEST_MAJOR, msgs=p(msgs), hdrs=p(hdrs), last_len=None)
        f.update(kw)
        return fn(ctypes.byref(rhp.MsgBatch(*(f[k] for k, _ in rhp.MsgBatch._fields_))))

    E = -22
    assert fn(None) == E
    for f in ("bytes", "offsets", "msgs", "hdrs"):
        assert call(**{f: None}) == E, f
    assert call(kind=2) == E and call(kind=0xFFFFFFFF) == E
    for layout in (rhp.LAYOUT_COMPACT, rhp.LAYOUT_DENSE, rhp.LAYOUT_DENSE_RM, 5):
        assert call(layout=layout) == E
    assert call(max_headers=rhp.RHP_MAX_HEADERS + 1) == E
    assert call(n=2 ** 32 - 1, max_headers=2) == E and call(n=2 ** 26, max_headers=64) == E   # n * max_headers >= 2^32
    assert call(bytes_size=rhp.RHP_PAD - 1) == E and call(bytes_size=0) == E
    assert call(n=0, kind=7) == E and call(n=0, layout=9) == E   # the rules come before the empty batch
    if gpu:   # the device's alone: the reader's lines and the whole-record stores
        assert call(bytes=p(buf) + 8, bytes_size=buf.size - 8) == E and call(bytes=p(buf) + 1, bytes_size=buf.size - 1) == E
        assert call(msgs=p(msgs) + 8) == E and call(hdrs=p(hdrs) + 4) == E
    assert (msgs == 0x77).all() and (hdrs == 0x77).all(), "a refused call writes nothing"
    # accepted: an empty batch asks no pointer and launches nothing
    assert call(n=0) == 0 and call(n=0, bytes=None, offsets=None, msgs=None, hdrs=None, bytes_size=0) == 0
    assert (msgs == 0x77).all() and (hdrs == 0x77).all()
    if gpu:
        return
    # accepted by the host twin: any alignment; no hdrs with max_headers 0 (another line is then -1, none is fine)
    assert call(bytes=p(buf) + 1, offsets=p(np.array([0, 18, 18], dtype=np.uint64)), bytes_size=buf.size - 1) == 0
    assert msgs[:16].view(rhp.MSG_DTYPE)[0]["ret"] == -1
    assert call(max_headers=0, hdrs=None) == 0
    got = msgs.view(rhp.MSG_DTYPE)
    assert got["ret"].tolist() == [19, -2] and got["status"][0] == 200 and (got["msg_off"][0], got["msg_len"][0]) == (13, 2)
    assert (hdrs == 0x77).all()


def test_host_twins_asan_ubsan_clean():
    """`make messages-asan`: a stand-alone program over the host sources (tests/messages_host_test.c) that runs
    the batch twin and the pointer-based twins over the golden file's sets"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "messages-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "messages_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernel against the golden file


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_equals_golden(name, layout):
    """records poisoned first (an unwritten ret is no answer's value), guard bytes beside bytes, msgs and hdrs"""
    kind, maxh, buf, off, ll, _ = golden_set(name)
    check(name, *rhp.parse_messages_gpu(buf, off, kind, maxh, layout, ll, guard=GUARD), "rhp_parse_messages")


@pytest.mark.gpu
def test_gpu_device_call_takes_and_leaves_tensors():
    """parse_messages_device on the caller's stream and tensors, bytes 16 bytes into their allocation; n == 0
    launches nothing and leaves the records as they were"""
    import torch
    kind, maxh, buf, off, _, _ = golden_set("response_n65")
    n = len(off) - 1
    raw = torch.zeros(buf.size + 16, dtype=torch.uint8, device="cuda")
    raw[16:].copy_(torch.from_numpy(buf.copy()))
    doff = torch.from_numpy(off.view(np.int64).copy()).to("cuda")
    msgs = torch.full((16 * n,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
    hdrs = torch.full((8 * n * maxh,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    rhp.parse_messages_device(raw[16:], buf.size, doff, 0, kind, maxh, rhp.LAYOUT_HEADER_MAJOR, msgs, hdrs, stream=s)
    s.synchronize()
    assert bool((msgs == rhp.MSG_POISON).all()) and bool((hdrs == rhp.MSG_POISON).all())
    rhp.parse_messages_device(raw[16:], buf.size, doff, n, kind, maxh, rhp.LAYOUT_HEADER_MAJOR, msgs, hdrs, stream=s)
    s.synchronize()
    m = msgs.cpu().numpy().view(rhp.MSG_DTYPE)
    h = rhp.hdr_view(hdrs.cpu().numpy().view(rhp.HDR_DTYPE), n, maxh, rhp.LAYOUT_HEADER_MAJOR)
    check("response_n65", m, h, "parse_messages_device")
