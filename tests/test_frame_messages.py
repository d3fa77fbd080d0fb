"""rhp_frame_messages (include/rhp.h): the body framing of http.c:204-233 over the records rhp_parse_messages
leaves, the header lookup of rhp_classify_batch over the same records, and the decoders rhp_decode_chunked
starts from.

The expected answers are the compiled reference's own, recorded in tests/golden/frame_messages.npz by
tests/golden/make_golden_frame_messages.py in two ways that must agree (http_field_lookup, data_equal_case and
strtoull composed in the order of http.c; http_read_request itself on a twin request), for every message of every
set of tests/frame_sets.py.  Held to them, value for value:
  CPU  the host twin rhp_cpu_frame_messages, both layouts; the live reference where oracle/_ref/libref.so is
       built; the refusals of rhp_frame_args.h; records that are never to be read, poisoned; a sanitizer build
       of the twin as a stand-alone program
  GPU  the kernel on every set in both layouts, outputs poisoned first and guard bytes on both sides of bytes,
       frames, fields and decoders; the decoders it arms and those it leaves; the chain parse -> frame ->
       decode with the decoders armed on the device
Compared: result, body_kind and body_len always, the fields of every name always.
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import frame_sets as fs

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "frame_messages.npz")
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
    """(kind, max_headers, buf u8, off u64 [n + 1], names [bytes], expected) of one set; expected: ret (the
    reference's parse result), result, body_kind, body_len (arrays [n]) and fields FIELDREF_DTYPE [n_names, n]"""
    g = golden()
    s = SET_NAMES.index(name)
    lo, hi = int(g["set_msg"][s]), int(g["set_msg"][s + 1])
    buf = g["bytes"][int(g["set_byte"][s]): int(g["set_byte"][s + 1])].copy()
    off = g["offsets"][lo + s: hi + s + 1].copy()
    text = g["name_text"].tobytes()
    names = [text[int(o): int(o + l)] for o, l in g["name_span"][int(g["set_names"][s]): int(g["set_names"][s + 1])]]
    exp = {k: g[k][lo:hi].copy() for k in ("ret", "result", "body_kind", "body_len")}
    f = g["field"][int(g["set_field"][s]): int(g["set_field"][s + 1])]
    exp["fields"] = np.ascontiguousarray(f).view(rhp.FIELDREF_DTYPE).reshape(len(names), hi - lo)
    for a in (buf, off) + tuple(exp.values()):
        a.setflags(write=False)
    return int(g["set_kind"][s]), int(g["set_maxh"][s]), buf, off, names, exp


def check(name, frames, fields, what):
    """the frames and fields of one set against the golden file"""
    _, _, buf, off, names, exp = golden_set(name)
    n = len(off) - 1
    assert len(frames) == n and fields.shape == (len(names), n)
    for f in ("result", "body_kind", "body_len"):
        bad = np.flatnonzero(frames[f] != exp[f])
        assert not len(bad), (f"{what} {name}: {f} of message {int(bad[0])} is {int(frames[f][bad[0]])}, the reference's "
                              f"{int(exp[f][bad[0]])} ({len(bad)} differ): {bytes(buf[int(off[bad[0]]): int(off[bad[0] + 1])][:120])!r}")
    bad = np.argwhere(fields != exp["fields"])
    assert not len(bad), (f"{what} {name}: field {names[int(bad[0][0])]!r} of message {int(bad[0][1])} is "
                          f"{fields[tuple(bad[0])]}, the reference's {exp['fields'][tuple(bad[0])]}")


def check_decoders(name, dec, consume_trailer, what):
    """armed where the golden kind is CHUNKED: zero but consume_trailer; every other decoder keeps its poison"""
    exp = golden_set(name)[5]
    raw = np.ascontiguousarray(dec).view(np.uint8).reshape(-1, 16)
    chunked = exp["body_kind"] == rhp.FRAME_CHUNKED
    armed = np.zeros(16, dtype=np.uint8)
    armed[8] = consume_trailer
    assert (raw[chunked] == armed).all(), f"{what} {name}: an armed decoder is 16 zero bytes apart from consume_trailer"
    assert (raw[~chunked] == rhp.FRAME_POISON).all(), f"{what} {name}: a decoder of a message that is not chunked was written"


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_sets():
    """the golden file's bytes, offsets, kinds, capacities and names are what tests/frame_sets.py builds"""
    sets = fs.all_sets()
    assert [s[0] for s in sets] == SET_NAMES
    for name, kind, maxh, msgs, names in sets:
        gk, gm, buf, off, gnames, _ = golden_set(name)
        b, o = fs.pack(msgs)
        assert (gk, gm, gnames) == (kind, maxh, names) and (o == off).all() and (buf[: b.size] == b).all() and not buf[b.size:].any(), name


def test_golden_covers_what_the_sets_are_for():
    """the reference's answers that the sets exist to produce are in the file"""
    M = 2 ** 64 - 1
    for kind, kn in ((fs.RESPONSE, "response"), (fs.HEADERS, "headers")):
        e = lambda name: golden_set(f"{kn}_{name}")[5]
        row = lambda name, i: (int(e(name)["result"][i]), int(e(name)["body_kind"][i]), int(e(name)["body_len"][i]))
        for n in fs.BATCH_SIZES:
            x = e(f"n{n}")
            assert len(x["ret"]) == n
            if n >= 63:
                assert set(x["body_kind"].tolist()) == {0, 1, 2} and set(x["result"].tolist()) == {1, 0, -1}
                assert ((x["ret"] > 0) & (x["result"] == -1)).any() and (x["ret"] == -1).any() and (x["ret"] == -2).any()
        for maxh in fs.CAPACITIES:
            x = e(f"max{maxh}")
            assert x["ret"][0] > 0 and (x["ret"][-1] == -1 or maxh == 0), "exactly max_headers lines fit, one more is -1"
            if maxh:
                assert row(f"max{maxh}", 1) == (1, rhp.FRAME_LENGTH, 42) and row(f"max{maxh}", 2) == (1, rhp.FRAME_CHUNKED, 0)
                assert e(f"max{maxh}")["fields"][1, 3]["value_len"] == 5, "Connection as the last record"
        # placement: record 0 and the last, five spellings, four alignments; the duplicate rules; obs-fold
        pl = fs._placement(kind)
        assert len(pl) == 2 * fs.PLACEMENT_PER_NAME
        for i in range(len(pl)):
            framed = (1, rhp.FRAME_LENGTH, 17) if i < fs.PLACEMENT_PER_NAME else (1, rhp.FRAME_CHUNKED, 0)
            absent = i % fs.PLACEMENT_PER_NAME in fs.PLACEMENT_ABSENT   # first empty then set (x2), the name in a folded line
            assert row("placement", i) == ((1, 0, 0) if absent else framed), (i, pl[i])
        # near misses: none of them is a framing header; the 0x20 pairs stay apart
        near, x = fs._near(kind), e("near")
        tail = len(near) - len(fs.NEAR_PAIRS)   # A~B A^B A`B A_B a~b A|B
        assert all(row("near", i) == (1, 0, 0) for i in range(tail)), "a near miss is no framing header"
        names, f = fs.NEAR_NAMES, x["fields"]
        present = lambda nm, i: f[names.index(nm), i]["value_off"] != rhp.RHP_NAME_NULL
        assert present(b"A~B", tail) and not present(b"A^B", tail) and present(b"A^B", tail + 1) and not present(b"A~B", tail + 1)
        assert present(b"A`B", tail + 2) and not present(b"A@B", tail + 2) and present(b"A_B", tail + 3) and not present(b"A\x7fB", tail + 3)
        assert present(b"A~B", tail + 4) and present(b"a|b", tail + 5) and not present(b"A\x5cB", tail + 5)
        assert present(b"Content-Length", tail) and not present(b"Content-Lengtx", tail) and not present(b"transfer-encoding", tail)
        assert (x["ret"] > 0).all()
        # the values
        v = dict(zip(fs.CL_VALUES, range(len(fs.CL_VALUES))))
        want = {b"0": 0, b"1": 1, b"18446744073709551615": M, b"18446744073709551616": M, b"-1": M, b"+5": 5, b"12abc": 12,
                b"abc": 0, b"0" * 40 + b"7": 7, b"0" * 23 + b"9": 9, b"0" * 24 + b"9": 9, b"99999999999999999999999999": M,
                b"-18446744073709551615": 1, b"-": 0, b"4294967296": 2 ** 32, b"5 6": 5}
        for val, num in want.items():
            assert row("values", v[val]) == (1, rhp.FRAME_LENGTH, num), val
        t0 = len(fs.CL_VALUES) + 9 + 8 + 4
        tv = dict(zip(fs.TE_VALUES, range(t0, t0 + len(fs.TE_VALUES))))
        for val in (b"chunked", b"Chunked", b"CHUNKED", b"cHuNkEd", b"chunkeD"):
            assert row("values", tv[val]) == (1, rhp.FRAME_CHUNKED, 0), val
        for val in (b"chunke", b"chunkedx", b"gzip, chunked", b"identity", b"xhunked", b"chunke\xc4"):
            assert row("values", tv[val]) == (-1, 0, 0), val
        last = len(fs._values(kind))
        combos = [row("values", i) for i in range(last - 10, last)]
        assert combos == [(-1, 0, 0)] * 4 + [(1, 1, 5)] * 2 + [(1, 2, 0)] * 2 + [(-1, 0, 0), (1, 0, 0)], combos
        # not ready
        x = e("not_ready")
        assert x["ret"][1] == -1 and x["result"][1] == -1 and x["ret"][2] == -2 and x["result"][2] == 0 and x["ret"][3] == -2
        assert (x["body_kind"][x["result"] != 1] == 0).all() and (x["fields"]["value_off"][:, x["ret"] <= 0] == rhp.RHP_NAME_NULL).all()
        fz = e("fuzz")
        assert ((fz["body_kind"] == 1).sum() > 50 and (fz["body_kind"] == 2).sum() > 20 and ((fz["ret"] > 0) & (fz["result"] == -1)).sum() > 20
                and (fz["result"] == 0).sum() > 50 and (fz["fields"]["value_off"] != rhp.RHP_NAME_NULL).sum() > 20)
    x = golden_set("response_not_ready")[5]
    assert x["ret"][4] == rhp.RHP_MAX_LEN + 1 and x["result"][4] == rhp.RHP_RET_TOOLONG, "one message past RHP_MAX_LEN"
    assert x["ret"][5] == rhp.RHP_MAX_LEN and (x["result"][5], x["body_kind"][5], x["body_len"][5]) == (1, 1, M), \
        "the value's last byte is the last before the line end of the last line, at the records' reach"


def frame_cpu(name, layout, **kw):
    kind, maxh, buf, off, names, _ = golden_set(name)
    msgs, hdrs = rhp.parse_messages_cpu(buf, off, kind, maxh, layout)
    return rhp.frame_messages_cpu(buf, off, kind, msgs, hdrs, names, maxh, layout, **kw)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_twin_equals_golden(name, layout):
    frames, fields, dec = frame_cpu(name, layout, consume_trailer=1)
    check(name, frames, fields, "rhp_cpu_frame_messages")
    check_decoders(name, dec, 1, "rhp_cpu_frame_messages")


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
@pytest.mark.parametrize("name", [n for n in SET_NAMES if "fuzz" in n or "values" in n])
def test_twin_equals_live_reference(name):
    """the compiled reference, called now (the maker's composition), against the file and against the host twin"""
    from golden.make_golden_frame_messages import composer
    from golden.make_golden_messages import reference
    kind, maxh, buf, off, names, exp = golden_set(name)
    compose = composer(reference())
    live = buf.copy()
    rows = [compose(kind, live, int(off[i]), int(off[i + 1] - off[i]), maxh, names) for i in range(len(off) - 1)]
    frames, fields, _ = frame_cpu(name, rhp.LAYOUT_REQUEST_MAJOR)
    for i, (ret, result, fkind, blen, fl) in enumerate(rows):
        assert (ret, result, fkind, blen) == (int(exp["ret"][i]), int(exp["result"][i]), int(exp["body_kind"][i]), int(exp["body_len"][i])), (name, i)
        assert (int(frames["result"][i]), int(frames["body_kind"][i]), int(frames["body_len"][i])) == (result, fkind, blen), (name, i)
        assert [tuple(int(v) for v in fields[j, i]) for j in range(len(names))] == [tuple(x) for x in fl], (name, i)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", ["response_n257", "headers_fuzz", "response_max64", "headers_max0"])
def test_cpu_records_never_read_may_hold_anything(name, layout):
    """0xFF in every byte but ret of the records of messages that are not ready, and in the header records at
    k >= num_headers: the answers do not change"""
    kind, maxh, buf, off, names, _ = golden_set(name)
    msgs, hdrs = (a.copy() for a in rhp.parse_messages_cpu(buf, off, kind, maxh, layout))
    poison_unread(msgs, hdrs)
    frames, fields, dec = rhp.frame_messages_cpu(buf, off, kind, msgs, hdrs, names, maxh, layout)
    check(name, frames, fields, "rhp_cpu_frame_messages over poisoned records")
    check_decoders(name, dec, 0, "rhp_cpu_frame_messages over poisoned records")


def poison_unread(msgs, hdrs):
    """what rhp.h leaves unspecified, as 0xFF: all of a record with ret <= 0 but ret, header records k >= num_headers"""
    ok = msgs["ret"] > 0
    raw = msgs.view(np.uint8).reshape(-1, 16)
    raw[~ok, 4:] = 0xFF
    nh = np.where(ok, msgs["num_headers"], 0)
    hdrs.view(np.uint8).reshape(hdrs.shape + (8,))[np.arange(hdrs.shape[1])[None, :] >= nh[:, None]] = 0xFF


def crafted():
    """records no parse leaves: rets and offsets that reach past the message, past the batch's bytes and past
    bytes_size.  (buf, off, bytes_size, msgs, hdrs [n, 4], expected rows (result, kind, len), expected fields
    for NAMES)"""
    m = fs.msg(fs.RESPONSE, [b"Content-Length: 25", b"Connection: close"])
    msgs_b = [m, m, m, m, m, m]
    buf, off = fs.pack(msgs_b)
    size = int(off[5]) + 40   # the last message ends past bytes_size; the fifth ends inside it
    good_m, good_h = rhp.parse_messages_cpu(buf, off, fs.RESPONSE, 4)
    msgs, hdrs = good_m.copy(), good_h.copy()
    ret = int(good_m["ret"][0])
    co_v = (int(good_h[0, 1]["value_off"]), 5)
    A = (rhp.RHP_NAME_NULL, 0)
    rows, fields = [(1, 1, 25)], [(A, co_v)]                                  # 0: as parsed (Content-Type absent, Connection present)
    msgs["ret"][1] = 0x7FFFFFFF                             # 1: ret past bytes_size
    rows.append((0, 0, 0)); fields.append((A, A))
    hdrs[2, 0]["value_len"] = 0xFFFF                        # 2: Content-Length's value runs past ret: the record matches nothing
    hdrs[2, 1]["name_off"] = 0xFF00                         #    Connection's name lies past ret
    rows.append((1, 0, 0)); fields.append((A, A))
    hdrs[3, 1]["value_off"], hdrs[3, 1]["value_len"] = 0xFFF0, 0xFFFF   # 3: a caller's value is not read: reported as it stands
    rows.append((1, 1, 25)); fields.append((A, (0xFFF0, 0xFFFF)))
    msgs["num_headers"][4] = 0xFFFF                         # 4: num_headers above max_headers: records k < max_headers (2 parsed, 2 empty names)
    hdrs[4, 2:] = (0, 0, 0, 0)
    rows.append((1, 1, 25)); fields.append((A, co_v))
    rows.append((0, 0, 0)); fields.append((A, A))           # 5: offsets[i] + ret > bytes_size
    assert int(off[4]) + ret <= size < int(off[5]) + ret
    return buf, off, size, msgs, hdrs, rows, fields


def check_crafted(frames, fields, what):
    _, _, _, _, _, rows, want = crafted()
    got = [(int(f["result"]), int(f["body_kind"]), int(f["body_len"])) for f in frames]
    assert got == rows, (what, got)
    assert [tuple(tuple(int(v) for v in fields[j, i]) for j in range(2)) for i in range(len(rows))] == want, what


@pytest.mark.parametrize("layout", LAYOUTS)
def test_cpu_crafted_records_stay_inside_the_message(layout):
    buf, off, size, msgs, hdrs, _, _ = crafted()
    frames, fields, _ = rhp.frame_messages_cpu(buf[:size].copy(), off, fs.RESPONSE, msgs, hdrs, fs.NAMES, 4, layout, bytes_size=size)
    check_crafted(frames, fields, "rhp_cpu_frame_messages")


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls and
    n == 0 go to the GPU library here: any other accepted one would launch a kernel over host memory"""
    gpu = which == "gpu-library"
    fn = ((lambda b, f: rhp.lib().rhp_frame_messages(b, f, None)) if gpu else
          (lambda b, f: rhp.host().rhp_cpu_frame_messages(b, f)))
    raw = np.zeros(512 + 16, dtype=np.uint8)
    buf = raw[(-raw.ctypes.data) % 16:][:512]
    buf[:38] = np.frombuffer(b"HTTP/1.1 200 OK\r\nContent-Length: 7\r\n\r\n", dtype=np.uint8)
    off = np.array([0, 38, 38], dtype=np.uint64)
    al = lambda nbytes, fill: (lambda r: r[(-r.ctypes.data) % 16:][:nbytes])(np.full(nbytes + 16, fill, dtype=np.uint8))
    msgs, frames, dec = al(32, 0), al(32, 0x77), al(32, 0x77)
    hdrs, fields = np.zeros(2 * 4 * 8, dtype=np.uint8), np.full(2 * 2 * 4, 0x77, dtype=np.uint8)
    mb = rhp.MsgBatch(buf.ctypes.data, off.ctypes.data, 512, 2, 4, rhp.MSG_RESPONSE, rhp.LAYOUT_REQUEST_MAJOR,
                      msgs.ctypes.data, hdrs.ctypes.data, None)
    assert rhp.host().rhp_cpu_parse_messages(ctypes.byref(mb)) == 0
    text, nm, _ = rhp.classify_tables(fs.NAMES)
    p = lambda a: a.ctypes.data

    def call(batch=None, **kw):
        b = dict(bytes=p(buf), offsets=p(off), bytes_size=512, n=2, max_headers=4, kind=rhp.MSG_RESPONSE,
                 layout=rhp.LAYOUT_REQUEST_MAJOR, msgs=p(msgs), hdrs=p(hdrs), last_len=None)
        b.update(batch or {})
        f = dict(text=p(text), names=p(nm), n_names=2, consume_trailer=0, fields=p(fields), frames=p(frames), decoders=p(dec),
                 reserved=0)
        f.update(kw)
        return fn(ctypes.byref(rhp.MsgBatch(*(b[k] for k, _ in rhp.MsgBatch._fields_))),
                  ctypes.byref(rhp.FrameArgs(*(f[k] for k, _ in rhp.FrameArgs._fields_))))

    E = -22
    ok_f = rhp.FrameArgs(p(text), p(nm), 2, 0, p(fields), p(frames), p(dec), 0)
    assert fn(None, ctypes.byref(ok_f)) == E and fn(ctypes.byref(mb), None) == E
    for k in ("bytes", "offsets", "msgs", "hdrs"):   # what rhp_msg_args.h refuses
        assert call({k: None}) == E, k
    assert call({"kind": 2}) == E and call({"layout": rhp.LAYOUT_COMPACT}) == E and call({"layout": rhp.LAYOUT_DENSE}) == E
    assert call({"max_headers": rhp.RHP_MAX_HEADERS + 1}) == E and call({"n": 2 ** 32 - 1, "max_headers": 2}) == E
    assert call({"bytes_size": rhp.RHP_PAD - 1}) == E
    assert call({"n": 0, "kind": 7}) == E, "the rules come before the empty batch"
    assert call(n_names=rhp.CLASSIFY_MAX_NAMES + 1) == E
    for k in ("text", "names", "fields"):
        assert call(**{k: None}) == E, k
    for bad in (0, rhp.CLASSIFY_NAME_MAX + 1):
        spans = nm.copy()
        spans[1, 1] = bad
        assert call(names=p(spans)) == E, f"a name of {bad} bytes"
    assert call(frames=None) == E and call(consume_trailer=2) == E and call(reserved=1) == E and call(reserved=1 << 40) == E
    assert call({"n": 0}, consume_trailer=2) == E and call({"n": 0}, reserved=1) == E
    if gpu:   # the device's alone: the whole-record loads and stores
        assert call(frames=p(frames) + 8) == E and call(decoders=p(dec) + 8) == E and call(frames=p(frames) + 4) == E
        assert call({"msgs": p(msgs) + 8}) == E and call({"bytes": p(buf) + 8, "bytes_size": 504}) == E and call({"hdrs": p(hdrs) + 4}) == E
    assert (frames == 0x77).all() and (fields == 0x77).all() and (dec == 0x77).all(), "a refused call writes nothing"
    # accepted: an empty batch asks no pointer and launches nothing; last_len is not looked at
    assert call({"n": 0}) == 0 and call({"n": 0, "bytes": None, "offsets": None, "msgs": None, "hdrs": None, "bytes_size": 0},
                                        frames=None, fields=None, decoders=None, n_names=0, text=None, names=None) == 0
    assert call({"n": 0, "last_len": 1}) == 0
    assert (frames == 0x77).all() and (fields == 0x77).all() and (dec == 0x77).all()
    if gpu:
        return
    # accepted by the host twin: any alignment, no decoders, no names
    odd = np.full(33, 0x77, dtype=np.uint8)
    assert call(frames=p(odd) + 1, decoders=None) == 0 and odd[0] == 0x77
    got = odd[1:].copy().view(rhp.FRAME_DTYPE)
    assert got.tolist() == [(1, rhp.FRAME_LENGTH, 7), (0, 0, 0)] and (dec == 0x77).all()
    assert fields.view(rhp.FIELDREF_DTYPE).tolist() == [(rhp.RHP_NAME_NULL, 0)] * 4
    fields[:] = 0x77
    assert call(n_names=0, text=None, names=None, fields=None, frames=p(frames[:32])) == 0 and (fields == 0x77).all()


def test_host_twin_asan_ubsan_clean():
    """`make frame-messages-asan`: a stand-alone program over the host sources (tests/frame_messages_host_test.c)
    that parses and frames the golden file's sets with the host twins"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "frame-messages-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "frame_messages_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernel against the golden file


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_equals_golden(name, layout):
    """parsed and framed on the device; outputs poisoned first, guard bytes beside bytes, frames, fields and
    decoders; the decoders of messages that are not chunked keep their poison"""
    kind, maxh, buf, off, names, _ = golden_set(name)
    ct = SET_NAMES.index(name) & 1   # both values of consume_trailer over the sets
    frames, fields, dec = rhp.frame_messages_gpu(buf, off, kind, names, maxh, layout, consume_trailer=ct, guard=GUARD)
    check(name, frames, fields, "rhp_frame_messages")
    check_decoders(name, dec, ct, "rhp_frame_messages")


@pytest.mark.gpu
@pytest.mark.parametrize("consume_trailer", [0, 1])
def test_gpu_decoders_armed_or_left(consume_trailer):
    name = "response_n257"
    kind, maxh, buf, off, names, exp = golden_set(name)
    frames, fields, dec = rhp.frame_messages_gpu(buf, off, kind, names, maxh, rhp.LAYOUT_HEADER_MAJOR,
                                                 consume_trailer=consume_trailer, guard=GUARD)
    check(name, frames, fields, "rhp_frame_messages")
    check_decoders(name, dec, consume_trailer, "rhp_frame_messages")
    assert (exp["body_kind"] == rhp.FRAME_CHUNKED).sum() >= 50


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_without_decoders_and_without_names(layout):
    """decoders == NULL runs; n_names == 0 runs and writes no field"""
    for name in ("headers_n65", "response_values_no_names"):
        kind, maxh, buf, off, names, _ = golden_set(name)
        frames, fields, dec = rhp.frame_messages_gpu(buf, off, kind, names, maxh, layout, decoders=False, guard=GUARD)
        assert dec is None
        check(name, frames, fields, "rhp_frame_messages without decoders")
    kind, maxh, buf, off, names, _ = golden_set("response_n65")
    frames, fields, _ = rhp.frame_messages_gpu(buf, off, kind, [], maxh, layout, guard=GUARD)
    assert fields.shape == (0, 65)
    assert (frames["result"] == golden_set("response_n65")[5]["result"]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_records_never_read_may_hold_anything(layout):
    name = "response_n257"
    kind, maxh, buf, off, names, _ = golden_set(name)
    msgs, hdrs = (a.copy() for a in rhp.parse_messages_cpu(buf, off, kind, maxh, layout))
    poison_unread(msgs, hdrs)
    frames, fields, dec = rhp.frame_messages_gpu(buf, off, kind, names, maxh, layout, guard=GUARD, records=(msgs, hdrs))
    check(name, frames, fields, "rhp_frame_messages over poisoned records")
    check_decoders(name, dec, 0, "rhp_frame_messages over poisoned records")


@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_gpu_crafted_records_stay_inside_the_message(layout):
    """every crafted offset is checked against ret, and ret against bytes_size, before it becomes an address"""
    buf, off, size, msgs, hdrs, _, _ = crafted()
    frames, fields, _ = rhp.frame_messages_gpu(buf[:size].copy(), off, fs.RESPONSE, fs.NAMES, 4, layout, guard=GUARD,
                                               records=(msgs, hdrs), bytes_size=size)
    check_crafted(frames, fields, "rhp_frame_messages")


@pytest.mark.gpu
def test_gpu_chain_parse_frame_decode():
    """n = 65 chunked responses parsed on the device, framed there with the decoders armed there, their bodies
    gathered into a second device buffer with torch ops and decoded with those decoders: the payloads, and the
    results of a run whose decoders the host zero-filled"""
    import torch
    n, maxh = 65, 8
    rng = np.random.default_rng(65)
    payloads, bodies, msgs = [], [], []
    for i in range(n):
        parts = [bytes(rng.integers(97, 123, size=int(rng.integers(1, 40)), dtype=np.uint8)) for _ in range(i % 4 + 1)]
        body = b"".join(b"%x\r\n" % len(x) + x + b"\r\n" for x in parts) + b"0\r\n" + (b"X-T: 1\r\n" if i % 3 == 0 else b"") + b"\r\n"
        payloads.append(b"".join(parts))
        bodies.append(body)
        msgs.append(fs.msg(fs.RESPONSE, [b"Server: s%d" % i, b"transfer-Encoding: CHUNKed" if i % 2 else b"Transfer-Encoding: chunked"], body=body))
    buf, off = fs.pack(msgs)
    dbytes = torch.from_numpy(buf).to("cuda")
    doff = torch.from_numpy(off.view(np.int64).copy()).to("cuda")
    dmsgs = torch.full((16 * n,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
    dhdrs = torch.full((8 * n * maxh,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
    dframes = torch.full((16 * n,), rhp.FRAME_POISON, dtype=torch.uint8, device="cuda")
    ddec = torch.full((16 * n,), rhp.FRAME_POISON, dtype=torch.uint8, device="cuda")
    L = rhp.LAYOUT_HEADER_MAJOR
    rhp.parse_messages_device(dbytes, buf.size, doff, n, rhp.MSG_RESPONSE, maxh, L, dmsgs, dhdrs)
    rhp.frame_messages_device(dbytes, buf.size, doff, n, rhp.MSG_RESPONSE, maxh, L, dmsgs, dhdrs, dframes, decoders_t=ddec,
                              consume_trailer=1)
    # the bodies, gathered on the device: message i's bytes behind ret, back to back
    ret = dmsgs.view(torch.int32)[0::4].to(torch.int64)
    start, end = doff[:-1] + ret, doff[1:]
    blen = end - start
    boff = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    boff[1:] = torch.cumsum(blen, 0)
    total = int(boff[-1])
    idx = torch.arange(total, device="cuda")
    owner = torch.searchsorted(boff[1:].contiguous(), idx, right=True)
    dbody = torch.zeros((total + 15) // 16 * 16, dtype=torch.uint8, device="cuda")
    dbody[:total] = dbytes[start[owner] + idx - boff[owner]]
    dres = torch.full((16 * n,), rhp.CHUNKED_POISON, dtype=torch.uint8, device="cuda")
    rhp.decode_chunked_device(dbody, dbody.numel(), boff, n, ddec, dres)
    torch.cuda.synchronize()
    frames = dframes.cpu().numpy().view(rhp.FRAME_DTYPE)
    assert (frames["result"] == 1).all() and (frames["body_kind"] == rhp.FRAME_CHUNKED).all() and (frames["body_len"] == 0).all()
    res = dres.cpu().numpy().view(rhp.CHUNKED_RESULT_DTYPE)
    out, bo = dbody.cpu().numpy(), boff.cpu().numpy()
    assert bo[-1] == sum(len(b) for b in bodies)
    for i in range(n):
        assert res["ret"][i] == 0 and res["size"][i] == len(payloads[i]), (i, res[i])
        assert bytes(out[int(bo[i]): int(bo[i]) + len(payloads[i])]) == payloads[i], i
    # the same bodies with decoders the host zero-filled
    host_dec = np.zeros(n, dtype=rhp.CHUNKED_DTYPE)
    host_dec["consume_trailer"] = 1
    packed = np.frombuffer(b"".join(bodies), dtype=np.uint8)
    want, want_dec, _ = rhp.decode_chunked_gpu(packed, bo.astype(np.uint64), host_dec)
    assert (res == want).all()
    assert (ddec.cpu().numpy().view(rhp.CHUNKED_DTYPE) == want_dec).all()
