#!/usr/bin/env python3
"""Writes tests/golden/frame_messages.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every set of tests/frame_sets.py the expected frames and fields come from the
compiled reference in two independent ways, which must agree for every message
with ret > 0 (the maker stops where they do not, and prints any message it could
not cross-check):
  1. composition.  phr_parse_response / phr_parse_headers give the header array
     (make_golden_messages.reference_message); http_field_lookup is called on it
     for Transfer-Encoding, Content-Length and the set's names; data_equal_case
     against "Chunked" and libc strtoull on the value where it lies are applied
     in the order of http.c:204-233.
  2. http_read_request itself on a twin request (oracle_util.run_reference,
     MODE_HTTP): "POST / HTTP/1.1" and the message's header lines (a response's
     start behind its first LF), parsed at the same max_headers, followed by the
     message's own bytes behind ret -- by "0\\r\\n\\r\\n" where the composition
     says CHUNKED.  -1 on the twin exactly when the frame result is -1; NONE:
     1 with no body; LENGTH: 1 exactly when !(len < ret + body_len) mod 2^64,
     then an equal body_len; CHUNKED: 1.

The file is flat, so that the stand-alone C test (tests/frame_messages_host_test.c)
reads it as well: np.savez, not compressed; S sets, N messages.
  set_name  str [S]        set_kind, set_maxh  u32 [S]
  set_msg   u32 [S + 1]    set s holds messages [set_msg[s], set_msg[s + 1])
  set_byte  u64 [S + 1]    its buffer is bytes[set_byte[s], set_byte[s + 1]) (16-byte aligned start, pad included)
  bytes     u8
  offsets   u64 [N + S]    set s: offsets[set_msg[s] + s ..], n + 1 entries from its buffer's start
  set_names u32 [S + 1]    its lookup names are name_span[set_names[s], set_names[s + 1])
  name_span u32 [T, 2]     (off, len) into name_text
  name_text u8
  ret       i32 [N]        the reference's own parse result (above RHP_MAX_LEN: the batch answers RHP_RET_TOOLONG)
  result    i32 [N]        body_kind u32 [N]        body_len u64 [N]        (rhp_frame_t)
  set_field u32 [S + 1]    its fields are field[set_field[s], set_field[s + 1]): n_names * n entries, name-major
  field     u16 [F, 2]     value_off (RHP_NAME_NULL: absent), value_len
usage: python tests/golden/make_golden_frame_messages.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import libreactorng_amd as rhp  # noqa: E402
import frame_sets as fs  # noqa: E402
from make_golden_classify import Field, String  # noqa: E402
from make_golden_messages import reference, reference_message  # noqa: E402
from oracle_util import run_reference  # noqa: E402

GOLDEN = os.path.join(HERE, "frame_messages.npz")
POST = b"POST / HTTP/1.1\r\n"
M64 = (1 << 64) - 1


def composer(ref):
    """message -> (ret, result, kind, body_len, [(value_off | RHP_NAME_NULL, value_len) per name]) by composition"""
    lookup = ref.http_field_lookup
    lookup.argtypes = [ctypes.POINTER(Field), ctypes.c_size_t, String]
    lookup.restype = String
    ref.string_null.restype = String
    null = ref.string_null().base
    ref.data_equal_case.argtypes = [String, String]
    ref.data_equal_case.restype = ctypes.c_bool
    libc = ctypes.CDLL(None)
    libc.strtoull.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    libc.strtoull.restype = ctypes.c_ulonglong
    fixed = {x: ctypes.create_string_buffer(x, len(x)) for x in (b"Transfer-Encoding", b"Content-Length", b"Chunked")}
    as_string = lambda cbuf, size: String(ctypes.addressof(cbuf), size)

    def compose(kind, buf, start, length, maxh, names):
        absent = [(rhp.RHP_NAME_NULL, 0)] * len(names)
        ret, _, _, _, _, recs = reference_message(ref, kind, buf, start, length, maxh, 0)
        if ret <= 0 or ret > rhp.RHP_MAX_LEN:
            return ret, (-1 if ret == -1 else rhp.RHP_RET_TOOLONG if ret > 0 else 0), rhp.FRAME_NONE, 0, absent
        base = buf.ctypes.data + start
        arr = (Field * max(len(recs), 1))()
        for k, (no, nl, vo, vl) in enumerate(recs):
            arr[k].name = String(None if no == rhp.RHP_NAME_NULL else base + no, nl)
            arr[k].value = String(base + vo, vl)
        keep = [ctypes.create_string_buffer(bytes(x), len(x)) for x in names]
        fields = []
        for j, x in enumerate(names):
            v = lookup(arr, len(recs), as_string(keep[j], len(x)))
            fields.append((v.base - base, v.size) if v.base != null else (rhp.RHP_NAME_NULL, 0))
        encoding = lookup(arr, len(recs), as_string(fixed[b"Transfer-Encoding"], 17))
        length_ = lookup(arr, len(recs), as_string(fixed[b"Content-Length"], 14))
        if length_.size:                                     # http.c:208
            if encoding.size:                                # :210
                return ret, -1, rhp.FRAME_NONE, 0, fields
            return ret, 1, rhp.FRAME_LENGTH, int(libc.strtoull(length_.base, None, 10)), fields   # :212
        if encoding.size:                                    # :221
            if not ref.data_equal_case(encoding, as_string(fixed[b"Chunked"], 7)):   # :223
                return ret, -1, rhp.FRAME_NONE, 0, fields
            return ret, 1, rhp.FRAME_CHUNKED, 0, fields
        return ret, 1, rhp.FRAME_NONE, 0, fields

    return compose


def cross_check(name, kind, maxh, msgs, rows):
    """http_read_request on the twin requests of the messages with ret > 0 against the composition's rows"""
    twins, which = [], []
    for i, (m, (ret, result, fkind, blen, _)) in enumerate(zip(msgs, rows)):
        if ret <= 0:
            continue
        if ret > rhp.RHP_MAX_LEN:
            print(f"  {name} message {i}: not cross-checked (ret {ret} above RHP_MAX_LEN: the batch answers RHP_RET_TOOLONG)")
            continue
        first = m.index(b"\n") + 1 if kind == fs.RESPONSE else 0
        tail = b"0\r\n\r\n" if fkind == rhp.FRAME_CHUNKED else m[ret:]
        twins.append(POST + m[first:ret] + tail)
        which.append((i, ret - first + len(POST)))
    if not twins:
        return 0
    buf, off = fs.pack(twins)
    reqs, _, http, _ = run_reference(buf, off, maxh, rhp.MODE_HTTP)
    for t, (i, tret) in enumerate(which):
        _, result, fkind, blen, _ = rows[i]
        got, tlen = int(http["result"][t]), len(twins[t])
        what = f"{name} message {i} {msgs[i][:120]!r}: the twin request gives {got}"
        assert (got == -1) == (result == -1), what + f", the composition {result}"
        if result == -1:
            continue
        if fkind == rhp.FRAME_LENGTH:
            whole = not (tlen < ((tret + blen) & M64))
            assert got == (1 if whole else 0), what + f" with body_len {blen}, len {tlen}, ret {tret}"
            if whole:
                assert int(http["body_kind"][t]) == 1 and int(http["body_len"][t]) == blen, what + " and another body_len"
        else:
            assert got == 1, what
            if fkind == rhp.FRAME_NONE:
                assert int(http["body_kind"][t]) == 0 and int(http["consumed"][t]) == tret, what + " with a body"
    return len(which)


def main():
    compose = composer(reference())
    names_, kinds, maxhs, set_msg, set_byte, set_names, set_field = [], [], [], [0], [0], [0], [0]
    chunks, offsets, rows_all, spans, text, fields = [], [], [], [], b"", []
    for name, kind, maxh, msgs, names in fs.all_sets():
        buf, off = fs.pack(msgs)
        buf = np.concatenate([buf, np.zeros((-buf.size) % 16, dtype=np.uint8)])   # the next set starts 16-aligned
        rows = [compose(kind, buf, int(off[i]), int(off[i + 1] - off[i]), maxh, names) for i in range(len(msgs))]
        checked = cross_check(name, kind, maxh, msgs, rows)
        rows_all += [r[:4] for r in rows]
        fields += [rows[i][4][j] for j in range(len(names)) for i in range(len(msgs))]
        for x in names:
            spans.append((len(text), len(x)))
            text += bytes(x)
        names_.append(name)
        kinds.append(kind)
        maxhs.append(maxh)
        set_msg.append(set_msg[-1] + len(msgs))
        set_byte.append(set_byte[-1] + buf.size)
        set_names.append(len(spans))
        set_field.append(len(fields))
        chunks.append(buf)
        offsets.append(off)
        res = np.array([r[1] for r in rows])
        k = np.array([r[2] for r in rows])
        print(f"{name}: {len(msgs)} messages, max_headers {maxh}, {len(names)} names: result 1 x {int((res == 1).sum())} "
              f"(none {int(((res == 1) & (k == 0)).sum())}, length {int((k == 1).sum())}, chunked {int((k == 2).sum())}), "
              f"-1 x {int((res == -1).sum())}, 0 x {int((res == 0).sum())}; {checked} cross-checked with http_read_request")
    u32 = lambda a: np.array(a, dtype=np.uint32)
    out = dict(set_name=np.array(names_), set_kind=u32(kinds), set_maxh=u32(maxhs), set_msg=u32(set_msg),
               set_byte=np.array(set_byte, dtype=np.uint64), bytes=np.concatenate(chunks), offsets=np.concatenate(offsets),
               set_names=u32(set_names), name_span=u32(spans).reshape(-1, 2), name_text=np.frombuffer(text, dtype=np.uint8),
               ret=np.array([r[0] for r in rows_all], dtype=np.int32), result=np.array([r[1] for r in rows_all], dtype=np.int32),
               body_kind=u32([r[2] for r in rows_all]), body_len=np.array([r[3] for r in rows_all], dtype=np.uint64),
               set_field=u32(set_field), field=np.array(fields, dtype=np.uint16).reshape(-1, 2))
    np.savez(GOLDEN, **out)
    print(f"{GOLDEN}: {len(names_)} sets, {len(rows_all)} messages, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
