#!/usr/bin/env python3
"""Writes tests/golden/messages.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every set of tests/message_sets.py the messages are packed as the batch has
them (back to back, RHP_PAD zero bytes behind the last: what the reference reads
past a message's end is its neighbour) and phr_parse_response / phr_parse_headers
of the compiled reference are called directly, through ctypes, on every message
in place.  Pointers become offsets from the message start.

The file is flat, so that the stand-alone C test (tests/messages_host_test.c)
reads it as well: np.savez, not compressed; S sets, N messages, H header records.
  set_name  str [S]        set_kind, set_maxh, set_has_ll  u32 [S]
  set_msg   u32 [S + 1]    set s holds messages [set_msg[s], set_msg[s + 1])
  set_byte  u64 [S + 1]    its buffer is bytes[set_byte[s], set_byte[s + 1]) (16-byte aligned start, pad included)
  bytes     u8
  offsets   u64 [N + S]    set s: offsets[set_msg[s] + s ..], n + 1 entries from its buffer's start
  last_len  u64 [N]        (0 where the set has none)
  ret       i32 [N]        the reference's own value (above RHP_MAX_LEN: the batch answers RHP_RET_TOOLONG)
  status, msg_off, msg_len, minor, num_headers  i32 [N]   (meaningful for ret > 0; msg_* and status: responses)
  hdr_lo    u32 [N + 1]    message i's header records: hdr[hdr_lo[i], hdr_lo[i + 1]) (none unless 0 < ret <= RHP_MAX_LEN)
  hdr       u16 [H, 4]     name_off (RHP_NAME_NULL: name == NULL), name_len, value_off, value_len
usage: python tests/golden/make_golden_messages.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import libreactorng_amd as rhp  # noqa: E402
import message_sets as ms  # noqa: E402

GOLDEN = os.path.join(HERE, "messages.npz")


def reference():
    ref = ctypes.CDLL(os.path.join(ROOT, "oracle", "_ref", "libref.so"))
    vp, sz, P = ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER
    ref.phr_parse_response.argtypes = [vp, sz, P(ctypes.c_int), P(ctypes.c_int), P(vp), P(sz), P(rhp.PhrHeader), P(sz), sz]
    ref.phr_parse_response.restype = ctypes.c_int
    ref.phr_parse_headers.argtypes = [vp, sz, P(rhp.PhrHeader), P(sz), sz]
    ref.phr_parse_headers.restype = ctypes.c_int
    return ref


def reference_message(ref, kind, buf, start, length, max_headers, last_len):
    """(ret, status, msg_off, msg_len, minor, [(name_off | RHP_NAME_NULL, name_len, value_off, value_len)])"""
    hdrs = (rhp.PhrHeader * max(max_headers, 1))()
    msg, ml, nh = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(max_headers)
    minor, status = ctypes.c_int(-1), ctypes.c_int(0)
    base = buf.ctypes.data + start
    if kind == ms.RESPONSE:
        ret = ref.phr_parse_response(base, length, ctypes.byref(minor), ctypes.byref(status), ctypes.byref(msg),
                                     ctypes.byref(ml), hdrs, ctypes.byref(nh), last_len)
    else:
        ret = ref.phr_parse_headers(base, length, hdrs, ctypes.byref(nh), last_len)
    if ret <= 0:
        return ret, 0, 0, 0, -1, []
    mo = (msg.value - base, ml.value) if kind == ms.RESPONSE else (0, 0)
    recs = [((x.name - base) if x.name else rhp.RHP_NAME_NULL, x.name_len, x.value - base, x.value_len)
            for x in hdrs[: nh.value]]
    return ret, status.value, mo[0], mo[1], minor.value, recs


def main():
    ref = reference()
    sets = ms.all_sets()
    names, kinds, maxhs, has_ll, set_msg, set_byte = [], [], [], [], [0], [0]
    chunks, offsets, last_len, rows, hdr_lo, hdr = [], [], [], [], [0], []
    for name, kind, maxh, msgs, ll in sets:
        buf, off = ms.pack(msgs)
        buf = np.concatenate([buf, np.zeros((-buf.size) % 16, dtype=np.uint8)])   # the next set starts 16-aligned
        for i in range(len(msgs)):
            v = 0 if ll is None else ll[i]
            r = reference_message(ref, kind, buf, int(off[i]), int(off[i + 1] - off[i]), maxh, v)
            rows.append((r[0], r[1], r[2], r[3], r[4], len(r[5])))
            if 0 < r[0] <= ms.RHP_MAX_LEN:
                hdr += r[5]
            hdr_lo.append(len(hdr))
            last_len.append(v)
        names.append(name)
        kinds.append(kind)
        maxhs.append(maxh)
        has_ll.append(int(ll is not None))
        set_msg.append(set_msg[-1] + len(msgs))
        set_byte.append(set_byte[-1] + buf.size)
        chunks.append(buf)
        offsets.append(off)
        rets = np.array([x[0] for x in rows[set_msg[-2]:]])
        print(f"{name}: {len(msgs)} messages, max_headers {maxh}: {int((rets > 0).sum())} parsed, "
              f"{int((rets == -1).sum())} x -1, {int((rets == -2).sum())} x -2")
    rows = np.array(rows, dtype=np.int64)
    u32 = lambda a: np.array(a, dtype=np.uint32)
    out = dict(set_name=np.array(names), set_kind=u32(kinds), set_maxh=u32(maxhs), set_has_ll=u32(has_ll),
               set_msg=u32(set_msg), set_byte=np.array(set_byte, dtype=np.uint64), bytes=np.concatenate(chunks),
               offsets=np.concatenate(offsets), last_len=np.array(last_len, dtype=np.uint64),
               hdr_lo=u32(hdr_lo), hdr=np.array(hdr, dtype=np.uint16).reshape(-1, 4))
    for k, col in enumerate(("ret", "status", "msg_off", "msg_len", "minor", "num_headers")):
        out[col] = rows[:, k].astype(np.int32)
    np.savez(GOLDEN, **out)
    print(f"{GOLDEN}: {len(sets)} sets, {len(rows)} messages, {len(hdr)} header records, {os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
