#!/usr/bin/env python3
"""Writes tests/golden/walk_responses.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every set of tests/walk_sets.py the walk of rhp.h (rhp_walk_responses) is
written out here in plain Python, session by session, and every value it steps
by is the compiled reference's:
  parse    phr_parse_response, called in place on the packed buffer, so that what
           it reads past the session's end is the next session's bytes and then
           the pad (make_golden_messages.reference_message)
  framing  http_field_lookup for Transfer-Encoding and Content-Length over the
           header array that parse returned, data_equal_case against "Chunked",
           libc strtoull (make_golden_frame_messages.composer)
  body     phr_decode_chunked from a zero decoder on a private copy of
           [pos + ret, e) (make_golden_decode_chunked.reference_call); for the
           de-framed bytes a second call on a copy of the body's own wire span
The one rule that is not the reference's is stated here as rhp.h states it: a
status of 100..199, 204 or 304 has no body.

The file is flat, so that the stand-alone C test (tests/walk_responses_host_test.c)
reads it as well: np.savez, not compressed; S sets, NS sessions, NT slots.
  set_name  str [S]        set_maxh, set_flags  u32 [S]
  set_sess  u32 [S + 1]    set s holds sessions [set_sess[s], set_sess[s + 1])
  set_slot  u32 [S + 1]    and the slots [set_slot[s], set_slot[s + 1]) (its n_slots_total)
  set_byte  u64 [S + 1]    its buffer is bytes[set_byte[s], set_byte[s + 1]) (16-byte aligned start, pad included)
  bytes     u8             deframed  u8   the same bytes after a call with RHP_WALK_DEFRAME
  sess_off, slot_off  u64 [NS + S]   set s: entries [set_sess[s] + s ..], n + 1 of them, from its buffer's / slots' start
  n_slots, stop  u32 [NS]  consumed  u64 [NS]                 (rhp_walk_result_t)
  written   u8 [NT]        1: the slot is one of its session's n_slots
  start, body_len, wire_len  u64 [NT]   result  i32 [NT]   body_kind  u32 [NT]   (rhp_walk_slot_t)
  ret, status, msg_off, msg_len, minor, num_headers  i32 [NT]  (rhp_msg_t; but for ret meaningful for ret > 0)
  hdr_lo    u32 [NT + 1]   slot i's header records: hdr[hdr_lo[i], hdr_lo[i + 1]) (none unless ret > 0)
  hdr       u16 [H, 4]     name_off (RHP_NAME_NULL: name == NULL), name_len, value_off, value_len
usage: python tests/golden/make_golden_walk.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import libreactorng_amd as rhp  # noqa: E402
import walk_sets as ws  # noqa: E402
import make_golden_decode_chunked as mdc  # noqa: E402
from make_golden_frame_messages import composer  # noqa: E402
from make_golden_messages import reference, reference_message  # noqa: E402

GOLDEN = os.path.join(HERE, "walk_responses.npz")
NO_BODY = lambda status: 100 <= status <= 199 or status in (204, 304)   # RFC 9112 6.3: the walk's one invented rule


def walker(ref, ref_chunked):
    compose = composer(ref)

    def decode(piece: bytes, trailers: bool):
        dec = bytes(8) + bytes([int(trailers)]) + bytes(7)
        ret, size, _, after = mdc.reference_call(ref_chunked, dec, piece)
        return ret, size, after

    def walk(buf, out, a, e, n_slots, maxh, flags):
        """the walk of one session over `buf` (read in place); `out` gets the de-framed bytes.  Returns
        ((n_slots, stop, consumed), [slot rows]); a slot row: (start, body_len, wire_len, result, body_kind, msg, hdrs)"""
        trailers = bool(flags & ws.TRAILERS)
        pos, rows, stop = a, [], rhp.WALK_END
        while pos < e:
            if len(rows) == n_slots:
                stop = rhp.WALK_MORE
                break
            ret, status, mo, ml, minor, recs = reference_message(ref, rhp.MSG_RESPONSE, buf, pos, e - pos, maxh, 0)
            assert ret <= rhp.RHP_MAX_LEN, "no set holds a head the records cannot encode"
            msg = (ret, status, mo, ml, minor, len(recs))
            body_len = wire_len = 0
            kind = rhp.FRAME_NONE
            if ret <= 0:
                result = -1 if ret == -1 else 0
                stop = rhp.WALK_HEAD if ret == -2 else rhp.WALK_BAD
            else:
                ret2, result, kind, body_len, _ = compose(rhp.MSG_RESPONSE, buf, pos, e - pos, maxh, [])
                assert ret2 == ret
                body, avail = pos + ret, e - (pos + ret)
                if result != 1:
                    stop = rhp.WALK_BAD
                elif NO_BODY(status):
                    body_len = 0
                elif kind == rhp.FRAME_LENGTH:
                    wire_len = min(body_len, avail)
                    if body_len > avail:
                        stop = rhp.WALK_BODY
                elif kind == rhp.FRAME_CHUNKED:
                    r, size, _ = decode(bytes(buf[body: e]), trailers)
                    if r == -1:
                        result, kind, stop = -1, rhp.FRAME_NONE, rhp.WALK_BAD
                    elif r == -2:
                        body_len, wire_len, stop = size, avail, rhp.WALK_BODY
                    else:
                        body_len, wire_len = size, avail - r
                        r2, size2, after = decode(bytes(buf[body: body + wire_len]), trailers)
                        assert (r2, size2) == (0, size), "the body's own wire span decodes to the same body"
                        out[body: body + wire_len] = np.frombuffer(after, dtype=np.uint8)
                elif not flags & ws.NONE_EMPTY:
                    wire_len, stop = avail, rhp.WALK_CLOSE
            rows.append((pos, body_len, wire_len, result, kind, msg, recs if ret > 0 else []))
            if stop != rhp.WALK_END:
                break
            pos += ret + wire_len
        return (len(rows), stop, pos - a), rows

    return walk


def main():
    walk = walker(reference(), mdc.reference())
    names, maxhs, flagss, set_sess, set_slot, set_byte = [], [], [], [0], [0], [0]
    chunks, after, sess_offs, slot_offs, results, slots, msgs, hdr_lo, hdr, written = [], [], [], [], [], [], [], [0], [], []
    for name, maxh, flags, sessions, nslots in ws.all_sets():
        buf, off = ws.pack(sessions)
        buf = np.concatenate([buf, np.zeros((-buf.size) % 16, dtype=np.uint8)])   # the next set starts 16-aligned
        out = buf.copy()
        sl = ws.slot_offsets(nslots)
        stops = []
        for s in range(len(sessions)):
            res, rows = walk(buf, out, int(off[s]), int(off[s + 1]), nslots[s], maxh, flags)
            results.append(res)
            stops.append(res[1])
            for k in range(nslots[s]):
                if k < len(rows):
                    slots.append(rows[k][:5])
                    msgs.append(rows[k][5])
                    hdr += rows[k][6]
                else:
                    slots.append((0, 0, 0, 0, 0))
                    msgs.append((0, 0, 0, 0, 0, 0))
                written.append(int(k < len(rows)))
                hdr_lo.append(len(hdr))
        names.append(name)
        maxhs.append(maxh)
        flagss.append(flags)
        set_sess.append(set_sess[-1] + len(sessions))
        set_slot.append(set_slot[-1] + int(sl[-1]))
        set_byte.append(set_byte[-1] + buf.size)
        chunks.append(buf)
        after.append(out)
        sess_offs.append(off)
        slot_offs.append(sl)
        print(f"{name}: {len(sessions)} sessions, max_headers {maxh}, flags {flags}, {int(sl[-1])} slots: stops "
              + ", ".join(f"{c} x {stops.count(c)}" for c in sorted(set(stops)))
              + f"; {int((buf != out).sum())} bytes moved by the de-framing")
    u32 = lambda a: np.array(a, dtype=np.uint32)
    u64 = lambda a: np.array(a, dtype=np.uint64)
    col = lambda rows, k, dt: np.array([r[k] for r in rows], dtype=dt)
    out = dict(set_name=np.array(names), set_maxh=u32(maxhs), set_flags=u32(flagss), set_sess=u32(set_sess), set_slot=u32(set_slot),
               set_byte=u64(set_byte), bytes=np.concatenate(chunks), deframed=np.concatenate(after),
               sess_off=np.concatenate(sess_offs), slot_off=np.concatenate(slot_offs),
               n_slots=col(results, 0, np.uint32), stop=col(results, 1, np.uint32), consumed=col(results, 2, np.uint64),
               written=np.array(written, dtype=np.uint8),
               start=col(slots, 0, np.uint64), body_len=col(slots, 1, np.uint64), wire_len=col(slots, 2, np.uint64),
               result=col(slots, 3, np.int32), body_kind=col(slots, 4, np.uint32),
               hdr_lo=u32(hdr_lo), hdr=np.array(hdr, dtype=np.uint16).reshape(-1, 4))
    for k, c in enumerate(("ret", "status", "msg_off", "msg_len", "minor", "num_headers")):
        out[c] = col(msgs, k, np.int32)
    np.savez(GOLDEN, **out)
    print(f"{GOLDEN}: {len(names)} sets, {len(results)} sessions, {len(slots)} slots, {len(hdr)} header records, "
          f"{os.path.getsize(GOLDEN)} bytes")


if __name__ == "__main__":
    main()
