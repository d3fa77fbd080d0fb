#!/usr/bin/env python3
"""Writes tests/golden/forward_sessions.npz (dev container only: needs the
compiled reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every case of tests/forward_sets.py the records are the host fix-up's and
the host classify's (held to their own golden files by their own tests), in
both layouts, which must agree.  rule() is rhp.h's rhp_forward_sessions in
plain Python over those records: which slot is forwarded, why not, and a
forwarded slot's bytes.  The reference has no request writer, so what it has
to say about those bytes is the round trip: accept() reads every forwarded
slot's bytes back with the compiled reference's http_read_request and holds
the answer to the records the bytes were written from.  Nothing is written
unless every slot passes.

The file (np.savez_compressed), C cases:
  case_name str [C]
  case_slot u32 [C + 1]: the case's slots are why / size [lo, hi)   why u8, size u32
  case_byte u64 [C + 1]: its forwarded bytes are out [lo, hi), slot after slot
  case_sess u32 [C + 1]: its fwd_off row is fwd_off [lo, hi) (n_sessions + 1 entries)
  case_word u32 [C + 1]: its head_bits words are head_bits [lo, hi)
usage: python tests/golden/make_golden_forward.py
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

GOLDEN = os.path.join(HERE, "forward_sessions.npz")
NULL = rhp.RHP_NAME_NULL
BUILTIN = (b"Content-Length", b"Transfer-Encoding")


def rule(res, sessions, results, starts, route, off, bytes_size, maxh, n_routes, mask, names, extra):
    """rhp.h's rule over any records, sessions ascending: (why u8 [n], rows, fwd_off u32 [ns + 1], head_bits u32);
    a row, one per forwarded slot in slot order: (slot, bytes, method, target, kept [(name, value)], body or None).
    bytes.upper maps a..z alone: the classify fold."""
    reqs, hdrs, http, buf = res.reqs, res.hdrs, res.http, res.bytes_out
    n, ns = len(reqs), len(sessions)
    why = np.zeros(n, dtype=np.uint8)
    rows = []
    drop = tuple(BUILTIN) + tuple(names)
    same = lambda a, b: len(a) == len(b) and bytes(a).upper() == bytes(b).upper()
    readable = bytes_size & ~3
    for i in range(n):
        owners = [s for s in range(ns) if int(sessions["piece_lo"][s]) <= i]
        s = owners[-1] if owners else None
        if s is not None:
            lo, hi, nsl = int(sessions["piece_lo"][s]), int(sessions["piece_hi"][s]), int(results["n_slots"][s])
        if s is None or not (lo <= i < lo + nsl and lo <= hi <= n):
            why[i] = rhp.FORWARD_UNUSED
            continue
        ret, rs = int(reqs["ret"][i]), int(starts[i])
        a, e = int(off[lo]), int(off[hi])
        last = lo + nsl - 1
        if not (int(http["result"][i]) == 1 and ret > 0):
            why[i] = rhp.FORWARD_NOT_READY
        elif not (a <= rs <= e and ret <= e - rs and rs + ret <= readable):
            why[i] = rhp.FORWARD_OUTSIDE
        elif last < n and int(http["result"][last]) == -1:
            why[i] = rhp.FORWARD_CLOSED
        elif not (int(route[i]) < n_routes and (mask >> int(route[i])) & 1):
            why[i] = rhp.FORWARD_ROUTE
        if why[i]:
            continue
        recs = [tuple(int(v) for v in hdrs[i, k].tolist()) for k in range(min(int(reqs["num_headers"][i]), maxh))]
        mo, ml, po, pl = (int(reqs[f][i]) for f in ("method_off", "method_len", "path_off", "path_len"))
        kind, bl = int(http["body_kind"][i]), int(http["body_len"][i])
        if any(no == NULL for no, _, _, _ in recs):
            why[i] = rhp.FORWARD_FOLD
        elif mo + ml > ret or po + pl > ret or any(no + nl > ret or vo + vl > ret for no, nl, vo, vl in recs):
            why[i] = rhp.FORWARD_SPAN
        elif kind > 1:
            why[i] = rhp.FORWARD_BODY
        elif kind == 1 and bl >= 2 ** 32:
            why[i] = rhp.FORWARD_LONG
        elif kind == 1 and not (rs + ret + bl <= e and rs + ret + bl <= readable):
            why[i] = rhp.FORWARD_BODY_OUTSIDE
        if why[i]:
            continue
        at = lambda o, l: bytes(buf[rs + o: rs + o + l])
        method, target = at(mo, ml), at(po, pl)
        kept = [(at(no, nl), at(vo, vl)) for no, nl, vo, vl in recs if not any(same(at(no, nl), d) for d in drop)]
        body = at(ret, bl) if kind == 1 else None
        text = method + b" " + target + b" HTTP/1.1\r\n" + b"".join(k + b": " + v + b"\r\n" for k, v in kept)
        if body is not None:
            text += b"Content-Length: %d\r\n" % bl
        text += bytes(extra) + b"\r\n" + (body or b"")
        rows.append((i, text, method, target, kept, body))
    fwd = np.concatenate([[0], np.cumsum(why == 0)]).astype(np.uint32)
    fwd_off = np.array([fwd[min(int(sessions["piece_lo"][s]), n)] for s in range(ns)] + [fwd[n]], dtype=np.uint32)
    head_bits = np.zeros((int(fwd[n]) + 31) // 32, dtype=np.uint32)
    for q, r in enumerate(rows):
        if r[2] == b"HEAD":
            head_bits[q >> 5] |= np.uint32(1 << (q & 31))
    return why, rows, fwd_off, head_bits


def extra_lines(extra):
    """the (name, value) pairs of the caller's whole header lines"""
    return [tuple(line.split(b": ", 1)) for line in bytes(extra).split(b"\r\n") if line]


def accept(run_reference, rows, extra, label):
    """the compiled reference's http_read_request over every forwarded slot's bytes gives back what they were
    written from"""
    for i, text, method, target, kept, body in rows:
        want = kept + ([(b"Content-Length", b"%d" % len(body))] if body is not None else []) + extra_lines(extra)
        buf = np.frombuffer(text + b"\0" * rhp.RHP_PAD, dtype=np.uint8).copy()
        off = np.array([0, len(text)], dtype=np.uint64)
        reqs, hdrs, http, rw = run_reference(buf, off, 64, rhp.MODE_HTTP)
        r, x = reqs[0], http[0]
        at = lambda o, l: bytes(rw[int(o): int(o) + int(l)])
        where = f"{label} slot {i}"
        assert int(x["result"]) == 1 and int(x["consumed"]) == len(text), f"{where}: result {x['result']} consumed {x['consumed']} of {len(text)}"
        assert at(r["method_off"], r["method_len"]) == method and at(r["path_off"], r["path_len"]) == target, f"{where}: method or target"
        got = [(at(h["name_off"], h["name_len"]), at(h["value_off"], h["value_len"])) for h in hdrs[0][: int(r["num_headers"])]]
        assert got == want, f"{where}: fields {got} != {want}"
        if body is None:
            assert int(x["body_kind"]) == 0, f"{where}: a body where none was written"
        else:
            assert int(x["body_kind"]) == 1 and at(x["body_off"], x["body_len"]) == body, f"{where}: the body differs"


def expected(fs, name, run_reference=None):
    """(why u8 [n], size u32 [n], out u8, fwd_off, head_bits) of a case: rule() over the host's records in both
    layouts, and with run_reference the acceptance check"""
    c = fs.by_name(name)
    buf, off, sess = fs.packed(name)
    got = []
    for layout in fs.LAYOUTS:
        res, results, starts, route = fs.host_round(name, layout)
        got.append(rule(res, sess, results, starts, route, off, buf.size, c["maxh"], len(fs.ROUTES), fs.FORWARD_MASK, c["names"], c["extra"]))
    (why, rows, fwd_off, head_bits), other = got
    assert (why == other[0]).all() and [r[1] for r in rows] == [r[1] for r in other[1]], f"{name}: the two layouts differ"
    if run_reference is not None:
        accept(run_reference, rows, c["extra"], name)
    size = np.zeros(len(why), dtype=np.uint32)
    for r in rows:
        size[r[0]] = len(r[1])
    return why, size, np.frombuffer(b"".join(r[1] for r in rows), dtype=np.uint8), fwd_off, head_bits


def main():
    import forward_sets as fs
    from oracle_util import reference, run_reference
    assert reference() is not None, "the compiled reference needs its sources"
    names, slot, byte, sessw, word, whys, sizes, outs, fwds, bits = [], [0], [0], [0], [0], [], [], [], [], []
    for c in fs.all_cases():
        why, size, out, fwd_off, head_bits = expected(fs, c["name"], run_reference)
        names.append(c["name"])
        whys.append(why); sizes.append(size); outs.append(out); fwds.append(fwd_off); bits.append(head_bits)
        slot.append(slot[-1] + len(why)); byte.append(byte[-1] + len(out)); sessw.append(sessw[-1] + len(fwd_off)); word.append(word[-1] + len(head_bits))
    np.savez_compressed(GOLDEN, case_name=np.array(names), case_slot=np.array(slot, dtype=np.uint32), case_byte=np.array(byte, dtype=np.uint64),
                        case_sess=np.array(sessw, dtype=np.uint32), case_word=np.array(word, dtype=np.uint32), why=np.concatenate(whys),
                        size=np.concatenate(sizes), out=np.concatenate(outs), fwd_off=np.concatenate(fwds), head_bits=np.concatenate(bits))
    size = os.path.getsize(GOLDEN)
    print(f"{GOLDEN}: {len(names)} cases, {slot[-1]} slots, {int((np.concatenate(whys) == 0).sum())} forwarded, {byte[-1]} bytes, {size} bytes")
    assert size <= 64 * 1024, "a few tens of KB, as its siblings"


if __name__ == "__main__":
    main()
