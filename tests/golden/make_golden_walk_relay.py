#!/usr/bin/env python3
"""Writes tests/golden/walk_relay.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every case of tests/walk_relay_sets.py, without and with RHP_WALK_DEFRAME,
the walk's records are the host twin's; for the cases that come from
walk_responses.npz, walk_resume.npz and walk_answers.npz they are first held to
those files by their tests' own checks, so the rule below runs over the walks'
golden records.  rule() is rhp.h's rhp_relay_walked in plain Python: which slot
is relayed, why not, and for a relayed slot the rhp_resp_t / rhp_resp_field_t
row a proxy would hand the writer.  The bytes are the compiled reference's
http_write_response over those rows (oracle_util.reference_write_responses).

The file (np.savez_compressed), C cases, two calls each (call 2c: the case's
own flags, call 2c + 1: with RHP_WALK_DEFRAME added):
  case_name str [C]
  call_slot u32 [2C + 1]: the call's slots are why / size [lo, hi)   why u8, size u32: per slot of the call
  call_byte u64 [2C + 1]: the call's replies are out [lo, hi), slot after slot
  same u8 [C]: 1: the second call's answers are the first's and are not stored again (its ranges are empty)
usage: python tests/golden/make_golden_walk_relay.py
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

GOLDEN = os.path.join(HERE, "walk_relay.npz")
NULL = rhp.RHP_NAME_NULL
BUILTIN = (b"Content-Type", b"Content-Length", b"Transfer-Encoding")


def rule(records, buf, bytes_size, sess_off, slot_off, nt, maxh, flags, names):
    """rhp.h's rule over any records, slot_off non-decreasing: (why u8 [nt], rows); a row, one per relayed slot in
    slot order: (slot, status text, type (off, len), body (off, len), [((name off, len), (value off, len))]), the
    offsets into buf.  bytes.upper maps a..z alone: the lookup's fold."""
    results, slots, msgs, hdrs = records
    ns = len(sess_off) - 1
    why = np.zeros(nt, dtype=np.uint8)
    rows = []
    same = lambda a, b: len(a) == len(b) and bytes(a).upper() == bytes(b).upper()
    drop = tuple(BUILTIN) + tuple(names)
    for i in range(nt):
        owners = [s for s in range(ns) if int(slot_off[s]) <= i]
        s = owners[-1] if owners else None
        if s is None or not (int(slot_off[s]) <= i < int(slot_off[s + 1]) and int(slot_off[s + 1]) <= nt and
                             i - int(slot_off[s]) < int(results["n_slots"][s])):
            why[i] = rhp.RELAY_UNUSED
            continue
        st, ret = int(slots["start"][i]), int(msgs["ret"][i])
        a, e = int(sess_off[s]), int(sess_off[s + 1])
        if not (int(slots["result"][i]) == 1 and ret > 0):
            why[i] = rhp.RELAY_NOT_HEAD
        elif not (a <= st <= e and ret <= e - st and st + ret <= (bytes_size & ~3)):
            why[i] = rhp.RELAY_OUTSIDE
        elif 100 <= int(msgs["status"][i]) <= 199:
            why[i] = rhp.RELAY_INTERIM
        elif i - int(slot_off[s]) + 1 == int(results["n_slots"][s]) and int(results["stop"][s]) in (rhp.WALK_BODY, rhp.WALK_CLOSE):
            why[i] = rhp.RELAY_PARTIAL
        if why[i]:
            continue
        recs = [tuple(int(v) for v in hdrs[i, k].tolist()) for k in range(min(int(msgs["num_headers"][i]), maxh))]
        mo, ml = int(msgs["msg_off"][i]), int(msgs["msg_len"][i])
        kind, bl, wl = int(slots["body_kind"][i]), int(slots["body_len"][i]), int(slots["wire_len"][i])
        readable = (bytes_size & ~15) - 16
        if any(no == NULL for no, _, _, _ in recs):
            why[i] = rhp.RELAY_FOLD
        elif (ml and mo + ml > ret) or any(no + nl > ret or vo + vl > ret for no, nl, vo, vl in recs):
            why[i] = rhp.RELAY_SPAN
        elif not ((bl == 0 and wl == 0) or (kind == rhp.FRAME_LENGTH and wl == bl) or (kind == rhp.FRAME_CHUNKED and flags & rhp.WALK_DEFRAME)):
            why[i] = rhp.RELAY_FRAMING
        elif bl >= 2 ** 32:
            why[i] = rhp.RELAY_LONG
        elif not (st + ret + bl <= e and ((st + ret + bl + 3) & ~3) <= readable):
            why[i] = rhp.RELAY_BODY_OUTSIDE
        if why[i]:
            continue
        text = b"%03d" % (int(msgs["status"][i]) % 1000) + (b" " + bytes(buf[st + mo: st + mo + ml]) if ml else b"")
        name_of = lambda r: buf[st + r[0]: st + r[0] + r[1]]
        types = [r for r in recs if same(name_of(r), BUILTIN[0])]
        type_ = (st + types[0][2], types[0][3]) if types else (0, 0)
        fields = [((st + no, nl), (st + vo, vl)) for no, nl, vo, vl in recs if not any(same(buf[st + no: st + no + nl], d) for d in drop)]
        rows.append((i, text, type_, (st + ret, bl), fields))
    return why, rows


def rows_for_writer(buf, rows):
    """(arena, resps u32 [n, 8], fields u32 [f, 4]) for oracle_util.*_write_responses: the batch's bytes with the
    status texts behind them"""
    arena = bytearray(bytes(buf))
    resps, fields = [], []
    for _, text, type_, body, fs in rows:
        resps.append((len(arena), len(text)) + tuple(type_) + tuple(body) + (len(fields), len(fs)))
        arena += text
        fields += [n + v for n, v in fs]
    return (np.frombuffer(bytes(arena) + b"\0" * 4, dtype=np.uint8), np.array(resps, dtype=np.uint32).reshape(-1, 8),
            np.array(fields, dtype=np.uint32).reshape(-1, 4))


def expected(write_responses, records, buf, bytes_size, sess_off, slot_off, nt, maxh, flags, names, date=rhp.DEFAULT_DATE):
    """(why u8 [nt], size u32 [nt], out u8) of one call: rule() and the writer"""
    why, rows = rule(records, buf, bytes_size, sess_off, slot_off, nt, maxh, flags, names)
    size = np.zeros(nt, dtype=np.uint32)
    out = np.zeros(0, dtype=np.uint8)
    if rows:
        out, off = write_responses(*rows_for_writer(buf, rows), date)
        size[[r[0] for r in rows]] = np.diff(off).astype(np.uint32)
    return why, size, out


def hold_to_walk_files(c, out, deframe):
    """the twin's records of a case that comes from one of the walk files are that file's"""
    import test_walk_answers as ta
    import test_walk_responses as t1
    import test_walk_resume as tr
    kind, _, rest = c["name"].partition("_")
    if kind == "walk" and rest in t1.SET_NAMES:
        t1.check(rest, out, "maker", deframe)
    elif kind in ("resume", "answers") and "_r" in rest:
        name, _, r = rest.rpartition("_r")
        if kind == "resume" and name in tr.SET_NAMES:
            tr.check(name, int(r), out, "maker", deframe)
        elif kind == "answers" and name in ta.SET_NAMES:
            mode = ta.golden_set(name)[2]
            ta.check(name, int(r), ta.named(out, mode), "maker", deframe, slot_req=False)


def main():
    import walk_relay_sets as wy
    from oracle_util import reference_write_responses
    names, same, call_slot, call_byte, whys, sizes, outs = [], [], [0], [0], [], [], []
    relayed = 0
    for c in wy.all_cases():
        got = []
        for deframe in (0, rhp.WALK_DEFRAME):
            out = wy.walk_cpu(rhp, c, deframe)
            if c in wy.file_cases():
                hold_to_walk_files(c, out, deframe)
            nt = int(c["slot_off"][-1])
            got.append(expected(reference_write_responses, out[:4], out[4], out[4].size, c["sess_off"], c["slot_off"], nt, c["maxh"],
                                c["flags"] | deframe, c["names"]))
        twice = not all((a == b).all() if a.shape == b.shape else False for a, b in zip(*got))
        names.append(c["name"])
        same.append(0 if twice else 1)
        for k, (why, size, out) in enumerate(got):
            if k == 0 or twice:
                whys.append(why); sizes.append(size); outs.append(out)
                relayed += int((why == 0).sum())
            call_slot.append(call_slot[-1] + (len(why) if k == 0 or twice else 0))
            call_byte.append(call_byte[-1] + (len(out) if k == 0 or twice else 0))
    np.savez_compressed(GOLDEN, case_name=np.array(names), same=np.array(same, dtype=np.uint8), call_slot=np.array(call_slot, dtype=np.uint32),
                        call_byte=np.array(call_byte, dtype=np.uint64), why=np.concatenate(whys), size=np.concatenate(sizes),
                        out=np.concatenate(outs))
    size, limit = os.path.getsize(GOLDEN), os.path.getsize(os.path.join(HERE, "walk_edges.npz"))
    print(f"{GOLDEN}: {len(names)} cases, {call_slot[-1]} slots, {relayed} relayed, {call_byte[-1]} reply bytes, {size} bytes")
    assert size <= limit, f"the file is no larger than walk_edges.npz ({limit} bytes)"


if __name__ == "__main__":
    main()
