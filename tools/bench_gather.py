#!/usr/bin/env python3
"""Times rhp_gather_wide (include/rhp.h) on the GPU beside what it replaces, in
one process: HIP events around each step, median of --reps after --warmup.

Rounds of TFB plaintext GETs, sessions x requests per session (one piece per
request): 64 x 64, 4096 x 1, 256 x 256 and 65536 x 1, each with 0 %, 1 % and
10 % of the requests made wide: half by a leading CRLF, half chunked POSTs with
64-byte bodies.  Per round one JSON line:
  old_us       the copy the reactor falls back to when one in-use slot is wide
               (reactor/batch.c): one D2H of 176 B per slot (the o_req .. o_sres
               span, a device buffer of that size) into pinned memory, plus, with
               chunked requests in the round, the D2H of the byte span from the
               first to the last of them
  gather_us    rhp_gather_wide (three launches) plus the D2H of totals and of the
               three areas at their used sizes, into pinned memory
  gather_call_us   the call alone
  pack_us      rhp_pack_dense over the same round, for scale
  parse_us, parse_fixup_us   the input restored and parsed, and the same with
               rhp_fixup_sessions behind it (the fix-up de-frames in place, so it
               cannot be repeated alone): their difference is the fix-up
The totals are compared with the round's make-up before anything is timed.
usage: python tools/bench_gather.py [--out profiles/gather/bench_gather.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import libreactorng_amd as rhp  # noqa: E402

TFB = (b"GET /plaintext HTTP/1.1\r\nHost: tfb-server:8080\r\nAccept: text/plain\r\n"
       b"Connection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n\r\n")
CRLF = b"\r\n" + TFB
CHUNKED = b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n40\r\n" + b"b" * 64 + b"\r\n0\r\n\r\n"
ROUNDS = ((64, 64), (4096, 1), (256, 256), (65536, 1))
PERCENT = (0, 1, 10)
OLD_BYTES_PER_SLOT = 16 + 16 * 8 + 24 + 8
MAXH = 16


def median_us(fn, reps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def make_round(sessions, per, percent):
    """(buf, off, sessions, kind u8 [n]: 0 TFB, 1 leading CRLF, 2 chunked POST)"""
    n = sessions * per
    kind = np.zeros(n, dtype=np.uint8)
    if percent:
        wide = np.random.default_rng(n + percent).choice(n, size=max(n * percent // 100, 2), replace=False)
        kind[wide[::2]], kind[wide[1::2]] = 1, 2
    reqs = (TFB, CRLF, CHUNKED)
    lens = np.array([len(r) for r in reqs], dtype=np.uint64)[kind]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    buf = np.zeros(int(off[-1]) + rhp.RHP_PAD, dtype=np.uint8)
    buf[: int(off[-1])] = np.frombuffer(b"".join(reqs[k] for k in kind.tolist()), dtype=np.uint8)
    sess = np.zeros(sessions, dtype=rhp.SESSION_DTYPE)
    sess["piece_lo"] = np.arange(sessions) * per
    sess["piece_hi"] = sess["piece_lo"] + per
    return buf, off, sess, kind


def bench_round(sessions, per, percent, reps, warmup):
    import torch
    buf, off, sess, kind = make_round(sessions, per, percent)
    n = sessions * per
    db = rhp.DeviceBatch(buf, off, MAXH, rhp.MODE_HTTP, flags=rhp.BATCH_SPECULATIVE)
    pristine = db.bytes.clone()
    u8 = lambda size: torch.zeros(max(size, 8), dtype=torch.uint8, device="cuda")
    pin = lambda size: torch.zeros(max(size, 8), dtype=torch.uint8).pin_memory()
    ds = torch.from_numpy(sess.view(np.uint8).copy()).to("cuda")
    dres, dst = u8(sessions * rhp.SESSION_RESULT_DTYPE.itemsize), u8(n * 8)
    ddq, dhc, dlens = u8(8 * n), u8(8 * n), u8(2 * MAXH * n)
    n_wide, n_chunked = int((kind != 0).sum()), int((kind == 2).sum())
    caps = (max(n_wide, 1), max(n_wide * MAXH, 1), max(n_chunked * 64, 1))
    totals, slots, hdrs, body = u8(16), u8(caps[0] * 64), u8(caps[1] * 8), u8(caps[2])
    work = u8(rhp.wide_work_words(n) * 8)
    o = rhp.WideOut(totals.data_ptr(), slots.data_ptr(), caps[0], hdrs.data_ptr(), caps[1], body.data_ptr(), caps[2],
                    work.data_ptr())
    d = db.desc()
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    L = rhp.lib()

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    def parse():
        db.bytes.copy_(pristine)
        db.launch()

    fixup = lambda: check(L.rhp_fixup_sessions(ctypes.byref(d), vp(ds.data_ptr()), sessions, vp(dres.data_ptr()),
                                               vp(dst.data_ptr()), stream), "rhp_fixup_sessions")
    pack = lambda: check(L.rhp_pack_dense(ctypes.byref(d), vp(ddq.data_ptr()), vp(dhc.data_ptr()), vp(dlens.data_ptr()),
                                          stream), "rhp_pack_dense")
    gather = lambda: check(L.rhp_gather_wide(ctypes.byref(d), vp(ds.data_ptr()), sessions, vp(dres.data_ptr()),
                                             vp(dst.data_ptr()), vp(ddq.data_ptr()), vp(dhc.data_ptr()), ctypes.byref(o),
                                             stream), "rhp_gather_wide")
    parse()
    fixup()
    pack()
    gather()
    torch.cuda.synchronize()
    t = totals.cpu().numpy().view(rhp.WIDE_TOTALS_DTYPE)[0]
    got = (int(t["n_wide"]), int(t["n_hdrs"]), int(t["body_bytes"]))
    want = (n_wide, 4 * int((kind == 1).sum()) + n_chunked, 64 * n_chunked)
    assert got == want, (got, want)

    # the copy it replaces: 176 B per slot, and the byte span of the chunked requests
    old_dev, old_host = u8(OLD_BYTES_PER_SLOT * n), pin(OLD_BYTES_PER_SLOT * n)
    ch = np.flatnonzero(kind == 2)
    span = (int(off[ch[0]]), int(off[ch[-1] + 1])) if len(ch) else (0, 0)
    span_host = pin(span[1] - span[0])

    def old():
        old_host.copy_(old_dev, non_blocking=True)
        if span[1] > span[0]:
            span_host[: span[1] - span[0]].copy_(db.bytes[span[0]: span[1]], non_blocking=True)

    used = (16, got[0] * 64, got[1] * 8, got[2])
    hosts = [pin(k) for k in used]
    devs = (totals, slots, hdrs, body)

    def new():
        gather()
        for h, dv, k in zip(hosts, devs, used):
            if k:
                h[:k].copy_(dv[:k], non_blocking=True)

    r = {"sessions": sessions, "per_session": per, "slots": n, "percent_wide": percent, "n_wide": got[0], "n_hdrs": got[1],
         "body_bytes": got[2], "old_bytes": OLD_BYTES_PER_SLOT * n + span[1] - span[0], "new_bytes": sum(used), "reps": reps,
         "old_us": median_us(old, reps, warmup), "gather_us": median_us(new, reps, warmup),
         "gather_call_us": median_us(gather, reps, warmup), "pack_us": median_us(pack, reps, warmup)}
    r["parse_us"] = median_us(parse, reps, warmup)
    r["parse_fixup_us"] = median_us(lambda: (parse(), fixup()), reps, warmup)
    r["gather_over_old"] = r["gather_us"] / r["old_us"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_gather needs a GPU"
    lines = []
    for sessions, per in ROUNDS:
        for percent in PERCENT:
            r = bench_round(sessions, per, percent, a.reps, a.warmup)
            r["library_sha256"] = rhp.library_sha256()
            lines.append(json.dumps(r))
            print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
