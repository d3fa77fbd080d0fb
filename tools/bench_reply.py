#!/usr/bin/env python3
"""Times rhp_reply_sessions (include/rhp.h) on the GPU beside its yardstick, in
one process: HIP events around each call, median of --reps after --warmup.

Rounds of TFB plaintext GETs, sessions x requests per session (one piece per
request): 64 x 64, 256 x 256, 4096 x 1, 65536 x 1 and 16384 x 64 (1M slots).
Every request matches the one route, which is static, so every slot is
answered.  Per round one JSON line:
  reply_us     rhp_reply_sessions (its four launches)
  writer_us    rhp_write_responses over the same number of plaintext rhp_resp_t
               records: the same bytes, assembled instead of copied
  fixup_us, classify_us   rhp_fixup_sessions and rhp_classify_sessions over the
               same round, for scale
  out_bytes, reply_GBps, writer_GBps   bytes written to `out` and per second
The reply bytes are compared with the writer's before anything is timed.
usage: python tools/bench_reply.py [--out profiles/reply/bench_reply.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

import libreactorng_amd as rhp  # noqa: E402

TFB = (b"GET /plaintext HTTP/1.1\r\nHost: tfb-server:8080\r\nAccept: text/plain\r\n"
       b"Connection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n\r\n")
ROUNDS = ((64, 64), (256, 256), (4096, 1), (65536, 1), (16384, 64))
ROUTES = ((b"GET", b"/plaintext"),)


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


def bench_round(sessions, per, reps, warmup):
    import torch
    n = sessions * per
    buf = np.zeros(n * len(TFB) + rhp.RHP_PAD, dtype=np.uint8)
    buf[: n * len(TFB)] = np.tile(np.frombuffer(TFB, dtype=np.uint8), n)
    off = (np.arange(n + 1, dtype=np.uint64) * len(TFB)).astype(np.uint64)
    sess = np.zeros(sessions, dtype=rhp.SESSION_DTYPE)
    sess["piece_lo"] = np.arange(sessions) * per
    sess["piece_hi"] = sess["piece_lo"] + per
    db = rhp.DeviceBatch(buf, off, 16, rhp.MODE_HTTP, flags=rhp.BATCH_SPECULATIVE)
    ds = torch.from_numpy(sess.view(np.uint8).copy()).to("cuda")
    dres = torch.zeros(sessions * rhp.SESSION_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    droute = torch.zeros(n, dtype=torch.int16, device="cuda")
    *_keep, c = rhp._classify_desc((), ROUTES, None, droute.data_ptr())
    one = rhp.DeviceResponses(*rhp.make_responses(1, 1, "plaintext"))       # the reply image of the route
    writer = rhp.DeviceResponses(*rhp.make_responses(n, 1, "plaintext"))    # the yardstick: n records
    out_bytes = writer.out_size
    out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
    replies = torch.zeros(sessions * rhp.SESSION_REPLY_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    total = torch.zeros(1, dtype=torch.int64, device="cuda")
    work = torch.zeros(rhp.reply_work_words(n, sessions), dtype=torch.int64, device="cuda")
    t = rhp.reply_table(one.out, one.out_off, 1)
    o = rhp.ReplyOut(replies.data_ptr(), total.data_ptr(), out.data_ptr(), out_bytes, work.data_ptr())
    d = db.desc()
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    L = rhp.lib()

    def check(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed: {rc}")

    fixup = lambda: check(L.rhp_fixup_sessions(ctypes.byref(d), vp(ds.data_ptr()), sessions, vp(dres.data_ptr()),
                                               vp(dst.data_ptr()), stream), "rhp_fixup_sessions")
    classify = lambda: check(L.rhp_classify_sessions(ctypes.byref(d), vp(ds.data_ptr()), sessions, vp(dres.data_ptr()),
                                                     vp(dst.data_ptr()), ctypes.byref(c), stream), "rhp_classify_sessions")
    reply = lambda: check(L.rhp_reply_sessions(ctypes.byref(d), vp(ds.data_ptr()), sessions, vp(dres.data_ptr()),
                                               vp(droute.data_ptr()), ctypes.byref(t), ctypes.byref(o), stream), "rhp_reply_sessions")
    db.launch()
    fixup()
    classify()
    one.launch()
    writer.launch()
    reply()
    torch.cuda.synchronize()
    assert int(total.item()) == out_bytes, (int(total.item()), out_bytes)
    assert torch.equal(out, writer.out[:out_bytes]), "the reply bytes differ from the writer's"
    r = {"sessions": sessions, "per_session": per, "slots": n, "out_bytes": out_bytes, "reps": reps,
         "reply_us": median_us(reply, reps, warmup), "writer_us": median_us(writer.launch, reps, warmup),
         "fixup_us": median_us(fixup, reps, warmup), "classify_us": median_us(classify, reps, warmup)}
    r["reply_over_writer"] = r["reply_us"] / r["writer_us"]
    r["reply_GBps"] = out_bytes / r["reply_us"] / 1e3
    r["writer_GBps"] = out_bytes / r["writer_us"] / 1e3
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_reply needs a GPU"
    lines = []
    for sessions, per in ROUNDS:
        r = bench_round(sessions, per, a.reps, a.warmup)
        r["library_sha256"] = rhp.library_sha256()
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
