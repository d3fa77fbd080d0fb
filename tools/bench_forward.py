#!/usr/bin/env python3
"""Times rhp_forward_sessions (include/rhp.h) behind the parse, the fix-up and the
classify, and its host twin rhp_cpu_forward_sessions on --threads host threads
(16), in one process on one GPU.

The input is DESIGN 3.5's: --sessions keep-alive connections (64K) that each
hold --depth (4) pipelined TFB-style GETs ("get"), and the same with POSTs that
carry a --size (256) byte Content-Length body ("post"), cut at every empty line.
Every request matches the one route, which is forwarded; Connection and
Keep-Alive are dropped and one Via line is added.  Parse, fix-up and classify
run once, outside the timing, on the device and on the host; the forward then
runs over the records as they lie, and its output is compared with the twin's
before anything is timed.

A HIP event pair around each of --reps calls after --warmup; the host: the
sessions cut into --threads ranges, each a batch of its own, wall time of the
round, median of --host-reps.  One JSON line per workload:
  forward_us, host_us          medians (and *_min, *_max)
  bytes_read, bytes_written    of the forward: records, request heads and bodies in; requests, out_off, why, fwd_off
                               and head_bits out (work not counted)
  hbm_share                    (bytes_read + bytes_written) / forward_us over --hbm-gbs (8000)
usage: python tools/bench_forward.py [--out profiles/forward/bench_forward.jsonl]
"""
import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import libreactorng_amd as rhp  # noqa: E402

MAXH = 16
ROUTES = ((b"", b"/plaintext"),)
DROP = (b"Connection", b"Keep-Alive")
EXTRA = b"Via: 1.1 rhp\r\n"
HEADERS = b"Host: tfb-server:8080\r\nAccept: text/plain\r\nConnection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n"


def request(kind: str, size: int, i: int) -> bytes:
    if kind == "get":
        return b"GET /plaintext HTTP/1.1\r\n" + HEADERS + b"X-Request-Id: %08d\r\n\r\n" % i
    body = bytes(0x61 + (i + k) % 26 for k in range(size))
    return b"POST /plaintext HTTP/1.1\r\n" + HEADERS + b"Content-Length: %d\r\n\r\n" % size + body


def stats(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1 << 16)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_forward needs the GPU: there is no other way to take its times"
    ns, depth = args.sessions, args.depth
    vp = ctypes.c_void_p
    lines = []
    for kind in ("get", "post"):
        pool = [request(kind, args.size, i) for i in range(1024)]
        sessions = [b"".join(pool[(s * depth + k) % len(pool)] for k in range(depth)) for s in range(ns)]
        buf, off, sess, _ = rhp.pack_sessions(sessions)
        n = len(off) - 1

        # the round on the host: the twin's records
        res, results, starts = rhp.fixup_cpu(buf, off, sess, MAXH)
        _, route = rhp.classify_sessions_cpu(res, sess, results, starts, (), ROUTES)
        assert (results["n_slots"] == depth).all()

        # the round on the device, where the records stay
        db = rhp.DeviceBatch(buf, off, MAXH, rhp.MODE_HTTP, flags=rhp.BATCH_SPECULATIVE)
        ds = torch.from_numpy(sess.view(np.uint8).copy()).to("cuda")
        dres = torch.zeros(ns * rhp.SESSION_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        dst = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
        droute = torch.zeros(n * 2, dtype=torch.uint8, device="cuda")
        *_keep, c = rhp._classify_desc((), ROUTES, None, droute.data_ptr())
        stream = vp(torch.cuda.current_stream().cuda_stream)
        db.launch()
        d = db.desc()
        assert rhp.lib().rhp_fixup_sessions(ctypes.byref(d), vp(ds.data_ptr()), ns, vp(dres.data_ptr()), vp(dst.data_ptr()), stream) == 0
        assert rhp.lib().rhp_classify_sessions(ctypes.byref(d), vp(ds.data_ptr()), ns, vp(dres.data_ptr()), vp(dst.data_ptr()),
                                               ctypes.byref(c), stream) == 0
        torch.cuda.synchronize()

        # the forward: sizes first, then an out of exactly their sum
        doff = torch.zeros(8 * (n + 1), dtype=torch.uint8, device="cuda")
        dwhy = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
        dfwd = torch.zeros(4 * (ns + 1), dtype=torch.uint8, device="cuda")
        dbits = torch.zeros(4 * ((n + 31) // 32), dtype=torch.uint8, device="cuda")
        dwork = torch.zeros(8 * rhp.forward_work_words(n, ns), dtype=torch.uint8, device="cuda")
        call = lambda out, size: rhp.forward_sessions_device(d, ds, ns, dres, dst, droute, len(ROUTES), 1, DROP, EXTRA, doff, dwhy, out, size,
                                                             dfwd, dbits, dwork)
        call(None, 0)
        torch.cuda.synchronize()
        total = int(doff.cpu().numpy().view(np.uint64)[n])
        dout = torch.zeros(total, dtype=torch.uint8, device="cuda")
        call(dout, total)
        torch.cuda.synchronize()
        got = dout.cpu().numpy()
        why = dwhy.cpu().numpy().view(np.uint32)
        assert int((why == 0).sum()) == ns * depth and int(dfwd.cpu().numpy().view(np.uint32)[ns]) == ns * depth

        # the host twin, --threads ranges of sessions at once, each a batch of its own over the same bytes
        text, nm, _ = rhp.classify_tables(DROP)
        raw_reqs, raw_hdrs, raw_http = res.raw_reqs, res.raw_hdrs, res.raw_http
        bytes_host = res.bytes_out
        cuts = [ns * t // args.threads for t in range(args.threads + 1)]
        calls, houts = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if hi == lo:
                continue
            s0, s1 = int(sess["piece_lo"][lo]), int(sess["piece_hi"][hi - 1])
            k = s1 - s0
            sub = sess[lo:hi].copy()
            sub["piece_lo"] -= s0
            sub["piece_hi"] -= s0
            o_off, o_why = np.zeros(k + 1, dtype=np.uint64), np.zeros(k, dtype=np.uint32)
            o_fwd, o_bits = np.zeros(hi - lo + 1, dtype=np.uint32), np.zeros((k + 31) // 32, dtype=np.uint32)
            work = np.zeros(rhp.forward_work_words(k, hi - lo), dtype=np.uint64)
            size = -(-total * (hi - lo) // ns) + 4096   # (an upper bound: the sessions are alike)
            out = np.zeros(size, dtype=np.uint8)
            b = rhp.Batch(rhp._ptr(bytes_host), rhp._ptr(bytes_host), off[s0:].ctypes.data, bytes_host.size, k, MAXH, rhp.MODE_HTTP,
                          rhp.LAYOUT_REQUEST_MAJOR, raw_reqs[16 * s0:].ctypes.data, raw_hdrs[8 * MAXH * s0:].ctypes.data,
                          raw_http[24 * s0:].ctypes.data, None, rhp.BATCH_SPECULATIVE, 0, None)
            f = rhp.Forward(len(ROUTES), 1, rhp._ptr(text), rhp._ptr(nm), len(nm), len(EXTRA), EXTRA, rhp._ptr(o_off), rhp._ptr(o_why),
                            rhp._ptr(out), size, rhp._ptr(o_fwd), rhp._ptr(o_bits), rhp._ptr(work))
            args_ = (ctypes.byref(b), rhp._ptr(sub), hi - lo, results[lo:hi].ctypes.data, starts[s0:].ctypes.data, route[s0:].ctypes.data,
                     ctypes.byref(f))
            calls.append((args_, (b, f, sub, work, o_why, o_fwd, o_bits)))   # (every array the call writes stays alive)
            houts.append((o_off, out, k))
        fn = rhp.host().rhp_cpu_forward_sessions
        with ThreadPoolExecutor(args.threads) as ex:
            def host_round():
                t0 = time.perf_counter()
                rcs = list(ex.map(lambda c_: fn(*c_[0]), calls))
                dt = time.perf_counter() - t0
                assert not any(rcs)
                return dt * 1e6
            host_us = [host_round() for _ in range(args.host_reps)]
        twin = np.concatenate([o[: int(oo[k])] for oo, o, k in houts])
        assert twin.size == got.size and (twin == got).all(), "the kernels' bytes are the twin's"

        # the timing: a HIP event pair around each call
        for _ in range(args.warmup):
            call(dout, total)
        torch.cuda.synchronize()
        us = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call(dout, total)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3)
        assert (dout.cpu().numpy() == got).all()

        used = int(results["n_slots"].sum())
        heads = int(res.reqs["ret"][why == 0].sum())
        bodies = int(res.http["body_len"][why == 0].sum()) if kind == "post" else 0
        bytes_read = 8 * ns + 16 * ns + used * (16 + 24 + 8 + 2) + int(res.reqs["num_headers"][why == 0].sum()) * 8 + heads + bodies + 8 * (ns + 1)
        bytes_written = total + 8 * (n + 1) + 4 * n + 4 * (ns + 1) + 4 * ((ns * depth + 31) // 32)
        m, lo_, hi_ = stats(us)
        hm, hlo, hhi = stats(host_us)
        line = {"bench": "forward_sessions", "workload": kind, "sessions": ns, "depth": depth, "slots": n, "forwarded": ns * depth,
                "out_bytes": total, "forward_us": round(m, 1), "forward_us_min": round(lo_, 1), "forward_us_max": round(hi_, 1),
                "host_threads": args.threads, "host_us": round(hm, 1), "host_us_min": round(hlo, 1), "host_us_max": round(hhi, 1),
                "bytes_read": bytes_read, "bytes_written": bytes_written,
                "hbm_share": round((bytes_read + bytes_written) / (m * 1e-6) / (args.hbm_gbs * 1e9), 4), "reps": args.reps, "warmup": args.warmup}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
