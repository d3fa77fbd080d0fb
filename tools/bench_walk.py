#!/usr/bin/env python3
"""Times rhp_walk_responses (include/rhp.h) against its host twin,
rhp_cpu_walk_responses on --threads host threads (16), in one process on one GPU.

The input: --sessions keep-alive connections (64K) that each hold --depth (4)
pipelined responses of --size (256) bytes: a status line, four header lines with
Content-Length the last, and the body.  Every session owns depth slots, so every
walk ends with RHP_WALK_END after depth messages.  This is the wide shape, many
short sessions; few long sessions, where a lane per session leaves most of a
wave idle, are not timed here.

The kernel: a HIP event pair around each of --reps calls after --warmup, median.
The host: the sessions cut into --threads equal ranges, one rhp_cpu_walk_responses
call per range on a thread of its own (ctypes releases the GIL), wall time of the
round, median of --host-reps.  The kernel's results, slots and message records
are compared with the host's before anything is timed.  One JSON line:
  kernel_us, host_us   medians (and *_min); ratio = host_us / kernel_us
  gbytes_per_s         the sessions' bytes over kernel_us
usage: python tools/bench_walk.py [--out profiles/walk/bench_walk.jsonl]
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

MAXH = 8


def response(size: int, i: int) -> bytes:
    head = lambda n: (b"HTTP/1.1 200 OK\r\nServer: bench\r\nContent-Type: text/plain\r\nX-Request-Id: %08d\r\nContent-Length: %d\r\n\r\n"
                      % (i % 10 ** 8, n))
    n = size - len(head(size))
    while len(head(n)) + n != size:   # (the length's digits move the head by a byte)
        n = size - len(head(n))
    return head(n) + bytes(97 + (i + k) % 26 for k in range(n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", type=int, default=1 << 16)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_walk needs the GPU: there is no other way to take its times"
    ns, depth = args.sessions, args.depth
    nt = ns * depth
    pool = [response(args.size, i) for i in range(1024)]
    data = b"".join(pool[(s * depth + k) % len(pool)] for s in range(ns) for k in range(depth))
    buf = np.zeros(len(data) + rhp.RHP_PAD, dtype=np.uint8)
    buf[: len(data)] = np.frombuffer(data, dtype=np.uint8)
    sess_off = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth * args.size))
    slot_off = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth))
    flags = rhp.WALK_TRAILERS

    # the host twin, --threads ranges of sessions at once
    msgs = np.full(16 * nt, rhp.WALK_POISON, dtype=np.uint8)
    hdrs = np.full(8 * nt * MAXH, rhp.WALK_POISON, dtype=np.uint8)
    slots = np.full(32 * nt, rhp.WALK_POISON, dtype=np.uint8)
    res = np.full(16 * ns, rhp.WALK_POISON, dtype=np.uint8)
    cuts = [ns * t // args.threads for t in range(args.threads + 1)]
    batches = [rhp.WalkBatch(buf.ctypes.data, None, buf.size, sess_off.ctypes.data + 8 * lo, slot_off.ctypes.data + 8 * lo, hi - lo,
                             nt, MAXH, flags, msgs.ctypes.data, hdrs.ctypes.data, slots.ctypes.data, res.ctypes.data + 16 * lo)
               for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
    fn = rhp.host().rhp_cpu_walk_responses
    host_t = []
    with ThreadPoolExecutor(args.threads) as ex:
        for _ in range(args.host_reps + 1):
            t0 = time.perf_counter()
            rcs = list(ex.map(lambda b: fn(ctypes.byref(b)), batches))
            host_t.append((time.perf_counter() - t0) * 1e6)
            assert not any(rcs)
    host_t = host_t[1:]
    want = rhp._walk_result(res, slots, msgs, hdrs, None, ns, nt, MAXH)
    assert (want[0]["n_slots"] == depth).all() and (want[0]["stop"] == rhp.WALK_END).all() and (want[0]["consumed"] == depth * args.size).all()

    dbytes = torch.from_numpy(buf).to("cuda")
    dso = torch.from_numpy(sess_off.view(np.int64)).to("cuda")
    dsl = torch.from_numpy(slot_off.view(np.int64)).to("cuda")
    dm, dh, ds, dr = (torch.full((k,), rhp.WALK_POISON, dtype=torch.uint8, device="cuda") for k in (16 * nt, 8 * nt * MAXH, 32 * nt, 16 * ns))
    walk = lambda: rhp.walk_responses_device(dbytes, buf.size, dso, dsl, ns, nt, MAXH, flags, dm, dh, ds, dr)
    walk()
    torch.cuda.synchronize()
    got = rhp._walk_result(dr.cpu().numpy(), ds.cpu().numpy(), dm.cpu().numpy(), dh.cpu().numpy(), None, ns, nt, MAXH)
    assert all((g == w).all() for g, w in zip(got[:3], want[:3])), "the kernel's results, slots or message records differ from the host twin's"
    for _ in range(args.warmup):
        walk()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
    for a, b in ev:
        a.record()
        walk()
        b.record()
    torch.cuda.synchronize()
    tk = [a.elapsed_time(b) * 1e3 for a, b in ev]
    med = lambda x: round(float(np.median(x)), 2)
    line = dict(bench="walk_responses", sessions=ns, depth=depth, response_bytes=args.size, max_headers=MAXH, flags=flags,
                reps=args.reps, warmup=args.warmup, host_threads=args.threads, host_reps=args.host_reps,
                kernel_us=med(tk), kernel_min=round(min(tk), 2), host_us=med(host_t), host_min=round(min(host_t), 2),
                ratio=round(float(np.median(host_t) / np.median(tk)), 2),
                gbytes_per_s=round(len(data) / (float(np.median(tk)) * 1e-6) / 1e9, 1), library_sha256=rhp.library_sha256())
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
