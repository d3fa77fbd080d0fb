#!/usr/bin/env python3
"""Times rhp_lookup_walked (include/rhp.h) against its host twin,
rhp_cpu_lookup_walked on --threads host threads (16), and beside the walk
kernel over the same input, in one process on one GPU.

The input is tools/bench_walk.py's: --sessions keep-alive connections (64K) that
each hold --depth (4) pipelined responses of --size (256) bytes: a status line,
four header lines (Server, Content-Type, X-Request-Id, Content-Length) and the
body; max_headers 8.  It is walked once, outside the timing, on the device and
on the host; the lookup then runs over the records as they lie.  Two name
lists: 2 names (Connection, which no response has, and Content-Type) and 16.

The kernels: a HIP event pair around each of --reps calls after --warmup,
median, for rhp_lookup_walked and for rhp_walk_responses.  The host: the
sessions cut into --threads equal ranges, each a batch of its own (its slots
renumbered from 0, its own fields), one rhp_cpu_lookup_walked call per range on
a thread of its own (ctypes releases the GIL), wall time of the round, median of
--host-reps.  The kernel's fields are compared with the host's before anything
is timed.  One JSON line per name list:
  kernel_us, host_us, walk_us   medians (and *_min)
  host_over_kernel = host_us / kernel_us   lookup_over_walk = kernel_us / walk_us
  fields_bytes                  what goes back to the host: 4 * n_names * n_slots_total
Not timed here: few long sessions, chunked bodies, a profile of the kernel.
usage: python tools/bench_lookup_walked.py [--out profiles/walk/bench_lookup_walked.jsonl]
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
sys.path.insert(0, HERE)

import libreactorng_amd as rhp  # noqa: E402
from bench_walk import MAXH, response  # noqa: E402

NAMES2 = (b"Connection", b"Content-Type")
NAMES16 = NAMES2 + (b"Content-Length", b"Server", b"X-Request-Id", b"Set-Cookie", b"Location", b"Transfer-Encoding", b"Cache-Control",
                    b"ETag", b"Date", b"Vary", b"Content-Encoding", b"Last-Modified", b"Age", b"Via")


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
    assert torch.cuda.is_available(), "bench_lookup_walked needs the GPU: there is no other way to take its times"
    ns, depth = args.sessions, args.depth
    nt = ns * depth
    pool = [response(args.size, i) for i in range(1024)]
    data = b"".join(pool[(s * depth + k) % len(pool)] for s in range(ns) for k in range(depth))
    buf = np.zeros(len(data) + rhp.RHP_PAD, dtype=np.uint8)
    buf[: len(data)] = np.frombuffer(data, dtype=np.uint8)
    sess_off = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth * args.size))
    slot_off = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth))
    flags = rhp.WALK_TRAILERS

    # walked once on the host: the records the twin looks up
    res, slots, msgs, hdrs, _ = rhp.walk_responses_cpu(buf, sess_off, slot_off, MAXH, flags)
    assert (res["n_slots"] == depth).all() and (res["stop"] == rhp.WALK_END).all()
    res, slots, msgs, hdrs = (np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (res, slots, msgs, hdrs))

    # ... and on the device, where they stay
    dbytes = torch.from_numpy(buf).to("cuda")
    dso = torch.from_numpy(sess_off.view(np.int64)).to("cuda")
    dsl = torch.from_numpy(slot_off.view(np.int64)).to("cuda")
    dm, dh, ds, dr = (torch.full((k,), rhp.WALK_POISON, dtype=torch.uint8, device="cuda") for k in (16 * nt, 8 * nt * MAXH, 32 * nt, 16 * ns))
    walk = lambda: rhp.walk_responses_device(dbytes, buf.size, dso, dsl, ns, nt, MAXH, flags, dm, dh, ds, dr)
    walk()
    torch.cuda.synchronize()

    def timed(call):
        for _ in range(args.warmup):
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in ev]

    med = lambda x: round(float(np.median(x)), 2)
    tw = timed(walk)
    cuts = [ns * t // args.threads for t in range(args.threads + 1)]
    ranges = [(lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]
    local_slot_off = [np.arange(hi - lo + 1, dtype=np.uint64) * np.uint64(depth) for lo, hi in ranges]
    fn = rhp.host().rhp_cpu_lookup_walked
    lines = []
    for names in (NAMES2, NAMES16):
        nn = len(names)
        text, nm, _ = rhp.classify_tables(names)
        # the host twin, --threads ranges of sessions at once, each a batch of its own
        hfields = [np.full(4 * nn * (hi - lo) * depth, rhp.LOOKUP_POISON, dtype=np.uint8) for lo, hi in ranges]
        calls = []
        for (lo, hi), sl, hf in zip(ranges, local_slot_off, hfields):
            s0 = lo * depth
            w = rhp.WalkBatch(buf.ctypes.data, None, buf.size, sess_off.ctypes.data + 8 * lo, sl.ctypes.data, hi - lo, (hi - lo) * depth,
                              MAXH, flags, msgs.ctypes.data + 16 * s0, hdrs.ctypes.data + 8 * MAXH * s0, slots.ctypes.data + 32 * s0,
                              res.ctypes.data + 16 * lo)
            calls.append((w, rhp.WalkLookup(text.ctypes.data, nm.ctypes.data, nn, 0, hf.ctypes.data)))
        host_t = []
        with ThreadPoolExecutor(args.threads) as ex:
            for _ in range(args.host_reps + 1):
                t0 = time.perf_counter()
                rcs = list(ex.map(lambda c: fn(ctypes.byref(c[0]), ctypes.byref(c[1])), calls))
                host_t.append((time.perf_counter() - t0) * 1e6)
                assert not any(rcs)
        host_t = host_t[1:]
        want = np.concatenate([hf.view(rhp.FIELDREF_DTYPE).reshape(nn, -1) for hf in hfields], axis=1)

        df = torch.full((4 * nn * nt,), rhp.LOOKUP_POISON, dtype=torch.uint8, device="cuda")
        lookup = lambda: rhp.lookup_walked_device(dbytes, buf.size, dso, dsl, ns, nt, MAXH, flags, dm, dh, ds, dr, names, df)
        lookup()
        torch.cuda.synchronize()
        got = df.cpu().numpy().view(rhp.FIELDREF_DTYPE).reshape(nn, nt)
        assert (got == want).all(), "the kernel's fields differ from the host twin's"
        present = int((want["value_off"] != rhp.RHP_NAME_NULL).sum())
        tk = timed(lookup)
        line = dict(bench="lookup_walked", n_names=nn, sessions=ns, depth=depth, response_bytes=args.size, max_headers=MAXH,
                    n_slots_total=nt, fields_present=present, reps=args.reps, warmup=args.warmup, host_threads=args.threads,
                    host_reps=args.host_reps, kernel_us=med(tk), kernel_min=round(min(tk), 2), host_us=med(host_t),
                    host_min=round(min(host_t), 2), walk_us=med(tw), walk_min=round(min(tw), 2),
                    host_over_kernel=round(float(np.median(host_t) / np.median(tk)), 2),
                    lookup_over_walk=round(float(np.median(tk) / np.median(tw)), 3), fields_bytes=4 * nn * nt,
                    library_sha256=rhp.library_sha256())
        print(json.dumps(line), flush=True)
        lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
