#!/usr/bin/env python3
"""Times rhp_walk_resume (include/rhp.h) over tools/bench_walk.py's workload delivered in two rounds, in one process
on one GPU.

The input: --sessions keep-alive connections (64K) that each hold --depth (4) pipelined Content-Length responses of
--size (256) bytes.  Round 1 delivers every session's bytes up to a cut inside the third response's body, round 2
the rest: round 1 ends every session with RHP_WALK_BODY and a state IN_LENGTH, round 2 starts with a continuation
slot and ends with RHP_WALK_END.  RHP_WALK_TRAILERS, max_headers 8, depth slots per session and round.

Timed, a HIP event pair around each of --reps calls after --warmup, medians and minima:
  round1_us, round2_us   rhp_walk_resume; the states are reset (a device copy outside the events) before each call
  walk_us                rhp_walk_responses over the round-1 input: what the walk costs with no state to carry
  host_us                rhp_cpu_walk_resume, both rounds, the sessions cut into --threads ranges (16), wall time
The kernel's results, slots, message records and states are compared with the host twin's before anything is timed.
Not timed here: chunked bodies, de-framing, few long sessions.
usage: python tools/bench_walk_resume.py [--out profiles/walk/bench_walk_resume.jsonl]
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
    assert torch.cuda.is_available(), "bench_walk_resume needs the GPU: there is no other way to take its times"
    ns, depth, size = args.sessions, args.depth, args.size
    nt = ns * depth
    pool = [response(size, i) for i in range(1024)]
    cut = 2 * size + size - 40   # inside the third response's body
    assert depth >= 3 and all(x.index(b"\r\n\r\n") + 4 < size - 40 for x in pool)
    whole = [b"".join(pool[(s * depth + k) % len(pool)] for k in range(depth)) for s in range(ns)]
    flags = rhp.WALK_TRAILERS
    slot_off = np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth)

    def packed(parts, n):
        data = b"".join(parts)
        buf = np.zeros(len(data) + rhp.RHP_PAD, dtype=np.uint8)
        buf[: len(data)] = np.frombuffer(data, dtype=np.uint8)
        return buf, np.arange(ns + 1, dtype=np.uint64) * np.uint64(n)

    rounds = [packed([x[:cut] for x in whole], cut), packed([x[cut:] for x in whole], depth * size - cut)]

    # the host twin, --threads ranges of sessions at once, both rounds
    recs = lambda: [np.full(k, rhp.WALK_POISON, dtype=np.uint8) for k in (16 * nt, 8 * nt * MAXH, 32 * nt, 16 * ns)]
    host_out = [recs(), recs()]
    hstates = np.zeros(32 * ns, dtype=np.uint8)
    cuts = [ns * t // args.threads for t in range(args.threads + 1)]
    fn = rhp.host().rhp_cpu_walk_resume

    def batches(r):
        buf, so = rounds[r]
        msgs, hdrs, slots, res = host_out[r]
        return [(rhp.WalkBatch(buf.ctypes.data, None, buf.size, so.ctypes.data + 8 * lo, slot_off.ctypes.data + 8 * lo, hi - lo, nt, MAXH,
                               flags, msgs.ctypes.data, hdrs.ctypes.data, slots.ctypes.data, res.ctypes.data + 16 * lo),
                 hstates.ctypes.data + 32 * lo) for lo, hi in zip(cuts[:-1], cuts[1:]) if hi > lo]

    work = [batches(0), batches(1)]
    host_t, states_after = [], []
    with ThreadPoolExecutor(args.threads) as ex:
        for _ in range(args.host_reps + 1):
            hstates[:] = 0
            states_after.clear()
            t0 = time.perf_counter()
            for r in (0, 1):
                rcs = list(ex.map(lambda b: fn(ctypes.byref(b[0]), b[1]), work[r]))
                assert not any(rcs)
                states_after.append(hstates.copy())   # (a 2 MB copy inside the timed span)
            host_t.append((time.perf_counter() - t0) * 1e6)
    host_t = host_t[1:]
    want = [rhp._walk_result(host_out[r][3], host_out[r][2], host_out[r][0], host_out[r][1], None, ns, nt, MAXH) for r in (0, 1)]
    assert (want[0][0]["stop"] == rhp.WALK_BODY).all() and (want[0][0]["n_slots"] == 3).all() and (want[0][0]["consumed"] == cut).all()
    assert (want[1][0]["stop"] == rhp.WALK_END).all() and (want[1][0]["n_slots"] == depth - 2).all()
    assert (states_after[0].view(rhp.WALK_STATE_DTYPE)["phase"] == rhp.WALK_IN_LENGTH).all() and not states_after[1].any()

    dev = lambda a: torch.from_numpy(a).to("cuda")
    dsl = dev(slot_off.view(np.int64))
    dbytes = [dev(rounds[r][0]) for r in (0, 1)]
    dso = [dev(rounds[r][1].view(np.int64)) for r in (0, 1)]
    dm, dh, ds, dr = (torch.full((k,), rhp.WALK_POISON, dtype=torch.uint8, device="cuda") for k in (16 * nt, 8 * nt * MAXH, 32 * nt, 16 * ns))
    dstates = torch.zeros(32 * ns, dtype=torch.uint8, device="cuda")
    entry = [torch.zeros(32 * ns, dtype=torch.uint8, device="cuda"), dev(states_after[0])]   # the states each round starts from
    resume = lambda r: rhp.walk_resume_device(dbytes[r], rounds[r][0].size, dso[r], dsl, ns, nt, MAXH, flags, dm, dh, ds, dr, dstates)
    walk = lambda: rhp.walk_responses_device(dbytes[0], rounds[0][0].size, dso[0], dsl, ns, nt, MAXH, flags, dm, dh, ds, dr)
    for r in (0, 1):   # the kernel against the twin, the states carried on the device
        for t in (dm, dh, ds, dr):
            t.fill_(rhp.WALK_POISON)   # (the twin's records of a round start from poison too)
        resume(r)
        torch.cuda.synchronize()
        got = rhp._walk_result(dr.cpu().numpy(), ds.cpu().numpy(), dm.cpu().numpy(), dh.cpu().numpy(), None, ns, nt, MAXH)
        assert all((g == w).all() for g, w in zip(got[:2], want[r][:2])), f"round {r + 1}: the kernel's results or slots differ from the host twin's"
        assert (got[2]["ret"] == want[r][2]["ret"]).all() and (dstates.cpu().numpy() == states_after[r]).all(), f"round {r + 1}: records or states differ"

    def timed(call, before=None):
        for _ in range(args.warmup):
            if before:
                before()
            call()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            if before:
                before()
            a.record()
            call()
            b.record()
        torch.cuda.synchronize()
        return [a.elapsed_time(b) * 1e3 for a, b in ev]

    t1 = timed(lambda: resume(0), lambda: dstates.copy_(entry[0]))
    t2 = timed(lambda: resume(1), lambda: dstates.copy_(entry[1]))
    tw = timed(walk)
    med = lambda x: round(float(np.median(x)), 2)
    line = dict(bench="walk_resume", sessions=ns, depth=depth, response_bytes=size, cut=cut, max_headers=MAXH, flags=flags,
                reps=args.reps, warmup=args.warmup, host_threads=args.threads, host_reps=args.host_reps,
                round1_us=med(t1), round1_min=round(min(t1), 2), round2_us=med(t2), round2_min=round(min(t2), 2),
                walk_us=med(tw), walk_min=round(min(tw), 2), round1_over_walk=round(float(np.median(t1) / np.median(tw)), 3),
                host_us=med(host_t), host_min=round(min(host_t), 2),
                host_over_kernel=round(float(np.median(host_t) / (np.median(t1) + np.median(t2))), 2),
                not_measured="chunked bodies, de-framing, few long sessions", library_sha256=rhp.library_sha256())
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
