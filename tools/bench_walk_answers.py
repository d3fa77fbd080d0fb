#!/usr/bin/env python3
"""Times rhp_walk_answers (include/rhp.h) against rhp_walk_responses, the walk
it runs, in one process on one GPU.

The input is tools/bench_walk.py's: --sessions keep-alive connections (64K) that
each hold --depth (4) pipelined responses of --size (256) bytes, every session
with depth slots and a queue of depth outstanding requests, the queues packed
back to back (eight sessions to a word of head_bits).  Three calls are timed, a
HIP event pair around each of --reps calls after --warmup:
  walk     rhp_walk_responses: the yardstick, in the same run
  clear    rhp_walk_answers with every bit clear: the same bytes, the same
           slots; its answers are compared with the walk's before anything is
           timed, byte for byte
  heads    rhp_walk_answers with one request in four a HEAD (request (s + k) % 4
           == 0 of session s): that reply is its head alone, so these sessions
           are a body shorter; answered and the HEAD slots are checked first
One JSON line: median and min of each, the spread of the walk's own samples
(max - min and the interquartile range), and the two ratios to the walk.
usage: python tools/bench_walk_answers.py [--out profiles/walk/bench_walk_answers.jsonl]
"""
import argparse
import json
import os
import sys

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
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_walk_answers needs the GPU: there is no other way to take its times"
    ns, depth = args.sessions, args.depth
    nt = ns * depth
    flags = rhp.WALK_TRAILERS
    pool = [response(args.size, i) for i in range(1024)]
    heads_of = [p[: p.index(b"\r\n\r\n") + 4] for p in pool]
    is_head = np.array([[(s + k) % 4 == 0 for k in range(depth)] for s in range(ns)], dtype=bool)

    def pack(head_mask):
        parts, lens = [], np.zeros(ns, dtype=np.uint64)
        for s in range(ns):
            x = b"".join((heads_of if head_mask[s, k] else pool)[(s * depth + k) % len(pool)] for k in range(depth))
            parts.append(x)
            lens[s] = len(x)
        data = b"".join(parts)
        buf = np.zeros(len(data) + rhp.RHP_PAD, dtype=np.uint8)
        buf[: len(data)] = np.frombuffer(data, dtype=np.uint8)
        return buf, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), len(data)

    slot_off = np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth)
    req_off = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth)).astype(np.uint32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")
    dsl, dq = dev(slot_off), dev(req_off)
    outs = lambda: tuple(torch.full((k,), rhp.WALK_POISON, dtype=torch.uint8, device="cuda")
                         for k in (16 * nt, 8 * nt * MAXH, 32 * nt, 16 * ns, 4 * ns, 4 * nt))

    buf0, so0, bytes0 = pack(np.zeros_like(is_head))
    buf1, so1, bytes1 = pack(is_head)
    db0, dso0, db1, dso1 = dev(buf0), dev(so0), dev(buf1), dev(so1)
    bits0, bits1 = dev(rhp.head_bits_of(np.zeros(nt, dtype=bool))), dev(rhp.head_bits_of(is_head.reshape(-1)))
    m0, h0, s0, r0, _, _ = outs()
    m1, h1, s1, r1, a1, q1 = outs()
    m2, h2, s2, r2, a2, q2 = outs()
    calls = dict(
        walk=lambda: rhp.walk_responses_device(db0, buf0.size, dso0, dsl, ns, nt, MAXH, flags, m0, h0, s0, r0),
        clear=lambda: rhp.walk_answers_device(db0, buf0.size, dso0, dsl, ns, nt, MAXH, flags, m1, h1, s1, r1, None, dq, bits0, nt, a1, q1),
        heads=lambda: rhp.walk_answers_device(db1, buf1.size, dso1, dsl, ns, nt, MAXH, flags, m2, h2, s2, r2, None, dq, bits1, nt, a2, q2))
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    for a, b in ((m0, m1), (h0, h1), (s0, s1), (r0, r1)):
        assert torch.equal(a, b), "with every bit clear the call leaves what rhp_walk_responses leaves"
    u32 = lambda t: t.cpu().numpy().view(np.uint32)
    assert (u32(a1) == depth).all() and (u32(a2) == depth).all() and (u32(q1).reshape(ns, depth) == np.arange(depth)).all()
    res2, slots2 = r2.cpu().numpy().view(rhp.WALK_RESULT_DTYPE), s2.cpu().numpy().view(rhp.WALK_SLOT_DTYPE).reshape(ns, depth)
    assert (res2["stop"] == rhp.WALK_END).all() and (res2["n_slots"] == depth).all() and (res2["consumed"] == np.diff(so1)).all()
    assert (slots2["wire_len"][is_head] == 0).all() and (slots2["wire_len"][~is_head] > 0).all() and (slots2["body_kind"] == rhp.FRAME_LENGTH).all()

    times = {}
    for name, fn in calls.items():
        for _ in range(args.warmup):
            fn()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
        for a, b in ev:
            a.record()
            fn()
            b.record()
        torch.cuda.synchronize()
        times[name] = [a.elapsed_time(b) * 1e3 for a, b in ev]
    med = lambda x: round(float(np.median(x)), 2)
    w = times["walk"]
    line = dict(bench="walk_answers", sessions=ns, depth=depth, response_bytes=args.size, max_headers=MAXH, flags=flags,
                reps=args.reps, warmup=args.warmup, head_share=round(float(is_head.mean()), 3), bytes_walk=bytes0, bytes_heads=bytes1)
    for name, t in times.items():
        line[f"{name}_us"], line[f"{name}_min"] = med(t), round(min(t), 2)
    line.update(walk_spread_us=round(max(w) - min(w), 2), walk_iqr_us=round(float(np.percentile(w, 75) - np.percentile(w, 25)), 2),
                clear_over_walk=round(float(np.median(times["clear"]) / np.median(w)), 3),
                heads_over_walk=round(float(np.median(times["heads"]) / np.median(w)), 3), library_sha256=rhp.library_sha256())
    print(json.dumps(line), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
