#!/usr/bin/env python3
"""Times rhp_relay_walked (include/rhp.h) behind the walk, against
rhp_write_responses producing the same bytes from host-built records, and
against its host twin rhp_cpu_relay_walked on --threads host threads (16), in
one process on one GPU.

The input is tools/bench_walk.py's: --sessions keep-alive connections (64K) that
each hold --depth (4) pipelined responses of --size (256) bytes with a
Content-Length body ("length"), and the same responses with the body as one
chunk, walked with RHP_WALK_DEFRAME ("chunked").  The walk runs once, outside
the timing, on the device and on the host; the relay then runs over the records
as they lie, with the drop names Connection, Keep-Alive, Server and Date.  The
writer's records are built here from the walked records (every response of this
workload keeps X-Request-Id and takes Content-Type's value), and its output is
compared with the relay's, as the relay's is with the twin's, before anything is
timed.

A HIP event pair around each of --reps calls after --warmup; the host: the
sessions cut into --threads ranges, each a batch of its own, wall time of the
round, median of --host-reps.  One JSON line per workload:
  relay_us, writer_us, host_us   medians (and *_min, *_max)
  relay_sizes_us, relay_scan_us, relay_copy_us, writer_sizes_us, ...
                                 the three steps of either device call (sizes with tile sums, the two scan kernels,
                                 the copy kernel), medians (and *_min, *_max) of --reps calls of rhp_relay_walked_steps /
                                 rhp_write_responses_steps: a HIP event between the launches, in a run of its own
  bytes_read, bytes_written      of the relay: records, heads and bodies in, replies and out_off and why out
  hbm_share                      (bytes_read + bytes_written) / relay_us over --hbm-gbs (8000)
Not timed here: few long sessions, large bodies, a profile of the kernels.
usage: python tools/bench_walk_relay.py [--out profiles/walk/bench_walk_relay.jsonl]
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

DROP = (b"Connection", b"Keep-Alive", b"Server", b"Date")


def chunked_response(size: int, i: int) -> bytes:
    """bench_walk's response with its body as one chunk"""
    r = response(size, i)
    head, _, body = r.partition(b"\r\n\r\n")
    head = head[: head.rindex(b"Content-Length")] + b"Transfer-Encoding: chunked"
    return head + b"\r\n\r\n" + b"%x\r\n" % len(body) + body + b"\r\n0\r\n\r\n"


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
    assert torch.cuda.is_available(), "bench_walk_relay needs the GPU: there is no other way to take its times"
    ns, depth = args.sessions, args.depth
    nt = ns * depth
    lines = []
    for kind, make, flags in (("length", response, rhp.WALK_TRAILERS), ("chunked", chunked_response, rhp.WALK_TRAILERS | rhp.WALK_DEFRAME)):
        pool = [make(args.size, i) for i in range(1024)]
        parts = [[pool[(s * depth + k) % len(pool)] for k in range(depth)] for s in range(ns)]
        data = b"".join(b"".join(p) for p in parts)
        buf = np.zeros((len(data) + rhp.RHP_PAD + 15) & ~15, dtype=np.uint8)
        buf[: len(data)] = np.frombuffer(data, dtype=np.uint8)
        sess_off = np.concatenate([[0], np.cumsum([sum(len(x) for x in p) for p in parts])]).astype(np.uint64)
        slot_off = (np.arange(ns + 1, dtype=np.uint64) * np.uint64(depth))

        # walked once on the host (the twin's records and bytes) and on the device, where they stay
        res, slots, msgs, hdrs, walked = rhp.walk_responses_cpu(buf, sess_off, slot_off, MAXH, flags)
        assert (res["n_slots"] == depth).all() and (res["stop"] == rhp.WALK_END).all()
        dbytes = torch.from_numpy(buf).to("cuda")
        dso = torch.from_numpy(sess_off.view(np.int64)).to("cuda")
        dsl = torch.from_numpy(slot_off.view(np.int64)).to("cuda")
        dm, dh, ds, dr = (torch.full((k,), rhp.WALK_POISON, dtype=torch.uint8, device="cuda") for k in (16 * nt, 8 * nt * MAXH, 32 * nt, 16 * ns))
        rhp.walk_responses_device(dbytes, buf.size, dso, dsl, ns, nt, MAXH, flags, dm, dh, ds, dr)
        torch.cuda.synchronize()

        # the relay: sizes first, then an out of exactly their sum
        doff = torch.zeros(8 * (nt + 1), dtype=torch.uint8, device="cuda")
        dwhy = torch.zeros(4 * nt, dtype=torch.uint8, device="cuda")
        dwork = torch.zeros(8 * rhp.relay_work_words(nt), dtype=torch.uint8, device="cuda")
        rhp.relay_walked_device(dbytes, buf.size, dso, dsl, ns, nt, MAXH, flags, dm, dh, ds, dr, DROP, doff, dwhy, None, 0, dwork)
        torch.cuda.synchronize()
        total = int(doff.cpu().numpy().view(np.uint64)[nt])
        dout = torch.zeros(total, dtype=torch.uint8, device="cuda")
        relay = lambda: rhp.relay_walked_device(dbytes, buf.size, dso, dsl, ns, nt, MAXH, flags, dm, dh, ds, dr, DROP, doff, dwhy, dout, total, dwork)
        relay()
        torch.cuda.synchronize()
        got = dout.cpu().numpy()
        assert not dwhy.cpu().numpy().view(np.uint32).any(), "every slot of this workload is relayed"

        # the host twin, --threads ranges of sessions at once, each a batch of its own
        raw = [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in (res, slots, msgs, hdrs)]
        text, nm, _ = rhp.classify_tables(DROP)
        cuts = [ns * t // args.threads for t in range(args.threads + 1)]
        calls, houts = [], []
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            if hi == lo:
                continue
            k, s0 = (hi - lo) * depth, lo * depth
            sl = np.arange(hi - lo + 1, dtype=np.uint64) * np.uint64(depth)
            off, why, work = np.zeros(k + 1, dtype=np.uint64), np.zeros(k, dtype=np.uint32), np.zeros(rhp.relay_work_words(k), dtype=np.uint64)
            out = np.zeros(total, dtype=np.uint8)   # (roomy: a range's share is not known before its first call)
            w = rhp.WalkBatch(walked.ctypes.data, walked.ctypes.data, walked.size, sess_off.ctypes.data + 8 * lo, sl.ctypes.data, hi - lo, k,
                              MAXH, flags, raw[2].ctypes.data + 16 * s0, raw[3].ctypes.data + 8 * MAXH * s0, raw[1].ctypes.data + 32 * s0,
                              raw[0].ctypes.data + 16 * lo)
            r = rhp.WalkRelay(text.ctypes.data, nm.ctypes.data, len(nm), 29, rhp.DEFAULT_DATE, off.ctypes.data, why.ctypes.data,
                              out.ctypes.data, out.size, work.ctypes.data)
            calls.append((w, r, sl, off, why, work))
            houts.append((out, off))
        fn = rhp.host().rhp_cpu_relay_walked
        host_t = []
        with ThreadPoolExecutor(args.threads) as ex:
            for _ in range(args.host_reps + 1):
                t0 = time.perf_counter()
                rcs = list(ex.map(lambda c: fn(ctypes.byref(c[0]), ctypes.byref(c[1])), calls))
                host_t.append((time.perf_counter() - t0) * 1e6)
                assert not any(rcs)
        host_t = host_t[1:]
        want = np.concatenate([out[: int(off[-1])] for out, off in houts])
        assert got.size == want.size and (got == want).all(), "the kernels' replies differ from the host twin's"

        # the writer's records from the walked ones: status "200 OK" behind the bytes, type = Content-Type's value,
        # one field (X-Request-Id), the body
        name_at = lambda k: bytes(walked[int(slots["start"][0]) + int(hdrs[0, k]["name_off"]):][: int(hdrs[0, k]["name_len"])])
        assert name_at(1) == b"Content-Type" and name_at(2) == b"X-Request-Id"
        arena = np.concatenate([walked, np.frombuffer(b"200 OK\0\0", dtype=np.uint8)])
        st = slots["start"].astype(np.uint32)
        resps = np.zeros((nt, 8), dtype=np.uint32)
        resps[:, 0], resps[:, 1] = walked.size, 6
        resps[:, 2], resps[:, 3] = st + hdrs[:, 1]["value_off"], hdrs[:, 1]["value_len"]
        resps[:, 4], resps[:, 5] = st + msgs["ret"].astype(np.uint32), slots["body_len"].astype(np.uint32)
        resps[:, 6], resps[:, 7] = np.arange(nt), 1
        fields = np.stack([st + hdrs[:, 2]["name_off"], hdrs[:, 2]["name_len"].astype(np.uint32), st + hdrs[:, 2]["value_off"],
                           hdrs[:, 2]["value_len"].astype(np.uint32)], axis=1).astype(np.uint32)
        darena, dresps, dfields = (torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to("cuda") for a in (arena, resps, fields))
        woff = torch.zeros(8 * (nt + 1), dtype=torch.uint8, device="cuda")
        wout = torch.zeros(total, dtype=torch.uint8, device="cuda")
        wwork = torch.zeros(8 * ((nt + 4095) // 4096 + 1), dtype=torch.uint8, device="cuda")
        batch = rhp.RespBatch(darena.data_ptr(), dresps.data_ptr(), dfields.data_ptr(), nt, 29, rhp.DEFAULT_DATE, woff.data_ptr(), wout.data_ptr(),
                              total, wwork.data_ptr())
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        writer = lambda: rhp.lib().rhp_write_responses(ctypes.byref(batch), stream)
        assert writer() == 0
        torch.cuda.synchronize()
        assert (wout.cpu().numpy() == got).all(), "the writer's bytes differ from the relay's"

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

        tw, tr = timed(writer), timed(relay)

        # the three steps of either call, from the events the measuring calls record between their launches
        def steps(call):
            for _ in range(args.warmup):
                call()
            got = np.array([call() for _ in range(args.reps)], dtype=np.float64)   # [reps, (sizes, scan, copy)]
            return {k: (round(float(np.median(got[:, j])), 2), round(float(got[:, j].min()), 2), round(float(got[:, j].max()), 2))
                    for j, k in enumerate(("sizes", "scan", "copy"))}

        def writer_steps():
            us = (ctypes.c_float * 3)()
            assert rhp.lib().rhp_write_responses_steps(ctypes.byref(batch), stream, ctypes.byref(us)) == 0
            return tuple(us)

        relay_steps = lambda: rhp.relay_walked_device(dbytes, buf.size, dso, dsl, ns, nt, MAXH, flags, dm, dh, ds, dr, DROP, doff, dwhy, dout, total,
                                                      dwork, steps=True)
        sw, sr = steps(writer_steps), steps(relay_steps)
        step_cols = {}
        for who, st in (("relay", sr), ("writer", sw)):
            for k, (m, lo, hi) in st.items():
                step_cols.update({f"{who}_{k}_us": m, f"{who}_{k}_min": lo, f"{who}_{k}_max": hi})
        stat = lambda name, x: {f"{name}_us": round(float(np.median(x)), 2), f"{name}_min": round(min(x), 2), f"{name}_max": round(max(x), 2)}
        nh = int(msgs["num_headers"].astype(np.int64).sum())
        bytes_read = (16 + 32) * nt + 8 * nh * 2 + int(msgs["ret"].astype(np.int64).sum()) + int(slots["body_len"].sum()) + 16 * nt + 16 * nt
        bytes_written = total + 8 * (nt + 1) * 2 + 4 * nt + 16 * nt
        line = dict(bench="walk_relay", workload=kind, sessions=ns, depth=depth, response_bytes=args.size, max_headers=MAXH, n_slots_total=nt,
                    reply_bytes=total, reps=args.reps, warmup=args.warmup, host_threads=args.threads, host_reps=args.host_reps,
                    **stat("relay", tr), **stat("writer", tw), **stat("host", host_t), **step_cols,
                    relay_over_writer=round(float(np.median(tr) / np.median(tw)), 3), host_over_relay=round(float(np.median(host_t) / np.median(tr)), 2),
                    bytes_read=bytes_read, bytes_written=bytes_written,
                    hbm_share=round((bytes_read + bytes_written) / (float(np.median(tr)) * 1e-6) / (args.hbm_gbs * 1e9), 4),
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
