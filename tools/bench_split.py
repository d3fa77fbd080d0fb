#!/usr/bin/env python3
"""Times rhp_split_sessions (include/rhp.h) on the GPU beside the parse of the
same bytes and beside the host scan it replaces, in one process.

Rounds of pipelined 128-byte GETs, sessions x requests per session: 64 x 64,
128 x 128 and 256 x 256 (the reactor's crossover shapes).  Per round one JSON
line:
  split_us       rhp_split_sessions (three launches), HIP events around the
                 call, median of --reps after --warmup
  parse_us       rhp_parse_batch of the speculative batch over the split's
                 offsets (n = n_pieces), the same way
  host_loop_us   the reactor's host split of the same bytes in host memory
                 (tools/split_host_loop.c: find_empty_line per session), a host
                 clock around the C call, median of --reps
  traffic_bytes  what the split's kernels load and store, counted from their
                 code: the input once, the work area written and read once,
                 sess_off, the outputs
The split's outputs are compared with the host twin's before anything is timed.

Kernel times come from a profiler run of their own:
  rocprofv3 --kernel-trace --stats -d DIR -o t -- python tools/bench_split.py --trace-round 64x64
runs the split and the parse of one round --reps times each and nothing else;
  python tools/bench_split.py --kernel-stats 64x64=DIR ... --out FILE
then writes, per round, the average time of each kernel from the run's database
and their sums as split_kernels_us and parse_kernel_us.
usage: python tools/bench_split.py [--out profiles/split/bench_split.jsonl]
"""
import argparse
import ctypes
import glob
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import libreactorng_amd as rhp  # noqa: E402

GET128 = (b"GET /plaintext HTTP/1.1\r\nHost: tfb-server:8080\r\nAccept: text/plain\r\n"
          b"Connection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n\r\n")
assert len(GET128) == 128
ROUNDS = ((64, 64), (128, 128), (256, 256))
MAXH = 16
SPLIT_KERNELS = ("rhp_split_mark_kernel", "rhp_split_scan_kernel", "rhp_split_write_kernel")


def host_loop():
    """tools/split_host_loop.c as a shared library beside it, built when missing or older than its source"""
    src, so = os.path.join(HERE, "split_host_loop.c"), os.path.join(HERE, "libsplit_host_loop.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.split_host_loop.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    lib.split_host_loop.restype = ctypes.c_uint64
    return lib


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


def traffic_bytes(end, n_sessions, n_pieces, cap):
    """the loads and stores of rhp_split.hip's three kernels for an input of `end` bytes: the 16-byte groups once,
    200 bytes of work per step written by the mark kernel and read by the write kernel (the scan reads and
    writes the steps' counts), sess_off by the mark's searches (once per step, not counted: cached), by the
    write kernel's session threads and, per cut, a bisection (not counted: cached), offsets and sessions"""
    steps = (end + rhp.SPLIT_STEP_BYTES - 1) // rhp.SPLIT_STEP_BYTES
    return {"input": (end + 15) // 16 * 16, "work_written": 200 * steps + 8 + 8 * steps, "work_read": 200 * steps + 8 * steps,
            "sess_off": 8 * (n_sessions + 1), "outputs": 8 * (cap + 1) + 8 * n_sessions + 8}


def setup(sessions, per):
    import torch
    data = [GET128 * per] * sessions
    buf, sess_off = rhp.pack_raw(data)
    end, n = int(sess_off[-1]), sessions * per
    want = rhp.split_sessions_cpu(buf, sess_off, n)
    assert want[0] == n
    db = rhp.DeviceBatch(buf, want[1].copy(), MAXH, rhp.MODE_HTTP, flags=rhp.BATCH_SPECULATIVE)
    dso = torch.from_numpy(sess_off.view(np.int64)).to("cuda")
    u8 = lambda size: torch.full((max(size, 8),), 0xFF, dtype=torch.uint8, device="cuda")
    n_pieces, offsets, dsess, work = u8(8), u8(8 * (n + 1)), u8(8 * sessions), u8(8 * rhp.split_work_words(end, sessions))
    o = rhp.SplitOut(n_pieces.data_ptr(), offsets.data_ptr(), n, dsess.data_ptr(), work.data_ptr())
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)

    def split():
        rc = rhp.lib().rhp_split_sessions(vp(db.bytes.data_ptr()), end, vp(dso.data_ptr()), sessions, ctypes.byref(o), stream)
        if rc != 0:
            raise RuntimeError(f"rhp_split_sessions failed: {rc}")

    split()
    torch.cuda.synchronize()
    got = rhp._split_result(n_pieces.cpu().numpy(), offsets.cpu().numpy(), dsess.cpu().numpy(), n, sessions)
    assert got[0] == want[0] and (got[1] == want[1]).all() and (got[2] == want[2]).all(), "the split differs from the twin"
    db.offsets = offsets.view(torch.int64)   # the parse runs over the split's own offsets
    keep = (dso, n_pieces, offsets, dsess, work, o)
    return buf, sess_off, end, n, db, split, keep


def bench_round(sessions, per, reps, warmup):
    buf, sess_off, end, n, db, split, keep = setup(sessions, per)
    hl = host_loop()
    host_off = np.zeros(n + 1, dtype=np.uint64)
    assert hl.split_host_loop(buf.ctypes.data, sess_off.ctypes.data, sessions, host_off.ctypes.data) == n
    assert (host_off == db.host_off).all()
    times = []
    for _ in range(reps + warmup):
        t0 = time.perf_counter()
        hl.split_host_loop(buf.ctypes.data, sess_off.ctypes.data, sessions, host_off.ctypes.data)
        times.append(time.perf_counter() - t0)
    r = {"sessions": sessions, "per_session": per, "pieces": n, "bytes": end, "reps": reps,
         "split_us": median_us(split, reps, warmup), "parse_us": median_us(db.launch, reps, warmup),
         "host_loop_us": float(np.median(times[warmup:])) * 1e6, "traffic_bytes": traffic_bytes(end, sessions, n, n)}
    r["split_over_parse"] = r["split_us"] / r["parse_us"]
    return r


def trace_round(sessions, per, reps, warmup):
    """what a profiler run records: the split and the parse of one round, reps + warmup times each"""
    import torch
    *_, db, split, keep = setup(sessions, per)
    for _ in range(reps + warmup):
        split()
    torch.cuda.synchronize()
    for _ in range(reps + warmup):
        db.launch()
    torch.cuda.synchronize()


def kernel_stats(directory):
    """{kernel name: average ns, calls} from the database a rocprofv3 --kernel-trace run leaves (its `kernels`
    view: one row per dispatch, duration in ns)"""
    import sqlite3
    files = sorted(glob.glob(os.path.join(directory, "**", "*_results.db"), recursive=True))
    if not files:
        raise RuntimeError(f"no *_results.db under {directory}")
    rows = sqlite3.connect(files[0]).execute("select name, avg(duration), count(*) from kernels group by name")
    return {name: {"avg_ns": float(avg), "calls": int(calls)} for name, avg, calls in rows}


def stats_line(spec):
    name, directory = spec.split("=", 1)
    sessions, per = (int(x) for x in name.split("x"))
    stats = kernel_stats(directory)
    pick = lambda key: [(k, v) for k, v in stats.items() if key in k]
    r = {"sessions": sessions, "per_session": per, "pieces": sessions * per, "bytes": sessions * per * len(GET128),
         "source": "rocprofv3 --kernel-trace --stats", "kernels": {}}
    for key in SPLIT_KERNELS:
        (k, v), = pick(key)
        r["kernels"][key] = v
    parse = [(k, v) for k, v in stats.items() if "rhp_" in k and not any(s in k for s in SPLIT_KERNELS)]
    (k, v), = parse
    r["kernels"]["rhp_parse_batch: " + k.split("(")[0]] = v
    r["split_kernels_us"] = sum(r["kernels"][key]["avg_ns"] for key in SPLIT_KERNELS) / 1e3
    r["parse_kernel_us"] = v["avg_ns"] / 1e3
    r["split_over_parse"] = r["split_kernels_us"] / r["parse_kernel_us"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--trace-round", default=None, help="SxP: run that round's split and parse only (for a profiler)")
    ap.add_argument("--kernel-stats", nargs="*", default=None, help="SxP=DIR ...: lines from rocprofv3 stats files")
    a = ap.parse_args()
    lines = []
    if a.kernel_stats is not None:
        lines = [json.dumps(stats_line(spec)) for spec in a.kernel_stats]
    else:
        import torch
        assert torch.cuda.is_available(), "bench_split needs a GPU"
        if a.trace_round:
            trace_round(*(int(x) for x in a.trace_round.split("x")), a.reps, a.warmup)
            return
        for sessions, per in ROUNDS:
            r = bench_round(sessions, per, a.reps, a.warmup)
            r["library_sha256"] = rhp.library_sha256()
            lines.append(json.dumps(r))
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
