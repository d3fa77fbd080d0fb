#!/usr/bin/env python3
"""Times rhp_decode_chunked (include/rhp.h) on the GPU beside a plain device copy
of the same bytes and beside the reference's own loop on the host, in one process.

The streams: --n of them (65 536 by default), each with one piece of --piece
bytes (4 KiB) that just arrived: the first bytes of a chunked body whose chunks
all hold --chunk data bytes, decoders zero-filled.  Per chunk size (1024 and 64
by default) one JSON line:
  decode_us    rhp_decode_chunked over the batch
  copy_us      hipMemcpyAsync, device to device, of the same byte count: what
               the moves cost at best
               both: HIP events around the call, median of --reps after
               --warmup, in two alternating blocks each (a.., b.., a.., b..);
               *_blocks are the blocks' medians, *_min / *_max the extremes.
               Before every timed decode the bytes and the decoders are put back
               by a device copy outside the events.
  ref_host_us  phr_decode_chunked of the compiled reference
               (oracle/_ref/libref.so), one call per stream on --threads host
               threads (tools/decode_chunked_host_loop.c), a host clock around
               the C call, median of --host-reps, the bytes put back before each;
               null where the library is not built
  bytes, decoded_bytes, chunks_per_piece  counted from the shapes
The kernel's results, decoders and bytes are compared with the host twin's (and
the reference's results with them) before anything is timed.
usage: python tools/bench_decode_chunked.py [--out profiles/decode_chunked/bench_decode_chunked.jsonl]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import libreactorng_amd as rhp  # noqa: E402

LIBREF_DIR = os.path.join(ROOT, "oracle", "_ref")


def piece_of(chunk: int, piece: int) -> np.ndarray:
    """the first `piece` bytes of a body of `chunk`-byte chunks"""
    data = bytes((i * 37 + 10) & 0xff for i in range(chunk))
    one = b"%x\r\n" % chunk + data + b"\r\n"
    return np.frombuffer((one * (piece // len(one) + 1))[:piece], dtype=np.uint8)


def host_loop():
    """tools/decode_chunked_host_loop.c linked with the compiled reference, built when missing or older than its
    source; None where oracle/_ref/libref.so is not built"""
    if not os.path.exists(os.path.join(LIBREF_DIR, "libref.so")):
        return None
    src, so = os.path.join(HERE, "decode_chunked_host_loop.c"), os.path.join(HERE, "libdecode_chunked_host_loop.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", src, "-o", so, "-L" + LIBREF_DIR, "-lref", "-lpthread",
                               "-Wl,-rpath," + LIBREF_DIR])
    lib = ctypes.CDLL(so)
    vp = ctypes.c_void_p
    lib.decode_chunked_host_loop.argtypes = [vp, vp, vp, vp, vp, ctypes.c_uint32, ctypes.c_uint32]
    lib.decode_chunked_host_loop.restype = ctypes.c_uint64
    return lib


def hip_runtime():
    """the HIP runtime this process already uses (the one librhp.so and torch share)"""
    rhp.lib()
    hip = ctypes.CDLL(rhp.hip_runtimes()[0])
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    hip.hipMemcpyAsync.restype = ctypes.c_int
    return hip


def timed(call, reps, before=None):
    """`reps` device times of call() in microseconds: an event pair around each (before() outside it), one
    synchronise at the end"""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        if before:
            before()
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 16)
    ap.add_argument("--piece", type=int, default=4096)
    ap.add_argument("--chunk", type=int, nargs="+", default=[1024, 64])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--build-only", action="store_true", help="build the host loop and stop (no GPU needed)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    loop = host_loop()
    if args.build_only:
        return
    import torch
    assert torch.cuda.is_available(), "bench_decode_chunked needs the GPU: there is no other way to take its times"
    hip = hip_runtime()
    n = args.n
    lines = []
    for chunk in args.chunk:
        one = piece_of(chunk, args.piece)
        buf = np.tile(one, n)
        off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(args.piece))
        dec0 = np.zeros(n, dtype=rhp.CHUNKED_DTYPE)
        want_res, want_dec, want_by = rhp.decode_chunked_cpu(buf, off, dec0)

        ref_us = None
        if loop is not None:
            t = []
            work, ret, size = buf.copy(), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint64)
            for _ in range(args.host_reps):
                work[:] = buf
                dec = dec0.copy()
                t0 = time.perf_counter()
                loop.decode_chunked_host_loop(work.ctypes.data, off.ctypes.data, dec.ctypes.data, ret.ctypes.data, size.ctypes.data,
                                              n, args.threads)
                t.append((time.perf_counter() - t0) * 1e6)
            assert (ret == want_res["ret"]).all() and (size == want_res["size"]).all() and (work == want_by).all() and \
                dec.tobytes() == want_dec.tobytes(), "the reference's answers differ from the host twin's"
            ref_us = float(np.median(t))
            del work

        pristine = torch.from_numpy(buf).to("cuda")
        dbytes, other = torch.empty_like(pristine), torch.empty_like(pristine)
        doff = torch.from_numpy(off.view(np.int64)).to("cuda")
        ddec0 = torch.zeros(16 * n, dtype=torch.uint8, device="cuda")
        ddec = torch.empty_like(ddec0)
        dres = torch.full((16 * n,), rhp.CHUNKED_POISON, dtype=torch.uint8, device="cuda")
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def restore():
            dbytes.copy_(pristine)
            ddec.copy_(ddec0)
        a = lambda: rhp.decode_chunked_device(dbytes, buf.size, doff, n, ddec, dres)

        def b():
            rc = hip.hipMemcpyAsync(other.data_ptr(), pristine.data_ptr(), buf.size, 3, stream)   # hipMemcpyDeviceToDevice
            assert rc == 0, f"hipMemcpyAsync failed: {rc}"
        restore()
        a()
        torch.cuda.synchronize()
        assert (dres.cpu().numpy().view(rhp.CHUNKED_RESULT_DTYPE) == want_res).all(), "the kernel's results differ from the host twin's"
        assert ddec.cpu().numpy().tobytes() == want_dec.tobytes(), "the kernel's decoders differ from the host twin's"
        assert (dbytes.cpu().numpy() == want_by).all(), "the kernel's bytes differ from the host twin's"

        for _ in range(args.warmup):
            restore()
            a()
            b()
        half = (args.reps + 1) // 2
        ta1, tb1 = timed(a, half, restore), timed(b, half)
        ta2, tb2 = timed(a, half, restore), timed(b, half)
        ta, tb = ta1 + ta2, tb1 + tb2
        med = lambda x: round(float(np.median(x)), 2)
        lines.append(dict(bench="decode_chunked", n=n, piece=args.piece, chunk=chunk, reps=len(ta), warmup=args.warmup,
                          decode_us=med(ta), decode_blocks=[med(ta1), med(ta2)], decode_min=round(min(ta), 2),
                          decode_max=round(max(ta), 2), copy_us=med(tb), copy_blocks=[med(tb1), med(tb2)],
                          copy_min=round(min(tb), 2), copy_max=round(max(tb), 2),
                          ratio_to_copy=round(float(np.median(ta) / np.median(tb)), 3),
                          ref_host_us=None if ref_us is None else round(ref_us, 1), ref_host_threads=args.threads,
                          ratio_to_host=None if ref_us is None else round(float(ref_us / np.median(ta)), 2),
                          bytes=int(buf.size), decoded_bytes=int(want_res["size"].sum()),
                          chunks_per_piece=round(args.piece / (len(b"%x" % chunk) + 4 + chunk), 2),
                          library_sha256=rhp.library_sha256()))
        del pristine, dbytes, other, ddec, ddec0, dres
    text = "".join(json.dumps(x) + "\n" for x in lines)
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
