#!/usr/bin/env python3
"""Times rhp_parse_messages (include/rhp.h) on the GPU beside the exact request
kernel and beside the reference's own loop on the host, in one process.

The messages: the requests of generator config 2 (--n of them, 1M by default)
with the request line replaced by "HTTP/1.1 200 OK": the same header sections
behind a status line.  Per record layout one JSON line:
  messages_us      rhp_parse_messages (RHP_MSG_RESPONSE) over the responses
  exact_request_us rhp_parse_batch under RHP_IMPL_EXACT (rhp_exact_kernel) over
                   the original requests: the same header loop and the same
                   line-cached reader, one request per lane
                   both: HIP events around the call, median of --reps after
                   --warmup, in two alternating blocks each (a.., b.., a.., b..);
                   *_blocks are the blocks' medians, *_min / *_max the extremes
  ref_host_us      phr_parse_response of the compiled reference
                   (oracle/_ref/libref.so), one call per message on --threads
                   host threads (tools/messages_host_loop.c), a host clock
                   around the C call, median of --host-reps; null where the
                   library is not built
  bytes, records_bytes  what the call reads and writes, counted from the shapes
The responses' records are compared with the host twin's before anything is
timed.
usage: python tools/bench_messages.py [--out profiles/messages/bench_messages.jsonl]
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

STATUS = b"HTTP/1.1 200 OK\r\n"
MAXH = 16
LIBREF_DIR = os.path.join(ROOT, "oracle", "_ref")


def responses(buf, off):
    """every request's first line replaced by STATUS -> (buf with RHP_PAD zeros behind, off)"""
    n = len(off) - 1
    lf = np.flatnonzero(buf[: int(off[-1])] == 10)
    first = lf[np.searchsorted(lf, off[:-1].astype(np.int64))] + 1   # behind each request's first LF
    assert (first <= off[1:].astype(np.int64)).all(), "every request has a request line"
    mv = memoryview(buf)
    data = b"".join(STATUS + bytes(mv[int(first[i]): int(off[i + 1])]) for i in range(n))
    out = np.zeros(len(data) + rhp.RHP_PAD, dtype=np.uint8)
    out[: len(data)] = np.frombuffer(data, dtype=np.uint8)
    new_off = np.zeros(n + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum(len(STATUS) + (off[1:].astype(np.int64) - first), dtype=np.uint64)
    return out, new_off


def host_loop():
    """tools/messages_host_loop.c linked with the compiled reference, built when missing or older than its source;
    None where oracle/_ref/libref.so is not built"""
    if not os.path.exists(os.path.join(LIBREF_DIR, "libref.so")):
        return None
    src, so = os.path.join(HERE, "messages_host_loop.c"), os.path.join(HERE, "libmessages_host_loop.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", src, "-o", so, "-L" + LIBREF_DIR, "-lref", "-lpthread",
                               "-Wl,-rpath," + LIBREF_DIR])
    lib = ctypes.CDLL(so)
    lib.messages_host_loop.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    lib.messages_host_loop.restype = ctypes.c_uint64
    return lib


def timed(call, reps):
    """`reps` device times of call() in microseconds: an event pair around each, one synchronise at the end"""
    import torch
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        call()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e3 for a, b in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=2024)
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
    assert torch.cuda.is_available(), "bench_messages needs the GPU: there is no other way to take its times"

    req_buf, req_off = rhp.generate(rhp.GEN_GET256, args.n, args.seed)
    buf, off = responses(req_buf, req_off)
    n = args.n
    ref_us = None
    if loop is not None:
        t = []
        for _ in range(args.host_reps):
            t0 = time.perf_counter()
            parsed = loop.messages_host_loop(buf.ctypes.data, off.ctypes.data, n, MAXH, args.threads)
            t.append((time.perf_counter() - t0) * 1e6)
        assert parsed == n, f"the reference parsed {parsed} of {n} responses"
        ref_us = float(np.median(t))

    dbytes = torch.from_numpy(buf).to("cuda")
    doff = torch.from_numpy(off.view(np.int64)).to("cuda")
    lines = []
    for layout, lname in ((rhp.LAYOUT_REQUEST_MAJOR, "request_major"), (rhp.LAYOUT_HEADER_MAJOR, "header_major")):
        msgs = torch.full((16 * n,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
        hdrs = torch.full((8 * n * MAXH,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
        a = lambda: rhp.parse_messages_device(dbytes, buf.size, doff, n, rhp.MSG_RESPONSE, MAXH, layout, msgs, hdrs)
        a()
        torch.cuda.synchronize()
        got = rhp._msg_result(msgs.cpu().numpy(), hdrs.cpu().numpy(), n, MAXH, layout)
        want = rhp.parse_messages_cpu(buf, off, rhp.MSG_RESPONSE, MAXH, layout)
        assert (got[0] == want[0]).all() and (got[0]["ret"] > 0).all(), "the kernel's message records differ from the host twin's"
        nh = got[0]["num_headers"]
        used = np.arange(MAXH)[None, :] < nh[:, None]
        assert (got[1][used] == want[1][used]).all(), "the kernel's header records differ from the host twin's"

        db = rhp.DeviceBatch(req_buf, req_off, MAXH, rhp.MODE_PHR, layout=layout)
        rhp.lib().rhp_set_impl(rhp.IMPL_EXACT)
        try:
            b = db.launch
            for _ in range(args.warmup):
                a()
                b()
            half = (args.reps + 1) // 2
            ta1, tb1 = timed(a, half), timed(b, half)
            ta2, tb2 = timed(a, half), timed(b, half)
            assert (db.result().reqs["ret"] > 0).all()
        finally:
            rhp.lib().rhp_set_impl(rhp.IMPL_DFA)
        ta, tb = ta1 + ta2, tb1 + tb2
        med = lambda x: round(float(np.median(x)), 2)
        records = 16 * n + 8 * int(nh.sum())
        lines.append(dict(bench="messages", n=n, seed=args.seed, max_headers=MAXH, layout=lname, reps=len(ta),
                          warmup=args.warmup, messages_us=med(ta), messages_blocks=[med(ta1), med(ta2)],
                          messages_min=round(min(ta), 2), messages_max=round(max(ta), 2),
                          exact_request_us=med(tb), exact_request_blocks=[med(tb1), med(tb2)],
                          exact_request_min=round(min(tb), 2), exact_request_max=round(max(tb), 2),
                          ratio=round(float(np.median(ta) / np.median(tb)), 4),
                          ref_host_us=None if ref_us is None else round(ref_us, 1), ref_host_threads=args.threads,
                          bytes=int(off[-1]), request_bytes=int(req_off[-1]), records_bytes=records,
                          headers_per_message=round(float(nh.mean()), 3), library_sha256=rhp.library_sha256()))
        del msgs, hdrs, db
    text = "".join(json.dumps(x) + "\n" for x in lines)
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
