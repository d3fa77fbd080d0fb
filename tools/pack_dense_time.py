"""Time rhp_pack_dense_kernel alone: a 64K-slot request-major http batch of the
POST workload (bench config 5's generator), parsed once, then `--steps` launches
of rhp_pack_dense between two events.  Prints one JSON line; RHP_LIB picks the
library (a same-box A/B runs this once per build).

usage: [RHP_LIB=...] python tools/pack_dense_time.py [--n 65536] [--steps 200]
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import libreactorng_amd as rhp  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    maxh = 16
    buf, off = rhp.generate(rhp.GEN_POST1K, args.n, 0x5EED0005)
    db = rhp.DeviceBatch(buf, off, maxh, rhp.MODE_HTTP, layout=rhp.LAYOUT_REQUEST_MAJOR)
    db.launch()
    n = db.n
    dd = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    dh = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    dl = torch.zeros(maxh * n, dtype=torch.int16, device="cuda")
    d = db.desc()
    s = torch.cuda.current_stream().cuda_stream

    def pack():
        rc = rhp.lib().rhp_pack_dense(ctypes.byref(d), dd.data_ptr(), dh.data_ptr(), dl.data_ptr(), s)
        if rc != 0:
            raise RuntimeError(f"rhp_pack_dense failed: {rc}")

    for _ in range(args.warmup):
        pack()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(args.steps):
        pack()
    t1.record()
    torch.cuda.synchronize()
    dense = int(((dd.cpu().numpy().reshape(n, 8)[:, 7] & rhp.DENSE_WIDE) == 0).sum())
    print(json.dumps({"lib": rhp.LIBRHP, "sha256": rhp.library_sha256(), "n": n, "dense_slots": dense,
                      "steps": args.steps, "us_per_launch": round(t0.elapsed_time(t1) * 1e3 / args.steps, 3)}))


if __name__ == "__main__":
    main()
