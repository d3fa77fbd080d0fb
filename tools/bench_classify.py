#!/usr/bin/env python3
"""Time of rhp_classify_batch (rhp_classify.hip) next to the parse kernel's, in one
process on one GPU: the bench.py workloads config 2 (1M x 256 B GET), config 3
(Zipf) and config 5 (1 KiB POST), each in the record layout bench.py times it in.

Per repetition: parse, then classify, on one stream with a HIP event around each;
after a warm-up.  Prints one JSON line per config: median and min of both kernels
in microseconds, the bytes classify moves per request (records and offsets read,
outputs written, and the 64-byte sectors of request bytes its two-stage compare
touches, counted on the host over a sample with the kernel's rule) and what
fraction of the HBM peak that is at the median time.

Without --config every config runs in a child process of its own under a time
limit, one after the other, and the first failure ends the run.
usage: python tools/bench_classify.py [--config get256|zipf|post] [--n N] [--reps K] [--warmup W]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import libreactorng_amd as rhp  # noqa: E402

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E
NAMES = (b"Host", b"Connection", b"Content-Length", b"Transfer-Encoding")
CONFIGS = {   # as bench.py CONFIGS
    "get256": dict(gen=rhp.GEN_GET256, seed=0x5EED0002, maxh=16, mode=rhp.MODE_PHR, layout=rhp.LAYOUT_DENSE),
    "zipf": dict(gen=rhp.GEN_ZIPF, seed=0x5EED0003, maxh=32, mode=rhp.MODE_PHR, layout=rhp.LAYOUT_DENSE_RM),
    "post": dict(gen=rhp.GEN_POST1K, seed=0x5EED0005, maxh=16, mode=rhp.MODE_HTTP, layout=rhp.LAYOUT_DENSE),
}
CHILD_LIMIT_S = 240


def routes_for(buf, off, res):
    """four routes, one of which hits: request 0's own method and path; one of the
    path's length with other bytes (read and rejected), two of other lengths"""
    ok = res.reqs["ret"] > 0
    if res.http is not None:
        ok &= res.http["result"] == 1
    i = int(np.flatnonzero(ok)[0])
    r, a = res.reqs[i], int(off[i])
    method = bytes(buf[a + int(r["method_off"]): a + int(r["method_off"]) + int(r["method_len"])])
    path = bytes(buf[a + int(r["path_off"]): a + int(r["path_off"]) + int(r["path_len"])])
    return ((b"BREW", path), (method, b"/" + b"~" * (len(path) - 1)), (method, path), (None, b"/not-there"))


def sectors_touched(buf, off, res, routes, sample):
    """64-byte sectors of request bytes the kernel's rule reads, per request (mean
    over the first `sample`): the name of a record whose length is that of a name
    not found yet (up to the first differing dword), the path when a route has
    its length, the method when a route with a method survives the path"""
    want = [x.upper() for x in NAMES]
    total = 0
    ok = res.reqs["ret"] > 0
    if res.http is not None:
        ok &= res.http["result"] == 1
    for i in range(sample):
        if not ok[i]:
            continue
        r, a = res.reqs[i], int(off[i])
        req = bytes(buf[a: a + int(r["ret"])])
        lines, found = set(), set()

        def read(at, text, cands):
            """dwords until every candidate is rejected, as same_text"""
            n = 0
            while n < len(text) and cands:
                n = min(n + 4, len(text))
                cands = [c for c in cands if c[:n] == text[:n]]
            lines.update(range(((a + at) & ~3) // 64, (a + at + max(n, 1) - 1) // 64 + 1))
            return cands

        for k in range(int(r["num_headers"])):
            h = res.hdrs[i, k]
            if int(h["name_off"]) == rhp.RHP_NAME_NULL or len(found) == len(want):
                continue
            nl, no = int(h["name_len"]), int(h["name_off"])
            cands = [w for w in want if len(w) == nl and w not in found]
            if cands:
                found.update(read(no, req[no: no + nl].upper(), cands))
        po, pl, mo, ml = (int(r[f]) for f in ("path_off", "path_len", "method_off", "method_len"))
        cands = [(m, t) for m, t in routes if len(t) == pl and (not m or len(m) == ml)]
        if cands:
            left = read(po, req[po: po + pl], [t for _, t in cands])
            if any(m for m, t in cands if t in left):
                read(mo, req[mo: mo + ml], [m for m, t in cands if m and t in left])
        total += len(lines)
    return total / max(sample, 1)


def run(key, n, reps, warmup):
    import torch
    cfg = CONFIGS[key]
    buf, off = rhp.generate(cfg["gen"], n, cfg["seed"])
    db = rhp.DeviceBatch(buf, off, cfg["maxh"], cfg["mode"], layout=cfg["layout"])
    db.launch()
    res = db.result()
    routes = routes_for(buf, off, res)
    launch, fields, route = db.classifier(NAMES, routes)
    s = torch.cuda.current_stream()
    for _ in range(warmup):
        db.launch()
        launch()
    torch.cuda.synchronize()
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(reps)]
    for e in ev:
        e[0].record(s)
        db.launch()
        e[1].record(s)
        launch()
        e[2].record(s)
    torch.cuda.synchronize()
    parse = np.array([e[0].elapsed_time(e[1]) for e in ev]) * 1e3
    cls = np.array([e[1].elapsed_time(e[2]) for e in ev]) * 1e3
    # the classification itself, against the host twin over the same records
    f = fields.cpu().numpy()[: len(NAMES) * n * 4].view(rhp.FIELDREF_DTYPE).reshape(len(NAMES), n)
    r = route.cpu().numpy().view(np.uint16)[:n]
    cf, cr = rhp.classify_cpu(db.result(), NAMES, routes)
    assert np.array_equal(f, cf) and np.array_equal(r, cr), "the kernel and the host twin differ"
    ok = res.reqs["ret"] > 0
    if res.http is not None:
        ok &= res.http["result"] == 1
    nh = float(res.reqs["num_headers"][ok].sum()) / n
    dense = cfg["layout"] in rhp.DENSE_LAYOUTS
    rec = (8 if dense else 16) + (8 if cfg["mode"] == rhp.MODE_HTTP else 0) + nh * (2 if dense else 8) + 8 * float(ok.mean())
    out = 4 * len(NAMES) + 2
    sect = sectors_touched(buf, off, res, routes, min(n, 4096))
    moved = rec + out + 64 * sect
    med = float(np.median(cls))
    print(json.dumps({
        "config": key, "requests": n, "layout": cfg["layout"], "mode": cfg["mode"], "reps": reps, "warmup": warmup,
        "parse_us_median": round(float(np.median(parse)), 2), "parse_us_min": round(float(parse.min()), 2),
        "classify_us_median": round(med, 2), "classify_us_min": round(float(cls.min()), 2),
        "classify_over_parse_median": round(med / float(np.median(parse)), 3),
        "headers_per_request": round(nh, 2), "fields_present": int((f["value_off"] != rhp.RHP_NAME_NULL).sum()),
        "routed": int((r != rhp.ROUTE_NONE).sum()),
        "bytes_per_request": {"records_and_offsets_read": round(rec, 1), "outputs_written": out,
                              "request_sectors_64B": round(sect, 2), "total": round(moved, 1)},
        "classify_GBps": round(moved * n / med / 1e3, 1),
        "hbm_peak_fraction": round(moved * n / med / 1e3 / HBM_PEAK_GBS, 3),
        "input_bytes": int(off[-1]), "librhp_sha256": rhp.library_sha256()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.config:
        run(a.config, a.n, a.reps, a.warmup)
        return 0
    for key in ("get256", "zipf", "post"):   # a fresh process each, under its own limit; stop at the first failure
        rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", key, "--n", str(a.n), "--reps",
                             str(a.reps), "--warmup", str(a.warmup)], timeout=CHILD_LIMIT_S).returncode
        if rc != 0:
            print(f"bench_classify: config {key} ended with status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
