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

--sessions times rhp_classify_sessions instead (rhp_classify.hip's second
kernel): rounds of TFB GETs as sessions x pipelined requests (64 x 64, 256 x
256, 4096 x 1, 65536 x 1), each parsed as a speculative batch; rhp_fixup_sessions
and rhp_classify_sessions between HIP events, and for comparison
rhp_classify_batch over the same requests parsed as a non-speculative
request-major batch.  One JSON line per round, a child process each.
usage: python tools/bench_classify.py [--config get256|zipf|post] [--n N] [--reps K] [--warmup W]
       python tools/bench_classify.py --sessions [--round SESSIONS PER_SESSION] [--reps K] [--warmup W]
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


TFB = (b"GET /plaintext HTTP/1.1\r\nHost: tfb-server:8080\r\nAccept: text/plain\r\n"
       b"Connection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n\r\n")
SESSION_ROUTES = ((b"GET", b"/plaintext"), (None, b"/c"), (b"POST", b"/cl"), (b"GET", b"/inside-a-body"))
SESSION_ROUNDS = ((64, 64), (256, 256), (4096, 1), (65536, 1))   # sessions x pipelined requests per session


def run_sessions(n_sessions, per_session, reps, warmup):
    """One round of TFB GETs as the reactor batches it: a speculative parse, then
    rhp_fixup_sessions and rhp_classify_sessions, each between HIP events; next
    to it rhp_classify_batch over the same requests parsed as a non-speculative
    request-major batch (every piece of this round is one request, so the two
    batches have the same offsets)."""
    import ctypes
    import torch
    maxh = 16
    one = TFB * per_session
    buf, off, sess, _ = rhp.pack_sessions([one] * n_sessions,
                                          split=lambda data: [len(TFB)] * per_session)   # (the server's split of it)
    n = len(off) - 1
    assert n == n_sessions * per_session
    vp = ctypes.c_void_p
    spec = rhp.DeviceBatch(buf, off, maxh, rhp.MODE_HTTP, layout=rhp.LAYOUT_REQUEST_MAJOR, flags=rhp.BATCH_SPECULATIVE)
    plain = rhp.DeviceBatch(buf, off, maxh, rhp.MODE_HTTP, layout=rhp.LAYOUT_REQUEST_MAJOR)
    ds = torch.from_numpy(sess.view(np.uint8).copy()).to("cuda")
    dres = torch.zeros(n_sessions * rhp.SESSION_RESULT_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dst = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    text, nm, rt = rhp.classify_tables(NAMES, SESSION_ROUTES)
    fields = torch.zeros(len(nm) * n * 4, dtype=torch.uint8, device="cuda")
    route = torch.zeros(n, dtype=torch.int16, device="cuda")
    c = rhp.Classify(text.ctypes.data, nm.ctypes.data, rt.ctypes.data, len(nm), len(rt), fields.data_ptr(), route.data_ptr())
    d = spec.desc()
    plain_launch, plain_fields, plain_route = plain.classifier(NAMES, SESSION_ROUTES)
    s = torch.cuda.current_stream()
    sp = vp(s.cuda_stream)
    lib = rhp.lib()

    def fixup():
        rc = lib.rhp_fixup_sessions(ctypes.byref(d), vp(ds.data_ptr()), n_sessions, vp(dres.data_ptr()), vp(dst.data_ptr()), sp)
        assert rc == 0, rc

    def classify():
        rc = lib.rhp_classify_sessions(ctypes.byref(d), vp(ds.data_ptr()), n_sessions, vp(dres.data_ptr()),
                                       vp(dst.data_ptr()), ctypes.byref(c), sp)
        assert rc == 0, rc

    def once(ev=None):
        mark = (lambda k: ev[k].record(s)) if ev else (lambda k: None)
        spec.launch()
        mark(0)
        fixup()
        mark(1)
        classify()
        mark(2)
        plain.launch()
        mark(3)
        plain_launch()
        mark(4)

    for _ in range(warmup):
        once()
    torch.cuda.synchronize()
    evs = [[torch.cuda.Event(enable_timing=True) for _ in range(5)] for _ in range(reps)]
    for ev in evs:
        once(ev)
    torch.cuda.synchronize()
    us = lambda a, b: np.array([ev[a].elapsed_time(ev[b]) for ev in evs]) * 1e3
    fix, cls, base = us(0, 1), us(1, 2), us(3, 4)
    # the classification itself: the host twin over the records the GPU left, and the plain batch's kernel
    f = fields.cpu().numpy().view(rhp.FIELDREF_DTYPE).reshape(len(nm), n)
    r = route.cpu().numpy().view(np.uint16)
    results = dres.cpu().numpy().view(rhp.SESSION_RESULT_DTYPE)
    starts = dst.cpu().numpy().view(np.uint64)
    cf, cr = rhp.classify_sessions_cpu(spec.result(), sess, results, starts, NAMES, SESSION_ROUTES)
    assert np.array_equal(f, cf) and np.array_equal(r, cr), "the kernel and the host twin differ"
    pf = plain_fields.cpu().numpy()[: len(nm) * n * 4].view(rhp.FIELDREF_DTYPE).reshape(len(nm), n)
    assert np.array_equal(f, pf) and np.array_equal(r, plain_route.cpu().numpy().view(np.uint16)[:n]), \
        "rhp_classify_sessions and rhp_classify_batch differ"
    assert (r == 0).all() and (results["n_slots"] == per_session).all()
    med = lambda a: round(float(np.median(a)), 2)
    print(json.dumps({
        "leg": "sessions", "sessions": n_sessions, "requests_per_session": per_session, "slots": n, "reps": reps,
        "warmup": warmup, "fixup_us_median": med(fix), "fixup_us_min": round(float(fix.min()), 2),
        "classify_sessions_us_median": med(cls), "classify_sessions_us_min": round(float(cls.min()), 2),
        "classify_batch_us_median": med(base), "classify_batch_us_min": round(float(base.min()), 2),
        "sessions_over_batch_median": round(float(np.median(cls)) / float(np.median(base)), 3),
        "input_bytes": int(off[-1]), "librhp_sha256": rhp.library_sha256()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sessions", action="store_true",
                    help="the rhp_classify_sessions leg: SESSION_ROUNDS of TFB GETs (--round S K: one of them)")
    ap.add_argument("--round", type=int, nargs=2, default=None, metavar=("SESSIONS", "PER_SESSION"))
    ap.add_argument("--config", choices=sorted(CONFIGS), default=None)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if a.sessions and a.round:
        run_sessions(a.round[0], a.round[1], a.reps, a.warmup)
        return 0
    if a.sessions:   # as the configs: a fresh process per round, under its own limit; stop at the first failure
        for n_sessions, per_session in SESSION_ROUNDS:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--sessions", "--round", str(n_sessions),
                                 str(per_session), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                timeout=CHILD_LIMIT_S).returncode
            if rc != 0:
                print(f"bench_classify: round {n_sessions} x {per_session} ended with status {rc}; stopping", file=sys.stderr)
                return rc
        return 0
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
