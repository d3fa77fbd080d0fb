#!/usr/bin/env python3
"""Times rhp_frame_messages (include/rhp.h) next to rhp_parse_messages over the
same batch, in one process on one GPU.

The messages: the requests of generator config 2 (--n of them, 1M by default,
about 256 B each) behind the status line "HTTP/1.1 200 OK", the request line kept
as the value of a first header `X-Request` (so a response keeps its request's
size), and one framing header appended as the last header line -- the longest walk the call
makes: `Content-Length: 1234` (workload "length") or `Transfer-Encoding:
chunked` (workload "chunked", the decoders armed).  The lookup names are
Content-Type and Connection.  Each workload in both record layouts.

Per repetition: parse, then frame, on one stream with a HIP event around each,
after a warm-up; median of --reps.  One JSON line per workload and layout:
  parse_us, frame_us   medians (and *_min) in microseconds; ratio = frame / parse
  bytes_per_message    what the frame call moves, counted on the host with the
                       kernel's rule over the first --sample messages: the message
                       record, offsets[i], the header records walked, the frame,
                       the fields, an armed decoder, and the 64-byte sectors of
                       message bytes the name compares and the value read touch
  hbm_share            bytes_per_message * n / frame_us over the 8 TB/s peak
The frames are compared with the host twin's before anything is timed.
usage: python tools/bench_frame.py [--out profiles/frame_messages/bench_frame.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

import libreactorng_amd as rhp  # noqa: E402

STATUS = b"HTTP/1.1 200 OK\r\n"
MAXH = 16
NAMES = (b"Content-Type", b"Connection")
FRAMING = {"length": b"Content-Length: 1234\r\n", "chunked": b"Transfer-Encoding: chunked\r\n"}
HBM_PEAK_GBS = 8000.0   # MI355X HBM3E


def responses(buf, off, line):
    """STATUS, every request's first line as the header X-Request, its header lines, and `line` in front of the
    empty line that ends it -> (buf with RHP_PAD zeros behind, off)"""
    n = len(off) - 1
    lf = np.flatnonzero(buf[: int(off[-1])] == 10)
    first = lf[np.searchsorted(lf, off[:-1].astype(np.int64))] + 1   # behind each request's first LF
    mv = memoryview(buf)
    parts = []
    for i in range(n):
        m = bytes(mv[int(first[i]): int(off[i + 1])])
        assert m.endswith(b"\r\n\r\n"), "a request of config 2 ends with its empty line"
        parts.append(STATUS + b"X-Request: " + bytes(mv[int(off[i]): int(first[i])]) + m[:-2] + line + b"\r\n")
    data = b"".join(parts)
    out = np.zeros(len(data) + rhp.RHP_PAD, dtype=np.uint8)
    out[: len(data)] = np.frombuffer(data, dtype=np.uint8)
    new_off = np.zeros(n + 1, dtype=np.uint64)
    new_off[1:] = np.cumsum([len(p) for p in parts], dtype=np.uint64)
    return out, new_off


def bytes_moved(buf, off, msgs, hdrs, armed, sample):
    """mean bytes per message the frame kernel reads and writes, by its own rule (rhp_classify.hip): records
    walked until every name is settled; of a record whose name_len is that of a name not settled yet, the name's
    dwords up to the one that rejects the last candidate; then the value the decision reads"""
    want = {x.upper() for x in NAMES} | {b"TRANSFER-ENCODING", b"CONTENT-LENGTH"}
    total = 0
    for i in range(sample):
        a, nh = int(off[i]), int(msgs["num_headers"][i])
        open_, sectors, walked, te, cl = set(want), set(), 0, None, None

        def touch(lo, hi):
            sectors.update(range(((a + lo) & ~3) // 64, (a + hi - 1) // 64 + 1))

        for k in range(nh):
            if not open_:
                break
            walked += 1
            h = hdrs[i, k]
            no, nl, vo, vl = (int(h[f]) for f in ("name_off", "name_len", "value_off", "value_len"))
            cand = [x for x in open_ if len(x) == nl]
            if no == rhp.RHP_NAME_NULL or not cand:
                continue
            name = bytes(buf[a + no: a + no + nl]).upper()
            for j in range(0, nl, 4):   # a dword at a time while a candidate is left
                if not cand:
                    break
                touch(no + j, no + min(j + 4, nl))
                cand = [x for x in cand if x[j: j + 4] == name[j: j + 4]]
            for x in cand:
                open_.discard(x)
                te = (vo, vl) if x == b"TRANSFER-ENCODING" else te
                cl = (vo, vl) if x == b"CONTENT-LENGTH" else cl
        if cl and cl[1] and not (te and te[1]):
            touch(cl[0], cl[0] + cl[1])
        elif te and te[1] == 7:
            touch(te[0], te[0] + 7)
        total += 16 + 8 + 8 * walked + 16 + 4 * len(NAMES) + (16 if armed else 0) + 64 * len(sectors)
    return total / sample


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=2024)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sample", type=int, default=4096)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_frame needs the GPU: there is no other way to take its times"
    n = args.n
    req_buf, req_off = rhp.generate(rhp.GEN_GET256, n, args.seed)
    lines = []
    for wname, line in FRAMING.items():
        buf, off = responses(req_buf, req_off, line)
        dbytes = torch.from_numpy(buf).to("cuda")
        doff = torch.from_numpy(off.view(np.int64)).to("cuda")
        armed = wname == "chunked"
        for layout, lname in ((rhp.LAYOUT_REQUEST_MAJOR, "request_major"), (rhp.LAYOUT_HEADER_MAJOR, "header_major")):
            msgs = torch.full((16 * n,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
            hdrs = torch.full((8 * n * MAXH,), rhp.MSG_POISON, dtype=torch.uint8, device="cuda")
            frames = torch.full((16 * n,), rhp.FRAME_POISON, dtype=torch.uint8, device="cuda")
            fields = torch.full((4 * len(NAMES) * n,), rhp.FRAME_POISON, dtype=torch.uint8, device="cuda")
            dec = torch.full((16 * n,), rhp.FRAME_POISON, dtype=torch.uint8, device="cuda")
            parse = lambda: rhp.parse_messages_device(dbytes, buf.size, doff, n, rhp.MSG_RESPONSE, MAXH, layout, msgs, hdrs)
            frame = lambda: rhp.frame_messages_device(dbytes, buf.size, doff, n, rhp.MSG_RESPONSE, MAXH, layout, msgs, hdrs,
                                                      frames, NAMES, fields, dec, 1)
            parse()
            frame()
            torch.cuda.synchronize()
            hm, hh = rhp._msg_result(msgs.cpu().numpy(), hdrs.cpu().numpy(), n, MAXH, layout)
            assert (hm["ret"] > 0).all(), "every response parses"
            got = rhp._frame_result(frames.cpu().numpy(), fields.cpu().numpy(), dec.cpu().numpy(), n, len(NAMES))
            want = rhp.frame_messages_cpu(buf, off, rhp.MSG_RESPONSE, hm, hh, NAMES, MAXH, layout, 1)
            assert all((g == w).all() for g, w in zip(got, want)), "the kernel's frames, fields or decoders differ from the host twin's"
            kind = rhp.FRAME_CHUNKED if armed else rhp.FRAME_LENGTH
            assert (got[0]["result"] == 1).all() and (got[0]["body_kind"] == kind).all() and (armed or (got[0]["body_len"] == 1234).all())
            for _ in range(args.warmup):
                parse()
                frame()
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.reps)]
            for a, b, c in ev:
                a.record()
                parse()
                b.record()
                frame()
                c.record()
            torch.cuda.synchronize()
            tp = [a.elapsed_time(b) * 1e3 for a, b, _ in ev]
            tf = [b.elapsed_time(c) * 1e3 for _, b, c in ev]
            per = bytes_moved(buf, off, hm, hh, armed, min(args.sample, n))
            med = lambda x: round(float(np.median(x)), 2)
            lines.append(dict(bench="frame_messages", workload=wname, layout=lname, n=n, seed=args.seed, max_headers=MAXH,
                              names=[x.decode() for x in NAMES], reps=args.reps, warmup=args.warmup,
                              parse_us=med(tp), parse_min=round(min(tp), 2), frame_us=med(tf), frame_min=round(min(tf), 2),
                              ratio=round(float(np.median(tf) / np.median(tp)), 4), message_bytes=round(int(off[-1]) / n, 1),
                              headers_per_message=round(float(hm["num_headers"].mean()), 3),
                              bytes_per_message=round(per, 1), bytes_sample=min(args.sample, n),
                              hbm_share=round(per * n / (float(np.median(tf)) * 1e-6) / (HBM_PEAK_GBS * 1e9), 4),
                              library_sha256=rhp.library_sha256()))
            print(json.dumps(lines[-1]), flush=True)
            del msgs, hdrs, frames, fields, dec
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("".join(json.dumps(x) + "\n" for x in lines))


if __name__ == "__main__":
    main()
