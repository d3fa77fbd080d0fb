"""Input sets of the classify tests (tests/test_classify.py) and of their golden
fixture (tests/golden/classify.npz, written by tests/golden/make_golden_classify.py
from the compiled reference's http_field_lookup).  Every set is rebuilt from
seeds or by hand here; the fixture holds only the sha256 of its bytes and the
expected (fields, route) arrays, which do not depend on the record layout."""
from __future__ import annotations

import hashlib
import os

import numpy as np

import libreactorng_amd as rhp
from batches import pack

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classify.npz")

P, H = rhp.MODE_PHR, rhp.MODE_HTTP
PHR_LAYOUTS = (rhp.LAYOUT_REQUEST_MAJOR, rhp.LAYOUT_HEADER_MAJOR, rhp.LAYOUT_COMPACT, rhp.LAYOUT_DENSE,
               rhp.LAYOUT_DENSE_RM)
HTTP_LAYOUTS = PHR_LAYOUTS[:4]   # rhp_parse_batch refuses RHP_LAYOUT_DENSE_RM in http mode


def layouts(mode):
    return PHR_LAYOUTS if mode == P else HTTP_LAYOUTS


# the generators emit these names' case variants and one-byte-off names (rhp_gen.c gen_fuzz)
FUZZ_NAMES = (b"Content-Length", b"transfer-encoding", b"HOST", b"Content-Lengt", b"Transfer-Encodings", b"X-Absent")
FUZZ_ROUTES = ((b"GET", b"/"), (None, b"/index.html"), (b"POST", b"/"), (None, b"/"))
WORK_NAMES = (b"Host", b"Connection", b"Content-Length", b"Transfer-Encoding")

# hand-built batch: lookup names of 1, 3, 4, 5, 7, 8, 9, 63 and 64 bytes.  The
# five 5-byte names differ from the header name a^_`| in its case, or in one byte
# by 0x20 outside a..z ('^' / '~', '_' / DEL, '`' / '@', '|' / '\\'): only the
# first may match.
N63, N64 = b"N" * 62 + b"z", b"M" * 63 + b"q"
HAND_TARGETS = (b"a", b"Via", b"Host", b"a^_`|", b"Upgrade", b"If-Match", b"Forwarded", N63, N64)
HAND_NAMES = (b"a", b"Via", b"Host", b"A^_`|", b"a~_`|", b"a^\x7f`|", b"a^_@|", b"a^_`\\", b"Upgrade", b"If-Match",
              b"Forwarded", N63, N64)
HAND_ROUTES = ((b"GET", b"/exact"), (None, b"/any"), (b"PUT", b"/exact"), (b"GET", b"/pre"), (b"GET", b"/prefix/long"))
HAND_LINES = (b"GET /exact", b"PUT /exact", b"POST /exact", b"DELETE /any", b"GET /prefix", b"GET /pre",
              b"GET /prefix/long", b"GET /exac", b"GET /exact/")


def _last_off(name):
    """the name with its last byte changed (still a token byte)"""
    return name[:-1] + (b"u" if name[-1:] != b"u" else b"v")


def _near(name):
    """a header name that differs from the lookup name only by 0x20 in a byte outside a..z"""
    return name.replace(b"^", b"~") if b"^" in name else _last_off(name)


def hand_batch():
    """(requests, name alignments hit): every HAND_TARGETS name, in another case,
    in six header arrangements, each at all four alignments of the name's
    absolute address (a padding request before it sets the alignment)."""
    reqs, hit = [], set()
    total = 0

    def add(r):
        nonlocal total
        reqs.append(r)
        total += len(r)

    lines = 0
    for t in HAND_TARGETS:
        hn = t.swapcase()
        fill = b"".join(b"F%d: y\r\n" % k for k in range(63))
        for v in range(6):
            for r4 in range(4):
                line = HAND_LINES[lines % len(HAND_LINES)] + b" HTTP/1.1\r\n"
                lines += 1
                head = {
                    0: hn + b": first\r\nOther: x\r\n",                                     # at index 0
                    1: fill + hn + b": last\r\n",                                           # the last of 64 records
                    2: b"Other: x\r\n" + hn + b": one\r\n" + t + b": two\r\n",              # a duplicate: the first wins
                    3: (hn + b":\r\n" if r4 & 1 else hn + b": \r\n") + t + b": late\r\n",    # present, empty value
                    4: _near(hn) + b": near\r\n folded\r\n" + hn + b": after-fold\r\n",      # obs-fold between candidates
                    5: _near(hn) + b": near\r\n" + _last_off(hn) + b": off\r\n",             # near misses only
                }[v]
                name_at = len(line) + (len(fill) if v == 1 else len(b"Other: x\r\n") if v == 2 else
                                       head.index(hn + b": after") if v == 4 else 0)
                base = len(b"GET / HTTP/1.1\r\n\r\n")
                x = (r4 - total - base - name_at) % 4
                add(b"GET /" + b"p" * x + b" HTTP/1.1\r\n\r\n")
                hit.add((len(t), (total + name_at) % 4))
                add(line + head + b"\r\n")
    big = b"GET /exact HTTP/1.1\r\n" + N63.swapcase() + b": " + b"v" * 1008 + b"\r\nHost: after-big\r\n\r\n"
    extra = [
        big,                                                                   # the dense overflow area
        b"GET /exact HTTP/1.1\r\nHost: h\r\n" + N64 + b": " + b"w" * 1007 + b"\r\n\r\n",
        b"\r\nGET /exact HTTP/1.1\r\nHost: after-crlf\r\nVia: 1.1 x\r\n\r\n",    # leading CRLF: wide records
        b"\nPUT /exact HTTP/1.0\nhost:lf-only\n\n",
        b"GET /exact HTTP/1.1\r\nHost : bad\r\n\r\n",                           # -1
        b"GET /exact HTTP/1.1\r\nHost: partial\r\n",                           # -2
        b"GET /exact HTTP/1.1\r\nHo\x01st: ctl\r\n\r\n",                         # -1
        b"POST /any HTTP/1.1\r\nHost: b\r\nContent-Length: 4\r\n\r\nbody",
        b"POST /any HTTP/1.1\r\nHost: b\r\nContent-Length: 9\r\n\r\nbody",        # http: body still arriving
        b"POST /any HTTP/1.1\r\nVIA: c\r\nTransfer-Encoding: chunked\r\n\r\n4\r\nbody\r\n0\r\n\r\n",
        b"GET /exact HTTP/1.1\r\n\r\n",                                         # no headers
    ]
    for e in extra:
        add(e)
    return reqs, hit


def poison_batch():
    """More than a quarter of the requests fail (-1, -2, one RHP_RET_TOOLONG) and
    every other one has fewer headers than max_headers = 16: most records of the
    batch are never written by the parse."""
    ok = [b"GET /exact HTTP/1.1\r\nHost: p%d\r\nConnection: keep-alive\r\n\r\n" % k for k in range(8)]
    ok += [b"POST /any HTTP/1.1\r\nhost: q\r\ncontent-length: 2\r\nVia: z\r\n\r\nhi"]
    bad = [b"GET /exact HTTP/1.1\r\nHost : x\r\n\r\n", b"GET /exact HTTP/1.1\r\nHost: x\r\n", b"GET /exact HTTP/9.9\r\n\r\n",
           b"GET /exact", b"\x01GET /exact HTTP/1.1\r\nHost: x\r\n\r\n"]
    out = []
    for k in range(40):
        out += [ok[k % len(ok)], bad[k % len(bad)]] if k % 3 else [ok[k % len(ok)]]
    out.insert(17, b"GET /exact HTTP/1.1\r\nHost: x\r\nX: " + b"v" * 70000 + b"\r\n\r\n")   # RHP_RET_TOOLONG
    return out


def _gen(cfg, n, seed, lo=0):
    return lambda: rhp.generate(cfg, n, seed, lo=lo)


# name -> (inputs() -> (buf, off), max_headers, mode, layouts, names, routes)
SETS = {}
for _m in (0, 1, 16, 64):
    SETS[f"fuzz_phr_m{_m}"] = (_gen(rhp.GEN_FUZZ, 4096, 1000 + _m), _m, P, PHR_LAYOUTS, FUZZ_NAMES, FUZZ_ROUTES)
    SETS[f"fuzz_http_m{_m}"] = (_gen(rhp.GEN_FUZZ_HTTP, 4096, 2000 + _m), _m, H, HTTP_LAYOUTS, FUZZ_NAMES, FUZZ_ROUTES)
# 1024-request slices of the timed workloads, each in the layout bench.py --layout auto times it in
def _get256_routes():
    """the generator's paths are 138 random bytes: the paths of two requests of the
    slice, one of another length, and one of their length that no request has"""
    buf, off = inputs("get256")
    path = lambda i: bytes(buf[int(off[i]) + 4: int(off[i]) + 4 + 138])
    return ((b"POST", path(5)), (b"GET", b"/plaintext"), (b"GET", path(5)), (None, path(700)), (b"GET", b"/" + b"x" * 137))


SETS["get256"] = (_gen(rhp.GEN_GET256, 1024, 0x5EED0002, 300000), 16, P, (rhp.LAYOUT_DENSE,), WORK_NAMES, _get256_routes)
SETS["zipf"] = (_gen(rhp.GEN_ZIPF, 1024, 0x5EED0003, 500000), 32, P, (rhp.LAYOUT_DENSE_RM,), WORK_NAMES, FUZZ_ROUTES)
SETS["post1k"] = (_gen(rhp.GEN_POST1K, 1024, 0x5EED0005, 700000), 16, H, (rhp.LAYOUT_DENSE,), WORK_NAMES,
                  ((b"POST", b"/upload"), (None, b"/"), (b"GET", b"/upload")))
SETS["chunked"] = (_gen(rhp.GEN_CHUNKED, 1024, 0x5EED0006, 900000), 16, H, (rhp.LAYOUT_HEADER_MAJOR,), WORK_NAMES,
                   ((b"POST", b"/upload"), (None, b"/"), (b"GET", b"/upload")))
SETS["hand_phr"] = (lambda: pack(hand_batch()[0]), 64, P, PHR_LAYOUTS, HAND_NAMES, HAND_ROUTES)
SETS["hand_http"] = (lambda: pack(hand_batch()[0]), 64, H, HTTP_LAYOUTS, HAND_NAMES, HAND_ROUTES)
SETS["poison_phr"] = (lambda: pack(poison_batch()), 16, P, PHR_LAYOUTS, HAND_NAMES[:3] + WORK_NAMES[1:], HAND_ROUTES)
SETS["poison_http"] = (lambda: pack(poison_batch()), 16, H, HTTP_LAYOUTS, HAND_NAMES[:3] + WORK_NAMES[1:], HAND_ROUTES)

# wave and block edges of the kernel's 256-lane blocks: prefixes of one set
EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257)
EDGE_SET = "fuzz_phr_m16"

_golden = None
_inputs = {}


def inputs(name):
    """(buf, off) of a set, built once and checked against the fixture's sha256"""
    if name not in _inputs:
        buf, off = SETS[name][0]()
        g = golden()
        if g is not None:
            assert hashlib.sha256(buf.tobytes()).hexdigest() == str(g[name + "/sha256"]), f"{name}: input drifted"
        _inputs[name] = (buf, off)
    return _inputs[name]


def tables(name):
    """(names, routes) of a set"""
    names, routes = SETS[name][4:6]
    return names, routes() if callable(routes) else routes


def golden():
    global _golden
    if _golden is None and os.path.exists(GOLDEN):
        _golden = dict(np.load(GOLDEN))
    return _golden


def expected(name):
    """(fields FIELDREF_DTYPE [n_names, n], route u16 [n]) of the compiled reference"""
    g = golden()
    assert g is not None, f"{GOLDEN} is missing (tests/golden/make_golden_classify.py writes it)"
    f = g[name + "/fields"]
    out = np.zeros(f.shape[:2], dtype=rhp.FIELDREF_DTYPE)
    out["value_off"], out["value_len"] = f[..., 0], f[..., 1]
    return out, g[name + "/route"]
