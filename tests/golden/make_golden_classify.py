#!/usr/bin/env python3
"""Writes tests/golden/classify.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so).

For every input set of tests/classify_sets.py the expected fields come from the
reference's own http_field_lookup (src/reactor/http.c:167-175), called through
ctypes over the header arrays its parser returns (oracle_util.run_reference),
and the expected route from length and memcmp (string_equal) of the method and
target it returns.  A request that is not ready in the batch format (ret <= 0, a
header section past RHP_MAX_LEN, http result != 1) has no fields and no route.
usage: python tests/golden/make_golden_classify.py
"""
import ctypes
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import libreactorng_amd as rhp  # noqa: E402
import classify_sets as cs  # noqa: E402
from oracle_util import reference, run_reference  # noqa: E402


class String(ctypes.Structure):
    """string_t = data_t = struct iovec, by value"""
    _fields_ = [("base", ctypes.c_void_p), ("size", ctypes.c_size_t)]


class Field(ctypes.Structure):
    """http_field_t"""
    _fields_ = [("name", String), ("value", String)]


def classify_reference(buf, off, maxh, mode, names, routes):
    ref = reference()
    lookup = ref.http_field_lookup
    lookup.argtypes = [ctypes.POINTER(Field), ctypes.c_size_t, String]
    lookup.restype = String
    ref.string_null.restype = String
    null = ref.string_null().base   # what the lookup returns for no match: not a pointer into the request
    reqs, hdrs, http, rw = run_reference(buf, off, maxh, mode)
    n = len(off) - 1
    fields = np.zeros((len(names), n, 2), dtype=np.uint16)
    fields[..., 0] = rhp.RHP_NAME_NULL
    route = np.full(n, rhp.ROUTE_NONE, dtype=np.uint16)
    keep = [ctypes.create_string_buffer(bytes(x), len(x)) for x in names]
    arr = (Field * max(maxh, 1))()
    for i in range(n):
        ret = int(reqs["ret"][i])
        if ret <= 0 or ret > rhp.RHP_MAX_LEN or (mode == rhp.MODE_HTTP and int(http["result"][i]) != 1):
            continue
        base = rw.ctypes.data + int(off[i])
        nh = int(reqs["num_headers"][i])
        for k in range(nh):
            h = hdrs[i, k]
            no = int(h["name_off"])
            arr[k].name = String(base + no if no >= 0 else None, int(h["name_len"]))
            arr[k].value = String(base + int(h["value_off"]), int(h["value_len"]))
        for j, x in enumerate(names):
            v = lookup(arr, nh, String(ctypes.addressof(keep[j]), len(x)))
            if v.base != null:
                fields[j, i] = (v.base - base, v.size)
        req = bytes(rw[int(off[i]): int(off[i]) + ret])
        mo, ml, po, pl = (int(reqs[f][i]) for f in ("method_off", "method_len", "path_off", "path_len"))
        method, path = req[mo: mo + ml], req[po: po + pl]
        for r, (m, t) in enumerate(routes):
            if path == t and (not m or method == m):
                route[i] = r
                break
    return fields, route


def main():
    out = {}
    for name, (make, maxh, mode, _, _, _) in cs.SETS.items():
        buf, off = make()
        cs._inputs[name] = (buf, off)   # (no fixture to check them against yet)
        names, routes = cs.tables(name)
        f, r = classify_reference(buf, off, maxh, mode, names, routes)
        out[name + "/sha256"] = np.array(hashlib.sha256(buf.tobytes()).hexdigest())
        out[name + "/fields"], out[name + "/route"] = f, r
        print(f"{name}: n {len(off) - 1}, present per name {(f[..., 0] != rhp.RHP_NAME_NULL).sum(axis=1).tolist()}, "
              f"routed {int((r != rhp.ROUTE_NONE).sum())}")
    np.savez_compressed(cs.GOLDEN, **out)
    print(f"{cs.GOLDEN}: {os.path.getsize(cs.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
