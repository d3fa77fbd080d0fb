#!/usr/bin/env python3
"""Writes tests/golden/classify_sessions.npz (dev container only: needs the
compiled reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).

For every input set of tests/classify_session_sets.py:
  1. the request boundaries of every session come from the sequential loop
     (tests/test_sessions.py oracle_sessions: one http_read_request per request
     from the front of the session's input, advancing by what it consumed);
  2. they become one flat offsets array -- sessions lie back to back, so request
     m of a session runs to the start of request m + 1 and a session's last
     entry to the session's end;
  3. the compiled reference parses that flat batch (oracle_util.run_reference)
     and its own http_field_lookup runs over the header arrays it returns
     (make_golden_classify.classify_reference, as for classify.npz).  The
     reference's result and consumed at every boundary must equal the loop's:
     the boundaries are the reference's, not only the oracle restatement's;
  4. request m of session s is scattered to record slot piece_lo + m; every
     other slot is absent ({RHP_NAME_NULL, 0}, RHP_ROUTE_NONE).
usage: python tests/golden/make_golden_classify_sessions.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import libreactorng_amd as rhp  # noqa: E402
import classify_session_sets as css  # noqa: E402
from make_golden_classify import classify_reference  # noqa: E402
from oracle_util import run_reference  # noqa: E402
from test_sessions import oracle_sessions  # noqa: E402


def expected_by_slot(buf, off, sess):
    n = len(off) - 1
    fields = np.zeros((len(css.NAMES), n, 2), dtype=np.uint16)
    fields[..., 0] = rhp.RHP_NAME_NULL
    route = np.full(n, rhp.ROUTE_NONE, dtype=np.uint16)
    sessions = [(int(a), int(b)) for a, b in sess]
    walks, _ = oracle_sessions(buf, off, sessions, css.MAX_HEADERS)
    flat, slot, loop, ends = [], [], [], []   # per boundary: its byte, its record slot, the loop's (result,
    #                                           consumed), and for a session's last one the session's end
    for (lo, hi), seq in zip(sessions, walks):
        assert len(seq) <= hi - lo, "a session with more requests than pieces"
        assert bool(seq) == (off[hi] > off[lo]), "a session with input has a first request, one without has none"
        for m, (res, pos, consumed, *_) in enumerate(seq):
            flat.append(pos)
            slot.append(lo + m)
            loop.append((res, consumed))
            ends.append(int(off[hi]) if m + 1 == len(seq) else None)
    if not flat:
        return fields, route, 0
    # an entry ends where the next one begins.  Sessions lie back to back, so a session's last entry ends at the
    # session's end: the first boundary of the next session that has input, or the end of the input
    flat_off = np.array(flat + [int(off[n])], dtype=np.uint64)
    assert (flat_off[1:] >= flat_off[:-1]).all()
    for q, end in enumerate(ends):
        assert end is None or int(flat_off[q + 1]) == end, f"boundary {q} does not end with its session"
    _, _, http, _ = run_reference(buf, flat_off, css.MAX_HEADERS, rhp.MODE_HTTP)
    for q, (res, consumed) in enumerate(loop):
        assert int(http["result"][q]) == res, f"boundary {q}: the reference's result {int(http['result'][q])}, the loop's {res}"
        if res == 1:
            assert int(http["consumed"][q]) == consumed, f"boundary {q}: consumed differs"
    f, r = classify_reference(buf, flat_off, css.MAX_HEADERS, rhp.MODE_HTTP, css.NAMES, css.ROUTES)
    fields[:, slot] = f
    route[slot] = r
    return fields, route, len(flat)


def main():
    out = {}
    for name, make in css.SETS.items():
        buf, off, sess = make()
        f, r, requests = expected_by_slot(buf, off, sess)
        out[name + "/sha256"] = np.array(css.digest(buf, off, sess))
        out[name + "/fields"], out[name + "/route"] = f, r
        print(f"{name}: {len(off) - 1} slots, {len(sess)} sessions, {requests} boundaries, present per name "
              f"{(f[..., 0] != rhp.RHP_NAME_NULL).sum(axis=1).tolist()}, routed {int((r != rhp.ROUTE_NONE).sum())}")
    np.savez_compressed(css.GOLDEN, **out)
    print(f"{css.GOLDEN}: {os.path.getsize(css.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
