#!/usr/bin/env python3
"""Writes tests/golden/reply_sessions.npz (dev container only: needs the compiled
reference, oracle/_ref/libref.so, which `make -C oracle ref` builds).  Nothing
of the code under test takes part.

For every input set of tests/reply_session_sets.py:
  1. the request boundaries and the last result of every session come from the
     sequential loop (tests/test_sessions.py oracle_sessions), asserted against
     the compiled reference's own parse of the flat batch of boundaries
     (oracle_util.run_reference), as make_golden_classify_sessions.py does;
  2. the route at every boundary is make_golden_classify.classify_reference's;
  3. the leading-run rule and the -1 rule (rhp.h rhp_reply_sessions), in Python:
     a session that ended on -1 answers nothing, any other its leading requests
     whose route is in the static mask;
  4. the reference's http_write_response (oracle_util.reference_write_responses)
     runs over the answered requests' responses in session order: that byte
     stream is `out`.
Stored per set: the inputs' sha256, count[s], out_len[s], total, the sha256 of
out, and for `shapes` the bytes themselves.
usage: python tests/golden/make_golden_reply_sessions.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import libreactorng_amd as rhp  # noqa: E402
import reply_session_sets as rss  # noqa: E402
from make_golden_classify import classify_reference  # noqa: E402
from oracle_util import reference_write_responses, run_reference  # noqa: E402
from test_sessions import oracle_sessions  # noqa: E402


def boundaries(buf, off, sess):
    """per session [(result, route)] of its requests in order, from the reference"""
    n = len(off) - 1
    sessions = [(int(a), int(b)) for a, b in sess]
    walks, _ = oracle_sessions(buf, off, sessions, rss.MAX_HEADERS)
    flat, loop, ends = [], [], []
    for (lo, hi), seq in zip(sessions, walks):
        assert len(seq) <= hi - lo, "a session with more requests than pieces"
        for m, (res, pos, consumed, *_) in enumerate(seq):
            flat.append(pos)
            loop.append((res, consumed))
            ends.append(int(off[hi]) if m + 1 == len(seq) else None)
    if not flat:
        return [[] for _ in sessions]
    flat_off = np.array(flat + [int(off[n])], dtype=np.uint64)
    assert (flat_off[1:] >= flat_off[:-1]).all()
    for q, end in enumerate(ends):
        assert end is None or int(flat_off[q + 1]) == end, f"boundary {q} does not end with its session"
    _, _, http, _ = run_reference(buf, flat_off, rss.MAX_HEADERS, rhp.MODE_HTTP)
    for q, (res, consumed) in enumerate(loop):
        assert int(http["result"][q]) == res, f"boundary {q}: the reference's result differs from the loop's"
        assert res != 1 or int(http["consumed"][q]) == consumed, f"boundary {q}: consumed differs"
    _, route = classify_reference(buf, flat_off, rss.MAX_HEADERS, rhp.MODE_HTTP, (), rss.ROUTES)
    out, q = [], 0
    for seq in walks:
        out.append([(res, int(route[q + m])) for m, (res, *_) in enumerate(seq)])
        q += len(seq)
    return out


def expected(buf, off, sess):
    arena, resps, fields = rss.responses()
    count, answered = [], []
    for seq in boundaries(buf, off, sess):
        k = 0
        if seq and seq[-1][0] != -1:
            while k < len(seq) and seq[k][1] < len(resps) and (rss.STATIC_MASK >> seq[k][1]) & 1:
                k += 1
        count.append(k)
        answered.append([r for _, r in seq[:k]])
    rows = resps[[r for a in answered for r in a]] if any(answered) else resps[:0]
    out, out_off = reference_write_responses(arena, rows, fields)
    at = np.cumsum([0] + count)
    out_len = np.array([int(out_off[at[s + 1]] - out_off[at[s]]) for s in range(len(count))], dtype=np.uint64)
    assert int(out_len.sum()) == len(out)
    return np.array(count, dtype=np.uint32), out_len, out


def main():
    res = {}
    for name, make in rss.SETS.items():
        buf, off, sess = make()
        count, out_len, out = expected(buf, off, sess)
        res[name + "/sha256"] = np.array(rss.digest(buf, off, sess))
        res[name + "/count"], res[name + "/out_len"] = count, out_len
        res[name + "/total"] = np.array(len(out), dtype=np.uint64)
        res[name + "/out_sha256"] = np.array(hashlib.sha256(out.tobytes()).hexdigest())
        if name == "shapes":
            res[name + "/out"] = out
        print(f"{name}: {len(sess)} sessions, {int(count.sum())} replies, longest run {int(count.max()) if len(count) else 0}, "
              f"total {len(out)} bytes")
    np.savez_compressed(rss.GOLDEN, **res)
    print(f"{rss.GOLDEN}: {os.path.getsize(rss.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
