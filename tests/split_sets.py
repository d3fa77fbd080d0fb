"""Input sets of the rhp_split_sessions tests (tests/test_split_sessions.py):
name -> (buf u8, sess_off u64 [n_sessions + 1]), built by hand around the places
where the split's kernels (rhp_split.hip) change what they do: a lane's 16-byte
group, a dword inside it, the 64 bytes of a mask word, a wave's step
(rhp.SPLIT_STEP_BYTES), the four steps of a workgroup, a session's first three
bytes, and sess_off[0].

A set is session inputs packed back to back by rhp.pack_raw: the bytes in front
of sess_off[0] are LF (no session may look back at them), and the bytes behind
the last session are made LF here too (no cut may lie at or behind the end)."""
from __future__ import annotations

import functools

import numpy as np

import libreactorng_amd as rhp

STEP = rhp.SPLIT_STEP_BYTES
GROUP = 4 * STEP   # a workgroup of the mark kernel: four waves
LF, CR = b"\n", b"\r"

PATTERNS = (b"\n\n", b"\n\r\n", b"\r\n\r\n", b"\n\n\n", b"\n\r\n\n")
DELTAS = tuple(range(-3, 4))


def edge_boundaries(i):
    """the five boundaries of pattern i's stretch of the buffer: a dword's, a 16-byte group's, a mask word's,
    a step's and a workgroup's -- each no boundary of the next kind"""
    base = GROUP * i
    return (base + 2048 + 512 + 4, base + 2048 + 256 + 16, base + 2048 + 64, base + STEP, base + GROUP)


def _edges(delta, kind):
    """Every pattern around every kind of boundary.  kind "end": the pattern's last byte is at boundary + delta
    - 1 (the cut it makes is at boundary + delta); kind "start": its first byte is at boundary + delta.  One
    session of filler with the patterns in it."""
    size = GROUP * len(PATTERNS) + 64
    data = bytearray(b"x" * size)
    for i, pat in enumerate(PATTERNS):
        for b in edge_boundaries(i):
            at = b + delta - (len(pat) if kind == "end" else 0)
            data[at: at + len(pat)] = pat
    return [bytes(data)], 0


def _starts_at_edges(delta):
    """Sessions that start at boundary + delta, for a step's and a workgroup's boundary and a group's: the
    session before ends in LF CR or LF, the one that starts there with LF LF CR LF LF (its cuts: 2, 5 -- not 1)"""
    out, at = [], 0
    for b in (16 * 3, 64 * 5, STEP, 2 * STEP, GROUP, GROUP + STEP):
        start = b + delta
        fill = start - at
        out.append(b"y" * (fill - 2) + (b"\n\r" if (b // 16) % 2 else b"y\n"))
        out.append(b"\n\n\r\n\nz")
        at = start + 6
    return out, 0


def _fuzz(seed):
    """a few steps of LF / CR / filler soup in sessions of 0..40 bytes, sess_off[0] anywhere in the first group"""
    rng = np.random.default_rng(seed)
    out, total = [], 0
    while total < 3 * STEP + 100:
        k = int(rng.integers(0, 41)) if rng.integers(4) else int(rng.integers(0, 4))
        out.append(bytes(rng.choice(np.frombuffer(b"\n\n\n\r\rx", dtype=np.uint8), size=k).tobytes()))
        total += k
    return out, int(rng.integers(0, 17))


SCAN_STEPS = 1024   # rhp_split.hip kScanThreads: above it the scan gives a thread more than one step's count


def _past_the_scan_edge():
    """SCAN_STEPS + 1 steps of input in three sessions, an empty line every 997 bytes"""
    line = b"x" * 995 + b"\n\n"
    n = (SCAN_STEPS * STEP) // len(line) + 2
    return [line * 400, line * 401, line * (n - 801)], 0


REQ = b"GET /r HTTP/1.1\r\nHost: h\r\n\r\n"
BASE = [REQ * 3, b"GET /lf HTTP/1.1\nX: y\n\n" * 2 + b"GET /partial HTTP/1.1\r\nHo", REQ, b"\r\n" + REQ + b"\n\n\n"]

SETS = {
    "tiny": lambda: ([b"\n", b"\n\n", b"\n\n\n"], 0),
    "tiny_only_1": lambda: ([b"\n"], 0),
    "tiny_only_2": lambda: ([b"\n\n"], 0),
    "tiny_only_3": lambda: ([b"\n\n\n"], 0),
    "end_lf_start_lf": lambda: ([b"ab\n", b"\nxy", b"cd\n", b"\n\nxy"], 0),
    "end_lfcr_start_lf": lambda: ([b"ab\n\r", b"\nxy", b"ab\n\r", b"\n\nxy"], 0),
    "end_lf_start_crlf": lambda: ([b"ab\n", b"\r\nxy", b"\n", b"\r\n\r\nxy"], 0),
    "empty_first": lambda: ([b""] + BASE, 0),
    "empty_last": lambda: (BASE + [b""], 0),
    "empty_middle": lambda: (BASE[:2] + [b""] + BASE[2:], 0),
    "empty_three": lambda: (BASE[:1] + [b"", b"", b""] + BASE[1:] + [b"", b"", b""], 0),
    "empty_only": lambda: ([b""], 7),
    "first_0": lambda: (BASE, 0),
    "first_5": lambda: (BASE, 5),
    "first_16": lambda: (BASE, 16),
    "all_lf_three_steps": lambda: ([b"\n" * (3 * STEP)], 5),
    "all_lf_two_sessions": lambda: ([b"\n" * (STEP + 1), b"\n" * (2 * STEP - 1)], 0),
    "no_lf": lambda: ([b"x" * (2 * STEP + 37)], 0),
    "cr_only": lambda: ([b"\r" * 200, b"\r\r\r"], 3),
    "many_in_one_step": lambda: ([(b"\n\n\nx", b"", b"\n\n", b"\n\r\n\n", b"", b"", b"", b"q")[k % 8] for k in range(2000)], 0),
    "many_empty_at_step_edge": lambda: ([b"x" * (STEP - 1) + b"\n"] + [b""] * 150 + [b"\n\nrest"] + [b""] * 70, 0),
    "ends_on_step": lambda: ([b"a" * (STEP - 2) + b"\n\n"], 0),
    "ends_on_step_then_more": lambda: ([b"a" * (STEP - 2) + b"\n\n", b"\n\nb"], 0),
    "past_the_scan_edge": lambda: _past_the_scan_edge(),
    "no_session": lambda: ([], 0),
    "no_session_at_5": lambda: ([], 5),
}
for _d in DELTAS:
    SETS[f"edges_end_{_d}"] = lambda d=_d: _edges(d, "end")
    SETS[f"edges_start_{_d}"] = lambda d=_d: _edges(d, "start")
    SETS[f"starts_at_edges_{_d}"] = lambda d=_d: _starts_at_edges(d)
for _s in (1, 2, 3, 4):
    SETS[f"fuzz_{_s}"] = lambda s=_s: _fuzz(s)
NAMES = tuple(SETS)


@functools.lru_cache(maxsize=None)
def sessions(name):
    """(the session inputs, sess_off[0]) of a set"""
    return SETS[name]()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(buf, sess_off) of a set, built once; the tests only read them"""
    data, first = sessions(name)
    buf, sess_off = rhp.pack_raw(data, first)
    end = int(sess_off[-1])
    buf[end: end + 8] = 10
    return buf, sess_off
