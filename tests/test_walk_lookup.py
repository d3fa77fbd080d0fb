"""rhp_lookup_walked (include/rhp.h): the header lookup over the slots a response walk left -- the records stay
where rhp_walk_responses or rhp_walk_resume wrote them, and the slot's first byte is slots[i].start.

The expected answers are in tests/golden/walk_lookup.npz, written by tests/golden/make_golden_walk_lookup.py: the
walks stated in plain Python over the compiled reference, and for every head slot the reference's own
http_field_lookup over the header array its phr_parse_response returned, for every call of every set of
tests/walk_lookup_sets.py.  Held to them, every field of every slot, the absent ones included:
  CPU  the host twin rhp_cpu_lookup_walked behind rhp_cpu_walk_responses / rhp_cpu_walk_resume on every set and on
       every round of every chain, with and without RHP_WALK_DEFRAME; the live reference where oracle/_ref/libref.so
       is built; the refusals of rhp_lookup_args.h; records built by hand that each gate of rhp.h has to stop; a
       sanitizer build of the twin as a stand-alone program
  GPU  the kernel behind the walk kernels on the same stream, the records left on the device, fields poisoned first
       and guard bytes on both sides of every buffer; the kernel against the twin on a seeded mix of 512 sessions;
       the hand-built records; n_slots_total 1, 255, 256, 257
"""
from __future__ import annotations

import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
import walk_lookup_sets as wl
import walk_resume_sets as wr
import walk_sets as ws

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "walk_lookup.npz")
OLD_GOLDEN = os.path.join(HERE, "golden", "walk_responses.npz")
LIBREF = os.path.join(os.path.dirname(HERE), "oracle", "_ref", "libref.so")
GUARD = 256
NULL = rhp.RHP_NAME_NULL
DEFRAMES = (0, ws.DEFRAME)


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    g["hdr_lo"] = np.concatenate([[0], np.cumsum(g["num_headers"].astype(np.int64))])
    assert g["hdr_lo"][-1] == len(g["hdr"])
    return g


SET_NAMES = [str(x) for x in golden()["set_name"]]


def absent(n_names, n_slots):
    f = np.zeros((n_names, n_slots), dtype=rhp.FIELDREF_DTYPE)
    f["value_off"] = NULL
    return f


@functools.lru_cache(maxsize=None)
def golden_set(name):
    """(max_headers, flags, resume, names, states before the first call, [call]); a call: dict of buf (u8, RHP_PAD
    zero bytes behind the sessions), sess_off, slot_off (u64 [n + 1]), n_slots, stop [n], fields (FIELDREF_DTYPE
    [n_names, n_slots_total], the expected answer) and, per written slot, where (its index in the call), start, ret,
    result, num_headers and hdrs (u16 [num_headers, 4])"""
    g = golden()
    s = SET_NAMES.index(name)
    n = int(g["set_nsess"][s])
    f0, f1 = int(g["set_first"][s]), int(g["set_first"][s + 1])
    states = g["states_in"][32 * f0: 32 * f1].copy().view(rhp.WALK_STATE_DTYPE) if f1 > f0 else np.zeros(n, dtype=rhp.WALK_STATE_DTYPE)
    text = g["name_text"].tobytes()
    names = tuple(text[int(o): int(o) + int(ln)] for o, ln in g["name_span"][int(g["set_names"][s]): int(g["set_names"][s + 1])])
    calls = []
    for c in range(int(g["set_call"][s]), int(g["set_call"][s + 1])):
        q0, q1, w0, w1 = int(g["call_q"][c]), int(g["call_q"][c + 1]), int(g["call_w"][c]), int(g["call_w"][c + 1])
        assert q1 - q0 == n
        x = {k: g[k][q0:q1].copy() for k in ("len", "cap", "n_slots", "stop")}
        x["buf"] = np.concatenate([g["bytes"][int(g["call_byte"][c]): int(g["call_byte"][c + 1])], np.zeros(ws.RHP_PAD, dtype=np.uint8)])
        x["sess_off"] = np.concatenate([[0], np.cumsum(x["len"].astype(np.uint64))]).astype(np.uint64)
        x["slot_off"] = ws.slot_offsets(x["cap"].astype(np.uint64))
        nt = int(x["slot_off"][-1])
        x["where"] = np.concatenate([int(x["slot_off"][i]) + np.arange(int(x["n_slots"][i])) for i in range(n)] +
                                    [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        assert len(x["where"]) == w1 - w0
        for k in ("start", "ret", "result", "num_headers"):
            x[k] = g[k][w0:w1].copy()
        x["hdrs"] = [g["hdr"][int(g["hdr_lo"][w]): int(g["hdr_lo"][w + 1])] for w in range(w0, w1)]
        f = absent(len(names), nt)
        for h in range(int(g["call_f"][c]), int(g["call_f"][c + 1])):
            f[int(g["f_name"][h]), int(g["f_slot"][h])] = (g["f_off"][h], g["f_len"][h])
        x["fields"] = f
        for a in x.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        calls.append(x)
    return int(g["set_maxh"][s]), int(g["set_flags"][s]), bool(g["set_resume"][s]), names, states, calls


def same_fields(got, want, what):
    """every field of every slot, the absent ones included: an unwritten entry shows as poison"""
    assert got.shape == want.shape, what
    bad = np.argwhere(got != want)
    assert not len(bad), (f"{what}: name {int(bad[0][0])} of slot {int(bad[0][1])} is {got[tuple(bad[0])]}, the reference's "
                          f"{want[tuple(bad[0])]} ({len(bad)} differ)")


def set_plan(name):
    return next(s for s in wl.all_sets() if s[0] == name)


def run_set(name, deframe, walk_once, walk_round, what):
    """every call of the set through the walk and the lookup, chained through the driver, against the file.
      walk_once(buf, sess_off, slot_off, names, max_headers, flags), walk_round(buf, sess_off, slot_off, states, names,
      max_headers, flags) -> (fields, what the walk returns)"""
    _, maxh, flags, resume, deliveries, caps, states, names = set_plan(name)
    calls = golden_set(name)[5]
    if not resume:
        buf, off = ws.pack(deliveries[0])
        fields, _ = walk_once(buf, off, ws.slot_offsets(caps[0]), names, maxh, flags | deframe)
        same_fields(fields, calls[0]["fields"], f"{what} {name}")
        return
    it = iter(range(len(calls)))

    def step(buf, off, sl, st, maxh_, flags_):
        r = next(it)
        fields, out = walk_round(buf, off, sl, st, names, maxh_, flags_ | deframe)
        same_fields(fields, calls[r]["fields"], f"{what} {name} round {r}")
        return out

    wr.walk_rounds(step, deliveries, caps, maxh, flags, states)


def cpu_once(buf, off, sl, names, maxh, flags):
    out = rhp.walk_responses_cpu(buf, off, sl, maxh, flags)
    return rhp.lookup_walked_cpu(out, out[4], off, sl, names, maxh, flags), out


def cpu_round(buf, off, sl, st, names, maxh, flags):
    out = rhp.walk_resume_cpu(buf, off, sl, st, maxh, flags)
    return rhp.lookup_walked_cpu(out, out[4], off, sl, names, maxh, flags), out


def model(buf, bytes_size, sess_off, slot_off, nt, maxh, records, names):
    """rhp.h's rule (rhp_lookup_walked) in plain Python over any records, slot_off non-decreasing"""
    results, slots, msgs, hdrs = records
    ns = len(sess_off) - 1
    out = absent(len(names), nt)
    for i in range(nt):
        owners = [s for s in range(ns) if int(slot_off[s]) <= i]
        if not owners:
            continue
        s = owners[-1]
        lo, hi = int(slot_off[s]), int(slot_off[s + 1])
        if not (lo <= i < hi and hi <= nt and i - lo < int(results["n_slots"][s])):
            continue
        st, ret = int(slots["start"][i]), int(msgs["ret"][i])
        if not (int(slots["result"][i]) == 1 and ret > 0):
            continue
        a, e = int(sess_off[s]), int(sess_off[s + 1])
        if not (a <= st <= e and ret <= e - st and st + ret <= (bytes_size & ~3)):
            continue
        for j, name in enumerate(names):
            for k in range(min(int(msgs["num_headers"][i]), maxh)):
                no, nl, vo, vl = (int(v) for v in hdrs[i, k].tolist())
                if no == NULL or nl != len(name) or no + nl > ret:
                    continue
                if bytes(buf[st + no: st + no + nl]).upper() == bytes(name).upper():   # (bytes.upper maps a..z alone)
                    out[j, i] = (vo, vl)
                    break
    return out


# ---------------------------------------------------------------------------
# CPU


def test_golden_holds_the_sets():
    """the file's sets, names, bytes, offsets, capacities and first states are what tests/walk_lookup_sets.py
    builds, the rounds made by the driver over the host twin; it is no larger than walk_responses.npz"""
    sets = wl.all_sets()
    assert [s[0] for s in sets] == SET_NAMES
    for name, maxh, flags, resume, deliveries, caps, states, names in sets:
        gm, gf, gr, gn, gs, calls = golden_set(name)
        assert (gm, gf, gr, gn, len(calls)) == (maxh, flags, resume, tuple(names), len(deliveries)), name
        assert states is None or (np.ascontiguousarray(states).view(np.uint8) == gs.view(np.uint8)).all(), name
        it = iter(calls)

        def see(buf, off, sl):
            x = next(it)
            assert (buf == x["buf"]).all() and (off == x["sess_off"]).all() and (sl == x["slot_off"]).all(), name

        if not resume:
            see(*ws.pack(deliveries[0]), ws.slot_offsets(caps[0]))
        else:
            wr.walk_rounds(lambda buf, off, sl, st, m, f: (see(buf, off, sl), rhp.walk_resume_cpu(buf, off, sl, st, m, f))[1],
                           deliveries, caps, maxh, flags, states)
    assert os.path.getsize(GOLDEN) <= os.path.getsize(OLD_GOLDEN)


def test_golden_covers():
    """each situation the sets exist for is in the file: a thinned fixture cannot pass silently"""
    seen = dict(first_empty=0, fold_skipped=0, hit64=0, miss65=0, starts=set(), name_at=set(), continuation=0, head_behind=0,
                last_stop=set(), unwritten=0, maxh0=0, capped=0, sixteen=0, duplicate=0)
    for name in SET_NAMES:
        maxh, _, _, names, _, calls = golden_set(name)
        seen["sixteen"] += len(names) == 16
        for x in calls:
            f, buf = x["fields"], x["buf"]
            nt = f.shape[1]
            written = np.zeros(nt, dtype=bool)
            written[x["where"]] = True
            seen["unwritten"] += int((~written).sum())
            assert (f["value_off"][:, ~written] == NULL).all() and (f["value_len"][:, ~written] == 0).all()
            for s in range(len(x["len"])):
                if x["n_slots"][s]:
                    last = int(x["slot_off"][s]) + int(x["n_slots"][s]) - 1
                    w = int(np.flatnonzero(x["where"] == last)[0])
                    head = x["result"][w] == 1 and x["ret"][w] > 0
                    seen["last_stop"].add((int(x["stop"][s]), bool(head)))
            for w, i in enumerate(x["where"]):
                ret, result, recs = int(x["ret"][w]), int(x["result"][w]), x["hdrs"][w]
                present = f["value_off"][:, i] != NULL
                if not (result == 1 and ret > 0):
                    assert not present.any(), (name, int(i))
                    if result == 1 and ret == 0:
                        seen["continuation"] += 1
                        seen["head_behind"] += bool(w + 1 < len(x["where"]) and x["where"][w + 1] == i + 1 and
                                                    (f["value_off"][:, i + 1] != NULL).any())
                    continue
                seen["maxh0"] += maxh == 0
                st = int(x["start"][w])
                rec_name = lambda r: bytes(buf[st + int(r[0]): st + int(r[0]) + int(r[1])]).upper()
                seen["miss65"] += any(int(r[1]) == 65 for r in recs)
                for j in np.flatnonzero(present):
                    vo, vl = int(f["value_off"][j, i]), int(f["value_len"][j, i])
                    k = next(k for k, r in enumerate(recs) if int(r[0]) != NULL and int(r[2]) == vo and rec_name(r) == names[j].upper())
                    assert not any(int(r[0]) != NULL and rec_name(r) == names[j].upper() for r in recs[:k]), "the first match"
                    later = [r for r in recs[k + 1:] if int(r[0]) != NULL and rec_name(r) == names[j].upper()]
                    seen["duplicate"] += bool(later)
                    seen["first_empty"] += vl == 0 and any(int(r[3]) > 0 for r in later)
                    seen["fold_skipped"] += any(int(r[0]) == NULL for r in recs[:k])
                    seen["hit64"] += len(names[j]) == 64
                    seen["starts"].add(st % 16)
                    seen["name_at"].add((st + int(recs[k][0])) % 4)
                seen["capped"] += len(recs) == maxh and maxh > 0
    assert seen["first_empty"] and seen["fold_skipped"] and seen["hit64"] and seen["miss65"] and seen["duplicate"], seen
    assert seen["starts"] == set(range(16)) and seen["name_at"] == set(range(4)), seen
    assert seen["continuation"] and seen["head_behind"] and seen["unwritten"] and seen["maxh0"] and seen["capped"] and seen["sixteen"], seen
    # every stop code's last slot: END, BODY, CLOSE and MORE end on a head or a continuation, HEAD and BAD on a slot that is none
    stops = {s for s, _ in seen["last_stop"]}
    assert stops == set(range(6)), seen["last_stop"]
    assert (rhp.WALK_HEAD, False) in seen["last_stop"] and (rhp.WALK_BAD, False) in seen["last_stop"] and (rhp.WALK_MORE, True) in seen["last_stop"]


@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_cpu_twin_equals_golden(name, deframe):
    run_set(name, deframe, cpu_once, cpu_round, "rhp_cpu_lookup_walked")


def test_cpu_fewer_names_are_the_same_rows():
    """one name, three names: the rows of the sixteen"""
    for name in ("n65", "resume_stops"):
        maxh, flags, resume, names, states, calls = golden_set(name)
        x = calls[0]
        out = (rhp.walk_resume_cpu(x["buf"], x["sess_off"], x["slot_off"], states, maxh, flags) if resume else
               rhp.walk_responses_cpu(x["buf"], x["sess_off"], x["slot_off"], maxh, flags))
        for pick in ((0,), (2, 0, 5), (15,)):
            got = rhp.lookup_walked_cpu(out, out[4], x["sess_off"], x["slot_off"], [names[j] for j in pick], maxh, flags)
            same_fields(got, x["fields"][list(pick)], f"{name} names {pick}")


@pytest.mark.skipif(not os.path.exists(LIBREF), reason="oracle/_ref/libref.so is built where the reference's sources are")
def test_golden_equals_live_reference():
    """the reference's http_field_lookup, run now over every head slot of the file, against the file"""
    from golden.make_golden_frame_messages import composer
    from golden.make_golden_messages import reference
    compose = composer(reference())
    heads = 0
    for name in SET_NAMES:
        maxh, _, _, names, _, calls = golden_set(name)
        for c, x in enumerate(calls):
            buf = x["buf"].copy()
            want = absent(len(names), x["fields"].shape[1])
            owner = np.searchsorted(x["slot_off"], x["where"], side="right") - 1
            for w, i in enumerate(x["where"]):
                if x["result"][w] != 1 or x["ret"][w] <= 0:
                    continue
                st = int(x["start"][w])
                ret, _, _, _, fields = compose(rhp.MSG_RESPONSE, buf, st, int(x["sess_off"][owner[w] + 1]) - st, maxh, list(names))
                assert ret == x["ret"][w], (name, c, int(i))
                want[:, i] = np.array(fields, dtype=rhp.FIELDREF_DTYPE)
                heads += 1
            same_fields(x["fields"], want, f"the file, {name} call {c}")
    assert heads > 2000


def crafted():
    """Records built by hand, each against one gate of rhp.h; [(label, kw of the call, records, names, slots that
    the gate has to make absent)].  The base is a walk of the twin's: three sessions of two heads in three slots."""
    close = ws.resp([b"Connection: close", b"Content-Length: 0"])
    nxt = ws.resp([b"X-Next: 1", b"Content-Length: 0"])
    long_ = ws.length(b"x" * 300)
    sessions, caps = [close + nxt, long_ + close, nxt + close], [3, 3, 3]
    buf, off = ws.pack(sessions)
    sl = ws.slot_offsets(caps)
    names = (b"Connection", b"X-Next", b"Content-Length", wl.NAME64)
    maxh = 2
    base = tuple(a.copy() for a in rhp.walk_responses_cpu(buf, off, sl, maxh, ws.TRAILERS)[:4])
    ret = int(base[2]["ret"][0])
    kw = dict(buf=buf, sess_off=off, slot_off=sl, nt=9, bytes_size=buf.size, maxh=maxh)
    cases = [("base", kw, base, names, [])]

    def case(label, gone, **change):
        r = tuple(a.copy() for a in base)
        k = dict(kw)
        for key, f in change.items():
            if key in k:
                k[key] = f(k[key].copy() if isinstance(k[key], np.ndarray) else k[key])
            else:
                f(dict(results=r[0], slots=r[1], msgs=r[2], hdrs=r[3])[key])
        cases.append((label, k, r, names, gone))

    def put(field, at, value):
        def f(a):
            a[field][at] = value
        return f

    def put_off(at, value):
        def f(a):
            a[at] = value
            return a
        return f

    case("n_slots above hi - lo", [2], results=put("n_slots", 0, 7))            # slot 2 holds poison and is then in use: no head
    case("slot_off[s+1] above n_slots_total", [6, 7], slot_off=put_off(3, 10))
    case("start below sess_off[s]", [3], slots=put("start", 3, int(off[1]) - 1))
    case("start + ret past sess_off[s+1]", [1], slots=put("start", 1, int(off[1]) - int(base[2]["ret"][1]) + 1))
    case("start far away", [0, 4], slots=lambda a: (put("start", 0, 2 ** 64 - 1)(a), put("start", 4, 2 ** 63 + 5)(a)))
    st7 = int(base[1]["start"][7])
    case("start + ret past bytes_size & ~3", [7], bytes_size=lambda _: st7 + int(base[2]["ret"][7]) - 1)
    case("name_off + name_len past ret", [], hdrs=lambda a: a.__setitem__((0, 0), (ret - 10, 64, 5, 1)))
    case("name_off far past ret", [], hdrs=lambda a: a.__setitem__((0, 1), (0xFFF0, 10, 5, 1)))
    case("num_headers above max_headers", [], msgs=lambda a: (put("num_headers", 0, 60)(a), put("num_headers", 7, 0xFFFF)(a)))
    case("a continuation and a stop slot in place of heads", [0, 3, 6],
         msgs=put("ret", 0, 0), slots=lambda a: (put("result", 3, 0)(a), put("result", 6, -1)(a)))
    case("ret too long or negative", [0, 1], msgs=lambda a: (put("ret", 0, rhp.RHP_RET_TOOLONG)(a), put("ret", 1, -2)(a)))
    return cases


CRAFTED = crafted()


def crafted_want(kw, records, names, gone, label):
    want = model(kw["buf"], kw["bytes_size"], kw["sess_off"], kw["slot_off"], kw["nt"], kw["maxh"], records, names)
    base = CRAFTED[0]
    if label == "base":
        assert [int(i) for i in np.flatnonzero((want["value_off"] != NULL).any(axis=0))] == [0, 1, 3, 4, 6, 7]
        assert (want["value_off"][3] == NULL).all(), "no message has the 64-byte name"
    for i in gone:
        assert (want["value_off"][:, i] == NULL).all(), (label, i)
    if label.startswith("name_off"):   # a gate inside a head: that record matches nothing, the head's other names stay
        was = model(base[1]["buf"], base[1]["bytes_size"], base[1]["sess_off"], base[1]["slot_off"], 9, 2, base[2], names)
        assert (want[:, 0] != was[:, 0]).sum() == 1 and (want[:, 1:] == was[:, 1:]).all(), label
    return want


@pytest.mark.parametrize("case", CRAFTED, ids=[c[0].replace(" ", "_") for c in CRAFTED])
def test_cpu_crafted_records(case):
    label, kw, records, names, gone = case
    got = rhp.lookup_walked_cpu(records, kw["buf"], kw["sess_off"], kw["slot_off"], names, kw["maxh"], ws.TRAILERS,
                                bytes_size=kw["bytes_size"], n_slots_total=kw["nt"])
    same_fields(got, crafted_want(kw, records, names, gone, label), f"rhp_cpu_lookup_walked, {label}")


@pytest.mark.parametrize("which", ["gpu-library", "host-library"])
def test_refused_arguments(which):
    """-EINVAL before anything is launched or read (the HIP library loads without a GPU).  Only refused calls and
    calls that launch nothing go to the GPU library here"""
    gpu = which == "gpu-library"
    fn = ((lambda w, l: rhp.lib().rhp_lookup_walked(w, l, None)) if gpu else (lambda w, l: rhp.host().rhp_cpu_lookup_walked(w, l)))
    al = lambda nbytes, fill: (lambda r: r[(-r.ctypes.data) % 16:][:nbytes])(np.full(nbytes + 16, fill, dtype=np.uint8))
    buf = al(512, 0)
    buf[: len(ws.HELLO)] = np.frombuffer(ws.HELLO, dtype=np.uint8)
    so = np.array([0, len(ws.HELLO), len(ws.HELLO)], dtype=np.uint64)
    sl = np.array([0, 2, 4], dtype=np.uint64)
    msgs, hdrs, slots, results, fields = al(64, 0x77), al(4 * 4 * 8, 0x77), al(128, 0x77), al(32, 0x77), al(4 * 16 * 4, 0x77)
    results[:] = 0   # n_slots 0: no slot is in use
    text, nm, _ = rhp.classify_tables([b"Content-Length", b"x" * 64])
    p = lambda a: a.ctypes.data
    KEEP = object()

    def call(l=KEEP, lk=None, **kw):
        a = dict(bytes=p(buf), bytes_rw=p(buf), bytes_size=512, sess_off=p(so), slot_off=p(sl), n_sessions=2, n_slots_total=4,
                 max_headers=4, flags=0, msgs=p(msgs), hdrs=p(hdrs), slots=p(slots), results=p(results))
        a.update(kw)
        b = dict(text=p(text), names=p(nm), n_names=2, reserved=0, fields=p(fields))
        b.update(lk or {})
        lookup = rhp.WalkLookup(*(b[k] for k, _ in rhp.WalkLookup._fields_))
        return fn(ctypes.byref(rhp.WalkBatch(*(a[k] for k, _ in rhp.WalkBatch._fields_))), ctypes.byref(lookup) if l is KEEP else l)

    E = -22
    assert fn(None, ctypes.byref(rhp.WalkLookup(p(text), p(nm), 2, 0, p(fields)))) == E and call(l=None) == E
    for k in ("bytes", "sess_off", "slot_off", "results", "msgs", "slots", "hdrs"):
        assert call(**{k: None}) == E, k
    assert call(max_headers=rhp.RHP_MAX_HEADERS + 1) == E and call(n_slots_total=2 ** 32 - 1, max_headers=2) == E
    assert call(flags=8) == E and call(bytes_size=rhp.RHP_PAD - 1) == E
    assert call(flags=ws.DEFRAME, bytes_rw=None) == E and call(flags=ws.DEFRAME, bytes_rw=p(buf) + 16) == E
    for k in ("text", "names", "fields"):
        assert call(lk={k: None}) == E, k
    assert call(lk=dict(reserved=1)) == E and call(lk=dict(n_names=0)) == E and call(lk=dict(n_names=rhp.CLASSIFY_MAX_NAMES + 1)) == E
    for bad in ([b""], [b"a", b""], [b"y" * 65]):
        t2, n2, _ = rhp.classify_tables(bad)
        n2 = n2 if len(n2) else np.zeros((1, 2), dtype=np.uint32)
        assert call(lk=dict(text=p(t2), names=p(n2), n_names=len(bad))) == E, bad
    assert call(n_sessions=0, flags=8) == E and call(n_sessions=0, lk=dict(reserved=1)) == E and call(n_slots_total=0, lk=dict(n_names=0)) == E, \
        "the rules come before the empty call"
    if gpu:   # the device's alone: whole-record loads, whole-field stores
        for k, a in (("bytes", buf), ("msgs", msgs), ("slots", slots), ("results", results)):
            assert call(**{k: p(a) + 8}) == E, k
        assert call(hdrs=p(hdrs) + 4) == E and call(lk=dict(fields=p(fields) + 2)) == E
    assert (fields == 0x77).all(), "a refused call writes nothing"
    # accepted, and nothing is launched: no slot, or no session to own one -- fields is not touched
    assert call(n_slots_total=0, msgs=None, hdrs=None, slots=None) == 0 and call(n_sessions=0) == 0
    assert call(n_sessions=0, bytes=None, bytes_rw=None, sess_off=None, slot_off=None, msgs=None, hdrs=None, slots=None, results=None,
                bytes_size=0) == 0
    assert (fields == 0x77).all()
    if gpu:
        return
    # accepted by the host twin: any alignment; every slot absent (no session wrote one)
    odd = np.full(4 * 2 * 4 + 1, 0x77, dtype=np.uint8)
    assert call(lk=dict(fields=p(odd) + 1), bytes_rw=None) == 0 and odd[0] == 0x77
    assert (odd[1:].copy().view(rhp.FIELDREF_DTYPE) == absent(2, 4).reshape(-1)).all()


def test_host_twin_asan_ubsan_clean():
    """`make walk-lookup-asan`: a stand-alone program over the host sources (tests/walk_lookup_host_test.c) that
    runs the calls of the golden file with the host twins"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(rhp.__file__)), "csrc")
    out = subprocess.run(["make", "-s", "-C", csrc, "walk-lookup-asan"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "walk_lookup_host_test OK" in out.stdout


# ---------------------------------------------------------------------------
# GPU: the kernel behind the walk kernels, against the golden file and against the twin


def gpu_once(buf, off, sl, names, maxh, flags):
    return rhp.lookup_walked_gpu(buf, off, sl, names, maxh, flags, guard=GUARD)


def gpu_round(buf, off, sl, st, names, maxh, flags):
    return rhp.lookup_walked_gpu(buf, off, sl, names, maxh, flags, guard=GUARD, states=st, resume=True)


@pytest.mark.gpu
@pytest.mark.parametrize("deframe", DEFRAMES)
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_equals_golden(name, deframe):
    """the walk and the lookup on one stream, the records left on the device (a chain's states too); fields
    poisoned first, guard bytes beside bytes, msgs, hdrs, slots, results, states and fields"""
    run_set(name, deframe, gpu_once, gpu_round, "rhp_lookup_walked")


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [ws.TRAILERS, ws.TRAILERS | ws.DEFRAME | ws.NONE_EMPTY])
def test_gpu_equals_twin_on_a_random_mix(flags):
    deliveries, caps = wr.random_mix(512, 20261020)
    names = wl.FIXED_NAMES
    want, got = [], []
    wr.walk_rounds(lambda *a: (lambda f, out: (want.append(f), out)[1])(*cpu_round(*a[:4], names, *a[4:])), deliveries, caps, 8, flags)
    wr.walk_rounds(lambda *a: (lambda f, out: (got.append(f), out)[1])(*gpu_round(*a[:4], names, *a[4:])), deliveries, caps, 8, flags)
    assert len(want) == len(got) == 3
    present = 0
    for r, (w, g) in enumerate(zip(want, got)):
        same_fields(g, w, f"the kernel against the host twin, round {r}")
        present += int((w["value_off"] != NULL).sum())
    assert present > 1000


@pytest.mark.gpu
@pytest.mark.parametrize("case", CRAFTED, ids=[c[0].replace(" ", "_") for c in CRAFTED])
def test_gpu_crafted_records(case):
    """the hand-built records copied to the device, what lies behind them and every slot not in use 0xC3, msgs,
    hdrs and slots between guard bytes"""
    label, kw, records, names, gone = case
    got, _ = rhp.lookup_walked_gpu(kw["buf"], kw["sess_off"], kw["slot_off"], names, kw["maxh"], ws.TRAILERS, guard=GUARD,
                                   records=records, bytes_size=kw["bytes_size"], n_slots_total=kw["nt"])
    same_fields(got, crafted_want(kw, records, names, gone, label), f"rhp_lookup_walked, {label}")


@pytest.mark.gpu
@pytest.mark.parametrize("nt", [1, 255, 256, 257])
def test_gpu_slot_counts(nt):
    """n_slots_total at the block's edges: the sessions of n257 that fit, the last one's slots cut to the count;
    against the twin and against rhp.h's rule in plain Python"""
    maxh, flags, _, names, _, calls = golden_set("n257")
    x = calls[0]
    n = int(np.searchsorted(x["slot_off"], nt, side="left"))
    off, sl = x["sess_off"][: n + 1].copy(), x["slot_off"][: n + 1].copy()
    sl[-1] = nt
    buf = np.concatenate([x["buf"][: int(off[-1])], np.zeros(ws.RHP_PAD, dtype=np.uint8)])
    want, out = cpu_once(buf, off, sl, names, maxh, flags)
    same_fields(want, model(buf, buf.size, off, sl, nt, maxh, out[:4], names), f"the twin against the rule, {nt} slots")
    got, _ = gpu_once(buf, off, sl, names, maxh, flags)
    assert got.shape == (16, nt)
    same_fields(got, want, f"the kernel against the host twin, {nt} slots")
    whole = int(sl[n - 1]) if n > 1 else 0   # the sessions before the last keep the file's answers
    same_fields(got[:, :whole], x["fields"][:, :whole], f"the kernel against the file, {nt} slots")
