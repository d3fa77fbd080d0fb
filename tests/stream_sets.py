"""The calls of tests/test_gpu_streams.py: every stream-taking entry point of include/rhp.h as a Case, with a decoy
input A and the real input B of identical shapes (the same counts, buffer sizes and table sizes), both valid.

A Case states its call once: the device inputs of a side as flat u8 arrays (the buffers the call writes in place
among them), the sizes of its pure outputs and of `work`, the poison they hold first, the host twin's answer as a
dict of arrays, the same dict made from the device buffers, and the launch itself on an explicit stream.  A launch
returns every host object it handed to the library -- tables, the date, the argument structs -- so that the test can
overwrite them once the call has returned.

B is A with its sessions (messages, requests, responses) rotated by one: every count and size stays, every offset
and every answer moves.  The inputs that earlier calls leave (records, session results, route[], slots, states) are
the host twins', for each side.  Nothing here touches a GPU.
"""
import ctypes
import functools
import types

import numpy as np

import libreactorng_amd as rhp
import batches
import decode_chunked_sets as dcs
import forward_sets as fs
import walk_sets as ws

VP = ctypes.c_void_p
RM = rhp.LAYOUT_REQUEST_MAJOR


def u8(a):
    """a flat u8 copy of an array's bytes"""
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()


def rot(items, which):
    items = list(items)
    return items if which == "A" else items[1:] + items[:1]


def ptr(t):
    """the address of a device tensor or of a host array"""
    return rhp._addr(t)


def cbytes(b: bytes):
    """bytes in a buffer the caller owns and may overwrite: (the buffer, its char pointer)"""
    buf = ctypes.create_string_buffer(bytes(b), max(len(b), 1))
    return buf, ctypes.cast(buf, ctypes.c_char_p)


def check_rc(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {rc}")


def zero_where(a, keep):
    """a copy of a structured array with the elements outside `keep` zeroed"""
    a = a.copy()
    a[~keep] = np.zeros((), dtype=a.dtype)
    return a


class Side:
    """one input of a case: `inputs` name -> u8 array (what the device tensors hold), `want` name -> array (the twin's
    answer), and whatever the launch needs beside the tensors"""

    def __init__(self, inputs, want, **more):
        self.inputs, self.want = inputs, want
        self.__dict__.update(more)


class Case:
    name = ""
    poison = 0xC3
    multi = False        # several launches and a caller-supplied work area: run with two batches in flight too
    tables = False       # host tables travel in the launch

    def __init__(self):
        self._sides = {}

    def side(self, which) -> Side:
        if which not in self._sides:
            self._sides[which] = self.build(which)
        return self._sides[which]

    def outs(self) -> dict:
        """name -> bytes of every pure output and of work (the same for both sides)"""
        raise NotImplementedError

    def build(self, which) -> Side:
        raise NotImplementedError

    def launch(self, T, side, stream) -> list:
        """the call over the tensors T (name -> u8 device tensor) on `stream`; returns the host objects handed over"""
        raise NotImplementedError

    def got(self, raw, side) -> dict:
        """the dict of `want` from the device buffers' bytes (name -> u8 array)"""
        raise NotImplementedError


# ---------------------------------------------------------------------------
# rhp_parse_messages, rhp_frame_messages, rhp_decode_chunked

MSG_MAXH = 8
MESSAGES = (ws.HELLO, ws.CHUNKS, ws.NO_CONTENT, ws.SWITCHING, ws.BARE, ws.SHORT, ws.CHUNKS_T, ws.NOT_MODIFIED,
            ws.HELLO[:30], b"HTTP/2.0 200 OK\r\n\r\n", ws.resp([b"Bad Name: x"]),
            ws.resp([b"H%d: v" % i for i in range(MSG_MAXH + 1)]), ws.resp([b"Content-Length: 3", b"X-Long: a", b" folded"], b"abc"))
MSG_NAMES = (b"Content-Type", b"Connection", b"Server", b"ETag")


def message_views(msgs, hdrs):
    """what rhp.h specifies of the two record arrays: ret; the record where ret > 0; the header rows below num_headers"""
    ok = msgs["ret"] > 0
    rows = np.arange(hdrs.shape[1])[None, :] < np.where(ok, msgs["num_headers"], 0)[:, None]
    return {"ret": msgs["ret"].copy(), "msgs": zero_where(msgs, ok), "hdrs": zero_where(hdrs, rows)}


@functools.lru_cache(maxsize=None)
def message_batch(which, n=257):
    buf, off = batches.pack(rot([MESSAGES[(i * 5 + i // 13) % len(MESSAGES)] for i in range(n)], which))
    msgs, hdrs = rhp.parse_messages_cpu(buf, off, rhp.MSG_RESPONSE, MSG_MAXH)
    return buf, off, msgs, hdrs


class ParseMessages(Case):
    name, poison, n = "parse_messages", rhp.MSG_POISON, 257

    def outs(self):
        return {"msgs": 16 * self.n, "hdrs": 8 * self.n * MSG_MAXH}

    def build(self, which):
        buf, off, msgs, hdrs = message_batch(which)
        return Side({"bytes": u8(buf), "off": u8(off)}, message_views(msgs, hdrs), size=buf.size)

    def launch(self, T, side, stream):
        rhp.parse_messages_device(T["bytes"], side.size, T["off"], self.n, rhp.MSG_RESPONSE, MSG_MAXH, RM, T["msgs"], T["hdrs"],
                                  stream=stream)
        return []

    def got(self, raw, side):
        return message_views(*rhp._msg_result(raw["msgs"], raw["hdrs"], self.n, MSG_MAXH, RM))


class FrameMessages(Case):
    name, poison, n, tables = "frame_messages", rhp.FRAME_POISON, 257, True

    def outs(self):
        return {"frames": 16 * self.n, "fields": 4 * len(MSG_NAMES) * self.n, "decoders": 16 * self.n}

    def build(self, which):
        buf, off, msgs, hdrs = message_batch(which)
        frames, fields, dec = rhp.frame_messages_cpu(buf, off, rhp.MSG_RESPONSE, msgs, hdrs, MSG_NAMES, MSG_MAXH, consume_trailer=1)
        return Side({"bytes": u8(buf), "off": u8(off), "msgs": u8(msgs), "hdrs": u8(hdrs)},
                    {"frames": frames, "fields": fields, "decoders": dec}, size=buf.size)

    def launch(self, T, side, stream):
        text, nm, _ = rhp.classify_tables(MSG_NAMES)
        b = rhp.MsgBatch(ptr(T["bytes"]), ptr(T["off"]), side.size, self.n, MSG_MAXH, rhp.MSG_RESPONSE, RM, ptr(T["msgs"]),
                         ptr(T["hdrs"]), None)
        f = rhp.FrameArgs(ptr(text), ptr(nm), len(nm), 1, ptr(T["fields"]), ptr(T["frames"]), ptr(T["decoders"]), 0)
        check_rc(rhp.lib().rhp_frame_messages(ctypes.byref(b), ctypes.byref(f), VP(stream.cuda_stream)), "rhp_frame_messages")
        return [text, nm, b, f]

    def got(self, raw, side):
        frames, fields, dec = rhp._frame_result(raw["frames"], raw["fields"], raw["decoders"], self.n, len(MSG_NAMES))
        return {"frames": frames, "fields": fields, "decoders": dec}


class DecodeChunked(Case):
    name, poison, n = "decode_chunked", rhp.CHUNKED_POISON, 65

    def outs(self):
        return {"results": 16 * self.n}

    def build(self, which):
        streams = rot(dcs.batch_of(self.n), which)
        buf, off = batches.pack([s.pieces[0] for s in streams])
        dec = np.frombuffer(b"".join(dcs.fresh_decoder(s) for s in streams), dtype=rhp.CHUNKED_DTYPE)
        results, after, left = rhp.decode_chunked_cpu(buf, off, dec)
        return Side({"bytes": u8(buf), "off": u8(off), "decoders": u8(dec)},
                    {"results": results, "decoders": after, "bytes": left}, size=buf.size)

    def launch(self, T, side, stream):
        rhp.decode_chunked_device(T["bytes"], side.size, T["off"], self.n, T["decoders"], T["results"], stream=stream)
        return []

    def got(self, raw, side):
        return {"results": raw["results"].view(rhp.CHUNKED_RESULT_DTYPE), "decoders": raw["decoders"].view(rhp.CHUNKED_DTYPE),
                "bytes": raw["bytes"]}


# ---------------------------------------------------------------------------
# the response walk and what runs over its slots

WALK_MAXH, WALK_FLAGS = 8, ws.TRAILERS | ws.DEFRAME
WALK_NAMES = (b"Content-Length", b"Transfer-Encoding", b"Server", b"ETag")
RELAY_DROP = (b"Connection", b"Upgrade", b"Server")
POISON64 = int(np.frombuffer(bytes([rhp.WALK_POISON]) * 8, dtype=np.uint64)[0])


@functools.lru_cache(maxsize=None)
def walk_input(which, n):
    """(buf, sess_off, slot_off) of walk_sets.geometry(n), rotated for B"""
    s, k = ws.geometry(n)
    buf, so = ws.pack(rot(s, which))
    return buf, so, ws.slot_offsets(rot(k, which))


def walk_views(results, slots, msgs, hdrs, bytes_out):
    """what rhp.h specifies of a walk's outputs (an unwritten slot holds the poison on both sides)"""
    ok = (slots["start"] != POISON64) & (msgs["ret"] > 0)
    rows = np.arange(hdrs.shape[1])[None, :] < np.where(ok, msgs["num_headers"], 0)[:, None]
    return {"results": results, "slots": slots, "ret": msgs["ret"].copy(), "msgs": zero_where(msgs, ok), "hdrs": zero_where(hdrs, rows),
            "bytes": bytes_out}


class WalkCase(Case):
    poison, n_sessions = rhp.WALK_POISON, 65

    def shape(self):
        buf, so, sl = walk_input("A", self.n_sessions)
        return len(so) - 1, int(sl[-1]), buf.size

    def record_outs(self):
        ns, nt, _ = self.shape()
        return dict(zip(rhp._WALK_RECORDS, rhp._walk_record_sizes(ns, nt, WALK_MAXH)))

    def batch_inputs(self, which):
        buf, so, sl = walk_input(which, self.n_sessions)
        return {"bytes": u8(buf), "sess_off": u8(so), "slot_off": u8(sl)}

    def batch(self, T):
        """the twelve arguments every walk_*_device function starts with"""
        ns, nt, size = self.shape()
        return (T["bytes"], size, T["sess_off"], T["slot_off"], ns, nt, WALK_MAXH, WALK_FLAGS, T["msgs"], T["hdrs"], T["slots"],
                T["results"])

    def walk_got(self, raw):
        ns, nt, _ = self.shape()
        return walk_views(*rhp._walk_result(raw["results"], raw["slots"], raw["msgs"], raw["hdrs"], raw["bytes"], ns, nt, WALK_MAXH))


class WalkResponses(WalkCase):
    name = "walk_responses"

    def outs(self):
        return self.record_outs()

    def build(self, which):
        return Side(self.batch_inputs(which), walk_views(*rhp.walk_responses_cpu(*walk_input(which, self.n_sessions), WALK_MAXH, WALK_FLAGS)))

    def launch(self, T, side, stream):
        rhp.walk_responses_device(*self.batch(T), stream=stream)
        return []

    def got(self, raw, side):
        return self.walk_got(raw)


def states_before(which, n):
    """the states a round over the side's sessions left (any state is a valid input of the resumed walk)"""
    buf, so, sl = walk_input(which, n)
    return rhp.walk_resume_cpu(buf, so, sl, None, WALK_MAXH, ws.TRAILERS)[5].copy()


class WalkResume(WalkCase):
    name = "walk_resume"

    def outs(self):
        return self.record_outs()

    def build(self, which):
        st = states_before(which, self.n_sessions)
        out = rhp.walk_resume_cpu(*walk_input(which, self.n_sessions), st, WALK_MAXH, WALK_FLAGS)
        want = walk_views(*out[:5])
        want["states"] = out[5]
        inputs = self.batch_inputs(which)
        inputs["states"] = u8(st)
        return Side(inputs, want)

    def launch(self, T, side, stream):
        rhp.walk_resume_device(*self.batch(T), T["states"], stream=stream)
        return []

    def got(self, raw, side):
        out = self.walk_got(raw)
        out["states"] = raw["states"].view(rhp.WALK_STATE_DTYPE)
        return out


class WalkAnswers(WalkCase):
    name, per_session = "walk_answers", 3

    def outs(self):
        ns, nt, _ = self.shape()
        return dict(self.record_outs(), answered=4 * ns, slot_req=4 * nt)

    def queue(self, which):
        ns = self.shape()[0]
        req_off = (np.arange(ns + 1) * self.per_session).astype(np.uint32)
        q = np.arange(ns * self.per_session)
        return req_off, rhp.head_bits_of(q % 3 == 0 if which == "A" else q % 2 == 0)

    def build(self, which):
        req_off, bits = self.queue(which)
        out = rhp.walk_answers_cpu(*walk_input(which, self.n_sessions), req_off, bits, max_headers=WALK_MAXH, flags=WALK_FLAGS)
        want = walk_views(*out[:5])
        want["answered"], want["slot_req"] = out[5], out[6]
        inputs = self.batch_inputs(which)
        inputs["req_off"], inputs["head_bits"] = u8(req_off), u8(bits)
        return Side(inputs, want, n_req=int(req_off[-1]))

    def launch(self, T, side, stream):
        rhp.walk_answers_device(*self.batch(T), None, T["req_off"], T["head_bits"], side.n_req, T["answered"], T["slot_req"],
                                stream=stream)
        return []

    def got(self, raw, side):
        out = self.walk_got(raw)
        out["answered"], out["slot_req"] = raw["answered"].view(np.uint32), raw["slot_req"].view(np.uint32)
        return out


class WalkedCase(WalkCase):
    """a call over the records a walk left: they are inputs, from the host twin's walk"""

    def walked(self, which):
        buf, so, sl = walk_input(which, self.n_sessions)
        results, slots, msgs, hdrs, left = rhp.walk_responses_cpu(buf, so, sl, WALK_MAXH, WALK_FLAGS)
        inputs = {"bytes": u8(left), "sess_off": u8(so), "slot_off": u8(sl), "results": u8(results), "slots": u8(slots),
                  "msgs": u8(msgs), "hdrs": u8(hdrs)}
        return (results, slots, msgs, hdrs), left, so, sl, inputs

    def walk_batch(self, T):
        return rhp._walk_batch(*self.batch(T))


class LookupWalked(WalkedCase):
    name, poison, tables = "lookup_walked", rhp.LOOKUP_POISON, True

    def outs(self):
        return {"fields": 4 * len(WALK_NAMES) * self.shape()[1]}

    def build(self, which):
        records, left, so, sl, inputs = self.walked(which)
        return Side(inputs, {"fields": rhp.lookup_walked_cpu(records, left, so, sl, WALK_NAMES, WALK_MAXH, WALK_FLAGS)})

    def launch(self, T, side, stream):
        text, nm, _ = rhp.classify_tables(WALK_NAMES)
        w = self.walk_batch(T)
        l = rhp.WalkLookup(ptr(text), ptr(nm), len(nm), 0, ptr(T["fields"]))
        check_rc(rhp.lib().rhp_lookup_walked(ctypes.byref(w), ctypes.byref(l), VP(stream.cuda_stream)), "rhp_lookup_walked")
        return [text, nm, w, l]

    def got(self, raw, side):
        return {"fields": rhp._lookup_fields(raw["fields"], len(WALK_NAMES), self.shape()[1])}


def written_out(out_off, out, poison, label):
    """the bytes of `out` below the total; what lies behind them must hold the poison"""
    total = int(out_off[-1])
    assert total <= out.size, f"{label}: the total {total} does not fit out ({out.size} bytes)"
    assert (out[total:] == poison).all(), f"{label}: bytes behind the total were written"
    return out[:total]


class RelayWalked(WalkedCase):
    """more than 4096 slots: two scan tiles and a carry between them"""
    name, poison, tables, multi, n_sessions = "relay_walked", rhp.RELAY_POISON, True, True, 1000

    def out_size(self):
        return max(int(self.side(w).want["out_off"][-1]) for w in "AB") + 64

    def outs(self):
        nt = self.shape()[1]
        assert nt > 4096
        return {"out_off": 8 * (nt + 1), "why": 4 * nt, "out": self.out_size(), "work": 8 * rhp.relay_work_words(nt)}

    def build(self, which):
        records, left, so, sl, inputs = self.walked(which)
        out_off, why, out = rhp.relay_walked_cpu(records, left, so, sl, RELAY_DROP, WALK_MAXH, WALK_FLAGS)
        return Side(inputs, {"out_off": out_off, "why": why, "out": out})

    def launch(self, T, side, stream):
        text, nm, _ = rhp.classify_tables(RELAY_DROP)
        date, date_p = cbytes(rhp.DEFAULT_DATE)
        w = self.walk_batch(T)
        r = rhp.WalkRelay(ptr(text), ptr(nm), len(nm), len(rhp.DEFAULT_DATE), date_p, ptr(T["out_off"]), ptr(T["why"]), ptr(T["out"]),
                          T["out"].numel(), ptr(T["work"]))
        check_rc(rhp.lib().rhp_relay_walked(ctypes.byref(w), ctypes.byref(r), VP(stream.cuda_stream)), "rhp_relay_walked")
        return [text, nm, date, w, r]

    def got(self, raw, side):
        nt = self.shape()[1]
        out_off = raw["out_off"].view(np.uint64)
        return {"out_off": out_off, "why": raw["why"][: 4 * nt].view(np.uint32),
                "out": written_out(out_off, raw["out"], self.poison, self.name)}


# ---------------------------------------------------------------------------
# rhp_write_responses

class WriteResponses(Case):
    """4097 responses: two scan tiles and a carry"""
    name, poison, multi, tables, n = "write_responses", 0xC3, True, True, 4097

    @functools.lru_cache(maxsize=None)
    def batch(self, which):
        arena, resps, fields = rhp.make_responses(self.n, 20261021, "mixed")
        pad = np.full((-len(arena)) % 4, 0xEE, dtype=np.uint8)   # readable to the next 4-byte boundary (rhp.h)
        return np.concatenate([arena, pad]), (resps if which == "A" else np.roll(resps, -1, axis=0)), fields

    def out_size(self):
        return int(self.side("A").want["out_off"][-1]) + 64

    def outs(self):
        return {"out_off": 8 * (self.n + 1), "out": self.out_size(), "work": 8 * ((self.n + 4095) // 4096 + 1)}

    def build(self, which):
        from oracle_util import oracle_write_responses
        arena, resps, fields = self.batch(which)
        out, off = oracle_write_responses(arena, resps, fields)
        return Side({"arena": u8(arena), "resps": u8(resps), "fields": u8(fields)}, {"out_off": np.asarray(off, dtype=np.uint64), "out": out})

    def launch(self, T, side, stream, n=None):
        date, date_p = cbytes(rhp.DEFAULT_DATE)
        d = rhp.RespBatch(ptr(T["arena"]), ptr(T["resps"]), ptr(T["fields"]), self.n if n is None else n, len(rhp.DEFAULT_DATE), date_p,
                          ptr(T["out_off"]), ptr(T["out"]), T["out"].numel(), ptr(T["work"]))
        check_rc(rhp.lib().rhp_write_responses(ctypes.byref(d), VP(stream.cuda_stream)), "rhp_write_responses")
        return [date, d]

    def got(self, raw, side):
        out_off = raw["out_off"].view(np.uint64)
        return {"out_off": out_off, "out": written_out(out_off, raw["out"], self.poison, self.name)}


# ---------------------------------------------------------------------------
# rhp_split_sessions

class SplitSessions(Case):
    """one step of the mark kernel plus a few bytes"""
    name, poison, multi = "split_sessions", rhp.SPLIT_POISON, True
    REQ = b"GET /r HTTP/1.1\r\nHost: h\r\n\r\n"

    @functools.lru_cache(maxsize=None)
    def packed(self, which):
        s = [self.REQ * 3, b"GET /lf HTTP/1.1\nX: y\n\n" * 2 + b"GET /partial HTTP/1.1\r\nHo", self.REQ, b"\r\n" + self.REQ + b"\n\n\n",
             b"", self.REQ * 9, b"POST /p HTTP/1.1\r\nContent-Length: 4\r\n\r\n\r\n\r\n"]
        fill = rhp.SPLIT_STEP_BYTES + 5 - sum(len(x) for x in s)
        # (A's filler holds one empty line more: n_pieces differs between the sides, under one cap)
        s.append(b"x" * (fill - 10) + (b"\n\n" if which == "A" else b"yy") + b"x" * 8)
        return rhp.pack_raw(rot(s, which))

    @functools.lru_cache(maxsize=None)
    def shape(self):
        """(bytes_end, n_sessions, the cap both sides share: the larger n_pieces, from a count-only call each)"""
        buf, so = self.packed("A")
        return int(so[-1]), len(so) - 1, max(rhp.split_sessions_cpu(*self.packed(w), 0)[0] for w in "AB")

    def outs(self):
        end, ns, cap = self.shape()
        assert rhp.SPLIT_STEP_BYTES < end < rhp.SPLIT_STEP_BYTES + 16
        return {"n_pieces": 8, "offsets": 8 * (cap + 1), "sessions": 8 * ns, "work": 8 * rhp.split_work_words(end, ns)}

    def build(self, which):
        buf, so = self.packed(which)
        n_pieces, offsets, sessions = rhp.split_sessions_cpu(buf, so, self.shape()[2])
        return Side({"bytes": u8(buf), "sess_off": u8(so)},
                    {"n_pieces": np.array([n_pieces], dtype=np.uint64), "offsets": offsets, "sessions": sessions})

    def launch(self, T, side, stream):
        end, ns, cap = self.shape()
        o = rhp.SplitOut(ptr(T["n_pieces"]), ptr(T["offsets"]), cap, ptr(T["sessions"]), ptr(T["work"]))
        check_rc(rhp.lib().rhp_split_sessions(VP(ptr(T["bytes"])), end, VP(ptr(T["sess_off"])), ns, ctypes.byref(o),
                                              VP(stream.cuda_stream)), "rhp_split_sessions")
        return [o]

    def got(self, raw, side):
        return {"n_pieces": raw["n_pieces"].view(np.uint64), "offsets": raw["offsets"].view(np.uint64),
                "sessions": raw["sessions"].view(rhp.SESSION_DTYPE)}


# ---------------------------------------------------------------------------
# rhp_parse_batch and rhp_classify_batch

PARSE_MAXH = 16
REQUESTS = (fs.GET, fs.TFB, fs.STATIC, fs.HEAD, fs.BAD, fs.PARTIAL, fs.FOLD, fs.post(5), fs.DROPS, fs.FIVE, fs.NOWHERE, fs.CHUNKED,
            fs.post(300), fs.CHUNKED_EMPTY, fs.NO_FRAMING, b"\r\n" + fs.GET, fs.CL_SPLIT)
BATCH_NAMES = (b"Host", b"Connection", b"Content-Length", b"Transfer-Encoding")


@functools.lru_cache(maxsize=None)
def request_batch(which, mode, n=257):
    buf, off = batches.pack(rot([REQUESTS[(i * 7 + i // 17) % len(REQUESTS)] for i in range(n)], which))
    res, _ = rhp.emulate(buf, off, PARSE_MAXH, mode, RM)
    return buf, off, res


def parse_views(res, mode):
    reqs, hdrs, http = rhp.canonical(res, mode)
    out = {"reqs": reqs, "hdrs": hdrs}
    if mode == rhp.MODE_HTTP:
        out["http"], out["bytes"] = http, res.bytes_out
    return out


class ParseBatch(Case):
    poison, n = 0xFF, 257

    def __init__(self, mode):
        super().__init__()
        self.mode = mode
        self.name = "parse_batch_http" if mode == rhp.MODE_HTTP else "parse_batch_phr"

    def outs(self):
        return {"reqs": rhp.reqs_bytes(self.n, RM), "hdrs": rhp.hdrs_bytes(self.n, PARSE_MAXH, RM), "http": rhp.http_bytes(self.n, self.mode, RM)}

    def build(self, which):
        buf, off, res = request_batch(which, self.mode)
        # (work holds zeros before a launch, as DeviceBatch leaves it: an input, the same for both sides)
        return Side({"bytes": u8(buf), "off": u8(off), "work": np.zeros(4 * rhp.RHP_WORK_WORDS, dtype=np.uint8)},
                    parse_views(res, self.mode), size=buf.size)

    def desc(self, T, side):
        return rhp.Batch(ptr(T["bytes"]), ptr(T["bytes"]), ptr(T["off"]), side.size, self.n, PARSE_MAXH, self.mode, RM, ptr(T["reqs"]),
                         ptr(T["hdrs"]), ptr(T["http"]), ptr(T["work"]), 0, 0, None)

    def launch(self, T, side, stream):
        d = self.desc(T, side)
        check_rc(rhp.lib().rhp_parse_batch(ctypes.byref(d), VP(stream.cuda_stream)), "rhp_parse_batch")
        return []

    def got(self, raw, side):
        n = self.n
        res = rhp.Result(raw["reqs"][: 16 * n].view(rhp.REQ_DTYPE), raw["hdrs"].view(rhp.HDR_DTYPE).reshape(n, PARSE_MAXH),
                         raw["http"][: 24 * n].view(rhp.HTTP_DTYPE) if self.mode == rhp.MODE_HTTP else None, raw["bytes"])
        return parse_views(res, self.mode)


class ClassifyBatch(Case):
    name, tables, n = "classify_batch", True, 257

    def outs(self):
        return {"fields": 4 * len(BATCH_NAMES) * self.n, "route": 2 * self.n}

    def build(self, which):
        buf, off, res = request_batch(which, rhp.MODE_PHR)
        fields, route = rhp.classify_cpu(res, BATCH_NAMES, fs.ROUTES)
        return Side({"bytes": u8(buf), "off": u8(off), "reqs": u8(res.raw_reqs), "hdrs": u8(res.raw_hdrs)},
                    {"fields": fields, "route": route}, size=buf.size)

    def launch(self, T, side, stream):
        text, nm, rt = rhp.classify_tables(BATCH_NAMES, fs.ROUTES)
        d = rhp.Batch(ptr(T["bytes"]), ptr(T["bytes"]), ptr(T["off"]), side.size, self.n, PARSE_MAXH, rhp.MODE_PHR, RM, ptr(T["reqs"]),
                      ptr(T["hdrs"]), None, None, 0, 0, None)
        c = rhp.Classify(ptr(text), ptr(nm), ptr(rt), len(nm), len(rt), ptr(T["fields"]), ptr(T["route"]))
        check_rc(rhp.lib().rhp_classify_batch(ctypes.byref(d), ctypes.byref(c), VP(stream.cuda_stream)), "rhp_classify_batch")
        return [text, nm, rt, d, c]

    def got(self, raw, side):
        fields, route = rhp._classify_out(raw["fields"], raw["route"], len(BATCH_NAMES), self.n)
        return {"fields": fields, "route": route}


# ---------------------------------------------------------------------------
# the session round: fix-up, classify, dense pack, gather, reply, forward

ROUND_MAXH = 16
ROUND_NAMES = (b"Host", b"Connection", b"Content-Length", b"Transfer-Encoding")
STATIC_MASK = 0b1010   # /static and /host are answered; fs.FORWARD_MASK forwards /up and /plaintext
WIDE_SESSION = b"\r\n" + fs.GET + fs.STATIC                                  # a leading CRLF: a wide slot
NARROW_SESSION = fs.GET.replace(b"upstream", b"upstream12") + fs.STATIC
assert len(WIDE_SESSION) == len(NARROW_SESSION)
SESSIONS = (fs.GET, fs.GET * 3, fs.TFB * 5 + fs.GET, fs.post(0), fs.post(1) + fs.post(300), fs.CHUNKED, fs.GET + fs.CHUNKED.replace(b"hello", b"HOWDY") + fs.GET,
            fs.HEAD, fs.GET + fs.HEAD + fs.LOWER_HEAD + fs.HEAD, fs.DROPS, fs.GET * 2 + fs.PARTIAL, fs.GET + fs.post(5) + fs.BAD + fs.GET,
            fs.STATIC * 2, fs.HOST + fs.GET, fs.GET + fs.STATIC + fs.NOWHERE + fs.GET + fs.HOST + fs.post(7) + fs.FOLD + fs.GET,
            fs.CL_SPLIT + fs.GET, b"", WIDE_SESSION, fs.STATIC + fs.HOST + fs.STATIC + fs.BAD)
IMAGES = (b"HTTP/1.1 200 OK\r\nContent-Length: 2\r\n\r\nup", b"HTTP/1.1 200 OK\r\nServer: s\r\nContent-Length: 6\r\n\r\nstatic",
          b"HTTP/1.1 204 No Content\r\n\r\n", b"HTTP/1.1 200 OK\r\nContent-Length: 40\r\n\r\n" + b"h" * 40)


class Round:
    """a side's sessions parsed (the kernel's DFA emulation), fixed up (the twin of the kernel's prefix), classified and
    packed on the host: what every call of the device round finds, and leaves"""

    def __init__(self, which, n_sessions):
        sessions = rot([SESSIONS[(i * 5 + i // 19) % len(SESSIONS)] for i in range(n_sessions)], which)
        if which == "B":   # one wide request less, in as many bytes and pieces: the gather's totals differ too
            k = sessions.index(WIDE_SESSION)
            sessions[k] = NARROW_SESSION
            sessions[sessions.index(fs.CHUNKED)] = fs.CHUNKED.replace(b"hello", b"jelly")   # (and the gathered bodies)
        self.buf, self.off, self.sess, _ = rhp.pack_sessions(sessions)
        self.n, self.ns, self.end = len(self.off) - 1, len(self.sess), int(self.off[-1])
        self.b, self.res = rhp.speculative_cpu(self.buf, self.off, ROUND_MAXH, emulate_dfa=True)
        self.parsed = self.records()
        _, self.results, self.starts = rhp.fixup_host(self.b, self.res, self.sess, prefix=True)
        self.fixed = self.records()
        self.fields, self.route = rhp.classify_sessions_cpu(self.b, self.sess, self.results, self.starts, ROUND_NAMES, fs.ROUTES)
        self.dreq, self.hc, self.lens = rhp.pack_dense_cpu(self.res, self.n, ROUND_MAXH)

    def records(self):
        rw, _, reqs, hdrs, http = self.res.keep
        return {"bytes": u8(rw), "off": u8(self.off), "reqs": u8(reqs), "hdrs": u8(hdrs), "http": u8(http)}

    def session_inputs(self, *more):
        d = dict(self.fixed, sessions=u8(self.sess), results=u8(self.results), starts=u8(self.starts))
        for k in more:
            d[k] = u8(getattr(self, k))
        return d


@functools.lru_cache(maxsize=None)
def session_round(which, n_sessions):
    return Round(which, n_sessions)


class RoundCase(Case):
    n_sessions = 90   # 257 pieces and more

    def round(self, which) -> Round:
        return session_round(which, self.n_sessions)

    def shape(self):
        r = self.round("A")
        assert (r.n, r.ns, r.buf.size) == (self.round("B").n, r.ns, self.round("B").buf.size) and r.n >= 257
        return r.n, r.ns

    def desc(self, T, side=None):
        r = self.round("A")
        return rhp.Batch(ptr(T["bytes"]), ptr(T["bytes"]), ptr(T["off"]), r.buf.size, r.n, ROUND_MAXH, rhp.MODE_HTTP, RM, ptr(T["reqs"]),
                         ptr(T["hdrs"]), ptr(T["http"]), None, rhp.BATCH_SPECULATIVE, 0, None)


def fixup_views(rec, results, starts, sess, n, end):
    """what two fix-ups of one batch agree on (tests/test_sessions.py assert_same_fixup, every_row=False)"""
    from test_sessions import used_slots   # (the fix-up's own test module: the slots a fix-up filled)
    u = used_slots(sess, results)
    reqs = rec["reqs"][: 16 * n].view(rhp.REQ_DTYPE)[u]
    hdrs = rec["hdrs"][: 8 * n * ROUND_MAXH].view(rhp.HDR_DTYPE).reshape(n, ROUND_MAXH)[u]
    rows = np.arange(ROUND_MAXH)[None, :] < np.where(reqs["ret"] > 0, reqs["num_headers"], 0)[:, None]
    return {"results": results, "starts": starts[u], "reqs": reqs, "http": rec["http"][: 24 * n].view(rhp.HTTP_DTYPE)[u],
            "hdrs": zero_where(hdrs, rows), "bytes": rec["bytes"][:end]}


class FixupSessions(RoundCase):
    name, poison, multi = "fixup_sessions", 0xFF, True

    def outs(self):
        n, ns = self.shape()
        return {"results": 16 * ns, "starts": 8 * n}

    def build(self, which):
        r = self.round(which)
        return Side(dict(r.parsed, sessions=u8(r.sess)), fixup_views(r.fixed, r.results, r.starts, r.sess, r.n, r.end), sess=r.sess, end=r.end)

    def launch(self, T, side, stream):
        n, ns = self.shape()
        rhp.fixup_sessions_device(self.desc(T), T["sessions"], ns, T["results"], T["starts"], stream=stream)
        return []

    def got(self, raw, side):
        n, ns = self.shape()
        return fixup_views(raw, raw["results"].view(rhp.SESSION_RESULT_DTYPE), raw["starts"].view(np.uint64), side.sess, n, side.end)


class ClassifySessions(RoundCase):
    name, poison, multi, tables = "classify_sessions", 0xC3, True, True

    def outs(self):
        n, ns = self.shape()
        return {"fields": 4 * len(ROUND_NAMES) * n, "route": 2 * n}

    def build(self, which):
        r = self.round(which)
        return Side(r.session_inputs(), {"fields": r.fields, "route": r.route})

    def launch(self, T, side, stream):
        n, ns = self.shape()
        tables = rhp.classify_tables(ROUND_NAMES, fs.ROUTES)
        rhp.classify_sessions_device(self.desc(T), T["sessions"], ns, T["results"], T["starts"], T["fields"], T["route"],
                                     tables=tables, stream=stream)
        return list(tables)

    def got(self, raw, side):
        fields, route = rhp._classify_out(raw["fields"], raw["route"], len(ROUND_NAMES), self.shape()[0])
        return {"fields": fields, "route": route}


class PackDense(RoundCase):
    name, poison = "pack_dense", rhp.WIDE_POISON

    def outs(self):
        n, ns = self.shape()
        return {"dreq": 8 * n, "hc": 8 * n, "lens16": 2 * ROUND_MAXH * n}

    def build(self, which):
        r = self.round(which)
        return Side(dict(r.fixed), {"dreq": r.dreq, "hc": r.hc, "lens16": self.used_lens(r.dreq, r.lens)})

    def used_lens(self, dreq, lens16):
        """lens16 [max_headers, n] with the rows past a dense request's num_headers, which are unspecified, zeroed"""
        n = self.shape()[0]
        d = np.asarray(dreq).reshape(n, 8)
        nh = np.where((d[:, 7] & rhp.DENSE_WIDE) == 0, d[:, 5], 0)
        return np.where(np.arange(ROUND_MAXH)[:, None] < nh[None, :], np.asarray(lens16).reshape(ROUND_MAXH, n), 0)

    def launch(self, T, side, stream):
        n, ns = self.shape()
        rhp.pack_dense_device(types.SimpleNamespace(n=n, max_headers=ROUND_MAXH, desc=lambda: self.desc(T)), stream=stream,
                              outs=(T["dreq"], T["hc"], T["lens16"]))
        return []

    def got(self, raw, side):
        return {"dreq": raw["dreq"], "hc": raw["hc"], "lens16": self.used_lens(raw["dreq"], raw["lens16"].view(np.uint16))}


class GatherWide(RoundCase):
    name, poison, multi = "gather_wide", rhp.WIDE_POISON, True

    def caps(self):
        t = [self.side(w).want["totals"] for w in "AB"]
        return tuple(max(int(x[f]) for x in t) for f in ("n_wide", "n_hdrs", "body_bytes"))

    def outs(self):
        c = self.caps()
        assert min(c) > 0, "the round has wide slots, wide header rows and gathered bodies"
        return {"totals": 16, "slots": 64 * c[0], "whdrs": 8 * c[1], "body": c[2], "work": 8 * rhp.wide_work_words(self.shape()[0])}

    def build(self, which):
        r = self.round(which)
        totals, slots, hdrs, body = rhp.gather_wide_cpu(r.b, r.sess, r.results, r.starts, r.dreq, r.hc)
        return Side(r.session_inputs("dreq", "hc"), {"totals": totals, "slots": slots, "whdrs": hdrs, "body": body})

    def launch(self, T, side, stream):
        n, ns = self.shape()
        o = rhp._wide_out(T["totals"], T["slots"], T["whdrs"], T["body"], T["work"], self.caps())
        d = self.desc(T)
        check_rc(rhp.lib().rhp_gather_wide(ctypes.byref(d), VP(ptr(T["sessions"])), ns, VP(ptr(T["results"])), VP(ptr(T["starts"])),
                                           VP(ptr(T["dreq"])), VP(ptr(T["hc"])), ctypes.byref(o), VP(stream.cuda_stream)), "rhp_gather_wide")
        return [o]

    def got(self, raw, side):
        totals, slots, hdrs, body = rhp._wide_result(raw["totals"], raw["slots"], raw["whdrs"], raw["body"], self.caps())
        t = side.want["totals"]
        nw, nh, nb = int(t["n_wide"]), int(t["n_hdrs"]), int(t["body_bytes"])
        for a, k, label in ((slots, nw, "slots"), (hdrs, nh, "hdrs"), (body, nb, "body")):
            assert (u8(a[k:]) == self.poison).all(), f"gather_wide: {label} behind the total were written"
        return {"totals": totals, "slots": slots[:nw], "whdrs": hdrs[:nh], "body": body[:nb]}


class ReplySessions(RoundCase):
    name, poison, multi, tables = "reply_sessions", rhp.REPLY_POISON, True, True

    def images(self, which):
        imgs = rot(IMAGES, which)   # (the images are device inputs: B's differ too)
        off = np.zeros(len(imgs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in imgs])
        return np.frombuffer(b"".join(imgs), dtype=np.uint8).copy(), off

    def out_size(self):
        return max(self.side(w).want["total"] for w in "AB") + 64

    def outs(self):
        n, ns = self.shape()
        return {"replies": 24 * ns, "total": 8, "out": self.out_size(), "work": 8 * rhp.reply_work_words(n, ns)}

    def build(self, which):
        r = self.round(which)
        imgs, off = self.images(which)
        replies, total, out = rhp.reply_sessions_cpu(r.b, r.sess, r.results, r.route, imgs, off, STATIC_MASK)
        assert total > 0
        return Side(dict(r.session_inputs("route"), images=u8(imgs), image_off=u8(off)), {"replies": replies, "total": total, "out": out})

    def launch(self, T, side, stream):
        n, ns = self.shape()
        t = rhp.ReplyTable(ptr(T["images"]), ptr(T["image_off"]), len(IMAGES), STATIC_MASK)
        o = rhp.ReplyOut(ptr(T["replies"]), ptr(T["total"]), ptr(T["out"]), T["out"].numel(), ptr(T["work"]))
        d = self.desc(T)
        check_rc(rhp.lib().rhp_reply_sessions(ctypes.byref(d), VP(ptr(T["sessions"])), ns, VP(ptr(T["results"])), VP(ptr(T["route"])),
                                              ctypes.byref(t), ctypes.byref(o), VP(stream.cuda_stream)), "rhp_reply_sessions")
        return [t, o]

    def got(self, raw, side):
        total = int(raw["total"].view(np.uint64)[0])
        assert total <= raw["out"].size and (raw["out"][total:] == self.poison).all(), "reply_sessions: bytes behind the total were written"
        return {"replies": raw["replies"].view(rhp.SESSION_REPLY_DTYPE), "total": total, "out": raw["out"][:total]}


class ForwardSessions(RoundCase):
    """more than 4096 record slots: two scan tiles and a carry"""
    name, poison, multi, tables, n_sessions = "forward_sessions", rhp.FORWARD_POISON, True, True, 1400

    def out_size(self):
        return max(int(self.side(w).want["out_off"][-1]) for w in "AB") + 64

    def outs(self):
        n, ns = self.shape()
        assert n > 4096
        return {"out_off": 8 * (n + 1), "why": 4 * n, "out": self.out_size(), "fwd_off": 4 * (ns + 1), "head_bits": 4 * ((n + 31) // 32),
                "work": 8 * rhp.forward_work_words(n, ns)}

    def build(self, which):
        r = self.round(which)
        out_off, why, out, fwd_off, bits = rhp.forward_sessions_cpu(r.b, r.sess, r.results, r.starts, r.route, len(fs.ROUTES),
                                                                    fs.FORWARD_MASK, fs.DROP, fs.VIA)
        return Side(r.session_inputs("route"), {"out_off": out_off, "why": why, "out": out, "fwd_off": fwd_off, "head_bits": bits})

    def launch(self, T, side, stream, ns=None, n=None):
        """ns=0, n=0: the two empty forms (the host's counts; the tensors stay)"""
        n_sessions = self.shape()[1]
        ns = n_sessions if ns is None else ns
        text, nm, _ = rhp.classify_tables(fs.DROP)
        extra, extra_p = cbytes(fs.VIA)
        f = rhp.Forward(len(fs.ROUTES), fs.FORWARD_MASK, ptr(text), ptr(nm), len(nm), len(fs.VIA), extra_p, ptr(T["out_off"]), ptr(T["why"]),
                        ptr(T["out"]), T["out"].numel(), ptr(T["fwd_off"]), ptr(T["head_bits"]), ptr(T["work"]))
        d = self.desc(T)
        if n is not None:
            d.n = n
        check_rc(rhp.lib().rhp_forward_sessions(ctypes.byref(d), VP(ptr(T["sessions"])), ns, VP(ptr(T["results"])), VP(ptr(T["starts"])),
                                                VP(ptr(T["route"])), ctypes.byref(f), VP(stream.cuda_stream)), "rhp_forward_sessions")
        return [text, nm, extra, f]

    def got(self, raw, side):
        n, ns = self.shape()
        out_off, why, out, fwd_off, bits = rhp._forward_result(raw["out_off"], raw["why"], raw["out"], raw["fwd_off"], raw["head_bits"],
                                                               n, ns, self.poison)
        return {"out_off": out_off, "why": why, "out": written_out(out_off, raw["out"], self.poison, self.name), "fwd_off": fwd_off,
                "head_bits": bits}


CASES = (ParseBatch(rhp.MODE_PHR), ParseBatch(rhp.MODE_HTTP), FixupSessions(), PackDense(), WriteResponses(), ClassifyBatch(),
         ClassifySessions(), ReplySessions(), GatherWide(), SplitSessions(), ParseMessages(), DecodeChunked(), FrameMessages(),
         WalkResponses(), WalkResume(), WalkAnswers(), LookupWalked(), RelayWalked(), ForwardSessions())
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == 19


def differing(a, b):
    """whether two answers of one key differ (arrays of any dtype, or numbers)"""
    if isinstance(a, np.ndarray):
        return a.shape != b.shape or bool((u8(a) != u8(b)).any())
    return a != b
