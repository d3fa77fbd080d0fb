"""libreactorng_amd -- MI355X-native batched HTTP/1.1 request parser (rhp).

Python plumbing over the C-ABI in include/rhp.h (librhp.so, HIP/gfx950) and the
host helpers in include/rhp_gen.h (librhp_host.so).  The product path is the HIP
kernel: `parse_batch` raises if librhp.so is missing or no GPU is visible; it
never falls back to a CPU parser.

Reference interface mirrored (record fields are offsets from each request start):
  phr_parse_request   /root/reference/src/picohttpparser/picohttpparser.h:51-52
  http_read_request   /root/reference/src/reactor/http.h:36
"""
from __future__ import annotations

import contextlib
import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBRHP = os.environ.get("RHP_LIB", os.path.join(_HERE, "librhp.so"))  # RHP_LIB: A/B experiments only
LIBHOST = os.path.join(_HERE, "librhp_host.so")

RHP_PAD = 256
RHP_MAX_LEN = 65535
RHP_MAX_HEADERS = 64
RHP_RET_TOOLONG = -3
RHP_WORK_WORDS = 64
MODE_PHR, MODE_HTTP = 0, 1
LAYOUT_REQUEST_MAJOR, LAYOUT_HEADER_MAJOR, LAYOUT_COMPACT, LAYOUT_DENSE, LAYOUT_DENSE_RM = 0, 1, 2, 3, 4
DENSE_LAYOUTS = (LAYOUT_DENSE, LAYOUT_DENSE_RM)            # rhp.h: 8-byte request records, u16 lengths
LENGTH_LAYOUTS = (LAYOUT_COMPACT,) + DENSE_LAYOUTS          # records expanded by the running sum
IMPL_DFA, IMPL_EXACT, IMPL_DFA_LATE = 0, 1, 2
RHP_NAME_NULL = 0xFFFF
F_EXACT = 0x1
F_WIDE = 0x2   # compact layout: the request's header records are in the wide area (rhp.h)
HTTP_WIDE = 0x1   # compact http records (rhp_http_compact_t.flags): the record is in the wide area (rhp.h)
DENSE_WIDE, DENSE_BAD = 0x1, 0x2   # dense request records (rhp_req_dense_t.flags, rhp.h)

GEN_TFB128, GEN_GET256, GEN_ZIPF, GEN_POST1K, GEN_CHUNKED, GEN_FUZZ, GEN_FUZZ_HTTP = 1, 2, 3, 5, 6, 100, 101

# numpy views of the C records (rhp.h)
REQ_DTYPE = np.dtype([("ret", "<i4"), ("method_len", "<u2"), ("path_off", "<u2"), ("path_len", "<u2"),
                      ("method_off", "u1"), ("minor_version", "i1"), ("num_headers", "<u2"),
                      ("flags", "<u2")])
HDR_DTYPE = np.dtype([("name_off", "<u2"), ("name_len", "<u2"), ("value_off", "<u2"), ("value_len", "<u2")])
HTTP_DTYPE = np.dtype([("result", "<i4"), ("body_kind", "<u4"), ("consumed", "<u8"), ("body_len", "<u8")])
assert REQ_DTYPE.itemsize == 16 and HDR_DTYPE.itemsize == 8 and HTTP_DTYPE.itemsize == 24


class Batch(ctypes.Structure):
    """struct rhp_batch (include/rhp.h)."""
    _fields_ = [("bytes", ctypes.c_void_p), ("bytes_rw", ctypes.c_void_p), ("offsets", ctypes.c_void_p),
                ("bytes_size", ctypes.c_uint64), ("n", ctypes.c_uint32), ("max_headers", ctypes.c_uint32),
                ("mode", ctypes.c_uint32), ("layout", ctypes.c_uint32), ("reqs", ctypes.c_void_p),
                ("hdrs", ctypes.c_void_p), ("http", ctypes.c_void_p), ("work", ctypes.c_void_p),
                ("flags", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("last_len", ctypes.c_void_p)]


BATCH_SPECULATIVE = 1        # rhp_batch_t.flags (rhp.h RHP_BATCH_SPECULATIVE)
BODY_CHUNKED_PENDING = 2
SESSION_DTYPE = np.dtype([("piece_lo", "<u4"), ("piece_hi", "<u4")])
SESSION_RESULT_DTYPE = np.dtype([("n_slots", "<u4"), ("more", "<u4"), ("consumed", "<u8")])


# exported C-ABI symbols of librhp.so, as declared in include/rhp.h
RHP_SYMBOLS = ("rhp_parse_batch", "rhp_set_impl", "rhp_kernel_name", "rhp_version", "rhp_write_responses",
               "rhp_fixup_sessions", "rhp_pack_dense", "rhp_classify_batch", "rhp_classify_sessions", "rhp_reply_sessions",
               "rhp_gather_wide", "rhp_split_sessions", "rhp_parse_messages", "rhp_decode_chunked", "rhp_frame_messages",
               "rhp_walk_responses", "rhp_walk_resume", "rhp_lookup_walked", "rhp_walk_answers", "rhp_relay_walked",
               "rhp_relay_walked_steps", "rhp_write_responses_steps", "rhp_forward_sessions")
HOST_SYMBOLS = ("rhp_gen_size", "rhp_gen_fill", "rhp_gen_header_bytes", "rhp_splitmix64",
                "rhp_emu_parse_batch", "rhp_cpu_parse_batch", "rhp_phr_parse_request", "rhp_http_read_cpu",
                "rhp_cpu_fixup_sessions", "rhp_expand_records", "rhp_expand_http", "rhp_expand_reqs", "rhp_cpu_pack_dense",
                "rhp_cpu_classify_batch", "rhp_emu_fixup_sessions", "rhp_test_fixup_whole", "rhp_test_chunk_window",
                "rhp_test_chunk_exact", "rhp_cpu_classify_sessions", "rhp_cpu_reply_sessions", "rhp_cpu_gather_wide",
                "rhp_cpu_split_sessions", "rhp_cpu_parse_messages", "rhp_phr_parse_response", "rhp_phr_parse_headers",
                "rhp_cpu_decode_chunked", "rhp_phr_decode_chunked", "rhp_phr_decode_chunked_is_in_data",
                "rhp_cpu_frame_messages", "rhp_cpu_walk_responses", "rhp_cpu_walk_resume",
                "rhp_cpu_lookup_walked", "rhp_cpu_walk_answers", "rhp_cpu_relay_walked",
                "rhp_cpu_forward_sessions")

_rhp = None
_host = None


class RespBatch(ctypes.Structure):
    """rhp_resp_batch_t (include/rhp.h): http_write_response over a batch"""
    _fields_ = [("arena", ctypes.c_void_p), ("resps", ctypes.c_void_p), ("fields", ctypes.c_void_p),
                ("n", ctypes.c_uint32), ("date_len", ctypes.c_uint32), ("date", ctypes.c_char_p),
                ("out_off", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_size", ctypes.c_uint64),
                ("work", ctypes.c_void_p)]


RHP_DATE_LEN = 29


class Classify(ctypes.Structure):
    """rhp_classify_t (include/rhp.h): header lookup and route match over a parsed batch"""
    _fields_ = [("text", ctypes.c_void_p), ("names", ctypes.c_void_p), ("routes", ctypes.c_void_p),
                ("n_names", ctypes.c_uint32), ("n_routes", ctypes.c_uint32), ("fields", ctypes.c_void_p),
                ("route", ctypes.c_void_p)]


CLASSIFY_MAX_NAMES, CLASSIFY_NAME_MAX, CLASSIFY_MAX_ROUTES, CLASSIFY_TEXT_MAX = 16, 64, 32, 2048
ROUTE_NONE = 0xFFFF
FIELDREF_DTYPE = np.dtype([("value_off", "<u2"), ("value_len", "<u2")])   # absent: (RHP_NAME_NULL, 0)


class ReplyTable(ctypes.Structure):
    """rhp_reply_table_t (include/rhp.h): the reply images of the static routes"""
    _fields_ = [("images", ctypes.c_void_p), ("image_off", ctypes.c_void_p), ("n_routes", ctypes.c_uint32),
                ("static_mask", ctypes.c_uint32)]


class ReplyOut(ctypes.Structure):
    """rhp_reply_out_t (include/rhp.h): the outputs of rhp_reply_sessions"""
    _fields_ = [("replies", ctypes.c_void_p), ("total", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("out_size", ctypes.c_uint64), ("work", ctypes.c_void_p)]


SESSION_REPLY_DTYPE = np.dtype([("count", "<u4"), ("reserved", "<u4"), ("out_off", "<u8"), ("out_len", "<u8")])
assert SESSION_REPLY_DTYPE.itemsize == 24 and ctypes.sizeof(ReplyTable) == 24 and ctypes.sizeof(ReplyOut) == 40


def reply_work_words(n: int, n_sessions: int = 0) -> int:
    """RHP_REPLY_WORK_WORDS (include/rhp.h)"""
    return n + 1 + (n + 63) // 64 + 3 * ((n + 255) // 256)


class WideOut(ctypes.Structure):
    """rhp_wide_out_t (include/rhp.h): the outputs of rhp_gather_wide"""
    _fields_ = [("totals", ctypes.c_void_p), ("slots", ctypes.c_void_p), ("cap_slots", ctypes.c_uint32),
                ("hdrs", ctypes.c_void_p), ("cap_hdrs", ctypes.c_uint32), ("body", ctypes.c_void_p),
                ("cap_body", ctypes.c_uint64), ("work", ctypes.c_void_p)]


WIDE_NO_BODY = 0xFFFFFFFFFFFFFFFF
WIDE_SLOT_DTYPE = np.dtype([("slot", "<u4"), ("hdr_first", "<u4"), ("req", REQ_DTYPE), ("http", HTTP_DTYPE),
                            ("req_start", "<u8"), ("body_off", "<u8")])
WIDE_TOTALS_DTYPE = np.dtype([("n_wide", "<u4"), ("n_hdrs", "<u4"), ("body_bytes", "<u8")])
REQ_DENSE_DTYPE = np.dtype([("ret", "<u2"), ("path_len", "<u2"), ("method_len", "u1"), ("num_headers", "u1"),
                            ("minor_version", "u1"), ("flags", "u1")])
HTTP_COMPACT_DTYPE = np.dtype([("result", "i1"), ("body_kind", "u1"), ("flags", "u1"), ("reserved", "u1"),
                               ("body_len", "<u4")])
assert WIDE_SLOT_DTYPE.itemsize == 64 and WIDE_TOTALS_DTYPE.itemsize == 16 and ctypes.sizeof(WideOut) == 64
assert REQ_DENSE_DTYPE.itemsize == 8 and HTTP_COMPACT_DTYPE.itemsize == 8


def wide_work_words(n: int) -> int:
    """RHP_WIDE_WORK_WORDS (include/rhp.h)"""
    return 5 * ((n + 63) // 64) + 1


class SplitOut(ctypes.Structure):
    """rhp_split_out_t (include/rhp.h): the outputs of rhp_split_sessions"""
    _fields_ = [("n_pieces", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("cap_pieces", ctypes.c_uint32),
                ("sessions", ctypes.c_void_p), ("work", ctypes.c_void_p)]


SPLIT_STEP_BYTES = 1024   # RHP_SPLIT_STEP_BYTES (include/rhp.h): what one wave of the mark kernel takes
assert ctypes.sizeof(SplitOut) == 40


def split_work_words(bytes_end: int, n_sessions: int = 0) -> int:
    """RHP_SPLIT_WORK_WORDS (include/rhp.h)"""
    return 25 * ((bytes_end + SPLIT_STEP_BYTES - 1) // SPLIT_STEP_BYTES) + 1


class MsgBatch(ctypes.Structure):
    """rhp_msg_batch_t (include/rhp.h): a batch of responses or bare header blocks for rhp_parse_messages"""
    _fields_ = [("bytes", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("bytes_size", ctypes.c_uint64),
                ("n", ctypes.c_uint32), ("max_headers", ctypes.c_uint32), ("kind", ctypes.c_uint32),
                ("layout", ctypes.c_uint32), ("msgs", ctypes.c_void_p), ("hdrs", ctypes.c_void_p),
                ("last_len", ctypes.c_void_p)]


MSG_RESPONSE, MSG_HEADERS = 0, 1   # enum rhp_msg_kind
MSG_DTYPE = np.dtype([("ret", "<i4"), ("status", "<u2"), ("msg_off", "<u2"), ("msg_len", "<u2"),
                      ("minor_version", "i1"), ("reserved", "u1"), ("num_headers", "<u2"), ("flags", "<u2")])
assert MSG_DTYPE.itemsize == 16 and ctypes.sizeof(MsgBatch) == 64


class ChunkedBatch(ctypes.Structure):
    """rhp_chunked_batch_t (include/rhp.h): the new bytes of n chunked streams for rhp_decode_chunked"""
    _fields_ = [("bytes", ctypes.c_void_p), ("offsets", ctypes.c_void_p), ("bytes_size", ctypes.c_uint64),
                ("n", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("decoders", ctypes.c_void_p),
                ("results", ctypes.c_void_p)]


# enum RHP_CHUNKED_IN_* (rhp.h; picohttpparser.c:501-508)
(CHUNKED_IN_CHUNK_SIZE, CHUNKED_IN_CHUNK_EXT, CHUNKED_IN_CHUNK_DATA, CHUNKED_IN_CHUNK_CRLF, CHUNKED_IN_TRAILERS_LINE_HEAD,
 CHUNKED_IN_TRAILERS_LINE_MIDDLE) = range(6)
CHUNKED_DTYPE = np.dtype([("bytes_left_in_chunk", "<u8"), ("consume_trailer", "u1"), ("hex_count", "u1"), ("state", "u1"),
                          ("reserved", "u1", (5,))])   # rhp_chunked_t = struct phr_chunked_decoder
CHUNKED_RESULT_DTYPE = np.dtype([("ret", "<i8"), ("size", "<u8")])
assert CHUNKED_DTYPE.itemsize == 16 and CHUNKED_RESULT_DTYPE.itemsize == 16 and ctypes.sizeof(ChunkedBatch) == 48


class FrameArgs(ctypes.Structure):
    """rhp_frame_args_t (include/rhp.h): the lookup names and the outputs of rhp_frame_messages"""
    _fields_ = [("text", ctypes.c_void_p), ("names", ctypes.c_void_p), ("n_names", ctypes.c_uint32),
                ("consume_trailer", ctypes.c_uint32), ("fields", ctypes.c_void_p), ("frames", ctypes.c_void_p),
                ("decoders", ctypes.c_void_p), ("reserved", ctypes.c_uint64)]


FRAME_NONE, FRAME_LENGTH, FRAME_CHUNKED = 0, 1, 2   # enum RHP_FRAME_*
FRAME_DTYPE = np.dtype([("result", "<i4"), ("body_kind", "<u4"), ("body_len", "<u8")])   # rhp_frame_t
assert FRAME_DTYPE.itemsize == 16 and ctypes.sizeof(FrameArgs) == 56


class WalkBatch(ctypes.Structure):
    """rhp_walk_batch_t (include/rhp.h): the sessions, slots and outputs of rhp_walk_responses"""
    _fields_ = [("bytes", ctypes.c_void_p), ("bytes_rw", ctypes.c_void_p), ("bytes_size", ctypes.c_uint64),
                ("sess_off", ctypes.c_void_p), ("slot_off", ctypes.c_void_p), ("n_sessions", ctypes.c_uint32),
                ("n_slots_total", ctypes.c_uint32), ("max_headers", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("msgs", ctypes.c_void_p), ("hdrs", ctypes.c_void_p), ("slots", ctypes.c_void_p),
                ("results", ctypes.c_void_p)]


WALK_END, WALK_HEAD, WALK_BAD, WALK_BODY, WALK_CLOSE, WALK_MORE = range(6)   # enum rhp_walk_stop
WALK_TRAILERS, WALK_DEFRAME, WALK_NONE_EMPTY = 1, 2, 4                       # RHP_WALK_* flags
WALK_SLOT_DTYPE = np.dtype([("start", "<u8"), ("body_len", "<u8"), ("wire_len", "<u8"), ("result", "<i4"),
                            ("body_kind", "<u4")])                           # rhp_walk_slot_t
WALK_RESULT_DTYPE = np.dtype([("n_slots", "<u4"), ("stop", "<u4"), ("consumed", "<u8")])   # rhp_walk_result_t
assert WALK_SLOT_DTYPE.itemsize == 32 and WALK_RESULT_DTYPE.itemsize == 16 and ctypes.sizeof(WalkBatch) == 88
WALK_AT_HEAD, WALK_IN_LENGTH, WALK_IN_CHUNKED, WALK_IN_CLOSE, WALK_DEAD = range(5)   # enum rhp_walk_phase
WALK_STATE_DTYPE = np.dtype([("decoder", CHUNKED_DTYPE), ("left", "<u8"), ("phase", "<u4"), ("reserved", "<u4")])   # rhp_walk_state_t
assert WALK_STATE_DTYPE.itemsize == 32


class WalkLookup(ctypes.Structure):
    """rhp_walk_lookup_t (include/rhp.h): the lookup names and the output of rhp_lookup_walked"""
    _fields_ = [("text", ctypes.c_void_p), ("names", ctypes.c_void_p), ("n_names", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("fields", ctypes.c_void_p)]


assert ctypes.sizeof(WalkLookup) == 32


class WalkAsked(ctypes.Structure):
    """rhp_walk_asked_t (include/rhp.h): the sessions' queues of outstanding requests and the outputs of rhp_walk_answers"""
    _fields_ = [("req_off", ctypes.c_void_p), ("head_bits", ctypes.c_void_p), ("n_req_total", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("answered", ctypes.c_void_p), ("slot_req", ctypes.c_void_p)]


WALK_REQ_NONE = 0xFFFFFFFF   # RHP_WALK_REQ_NONE
assert ctypes.sizeof(WalkAsked) == 40


class WalkRelay(ctypes.Structure):
    """rhp_walk_relay_t (include/rhp.h): the drop names, the date and the outputs of rhp_relay_walked"""
    _fields_ = [("text", ctypes.c_void_p), ("names", ctypes.c_void_p), ("n_names", ctypes.c_uint32),
                ("date_len", ctypes.c_uint32), ("date", ctypes.c_char_p), ("out_off", ctypes.c_void_p),
                ("why", ctypes.c_void_p), ("out", ctypes.c_void_p), ("out_size", ctypes.c_uint64), ("work", ctypes.c_void_p)]


assert ctypes.sizeof(WalkRelay) == 72
RELAY_MAX_NAMES = 13   # RHP_RELAY_MAX_NAMES
(RELAY_OK, RELAY_UNUSED, RELAY_NOT_HEAD, RELAY_OUTSIDE, RELAY_INTERIM, RELAY_PARTIAL, RELAY_FOLD, RELAY_SPAN, RELAY_FRAMING,
 RELAY_LONG, RELAY_BODY_OUTSIDE) = range(11)   # enum rhp_relay_why


def relay_work_words(n: int) -> int:
    """RHP_RELAY_WORK_WORDS (include/rhp.h)"""
    return (n + 4095) // 4096 + 1 + 2 * n


class Forward(ctypes.Structure):
    """rhp_forward_t (include/rhp.h): the forwarded routes, the drop names, the extra lines and the outputs of
    rhp_forward_sessions"""
    _fields_ = [("n_routes", ctypes.c_uint32), ("forward_mask", ctypes.c_uint32), ("text", ctypes.c_void_p),
                ("names", ctypes.c_void_p), ("n_names", ctypes.c_uint32), ("extra_len", ctypes.c_uint32),
                ("extra", ctypes.c_char_p), ("out_off", ctypes.c_void_p), ("why", ctypes.c_void_p), ("out", ctypes.c_void_p),
                ("out_size", ctypes.c_uint64), ("fwd_off", ctypes.c_void_p), ("head_bits", ctypes.c_void_p),
                ("work", ctypes.c_void_p)]


assert ctypes.sizeof(Forward) == 96
FORWARD_MAX_NAMES = 14    # RHP_FORWARD_MAX_NAMES
FORWARD_EXTRA_MAX = 128   # RHP_FORWARD_EXTRA_MAX
(FORWARD_OK, FORWARD_UNUSED, FORWARD_NOT_READY, FORWARD_OUTSIDE, FORWARD_CLOSED, FORWARD_ROUTE, FORWARD_FOLD, FORWARD_SPAN,
 FORWARD_BODY, FORWARD_LONG, FORWARD_BODY_OUTSIDE) = range(11)   # enum rhp_forward_why


def forward_work_words(n: int, n_sessions: int = 0) -> int:
    """RHP_FORWARD_WORK_WORDS (include/rhp.h)"""
    return 2 * ((n + 4095) // 4096 + 1) + 2 * n + 1 + (n + 63) // 64


def _torch_hip_runtime() -> str | None:
    """Path of the HIP runtime torch ships (torch/lib/libamdhip64.so), found
    without importing torch."""
    import importlib.util
    spec = importlib.util.find_spec("torch")
    if spec is None or not spec.submodule_search_locations:
        return None
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return path if os.path.exists(path) else None


def hip_runtimes() -> list[str]:
    """The libamdhip64 files mapped into this process (Linux /proc/self/maps)."""
    try:
        with open("/proc/self/maps") as f:
            return sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln and "/" in ln})
    except OSError:
        return []


def check_one_hip_runtime() -> None:
    """Two HIP runtimes in one process (torch's and /opt/rocm's) each own their
    device memory: a kernel of one launched on buffers of the other fails with
    error 100.  Raise with the cause instead."""
    rt = [os.path.realpath(p) for p in hip_runtimes()]
    if len(set(rt)) > 1:
        raise RuntimeError("two HIP runtimes are loaded (" + ", ".join(sorted(set(rt))) + "): librhp.so was "
                           "loaded before torch without libreactorng_amd.lib(); load it through lib(), or "
                           "import torch first")


def lib() -> ctypes.CDLL:
    """librhp.so (HIP).  Raises if it is missing: there is no fallback.

    Load order.  librhp.so's DT_NEEDED is libamdhip64.so.7 (the
    soname of both /opt/rocm's runtime and the one torch ships); torch's
    libc10_hip.so asks for the unversioned libamdhip64.so through its $ORIGIN
    rpath.  ld.so reuses a loaded library only when a request matches its soname
    or the name it was loaded by, so torch-first gives one runtime (librhp's
    request matches the soname of torch's copy), while librhp-first loads
    /opt/rocm's copy and torch's later request for `libamdhip64.so` matches
    neither name: torch then loads its own copy, and tensors it allocates are
    foreign to librhp's runtime.  So torch's runtime, when torch is installed, is
    preloaded by path (RTLD_GLOBAL) before librhp.so, without importing torch;
    a process without torch uses /opt/rocm's."""
    global _rhp
    if _rhp is None:
        if not os.path.exists(LIBRHP):
            raise RuntimeError(f"{LIBRHP} missing: run __graft_entry__.build() (hipcc gfx950)")
        rt = _torch_hip_runtime()
        if rt is not None:
            ctypes.CDLL(rt, mode=ctypes.RTLD_GLOBAL)
        _rhp = ctypes.CDLL(LIBRHP)
        check_one_hip_runtime()
        _rhp.rhp_parse_batch.argtypes = [ctypes.POINTER(Batch), ctypes.c_void_p]
        _rhp.rhp_parse_batch.restype = ctypes.c_int
        _rhp.rhp_set_impl.argtypes = [ctypes.c_int]
        _rhp.rhp_set_impl.restype = ctypes.c_int
        _rhp.rhp_kernel_name.restype = ctypes.c_char_p
        _rhp.rhp_version.restype = ctypes.c_char_p
        _rhp.rhp_write_responses.argtypes = [ctypes.POINTER(RespBatch), ctypes.c_void_p]
        _rhp.rhp_write_responses.restype = ctypes.c_int
        vp = ctypes.c_void_p
        _rhp.rhp_pack_dense.argtypes = [ctypes.POINTER(Batch), vp, vp, vp, vp]
        _rhp.rhp_pack_dense.restype = ctypes.c_int
        _rhp.rhp_classify_batch.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(Classify), vp]
        _rhp.rhp_classify_batch.restype = ctypes.c_int
        _rhp.rhp_classify_sessions.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp,
                                               ctypes.POINTER(Classify), vp]
        _rhp.rhp_classify_sessions.restype = ctypes.c_int
        _rhp.rhp_reply_sessions.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp,
                                            ctypes.POINTER(ReplyTable), ctypes.POINTER(ReplyOut), vp]
        _rhp.rhp_reply_sessions.restype = ctypes.c_int
        _rhp.rhp_gather_wide.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp, vp, vp,
                                         ctypes.POINTER(WideOut), vp]
        _rhp.rhp_gather_wide.restype = ctypes.c_int
        _rhp.rhp_split_sessions.argtypes = [vp, ctypes.c_uint64, vp, ctypes.c_uint32, ctypes.POINTER(SplitOut), vp]
        _rhp.rhp_split_sessions.restype = ctypes.c_int
        _rhp.rhp_parse_messages.argtypes = [ctypes.POINTER(MsgBatch), vp]
        _rhp.rhp_parse_messages.restype = ctypes.c_int
        _rhp.rhp_decode_chunked.argtypes = [ctypes.POINTER(ChunkedBatch), vp]
        _rhp.rhp_decode_chunked.restype = ctypes.c_int
        _rhp.rhp_frame_messages.argtypes = [ctypes.POINTER(MsgBatch), ctypes.POINTER(FrameArgs), vp]
        _rhp.rhp_frame_messages.restype = ctypes.c_int
        _rhp.rhp_walk_responses.argtypes = [ctypes.POINTER(WalkBatch), vp]
        _rhp.rhp_walk_responses.restype = ctypes.c_int
        _rhp.rhp_walk_resume.argtypes = [ctypes.POINTER(WalkBatch), vp, vp]
        _rhp.rhp_walk_resume.restype = ctypes.c_int
        _rhp.rhp_lookup_walked.argtypes = [ctypes.POINTER(WalkBatch), ctypes.POINTER(WalkLookup), vp]
        _rhp.rhp_lookup_walked.restype = ctypes.c_int
        _rhp.rhp_relay_walked.argtypes = [ctypes.POINTER(WalkBatch), ctypes.POINTER(WalkRelay), vp]
        _rhp.rhp_relay_walked.restype = ctypes.c_int
        _rhp.rhp_relay_walked_steps.argtypes = [ctypes.POINTER(WalkBatch), ctypes.POINTER(WalkRelay), vp, ctypes.POINTER(ctypes.c_float * 3)]
        _rhp.rhp_relay_walked_steps.restype = ctypes.c_int
        _rhp.rhp_forward_sessions.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp, vp, ctypes.POINTER(Forward), vp]
        _rhp.rhp_forward_sessions.restype = ctypes.c_int
        _rhp.rhp_write_responses_steps.argtypes = [ctypes.POINTER(RespBatch), vp, ctypes.POINTER(ctypes.c_float * 3)]
        _rhp.rhp_write_responses_steps.restype = ctypes.c_int
        _rhp.rhp_walk_answers.argtypes = [ctypes.POINTER(WalkBatch), vp, ctypes.POINTER(WalkAsked), vp]
        _rhp.rhp_walk_answers.restype = ctypes.c_int
    return _rhp


def host() -> ctypes.CDLL:
    """librhp_host.so: generator, CPU exact parser, DFA emulator."""
    global _host
    if _host is None:
        if not os.path.exists(LIBHOST):
            raise RuntimeError(f"{LIBHOST} missing: run __graft_entry__.build()")
        _host = ctypes.CDLL(LIBHOST)
        u64 = ctypes.c_uint64
        _host.rhp_gen_size.argtypes = [ctypes.c_int, u64, u64, u64]
        _host.rhp_gen_size.restype = u64
        _host.rhp_gen_fill.argtypes = [ctypes.c_int, u64, u64, u64, ctypes.c_void_p, ctypes.c_void_p]
        _host.rhp_gen_fill.restype = ctypes.c_int
        _host.rhp_gen_header_bytes.argtypes = [ctypes.c_int, u64, u64, u64]
        _host.rhp_gen_header_bytes.restype = u64
        _host.rhp_emu_parse_batch.argtypes = [ctypes.POINTER(Batch), ctypes.c_void_p]
        _host.rhp_emu_parse_batch.restype = ctypes.c_int
        _host.rhp_cpu_parse_batch.argtypes = [ctypes.POINTER(Batch)]
        _host.rhp_cpu_parse_batch.restype = ctypes.c_int
        sz, vp = ctypes.c_size_t, ctypes.c_void_p
        P = ctypes.POINTER
        _host.rhp_phr_parse_request.argtypes = [vp, sz, P(vp), P(sz), P(vp), P(sz), P(ctypes.c_int),
                                                P(PhrHeader), P(sz), sz]
        _host.rhp_phr_parse_request.restype = ctypes.c_int
        _host.rhp_http_read_cpu.argtypes = [vp, sz, P(HttpReq), P(PhrHeader), P(sz)]
        _host.rhp_http_read_cpu.restype = ctypes.c_int
        _host.rhp_cpu_fixup_sessions.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp]
        _host.rhp_cpu_fixup_sessions.restype = ctypes.c_int
        _host.rhp_emu_fixup_sessions.argtypes = _host.rhp_cpu_fixup_sessions.argtypes
        _host.rhp_emu_fixup_sessions.restype = ctypes.c_int
        _host.rhp_test_fixup_whole.argtypes = [ctypes.POINTER(Batch), vp]
        _host.rhp_test_fixup_whole.restype = ctypes.c_int
        _host.rhp_expand_records.argtypes = [ctypes.POINTER(Batch), vp, vp, vp]
        _host.rhp_expand_records.restype = ctypes.c_int
        _host.rhp_expand_http.argtypes = [ctypes.POINTER(Batch), vp, vp, vp]
        _host.rhp_expand_reqs.argtypes = [ctypes.POINTER(Batch), vp, vp]
        _host.rhp_cpu_pack_dense.argtypes = [ctypes.POINTER(Batch), vp, vp, vp]
        _host.rhp_cpu_pack_dense.restype = ctypes.c_int
        _host.rhp_expand_reqs.restype = ctypes.c_int
        _host.rhp_expand_http.restype = ctypes.c_int
        _host.rhp_cpu_classify_batch.argtypes = [ctypes.POINTER(Batch), ctypes.POINTER(Classify)]
        _host.rhp_cpu_classify_batch.restype = ctypes.c_int
        _host.rhp_cpu_classify_sessions.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp,
                                                    ctypes.POINTER(Classify)]
        _host.rhp_cpu_classify_sessions.restype = ctypes.c_int
        _host.rhp_cpu_reply_sessions.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp,
                                                 ctypes.POINTER(ReplyTable), ctypes.POINTER(ReplyOut)]
        _host.rhp_cpu_reply_sessions.restype = ctypes.c_int
        _host.rhp_cpu_gather_wide.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp, vp, vp,
                                              ctypes.POINTER(WideOut)]
        _host.rhp_cpu_gather_wide.restype = ctypes.c_int
        _host.rhp_cpu_split_sessions.argtypes = [vp, u64, vp, ctypes.c_uint32, ctypes.POINTER(SplitOut)]
        _host.rhp_cpu_split_sessions.restype = ctypes.c_int
        _host.rhp_cpu_parse_messages.argtypes = [ctypes.POINTER(MsgBatch)]
        _host.rhp_cpu_parse_messages.restype = ctypes.c_int
        _host.rhp_phr_parse_response.argtypes = [vp, sz, P(ctypes.c_int), P(ctypes.c_int), P(vp), P(sz), P(PhrHeader),
                                                 P(sz), sz]
        _host.rhp_phr_parse_response.restype = ctypes.c_int
        _host.rhp_phr_parse_headers.argtypes = [vp, sz, P(PhrHeader), P(sz), sz]
        _host.rhp_phr_parse_headers.restype = ctypes.c_int
        _host.rhp_cpu_decode_chunked.argtypes = [ctypes.POINTER(ChunkedBatch)]
        _host.rhp_cpu_decode_chunked.restype = ctypes.c_int
        _host.rhp_phr_decode_chunked.argtypes = [vp, vp, P(sz)]
        _host.rhp_phr_decode_chunked.restype = ctypes.c_ssize_t
        _host.rhp_phr_decode_chunked_is_in_data.argtypes = [vp]
        _host.rhp_phr_decode_chunked_is_in_data.restype = ctypes.c_int
        _host.rhp_cpu_frame_messages.argtypes = [ctypes.POINTER(MsgBatch), ctypes.POINTER(FrameArgs)]
        _host.rhp_cpu_frame_messages.restype = ctypes.c_int
        _host.rhp_cpu_walk_responses.argtypes = [ctypes.POINTER(WalkBatch)]
        _host.rhp_cpu_walk_responses.restype = ctypes.c_int
        _host.rhp_cpu_walk_resume.argtypes = [ctypes.POINTER(WalkBatch), vp]
        _host.rhp_cpu_walk_resume.restype = ctypes.c_int
        _host.rhp_cpu_lookup_walked.argtypes = [ctypes.POINTER(WalkBatch), ctypes.POINTER(WalkLookup)]
        _host.rhp_cpu_lookup_walked.restype = ctypes.c_int
        _host.rhp_cpu_relay_walked.argtypes = [ctypes.POINTER(WalkBatch), ctypes.POINTER(WalkRelay)]
        _host.rhp_cpu_relay_walked.restype = ctypes.c_int
        _host.rhp_cpu_forward_sessions.argtypes = [ctypes.POINTER(Batch), vp, ctypes.c_uint32, vp, vp, vp, ctypes.POINTER(Forward)]
        _host.rhp_cpu_forward_sessions.restype = ctypes.c_int
        _host.rhp_cpu_walk_answers.argtypes = [ctypes.POINTER(WalkBatch), vp, ctypes.POINTER(WalkAsked)]
        _host.rhp_cpu_walk_answers.restype = ctypes.c_int
    return _host


class PhrHeader(ctypes.Structure):
    """struct phr_header (picohttpparser.h:42-47) = rhp_phr_header_t (include/rhp_host.h)."""
    _fields_ = [("name", ctypes.c_void_p), ("name_len", ctypes.c_size_t), ("value", ctypes.c_void_p),
                ("value_len", ctypes.c_size_t)]


class HttpReq(ctypes.Structure):
    """rhp_http_req_t (include/rhp_host.h)."""
    _fields_ = [("method", ctypes.c_void_p), ("method_len", ctypes.c_size_t), ("target", ctypes.c_void_p),
                ("target_len", ctypes.c_size_t), ("minor_version", ctypes.c_int), ("body", ctypes.c_void_p),
                ("body_len", ctypes.c_size_t), ("consumed", ctypes.c_uint64)]


def phr_parse_request_cpu(buf: np.ndarray, start: int, length: int, max_headers: int, last_len: int = 0):
    """rhp_phr_parse_request (the host drop-in for phr_parse_request) on bytes
    buf[start:start+length] (buf may be read past the end, as the reference does).
    Returns (ret, minor, method(off,len), path(off,len), [(name_off|-1, name_len,
    value_off, value_len)]) with offsets from `start`."""
    h = host()
    hdrs = (PhrHeader * max(max_headers, 1))()
    m, pth = ctypes.c_void_p(), ctypes.c_void_p()
    ml, pl, nh = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t(max_headers)
    minor = ctypes.c_int()
    base = buf.ctypes.data + start
    ret = h.rhp_phr_parse_request(base, length, ctypes.byref(m), ctypes.byref(ml), ctypes.byref(pth),
                                  ctypes.byref(pl), ctypes.byref(minor), hdrs, ctypes.byref(nh), last_len)
    if ret <= 0:
        return ret, -1, (0, 0), (0, 0), []
    rel = lambda p: (p or 0) - base
    hs = [(rel(x.name) if x.name else -1, x.name_len, rel(x.value), x.value_len) for x in hdrs[: nh.value]]
    return ret, minor.value, (rel(m.value), ml.value), (rel(pth.value), pl.value), hs


def http_read_cpu(buf: np.ndarray, start: int, length: int, max_headers: int = 16):
    """rhp_http_read_cpu (http_read_request with pointer outputs) on buf[start:start+length]
    (written in place for chunked bodies).  Returns (result, consumed, body(off,len) | None)."""
    h = host()
    hdrs = (PhrHeader * max(max_headers, 1))()
    r = HttpReq()
    nh = ctypes.c_size_t(max_headers)
    base = buf.ctypes.data + start
    res = h.rhp_http_read_cpu(base, length, ctypes.byref(r), hdrs, ctypes.byref(nh))
    if res != 1:
        return res, 0, None
    body = (r.body - base, r.body_len) if r.body else None
    return res, int(r.consumed), body


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def _stream(stream=None) -> ctypes.c_void_p:
    """the stream as the library's calls take it; None: the current one"""
    import torch
    return ctypes.c_void_p((stream if stream is not None else torch.cuda.current_stream()).cuda_stream)


@contextlib.contextmanager
def _impl(impl: int):
    """the parse kernel's implementation set for the block, IMPL_DFA again behind it"""
    lib().rhp_set_impl(impl)
    try:
        yield
    finally:
        lib().rhp_set_impl(IMPL_DFA)


def _aligned(size: int, shift: int = 0, fill: int = 0) -> np.ndarray:
    """`size` host bytes that hold `fill` and start `shift` bytes behind a 16-byte boundary"""
    raw = np.full(size + shift + 16, fill, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16 + shift
    return raw[at: at + size]


def generate(config: int, n: int, seed: int, lo: int = 0):
    """Requests [lo, lo+n) of a generator config -> (bytes uint8[size+RHP_PAD], offsets uint64[n+1])."""
    h = host()
    size = h.rhp_gen_size(config, lo, lo + n, seed)
    if size == 0 and n > 0 and config not in (GEN_FUZZ, GEN_FUZZ_HTTP):
        raise ValueError(f"bad generator config {config}")
    buf = np.zeros(size + RHP_PAD, dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    if h.rhp_gen_fill(config, lo, lo + n, seed, _ptr(buf), _ptr(off)) != 0:
        raise ValueError(f"generator failed for config {config}")
    return buf, off


def header_bytes(config: int, n: int, seed: int, lo: int = 0) -> int:
    """Algorithmic bytes of requests [lo, lo+n)."""
    return int(host().rhp_gen_header_bytes(config, lo, lo + n, seed))


@dataclass
class Result:
    reqs: np.ndarray           # REQ_DTYPE [n]
    hdrs: np.ndarray           # HDR_DTYPE [n, max_headers] (a view of the header-major batch array; the
    #                            compact layout's records expanded by rhp_expand_records)
    http: np.ndarray | None    # HTTP_DTYPE [n] (http mode)
    bytes_out: np.ndarray | None = None  # request bytes after http mode (chunked bodies rewritten)
    raw_hdrs: np.ndarray | None = None   # the hdrs buffer as the parser left it (its layout's bytes)
    raw_http: np.ndarray | None = None   # the http buffer as the parser left it (compact: rhp_http_compact_t)
    raw_reqs: np.ndarray | None = None   # the reqs buffer as the parser left it (dense: rhp_req_dense_t + wide)
    batch: Batch | None = None           # the parsed batch over host memory (bytes, offsets, the raw records):
    #                                      what classify_cpu reads; `keep` holds the arrays it points into
    keep: tuple = ()


def canonical(res: Result, mode: int):
    """Result -> canonical (reqs, hdrs[n, max_headers], http) records: the fields
    the reference leaves unspecified for a request that did not parse (its
    method/path/header outputs, phr_parse_request's minor_version, the records
    past num_headers, flags) zeroed, so two parsers compare with one array
    equality and hash to one digest (tests/golden/full_digests.json)."""
    reqs = res.reqs.copy()
    n = len(reqs)
    maxh = res.hdrs.shape[1] if res.hdrs.ndim == 2 else 0
    ok = reqs["ret"] > 0
    if mode == MODE_HTTP:
        ok &= res.http["result"] == 1
    for f in ("method_off", "method_len", "path_off", "path_len", "num_headers"):
        reqs[f][~ok] = 0
    reqs["minor_version"][~ok] = -1
    reqs["flags"] = 0
    h = res.hdrs.copy() if maxh else np.zeros((n, 0), dtype=HDR_DTYPE)   # C order (header-major views too)
    if maxh:
        valid = ok[:, None] & (np.arange(maxh)[None, :] < reqs["num_headers"][:, None])
        for f in h.dtype.names:
            h[f] = np.where(valid, h[f], 0)
    x = None
    if mode == MODE_HTTP:
        x = res.http.copy()
        one = x["result"] == 1
        for f in ("body_kind", "consumed", "body_len"):
            x[f][~one] = 0
    return reqs, h, x


def record_digest(reqs, hdrs, http=None) -> str:
    """sha256 of a canonical record stream: reqs, then hdrs (request-major), then http."""
    import hashlib
    d = hashlib.sha256()
    d.update(np.ascontiguousarray(reqs).tobytes())
    d.update(np.ascontiguousarray(hdrs).tobytes())
    if http is not None:
        d.update(np.ascontiguousarray(http).tobytes())
    return d.hexdigest()


def library_sha256(path: str | None = None) -> str:
    """sha256 of librhp.so as it lies on disk (the file lib() loads): logs and
    profiles carry it so a result can be tied to the binary it came from."""
    import hashlib
    p = path or LIBRHP
    if not os.path.exists(p):
        return "missing"
    return hashlib.sha256(open(p, "rb").read()).hexdigest()


def hdrs_bytes(n: int, max_headers: int, layout: int) -> int:
    """bytes the batch's hdrs buffer needs (rhp.h; RHP_COMPACT_HDRS_BYTES / RHP_DENSE_HDRS_BYTES)"""
    if layout == LAYOUT_COMPACT:
        return ((n * max_headers * 4 + 15) & ~15) + n * max_headers * HDR_DTYPE.itemsize
    if layout in DENSE_LAYOUTS:   # u16 lengths, the u32 overflow area, the wide records
        return ((n * max_headers * 2 + 15) & ~15) + ((n * max_headers * 4 + 15) & ~15) + n * max_headers * HDR_DTYPE.itemsize
    return n * max_headers * HDR_DTYPE.itemsize


def reqs_bytes(n: int, layout: int) -> int:
    """bytes the batch's reqs buffer needs (rhp.h; RHP_DENSE_REQS_BYTES for the dense layout)"""
    if layout in DENSE_LAYOUTS:
        return ((n * 8 + 15) & ~15) + n * REQ_DTYPE.itemsize
    return n * REQ_DTYPE.itemsize


def expand_reqs(raw: np.ndarray, n: int, layout: int) -> np.ndarray:
    """[n] rhp_req_t records of a parsed batch from its raw reqs bytes in any layout
    (rhp_expand_reqs, include/rhp_host.h: dense records expanded)."""
    raw = np.ascontiguousarray(raw).view(np.uint8)
    if layout not in DENSE_LAYOUTS:
        return raw[: n * REQ_DTYPE.itemsize].view(REQ_DTYPE).copy()
    out = np.zeros(n, dtype=REQ_DTYPE)
    if n == 0:
        return out
    b = Batch(None, None, None, 0, n, 0, MODE_PHR, layout, None, None, None, None, 0, 0, None)
    rc = host().rhp_expand_reqs(ctypes.byref(b), _ptr(raw), _ptr(out))
    if rc != 0:
        raise RuntimeError(f"rhp_expand_reqs failed: {rc}")
    return out


def http_bytes(n: int, mode: int, layout: int) -> int:
    """bytes the batch's http buffer needs (rhp.h; RHP_COMPACT_HTTP_BYTES for the compact layout)"""
    if mode != MODE_HTTP:
        return HTTP_DTYPE.itemsize
    if layout in (LAYOUT_COMPACT, LAYOUT_DENSE):   # compact http records and their wide area
        return ((n * 8 + 15) & ~15) + n * HTTP_DTYPE.itemsize
    return n * HTTP_DTYPE.itemsize


def expand_http(reqs: np.ndarray, raw: np.ndarray, n: int, layout: int) -> np.ndarray:
    """[n] rhp_http_t records of a parsed http batch from its raw http bytes in any
    layout (rhp_expand_http, include/rhp_host.h: compact records expanded)."""
    raw = np.ascontiguousarray(raw).view(np.uint8)
    if layout not in (LAYOUT_COMPACT, LAYOUT_DENSE):
        return raw[: n * HTTP_DTYPE.itemsize].view(HTTP_DTYPE).copy()
    out = np.zeros(n, dtype=HTTP_DTYPE)
    if n == 0:
        return out
    reqs = np.ascontiguousarray(reqs)
    b = Batch(None, None, None, 0, n, 0, MODE_HTTP, layout, None, None, None, None, 0, 0, None)
    rc = host().rhp_expand_http(ctypes.byref(b), _ptr(reqs), _ptr(raw), _ptr(out))
    if rc != 0:
        raise RuntimeError(f"rhp_expand_http failed: {rc}")
    return out


def expand_records(reqs: np.ndarray, raw: np.ndarray, n: int, max_headers: int, layout: int) -> np.ndarray:
    """[n, max_headers] rhp_hdr_t records of a parsed batch from its raw hdrs bytes
    in any layout (rhp_expand_records, include/rhp_host.h): records of requests
    with ret <= 0 and past num_headers are zero."""
    out = np.zeros((n, max_headers), dtype=HDR_DTYPE)
    if n == 0 or max_headers == 0:
        return out
    reqs = np.ascontiguousarray(reqs)
    raw = np.ascontiguousarray(raw).view(np.uint8)
    b = Batch(None, None, None, 0, n, max_headers, MODE_PHR, layout, None, None, None, None, 0, 0, None)
    rc = host().rhp_expand_records(ctypes.byref(b), _ptr(reqs), _ptr(raw), _ptr(out))
    if rc != 0:
        raise RuntimeError(f"rhp_expand_records failed: {rc}")
    return out


def hdr_view(flat: np.ndarray, n: int, max_headers: int, layout: int) -> np.ndarray:
    """The [n, max_headers] view of a batch's record array in either layout (include/rhp.h)."""
    if layout == LAYOUT_HEADER_MAJOR:
        return flat[: n * max_headers].reshape(max_headers, n).T
    return flat[: n * max_headers].reshape(n, max_headers)


def _host_batch(buf, off, max_headers, mode, layout=LAYOUT_REQUEST_MAJOR, last_len=None, flags=0):
    n = len(off) - 1
    raw_reqs = np.zeros(max(reqs_bytes(n, layout), 8), dtype=np.uint8)
    reqs = raw_reqs[: n * REQ_DTYPE.itemsize].view(REQ_DTYPE)   # (dense: expanded by _host_done)
    raw = np.zeros(max(hdrs_bytes(n, max_headers, layout), 8), dtype=np.uint8)
    raw_http = np.zeros(max(http_bytes(n, mode, layout), 8), dtype=np.uint8)
    rw = buf.copy()
    b = Batch(_ptr(rw), _ptr(rw), _ptr(off), rw.size, n, max_headers, mode, layout, _ptr(raw_reqs), _ptr(raw),
              _ptr(raw_http), 0, flags, 0, _ptr(last_len) if last_len is not None else None)
    hv = None if layout in LENGTH_LAYOUTS else hdr_view(raw.view(HDR_DTYPE), n, max_headers, layout)
    res = Result(reqs, hv, None, rw)
    res.raw_reqs = raw_reqs
    res.raw_hdrs = raw   # the compact layout's records are expanded once the parse has run (_host_done)
    res.raw_http = raw_http if mode == MODE_HTTP else None
    res.batch, res.keep = b, (rw, off, raw_reqs, raw, raw_http)
    return b, res


def _host_done(res: Result, n: int, max_headers: int, layout: int) -> Result:
    if layout in DENSE_LAYOUTS:
        res.reqs = expand_reqs(res.raw_reqs, n, layout)
    if layout in LENGTH_LAYOUTS:
        res.hdrs = expand_records(res.reqs, res.raw_hdrs, n, max_headers, layout)
    if res.raw_http is not None:
        res.http = expand_http(res.reqs, res.raw_http, n, layout)
    return res


def emulate(buf: np.ndarray, off: np.ndarray, max_headers: int = 16, mode: int = MODE_PHR,
            layout: int = LAYOUT_REQUEST_MAJOR, last_len: np.ndarray | None = None):
    """Run the kernel's DFA algorithm on the CPU (tests).  Returns (Result, stats[3]).
    last_len: optional u64[n], phr_parse_request's last_len per request (phr mode)."""
    if last_len is not None:
        last_len = np.ascontiguousarray(last_len, dtype=np.uint64)
    b, res = _host_batch(buf, off, max_headers, mode, layout, last_len)
    stats = np.zeros(3, dtype=np.uint64)
    rc = host().rhp_emu_parse_batch(ctypes.byref(b), _ptr(stats))
    if rc != 0:
        raise RuntimeError(f"rhp_emu_parse_batch failed: {rc}")
    return _host_done(res, len(off) - 1, max_headers, layout), stats


def parse_cpu_exact(buf: np.ndarray, off: np.ndarray, max_headers: int = 16, mode: int = MODE_PHR,
                    layout: int = LAYOUT_REQUEST_MAJOR):
    """The product's exact scalar parser on the host (rhp_scalar.h), e.g. for the reactor shim."""
    b, res = _host_batch(buf, off, max_headers, mode, layout)
    rc = host().rhp_cpu_parse_batch(ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_parse_batch failed: {rc}")
    return _host_done(res, len(off) - 1, max_headers, layout)


GUARD_BYTE, GUARD_BYTE_ALT = 0xA5, 0x3C   # the guard pattern; the second where the fill is the first


class GuardError(AssertionError):
    """a guard byte beside a buffer no longer holds the pattern"""


def check_guard_bytes(name: str, before: np.ndarray, after: np.ndarray, pattern: int) -> None:
    """Raise GuardError if a byte of `before` (the bytes that end where the
    buffer starts) or `after` (the bytes that start where it ends) is not
    `pattern`: the buffer, the side and the first offset, counted from the
    buffer's start (negative) or from its end."""
    for side, g, base in (("before", before, -len(before)), ("after", after, 0)):
        bad = np.flatnonzero(np.asarray(g) != pattern)
        if len(bad):
            raise GuardError(f"{name}: {len(bad)} guard bytes {side} the buffer overwritten, first at offset "
                             f"{base + int(bad[0])} from its {'start' if side == 'before' else 'end'} "
                             f"(holds 0x{int(g[bad[0]]):02x}, pattern 0x{pattern:02x})")


class Guarded:
    """`size` bytes (tests: a device buffer the library writes) as a slice of a
    larger allocation: `guard` bytes of a pattern directly before and after
    it, `shift` more bytes of the pattern before it.  The slice starts at the
    allocation's base plus a multiple of ALIGN (the alignment of a torch
    allocation) plus `shift`.  fill: the byte the slice holds at first (None:
    zero); the pattern differs from it.  data: the slice's first bytes.
    Without guard and shift the allocation is the plain one (torch.zeros)."""

    ALIGN = 512

    def __init__(self, name: str, size: int, guard: int = 0, fill: int | None = None, device: str = "cuda",
                 shift: int = 0, data: np.ndarray | None = None):
        import torch
        self.name, self.size, self.guard = name, size, guard
        self.pattern = GUARD_BYTE_ALT if fill == GUARD_BYTE else GUARD_BYTE
        self.front = ((guard + self.ALIGN - 1) & ~(self.ALIGN - 1)) + shift
        if self.front or guard:
            self.buf = torch.full((self.front + size + guard,), self.pattern, dtype=torch.uint8, device=device)
            self.view = self.buf[self.front: self.front + size]
            self.view.fill_(fill or 0)
        else:
            self.buf = self.view = (torch.zeros(size, dtype=torch.uint8, device=device) if not fill
                                    else torch.full((size,), fill, dtype=torch.uint8, device=device))
        if data is not None:
            self.view[: data.size].copy_(torch.from_numpy(np.ascontiguousarray(data).view(np.uint8).reshape(-1)))

    def guards(self):
        """(the bytes before the slice, the bytes after it) as host arrays: an ordinary copy"""
        return self.buf[: self.front].cpu().numpy(), self.buf[self.front + self.size:].cpu().numpy()

    def check(self) -> None:
        check_guard_bytes(self.name, *self.guards(), self.pattern)


class DeviceBatch:
    """A batch resident in HBM plus its output buffers (torch tensors as plumbing).

    fill (a byte, tests): reqs, hdrs and http hold it before the launch, not
    zero (rhp.h asks no caller to zero them): a record the parser never wrote
    reads back as the fill.  guard (bytes, tests): reqs, hdrs, http and bytes
    are Guarded slices, with that many pattern bytes on both sides; result()
    then calls check_guards().  bytes_shift (a multiple of 16, tests): bytes /
    bytes_rw point that far into their allocation (rhp.h: 16-byte aligned)."""

    def __init__(self, buf: np.ndarray, off: np.ndarray, max_headers: int = 16, mode: int = MODE_PHR,
                 device: str = "cuda", layout: int = LAYOUT_REQUEST_MAJOR, last_len: np.ndarray | None = None,
                 flags: int = 0, fill: int | None = None, guard: int = 0, bytes_shift: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the rhp product path runs on MI355X only")
        self.n = len(off) - 1
        self.max_headers = max_headers
        self.mode = mode
        self.layout = layout
        self.flags = flags
        self.host_buf, self.host_off = buf, off   # (references: result() describes the parsed batch over them)
        if bytes_shift < 0 or bytes_shift % 16:
            raise ValueError("bytes_shift: a multiple of 16 (rhp.h: bytes is 16-byte aligned)")
        self.fill, self.guard = fill, guard
        self.guarded = {}   # name -> Guarded, the buffers check_guards() looks beside

        def area(name, size, **kw):
            g = self.guarded[name] = Guarded(name, size, guard, device=device, **kw)
            return g.view

        if guard or bytes_shift:
            self.bytes = area("bytes", buf.size, shift=bytes_shift, data=buf)
        else:
            self.bytes = torch.from_numpy(buf).to(device)
        self.offsets = torch.from_numpy(off.view(np.int64)).to(device)
        self.reqs = area("reqs", max(reqs_bytes(self.n, layout), 8), fill=fill)
        self.hdrs = area("hdrs", max(hdrs_bytes(self.n, max_headers, layout), 8), fill=fill)
        self.http = area("http", http_bytes(self.n, mode, layout), fill=fill)
        self.work = torch.zeros(RHP_WORK_WORDS, dtype=torch.int32, device=device)
        self.last_len = (torch.from_numpy(np.ascontiguousarray(last_len, dtype=np.uint64).view(np.int64)).to(device)
                         if last_len is not None else None)

    def desc(self) -> Batch:
        return Batch(self.bytes.data_ptr(), self.bytes.data_ptr(), self.offsets.data_ptr(), self.bytes.numel(),
                     self.n, self.max_headers, self.mode, self.layout, self.reqs.data_ptr(), self.hdrs.data_ptr(),
                     self.http.data_ptr(), self.work.data_ptr(), self.flags, 0,
                     self.last_len.data_ptr() if self.last_len is not None else None)

    def fill_records(self, fill: int | None = None) -> None:
        """reqs, hdrs and http filled again (default: with the batch's fill byte), on the current stream"""
        v = self.fill or 0 if fill is None else fill
        for t in (self.reqs, self.hdrs, self.http):
            t.fill_(v)

    def check_guards(self) -> None:
        """Read the guards back (after a synchronize, ordinary copies); GuardError
        names the buffer, the side and the first offset."""
        import torch
        torch.cuda.synchronize()
        for g in self.guarded.values():
            g.check()

    _runtime_checked = False   # one /proc/self/maps scan per process (it costs ~0.2 ms: not per launch)

    def launch(self, stream=None) -> None:
        d = self.desc()
        if not DeviceBatch._runtime_checked:
            check_one_hip_runtime()   # the device buffers were allocated by torch's runtime by now
            DeviceBatch._runtime_checked = True
        rc = lib().rhp_parse_batch(ctypes.byref(d), _stream(stream))
        if rc != 0:
            raise RuntimeError(f"rhp_parse_batch failed: {rc}")

    def result(self) -> Result:
        import torch
        torch.cuda.synchronize()
        if self.guard:
            self.check_guards()
        raw_reqs = self.reqs.cpu().numpy()
        reqs = expand_reqs(raw_reqs, self.n, self.layout)
        raw = self.hdrs.cpu().numpy()
        hdrs = (expand_records(reqs, raw, self.n, self.max_headers, self.layout)
                if self.layout in LENGTH_LAYOUTS
                else hdr_view(raw.view(HDR_DTYPE), self.n, self.max_headers, self.layout))
        raw_http = self.http.cpu().numpy() if self.mode == MODE_HTTP else None
        http = expand_http(reqs, raw_http, self.n, self.layout) if self.mode == MODE_HTTP else None
        out = self.bytes.cpu().numpy() if self.mode == MODE_HTTP else None
        res = Result(reqs, hdrs, http, out, raw, raw_http, raw_reqs)
        hb = out if out is not None else self.host_buf   # the bytes as the parse left them
        res.batch = Batch(_ptr(hb), _ptr(hb), _ptr(self.host_off), hb.size, self.n, self.max_headers, self.mode,
                          self.layout, _ptr(raw_reqs), _ptr(raw), _ptr(raw_http) if raw_http is not None else None,
                          None, self.flags, 0, None)
        res.keep = (hb, self.host_off, raw_reqs, raw, raw_http)
        return res

    def classifier(self, names, routes=()):
        """rhp_classify_batch over this batch, prepared once: (launch(stream=None),
        fields tensor u8 [n_names * n * 4], route tensor i16 [n] or None).  Each
        launch() is one asynchronous call on the stream (default: the current one)."""
        import torch
        dev = self.reqs.device
        fields = torch.zeros(max(len(names) * self.n, 1) * FIELDREF_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        route = torch.zeros(max(self.n, 1), dtype=torch.int16, device=dev) if len(routes) else None
        *keep, c = _classify_desc(names, routes, fields.data_ptr(), route.data_ptr() if route is not None else None)
        d = self.desc()

        def launch(stream=None, _keep=keep):
            rc = lib().rhp_classify_batch(ctypes.byref(d), ctypes.byref(c), _stream(stream))
            if rc != 0:
                raise RuntimeError(f"rhp_classify_batch failed: {rc}")
        return launch, fields, route

    def classify(self, names, routes=(), stream=None):
        """Header lookup and route match of the parsed batch on the GPU (after
        launch(), on the same stream): (fields FIELDREF_DTYPE [n_names, n], route u16 [n])."""
        import torch
        launch, fields, route = self.classifier(names, routes)
        launch(stream)
        torch.cuda.synchronize()
        return _classify_out(fields, route, len(names), self.n)


def parse_batch(buf: np.ndarray, off: np.ndarray, max_headers: int = 16, mode: int = MODE_PHR,
                impl: int = IMPL_DFA, layout: int = LAYOUT_REQUEST_MAJOR, last_len: np.ndarray | None = None,
                **device_batch) -> Result:
    """Parse a host batch on the GPU (copies in, one launch, copies out).
    device_batch: DeviceBatch's fill / guard / bytes_shift (tests)."""
    with _impl(impl):
        db = DeviceBatch(buf, off, max_headers, mode, layout=layout, last_len=last_len, **device_batch)
        db.launch()
        return db.result()


def classify_tables(names, routes=()):
    """The host tables of rhp_classify_t: (text u8, names u32 [n_names, 2], routes
    u32 [n_routes, 4]) for header names (bytes) and (method, target) routes; an
    empty or None method takes any method."""
    parts, at = [], 0

    def span(b):
        nonlocal at
        b = bytes(b or b"")
        parts.append(b)
        at += len(b)
        return at - len(b), len(b)

    nm = np.array([span(x) for x in names], dtype=np.uint32).reshape(-1, 2)
    rt = np.array([span(m) + span(t) for m, t in routes], dtype=np.uint32).reshape(-1, 4)
    text = np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy()
    return text, nm, rt


def _classify_desc(names, routes, fields_ptr, route_ptr):
    """(text, names, routes, Classify): rhp_classify_t over classify_tables(names,
    routes) and the two output buffers; a table or an output that nothing uses
    is NULL.  The Classify points into the three arrays: keep them alive."""
    text, nm, rt = classify_tables(names, routes)
    return text, nm, rt, Classify(_ptr(text), _ptr(nm) if len(nm) else None, _ptr(rt) if len(rt) else None, len(nm),
                                  len(rt), fields_ptr if len(nm) else None, route_ptr if len(rt) else None)


def _classify_out(fields, route, n_names, n):
    """The output buffers of a classify call, device tensors or numpy arrays, as
    (fields FIELDREF_DTYPE [n_names, n], route u16 [n]); route None (no routes):
    RHP_ROUTE_NONE everywhere."""
    def u8(a):
        return (a if isinstance(a, np.ndarray) else a.cpu().numpy()).reshape(-1).view(np.uint8)
    f = u8(fields)[: n_names * n * FIELDREF_DTYPE.itemsize].view(FIELDREF_DTYPE).reshape(n_names, n)
    r = u8(route)[: n * 2].view(np.uint16) if route is not None else np.full(n, ROUTE_NONE, dtype=np.uint16)
    return f, r


def _batch_of(b_or_res) -> Batch:
    """what a *_cpu form takes first: a Batch, or a Result that describes its batch"""
    b = b_or_res.batch if isinstance(b_or_res, Result) else b_or_res
    if b is None:
        raise ValueError("this Result does not describe its batch")
    return b


def _session_arrays(sessions, results, starts=None, route=None):
    """(sessions, results, req_start, route) of a *_cpu form, contiguous in their dtypes; None stays None"""
    dtypes = (SESSION_DTYPE, SESSION_RESULT_DTYPE, np.uint64, np.uint16)
    return tuple(a if a is None else np.ascontiguousarray(a, dtype=t) for a, t in zip((sessions, results, starts, route), dtypes))


def classify_cpu(res_or_batch, names, routes=()):
    """rhp_cpu_classify_batch (include/rhp_host.h) over a parsed batch in host
    memory: a Result of emulate / parse_cpu_exact / parse_batch / DeviceBatch.result
    (its `batch`), or a Batch.  Returns (fields FIELDREF_DTYPE [n_names, n], route
    u16 [n]; RHP_ROUTE_NONE everywhere without routes)."""
    b = _batch_of(res_or_batch)
    fields = np.zeros((len(names), b.n), dtype=FIELDREF_DTYPE)
    route = np.zeros(b.n, dtype=np.uint16)
    *_keep, c = _classify_desc(names, routes, _ptr(fields), _ptr(route))
    rc = host().rhp_cpu_classify_batch(ctypes.byref(b), ctypes.byref(c))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_classify_batch failed: {rc}")
    return _classify_out(fields, route if len(routes) else None, len(names), b.n)


def classify_batch(buf: np.ndarray, off: np.ndarray, names, routes=(), max_headers: int = 16, mode: int = MODE_PHR,
                   layout: int = LAYOUT_REQUEST_MAJOR):
    """Parse a host batch on the GPU and classify it there, on one stream (copies
    in, two launches, copies the classification out): (fields, route) as classify_cpu."""
    db = DeviceBatch(buf, off, max_headers, mode, layout=layout)
    db.launch()
    return db.classify(names, routes)


def pack_dense_cpu(res: Result, n: int, max_headers: int):
    """rhp_cpu_pack_dense over the request-major http records of `res`: (dreq
    u8[8n], hc u8[8n], lens16 u16[max_headers * n]) -- what rhp_pack_dense makes
    on the device (include/rhp.h), the reactor's copy-back."""
    reqs = np.ascontiguousarray(res.raw_reqs[: n * REQ_DTYPE.itemsize]) if res.raw_reqs is not None \
        else np.ascontiguousarray(res.reqs).view(np.uint8)
    hdrs = np.ascontiguousarray(res.raw_hdrs)
    http = np.ascontiguousarray(res.raw_http)
    b = Batch(None, None, None, 0, n, max_headers, MODE_HTTP, LAYOUT_REQUEST_MAJOR, _ptr(reqs), _ptr(hdrs),
              _ptr(http), 0, 0, 0, None)
    dreq = np.zeros(max(8 * n, 8), dtype=np.uint8)
    hc = np.zeros(max(8 * n, 8), dtype=np.uint8)
    lens = np.zeros(max(max_headers * n, 1), dtype=np.uint16)
    rc = host().rhp_cpu_pack_dense(ctypes.byref(b), _ptr(dreq), _ptr(hc), _ptr(lens))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_pack_dense failed: {rc}")
    return dreq[: 8 * n], hc[: 8 * n], lens[: max_headers * n]


# ---------------------------------------------------------------------------
# Pipelined input (rhp.h rhp_fixup_sessions; the reference's server_session_read
# loop, /root/reference/src/reactor/server.c:37-65): a session's bytes split at
# every empty line into pieces, parsed speculatively, then walked in order.

def split_pieces(data: bytes):
    """Piece lengths of one session's input: a cut after every empty line (LF LF
    or LF CR LF, where a header section can end) and at the end."""
    cuts, n = [], len(data)
    p = data.find(b"\n")
    while p != -1:
        q = p + 1
        if q < n and data[q] == 10:
            cuts.append(q + 1)
        elif q + 1 < n and data[q] == 13 and data[q + 1] == 10:
            cuts.append(q + 2)
        p = data.find(b"\n", p + 1)
    out, at = [], 0
    for c in cuts:
        if c > at and c < n:
            out.append(c - at)
            at = c
    if at < n or not out:
        out.append(n - at)
    return out


def pack_sessions(sessions, split=True):
    """(buf, piece offsets, rhp_session_t array, session byte starts) for a list
    of session inputs packed back to back (split=False: one piece per session;
    a callable: data -> piece lengths, any split of the input)."""
    pieces, sess, starts, at = [], [], [], 0
    for data in sessions:
        lo = len(pieces)
        starts.append(at)
        for ln in (split(data) if callable(split) else split_pieces(data) if split else [len(data)]):
            pieces.append((at, ln))
            at += ln
        sess.append((lo, len(pieces)))
    off = np.zeros(len(pieces) + 1, dtype=np.uint64)
    for i, (a, ln) in enumerate(pieces):
        off[i] = a
    off[len(pieces)] = at
    buf = np.zeros(at + RHP_PAD, dtype=np.uint8)
    if at:
        buf[:at] = np.frombuffer(b"".join(sessions), dtype=np.uint8)
    ss = np.zeros(len(sess), dtype=SESSION_DTYPE)
    for i, (lo, hi) in enumerate(sess):
        ss[i] = (lo, hi)
    return buf, off, ss, np.array(starts, dtype=np.uint64)


def speculative_cpu(buf, off, max_headers: int = 16, emulate_dfa: bool = False, layout: int = LAYOUT_REQUEST_MAJOR):
    """The speculative http batch of the pieces on the host (the exact parser,
    or the kernel's DFA emulation): (Batch, Result over the same records)."""
    b, res = _host_batch(buf, off, max_headers, MODE_HTTP, layout, None, BATCH_SPECULATIVE)
    if emulate_dfa:
        rc = host().rhp_emu_parse_batch(ctypes.byref(b), None)
    else:
        rc = host().rhp_cpu_parse_batch(ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"host parse failed: {rc}")
    return b, res


def whole_pieces(b) -> np.ndarray:
    """bool [n]: the pieces of speculative_cpu's batch that the fix-up's prefix
    takes as they are (rhp_scalar.h fixup_piece_whole, the kernel's predicate)."""
    whole = np.zeros(max(b.n, 1), dtype=np.uint8)
    rc = host().rhp_test_fixup_whole(ctypes.byref(b), _ptr(whole))
    if rc != 0:
        raise RuntimeError(f"rhp_test_fixup_whole failed: {rc}")
    return whole[: b.n].astype(bool)


def fixup_host(b, res, sessions, prefix: bool = False):
    """rhp_cpu_fixup_sessions, or with `prefix` rhp_emu_fixup_sessions (the
    kernel's prefix of whole pieces, then the walk), over the records of
    speculative_cpu.  Returns (Result, session results, req_start)."""
    fn = host().rhp_emu_fixup_sessions if prefix else host().rhp_cpu_fixup_sessions
    out = np.zeros(len(sessions), dtype=SESSION_RESULT_DTYPE)
    starts = np.zeros(max(b.n, 1), dtype=np.uint64)
    rc = fn(ctypes.byref(b), _ptr(sessions), len(sessions), _ptr(out), _ptr(starts))
    if rc != 0:
        raise RuntimeError(f"host session fix-up failed: {rc}")
    return _host_done(res, b.n, b.max_headers, b.layout), out, starts


def fixup_cpu(buf, off, sessions, max_headers: int = 16, emulate_dfa: bool = False, layout: int = LAYOUT_REQUEST_MAJOR,
              prefix: bool = False):
    """Speculative http batch (host exact parser, or the kernel's DFA emulation)
    + rhp_cpu_fixup_sessions (prefix: rhp_emu_fixup_sessions, the host twin of
    the kernel's wave-parallel prefix).  Returns (Result, session results, req_start)."""
    b, res = speculative_cpu(buf, off, max_headers, emulate_dfa, layout)
    return fixup_host(b, res, sessions, prefix)


class _SessionRound:
    """The device side of a session *_gpu form: `db` the speculative http DeviceBatch and `d` its descriptor, the
    sessions uploaded as bytes (a device tensor is taken as it lies, with n_sessions; None: NULL, no session), and
    results, req_start and, where asked for, route as Guarded buffers with the batch's guard, each stated as (bytes,
    fill byte); fields, the same pair, is a plain tensor.  A form runs the steps (fixup and classify, or load), makes
    its own call over the buffers, synchronises once, checks every guard (check; add: one more buffer for it) and
    copies back (result)."""

    def __init__(self, db: DeviceBatch, sessions, results, req_start, route=None, fields=None, n_sessions: int | None = None):
        import torch
        self.db, self.d, self.guard = db, db.desc(), db.guard
        self.ns = n_sessions if n_sessions is not None else 0 if sessions is None else len(sessions)
        if sessions is not None and not torch.is_tensor(sessions):
            sessions = torch.from_numpy(np.ascontiguousarray(sessions).view(np.uint8).reshape(-1).copy()).to("cuda")
        self.sessions = sessions
        self.results, self.req_start, self.route = (
            a if a is None else Guarded(name, a[0], db.guard, fill=a[1])
            for name, a in (("results", results), ("req_start", req_start), ("route", route)))
        self.fields = fields if fields is None else torch.full((fields[0],), fields[1], dtype=torch.uint8, device="cuda")
        self.guarded = [g for g in (self.results, self.req_start, self.route) if g is not None]

    def add(self, g: Guarded) -> Guarded:
        """one more buffer for check()"""
        self.guarded.append(g)
        return g

    def fixup(self) -> None:
        """the parse launch, then rhp_fixup_sessions over what it left; nothing synchronised"""
        self.db.launch()
        fixup_sessions_device(self.d, self.sessions, self.ns, self.results.view, self.req_start.view)

    def classify(self, names, routes) -> None:
        """rhp_classify_sessions after fixup(), into fields and route"""
        classify_sessions_device(self.d, self.sessions, self.ns, self.results.view, self.req_start.view, self.fields,
                                 self.route.view, names, routes)

    def load(self, records) -> None:
        """(raw reqs, raw hdrs, raw http, session results, req_start, route) copied in, in place of fixup and classify"""
        import torch
        for t, a in zip((self.db.reqs, self.db.hdrs, self.db.http, self.results.view, self.req_start.view, self.route.view), records):
            a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
            if a.size:
                t[: a.size].copy_(torch.from_numpy(a.copy()))

    def check(self) -> None:
        """every buffer's guard bytes, the batch's too (after the synchronise); nothing without guard"""
        if self.guard:
            self.db.check_guards()
            for g in self.guarded:
                g.check()

    def result(self, route: bool = False):
        """the host copies: (Result, session results [n_sessions], req_start as allocated), and route u16 [n] on request"""
        out = (self.db.result(), self.results.view.cpu().numpy().view(SESSION_RESULT_DTYPE)[: self.ns],
               self.req_start.view.cpu().numpy().view(np.uint64))
        return out + (self.route.view.cpu().numpy().view(np.uint16)[: self.db.n],) if route else out


def _fixup_round(buf, off, sessions, max_headers, impl, layout=LAYOUT_REQUEST_MAJOR, guard=0) -> _SessionRound:
    """fixup_gpu's round, run and checked: gather_wide_gpu goes on over its device buffers"""
    import torch
    with _impl(impl):
        db = DeviceBatch(buf, off, max_headers, MODE_HTTP, layout=layout, flags=BATCH_SPECULATIVE, guard=guard)
        r = _SessionRound(db, sessions, (len(sessions) * SESSION_RESULT_DTYPE.itemsize, None), (max(db.n, 1) * 8, None))
        r.fixup()
        torch.cuda.synchronize()
        r.check()
    return r


def fixup_gpu(buf, off, sessions, max_headers: int = 16, impl: int = IMPL_DFA, layout: int = LAYOUT_REQUEST_MAJOR,
              with_batch: bool = False, guard: int = 0):
    """Speculative http batch on the GPU + rhp_fixup_sessions, one stream.
    with_batch: the DeviceBatch too, as a fourth value (its device records are
    what the fix-up left: rhp_pack_dense can run over them).  guard (bytes,
    tests): the batch's buffers and the fix-up's two outputs are Guarded, and
    checked once both kernels have run."""
    r = _fixup_round(buf, off, sessions, max_headers, impl, layout, guard)
    return r.result() + ((r.db,) if with_batch else ())


def fixup_sessions_device(d: Batch, sessions_t, n_sessions: int, results_t, starts_t, stream=None):
    """One rhp_fixup_sessions call over device tensors on the stream (default: the current one): `d` the
    speculative batch's descriptor as rhp_parse_batch left it, sessions_t (8 * n_sessions bytes); the session
    results are left in results_t (16 * n_sessions bytes) and req_start in starts_t (8 * n bytes).  Nothing is
    synchronised or copied: the tensors are the call's only inputs and outputs."""
    vp = ctypes.c_void_p
    rc = lib().rhp_fixup_sessions(ctypes.byref(d), vp(_addr(sessions_t)), n_sessions, vp(_addr(results_t)),
                                  vp(_addr(starts_t)), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_fixup_sessions failed: {rc}")


def classify_sessions_device(d: Batch, sessions_t, n_sessions: int, results_t, starts_t, fields_t, route_t, names=(), routes=(),
                             *, tables=None, stream=None):
    """One rhp_classify_sessions call over device tensors on the stream (default: the current one): `d` the batch's
    descriptor after the fix-up, whose results_t and starts_t it reads; fields_t (4 * n_names * n bytes) and route_t
    (2 * n bytes) are the outputs.  The host tables are classify_tables(names, routes), or `tables`: (text, names,
    routes) as that function returns them, where the caller owns the arrays (they may be freed or overwritten once
    the call has returned).  Nothing is synchronised or copied."""
    text, nm, rt = tables if tables is not None else classify_tables(names, routes)
    c = Classify(_ptr(text), _ptr(nm) if len(nm) else None, _ptr(rt) if len(rt) else None, len(nm), len(rt),
                 _addr(fields_t) if len(nm) else None, _addr(route_t) if len(rt) else None)
    vp = ctypes.c_void_p
    rc = lib().rhp_classify_sessions(ctypes.byref(d), vp(_addr(sessions_t)), n_sessions, vp(_addr(results_t)),
                                     vp(_addr(starts_t)), ctypes.byref(c), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_classify_sessions failed: {rc}")


def classify_sessions_cpu(b_or_res, sessions, results, starts, names, routes=()):
    """rhp_cpu_classify_sessions (include/rhp_host.h) over a speculative batch in
    host memory after a fix-up: the Batch of speculative_cpu, or a Result that
    describes its batch (fixup_cpu's, fixup_gpu's), with the fix-up's session
    results and req_start.  Returns (fields FIELDREF_DTYPE [n_names, n], route
    u16 [n]) by record slot."""
    b = _batch_of(b_or_res)
    sessions, results, starts, _ = _session_arrays(sessions, results, starts)
    fields = np.zeros((len(names), b.n), dtype=FIELDREF_DTYPE)
    route = np.zeros(b.n, dtype=np.uint16)
    *_keep, c = _classify_desc(names, routes, _ptr(fields), _ptr(route))
    rc = host().rhp_cpu_classify_sessions(ctypes.byref(b), _ptr(sessions), len(sessions), _ptr(results), _ptr(starts),
                                          ctypes.byref(c))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_classify_sessions failed: {rc}")
    return _classify_out(fields, route if len(routes) else None, len(names), b.n)


def classify_sessions_gpu(buf, off, sessions, names, routes=(), max_headers: int = 16, impl: int = IMPL_DFA,
                          layout: int = LAYOUT_REQUEST_MAJOR, fill: int | None = None):
    """Speculative http batch on the GPU + rhp_fixup_sessions +
    rhp_classify_sessions, three launches on one stream.  Returns (fields, route)
    as classify_sessions_cpu, then what fixup_gpu returns: (Result, session
    results, req_start).  fill (a byte, tests): the record buffers, req_start and
    the session results hold it before the first launch, so that a slot the
    fix-up never wrote reads back as that byte."""
    import torch
    with _impl(impl):
        db = DeviceBatch(buf, off, max_headers, MODE_HTTP, layout=layout, flags=BATCH_SPECULATIVE, fill=fill)
        # (the outputs hold 0xA5 first: the kernel writes every slot)
        r = _SessionRound(db, sessions, (len(sessions) * SESSION_RESULT_DTYPE.itemsize, fill), (max(db.n, 1) * 8, fill),
                          route=(max(db.n, 1) * 2, GUARD_BYTE),
                          fields=(max(len(names) * db.n, 1) * FIELDREF_DTYPE.itemsize, GUARD_BYTE))
        r.fixup()
        r.classify(names, routes)
        torch.cuda.synchronize()
        r.check()
        return _classify_out(r.fields, r.route.view if len(routes) else None, len(names), db.n) + r.result()


# ---------------------------------------------------------------------------
# Batched response serialization: http_write_response (src/reactor/http.c:286-297)
# for n responses on the device (rhp_writer.hip).  A batch is an arena of bytes
# plus rhp_resp_t records (n x 8 u32: status off,len, type off,len, body off,len,
# fields_first, fields_count) and rhp_resp_field_t records (m x 4 u32).

RESP_STATUS = (b"200 OK", b"404 Not Found", b"500 Internal Server Error", b"204 No Content",
               b"101 Switching Protocols")
RESP_TYPES = (b"text/plain", b"application/json", b"text/html; charset=UTF-8")
RESP_FIELD_NAMES = (b"Cookie", b"Set-Cookie", b"X-Request-Id", b"Cache-Control")
DEFAULT_DATE = b"Wed, 16 Aug 2023 10:29:23 GMT"


EDGE_SPAN_LENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 143, 144, 145, 255, 256, 257,
                  1023, 1024, 1025)
EDGE_BODY_LENS = (0, 9, 10, 99, 100, 999, 1000, 9999, 10000)
EDGE_FIELD_COUNTS = (0, 0, 1, 2, 7)
EDGE_COOP_BODY = 17000   # larger than the writer's 16 KiB stage


def _edge_responses(n: int, seed: int, coop: bool):
    """make_responses kinds "edge" and "edge-coop" (vectorised: one draw per column)"""
    rng = np.random.default_rng(seed)
    arena = rng.integers(0x20, 0x7F, size=(1 << 15) + 3, dtype=np.uint8)   # (a length that is no multiple of 4)
    lens = np.array(EDGE_SPAN_LENS, dtype=np.int64)

    def spans(ln):
        """a random start for every length; a quarter of the empty spans at the arena's end"""
        off = rng.integers(0, len(arena) - ln + 1)
        at_end = (ln == 0) & (rng.random(len(ln)) < 0.25)
        return np.where(at_end, len(arena), off)

    def pick(count):
        return lens[rng.integers(0, len(lens), size=count)]

    st, ty = pick(n), pick(n)
    body = np.where(rng.random(n) < 0.5, pick(n),
                    np.array(EDGE_BODY_LENS, dtype=np.int64)[rng.integers(0, len(EDGE_BODY_LENS), size=n)])
    if coop:
        body[::64] = EDGE_COOP_BODY
    nf = np.array(EDGE_FIELD_COUNTS, dtype=np.int64)[rng.integers(0, len(EDGE_FIELD_COUNTS), size=n)]
    m = int(nf.sum())
    name, value = pick(m), pick(m)
    resps = np.zeros((n, 8), dtype=np.uint32)
    for col, ln in ((0, st), (2, ty), (4, body)):
        resps[:, col], resps[:, col + 1] = spans(ln), ln
    resps[:, 6], resps[:, 7] = np.cumsum(nf) - nf, nf
    fields = np.zeros((m, 4), dtype=np.uint32)
    for col, ln in ((0, name), (2, value)):
        fields[:, col], fields[:, col + 1] = spans(ln), ln
    return arena, resps, fields


def make_responses(n: int, seed: int, kind: str = "mixed"):
    """Synthetic response batch (arena, resps, fields).  kind "plaintext": every
    response is the TechEmpower plaintext reply (200 OK, text/plain,
    "Hello, World!"); "mixed": seeded statuses/types, 0-3 extra fields, body
    lengths 0-2000 B with 1 % up to 100 kB (all digit counts of Content-Length).
    "edge": every status, type, field name and field value, and half of the
    bodies, has a length from EDGE_SPAN_LENS (around every power of two the
    writer's copy loops step by, and the 128 B switch of its cooperative copy),
    the other bodies one from EDGE_BODY_LENS (Content-Length digit counts);
    every span starts at a random arena byte (all four source alignments), some
    empty spans at the arena's end; EDGE_FIELD_COUNTS extra fields.
    "edge-coop": "edge" with an EDGE_COOP_BODY-byte body in every 64th response,
    so that every group of 64 is larger than the writer's stage."""
    if kind in ("edge", "edge-coop"):
        return _edge_responses(n, seed, kind == "edge-coop")
    if kind not in ("plaintext", "mixed"):
        raise ValueError(f"unknown response kind {kind!r}")
    rng = np.random.default_rng(seed)
    parts, pos = [], 0

    def add(b: bytes):
        nonlocal pos
        parts.append(b)
        pos += len(b)
        return pos - len(b), len(b)

    st = [add(x) for x in RESP_STATUS]
    ty = [add(x) for x in RESP_TYPES]
    nm = [add(x) for x in RESP_FIELD_NAMES]
    resps = np.zeros((n, 8), dtype=np.uint32)
    fields = []
    if kind == "plaintext":
        body = add(b"Hello, World!")
        resps[:] = [st[0][0], st[0][1], ty[0][0], ty[0][1], body[0], body[1], 0, 0]
    else:
        pool = rng.integers(0x20, 0x7F, size=1 << 17, dtype=np.uint8).tobytes()
        pool_off, _ = add(pool)
        for i in range(n):
            s_, t_ = st[int(rng.integers(len(st)))], ty[int(rng.integers(len(ty)))]
            blen = int(rng.integers(0, 100001)) if rng.random() < 0.01 else int(rng.integers(0, 2001))
            bo = pool_off + int(rng.integers(0, len(pool) - blen + 1))
            nf = int(rng.integers(0, 4))
            first = len(fields)
            for _ in range(nf):
                vlen = int(rng.integers(0, 48))
                fields.append([*nm[int(rng.integers(len(nm)))], pool_off + int(rng.integers(0, 4096)), vlen])
            resps[i] = [s_[0], s_[1], t_[0], t_[1], bo, blen, first, nf]
    arena = np.frombuffer(b"".join(parts), dtype=np.uint8).copy()
    f = np.array(fields, dtype=np.uint32).reshape(-1, 4) if fields else np.zeros((0, 4), dtype=np.uint32)
    return arena, resps, f


class DeviceResponses:
    """A response batch resident in HBM and its output (torch tensors as plumbing).

    out_shift, arena_shift (bytes, tests): the `out` and `arena` pointers handed
    to the library are an allocation's base plus the shift, so every alignment
    of either can be run.  guard (bytes, tests): that many bytes of 0xA5 lie
    directly before and after the out_size bytes of `out`, and result() returns
    them too.  out_size 0: `out` is NULL (sizes only, rhp.h)."""

    GUARD_BYTE = 0xA5

    def __init__(self, arena: np.ndarray, resps: np.ndarray, fields: np.ndarray, date: bytes = DEFAULT_DATE,
                 out_size: int | None = None, device: str = "cuda", out_shift: int = 0, arena_shift: int = 0,
                 guard: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible: the rhp product path runs on MI355X only")
        self.n = len(resps)
        self.date = bytes(date)
        arena = np.ascontiguousarray(arena, dtype=np.uint8)
        if arena_shift or len(arena) & 3:   # (the arena's bytes moved up;) readable to the next 4-byte boundary (rhp.h)
            moved = np.full((arena_shift + len(arena) + 3) & ~3, 0xEE, dtype=np.uint8)
            moved[arena_shift: arena_shift + len(arena)] = arena
            arena = moved
        self.arena = torch.from_numpy(arena).to(device)
        self.arena_shift = arena_shift
        self.resps = torch.from_numpy(np.ascontiguousarray(resps, dtype=np.uint32).view(np.int32)).to(device)
        fl = np.ascontiguousarray(fields, dtype=np.uint32).reshape(-1, 4)
        self.fields = torch.from_numpy(fl.view(np.int32)).to(device) if len(fl) else None
        self.out_off = torch.zeros(self.n + 1, dtype=torch.int64, device=device)
        if out_size is None:   # exact size from the host copy of the records
            r = np.asarray(resps, dtype=np.uint64).reshape(-1, 8)
            extra = 0
            if len(fl):
                fl64 = fl.astype(np.uint64)
                per = fl64[:, 1] + fl64[:, 3] + 4
                extra = int(sum(int(per[a:a + c].sum()) for a, c in zip(r[:, 6], r[:, 7]) if c))
            digits = np.array([len(str(int(v))) for v in r[:, 5]], dtype=np.uint64)
            out_size = int((95 + r[:, 1] + r[:, 3] + r[:, 5] + digits).sum()) + extra
        # [front: guard rounded up to 256 B, + out_shift][out_size bytes][guard]; front and back hold GUARD_BYTE
        self.guard = guard
        self.front = ((guard + 255) & ~255) + out_shift
        self.buf = torch.zeros(self.front + max(out_size, 1) + guard, dtype=torch.uint8, device=device)
        if self.front:
            self.buf[: self.front] = self.GUARD_BYTE
        if guard:
            self.buf[self.front + out_size:] = self.GUARD_BYTE
        self.out = self.buf[self.front: self.front + max(out_size, 1)]
        self.out_size = out_size
        self.work = torch.zeros((self.n + 4095) // 4096 + 1, dtype=torch.int64, device=device)

    def desc(self) -> RespBatch:
        return RespBatch(self.arena.data_ptr() + self.arena_shift, self.resps.data_ptr(),
                         self.fields.data_ptr() if self.fields is not None else None, self.n, len(self.date),
                         self.date, self.out_off.data_ptr(), self.out.data_ptr() if self.out_size else None,
                         self.out_size, self.work.data_ptr())

    def launch(self, stream=None) -> None:
        d = self.desc()
        rc = lib().rhp_write_responses(ctypes.byref(d), _stream(stream))
        if rc != 0:
            raise RuntimeError(f"rhp_write_responses failed: {rc}")

    def result(self):
        """(bytes, offsets[n + 1]); with a guard, also the guard bytes before and after `out`"""
        import torch
        torch.cuda.synchronize()
        off = self.out_off.cpu().numpy().view(np.uint64)
        buf = self.buf.cpu().numpy()
        out = buf[self.front: self.front + self.out_size][: int(off[-1])]
        if not self.guard:
            return out, off
        return out, off, buf[self.front - self.guard: self.front], buf[self.front + self.out_size:]


def write_responses(arena: np.ndarray, resps: np.ndarray, fields: np.ndarray, date: bytes = DEFAULT_DATE):
    """Serialize a host response batch on the GPU (copies in, one call, copies out):
    returns (bytes, offsets[n + 1])."""
    d = DeviceResponses(arena, resps, fields, date)
    d.launch()
    return d.result()


# ---------------------------------------------------------------------------
# Static routes answered on the device (rhp.h rhp_reply_sessions): route[] and the
# fix-up's results -> every session's reply bytes, copied from one serialized
# reply per route (the `out` / `out_off` of a write_responses call).

REPLY_POISON = 0xFF   # what replies, total, out and work hold before a call (tests)


def _addr(a) -> int | None:
    """the address of a numpy array's or a torch tensor's first element"""
    if a is None:
        return None
    return a.ctypes.data if isinstance(a, np.ndarray) else a.data_ptr()


def reply_table(images, image_off, static_mask: int) -> ReplyTable:
    """rhp_reply_table_t over `images` (u8) and `image_off` (u64 / i64 [n_routes + 1]): both numpy arrays (the
    host twin) or both torch device tensors; slices are taken at their first element.  Keep them alive."""
    return ReplyTable(_addr(images), _addr(image_off), len(image_off) - 1, static_mask)


def response_sizes(resps, fields) -> np.ndarray:
    """bytes of every serialized response of a make_responses-style batch (http.c:244-246, 270-272), on the host"""
    r = np.asarray(resps, dtype=np.uint64).reshape(-1, 8)
    fl = np.asarray(fields, dtype=np.uint64).reshape(-1, 4)
    per = fl[:, 1] + fl[:, 3] + 4 if len(fl) else np.zeros(0, dtype=np.uint64)
    extra = np.array([int(per[int(a): int(a) + int(c)].sum()) for a, c in zip(r[:, 6], r[:, 7])], dtype=np.uint64)
    digits = np.array([len(str(int(v))) for v in r[:, 5]], dtype=np.uint64)
    return 95 + r[:, 1] + r[:, 3] + r[:, 5] + digits + extra


def reply_sessions_cpu(b_or_res, sessions, results, route, images, image_off, static_mask: int,
                       out_size: int | None = None, out_shift: int = 0):
    """rhp_cpu_reply_sessions (include/rhp_host.h) over a speculative batch in host memory after a fix-up and a
    classify (the Batch of speculative_cpu or a Result that describes its batch; route u16 [n] by record slot).
    Returns (replies SESSION_REPLY_DTYPE [n_sessions], total, out u8 [out_size]): every output held REPLY_POISON
    before the call.  out_size None: the exact size, from a sizes-only call first.  out_shift: `out` starts that
    many bytes after a 16-byte boundary."""
    b = _batch_of(b_or_res)
    sessions, results, _, route = _session_arrays(sessions, results, route=route)
    image_off = np.ascontiguousarray(image_off, dtype=np.uint64)
    t = reply_table(images, image_off, static_mask)
    ns = len(sessions)
    work = np.full(reply_work_words(b.n, ns), REPLY_POISON, dtype=np.uint8).repeat(8)

    def call(size, shift):
        replies = np.full(max(ns, 1) * SESSION_REPLY_DTYPE.itemsize, REPLY_POISON, dtype=np.uint8)
        total = np.full(8, REPLY_POISON, dtype=np.uint8)
        out = _aligned(size, shift, REPLY_POISON)
        o = ReplyOut(_ptr(replies), _ptr(total), _ptr(out) if size else None, size, _ptr(work))
        rc = host().rhp_cpu_reply_sessions(ctypes.byref(b), _ptr(sessions), ns, _ptr(results), _ptr(route),
                                           ctypes.byref(t), ctypes.byref(o))
        if rc != 0:
            raise RuntimeError(f"rhp_cpu_reply_sessions failed: {rc}")
        return replies.view(SESSION_REPLY_DTYPE)[:ns], int(total.view(np.uint64)[0]), out

    if out_size is None:
        out_size = call(0, 0)[1]
    return call(out_size, out_shift)


def reply_sessions_device(d: Batch, sessions_t, n_sessions: int, results_t, route_t, images_t, image_off_t,
                          static_mask: int, out_size: int, guard: int = 0, out_shift: int = 0, stream=None):
    """One rhp_reply_sessions call over device buffers (torch tensors; `d` the parsed, fixed-up batch's descriptor)
    on the stream (default: the current one).  replies, total, out and work are Guarded (guard bytes on both
    sides, `out` out_shift bytes into its allocation) and hold REPLY_POISON first.  Returns finish(): synchronize,
    check the guards, (replies SESSION_REPLY_DTYPE [n_sessions], total, out u8 [out_size])."""
    import torch
    g = {"replies": Guarded("replies", max(n_sessions, 1) * SESSION_REPLY_DTYPE.itemsize, guard, fill=REPLY_POISON),
         "total": Guarded("total", 8, guard, fill=REPLY_POISON),
         "out": Guarded("out", max(out_size, 1), guard, fill=REPLY_POISON, shift=out_shift),
         "work": Guarded("work", reply_work_words(d.n, n_sessions) * 8, guard, fill=REPLY_POISON)}
    t = reply_table(images_t, image_off_t, static_mask)
    o = ReplyOut(g["replies"].view.data_ptr(), g["total"].view.data_ptr(), g["out"].view.data_ptr() if out_size else None,
                 out_size, g["work"].view.data_ptr())
    vp = ctypes.c_void_p
    rc = lib().rhp_reply_sessions(ctypes.byref(d), vp(_addr(sessions_t)), n_sessions, vp(_addr(results_t)),
                                  vp(_addr(route_t)), ctypes.byref(t), ctypes.byref(o), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_reply_sessions failed: {rc}")

    def finish(_keep=(sessions_t, results_t, route_t, images_t, image_off_t)):
        torch.cuda.synchronize()
        if guard:
            for x in g.values():
                x.check()
        replies = g["replies"].view.cpu().numpy().view(SESSION_REPLY_DTYPE)[:n_sessions]
        total = int(g["total"].view.cpu().numpy().view(np.uint64)[0])
        return replies, total, g["out"].view.cpu().numpy()[:out_size]
    return finish


def reply_sessions_gpu(buf, off, sessions, names, routes, resps_for_routes, static_mask: int, max_headers: int = 16,
                       impl: int = IMPL_DFA, layout: int = LAYOUT_REQUEST_MAJOR, guard: int = 0,
                       out_size: int | None = None, out_shift: int = 0, date: bytes = DEFAULT_DATE, details: bool = False):
    """A round of pipelined input answered on the GPU: speculative parse -> rhp_fixup_sessions ->
    rhp_classify_sessions -> rhp_write_responses over resps_for_routes (arena, resps, fields: one response per
    route, the reply images) -> rhp_reply_sessions, on one stream with no synchronisation in between.  out_size
    None: every slot's worth of the largest image.  Returns (replies, total, out bytes) as reply_sessions_device;
    details: also (Result, session results, route u16 [n]) as the GPU left them."""
    arena, resps, fields = resps_for_routes
    if len(resps) != len(routes):
        raise ValueError("one response per route")
    with _impl(impl):
        db = DeviceBatch(buf, off, max_headers, MODE_HTTP, layout=layout, flags=BATCH_SPECULATIVE, guard=guard)
        r = _SessionRound(db, sessions, (max(len(sessions), 1) * SESSION_RESULT_DTYPE.itemsize, REPLY_POISON),
                          (max(db.n, 1) * 8, REPLY_POISON), route=(max(db.n, 1) * 2, GUARD_BYTE))
        images = DeviceResponses(arena, resps, fields, date)
        if out_size is None:
            out_size = db.n * int(response_sizes(resps, fields).max())
        r.fixup()
        r.classify((), routes)
        images.launch()
        out = reply_sessions_device(r.d, r.sessions, r.ns, r.results.view, r.route.view, images.out, images.out_off,
                                    static_mask, out_size, guard, out_shift)()   # (synchronizes)
        r.check()
        if not details:
            return out
        res, results, _, route = r.result(route=True)
        return out + (res, results, route)


# ---------------------------------------------------------------------------
# The wide slots of a round in one area (rhp.h rhp_gather_wide): after the
# parse, the fix-up and the dense pack, the records of the slots the dense copies
# cannot hold and the de-framed chunked bodies, in three small contiguous areas.

WIDE_POISON = 0xFF   # what totals, the three areas and work hold before a call (tests)


def _wide_out(totals, slots, hdrs, body, work, caps) -> WideOut:
    """rhp_wide_out_t over numpy arrays or torch tensors; an area whose cap is 0 is NULL"""
    return WideOut(_addr(totals), _addr(slots) if caps[0] else None, caps[0], _addr(hdrs) if caps[1] else None, caps[1],
                   _addr(body) if caps[2] else None, caps[2], _addr(work))


def _wide_result(totals, slots, hdrs, body, caps):
    """(totals WIDE_TOTALS_DTYPE scalar, slots WIDE_SLOT_DTYPE [cap_slots], hdrs HDR_DTYPE [cap_hdrs], body u8
    [cap_body]) from the bytes of the four outputs"""
    return (totals.view(WIDE_TOTALS_DTYPE)[0], slots[: caps[0] * 64].view(WIDE_SLOT_DTYPE),
            hdrs[: caps[1] * 8].view(HDR_DTYPE), body[: caps[2]])


def gather_wide_cpu(b_or_res, sessions, results, starts, dreq, hc, caps=None, body_shift: int = 0):
    """rhp_cpu_gather_wide (include/rhp_host.h) over a speculative request-major batch in host memory after a
    fix-up (the Batch of speculative_cpu or a Result that describes its batch) and its dense pack (dreq, hc of
    pack_dense_cpu).  caps (cap_slots, cap_hdrs, cap_body); None: the exact ones, from a totals-only call first.
    Returns (totals, slots [cap_slots], hdrs [cap_hdrs], body [cap_body]): every output held WIDE_POISON before
    the call.  body_shift: `body` starts that many bytes after a 16-byte boundary."""
    b = _batch_of(b_or_res)
    sessions, results, starts, _ = _session_arrays(sessions, results, starts)
    dreq, hc = np.ascontiguousarray(dreq).view(np.uint8), np.ascontiguousarray(hc).view(np.uint8)
    work = np.full(wide_work_words(b.n) * 8, WIDE_POISON, dtype=np.uint8)

    def call(caps):
        totals, slots, hdrs, body = (_aligned(size, shift, WIDE_POISON) for size, shift in
                                     ((16, 0), (caps[0] * 64, 0), (caps[1] * 8, 0), (caps[2], body_shift)))
        o = _wide_out(totals, slots, hdrs, body, work, caps)
        rc = host().rhp_cpu_gather_wide(ctypes.byref(b), _ptr(sessions), len(sessions), _ptr(results), _ptr(starts),
                                        _ptr(dreq), _ptr(hc), ctypes.byref(o))
        if rc != 0:
            raise RuntimeError(f"rhp_cpu_gather_wide failed: {rc}")
        return _wide_result(totals, slots, hdrs, body, caps)

    if caps is None:
        t = call((0, 0, 0))[0]
        caps = (int(t["n_wide"]), int(t["n_hdrs"]), int(t["body_bytes"]))
    return call(tuple(int(c) for c in caps))


def gather_wide_device(d: Batch, sessions_t, n_sessions: int, results_t, starts_t, dreq_t, hc_t, caps, guard: int = 0,
                       body_shift: int = 0, stream=None):
    """One rhp_gather_wide call over device buffers (torch tensors; `d` the parsed, fixed-up and packed batch's
    descriptor) on the stream (default: the current one).  totals, slots, hdrs, body and work are Guarded (guard
    bytes on both sides, `body` body_shift bytes into its allocation) and hold WIDE_POISON first.  Returns
    finish(): synchronize, check the guards, (totals, slots, hdrs, body) as gather_wide_cpu."""
    import torch
    caps = tuple(int(c) for c in caps)
    g = {"totals": Guarded("totals", 16, guard, fill=WIDE_POISON),
         "slots": Guarded("slots", max(caps[0] * 64, 1), guard, fill=WIDE_POISON),
         "hdrs": Guarded("wide hdrs", max(caps[1] * 8, 1), guard, fill=WIDE_POISON),
         "body": Guarded("body", max(caps[2], 1), guard, fill=WIDE_POISON, shift=body_shift),
         "work": Guarded("work", wide_work_words(d.n) * 8, guard, fill=WIDE_POISON)}
    o = _wide_out(*(g[k].view for k in ("totals", "slots", "hdrs", "body", "work")), caps)
    vp = ctypes.c_void_p
    rc = lib().rhp_gather_wide(ctypes.byref(d), vp(_addr(sessions_t)), n_sessions, vp(_addr(results_t)), vp(_addr(starts_t)),
                               vp(_addr(dreq_t)), vp(_addr(hc_t)), ctypes.byref(o), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_gather_wide failed: {rc}")

    def finish(_keep=(sessions_t, results_t, starts_t, dreq_t, hc_t)):
        torch.cuda.synchronize()
        if guard:
            for x in g.values():
                x.check()
        return _wide_result(*(g[k].view.cpu().numpy() for k in ("totals", "slots", "hdrs", "body")), caps)
    return finish


def pack_dense_device(db: "DeviceBatch", guard: int = 0, stream=None, outs=None):
    """rhp_pack_dense over the device records of `db` as they are now, on the stream (default: the current one): the
    three outputs as Guarded device buffers (dreq 8n, hc 8n, lens16 2 * max_headers * n bytes), holding WIDE_POISON
    first.  outs: (dreq, hc, lens16) device tensors of those sizes that the caller made instead; nothing is then
    allocated or filled, and they are returned.  `db`: a DeviceBatch, or anything with its n, max_headers and desc()."""
    n, m = db.n, db.max_headers
    if outs is None:
        outs = [Guarded(name, max(size, 8), guard, fill=WIDE_POISON) for name, size in
                (("dreq", 8 * n), ("hc", 8 * n), ("lens16", 2 * m * n))]
    d = db.desc()
    rc = lib().rhp_pack_dense(ctypes.byref(d), *(_addr(o.view if isinstance(o, Guarded) else o) for o in outs), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_pack_dense failed: {rc}")
    return outs


def gather_wide_gpu(buf, off, sessions, max_headers: int = 16, impl: int = IMPL_DFA, caps=None, guard: int = 0,
                    body_shift: int = 0, details: bool = False):
    """A round of pipelined input on the GPU up to its one D2H: speculative parse -> rhp_fixup_sessions
    (fixup_gpu) -> rhp_pack_dense -> rhp_gather_wide.  caps None: the exact ones, from a totals-only call first.
    Returns (totals, slots, hdrs, body) as gather_wide_cpu; details: also (Result, session results, req_start,
    dreq u8 [8n], hc u8 [8n], lens16 u16 [max_headers * n]) as the GPU left them."""
    r = _fixup_round(buf, off, np.ascontiguousarray(sessions, dtype=SESSION_DTYPE), max_headers, impl, guard=guard)
    db, n = r.db, r.db.n
    packed = pack_dense_device(db, guard)

    def call(caps):
        return gather_wide_device(r.d, r.sessions, r.ns, r.results.view, r.req_start.view, packed[0].view, packed[1].view,
                                  caps, guard, body_shift)()

    if caps is None:
        t = call((0, 0, 0))[0]
        caps = (int(t["n_wide"]), int(t["n_hdrs"]), int(t["body_bytes"]))
    out = call(caps)
    if guard:
        db.check_guards()
        for x in packed:
            x.check()
    if not details:
        return out
    dreq, hc, lens = (x.view.cpu().numpy() for x in packed)
    return out + r.result() + (dreq[: 8 * n], hc[: 8 * n], lens.view(np.uint16)[: max_headers * n])


def rebuild_records(n: int, max_headers: int, sessions, results, dreq, hc, lens16, totals, slots, hdrs, body):
    """What the reactor holds after one D2H, from the dense copies (dreq, hc, lens16 of rhp_pack_dense), the
    fix-up's session results and the three gathered areas of rhp_gather_wide alone: a dict with
      in_use     bool [n]: the record slots the sessions own (rhp.h)
      wide       bool [n]: the in-use slots found in slots[]
      reqs       REQ_DTYPE [n], hdrs HDR_DTYPE [n, max_headers], http HTTP_DTYPE [n]: the records of the in-use
                 slots, the dense ones expanded (rhp_expand_reqs / _records / _http over an RHP_LAYOUT_DENSE
                 image whose wide areas hold the gathered records), zero elsewhere; of a slot whose http result
                 is not 1 only that result means anything (rhp.h)
      req_start  {slot: req_start} of the wide slots
      bodies     {slot: bytes} of the gathered bodies.
    The wide slots are visited with a cursor over slots[], which ascend by slot."""
    m = max_headers
    sessions = np.ascontiguousarray(sessions, dtype=SESSION_DTYPE)
    results = np.ascontiguousarray(results, dtype=SESSION_RESULT_DTYPE)
    dreq = np.ascontiguousarray(dreq).view(np.uint8)[: 8 * n].view(REQ_DENSE_DTYPE).copy()
    hc = np.ascontiguousarray(hc).view(np.uint8)[: 8 * n].view(HTTP_COMPACT_DTYPE).copy()
    lens16 = np.ascontiguousarray(lens16).view(np.uint16)[: m * n]
    nw = int(totals["n_wide"])
    slots = slots[:nw]
    in_use = np.zeros(n, dtype=bool)
    for (lo, hi), k in zip(sessions.tolist(), results["n_slots"].tolist()):
        if lo + k <= hi <= n:
            in_use[lo: lo + k] = True
    # an RHP_LAYOUT_DENSE image of the round: the dense copies, the gathered records in the wide areas
    raw_reqs = np.zeros(max(reqs_bytes(n, LAYOUT_DENSE), 8), dtype=np.uint8)
    raw_hdrs = np.zeros(max(hdrs_bytes(n, m, LAYOUT_DENSE), 8), dtype=np.uint8)
    raw_http = np.zeros(max(http_bytes(n, MODE_HTTP, LAYOUT_DENSE), 8), dtype=np.uint8)
    wide_reqs = raw_reqs[(n * 8 + 15) & ~15:][: n * 16].view(REQ_DTYPE)
    wide_hdrs = raw_hdrs[hdrs_bytes(n, m, LAYOUT_DENSE) - n * m * 8:][: n * m * 8].view(HDR_DTYPE).reshape(n, m)
    wide_http = raw_http[(n * 8 + 15) & ~15:][: n * 24].view(HTTP_DTYPE)
    wide = np.zeros(n, dtype=bool)
    req_start, bodies, cursor = {}, {}, 0
    for i in np.flatnonzero(in_use).tolist():   # the dispatch loop: ascending slots, a cursor over slots[]
        if cursor < nw and int(slots["slot"][cursor]) == i:
            w = slots[cursor]
            cursor += 1
            wide[i] = True
            wide_reqs[i], wide_http[i] = w["req"], w["http"]
            wide_reqs["flags"][i] |= F_WIDE   # (in the dense image: its header records are the wide ones)
            r, x = w["req"], w["http"]
            nh = int(r["num_headers"]) if x["result"] == 1 and r["ret"] > 0 and r["num_headers"] <= m else 0
            wide_hdrs[i, :nh] = hdrs[int(w["hdr_first"]): int(w["hdr_first"]) + nh]
            req_start[i] = int(w["req_start"])
            if int(w["body_off"]) != WIDE_NO_BODY:
                bodies[i] = bytes(body[int(w["body_off"]): int(w["body_off"]) + int(x["body_len"])])
    assert cursor == nw, "slots[] holds a slot that is not in use, or out of order"
    # a wide slot reads its records from the wide areas whatever its dense copies say
    dreq["flags"][wide] = DENSE_WIDE
    hc["flags"][wide] = HTTP_WIDE
    dreq[~in_use] = np.zeros((), dtype=REQ_DENSE_DTYPE)
    dreq["flags"][~in_use] = DENSE_BAD
    hc[~in_use] = np.zeros((), dtype=HTTP_COMPACT_DTYPE)
    raw_reqs[: 8 * n] = dreq.view(np.uint8)
    raw_http[: 8 * n] = hc.view(np.uint8)
    raw_hdrs[: 2 * m * n] = lens16.view(np.uint8)
    reqs = expand_reqs(raw_reqs, n, LAYOUT_DENSE)
    # (a dense request that is not ready -- hc says so -- has no header rows)
    reqs["num_headers"][(~wide) & (hc["result"] != 1)] = 0
    out_hdrs = expand_records(reqs, raw_hdrs, n, m, LAYOUT_DENSE)
    http = expand_http(reqs, raw_http, n, LAYOUT_DENSE)
    for a in (reqs, out_hdrs, http):
        a[~in_use] = np.zeros((), dtype=a.dtype)
    return {"in_use": in_use, "wide": wide, "reqs": reqs, "hdrs": out_hdrs, "http": http, "req_start": req_start,
            "bodies": bodies}


# ---------------------------------------------------------------------------
# The split in front of the parse (rhp.h rhp_split_sessions): the sessions'
# packed input cut at every empty line into offsets[] and rhp_session_t[] --
# split_pieces and pack_sessions above, for input that is already in HBM.

SPLIT_POISON = 0xFF   # what n_pieces, offsets, sessions and work hold before a call (tests)


def pack_raw(session_bytes_list, first: int = 0):
    """(buf u8, sess_off u64 [n_sessions + 1]) for session inputs packed back to back from byte `first` of the
    buffer (the bytes before it are LF, which no session may look back at), RHP_PAD zero bytes behind them."""
    sess_off = np.zeros(len(session_bytes_list) + 1, dtype=np.uint64)
    sess_off[0] = first
    if len(session_bytes_list):
        sess_off[1:] = first + np.cumsum([len(d) for d in session_bytes_list], dtype=np.uint64)
    end = int(sess_off[-1])
    buf = np.zeros(end + RHP_PAD, dtype=np.uint8)
    buf[:first] = 10
    buf[first:end] = np.frombuffer(b"".join(session_bytes_list), dtype=np.uint8)
    return buf, sess_off


def _split_result(n_pieces, offsets, sessions, cap, n_sessions):
    """(n_pieces int, offsets u64 [cap + 1], sessions SESSION_DTYPE [n_sessions]) from the bytes of the outputs"""
    return (int(n_pieces.view(np.uint64)[0]), offsets[: 8 * (cap + 1)].view(np.uint64),
            sessions[: 8 * n_sessions].view(SESSION_DTYPE))


def split_sessions_cpu(buf, sess_off, cap: int | None = None, bytes_end: int | None = None):
    """rhp_cpu_split_sessions (include/rhp_host.h): `buf` the packed bytes (u8), sess_off u64 [n_sessions + 1],
    bytes_end (default: sess_off's last).  cap None: the exact one, from a count-only call first.  Returns
    (n_pieces, offsets u64 [cap + 1], sessions SESSION_DTYPE [n_sessions]); every output held SPLIT_POISON
    before the call."""
    sess_off = np.ascontiguousarray(sess_off, dtype=np.uint64)
    ns = len(sess_off) - 1
    bytes_end = int(sess_off[-1]) if bytes_end is None else bytes_end
    raw = np.zeros(max(bytes_end, 1) + 16, dtype=np.uint8)   # (rhp.h: bytes is 16-byte aligned)
    at = (-raw.ctypes.data) % 16
    b = raw[at: at + bytes_end]
    b[:] = np.asarray(buf, dtype=np.uint8)[:bytes_end]
    work = np.full(split_work_words(bytes_end, ns) * 8, SPLIT_POISON, dtype=np.uint8)

    def call(cap):
        n_pieces, offsets, sessions = (np.full(size, SPLIT_POISON, dtype=np.uint8) for size in
                                       (8, 8 * (cap + 1), max(8 * ns, 1)))
        o = SplitOut(_ptr(n_pieces), _ptr(offsets), cap, _ptr(sessions), _ptr(work))
        rc = host().rhp_cpu_split_sessions(_ptr(b), bytes_end, _ptr(sess_off), ns, ctypes.byref(o))
        if rc != 0:
            raise RuntimeError(f"rhp_cpu_split_sessions failed: {rc}")
        return _split_result(n_pieces, offsets, sessions, cap, ns)

    return call(call(0)[0] if cap is None else int(cap))


def split_sessions_device(bytes_t, bytes_end: int, sess_off_t, n_sessions: int, cap: int, guard: int = 0,
                          fill: int = SPLIT_POISON, stream=None):
    """One rhp_split_sessions call over device tensors (`bytes_t` u8, 16-byte aligned; sess_off_t i64 / u64
    [n_sessions + 1]) on the stream (default: the current one).  n_pieces, offsets [cap + 1], sessions and work
    are Guarded device buffers (guard bytes on both sides) that hold `fill` first.  Returns (outs, finish): outs
    the Guarded buffers by name -- outs["offsets"].view and outs["sessions"].view are what rhp_parse_batch
    (n = cap) and rhp_fixup_sessions take, on the same stream, with no host step; finish(): synchronize, check
    the guards, (n_pieces, offsets, sessions) as split_sessions_cpu."""
    import torch
    cap = int(cap)
    outs = {"n_pieces": Guarded("n_pieces", 8, guard, fill=fill),
            "offsets": Guarded("offsets", 8 * (cap + 1), guard, fill=fill),
            "sessions": Guarded("sessions", max(8 * n_sessions, 1), guard, fill=fill),
            "work": Guarded("work", split_work_words(bytes_end, n_sessions) * 8, guard, fill=fill)}
    o = SplitOut(*(outs[k].view.data_ptr() for k in ("n_pieces", "offsets")), cap,
                 *(outs[k].view.data_ptr() for k in ("sessions", "work")))
    vp = ctypes.c_void_p
    rc = lib().rhp_split_sessions(vp(_addr(bytes_t)), bytes_end, vp(_addr(sess_off_t)), n_sessions, ctypes.byref(o),
                                  _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_split_sessions failed: {rc}")

    def finish(_keep=(bytes_t, sess_off_t)):
        torch.cuda.synchronize()
        if guard:
            for x in outs.values():
                x.check()
        return _split_result(*(outs[k].view.cpu().numpy() for k in ("n_pieces", "offsets", "sessions")), cap, n_sessions)
    return outs, finish


def split_sessions_gpu(session_bytes_list, cap: int | None = None, first: int = 0, guard: int = 0):
    """The sessions' inputs packed back to back (pack_raw) and split on the GPU.  cap None: the exact one, from
    a count-only call first.  Returns (n_pieces, offsets, sessions) as split_sessions_cpu."""
    import torch
    buf, sess_off = pack_raw(session_bytes_list, first)
    db = Guarded("bytes", buf.size, guard, data=buf)
    dso = torch.from_numpy(sess_off.view(np.int64)).to("cuda")
    end, ns = int(sess_off[-1]), len(session_bytes_list)

    def call(cap):
        out = split_sessions_device(db.view, end, dso, ns, cap, guard)[1]()
        if guard:
            db.check()
        return out

    return call(call(0)[0] if cap is None else int(cap))


def fixup_raw_gpu(session_bytes_list, cap: int, max_headers: int = 16, impl: int = IMPL_DFA, guard: int = 0):
    """A round from plain session input, on the GPU with no host step between the launches: rhp_split_sessions
    -> rhp_parse_batch (n = cap, speculative, over the split's offsets) -> rhp_fixup_sessions (over the
    split's sessions), one stream.  offsets and sessions hold zeros first, so a cap below n_pieces parses empty
    pieces only (rhp.h); it raises once the round has run.  Returns (Result over the cap record slots, session
    results, req_start, n_pieces, offsets u64 [cap + 1], sessions SESSION_DTYPE)."""
    import torch
    buf, sess_off = pack_raw(session_bytes_list)
    end, ns, cap = int(sess_off[-1]), len(session_bytes_list), int(cap)
    with _impl(impl):
        db = DeviceBatch(buf, np.zeros(cap + 1, dtype=np.uint64), max_headers, MODE_HTTP, flags=BATCH_SPECULATIVE,
                         guard=guard)
        dso = torch.from_numpy(sess_off.view(np.int64)).to("cuda")
        outs, finish = split_sessions_device(db.bytes, end, dso, ns, cap, guard, fill=0)
        db.offsets = outs["offsets"].view.view(torch.int64)
        r = _SessionRound(db, outs["sessions"].view, (ns * SESSION_RESULT_DTYPE.itemsize, None), (max(cap, 1) * 8, None),
                          n_sessions=ns)
        r.fixup()
        n_pieces, offsets, sessions = finish()   # (synchronizes)
        if n_pieces > cap:
            raise RuntimeError(f"fixup_raw_gpu: {n_pieces} pieces do not fit cap {cap}")
        db.host_off = offsets.copy()   # (result() describes the parsed batch over the split's offsets)
        r.check()
        return r.result() + (n_pieces, offsets, sessions)


# The parser's other two entry points (rhp.h rhp_parse_messages): batches of
# responses (phr_parse_response) and of bare header blocks (phr_parse_headers).

MSG_POISON = 0xC3   # what msgs and hdrs hold before a call (tests): an unwritten ret reads back as -1010580541, no answer's value


def phr_parse_message_cpu(kind: int, buf: np.ndarray, start: int, length: int, max_headers: int, last_len: int = 0):
    """rhp_phr_parse_response / rhp_phr_parse_headers (the host drop-ins) on bytes buf[start:start+length].
    Returns (ret, minor, status, msg(off,len), [(name_off|-1, name_len, value_off, value_len)]) with offsets from
    `start`; a header block: minor -1, status 0, msg (0, 0)."""
    h = host()
    hdrs = (PhrHeader * max(max_headers, 1))()
    msg, ml, nh = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t(max_headers)
    minor, status = ctypes.c_int(-1), ctypes.c_int(0)
    base = buf.ctypes.data + start
    if kind == MSG_RESPONSE:
        ret = h.rhp_phr_parse_response(base, length, ctypes.byref(minor), ctypes.byref(status), ctypes.byref(msg),
                                       ctypes.byref(ml), hdrs, ctypes.byref(nh), last_len)
    else:
        ret = h.rhp_phr_parse_headers(base, length, hdrs, ctypes.byref(nh), last_len)
    if ret <= 0:
        return ret, -1, 0, (0, 0), []
    rel = lambda p: (p or 0) - base
    hs = [(rel(x.name) if x.name else -1, x.name_len, rel(x.value), x.value_len) for x in hdrs[: nh.value]]
    return ret, minor.value, status.value, ((rel(msg.value), ml.value) if kind == MSG_RESPONSE else (0, 0)), hs


def _msg_result(msgs, hdrs, n, max_headers, layout):
    """(msgs MSG_DTYPE [n], hdrs HDR_DTYPE [n, max_headers]) from the bytes of the two record arrays"""
    return (msgs[: 16 * n].view(MSG_DTYPE),
            hdr_view(hdrs[: 8 * n * max_headers].view(HDR_DTYPE), n, max_headers, layout))


def parse_messages_cpu(buf, off, kind: int, max_headers: int = 16, layout: int = LAYOUT_REQUEST_MAJOR, last_len=None):
    """rhp_cpu_parse_messages (include/rhp_host.h): `buf` the packed messages with RHP_PAD zero bytes behind
    them (u8), off u64 [n + 1], last_len u64 [n] or None.  Returns (msgs MSG_DTYPE [n], hdrs HDR_DTYPE
    [n, max_headers]); both held MSG_POISON before the call."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    ll = None if last_len is None else np.ascontiguousarray(last_len, dtype=np.uint64)
    msgs = np.full(max(16 * n, 1), MSG_POISON, dtype=np.uint8)
    hdrs = np.full(max(8 * n * max_headers, 1), MSG_POISON, dtype=np.uint8)
    b = MsgBatch(_ptr(buf), _ptr(off), buf.size, n, max_headers, kind, layout, _ptr(msgs), _ptr(hdrs),
                 _ptr(ll) if ll is not None else None)
    rc = host().rhp_cpu_parse_messages(ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_parse_messages failed: {rc}")
    return _msg_result(msgs, hdrs, n, max_headers, layout)


def parse_messages_device(bytes_t, bytes_size: int, off_t, n: int, kind: int, max_headers: int, layout: int,
                          msgs_t, hdrs_t, last_len_t=None, stream=None):
    """One rhp_parse_messages call over device tensors on the stream (default: the current one): bytes_t u8
    (16-byte aligned), off_t i64 / u64 [n + 1], last_len_t the same [n] or None; the records are left in msgs_t
    (u8, 16 * n bytes) and hdrs_t (u8, 8 * n * max_headers bytes; None when max_headers == 0).  Nothing is
    synchronised or copied: the tensors are the call's only inputs and outputs."""
    b = MsgBatch(_addr(bytes_t), _addr(off_t), bytes_size, n, max_headers, kind, layout, _addr(msgs_t), _addr(hdrs_t),
                 _addr(last_len_t))
    rc = lib().rhp_parse_messages(ctypes.byref(b), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_parse_messages failed: {rc}")


def parse_messages_gpu(buf, off, kind: int, max_headers: int = 16, layout: int = LAYOUT_REQUEST_MAJOR, last_len=None,
                       guard: int = 0, fill: int = MSG_POISON):
    """The messages parsed on the GPU.  bytes, msgs and hdrs are Guarded device buffers (guard bytes on both
    sides, checked after the call); msgs and hdrs hold `fill` first.  Returns (msgs, hdrs) as parse_messages_cpu."""
    import torch
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    db = Guarded("bytes", buf.size, guard, data=buf if buf.flags.writeable else buf.copy())   # (torch takes writable arrays)
    gm = Guarded("msgs", max(16 * n, 1), guard, fill=fill)
    gh = Guarded("hdrs", max(8 * n * max_headers, 1), guard, fill=fill)
    doff = torch.from_numpy(off.view(np.int64).copy()).to("cuda")
    dll = None if last_len is None else torch.from_numpy(np.array(last_len, dtype=np.uint64).view(np.int64)).to("cuda")
    parse_messages_device(db.view, buf.size, doff, n, kind, max_headers, layout, gm.view, gh.view, dll)
    torch.cuda.synchronize()
    if guard:
        for g in (db, gm, gh):
            g.check()
    return _msg_result(gm.view.cpu().numpy(), gh.view.cpu().numpy(), n, max_headers, layout)


# The parser's fourth entry point (rhp.h rhp_decode_chunked): the resumable de-framer of chunked bodies over
# the new bytes of a batch of streams.

CHUNKED_POISON = 0xC3   # what results hold before a call (tests): an unwritten ret is no answer's value


def phr_decode_chunked_cpu(decoder: np.ndarray, piece: np.ndarray):
    """rhp_phr_decode_chunked (the host drop-in for phr_decode_chunked) on one piece (u8, decoded in place) with
    one decoder (CHUNKED_DTYPE [1], carried on in place).  Returns (ret, size)."""
    sz = ctypes.c_size_t(piece.size)
    ret = host().rhp_phr_decode_chunked(_ptr(decoder), _ptr(piece), ctypes.byref(sz))
    return int(ret), int(sz.value)


def decode_chunked_cpu(buf, off, decoders):
    """rhp_cpu_decode_chunked (include/rhp_host.h): `buf` the packed pieces (u8), off u64 [n + 1], decoders
    CHUNKED_DTYPE [n].  Nothing passed in is changed.  Returns (results CHUNKED_RESULT_DTYPE [n], decoders
    CHUNKED_DTYPE [n], bytes u8 as the call left them); results held CHUNKED_POISON before the call."""
    buf = np.array(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    dec = np.array(decoders, dtype=CHUNKED_DTYPE)
    n = len(off) - 1
    res = np.full(max(16 * n, 1), CHUNKED_POISON, dtype=np.uint8)
    b = ChunkedBatch(_ptr(buf), _ptr(off), buf.size, n, 0, _ptr(dec), _ptr(res))
    rc = host().rhp_cpu_decode_chunked(ctypes.byref(b))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_decode_chunked failed: {rc}")
    return res[: 16 * n].view(CHUNKED_RESULT_DTYPE), dec, buf


def decode_chunked_device(bytes_t, bytes_size: int, off_t, n: int, decoders_t, results_t, stream=None):
    """One rhp_decode_chunked call over device tensors on the stream (default: the current one): bytes_t u8
    (16-byte aligned, decoded in place), off_t i64 / u64 [n + 1], decoders_t and results_t u8, 16 * n bytes each
    (16-byte aligned; the decoders are carried on in place).  Nothing is synchronised or copied: the tensors are
    the call's only inputs and outputs."""
    b = ChunkedBatch(_addr(bytes_t), _addr(off_t), bytes_size, n, 0, _addr(decoders_t), _addr(results_t))
    rc = lib().rhp_decode_chunked(ctypes.byref(b), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_decode_chunked failed: {rc}")


def decode_chunked_gpu(buf, off, decoders, guard: int = 0, fill: int = CHUNKED_POISON, bytes_size: int | None = None):
    """The pieces decoded on the GPU.  bytes, decoders and results are Guarded device buffers (guard bytes on
    both sides, checked after the call); results hold `fill` first.  bytes_size: what the batch states (default:
    all of buf).  Returns (results, decoders, bytes) as decode_chunked_cpu."""
    import torch
    buf = np.array(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    dec = np.array(decoders, dtype=CHUNKED_DTYPE)
    n = len(off) - 1
    db = Guarded("bytes", max(buf.size, 1), guard, data=buf)
    gd = Guarded("decoders", max(16 * n, 1), guard, data=dec.view(np.uint8).reshape(-1))
    gr = Guarded("results", max(16 * n, 1), guard, fill=fill)
    doff = torch.from_numpy(off.view(np.int64).copy()).to("cuda")
    decode_chunked_device(db.view, buf.size if bytes_size is None else bytes_size, doff, n, gd.view, gr.view)
    torch.cuda.synchronize()
    if guard:
        for g in (db, gd, gr):
            g.check()
    return (gr.view.cpu().numpy()[: 16 * n].view(CHUNKED_RESULT_DTYPE), gd.view.cpu().numpy()[: 16 * n].view(CHUNKED_DTYPE),
            db.view.cpu().numpy()[: buf.size])


# Between the two (rhp.h rhp_frame_messages): the body framing of every message rhp_parse_messages parsed
# (http.c:204-233 over its header records), the header lookup of rhp_classify_batch over the same records, and
# the decoders rhp_decode_chunked starts from.

FRAME_POISON = 0xC3   # what frames, fields and decoders hold before a call (tests): no answer's value


def _frame_result(frames, fields, decoders, n, n_names):
    """(frames FRAME_DTYPE [n], fields FIELDREF_DTYPE [n_names, n], decoders CHUNKED_DTYPE [n] | None) from the
    bytes of the three outputs"""
    return (frames[: 16 * n].view(FRAME_DTYPE), fields[: 4 * n_names * n].view(FIELDREF_DTYPE).reshape(n_names, n),
            None if decoders is None else decoders[: 16 * n].view(CHUNKED_DTYPE))


def frame_messages_cpu(buf, off, kind: int, msgs, hdrs, names=(), max_headers: int = 16,
                       layout: int = LAYOUT_REQUEST_MAJOR, consume_trailer: int = 0, decoders: bool = True,
                       bytes_size: int | None = None):
    """rhp_cpu_frame_messages (include/rhp_host.h) over the records parse_messages_cpu returned: msgs MSG_DTYPE
    [n], hdrs HDR_DTYPE [n, max_headers] (put back into `layout`).  bytes_size: what the batch states (default:
    all of buf).  Returns (frames FRAME_DTYPE [n], fields FIELDREF_DTYPE [n_names, n], decoders CHUNKED_DTYPE [n]
    or None); all three held FRAME_POISON before the call."""
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(off) - 1
    m = np.ascontiguousarray(msgs).view(np.uint8).reshape(-1)
    h = np.ascontiguousarray(hdrs.T if layout == LAYOUT_HEADER_MAJOR else hdrs).view(np.uint8).reshape(-1)
    text, nm, _ = classify_tables(names)
    frames = np.full(max(16 * n, 1), FRAME_POISON, dtype=np.uint8)
    fields = np.full(max(4 * len(nm) * n, 1), FRAME_POISON, dtype=np.uint8)
    dec = np.full(max(16 * n, 1), FRAME_POISON, dtype=np.uint8) if decoders else None
    b = MsgBatch(_ptr(buf), _ptr(off), buf.size if bytes_size is None else bytes_size, n, max_headers, kind, layout,
                 _ptr(m) if m.size else None, _ptr(h) if h.size else None, None)
    f = FrameArgs(_ptr(text), _ptr(nm) if len(nm) else None, len(nm), consume_trailer, _ptr(fields) if len(nm) else None,
                  _ptr(frames), _ptr(dec) if decoders else None, 0)
    rc = host().rhp_cpu_frame_messages(ctypes.byref(b), ctypes.byref(f))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_frame_messages failed: {rc}")
    return _frame_result(frames, fields, dec, n, len(nm))


def frame_messages_device(bytes_t, bytes_size: int, off_t, n: int, kind: int, max_headers: int, layout: int, msgs_t,
                          hdrs_t, frames_t, names=(), fields_t=None, decoders_t=None, consume_trailer: int = 0,
                          stream=None):
    """One rhp_frame_messages call over device tensors on the stream (default: the current one): the batch as
    parse_messages_device left it; frames_t u8 (16 * n bytes, 16-byte aligned), fields_t u8 (4 * len(names) * n
    bytes), decoders_t u8 (16 * n bytes, 16-byte aligned) or None.  Nothing is synchronised or copied: the tensors
    are the call's only inputs and outputs (the names travel in the launch)."""
    text, nm, _ = classify_tables(names)
    b = MsgBatch(_addr(bytes_t), _addr(off_t), bytes_size, n, max_headers, kind, layout, _addr(msgs_t), _addr(hdrs_t), None)
    f = FrameArgs(_ptr(text), _ptr(nm) if len(nm) else None, len(nm), consume_trailer, _addr(fields_t) if len(nm) else None,
                  _addr(frames_t), _addr(decoders_t), 0)
    rc = lib().rhp_frame_messages(ctypes.byref(b), ctypes.byref(f), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_frame_messages failed: {rc}")


def frame_messages_gpu(buf, off, kind: int, names=(), max_headers: int = 16, layout: int = LAYOUT_REQUEST_MAJOR,
                       consume_trailer: int = 0, decoders: bool = True, guard: int = 0, fill: int = FRAME_POISON,
                       records=None, bytes_size: int | None = None):
    """The messages parsed (rhp_parse_messages) and framed (rhp_frame_messages) on the GPU, on one stream.
    bytes, frames, fields and decoders are Guarded device buffers (guard bytes on both sides, checked after the
    call); the three outputs hold `fill` first.  records: (msgs, hdrs) as parse_messages_cpu returns them, copied
    in instead of parsing (tests: crafted records).  Returns (frames, fields, decoders) as frame_messages_cpu."""
    import torch
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n, nn = len(off) - 1, len(names)
    db = Guarded("bytes", buf.size, guard, data=buf if buf.flags.writeable else buf.copy())
    gm = Guarded("msgs", max(16 * n, 1), 0, fill=MSG_POISON)
    gh = Guarded("hdrs", max(8 * n * max_headers, 1), 0, fill=MSG_POISON)
    gf = Guarded("frames", max(16 * n, 1), guard, fill=fill)
    gl = Guarded("fields", max(4 * nn * n, 1), guard, fill=fill)
    gd = Guarded("decoders", max(16 * n, 1), guard, fill=fill) if decoders else None
    doff = torch.from_numpy(off.view(np.int64).copy()).to("cuda")
    size = buf.size if bytes_size is None else bytes_size
    if records is None:
        parse_messages_device(db.view, size, doff, n, kind, max_headers, layout, gm.view, gh.view)
    else:
        m, h = records
        h = np.ascontiguousarray(h.T if layout == LAYOUT_HEADER_MAJOR else h)
        for g, a in ((gm, np.ascontiguousarray(m)), (gh, h)):
            if a.size:
                g.view[: a.nbytes].copy_(torch.from_numpy(a.view(np.uint8).reshape(-1).copy()))
    frame_messages_device(db.view, size, doff, n, kind, max_headers, layout, gm.view, gh.view, gf.view, names, gl.view,
                          gd.view if decoders else None, consume_trailer)
    torch.cuda.synchronize()
    if guard:
        for g in (db, gf, gl) + ((gd,) if decoders else ()):
            g.check()
    return _frame_result(gf.view.cpu().numpy(), gl.view.cpu().numpy(), gd.view.cpu().numpy() if decoders else None, n, nn)


# The three calls above as one loop per connection (rhp.h rhp_walk_responses): the pipelined responses of a
# batch of keep-alive upstream connections, parsed, framed and stepped over on the device.

WALK_POISON = 0xC3   # what msgs, hdrs, slots and results hold before a call (tests): no answer's value


def _walk_result(results, slots, msgs, hdrs, bytes_out, n_sessions, n_slots, max_headers):
    """(results WALK_RESULT_DTYPE [n_sessions], slots WALK_SLOT_DTYPE [n_slots], msgs MSG_DTYPE [n_slots], hdrs
    HDR_DTYPE [n_slots, max_headers], the bytes as the call left them) from the bytes of the outputs"""
    return (results[: 16 * n_sessions].view(WALK_RESULT_DTYPE), slots[: 32 * n_slots].view(WALK_SLOT_DTYPE),
            msgs[: 16 * n_slots].view(MSG_DTYPE), hdrs[: 8 * n_slots * max_headers].view(HDR_DTYPE).reshape(n_slots, max_headers),
            bytes_out)


# What the five calls of the family share (rhp_walk_batch_t), each stated once.  The *_device functions take the
# batch as twelve arguments in the order of _walk_batch; the *_cpu and *_gpu forms get them from these helpers.


def _walk_inputs(buf, sess_off, slot_off, n_slots_total, bytes_size, copy: bool = True):
    """(buf u8, sess_off u64, slot_off u64, n_sessions, n_slots_total, bytes_size) as the calls take them.
    n_slots_total None: slot_off[-1]; bytes_size None: all of buf.  copy: buf is a private copy, for the forms
    that walk (RHP_WALK_DEFRAME writes it) or upload; without, the caller's array where it is contiguous u8."""
    buf = np.array(buf, dtype=np.uint8) if copy else np.ascontiguousarray(buf, dtype=np.uint8)
    sess_off = np.ascontiguousarray(sess_off, dtype=np.uint64)
    slot_off = np.ascontiguousarray(slot_off, dtype=np.uint64)
    return (buf, sess_off, slot_off, len(sess_off) - 1, int(slot_off[-1]) if n_slots_total is None else n_slots_total,
            buf.size if bytes_size is None else bytes_size)


def _walk_batch(bytes_t, bytes_size, sess_off_t, slot_off_t, n_sessions, n_slots_total, max_headers, flags, msgs_t, hdrs_t,
                slots_t, results_t) -> WalkBatch:
    """rhp_walk_batch_t over numpy arrays or device tensors (None: a NULL pointer); bytes_rw is bytes.  It holds
    addresses only: the caller keeps the arrays alive over the call."""
    b = _addr(bytes_t)
    return WalkBatch(b, b, bytes_size, _addr(sess_off_t), _addr(slot_off_t), n_sessions, n_slots_total, max_headers, flags,
                     _addr(msgs_t), _addr(hdrs_t), _addr(slots_t), _addr(results_t))


_WALK_RECORDS = ("results", "slots", "msgs", "hdrs")   # the order of _walk_result's arguments and of a `records` tuple


def _walk_record_sizes(n_sessions, n_slots, max_headers):
    """the bytes of (results, slots, msgs, hdrs) as the host and the Guarded buffers are allocated: at least 1 each"""
    return max(16 * n_sessions, 1), max(32 * n_slots, 1), max(16 * n_slots, 1), max(8 * n_slots * max_headers, 1)


def _walk_records_host(n_sessions, n_slots, max_headers):
    """(results, slots, msgs, hdrs) for a host walk: u8 arrays of _walk_record_sizes that hold WALK_POISON"""
    return tuple(np.full(n, WALK_POISON, dtype=np.uint8) for n in _walk_record_sizes(n_sessions, n_slots, max_headers))


def _walk_records_u8(records):
    """the (results, slots, msgs, hdrs) of a `records` tuple, as a walk returned them or crafted, as flat u8 arrays"""
    return [np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in records[:4]]


def _walk_states(states, n_sessions):
    """a private, contiguous copy of the states as u8 (32 bytes each); None: all zero"""
    if states is None:
        return np.zeros(max(32 * n_sessions, 1), dtype=np.uint8)
    st = np.ascontiguousarray(states).view(np.uint8).reshape(-1).copy()
    assert st.size == 32 * n_sessions, "one rhp_walk_state_t per session"
    return st if st.size else np.zeros(1, dtype=np.uint8)


def _walk_asked(req_off, head_bits, n_req_total):
    """(req_off u32, head_bits u32 with at least one word, n_req_total) as the call takes them"""
    req_off = np.ascontiguousarray(req_off, dtype=np.uint32)
    head_bits = np.ascontiguousarray(head_bits, dtype=np.uint32).reshape(-1)
    if head_bits.size == 0:
        head_bits = np.zeros(1, dtype=np.uint32)
    return req_off, head_bits, int(req_off[-1]) if n_req_total is None else n_req_total


class _WalkDevice:
    """The device side of a *_gpu form: the bytes and the four records as Guarded buffers (`guard` bytes on both
    sides; the records at _walk_record_sizes, holding `fill`), sess_off and slot_off uploaded as i64.  `batch` is
    the twelve arguments every *_device function starts with.  A form adds the buffers of its own call (add), fills
    the records (walk), makes its own calls, synchronises once, checks every guard (check) and copies back (result)."""

    def __init__(self, buf, sess_off, slot_off, max_headers, flags, guard, fill, bytes_size, n_slots_total):
        import torch
        buf, sess_off, slot_off, self.ns, self.nt, size = _walk_inputs(buf, sess_off, slot_off, n_slots_total, bytes_size)
        self.max_headers, self.guard, self.fill = max_headers, guard, fill
        self.bytes = Guarded("bytes", buf.size, guard, data=buf)
        self.records = [Guarded(name, n, guard, fill=fill)
                        for name, n in zip(_WALK_RECORDS, _walk_record_sizes(self.ns, self.nt, max_headers))]
        self.states = self.answered = self.slot_req = None
        self.guarded = [self.bytes] + self.records
        res, slots, msgs, hdrs = (g.view for g in self.records)
        self.batch = (self.bytes.view, size, torch.from_numpy(sess_off.view(np.int64).copy()).to("cuda"),
                      torch.from_numpy(slot_off.view(np.int64).copy()).to("cuda"), self.ns, self.nt, max_headers, flags,
                      msgs, hdrs, slots, res)

    def add(self, g: Guarded) -> Guarded:
        """one more buffer for check()"""
        self.guarded.append(g)
        return g

    def walk(self, states=None, resume: bool = False, asked=None, slot_req: bool = False, records=None):
        """The records filled, nothing synchronised.  records: their bytes copied in, `fill` left behind them, and no
        walk.  Otherwise one walk: rhp_walk_answers with asked = (req_off, head_bits, n_req_total), whose queue,
        `answered` and (slot_req) `slot_req` become Guarded buffers, the last two at least 4 bytes; else
        rhp_walk_resume with resume or states; else rhp_walk_responses.  The states of a resumed walk: None is all
        zero, an array is copied (_walk_states), a Guarded buffer an earlier round returned is used as it lies."""
        import torch
        if records is not None:
            for g, a in zip(self.records, _walk_records_u8(records)):
                if a.size:
                    g.view[: a.size].copy_(torch.from_numpy(a.copy()))
            return
        if resume or states is not None:
            self.states = self.add(states if isinstance(states, Guarded) else
                                   Guarded("states", max(32 * self.ns, 1), self.guard, data=_walk_states(states, self.ns)))
        st = self.states.view if self.states is not None else None
        if asked is not None:
            req_off, head_bits, nq = _walk_asked(*asked)
            gq = self.add(Guarded("req_off", 4 * req_off.size, self.guard, data=req_off.view(np.uint8).copy()))
            gb = self.add(Guarded("head_bits", 4 * head_bits.size, self.guard, data=head_bits.view(np.uint8).copy()))
            self.answered = self.add(Guarded("answered", max(4 * self.ns, 4), self.guard, fill=self.fill))
            if slot_req:
                self.slot_req = self.add(Guarded("slot_req", max(4 * self.nt, 4), self.guard, fill=self.fill))
            walk_answers_device(*self.batch, st, gq.view, gb.view, nq, self.answered.view,
                                self.slot_req.view if slot_req else None)
        elif st is not None:
            walk_resume_device(*self.batch, st)
        else:
            walk_responses_device(*self.batch)

    def check(self) -> None:
        """every buffer's guard bytes (after the synchronise); nothing without guard"""
        if self.guard:
            for g in self.guarded:
                g.check()

    def result(self, *behind):
        """What the walk's *_gpu form returns: _walk_result's five from the device; after a resumed walk the states
        (WALK_STATE_DTYPE [n_sessions]) behind them and their Guarded buffer, for the next round, last; `behind`
        between the two."""
        res, slots, msgs, hdrs = (g.view.cpu().numpy() for g in self.records)
        out = _walk_result(res, slots, msgs, hdrs, self.bytes.view.cpu().numpy(), self.ns, self.nt, self.max_headers)
        if self.states is None:
            return out + behind
        return out + (self.states.view.cpu().numpy()[: 32 * self.ns].view(WALK_STATE_DTYPE),) + behind + (self.states,)


def walk_responses_cpu(buf, sess_off, slot_off, max_headers: int = 16, flags: int = 0, bytes_size: int | None = None,
                       n_slots_total: int | None = None):
    """rhp_cpu_walk_responses (include/rhp_host.h): `buf` the sessions back to back with RHP_PAD zero bytes
    behind them (u8), sess_off and slot_off u64 [n_sessions + 1].  Nothing passed in is changed.  bytes_size: what
    the batch states (default: all of buf); n_slots_total: the host's copy (default: slot_off[-1]).  Returns
    (results, slots, msgs, hdrs, bytes) as _walk_result; the four records held WALK_POISON before the call."""
    buf, sess_off, slot_off, ns, nt, size = _walk_inputs(buf, sess_off, slot_off, n_slots_total, bytes_size)
    res, slots, msgs, hdrs = _walk_records_host(ns, nt, max_headers)
    w = _walk_batch(buf, size, sess_off, slot_off, ns, nt, max_headers, flags, msgs, hdrs, slots, res)
    rc = host().rhp_cpu_walk_responses(ctypes.byref(w))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_walk_responses failed: {rc}")
    return _walk_result(res, slots, msgs, hdrs, buf, ns, nt, max_headers)


def walk_responses_device(bytes_t, bytes_size: int, sess_off_t, slot_off_t, n_sessions: int, n_slots_total: int,
                          max_headers: int, flags: int, msgs_t, hdrs_t, slots_t, results_t, stream=None):
    """One rhp_walk_responses call over device tensors on the stream (default: the current one): bytes_t u8
    (16-byte aligned; written with WALK_DEFRAME), sess_off_t and slot_off_t i64 / u64 [n_sessions + 1]; the
    records are left in msgs_t (u8, 16 * n_slots_total bytes), hdrs_t (u8, 8 * n_slots_total * max_headers bytes;
    None when max_headers == 0), slots_t (u8, 32 * n_slots_total bytes) and results_t (u8, 16 * n_sessions bytes).
    Nothing is synchronised or copied: the tensors are the call's only inputs and outputs."""
    w = _walk_batch(bytes_t, bytes_size, sess_off_t, slot_off_t, n_sessions, n_slots_total, max_headers, flags, msgs_t, hdrs_t,
                    slots_t, results_t)
    rc = lib().rhp_walk_responses(ctypes.byref(w), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_walk_responses failed: {rc}")


def walk_responses_gpu(buf, sess_off, slot_off, max_headers: int = 16, flags: int = 0, guard: int = 0,
                       fill: int = WALK_POISON, bytes_size: int | None = None, n_slots_total: int | None = None):
    """The sessions walked on the GPU.  bytes, msgs, hdrs, slots and results are Guarded device buffers (guard
    bytes on both sides, checked after the call; _WalkDevice); the four records hold `fill` first.  Returns what
    walk_responses_cpu returns."""
    import torch
    d = _WalkDevice(buf, sess_off, slot_off, max_headers, flags, guard, fill, bytes_size, n_slots_total)
    d.walk()
    torch.cuda.synchronize()
    d.check()
    return d.result()


# The walk carried across rounds (rhp.h rhp_walk_resume): `states` (WALK_STATE_DTYPE [n_sessions], all zero before a
# connection's first round) goes in and comes out; a round's input is what the round before left unconsumed and the
# new bytes behind it.


def walk_resume_cpu(buf, sess_off, slot_off, states=None, max_headers: int = 16, flags: int = 0, bytes_size: int | None = None,
                    n_slots_total: int | None = None):
    """rhp_cpu_walk_resume (include/rhp_host.h): one round.  Arguments as walk_responses_cpu, and `states`
    (WALK_STATE_DTYPE [n_sessions]; None: all zero).  Nothing passed in is changed.  Returns (results, slots, msgs,
    hdrs, bytes, states): walk_responses_cpu's five and the states the round left."""
    buf, sess_off, slot_off, ns, nt, size = _walk_inputs(buf, sess_off, slot_off, n_slots_total, bytes_size)
    st = _walk_states(states, ns)
    res, slots, msgs, hdrs = _walk_records_host(ns, nt, max_headers)
    w = _walk_batch(buf, size, sess_off, slot_off, ns, nt, max_headers, flags, msgs, hdrs, slots, res)
    rc = host().rhp_cpu_walk_resume(ctypes.byref(w), _ptr(st))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_walk_resume failed: {rc}")
    return _walk_result(res, slots, msgs, hdrs, buf, ns, nt, max_headers) + (st[: 32 * ns].view(WALK_STATE_DTYPE),)


def walk_resume_device(bytes_t, bytes_size: int, sess_off_t, slot_off_t, n_sessions: int, n_slots_total: int,
                       max_headers: int, flags: int, msgs_t, hdrs_t, slots_t, results_t, states_t, stream=None):
    """One rhp_walk_resume call over device tensors on the stream (default: the current one): the tensors of
    walk_responses_device, and states_t (u8, 32 * n_sessions bytes, 16-byte aligned), read at entry and written at
    exit.  It stays on the device: a chain of rounds hands the same tensor to every call.  Nothing is synchronised
    or copied."""
    w = _walk_batch(bytes_t, bytes_size, sess_off_t, slot_off_t, n_sessions, n_slots_total, max_headers, flags, msgs_t, hdrs_t,
                    slots_t, results_t)
    rc = lib().rhp_walk_resume(ctypes.byref(w), _addr(states_t), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_walk_resume failed: {rc}")


def walk_resume_gpu(buf, sess_off, slot_off, states=None, max_headers: int = 16, flags: int = 0, guard: int = 0,
                    fill: int = WALK_POISON, bytes_size: int | None = None, n_slots_total: int | None = None):
    """One round on the GPU.  bytes, msgs, hdrs, slots, results and states are Guarded device buffers (guard bytes
    on both sides, checked after the call; _WalkDevice); the four records hold `fill` first.  `states`:
    WALK_STATE_DTYPE [n_sessions] (None: all zero), or a Guarded buffer an earlier round returned, which is used as it
    lies on the device.  Returns what walk_resume_cpu returns, and behind it the Guarded states buffer for the next
    round."""
    import torch
    d = _WalkDevice(buf, sess_off, slot_off, max_headers, flags, guard, fill, bytes_size, n_slots_total)
    d.walk(states, resume=True)
    torch.cuda.synchronize()
    d.check()
    return d.result()


# The walk told which requests were HEAD (rhp.h rhp_walk_answers): req_off (u32 [n_sessions + 1]) cuts the
# sessions' queues of outstanding requests out of head_bits (u32 words, bit q: request q was a HEAD); `answered`
# (u32 [n_sessions]) and `slot_req` (u32 [n_slots_total]) come back behind the walk's own outputs.


def head_bits_of(heads) -> np.ndarray:
    """head_bits (u32 [(n + 31) // 32], at least one word) from one truth value per request"""
    heads = np.asarray(heads, dtype=bool)
    words = np.zeros(max((heads.size + 31) // 32, 1), dtype=np.uint32)
    for q in np.flatnonzero(heads):
        words[q >> 5] |= np.uint32(1 << (int(q) & 31))
    return words


def walk_answers_cpu(buf, sess_off, slot_off, req_off, head_bits, states=None, resume: bool = False, max_headers: int = 16,
                     flags: int = 0, bytes_size: int | None = None, n_slots_total: int | None = None,
                     n_req_total: int | None = None, slot_req: bool = True):
    """rhp_cpu_walk_answers (include/rhp_host.h).  Arguments as walk_responses_cpu, the queue (req_off, head_bits;
    n_req_total: the host's copy, default req_off[-1]) and, for a round of the resumed walk, `states`
    (WALK_STATE_DTYPE [n_sessions]) or resume=True (all-zero states).  Nothing passed in is changed.  Returns the
    walk's tuple -- walk_responses_cpu's five, or walk_resume_cpu's six -- and behind it answered (u32 [n_sessions])
    and slot_req (u32 [n_slots_total]; None with slot_req=False); both held WALK_POISON before the call."""
    buf, sess_off, slot_off, ns, nt, size = _walk_inputs(buf, sess_off, slot_off, n_slots_total, bytes_size)
    req_off, head_bits, nq = _walk_asked(req_off, head_bits, n_req_total)
    resume = resume or states is not None
    st = _walk_states(states, ns) if resume else None
    res, slots, msgs, hdrs = _walk_records_host(ns, nt, max_headers)
    ans = np.full(max(4 * ns, 1), WALK_POISON, dtype=np.uint8)
    sreq = np.full(max(4 * nt, 1), WALK_POISON, dtype=np.uint8) if slot_req else None
    w = _walk_batch(buf, size, sess_off, slot_off, ns, nt, max_headers, flags, msgs, hdrs, slots, res)
    x = WalkAsked(_ptr(req_off), _ptr(head_bits), nq, 0, _ptr(ans), _addr(sreq))
    rc = host().rhp_cpu_walk_answers(ctypes.byref(w), _addr(st), ctypes.byref(x))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_walk_answers failed: {rc}")
    out = _walk_result(res, slots, msgs, hdrs, buf, ns, nt, max_headers)
    if resume:
        out += (st[: 32 * ns].view(WALK_STATE_DTYPE),)
    return out + (ans[: 4 * ns].view(np.uint32), sreq[: 4 * nt].view(np.uint32) if slot_req else None)


def walk_answers_device(bytes_t, bytes_size: int, sess_off_t, slot_off_t, n_sessions: int, n_slots_total: int,
                        max_headers: int, flags: int, msgs_t, hdrs_t, slots_t, results_t, states_t, req_off_t, head_bits_t,
                        n_req_total: int, answered_t, slot_req_t, stream=None):
    """One rhp_walk_answers call over device tensors on the stream (default: the current one): the tensors of
    walk_resume_device (states_t None: the one-shot walk), req_off_t (i32 / u32 [n_sessions + 1]), head_bits_t (i32 /
    u32 words), answered_t (u8, 4 * n_sessions bytes) and slot_req_t (u8, 4 * n_slots_total bytes, or None), all
    4-byte aligned.  Nothing is synchronised or copied."""
    w = _walk_batch(bytes_t, bytes_size, sess_off_t, slot_off_t, n_sessions, n_slots_total, max_headers, flags, msgs_t, hdrs_t,
                    slots_t, results_t)
    x = WalkAsked(_addr(req_off_t), _addr(head_bits_t), n_req_total, 0, _addr(answered_t), _addr(slot_req_t))
    rc = lib().rhp_walk_answers(ctypes.byref(w), _addr(states_t), ctypes.byref(x), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_walk_answers failed: {rc}")


def walk_answers_gpu(buf, sess_off, slot_off, req_off, head_bits, states=None, resume: bool = False, max_headers: int = 16,
                     flags: int = 0, guard: int = 0, fill: int = WALK_POISON, bytes_size: int | None = None,
                     n_slots_total: int | None = None, n_req_total: int | None = None, slot_req: bool = True):
    """The call on the GPU.  bytes, msgs, hdrs, slots, results, states, req_off, head_bits, answered and slot_req
    are Guarded device buffers (guard bytes on both sides, checked after the call; _WalkDevice); the records,
    answered and slot_req hold `fill` first.  `states`: as walk_resume_gpu takes them (a Guarded buffer an earlier round returned
    is used as it lies on the device); resume=True with states None: all-zero states.  Returns what
    walk_answers_cpu returns; with states, the Guarded states buffer for the next round comes last."""
    import torch
    d = _WalkDevice(buf, sess_off, slot_off, max_headers, flags, guard, fill, bytes_size, n_slots_total)
    d.walk(states, resume, (req_off, head_bits, n_req_total), slot_req)
    torch.cuda.synchronize()
    d.check()
    return d.result(d.answered.view.cpu().numpy()[: 4 * d.ns].view(np.uint32),
                    d.slot_req.view.cpu().numpy()[: 4 * d.nt].view(np.uint32) if slot_req else None)


# The header lookup over the slots of a walk (rhp.h rhp_lookup_walked): the records stay where the walk left
# them, and only `fields` goes back to the host.

LOOKUP_POISON = 0xC3   # what fields holds before a call (tests): no answer's value


def _lookup_fields(fields, n_names, n_slots):
    """fields FIELDREF_DTYPE [n_names, n_slots] from the output's bytes"""
    return fields[: 4 * n_names * n_slots].view(FIELDREF_DTYPE).reshape(n_names, n_slots)


def lookup_walked_cpu(records, buf, sess_off, slot_off, names, max_headers: int = 16, flags: int = 0,
                      bytes_size: int | None = None, n_slots_total: int | None = None):
    """rhp_cpu_lookup_walked (include/rhp_host.h) over `records`: (results, slots, msgs, hdrs) as
    walk_responses_cpu or walk_resume_cpu returned them (their first four), or crafted ones; buf, sess_off and
    slot_off as that walk got them (buf may be the bytes it left).  Returns fields FIELDREF_DTYPE [n_names,
    n_slots_total]; it held LOOKUP_POISON before the call."""
    buf, sess_off, slot_off, ns, nt, size = _walk_inputs(buf, sess_off, slot_off, n_slots_total, bytes_size, copy=False)
    res, slots, msgs, hdrs = (a if a.size else None for a in _walk_records_u8(records))   # an empty record array: NULL
    text, nm, _ = classify_tables(names)
    fields = np.full(max(4 * len(nm) * nt, 1), LOOKUP_POISON, dtype=np.uint8)
    w = _walk_batch(buf, size, sess_off, slot_off, ns, nt, max_headers, flags, msgs, hdrs, slots, res)
    l = WalkLookup(_ptr(text), _ptr(nm), len(nm), 0, _ptr(fields))
    rc = host().rhp_cpu_lookup_walked(ctypes.byref(w), ctypes.byref(l))
    if rc != 0:
        raise RuntimeError(f"rhp_cpu_lookup_walked failed: {rc}")
    return _lookup_fields(fields, len(nm), nt)


def lookup_walked_device(bytes_t, bytes_size: int, sess_off_t, slot_off_t, n_sessions: int, n_slots_total: int,
                         max_headers: int, flags: int, msgs_t, hdrs_t, slots_t, results_t, names, fields_t, stream=None):
    """One rhp_lookup_walked call over device tensors on the stream (default: the current one): the batch as
    walk_responses_device or walk_resume_device left it; fields_t u8 (4 * len(names) * n_slots_total bytes).
    Nothing is synchronised or copied: the tensors are the call's only inputs and outputs (the names travel in
    the launch)."""
    text, nm, _ = classify_tables(names)
    w = _walk_batch(bytes_t, bytes_size, sess_off_t, slot_off_t, n_sessions, n_slots_total, max_headers, flags, msgs_t, hdrs_t,
                    slots_t, results_t)
    l = WalkLookup(_ptr(text), _ptr(nm), len(nm), 0, _addr(fields_t))
    rc = lib().rhp_lookup_walked(ctypes.byref(w), ctypes.byref(l), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_lookup_walked failed: {rc}")


def lookup_walked_gpu(buf, sess_off, slot_off, names, max_headers: int = 16, flags: int = 0, guard: int = 0,
                      fill: int = LOOKUP_POISON, records=None, states=None, resume: bool = False,
                      bytes_size: int | None = None, n_slots_total: int | None = None):
    """The sessions walked (rhp_walk_responses; with resume or states: one round of rhp_walk_resume, states as
    walk_resume_gpu takes them) and looked up (rhp_lookup_walked) on the GPU, on one stream, the walk's records
    left on the device between the two.  bytes, msgs, hdrs, slots, results, states and fields are Guarded device
    buffers (guard bytes on both sides, checked after the call); the records and fields hold `fill` first.
    records: (results, slots, msgs, hdrs) copied in instead of walking (tests: crafted records; their own bytes
    in front, `fill` behind them).  Returns (fields as lookup_walked_cpu, what walk_responses_gpu or
    walk_resume_gpu returns)."""
    import torch
    d = _WalkDevice(buf, sess_off, slot_off, max_headers, flags, guard, fill, bytes_size, n_slots_total)
    gf = d.add(Guarded("fields", max(4 * len(names) * d.nt, 1), guard, fill=fill))
    d.walk(states, resume, records=records)
    lookup_walked_device(*d.batch, names, gf.view)
    torch.cuda.synchronize()
    d.check()
    return _lookup_fields(gf.view.cpu().numpy(), len(names), d.nt), d.result()


# The walked responses re-written for the client side (rhp.h rhp_relay_walked): the records stay where the walk
# left them; out_off, why and the replies come back.

RELAY_POISON = 0xC3   # what out_off, why and out hold before a call (tests)


def _relay_result(out_off, why, out, n_slots):
    """(out_off u64 [n_slots + 1], why u32 [n_slots], the replies u8 [out_off[-1]], or None when they did not fit
    the `out` that was passed) from the outputs' bytes"""
    off = out_off[: 8 * (n_slots + 1)].view(np.uint64)
    total = int(off[-1])
    return off, why[: 4 * n_slots].view(np.uint32), out[:total] if total <= out.size else None


def relay_walked_cpu(records, buf, sess_off, slot_off, names=(), max_headers: int = 16, flags: int = 0,
                     bytes_size: int | None = None, n_slots_total: int | None = None, out_size: int | None = None,
                     date: bytes = DEFAULT_DATE):
    """rhp_cpu_relay_walked (include/rhp_host.h) over `records`: (results, slots, msgs, hdrs) as a host walk
    returned them (its first four), or crafted ones; buf the bytes that walk left (its fifth), sess_off, slot_off
    and flags as it got them.  out_size None: the call runs twice, for the sizes and then with an `out` of exactly
    their sum.  Returns (out_off, why, out) as _relay_result; all three held RELAY_POISON before the call."""
    buf, sess_off, slot_off, ns, nt, size = _walk_inputs(buf, sess_off, slot_off, n_slots_total, bytes_size, copy=False)
    res, slots, msgs, hdrs = (a if a.size else None for a in _walk_records_u8(records))   # an empty record array: NULL
    text, nm, _ = classify_tables(names)
    work = np.zeros(relay_work_words(nt), dtype=np.uint64)
    w = _walk_batch(buf, size, sess_off, slot_off, ns, nt, max_headers, flags, msgs, hdrs, slots, res)

    def run(size):
        off = np.full(8 * (nt + 1), RELAY_POISON, dtype=np.uint8)
        why = np.full(max(4 * nt, 1), RELAY_POISON, dtype=np.uint8)
        out = np.full(size, RELAY_POISON, dtype=np.uint8)
        r = WalkRelay(_ptr(text), _ptr(nm) if len(nm) else None, len(nm), len(date), date, _ptr(off), _ptr(why),
                      _ptr(out) if size else None, size, _ptr(work))
        rc = host().rhp_cpu_relay_walked(ctypes.byref(w), ctypes.byref(r))
        if rc != 0:
            raise RuntimeError(f"rhp_cpu_relay_walked failed: {rc}")
        return off, why, out

    if out_size is None:
        out_size = int(run(0)[0].view(np.uint64)[-1])
    return _relay_result(*run(out_size), nt)


def relay_walked_device(bytes_t, bytes_size: int, sess_off_t, slot_off_t, n_sessions: int, n_slots_total: int,
                        max_headers: int, flags: int, msgs_t, hdrs_t, slots_t, results_t, names, out_off_t, why_t, out_t,
                        out_size: int, work_t, date: bytes = DEFAULT_DATE, stream=None, steps: bool = False):
    """One rhp_relay_walked call over device tensors on the stream (default: the current one): the batch as a
    walk left it; out_off_t (8 * (n_slots_total + 1) bytes, 8-byte aligned), why_t (4 * n_slots_total bytes), out_t
    (out_size bytes, any alignment; None with out_size 0) and work_t (8 * relay_work_words(n_slots_total) bytes).
    Nothing is synchronised or copied (the names and the date travel in the launch).  steps: the measuring call
    rhp_relay_walked_steps instead, which waits for the stream; returns (sizes, scan, copy) in microseconds."""
    text, nm, _ = classify_tables(names)
    w = _walk_batch(bytes_t, bytes_size, sess_off_t, slot_off_t, n_sessions, n_slots_total, max_headers, flags, msgs_t, hdrs_t,
                    slots_t, results_t)
    r = WalkRelay(_ptr(text), _ptr(nm) if len(nm) else None, len(nm), len(date), date, _addr(out_off_t), _addr(why_t),
                  _addr(out_t), out_size, _addr(work_t))
    if steps:
        us = (ctypes.c_float * 3)()
        rc = lib().rhp_relay_walked_steps(ctypes.byref(w), ctypes.byref(r), _stream(stream), ctypes.byref(us))
    else:
        rc = lib().rhp_relay_walked(ctypes.byref(w), ctypes.byref(r), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_relay_walked failed: {rc}")
    return tuple(us) if steps else None


def relay_walked_gpu(buf, sess_off, slot_off, names=(), max_headers: int = 16, flags: int = 0, guard: int = 0,
                     fill: int = RELAY_POISON, records=None, states=None, resume: bool = False, asked=None,
                     bytes_size: int | None = None, n_slots_total: int | None = None, out_size: int | None = None,
                     out_shift: int = 0, date: bytes = DEFAULT_DATE, steps: bool = False):
    """The sessions walked and relayed on the GPU, on one stream, the walk's records left on the device between
    the two.  The walk: rhp_walk_responses; with resume or states one round of rhp_walk_resume (states as
    walk_resume_gpu takes them); with asked = (req_off, head_bits, n_req_total) rhp_walk_answers over that queue.
    records: (results, slots, msgs, hdrs) copied in instead of walking (tests: crafted records).  out_size None:
    the relay runs twice, for the sizes and then with an `out` of exactly their sum, `out_shift` bytes off a
    512-byte boundary.  Every buffer is a Guarded device buffer (guard bytes on both sides, checked after the
    calls; the walk's by _WalkDevice); out_off, why and out hold `fill` first; steps: the call that writes the replies is rhp_relay_walked_steps;
    replies that do not fit must leave out as it was.  Returns ((out_off, why, out) as relay_walked_cpu, what the
    walk's *_gpu function returns up to the states)."""
    import torch
    d = _WalkDevice(buf, sess_off, slot_off, max_headers, flags, guard, fill, bytes_size, n_slots_total)
    nt = d.nt
    go = d.add(Guarded("out_off", 8 * (nt + 1), guard, fill=fill))
    gy = d.add(Guarded("why", max(4 * nt, 4), guard, fill=fill))
    gw = d.add(Guarded("work", 8 * relay_work_words(nt), guard, fill=fill))
    d.walk(states, resume, asked, records=records)

    def run(n_out):
        g = Guarded("out", max(n_out, 1), max(guard, 16) if out_shift else guard, fill=fill, shift=out_shift)
        relay_walked_device(*d.batch, names, go.view, gy.view, g.view if n_out else None, n_out, gw.view, date, steps=steps and n_out > 0)
        torch.cuda.synchronize()
        return g

    if out_size is None:
        run(0)
        out_size = int(go.view.cpu().numpy().view(np.uint64)[nt])
        go.view.fill_(fill)
        gy.view.fill_(fill)
    gout = run(out_size)
    if int(go.view.cpu().numpy().view(np.uint64)[nt]) > out_size:
        assert bool((gout.view == (fill or 0)).all()), "the replies do not fit, and out was written"
    d.add(gout)
    d.check()
    return _relay_result(go.view.cpu().numpy(), gy.view.cpu().numpy(), gout.view.cpu().numpy()[: max(out_size, 0)], nt), d.result()


# The requests of a proxied route re-written for the upstream (rhp.h rhp_forward_sessions): the records stay where
# the parse and the fix-up left them; out_off, why, the requests and the queue for rhp_walk_answers come back.

FORWARD_POISON = 0xC3   # what out_off, why, out, fwd_off and head_bits hold before a call (tests)


def _forward_desc(n_routes, forward_mask, names, extra, out_off, why, out, out_size, fwd_off, head_bits, work):
    """(text, names, Forward): rhp_forward_t over classify_tables(names), the extra bytes and the outputs'
    addresses.  The Forward points into the two arrays: keep them alive."""
    text, nm, _ = classify_tables(names)
    extra = bytes(extra)
    return text, nm, Forward(n_routes, forward_mask, _ptr(text), _ptr(nm) if len(nm) else None, len(nm), len(extra),
                             extra if extra else None, out_off, why, out, out_size, fwd_off, head_bits, work)


def _forward_result(out_off, why, out, fwd_off, head_bits, n, n_sessions, fill=FORWARD_POISON):
    """(out_off u64 [n + 1], why u32 [n], the requests u8 [out_off[-1]] or None when they did not fit the `out` that
    was passed, fwd_off u32 [n_sessions + 1], head_bits u32 [(total + 31) / 32]) from the outputs' bytes; the words
    of head_bits beyond those must still hold `fill`"""
    off = out_off[: 8 * (n + 1)].view(np.uint64)
    total = int(off[-1])
    fo = fwd_off[: 4 * (n_sessions + 1)].view(np.uint32)
    words = (int(fo[-1]) + 31) // 32
    assert bool((head_bits[4 * words:] == fill).all()), "a word of head_bits beyond (total + 31) / 32 was written"
    return off, why[: 4 * n].view(np.uint32), out[:total] if total <= out.size else None, fo, head_bits[: 4 * words].view(np.uint32)


def _forward_sizes(n, n_sessions):
    """the bytes of (out_off, why, fwd_off, head_bits) as the host and the Guarded buffers are allocated"""
    return 8 * (n + 1), max(4 * n, 4), 4 * (n_sessions + 1), max(4 * ((n + 31) // 32), 4)


def forward_sessions_cpu(b_or_res, sessions, results, starts, route, n_routes: int, forward_mask: int, names=(),
                         extra: bytes = b"", out_size: int | None = None):
    """rhp_cpu_forward_sessions (include/rhp_host.h) over a speculative batch in host memory after a fix-up and a
    classify (the Batch of speculative_cpu or a Result that describes its batch; route u16 [n] by record slot).
    out_size None: the call runs twice, for the sizes and then with an `out` of exactly their sum.  Returns
    (out_off, why, out, fwd_off, head_bits) as _forward_result; all five held FORWARD_POISON before the call,
    head_bits at (n + 31) / 32 words."""
    b = _batch_of(b_or_res)
    sessions, results, starts, route = _session_arrays(sessions, results, starts, route)
    n, ns = b.n, len(sessions)
    work = np.zeros(forward_work_words(n, ns), dtype=np.uint64)

    def run(size):
        off, why, fo, hb, out = (np.full(k, FORWARD_POISON, dtype=np.uint8) for k in _forward_sizes(n, ns) + (size,))
        *_keep, f = _forward_desc(n_routes, forward_mask, names, extra, _ptr(off), _ptr(why), _ptr(out) if size else None, size,
                                  _ptr(fo), _ptr(hb), _ptr(work))
        rc = host().rhp_cpu_forward_sessions(ctypes.byref(b), _ptr(sessions) if ns else None, ns, _ptr(results) if ns else None,
                                             _ptr(starts) if ns else None, _ptr(route), ctypes.byref(f))
        if rc != 0:
            raise RuntimeError(f"rhp_cpu_forward_sessions failed: {rc}")
        if n == 0 or ns == 0:   # the empty call: out_off[0] and fwd_off only
            return np.zeros(8, dtype=np.uint8), why[:0], out, fo, hb
        return off, why, out, fo, hb

    if out_size is None:
        out_size = int(run(0)[0].view(np.uint64)[-1])
    return _forward_result(*run(out_size), n if ns else 0, ns)


def forward_sessions_device(d: Batch, sessions_t, n_sessions: int, results_t, starts_t, route_t, n_routes: int,
                            forward_mask: int, names, extra: bytes, out_off_t, why_t, out_t, out_size: int, fwd_off_t,
                            head_bits_t, work_t, stream=None):
    """One rhp_forward_sessions call over device tensors on the stream (default: the current one): `d` the parsed,
    fixed-up batch's descriptor, route_t rhp_classify_sessions' output; out_off_t (8 * (n + 1) bytes, 8-byte aligned),
    why_t (4 * n bytes), out_t (out_size bytes, any alignment; None with out_size 0), fwd_off_t (4 * (n_sessions + 1)
    bytes), head_bits_t (4 * ((n + 31) / 32) bytes) and work_t (8 * forward_work_words(n, n_sessions) bytes).
    Nothing is synchronised or copied (the names and the extra lines travel in the launches)."""
    *_keep, f = _forward_desc(n_routes, forward_mask, names, extra, _addr(out_off_t), _addr(why_t), _addr(out_t), out_size,
                              _addr(fwd_off_t), _addr(head_bits_t), _addr(work_t))
    vp = ctypes.c_void_p
    rc = lib().rhp_forward_sessions(ctypes.byref(d), vp(_addr(sessions_t)), n_sessions, vp(_addr(results_t)),
                                    vp(_addr(starts_t)), vp(_addr(route_t)), ctypes.byref(f), _stream(stream))
    if rc != 0:
        raise RuntimeError(f"rhp_forward_sessions failed: {rc}")


def forward_sessions_gpu(buf, off, sessions, routes, forward_mask: int, names=(), extra: bytes = b"", max_headers: int = 16,
                         impl: int = IMPL_DFA, layout: int = LAYOUT_REQUEST_MAJOR, guard: int = 0, fill: int = FORWARD_POISON,
                         records=None, out_size: int | None = None, out_shift: int = 0, details: bool = False):
    """A round of split-free pipelined input forwarded on the GPU: speculative parse -> rhp_fixup_sessions ->
    rhp_classify_sessions over `routes` -> rhp_forward_sessions, on one stream with no synchronisation in between.
    records: (raw reqs, raw hdrs, raw http, session results, req_start, route) copied in instead of the first three
    calls (tests: crafted records).  out_size None: the forward runs twice, for the sizes and then with an `out` of
    exactly their sum, `out_shift` bytes off a 512-byte boundary.  Every buffer is a Guarded device buffer (guard
    bytes on both sides, checked after the calls); the outputs hold `fill` first; requests that do not fit must leave
    out as it was.  Returns (out_off, why, out, fwd_off, head_bits) as forward_sessions_cpu; details: also (Result,
    session results, req_start, route u16 [n]) as the GPU left them."""
    import torch
    with _impl(impl):
        db = DeviceBatch(buf, off, max_headers, MODE_HTTP, layout=layout, flags=BATCH_SPECULATIVE, guard=guard, fill=fill)
        n, ns = db.n, len(sessions)
        r = _SessionRound(db, np.ascontiguousarray(sessions, dtype=SESSION_DTYPE) if ns else None,
                          (max(ns, 1) * SESSION_RESULT_DTYPE.itemsize, fill), (max(n, 1) * 8, fill), route=(max(n, 1) * 2, GUARD_BYTE))
        sizes = _forward_sizes(n, ns) + (8 * forward_work_words(n, ns),)
        go, gy, gf, gb, gw = (r.add(Guarded(name, size, guard, fill=fill))
                              for name, size in zip(("out_off", "why", "fwd_off", "head_bits", "work"), sizes))
        if records is not None:
            r.load(records)
        else:
            r.fixup()
            r.classify((), routes)

        def run(n_out):
            g = Guarded("out", max(n_out, 1), max(guard, 16) if out_shift else guard, fill=fill, shift=out_shift)
            forward_sessions_device(r.d, r.sessions, ns, r.results.view, r.req_start.view, r.route.view, len(routes), forward_mask,
                                    names, extra, go.view, gy.view, g.view if n_out else None, n_out, gf.view, gb.view, gw.view)
            torch.cuda.synchronize()
            return g

        empty = n == 0 or ns == 0
        if out_size is None:
            run(0)
            out_size = 0 if empty else int(go.view.cpu().numpy().view(np.uint64)[n])
            for g in (go, gy, gf, gb):
                g.view.fill_(fill)
        gout = run(out_size)
        if not empty and int(go.view.cpu().numpy().view(np.uint64)[n]) > out_size:
            assert bool((gout.view == (fill or 0)).all()), "the requests do not fit, and out was written"
        r.add(gout)
        r.check()
        off_b = go.view.cpu().numpy()
        out = _forward_result(off_b[:8] if empty else off_b, gy.view.cpu().numpy(), gout.view.cpu().numpy()[: max(out_size, 0)],
                              gf.view.cpu().numpy(), gb.view.cpu().numpy(), 0 if empty else n, ns, fill)
        if not details:
            return out
        res, results, starts, route = r.result(route=True)
        return out + (res, results, starts[:n], route)
