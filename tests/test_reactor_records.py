"""What the server hands to SERVER_REQUEST, request by request, against the
oracle's sequential http_read_request loop over the same byte stream (the
reference's server_session_read loop, server.c:37-65, over http.c:177-234).

tests/reactor/echo_test.c serves one connection that sends a stream in chunks
(so rounds see partial requests and pipelined runs); its handler echoes the
parsed method, target, fields and body.  The oracle parses the stream from the
front, one request at a time, exactly as the reference's loop consumes it:
result 1 -> the request, advance by `consumed`; 0 -> wait (the tail gets no
answer); -1 -> the connection closes.  The streams mix pipelined GETs,
Content-Length and chunked bodies (de-framed in place), LF-only line ends,
HTTP/1.0, a request at the 16-field limit and bodies larger than a chunk;
stream_wide has the requests whose record slots the dense copy-back
(RHP_REACTOR_PACK, reactor/batch.c) leaves wide, run with and without it.
Host parsers on CPU; the MI355X batch parser (asynchronous rounds) on the GPU.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import libreactorng_amd as rhp
from oracle_util import run_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ECHO = os.path.join(ROOT, "libreactorng_amd", "bin", "echo_test")
TFB = (b"GET /plaintext HTTP/1.1\r\nHost: tfb-server:8080\r\nAccept: text/plain\r\n"
       b"Connection: keep-alive\r\nUser-Agent: wrk/4.2.0 (tfb-load)\r\n\r\n")


def stream_mixed(seed=7):
    rng = np.random.default_rng(seed)
    parts = [b"GET / HTTP/1.1\r\nHost: a\r\n\r\n",
             b"GET /path?q=1 HTTP/1.0\r\nA: 1\r\nB:  two words  \r\n\r\n",
             b"POST /body HTTP/1.1\r\nContent-Length: 5\r\n\r\nhello",
             b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n",
             b"GET /lf HTTP/1.1\nX: y\nZ:  w\n\n",
             b"GET /sixteen HTTP/1.1\r\n" + b"".join(b"H%d: v%d\r\n" % (i, i) for i in range(16)) + b"\r\n"]
    parts += [TFB] * 8
    big = bytes(rng.integers(97, 123, 3000, dtype=np.uint8))
    parts += [b"POST /big HTTP/1.1\r\nContent-Length: 3000\r\n\r\n" + big]
    parts += [b"PUT /chunked-hex HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n1a\r\n" + b"z" * 26 +
              b"\r\n0\r\n\r\n"]
    parts += [b"GET /t%d HTTP/1.1\r\nX-I: %d\r\n\r\n" % (i, i) for i in range(20)]
    parts += [b"GET /last HTTP/1.1\r\nHost:"]   # incomplete: no answer
    return b"".join(parts)


def stream_wide():
    """Requests whose record slots rhp_pack_dense must leave wide for a length
    (name over 62, value over 1007, method over 255 bytes: include/rhp.h) or
    because the DFA hands them to the exact parser (leading CRLF, no space
    after the colon, trailing OWS, obs-fold), beside ones just inside each
    limit, canonical GETs around each, a chunked POST and an incomplete tail:
    the server reads a wide slot's request-major records end to end."""
    get = b"GET /g HTTP/1.1\r\nHost: a\r\n\r\n"
    rest = [b"GET /n%d HTTP/1.1\r\n" % k + b"N" * k + b": v\r\nHost: a\r\n\r\n" for k in (62, 63, 100)]
    rest += [b"GET /v%d HTTP/1.1\r\nHost: a\r\nX: " % k + b"v" * k + b"\r\n\r\n" for k in (1007, 1008, 1023, 1024, 1500)]
    rest += [b"M" * k + b" /m HTTP/1.1\r\nHost: a\r\n\r\n" for k in (255, 256)]
    rest += [b"\r\nGET /crlf HTTP/1.1\r\nHost: a\r\n\r\n",
             b"GET /nospace HTTP/1.1\r\nHost:x\r\n\r\n",
             b"GET /ows HTTP/1.1\r\nHost: a \t \r\nB: c\r\n\r\n",
             b"GET /fold HTTP/1.1\r\nA: b\r\n \tfolded\r\nHost: a\r\n\r\n",
             b"POST /c HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n5\r\nhello\r\n6\r\n world\r\n0\r\n\r\n"]
    parts = [get]
    for r in rest:
        parts += [r, get, TFB]
    parts += [b"GET /last HTTP/1.1\r\nX: " + b"v" * 1100]   # incomplete: no answer
    return b"".join(parts)


def stream_bad():
    return TFB * 3 + b"GET /x HTTP/1.1\r\nBad Header\r\n\r\n" + TFB


def oracle_sequential(stream: bytes, max_headers=16):
    """(method, target, fields, body) per request the reference's loop dispatches."""
    out, p = [], 0
    while p < len(stream):
        seg = stream[p:]
        buf = np.zeros(len(seg) + rhp.RHP_PAD, dtype=np.uint8)
        buf[: len(seg)] = np.frombuffer(seg, dtype=np.uint8)
        off = np.array([0, len(seg)], dtype=np.uint64)
        reqs, hdrs, http, rw = run_oracle(buf, off, max_headers, rhp.MODE_HTTP)
        res = int(http["result"][0])
        if res != 1:
            break
        r, b = reqs[0], bytes(rw[: len(seg)])
        fields = []
        for k in range(int(r["num_headers"])):
            h = hdrs[0][k]
            name = b"" if h["name_off"] < 0 else b[h["name_off"]: h["name_off"] + h["name_len"]]
            fields.append((name, b[h["value_off"]: h["value_off"] + h["value_len"]]))
        body = b""
        if http["body_kind"][0]:
            o = int(http["body_off"][0])
            body = b[o: o + int(http["body_len"][0])]
        out.append((b[r["method_off"]: r["method_off"] + r["method_len"]],
                    b[r["path_off"]: r["path_off"] + r["path_len"]], fields, body))
        p += int(http["consumed"][0])
    return out


def decode_echoes(raw: bytes):
    """Responses -> (method, target, fields, body) from echo_test's encoding."""
    out, p = [], 0
    while p < len(raw):
        end = raw.index(b"\r\n\r\n", p)
        head = raw[p:end].decode("latin-1")
        n = int([l for l in head.split("\r\n") if l.lower().startswith("content-length:")][0].split(":")[1])
        body = raw[end + 4: end + 4 + n]
        p = end + 4 + n
        q, items = 0, []
        while q < len(body):
            ln = struct.unpack_from("<I", body, q)[0]
            items.append(body[q + 4: q + 4 + ln])
            q += 4 + ln
        nf = struct.unpack("<I", items[2])[0]
        fields = [(items[3 + 2 * i], items[4 + 2 * i]) for i in range(nf)]
        out.append((items[0], items[1], fields, items[3 + 2 * nf]))
    return out


def run_echo(tmp_path, stream: bytes, chunk: int, parser: str, writer: str = "host", env=None):
    """env: further environment variables of the server (e.g. RHP_REACTOR_PACK)"""
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(stream)
    p = subprocess.run([ECHO, str(src), str(chunk), str(dst)],
                       env=dict(os.environ, RHP_REACTOR_PARSER=parser, RHP_REACTOR_WRITER=writer, **(env or {})),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr
    assert f"parser: {parser}" in p.stdout
    return decode_echoes(dst.read_bytes())


CASES = [("mixed", stream_mixed, 1 << 20), ("mixed", stream_mixed, 1000), ("mixed", stream_mixed, 61),
         ("mixed", stream_mixed, 7), ("bad", stream_bad, 1 << 20), ("bad", stream_bad, 50),
         ("wide", stream_wide, 1 << 20), ("wide", stream_wide, 1000), ("wide", stream_wide, 61)]
# the copy-back of the asynchronous parsers (reactor/batch.c): "1" the dense copies of
# rhp_pack_dense / rhp_cpu_pack_dense (the default), "0" the request-major records
PACK_CASES = [(name, make, chunk, pack) for name, make, chunk in CASES if name == "wide" for pack in ("0", "1")]
PACK_CASES += [("mixed", stream_mixed, 1000, "0")]


def check_echoes(got, want, name, chunk):
    """A stream that ends in a malformed request: the reference closes the
    session in the same parse pass (server.c:47-51) and never reaches the
    stream_flush at the end of that pass (:64), so the replies to the requests
    parsed in that pass are never sent -- with the whole stream in one recv,
    none at all.  The echoes are the oracle's requests up to the last pass
    before the close: a prefix, all of it for well-formed streams."""
    if name == "bad":
        assert got == want[: len(got)]
        if chunk >= 1 << 20:
            assert got == []
    else:
        assert got == want


@pytest.mark.parametrize("parser,writer", [("host", "host"), ("host-async", "host"), ("host-async", "host-batch")])
@pytest.mark.parametrize("name,make,chunk", CASES)
def test_server_records_match_oracle_sequential_loop(tmp_path, name, make, chunk, parser, writer):
    s = make()
    want = oracle_sequential(s)
    assert len(want) >= 3
    check_echoes(run_echo(tmp_path, s, chunk, parser, writer), want, name, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("writer", ["host", "gpu"])
@pytest.mark.parametrize("name,make,chunk", CASES)
def test_server_records_gpu_match_oracle_sequential_loop(tmp_path, name, make, chunk, writer):
    """GPU parser (asynchronous rounds); replies written by the host as the
    reference does, or by rhp_write_responses once per round."""
    s = make()
    check_echoes(run_echo(tmp_path, s, chunk, "gpu", writer), oracle_sequential(s), name, chunk)


@pytest.mark.parametrize("name,make,chunk,pack", PACK_CASES)
def test_server_records_pack_modes(tmp_path, name, make, chunk, pack):
    """host-async (the gpu parser's protocol on the CPU) with and without the dense copy-back"""
    s = make()
    want = oracle_sequential(s)
    assert len(want) >= 30
    check_echoes(run_echo(tmp_path, s, chunk, "host-async", env={"RHP_REACTOR_PACK": pack}), want, name, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("name,make,chunk,pack", PACK_CASES)
def test_server_records_gpu_pack_modes(tmp_path, name, make, chunk, pack):
    s = make()
    check_echoes(run_echo(tmp_path, s, chunk, "gpu", env={"RHP_REACTOR_PACK": pack}), oracle_sequential(s), name, chunk)


def test_stream_wide_slots():
    """stream_wide is what it says: every request is answered, and parsed as
    one batch, rhp_cpu_pack_dense leaves the slots named in its docstring wide
    and packs the ones inside the limits"""
    s = stream_wide()
    want = oracle_sequential(s)
    targets = [t for _, t, _, _ in want]
    for t in (b"/n62", b"/n63", b"/n100", b"/v1007", b"/v1008", b"/v1023", b"/v1024", b"/v1500", b"/m", b"/crlf",
              b"/nospace", b"/ows", b"/fold", b"/c"):
        assert t in targets, t
    assert b"/last" not in targets
    assert {len(m) for m, _, _, _ in want} >= {3, 255, 256}
    buf, off, sess, _ = rhp.pack_sessions([s])
    res, sres, starts = rhp.fixup_cpu(buf, off, sess, 16)
    n = len(off) - 1
    assert int(sres[0]["n_slots"]) == len(want) + 1   # (the incomplete tail's slot: result 0)
    assert (res.http["result"][: len(want)] == 1).all() and res.http["result"][len(want)] == 0
    dreq, _, _ = rhp.pack_dense_cpu(res, n, 16)
    wide = {}
    for i in range(len(want)):
        r = res.reqs[i]
        if res.http[i]["result"] == 1 and r["ret"] > 0:
            a = int(starts[i]) + int(r["path_off"])
            wide.setdefault(bytes(buf[a: a + int(r["path_len"])]), bool(dreq[8 * i + 7] & rhp.DENSE_WIDE))
    for t, w in ((b"/n62", False), (b"/n63", True), (b"/n100", True), (b"/v1007", False), (b"/v1008", True),
                 (b"/v1023", True), (b"/v1024", True), (b"/v1500", True), (b"/g", False), (b"/plaintext", False)):
        assert wide[t] == w, (t, wide)


def stream_posts():
    """64 pipelined Content-Length POSTs and 16 chunked POSTs in one write (VERDICT r2
    'What's missing' 1): bodies end past their speculative pieces, one body holds
    empty lines and a whole fake request."""
    parts = []
    for i in range(64):
        body = b"b%03d" % i + (b"\r\n\r\nGET /fake HTTP/1.1\r\n\r\n" if i == 7 else b"")
        parts.append(b"POST /p%d HTTP/1.1\r\nContent-Length: %d\r\n\r\n" % (i, len(body)) + body)
    for i in range(16):
        parts.append(b"POST /c%d HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n3\r\nc%02d\r\n0\r\n\r\n" % (i, i))
    return b"".join(parts)


def rounds_of(tmp_path, stream, parser):
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(stream)
    p = subprocess.run([ECHO, str(src), str(1 << 20), str(dst)],
                       env=dict(os.environ, RHP_REACTOR_PARSER=parser, RHP_REACTOR_STATS="1"),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "OK" in p.stdout, p.stdout + p.stderr
    line = [l for l in p.stderr.splitlines() if l.startswith("server rounds:")][0]
    return int(line.split(":")[1].split(",")[0]), decode_echoes(dst.read_bytes())


@pytest.mark.parametrize("parser", ["host", "host-async"])
def test_pipelined_bodies_in_one_round(tmp_path, parser):
    s = stream_posts()
    rounds, got = rounds_of(tmp_path, s, parser)
    assert got == oracle_sequential(s)
    assert len(got) == 80
    assert rounds <= 2, rounds


@pytest.mark.gpu
def test_pipelined_bodies_in_one_round_gpu(tmp_path):
    s = stream_posts()
    rounds, got = rounds_of(tmp_path, s, "gpu")
    assert got == oracle_sequential(s)
    assert rounds <= 2, rounds


def stream_fake_chunked():
    """Content-Length bodies that hold whole chunked requests: the
    server's empty-line splitter makes pieces of them whose speculative parses
    are chunked requests, some complete within the bytes after them, that the
    fix-up absorbs into the body; real chunked requests around them are
    de-framed, so the round copies de-framed bytes back (reactor/batch.c walks
    only the record slots each session filled)."""
    fake = (b"POST /fake HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n4\r\nfake\r\n0\r\n\r\n")
    parts = []
    for i in range(12):
        body = b"x\r\n\r\n" + fake * (1 + i % 3) + b"tail%02d" % i
        parts.append(b"POST /cl%d HTTP/1.1\r\nContent-Length: %d\r\n\r\n" % (i, len(body)) + body)
        parts.append(b"POST /ch%d HTTP/1.1\r\nTransfer-Encoding: chunked\r\n\r\n2\r\nc%d\r\n0\r\n\r\n" % (i, i % 10))
    parts.append(fake)   # a real one at the end
    return b"".join(parts)


@pytest.mark.parametrize("parser", ["host", "host-async"])
def test_fake_chunked_inside_bodies(tmp_path, parser):
    s = stream_fake_chunked()
    _, got = rounds_of(tmp_path, s, parser)
    want = oracle_sequential(s)
    assert len(want) == 25 and got == want


@pytest.mark.gpu
def test_fake_chunked_inside_bodies_gpu(tmp_path):
    s = stream_fake_chunked()
    _, got = rounds_of(tmp_path, s, "gpu")
    assert got == oracle_sequential(s)
