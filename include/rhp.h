/*
 * rhp.h -- MI355X batched HTTP/1.1 request parser: the C-ABI drop-in boundary.
 *
 * Replaces, for a batch of independent request buffers already in HBM:
 *   int phr_parse_request(const char *buf, size_t len, const char **method,
 *       size_t *method_len, const char **path, size_t *path_len, int *minor_version,
 *       struct phr_header *headers, size_t *num_headers, size_t last_len);
 *                       /root/reference/src/picohttpparser/picohttpparser.h:51-52
 *   int http_read_request(stream_t *, string_t *method, string_t *target, data_t *body,
 *       http_field_t *fields, size_t *fields_count);
 *                       /root/reference/src/reactor/http.h:36 (http.c:177-234)
 *
 * One call parses n requests.  Request i is bytes[offsets[i] .. offsets[i+1]) (its
 * `len`); the bytes after it (the next request, then >= RHP_PAD zero bytes after
 * the last one) are what the reference would read past the end.
 * Every pointer the reference returns into `buf` is returned here as an offset
 * from the request start (pointer - buf).  All buffers are device memory owned by
 * the caller; the call is asynchronous on `stream` (a hipStream_t).
 *
 * Requests of any length are parsed.  Records are compact (u16 offsets), so
 * the one answer they cannot carry is a successful parse whose header section
 * is longer than RHP_MAX_LEN bytes (phr ret > 65535): that request gets
 * ret = RHP_RET_TOOLONG (and in RHP_MODE_HTTP result = RHP_RET_TOOLONG) and no
 * other output; the caller parses it with a pointer-based parser
 * (rhp_phr_parse_request / rhp_http_read_cpu, include/rhp_host.h).  -1, -2 and
 * http results 0/-1 are exact at every length; body lengths and `consumed` are
 * u64.
 */
#ifndef RHP_H
#define RHP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RHP_PAD 256u            /* zero bytes required after the last request */
#define RHP_MAX_LEN 65535u      /* longest header section (phr ret) the u16 records hold */
#define RHP_MAX_HEADERS 64u     /* largest supported *num_headers capacity */
#define RHP_RET_TOOLONG (-3)

enum rhp_mode {
  RHP_MODE_PHR = 0,   /* phr_parse_request(buf, len, ..., &num_headers = max, last_len = 0) */
  RHP_MODE_HTTP = 1   /* http_read_request over a stream whose unconsumed input is the request */
};

/* phr_parse_request result for one request (16 B).  For ret <= 0 only `ret`
 * is meaningful (the reference leaves the other outputs unspecified). */
typedef struct rhp_req {
  int32_t  ret;            /* >0 bytes consumed, -1 malformed, -2 partial, RHP_RET_TOOLONG (ret > RHP_MAX_LEN) */
  uint16_t method_len;
  uint16_t path_off;
  uint16_t path_len;
  uint8_t  method_off;     /* 0, 1 or 2 (one optional leading CRLF / LF) */
  int8_t   minor_version;
  uint16_t num_headers;
  uint16_t flags;          /* RHP_F_* diagnostics, not part of parity */
} rhp_req_t;

#define RHP_F_EXACT 0x1u   /* resolved by the exact (scalar) device path, not the DFA */
#define RHP_F_WIDE  0x2u   /* RHP_LAYOUT_COMPACT: this request's header records are the wide ones */

/* struct phr_header as offsets (8 B); name_off == RHP_NAME_NULL encodes name ==
 * NULL (obs-fold continuation line, picohttpparser.c:318-321). */
typedef struct rhp_hdr {
  uint16_t name_off, name_len;
  uint16_t value_off, value_len;
} rhp_hdr_t;

#define RHP_NAME_NULL 0xFFFFu

/* Layout of the header records.  Request-major (the C array hdrs[n][max_headers],
 * the default): a request's records are contiguous.  Header-major
 * (hdrs[max_headers][n]): the records of one header index are contiguous across
 * requests, so the records a wave completes together for consecutive requests of
 * a uniform batch are whole lines (request-major writes them as one partial
 * line per request, which HBM handles at a fraction of its write rate:
 * profiles/r02/ubench_records.txt).  Records past num_headers are unspecified. */
enum rhp_layout {
  RHP_LAYOUT_REQUEST_MAJOR = 0,
  RHP_LAYOUT_HEADER_MAJOR = 1,
  RHP_LAYOUT_COMPACT = 2,     /* 4-byte header records, below (http mode: 8-byte http records too;
                                 not with RHP_BATCH_SPECULATIVE) */
  RHP_LAYOUT_DENSE = 3,       /* 8-byte request and 2-byte header records, below (both modes; in
                                 RHP_MODE_HTTP the http records are the compact ones and `http`
                                 holds RHP_COMPACT_HTTP_BYTES(n) bytes; not with
                                 RHP_BATCH_SPECULATIVE) */
  RHP_LAYOUT_DENSE_RM = 4     /* the same, the header records request-major (RHP_MODE_PHR only:
                                 refused in RHP_MODE_HTTP) */
};
/* Compact records (RHP_LAYOUT_COMPACT).  A header line the DFA
 * parses is `name ": " value CRLF` and the first one starts right after the
 * request line `method SP path SP "HTTP/1." digit CRLF`, so its record is two
 * lengths: hdrs holds u32 lens[max_headers][n] (header-major), name_len |
 * value_len << 16, and the offsets follow by a running sum,
 *   name_off(0) = path_off + path_len + 11
 *   value_off(k) = name_off(k) + name_len(k) + 2
 *   name_off(k + 1) = value_off(k) + value_len(k) + 2.
 * A request whose flags hold RHP_F_WIDE (the exact path parsed it: leading
 * CRLF, OWS, obs-fold, bare LF, ...) has its records as rhp_hdr_t in the wide
 * area, wide[n][max_headers] (request-major) at byte RHP_COMPACT_WIDE_OFF(n, m)
 * of hdrs.  hdrs holds RHP_COMPACT_HDRS_BYTES(n, m) bytes; rhp_expand_records
 * (rhp_host.h) turns a batch's records into rhp_hdr_t on the host.  The
 * records a uniform batch writes shrink from 8 to 4 bytes per header (config
 * 2: 48 -> 32 B per request with the 16-B request record). */
#define RHP_COMPACT_WIDE_OFF(n, m) ((((size_t) (n) * (size_t) (m) * 4u) + 15u) & ~(size_t) 15u)
#define RHP_COMPACT_HDRS_BYTES(n, m) (RHP_COMPACT_WIDE_OFF(n, m) + (size_t) (n) * (size_t) (m) * 8u)
/* Dense records (RHP_LAYOUT_DENSE in both modes, RHP_LAYOUT_DENSE_RM in
 * RHP_MODE_PHR; round 6).  The compact layout's running-sum offsets with
 * narrower fields, for the DFA's records.  In RHP_MODE_HTTP the http records
 * of a dense batch are the compact ones (rhp_http_compact_t, below).  reqs holds rhp_req_dense_t dreq[n] (8 B) and, at byte
 * RHP_DENSE_REQ_WIDE_OFF(n), a wide area rhp_req_t wide[n]
 * (RHP_DENSE_REQS_BYTES(n) bytes in all).  hdrs holds u16 lens, name_len |
 * value_len << 6, at index k * n + i (RHP_LAYOUT_DENSE, header-major) or
 * i * m + k (RHP_LAYOUT_DENSE_RM, request-major); a header whose name is longer
 * than RHP_DENSE_NAME_MAX or value longer than RHP_DENSE_VALUE_MAX has
 * RHP_DENSE_OVERFLOW there and its u32 lengths, name_len | value_len << 16, at
 * the same index of the overflow area at byte RHP_DENSE_OVF_OFF(n, m); the wide
 * header records rhp_hdr_t wide[n][m] follow at RHP_DENSE_WIDE_OFF(n, m)
 * (RHP_DENSE_HDRS_BYTES(n, m) bytes in all).  A DFA request is dense when its
 * method is at most 255 bytes (path_off = method_len + 1, method_off = 0); any
 * other (and every request the exact path parses) is wide: dreq[i].flags holds
 * RHP_DENSE_WIDE, its records are wide[i] and the wide header records.
 * RHP_DENSE_BAD: ret = -1 (the other outputs unspecified, as in rhp_req_t).
 * Config 2 writes 8 + 4 x 2 = 16 B of records per request (compact: 32 B).
 * rhp_expand_reqs / rhp_expand_records / rhp_expand_http (rhp_host.h) expand
 * them on the host; rhp_records.h states every encoding and area of this file
 * once, as inline C (its decoders are what a C consumer calls). */
typedef struct rhp_req_dense {
  uint16_t ret;           /* 1..65535 (the header section), when neither flag is set */
  uint16_t path_len;
  uint8_t  method_len;
  uint8_t  num_headers;
  uint8_t  minor_version;
  uint8_t  flags;         /* RHP_DENSE_WIDE, RHP_DENSE_BAD */
} rhp_req_dense_t;
#define RHP_DENSE_WIDE 1u
#define RHP_DENSE_BAD  2u
#define RHP_DENSE_NAME_MAX 62u    /* longest name a dense header record holds */
#define RHP_DENSE_VALUE_MAX 1007u /* longest value */
#define RHP_DENSE_REQ_WIDE_OFF(n) ((((size_t) (n) * 8u) + 15u) & ~(size_t) 15u)
#define RHP_DENSE_REQS_BYTES(n) (RHP_DENSE_REQ_WIDE_OFF(n) + (size_t) (n) * 16u)
#define RHP_DENSE_OVERFLOW 0xFFFFu
#define RHP_DENSE_OVF_OFF(n, m) ((((size_t) (n) * (size_t) (m) * 2u) + 15u) & ~(size_t) 15u)
#define RHP_DENSE_WIDE_OFF(n, m) (RHP_DENSE_OVF_OFF(n, m) + ((((size_t) (n) * (size_t) (m) * 4u) + 15u) & ~(size_t) 15u))
#define RHP_DENSE_HDRS_BYTES(n, m) (RHP_DENSE_WIDE_OFF(n, m) + (size_t) (n) * (size_t) (m) * 8u)

/* record k of request i in a batch of n requests with capacity m */
#define RHP_HDR(hdrs, layout, n, m, i, k) \
  ((hdrs)[(layout) == RHP_LAYOUT_HEADER_MAJOR ? (size_t) (k) * (n) + (i) : (size_t) (i) * (m) + (k)])

/* http_read_request result (24 B), RHP_MODE_HTTP only */
typedef struct rhp_http {
  int32_t  result;         /* 1 ready, 0 need more bytes / empty, -1 malformed, RHP_RET_TOOLONG */
  uint32_t body_kind;      /* 0: data_null(); 1: body = (req.ret, body_len);
                              RHP_BODY_CHUNKED_PENDING: a speculative batch's chunked body,
                              validated, not yet de-framed (rhp_fixup_sessions finishes it) */
  uint64_t consumed;       /* bytes stream_consume() is given (mod 2^64, http.c:216) */
  uint64_t body_len;
} rhp_http_t;

/* Compact http records (RHP_LAYOUT_COMPACT and RHP_LAYOUT_DENSE, RHP_MODE_HTTP): http holds
 * rhp_http_compact_t hc[n] (8 B) and, at byte RHP_COMPACT_HTTP_WIDE_OFF(n), a
 * wide area rhp_http_t wide[n]; RHP_COMPACT_HTTP_BYTES(n) bytes in all.  A
 * record without RHP_HTTP_WIDE holds result, body_kind and body_len, and
 * consumed = ret + (body_kind == 1 ? body_len : 0) for result 1, else 0 (the
 * DFA path's framing: no body, or a Content-Length body).  A record with
 * RHP_HTTP_WIDE (the exact path, a chunked body de-framed in place) is
 * wide[i].  rhp_expand_http (rhp_host.h) turns them into rhp_http_t.  With
 * the compact header records, a uniform batch writes 16 + 4 h + 8 bytes per
 * request (config 5: 40 B, was 16 + 8 h + 24 = 70 B header-major). */
typedef struct rhp_http_compact {
  int8_t   result;
  uint8_t  body_kind;
  uint8_t  flags;       /* RHP_HTTP_WIDE */
  uint8_t  reserved;
  uint32_t body_len;
} rhp_http_compact_t;
#define RHP_HTTP_WIDE 1u
#define RHP_COMPACT_HTTP_WIDE_OFF(n) ((((size_t) (n) * 8u) + 15u) & ~(size_t) 15u)
#define RHP_COMPACT_HTTP_BYTES(n) (RHP_COMPACT_HTTP_WIDE_OFF(n) + (size_t) (n) * 24u)

typedef struct rhp_batch {
  const uint8_t  *bytes;   /* device, 16-byte aligned: packed requests + RHP_PAD zero bytes */
  uint8_t        *bytes_rw;/* device, RHP_MODE_HTTP: same buffer, writable (chunked
                              bodies are de-framed in place, http.c:134-160; a request's
                              writes stay inside its own [offsets[i], offsets[i+1]), the
                              bytes around its body rewritten with their own values, so
                              the caller may fill other requests meanwhile); may be NULL
                              in RHP_MODE_PHR */
  const uint64_t *offsets; /* device: n + 1 offsets, non-decreasing */
  uint64_t        bytes_size; /* readable bytes at `bytes` (>= offsets[n] + RHP_PAD) */
  uint32_t        n;
  uint32_t        max_headers; /* headers capacity per request (*num_headers in) */
  uint32_t        mode;        /* enum rhp_mode */
  uint32_t        layout;      /* enum rhp_layout: where record k of request i lives in hdrs */
  rhp_req_t      *reqs;        /* device [n] (RHP_LAYOUT_DENSE / _DENSE_RM: RHP_DENSE_REQS_BYTES(n) bytes,
                                  rhp_req_dense_t and the wide area) */
  rhp_hdr_t      *hdrs;        /* device [n * max_headers] records, laid out as `layout` says
                                  (n * max_headers < 2^32); RHP_LAYOUT_COMPACT:
                                  RHP_COMPACT_HDRS_BYTES(n, max_headers) bytes; RHP_LAYOUT_DENSE:
                                  RHP_DENSE_HDRS_BYTES(n, max_headers) bytes */
  rhp_http_t     *http;        /* device [n], RHP_MODE_HTTP (RHP_LAYOUT_COMPACT and RHP_LAYOUT_DENSE:
                                  RHP_COMPACT_HTTP_BYTES(n) bytes, rhp_http_compact_t) */
  uint32_t       *work;        /* reserved, may be NULL (device scratch of RHP_WORK_WORDS u32
                                  for future kernels; the current ones keep their scheduling
                                  state in LDS) */
  uint32_t        flags;       /* RHP_BATCH_* */
  uint32_t        reserved;
  const uint64_t *last_len;    /* device [n] or NULL (= all 0), RHP_MODE_PHR only:
                                  phr_parse_request's last_len per request
                                  (picohttpparser.c:383, 399-401): when last_len[i] != 0 the
                                  slowloris pre-check is_complete (:197-223) runs first and
                                  its -2 / -1 is the answer.  Contract: last_len[i] <= len
                                  (the reference reads before `buf_end` only then) */
} rhp_batch_t;

#define RHP_WORK_WORDS 64u
#define RHP_BODY_CHUNKED_PENDING 2u

/* rhp_batch_t.flags */
#define RHP_BATCH_SPECULATIVE 1u   /* RHP_MODE_HTTP: the requests may be speculative pieces of
                                      pipelined input (rhp_fixup_sessions below): nothing is
                                      written to bytes_rw (chunked bodies are validated and
                                      left framed, body_kind RHP_BODY_CHUNKED_PENDING) */

/* Parse a batch on `stream` (hipStream_t) of the calling thread's current
 * device.  Returns 0 on successful launch, a negative errno-style code for bad
 * arguments, or a positive hipError_t.  Thread-safe: one host thread per GPU
 * may call it concurrently (per-device state is cached per device id). */
int rhp_parse_batch(const rhp_batch_t *batch, void *stream);

/*
 * Pipelined input (the reference's server_session_read loop,
 * /root/reference/src/reactor/server.c:37-65, advancing by http.c:200, 216, 232).
 * A session's unconsumed input is split by the caller at every empty line (the
 * end of a header section: LF LF or LF CR LF) into pieces that are consecutive
 * requests of a RHP_BATCH_SPECULATIVE http batch, so every request's header
 * section ends a piece (#pieces >= #requests); rhp_split_sessions (below) is
 * that split on the device, from the sessions' packed bytes to offsets[] and
 * rhp_session_t[].  After rhp_parse_batch,
 * rhp_fixup_sessions walks each session in order, as http_read_request would be
 * called in a loop over the whole input: a piece that starts at the next request
 * boundary and whose result cannot change with more input (1 within the piece,
 * -1, RHP_RET_TOOLONG, or 0 for the session's last piece) is taken (a pending
 * chunked body is de-framed in place now); anything else (a body that ran past
 * its piece, a piece that started inside a body) is parsed again from the true
 * boundary over the rest of the session's input.  Request m of a session is
 * left in record slot piece_lo + m (reqs/hdrs/http of the batch), its start
 * in req_start[piece_lo + m].  One launch, one thread per session.  Any split
 * gives the reference's answers: with a coarser one (a piece holding several
 * requests) a piece whose records an earlier request of the walk has already
 * overwritten is parsed again from its boundary, and a session with more
 * requests than pieces stops with `more`.
 */
typedef struct rhp_session {
  uint32_t piece_lo, piece_hi;   /* the session's pieces: requests [piece_lo, piece_hi) of the
                                    batch, its bytes [offsets[piece_lo], offsets[piece_hi]) */
} rhp_session_t;

typedef struct rhp_session_result {
  uint32_t n_slots;   /* record slots filled: every one but the last has result 1; the last
                         one's result says where the session stopped (1: input used up) */
  uint32_t more;      /* 1: more requests than pieces (a coarser split than one per empty
                         line): the rest from offsets[piece_lo] + consumed needs another batch */
  uint64_t consumed;  /* bytes of the session's input taken by its result-1 requests */
} rhp_session_result_t;

/* Launch status as rhp_parse_batch.  `batch` is the speculative batch already
 * parsed on `stream`; sessions, results and req_start (u64 [n]) are device
 * memory. */
int rhp_fixup_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                       rhp_session_result_t *results, uint64_t *req_start, void *stream);

/* Dense copies of a parsed http batch's records (round 6: what the reactor
 * copies back to the host, reactor/batch.c).  For each record slot i of a
 * RHP_MODE_HTTP batch in RHP_LAYOUT_REQUEST_MAJOR (speculative or not), after
 * the parse (and rhp_fixup_sessions, when used): the request record as
 * rhp_req_dense_t dreq[i], the http record as rhp_http_compact_t hc[i] and the
 * header lengths as u16 lens16[k * n + i], k < num_headers, in
 * RHP_LAYOUT_DENSE's encodings (a record whose consumed follows from ret and
 * body_len; a request whose http record is such a record and whose offsets
 * follow the running sum with names of at most RHP_DENSE_NAME_MAX and values of
 * at most RHP_DENSE_VALUE_MAX bytes -- a de-framed chunked body moves its
 * request's bytes, so that request stays wide).
 * Any other slot is marked RHP_HTTP_WIDE / RHP_DENSE_WIDE: its records are the
 * batch's own.  Device pointers; launch status as rhp_parse_batch. */
int rhp_pack_dense(const rhp_batch_t *batch, rhp_req_dense_t *dreq, rhp_http_compact_t *hc, uint16_t *lens16,
                   void *stream);

/* Which kernel implementation rhp_parse_batch uses (diagnostics / A-B tests). */
enum rhp_impl {
  RHP_IMPL_DFA = 0,    /* lane-per-request byte DFA with LDS tables (default) */
  RHP_IMPL_EXACT = 1,  /* lane-per-request exact scalar path only (slow reference path) */
  RHP_IMPL_DFA_LATE = 2 /* the DFA kernel in its late-issue form in both modes (the default
                           uses that form in RHP_MODE_HTTP only) */
};
int rhp_set_impl(int impl);   /* per calling thread */

/* Name of the kernel symbol the default implementation launches (for profiles). */
const char *rhp_kernel_name(void);

/* Library version string. */
const char *rhp_version(void);

/*
 * Batched response serialization: http_write_response (src/reactor/http.c:236-297,
 * decl http.h:37) for n responses at once, on the device.  Response i is written to
 * out[out_off[i], out_off[i+1]) byte for byte as the reference appends it to the
 * stream's output:
 *   "HTTP/1.1 " status CRLF "Server: *" CRLF "Date: " date CRLF
 *   "Content-Type: " type CRLF "Content-Length: " decimal(body_len) CRLF
 *   { name ": " value CRLF }  CRLF body
 * Every string of a response is a span of the device `arena`.  The date is one
 * 29-byte IMF-fixdate for the batch (the reactor's cached date; http.c:244 sizes
 * the response for exactly 29 date bytes, so other lengths are rejected).
 */
typedef struct rhp_span {
  uint32_t off, len;         /* bytes arena[off, off + len) */
} rhp_span_t;

typedef struct rhp_resp {
  rhp_span_t status;         /* e.g. "200 OK" */
  rhp_span_t type;           /* Content-Type value */
  rhp_span_t body;
  uint32_t   fields_first;   /* extra fields: fields[fields_first .. + fields_count) */
  uint32_t   fields_count;
} rhp_resp_t;

typedef struct rhp_resp_field {
  rhp_span_t name, value;
} rhp_resp_field_t;

#define RHP_DATE_LEN 29u

typedef struct rhp_resp_batch {
  const uint8_t          *arena;    /* device, any alignment.  The writer reads a span as the whole
                                       aligned dwords that hold it: up to 3 bytes before a span's
                                       first byte and up to 3 bytes beyond its last.  So the
                                       arena's memory must be readable from the 4-byte boundary at
                                       or below its first byte up to the next 4-byte boundary
                                       after its last byte (an arena inside a device allocation
                                       whose start and size are multiples of 4 is); an empty span
                                       is not read at all, wherever its off points */
  const rhp_resp_t       *resps;    /* device [n] */
  const rhp_resp_field_t *fields;   /* device, may be NULL when no response has fields */
  uint32_t                n;
  uint32_t                date_len; /* must be RHP_DATE_LEN */
  const char             *date;     /* host, date_len bytes */
  uint64_t               *out_off;  /* device [n + 1]: written (exclusive prefix sum of sizes) */
  uint8_t                *out;      /* device, out_size bytes */
  uint64_t                out_size; /* when out_off[n] > out_size nothing is written to `out`
                                       (out_off still holds every size: grow and call again) */
  uint64_t               *work;     /* device scratch, >= RHP_RESP_WORK_WORDS(n) u64 */
} rhp_resp_batch_t;

#define RHP_RESP_WORK_WORDS(n) (((uint64_t) (n) + 4095u) / 4096u + 1u)

/* Launch status as rhp_parse_batch; four kernels on `stream` (sizes with tile
 * sums, two scan passes, copy). */
int rhp_write_responses(const rhp_resp_batch_t *batch, void *stream);

/*
 * Batched header lookup and route match: what a server does between
 * http_read_request and http_write_response, for a parsed batch whose bytes and
 * records stay in HBM.
 *   string_t http_field_lookup(http_field_t *, size_t, string_t name);
 *                       src/reactor/http.c:167-175 (decl http.h:35): the value of
 *                       the first field whose name is string_equal_case to `name`
 *                       (equal sizes and gnulib memcasecmp, src/reactor/data.c:11-28,
 *                       string.c), string_null() when there is none
 *   string_equal(request.method / request.target, ...)
 *                       the dispatch of the reference's users (http.c:198,
 *                       test/server.c:75-82): equal sizes and memcmp
 * For request i of a batch that rhp_parse_batch has parsed on `stream`, in any
 * record layout and either mode the parser accepts (the combinations it
 * refuses are refused here with the same code):
 *   a request is "ready" when ret > 0 (RHP_MODE_PHR; RHP_RET_TOOLONG is not) or
 *   result == 1 (RHP_MODE_HTTP);
 *   fields[j * n + i] is the value span (offsets from the request's start, as
 *   rhp_hdr_t) of the first header record k < num_headers whose name is not
 *   NULL (an obs-fold line never matches), has the length of name j and equals
 *   it byte for byte after both sides' ASCII a..z are mapped to A..Z (the C
 *   locale's toupper: no other byte is mapped, so '^' and '~', '_' and DEL, '`'
 *   and '@' differ); a header that is present with an empty value gives
 *   {value_off, 0}; no such header, or a request that is not ready, gives
 *   {RHP_NAME_NULL, 0};
 *   route[i] is the index of the first route whose target has the path's length
 *   and bytes and whose method has the method's (a route with method.len == 0
 *   takes any method); RHP_ROUTE_NONE when there is none or the request is not
 *   ready.
 * The records of a request that is not ready and those past num_headers are
 * unspecified and are not used.  The request's bytes are read as the parse
 * left them (http mode: through bytes_rw, after chunked bodies were de-framed
 * in place), the name bytes only of records whose name_len is a lookup name's,
 * as the aligned dwords that hold them.
 * RHP_BATCH_SPECULATIVE batches are refused (-EINVAL): after
 * rhp_fixup_sessions a slot's offsets are relative to req_start, not to
 * offsets[i]; rhp_classify_sessions (below) classifies those slots.  Also -EINVAL: an empty
 * name or one longer than RHP_CLASSIFY_NAME_MAX, a count above its limit,
 * route text above RHP_CLASSIFY_TEXT_MAX, n_names == 0 && n_routes == 0, a
 * missing table or output.  n == 0 succeeds and launches nothing.
 * Launch contract as rhp_parse_batch: asynchronous on `stream`, no allocation
 * and no synchronisation; the host tables (text, names, routes) are copied
 * into the launch and may be freed when the call returns; thread-safe.
 */
#define RHP_CLASSIFY_MAX_NAMES   16u   /* header names looked up per call */
#define RHP_CLASSIFY_NAME_MAX    64u   /* longest lookup name, bytes; names are non-empty */
#define RHP_CLASSIFY_MAX_ROUTES  32u
#define RHP_CLASSIFY_TEXT_MAX  2048u   /* total bytes of all route methods + targets */
#define RHP_ROUTE_NONE       0xFFFFu

typedef struct rhp_fieldref {
  uint16_t value_off, value_len;   /* absent: value_off == RHP_NAME_NULL, value_len == 0 */
} rhp_fieldref_t;

typedef struct rhp_route {
  rhp_span_t method, target;       /* spans of `text`; method.len == 0: any method */
} rhp_route_t;

typedef struct rhp_classify {
  const uint8_t     *text;      /* host: the bytes of the names and routes */
  const rhp_span_t  *names;     /* host [n_names]: spans of `text` */
  const rhp_route_t *routes;    /* host [n_routes], may be NULL when n_routes == 0 */
  uint32_t           n_names, n_routes;
  rhp_fieldref_t    *fields;    /* device [n_names * n], name-major: fields[j * n + i] */
  uint16_t          *route;     /* device [n]; may be NULL when n_routes == 0 */
} rhp_classify_t;

int rhp_classify_batch(const rhp_batch_t *batch, const rhp_classify_t *c, void *stream);

/*
 * The same lookup and route match over pipelined input: `batch` is a
 * RHP_BATCH_SPECULATIVE http batch exactly as rhp_parse_batch and
 * rhp_fixup_sessions left it on `stream`; sessions, results (as
 * rhp_fixup_sessions wrote them) and req_start (u64 [n], the same) are the
 * fix-up's arguments, device memory.  Outputs as rhp_classify_batch, indexed by
 * record slot: fields[j * n + i] and route[i] for every i < batch->n.
 *   Slot i is in use when some session s has
 *   piece_lo(s) <= i < piece_lo(s) + results[s].n_slots.  An in-use slot whose
 *   http[i].result == 1 and reqs[i].ret > 0 is ready and is classified as
 *   rhp_classify_batch documents, with one difference: the request's first
 *   byte is req_start[i], not offsets[i] (the value spans are offsets from
 *   there).  A ready request lies inside its session's input,
 *   offsets[piece_lo] <= req_start[i] and req_start[i] + ret <=
 *   offsets[piece_hi]; a slot whose records say otherwise is absent.
 *   Every other slot -- one that is not in use, a session's last slot that
 *   stopped on 0 / -1 / RHP_RET_TOOLONG, every slot when n_sessions == 0 --
 *   gets {RHP_NAME_NULL, 0} for every name and RHP_ROUTE_NONE.  Of a slot that
 *   is not in use neither the records nor req_start[i] are read: they hold
 *   stale speculative records or nothing at all, and nobody has to zero them.
 * The bytes are read through bytes_rw when it is set (the fix-up de-frames
 * chunked bodies in place; a header section does not move).
 * Contract: `sessions` is in ascending piece_lo order with disjoint
 * [piece_lo, piece_hi) ranges (one session's pieces follow the previous
 * one's).  When the order is violated a slot may be reported absent; nothing
 * outside the batch's buffers is read.
 * -EINVAL: a batch that is not RHP_MODE_HTTP or whose flags are not exactly
 * RHP_BATCH_SPECULATIVE; anything rhp_parse_batch refuses for such a batch
 * (which leaves RHP_LAYOUT_REQUEST_MAJOR and RHP_LAYOUT_HEADER_MAJOR);
 * n_sessions > 0 with a NULL sessions, results or req_start; every table and
 * output rule of rhp_classify_batch.  n == 0 succeeds and launches nothing;
 * bytes_rw may be NULL.  Launch contract as rhp_classify_batch: one launch,
 * no copy, no allocation, no synchronisation.
 */
int rhp_classify_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                          const rhp_session_result_t *results, const uint64_t *req_start,
                          const rhp_classify_t *c, void *stream);

/*
 * Static routes answered on the device: from route[] (rhp_classify_sessions'
 * output) and the fix-up's results straight to each session's reply bytes,
 * ready for one D2H copy and one write() per session.  A static route's reply
 * is one byte string per round (the date is one per batch), so the caller
 * serializes one response per route with rhp_write_responses whenever the date
 * changes; that call's `out` and `out_off` are the reply images here.  The
 * replies of a session lie back to back in request order, as the reference
 * appends them to the stream (src/reactor/server.c:174, http.c:248, 276).
 *   batch, sessions, n_sessions, results: rhp_classify_sessions' arguments;
 *   route: its output, device u16 [n].
 *   Slot i is static when route[i] < table->n_routes and bit route[i] of
 *   static_mask is set (rhp_classify_sessions writes RHP_ROUTE_NONE to every
 *   slot that is not an in-use, ready request; a value >= n_routes is not
 *   static and never indexes image_off).
 *   count(s) is the length of the leading run of static slots in
 *   [piece_lo, piece_lo + results[s].n_slots): the run stops at the first
 *   request the host must answer, since a later reply cannot be sent ahead of
 *   it.  count(s) is 0 when the session's walk stopped on -1 (n_slots >= 1 and
 *   http[piece_lo + n_slots - 1].result == -1: the reference closes such a
 *   session without flushing what it wrote, server.c:47-51, 64; this is the
 *   only record of the batch that is read), and for a session whose fields do
 *   not satisfy piece_lo <= piece_lo + n_slots <= piece_hi <= n.
 *   out holds the sessions' replies in ascending session index, each
 *   session's in request order: out_off(s) is the sum of the earlier sessions'
 *   out_len, out_len(s) the sum of its answered slots' image lengths (an empty
 *   image is an answered request).  replies[s] for every s < n_sessions and
 *   *total are always written.
 * Contract: `sessions` ascends by piece_lo with disjoint ranges, as for
 * rhp_classify_sessions.  With that order violated the answers are unspecified;
 * still nothing is read outside the arguments' buffers and nothing is written
 * outside replies[0, n_sessions), total, work and out[0, out_size).
 * The images are read as the aligned dwords that hold them: no byte outside
 * images[image_off[0], image_off[n_routes]) rounded out to 4-byte boundaries
 * (the `out` of rhp_write_responses inside an allocation whose start and size
 * are multiples of 4 is readable so), and none of an image whose route is not
 * in static_mask or is not answered.
 * -EINVAL: whatever rhp_classify_sessions refuses about the batch, sessions and
 * results; a NULL route, table, o, image_off, replies, total or work; n_routes
 * 0 or above RHP_CLASSIFY_MAX_ROUTES; a NULL out with out_size > 0; a NULL
 * images unless every image is empty (the host twin, rhp_host.h, checks the
 * lengths; the device entry cannot read image_off and with a NULL images copies
 * no image byte at all).  n_sessions == 0 writes *total = 0 and nothing else;
 * n == 0 with sessions gives every session count 0.
 * Launch contract as rhp_classify_sessions: asynchronous on `stream`, no
 * allocation, no host synchronisation, no copy; thread-safe.  Four launches
 * (tile sums, one workgroup's scan of them, the tiles' scan, copy with the
 * per-session records), as rhp_write_responses; two when n == 0, one when
 * n_sessions == 0.
 */
typedef struct rhp_reply_table {
  const uint8_t  *images;      /* device: serialized replies back to back, any alignment
                                  (rhp_write_responses' `out` for n_routes responses) */
  const uint64_t *image_off;   /* device [n_routes + 1], non-decreasing (its `out_off`):
                                  route r's reply is images[image_off[r], image_off[r+1]) */
  uint32_t        n_routes;    /* 1..RHP_CLASSIFY_MAX_ROUTES: the classify call's n_routes */
  uint32_t        static_mask; /* bit r set: route r is answered here; clear: the host answers it */
} rhp_reply_table_t;

typedef struct rhp_session_reply {     /* 24 B */
  uint32_t count;     /* the session's first `count` requests (slots piece_lo .. piece_lo+count-1) are answered */
  uint32_t reserved;  /* written 0 */
  uint64_t out_off;   /* their replies, in request order: out[out_off, out_off + out_len) */
  uint64_t out_len;
} rhp_session_reply_t;

typedef struct rhp_reply_out {
  rhp_session_reply_t *replies;  /* device [n_sessions] */
  uint64_t            *total;    /* device [1]: sum of every out_len */
  uint8_t             *out;      /* device, out_size bytes, any alignment */
  uint64_t             out_size; /* when *total > out_size nothing is written to `out`; replies and total are still
                                    complete (grow and call again), as rhp_write_responses */
  uint64_t            *work;     /* device scratch, >= RHP_REPLY_WORK_WORDS(n, n_sessions) u64 */
} rhp_reply_out_t;

/* per slot an offset (and one more), per 64 slots a mask, per 256 slots three words of its tile's sum */
#define RHP_REPLY_WORK_WORDS(n, n_sessions) \
  ((uint64_t) (n) + 1u + ((uint64_t) (n) + 63u) / 64u + 3u * (((uint64_t) (n) + 255u) / 256u) + 0u * (uint64_t) (n_sessions))

int rhp_reply_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                       const rhp_session_result_t *results, const uint16_t *route,
                       const rhp_reply_table_t *table, const rhp_reply_out_t *o, void *stream);

/*
 * The wide slots of a round in one contiguous area: after rhp_parse_batch,
 * rhp_fixup_sessions and rhp_pack_dense, everything the host still needs about
 * the slots the dense copies (dreq, hc, lens16) cannot hold -- their
 * request-major records and the chunked bodies the fix-up de-framed -- is left
 * in three small areas, so that one D2H copy of their used parts (with the
 * dense copies) carries the whole round and nothing is fetched afterwards.
 *   batch: the RHP_MODE_HTTP, RHP_LAYOUT_REQUEST_MAJOR, RHP_BATCH_SPECULATIVE
 *   batch as the parse, the fix-up and rhp_pack_dense left it on `stream`;
 *   sessions, results, req_start: the fix-up's arguments; dreq, hc: the pack's
 *   outputs.  All device memory.
 *   In use.  Slot i is in use exactly as rhp_classify_sessions defines it: some
 *   session has piece_lo <= i < piece_lo + n_slots; a session whose fields do
 *   not satisfy piece_lo <= piece_lo + n_slots <= piece_hi <= n owns nothing.
 *   Wide.  An in-use slot is wide when hc[i].flags & RHP_HTTP_WIDE, or
 *   hc[i].result == 1 && (dreq[i].flags & RHP_DENSE_WIDE).  A slot that is not
 *   in use often carries a wide mark from a stale speculative record: it is
 *   never gathered, and nothing of it but hc[i] and dreq[i] is read.
 *   A wide slot's record (rhp_wide_slot_t, 64 B) holds reqs[i], http[i] and
 *   req_start[i] as the batch holds them.
 *   Headers.  n_hdrs(i) is req.num_headers when http.result == 1 && req.ret > 0
 *   && req.num_headers <= max_headers, else 0; the slot's header records
 *   batch->hdrs[i * max_headers + k], k < n_hdrs(i), are hdrs[hdr_first + k].
 *   Body.  A wide slot has a body to gather when http.result == 1, body_kind ==
 *   1, consumed != ret + body_len (mod 2^64, ret sign-extended: a chunked body
 *   was de-framed in place) and, with a = req_start + ret (mod 2^64), the range
 *   [a, a + body_len) lies inside its session's input:
 *   offsets[piece_lo] <= a <= offsets[piece_hi] and body_len <=
 *   offsets[piece_hi] - a.  Its bytes (read through bytes_rw when it is set) are
 *   body[body_off, body_off + http.body_len).  Any other wide slot has body_off
 *   == RHP_WIDE_NO_BODY and adds nothing to body_bytes.
 *   Order.  Wide slots appear in ascending slot index; hdr_first and body_off
 *   are the exclusive prefix sums of n_hdrs and of the gathered body lengths in
 *   that order.
 *   Totals.  *totals is always written and exact.  When n_wide > cap_slots,
 *   n_hdrs > cap_hdrs or body_bytes > cap_body nothing is written to any of the
 *   three areas (grow and call again, as rhp_write_responses and
 *   rhp_reply_sessions).  n_sessions == 0 or n == 0: zero totals, nothing else.
 * Contract: `sessions` ascends by piece_lo with disjoint ranges, as for
 * rhp_classify_sessions.  With that order violated the answers are unspecified;
 * still nothing is read outside the arguments' buffers and nothing is written
 * outside totals, work, slots[0, cap_slots), hdrs[0, cap_hdrs) and
 * body[0, cap_body).
 * -EINVAL: whatever rhp_pack_dense or rhp_classify_sessions refuses about the
 * batch, sessions and results (so any layout but RHP_LAYOUT_REQUEST_MAJOR; a
 * NULL req_start with sessions); a NULL dreq, hc, o, totals or work; a NULL
 * area with a non-zero cap; slots not 16-byte or hdrs not 8-byte aligned (the
 * records leave as whole 16- and 8-byte stores; body: any alignment).
 * Launch contract as rhp_reply_sessions: asynchronous on `stream`, no
 * allocation, no host synchronisation, no copy; thread-safe.  Three launches
 * (a wave's sums per 64 slots, one workgroup's scan of them with *totals, the
 * offsets and the copy); one when n == 0 or n_sessions == 0.
 */
typedef struct rhp_wide_slot {   /* 64 B, no padding: one sector per wide slot */
  uint32_t   slot;               /* record slot index i */
  uint32_t   hdr_first;          /* its header records: hdrs[hdr_first .. + n_hdrs(i)) */
  rhp_req_t  req;                /* reqs[i] */
  rhp_http_t http;               /* http[i] */
  uint64_t   req_start;          /* req_start[i] */
  uint64_t   body_off;           /* body[body_off .. + http.body_len), or RHP_WIDE_NO_BODY */
} rhp_wide_slot_t;
#define RHP_WIDE_NO_BODY (~(uint64_t) 0)

typedef struct rhp_wide_totals {   /* 16 B */
  uint32_t n_wide, n_hdrs;
  uint64_t body_bytes;
} rhp_wide_totals_t;

typedef struct rhp_wide_out {
  rhp_wide_totals_t *totals;     /* device [1] */
  rhp_wide_slot_t   *slots;      /* device [cap_slots], 16-byte aligned */
  uint32_t           cap_slots;
  rhp_hdr_t         *hdrs;       /* device [cap_hdrs], 8-byte aligned */
  uint32_t           cap_hdrs;
  uint8_t           *body;       /* device, cap_body bytes, any alignment */
  uint64_t           cap_body;
  uint64_t          *work;       /* device scratch, >= RHP_WIDE_WORK_WORDS(n) u64 */
} rhp_wide_out_t;

/* per 64 slots: three sums and two masks (wide, with a body) */
#define RHP_WIDE_WORK_WORDS(n) (5u * (((uint64_t) (n) + 63u) / 64u) + 1u)

int rhp_gather_wide(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                    const rhp_session_result_t *results, const uint64_t *req_start,
                    const rhp_req_dense_t *dreq, const rhp_http_compact_t *hc,
                    const rhp_wide_out_t *o, void *stream);

/*
 * The split in front of the parse, on the device: the packed input of a
 * round's sessions cut at every empty line into the pieces of a
 * RHP_BATCH_SPECULATIVE batch (offsets[]) and the sessions' piece ranges
 * (rhp_session_t[]), as rhp_fixup_sessions documents the split above.
 *   Session s is bytes[sess_off[s], sess_off[s+1]), a = sess_off[s], e =
 *   sess_off[s+1]: the sessions lie back to back.  sess_off (device
 *   [n_sessions + 1]) is non-decreasing, sess_off[0] may be non-zero and
 *   sess_off[n_sessions] <= bytes_end; bytes_end is the host's copy of the packed
 *   length and sizes the launch.
 *   Cut.  An absolute position p, a < p < e, is a cut when bytes[p-1] == LF and
 *   either p-2 >= a && bytes[p-2] == LF, or p-3 >= a && bytes[p-2] == CR &&
 *   bytes[p-3] == LF: the look-back never crosses the session's start.  p == a and
 *   p == e are never cuts (an empty line that ends the input makes no empty
 *   piece); overlapping empty lines each cut (LF LF LF x: at 2 and at 3).
 *   Pieces.  Session s has 1 + cuts(s) pieces, an empty session one empty piece:
 *   *n_pieces = n_sessions + the cuts of all sessions.  sessions[s].piece_lo = s +
 *   (the cuts at positions < a), piece_hi = piece_lo + 1 + cuts(s);
 *   offsets[piece_lo(s)] = a; the j-th cut over all sessions (ascending position,
 *   from 0), lying in session s, is offsets[s + j + 1]; offsets[k] =
 *   sess_off[n_sessions] for n_pieces <= k <= cap_pieces.
 *   The tail fill lets the caller go on without a host step: rhp_parse_batch
 *   with n = cap_pieces and RHP_BATCH_SPECULATIVE over these offsets (the
 *   trailing pieces are empty, no session owns them, and every *_sessions call
 *   treats such slots as not in use).
 *   Overflow.  When *n_pieces > cap_pieces nothing is written to offsets or
 *   sessions; *n_pieces is always written and exact (grow and call again, as
 *   rhp_write_responses and rhp_gather_wide).  A caller who launches the parse
 *   without reading *n_pieces first either holds cap_pieces >= n_sessions +
 *   sess_off[n_sessions] - sess_off[0] (no input has more pieces) or zeroes
 *   offsets and sessions before the call (every piece empty, no session owns one).
 *   n_sessions == 0: *n_pieces = 0, offsets[0 .. cap_pieces] = sess_off[0].
 * Memory.  `bytes` is 16-byte aligned (as rhp_batch_t.bytes) and is read only as
 * the aligned 16-byte groups that hold [sess_off[0], sess_off[n_sessions]).  With
 * sess_off not monotone the answers are unspecified; still nothing is read
 * outside bytes[0, bytes_end) rounded out to 16 bytes and sess_off, and nothing
 * is written outside n_pieces, work, offsets[0, cap_pieces] and
 * sessions[0, n_sessions).
 * -EINVAL: a NULL sess_off, o, n_pieces, offsets or work; a NULL sessions with
 * n_sessions > 0; a NULL or misaligned bytes with bytes_end > 0; bytes_end +
 * n_sessions >= 2^32.
 * Launch contract as rhp_gather_wide: asynchronous on `stream`, no allocation,
 * no copy, no host synchronisation; thread-safe.  Three launches (a wave's cut
 * masks and count per RHP_SPLIT_STEP_BYTES of input, one workgroup's scan of the
 * counts with *n_pieces, the offsets and sessions with the tail fill); two when
 * bytes_end == 0.
 */
#define RHP_SPLIT_STEP_BYTES 1024u   /* what one wave marks: 64 lanes x 16 bytes */

typedef struct rhp_split_out {
  uint64_t      *n_pieces;   /* device [1]: always written, exact */
  uint64_t      *offsets;    /* device [cap_pieces + 1] */
  uint32_t       cap_pieces;
  rhp_session_t *sessions;   /* device [n_sessions] */
  uint64_t      *work;       /* device scratch, >= RHP_SPLIT_WORK_WORDS(bytes_end, n_sessions) u64 */
} rhp_split_out_t;

/* per step: 16 cut masks (a u64 per 64 bytes), 16 u32 counts of the cuts before each mask inside its step, the
 * step's count; one word for the total */
#define RHP_SPLIT_WORK_WORDS(bytes_end, n_sessions) \
  (25u * (((uint64_t) (bytes_end) + RHP_SPLIT_STEP_BYTES - 1u) / RHP_SPLIT_STEP_BYTES) + 1u + 0u * (uint64_t) (n_sessions))

int rhp_split_sessions(const uint8_t *bytes, uint64_t bytes_end,
                       const uint64_t *sess_off /* device [n_sessions + 1] */, uint32_t n_sessions,
                       const rhp_split_out_t *o, void *stream);

/*
 * The parser's other two entry points, batched: for n messages already in HBM,
 *   int phr_parse_response(const char *buf, size_t len, int *minor_version, int *status,
 *       const char **msg, size_t *msg_len, struct phr_header *headers, size_t *num_headers,
 *       size_t last_len);
 *   int phr_parse_headers(const char *buf, size_t len, struct phr_header *headers,
 *       size_t *num_headers, size_t last_len);
 *                       /root/reference/src/picohttpparser/picohttpparser.h:55-59
 *                       (picohttpparser.c:411-478, 480-499)
 * what a proxy's upstream side, a load generator or a capture analyser holds:
 * status lines with their headers, or bare header blocks (trailers, multipart
 * parts).  Message i is bytes[offsets[i], offsets[i+1]); as in rhp_batch_t the
 * bytes after it (the next message, RHP_PAD zero bytes after the last) are
 * what the reference would read past the end, and every pointer it returns is
 * returned as an offset from the message start.
 *   RHP_MSG_RESPONSE.  No leading CRLF is skipped.  "HTTP/1." and a digit
 *   (fewer than 9 bytes: -2), one SP, then further SPs skipped with no end test
 *   (the skip may run into the bytes after the message), fewer than 4 bytes
 *   left: -2, three digits, the reason phrase up to CRLF or LF (a control byte
 *   other than HT, or DEL: -1).  A phrase that is not empty starts with SP and
 *   loses all its leading SPs; msg_off / msg_len are what is left (an empty
 *   phrase: msg_off at the line end, msg_len 0).  Then the header lines.
 *   RHP_MSG_HEADERS.  The header lines from byte 0.
 *   Both.  last_len[i] != 0 runs is_complete first, as rhp_batch_t.last_len
 *   says.  The header lines are those of a request: an obs-fold line gives
 *   RHP_NAME_NULL and cannot be the first line, trailing OWS is trimmed, a
 *   line beyond max_headers gives -1.  A header section longer than
 *   RHP_MAX_LEN gives RHP_RET_TOOLONG and no other output (the caller parses it
 *   with rhp_phr_parse_response / rhp_phr_parse_headers, rhp_host.h).  Records
 *   past num_headers are unspecified.
 * Memory.  No byte at or beyond bytes + bytes_size is read, whatever offsets
 * holds (there the reader sees zeros); nothing is written outside msgs[0, n)
 * and hdrs[0, n * max_headers).  A message record leaves as one 16-byte store
 * (msgs is 16-byte aligned), a header record as one 8-byte store.
 * -EINVAL: a NULL batch; a kind or layout other than those named; max_headers
 * above RHP_MAX_HEADERS; n * max_headers >= 2^32; with n > 0: a NULL bytes,
 * offsets or msgs, a NULL hdrs with max_headers > 0, bytes_size below RHP_PAD,
 * bytes or msgs not 16-byte aligned, hdrs not 8-byte aligned (the alignments:
 * device pointers only).  n == 0 succeeds and launches nothing.
 * Launch contract as rhp_parse_batch: asynchronous on `stream`, no allocation,
 * no copy, no host synchronisation; thread-safe.  One launch, one message per
 * lane.
 */
enum rhp_msg_kind { RHP_MSG_RESPONSE = 0,   /* phr_parse_response, picohttpparser.c:411-478 */
                    RHP_MSG_HEADERS  = 1 }; /* phr_parse_headers,  picohttpparser.c:480-499 */

typedef struct rhp_msg {          /* 16 B; for ret <= 0 only ret is meaningful */
  int32_t  ret;                   /* >0 bytes consumed, -1, -2, RHP_RET_TOOLONG (ret > RHP_MAX_LEN) */
  uint16_t status;                /* RESPONSE: 100 * d0 + 10 * d1 + d2; HEADERS: 0 */
  uint16_t msg_off, msg_len;      /* RESPONSE: reason phrase after its leading spaces; HEADERS: 0, 0 */
  int8_t   minor_version;         /* RESPONSE; HEADERS: -1 */
  uint8_t  reserved;              /* written 0 */
  uint16_t num_headers;
  uint16_t flags;                 /* written 0 */
} rhp_msg_t;

typedef struct rhp_msg_batch {
  const uint8_t  *bytes;          /* as rhp_batch_t.bytes: 16-byte aligned, RHP_PAD zero bytes after the last message */
  const uint64_t *offsets;        /* device [n + 1], non-decreasing */
  uint64_t        bytes_size;
  uint32_t        n, max_headers; /* max_headers <= RHP_MAX_HEADERS, 0 allowed */
  uint32_t        kind;           /* enum rhp_msg_kind */
  uint32_t        layout;         /* RHP_LAYOUT_REQUEST_MAJOR or RHP_LAYOUT_HEADER_MAJOR; any other: -EINVAL */
  rhp_msg_t      *msgs;           /* device [n] */
  rhp_hdr_t      *hdrs;           /* device [n * max_headers], RHP_HDR() indexing; may be NULL when max_headers == 0 */
  const uint64_t *last_len;       /* device [n] or NULL (= all 0); contract last_len[i] <= len, as rhp_batch_t */
} rhp_msg_batch_t;

int rhp_parse_messages(const rhp_msg_batch_t *batch, void *stream);

/*
 * The parser's fourth entry point, batched: for n streams whose newly arrived
 * bytes lie in HBM,
 *   ssize_t phr_decode_chunked(struct phr_chunked_decoder *decoder, char *buf, size_t *bufsz);
 *                       /root/reference/src/picohttpparser/picohttpparser.h:62-81
 *                       (picohttpparser.c:523-636)
 * the resumable de-framer of a chunked body: a caller who parsed a response's
 * headers (rhp_parse_messages) feeds it whatever arrived of the body, call
 * after call.  Stream i's piece is bytes[offsets[i], offsets[i+1]) (`buf`, its
 * length `*bufsz` on entry) and decoders[i] its struct phr_chunked_decoder,
 * zero-filled (but for consume_trailer) before the stream's first call and
 * carried from call to call as it is left.  The call leaves what the
 * reference leaves, value for value: results[i].ret, results[i].size (*bufsz
 * on return, written on every exit), the decoder's three fields on every exit,
 * and every byte of the piece: the decoded bytes in [0, size); right behind
 * them the bytes the reference's closing memmove (:632-633) carries down (the
 * `ret` bytes that follow the body's end; on -1 the bytes from the offending
 * one on); every byte beyond those keeps its value.
 *   The state machine.  A piece is walked from the decoder's state on; when
 *   the piece ends inside a state the answer is -2 and the state is kept.
 *   RHP_CHUNKED_IN_CHUNK_SIZE   hex digits (0-9, A-F, a-f; leading zeros count)
 *                       shift into bytes_left_in_chunk, hex_count counts them
 *                       across calls: 16 at most, a 17th gives -1; the first
 *                       other byte ends them (hex_count back to 0) and is -1
 *                       when no digit came before it.
 *   RHP_CHUNKED_IN_CHUNK_EXT    the rest of the size line is skipped up to its
 *                       LF with no look at its bytes (a bare LF ends a size
 *                       line).  Then bytes_left_in_chunk != 0: the data; == 0
 *                       (the last chunk): with consume_trailer the trailer
 *                       lines, without it the body ends at this LF.
 *   RHP_CHUNKED_IN_CHUNK_DATA   min(bytes_left_in_chunk, what the piece holds)
 *                       bytes move down behind the decoded ones and are
 *                       counted off; the data is not looked at.
 *   RHP_CHUNKED_IN_CHUNK_CRLF   any run of CRs, then the LF: the next size line;
 *                       any other byte gives -1.
 *   RHP_CHUNKED_IN_TRAILERS_LINE_HEAD   any run of CRs; then an LF ends the body
 *                       (the empty line; an empty trailer section is just it);
 *                       any other byte starts a line,
 *   RHP_CHUNKED_IN_TRAILERS_LINE_MIDDLE   which is skipped up to its LF.
 *   The body's end leaves the state as it is then (IN_CHUNK_EXT or
 *   IN_TRAILERS_LINE_HEAD).  An empty piece gives -2 and changes nothing.
 * Corrupt decoder.  state > 5 (the reference asserts) or hex_count > 16 (the
 * reference cannot leave it): ret = -1, size = 0, the piece and the decoder
 * untouched.
 * Memory.  A piece's start and end are clamped to bytes_size (and the end to
 * at least the start) whatever offsets holds.  Only a piece's own bytes are
 * looked at: no pad is asked for.  They are loaded as bytes or as the aligned
 * dwords that hold them (inside the aligned 16-byte lines that hold the piece;
 * so with bytes_size a multiple of 4 no byte at or beyond bytes + bytes_size
 * is read).  Stores go to the piece's own bytes only -- a byte of a
 * neighbouring piece, which belongs to another wave, is not even rewritten
 * with its own value.  decoders[i] and results[i] are each read and written
 * as one 16-byte access.
 * -EINVAL (rhp_chunked_args.h): a NULL batch; reserved != 0; with n > 0 a NULL
 * bytes, offsets, decoders or results; bytes, decoders or results not 16-byte
 * aligned (device pointers only).  n == 0 succeeds and launches nothing.
 * Launch contract as rhp_parse_messages: asynchronous on `stream`, one launch,
 * no allocation, no copy, no host synchronisation; thread-safe.  One wave per
 * stream.
 */
enum { RHP_CHUNKED_IN_CHUNK_SIZE, RHP_CHUNKED_IN_CHUNK_EXT, RHP_CHUNKED_IN_CHUNK_DATA,
       RHP_CHUNKED_IN_CHUNK_CRLF, RHP_CHUNKED_IN_TRAILERS_LINE_HEAD,
       RHP_CHUNKED_IN_TRAILERS_LINE_MIDDLE };     /* picohttpparser.c:501-508, same values */

typedef struct rhp_chunked {            /* 16 B: struct phr_chunked_decoder; zero-filled before a stream's first call */
  uint64_t bytes_left_in_chunk;
  uint8_t  consume_trailer;             /* the caller's; never written */
  uint8_t  hex_count;                   /* _hex_count */
  uint8_t  state;                       /* _state, RHP_CHUNKED_IN_* */
  uint8_t  reserved[5];                 /* kept as they are */
} rhp_chunked_t;

typedef struct rhp_chunked_result {     /* 16 B */
  int64_t  ret;    /* >= 0: end of the body found, `ret` undecoded bytes follow the decoded ones; -1 error; -2 incomplete */
  uint64_t size;   /* *bufsz on return: decoded bytes at the piece's start */
} rhp_chunked_result_t;

typedef struct rhp_chunked_batch {
  uint8_t              *bytes;       /* device, 16-byte aligned, read and written */
  const uint64_t       *offsets;     /* device [n + 1]: stream i's new input is bytes[offsets[i], offsets[i+1]) */
  uint64_t              bytes_size;
  uint32_t              n, reserved; /* reserved must be 0 */
  rhp_chunked_t        *decoders;    /* device [n], 16-byte aligned, read and written */
  rhp_chunked_result_t *results;     /* device [n], 16-byte aligned */
} rhp_chunked_batch_t;

int rhp_decode_chunked(const rhp_chunked_batch_t *batch, void *stream);

/*
 * Between the two calls above: how the body of every message
 * rhp_parse_messages parsed is framed, with the header lookup of
 * rhp_classify_batch over the same records, in one launch.  The framing is the
 * reference's rule for a request that is not a GET,
 *   http_read_request   src/reactor/http.c:204-233
 * applied to the message's header records:
 *   encoding = http_field_lookup(fields, count, "Transfer-Encoding");
 *   length   = http_field_lookup(fields, count, "Content-Length");
 * `batch` is the batch as rhp_parse_messages left it on `stream`, either kind
 * and either layout; last_len is not looked at.  For message i:
 *   Not ready.  msgs[i].ret <= 0 gives result = -1 for ret == -1,
 *   RHP_RET_TOOLONG for RHP_RET_TOOLONG and 0 for anything else (http.c:194-195),
 *   body_kind RHP_FRAME_NONE, body_len 0 and every field absent; of such a
 *   message nothing but msgs[i].ret is read.  A message whose bytes do not lie
 *   inside the batch's -- offsets[i] + ret above bytes_size rounded down to a
 *   multiple of 4; a batch that keeps its RHP_PAD has none -- counts as not
 *   ready too: result 0.
 *   Lookup.  te and cl are the values of the first record k <
 *   min(num_headers, max_headers) whose name is not NULL (an obs-fold line) and
 *   is string_equal_case to Transfer-Encoding and to Content-Length (as
 *   rhp_classify_batch compares: equal lengths, a..z mapped to A..Z, no other
 *   byte).  Only the first match counts: a first match with an empty value
 *   makes the header absent, even when a later duplicate has a value.
 *   cl not empty and te not empty: result -1.
 *   cl not empty alone: RHP_FRAME_LENGTH, body_len = strtoull(cl, NULL, 10) as
 *   glibc's C locale gives it: a sign is accepted and '-' negates mod 2^64, no
 *   digit gives 0, overflow saturates to 2^64 - 1.  result is 1 whether or not
 *   the body has arrived: the caller's completeness test is the reference's own,
 *   len < ret + body_len in size_t arithmetic, i.e. mod 2^64 (http.c:213).
 *   Otherwise te not empty: it must be `chunked` (7 bytes, a..z mapped to A..Z:
 *   data_equal_case, http.c:223), else result -1; then RHP_FRAME_CHUNKED.
 *   Otherwise RHP_FRAME_NONE.  What that means for a response -- a status that
 *   has no body, or a body that runs until the connection closes -- is the
 *   caller's decision from msgs[i].status: the reference has no rule for it
 *   and this call invents none.
 *   Decoders.  With decoders != NULL, decoders[i] of an RHP_FRAME_CHUNKED
 *   message is written with one 16-byte store: all zero but consume_trailer,
 *   what rhp_decode_chunked wants to find when the body starts.  Every other
 *   message's decoder is not touched, not even rewritten with its own value.
 *   Fields.  fields[j * n + i] is what rhp_classify_batch documents for name j,
 *   offsets from the message's start; {RHP_NAME_NULL, 0} for a missing header
 *   and for a message that is not ready.
 * Memory.  No byte at or beyond bytes + bytes_size is read, whatever offsets or
 * the records hold: every offset that becomes an address is checked against
 * the message's own ret first, and a record whose name -- for the two framing
 * names also its value -- does not lie inside [0, ret) matches nothing (no
 * parsed record is like that).  Records of a message that is not ready and
 * records k >= num_headers are never read.  Name and value bytes are read as
 * the aligned dwords that hold them, and only those of records whose name_len
 * is a name's.  Nothing is written outside frames[0, n), fields[0, n_names * n)
 * and the armed decoders; a frame leaves as one 16-byte store.
 * -EINVAL (rhp_frame_args.h): a NULL batch or f; whatever rhp_parse_messages
 * refuses about the batch (last_len apart); n_names above
 * RHP_CLASSIFY_MAX_NAMES; an empty name or one longer than
 * RHP_CLASSIFY_NAME_MAX; n_names > 0 with a NULL text, names or fields; with
 * n > 0 a NULL frames, frames or decoders not 16-byte aligned (device pointers
 * only); consume_trailer > 1; reserved != 0.  n == 0 succeeds and launches
 * nothing.
 * Launch contract as rhp_classify_batch: one launch, asynchronous on `stream`,
 * no allocation, no copy, no synchronisation; the names travel in the kernel
 * argument and the caller's tables are free when the call returns;
 * thread-safe.  One message per lane.
 */
enum { RHP_FRAME_NONE = 0, RHP_FRAME_LENGTH = 1, RHP_FRAME_CHUNKED = 2 };

typedef struct rhp_frame {        /* 16 B, leaves as one 16-byte store */
  int32_t  result;                /* 1 framing decided; 0 the message is not there yet; -1 malformed; RHP_RET_TOOLONG */
  uint32_t body_kind;             /* RHP_FRAME_* ; NONE unless result == 1 */
  uint64_t body_len;              /* LENGTH: strtoull of the value, as u64; otherwise 0 */
} rhp_frame_t;

typedef struct rhp_frame_args {
  const uint8_t    *text;         /* host: the bytes of the lookup names (as rhp_classify_t) */
  const rhp_span_t *names;        /* host [n_names] */
  uint32_t          n_names;      /* 0 .. RHP_CLASSIFY_MAX_NAMES; 0: framing only */
  uint32_t          consume_trailer; /* 0 or 1: what an armed decoder gets */
  rhp_fieldref_t   *fields;       /* device [n_names * n], name-major, as rhp_classify_t.fields */
  rhp_frame_t      *frames;       /* device [n], 16-byte aligned */
  rhp_chunked_t    *decoders;     /* device [n], 16-byte aligned, or NULL */
  uint64_t          reserved;     /* must be 0 */
} rhp_frame_args_t;

int rhp_frame_messages(const rhp_msg_batch_t *batch, const rhp_frame_args_t *f, void *stream);

/*
 * The three calls above as one loop per connection: the pipelined responses of
 * n_sessions keep-alive upstream connections walked on the device.  The next
 * response of a connection starts at start + ret + the body's length on the
 * wire, known only when the one before it has been parsed and framed; the walk
 * is that loop, sequential inside a session and parallel across sessions.
 *   Session s is bytes[sess_off[s], sess_off[s+1]), a = sess_off[s], e =
 *   sess_off[s+1]: the sessions lie back to back as for rhp_split_sessions,
 *   sess_off is non-decreasing and RHP_PAD zero bytes follow the last session.
 *   It owns the record slots [slot_off[s], slot_off[s+1]), slot_off
 *   non-decreasing, slot_off[n_sessions] == n_slots_total.
 *   The walk.  pos = a, slot = slot_off[s]; while pos < e:
 *     no slot left: stop = RHP_WALK_MORE.
 *     Parse.  RHP_MSG_RESPONSE of rhp_parse_messages for the message [pos, e)
 *     with last_len 0 -- phr_parse_response(bytes + pos, e - pos, ...), with what
 *     it reads past e (the next session's bytes, then the pad) -- into msgs[slot]
 *     and hdrs[slot * max_headers + k]; slots[slot].start = pos.
 *     ret == -2: result 0, stop = RHP_WALK_HEAD.  ret == -1: result -1, stop =
 *     RHP_WALK_BAD.  RHP_RET_TOOLONG: result RHP_RET_TOOLONG, stop = RHP_WALK_BAD.
 *     Framing.  rhp_frame_messages' rule over the records just written (first
 *     match only, an empty value is absent, strtoull, `chunked`); its -1 gives
 *     result -1, stop = RHP_WALK_BAD.
 *     Body, with avail = e - (pos + ret):
 *       A status of 100..199, 204 or 304 has no body whatever its headers say
 *       (RFC 9112 section 6.3): body_kind stays what the framing said, body_len =
 *       wire_len = 0.  THE REFERENCE HAS NO RULE HERE: this is the one rule of
 *       the walk that is invented, not taken from it.
 *       RHP_FRAME_LENGTH: body_len is the framing's value; body_len > avail
 *       (compared as u64, nothing is added): wire_len = avail, stop =
 *       RHP_WALK_BODY; otherwise wire_len = body_len.
 *       RHP_FRAME_CHUNKED: phr_decode_chunked from a zero decoder, consume_trailer
 *       = (flags & RHP_WALK_TRAILERS) != 0, over [pos + ret, e), no byte moved.
 *       Its ret >= 0: body_len = *bufsz, wire_len = avail - ret.  -2: body_len =
 *       *bufsz so far, wire_len = avail, stop = RHP_WALK_BODY.  -1: result -1,
 *       stop = RHP_WALK_BAD.  With RHP_WALK_DEFRAME a body whose decode completed
 *       is then de-framed in place: [pos + ret, pos + ret + wire_len) is left as
 *       rhp_decode_chunked leaves that piece (body_len decoded bytes first).  A
 *       partial or bad body is never touched.
 *       RHP_FRAME_NONE on any other status: the body runs until the connection
 *       closes: wire_len = avail, body_len = 0, stop = RHP_WALK_CLOSE.  With
 *       RHP_WALK_NONE_EMPTY it is an empty body instead and the walk goes on.
 *     A slot that stops the walk with HEAD or BAD has body_kind RHP_FRAME_NONE
 *     and both lengths 0.  Every other slot has result 1; one that did not stop
 *     the walk advances it: pos += ret + wire_len.  slot++.
 *   The loop left with pos == e: stop = RHP_WALK_END.
 *   results[s]: n_slots counts every written slot, the stopping one included;
 *   consumed = pos - a counts complete messages only (the bytes of a BODY or
 *   CLOSE slot are not in it).  An empty session: n_slots 0, RHP_WALK_END.
 *   Slots at and past slot_off[s] + n_slots are not written, not even with
 *   their own value.  A session whose slot_off pair is not ordered or reaches
 *   beyond n_slots_total owns no slot: n_slots 0, RHP_WALK_MORE unless empty.
 * Memory.  No byte at or beyond bytes + bytes_size is read, whatever sess_off
 * holds: a session's ends are clamped to the readable end, bytes_size rounded
 * down to whole 16-byte lines less one line (the de-framing move may load the
 * line behind its last source byte); with RHP_PAD kept no session reaches it.
 * The reader sees zeros from there on.  With sess_off not monotone or beyond
 * bytes_size the answers are unspecified.  Stores: msgs, hdrs and slots of the
 * written slots, results[0, n_sessions) and, with RHP_WALK_DEFRAME, bytes
 * inside the wire span of a completed chunked body -- nothing else.  A message
 * record and a result leave as one 16-byte store, a slot as two, a header
 * record as one 8-byte store.
 * Not here: responses to HEAD requests (their framing headers describe a body
 * that is not sent; the answer is in the request, and rhp_walk_answers, below,
 * is this walk told which requests were HEAD); resuming a partial
 * chunked body across rounds (rhp_walk_resume, below, carries the walk from
 * round to round).  The header lookup over the walked slots is
 * rhp_lookup_walked, below (rhp_frame_messages addresses messages by
 * offsets[i], not by slots[i].start).
 * -EINVAL (rhp_walk_args.h): a NULL w; max_headers above RHP_MAX_HEADERS; a
 * flag bit that is not named here; n_slots_total * max_headers >= 2^32;
 * RHP_WALK_DEFRAME with a bytes_rw that is NULL or not `bytes`; with
 * n_sessions > 0: a NULL bytes, sess_off, slot_off or results; a NULL msgs or
 * slots with n_slots_total > 0; a NULL hdrs with n_slots_total > 0 and
 * max_headers > 0; bytes_size below RHP_PAD; bytes, msgs, slots or results not
 * 16-byte aligned, hdrs not 8-byte aligned (the alignments: device pointers
 * only).  n_sessions == 0 succeeds and launches nothing.
 * Launch contract as rhp_parse_messages: one launch, asynchronous on `stream`,
 * no allocation, no copy, no synchronisation; thread-safe.  One session per
 * lane.
 */
enum rhp_walk_stop { RHP_WALK_END = 0,    /* the session's bytes are used up */
                     RHP_WALK_HEAD,       /* the last slot's head is not complete (ret -2) */
                     RHP_WALK_BAD,        /* the last slot is malformed (head, framing or chunk) or too long */
                     RHP_WALK_BODY,       /* the last slot's body has not arrived in full */
                     RHP_WALK_CLOSE,      /* the last slot's body runs until the connection closes */
                     RHP_WALK_MORE };     /* the session's slots ran out with bytes left */

#define RHP_WALK_TRAILERS   1u   /* chunked bodies: consume_trailer = 1 */
#define RHP_WALK_DEFRAME    2u   /* de-frame completed chunked bodies in place (bytes_rw) */
#define RHP_WALK_NONE_EMPTY 4u   /* RHP_FRAME_NONE on a status with a body: an empty body, the walk goes on */

typedef struct rhp_walk_slot {    /* 32 B, leaves as two 16-byte stores */
  uint64_t start;                 /* the message starts at bytes[start] */
  uint64_t body_len;              /* LENGTH: the header's value; CHUNKED: decoded bytes (so far); else 0 */
  uint64_t wire_len;              /* body bytes of this session's input: [start + ret, start + ret + wire_len) */
  int32_t  result;                /* 1; 0 head incomplete; -1 malformed; RHP_RET_TOOLONG */
  uint32_t body_kind;             /* RHP_FRAME_* */
} rhp_walk_slot_t;

typedef struct rhp_walk_result {  /* 16 B, leaves as one 16-byte store */
  uint32_t n_slots;               /* slots written, the stopping one included */
  uint32_t stop;                  /* enum rhp_walk_stop */
  uint64_t consumed;              /* bytes of the complete messages, from the session's start */
} rhp_walk_result_t;

typedef struct rhp_walk_batch {
  const uint8_t     *bytes;         /* device, 16-byte aligned */
  uint8_t           *bytes_rw;      /* == bytes, writable: RHP_WALK_DEFRAME; otherwise may be NULL */
  uint64_t           bytes_size;
  const uint64_t    *sess_off;      /* device [n_sessions + 1] */
  const uint64_t    *slot_off;      /* device [n_sessions + 1] */
  uint32_t           n_sessions;
  uint32_t           n_slots_total; /* host copy of slot_off[n_sessions] */
  uint32_t           max_headers;   /* <= RHP_MAX_HEADERS, 0 allowed */
  uint32_t           flags;         /* RHP_WALK_* */
  rhp_msg_t         *msgs;          /* device [n_slots_total], 16-byte aligned */
  rhp_hdr_t         *hdrs;          /* device [n_slots_total * max_headers], request-major; may be NULL when max_headers == 0 */
  rhp_walk_slot_t   *slots;         /* device [n_slots_total], 16-byte aligned */
  rhp_walk_result_t *results;       /* device [n_sessions], 16-byte aligned */
} rhp_walk_batch_t;

int rhp_walk_responses(const rhp_walk_batch_t *w, void *stream);

/*
 * The walk above carried across rounds.  An upstream connection does not
 * deliver whole responses per round: a round ends inside a Content-Length body,
 * inside a chunk, inside a size line, inside a head.  states[s], 32 bytes that
 * stay in HBM, say where session s stands between rounds: read at entry,
 * written at exit, all zero before the connection's first round.  The batch,
 * the flags, the clamps and the memory contract are rhp_walk_responses'.
 *   A round's input.  Session s's bytes [a, e) of a round are the bytes the
 *   round before left unconsumed, [a + consumed, e) of that round, with the
 *   newly arrived bytes behind them.  The unconsumed bytes are not empty only
 *   after RHP_WALK_HEAD (the incomplete head) and RHP_WALK_MORE.
 *   On an all-zero state the call is rhp_walk_responses but for two things,
 *   both because the bytes of a body that has started are taken:
 *     1. a slot that stops with RHP_WALK_BODY or RHP_WALK_CLOSE sets pos = e, so
 *        consumed = e - a counts the head and the body bytes that are there, and
 *        the state is armed (below): the next round starts inside the body;
 *     2. with RHP_WALK_DEFRAME a partial chunked body (the RHP_WALK_BODY slot)
 *        is de-framed too: [body, body + wire_len) is left as rhp_decode_chunked
 *        leaves that piece from that decoder -- body_len decoded bytes first,
 *        behind them every byte keeps its value.
 *   One round of session s:
 *   1. Corrupt or dead state: phase >= RHP_WALK_DEAD, reserved != 0, or
 *      RHP_WALK_IN_CHUNKED with decoder.state > 5 or decoder.hex_count > 16:
 *      n_slots 0, stop RHP_WALK_BAD, consumed 0; the state keeps its value, no
 *      byte is read or written.
 *   2. Empty round, a == e: n_slots 0, consumed 0, the state is kept; stop is
 *      RHP_WALK_END at AT_HEAD, RHP_WALK_BODY at IN_LENGTH and IN_CHUNKED,
 *      RHP_WALK_CLOSE at IN_CLOSE.
 *   3. Continuation, an IN_* phase and a < e.  With no slot left: RHP_WALK_MORE,
 *      consumed 0, the state is kept, nothing is touched.  Otherwise the
 *      session's first slot is a continuation slot: start = a, result = 1,
 *      msgs[slot] sixteen zero bytes, no header record written.  (A slot with
 *      result == 1 and msgs[slot].ret == 0 is a continuation; a head slot with
 *      result == 1 has ret > 0.)
 *        IN_LENGTH: body_kind LENGTH, body_len = left at entry, wire_len =
 *        min(left, e - a), left -= wire_len; left != 0: stop RHP_WALK_BODY;
 *        otherwise the walk goes on at a + wire_len from AT_HEAD.
 *        IN_CHUNKED: phr_decode_chunked from states[s].decoder over [a, e), with
 *        the decoder's own consume_trailer; body_kind CHUNKED, body_len = *bufsz.
 *        ret >= 0: wire_len = (e - a) - ret, on from AT_HEAD.  -2: wire_len =
 *        e - a, stop RHP_WALK_BODY, the decoder saved as it was left.  -1:
 *        result -1, body_kind NONE, both lengths 0, stop RHP_WALK_BAD, no byte
 *        touched.  With RHP_WALK_DEFRAME [a, a + wire_len) is de-framed as in 2
 *        above, unless the answer is -1.
 *        IN_CLOSE: body_kind NONE, body_len 0, wire_len = e - a, stop
 *        RHP_WALK_CLOSE.
 *   4. Heads: rhp_walk_responses' loop from there, with the two differences.
 *      Arming: IN_LENGTH with left = body_len - avail; IN_CHUNKED with the
 *      decoder as the decode over [body, e) left it, started from a zero decoder
 *      with consume_trailer = (flags & RHP_WALK_TRAILERS) != 0 (a head that ends
 *      exactly at e: the zero decoder, wire_len 0); IN_CLOSE.
 *   5. The state at exit, written whole: phase AT_HEAD after RHP_WALK_END, HEAD
 *      and MORE; IN_LENGTH / IN_CHUNKED after RHP_WALK_BODY; IN_CLOSE after
 *      RHP_WALK_CLOSE; DEAD after RHP_WALK_BAD (consumed still counts the
 *      complete messages before it).  left is 0 unless IN_LENGTH, the decoder
 *      zero unless IN_CHUNKED, reserved 0.
 *   results[s].consumed counts, from a: the continuation's wire_len, every
 *   complete message, and the head and body bytes of a BODY or CLOSE slot.
 * Memory as rhp_walk_responses; in addition states[s] is loaded and stored as
 * two 16-byte accesses each, and with RHP_WALK_DEFRAME bytes inside the wire
 * span of a partial chunked body are written too.  A session's answers do not
 * depend on its neighbours' bytes, moved or not: the one read past e that can
 * reach them is the SP run behind the version, and a run that reaches e gives
 * -2 whatever lies beyond.
 * -EINVAL (rhp_walk_args.h): whatever rhp_walk_responses refuses; with
 * n_sessions > 0 a NULL states; states not 16-byte aligned (device pointers
 * only).  n_sessions == 0 succeeds and launches nothing.
 * Launch contract as rhp_walk_responses: one launch, one session per lane,
 * asynchronous on `stream`, no allocation, no copy, no synchronisation.
 */
enum rhp_walk_phase { RHP_WALK_AT_HEAD = 0,   /* the round's first byte starts a head */
                      RHP_WALK_IN_LENGTH,     /* inside a Content-Length body: `left` bytes still to come */
                      RHP_WALK_IN_CHUNKED,    /* inside a chunked body: `decoder` is where it stands */
                      RHP_WALK_IN_CLOSE,      /* inside a body that runs until the connection closes */
                      RHP_WALK_DEAD };        /* a round stopped with RHP_WALK_BAD */

typedef struct rhp_walk_state {   /* 32 B, two 16-byte accesses; all zero before a connection's first round */
  rhp_chunked_t decoder;          /* as rhp_decode_chunked carries it */
  uint64_t      left;
  uint32_t      phase;            /* enum rhp_walk_phase */
  uint32_t      reserved;         /* 0 */
} rhp_walk_state_t;

int rhp_walk_resume(const rhp_walk_batch_t *w, rhp_walk_state_t *states /* device [n_sessions], 16-byte aligned */, void *stream);

/*
 * The two walks above told what was asked.  A reply to a HEAD request carries
 * the framing headers of the GET's reply and no body; which reply that is
 * stands in the request, not in the response, and a proxy knows which of its
 * outstanding requests were HEAD.  The same queue says which request a slot
 * answers: the count of slots is not the count of answered requests, since an
 * interim response takes a slot and answers nothing and a continuation slot is
 * no response at all.  With states == NULL the call is rhp_walk_responses with
 * the rules below added, with states it is rhp_walk_resume with them added; the
 * batch, the flags, the clamps, the stop codes, the state and the memory
 * contract are theirs, word for word.
 *   Queue.  Session s's outstanding requests, oldest first, are q in
 *   [req_off[s], req_off[s+1]): nq = req_off[s+1] - req_off[s].  A pair that is
 *   not ordered or reaches beyond n_req_total owns no request: nq = 0.  k = 0
 *   at the start of every round: the caller pops answered[s] requests after
 *   each round, so a round's queue starts at the first unanswered request
 *   (which is why rhp_walk_state_t carries no count).
 *   Interim.  A head -- a slot with msgs[slot].ret > 0 and result 1 -- whose
 *   status is 100..199 is interim: it has no body already (the rule above) and
 *   does not advance k.  101 counts as interim: a protocol switch, like a 2xx
 *   to CONNECT, makes the connection something other than HTTP, and neither is
 *   handled here.
 *   Final.  Every other head with result 1 answers request k.  If k < nq and
 *   bit req_off[s] + k of head_bits is set the request was a HEAD: body_kind
 *   stays what the framing said, body_len = wire_len = 0, and the walk goes on
 *   behind the head -- the shape of the 1xx/204/304 rule.  No byte is moved,
 *   also with RHP_WALK_DEFRAME; no stop of BODY or CLOSE follows and no state
 *   is armed, also when Content-Length exceeds what is there or when neither
 *   header is present without RHP_WALK_NONE_EMPTY.  A framing answer of -1 (a
 *   bad Content-Length) is still RHP_WALK_BAD.  A HEAD bit on a 204 or 304
 *   reply changes nothing.  After the slot, k++.  Requests at k >= nq count as
 *   not HEAD; nothing is read for them.
 *   THE REFERENCE HAS NO RULE HERE, and no response walker: this is the walk's
 *   second invented rule (RFC 9112 section 6.3 item 1), beside the
 *   1xx/204/304 one.
 *   Outputs.  answered[s] = k at exit, for every session; 0 on the paths that
 *   keep the state as it lies (a corrupt or dead state, an empty round, a
 *   continuation with no slot).  It may exceed nq when responses arrive that
 *   nobody asked for: that is the caller's finding.  With slot_req != NULL
 *   every written slot gets its entry and no other slot does: a head with
 *   result 1 gets k as it was before the slot advanced it (an interim head
 *   names the request it precedes); a continuation slot and a slot that
 *   stopped with HEAD or BAD get RHP_WALK_REQ_NONE.
 *   Equivalence.  With every bit clear, or every nq == 0, the call leaves byte
 *   for byte what rhp_walk_responses / rhp_walk_resume leave in msgs, hdrs,
 *   slots, results, states and bytes.
 * Memory as the walk's; in addition req_off[0, n_sessions] is read, and of
 * head_bits words below (n_req_total + 31) / 32, a word only when some k < nq
 * of the session falls into it (one 4-byte load per 32 requests of a session's
 * queue); answered[0, n_sessions) is written, and the slot_req entries of the
 * written slots, as plain 4-byte stores.
 * -EINVAL (rhp_walk_args.h): whatever the underlying walk refuses; a NULL x;
 * reserved != 0; with n_sessions > 0 a NULL req_off or answered; a NULL
 * head_bits with n_req_total > 0; req_off, head_bits, answered or slot_req not
 * 4-byte aligned (device pointers only).  n_sessions == 0 succeeds and
 * launches nothing.
 * Launch contract as rhp_walk_responses: one launch, one session per lane,
 * asynchronous on `stream`, no allocation, no copy, no synchronisation.
 */
#define RHP_WALK_REQ_NONE 0xFFFFFFFFu   /* slot_req: the slot answers no request */

typedef struct rhp_walk_asked {
  const uint32_t *req_off;     /* device [n_sessions + 1]: session s's outstanding requests, oldest first,
                                  are q in [req_off[s], req_off[s+1]) */
  const uint32_t *head_bits;   /* device [(n_req_total + 31) / 32]: bit (q & 31) of word q >> 5 set: request q was a HEAD */
  uint32_t        n_req_total; /* host copy of req_off[n_sessions] */
  uint32_t        reserved;    /* must be 0 */
  uint32_t       *answered;    /* device [n_sessions] */
  uint32_t       *slot_req;    /* device [n_slots_total], or NULL */
} rhp_walk_asked_t;

int rhp_walk_answers(const rhp_walk_batch_t *w, rhp_walk_state_t *states /* or NULL */, const rhp_walk_asked_t *x,
                     void *stream);

/*
 * The header lookup over the slots of a walk: http_field_lookup
 * (src/reactor/http.c:167-175) for up to 16 names over the rhp_msg_t /
 * rhp_hdr_t records rhp_walk_responses or rhp_walk_resume left on the device,
 * the response side's rhp_classify_sessions.  w is the batch exactly as the
 * walk left it on `stream`; RHP_WALK_DEFRAME may be set or clear (a head never
 * moves: the de-framing writes only inside the wire span of a chunked body).
 * For every slot i < n_slots_total and every name j, fields[j * n_slots_total
 * + i] is written.
 *   Owner.  s is the last session with slot_off[s] <= i, s < n_sessions (a
 *   bisection per slot).
 *   In use.  With lo = slot_off[s], hi = slot_off[s+1]: lo <= i < hi, hi <=
 *   n_slots_total and i - lo < results[s].n_slots.  This one test is what lets
 *   any load of slots[i], msgs[i] or hdrs[i * max_headers + k] through,
 *   whatever the search returned: a slot the walk did not write holds stale
 *   records or nothing and is never read.
 *   Head.  An in-use slot is a head when slots[i].result == 1 and msgs[i].ret
 *   > 0.  (A continuation slot of rhp_walk_resume has ret == 0, a slot that
 *   stopped with RHP_WALK_HEAD or RHP_WALK_BAD has result != 1,
 *   RHP_RET_TOOLONG is negative.)
 *   Inside.  With st = slots[i].start and ret = msgs[i].ret, a head is looked
 *   up only when sess_off[s] <= st <= sess_off[s+1], ret <= sess_off[s+1] - st
 *   and st + ret <= bytes_size rounded down to a multiple of 4 (names are read
 *   as the aligned dwords that hold them, as rhp_frame_messages reads them).
 *   Every head the walk wrote passes; a crafted record that does not is absent.
 *   Lookup.  rhp_frame_messages' lookup for its caller's names: of the records
 *   k < min(num_headers, max_headers), request-major, those with name_off ==
 *   RHP_NAME_NULL (an obs-fold line) are skipped, and the first counts whose
 *   name has name j's length and equals it with a..z mapped to A..Z on both
 *   sides, no other byte.  fields[j * n_slots_total + i] = {value_off,
 *   value_len}, an offset from st; a present header with an empty value gives
 *   {value_off, 0}.  A record whose name does not lie inside [0, ret) matches
 *   nothing (no parsed record is like that).
 *   Absent.  Every other slot gets {RHP_NAME_NULL, 0} for every name: a slot
 *   not in use, a continuation slot, a slot that stopped with HEAD or BAD, a
 *   head that is not inside, a missing header, any slot when max_headers == 0.
 * Memory.  Nothing is read outside bytes[0, bytes_size), sess_off[0,
 * n_sessions], slot_off[0, n_sessions], results[0, n_sessions) and the records
 * of the slots in use, whatever slot_off, sess_off, results or the records
 * hold; records k >= num_headers are never read, name bytes only of records
 * whose name_len is a name's.  Nothing is written outside fields[0, n_names *
 * n_slots_total).  With slot_off not monotone a slot may be reported absent;
 * the answers are otherwise unspecified.
 * -EINVAL (rhp_lookup_args.h): whatever rhp_walk_responses refuses about w; a
 * NULL l; reserved != 0; n_names == 0 or above RHP_CLASSIFY_MAX_NAMES; an empty
 * name or one longer than RHP_CLASSIFY_NAME_MAX; a NULL text, names or fields;
 * a NULL results with n_sessions > 0; fields not 4-byte aligned (device
 * pointers only).  n_slots_total == 0 or n_sessions == 0 succeeds and launches
 * nothing: with no session there is none to own a slot, so with n_sessions ==
 * 0 and slots present nothing is launched either and fields is not touched.
 * Launch contract as rhp_classify_sessions: one launch, one slot per lane,
 * asynchronous on `stream`, no allocation, no copy, no synchronisation; the
 * names travel in the kernel argument and the caller's tables are free when
 * the call returns; thread-safe.
 */
typedef struct rhp_walk_lookup {
  const uint8_t    *text;      /* host: the bytes of the names (as rhp_classify_t) */
  const rhp_span_t *names;     /* host [n_names]: spans of `text` */
  uint32_t          n_names;   /* 1 .. RHP_CLASSIFY_MAX_NAMES */
  uint32_t          reserved;  /* must be 0 */
  rhp_fieldref_t   *fields;    /* device [n_names * n_slots_total], name-major: fields[j * n_slots_total + i] */
} rhp_walk_lookup_t;

int rhp_lookup_walked(const rhp_walk_batch_t *w, const rhp_walk_lookup_t *l, void *stream);

/*
 * The walked responses re-written for the client side: what a proxy does next
 * with each upstream response is one call of the reference's writer,
 *   http_write_response(&client->stream, status, date, type, body, fields, fields_count)
 * (src/reactor/http.c:236-297), and this is that call for every slot of a walk
 * that holds a whole response, from the records where they lie.  w is the batch
 * exactly as rhp_walk_responses, rhp_walk_resume or rhp_walk_answers left it on
 * `stream`.  For every slot i < n_slots_total, why[i] and out_off[i + 1] -
 * out_off[i] are written; out_off is the exclusive prefix sum of the sizes.
 *   Relayed.  Slot i is relayed -- why[i] == RHP_RELAY_OK -- when every test
 *   below holds; otherwise its size is 0 and why[i] names the first that failed
 *   (enum rhp_relay_why, in this order):
 *     UNUSED    it is in use, NOT_HEAD a head, OUTSIDE and inside, the three
 *               words as rhp_lookup_walked defines them (owner by the same
 *               bisection; nothing of a slot not in use is read);
 *     INTERIM   its status is not 100..199: interim heads are the proxy's own
 *               business;
 *     PARTIAL   it is not the session's last written slot (i - slot_off[s] + 1 ==
 *               n_slots) of a round that stopped with RHP_WALK_BODY or
 *               RHP_WALK_CLOSE: that body is not all there, the host streams it;
 *     FOLD      none of its header records k < min(num_headers, max_headers) has
 *               name_off == RHP_NAME_NULL: the reference's writer has no form for
 *               an obs-fold line, such a head goes to the host;
 *     SPAN      its phrase (msg_len > 0) and the name and value of every such
 *               record lie inside [0, ret) (every parsed record does; a crafted
 *               one that does not is never read through);
 *     FRAMING   its body can be named: both lengths 0 whatever the kind (the
 *               1xx/204/304 rule, a reply to a HEAD, RHP_WALK_NONE_EMPTY, an
 *               empty body); RHP_FRAME_LENGTH with wire_len == body_len;
 *               RHP_FRAME_CHUNKED only when w->flags has RHP_WALK_DEFRAME, the
 *               body then being the first body_len bytes of the wire span;
 *     LONG      body_len < 2^32 (the reference prints Content-Length with
 *               http_u32_sprint);
 *     BODY_OUTSIDE  [start + ret, start + ret + body_len) lies inside the
 *               session and below the readable end (Memory, below).
 *   Bytes.  A relayed slot's bytes are exactly what http_write_response
 *   appends (the layout is rhp_write_responses', above) for
 *     status  three decimal digits, those of msgs[i].status modulo 1000 with
 *             leading zeros kept (a parsed status is below 1000; of a crafted
 *             one above, the thousands are not printed, and the INTERIM test
 *             looks at the whole value), and, when msg_len > 0, one SP and the
 *             phrase bytes.  The digits are printed, not copied: the record
 *             does not say where they stood;
 *     type    the value of the first header whose name equals Content-Type;
 *             empty when there is none;
 *     body    as above;
 *     fields  the head's header records in order, name and value bytes as they
 *             lie, but for every record -- every match, not only the first --
 *             whose name equals Content-Type, Content-Length, Transfer-Encoding
 *             or one of the caller's n_names names (typically Connection,
 *             Keep-Alive, Server, Date).
 *   Names are equal under rhp_lookup_walked's fold: equal lengths and equal
 *   bytes with a..z mapped to A..Z on both sides, no other byte.
 *   THE REFERENCE HAS NO RULE HERE for four things, which are this call's
 *   invented part: the fold above and which names are dropped; the status text
 *   (printed digits, one SP, the phrase); the upstream's minor version is not
 *   carried, the writer's text being "HTTP/1.1"; and a reply to a HEAD and a
 *   304 go out with "Content-Length: 0", as a libreactor server would send
 *   them, whatever the upstream's Content-Length said.  Everything else is the
 *   reference's writer, byte for byte.
 *   Order.  Slots are written in ascending index, so a session's replies are
 *   contiguous: out[out_off[slot_off[s]], out_off[slot_off[s+1]]).
 *   When out_off[n_slots_total] > out_size nothing is written to `out`; out_off
 *   and why are still complete: grow and call again.
 * Memory.  Nothing is read but what rhp_lookup_walked reads and, of a relayed
 * slot, its body.  Phrase, names, values and bodies are read as the aligned
 * dwords that hold them, so the BODY_OUTSIDE test bounds start + ret +
 * body_len, rounded up to 4, by the readable end the walk clamps its sessions
 * to (bytes_size rounded down to whole 16-byte lines, less one line), and the
 * head lies below bytes_size rounded down to 4 as for the lookup.  Nothing is
 * written outside out_off[0, n_slots_total], why[0, n_slots_total), work and
 * out[0, out_off[n_slots_total]).
 * -EINVAL (rhp_relay_args.h): whatever rhp_walk_responses refuses about w; a
 * NULL r, out_off, why, date or work; date_len != RHP_DATE_LEN; n_names above
 * RHP_RELAY_MAX_NAMES; a NULL text or names with n_names > 0; an empty name or
 * one longer than RHP_CLASSIFY_NAME_MAX; a NULL out with out_size != 0; a NULL
 * results with n_sessions > 0; out_off not 8-byte aligned, why not 4-byte
 * aligned, work not 8-byte aligned (device pointers only).  n_slots_total == 0
 * or n_sessions == 0 writes out_off[0] = 0 and nothing else.
 * Launch contract as rhp_write_responses: four kernels on `stream` (sizes with
 * tile sums, two scan passes, copy), asynchronous, no allocation, no copy, no
 * synchronisation; the names and the date travel in the kernel argument and
 * the caller's tables are free when the call returns; thread-safe.  The empty
 * call (n_slots_total == 0 or n_sessions == 0) launches no kernel: its
 * out_off[0] = 0 is one 8-byte hipMemsetAsync on `stream`, as
 * rhp_write_responses' with n == 0.
 */
#define RHP_RELAY_MAX_NAMES (RHP_CLASSIFY_MAX_NAMES - 3u)   /* the three built-in names take the rest */

enum rhp_relay_why { RHP_RELAY_OK = 0,        /* relayed */
                     RHP_RELAY_UNUSED,        /* the walk did not write the slot */
                     RHP_RELAY_NOT_HEAD,      /* a continuation slot, a HEAD or BAD stop slot */
                     RHP_RELAY_OUTSIDE,       /* the head does not lie inside its session */
                     RHP_RELAY_INTERIM,       /* status 100..199 */
                     RHP_RELAY_PARTIAL,       /* the last slot of a BODY or CLOSE round */
                     RHP_RELAY_FOLD,          /* an obs-fold line among the headers */
                     RHP_RELAY_SPAN,          /* a phrase, name or value outside [0, ret) */
                     RHP_RELAY_FRAMING,       /* the body cannot be named */
                     RHP_RELAY_LONG,          /* body_len >= 2^32 */
                     RHP_RELAY_BODY_OUTSIDE}; /* the body does not lie inside its session */

typedef struct rhp_walk_relay {
  const uint8_t    *text;       /* host: the bytes of the caller's drop names (as rhp_walk_lookup_t) */
  const rhp_span_t *names;      /* host [n_names]: spans of `text` */
  uint32_t          n_names;    /* 0 .. RHP_RELAY_MAX_NAMES */
  uint32_t          date_len;   /* must be RHP_DATE_LEN */
  const char       *date;       /* host, date_len bytes */
  uint64_t         *out_off;    /* device [n_slots_total + 1]: exclusive prefix sum of the sizes, always written */
  uint32_t         *why;        /* device [n_slots_total]: enum rhp_relay_why */
  uint8_t          *out;        /* device, out_size bytes, any alignment */
  uint64_t          out_size;   /* out_off[n_slots_total] > out_size: nothing is written to out */
  uint64_t         *work;       /* device scratch, >= RHP_RELAY_WORK_WORDS(n_slots_total) u64 */
} rhp_walk_relay_t;

/* the tile sums of the scan, and per slot the plan the sizes step leaves the
 * copy step: which header records are kept, and the type's value */
#define RHP_RELAY_WORK_WORDS(n) (((uint64_t) (n) + 4095u) / 4096u + 1u + 2u * (uint64_t) (n))

int rhp_relay_walked(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, void *stream);

/* For measuring, not for a reactor's round: rhp_relay_walked and
 * rhp_write_responses with a HIP event recorded on `stream` before the sizes
 * step, behind it, behind the two scan kernels and behind the copy step.  The
 * call creates and destroys its four events, waits for the last one (a host
 * synchronisation) and returns the three elapsed times in microseconds: us[0]
 * sizes, us[1] scan, us[2] copy.  The same kernels, arguments, outputs and
 * codes as the plain call; an empty call (no slot, n == 0) and a NULL us are
 * -EINVAL.  tools/bench_walk_relay.py. */
int rhp_relay_walked_steps(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r, void *stream, float us[3]);
int rhp_write_responses_steps(const rhp_resp_batch_t *batch, void *stream, float us[3]);

/*
 * The requests of a proxied route re-written for the upstream: the request
 * side's rhp_relay_walked.  batch, sessions, results and req_start are
 * rhp_classify_sessions' arguments as the parse and the fix-up left them on
 * `stream` (an RHP_MODE_HTTP batch whose flags are exactly
 * RHP_BATCH_SPECULATIVE, request-major or header-major), route is its output.
 * For every slot i < batch->n, why[i] and out_off[i + 1] - out_off[i] are
 * written; out_off is the exclusive prefix sum of the sizes.
 *   Forwarded.  Slot i is forwarded -- why[i] == RHP_FORWARD_OK -- when every
 *   test below holds; otherwise its size is 0 and why[i] names the first that
 *   failed (enum rhp_forward_why, in this order):
 *     UNUSED    some session owns it: s is the last session with piece_lo <= i
 *               (a bisection per slot) and piece_lo <= i < piece_lo + n_slots,
 *               piece_lo <= piece_hi <= n, the test of rhp_classify_sessions.
 *               Nothing of a slot that is not in use is read;
 *     NOT_READY http[i].result == 1 and reqs[i].ret > 0;
 *     OUTSIDE   [req_start[i], req_start[i] + ret) lies inside the session's
 *               input [offsets[piece_lo], offsets[piece_hi]) and below
 *               bytes_size rounded down to a multiple of 4;
 *     CLOSED    the session's walk did not stop on -1: with last = piece_lo +
 *               n_slots - 1, http[last].result != -1 (last < n is a slot of the
 *               batch; a session whose n_slots runs past n is not closed and its
 *               record is not read);
 *     ROUTE     route[i] < n_routes and bit route[i] of forward_mask is set;
 *     FOLD      no header record k < min(num_headers, max_headers) has name_off
 *               == RHP_NAME_NULL (an obs-fold line has no name to write);
 *     SPAN      method, path and every such record's name and value lie inside
 *               [0, ret) (every parsed record does; a crafted one that does not
 *               is never read through);
 *     BODY      body_kind is 0 or 1 (RHP_BODY_CHUNKED_PENDING cannot remain
 *               after the fix-up; a crafted one goes to the host);
 *     LONG      body_len < 2^32 when body_kind == 1;
 *     BODY_OUTSIDE  when body_kind == 1, [req_start + ret, req_start + ret +
 *               body_len) lies inside the session's input and below bytes_size
 *               rounded down to a multiple of 4 (Memory, below).
 *   There is no leading-run rule: a forwarded request may stand behind one the
 *   host answers.
 *   THE REFERENCE HAS NO RULE HERE.  The reference writes responses
 *   (http_write_response) and never a request, so the whole serialization is
 *   this call's invention: the fixed text "HTTP/1.1" (the client's minor
 *   version is not carried), which names are dropped, where Content-Length and
 *   `extra` stand, and the CLOSED rule (the reference closes such a session,
 *   server.c:47-51; rhp_reply_sessions answers none of it).  What ties it to the
 *   reference is the round trip: http_read_request over a forwarded slot's
 *   bytes gives result 1, consumed == the size, the same method, target and
 *   body, and as fields the kept records, then Content-Length when written,
 *   then the lines of `extra` (tests/golden/make_golden_forward.py).
 *   Bytes.  A forwarded slot's bytes are, in order: the method bytes; one SP;
 *   the path bytes; the 11 bytes " HTTP/1.1\r\n"; every kept header record in
 *   order as name ": " value CRLF, name and value bytes as they lie
 *   (http_push_field's form, http.c:63-71) -- every record is kept but for
 *   every one, not only the first, whose name equals Content-Length,
 *   Transfer-Encoding or one of the caller's n_names names under the classify
 *   fold (equal lengths, a..z mapped to A..Z on both sides, no other byte);
 *   when body_kind == 1, "Content-Length: ", body_len in decimal and CRLF (also
 *   for length 0, and also for a chunked body the fix-up de-framed); the
 *   extra_len bytes of `extra` as they lie; CRLF; the body_len body bytes from
 *   req_start + ret.  body_kind == 0 writes no Content-Length line.
 *   Order.  Slots are written in ascending index.  When out_off[n] > out_size
 *   nothing is written to `out`; out_off, why, fwd_off and head_bits are still
 *   complete: grow and call again.
 *   The queue for the upstream walk.  fwd_off[s], s < n_sessions, is the number
 *   of forwarded slots below min(piece_lo(s), n) -- with the sessions in order,
 *   the count of forwarded slots owned by the sessions before s --
 *   and fwd_off[n_sessions] the total.  The q-th forwarded slot in ascending
 *   slot order sets bit q & 31 of head_bits[q >> 5] when its method is the four
 *   bytes "HEAD" (string_equal: case matters).  Every word below (total + 31) /
 *   32 is written whole, its bits at and above `total` clear; no word beyond
 *   that is touched.  With one upstream connection per client session these
 *   are rhp_walk_asked_t's req_off and head_bits as they stand.
 * The bytes are read through bytes_rw when it is set, as rhp_classify_sessions
 * reads them.  Contract: `sessions` ascends by piece_lo with disjoint ranges.
 * With that order violated a slot may be reported UNUSED and fwd_off is as
 * defined above; nothing is read outside the arguments' buffers.
 * Memory.  Method, path, names, values and bodies are read as the aligned
 * dwords that hold them, so OUTSIDE and BODY_OUTSIDE bound the request's and the
 * body's end by bytes_size rounded down to 4: an end at or below a multiple of
 * 4 stays there when it is rounded up to 4.  Nothing is written outside
 * out_off[0, n], why[0, n), fwd_off[0, n_sessions], head_bits[0, (total + 31) /
 * 32), work and out[0, out_off[n]).
 * -EINVAL (rhp_forward_args.h): whatever rhp_classify_sessions refuses about the
 * batch, sessions, results and req_start; a NULL route, f, out_off, why,
 * fwd_off, head_bits or work; a NULL out with out_size != 0; n_routes 0 or above
 * RHP_CLASSIFY_MAX_ROUTES; n_names above RHP_FORWARD_MAX_NAMES; a NULL text or
 * names with n_names > 0; an empty name or one longer than
 * RHP_CLASSIFY_NAME_MAX; extra_len above RHP_FORWARD_EXTRA_MAX; a NULL extra
 * with extra_len > 0, or extra bytes that do not end in CRLF; out_off or work not
 * 8-byte aligned, why, fwd_off or head_bits not 4-byte aligned (device pointers
 * only).  n == 0 or n_sessions == 0 writes out_off[0] = 0 and fwd_off[0,
 * n_sessions] = 0 and nothing else, by two hipMemsetAsync on `stream` and no
 * kernel.
 * Launch contract: seven kernels on `stream` (sizes with tile sums; two scan
 * passes over the sizes, the same two over the forwarded counts; fwd_off and the
 * zeroed head_bits words; copy), asynchronous, no allocation, no copy, no
 * synchronisation; the names and `extra` travel in the kernel arguments and the
 * caller's tables are free when the call returns; thread-safe.
 */
#define RHP_FORWARD_MAX_NAMES (RHP_CLASSIFY_MAX_NAMES - 2u)   /* the two built-in names take the rest */
#define RHP_FORWARD_EXTRA_MAX 128u

enum rhp_forward_why { RHP_FORWARD_OK = 0,        /* forwarded */
                       RHP_FORWARD_UNUSED,        /* no session owns the slot */
                       RHP_FORWARD_NOT_READY,     /* result != 1 or ret <= 0 */
                       RHP_FORWARD_OUTSIDE,       /* the request does not lie inside its session */
                       RHP_FORWARD_CLOSED,        /* the session's walk stopped on -1 */
                       RHP_FORWARD_ROUTE,         /* not a forwarded route */
                       RHP_FORWARD_FOLD,          /* an obs-fold line among the headers */
                       RHP_FORWARD_SPAN,          /* method, path, a name or a value outside [0, ret) */
                       RHP_FORWARD_BODY,          /* body_kind is neither 0 nor 1 */
                       RHP_FORWARD_LONG,          /* body_len >= 2^32 */
                       RHP_FORWARD_BODY_OUTSIDE}; /* the body does not lie inside its session */

typedef struct rhp_forward {
  uint32_t          n_routes;      /* 1..RHP_CLASSIFY_MAX_ROUTES: the classify call's n_routes */
  uint32_t          forward_mask;  /* bit r set: route r goes upstream */
  const uint8_t    *text;          /* host: the bytes of the caller's drop names (as rhp_walk_relay_t) */
  const rhp_span_t *names;         /* host [n_names]: spans of `text` */
  uint32_t          n_names;       /* 0 .. RHP_FORWARD_MAX_NAMES */
  uint32_t          extra_len;     /* 0 .. RHP_FORWARD_EXTRA_MAX */
  const uint8_t    *extra;         /* host, extra_len bytes: whole header lines, the last ending in CRLF */
  uint64_t         *out_off;       /* device [n + 1]: exclusive prefix sum of the sizes, always written */
  uint32_t         *why;           /* device [n]: enum rhp_forward_why */
  uint8_t          *out;           /* device, out_size bytes, any alignment */
  uint64_t          out_size;      /* out_off[n] > out_size: nothing is written to out */
  uint32_t         *fwd_off;       /* device [n_sessions + 1] */
  uint32_t         *head_bits;     /* device [(n + 31) / 32] at the most; (total + 31) / 32 words are written */
  uint64_t         *work;          /* device scratch, >= RHP_FORWARD_WORK_WORDS(n, n_sessions) u64 */
} rhp_forward_t;

/* two rows of tile sums (sizes, forwarded counts), the n + 1 counts, per slot
 * the plan the sizes step leaves the copy step (which header records are kept)
 * and per 64 slots the HEAD flags of the forwarded ones */
#define RHP_FORWARD_WORK_WORDS(n, n_sessions) \
  (2u * (((uint64_t) (n) + 4095u) / 4096u + 1u) + 2u * (uint64_t) (n) + 1u + ((uint64_t) (n) + 63u) / 64u + 0u * (uint64_t) (n_sessions))

int rhp_forward_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                         const rhp_session_result_t *results, const uint64_t *req_start,
                         const uint16_t *route, const rhp_forward_t *f, void *stream);


#ifdef __cplusplus
}
#endif
#endif
