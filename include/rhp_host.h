/*
 * rhp_host.h -- host-side entry points of librhp_host.so (no GPU): the
 * product's (csrc/rhp_host.cpp; libreactor.so links them) and, for tests, the
 * DFA emulator and the rhp_test_* hooks (csrc/rhp_emu.cpp).
 *
 *   rhp_cpu_parse_batch   the product's exact scalar parser (rhp_scalar.h, the
 *                         same code the kernel's rare paths run) over a batch in
 *                         host memory; the reactor's http_read_request and its
 *                         "host" session parser use it
 *   rhp_emu_parse_batch   CPU emulation of the kernel's DFA algorithm, block for
 *                         block (tests only); stats[3] = fast ok, fast -1, exact
 *   rhp_emu_fixup_sessions  rhp_fixup_kernel's prefix and walk per session, on
 *                         the host (tests only)
 *   (both take an rhp_batch_t (include/rhp.h) whose pointers are host memory,
 *   of any alignment, and refuse with -22 what rhp_parse_batch refuses:
 *   rhp_records.h rhp_batch_check)
 *   rhp_expand_records    any layout's header records (the compact and dense
 *                         ones included) as rhp_hdr_t, on the host;
 *   rhp_expand_reqs       the dense layouts' request records as rhp_req_t
 *   rhp_expand_http       the compact http records (RHP_LAYOUT_COMPACT and
 *                         RHP_LAYOUT_DENSE) as rhp_http_t
 *   rhp_cpu_classify_batch  rhp_classify_batch (rhp.h) over a parsed batch in
 *                         host memory, written over the three rhp_expand_*
 *   rhp_cpu_classify_sessions  rhp_classify_sessions (rhp.h) over the slots a
 *                         host fix-up left in a speculative batch
 *   rhp_cpu_reply_sessions, rhp_cpu_gather_wide  rhp_reply_sessions and
 *                         rhp_gather_wide (rhp.h) as sequential walks
 *   rhp_cpu_split_sessions  rhp_split_sessions (rhp.h) as a walk over the bytes
 *   rhp_cpu_parse_messages  rhp_parse_messages (rhp.h): the kernel's templates
 *                         over host memory
 *   rhp_cpu_decode_chunked  rhp_decode_chunked (rhp.h): the scalar statement of
 *                         phr_decode_chunked over host memory, and
 *                         rhp_phr_decode_chunked, the pointer-based drop-in
 *
 *   rhp_phr_parse_request the same exact parser with phr_parse_request's own
 *                         signature and outputs (pointers into buf, no length
 *                         limit): a drop-in for
 *                         /root/reference/src/picohttpparser/picohttpparser.h:51-52
 *                         (last_len != 0 runs is_complete first, :197-223, :399-401)
 *   rhp_http_read_cpu     http_read_request (/root/reference/src/reactor/http.c:177-234)
 *                         over one buffer with pointer outputs: the reactor's
 *                         http_read_request, and the server's path for requests
 *                         whose records do not fit the batch format (RHP_RET_TOOLONG)
 */
#ifndef RHP_HOST_H
#define RHP_HOST_H

#include <stdint.h>
#include <sys/types.h>
#include "rhp.h"

#ifdef __cplusplus
extern "C" {
#endif

int rhp_cpu_parse_batch(const rhp_batch_t *batch);
/* rhp_fixup_sessions (rhp.h) on the host, over a RHP_BATCH_SPECULATIVE batch
 * parsed by rhp_cpu_parse_batch; 0 or -22 */
int rhp_cpu_fixup_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                           rhp_session_result_t *results, uint64_t *req_start);
int rhp_emu_parse_batch(const rhp_batch_t *batch, uint64_t *stats);
/* rhp_cpu_fixup_sessions as the device runs it (tests only): per session the
 * kernel's prefix of whole pieces, 64 per step (rhp_scalar.h fixup_lane_other,
 * fixup_step_stop: the code rhp_fixup_kernel runs), then the walk from the
 * first other piece.  The same outputs as rhp_cpu_fixup_sessions. */
int rhp_emu_fixup_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                           rhp_session_result_t *results, uint64_t *req_start);
/* rhp_pack_dense (rhp.h) on the host, over host copies of the batch's records
 * (the reactor's host-async parser exercises the dense copy-back with it) */
int rhp_cpu_pack_dense(const rhp_batch_t *batch, rhp_req_dense_t *dreq, rhp_http_compact_t *hc, uint16_t *lens16);

/* rhp_classify_batch (rhp.h) on the host: `batch` is a parsed batch whose
 * pointers, and c->fields and c->route, are host memory.  The same results
 * and the same -22 for refused arguments (the GPU tests compare the two). */
int rhp_cpu_classify_batch(const rhp_batch_t *batch, const rhp_classify_t *c);
/* rhp_classify_sessions (rhp.h) on the host: `batch` is the speculative batch a
 * host parse and rhp_cpu_fixup_sessions / rhp_emu_fixup_sessions left, and
 * every pointer is host memory.  The same results and the same -22.  The
 * slots in use are found by a walk over the sessions, one after the other (the
 * kernel searches sessions[].piece_lo): the two share the argument check and
 * nothing else, and this one gives the right answers for sessions in any order. */
int rhp_cpu_classify_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                              const rhp_session_result_t *results, const uint64_t *req_start,
                              const rhp_classify_t *c);

/* A parsed batch's header records as rhp_hdr_t, out[i * max_headers + k]
 * (request-major), from host copies of its reqs and hdrs in the batch's
 * layout; records past num_headers and those of requests with ret <= 0 are
 * zeroed.  For RHP_LAYOUT_COMPACT / RHP_LAYOUT_DENSE this is the running sum
 * of rhp.h (the wide records for RHP_F_WIDE requests; reqs as rhp_expand_reqs
 * makes them).  `batch` supplies n, max_headers and
 * layout only.  0, or -22 on bad arguments. */
int rhp_expand_records(const rhp_batch_t *batch, const rhp_req_t *reqs, const void *hdrs, rhp_hdr_t *out);
/* A parsed batch's request records as rhp_req_t[n]: copied, or for
 * RHP_LAYOUT_DENSE expanded from rhp_req_dense_t and the wide area (rhp.h;
 * a dense record's flags become 0, a wide one's RHP_F_WIDE is set).  `reqs` is
 * the batch's reqs buffer as the parser left it.  0, or -22.  Expand the
 * requests first: rhp_expand_records and rhp_expand_http take rhp_req_t. */
int rhp_expand_reqs(const rhp_batch_t *batch, const void *reqs, rhp_req_t *out);
/* A batch's http records (RHP_MODE_HTTP) as rhp_http_t[n]: copied, or for
 * RHP_LAYOUT_COMPACT and RHP_LAYOUT_DENSE (both hold RHP_COMPACT_HTTP_BYTES(n)
 * bytes) expanded from the compact records and their wide area (rhp.h
 * rhp_http_compact_t; consumed from reqs[i].ret).  0, or -22. */
int rhp_expand_http(const rhp_batch_t *batch, const rhp_req_t *reqs, const void *http, rhp_http_t *out);

/* rhp_reply_sessions (rhp.h) over a speculative batch in host memory after a
 * host fix-up and classify: every pointer of the arguments is host memory, there
 * is no stream, `work` is not used (it must still be there, as for the device
 * call).  A sequential walk over the sessions; it shares only the argument check
 * with the kernels.  A NULL `images` is refused unless every image is empty.
 * 0, or -22. */
int rhp_cpu_reply_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                           const rhp_session_result_t *results, const uint16_t *route,
                           const rhp_reply_table_t *table, const rhp_reply_out_t *o);

/* rhp_gather_wide (rhp.h) over a speculative batch in host memory after a host
 * fix-up and rhp_cpu_pack_dense: every pointer of the arguments is host memory,
 * there is no stream, `work` is not used (it must still be there, as for the
 * device call).  A sequential walk over the sessions, the totals first and then
 * the three areas; it shares only the argument check with the kernels.  The
 * same results for sessions in order and the same -22. */
int rhp_cpu_gather_wide(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                        const rhp_session_result_t *results, const uint64_t *req_start,
                        const rhp_req_dense_t *dreq, const rhp_http_compact_t *hc, const rhp_wide_out_t *o);

/* rhp_split_sessions (rhp.h) over bytes and sess_off in host memory: every
 * pointer of the arguments is host memory, there is no stream, `work` is not
 * used (it must still be there, as for the device call).  A sequential walk
 * over each session's bytes; it shares only the argument check with the
 * kernels.  Only the bytes of [sess_off[0], sess_off[n_sessions]) are read.  The
 * same outputs, the same overflow and tail behaviour and the same -22. */
int rhp_cpu_split_sessions(const uint8_t *bytes, uint64_t bytes_end, const uint64_t *sess_off, uint32_t n_sessions,
                           const rhp_split_out_t *o);

/* rhp_parse_messages (rhp.h) over a batch in host memory: every pointer of the
 * batch is host memory, of any alignment, and there is no stream.  The same
 * records and the same -22 (rhp_msg_args.h; the alignment rules are the
 * device's alone).  As the reference, it reads the bytes after a message while
 * the SP skip behind a response's version runs (rhp.h). */
int rhp_cpu_parse_messages(const rhp_msg_batch_t *batch);

/* rhp_frame_messages (rhp.h) over a batch in host memory, as
 * rhp_cpu_parse_messages left it: every pointer of the batch and of `f` is host
 * memory, of any alignment, and there is no stream.  The same frames, fields
 * and armed decoders and the same -22 (rhp_frame_args.h; the alignment rules
 * are the device's alone).  Of a message's bytes only names and values inside
 * [0, ret) are read. */
int rhp_cpu_frame_messages(const rhp_msg_batch_t *batch, const rhp_frame_args_t *f);

/* rhp_walk_responses (rhp.h) over sessions in host memory: every pointer of
 * `w` is host memory, of any alignment, and there is no stream.  The same
 * msgs, hdrs, slots, results and de-framed bytes and the same -22
 * (rhp_walk_args.h; the alignment rules are the device's alone).  No byte at or
 * beyond bytes + bytes_size is read. */
int rhp_cpu_walk_responses(const rhp_walk_batch_t *w);

/* rhp_walk_resume (rhp.h) over sessions and states in host memory, of any
 * alignment, with no stream: one round, states[s] read at entry and written at
 * exit.  The same msgs, hdrs, slots, results, states and de-framed bytes and
 * the same -22 (rhp_walk_args.h; the alignment rules are the device's alone).
 * Sequential; a caller with threads hands each a range of sessions. */
int rhp_cpu_walk_resume(const rhp_walk_batch_t *w, rhp_walk_state_t *states);

/* rhp_walk_answers (rhp.h) over sessions, states (or NULL) and a queue in host
 * memory: every pointer of `w` and `x` is a host pointer, the four arrays of
 * `x` uint32_t arrays as the language aligns them.  The statement is the
 * kernels' (rhp_scalar.h walk_session_t / walk_resume_t with the Asked policy),
 * session by session, with the same argument check, the same clamps and the
 * same -22 (rhp_walk_args.h; the alignment rules are the device's alone).
 * Returns 0. */
int rhp_cpu_walk_answers(const rhp_walk_batch_t *w, rhp_walk_state_t *states /* or NULL */, const rhp_walk_asked_t *x);

/* rhp_lookup_walked (rhp.h) over a walk's records in host memory, as
 * rhp_cpu_walk_responses or rhp_cpu_walk_resume left them: every pointer of `w`
 * and of `l` is host memory, of any alignment, and there is no stream.  The
 * same fields and the same -22 (rhp_lookup_args.h; the alignment rules are the
 * device's alone).  Of the bytes only names inside a looked-up head are read,
 * and no record of a slot that is not in use.  Sequential. */
int rhp_cpu_lookup_walked(const rhp_walk_batch_t *w, const rhp_walk_lookup_t *l);

/* rhp_relay_walked (rhp.h) over a walk's records in host memory: every pointer
 * of `w` and of `r` is host memory, of any alignment, and there is no stream.
 * The same out_off, why and out and the same -22 (rhp_relay_args.h; the
 * alignment rules are the device's alone).  work has to be there and is not
 * touched.  Bytes are read one at a time: of the batch's bytes only the heads
 * and bodies of relayed slots, and no record of a slot that is not in use.
 * Sequential. */
int rhp_cpu_relay_walked(const rhp_walk_batch_t *w, const rhp_walk_relay_t *r);

/* rhp_forward_sessions (rhp.h) over a speculative batch in host memory after a
 * host fix-up and classify: every pointer of the arguments is host memory, of
 * any alignment for the outputs, and there is no stream.  The same out_off,
 * why, out, fwd_off and head_bits and the same -22 (rhp_forward_args.h; the
 * alignment rules are the device's alone).  work has to be there and is not
 * touched.  Bytes are read one at a time: of the batch's bytes only the
 * requests and bodies of forwarded slots, and no record of a slot that is not
 * in use.  Sequential. */
int rhp_cpu_forward_sessions(const rhp_batch_t *batch, const rhp_session_t *sessions, uint32_t n_sessions,
                             const rhp_session_result_t *results, const uint64_t *req_start,
                             const uint16_t *route, const rhp_forward_t *f);

/* struct phr_header (picohttpparser.h:42-47): name == NULL for an obs-fold line */
typedef struct rhp_phr_header {
  const char *name;
  size_t      name_len;
  const char *value;
  size_t      value_len;
} rhp_phr_header_t;

/* phr_parse_request: >0 bytes consumed, -1 malformed, -2 partial.  *num_headers
 * is the capacity on input and the count on output.  As the reference, it may
 * read bytes past buf + len while they are SP (picohttpparser.c:356-362). */
int rhp_phr_parse_request(const char *buf, size_t len, const char **method, size_t *method_len, const char **path,
                          size_t *path_len, int *minor_version, rhp_phr_header_t *headers, size_t *num_headers,
                          size_t last_len);

/* phr_parse_response and phr_parse_headers (picohttpparser.h:55-59) with
 * their own signatures and outputs, no length limit: what a caller runs on a
 * message rhp_parse_messages answered with RHP_RET_TOOLONG.  *num_headers is
 * the capacity on input and the count on output; last_len != 0 runs
 * is_complete first.  rhp_phr_parse_response may read bytes past buf + len
 * while they are SP (picohttpparser.c:423-425). */
int rhp_phr_parse_response(const char *buf, size_t len, int *minor_version, int *status, const char **msg,
                           size_t *msg_len, rhp_phr_header_t *headers, size_t *num_headers, size_t last_len);
int rhp_phr_parse_headers(const char *buf, size_t len, rhp_phr_header_t *headers, size_t *num_headers, size_t last_len);

/* rhp_decode_chunked (rhp.h) over a batch in host memory: every pointer of the
 * batch is host memory, of any alignment, and there is no stream.  The same
 * results, decoders and bytes and the same -22 (rhp_chunked_args.h; the
 * alignment rules are the device's alone).  Only a piece's own bytes are read. */
int rhp_cpu_decode_chunked(const rhp_chunked_batch_t *batch);

/* phr_decode_chunked and phr_decode_chunked_is_in_data (picohttpparser.h:62-86)
 * with their own signatures: rhp_chunked_t has struct phr_chunked_decoder's
 * layout.  A corrupt decoder (rhp.h) gives -1 and *bufsz = 0 where the
 * reference asserts. */
ssize_t rhp_phr_decode_chunked(rhp_chunked_t *decoder, char *buf, size_t *bufsz);
int rhp_phr_decode_chunked_is_in_data(rhp_chunked_t *decoder);

/* http_read_request's outputs for one buffer (http.c:177-234) */
typedef struct rhp_http_req {
  const char    *method;
  size_t         method_len;
  const char    *target;
  size_t         target_len;
  int            minor_version;
  const uint8_t *body;       /* NULL: data_null() */
  size_t         body_len;
  uint64_t       consumed;   /* bytes stream_consume() is given (result 1) */
} rhp_http_req_t;

/* 1 ready, 0 need more bytes (or empty), -1 malformed.  *fields_count is the
 * capacity on input, the count on output.  A chunked body is de-framed in place
 * (http.c:155), so buf is written. */
int rhp_http_read_cpu(uint8_t *buf, size_t len, rhp_http_req_t *req, rhp_phr_header_t *fields, size_t *fields_count);

/* Test hooks (tests/test_cpu_units.py): the GPU replay's windowed chunk-size-line
 * parse (rhp_scalar.h one_chunk_window: the nw <= 32 bytes at `line`, 32
 * readable; 0 = undecided) and the byte-wise one it must equal (one_chunk_t,
 * the size line at body offset `at`; the body readable to size + 64). */
int rhp_test_chunk_window(const uint8_t *line, uint32_t nw, uint64_t avail, int64_t *res, uint64_t *data_off,
                          uint64_t *data_len);
int64_t rhp_test_chunk_exact(const uint8_t *body, uint64_t at, uint64_t size, uint64_t *data_off, uint64_t *data_len);
/* Test hook (tests/test_sessions.py): whole[j] = 1 where piece j of a parsed
 * speculative batch is one the fix-up's prefix takes (rhp_scalar.h
 * fixup_piece_whole), else 0; 0 or -22 */
int rhp_test_fixup_whole(const rhp_batch_t *batch, uint8_t *whole);

#ifdef __cplusplus
}
#endif
#endif
