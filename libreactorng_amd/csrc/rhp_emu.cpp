/*
 * rhp_emu.cpp -- CPU emulation of rhp_dfa_kernel, for tests only (and the
 * rhp_test_* hooks).
 *
 * Runs the same pair transition table (rhp_dfa.h Table2), windows starting in the
 * same S_PRE state with the bytes before the request zeroed (a request whose
 * first byte is of their class goes to the exact path, as in the kernel; the
 * same window geometry: phr mode's first windows start at the 128-byte line
 * holding the request, http mode's at its dword), the same blocks with one
 * event-mask decode per block
 * (rhp_dfa.h dec_event) and the same finalize decisions as the kernel, one
 * request at a time on the host.  Lets the DFA design be checked against
 * the oracle on millions of requests without a GPU; the GPU tests then check
 * the kernel itself.  Where the records go and how they are encoded is
 * rhp_records.h's; the exact path is the host library's (rhp_host.cpp).
 */
#include <stdint.h>
#include <string.h>

#include "rhp.h"
#include "rhp_host.h"
#include "rhp_records.h"
#include "rhp_dfa.h"
#include "rhp_scalar.h"
#include "rhp_host_exact.h"

using namespace rhp;

static_assert(RHP_BLOCK == 128, "the emulator walks the kernel's 128-byte windows");

namespace {

const Table2 &table()
{
  static const Table2 t = make_table2();
  return t;
}

struct Stats {
  uint64_t fast_ok, fast_bad, exact;
};

}  // namespace

extern "C" int rhp_emu_parse_batch(const rhp_batch_t *b, uint64_t *stats /* [3] or NULL */)
{
  if (rhp_batch_check(b, 0) < 0) return -22;
  const rhp_view_t v = rhp_batch_view(b);
  const Table2 &T = table();
  const uint8_t *cls = T.b + kClassRow * 256u;
  Stats st_count = {0, 0, 0};
  const uint32_t maxh = b->max_headers;
  const bool dense = v.dreq != nullptr, lens = rhp_layout_lens(b->layout);   /* header records as lengths */

  for (uint32_t i = 0; i < b->n; i++) {
    const uint64_t off = b->offsets[i], len = b->offsets[i + 1] - off;
    /* the kernel's first window: from the 128-byte line (phr mode) or the dword
     * (http mode) holding the request's first byte, offsets from the batch's
     * bytes.  The geometry decides, in rare cases, whether the DFA path or the
     * exact path answers (a max_headers overflow whose colon lies in the window
     * that also holds a SLOW, or lies past len): the flags follow it, the
     * answers do not */
    const uint32_t mis = (uint32_t) off & (b->mode == RHP_MODE_PHR ? 127u : 3u);
    const uint8_t *win = b->bytes + (off - mis);
    int32_t pos = -(int32_t) mis;
    uint32_t st = idx2(byte_class_ctlx(b->bytes[off]) ? S_SLOW : S_PRE, 0);
    Dec d;
    dec_reset(d);
    rhp_hdr_t *hout = v.hdrs + i * v.hs_req;   /* the rhp_hdr_t records (no length layout) */
    /* the kernel's window, in both modes */
    constexpr int32_t block = RHP_BLOCK;
    constexpr int words = block / 32;
    for (;;) {
      /* one window: steps, then the decode of its event mask (32 bytes per word) */
      const int32_t block_pos = pos;
      uint32_t evw[words];
      for (int w = 0; w < words; w++) {
        uint32_t ev = 0;
        for (int k = 0; k < 32; k += 2) {   /* one table read per byte pair */
          const int32_t at = block_pos + 32 * w + k;   /* the bytes before the request read as 0 */
          st = T.b[st * kStride + (at < 0 ? 0u : cls[win[32 * w + k]]) * 16u + (at + 1 < 0 ? 0u : cls[win[32 * w + k + 1]])];
          ev |= (st & 3u) << k;
        }
        evw[w] = ev;
      }
      win += block;
      pos += block;
      const bool slow = is_slow2(st);
      const bool term_ev = is_done2(st) || is_err2(st);
      uint32_t term_pos = 0xffffffffu;
      if (term_ev) {   /* the terminal is the window's last event */
        for (int w = words - 1; w >= 0; w--)
          if (evw[w]) {
            const uint32_t bt = 31u - (uint32_t) __builtin_clz(evw[w]);
            term_pos = (uint32_t) (block_pos + 32 * w) + bt;
            evw[w] &= ~(1u << bt);
            break;
          }
      }
      for (int w = 0; w < words && !slow; w++) {
        uint32_t m = evw[w];
        while (m && !d.ovf) {
          const uint32_t bit = (uint32_t) __builtin_ctz(m);
          m &= m - 1;
          uint32_t lo, hi;
          if (dec_event(d, (uint32_t) (block_pos + 32 * w) + bit, maxh, lo, hi)) {
            if (lens) {   /* as the kernel: the two lengths (rhp.h RHP_LAYOUT_COMPACT, RHP_LAYOUT_DENSE) */
              rhp_view_put_len(&v, i, d.nh - 1, lo >> 16, hi >> 16);
            } else {
              rhp_hdr_t &o = hout[(uint64_t) (d.nh - 1) * v.hs_hdr];
              o.name_off = (uint16_t) lo;
              o.name_len = (uint16_t) (lo >> 16);
              o.value_off = (uint16_t) hi;
              o.value_len = (uint16_t) (hi >> 16);
            }
          }
        }
      }
      const bool ovf = d.ovf != 0;
      if (!(ovf || slow || term_ev || pos >= (int32_t) len)) continue;
      /* ---- finalize (same decisions as the kernel) ---- */
      bool ok = !ovf && is_done2(st) && term_pos < len && term_pos < RHP_MAX_LEN;
      /* an ERR in the version (request line events ME, PE consumed) needs the
       * version's 9 bytes: len >= PE + 10 (picohttpparser.c:248-251) */
      bool bad = ovf ? d.ovf - 1u < len
                     : (is_err2(st) && term_pos < len && (d.k != 2 || d.e[0] + 10u <= len));
      if (b->mode == RHP_MODE_PHR && b->last_len && b->last_len[i] != 0) {   /* as the kernel's decode_end */
        ok = ok && (b->last_len[i] < 3u || b->last_len[i] <= term_pos);
        bad = false;
      }
      if (ok && dense && (d.rl01 & 0xffffu) > 255u) {
        /* as the kernel: a method longer than the dense record holds takes the exact path (wide) */
        st_count.exact++;
        host_exact(b, v, i, off, len);
        break;
      }
      if (ok) {
        st_count.fast_ok++;
        rhp_req_t r;
        r.ret = (int32_t) term_pos + 1;
        r.method_off = 0;
        r.method_len = (uint16_t) d.rl01;
        r.path_off = (uint16_t) (d.rl01 >> 16);
        r.path_len = (uint16_t) d.rl23;
        r.minor_version = (int8_t) (d.rl23 >> 16);
        r.num_headers = (uint16_t) d.nh;
        r.flags = 0;
        if (dense) v.dreq[i] = rhp_req_dense_encode(&r);
        else v.reqs[i] = r;
        if (b->mode == RHP_MODE_HTTP && lens) {
          /* as the kernel: with compact records a request that is not GET and
           * has three or more framing candidates (names of 14 or 17 bytes), or
           * one at header index >= 30, is framed by the exact path (its http_frame
           * has no rhp_hdr_t records to read) */
          uint32_t ncand = 0;
          bool late = false;
          for (uint32_t k = 0; k < d.nh && k < maxh; k++) {
            const uint32_t nl = rhp_view_len32(&v, i, k) & 0xffffu;
            if (nl == 14u || nl == 17u) {
              ncand++;
              late |= k >= 30u;
            }
          }
          const bool get = len >= 4 && memcmp(b->bytes + off, "GET ", 4) == 0;
          if (!get && (ncand >= 3 || late)) {
            st_count.fast_ok--;
            st_count.exact++;
            host_exact(b, v, i, off, len);
            break;
          }
        }
        if (b->mode == RHP_MODE_HTTP) {
          rhp_http_t x;
          if (lens) {   /* http_frame reads rhp_hdr_t records: the lengths expanded */
            rhp_hdr_t tmp[RHP_MAX_HEADERS];
            uint32_t at = rhp_hdr_first(&r);
            for (uint32_t k = 0; k < d.nh && k < maxh; k++) tmp[k] = rhp_hdr_next(&at, rhp_view_len32(&v, i, k));
            http_frame(b->bytes_rw + off, len, r, tmp, 1u, &x, ~0ull, !(b->flags & RHP_BATCH_SPECULATIVE));
          } else {
            http_frame(b->bytes_rw + off, len, r, hout, v.hs_hdr, &x, ~0ull, !(b->flags & RHP_BATCH_SPECULATIVE));
          }
          host_put_http(v, i, x, !rhp_http_compact_fits(r.ret, &x));
        }
      } else if (bad) {
        st_count.fast_bad++;
        rhp_req_t r;
        memset(&r, 0, sizeof r);
        r.ret = -1;
        r.minor_version = -1;
        if (dense) v.dreq[i] = rhp_req_dense_mark(RHP_DENSE_BAD);
        else v.reqs[i] = r;
        if (b->mode == RHP_MODE_HTTP) {
          rhp_http_t x;
          memset(&x, 0, sizeof x);
          x.result = -1;
          host_put_http(v, i, x, false);
        }
      } else {
        st_count.exact++;
        host_exact(b, v, i, off, len);
      }
      break;
    }
  }
  if (stats) {
    stats[0] = st_count.fast_ok;
    stats[1] = st_count.fast_bad;
    stats[2] = st_count.exact;
  }
  return 0;
}

/* test hook: rhp_fixup_kernel's work per session on the host (as
 * rhp_cpu_fixup_sessions, which walks every session from its first piece):
 * the prefix of whole pieces taken kFixupStep per step by the kernel's own
 * predicate and stop rule (rhp_scalar.h), the lanes of a step in a loop, then
 * the walk from the first other piece. */
extern "C" int rhp_emu_fixup_sessions(const rhp_batch_t *b, const rhp_session_t *sessions, uint32_t n_sessions,
                                      rhp_session_result_t *results, uint64_t *req_start)
{
  if (!b || b->mode != RHP_MODE_HTTP || !(b->flags & RHP_BATCH_SPECULATIVE)) return -22;
  const rhp_view_t v = rhp_batch_view(b);
  const FixupIO io{b->bytes_rw, b->offsets, v.reqs, v.hdrs, v.http, v.hs_req, v.hs_hdr, b->max_headers};
  for (uint32_t k = 0; k < n_sessions; k++) {
    const rhp_session_t ss = sessions[k];
    uint32_t from = ss.piece_lo;
    while (from < ss.piece_hi) {
      uint64_t a[kFixupStep], other = 0;
      for (uint32_t lane = 0; lane < kFixupStep; lane++)
        other |= (uint64_t) fixup_lane_other(io.http, io.off, from + lane, ss.piece_hi, &a[lane]) << lane;
      const uint32_t stop = fixup_step_stop(from, ss.piece_hi, other);
      for (uint32_t lane = 0; lane < kFixupStep && from + lane < stop; lane++) req_start[from + lane] = a[lane];
      from = stop;
      if (other) break;
    }
    fixup_session_t(io, ss.piece_lo, ss.piece_hi, req_start, &results[k],
                    [&](uint64_t at) { return PlainBytes{b->bytes_rw + at}; }, PlainDechunk(), from);
  }
  return 0;
}

/* test hook: fixup_piece_whole (rhp_scalar.h) of every piece of a parsed
 * speculative batch, whole[j] = 0 / 1 */
extern "C" int rhp_test_fixup_whole(const rhp_batch_t *b, uint8_t *whole)
{
  if (!b || b->mode != RHP_MODE_HTTP || !(b->flags & RHP_BATCH_SPECULATIVE)) return -22;
  const rhp_view_t v = rhp_batch_view(b);
  for (uint32_t j = 0; j < b->n; j++) whole[j] = fixup_piece_whole(v.http[j], b->offsets[j + 1] - b->offsets[j]) ? 1 : 0;
  return 0;
}

/* test hook: one_chunk_window over the nw (<= 32) bytes at `line`
 * (tests/test_cpu_units.py compares it with one_chunk_t); returns 0 when the
 * window cannot decide */
extern "C" int rhp_test_chunk_window(const uint8_t *line, uint32_t nw, uint64_t avail, int64_t *res, uint64_t *doff,
                                     uint64_t *dlen)
{
  uint32_t W[8];
  memcpy(W, line, 32);
  return one_chunk_window(W, nw, avail, res, doff, dlen) ? 1 : 0;
}

/* test hook: one_chunk_head over the first 4 * nd bytes at `line` (nd 5: the
 * GPU replay's 20-byte window, or 8); returns 0 when it leaves the line to
 * one_chunk_window */
extern "C" int rhp_test_chunk_head(const uint8_t *line, uint32_t nw, uint64_t avail, int64_t *res, uint64_t *doff,
                                   uint64_t *dlen, uint32_t nd)
{
  uint32_t W[8];
  memcpy(W, line, 32);
  return (nd == 5 ? one_chunk_head<5>(W, nw, avail, res, doff, dlen) : one_chunk_head<8>(W, nw, avail, res, doff, dlen))
             ? 1 : 0;
}

/* test hook: the pair table the kernel copies into LDS (rhp_dfa.h make_table2)
 * and its geometry: meta = {bytes, row stride, kClassRowR, kClassRow, idx2(S_SLOW, 1), kClassRow16} */
extern "C" uint32_t rhp_test_table2(uint8_t *out, uint32_t *meta)
{
  const Table2 &t = table();
  if (out) memcpy(out, t.b, kTable2Bytes);
  if (meta) {
    meta[0] = kTable2Bytes;
    meta[1] = kStride;
    meta[2] = kClassRowR;
    meta[3] = kClassRow;
    meta[4] = idx2(S_SLOW, 1);
    meta[5] = kClassRow16;
  }
  return kTable2Bytes;
}

/* test hook: one_chunk_t over `body` (size bytes, readable to size + 64) */
extern "C" int64_t rhp_test_chunk_exact(const uint8_t *body, uint64_t at, uint64_t size, uint64_t *doff, uint64_t *dlen)
{
  PlainBytes B{body};
  return one_chunk_t(B, at, size, doff, dlen);
}
