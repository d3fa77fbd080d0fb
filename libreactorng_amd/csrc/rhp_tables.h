/*
 * rhp_tables.h -- the lookup tables of the classify kernels and what reads
 * them, for the two files whose kernels compare header names with names the
 * host folded once (rhp_classify.hip, rhp_forward.hip): the tables as they
 * travel in a kernel argument, the host's packing of them, the SWAR fold and
 * the compare of a byte range with the candidates' table text.  Everything is
 * local to the including file (an unnamed namespace), as it was when it stood
 * in rhp_classify.hip.
 */
#ifndef RHP_TABLES_H
#define RHP_TABLES_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "rhp.h"

namespace {

constexpr uint32_t kNameDwords = RHP_CLASSIFY_NAME_MAX / 4u;
/* route methods and targets, each starting at a dword and zero-padded to one */
constexpr uint32_t kTextDwords = (RHP_CLASSIFY_TEXT_MAX + 2u * RHP_CLASSIFY_MAX_ROUTES * 3u) / 4u;

struct CTables {
  uint32_t name[RHP_CLASSIFY_MAX_NAMES][kNameDwords];   /* folded to upper case, zero-padded */
  uint32_t text[kTextDwords];
  uint16_t r_moff[RHP_CLASSIFY_MAX_ROUTES], r_mlen[RHP_CLASSIFY_MAX_ROUTES];   /* dword index into text, bytes */
  uint16_t r_toff[RHP_CLASSIFY_MAX_ROUTES], r_tlen[RHP_CLASSIFY_MAX_ROUTES];
  uint8_t  name_len[RHP_CLASSIFY_MAX_NAMES];
};
constexpr uint32_t kTabDwords = sizeof(CTables) / 4u;
static_assert(sizeof(CTables) % 4u == 0 && offsetof(CTables, name_len) % 4u == 0, "copied to LDS as dwords");

/* C-locale toupper of four bytes at once: a byte in 'a'..'z' (bit 7 clear,
 * low seven bits in 0x61..0x7a) loses bit 5, every other byte stays */
__host__ __device__ inline uint32_t fold4(uint32_t x)
{
  const uint32_t x7 = x & 0x7f7f7f7fu;
  const uint32_t ge_a = x7 + 0x1f1f1f1fu, gt_z = x7 + 0x05050505u;   /* bit 7: >= 0x61, >= 0x7b (no carry out of a byte) */
  const uint32_t is = ge_a & ~gt_z & ~x & 0x80808080u;
  return x ^ (is >> 2);
}

/* The candidates of `cand` whose table text equals the len bytes at src:
 * candidate j's text is tab[off(j) ...], zero-padded to a dword.  Reads the
 * aligned dwords that hold the bytes, none past the one with the last byte,
 * and stops at the dword that rejects the last candidate. */
template <bool FOLD, class Off>
__device__ __forceinline__ uint32_t same_text(const uint8_t *src, uint32_t len, uint32_t cand, const uint32_t *tab, Off off)
{
  if (len == 0) return cand;
  const uintptr_t a = (uintptr_t) src;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(a & ~(uintptr_t) 3);
  const uint32_t sh = (uint32_t) a & 3u, nd = (sh + len + 3u) >> 2;
  uint32_t lo = w[0];
  for (uint32_t j = 0; j < len && cand; j += 4) {
    const uint32_t k = (j >> 2) + 1u;
    const uint32_t hi = k < nd ? w[k] : 0u;
    uint32_t x = __builtin_amdgcn_alignbyte(hi, lo, sh);
    if (len - j < 4u) x &= (1u << (8u * (len - j))) - 1u;
    if (FOLD) x = fold4(x);
    for (uint32_t c = cand; c; c &= c - 1u) {
      const uint32_t q = (uint32_t) __builtin_ctz(c);
      if (tab[off(q) + (j >> 2)] != x) cand &= ~(1u << q);
    }
    lo = hi;
  }
  return cand;
}

typedef __attribute__((address_space(4))) uint32_t ka32;   /* a dword of the kernel argument segment */

/* row j of the tables' names: the len bytes at s, folded to upper case */
inline void pack_name(CTables &t, uint32_t j, const uint8_t *s, uint32_t len)
{
  uint8_t *d = reinterpret_cast<uint8_t *>(t.name[j]);
  for (uint32_t q = 0; q < len; q++) d[q] = s[q] >= 'a' && s[q] <= 'z' ? (uint8_t) (s[q] - 0x20) : s[q];
  t.name_len[j] = (uint8_t) len;
}

/* the caller's tables as the kernel's: names folded, route text packed */
inline void pack_tables(const rhp_classify_t *c, CTables &t)
{
  memset(&t, 0, sizeof t);
  for (uint32_t j = 0; j < c->n_names; j++) pack_name(t, j, c->text + c->names[j].off, c->names[j].len);
  uint32_t at = 0;   /* dwords of t.text in use */
  uint8_t *d = reinterpret_cast<uint8_t *>(t.text);
  for (uint32_t r = 0; r < c->n_routes; r++) {
    const rhp_span_t sp[2] = {c->routes[r].method, c->routes[r].target};
    uint16_t off[2];
    for (int q = 0; q < 2; q++) {
      off[q] = (uint16_t) at;
      memcpy(d + 4u * at, c->text + sp[q].off, sp[q].len);
      at += (sp[q].len + 3u) >> 2;
    }
    t.r_moff[r] = off[0];
    t.r_mlen[r] = (uint16_t) sp[0].len;
    t.r_toff[r] = off[1];
    t.r_tlen[r] = (uint16_t) sp[1].len;
  }
}

}  // namespace

#endif
