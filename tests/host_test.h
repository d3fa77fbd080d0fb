/*
 * host_test.h -- what the stand-alone host programs (the _host_test.c files here) share:
 * FAIL, the reader of a golden .npz file (npz_open, npz_array, LOAD), all_poison,
 * the sanitizer's POISON / UNPOISON, and state_of for the resumed walks.
 *
 * A program states its name once, before the include:
 *
 *   #define HOST_TEST_NAME "walk_responses_host_test"
 *   #include "host_test.h"
 *
 * Everything here is static: each program is one translation unit of its own.
 */
#ifndef HOST_TEST_H
#define HOST_TEST_H

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rhp.h"

#ifndef HOST_TEST_NAME
#error "define HOST_TEST_NAME, the program's name in its messages, before including host_test.h"
#endif

/* One line on stdout with the program's name in front; the calling function returns 1. */
#define FAIL(...) do { printf(HOST_TEST_NAME ": " __VA_ARGS__); printf("\n"); return 1; } while (0)

/* A region no code may touch until UNPOISON (ASan builds; nothing otherwise). */
#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void) (p), (void) (n))
#define UNPOISON(p, n) ((void) (p), (void) (n))
#endif

/* The golden file that npz_array reads: all of it, in one allocation.  A function that reads a second file
 * keeps both values, calls npz_open, and frees g_file and puts them back when it is done. */
static uint8_t *g_file;
static size_t g_size;

static inline uint32_t rd16(const uint8_t *p) { return (uint32_t) p[0] | (uint32_t) p[1] << 8; }
static inline uint32_t rd32(const uint8_t *p) { return rd16(p) | rd16(p + 2) << 16; }
static inline uint64_t rd64(const uint8_t *p) { return (uint64_t) rd32(p) | (uint64_t) rd32(p + 4) << 32; }

/* `path` read whole into g_file / g_size; non-zero (after a FAIL line): it cannot be opened or read. */
static inline int npz_open(const char *path)
{
  FILE *fp = fopen(path, "rb");
  if (!fp) FAIL("cannot open %s", path);
  fseek(fp, 0, SEEK_END);
  g_size = (size_t) ftell(fp);
  fseek(fp, 0, SEEK_SET);
  g_file = (uint8_t *) malloc(g_size);
  if (!g_file || fread(g_file, 1, g_size, fp) != g_size) FAIL("cannot read %s", path);
  fclose(fp);
  return 0;
}

/* The data of member `name`.npy of the stored (not compressed) zip in g_file,
 * copied into an allocation of exactly its size; *count = its elements of
 * `elem` bytes, whose dtype string must be `descr`.  NULL: not found / not
 * understood. */
static inline void *npz_array(const char *name, const char *descr, size_t elem, size_t *count)
{
  char want[64];
  snprintf(want, sizeof want, "%s.npy", name);
  size_t at = 0;
  while (at + 30 <= g_size && rd32(g_file + at) == 0x04034b50u) {   /* a local file header */
    const uint8_t *h = g_file + at;
    const uint32_t flags = rd16(h + 6), method = rd16(h + 8), nlen = rd16(h + 26), xlen = rd16(h + 28);
    uint64_t csize = rd32(h + 18), usize = rd32(h + 22);
    if (at + 30 + nlen + xlen > g_size) return NULL;
    const uint8_t *x = h + 30 + nlen;
    for (uint32_t q = 0; q + 4 <= xlen;) {   /* zip64: the sizes are in the extra field */
      const uint32_t id = rd16(x + q), len = rd16(x + q + 2);
      if (q + 4 + len > xlen) return NULL;
      if (id == 1 && len >= 16 && usize == 0xffffffffu) {
        usize = rd64(x + q + 4);
        csize = rd64(x + q + 12);
      }
      q += 4 + len;
    }
    const size_t data = at + 30 + nlen + xlen;
    if ((flags & 8u) || method != 0 || csize != usize || csize > g_size - data) return NULL;
    if (nlen == strlen(want) && memcmp(h + 30, want, nlen) == 0) {
      const uint8_t *d = g_file + data;
      if (usize < 12 || memcmp(d, "\x93NUMPY", 6) != 0) return NULL;
      const size_t hl = d[6] == 1 ? 10 + rd16(d + 8) : 12 + rd32(d + 8);
      if (hl > usize) return NULL;
      char head[512];
      const size_t tl = hl < sizeof head ? hl : sizeof head - 1;
      memcpy(head, d, tl);
      for (size_t i = 0; i < tl; i++) if (!head[i]) head[i] = ' ';
      head[tl] = 0;
      if (!strstr(head + 10, descr) || strstr(head + 10, "'fortran_order': True")) return NULL;
      const size_t bytes = (size_t) usize - hl;
      if (bytes % elem) return NULL;
      *count = bytes / elem;
      void *out = malloc(bytes ? bytes : 1);
      if (out && bytes) memcpy(out, d + hl, bytes);
      return out;
    }
    at = data + (size_t) csize;
  }
  return NULL;
}

/* `type *var` and `size_t n_var`: array `var` of the open file; `path` (the file's, in scope) goes into the message. */
#define LOAD(var, type, descr) \
  size_t n_##var = 0; \
  type *var = (type *) npz_array(#var, descr, sizeof(type), &n_##var); \
  if (!var) FAIL("%s: array '%s' (%s) not found", path, #var, descr)

/* every one of the n bytes at p still holds 0xC3, what the programs fill their outputs with */
static inline int all_poison(const void *p, size_t n)
{
  for (size_t i = 0; i < n; i++) if (((const uint8_t *) p)[i] != 0xC3) return 0;
  return 1;
}

/* the state a golden file of the resumed walks holds for session-round q, or `in` where it says kept */
static inline rhp_walk_state_t state_of(const uint8_t *kept, const uint8_t *phase, const uint8_t *ct, const uint8_t *hex,
                                        const uint8_t *st, const uint64_t *left, size_t q, rhp_walk_state_t in)
{
  if (kept[q]) return in;
  rhp_walk_state_t s;
  memset(&s, 0, sizeof s);
  s.phase = phase[q];
  if (s.phase == RHP_WALK_IN_LENGTH) s.left = left[q];
  if (s.phase == RHP_WALK_IN_CHUNKED) s.decoder.bytes_left_in_chunk = left[q];
  s.decoder.consume_trailer = ct[q];
  s.decoder.hex_count = hex[q];
  s.decoder.state = st[q];
  return s;
}

#endif
