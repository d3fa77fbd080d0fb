/*
 * split_host_loop.c -- the host scan that rhp_split_sessions replaces, as a
 * loop to time (tools/bench_split.py builds it into tools/libsplit_host_loop.so):
 * the reactor's search for the end of an empty line (reactor/server.c
 * find_empty_line: a memchr that returns at every line end) run over every
 * session of a round, leaving the piece offsets as the reactor's split does.
 */
#include <stdint.h>
#include <string.h>

static const uint8_t *find_empty_line(const uint8_t *p, const uint8_t *end)
{
  while (p < end) {
    const uint8_t *q = memchr(p, '\n', (size_t) (end - p));
    if (!q || q + 1 >= end) return NULL;
    if (q[1] == '\n') return q + 2;
    if (q[1] == '\r' && q + 2 < end && q[2] == '\n') return q + 3;
    p = q + 1;
  }
  return NULL;
}

/* offsets[0 .. pieces] of the sessions bytes[sess_off[s], sess_off[s+1]); returns the pieces */
uint64_t split_host_loop(const uint8_t *bytes, const uint64_t *sess_off, uint32_t n_sessions, uint64_t *offsets)
{
  uint64_t k = 0;
  for (uint32_t s = 0; s < n_sessions; s++) {
    const uint8_t *p = bytes + sess_off[s], *end = bytes + sess_off[s + 1];
    offsets[k++] = sess_off[s];
    while ((p = find_empty_line(p, end)) != NULL && p < end) offsets[k++] = (uint64_t) (p - bytes);
  }
  offsets[k] = sess_off[n_sessions];
  return k;
}
