/*
 * messages_host_loop.c -- the host yardstick of tools/bench_messages.py: one
 * phr_parse_response call per message, the messages shared among `threads`
 * host threads in contiguous ranges.  phr_parse_response is whatever library
 * the benchmark links this file with provides (the compiled reference,
 * oracle/_ref/libref.so; its signature: picohttpparser.h).  Returns the number
 * of messages whose ret was > 0.
 */
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>

struct phr_header {
  const char *name;
  size_t name_len;
  const char *value;
  size_t value_len;
};
int phr_parse_response(const char *buf, size_t len, int *minor_version, int *status, const char **msg, size_t *msg_len,
                       struct phr_header *headers, size_t *num_headers, size_t last_len);

struct job {
  const char *bytes;
  const uint64_t *off;
  uint32_t lo, hi, max_headers;
  uint64_t parsed;
};

static void *run(void *arg)
{
  struct job *j = (struct job *) arg;
  struct phr_header h[64];
  for (uint32_t i = j->lo; i < j->hi; i++) {
    int minor, status;
    const char *msg;
    size_t msg_len, nh = j->max_headers;
    j->parsed += phr_parse_response(j->bytes + j->off[i], (size_t) (j->off[i + 1] - j->off[i]), &minor, &status, &msg,
                                    &msg_len, h, &nh, 0) > 0;
  }
  return NULL;
}

uint64_t messages_host_loop(const char *bytes, const uint64_t *off, uint32_t n, uint32_t max_headers, uint32_t threads)
{
  pthread_t t[64];
  struct job j[64];
  if (threads < 1) threads = 1;
  if (threads > 64) threads = 64;
  if (max_headers > 64) max_headers = 64;
  for (uint32_t k = 0; k < threads; k++) {
    j[k] = (struct job){bytes, off, (uint32_t) ((uint64_t) n * k / threads), (uint32_t) ((uint64_t) n * (k + 1) / threads),
                        max_headers, 0};
    pthread_create(&t[k], NULL, run, &j[k]);
  }
  uint64_t parsed = 0;
  for (uint32_t k = 0; k < threads; k++) {
    pthread_join(t[k], NULL);
    parsed += j[k].parsed;
  }
  return parsed;
}
