/*
 * decode_chunked_host_loop.c -- the host yardstick of
 * tools/bench_decode_chunked.py: one phr_decode_chunked call per stream on its
 * piece, in place, the streams shared among `threads` host threads in
 * contiguous ranges.  phr_decode_chunked is whatever library the benchmark
 * links this file with provides (the compiled reference, oracle/_ref/libref.so;
 * its signature and its decoder: picohttpparser.h).  ret[i] and size[i] are
 * left for the caller to compare; returns the sum of the decoded sizes.
 */
#include <pthread.h>
#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>

struct phr_chunked_decoder {
  size_t bytes_left_in_chunk;
  char consume_trailer;
  char _hex_count;
  char _state;
};
ssize_t phr_decode_chunked(struct phr_chunked_decoder *decoder, char *buf, size_t *bufsz);

struct job {
  char *bytes;
  const uint64_t *off;
  struct phr_chunked_decoder *dec;
  int64_t *ret;
  uint64_t *size;
  uint32_t lo, hi;
  uint64_t decoded;
};

static void *run(void *arg)
{
  struct job *j = (struct job *) arg;
  for (uint32_t i = j->lo; i < j->hi; i++) {
    size_t sz = (size_t) (j->off[i + 1] - j->off[i]);
    j->ret[i] = phr_decode_chunked(&j->dec[i], j->bytes + j->off[i], &sz);
    j->size[i] = sz;
    j->decoded += sz;
  }
  return NULL;
}

uint64_t decode_chunked_host_loop(char *bytes, const uint64_t *off, void *decoders, int64_t *ret, uint64_t *size, uint32_t n,
                                  uint32_t threads)
{
  pthread_t t[64];
  struct job j[64];
  if (threads < 1) threads = 1;
  if (threads > 64) threads = 64;
  for (uint32_t k = 0; k < threads; k++) {
    j[k] = (struct job){bytes, off, (struct phr_chunked_decoder *) decoders, ret, size, (uint32_t) ((uint64_t) n * k / threads),
                        (uint32_t) ((uint64_t) n * (k + 1) / threads), 0};
    pthread_create(&t[k], NULL, run, &j[k]);
  }
  uint64_t decoded = 0;
  for (uint32_t k = 0; k < threads; k++) {
    pthread_join(t[k], NULL);
    decoded += j[k].decoded;
  }
  return decoded;
}
