/*
 * rhp_digits.h -- the decimal digit count of a Content-Length (http_u32_len,
 * src/reactor/http.c:8-15), one statement of it for the relay's kernels
 * (rhp_classify.hip) and the relay's host twin (rhp_host.cpp), both through
 * rhp_relay_args.h.  rhp_writer.hip keeps its table-driven u32_len: with this one
 * its two kernels compile to other register counts.
 */
#ifndef RHP_DIGITS_H
#define RHP_DIGITS_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RHP_DIGITS_HD __host__ __device__ __forceinline__
#else
#define RHP_DIGITS_HD static inline
#endif

RHP_DIGITS_HD uint32_t rhp_u32_len(uint32_t v)
{
  uint32_t l = 1;
  for (uint32_t p = 10; l < 10 && v >= p; p *= 10u) l++;   /* (l == 10 ends the loop before p would wrap) */
  return l;
}

#endif
