/*
 * rhp_host_exact.h -- internal to librhp_host.so: the exact path for one
 * request of a host batch (rhp_host.cpp), which rhp_cpu_parse_batch runs for
 * every request and the emulator (rhp_emu.cpp) where the kernel would.
 */
#ifndef RHP_HOST_EXACT_H
#define RHP_HOST_EXACT_H

#include "rhp.h"
#include "rhp_records.h"

/* not part of librhp_host.so's surface */
#define RHP_INTERNAL __attribute__((visibility("hidden")))

namespace rhp {

/* request i's http record: x itself, or with compact records (v.hc) the compact
 * one, `wide` sending x to the wide area */
RHP_INTERNAL void host_put_http(const rhp_view_t &v, uint32_t i, const rhp_http_t &x, bool wide);
/* request i = bytes [off, off + len) parsed by the scalar parser (rhp_scalar.h),
 * its records the wide ones of the batch's layout; v is rhp_batch_view(b) */
RHP_INTERNAL void host_exact(const rhp_batch_t *b, const rhp_view_t &v, uint32_t i, uint64_t off, uint64_t len);

}  // namespace rhp

#endif
