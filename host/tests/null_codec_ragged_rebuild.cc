// null_codec_ragged_rebuild.cc -- the ragged rebuild of the libmemo_ec TEST
// DOUBLE (null_codec.cc, which see): the rebuilt shards written as zeros.
// Linked into host/_build/hostprof/ only.
#include <cstring>

#include "../../include/memo_ec.h"

extern "C" {
int memo_ec_rebuild_ragged(memo_ec_ctx*, int, int, size_t n, const size_t* sizes, const uint8_t*,
                           const uint8_t*, const uint8_t*, int e, int, uint8_t* out, int) {
  size_t T = 0;
  for (size_t b = 0; b < n; ++b) T += sizes[b];
  if (T && e > 0) std::memset(out, 0, (size_t)e * T);
  return MEMO_EC_OK;
}
}
