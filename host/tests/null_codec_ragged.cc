// null_codec_ragged.cc -- the ragged calls of the libmemo_ec TEST DOUBLE
// (null_codec.cc, which see): parity written as zeros, every block
// "consistent".  Linked into host/_build/hostprof/ only.
#include <cstring>

#include "../../include/memo_ec.h"

extern "C" {
int memo_ec_encode_ragged(memo_ec_ctx*, int, int m, size_t n, const size_t* sizes, const uint8_t*,
                          uint8_t* parity, int) {
  size_t T = 0;
  for (size_t b = 0; b < n; ++b) T += sizes[b];
  if (T) std::memset(parity, 0, (size_t)m * T);
  return MEMO_EC_OK;
}
int memo_ec_verify_ragged(memo_ec_ctx*, int, int, size_t n, const size_t*, const uint8_t*,
                          const uint8_t*, uint32_t* verdict, int) {
  if (n) std::memset(verdict, 0, n * sizeof(uint32_t));
  return MEMO_EC_OK;
}
}
