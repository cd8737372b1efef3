// check_plan.h -- GPU-free arithmetic of memo_ec_check_batch: where the call's
// device scratch lies, the strides its multiply-accumulate launch gets and
// the offsets of a launch span.  Every offset the check's kernels are handed
// comes from here (memo_ec.cpp adds none of its own).  Plain C++17, no HIP
// include: tests/test_check_plan.py builds it into a stand-alone program with
// the host sanitizers and walks every shape before anything runs on a GPU.
//
// A batch of n blocks holds k + x shards of S bytes per block, block-major:
// block b's shard in position t at (b * (k + x) + t) * S.  Positions 0..k-1
// are the basis, k..k+x-1 the spares.
#pragma once
#include <cstddef>
#include <cstdint>

namespace memo_ec {
namespace check {

constexpr size_t kAlign = 256;  // every scratch region starts on this boundary
constexpr uint32_t kTileCols = 256;  // MAC_TILE of ec_kernels.h

inline size_t round_up(size_t b) { return (b + kAlign - 1) & ~(kAlign - 1); }

// The call's device scratch (byte offsets from a 256-byte aligned base):
// the basis and spare indices split out of have_idx by check_prepare_kernel
// (n x k and n x x bytes, what the decode reads as survivors and lost
// shards), then the decode rows (n x x x k bytes).  `total` is a multiple of
// 256, so scratches laid end to end (one per pipeline slot) stay aligned.
struct Scratch {
  size_t basis, spares, rows, total;
};
inline Scratch scratch_layout(size_t n, unsigned k, unsigned x) {
  Scratch s;
  s.basis = 0;
  s.spares = round_up(n * (size_t)k);
  s.rows = s.spares + round_up(n * (size_t)x);
  s.total = s.rows + round_up(n * (size_t)x * k);
  return s;
}

// What the MAC launch of gf_check_kernel gets: the basis shards are its
// inputs, the spares the rows it compares with.
struct Strides {
  uint64_t block;   // bytes between blocks, inputs and spares alike: (k + x) * S
  uint64_t shard;   // bytes between a block's shards: S
  uint64_t spares;  // a block's first spare, from its first basis shard: k * S
  uint64_t rows;    // bytes between blocks' decode rows: x * k
};
inline Strides strides(unsigned k, unsigned x, size_t S) {
  Strides s;
  s.block = (uint64_t)(k + x) * S;
  s.shard = (uint64_t)S;
  s.spares = (uint64_t)k * S;
  s.rows = (uint64_t)x * k;
  return s;
}

// A launch span starting at block b0: its first byte of `have`, of the
// decode rows, and its first verdict word.
struct SpanOff {
  uint64_t have, rows, verdict;
};
inline SpanOff span_offsets(size_t b0, unsigned k, unsigned x, size_t S) {
  const Strides s = strides(k, x, S);
  SpanOff o;
  o.have = (uint64_t)b0 * s.block;
  o.rows = (uint64_t)b0 * s.rows;
  o.verdict = (uint64_t)b0;
  return o;
}

// Blocks one MAC launch takes under a limit of `tile_limit` tiles: a block
// of S-byte shards weighs its whole tiles plus one (a flat tile may straddle
// two blocks).  memo_ec.cpp cuts every uniform call's spans by this rule.
inline size_t span_blocks(size_t S, uint64_t tile_limit) {
  const uint64_t per = ((uint64_t)S / 16 + kTileCols - 1) / kTileCols + 1;
  const uint64_t n = tile_limit / per;
  return (size_t)(n ? n : 1);
}

}  // namespace check
}  // namespace memo_ec
