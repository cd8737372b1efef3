// correct_pair_plan.h -- GPU-free arithmetic of memo_ec_correct_pair_batch:
// where the call's device scratch lies (memo_ec_correct_batch's, a second
// count word, the list of the pair blocks), what a pair entry holds, which k
// positions of a block the rebuild of its two named shards reads, which decode
// rows its coefficients come from and where the two shards are written.  Every
// offset the pair correction's kernels use comes from here or from
// correct_plan.h (memo_ec.cpp and ec_kernels.hip add none of their own).
// Plain C++17, no HIP include; the functions the kernels call are constexpr.
// tests/test_correct_pair_plan.py builds the header into a stand-alone program
// with the host sanitizers and walks every shape before anything runs on a GPU.
//
// The batch is memo_ec_check_batch's: n blocks of k + x shards of S bytes,
// block-major, positions 0..k-1 the basis, k..k+x-1 the spares.  A pair
// block's wrong shards sit in positions qa < qb (x >= 3).  Their new bytes are
// a two-row multiply-accumulate over k input positions that are neither
// target: input slot j is basis position j, and the slot of a basis target is
// filled by the lowest spare positions that are no target, in ascending order.
// Those spares are the "clean rows": their decode rows tie the inputs to the
// targets.
//   qa, qb >= k          the basis as it stands; rows qa - k and qb - k
//   qa < k <= qb         spare c in slot qa, c = 0 unless qb == k, then 1
//   qa < qb < k          spare 0 in slot qa, spare 1 in slot qb
#pragma once
#include <cstddef>
#include <cstdint>

#include "correct_plan.h"

namespace memo_ec {
namespace correct_pair {

// The call's device scratch (byte offsets from a 256-byte aligned base):
// memo_ec_correct_batch's scratch unmoved, a second count word on a boundary
// of its own, the pair list of up to n 8-byte entries.  `total` is a multiple
// of 256.
struct Scratch {
  correct::Scratch one;
  size_t count, list, total;
};
inline Scratch scratch_layout(size_t n, unsigned k, unsigned x) {
  Scratch s;
  s.one = correct::scratch_layout(n, k, x);
  s.count = s.one.total;
  s.list = s.count + check::kAlign;
  s.total = s.list + check::round_up(n * sizeof(uint64_t));
  return s;
}

// A pair entry: block index in bits 0..47, position qa in bits 48..55,
// position qb in bits 56..63 (qa < qb).
constexpr uint64_t make_entry(uint64_t block, uint32_t qa, uint32_t qb) {
  return (block & correct::kBlockMask) | ((uint64_t)(qa & 0xFFu) << 48) | ((uint64_t)(qb & 0xFFu) << 56);
}
constexpr uint64_t entry_block(uint64_t e) { return e & correct::kBlockMask; }
constexpr uint32_t entry_qa(uint64_t e) { return (uint32_t)(e >> 48) & 0xFFu; }
constexpr uint32_t entry_qb(uint64_t e) { return (uint32_t)(e >> 56) & 0xFFu; }

// Does a verdict word name a pair (bits 25..31 nonzero, not
// MEMO_EC_VERDICT_INVALID)?
constexpr bool names_pair(uint32_t word) { return word != 0xFFFFFFFFu && (word >> 25) != 0u; }

// Is spare row r the row of a target?
constexpr bool row_is_target(uint32_t r, uint32_t qa, uint32_t qb, uint32_t k) {
  return k + r == qa || k + r == qb;
}
// Clean row i (i < 2): the i-th spare row, ascending, that is no target.  With
// x >= 3 and at most two targets both exist whenever they are asked for (row
// i is asked for only when at least i + 1 targets are basis shards).
constexpr uint32_t first_clean_row(uint32_t qa, uint32_t qb, uint32_t k) {
  uint32_t r = 0;
  while (row_is_target(r, qa, qb, k)) ++r;
  return r;
}
constexpr uint32_t clean_row(uint32_t i, uint32_t qa, uint32_t qb, uint32_t k) {
  uint32_t r = first_clean_row(qa, qb, k);
  if (i == 0) return r;
  ++r;
  while (row_is_target(r, qa, qb, k)) ++r;
  return r;
}

// The position input slot j (j < k) is read from.
constexpr uint32_t input_pos(uint32_t j, uint32_t qa, uint32_t qb, uint32_t k) {
  if (j == qa) return k + clean_row(0, qa, qb, k);  // qa < qb: a basis qb means a basis qa
  if (j == qb) return k + clean_row(1, qa, qb, k);
  return j;
}

// The decode row of output i (i < 2) when both targets are spares.
constexpr uint32_t spare_row(uint32_t i, uint32_t qa, uint32_t qb, uint32_t k) { return (i ? qb : qa) - k; }

// First byte of decode row r of block b in the rows region (x rows of k bytes
// per block).
constexpr uint64_t row_off(uint64_t b, uint32_t r, uint32_t k, uint32_t x) {
  return b * ((uint64_t)x * k) + (uint64_t)r * k;
}

// Byte offset into `have` of target i (0: qa, 1: qb) of block b.
constexpr uint64_t target_off(uint64_t b, uint32_t i, uint32_t qa, uint32_t qb, uint32_t k, uint32_t x,
                              uint64_t S) {
  return correct::shard_off(b, i ? qb : qa, k, x, S);
}
// ... and of input slot j.
constexpr uint64_t input_off(uint64_t b, uint32_t j, uint32_t qa, uint32_t qb, uint32_t k, uint32_t x,
                             uint64_t S) {
  return correct::shard_off(b, input_pos(j, qa, qb, k), k, x, S);
}

// Work items are (entry, 4 KiB tile), dealt to the workgroups in contiguous
// ranges: correct::tiles_per_block, work_items, item_of, wg_items, col_off.
// The two grids are the single correction's too.
constexpr uint32_t grid_for(uint64_t n, uint64_t S) { return correct::grid_for(n, S); }
constexpr uint32_t list_grid_for(uint64_t n) { return correct::list_grid_for(n); }

}  // namespace correct_pair
}  // namespace memo_ec
