// correct_plan.h -- GPU-free arithmetic of memo_ec_correct_batch: where the
// call's device scratch lies (the check's, a count word, the work list), what
// a list entry holds, how the correction kernel's work items map to (entry,
// tile), which items a workgroup takes and every byte offset a work item
// reads or writes.  Every offset the correction's kernels use comes from here
// (memo_ec.cpp and ec_kernels.hip add none of their own).  Plain C++17, no
// HIP include; the functions the kernels call are constexpr, so they compile
// for the device as they stand.  tests/test_correct_plan.py builds the header
// into a stand-alone program with the host sanitizers and walks every shape
// before anything runs on a GPU.
//
// The batch is memo_ec_check_batch's: n blocks of k + x shards of S bytes,
// block-major, positions 0..k-1 the basis, k..k+x-1 the spares.  A located
// block's wrong shard sits in position q; its new bytes are a one-row
// multiply-accumulate over k input shards that never reads position q:
//   q >= k: row q - k of the block's decode rows D over the basis;
//   q <  k: row 0 scaled by 1 / D[0][q], with spare 0 standing in for basis q
//           (coefficient 1 / D[0][q]).
#pragma once
#include <cstddef>
#include <cstdint>

#include "check_plan.h"

namespace memo_ec {
namespace correct {

constexpr uint32_t kTileBytes = 4096;  // one work item: 256 lanes x 16 bytes of the target shard
constexpr uint32_t kLaneBytes = 16;
constexpr uint32_t kGridCap = 2048;    // workgroups of the correction kernel at most
constexpr uint32_t kListGridCap = 1024;  // workgroups of the list kernel at most
constexpr uint64_t kBlockMask = ((uint64_t)1 << 48) - 1;

// The call's device scratch (byte offsets from a 256-byte aligned base): the
// check's scratch, a count word on a boundary of its own, the work list of up
// to n 8-byte entries.  `total` is a multiple of 256, as the check's.
struct Scratch {
  check::Scratch chk;
  size_t count, list, total;
};
inline Scratch scratch_layout(size_t n, unsigned k, unsigned x) {
  Scratch s;
  s.chk = check::scratch_layout(n, k, x);
  s.count = s.chk.total;
  s.list = s.count + check::kAlign;
  s.total = s.list + check::round_up(n * sizeof(uint64_t));
  return s;
}

// A list entry: block index in bits 0..47, position q in bits 48..55.
constexpr uint64_t make_entry(uint64_t block, uint32_t q) {
  return (block & kBlockMask) | ((uint64_t)(q & 0xFFu) << 48);
}
constexpr uint64_t entry_block(uint64_t e) { return e & kBlockMask; }
constexpr uint32_t entry_pos(uint64_t e) { return (uint32_t)(e >> 48) & 0xFFu; }

// Tiles of one target shard: ceil(S / 4096).
constexpr uint64_t tiles_per_block(uint64_t S) { return (S + kTileBytes - 1) / kTileBytes; }

// Work items of `count` list entries, and item w's (entry, tile).
constexpr uint64_t work_items(uint64_t count, uint64_t tpb) { return count * tpb; }
struct Item {
  uint64_t entry, tile;
};
constexpr Item item_of(uint64_t w, uint64_t tpb) { return Item{w / tpb, w % tpb}; }

// The items workgroup wg of `grid` takes: a contiguous range, so that the
// consecutive tiles of one entry share the images a workgroup built.
struct ItemRange {
  uint64_t first, end;
};
constexpr ItemRange wg_items(uint64_t total, uint32_t grid, uint32_t wg) {
  const uint64_t per = (total + grid - 1) / grid;
  const uint64_t f = (uint64_t)wg * per;
  const uint64_t e = f + per;
  return ItemRange{f < total ? f : total, e < total ? e : total};
}

// Workgroups of the correction kernel for a batch: one per possible item, up
// to the cap (the count is known only on the device).
constexpr uint32_t grid_for(uint64_t n, uint64_t S) {
  const uint64_t most = n * tiles_per_block(S);
  return (uint32_t)(most < kGridCap ? most : kGridCap);
}
constexpr uint32_t list_grid_for(uint64_t n) {
  const uint64_t wgs = (n + 255) / 256;
  return (uint32_t)(wgs < kListGridCap ? wgs : kListGridCap);
}

// Byte offsets into `have` and the decode rows for a target in position q of
// block b.
constexpr uint64_t block_base(uint64_t b, uint32_t k, uint32_t x, uint64_t S) {
  return b * ((uint64_t)(k + x) * S);
}
// the position input slot j (j < k) is read from: the basis, with spare 0 in
// place of basis q
constexpr uint32_t input_pos(uint32_t j, uint32_t q, uint32_t k) { return (q < k && j == q) ? k : j; }
constexpr uint64_t shard_off(uint64_t b, uint32_t pos, uint32_t k, uint32_t x, uint64_t S) {
  return block_base(b, k, x, S) + (uint64_t)pos * S;
}
// the decode row the coefficients come from, and its first byte in the rows region
constexpr uint32_t row_of(uint32_t q, uint32_t k) { return q >= k ? q - k : 0u; }
constexpr uint64_t row_off(uint64_t b, uint32_t q, uint32_t k, uint32_t x) {
  return b * ((uint64_t)x * k) + (uint64_t)row_of(q, k) * k;
}
// a lane's 16-byte column inside the shard; active while below S
constexpr uint64_t col_off(uint64_t tile, uint32_t lane) {
  return tile * kTileBytes + (uint64_t)lane * kLaneBytes;
}

}  // namespace correct
}  // namespace memo_ec
