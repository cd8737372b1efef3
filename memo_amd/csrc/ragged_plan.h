// ragged_plan.h -- GPU-free planning of ragged batches (memo_ec_encode_ragged /
// memo_ec_verify_ragged / memo_ec_rebuild_ragged): size validation, prefix
// sums, launch spans, pipeline waves and the per-tile descriptors the ragged
// kernels read; at the end (namespace stage) the slot layout of every
// host-memory call.  Plain C++17, no HIP include: tests/test_ragged_plan.py,
// tests/test_ragged_rebuild_plan.py and tests/test_stage_plan.py build it
// into stand-alone programs with the host sanitizers.
//
// A ragged batch of n blocks has shard sizes S[b] (multiples of 64, < 2^32,
// 0 allowed), packed back to back: off[b] = S[0] + ... + S[b-1], T = off[n].
// Its column space is the T / 16 16-byte columns of one shard row,
// concatenated over the blocks; tile t covers columns [256 t, 256 t + 256).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace memo_ec {
namespace ragged {

constexpr uint32_t kTileCols = 256;              // MAC_TILE of ec_kernels.h
constexpr uint64_t kMaxShard = 1ull << 32;       // shard sizes stay below
constexpr uint64_t kMaxCallBytes = 1ull << 50;   // k * T and m * T stay below
constexpr uint64_t kMaxSpanBlocks = 0x7fffffffull;  // non-empty blocks of one launch (32-bit index)

enum Status { kOk = 0, kInvalid = 1, kRange = 2 };

// Validates sizes and forms off[0..n] (bytes).  kInvalid: sizes null with
// n > 0, a size that is no multiple of 64 or is >= 2^32; kRange: k * T or
// m * T >= 2^50.  An invalid size anywhere wins over the range.
inline Status prefix_sums(const size_t* sizes, size_t n, unsigned k, unsigned m,
                          std::vector<uint64_t>& off) {
  off.clear();
  if (n && !sizes) return kInvalid;
  const unsigned per = k > m ? k : m;
  bool range = false;
  uint64_t t = 0;
  off.reserve(n < (1u << 20) ? n + 1 : (1u << 20));
  off.push_back(0);
  for (size_t b = 0; b < n; ++b) {
    const uint64_t s = (uint64_t)sizes[b];
    if (s % 64 != 0 || s >= kMaxShard) return kInvalid;
    if (!range) {
      t += s;  // < 2^50 + 2^32: no overflow
      if (per && t >= (kMaxCallBytes + per - 1) / per) range = true;
      else off.push_back(t);
    }
  }
  if (range) {
    off.clear();
    return kRange;
  }
  return kOk;
}

struct Range {
  size_t b0, b1;  // blocks [b0, b1)
};

// Launch spans: consecutive block ranges that cover every block once, cut on
// block boundaries only, each of at most tile_limit tiles and kMaxSpanBlocks
// blocks.  A block of more tiles than the limit gets a span of its own.
inline std::vector<Range> cut_spans(const size_t* sizes, size_t n, uint64_t tile_limit,
                                    uint64_t block_limit = kMaxSpanBlocks) {
  std::vector<Range> out;
  size_t b0 = 0;
  uint64_t cols = 0;
  for (size_t b = 0; b < n; ++b) {
    const uint64_t c = (uint64_t)sizes[b] / 16;
    const uint64_t tiles = (cols + c + kTileCols - 1) / kTileCols;
    if (b > b0 && (tiles > tile_limit || b - b0 >= block_limit)) {
      out.push_back({b0, b});
      b0 = b;
      cols = 0;
    }
    cols += c;
  }
  if (n > b0) out.push_back({b0, n});
  return out;
}

// Pipeline waves: consecutive block ranges that cover every block once, cut
// on block boundaries only, each of at most byte_limit bytes where block b
// weighs per * size(b).  A block heavier than the limit gets a wave of its
// own.  Equal sizes S give max(1, byte_limit / (per * S)) blocks per wave, so
// the uniform calls cut by the same rule, without a size array.
template <class Size>
inline std::vector<Range> cut_waves_by(Size size, size_t n, uint64_t per, uint64_t byte_limit) {
  std::vector<Range> out;
  size_t b0 = 0;
  uint64_t bytes = 0;
  for (size_t b = 0; b < n; ++b) {
    const uint64_t w = per * (uint64_t)size(b);
    if (b > b0 && bytes + w > byte_limit) {
      out.push_back({b0, b});
      b0 = b;
      bytes = 0;
    }
    bytes += w;
  }
  if (n > b0) out.push_back({b0, n});
  return out;
}
inline std::vector<Range> cut_waves(const size_t* sizes, size_t n, uint64_t per,
                                    uint64_t byte_limit) {
  return cut_waves_by([sizes](size_t b) { return sizes[b]; }, n, per, byte_limit);
}

// One tile of the column space.  The index leaves zero-size blocks out:
// q numbers the non-empty blocks of the span, orig[q] is the caller's block
// (relative to the span's first), coff[q] its first column and coff[nq] the
// span's column count.
struct TileDesc {
  uint32_t q_first;  // non-empty block holding the tile's first column
  uint32_t nblk;     // non-empty blocks the tile's columns touch (1..64); 1: inside one block
  uint32_t c0;       // the tile's first column, inside block q_first
  uint32_t cols;     // columns of block q_first (S / 16)
};
static_assert(sizeof(TileDesc) == 16, "read as one 16-byte load");

struct Counts {
  uint64_t nq = 0, cols = 0, tiles = 0;
};
inline Counts index_counts(const size_t* sizes, size_t n) {
  Counts c;
  for (size_t b = 0; b < n; ++b)
    if (sizes[b]) {
      ++c.nq;
      c.cols += (uint64_t)sizes[b] / 16;
    }
  c.tiles = (c.cols + kTileCols - 1) / kTileCols;
  return c;
}

// Fills coff[nq + 1], orig[nq] and desc[tiles] (index_counts' figures) of
// the span `sizes[0..n)`.
inline void build_index(const size_t* sizes, size_t n, uint64_t* coff, uint32_t* orig,
                        TileDesc* desc) {
  uint64_t nq = 0, cols = 0;
  for (size_t b = 0; b < n; ++b)
    if (sizes[b]) {
      orig[nq] = (uint32_t)b;
      coff[nq++] = cols;
      cols += (uint64_t)sizes[b] / 16;
    }
  coff[nq] = cols;
  const uint64_t tiles = (cols + kTileCols - 1) / kTileCols;
  uint64_t q = 0;
  for (uint64_t t = 0; t < tiles; ++t) {
    const uint64_t c = t * kTileCols;
    const uint64_t end = c + kTileCols < cols ? c + kTileCols : cols;
    while (coff[q + 1] <= c) ++q;
    uint64_t qe = q;
    while (coff[qe + 1] < end) ++qe;
    TileDesc& d = desc[t];
    d.q_first = (uint32_t)q;
    d.nblk = (uint32_t)(qe - q + 1);
    d.c0 = (uint32_t)(c - coff[q]);
    d.cols = (uint32_t)(coff[q + 1] - coff[q]);
  }
}

struct Index {
  std::vector<uint64_t> coff;
  std::vector<uint32_t> orig;
  std::vector<TileDesc> desc;
};
inline Index build_index(const size_t* sizes, size_t n) {
  const Counts c = index_counts(sizes, n);
  Index ix;
  ix.coff.resize(c.nq + 1);
  ix.orig.resize(c.nq);
  ix.desc.resize(c.tiles);
  build_index(sizes, n, ix.coff.data(), ix.orig.data(), ix.desc.data());
  return ix;
}

// ---- Ragged rebuild with per-block patterns (memo_ec_rebuild_ragged).
// Every non-empty block of a tile has a table set of its own, so a tile
// touches at most `cap` blocks (rows_cap): a tile starts where the previous
// one ended and covers 256 columns, or ends at the start of non-empty block
// q_first + cap if that comes first.  A tile cut by the cap ends on a block
// boundary and its trailing lanes are idle; tiles are no longer at 256 * t,
// so the descriptor carries the tile's first column.

// Table sets one tile may build: `per` = R * kpad coefficient slots per set,
// `stage_slots` the coefficients a tile stages through registers, LDS of
// (per + 1) * 20 bytes per set within `lds_bytes`; never above the 64 blocks
// 256 columns can touch.
inline uint32_t rows_cap(uint64_t per, uint64_t stage_slots, uint64_t lds_bytes) {
  uint64_t cap = 64;
  if (stage_slots / per < cap) cap = stage_slots / per;
  if (lds_bytes / ((per + 1) * 20) < cap) cap = lds_bytes / ((per + 1) * 20);
  return cap < 1 ? 1u : (uint32_t)cap;
}

struct RowsTileDesc {
  uint32_t q_first;  // non-empty block holding the tile's first column
  uint32_t nblk;     // non-empty blocks the tile's columns touch (1..cap)
  uint32_t c0;       // the tile's first column, inside block q_first
  uint32_t cols;     // columns of block q_first (S / 16)
  uint64_t col;      // the tile's first column in the span's column space
  uint32_t ncols;    // the tile's columns (1..256)
  uint32_t pad;
};
static_assert(sizeof(RowsTileDesc) == 32, "read as two 16-byte loads");

// Tiles of a column space fed one non-empty block at a time.
struct RowsCounter {
  uint32_t cap = 1;
  uint64_t nq = 0, cols = 0, tiles = 0;
  uint32_t tcols = 0, tblk = 0;  // the open tile's columns and blocks
  explicit RowsCounter(uint32_t cap_) : cap(cap_ ? cap_ : 1) {}
  void add(uint64_t c) {  // a block of c > 0 columns
    ++nq;
    cols += c;
    bool fresh = true;  // the block's first piece: counts against the cap
    while (c) {
      if (tiles == 0 || tcols == kTileCols || (fresh && tblk == cap)) {
        ++tiles;
        tcols = 0;
        tblk = 0;
      }
      fresh = false;
      if (tcols == 0 && c >= kTileCols) {  // whole tiles inside the block
        const uint64_t w = c / kTileCols;
        tiles += w - 1;
        tcols = kTileCols;
        tblk = 1;
        c -= w * kTileCols;
        continue;
      }
      const uint64_t take = c < kTileCols - tcols ? c : kTileCols - tcols;
      tcols += (uint32_t)take;
      ++tblk;
      c -= take;
    }
  }
};

inline Counts rows_index_counts(const size_t* sizes, size_t n, uint32_t cap) {
  RowsCounter rc(cap);
  for (size_t b = 0; b < n; ++b)
    if (sizes[b]) rc.add((uint64_t)sizes[b] / 16);
  Counts c;
  c.nq = rc.nq;
  c.cols = rc.cols;
  c.tiles = rc.tiles;
  return c;
}

// cut_spans for the capped tiles: each span of at most tile_limit tiles as
// rows_index_counts counts them (tiles restart at a span's first column).
inline std::vector<Range> cut_rows_spans(const size_t* sizes, size_t n, uint32_t cap,
                                         uint64_t tile_limit,
                                         uint64_t block_limit = kMaxSpanBlocks) {
  std::vector<Range> out;
  size_t b0 = 0;
  RowsCounter cur(cap);
  for (size_t b = 0; b < n; ++b) {
    RowsCounter nxt = cur;
    if (sizes[b]) nxt.add((uint64_t)sizes[b] / 16);
    if (b > b0 && (nxt.tiles > tile_limit || b - b0 >= block_limit)) {
      out.push_back({b0, b});
      b0 = b;
      nxt = RowsCounter(cap);
      if (sizes[b]) nxt.add((uint64_t)sizes[b] / 16);
    }
    cur = nxt;
  }
  if (n > b0) out.push_back({b0, n});
  return out;
}

// Fills coff[nq + 1], orig[nq] and desc[tiles] (rows_index_counts' figures)
// of the span `sizes[0..n)`.
inline void build_rows_index(const size_t* sizes, size_t n, uint32_t cap, uint64_t* coff,
                             uint32_t* orig, RowsTileDesc* desc) {
  if (cap < 1) cap = 1;
  uint64_t nq = 0, cols = 0;
  for (size_t b = 0; b < n; ++b)
    if (sizes[b]) {
      orig[nq] = (uint32_t)b;
      coff[nq++] = cols;
      cols += (uint64_t)sizes[b] / 16;
    }
  coff[nq] = cols;
  uint64_t q = 0, t = 0;
  for (uint64_t c = 0; c < cols; ++t) {
    while (coff[q + 1] <= c) ++q;
    uint64_t end = c + kTileCols < cols ? c + kTileCols : cols;
    if (q + cap <= nq && coff[q + cap] < end) end = coff[q + cap];
    uint64_t qe = q;
    while (coff[qe + 1] < end) ++qe;
    RowsTileDesc& d = desc[t];
    d.q_first = (uint32_t)q;
    d.nblk = (uint32_t)(qe - q + 1);
    d.c0 = (uint32_t)(c - coff[q]);
    d.cols = (uint32_t)(coff[q + 1] - coff[q]);
    d.col = c;
    d.ncols = (uint32_t)(end - c);
    d.pad = 0;
    c = end;
  }
}

struct RowsIndex {
  std::vector<uint64_t> coff;
  std::vector<uint32_t> orig;
  std::vector<RowsTileDesc> desc;
};
inline RowsIndex build_rows_index(const size_t* sizes, size_t n, uint32_t cap) {
  const Counts c = rows_index_counts(sizes, n, cap);
  RowsIndex ix;
  ix.coff.resize(c.nq + 1);
  ix.orig.resize(c.nq);
  ix.desc.resize(c.tiles);
  build_rows_index(sizes, n, cap, ix.coff.data(), ix.orig.data(), ix.desc.data());
  return ix;
}

}  // namespace ragged

// ---- Staging layout of a host-memory call (memo_ec.cpp: run_staged).  A
// call is a list of waves, a wave a list of extents of host memory that its
// kernels read (kIn) or write (kOut).  A kCaller extent is the caller's own
// buffer (shards, outputs, verdict words): pinned memory is used in place
// (zero-copy) or moved by DMA directly, pageable memory goes through the
// ctx's host slot.  A kSlot extent (bytes the library stages: a rebuild's
// per-block indices) always goes through the host slot.
// tests/test_stage_plan.py checks the layout on the CPU.
namespace stage {

enum Dir : uint8_t { kIn, kOut };
enum Via : uint8_t { kCaller, kSlot };
constexpr size_t kNone = ~(size_t)0;

struct Extent {
  void* host;  // kIn extents are only read
  size_t bytes;
  Dir dir;
  Via via;
  size_t at;   // offset in the wave's device slot
  size_t hat;  // offset in the wave's host slot; kNone: not staged there (pinned caller memory)
};

struct Sizes {
  size_t dev = 0, host = 0;  // the largest wave's device and host slot
};

struct Plan {
  std::vector<Extent> ext;
  std::vector<size_t> first;  // wave w: ext[first[w]] .. ext[first[w + 1]]

  // room for `waves` waves of `extents` extents in all: one allocation each
  Plan(size_t waves, size_t extents) {
    ext.reserve(extents);
    first.reserve(waves + 1);
    first.push_back(0);
  }
  void add(const void* host, size_t bytes, Dir dir, Via via = kCaller) {
    ext.push_back({const_cast<void*>(host), bytes, dir, via, 0, 0});
  }
  // `per` shards of blocks [w.b0, w.b1) of a buffer whose block b starts at
  // per * off(b)
  template <class Off>
  void add_blocks(const ragged::Range& w, Off off, const void* base, uint64_t per, Dir dir) {
    add(static_cast<const uint8_t*>(base) + per * off(w.b0), (size_t)(per * (off(w.b1) - off(w.b0))), dir);
  }
  void end_wave() { first.push_back(ext.size()); }
  size_t waves() const { return first.size() - 1; }

  // Places every wave's extents in its slot: the caller's inputs in the order
  // added, then its outputs (each 16-byte aligned: the kernels' vector loads
  // and stores), then the kSlot bytes, packed.  Inputs and outputs are each
  // contiguous, so a pageable wave moves with one copy per direction.  A
  // pageable caller's host slot mirrors the device slot; a pinned caller's
  // holds the kSlot bytes only -- no pinned bounce buffer of the payload's
  // size for memory the DMA engines and kernels reach as it lies.
  Sizes layout(bool pinned) {
    Sizes sz;
    for (size_t w = 0; w < waves(); ++w) {
      size_t at = 0, slot0 = 0;
      for (int pass = 0; pass < 3; ++pass) {
        if (pass == 2) slot0 = at;
        for (size_t i = first[w]; i < first[w + 1]; ++i) {
          Extent& e = ext[i];
          if ((e.via == kSlot ? 2 : e.dir == kIn ? 0 : 1) != pass) continue;
          if (e.via == kCaller) at = (at + 15) & ~(size_t)15;
          e.at = at;
          e.hat = e.via == kSlot ? at - (pinned ? slot0 : 0) : pinned ? kNone : at;
          at += e.bytes;
        }
      }
      sz.dev = sz.dev > at ? sz.dev : at;
      const size_t h = pinned ? at - slot0 : at;
      sz.host = sz.host > h ? sz.host : h;
    }
    return sz;
  }
};

}  // namespace stage
}  // namespace memo_ec
