// ragged_rebuild_plan_check.cc -- stand-alone check of the capped tiles of
// memo_amd/csrc/ragged_plan.h (the index of memo_ec_rebuild_ragged's
// per-block patterns; tests/test_ragged_rebuild_plan.py builds it with the
// host sanitizers and runs it).
// stdin: one size list per line, "name s0 s1 ...".  For each list and each
// cap of 1, 2, 9, 24, 38 and 64 it checks, against a brute-force walk over
// the columns: that the tiles partition the columns in order; that no tile
// has more than 256 columns or more than cap blocks; that a tile shorter
// than 256 columns, other than the last, ends on a block boundary with
// exactly cap blocks; that a host restatement of the kernel's lane search
// finds every column's block and size; and that the span cuts under tile
// limits 1, 2, 3 cover every block once by the planner's own tile count.
// Then rows_cap.  Exit status 0 and a last line "ok <lists>".
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../memo_amd/csrc/ragged_plan.h"

using namespace memo_ec::ragged;

static int g_fail = 0;
#define CHECK(cond, ...)                         \
  do {                                           \
    if (!(cond)) {                               \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
      if (++g_fail > 20) std::exit(1);           \
    }                                            \
  } while (0)

// What locate_ragged_rows of ec_kernels.hip computes for lane `tid` of tile
// t: the lane's table set (its non-empty block q = q_first + set), its column
// inside the block and its shard size.
struct Lane {
  bool valid;
  uint32_t set;
  uint32_t col, S;
};
static Lane lane_locate(const RowsIndex& ix, uint64_t t, uint32_t tid) {
  const RowsTileDesc& d = ix.desc[t];
  int32_t start = -(int32_t)d.c0, end = (int32_t)(d.cols - d.c0);
  uint32_t cnt = 0;
  bool valid;
  if (d.nblk == 1) {
    valid = tid < d.ncols;
  } else {
    const uint64_t base = d.col;
    std::vector<int32_t> e(64, 0x7fffffff);
    for (uint32_t l = 0; l < 64 && l < d.nblk; ++l)
      e[l] = (int32_t)(uint32_t)(ix.coff.at(d.q_first + 1 + l) - base);
    const int32_t first_end = e[0];
    end = 0x7fffffff;
    for (uint32_t j = 0; j < d.nblk; ++j) {
      const int32_t r = e[j];
      const bool take = r <= (int32_t)tid;
      start = take ? r : start;
      cnt += take;
      end = take ? end : (r < end ? r : end);
    }
    valid = cnt < d.nblk;
    if (!valid) {
      cnt = 0;
      start = -(int32_t)d.c0;
      end = first_end;
    }
  }
  const uint32_t tt = valid ? tid : 0;
  return Lane{valid, cnt, (uint32_t)((int32_t)tt - start), (uint32_t)(end - start) * 16u};
}

static void check_list(const char* name, const std::vector<size_t>& sz, uint32_t cap) {
  const size_t n = sz.size();
  // brute force: the block and column inside it of every column
  std::vector<uint32_t> col_block, col_in;
  for (size_t b = 0; b < n; ++b)
    for (uint64_t c = 0; c < sz[b] / 16; ++c) {
      col_block.push_back((uint32_t)b);
      col_in.push_back((uint32_t)c);
    }
  const uint64_t cols = col_block.size();
  const Counts cn = rows_index_counts(sz.data(), n, cap);
  const RowsIndex ix = build_rows_index(sz.data(), n, cap);
  CHECK(cn.cols == cols && ix.coff.size() == cn.nq + 1 && ix.coff[cn.nq] == cols, "%s cap %u: counts", name, cap);
  CHECK(ix.desc.size() == cn.tiles, "%s cap %u: tiles", name, cap);
  // brute-force tile count: a tile takes columns until it has 256 or the
  // next column would be its (cap + 1)-th block
  uint64_t walk_tiles = 0;
  for (uint64_t c = 0; c < cols;) {
    uint64_t x = c + 1;
    uint32_t blocks = 1;
    while (x < cols && x - c < 256) {
      if (col_block[x] != col_block[x - 1] && ++blocks > cap) break;
      ++x;
    }
    ++walk_tiles;
    c = x;
  }
  CHECK(cn.tiles == walk_tiles, "%s cap %u: %llu tiles, walk %llu", name, cap, (unsigned long long)cn.tiles,
        (unsigned long long)walk_tiles);
  uint64_t at = 0;
  for (uint64_t tl = 0; tl < ix.desc.size(); ++tl) {
    const RowsTileDesc& d = ix.desc[tl];
    const uint64_t c = d.col, end = c + d.ncols;
    CHECK(c == at && d.ncols >= 1 && d.ncols <= 256 && end <= cols, "%s cap %u: tile %llu at %llu + %u after %llu",
          name, cap, (unsigned long long)tl, (unsigned long long)c, d.ncols, (unsigned long long)at);
    if (!(c == at && d.ncols >= 1 && end <= cols)) return;
    at = end;
    CHECK(d.q_first < cn.nq && ix.orig[d.q_first] == col_block[c] && d.c0 == col_in[c],
          "%s cap %u: tile %llu first block / column", name, cap, (unsigned long long)tl);
    CHECK((uint64_t)d.cols * 16 == sz[col_block[c]], "%s cap %u: tile %llu cols", name, cap, (unsigned long long)tl);
    uint32_t distinct = 1;
    for (uint64_t x = c + 1; x < end; ++x) distinct += col_block[x] != col_block[x - 1];
    CHECK(d.nblk == distinct && d.nblk <= cap && d.nblk <= 64, "%s cap %u: tile %llu nblk %u, walk %u", name, cap,
          (unsigned long long)tl, d.nblk, distinct);
    if (d.ncols < 256 && tl + 1 < ix.desc.size())
      CHECK(d.nblk == cap && col_block[end] != col_block[end - 1],
            "%s cap %u: short tile %llu (%u columns, %u blocks) not cut by the cap", name, cap,
            (unsigned long long)tl, d.ncols, d.nblk);
    for (uint32_t tid = 0; tid < 256; ++tid) {
      const Lane l = lane_locate(ix, tl, tid);
      CHECK(l.valid == (tid < d.ncols), "%s cap %u: tile %llu lane %u valid", name, cap, (unsigned long long)tl, tid);
      const uint64_t want = l.valid ? c + tid : c;  // idle lanes clamp to the tile's first column
      const uint64_t q = (uint64_t)d.q_first + l.set;
      CHECK(l.set < d.nblk && q < cn.nq && ix.orig[q] == col_block[want] && l.col == col_in[want] &&
                l.S == sz[col_block[want]],
            "%s cap %u: tile %llu lane %u: set %u col %u S %u", name, cap, (unsigned long long)tl, tid, l.set,
            l.col, l.S);
    }
  }
  CHECK(at == cols, "%s cap %u: tiles cover %llu of %llu columns", name, cap, (unsigned long long)at,
        (unsigned long long)cols);

  auto tiles_of = [&](size_t b0, size_t b1) { return rows_index_counts(sz.data() + b0, b1 - b0, cap).tiles; };
  for (uint64_t limit : {1, 2, 3}) {
    const std::vector<Range> sp = cut_rows_spans(sz.data(), n, cap, limit);
    size_t b = 0;
    for (size_t i = 0; i < sp.size(); ++i) {
      const Range& r = sp[i];
      CHECK(r.b0 == b && r.b1 > r.b0, "%s cap %u: span [%zu, %zu) after %zu", name, cap, r.b0, r.b1, b);
      b = r.b1;
      CHECK(r.b1 - r.b0 == 1 || tiles_of(r.b0, r.b1) <= limit, "%s cap %u: span [%zu, %zu) of %llu tiles, limit %llu",
            name, cap, r.b0, r.b1, (unsigned long long)tiles_of(r.b0, r.b1), (unsigned long long)limit);
      CHECK(i + 1 == sp.size() || tiles_of(r.b0, r.b1 + 1) > limit, "%s cap %u: span [%zu, %zu) cut early", name,
            cap, r.b0, r.b1);
    }
    CHECK(b == n, "%s cap %u: spans cover %zu of %zu blocks", name, cap, b, n);
  }
}

static void check_cap() {
  // RS(10,4) e = 4, RS(16,4) e = 4, RS(20,8) e = 8, RS(64,16) e = 16, one slot
  CHECK(rows_cap(40, 1536, 49152) == 38, "cap of 40 slots");
  CHECK(rows_cap(64, 1536, 49152) == 24, "cap of 64 slots");
  CHECK(rows_cap(160, 1536, 49152) == 9, "cap of 160 slots");
  CHECK(rows_cap(1024, 1536, 49152) == 1, "cap of 1024 slots");
  CHECK(rows_cap(4096, 1536, 49152) == 1, "cap never below 1");
  CHECK(rows_cap(1, 1536, 49152) == 64, "cap never above 64");
  CHECK(rows_cap(10, 1536, 4000) == 18, "cap by the LDS");
}

int main() {
  std::string line;
  int lists = 0;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string name;
    if (!(in >> name)) continue;
    std::vector<size_t> sz;
    unsigned long long v;
    while (in >> v) sz.push_back((size_t)v);
    for (uint32_t cap : {1u, 2u, 9u, 24u, 38u, 64u}) check_list(name.c_str(), sz, cap);
    ++lists;
  }
  check_cap();
  if (g_fail) return 1;
  std::printf("ok %d\n", lists);
  return 0;
}
