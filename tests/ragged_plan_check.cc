// ragged_plan_check.cc -- stand-alone check of memo_amd/csrc/ragged_plan.h
// (tests/test_ragged_plan.py builds it with the host sanitizers and runs it).
// stdin: one size list per line, "name s0 s1 ...".  For each list it checks
// the prefix sums, the per-tile descriptors against a brute-force walk over
// the columns, a host restatement of the kernels' lane search against the
// same walk, the launch spans under tile limits 1, 2, 3 and the pipeline
// waves under 4 KiB and 64 KiB.  Then each class of invalid size.  Exit
// status 0 and a last line "ok <lists>" when everything held.
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

// What the ragged locate of ec_kernels.hip computes for lane `tid` of tile t:
// the lane's non-empty block q, its column inside it and its shard size.
struct Lane {
  bool valid;
  uint64_t q;
  uint32_t col, S;
};
static Lane lane_locate(const Index& ix, uint64_t t, uint32_t tid) {
  const TileDesc& d = ix.desc[t];
  int32_t start = -(int32_t)d.c0, end = (int32_t)(d.cols - d.c0);
  uint32_t cnt = 0;
  bool valid;
  if (d.nblk == 1) {
    valid = tid < (uint32_t)end;
  } else {
    const uint64_t base = t * kTileCols;
    std::vector<int32_t> e(64, 0x7fffffff);
    for (uint32_t l = 0; l < 64 && l < d.nblk; ++l) e[l] = (int32_t)(uint32_t)(ix.coff.at(d.q_first + 1 + l) - base);
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
  return Lane{valid, (uint64_t)d.q_first + cnt, (uint32_t)((int32_t)tt - start), (uint32_t)(end - start) * 16u};
}

static void check_ranges(const char* name, const char* what, const std::vector<Range>& rs, size_t n) {
  size_t at = 0;
  for (const Range& r : rs) {
    CHECK(r.b0 == at && r.b1 > r.b0, "%s %s: range [%zu, %zu) after %zu", name, what, r.b0, r.b1, at);
    at = r.b1;
  }
  CHECK(at == n, "%s %s: covers %zu of %zu blocks", name, what, at, n);
}

static void check_list(const char* name, const std::vector<size_t>& sz) {
  const size_t n = sz.size();
  std::vector<uint64_t> off;
  CHECK(prefix_sums(sz.data(), n, 10, 4, off) == kOk, "%s: prefix_sums refused", name);
  CHECK(off.size() == n + 1, "%s: %zu offsets", name, off.size());
  uint64_t t = 0;
  for (size_t b = 0; b < n; ++b) {
    CHECK(off[b] == t, "%s: off[%zu]", name, b);
    t += sz[b];
  }
  CHECK(off[n] == t, "%s: T", name);

  // brute force: the block and column inside it of every column
  std::vector<uint32_t> col_block, col_in;
  for (size_t b = 0; b < n; ++b)
    for (uint64_t c = 0; c < sz[b] / 16; ++c) {
      col_block.push_back((uint32_t)b);
      col_in.push_back((uint32_t)c);
    }
  const uint64_t cols = col_block.size();
  const Counts cn = index_counts(sz.data(), n);
  CHECK(cn.cols == cols && cn.tiles == (cols + 255) / 256, "%s: counts", name);
  const Index ix = build_index(sz.data(), n);
  CHECK(ix.coff.size() == cn.nq + 1 && ix.coff[cn.nq] == cols, "%s: coff end", name);
  for (uint64_t q = 0; q < cn.nq; ++q) {
    CHECK(sz[ix.orig[q]] != 0, "%s: orig[%llu] is a zero-size block", name, (unsigned long long)q);
    CHECK(ix.coff[q] * 16 == off[ix.orig[q]], "%s: coff[%llu]", name, (unsigned long long)q);
    CHECK(q == 0 || ix.orig[q] > ix.orig[q - 1], "%s: orig order", name);
  }
  for (uint64_t tl = 0; tl < cn.tiles; ++tl) {
    const TileDesc& d = ix.desc[tl];
    const uint64_t c = tl * 256, end = c + 256 < cols ? c + 256 : cols;
    CHECK(ix.orig[d.q_first] == col_block[c] && d.c0 == col_in[c], "%s: tile %llu first block / column",
          name, (unsigned long long)tl);
    CHECK((uint64_t)d.cols * 16 == sz[col_block[c]], "%s: tile %llu cols", name, (unsigned long long)tl);
    uint32_t distinct = 1;
    for (uint64_t x = c + 1; x < end; ++x) distinct += col_block[x] != col_block[x - 1];
    CHECK(d.nblk == distinct && d.nblk <= 64, "%s: tile %llu nblk %u, walk %u", name,
          (unsigned long long)tl, d.nblk, distinct);
    for (uint32_t tid = 0; tid < 256; ++tid) {
      const Lane l = lane_locate(ix, tl, tid);
      const uint64_t x = c + tid;
      CHECK(l.valid == (x < cols), "%s: tile %llu lane %u valid", name, (unsigned long long)tl, tid);
      const uint64_t want = l.valid ? x : c;  // lanes past the end clamp to the tile's first column
      CHECK(l.q < cn.nq && ix.orig[l.q] == col_block[want] && l.col == col_in[want] &&
                l.S == sz[col_block[want]],
            "%s: tile %llu lane %u: block %u col %u S %u", name, (unsigned long long)tl, tid,
            l.q < cn.nq ? ix.orig[l.q] : ~0u, l.col, l.S);
    }
  }

  auto tiles_of = [&](size_t b0, size_t b1) { return ((off[b1] - off[b0]) / 16 + 255) / 256; };
  for (uint64_t limit : {1, 2, 3}) {
    const std::vector<Range> sp = cut_spans(sz.data(), n, limit);
    check_ranges(name, "spans", sp, n);
    for (size_t i = 0; i < sp.size(); ++i) {
      const Range& r = sp[i];
      CHECK(r.b1 - r.b0 == 1 || tiles_of(r.b0, r.b1) <= limit, "%s: span [%zu, %zu) of %llu tiles, limit %llu",
            name, r.b0, r.b1, (unsigned long long)tiles_of(r.b0, r.b1), (unsigned long long)limit);
      // as long as the limit allows: the next block would not have fitted
      CHECK(i + 1 == sp.size() || tiles_of(r.b0, r.b1 + 1) > limit, "%s: span [%zu, %zu) cut early", name,
            r.b0, r.b1);
    }
  }
  for (uint64_t per : {1, 3})
    for (uint64_t limit : {4096, 65536}) {
      const std::vector<Range> wv = cut_waves(sz.data(), n, per, limit);
      check_ranges(name, "waves", wv, n);
      for (size_t i = 0; i < wv.size(); ++i) {
        const Range& r = wv[i];
        CHECK(r.b1 - r.b0 == 1 || per * (off[r.b1] - off[r.b0]) <= limit, "%s: wave [%zu, %zu) over %llu",
              name, r.b0, r.b1, (unsigned long long)limit);
        CHECK(i + 1 == wv.size() || per * (off[r.b1 + 1] - off[r.b0]) > limit, "%s: wave [%zu, %zu) cut early",
              name, r.b0, r.b1);
      }
    }
}

static void check_invalid() {
  std::vector<uint64_t> off;
  CHECK(prefix_sums(nullptr, 0, 10, 4, off) == kOk && off.size() == 1, "n == 0 is fine without sizes");
  CHECK(prefix_sums(nullptr, 3, 10, 4, off) == kInvalid, "NULL sizes with n > 0");
  for (size_t bad : {(size_t)1, (size_t)63, (size_t)65, (size_t)4096 + 16, (size_t)1 << 32, ((size_t)1 << 32) + 64,
                     ~(size_t)0 & ~(size_t)63}) {
    const size_t sz[3] = {64, bad, 128};
    CHECK(prefix_sums(sz, 3, 10, 4, off) == kInvalid, "size %zu accepted", bad);
  }
  const size_t big = ((size_t)1 << 32) - 64;  // the largest valid size
  {
    const size_t sz[2] = {big, 0};
    CHECK(prefix_sums(sz, 2, 10, 4, off) == kOk && off[2] == big, "largest size refused");
  }
  // k * T >= 2^50: k = 64, T = 2^44
  {
    std::vector<size_t> sz(4097, big);  // T just above 2^44
    CHECK(prefix_sums(sz.data(), sz.size(), 64, 16, off) == kRange, "k * T >= 2^50 accepted");
    CHECK(prefix_sums(sz.data(), sz.size(), 1, 1, off) == kOk, "T of 2^44 refused for k = m = 1");
    CHECK(prefix_sums(sz.data(), sz.size(), 1, 64, off) == kRange, "m * T >= 2^50 accepted");
    sz[4096] = 65;  // an invalid size behind the point where the range is passed
    CHECK(prefix_sums(sz.data(), sz.size(), 64, 16, off) == kInvalid, "invalid size behind the range");
  }
  {
    // exactly 2^50: 16 * 2^46 with sizes of 2^31
    std::vector<size_t> sz((size_t)1 << 15, (size_t)1 << 31);
    CHECK(prefix_sums(sz.data(), sz.size(), 16, 4, off) == kRange, "k * T == 2^50 accepted");
    sz.back() -= 64;
    CHECK(prefix_sums(sz.data(), sz.size(), 16, 4, off) == kOk, "k * T == 2^50 - 1024 refused");
  }
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
    check_list(name.c_str(), sz);
    ++lists;
  }
  check_invalid();
  if (g_fail) return 1;
  std::printf("ok %d\n", lists);
  return 0;
}
