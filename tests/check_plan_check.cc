// check_plan_check.cc -- the arithmetic of memo_ec_check_batch
// (memo_amd/csrc/check_plan.h) walked on the CPU, before anything runs on a
// GPU.  Stand-alone: its own main, built by tests/test_check_plan.py with the
// host sanitizers.
//
// stdin: one shape per line, "k m x S n".  For each shape, with launch spans
// cut at the tile limits 3 and 2^31 - 257, the program asserts
//   - the three scratch regions are disjoint, 256-byte aligned and inside the
//     layout's total;
//   - the ranges the MAC launch reads -- per span and block, k basis shards
//     from the span's base and x spares from the spares' base, by the strides
//     the header hands out -- cover [0, n (k + x) S) exactly once (counted
//     per 16-byte column, what one lane loads);
//   - every block's decode rows lie inside the rows region, where a
//     block-by-block walk puts them;
//   - every span's three offsets equal those of a brute-force walk that adds
//     one block at a time, and a span of several blocks keeps to the limit.
// stdout: "ok <shapes>"; any failure prints what and where and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../memo_amd/csrc/check_plan.h"

using namespace memo_ec;

#define REQUIRE(cond, ...)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                              \
      std::printf("\n");                                     \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

static void walk(unsigned k, unsigned m, unsigned x, size_t S, size_t n, uint64_t tile_limit) {
  (void)m;
  const size_t kx = k + x;
  // scratch
  const check::Scratch lay = check::scratch_layout(n, k, x);
  const size_t beg[3] = {lay.basis, lay.spares, lay.rows};
  const size_t len[3] = {n * k, n * x, n * x * k};
  for (int i = 0; i < 3; ++i) {
    REQUIRE(beg[i] % 256 == 0, "region %d at %zu", i, beg[i]);
    REQUIRE(beg[i] + len[i] <= lay.total, "region %d ends at %zu, total %zu", i, beg[i] + len[i], lay.total);
    for (int j = 0; j < i; ++j)
      REQUIRE(beg[j] + len[j] <= beg[i] || beg[i] + len[i] <= beg[j], "regions %d and %d overlap", j, i);
  }
  REQUIRE(lay.total % 256 == 0, "total %zu", lay.total);

  const check::Strides str = check::strides(k, x, S);
  const uint64_t bytes = (uint64_t)n * kx * S;
  std::vector<uint8_t> seen(bytes / 16, 0);
  auto touch = [&](uint64_t at, const char* what, size_t b, unsigned t) {
    REQUIRE(at % 16 == 0, "%s of block %zu, shard %u at %llu", what, b, t, (unsigned long long)at);
    REQUIRE(at + S <= bytes, "%s of block %zu, shard %u ends at %llu of %llu", what, b, t,
            (unsigned long long)(at + S), (unsigned long long)bytes);
    for (uint64_t c = at / 16; c < (at + S) / 16; ++c) {
      REQUIRE(seen[c] == 0, "%s of block %zu, shard %u: column %llu read twice", what, b, t,
              (unsigned long long)c);
      seen[c] = 1;
    }
  };
  const size_t step = check::span_blocks(S, tile_limit);
  REQUIRE(step >= 1, "step");
  uint64_t walk_have = 0, walk_rows = 0, walk_word = 0;  // the brute-force walk
  size_t spans = 0;
  for (size_t b0 = 0; b0 < n; b0 += step, ++spans) {
    const size_t cnt = n - b0 < step ? n - b0 : step;
    const check::SpanOff o = check::span_offsets(b0, k, x, S);
    REQUIRE(o.have == walk_have, "span at %zu: have %llu, walk %llu", b0, (unsigned long long)o.have,
            (unsigned long long)walk_have);
    REQUIRE(o.rows == walk_rows, "span at %zu: rows %llu, walk %llu", b0, (unsigned long long)o.rows,
            (unsigned long long)walk_rows);
    REQUIRE(o.verdict == walk_word, "span at %zu: word %llu, walk %llu", b0, (unsigned long long)o.verdict,
            (unsigned long long)walk_word);
    REQUIRE(o.verdict + cnt <= n, "span at %zu: words past the array", b0);
    if (cnt > 1) {
      const uint64_t tiles = ((uint64_t)cnt * (S / 16) + check::kTileCols - 1) / check::kTileCols;
      REQUIRE(tiles <= tile_limit, "span at %zu: %llu tiles", b0, (unsigned long long)tiles);
    }
    // what the launch of this span reads: in = have + o.have, the spares'
    // base = in + str.spares, block stride str.block, shard stride str.shard
    for (size_t i = 0; i < cnt; ++i) {
      for (unsigned t = 0; t < k; ++t) touch(o.have + i * str.block + t * str.shard, "basis", b0 + i, t);
      for (unsigned r = 0; r < x; ++r)
        touch(o.have + str.spares + i * str.block + r * str.shard, "spare", b0 + i, r);
      const uint64_t row0 = o.rows + i * str.rows;
      REQUIRE(row0 == walk_rows, "rows of block %zu at %llu, walk %llu", b0 + i, (unsigned long long)row0,
              (unsigned long long)walk_rows);
      REQUIRE(row0 + (uint64_t)x * k <= len[2], "rows of block %zu end past the region", b0 + i);
      REQUIRE(lay.rows + row0 + (uint64_t)x * k <= lay.total, "rows of block %zu end past the scratch", b0 + i);
      walk_have += (uint64_t)kx * S;
      walk_rows += (uint64_t)x * k;
      walk_word += 1;
    }
  }
  REQUIRE(spans == (n + step - 1) / step, "spans");
  for (uint64_t c = 0; c < seen.size(); ++c)
    REQUIRE(seen[c] == 1, "column %llu never read", (unsigned long long)c);
}

int main() {
  unsigned k, m, x;
  unsigned long long S, n;
  int shapes = 0;
  while (std::scanf("%u %u %u %llu %llu", &k, &m, &x, &S, &n) == 5) {
    REQUIRE(k >= 1 && k <= 64 && m <= 16 && x >= 1 && x <= m && S % 64 == 0, "bad shape");
    for (uint64_t limit : {(uint64_t)3, (uint64_t)0x7fffffffull - 256}) walk(k, m, x, (size_t)S, (size_t)n, limit);
    ++shapes;
  }
  std::printf("ok %d\n", shapes);
  return 0;
}
