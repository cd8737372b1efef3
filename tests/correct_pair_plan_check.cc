// correct_pair_plan_check.cc -- the arithmetic of memo_ec_correct_pair_batch
// (memo_amd/csrc/correct_pair_plan.h) walked on the CPU, before anything runs
// on a GPU.  Stand-alone: its own main, built by
// tests/test_correct_pair_plan.py with the host sanitizers.
//
// stdin: one shape per line, "k m x S n" (x >= 3).  A line that begins with
// "big" ("big k m x S b") holds the 64-bit arithmetic for block b of a batch
// that is never laid out: every offset against a 128-bit product.  For each
// shape the program asserts
//   - the scratch begins with memo_ec_correct_batch's scratch unmoved; the
//     second count word and the pair list are 256-byte aligned, disjoint from
//     it and from each other, and inside the layout's total, a multiple of 256;
//   - an entry gives back the block and the two positions it was made from,
//     for every qa < qb < k + x of the shape (and up to (64,16,16)) and at the
//     fields' limits;
//   - for every pair of positions: the k inputs are k distinct positions of
//     the block, neither of them a target, slot j reading basis j unless j is
//     a target, the substitutes being the lowest spares that are no target, in
//     ascending order; the rows read are rows of the block inside the rows
//     region, the clean rows distinct and no target's;
//   - with every block a pair, one a pair, none a pair, and singles and pairs
//     mixed (the pair list then holds every other block), for the launch's
//     grid and the grids 1 and 7: the workgroups' item ranges tile [0, count *
//     tiles) in order; the active lanes of an entry's tiles store each 16-byte
//     column of each of the two targets exactly once and nothing else, every
//     load and store inside `have`.
// stdout: "ok <lines>"; any failure prints what and where and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../memo_amd/csrc/correct_pair_plan.h"

using namespace memo_ec;
namespace cp = memo_ec::correct_pair;

#define REQUIRE(cond, ...)                                   \
  do {                                                       \
    if (!(cond)) {                                           \
      std::printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                              \
      std::printf("\n");                                     \
      std::exit(1);                                          \
    }                                                        \
  } while (0)

typedef unsigned long long ull;
typedef unsigned __int128 u128;

static void walk_scratch(unsigned k, unsigned x, size_t n) {
  const cp::Scratch lay = cp::scratch_layout(n, k, x);
  const correct::Scratch one = correct::scratch_layout(n, k, x);
  REQUIRE(lay.one.chk.basis == one.chk.basis && lay.one.chk.spares == one.chk.spares &&
              lay.one.chk.rows == one.chk.rows && lay.one.chk.total == one.chk.total &&
              lay.one.count == one.count && lay.one.list == one.list && lay.one.total == one.total,
          "the single correction's scratch moved");
  const size_t beg[3] = {0, lay.count, lay.list};
  const size_t len[3] = {one.total, sizeof(uint64_t), n * sizeof(uint64_t)};
  for (int i = 0; i < 3; ++i) {
    REQUIRE(beg[i] % 256 == 0, "region %d at %zu", i, beg[i]);
    REQUIRE(beg[i] + len[i] <= lay.total, "region %d ends at %zu, total %zu", i, beg[i] + len[i], lay.total);
    for (int j = 0; j < i; ++j)
      REQUIRE(beg[j] + len[j] <= beg[i] || beg[i] + len[i] <= beg[j], "regions %d and %d overlap", j, i);
  }
  REQUIRE(lay.total % 256 == 0, "total %zu", lay.total);
}

static void walk_entries(unsigned kx, uint64_t block) {
  for (unsigned qa = 0; qa < kx; ++qa)
    for (unsigned qb = qa + 1; qb < kx; ++qb) {
      const uint64_t e = cp::make_entry(block, qa, qb);
      REQUIRE(cp::entry_block(e) == block && cp::entry_qa(e) == qa && cp::entry_qb(e) == qb,
              "entry of block %llu, positions %u, %u", (ull)block, qa, qb);
    }
}

static void walk_entry_limits() {
  const uint64_t top = ((uint64_t)1 << 48) - 1;
  walk_entries(80, 0);
  walk_entries(80, top);
  const uint64_t e = cp::make_entry(top, 254, 255);
  REQUIRE(cp::entry_block(e) == top && cp::entry_qa(e) == 254 && cp::entry_qb(e) == 255, "the fields' limits");
  REQUIRE(cp::entry_qa(cp::make_entry(top, 0, 1)) == 0 && cp::entry_qb(cp::make_entry(top, 0, 1)) == 1,
          "the block spills into the positions");
  REQUIRE(cp::names_pair(1u << 25) && cp::names_pair((80u << 25) | (1u << 24)) && !cp::names_pair(0xFFFFFFFFu) &&
              !cp::names_pair(0x01FFFFFFu) && !cp::names_pair(0),
          "names_pair");
}

// The inputs and rows of one pair of targets of block b.
static void walk_pair(unsigned k, unsigned x, uint64_t S, uint64_t b, uint64_t n, unsigned qa, unsigned qb) {
  const unsigned kx = k + x;
  const u128 bytes = (u128)n * kx * S, rows = (u128)n * x * k;
  REQUIRE(qa < qb && qb < kx, "targets %u, %u", qa, qb);
  // what the definition says, spelled out: the lowest spares that are no target
  unsigned expect[64], next_spare = 0;
  for (unsigned j = 0; j < k; ++j) {
    if (j != qa && j != qb) {
      expect[j] = j;
      continue;
    }
    while (k + next_spare == qa || k + next_spare == qb) ++next_spare;
    expect[j] = k + next_spare++;
  }
  uint64_t seen[2] = {0, 0};
  for (unsigned j = 0; j < k; ++j) {
    const uint32_t pos = cp::input_pos(j, qa, qb, k);
    REQUIRE(pos < kx && pos != qa && pos != qb, "targets %u, %u: input %u reads position %u", qa, qb, j, pos);
    REQUIRE(pos == expect[j], "targets %u, %u: input %u reads position %u, the definition says %u", qa, qb, j, pos,
            expect[j]);
    REQUIRE(!(seen[pos >> 6] >> (pos & 63) & 1), "targets %u, %u: position %u read twice", qa, qb, pos);
    seen[pos >> 6] |= (uint64_t)1 << (pos & 63);
    const u128 off = ((u128)b * kx + pos) * S;
    REQUIRE((u128)cp::input_off(b, j, qa, qb, k, x, S) == off && off + S <= bytes, "input %u of block %llu", j, (ull)b);
  }
  for (unsigned i = 0; i < 2; ++i) {
    const u128 off = ((u128)b * kx + (i ? qb : qa)) * S;
    REQUIRE((u128)cp::target_off(b, i, qa, qb, k, x, S) == off && off + S <= bytes, "target %u of block %llu", i, (ull)b);
  }
  // the rows the coefficients come from
  unsigned rr[2], nr = 0;
  if (qa >= k) {  // two spares: their own rows
    rr[nr++] = cp::spare_row(0, qa, qb, k);
    rr[nr++] = cp::spare_row(1, qa, qb, k);
    REQUIRE(rr[0] == qa - k && rr[1] == qb - k, "spare rows");
  } else if (qb >= k) {  // the spare's row and one clean row
    rr[nr++] = cp::clean_row(0, qa, qb, k);
    rr[nr++] = cp::spare_row(1, qa, qb, k);
    REQUIRE(rr[1] == qb - k, "spare row");
    REQUIRE(rr[0] != rr[1] && rr[0] == (qb - k != 0 ? 0u : 1u), "clean row %u beside target row %u", rr[0], rr[1]);
    REQUIRE(cp::input_pos(qa, qa, qb, k) == k + rr[0], "the clean row's spare is not the one read");
  } else {  // two clean rows
    rr[nr++] = cp::clean_row(0, qa, qb, k);
    rr[nr++] = cp::clean_row(1, qa, qb, k);
    REQUIRE(rr[0] != rr[1], "targets %u, %u: both clean rows are row %u", qa, qb, rr[0]);
    REQUIRE(rr[0] == 0 && rr[1] == 1, "clean rows %u, %u", rr[0], rr[1]);
    REQUIRE(cp::input_pos(qa, qa, qb, k) == k + rr[0] && cp::input_pos(qb, qa, qb, k) == k + rr[1],
            "the clean rows' spares are not the ones read");
  }
  for (unsigned i = 0; i < nr; ++i) {
    REQUIRE(rr[i] < x, "row %u of %u", rr[i], x);
    const u128 off = ((u128)b * x + rr[i]) * k;
    REQUIRE((u128)cp::row_off(b, rr[i], k, x) == off && off + k <= rows, "row %u of block %llu", rr[i], (ull)b);
  }
}

static void walk_items(unsigned k, unsigned x, size_t S, size_t n, const std::vector<uint64_t>& list, uint32_t grid) {
  const unsigned kx = k + x;
  const uint64_t bytes = (uint64_t)n * kx * S;
  const uint64_t tpb = correct::tiles_per_block(S);
  const uint64_t count = list.size(), total = correct::work_items(count, tpb);
  std::vector<uint8_t> stored(count * 2 * (S / 16), 0);  // per entry, per target, per 16-byte column
  std::vector<uint8_t> hit(n * kx, 0);                   // shards written
  uint64_t next = 0, walk_entry = 0, walk_tile = 0;
  for (uint32_t wg = 0; wg < grid; ++wg) {
    const correct::ItemRange r = correct::wg_items(total, grid, wg);
    REQUIRE(r.first <= r.end && r.end <= total, "workgroup %u: [%llu, %llu) of %llu", wg, (ull)r.first, (ull)r.end,
            (ull)total);
    REQUIRE(r.first == next || r.first == r.end, "workgroup %u starts at %llu, the last ended at %llu", wg,
            (ull)r.first, (ull)next);
    for (uint64_t w = r.first; w < r.end; ++w, ++next) {
      const correct::Item it = correct::item_of(w, tpb);
      REQUIRE(it.entry == walk_entry && it.tile == walk_tile, "item %llu: (%llu, %llu), walk (%llu, %llu)", (ull)w,
              (ull)it.entry, (ull)it.tile, (ull)walk_entry, (ull)walk_tile);
      if (++walk_tile == tpb) walk_tile = 0, ++walk_entry;
      REQUIRE(it.entry < count && it.tile < tpb, "item %llu out of range", (ull)w);
      const uint64_t e = list[it.entry];
      const uint64_t b = cp::entry_block(e);
      const uint32_t qa = cp::entry_qa(e), qb = cp::entry_qb(e);
      REQUIRE(b < n, "entry %llu: block %llu", (ull)it.entry, (ull)b);
      if (it.tile == 0) walk_pair(k, x, S, b, n, qa, qb);
      for (uint32_t lane = 0; lane < 256; ++lane) {
        const uint64_t col = correct::col_off(it.tile, lane);
        if (col >= S) continue;  // an inactive lane neither loads nor stores
        REQUIRE(col % 16 == 0 && col + 16 <= S, "lane %u of tile %llu: column %llu of a %zu-byte shard", lane,
                (ull)it.tile, (ull)col, S);
        for (uint32_t j = 0; j < k; ++j)
          REQUIRE(cp::input_off(b, j, qa, qb, k, x, S) + col + 16 <= bytes, "load past `have`");
        for (uint32_t i = 0; i < 2; ++i) {
          const uint64_t out = cp::target_off(b, i, qa, qb, k, x, S);
          REQUIRE(out + col + 16 <= bytes, "store past `have`");
          REQUIRE(out / S == b * kx + (i ? qb : qa) && out % S == 0, "target %u of block %llu", i, (ull)b);
          uint8_t& s = stored[(it.entry * 2 + i) * (S / 16) + col / 16];
          REQUIRE(s == 0, "entry %llu, target %u: column %llu stored twice", (ull)it.entry, i, (ull)(col / 16));
          s = 1;
          hit[out / S] = 1;
        }
      }
    }
  }
  REQUIRE(next == total, "%llu of %llu items dealt", (ull)next, (ull)total);
  for (uint64_t c = 0; c < stored.size(); ++c) REQUIRE(stored[c] == 1, "column %llu never stored", (ull)c);
  uint64_t shards = 0;
  for (uint8_t h : hit) shards += h;
  REQUIRE(shards == 2 * count, "%llu shards written by %llu entries", (ull)shards, (ull)count);
}

static void walk(unsigned k, unsigned x, size_t S, size_t n) {
  const unsigned kx = k + x;
  walk_scratch(k, x, n);
  walk_entries(kx, 0);
  walk_entries(kx, n - 1);
  for (unsigned qa = 0; qa < kx; ++qa)
    for (unsigned qb = qa + 1; qb < kx; ++qb) {
      walk_pair(k, x, S, 0, n, qa, qb);
      walk_pair(k, x, S, n - 1, n, qa, qb);
    }
  const uint32_t grid = cp::grid_for(n, S);
  REQUIRE(grid <= correct::kGridCap && grid >= 1 && grid <= n * correct::tiles_per_block(S), "grid %u", grid);
  REQUIRE(cp::list_grid_for(n) == correct::list_grid_for(n) && cp::list_grid_for(n) >= 1, "list grid");
  const unsigned pairs = kx * (kx - 1) / 2;
  auto entry = [&](size_t b) {  // block b's pair: number b of the C(kx, 2), in order
    unsigned t = (unsigned)(b % pairs), qa = 0;
    while (t >= kx - 1 - qa) t -= kx - 1 - qa, ++qa;
    return cp::make_entry(b, qa, qa + 1 + t);
  };
  std::vector<uint64_t> all, one, mixed;
  for (size_t b = n; b-- > 0;) all.push_back(entry(b));  // in no order
  one.push_back(cp::make_entry(n - 1, kx - 2, kx - 1));
  for (size_t b = 0; b < n; b += 2) mixed.push_back(entry(b));  // every other block a pair, the rest singles
  for (uint32_t g : {grid, 1u, 7u}) {
    walk_items(k, x, S, n, all, g);
    walk_items(k, x, S, n, one, g);
    walk_items(k, x, S, n, mixed, g);
    walk_items(k, x, S, n, std::vector<uint64_t>(), g);
  }
}

// Block b of a batch too large to lay out: the offsets alone.
static void walk_big(unsigned k, unsigned x, uint64_t S, uint64_t b) {
  const unsigned kx = k + x;
  for (unsigned qa = 0; qa < kx; ++qa)
    for (unsigned qb = qa + 1; qb < kx; ++qb) walk_pair(k, x, S, b, b + 1, qa, qb);
  const uint64_t tpb = correct::tiles_per_block(S);
  REQUIRE(tpb == (S + 4095) / 4096, "tiles per block");
  const uint64_t col = correct::col_off(tpb - 1, 255);
  REQUIRE(col == (tpb - 1) * 4096 + 255 * 16, "last column");
  const uint64_t last = S - 16;
  REQUIRE(correct::col_off(last / 4096, (uint32_t)(last % 4096 / 16)) == last, "the shard's last column");
  REQUIRE((u128)cp::target_off(b, 1, kx - 2, kx - 1, k, x, S) + last + 16 == (u128)(b + 1) * kx * S,
          "the batch's last 16 bytes");
}

int main() {
  char word[16];
  unsigned k, m, x;
  unsigned long long S, n;
  int lines = 0;
  walk_entry_limits();
  while (std::scanf("%15s", word) == 1) {
    const bool big = std::strcmp(word, "big") == 0;
    if (big) {
      REQUIRE(std::scanf("%u %u %u %llu %llu", &k, &m, &x, &S, &n) == 5, "bad line");
    } else {
      k = (unsigned)std::strtoul(word, nullptr, 10);
      REQUIRE(std::scanf("%u %u %llu %llu", &m, &x, &S, &n) == 4, "bad line");
    }
    REQUIRE(k >= 1 && k <= 64 && m <= 16 && x >= 3 && x <= m && S % 64 == 0 && S > 0 && n >= 1, "bad shape");
    if (big)
      walk_big(k, x, S, n);
    else
      walk(k, x, (size_t)S, (size_t)n);
    ++lines;
  }
  std::printf("ok %d\n", lines);
  return 0;
}
