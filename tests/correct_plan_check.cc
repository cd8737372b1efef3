// correct_plan_check.cc -- the arithmetic of memo_ec_correct_batch
// (memo_amd/csrc/correct_plan.h) walked on the CPU, before anything runs on a
// GPU.  Stand-alone: its own main, built by tests/test_correct_plan.py with
// the host sanitizers.
//
// stdin: one shape per line, "k m x S n".  For each shape the program asserts
//   - the scratch begins with the check's scratch unchanged; the count word
//     and the list are 256-byte aligned, disjoint from it and from each
//     other, and inside the layout's total, itself a multiple of 256;
//   - a list entry gives back the block and position it was made from, for
//     every (block, position) of the shape and at the fields' limits;
//   - the list kernel's rounds visit every verdict word exactly once;
//   - with every block located (position b % (k + x)), with one block located
//     and with none, and for the launch's grid and the grids 1 and 7: the
//     workgroups' item ranges tile [0, count * tiles) in order; every item's
//     (entry, tile) equals a brute-force walk; the active lanes of an entry's
//     tiles store each 16-byte column of the target shard exactly once and
//     nothing else; the k inputs are k distinct positions of the same block,
//     none of them the target, each read inside `have`; the decode row lies
//     inside the rows region where a block-by-block walk puts it.
// stdout: "ok <shapes>"; any failure prints what and where and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../memo_amd/csrc/correct_plan.h"

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

typedef unsigned long long ull;

static void walk_scratch(unsigned k, unsigned x, size_t n) {
  const correct::Scratch lay = correct::scratch_layout(n, k, x);
  const check::Scratch chk = check::scratch_layout(n, k, x);
  REQUIRE(lay.chk.basis == chk.basis && lay.chk.spares == chk.spares && lay.chk.rows == chk.rows &&
              lay.chk.total == chk.total,
          "the check's scratch moved");
  const size_t beg[3] = {0, lay.count, lay.list};
  const size_t len[3] = {chk.total, sizeof(uint64_t), n * sizeof(uint64_t)};
  for (int i = 0; i < 3; ++i) {
    REQUIRE(beg[i] % 256 == 0, "region %d at %zu", i, beg[i]);
    REQUIRE(beg[i] + len[i] <= lay.total, "region %d ends at %zu, total %zu", i, beg[i] + len[i], lay.total);
    for (int j = 0; j < i; ++j)
      REQUIRE(beg[j] + len[j] <= beg[i] || beg[i] + len[i] <= beg[j], "regions %d and %d overlap", j, i);
  }
  REQUIRE(lay.total % 256 == 0, "total %zu", lay.total);
}

static void walk_entries(unsigned k, unsigned x, size_t n) {
  for (size_t b = 0; b < n; ++b)
    for (unsigned q = 0; q < k + x; ++q) {
      const uint64_t e = correct::make_entry(b, q);
      REQUIRE(correct::entry_block(e) == b && correct::entry_pos(e) == q, "entry of block %zu, position %u", b, q);
      REQUIRE((e >> 56) == 0, "entry of block %zu, position %u has bits past 55", b, q);
    }
  const uint64_t top = ((uint64_t)1 << 48) - 1;
  const uint64_t e = correct::make_entry(top, 255);
  REQUIRE(correct::entry_block(e) == top && correct::entry_pos(e) == 255, "the fields' limits");
  REQUIRE(correct::entry_pos(correct::make_entry(top, 0)) == 0, "the block spills into the position");
}

static void walk_list_rounds(size_t n) {
  const uint32_t grid = correct::list_grid_for(n);
  const uint64_t wgs = (n + 255) / 256;
  REQUIRE(grid >= 1 && grid == (wgs < correct::kListGridCap ? wgs : correct::kListGridCap), "list grid %u", grid);
  std::vector<uint8_t> seen(n, 0);
  for (uint32_t wg = 0; wg < grid; ++wg)
    for (uint64_t base = (uint64_t)wg * 256; base < n; base += (uint64_t)grid * 256)
      for (uint32_t lane = 0; lane < 256; ++lane)
        if (base + lane < n) {
          REQUIRE(seen[base + lane] == 0, "word %llu visited twice", (ull)(base + lane));
          seen[base + lane] = 1;
        }
  for (size_t b = 0; b < n; ++b) REQUIRE(seen[b] == 1, "word %zu never visited", b);
}

static void walk_items(unsigned k, unsigned x, size_t S, size_t n, const std::vector<uint64_t>& list,
                       uint32_t grid) {
  const unsigned kx = k + x;
  const uint64_t bytes = (uint64_t)n * kx * S, rows = (uint64_t)n * x * k;
  const uint64_t tpb = correct::tiles_per_block(S);
  REQUIRE(tpb == (S + 4095) / 4096 && tpb * 4096 >= S && (tpb - 1) * 4096 < S, "tiles per block %llu", (ull)tpb);
  const uint64_t count = list.size(), total = correct::work_items(count, tpb);
  REQUIRE(total == count * tpb, "work items");
  std::vector<uint8_t> stored(count * (S / 16), 0);  // per entry, per 16-byte column of its target
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
      const uint64_t b = correct::entry_block(list[it.entry]);
      const uint32_t q = correct::entry_pos(list[it.entry]);
      REQUIRE(b < n && q < kx, "entry %llu: block %llu, position %u", (ull)it.entry, (ull)b, q);
      // the decode row
      const uint64_t ro = correct::row_off(b, q, k, x);
      const uint32_t r0 = q >= k ? q - k : 0;
      REQUIRE(correct::row_of(q, k) == r0 && r0 < x, "row of position %u", q);
      REQUIRE(ro == (b * x + r0) * k && ro + k <= rows, "row of block %llu at %llu of %llu", (ull)b, (ull)ro, (ull)rows);
      // the inputs: k distinct positions of the block, none the target
      uint64_t posbits[2] = {0, 0};
      for (uint32_t j = 0; j < k; ++j) {
        const uint32_t pos = correct::input_pos(j, q, k);
        REQUIRE(pos < kx && pos != q, "block %llu, target %u: input %u reads position %u", (ull)b, q, j, pos);
        REQUIRE(pos == j || (j == q && pos == k), "input %u of target %u reads position %u", j, q, pos);
        REQUIRE(!(posbits[pos >> 6] >> (pos & 63) & 1), "position %u read twice", pos);
        posbits[pos >> 6] |= (uint64_t)1 << (pos & 63);
        REQUIRE(correct::shard_off(b, pos, k, x, S) == (b * kx + pos) * (uint64_t)S, "shard offset");
      }
      const uint64_t out = correct::shard_off(b, q, k, x, S);
      REQUIRE(out == (b * kx + q) * (uint64_t)S && correct::block_base(b, k, x, S) == b * kx * (uint64_t)S,
              "target offset");
      for (uint32_t lane = 0; lane < 256; ++lane) {
        const uint64_t col = correct::col_off(it.tile, lane);
        REQUIRE(col == it.tile * 4096 + lane * 16, "column of lane %u", lane);
        if (col >= S) continue;  // an inactive lane neither loads nor stores
        REQUIRE(col % 16 == 0 && col + 16 <= S, "lane %u of tile %llu: column %llu of a %zu-byte shard", lane,
                (ull)it.tile, (ull)col, S);
        REQUIRE(out + col + 16 <= bytes, "store past `have`");
        for (uint32_t j = 0; j < k; ++j)
          REQUIRE(correct::shard_off(b, correct::input_pos(j, q, k), k, x, S) + col + 16 <= bytes, "load past `have`");
        uint8_t& s = stored[it.entry * (S / 16) + col / 16];
        REQUIRE(s == 0, "entry %llu: column %llu stored twice", (ull)it.entry, (ull)(col / 16));
        s = 1;
      }
    }
  }
  REQUIRE(next == total, "%llu of %llu items dealt", (ull)next, (ull)total);
  for (uint64_t c = 0; c < stored.size(); ++c) REQUIRE(stored[c] == 1, "column %llu never stored", (ull)c);
}

static void walk(unsigned k, unsigned x, size_t S, size_t n) {
  walk_scratch(k, x, n);
  walk_entries(k, x, n);
  walk_list_rounds(n);
  const uint32_t grid = correct::grid_for(n, S);
  REQUIRE(grid <= correct::kGridCap && grid >= 1 && grid <= n * correct::tiles_per_block(S), "grid %u", grid);
  std::vector<uint64_t> all, one;
  for (size_t b = n; b-- > 0;) all.push_back(correct::make_entry(b, (unsigned)(b % (k + x))));  // in no order
  one.push_back(correct::make_entry(n - 1, k + x - 1));
  for (uint32_t g : {grid, 1u, 7u}) {
    walk_items(k, x, S, n, all, g);
    walk_items(k, x, S, n, one, g);
    walk_items(k, x, S, n, std::vector<uint64_t>(), g);
  }
  // first and last position of the basis and of the spares
  for (unsigned q : {0u, k - 1, k, k + x - 1}) {
    std::vector<uint64_t> l{correct::make_entry(0, q)};
    walk_items(k, x, S, n, l, grid);
  }
}

int main() {
  unsigned k, m, x;
  unsigned long long S, n;
  int shapes = 0;
  while (std::scanf("%u %u %u %llu %llu", &k, &m, &x, &S, &n) == 5) {
    REQUIRE(k >= 1 && k <= 64 && m <= 16 && x >= 1 && x <= m && S % 64 == 0 && S > 0 && n >= 1, "bad shape");
    walk(k, x, (size_t)S, (size_t)n);
    ++shapes;
  }
  std::printf("ok %d\n", shapes);
  return 0;
}
