// stage_plan_check.cc -- stand-alone check of the staging layout of
// host-memory calls (memo_amd/csrc/ragged_plan.h: stage::Plan, cut_waves_by;
// tests/test_stage_plan.py builds it with the host sanitizers and runs it).
// stdin: one size list per line, "name s0 s1 ...".  For each list, codes
// (10,4) and (3,2), pinned and pageable callers and pipeline batches of 4 KiB
// and 64 KiB it builds the plans the entry points build -- encode, verify,
// a rebuild with staged per-block indices, and the one-wave plan of a
// zero-copy call -- and checks the layout of every wave: extents inside the
// slot sizes reported, no two overlapping, inputs before outputs before
// staged bytes, the caller's extents 16-byte aligned, a pinned caller's host
// slot without payload, and the slot no larger than the sizes the entry
// points used to compute by hand.  Lists of equal sizes are also cut through
// the shared wave rule without a size array.  Exit status 0 and a last line
// "ok <lists>" when everything held.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../memo_amd/csrc/ragged_plan.h"

using namespace memo_ec;
using namespace memo_ec::stage;
using ragged::Range;

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

// The layout of `pl` for a pinned or pageable caller; `bound`: the slot
// bytes the entry point sized by hand, before alignment padding.
static void check_plan(const char* name, const char* what, Plan pl, bool pinned, size_t bound) {
  const Sizes sz = pl.layout(pinned);
  size_t host_want = 0;
  for (size_t w = 0; w < pl.waves(); ++w) {
    const Extent* x = pl.ext.data() + pl.first[w];
    const size_t nx = pl.first[w + 1] - pl.first[w];
    size_t slot_bytes = 0, last_in = 0, first_out = kNone, last_out = 0, first_slot = kNone;
    for (size_t i = 0; i < nx; ++i) {
      const Extent& e = x[i];
      CHECK(e.at + e.bytes <= sz.dev, "%s %s wave %zu extent %zu: [%zu, +%zu) past the device slot %zu", name,
            what, w, i, e.at, e.bytes, sz.dev);
      if (e.via == kCaller) {
        CHECK(e.at % 16 == 0, "%s %s wave %zu extent %zu: at %zu not 16-byte aligned", name, what, w, i, e.at);
        CHECK(pinned ? e.hat == kNone : e.hat == e.at, "%s %s wave %zu extent %zu: host place %zu", name, what,
              w, i, e.hat);
        if (e.dir == kIn) last_in = std::max(last_in, e.at + e.bytes);
        else {
          first_out = std::min(first_out, e.at);
          last_out = std::max(last_out, e.at + e.bytes);
        }
      } else {
        CHECK(e.hat != kNone, "%s %s wave %zu extent %zu: staged bytes without a host place", name, what, w, i);
        slot_bytes += e.bytes;
        first_slot = std::min(first_slot, e.at);
      }
      if (e.hat != kNone)
        CHECK(e.hat + e.bytes <= sz.host, "%s %s wave %zu extent %zu: [%zu, +%zu) past the host slot %zu", name,
              what, w, i, e.hat, e.bytes, sz.host);
      for (size_t j = 0; j < i; ++j) {
        const Extent& f = x[j];
        if (!e.bytes || !f.bytes) continue;
        CHECK(e.at + e.bytes <= f.at || f.at + f.bytes <= e.at, "%s %s wave %zu: extents %zu and %zu overlap",
              name, what, w, j, i);
        if (e.hat != kNone && f.hat != kNone)
          CHECK(e.hat + e.bytes <= f.hat || f.hat + f.bytes <= e.hat,
                "%s %s wave %zu: extents %zu and %zu overlap in the host slot", name, what, w, j, i);
      }
    }
    CHECK(first_out == kNone || last_in <= first_out, "%s %s wave %zu: an output before an input", name, what, w);
    CHECK(first_slot == kNone || std::max(last_in, last_out) <= first_slot,
          "%s %s wave %zu: staged bytes before the caller's", name, what, w);
    host_want = std::max(host_want, slot_bytes);
  }
  if (pinned) CHECK(sz.host == host_want, "%s %s: pinned host slot %zu, staged bytes %zu", name, what, sz.host, host_want);
  else CHECK(sz.host == sz.dev, "%s %s: pageable host slot %zu, device slot %zu", name, what, sz.host, sz.dev);
  size_t most = 0;  // extents of one wave: each may add < 16 bytes of padding
  for (size_t w = 0; w < pl.waves(); ++w) most = std::max(most, pl.first[w + 1] - pl.first[w]);
  CHECK(sz.dev <= bound + 15 * most, "%s %s: device slot %zu above the bound %zu", name, what, sz.dev, bound);
}

static void check_list(const char* name, const std::vector<size_t>& sz) {
  const size_t n = sz.size();
  std::vector<uint64_t> off;
  if (ragged::prefix_sums(sz.data(), n, 10, 4, off) != ragged::kOk) {
    CHECK(false, "%s: prefix_sums refused", name);
    return;
  }
  auto at = [&](size_t b) { return off[b]; };
  // stand-ins for the caller's buffers (never dereferenced)
  const uint8_t* data = reinterpret_cast<const uint8_t*>((uintptr_t)1 << 32);
  const uint8_t* parity = reinterpret_cast<const uint8_t*>((uintptr_t)2 << 32);
  const uint8_t* words = reinterpret_cast<const uint8_t*>((uintptr_t)3 << 32);
  const uint8_t* index = reinterpret_cast<const uint8_t*>((uintptr_t)4 << 32);
  bool equal = n > 0 && sz[0] > 0;
  for (size_t b = 0; b < n; ++b) equal = equal && sz[b] == sz[0];
  const int codes[2][2] = {{10, 4}, {3, 2}};
  for (const auto& code : codes)
    for (uint64_t pipe : {(uint64_t)4096, (uint64_t)65536, ~(uint64_t)0})  // ~0: the one wave of a zero-copy call
      for (int pinned = 0; pinned < 2; ++pinned) {
        const uint64_t k = code[0], r = code[1];
        auto extremes = [&](const std::vector<Range>& wv, uint64_t& tmax, size_t& nmax) {
          tmax = 0;
          nmax = 0;
          for (const Range& w : wv) {
            tmax = std::max<uint64_t>(tmax, off[w.b1] - off[w.b0]);
            nmax = std::max(nmax, w.b1 - w.b0);
          }
        };
        uint64_t tmax;
        size_t nmax;
        {  // encode: k shards in, r out, waves weighed by k
          const std::vector<Range> wv = ragged::cut_waves(sz.data(), n, k, pipe);
          extremes(wv, tmax, nmax);
          Plan pl(wv.size(), 2 * wv.size());
          for (const Range& w : wv) {
            pl.add_blocks(w, at, data, k, kIn);
            pl.add_blocks(w, at, parity, r, kOut);
            pl.end_wave();
          }
          CHECK(pipe != ~(uint64_t)0 || (pl.waves() <= 1 && pl.ext.size() <= 4), "%s: a one-wave call of %zu extents",
                name, pl.ext.size());
          check_plan(name, "encode", pl, pinned, (size_t)((k + r) * tmax));
        }
        {  // verify: k + r shards in, a word per block out, waves weighed by k + r
          const std::vector<Range> wv = ragged::cut_waves(sz.data(), n, k + r, pipe);
          extremes(wv, tmax, nmax);
          Plan pl(wv.size(), 3 * wv.size());
          for (const Range& w : wv) {
            pl.add_blocks(w, at, data, k, kIn);
            pl.add_blocks(w, at, parity, r, kIn);
            pl.add(words + 4 * w.b0, 4 * (w.b1 - w.b0), kOut);
            pl.end_wave();
          }
          check_plan(name, "verify", pl, pinned, (size_t)((k + r) * tmax + 4 * nmax));
        }
        {  // rebuild: k shards in, r out, k + r staged index bytes per block
          const std::vector<Range> wv = ragged::cut_waves(sz.data(), n, k + r, pipe);
          extremes(wv, tmax, nmax);
          Plan pl(wv.size(), 4 * wv.size());
          for (const Range& w : wv) {
            pl.add_blocks(w, at, data, k, kIn);
            pl.add(index + k * w.b0, k * (w.b1 - w.b0), kIn, kSlot);
            pl.add_blocks(w, at, parity, r, kOut);
            pl.add(index + r * w.b0, r * (w.b1 - w.b0), kIn, kSlot);
            pl.end_wave();
          }
          check_plan(name, "rebuild", pl, pinned, (size_t)((k + r) * tmax + (k + r) * nmax));
        }
        if (equal && pipe != ~(uint64_t)0) {
          // the uniform calls: the same rule without a size array
          const size_t S = sz[0];
          for (uint64_t per : {k, k + r}) {
            const std::vector<Range> u = ragged::cut_waves_by([S](size_t) { return S; }, n, per, pipe);
            const size_t nb = std::max<uint64_t>(1, pipe / (per * S));
            CHECK(u.size() == (n + nb - 1) / nb, "%s: %zu uniform waves of %zu blocks for %zu", name, u.size(), nb, n);
            for (size_t w = 0; w < u.size(); ++w)
              CHECK(u[w].b0 == w * nb && u[w].b1 == std::min(n, (w + 1) * nb), "%s: uniform wave %zu [%zu, %zu)",
                    name, w, u[w].b0, u[w].b1);
          }
        }
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
  if (g_fail) return 1;
  std::printf("ok %d\n", lists);
  return 0;
}
