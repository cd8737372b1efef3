// check_pair_logic_check.cc -- the decision of memo_ec_check_pair_batch for
// one unlocated block, made on the CPU with nothing but the algebra the
// kernel compiles (memo_amd/csrc/check_pair_logic.h) and a table multiply.
// Stand-alone: its own main, built by tests/test_check_pair_logic.py with the
// host sanitizers.
//
// stdin: blocks as text.  Per block "k x ns", then x * k decode-row entries
// (D, row-major), then ns syndrome vectors of x entries each (the block's
// distinct nonzero ones, in any order).
// stdout: per block "a b" -- the one pair of positions (a < b) that explains
// every syndrome -- or "none"; then "ok <blocks>".
//
// The procedure is check_pair_kernel's: v1 = any nonzero syndrome, v2 = any
// that is no multiple of v1; with a v2 every syndrome must lie in
// span{v1, v2} and exactly two columns of H = [D | I] must; without one the
// C(k + x, 2) pairs are counted.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../memo_amd/csrc/check_pair_logic.h"

using namespace memo_ec::pair_logic;

static uint8_t g_mul[256][256];

static void make_tables() {
  uint8_t ex[512], lg[256] = {0};
  unsigned v = 1;
  for (int i = 0; i < 255; ++i) {
    ex[i] = ex[i + 255] = (uint8_t)v;
    lg[v] = (uint8_t)i;
    v <<= 1;
    if (v & 0x100) v ^= 0x11D;
  }
  for (int a = 0; a < 256; ++a)
    for (int b = 0; b < 256; ++b) g_mul[a][b] = (a && b) ? ex[lg[a] + lg[b]] : 0;
}

static bool read_u(unsigned& out) { return std::scanf("%u", &out) == 1; }

static void fail(const char* what) {
  std::printf("FAILED %s\n", what);
  std::exit(1);
}

int main() {
  make_tables();
  const auto mul = [](uint32_t c, uint32_t v) -> uint32_t {
    if (c > 255 || v > 255) fail("multiply out of range");
    return g_mul[c][v];
  };
  unsigned k, x, ns, blocks = 0;
  while (read_u(k)) {
    if (!read_u(x) || !read_u(ns)) fail("short header");
    if (k < 1 || k > 64 || x < 3 || x > kMaxX || ns < 1) fail("bad header");
    std::vector<uint8_t> D(x * k), syn(ns * x);
    for (auto* vec : {&D, &syn})
      for (uint8_t& e : *vec) {
        unsigned t;
        if (!read_u(t) || t > 255) fail("bad entry");
        e = (uint8_t)t;
      }
    const uint32_t kx = k + x;
    Span sp;
    span_set1(sp, x, &syn[0]);
    if (sp.dim != 1) fail("zero syndrome given");
    const uint8_t* v2 = nullptr;
    for (unsigned s = 0; s < ns && !v2; ++s)
      if (!in_span(sp, &syn[s * x], mul)) v2 = &syn[s * x];
    uint32_t count = 0, lo = kNone, hi = 0;
    bool pair = false;
    if (v2) {
      if (!span_set2(sp, v2, mul) || sp.dim != 2) fail("v2 is a multiple of v1");
      bool inside = true;
      for (unsigned s = 0; s < ns; ++s) inside = inside && in_span(sp, &syn[s * x], mul);
      if (inside) {
        for (uint32_t q = 0; q < kx; ++q)
          if (column_in_span(sp, D.data(), k, q, mul)) {
            ++count;
            lo = q < lo ? q : lo;
            hi = q > hi ? q : hi;
          }
        if (count > 2) fail("three columns in a plane");
        pair = count == 2;
      }
    } else {
      const uint32_t pairs = kx * (kx - 1) / 2;
      uint32_t seen = 0;
      for (uint32_t t = 0; t < pairs; ++t) {
        uint32_t a, b;
        nth_pair(kx, t, a, b);
        if (!(a < b && b < kx)) fail("nth_pair out of range");
        ++seen;
        if (pair_explains(D.data(), k, x, sp.u1, a, b, mul)) {
          ++count;
          lo = a;
          hi = b;
        }
      }
      if (seen != pairs) fail("pairs");
      pair = count == 1;
    }
    if (pair)
      std::printf("%u %u\n", lo, hi);
    else
      std::printf("none\n");
    ++blocks;
  }
  std::printf("ok %u\n", blocks);
  return 0;
}
