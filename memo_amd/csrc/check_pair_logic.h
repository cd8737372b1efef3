// check_pair_logic.h -- the GF(2^8) algebra of memo_ec_check_pair_batch: is a
// syndrome vector in the span of one or two others, and the rank of an x x 3
// matrix.  Plain C++17, no HIP include, and every function takes the multiply
// as an argument, so the same text compiles into check_pair_kernel (log /
// antilog tables in LDS, four bytes to a dword) and into a stand-alone CPU
// program with a table multiply (tests/check_pair_logic_check.cc, built with
// the host sanitizers by tests/test_check_pair_logic.py).
//
// Notation (include/memo_ec.h, memo_ec_check_pair_batch): D (x x k) are a
// block's decode rows of the spares over the basis, row-major; H = [D | I_x]
// has one column per position q of have_idx, column q < k being D[:, q] and
// column k + r the unit vector e_r.  Vectors have x <= kMaxX entries.
//
// mul(c, v): c is one field element; v is one element too, or several packed
// into a word (one per byte), and the product has v's shape.  Everything
// below multiplies a coefficient by a value in this order, so a residual is
// computed for the four bytes of a dword at once where the multiply is.
// Nothing divides: u in span{a} is tested as u_i * a_p == a_i * u_p.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MEMO_EC_PAIR_FN __host__ __device__ inline
#else
#define MEMO_EC_PAIR_FN inline
#endif

namespace memo_ec {
namespace pair_logic {

constexpr uint32_t kMaxX = 16;     // MEMO_EC_MAX_M
constexpr uint32_t kNone = ~0u;

// Entry i of column q of H.
MEMO_EC_PAIR_FN uint32_t h_entry(const uint8_t* D, uint32_t k, uint32_t q, uint32_t i) {
  return q < k ? D[i * k + q] : (uint32_t)(i == q - k);
}

// A span of dimension 1 or 2, prepared for membership tests.
//   dim 1: u1 != 0, p0 = its first nonzero entry.
//   dim 2: e2 = u1[p0] * u2 XOR u2[p0] * u1 (u2 with entry p0 eliminated, so
//          e2[p0] == 0), p1 = e2's first nonzero entry: it exists exactly
//          when u2 is no multiple of u1.
struct Span {
  uint8_t u1[kMaxX], e2[kMaxX];
  uint32_t x, dim, p0, p1;
};

// span{v}; v must have a nonzero entry (dim stays 0 otherwise, and no
// membership test may follow).
MEMO_EC_PAIR_FN void span_set1(Span& s, uint32_t x, const uint8_t* v) {
  s.x = x;
  s.dim = 0;
  s.p0 = s.p1 = 0;
  for (uint32_t i = 0; i < kMaxX; ++i) {
    s.u1[i] = i < x ? v[i] : 0;
    s.e2[i] = 0;
  }
  for (uint32_t i = 0; i < x; ++i)
    if (s.u1[i]) {
      s.p0 = i;
      s.dim = 1;
      return;
    }
}

// span{u1, v} over a span_set1 of dimension 1; stays dimension 1 (false) when
// v is a multiple of u1.
template <class Mul>
MEMO_EC_PAIR_FN bool span_set2(Span& s, const uint8_t* v, Mul mul) {
  const uint32_t a = s.u1[s.p0], b = v[s.p0];
  uint32_t p1 = kNone;
  for (uint32_t i = 0; i < s.x; ++i) {
    const uint32_t e = mul(a, (uint32_t)v[i]) ^ mul(b, (uint32_t)s.u1[i]);
    s.e2[i] = (uint8_t)e;
    if (e && p1 == kNone) p1 = i;
  }
  if (p1 == kNone) return false;
  s.p1 = p1;
  s.dim = 2;
  return true;
}

// Row i of the membership test of a vector w: zero for every i < x exactly
// when w lies in the span.  wi = w[i], w0 = w[p0], w1 = w[p1] (unused for
// dimension 1); packed values test one vector per byte.
//   dim 1: w' = u1[p0] * w XOR w[p0] * u1 must vanish.
//   dim 2: w' must be a multiple of e2: e2[p1] * w'_i == e2[i] * w'_p1.
template <class Mul>
MEMO_EC_PAIR_FN uint32_t span_residual(const Span& s, uint32_t i, uint32_t wi, uint32_t w0, uint32_t w1,
                                       Mul mul) {
  const uint32_t a = s.u1[s.p0];
  const uint32_t ri = mul(a, wi) ^ mul((uint32_t)s.u1[i], w0);
  if (s.dim == 1) return ri;
  const uint32_t r1 = mul(a, w1) ^ mul((uint32_t)s.u1[s.p1], w0);
  return mul((uint32_t)s.e2[s.p1], ri) ^ mul((uint32_t)s.e2[i], r1);
}

// Is the x-vector w in the span?
template <class Mul>
MEMO_EC_PAIR_FN bool in_span(const Span& s, const uint8_t* w, Mul mul) {
  const uint32_t w0 = w[s.p0], w1 = w[s.p1];
  uint32_t bad = 0;
  for (uint32_t i = 0; i < s.x; ++i) bad |= span_residual(s, i, (uint32_t)w[i], w0, w1, mul);
  return bad == 0;
}

// Is column q of H in the span?
template <class Mul>
MEMO_EC_PAIR_FN bool column_in_span(const Span& s, const uint8_t* D, uint32_t k, uint32_t q, Mul mul) {
  const uint32_t w0 = h_entry(D, k, q, s.p0), w1 = h_entry(D, k, q, s.p1);
  uint32_t bad = 0;
  for (uint32_t i = 0; i < s.x; ++i) bad |= span_residual(s, i, h_entry(D, k, q, i), w0, w1, mul);
  return bad == 0;
}

// Rank (0..3) of the x x 3 matrix with columns a, b, c, each given as a
// callable i -> entry.  A small elimination with running pivots, nothing
// stored per entry: b' = a[pa] * b XOR b[pa] * a, likewise c', then c' against
// b'.  No fixed pair of rows would do: unit columns make 2 x 2 minors vanish.
template <class A, class B, class Mul>
MEMO_EC_PAIR_FN uint32_t rank2(uint32_t x, A a, B b, Mul mul) {
  uint32_t pa = kNone;
  for (uint32_t i = 0; i < x && pa == kNone; ++i)
    if (a(i)) pa = i;
  if (pa == kNone) {
    for (uint32_t i = 0; i < x; ++i)
      if (b(i)) return 1;
    return 0;
  }
  const uint32_t ap = a(pa), bp = b(pa);
  for (uint32_t i = 0; i < x; ++i)
    if (mul(ap, b(i)) ^ mul(bp, a(i))) return 2;
  return 1;
}

template <class A, class B, class C, class Mul>
MEMO_EC_PAIR_FN uint32_t rank3(uint32_t x, A a, B b, C c, Mul mul) {
  uint32_t pa = kNone;
  for (uint32_t i = 0; i < x && pa == kNone; ++i)
    if (a(i)) pa = i;
  if (pa == kNone) return rank2(x, b, c, mul);
  const uint32_t ap = a(pa), bp = b(pa), cp = c(pa);
  // b'_i and c'_i: entry pa of both is zero
  uint32_t pb = kNone, bq = 0, cq = 0;
  for (uint32_t i = 0; i < x && pb == kNone; ++i) {
    const uint32_t e = mul(ap, b(i)) ^ mul(bp, a(i));
    if (e) {
      pb = i;
      bq = e;
      cq = mul(ap, c(i)) ^ mul(cp, a(i));
    }
  }
  if (pb == kNone) {  // b is a multiple of a
    for (uint32_t i = 0; i < x; ++i)
      if (mul(ap, c(i)) ^ mul(cp, a(i))) return 2;
    return 1;
  }
  for (uint32_t i = 0; i < x; ++i) {
    const uint32_t bi = mul(ap, b(i)) ^ mul(bp, a(i));
    const uint32_t ci = mul(ap, c(i)) ^ mul(cp, a(i));
    if (mul(bq, ci) ^ mul(cq, bi)) return 3;
  }
  return 2;
}

// Do positions a != b explain a block whose syndromes are all multiples of
// v (v != 0): is v in span{H_a, H_b}?  H_a and H_b are independent (x >= 2),
// so this is rank [H_a H_b v] == 2.
template <class Mul>
MEMO_EC_PAIR_FN bool pair_explains(const uint8_t* D, uint32_t k, uint32_t x, const uint8_t* v, uint32_t a,
                                   uint32_t b, Mul mul) {
  return rank3(
             x, [=](uint32_t i) { return h_entry(D, k, a, i); }, [=](uint32_t i) { return h_entry(D, k, b, i); },
             [=](uint32_t i) { return (uint32_t)v[i]; }, mul) == 2;
}

// Pair number t of the C(kx, 2) pairs of positions below kx, in the order
// (0,1), (0,2), ..., (0,kx-1), (1,2), ...: a < b.
MEMO_EC_PAIR_FN void nth_pair(uint32_t kx, uint32_t t, uint32_t& a, uint32_t& b) {
  a = 0;
  while (t >= kx - 1 - a) {
    t -= kx - 1 - a;
    ++a;
  }
  b = a + 1 + t;
}

// The verdict word of a located pair: the check's mask, the smaller shard
// index in bits 16..23, the larger plus 1 in bits 25..31, bit 24 zero.
MEMO_EC_PAIR_FN uint32_t pair_word(uint32_t mask, uint32_t idx_a, uint32_t idx_b) {
  const uint32_t lo = idx_a < idx_b ? idx_a : idx_b, hi = idx_a < idx_b ? idx_b : idx_a;
  return (mask & 0xFFFFu) | (lo << 16) | ((hi + 1u) << 25);
}

}  // namespace pair_logic
}  // namespace memo_ec
