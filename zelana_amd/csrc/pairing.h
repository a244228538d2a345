// pairing.h — Fq12 arithmetic, the single-pair Tate Miller loop of the batched
// verifier (pairing.hip k_miller) and the final exponentiation of verify_each
// (k_final_exp), host+device like ff.h / ec.h so the same code runs in
// stand-alone host checks (tests/host/pairing_dev_check.cpp,
// final_exp_dev_check.cpp).
//
// Fq12 = Fq[w] / (w^12 - 18 w^6 + 82): 12 Fq coefficients of w^0 .. w^11, the
// representation of verify.cpp, so values compare coefficient by coefficient.
// With t = w^6 (t^2 = 18 t - 82) an element is sum_{i<6} A_i w^i with pairs
// A_i = (c_i, c_{i+6}) = c_i + c_{i+6} t, and
//   (a0 + a1 t)(b0 + b1 t) = (a0 b0 - 82 a1 b1) + (a0 b1 + a1 b0 + 18 a1 b1) t
//   t (x0 + x1 t)          = -82 x1 + (x0 + 18 x1) t.
// A product's pair d is P_d + t P_{d+6}, P_m = sum_{i+j=m} A_i B_j, and each
// P_m needs three sums of Fq products,
//   Sa = sum a_i0 b_j0   Sb = sum a_i1 b_j1   Sc = sum (a_i0 b_j1 + a_i1 b_j0),
// of up to 6 / 6 / 12 terms.  Each sum is ONE lazy accumulation (Dot: the
// double-width columns of every product added up, then a single Montgomery
// reduction), the many-term form of ff.h's mul2 / mul4; the factors 18 and 82
// are two Montgomery products by constants per pair.
//
// The Fq12 element lives behind an accessor (get(i) / set(i, v), i < 12) so
// the device keeps it in LDS as lane-private columns (runtime-indexed
// per-thread arrays would go to scratch) and the host in a plain array.
#pragma once
#include "ec.h"

namespace zk {

// ------------------------------------------------------------ lazy dot product
// sum of Montgomery products with one reduction.  Column k of c collects the
// limb products a_i b_j, i + j = k: at most 9 per term, each < 2^58 for
// normalised (< 2^29) limbs.  Bound relied on: 63 such products plus a carry
// stay below 2^64 (63 (2^29 - 1)^2 < 2^64 - 2^58, the bound of ff.h's mul4
// with one more row), so a column takes 6 terms (54 products) and still has
// room for the 9 m_j p products of the reduction.  After 6 units dot_carry
// normalises the columns (< 2^29 again, top carry in column 17) and 6 more fit.
// A term whose first factor is a lazy double (limbs < 2^30) counts 2 units.
// Value: the sum must stay below 169 p^2 (ff.h) for a result < 2p; 12 products
// of values < 2p are < 48 p^2.
struct Dot {
  uint64_t c[2 * NL];
  int units;
};
ZK_HD void dot_zero(Dot& d) {
#pragma unroll
  for (int i = 0; i < 2 * NL; i++) d.c[i] = 0;
  d.units = 0;
}
ZK_HD void dot_carry(Dot& d) {
  uint64_t cy = 0;
#pragma unroll
  for (int i = 0; i < 2 * NL - 1; i++) {
    const uint64_t t = d.c[i] + cy;
    d.c[i] = t & LMASK;
    cy = t >> 29;
  }
  d.c[2 * NL - 1] += cy;
  d.units = 0;
}
// d += a * b; units = 1 (a, b normalised) or 2 (a a lazy double, limbs < 2^30)
ZK_HD void dot_mac(Dot& d, const Fe& a, const Fe& b, int units = 1) {
  if (d.units + units > 6) dot_carry(d);
  d.units += units;
#pragma unroll
  for (int i = 0; i < NL; i++) {
#pragma unroll
    for (int j = 0; j < NL; j++) pmac<FqP>(d.c[i + j], a.v[i], b.v[j]);
  }
}
// (sum) * 2^-261 mod p, < 2p, normalised limbs
ZK_HD Fe dot_reduce(const Dot& d) {
  uint32_t m[NL];
  Fe r;
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < NL; k++) {
    acc += d.c[k];
#pragma unroll
    for (int j = 0; j < k; j++) pmacs<FqP>(acc, m[j], FqP::P[k - j]);
    m[k] = ((uint32_t)acc * FqP::PINV) & LMASK;
    pmacs<FqP>(acc, m[k], FqP::P[0]);
    acc >>= 29;
  }
#pragma unroll
  for (int k = NL; k < 2 * NL - 1; k++) {
    acc += d.c[k];
#pragma unroll
    for (int j = k - (NL - 1); j < NL; j++) pmacs<FqP>(acc, m[j], FqP::P[k - j]);
    r.v[k - NL] = (uint32_t)acc & LMASK;
    acc >>= 29;
  }
  r.v[NL - 1] = (uint32_t)(acc + d.c[2 * NL - 1]);
  return r;
}

// ------------------------------------------------------------ Fq12
struct F12Const {
  Fe k18, k82, k9;  // Montgomery 18, 82, 9
};
ZK_HD Fe fq_small(uint32_t v) {
  Fe s = fe_zero();
  s.v[0] = v;
  return to_mont<FqP>(s);
}
ZK_HD F12Const f12_const() { return {fq_small(18), fq_small(82), fq_small(9)}; }

// plain-array element (host, tests)
struct F12Reg {
  Fe c[12];
  ZK_HD Fe get(int i) const { return c[i]; }
  ZK_HD void set(int i, const Fe& v) { c[i] = v; }
};
template <class A>
ZK_HD void f12_set_one(A& f) {
  f.set(0, one<FqP>());
  for (int i = 1; i < 12; i++) f.set(i, fe_zero());
}

struct F12Sums {
  Dot a, b, c;
};
// out pair d <- P_d + t P_{d+6}.  The high sums first, folded to two values
// (so only three accumulators are live at a time):
//   P_{d+6} = V + U t,  U = Sc' + 18 Sb',  V = Sa' - 82 Sb'
//   out_d = Sa - 82 (Sb + U),  out_{d+6} = Sc + 18 (Sb + U) + V
struct F12Hi {
  Fe u, v;  // zero when pair d has no high part
};
ZK_HD F12Hi f12_hi(const F12Sums& hi, const F12Const& K) {
  const Fe hb = dot_reduce(hi.b);
  return {add<FqP>(dot_reduce(hi.c), mul<FqP>(hb, K.k18)), sub<FqP>(dot_reduce(hi.a), mul<FqP>(hb, K.k82))};
}
template <class O>
ZK_HD void f12_fold(O& out, int d, const F12Sums& lo, const F12Hi& h, const F12Const& K) {
  const Fe sb = add<FqP>(dot_reduce(lo.b), h.u);
  out.set(d, sub<FqP>(dot_reduce(lo.a), mul<FqP>(sb, K.k82)));
  out.set(d + 6, add<FqP>(add<FqP>(dot_reduce(lo.c), mul<FqP>(sb, K.k18)), h.v));
}
// the three sums of P_m = sum_{i+j=m} A_i B_j, 0 <= i, j <= 5
template <class A, class B>
ZK_HD void f12_sums_mul(F12Sums& s, const A& a, const B& b, int m) {
  dot_zero(s.a);
  dot_zero(s.b);
  dot_zero(s.c);
#pragma unroll 1
  for (int i = m > 5 ? m - 5 : 0; i <= (m < 5 ? m : 5); i++) {
    const Fe a0 = a.get(i), a1 = a.get(i + 6), b0 = b.get(m - i), b1 = b.get(m - i + 6);
    dot_mac(s.a, a0, b0);
    dot_mac(s.b, a1, b1);
    dot_mac(s.c, a0, b1);
    dot_mac(s.c, a1, b0);
  }
}
// the same for a square: the pairs (i, j) and (j, i) once, with a doubled factor
template <class A>
ZK_HD void f12_sums_sqr(F12Sums& s, const A& a, int m) {
  dot_zero(s.a);
  dot_zero(s.b);
  dot_zero(s.c);
#pragma unroll 1
  for (int i = m > 5 ? m - 5 : 0; 2 * i <= m; i++) {
    const int j = m - i;
    const Fe a0 = a.get(i), a1 = a.get(i + 6);
    const Fe d0 = add_lazy(a0, a0), d1 = add_lazy(a1, a1);  // limbs < 2^30: 2 units
    if (i == j) {
      dot_mac(s.a, a0, a0);
      dot_mac(s.b, a1, a1);
      dot_mac(s.c, d0, a1, 2);
    } else {
      const Fe b0 = a.get(j), b1 = a.get(j + 6);
      dot_mac(s.a, d0, b0, 2);
      dot_mac(s.b, d1, b1, 2);
      dot_mac(s.c, d0, b1, 2);
      dot_mac(s.c, d1, b0, 2);
    }
  }
}
// out = a * b (out must not alias a or b)
template <class O, class A, class B>
ZK_HD void f12_mul(O& out, const A& a, const B& b, const F12Const& K) {
#pragma unroll 1
  for (int d = 0; d < 6; d++) {
    F12Sums s;
    F12Hi h = {fe_zero(), fe_zero()};
    if (d < 5) {
      f12_sums_mul(s, a, b, d + 6);
      h = f12_hi(s, K);
    }
    f12_sums_mul(s, a, b, d);
    f12_fold(out, d, s, h, K);
  }
}
// out = a^2 (out must not alias a)
template <class O, class A>
ZK_HD void f12_sqr(O& out, const A& a, const F12Const& K) {
#pragma unroll 1
  for (int d = 0; d < 6; d++) {
    F12Sums s;
    F12Hi h = {fe_zero(), fe_zero()};
    if (d < 5) {
      f12_sums_sqr(s, a, d + 6);
      h = f12_hi(s, K);
    }
    f12_sums_sqr(s, a, d);
    f12_fold(out, d, s, h, K);
  }
}
// The line of a Miller step, a sparse element with five terms:
//   l0 + l2 w^2 + l3 w^3 + l8 w^8 + l9 w^9  =  L_0 + L_2 w^2 + L_3 w^3,
//   L_0 = (l0, 0), L_2 = (l2, l8), L_3 = (l3, l9).
struct Line {
  Fe l0, l2, l3, l8, l9;
};
// P_m = sum_{j in {0,2,3}} A_{m-j} L_j  (5 products a pair of A)
template <class A>
ZK_HD void f12_sums_line(F12Sums& s, const A& a, const Line& l, int m) {
  dot_zero(s.a);
  dot_zero(s.b);
  dot_zero(s.c);
  if (m <= 5) {
    dot_mac(s.a, a.get(m), l.l0);
    dot_mac(s.c, a.get(m + 6), l.l0);
  }
  if (m >= 2 && m - 2 <= 5) {
    const Fe a0 = a.get(m - 2), a1 = a.get(m + 4);
    dot_mac(s.a, a0, l.l2);
    dot_mac(s.b, a1, l.l8);
    dot_mac(s.c, a0, l.l8);
    dot_mac(s.c, a1, l.l2);
  }
  if (m >= 3 && m - 3 <= 5) {
    const Fe a0 = a.get(m - 3), a1 = a.get(m + 3);
    dot_mac(s.a, a0, l.l3);
    dot_mac(s.b, a1, l.l9);
    dot_mac(s.c, a0, l.l9);
    dot_mac(s.c, a1, l.l3);
  }
}
// out = a * line (out must not alias a); P_m is non-zero for m <= 8
template <class O, class A>
ZK_HD void f12_mul_line(O& out, const A& a, const Line& l, const F12Const& K) {
#pragma unroll 1
  for (int d = 0; d < 6; d++) {
    F12Sums s;
    F12Hi h = {fe_zero(), fe_zero()};
    if (d < 3) {
      f12_sums_line(s, a, l, d + 6);
      h = f12_hi(s, K);
    }
    f12_sums_line(s, a, l, d);
    f12_fold(out, d, s, h, K);
  }
}

// ------------------------------------------------------------ Miller loop
// G2 point untwisted into E(Fq12): x w^2, y w^3 with c0 + c1 u = (c0 - 9 c1) + c1 w^6
struct QUntw {
  Fe x2, x8, y3, y9;
};
ZK_HD QUntw untwist(const Fe2& x, const Fe2& y, const F12Const& K) {
  return {sub<FqP>(x.c0, mul<FqP>(K.k9, x.c1)), x.c1, sub<FqP>(y.c0, mul<FqP>(K.k9, y.c1)), y.c1};
}
// the line a yQ - b xQ + c  (a, b, c in Fq)
ZK_HD Line miller_line(const QUntw& q, const Fe& a, const Fe& b, const Fe& c) {
  const Fe nb = neg<FqP>(b);
  return {c, mul<FqP>(nb, q.x2), mul<FqP>(a, q.y3), mul<FqP>(nb, q.x8), mul<FqP>(a, q.y9)};
}
ZK_HD Fe fq_triple(const Fe& a) { return add<FqP>(dbl<FqP>(a), a); }

// Miller value of e(P, Q) for one pair of finite points (Montgomery affine
// coordinates < 2p), the loop of verify.cpp's miller_value: Jacobian T in G1,
// tangent and chord lines scaled by Fq factors (killed by the final
// exponentiation), T = -P in the last step.  f0 and f1 are two elements'
// storage; the value ends in the one returned (0 or 1).
template <class A>
ZK_HD int miller_loop(A& f0, A& f1, const Fe& px, const Fe& py, const Fe2& qx, const Fe2& qy) {
  const uint64_t R[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL,
                         0x30644e72e131a029ULL};  // the group order r, bit 253 set
  const F12Const K = f12_const();
  const QUntw q = untwist(qx, qy, K);
  Fe X = px, Y = py, Z = one<FqP>();
  bool t_inf = false;
  int cur = 0;
  f12_set_one(f0);
#pragma unroll 1
  for (int bit = 252; bit >= 0; bit--) {
    if (cur == 0) f12_sqr(f1, f0, K); else f12_sqr(f0, f1, K);
    cur ^= 1;
    if (!t_inf) {
      // tangent, scaled by 2 Y Z^3: a = 2 Y Z^3, b = 3 X^2 Z^2, c = 3 X^3 - 2 Y^2
      const Fe Z2 = sqr<FqP>(Z), X2 = sqr<FqP>(X), Y2 = sqr<FqP>(Y);
      const Fe Y_2 = dbl<FqP>(Y), E = fq_triple(X2);
      const Line l = miller_line(q, mul<FqP>(Y_2, mul<FqP>(Z2, Z)), mul<FqP>(E, Z2),
                                 sub<FqP>(mul<FqP>(E, X), dbl<FqP>(Y2)));
      if (cur == 0) f12_mul_line(f1, f0, l, K); else f12_mul_line(f0, f1, l, K);
      cur ^= 1;
      // T = 2T (dbl-2009-l, a = 0)
      const Fe C = sqr<FqP>(Y2);
      const Fe xy = add<FqP>(X, Y2);
      const Fe D = dbl<FqP>(sub<FqP>(sub<FqP>(sqr<FqP>(xy), X2), C));
      const Fe X3 = sub<FqP>(sqr<FqP>(E), dbl<FqP>(D));
      const Fe C8 = dbl<FqP>(dbl<FqP>(dbl<FqP>(C)));
      const Fe Y3 = sub<FqP>(mul<FqP>(E, sub<FqP>(D, X3)), C8);
      Z = mul<FqP>(Y_2, Z);
      X = X3;
      Y = Y3;
    }
    if (((R[bit >> 6] >> (bit & 63)) & 1) && !t_inf) {
      const Fe Z2 = sqr<FqP>(Z);
      const Fe H = sub<FqP>(mul<FqP>(px, Z2), X);
      const Fe Rr = sub<FqP>(mul<FqP>(py, mul<FqP>(Z2, Z)), Y);
      if (is_zero<FqP>(H)) {
        // T = -P: the vertical line lies in Fq6 and dies in the final
        // exponentiation (the last step of the loop: r P = O)
        t_inf = true;
        continue;
      }
      const Fe HZ = mul<FqP>(H, Z);
      const Line l = miller_line(q, HZ, Rr, sub<FqP>(mul<FqP>(Rr, px), mul<FqP>(HZ, py)));
      if (cur == 0) f12_mul_line(f1, f0, l, K); else f12_mul_line(f0, f1, l, K);
      cur ^= 1;
      const Fe HH = sqr<FqP>(H), HHH = mul<FqP>(H, HH), V = mul<FqP>(X, HH);
      const Fe X3 = sub<FqP>(sub<FqP>(sqr<FqP>(Rr), HHH), dbl<FqP>(V));
      Y = sub<FqP>(mul<FqP>(Rr, sub<FqP>(V, X3)), mul<FqP>(Y, HHH));
      X = X3;
      Z = HZ;
    }
  }
  return cur;
}

// ------------------------------------------------------------ final exponentiation
// What verify.cpp's final_exp_is_one decides, for verify_each's k_final_exp:
// with h = (f^(q^2) f)^((q^4 - q^2 + 1) / r), true iff h != 0 and h lies in
// Fq6 = span{w^even}.  q = 1 mod 6, so w^(q^2) = zeta w with zeta in Fq and
// Frobenius^2 multiplies coefficient i by zeta^i.
struct FinalExpConst {
  Fe zeta[12];        // zeta^i, Montgomery (verify.cpp's frob2_table)
  uint64_t hard[12];  // (q^4 - q^2 + 1) / r, little-endian (verify.cpp's HARD)
};
constexpr int HARD_BITS = 761;  // bit 760 is the exponent's top bit
template <class O, class A>
ZK_HD void f12_frob2(O& out, const A& a, const Fe* zeta) {
#pragma unroll 1
  for (int i = 0; i < 12; i++) out.set(i, mul<FqP>(a.get(i), zeta[i]));
}
// f holds the Miller value and is overwritten; t0 and t1 are two more
// elements' storage.  Plain left-to-right square-and-multiply over the 761
// bits of the exponent (weight 389: 760 squares, 388 products): t1 keeps the
// base, f and t0 ping-pong.  Every lane of a wave runs the same bits.  The
// verdict compares fully reduced values (is_zero reduces [0, 2p) to [0, p)).
template <class A>
ZK_HD bool final_exp_is_one(A& f, A& t0, A& t1, const Fe* zeta, const uint64_t* hard) {
  const F12Const K = f12_const();
  f12_frob2(t0, f, zeta);
  f12_mul(t1, t0, f, K);
#pragma unroll 1
  for (int i = 0; i < 12; i++) f.set(i, t1.get(i));
  int cur = 0;  // the running power lives in f (0) or t0 (1)
#pragma unroll 1
  for (int bit = HARD_BITS - 2; bit >= 0; bit--) {
    if (cur == 0) f12_sqr(t0, f, K); else f12_sqr(f, t0, K);
    cur ^= 1;
    if ((hard[bit >> 6] >> (bit & 63)) & 1) {
      if (cur == 0) f12_mul(t0, f, t1, K); else f12_mul(f, t0, t1, K);
      cur ^= 1;
    }
  }
  bool nonzero = false, odd_zero = true;
#pragma unroll 1
  for (int i = 0; i < 12; i++) {
    const bool z = is_zero<FqP>(cur == 0 ? f.get(i) : t0.get(i));
    nonzero |= !z;
    if (i & 1) odd_zero &= z;
  }
  return nonzero && odd_zero;
}

}  // namespace zk
