// fq_sqrt.h — square roots in Fq and Fq2 (q = 3 mod 4) over ff.h's 9 x 29-bit
// Montgomery form, host+device: one body for the proving-key decoders
// (groth16.hip k_decode_g1 / k_decode_g2), the proof decoder (proof_decode.h,
// pairing.hip k_proof_decode) and the stand-alone host check of the latter
// (tests/host/proof_decode_check.cpp).
#pragma once
#include "ff.h"

namespace zk {

// compare two fully reduced values limb-wise: -1, 0, 1
ZK_HD int fe_cmp(const Fe& a, const Fe& b) {
  for (int i = NL - 1; i >= 0; i--) {
    if (a.v[i] != b.v[i]) return a.v[i] > b.v[i] ? 1 : -1;
  }
  return 0;
}
ZK_HD Fe2 f2_pow(const Fe2& a, const uint64_t e[4]) {
  Fe2 r = f2_one();
  for (int i = 255; i >= 0; i--) {
    r = f2_sqr(r);
    if ((e[i >> 6] >> (i & 63)) & 1) r = f2_mul(r, a);
  }
  return r;
}
ZK_HD bool f2_eq(const Fe2& a, const Fe2& b) { return eq<FqP>(a.c0, b.c0) && eq<FqP>(a.c1, b.c1); }

// sqrt in Fq: a^((q+1)/4), false for a non-residue; which root is returned
// does not matter (the caller picks y or -y by the flag)
ZK_HD bool fq_sqrt(const Fe& a, Fe& out) {
  const uint64_t e14[4] = {0x4f082305b61f3f52ull, 0x65e05aa45a1c72a3ull, 0x6e14116da0605617ull,
                           0x0c19139cb84c680aull};  // (q+1)/4
  out = pow<FqP>(a, e14);
  return eq<FqP>(sqr<FqP>(out), a);
}

// sqrt in Fq2 for q = 3 mod 4 (Adj & Rodriguez-Henriquez, Alg. 9); which root
// is returned does not matter (the caller picks y or -y by the flag)
ZK_HD bool f2_sqrt(const Fe2& a, Fe2& out) {
  const uint64_t e34[4] = {0x4f082305b61f3f51ull, 0x65e05aa45a1c72a3ull, 0x6e14116da0605617ull,
                           0x0c19139cb84c680aull};  // (q-3)/4
  const uint64_t e12[4] = {0x9e10460b6c3e7ea3ull, 0xcbc0b548b438e546ull, 0xdc2822db40c0ac2eull,
                           0x183227397098d014ull};  // (q-1)/2
  Fe2 a1 = f2_pow(a, e34);
  Fe2 alpha = f2_mul(a1, f2_mul(a1, a));
  Fe2 conj = {alpha.c0, neg<FqP>(alpha.c1)};
  Fe2 a0 = f2_mul(conj, alpha);
  Fe2 m1 = {neg<FqP>(one<FqP>()), fe_zero()};
  if (f2_eq(a0, m1)) return false;
  Fe2 x0 = f2_mul(a1, a);
  if (f2_eq(alpha, m1)) {
    out = {neg<FqP>(x0.c1), x0.c0};
  } else {
    Fe2 b = {add<FqP>(alpha.c0, one<FqP>()), alpha.c1};
    out = f2_mul(f2_pow(b, e12), x0);
  }
  return f2_eq(f2_sqr(out), a);
}

}  // namespace zk
