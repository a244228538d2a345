// proof_decode.h — the four wire encodings of a Groth16 proof -> canonical
// affine words (A 16, B 32, C 16 u32; all-zero = infinity), host+device like
// pairing.h: the kernels of pairing.hip (k_proof_decode*) and the stand-alone
// host check (tests/host/proof_decode_check.cpp, against verify.cpp's
// zkmi_proof_decode) compile the very same flag, sign and range logic.
//
// Everything here decides "malformed" only (DESIGN.md §2.9's rule table): a
// coordinate >= q, a flag the format does not allow, an x with no root.
// Whether a well-formed point lies on the curve / in the subgroup is left to
// the verifier's point validation (pairing.hip v_validate), which sees the
// words written here.
//
// Input words are the encoding's bytes read as little-endian u32 (the bytes as
// they lie in memory, on the device and on an x86 host).
#pragma once
#include "fq_sqrt.h"

namespace zk {

constexpr int PROOF_ARK_COMPRESSED = 0;    // ZKMI_PROOF_* of include/zkmi.h
constexpr int PROOF_ARK_UNCOMPRESSED = 1;
constexpr int PROOF_SOLANA_LE = 2;
constexpr int PROOF_ALT_BN128_BE = 3;

ZK_HD size_t proof_encoded_len(int fmt) {
  return fmt == PROOF_ARK_COMPRESSED ? 128 : (fmt >= PROOF_ARK_UNCOMPRESSED && fmt <= PROOF_ALT_BN128_BE) ? 256 : 0;
}

struct PdC {
  static constexpr uint32_t Q[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                                    0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
  // 3 / (9 + u): the twist's b, canonical
  static constexpr uint32_t B0[8] = {0x24a138e5u, 0x3267e6dcu, 0x59dbefa3u, 0xb5b4c5e5u,
                                     0x1be06ac3u, 0x81be1899u, 0xceb8aaaeu, 0x2b149d40u};
  static constexpr uint32_t B1[8] = {0x85c315d2u, 0xe4a2bd06u, 0xe52d1852u, 0xa74fa084u,
                                     0xeed8fdf4u, 0xcd2cafadu, 0x3af0fed4u, 0x009713b0u};
};

ZK_HD bool pd_lt_q(const uint32_t* w) {
  bool lt = false, decided = false;  // no early exit: the caller's array stays in registers
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (!decided && w[i] != PdC::Q[i]) {
      lt = w[i] < PdC::Q[i];
      decided = true;
    }
  }
  return lt;
}
ZK_HD uint32_t pd_or8(const uint32_t* w) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) o |= w[i];
  return o;
}
ZK_HD Fe pd_const(const uint32_t (&c)[8]) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = c[i];
  return to_mont<FqP>(unpack(w));
}
// w <- q - w for 0 < w < q; 0 stays 0
ZK_HD void pd_neg(uint32_t* w) {
  if (pd_or8(w) == 0) return;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t t = (uint64_t)PdC::Q[i] - w[i] - br;
    w[i] = (uint32_t)t;
    br = (uint32_t)(t >> 63);
  }
}
ZK_HD uint32_t pd_bswap(uint32_t v) {
  return (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
}

// --------------------------------------------------------------- compressed
// arkworks SWFlags in the top two bits of the encoding's last byte: bit 7 =
// "y > -y", bit 6 = infinity.  The strict rule of verify.cpp's g1_decompress /
// g2_decompress: x < q after masking; the infinity flag needs every other
// bit, bit 7 included, to be zero; no root is malformed.  So every accepted
// string is the one the encoder writes for its point.
// in: 8 words, out: 16 words (x, y).  False = malformed, out not written.
ZK_HD bool pd_g1_compressed(const uint32_t* in, uint32_t* out) {
  uint32_t w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) w[i] = in[i];
  const bool larger = w[7] >> 31, inf = (w[7] >> 30) & 1;
  w[7] &= 0x3FFFFFFFu;
  if (inf) {
    if (larger || pd_or8(w)) return false;
    for (int i = 0; i < 16; i++) out[i] = 0;
    return true;
  }
  if (!pd_lt_q(w)) return false;
  const Fe x = to_mont<FqP>(unpack(w));
  Fe three = fe_zero();
  three.v[0] = 3;
  const Fe rhs = add<FqP>(mul<FqP>(sqr<FqP>(x), x), to_mont<FqP>(three));
  Fe y;
  if (!fq_sqrt(rhs, y)) return false;
  const Fe c = from_mont<FqP>(y), nc = from_mont<FqP>(neg<FqP>(y));
  const bool c_larger = fe_cmp(c, nc) > 0;
#pragma unroll
  for (int i = 0; i < 8; i++) out[i] = w[i];
  pack(out + 8, c_larger == larger ? c : nc);
  return true;
}
// in: 16 words (x.c0, x.c1 with the flags), out: 32 words (x.c0, x.c1, y.c0,
// y.c1).  Fq2 is ordered c1 first.  No subgroup check here.
ZK_HD bool pd_g2_compressed(const uint32_t* in, uint32_t* out) {
  uint32_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = in[i];
  const bool larger = w[15] >> 31, inf = (w[15] >> 30) & 1;
  w[15] &= 0x3FFFFFFFu;
  if (inf) {
    if (larger || pd_or8(w) || pd_or8(w + 8)) return false;
    for (int i = 0; i < 32; i++) out[i] = 0;
    return true;
  }
  if (!pd_lt_q(w) || !pd_lt_q(w + 8)) return false;
  const Fe2 x = {to_mont<FqP>(unpack(w)), to_mont<FqP>(unpack(w + 8))};
  const Fe2 tb = {pd_const(PdC::B0), pd_const(PdC::B1)};
  const Fe2 rhs = f2_add(f2_mul(f2_sqr(x), x), tb);
  Fe2 y;
  if (!f2_sqrt(rhs, y)) return false;
  const Fe2 ny = f2_neg(y);
  const Fe c0 = from_mont<FqP>(y.c0), c1 = from_mont<FqP>(y.c1);
  const Fe n0 = from_mont<FqP>(ny.c0), n1 = from_mont<FqP>(ny.c1);
  int cmp = fe_cmp(c1, n1);
  if (cmp == 0) cmp = fe_cmp(c0, n0);
  const bool keep = (cmp > 0) == larger;
#pragma unroll
  for (int i = 0; i < 16; i++) out[i] = w[i];
  pack(out + 16, keep ? c0 : n0);
  pack(out + 24, keep ? c1 : n1);
  return true;
}

// -------------------------------------------------------------- fixed width
// The three 256-byte formats: eight 32-byte coordinates A.x A.y | B (4) | C.x
// C.y, no power.  Every coordinate must be < q.
//   ARK_UNCOMPRESSED  little-endian; SWFlags in each point's last byte: bit 6 =
//                     infinity (every other bit of the point, bit 7 included,
//                     zero), bit 7 otherwise ignored; y as given
//   SOLANA_LE         little-endian, no flags; A's y is stored negated
//   ALT_BN128_BE      big-endian, G2 as c1 | c0; A's y is stored negated
// All-zero coordinates are the point at infinity in the canonical form.
// in: 64 words; a / b / c: 16 / 32 / 16 words, always written.  False =
// malformed (the caller then discards what was written).
template <int FMT>
ZK_HD bool pd_fixed(const uint32_t* in, uint32_t* a, uint32_t* b, uint32_t* c) {
  bool ok = true;
#pragma unroll
  for (int p = 0; p < 3; p++) {
    const int k0 = p == 0 ? 0 : p == 1 ? 2 : 6, nk = p == 1 ? 4 : 2;
    uint32_t* o = p == 0 ? a : p == 1 ? b : c;
    uint32_t any = 0;
    bool inf = false;
#pragma unroll
    for (int k = 0; k < nk; k++) {
      uint32_t w[8];
#pragma unroll
      for (int j = 0; j < 8; j++)
        w[j] = FMT == PROOF_ALT_BN128_BE ? pd_bswap(in[8 * (k0 + k) + 7 - j]) : in[8 * (k0 + k) + j];
      if (FMT == PROOF_ARK_UNCOMPRESSED && k == nk - 1) {
        inf = (w[7] >> 30) & 1;
        any |= w[7] & 0x80000000u;
        w[7] &= 0x3FFFFFFFu;
      }
      any |= pd_or8(w);
      ok &= pd_lt_q(w);
      if (FMT != PROOF_ARK_UNCOMPRESSED && p == 0 && k == 1) pd_neg(w);
      const int slot = FMT == PROOF_ALT_BN128_BE && p == 1 ? (k ^ 1) : k;
#pragma unroll
      for (int j = 0; j < 8; j++) o[8 * slot + j] = w[j];
    }
    if (inf && any) ok = false;
  }
  return ok;
}

}  // namespace zk
