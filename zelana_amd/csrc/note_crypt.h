// note_crypt.h — the four primitives of note decryption:
// GF(2^255 - 19) arithmetic and X25519 (RFC 7748), the one BLAKE3 compression
// of derive_key("zelana-note-v1", shared_secret || ephemeral_pk), ChaCha20 and
// Poly1305 (RFC 8439), and the parse of a note plaintext.  Host+device like
// mimc_hash.h / nullifier_set.h: the kernels of note_scan.hip, the device probe
// (tests/device/note_crypt_probe.hip) and the stand-alone host check
// (tests/host/note_crypt_check.cpp) compile the very same functions.  No HIP
// call is made here and nothing branches on secret data: a lane's control flow
// depends on lengths alone.
//
// Byte strings cross this header as little-endian u32 words (a 32-byte key is
// 8 words, a 12-byte nonce 3 words).  A ciphertext is read through a word
// pointer that is 4-byte aligned; bytes past its length are never used, and no
// word that lies wholly past its length is read.
//
// fe25519: ten limbs of alternating 26 and 25 bits, value = sum v[i] 2^ceil(25.5 i),
// so every product is a 32 x 32 -> 64 bit multiply-add and 19 b[j] and 2 a[i]
// still fit 32 bits.  Two bounds, on EVERY limb:
//   TIGHT  v[i] < 2^26      what load, mul, sqr, mul121665, sub and invert return
//   LOOSE  v[i] < 2^27      what add returns for TIGHT inputs
// mul, sqr, mul121665, sub, invert, cswap and store accept LOOSE (and so
// TIGHT) inputs; add accepts TIGHT ones.  The value of a TIGHT or LOOSE
// element may be any multiple-of-p shift of the residue it stands for; only
// store returns the canonical one.
#pragma once
#include <stdint.h>

#ifndef ZK_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZK_HD __host__ __device__ __forceinline__
#else
#define ZK_HD inline
#endif
#endif

namespace zk {

// ------------------------------------------------------------------- fe25519
struct Fe25 {
  uint32_t v[10];
};
constexpr uint32_t FE25_TIGHT = 1u << 26, FE25_LOOSE = 1u << 27;  // exclusive bounds of a limb
constexpr uint32_t FE25_M26 = (1u << 26) - 1, FE25_M25 = (1u << 25) - 1;

ZK_HD Fe25 fe25_zero() {
  Fe25 r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = 0;
  return r;
}
ZK_HD Fe25 fe25_one() {
  Fe25 r = fe25_zero();
  r.v[0] = 1;
  return r;
}
// 64-bit columns (each < 2^63) -> TIGHT.  The top carry comes back times 19;
// after it limb 0 is below 2^26 and limb 1 below 2^25 + 2^18.
ZK_HD Fe25 fe25_carry64(uint64_t* h) {
  Fe25 r;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    h[i + 1] += h[i] >> ((i & 1) ? 25 : 26);
    h[i] &= (i & 1) ? FE25_M25 : FE25_M26;
  }
  h[0] += 19 * (h[9] >> 25);
  h[9] &= FE25_M25;
  h[1] += h[0] >> 26;
  h[0] &= FE25_M26;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = (uint32_t)h[i];
  return r;
}
// TIGHT + TIGHT -> LOOSE
ZK_HD Fe25 fe25_add(const Fe25& a, const Fe25& b) {
  Fe25 r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = a.v[i] + b.v[i];
  return r;
}
// LOOSE - LOOSE -> TIGHT: a + 8p - b limb by limb (every limb of 8p is at
// least 2^28 - 8 > 2^27, so nothing goes below zero, and the sum stays below
// 2^30), then one carry pass
ZK_HD Fe25 fe25_sub(const Fe25& a, const Fe25& b) {
  uint64_t h[10];
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t p8 = i == 0 ? 0x1FFFFF68u : (i & 1) ? 0x0FFFFFF8u : 0x1FFFFFF8u;
    h[i] = (uint64_t)(a.v[i] + p8 - b.v[i]);
  }
  return fe25_carry64(h);
}
// LOOSE x LOOSE -> TIGHT.  Column k sums a[i] b[j] over i + j = k and 19 a[i]
// b[j] over i + j = k + 10, doubled where i and j are both odd (25.5 i rounds
// up twice).  With limbs < 2^27: 2 a[i] < 2^28, 19 b[j] < 2^31.3, a product <
// 2^59.3, a column of ten < 2^62.7.
ZK_HD Fe25 fe25_mul(const Fe25& a, const Fe25& b) {
  uint32_t a2[10], b19[10];
#pragma unroll
  for (int i = 0; i < 10; i++) {
    a2[i] = (i & 1) ? 2 * a.v[i] : a.v[i];
    b19[i] = 19 * b.v[i];
  }
  uint64_t h[10];
#pragma unroll
  for (int k = 0; k < 10; k++) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      const int j = k - i;
      if (j >= 0)
        acc += (uint64_t)(((i & 1) && (j & 1)) ? a2[i] : a.v[i]) * b.v[j];
      else
        acc += (uint64_t)(((i & 1) && ((j + 10) & 1)) ? a2[i] : a.v[i]) * b19[j + 10];
    }
    h[k] = acc;
  }
  return fe25_carry64(h);
}
// LOOSE -> TIGHT.  The symmetric products are taken once and doubled: 55
// multiplies where the product takes 100.  2 a[i] < 2^28 and, where i and j
// are both odd, 4 a[i] < 2^29; 19 a[j] < 2^31.3: a doubled product < 2^60.3
// stands for two of the product's terms, so a column is below 2^62.7 as there.
ZK_HD Fe25 fe25_sqr(const Fe25& a) {
  uint32_t a19[10];
#pragma unroll
  for (int i = 0; i < 10; i++) a19[i] = 19 * a.v[i];
  uint64_t h[10];
#pragma unroll
  for (int k = 0; k < 10; k++) {
    uint64_t acc = 0;
#pragma unroll
    for (int i = 0; i < 10; i++) {
      const int j = k - i >= 0 ? k - i : k - i + 10;
      if (i > j) continue;
      const uint32_t f = ((i < j) ? 2u : 1u) * (((i & 1) && (j & 1)) ? 2u : 1u);
      acc += (uint64_t)(f * a.v[i]) * (k - i >= 0 ? a.v[j] : a19[j]);
    }
    h[k] = acc;
  }
  return fe25_carry64(h);
}
// LOOSE -> TIGHT: a (A - 2) / 4 for curve25519's A = 486662
ZK_HD Fe25 fe25_mul121665(const Fe25& a) {
  uint64_t h[10];
#pragma unroll
  for (int i = 0; i < 10; i++) h[i] = (uint64_t)a.v[i] * 121665u;
  return fe25_carry64(h);
}
// swap a and b when bit = 1 (0 or 1), without a branch; any limbs
ZK_HD void fe25_cswap(Fe25& a, Fe25& b, uint32_t bit) {
  const uint32_t m = 0u - bit;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const uint32_t t = m & (a.v[i] ^ b.v[i]);
    a.v[i] ^= t;
    b.v[i] ^= t;
  }
}
// a^(2^n), n >= 1
ZK_HD Fe25 fe25_sqrn(Fe25 a, int n) {
#pragma unroll 1
  for (int i = 0; i < n; i++) a = fe25_sqr(a);
  return a;
}
// LOOSE -> TIGHT: a^(p - 2) = a^(2^255 - 21) by the fixed chain (254
// squarings, 11 products); 0 -> 0
ZK_HD Fe25 fe25_invert(const Fe25& z) {
  const Fe25 z2 = fe25_sqr(z);
  const Fe25 z9 = fe25_mul(fe25_sqrn(z2, 2), z);
  const Fe25 z11 = fe25_mul(z9, z2);
  const Fe25 z_5_0 = fe25_mul(fe25_sqr(z11), z9);                  // 2^5 - 1
  const Fe25 z_10_0 = fe25_mul(fe25_sqrn(z_5_0, 5), z_5_0);        // 2^10 - 1
  const Fe25 z_20_0 = fe25_mul(fe25_sqrn(z_10_0, 10), z_10_0);     // 2^20 - 1
  const Fe25 z_40_0 = fe25_mul(fe25_sqrn(z_20_0, 20), z_20_0);     // 2^40 - 1
  const Fe25 z_50_0 = fe25_mul(fe25_sqrn(z_40_0, 10), z_10_0);     // 2^50 - 1
  const Fe25 z_100_0 = fe25_mul(fe25_sqrn(z_50_0, 50), z_50_0);    // 2^100 - 1
  const Fe25 z_200_0 = fe25_mul(fe25_sqrn(z_100_0, 100), z_100_0); // 2^200 - 1
  const Fe25 z_250_0 = fe25_mul(fe25_sqrn(z_200_0, 50), z_50_0);   // 2^250 - 1
  return fe25_mul(fe25_sqrn(z_250_0, 5), z11);                     // 2^255 - 21
}
// 8 words -> TIGHT (even limbs < 2^26, odd < 2^25).  Bit 255 is dropped;
// values in [p, 2^255) are accepted as they are.
ZK_HD Fe25 fe25_load(const uint32_t* w) {
  Fe25 r;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    const int bit = (51 * i + 1) / 2;  // ceil(25.5 i)
    const int q = bit >> 5, s = bit & 31;
    uint64_t x = w[q];
    if (q + 1 < 8) x |= (uint64_t)w[q + 1] << 32;
    r.v[i] = (uint32_t)(x >> s) & ((i & 1) ? FE25_M25 : FE25_M26);
  }
  return r;
}
// LOOSE -> the canonical 32 bytes (8 words) of the value mod p
ZK_HD void fe25_store(uint32_t* w, const Fe25& a) {
  uint32_t h[10];
#pragma unroll
  for (int i = 0; i < 10; i++) h[i] = a.v[i];
  // two carry passes: after the first limb 0 is below 2^26 + 19 * 4 and the
  // others are in range, after the second every limb is: value < 2^255
#pragma unroll
  for (int pass = 0; pass < 2; pass++) {
#pragma unroll
    for (int i = 0; i < 9; i++) {
      h[i + 1] += h[i] >> ((i & 1) ? 25 : 26);
      h[i] &= (i & 1) ? FE25_M25 : FE25_M26;
    }
    h[0] += 19 * (h[9] >> 25);
    h[9] &= FE25_M25;
  }
  // q = 1 iff value >= p, iff value + 19 >= 2^255
  uint32_t q = (h[0] + 19) >> 26;
#pragma unroll
  for (int i = 1; i < 10; i++) q = (h[i] + q) >> ((i & 1) ? 25 : 26);
  h[0] += 19 * q;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    h[i + 1] += h[i] >> ((i & 1) ? 25 : 26);
    h[i] &= (i & 1) ? FE25_M25 : FE25_M26;
  }
  h[9] &= FE25_M25;  // drops 2^255 when q = 1
  uint64_t acc = 0;
  int have = 0, out = 0;
#pragma unroll
  for (int i = 0; i < 10; i++) {
    acc |= (uint64_t)h[i] << have;
    have += (i & 1) ? 25 : 26;
    if (have >= 32) {
      w[out++] = (uint32_t)acc;
      acc >>= 32;
      have -= 32;
    }
  }
  w[7] = (uint32_t)acc;  // 255 bits: the last word has 31
}

// -------------------------------------------------------------------- X25519
// out = X25519(scalar, u), RFC 7748 section 5: the scalar is clamped here, u's
// bit 255 is ignored, u >= p is taken mod p.  255 ladder steps from bit 254
// down, conditional swaps only.  No contributory check: a low-order u gives
// the all-zero output (z2 = 0, and 0^(p-2) = 0), as x25519-dalek's
// diffie_hellman does.
ZK_HD void x25519(uint32_t* out, const uint32_t* scalar, const uint32_t* u) {
  uint32_t k[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = scalar[i];
  k[0] &= 0xFFFFFFF8u;
  k[7] = (k[7] & 0x7FFFFFFFu) | 0x40000000u;
  const Fe25 x1 = fe25_load(u);
  Fe25 x2 = fe25_one(), z2 = fe25_zero(), x3 = x1, z3 = fe25_one();
  uint32_t swap = 0;
#pragma unroll 1
  for (int t = 254; t >= 0; t--) {
    const uint32_t kt = (k[t >> 5] >> (t & 31)) & 1;
    swap ^= kt;
    fe25_cswap(x2, x3, swap);
    fe25_cswap(z2, z3, swap);
    swap = kt;
    const Fe25 A = fe25_add(x2, z2), B = fe25_sub(x2, z2);
    const Fe25 AA = fe25_sqr(A), BB = fe25_sqr(B);
    const Fe25 E = fe25_sub(AA, BB);
    const Fe25 C = fe25_add(x3, z3), D = fe25_sub(x3, z3);
    const Fe25 DA = fe25_mul(D, A), CB = fe25_mul(C, B);
    x3 = fe25_sqr(fe25_add(DA, CB));
    z3 = fe25_mul(x1, fe25_sqr(fe25_sub(DA, CB)));
    x2 = fe25_mul(AA, BB);
    z2 = fe25_mul(E, fe25_add(AA, fe25_mul121665(E)));
  }
  fe25_cswap(x2, x3, swap);
  fe25_cswap(z2, z3, swap);
  fe25_store(out, fe25_mul(x2, fe25_invert(z2)));
}

// -------------------------------------------------------------------- BLAKE3
ZK_HD uint32_t nc_rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
ZK_HD uint32_t nc_rotl(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }
constexpr uint32_t B3_CHUNK_START = 1, B3_CHUNK_END = 2, B3_ROOT = 8, B3_DERIVE_KEY_CONTEXT = 1u << 5,
                   B3_DERIVE_KEY_MATERIAL = 1u << 6;
#define ZK_B3_G(a, b, c, d, x, y) \
  do {                            \
    a = a + b + (x);              \
    d = nc_rotr(d ^ a, 16);       \
    c = c + d;                    \
    b = nc_rotr(b ^ c, 12);       \
    a = a + b + (y);              \
    d = nc_rotr(d ^ a, 8);        \
    c = c + d;                    \
    b = nc_rotr(b ^ c, 7);        \
  } while (0)
// the first 8 output words of one compression (counter < 2^32)
ZK_HD void blake3_compress8(uint32_t* out, const uint32_t* cv, const uint32_t* block, uint32_t counter,
                            uint32_t block_len, uint32_t flags) {
  uint32_t s0 = cv[0], s1 = cv[1], s2 = cv[2], s3 = cv[3], s4 = cv[4], s5 = cv[5], s6 = cv[6], s7 = cv[7];
  uint32_t s8 = 0x6A09E667u, s9 = 0xBB67AE85u, s10 = 0x3C6EF372u, s11 = 0xA54FF53Au;
  uint32_t s12 = counter, s13 = 0, s14 = block_len, s15 = flags;
  uint32_t m[16], t[16];
#pragma unroll
  for (int i = 0; i < 16; i++) m[i] = block[i];
#pragma unroll
  for (int r = 0; r < 7; r++) {
    ZK_B3_G(s0, s4, s8, s12, m[0], m[1]);
    ZK_B3_G(s1, s5, s9, s13, m[2], m[3]);
    ZK_B3_G(s2, s6, s10, s14, m[4], m[5]);
    ZK_B3_G(s3, s7, s11, s15, m[6], m[7]);
    ZK_B3_G(s0, s5, s10, s15, m[8], m[9]);
    ZK_B3_G(s1, s6, s11, s12, m[10], m[11]);
    ZK_B3_G(s2, s7, s8, s13, m[12], m[13]);
    ZK_B3_G(s3, s4, s9, s14, m[14], m[15]);
    if (r < 6) {
      t[0] = m[2], t[1] = m[6], t[2] = m[3], t[3] = m[10], t[4] = m[7], t[5] = m[0], t[6] = m[4], t[7] = m[13];
      t[8] = m[1], t[9] = m[11], t[10] = m[12], t[11] = m[5], t[12] = m[9], t[13] = m[14], t[14] = m[15], t[15] = m[8];
#pragma unroll
      for (int i = 0; i < 16; i++) m[i] = t[i];
    }
  }
  out[0] = s0 ^ s8, out[1] = s1 ^ s9, out[2] = s2 ^ s10, out[3] = s3 ^ s11;
  out[4] = s4 ^ s12, out[5] = s5 ^ s13, out[6] = s6 ^ s14, out[7] = s7 ^ s15;
}
// derive_key(context, shared_secret || ephemeral_pk): ctx_key = the 8 words of
// the context's hash under DERIVE_KEY_CONTEXT (made once on the host); the 64
// bytes of material are one block, one chunk and the root
ZK_HD void note_key(uint32_t* key, const uint32_t* ctx_key, const uint32_t* shared, const uint32_t* epk) {
  uint32_t block[16];
#pragma unroll
  for (int i = 0; i < 8; i++) block[i] = shared[i], block[8 + i] = epk[i];
  blake3_compress8(key, ctx_key, block, 0, 64, B3_CHUNK_START | B3_CHUNK_END | B3_ROOT | B3_DERIVE_KEY_MATERIAL);
}

// ------------------------------------------------------------------ ChaCha20
#define ZK_CC_QR(a, b, c, d) \
  do {                       \
    a += b;                  \
    d = nc_rotl(d ^ a, 16);  \
    c += d;                  \
    b = nc_rotl(b ^ c, 12);  \
    a += b;                  \
    d = nc_rotl(d ^ a, 8);   \
    c += d;                  \
    b = nc_rotl(b ^ c, 7);   \
  } while (0)
// one 64-byte block of key stream (RFC 8439 section 2.3)
ZK_HD void chacha20_block(uint32_t* out, const uint32_t* key, uint32_t counter, const uint32_t* nonce) {
  const uint32_t i0 = 0x61707865u, i1 = 0x3320646Eu, i2 = 0x79622D32u, i3 = 0x6B206574u;
  uint32_t x0 = i0, x1 = i1, x2 = i2, x3 = i3, x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3], x8 = key[4],
           x9 = key[5], x10 = key[6], x11 = key[7], x12 = counter, x13 = nonce[0], x14 = nonce[1], x15 = nonce[2];
#pragma unroll 1
  for (int r = 0; r < 10; r++) {
    ZK_CC_QR(x0, x4, x8, x12);
    ZK_CC_QR(x1, x5, x9, x13);
    ZK_CC_QR(x2, x6, x10, x14);
    ZK_CC_QR(x3, x7, x11, x15);
    ZK_CC_QR(x0, x5, x10, x15);
    ZK_CC_QR(x1, x6, x11, x12);
    ZK_CC_QR(x2, x7, x8, x13);
    ZK_CC_QR(x3, x4, x9, x14);
  }
  out[0] = x0 + i0, out[1] = x1 + i1, out[2] = x2 + i2, out[3] = x3 + i3;
  out[4] = x4 + key[0], out[5] = x5 + key[1], out[6] = x6 + key[2], out[7] = x7 + key[3];
  out[8] = x8 + key[4], out[9] = x9 + key[5], out[10] = x10 + key[6], out[11] = x11 + key[7];
  out[12] = x12 + counter, out[13] = x13 + nonce[0], out[14] = x14 + nonce[1], out[15] = x15 + nonce[2];
}

// ------------------------------------------------------------------ Poly1305
// h and r in five 26-bit limbs.  Between blocks h[0], h[2..4] < 2^26 and h[1]
// < 2^26 + 2^7; a block adds a 129-bit value, so the limbs entering the
// product are below 2^27 and a column of five products (r < 2^26, 5 r < 2^29)
// below 2^59.
struct Poly1305 {
  uint32_t r[5], h[5], pad[4];
};
ZK_HD void poly1305_init(Poly1305& st, const uint32_t* key) {
  st.r[0] = key[0] & 0x3FFFFFFu;
  st.r[1] = ((key[0] >> 26) | (key[1] << 6)) & 0x3FFFF03u;
  st.r[2] = ((key[1] >> 20) | (key[2] << 12)) & 0x3FFC0FFu;
  st.r[3] = ((key[2] >> 14) | (key[3] << 18)) & 0x3F03FFFu;
  st.r[4] = (key[3] >> 8) & 0x00FFFFFu;
#pragma unroll
  for (int i = 0; i < 5; i++) st.h[i] = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) st.pad[i] = key[4 + i];
}
// h = (h + m + hibit 2^128) r, partially reduced; m: 16 bytes as 4 words,
// hibit 1 for a full block, 0 for a last block that carries its own 0x01 byte
ZK_HD void poly1305_block(Poly1305& st, const uint32_t* m, uint32_t hibit) {
  const uint32_t r0 = st.r[0], r1 = st.r[1], r2 = st.r[2], r3 = st.r[3], r4 = st.r[4];
  const uint32_t s1 = r1 * 5, s2 = r2 * 5, s3 = r3 * 5, s4 = r4 * 5;
  const uint32_t h0 = st.h[0] + (m[0] & 0x3FFFFFFu);
  const uint32_t h1 = st.h[1] + (((m[0] >> 26) | (m[1] << 6)) & 0x3FFFFFFu);
  const uint32_t h2 = st.h[2] + (((m[1] >> 20) | (m[2] << 12)) & 0x3FFFFFFu);
  const uint32_t h3 = st.h[3] + (((m[2] >> 14) | (m[3] << 18)) & 0x3FFFFFFu);
  const uint32_t h4 = st.h[4] + ((m[3] >> 8) | (hibit << 24));
  uint64_t d0 = (uint64_t)h0 * r0 + (uint64_t)h1 * s4 + (uint64_t)h2 * s3 + (uint64_t)h3 * s2 + (uint64_t)h4 * s1;
  uint64_t d1 = (uint64_t)h0 * r1 + (uint64_t)h1 * r0 + (uint64_t)h2 * s4 + (uint64_t)h3 * s3 + (uint64_t)h4 * s2;
  uint64_t d2 = (uint64_t)h0 * r2 + (uint64_t)h1 * r1 + (uint64_t)h2 * r0 + (uint64_t)h3 * s4 + (uint64_t)h4 * s3;
  uint64_t d3 = (uint64_t)h0 * r3 + (uint64_t)h1 * r2 + (uint64_t)h2 * r1 + (uint64_t)h3 * r0 + (uint64_t)h4 * s4;
  uint64_t d4 = (uint64_t)h0 * r4 + (uint64_t)h1 * r3 + (uint64_t)h2 * r2 + (uint64_t)h3 * r1 + (uint64_t)h4 * r0;
  d1 += d0 >> 26;
  d2 += d1 >> 26;
  d3 += d2 >> 26;
  d4 += d3 >> 26;
  uint32_t n0 = (uint32_t)d0 & 0x3FFFFFFu;
  n0 += (uint32_t)(d4 >> 26) * 5;  // d4 has no 5 r term: < 2^55.4, so this is below 2^26 + 2^31.7
  st.h[1] = ((uint32_t)d1 & 0x3FFFFFFu) + (n0 >> 26);
  st.h[0] = n0 & 0x3FFFFFFu;
  st.h[2] = (uint32_t)d2 & 0x3FFFFFFu;
  st.h[3] = (uint32_t)d3 & 0x3FFFFFFu;
  st.h[4] = (uint32_t)d4 & 0x3FFFFFFu;
}
// tag = ((h mod 2^130 - 5) + s) mod 2^128, 4 words
ZK_HD void poly1305_finish(const Poly1305& st, uint32_t* tag) {
  uint32_t h0 = st.h[0], h1 = st.h[1], h2 = st.h[2], h3 = st.h[3], h4 = st.h[4], c;
  c = h1 >> 26, h1 &= 0x3FFFFFFu, h2 += c;
  c = h2 >> 26, h2 &= 0x3FFFFFFu, h3 += c;
  c = h3 >> 26, h3 &= 0x3FFFFFFu, h4 += c;
  c = h4 >> 26, h4 &= 0x3FFFFFFu, h0 += c * 5;
  c = h0 >> 26, h0 &= 0x3FFFFFFu, h1 += c;
  // g = h + 5 - 2^130; take g when it did not borrow (h >= p)
  uint32_t g0 = h0 + 5;
  c = g0 >> 26, g0 &= 0x3FFFFFFu;
  uint32_t g1 = h1 + c;
  c = g1 >> 26, g1 &= 0x3FFFFFFu;
  uint32_t g2 = h2 + c;
  c = g2 >> 26, g2 &= 0x3FFFFFFu;
  uint32_t g3 = h3 + c;
  c = g3 >> 26, g3 &= 0x3FFFFFFu;
  const uint32_t g4 = h4 + c - (1u << 26);
  const uint32_t take_g = (g4 >> 31) - 1;  // all ones when g4 did not go negative
  h0 = (h0 & ~take_g) | (g0 & take_g);
  h1 = (h1 & ~take_g) | (g1 & take_g);
  h2 = (h2 & ~take_g) | (g2 & take_g);
  h3 = (h3 & ~take_g) | (g3 & take_g);
  h4 = (h4 & ~take_g) | (g4 & take_g);
  const uint32_t w0 = h0 | (h1 << 26), w1 = (h1 >> 6) | (h2 << 20), w2 = (h2 >> 12) | (h3 << 14),
                 w3 = (h3 >> 18) | (h4 << 8);
  uint64_t f = (uint64_t)w0 + st.pad[0];
  tag[0] = (uint32_t)f;
  f = (uint64_t)w1 + st.pad[1] + (f >> 32);
  tag[1] = (uint32_t)f;
  f = (uint64_t)w2 + st.pad[2] + (f >> 32);
  tag[2] = (uint32_t)f;
  f = (uint64_t)w3 + st.pad[3] + (f >> 32);
  tag[3] = (uint32_t)f;
}

// ------------------------------------------------------ bytes through words
// the 4 bytes at byte offset `off` of the string at word pointer p; reads the
// second word only when the offset is not a multiple of 4
ZK_HD uint32_t nc_word_at(const uint32_t* p, uint32_t off) {
  const uint32_t q = off >> 2, s = (off & 3) * 8;
  uint32_t x = p[q];
  if (s) x = (x >> s) | (p[q + 1] << (32 - s));
  return x;
}
// word `w` (bytes 4w .. 4w + 3) of the first `len` bytes of the string at p,
// bytes from `len` on read as zero; no word wholly past `len` is read
ZK_HD uint32_t nc_word_clip(const uint32_t* p, uint32_t w, uint32_t len) {
  const uint32_t b = 4 * w;
  if (b >= len) return 0;
  const uint32_t x = p[w];
  return len - b >= 4 ? x : x & ((1u << (8 * (len - b))) - 1);
}
// Poly1305 of an arbitrary message (RFC 8439 section 2.5): full blocks with
// the high bit, a last partial block with a 0x01 byte after its end
ZK_HD void poly1305_mac(uint32_t* tag, const uint32_t* key, const uint32_t* msg, uint32_t len) {
  Poly1305 st;
  poly1305_init(st, key);
  uint32_t m[4];
  uint32_t off = 0;
#pragma unroll 1
  for (; off + 16 <= len; off += 16) {
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = msg[off / 4 + i];
    poly1305_block(st, m, 1);
  }
  if (off < len) {
    const uint32_t rest = len - off;
#pragma unroll
    for (int i = 0; i < 4; i++) {
      m[i] = nc_word_clip(msg + off / 4, i, rest);
      if (rest / 4 == (uint32_t)i) m[i] |= 1u << (8 * (rest & 3));
    }
    poly1305_block(st, m, 0);
  }
  poly1305_finish(st, tag);
}

// -------------------------------------------- ChaCha20-Poly1305, open (AEAD)
// ct: `len` bytes, the 16-byte tag last; empty AAD.  len < 16 is "no".
constexpr uint32_t AEAD_TAG = 16;
// does the tag match?  The one-time key is the first 32 bytes of block 0; the
// MAC runs over body || pad16 || le64(0) || le64(body length); all 16 tag
// bytes are compared.
ZK_HD bool aead_tag_ok(const uint32_t* key, const uint32_t* nonce, const uint32_t* ct, uint32_t len) {
  if (len < AEAD_TAG) return false;
  const uint32_t body = len - AEAD_TAG;
  uint32_t ks[16];
  chacha20_block(ks, key, 0, nonce);
  Poly1305 st;
  poly1305_init(st, ks);
  uint32_t m[4];
#pragma unroll 1
  for (uint32_t off = 0; off < body; off += 16) {
#pragma unroll
    for (int i = 0; i < 4; i++) m[i] = nc_word_clip(ct, off / 4 + i, body);
    poly1305_block(st, m, 1);
  }
  m[0] = 0, m[1] = 0, m[2] = body, m[3] = 0;
  poly1305_block(st, m, 1);
  uint32_t tag[4];
  poly1305_finish(st, tag);
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 4; i++) d |= tag[i] ^ nc_word_at(ct, body + 4 * i);
  return d == 0;
}
// the plaintext words [16 b, 16 b + 16) of the body: key stream block b + 1
// over the ciphertext, bytes past the body zero
ZK_HD void aead_plain_block(uint32_t* pt, const uint32_t* key, const uint32_t* nonce, const uint32_t* ct,
                            uint32_t body, uint32_t b) {
  uint32_t ks[16];
  chacha20_block(ks, key, b + 1, nonce);
#pragma unroll
  for (int i = 0; i < 16; i++) {
    const uint32_t w = 16 * b + i;
    const uint32_t c = nc_word_clip(ct, w, body);
    const uint32_t left = 4 * w >= body ? 0 : body - 4 * w;
    pt[i] = c ^ (left >= 4 ? ks[i] : left ? ks[i] & ((1u << (8 * left)) - 1) : 0);
  }
}

// ------------------------------------------------------------ note plaintext
// value u64 | randomness 32 | memo_len u16 | memo (sdk/privacy/src/encryption.rs)
constexpr uint32_t NOTE_HEAD = 42;                      // bytes before the memo
constexpr uint32_t NOTE_MIN_CT = NOTE_HEAD + AEAD_TAG;  // 58: the shortest ciphertext that parses
// results of one (key, note) pair (zkmi.h ZKMI_SCAN_*)
constexpr uint32_t SCAN_NOT_MINE = 0, SCAN_MALFORMED = 1, SCAN_WRONG_COMMITMENT = 2, SCAN_HIT = 3;
struct NoteHead {
  uint32_t value[2], randomness[8], memo_len;
};
// head of the plaintext from its first block (pt: 16 words, body bytes in
// all); false when the body is shorter than 42 bytes or the declared memo
// passes its end.  Bytes after the memo are accepted and ignored.
ZK_HD bool note_parse(const uint32_t* pt, uint32_t body, NoteHead& h) {
  h.value[0] = pt[0], h.value[1] = pt[1];
#pragma unroll
  for (int i = 0; i < 8; i++) h.randomness[i] = pt[2 + i];
  h.memo_len = pt[10] & 0xFFFFu;
  return body >= NOTE_HEAD && body - NOTE_HEAD >= h.memo_len;
}
// Memo word j (bytes 4j .. 4j + 3 of the memo, bytes past memo_len zero) lies
// at plaintext bytes 42 + 4j: the high half of plaintext word 10 + j and the
// low half of word 11 + j.  memo_words(len) words hold a memo.
ZK_HD uint32_t note_memo_words(uint32_t memo_len) { return (memo_len + 3) / 4; }
ZK_HD uint32_t note_memo_word(uint32_t lo_word, uint32_t hi_word, uint32_t j, uint32_t memo_len) {
  const uint32_t x = (lo_word >> 16) | (hi_word << 16);
  const uint32_t left = memo_len - 4 * j;  // j < memo_words: left >= 1
  return left >= 4 ? x : x & ((1u << (8 * left)) - 1);
}
// the whole memo of a parsed note into out (memo_words(memo_len) words);
// block after block, every index static
ZK_HD void note_memo(uint32_t* out, const uint32_t* key, const uint32_t* nonce, const uint32_t* ct, uint32_t body,
                     uint32_t memo_len) {
  const uint32_t nw = note_memo_words(memo_len);
  if (nw == 0) return;
  const uint32_t blocks = (NOTE_HEAD + memo_len + 63) / 64;
  uint32_t prev = 0;
#pragma unroll 1
  for (uint32_t b = 0; b < blocks; b++) {
    uint32_t pt[16];
    aead_plain_block(pt, key, nonce, ct, body, b);
#pragma unroll
    for (int i = 0; i < 16; i++) {
      const uint32_t w = 16 * b + i;  // plaintext word: completes memo word w - 11
      if (w >= 11 && w - 11 < nw) out[w - 11] = note_memo_word(prev, pt[i], w - 11, memo_len);
      prev = pt[i];
    }
  }
  // a memo that ends in the low half of the word after the last block's
  if (16 * blocks >= 11 && 16 * blocks - 11 < nw) out[16 * blocks - 11] = note_memo_word(prev, 0, 16 * blocks - 11, memo_len);
}

}  // namespace zk
