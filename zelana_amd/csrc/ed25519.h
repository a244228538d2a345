// ed25519.h — the pieces of an Ed25519 verification: SHA-512,
// reduction mod the group order L, Edwards decompression, point doubling and
// addition in extended coordinates, compression, and the double-scalar
// multiplication [s]B + [k](-A) with the bytewise compare that decides a
// signature.  The field is note_crypt.h's Fe25 (GF(2^255 - 19) in 10 x 25.5-bit
// limbs) and nothing of it is repeated here.  Host+device like note_crypt.h:
// the kernels of ed25519.hip, the device probe (tests/device/ed25519_probe.hip)
// and the stand-alone host check (tests/host/ed25519_check.cpp) compile the very
// same functions.  No HIP call is made here.
//
// Semantics: ed25519-dalek 2.2.0 `verify` (not verify_strict) over
// curve25519-dalek 4.1.3, which the reference's tx_router.rs calls.  The
// equation has no cofactor, a small-order A is accepted, s >= L is refused, a
// non-canonical A is reduced and accepted, and R is never decoded: the
// canonical bytes of [s]B + [k](-A) are compared with the 32 bytes given.
//
// All data is public, so nothing here is constant time; what is kept is
// uniform control flow: the scalar multiplication runs the same doublings and
// additions for every input, and table entries are picked by index (the
// identity is entry 0), never by a branch.
//
// Byte strings cross this header as little-endian u32 words, as in
// note_crypt.h (a 32-byte string is 8 words); messages are read through a byte
// functor.  Field elements inside a point are TIGHT unless a comment says
// LOOSE (note_crypt.h's bounds).
#pragma once
#include "note_crypt.h"

namespace zk {

// results of one verification (zkmi.h ZKMI_SIG_*)
constexpr uint32_t SIG_OK = 0, SIG_BAD_PUBKEY = 1, SIG_BAD_S = 2, SIG_MISMATCH = 3;

// ------------------------------------------------------------------- SHA-512
struct Sha512K {
  static constexpr uint64_t K[80] = {
      0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull,
      0x3956c25bf348b538ull, 0x59f111f1b605d019ull, 0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull,
      0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
      0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull,
      0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull, 0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull,
      0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
      0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull,
      0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull, 0x06ca6351e003826full, 0x142929670a0e6e70ull,
      0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
      0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull,
      0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull, 0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull,
      0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
      0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull,
      0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull, 0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull,
      0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
      0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull,
      0xca273eceea26619cull, 0xd186b8c721c0c207ull, 0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull,
      0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
      0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull,
      0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull, 0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
};
struct Sha512 {
  uint64_t h[8];
};
ZK_HD uint64_t sha_rotr(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }
ZK_HD uint32_t sha_bswap32(uint32_t x) {
  return (x >> 24) | ((x >> 8) & 0xFF00u) | ((x << 8) & 0xFF0000u) | (x << 24);
}
ZK_HD void sha512_init(Sha512& st) {
  st.h[0] = 0x6a09e667f3bcc908ull, st.h[1] = 0xbb67ae8584caa73bull, st.h[2] = 0x3c6ef372fe94f82bull;
  st.h[3] = 0xa54ff53a5f1d36f1ull, st.h[4] = 0x510e527fade682d1ull, st.h[5] = 0x9b05688c2b3e6c1full;
  st.h[6] = 0x1f83d9abfb41bd6bull, st.h[7] = 0x5be0cd19137e2179ull;
}
// one 128-byte block, given as its 16 big-endian words.  The schedule is a
// ring of 16 words whose indices are all static: five passes of 16 unrolled
// rounds, the ring advanced from the second pass on.
ZK_HD void sha512_block(Sha512& st, const uint64_t* m) {
  uint64_t w[16];
#pragma unroll
  for (int i = 0; i < 16; i++) w[i] = m[i];
  uint64_t a = st.h[0], b = st.h[1], c = st.h[2], d = st.h[3], e = st.h[4], f = st.h[5], g = st.h[6], h = st.h[7];
#pragma unroll 1
  for (int r = 0; r < 80; r += 16) {
#pragma unroll
    for (int i = 0; i < 16; i++) {
      if (r) {
        const uint64_t x = w[(i + 1) & 15], y = w[(i + 14) & 15];
        w[i] += (sha_rotr(x, 1) ^ sha_rotr(x, 8) ^ (x >> 7)) + w[(i + 9) & 15] +
                (sha_rotr(y, 19) ^ sha_rotr(y, 61) ^ (y >> 6));
      }
      const uint64_t t1 = h + (sha_rotr(e, 14) ^ sha_rotr(e, 18) ^ sha_rotr(e, 41)) + ((e & f) ^ (~e & g)) +
                          Sha512K::K[r + i] + w[i];
      const uint64_t t2 = (sha_rotr(a, 28) ^ sha_rotr(a, 34) ^ sha_rotr(a, 39)) + ((a & b) ^ (a & c) ^ (b & c));
      h = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
  }
  st.h[0] += a, st.h[1] += b, st.h[2] += c, st.h[3] += d, st.h[4] += e, st.h[5] += f, st.h[6] += g, st.h[7] += h;
}
// SHA-512 of the `len` bytes at(0) .. at(len - 1) (len < 2^61), block by
// block: the standard padding (0x80, zeros, the bit length in the last 16
// bytes).  out: the 64 digest bytes as 16 little-endian words.  at() is never
// called with an index >= len.
template <class ByteAt>
ZK_HD void sha512(uint32_t* out, uint64_t len, const ByteAt& at) {
  Sha512 st;
  sha512_init(st);
  const uint64_t nblocks = (len + 17 + 127) / 128;
#pragma unroll 1
  for (uint64_t b = 0; b < nblocks; b++) {
    uint64_t m[16];
#pragma unroll
    for (int i = 0; i < 16; i++) {
      uint64_t x = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint64_t pos = 128 * b + 8 * i + j;
        x = (x << 8) | (pos < len ? (uint64_t)at(pos) : pos == len ? 0x80u : 0u);
      }
      m[i] = x;
    }
    if (b == nblocks - 1) m[15] = len * 8;  // bytes 112..127 of the last block lie past the 0x80: m[14] = 0
    sha512_block(st, m);
  }
#pragma unroll
  for (int i = 0; i < 8; i++) {
    out[2 * i] = sha_bswap32((uint32_t)(st.h[i] >> 32));
    out[2 * i + 1] = sha_bswap32((uint32_t)st.h[i]);
  }
}
// the bytes of a string held as little-endian words
struct WordBytes {
  const uint32_t* w;
  ZK_HD uint8_t operator()(uint64_t i) const { return (uint8_t)(w[i >> 2] >> (8 * (i & 3))); }
};

// ------------------------------------------------------------ scalars mod L
// L = 2^252 + 27742317777372353535851937790883648493
ZK_HD uint32_t sc_l_word(int i) {
  return i == 0 ? 0x5cf5d3edu : i == 1 ? 0x5812631au : i == 2 ? 0xa2f79cd6u : i == 3 ? 0x14def9deu : i == 7 ? 0x10000000u : 0u;
}
// r - L into t; -> the borrow (1 when r < L)
ZK_HD uint32_t sc_sub_l(uint32_t* t, const uint32_t* r) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)r[i] - sc_l_word(i) - borrow;
    t[i] = (uint32_t)d;
    borrow = (d >> 32) & 1;
  }
  return (uint32_t)borrow;
}
// s < L ?  (s: 8 words)
ZK_HD bool sc_is_canonical(const uint32_t* s) {
  uint32_t t[8];
  return sc_sub_l(t, s) != 0;
}
// the 512-bit little-endian integer x (16 words) mod L, 8 words.  The top 252
// bits are below L as they stand; the other 260 are shifted in one at a time,
// each followed by one conditional subtraction (r < L keeps 2 r + 1 < 2 L).
ZK_HD void sc_reduce512(uint32_t* r, const uint32_t* x) {
#pragma unroll
  for (int i = 0; i < 8; i++) r[i] = (x[8 + i] >> 4) | (i < 7 ? x[9 + i] << 28 : 0u);
#pragma unroll 1
  for (int bit = 259; bit >= 0; bit--) {
    uint32_t in = (x[bit >> 5] >> (bit & 31)) & 1;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const uint32_t out = r[i] >> 31;
      r[i] = (r[i] << 1) | in;
      in = out;
    }
    uint32_t t[8];
    const uint32_t keep = 0u - sc_sub_l(t, r);  // all ones when r < L
#pragma unroll
    for (int i = 0; i < 8; i++) r[i] = (r[i] & keep) | (t[i] & ~keep);
  }
}

// ------------------------------------------------------- field, a few more
ZK_HD Fe25 ed_words(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t w4, uint32_t w5, uint32_t w6,
                    uint32_t w7) {
  const uint32_t w[8] = {w0, w1, w2, w3, w4, w5, w6, w7};
  return fe25_load(w);
}
// d = -121665 / 121666, 2 d, sqrt(-1) = 2^((p - 1) / 4)
ZK_HD Fe25 ed_d() {
  return ed_words(0x135978a3u, 0x75eb4dcau, 0x4141d8abu, 0x00700a4du, 0x7779e898u, 0x8cc74079u, 0x2b6ffe73u, 0x52036ceeu);
}
ZK_HD Fe25 ed_2d() {
  return ed_words(0x26b2f159u, 0xebd69b94u, 0x8283b156u, 0x00e0149au, 0xeef3d130u, 0x198e80f2u, 0x56dffce7u, 0x2406d9dcu);
}
ZK_HD Fe25 ed_sqrtm1() {
  return ed_words(0x4a0ea0b0u, 0xc4ee1b27u, 0xad2fe478u, 0x2f431806u, 0x3dfbd7a7u, 0x2b4d0099u, 0x4fc1df0bu, 0x2b832480u);
}
// LOOSE -> TIGHT: -a
ZK_HD Fe25 fe25_neg(const Fe25& a) { return fe25_sub(fe25_zero(), a); }
// LOOSE: a = 0 mod p ?
ZK_HD bool fe25_is_zero(const Fe25& a) {
  uint32_t w[8];
  fe25_store(w, a);
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= w[i];
  return d == 0;
}
// bit = 1: b, bit = 0: a; any limbs
ZK_HD Fe25 fe25_select(const Fe25& a, const Fe25& b, uint32_t bit) {
  const uint32_t m = 0u - bit;
  Fe25 r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = a.v[i] ^ (m & (a.v[i] ^ b.v[i]));
  return r;
}
// LOOSE -> TIGHT: z^((p - 5) / 8) = z^(2^252 - 3), the chain of fe25_invert
// with another tail (251 squarings, 11 products)
ZK_HD Fe25 fe25_pow22523(const Fe25& z) {
  const Fe25 z2 = fe25_sqr(z);
  const Fe25 z9 = fe25_mul(fe25_sqrn(z2, 2), z);
  const Fe25 z11 = fe25_mul(z9, z2);
  const Fe25 z_5_0 = fe25_mul(fe25_sqr(z11), z9);
  const Fe25 z_10_0 = fe25_mul(fe25_sqrn(z_5_0, 5), z_5_0);
  const Fe25 z_20_0 = fe25_mul(fe25_sqrn(z_10_0, 10), z_10_0);
  const Fe25 z_40_0 = fe25_mul(fe25_sqrn(z_20_0, 20), z_20_0);
  const Fe25 z_50_0 = fe25_mul(fe25_sqrn(z_40_0, 10), z_10_0);
  const Fe25 z_100_0 = fe25_mul(fe25_sqrn(z_50_0, 50), z_50_0);
  const Fe25 z_200_0 = fe25_mul(fe25_sqrn(z_100_0, 100), z_100_0);
  const Fe25 z_250_0 = fe25_mul(fe25_sqrn(z_200_0, 50), z_50_0);
  return fe25_mul(fe25_sqrn(z_250_0, 2), z);
}

// -------------------------------------------------------------------- points
// -x^2 + y^2 = 1 + d x^2 y^2.  Extended coordinates: x = X / Z, y = Y / Z,
// T = X Y / Z.  With a = -1 a square and d none, the addition below is
// complete: it is right for every pair of points of the curve, doubling, the
// identity and the points of small order included.
struct EdPoint {
  Fe25 X, Y, Z, T;
};
// the second operand of an addition: Y + X (LOOSE), Y - X, Z, 2 d T
struct EdCached {
  Fe25 YpX, YmX, Z, T2d;
};
constexpr int ED_CACHED_WORDS = 40;
ZK_HD EdPoint ed_identity() {
  EdPoint p;
  p.X = fe25_zero(), p.Y = fe25_one(), p.Z = fe25_one(), p.T = fe25_zero();
  return p;
}
ZK_HD EdPoint ed_neg(const EdPoint& p) {
  EdPoint r;
  r.X = fe25_neg(p.X), r.Y = p.Y, r.Z = p.Z, r.T = fe25_neg(p.T);
  return r;
}
ZK_HD EdCached ed_to_cached(const EdPoint& p) {
  EdCached c;
  c.YpX = fe25_add(p.Y, p.X), c.YmX = fe25_sub(p.Y, p.X), c.Z = p.Z, c.T2d = fe25_mul(p.T, ed_2d());
  return c;
}
// 2 p (dbl-2008-hwcd, a = -1): 4 squarings and 3 products, 4 with T.  p.T is
// not read; without WANT_T the result's T is left as p's and must not be used.
template <bool WANT_T = true>
ZK_HD EdPoint ed_dbl(const EdPoint& p) {
  const Fe25 xx = fe25_sqr(p.X), yy = fe25_sqr(p.Y), zz = fe25_sqr(p.Z);
  const Fe25 h = fe25_add(yy, xx);                              // LOOSE
  const Fe25 g = fe25_sub(yy, xx);
  const Fe25 e = fe25_sub(fe25_sqr(fe25_add(p.X, p.Y)), h);     // 2 X Y
  const Fe25 f = fe25_sub(fe25_add(zz, zz), g);                 // 2 Z^2 - (Y^2 - X^2)
  EdPoint r;
  r.X = fe25_mul(e, f), r.Y = fe25_mul(h, g), r.Z = fe25_mul(g, f);
  r.T = WANT_T ? fe25_mul(e, h) : p.T;
  return r;
}
// p + q (add-2008-hwcd-3): 7 products, 8 with T
template <bool WANT_T = true>
ZK_HD EdPoint ed_add(const EdPoint& p, const EdCached& q) {
  const Fe25 a = fe25_mul(fe25_add(p.Y, p.X), q.YpX), b = fe25_mul(fe25_sub(p.Y, p.X), q.YmX);
  const Fe25 c = fe25_mul(p.T, q.T2d), zz = fe25_mul(p.Z, q.Z);
  const Fe25 d = fe25_add(zz, zz);                              // LOOSE
  const Fe25 e = fe25_sub(a, b), h = fe25_add(a, b);            // h LOOSE
  const Fe25 f = fe25_sub(d, c), g = fe25_sub(d, fe25_neg(c));  // d - c, d + c
  EdPoint r;
  r.X = fe25_mul(e, f), r.Y = fe25_mul(g, h), r.Z = fe25_mul(f, g);
  r.T = WANT_T ? fe25_mul(e, h) : p.T;
  return r;
}
// curve25519-dalek's CompressedEdwardsY::decompress.  b: 32 bytes as 8 words.
// Bit 255 is the sign of x; the low 255 bits are y and may be p or more (they
// stand for y mod p); x = 0 with the sign bit set is accepted.  -> false only
// when (y^2 - 1) / (d y^2 + 1) is no square; p is then left unwritten.
ZK_HD bool ed_decompress(EdPoint& p, const uint32_t* b) {
  const Fe25 y = fe25_load(b), one = fe25_one();
  const Fe25 yy = fe25_sqr(y);
  const Fe25 u = fe25_sub(yy, one), v = fe25_sub(fe25_mul(yy, ed_d()), fe25_neg(one));
  // x = u v^3 (u v^7)^((p - 5) / 8): a root of u / v, or of -u / v
  const Fe25 v3 = fe25_mul(fe25_sqr(v), v);
  const Fe25 v7 = fe25_mul(fe25_sqr(v3), v);
  Fe25 x = fe25_mul(fe25_mul(u, v3), fe25_pow22523(fe25_mul(u, v7)));
  const Fe25 c = fe25_mul(v, fe25_sqr(x));
  const bool plain = fe25_is_zero(fe25_sub(c, u)), flipped = fe25_is_zero(fe25_add(c, u));
  x = fe25_select(x, fe25_mul(x, ed_sqrtm1()), (flipped && !plain) ? 1u : 0u);
  if (!plain && !flipped) return false;
  uint32_t xb[8];
  fe25_store(xb, x);
  x = fe25_select(x, fe25_neg(x), (xb[0] & 1) ^ (b[7] >> 31));
  p.X = x, p.Y = y, p.Z = one, p.T = fe25_mul(x, y);
  return true;
}
// the canonical 32 bytes of p: y mod p with the parity of x mod p in bit 255
ZK_HD void ed_compress(uint32_t* out, const EdPoint& p) {
  const Fe25 zi = fe25_invert(p.Z);
  uint32_t xb[8];
  fe25_store(xb, fe25_mul(p.X, zi));
  fe25_store(out, fe25_mul(p.Y, zi));
  out[7] |= (xb[0] & 1) << 31;
}
// the base point: y = 4 / 5, x even
ZK_HD EdPoint ed_base() {
  const uint32_t b[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                         0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
  EdPoint p = ed_identity();
  (void)ed_decompress(p, b);
  return p;
}

// ------------------------------------------------- double-scalar multiplication
// Fixed 4-bit windows: a table holds j p for j = 0 .. 15, entry 0 the identity.
constexpr int ED_WINDOW = 4, ED_TABLE = 16, ED_WINDOWS = 64;
// put(j, cached j p) for j = 0 .. 15: 14 additions
template <class Put>
ZK_HD void ed_build_table(const EdPoint& p, const Put& put) {
  const EdCached c1 = ed_to_cached(p);
  put(0, ed_to_cached(ed_identity()));
  put(1, c1);
  EdPoint q = p;
#pragma unroll 1
  for (int j = 2; j < ED_TABLE; j++) {
    q = ed_add(q, c1);
    put(j, ed_to_cached(q));
  }
}
// [s]B + [k]Q, s and k 256-bit scalars as 8 words, tb(j) = cached j B and
// tq(j) = cached j Q.  Every input takes the same path: 64 windows from the
// top, each four doublings and two additions.
template <class TabB, class TabQ>
ZK_HD EdPoint ed_double_scalar_mul(const uint32_t* s, const uint32_t* k, const TabB& tb, const TabQ& tq) {
  EdPoint acc = ed_identity();
#pragma unroll 1
  for (int w = ED_WINDOWS - 1; w >= 0; w--) {
    acc = ed_dbl<false>(acc);
    acc = ed_dbl<false>(acc);
    acc = ed_dbl<false>(acc);
    acc = ed_dbl<true>(acc);
    const uint32_t js = (s[w >> 3] >> (4 * (w & 7))) & 15, jk = (k[w >> 3] >> (4 * (w & 7))) & 15;
    acc = ed_add<true>(acc, tb(js));
    acc = ed_add<false>(acc, tq(jk));
  }
  return acc;
}
// a table in an array of its own
struct EdTableArray {
  EdCached* t;
  ZK_HD void operator()(int j, const EdCached& c) const { t[j] = c; }
  ZK_HD const EdCached& operator()(uint32_t j) const { return t[j]; }
};
// R_bytes == compress([s]B + [k](-A)) ?  (dalek's recompute_R and its compare.)
// a: the decompressed A; tb(j) = cached j B.  `scratch` holds the table of -A.
template <class TabB>
ZK_HD bool ed_verify_point(const uint32_t* r_bytes, const EdPoint& a, const uint32_t* k, const uint32_t* s,
                           const TabB& tb, EdCached* scratch) {
  const EdTableArray tq{scratch};
  ed_build_table(ed_neg(a), tq);
  uint32_t got[8];
  ed_compress(got, ed_double_scalar_mul(s, k, tb, tq));
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= got[i] ^ r_bytes[i];
  return d == 0;
}
// The same from A's bytes, with tables of its own (2 x 16 cached points on the
// stack: the form the checks and the probe run; the kernels keep the table of
// B in LDS and the table of -A in the workspace).  -> 1 the equation holds, 0
// it does not, 2 A does not decompress.
ZK_HD uint32_t ed_verify_core(const uint32_t* r_bytes, const uint32_t* a_bytes, const uint32_t* k, const uint32_t* s) {
  EdPoint a;
  if (!ed_decompress(a, a_bytes)) return 2;
  EdCached tb[ED_TABLE], tq[ED_TABLE];
  ed_build_table(ed_base(), EdTableArray{tb});
  return ed_verify_point(r_bytes, a, k, s, EdTableArray{tb}, tq) ? 1u : 0u;
}
// k = SHA-512(R || A || M) mod L over the bytes as given.  sig: 16 words (R
// first), pk: 8 words, msg(i) = byte i of the message.
template <class ByteAt>
struct EdChallengeBytes {
  const uint32_t *r, *a;
  const ByteAt& m;
  ZK_HD uint8_t operator()(uint64_t i) const {
    return i < 32 ? WordBytes{r}(i) : i < 64 ? WordBytes{a}(i - 32) : m(i - 64);
  }
};
template <class ByteAt>
ZK_HD void ed_challenge(uint32_t* k, const uint32_t* sig, const uint32_t* pk, uint64_t len, const ByteAt& msg) {
  uint32_t h[16];
  sha512(h, 64 + len, EdChallengeBytes<ByteAt>{sig, pk, msg});
  sc_reduce512(k, h);
}
// a whole verification -> SIG_*: the key first, then s, then the equation
template <class ByteAt>
ZK_HD uint32_t ed_verify(const uint32_t* pk, const uint32_t* sig, uint64_t len, const ByteAt& msg) {
  EdPoint a;
  if (!ed_decompress(a, pk)) return SIG_BAD_PUBKEY;
  if (!sc_is_canonical(sig + 8)) return SIG_BAD_S;
  uint32_t k[8];
  ed_challenge(k, sig, pk, len, msg);
  EdCached tb[ED_TABLE], tq[ED_TABLE];
  ed_build_table(ed_base(), EdTableArray{tb});
  return ed_verify_point(sig, a, k, sig + 8, EdTableArray{tb}, tq) ? SIG_OK : SIG_MISMATCH;
}

}  // namespace zk
