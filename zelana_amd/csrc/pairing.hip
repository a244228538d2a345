// pairing.hip — batched Groth16 verification (zkmi_groth16_verify_many,
// DESIGN.md §2.7): two kernels on the context stream,
//   k_verify_prepare  one lane per proof: point validation as
//                     zkmi_groth16_verify's, rho_i A_i and rho_i C_i
//   k_miller          one lane per pair: the Tate Miller loop of pairing.h
// and the host half in verify.cpp (verify_many_combine): one final
// exponentiation for the batch, bisection when the combined check fails.
// And exact per-proof verdicts (zkmi_groth16_verify_each):
//   k_verify_each_prepare  the same validation, the pairs (A_i, B_i), (-C_i, delta)
//   k_verify_input_terms / k_verify_inputs  -X_i = -(IC[0] + sum_j x_ij IC[j+1])
//   k_miller               over 3 nb + 1 pairs
//   k_final_exp            one lane per proof: the final exponentiation and
//                          the verdict, the only thing downloaded
// which verify_many also uses for the proofs its bisection leaves undecided
// once a probe budget (zkmi_ctx_set_verify_probes) is spent.
// Both also take the proofs as wire bytes (zkmi_groth16_verify_*_encoded,
// DESIGN.md §2.9):
//   k_proof_decode / k_proof_decode_flag / k_proof_decode_fixed
//                          the encodings -> the words the prepare kernels read
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <vector>

#include "dev_io.h"
#include "pairing.h"
#include "proof_decode.h"
#include "verify_internal.h"
#include "zkmi_internal.h"

struct zkmi_vk {
  zkmi_ctx* ctx;
  zkv::Vk vk;
  uint64_t g2[3][16];  // beta, gamma, delta: canonical affine
};

namespace zk {

constexpr int VB = 64;        // lanes per block: one wave
constexpr int PAIR_WORDS = 48;  // G1 (16 u32) || G2 (32 u32), canonical affine, all-zero = infinity
constexpr int F12_WORDS = 96;   // 12 canonical Fq

__constant__ uint32_t VQ_MOD32[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u,
                                     0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
// 3 / (9 + u): the twist's b, canonical
__constant__ uint32_t VG2B_C0[8] = {0x24a138e5u, 0x3267e6dcu, 0x59dbefa3u, 0xb5b4c5e5u,
                                    0x1be06ac3u, 0x81be1899u, 0xceb8aaaeu, 0x2b149d40u};
__constant__ uint32_t VG2B_C1[8] = {0x85c315d2u, 0xe4a2bd06u, 0xe52d1852u, 0xa74fa084u,
                                    0xeed8fdf4u, 0xcd2cafadu, 0x3af0fed4u, 0x009713b0u};
__constant__ uint64_t VR_MOD64[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull,
                                     0x30644e72e131a029ull};

__device__ __forceinline__ bool v_lt_q(const uint32_t* w) {
  bool lt = false, decided = false;  // no early exit: the caller's array stays in registers
#pragma unroll
  for (int i = 7; i >= 0; i--) {
    if (!decided && w[i] != VQ_MOD32[i]) {
      lt = w[i] < VQ_MOD32[i];
      decided = true;
    }
  }
  return lt;
}
__device__ __forceinline__ bool v_all_zero(const uint32_t* w, int n) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < n; i++) o |= w[i];
  return o == 0;
}
__device__ __forceinline__ Fe v_fe(const uint32_t* w) { return to_mont<FqP>(unpack(w)); }
__device__ __forceinline__ bool v_g1_on_curve(const Fe& x, const Fe& y) {
  return eq<FqP>(sqr<FqP>(y), add<FqP>(mul<FqP>(sqr<FqP>(x), x), fq_small(3)));
}
// k * P for a 128-bit k (4 x u32) by double-and-add; canonical affine out,
// all-zero for infinity.  One inversion by Fermat: 1/zz = zzz i, 1/zzz = zz i
// with i = (zz zzz)^(q-2).  (Inlined, k by value: behind a call the point and
// the scalar would live in scratch.)
__device__ __forceinline__ void v_g1_mul128(const Aff<FqOps>& p, uint4 k, uint32_t* out) {
  Xyzz<FqOps> acc = xyzz_inf<FqOps>();
  for (int word = 3; word >= 0; word--) {
    const uint32_t kw = word == 3 ? k.w : word == 2 ? k.z : word == 1 ? k.y : k.x;
    for (int bit = 31; bit >= 0; bit--) {
      acc = xyzz_dbl(acc);
      if ((kw >> bit) & 1) acc = xyzz_madd(acc, p);
    }
  }
  if (xyzz_is_inf(acc)) {
    for (int i = 0; i < 16; i++) out[i] = 0;
    return;
  }
  const uint64_t qm2[4] = {0x3c208c16d87cfd45ull, 0x97816a916871ca8dull, 0xb85045b68181585dull,
                           0x30644e72e131a029ull};
  const Fe inv = pow<FqP>(mul<FqP>(acc.zz, acc.zzz), qm2);
  st_fe(out, from_mont<FqP>(mul<FqP>(acc.x, mul<FqP>(inv, acc.zzz))));
  st_fe(out + 8, from_mont<FqP>(mul<FqP>(acc.y, mul<FqP>(inv, acc.zz))));
}

// Point validation of one proof (wa, wb, wc: its canonical A, B, C), shared by
// k_verify_prepare and k_verify_each_prepare.  False when zkmi_groth16_verify
// would call the proof invalid for its points alone: a coordinate >= q, A or C
// off the curve, B off the twist or outside the order-r subgroup ([r] B, the
// loop of k_decode_g2).  The all-zero encoding is the point at infinity
// (valid).  A and C come back in Montgomery form.
struct VPoints {
  bool a_inf, b_inf, c_inf;
  Aff<FqOps> A, C;
};
__device__ __forceinline__ bool v_validate(const uint32_t* wa, const uint32_t* wb, const uint32_t* wc, VPoints& p) {
  bool lt = true;
#pragma unroll
  for (int t = 0; t < 2; t++) lt &= v_lt_q(wa + 8 * t) && v_lt_q(wc + 8 * t);
#pragma unroll
  for (int t = 0; t < 4; t++) lt &= v_lt_q(wb + 8 * t);
  if (!lt) return false;
  p.a_inf = v_all_zero(wa, 16);
  p.b_inf = v_all_zero(wb, 32);
  p.c_inf = v_all_zero(wc, 16);
  p.A = {v_fe(wa), v_fe(wa + 8)};
  p.C = {v_fe(wc), v_fe(wc + 8)};
  if (!p.a_inf && !v_g1_on_curve(p.A.x, p.A.y)) return false;
  if (!p.c_inf && !v_g1_on_curve(p.C.x, p.C.y)) return false;
  if (!p.b_inf) {
    const Aff<Fq2Ops> B = {{v_fe(wb), v_fe(wb + 8)}, {v_fe(wb + 16), v_fe(wb + 24)}};
    const Fe2 tb = {to_mont<FqP>(ldc_fe(VG2B_C0)), to_mont<FqP>(ldc_fe(VG2B_C1))};
    const Fe2 lhs = f2_sqr(B.y), rhs = f2_add(f2_mul(f2_sqr(B.x), B.x), tb);
    if (!eq<FqP>(lhs.c0, rhs.c0) || !eq<FqP>(lhs.c1, rhs.c1)) return false;
    Xyzz<Fq2Ops> acc = xyzz_inf<Fq2Ops>();
    for (int bit = 253; bit >= 0; bit--) {
      acc = xyzz_dbl(acc);
      if ((VR_MOD64[bit >> 6] >> (bit & 63)) & 1) acc = xyzz_madd(acc, B);
    }
    if (!xyzz_is_inf(acc)) return false;
  }
  return true;
}

// One lane per proof.  bad[i] = 1 when the proof fails point validation
// (v_validate).  Otherwise pairs[i] = (rho_i A_i, B_i) and rc[i] = rho_i C_i.
__global__ void __launch_bounds__(VB) k_verify_prepare(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                       const uint32_t* __restrict__ c,
                                                       const uint32_t* __restrict__ rho, size_t nb,
                                                       uint32_t* __restrict__ pairs, uint32_t* __restrict__ rc,
                                                       uint32_t* __restrict__ bad) {
  const size_t i = blockIdx.x * (size_t)VB + threadIdx.x;
  if (i >= nb) return;
  uint32_t wa[16], wb[32], wc[16];
#pragma unroll
  for (int t = 0; t < 16; t++) wa[t] = a[i * 16 + t];
#pragma unroll
  for (int t = 0; t < 32; t++) wb[t] = b[i * 32 + t];
#pragma unroll
  for (int t = 0; t < 16; t++) wc[t] = c[i * 16 + t];
  const uint4 k = reinterpret_cast<const uint4*>(rho)[i];
  bad[i] = 1;
  VPoints vp;
  if (!v_validate(wa, wb, wc, vp)) return;
  const bool a_inf = vp.a_inf, c_inf = vp.c_inf;
  const Aff<FqOps> A = vp.A, C = vp.C;
  bad[i] = 0;
  uint32_t* o = pairs + i * PAIR_WORDS;
#pragma unroll
  for (int t = 0; t < 32; t++) o[16 + t] = wb[t];
#pragma unroll 1
  for (int s = 0; s < 2; s++) {  // rho A, then rho C: one copy of the code
    uint32_t* dst = s ? rc + i * 16 : o;
    if (s ? c_inf : a_inf) {
      for (int t = 0; t < 16; t++) dst[t] = 0;
      continue;
    }
    Aff<FqOps> P;
#pragma unroll
    for (int l = 0; l < NL; l++) {
      P.x.v[l] = s ? C.x.v[l] : A.x.v[l];
      P.y.v[l] = s ? C.y.v[l] : A.y.v[l];
    }
    v_g1_mul128(P, k, dst);
  }
}

// The lane's Fq12 element in LDS: limb l of coefficient i at word
// (i * 9 + l) * VB + lane, so the 64 lanes of a wave read 64 consecutive words
// (distinct banks) and any coefficient index is a plain address.
struct F12Lds {
  uint32_t* base;
  __host__ __device__ __forceinline__ Fe get(int i) const {
    Fe r;
#pragma unroll
    for (int l = 0; l < NL; l++) r.v[l] = base[(i * NL + l) * VB];
    return r;
  }
  __host__ __device__ __forceinline__ void set(int i, const Fe& v) {
#pragma unroll
    for (int l = 0; l < NL; l++) base[(i * NL + l) * VB] = v.v[l];
  }
};

// One lane per pair: out[i] = the Miller value of pairs[i] as 12 canonical Fq,
// or 1 when either point is at infinity or the pair's proof is flagged
// (i < nbad and bad[i]).  The loop's bit pattern is r for every lane, so the
// wave diverges only on those flags.  LDS: two elements per lane (the loop
// ping-pongs between them), 2 x 64 x 12 x 36 B = 54 KB a block; no barriers
// (every column is private to its lane).
__global__ void __launch_bounds__(VB) k_miller(const uint32_t* __restrict__ pairs, const uint32_t* __restrict__ bad,
                                               size_t nbad, size_t n, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[2][12 * NL * VB];
  const size_t i = blockIdx.x * (size_t)VB + threadIdx.x;
  if (i >= n) return;
  uint32_t w[PAIR_WORDS];
#pragma unroll
  for (int t = 0; t < PAIR_WORDS; t++) w[t] = pairs[i * PAIR_WORDS + t];
  uint32_t* o = out + i * F12_WORDS;
  if (v_all_zero(w, 16) || v_all_zero(w + 16, 32) || (i < nbad && bad[i])) {
    for (int t = 0; t < F12_WORDS; t++) o[t] = t == 0;
    return;
  }
  F12Lds f[2] = {{&lds[0][threadIdx.x]}, {&lds[1][threadIdx.x]}};
  const Fe2 qx = {v_fe(w + 16), v_fe(w + 24)}, qy = {v_fe(w + 32), v_fe(w + 40)};
  const int cur = miller_loop(f[0], f[1], v_fe(w), v_fe(w + 8), qx, qy);
  const F12Lds r = {&lds[cur][threadIdx.x]};
  for (int t = 0; t < 12; t++) st_fe(o + 8 * t, from_mont<FqP>(r.get(t)));
}

// ------------------------------------------------------------ verify_each
// Exact per-proof verdicts (zkmi_groth16_verify_each): for n
// proofs the pair list is
//   [0, n)      (A_i, B_i)          k_verify_each_prepare
//   [n, 2n)     (-X_i, gamma)       k_verify_inputs
//   [2n, 3n)    (-C_i, delta)       k_verify_each_prepare
//   3n          (-alpha, beta)      the host, once a call
// so k_miller's flag test (i < nbad) covers the first n lanes; the G1 side of
// a flagged proof's other two pairs is written as infinity (Miller value 1).
constexpr int XYZZ_WORDS = 4 * NL;                   // one G1 term of X_i, Montgomery limbs
constexpr size_t EACH_TERM_BYTES = (size_t)96 << 20;  // term workspace of a chunk of proofs

// One lane per proof: lane t works on proof sel[t] of the uploaded arrays
// (sel = NULL: proof t).  With sel the proofs were validated by an earlier
// k_verify_prepare and are taken as they are; without, bad[t] is set as
// k_verify_prepare sets it.  No weights.
__global__ void __launch_bounds__(VB) k_verify_each_prepare(const uint32_t* __restrict__ a,
                                                            const uint32_t* __restrict__ b,
                                                            const uint32_t* __restrict__ c,
                                                            const uint32_t* __restrict__ sel, size_t n,
                                                            const uint32_t* __restrict__ delta,
                                                            uint32_t* __restrict__ pairs, uint32_t* __restrict__ bad) {
  const size_t t = blockIdx.x * (size_t)VB + threadIdx.x;
  if (t >= n) return;
  const size_t i = sel ? sel[t] : t;
  uint32_t wa[16], wb[32], wc[16];
#pragma unroll
  for (int k = 0; k < 16; k++) wa[k] = a[i * 16 + k];
#pragma unroll
  for (int k = 0; k < 32; k++) wb[k] = b[i * 32 + k];
#pragma unroll
  for (int k = 0; k < 16; k++) wc[k] = c[i * 16 + k];
  uint32_t* oc = pairs + (2 * n + t) * PAIR_WORDS;
#pragma unroll
  for (int k = 0; k < 32; k++) oc[16 + k] = delta[k];
  bool ok = true;
  if (!sel) {
    VPoints vp;
    ok = v_validate(wa, wb, wc, vp);
  }
  bad[t] = ok ? 0 : 1;
  if (!ok || v_all_zero(wc, 16)) {
    for (int k = 0; k < 16; k++) oc[k] = 0;
  } else {
#pragma unroll
    for (int k = 0; k < 8; k++) oc[k] = wc[k];
    st_fe(oc + 8, from_mont<FqP>(neg<FqP>(v_fe(wc + 8))));  // -C
  }
  if (!ok) return;
  uint32_t* o = pairs + t * PAIR_WORDS;
#pragma unroll
  for (int k = 0; k < 16; k++) o[k] = wa[k];
#pragma unroll
  for (int k = 0; k < 32; k++) o[16 + k] = wb[k];
}

// One lane per (proof, input) of a chunk of np proofs starting at proof p0:
// terms[g] = x_ij IC[j+1] by 254-bit double-and-add (x < r), XYZZ in Montgomery
// limbs; infinity (all zero) for x = 0 or an IC point at infinity.  ic: the
// key's n_in + 1 points, canonical affine; inputs: 8 u32 per value.
__global__ void __launch_bounds__(VB) k_verify_input_terms(const uint32_t* __restrict__ ic,
                                                           const uint32_t* __restrict__ inputs,
                                                           const uint32_t* __restrict__ bad, size_t p0, size_t np,
                                                           size_t n_in, uint32_t* __restrict__ terms) {
  const size_t g = blockIdx.x * (size_t)VB + threadIdx.x;
  if (g >= np * n_in) return;
  const size_t i = p0 + g / n_in, j = g % n_in;
  if (bad[i]) return;  // k_verify_inputs does not read a flagged proof's terms
  uint32_t w[16];
#pragma unroll
  for (int k = 0; k < 16; k++) w[k] = ic[(j + 1) * 16 + k];
  Xyzz<FqOps> acc = xyzz_inf<FqOps>();
  if (!v_all_zero(w, 16)) {
    const Aff<FqOps> P = {v_fe(w), v_fe(w + 8)};
    const uint32_t* x = inputs + (i * n_in + j) * 8;
    for (int word = 7; word >= 0; word--) {
      const uint32_t kw = x[word];
      for (int bit = 31; bit >= 0; bit--) {
        acc = xyzz_dbl(acc);
        if ((kw >> bit) & 1) acc = xyzz_madd(acc, P);
      }
    }
  }
  uint32_t* o = terms + g * XYZZ_WORDS;
#pragma unroll
  for (int l = 0; l < NL; l++) {
    o[l] = acc.x.v[l];
    o[NL + l] = acc.y.v[l];
    o[2 * NL + l] = acc.zz.v[l];
    o[3 * NL + l] = acc.zzz.v[l];
  }
}

// One lane per proof of the chunk: pairs[n + i] = (-X_i, gamma) with
// X_i = IC[0] + sum_j terms[i][j], canonical affine by one Fermat inversion
// (as v_g1_mul128); the G1 side is infinity for a flagged proof or X_i = O.
__global__ void __launch_bounds__(VB) k_verify_inputs(const uint32_t* __restrict__ ic,
                                                      const uint32_t* __restrict__ terms,
                                                      const uint32_t* __restrict__ bad, size_t p0, size_t np, size_t n,
                                                      size_t n_in, const uint32_t* __restrict__ gamma,
                                                      uint32_t* __restrict__ pairs) {
  const size_t t = blockIdx.x * (size_t)VB + threadIdx.x;
  if (t >= np) return;
  const size_t i = p0 + t;
  uint32_t* o = pairs + (n + i) * PAIR_WORDS;
#pragma unroll
  for (int k = 0; k < 32; k++) o[16 + k] = gamma[k];
  Xyzz<FqOps> acc = xyzz_inf<FqOps>();
  if (!bad[i]) {
    uint32_t w[16];
#pragma unroll
    for (int k = 0; k < 16; k++) w[k] = ic[k];
    if (!v_all_zero(w, 16)) acc = xyzz_from_aff<FqOps>({v_fe(w), v_fe(w + 8)});
#pragma unroll 1
    for (size_t j = 0; j < n_in; j++) {
      const uint32_t* s = terms + (t * n_in + j) * XYZZ_WORDS;
      Xyzz<FqOps> q;
#pragma unroll
      for (int l = 0; l < NL; l++) {
        q.x.v[l] = s[l];
        q.y.v[l] = s[NL + l];
        q.zz.v[l] = s[2 * NL + l];
        q.zzz.v[l] = s[3 * NL + l];
      }
      acc = xyzz_add(acc, q);
    }
  }
  if (xyzz_is_inf(acc)) {
    for (int k = 0; k < 16; k++) o[k] = 0;
    return;
  }
  const uint64_t qm2[4] = {0x3c208c16d87cfd45ull, 0x97816a916871ca8dull, 0xb85045b68181585dull,
                           0x30644e72e131a029ull};
  const Fe inv = pow<FqP>(mul<FqP>(acc.zz, acc.zzz), qm2);
  st_fe(o, from_mont<FqP>(mul<FqP>(acc.x, mul<FqP>(inv, acc.zzz))));
  st_fe(o + 8, from_mont<FqP>(neg<FqP>(mul<FqP>(acc.y, mul<FqP>(inv, acc.zz)))));
}

// One lane per proof: valid[i] = whether the product of the proof's three
// Miller values f[i], f[n + i], f[2n + i] and the shared f[3n] passes the
// final exponentiation (pairing.h final_exp_is_one); 0 with no work for a
// flagged proof.  LDS: three elements per lane (the chain's base and the two
// it ping-pongs between), 3 x 12 x 9 x 64 x 4 B = 82,944 B a block, so one
// block a CU; no barriers (every column is private to its lane).  The
// exponent's bits are the same for every lane: the wave diverges only on the
// flags.
__global__ void __launch_bounds__(VB) k_final_exp(const uint32_t* __restrict__ f, const uint32_t* __restrict__ bad,
                                                  size_t n, const FinalExpConst* __restrict__ fc,
                                                  uint8_t* __restrict__ valid) {
  __shared__ uint32_t lds[3][12 * NL * VB];
  const size_t i = blockIdx.x * (size_t)VB + threadIdx.x;
  if (i >= n) return;
  if (bad[i]) {
    valid[i] = 0;
    return;
  }
  F12Lds e0 = {&lds[0][threadIdx.x]}, e1 = {&lds[1][threadIdx.x]}, e2 = {&lds[2][threadIdx.x]};
  const F12Const K = f12_const();
  const uint32_t* src = f + i * F12_WORDS;
#pragma unroll 1
  for (int t = 0; t < 12; t++) {
    e0.set(t, to_mont<FqP>(ld_fe(src + 8 * t)));
    e1.set(t, to_mont<FqP>(ld_fe(src + n * F12_WORDS + 8 * t)));
  }
  f12_mul(e2, e0, e1, K);
#pragma unroll 1
  for (int t = 0; t < 12; t++) e0.set(t, to_mont<FqP>(ld_fe(src + 2 * n * F12_WORDS + 8 * t)));
  f12_mul(e1, e2, e0, K);
#pragma unroll 1
  for (int t = 0; t < 12; t++) e0.set(t, to_mont<FqP>(ld_fe(f + 3 * n * F12_WORDS + 8 * t)));
  f12_mul(e2, e1, e0, K);
  valid[i] = final_exp_is_one(e2, e0, e1, fc->zeta, fc->hard) ? 1 : 0;
}

// ------------------------------------------------------------ encoded proofs
// Proofs from their wire bytes (zkmi_groth16_verify_many_encoded / _each_encoded
// / zkmi_proofs_decode): the encodings are uploaded as they are
// and decoded by proof_decode.h into the d_a / d_b / d_c words that
// k_verify_prepare / k_verify_each_prepare read.  A malformed proof gets
// malformed[i] = 1 and ALL its words 0xFFFFFFFF, so v_validate rejects it
// through v_lt_q and nothing downstream knows about encodings.

// Compressed proofs (128 B: A 32 | B 64 | C 32), one lane per POINT, the two
// Fq2 powers of the G2 square roots kept together in waves: lanes [0, nb) take
// B, [nb, 2 nb) A, [2 nb, 3 nb) C, so a wave mixes G1 and G2 work only where
// nb is no multiple of 64.  slot_bad[t] = 1 when lane t's point is malformed.
__global__ void __launch_bounds__(VB) k_proof_decode(const uint32_t* __restrict__ raw, size_t nb,
                                                     uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                                                     uint32_t* __restrict__ c, uint32_t* __restrict__ slot_bad) {
  const size_t t = blockIdx.x * (size_t)VB + threadIdx.x;
  if (t >= 3 * nb) return;
  bool ok;
  if (t < nb) {
    ok = pd_g2_compressed(raw + t * 32 + 8, b + t * 32);
  } else {
    const bool is_c = t >= 2 * nb;
    const size_t i = t - (is_c ? 2 * nb : nb);
    ok = pd_g1_compressed(raw + i * 32 + (is_c ? 24 : 0), (is_c ? c : a) + i * 16);
  }
  slot_bad[t] = ok ? 0 : 1;
}
__device__ __forceinline__ void v_fill_malformed(size_t i, uint32_t* a, uint32_t* b, uint32_t* c) {
  for (int k = 0; k < 16; k++) a[i * 16 + k] = c[i * 16 + k] = 0xFFFFFFFFu;
  for (int k = 0; k < 32; k++) b[i * 32 + k] = 0xFFFFFFFFu;
}
// One lane per proof, after k_proof_decode: the three point flags of a proof
// become its malformed byte and, when set, its words.
__global__ void __launch_bounds__(VB) k_proof_decode_flag(const uint32_t* __restrict__ slot_bad, size_t nb,
                                                          uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                                                          uint32_t* __restrict__ c, uint8_t* __restrict__ malformed) {
  const size_t i = blockIdx.x * (size_t)VB + threadIdx.x;
  if (i >= nb) return;
  const bool bad = (slot_bad[i] | slot_bad[nb + i] | slot_bad[2 * nb + i]) != 0;
  malformed[i] = bad ? 1 : 0;
  if (bad) v_fill_malformed(i, a, b, c);
}
// The three 256-byte formats do no power: one lane per proof.
template <int FMT>
__global__ void __launch_bounds__(VB) k_proof_decode_fixed(const uint32_t* __restrict__ raw, size_t nb,
                                                           uint32_t* __restrict__ a, uint32_t* __restrict__ b,
                                                           uint32_t* __restrict__ c, uint8_t* __restrict__ malformed) {
  const size_t i = blockIdx.x * (size_t)VB + threadIdx.x;
  if (i >= nb) return;
  const bool ok = pd_fixed<FMT>(raw + i * 64, a + i * 16, b + i * 32, c + i * 16);
  malformed[i] = ok ? 0 : 1;
  if (!ok) v_fill_malformed(i, a, b, c);
}
// One lane per proof: bad[i] = 1 when the decoded proof fails point validation
// (v_validate), for zkmi_proofs_decode's status.
__global__ void __launch_bounds__(VB) k_proof_validate(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                       const uint32_t* __restrict__ c, size_t nb,
                                                       uint32_t* __restrict__ bad) {
  const size_t i = blockIdx.x * (size_t)VB + threadIdx.x;
  if (i >= nb) return;
  uint32_t wa[16], wb[32], wc[16];
#pragma unroll
  for (int t = 0; t < 16; t++) wa[t] = a[i * 16 + t];
#pragma unroll
  for (int t = 0; t < 32; t++) wb[t] = b[i * 32 + t];
#pragma unroll
  for (int t = 0; t < 16; t++) wc[t] = c[i * 16 + t];
  VPoints vp;
  bad[i] = v_validate(wa, wb, wc, vp) ? 0 : 1;
}

static unsigned vblocks(size_t n) { return (unsigned)((n + VB - 1) / VB); }

// Where a call's proofs come from: canonical points on the host (enc = NULL),
// or nb encodings of format fmt, decoded on the device.  malformed: nb bytes
// on the host or NULL; written by the time the context stream is next
// synchronised.
struct ProofSrc {
  const uint64_t *a, *b, *c;
  int fmt;
  const uint8_t* enc;
  uint8_t* malformed;
};
// d_a / d_b / d_c <- the proofs of src, on the context stream
static int proofs_to_device(zkmi_ctx* ctx, const ProofSrc& src, size_t nb, uint32_t* d_a, uint32_t* d_b,
                            uint32_t* d_c) {
  if (!src.enc) {
    ZK_HIP(hipMemcpyAsync(d_a, src.a, nb * 64, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipMemcpyAsync(d_b, src.b, nb * 128, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(hipMemcpyAsync(d_c, src.c, nb * 64, hipMemcpyHostToDevice, ctx->stream));
    return 0;
  }
  const size_t len = proof_encoded_len(src.fmt);
  uint32_t *d_raw, *d_slot;
  uint8_t* d_mal;
  ZK_TRY(ctx->ws.get("vd_raw", nb * len, (void**)&d_raw));
  ZK_TRY(ctx->ws.get("vd_slot", 3 * nb * 4, (void**)&d_slot));
  ZK_TRY(ctx->ws.get("vd_mal", nb, (void**)&d_mal));
  ZK_HIP(hipMemcpyAsync(d_raw, src.enc, nb * len, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "verify_decode");
    const unsigned grid = vblocks(nb);  // one lane per proof
    switch (src.fmt) {
      case PROOF_ARK_COMPRESSED:
        k_proof_decode<<<vblocks(3 * nb), VB, 0, ctx->stream>>>(d_raw, nb, d_a, d_b, d_c, d_slot);
        k_proof_decode_flag<<<grid, VB, 0, ctx->stream>>>(d_slot, nb, d_a, d_b, d_c, d_mal);
        break;
      case PROOF_ARK_UNCOMPRESSED:
        k_proof_decode_fixed<PROOF_ARK_UNCOMPRESSED><<<grid, VB, 0, ctx->stream>>>(d_raw, nb, d_a, d_b, d_c, d_mal);
        break;
      case PROOF_SOLANA_LE:
        k_proof_decode_fixed<PROOF_SOLANA_LE><<<grid, VB, 0, ctx->stream>>>(d_raw, nb, d_a, d_b, d_c, d_mal);
        break;
      default:
        k_proof_decode_fixed<PROOF_ALT_BN128_BE><<<grid, VB, 0, ctx->stream>>>(d_raw, nb, d_a, d_b, d_c, d_mal);
    }
  }
  ZK_HIP(hipGetLastError());
  if (src.malformed) ZK_HIP(hipMemcpyAsync(src.malformed, d_mal, nb, hipMemcpyDeviceToHost, ctx->stream));
  return 0;
}

// verify.cpp's Frobenius^2 constants and exponent, in the device's form
static const FinalExpConst& final_exp_const() {
  static const FinalExpConst fc = [] {
    FinalExpConst c;
    uint64_t zeta[48];
    zkv::final_exp_constants(zeta, c.hard);
    for (int i = 0; i < 12; i++) {
      uint32_t w[8];
      memcpy(w, zeta + 4 * i, 32);
      c.zeta[i] = to_mont<FqP>(unpack(w));
    }
    return c;
  }();
  return fc;
}

// The kernels of verify_each over n lanes: lane t is proof d_sel[t] of the
// uploaded d_a / d_b / d_c (d_sel = NULL: proof t, validated here); inputs are
// in lane order (n x n_inputs x 4 u64, each < r).  valid[n]; *invalid = lanes
// that failed point validation; *pairs / *fexps = Miller loops and final
// exponentiations run (0 when no lane passed validation).  Everything on the
// context stream; returns after the verdicts are on the host.
static int verify_each_run(zkmi_ctx* ctx, const zkmi_vk* vk, size_t n, const uint32_t* d_a, const uint32_t* d_b,
                           const uint32_t* d_c, const uint32_t* d_sel, const uint64_t* inputs, uint8_t* valid,
                           uint64_t* pairs, uint64_t* fexps, uint64_t* invalid) {
  const size_t n_in = vk->vk.ic.size() - 1, np = 3 * n + 1;
  const size_t chunk = std::min(n, std::max<size_t>(1, EACH_TERM_BYTES / (std::max<size_t>(1, n_in) * XYZZ_WORDS * 4)));
  uint32_t *d_pairs, *d_bad, *d_f, *d_key, *d_x, *d_terms;
  FinalExpConst* d_fc;
  uint8_t* d_valid;
  ZK_TRY(ctx->ws.get("ve_pairs", np * PAIR_WORDS * 4, (void**)&d_pairs));
  ZK_TRY(ctx->ws.get("ve_bad", n * 4, (void**)&d_bad));
  ZK_TRY(ctx->ws.get("ve_f", np * F12_WORDS * 4, (void**)&d_f));
  ZK_TRY(ctx->ws.get("ve_key", (64 + (n_in + 1) * 16) * 4, (void**)&d_key));
  ZK_TRY(ctx->ws.get("ve_x", std::max<size_t>(1, n * n_in) * 32, (void**)&d_x));
  ZK_TRY(ctx->ws.get("ve_terms", std::max<size_t>(1, chunk * n_in) * XYZZ_WORDS * 4, (void**)&d_terms));
  ZK_TRY(ctx->ws.get("ve_fc", sizeof(FinalExpConst), (void**)&d_fc));
  ZK_TRY(ctx->ws.get("ve_valid", n, (void**)&d_valid));
  // the key: delta | gamma | IC, and the call's one shared pair (-alpha, beta)
  std::vector<uint64_t> key(32 + (n_in + 1) * 8);
  memcpy(key.data(), vk->g2[2], 128);
  memcpy(key.data() + 16, vk->g2[1], 128);
  for (size_t j = 0; j <= n_in; j++) zkv::g1_to_canon(key.data() + 32 + 8 * j, vk->vk.ic[j]);
  uint64_t shared[24];
  zkv::g1_to_canon(shared, zkv::g1_neg(vk->vk.alpha));
  memcpy(shared + 8, vk->g2[0], 128);
  const uint32_t *d_delta = d_key, *d_gamma = d_key + 32, *d_ic = d_key + 64;
  ZK_HIP(hipMemcpyAsync(d_key, key.data(), key.size() * 8, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_pairs + 3 * n * PAIR_WORDS, shared, sizeof(shared), hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_fc, &final_exp_const(), sizeof(FinalExpConst), hipMemcpyHostToDevice, ctx->stream));
  if (n_in) ZK_HIP(hipMemcpyAsync(d_x, inputs, n * n_in * 32, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "verify_each_prepare");
    k_verify_each_prepare<<<vblocks(n), VB, 0, ctx->stream>>>(d_a, d_b, d_c, d_sel, n, d_delta, d_pairs, d_bad);
  }
  ZK_HIP(hipGetLastError());
  *pairs = *fexps = *invalid = 0;
  if (!d_sel) {  // how many lanes are left decides whether anything more runs
    std::vector<uint32_t> bad32(n);
    ZK_HIP(hipMemcpyAsync(bad32.data(), d_bad, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; i++) *invalid += bad32[i] != 0;
    if (*invalid == n) {
      memset(valid, 0, n);
      return timer_flush(ctx);
    }
  }
  {
    ScopedKernelTimer tm(ctx, "verify_inputs");
    for (size_t p0 = 0; p0 < n; p0 += chunk) {
      const size_t cp = std::min(chunk, n - p0);
      if (n_in)
        k_verify_input_terms<<<vblocks(cp * n_in), VB, 0, ctx->stream>>>(d_ic, d_x, d_bad, p0, cp, n_in, d_terms);
      k_verify_inputs<<<vblocks(cp), VB, 0, ctx->stream>>>(d_ic, d_terms, d_bad, p0, cp, n, n_in, d_gamma, d_pairs);
    }
  }
  ZK_HIP(hipGetLastError());
  {
    ScopedKernelTimer tm(ctx, "verify_miller");
    k_miller<<<vblocks(np), VB, 0, ctx->stream>>>(d_pairs, d_bad, n, np, d_f);
  }
  ZK_HIP(hipGetLastError());
  {
    ScopedKernelTimer tm(ctx, "verify_final_exp");
    k_final_exp<<<vblocks(n), VB, 0, ctx->stream>>>(d_f, d_bad, n, d_fc, d_valid);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(valid, d_valid, n, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  *pairs = np;
  *fexps = n - *invalid;
  return timer_flush(ctx);
}

static int verify_each(zkmi_ctx* ctx, const zkmi_vk* vk, size_t nb, const uint64_t* inputs, const ProofSrc& src,
                       uint8_t* valid, zkmi_verify_each_stats* stats) {
  const size_t n_in = vk->vk.ic.size() - 1;
  ZK_TRY(zkv::verify_many_check_scalars(nb, n_in, inputs, nullptr));
  uint32_t* d_in;
  ZK_TRY(ctx->ws.get("vm_in", nb * 68 * 4, (void**)&d_in));
  uint32_t *d_a = d_in, *d_b = d_a + nb * 16, *d_c = d_b + nb * 32;
  ZK_TRY(proofs_to_device(ctx, src, nb, d_a, d_b, d_c));
  uint64_t pairs, fexps, invalid;
  ZK_TRY(verify_each_run(ctx, vk, nb, d_a, d_b, d_c, nullptr, inputs, valid, &pairs, &fexps, &invalid));
  if (stats) *stats = {pairs, fexps, invalid};
  return 0;
}

static int draw_weights(uint64_t* w, size_t nb) {
  for (size_t i = 0; i < nb; i++) {
    do {
      size_t got = 0;
      while (got < 16) {
        const ssize_t r = getrandom((uint8_t*)(w + 2 * i) + got, 16 - got, 0);
        if (r < 0) {
          set_error("zkmi_groth16_verify_many: getrandom failed");
          return ZKMI_EINVAL;
        }
        got += (size_t)r;
      }
    } while ((w[2 * i] | w[2 * i + 1]) == 0);
  }
  return 0;
}

static int verify_many(zkmi_ctx* ctx, const zkmi_vk* vk, size_t nb, const uint64_t* inputs, const ProofSrc& src,
                       const uint64_t* rho_in, uint8_t* valid, zkmi_verify_stats* stats) {
  const size_t n_inputs = vk->vk.ic.size() - 1;
  std::vector<uint64_t> rho(2 * nb);
  if (rho_in)
    memcpy(rho.data(), rho_in, 16 * nb);
  else
    ZK_TRY(draw_weights(rho.data(), nb));
  ZK_TRY(zkv::verify_many_check_scalars(nb, n_inputs, inputs, rho.data()));
  const size_t np = nb + 3;
  uint32_t *d_in, *d_pairs, *d_rc, *d_bad, *d_f;
  ZK_TRY(ctx->ws.get("vm_in", nb * 68 * 4, (void**)&d_in));
  ZK_TRY(ctx->ws.get("vm_pairs", np * PAIR_WORDS * 4, (void**)&d_pairs));
  ZK_TRY(ctx->ws.get("vm_rc", nb * 16 * 4, (void**)&d_rc));
  ZK_TRY(ctx->ws.get("vm_bad", nb * 4, (void**)&d_bad));
  ZK_TRY(ctx->ws.get("vm_f", np * F12_WORDS * 4, (void**)&d_f));
  uint32_t *d_a = d_in, *d_b = d_a + nb * 16, *d_c = d_b + nb * 32, *d_rho = d_c + nb * 16;
  ZK_TRY(proofs_to_device(ctx, src, nb, d_a, d_b, d_c));
  ZK_HIP(hipMemcpyAsync(d_rho, rho.data(), nb * 16, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "verify_prepare");
    k_verify_prepare<<<(unsigned)((nb + VB - 1) / VB), VB, 0, ctx->stream>>>(d_a, d_b, d_c, d_rho, nb, d_pairs, d_rc,
                                                                           d_bad);
  }
  ZK_HIP(hipGetLastError());
  std::vector<uint32_t> bad32(nb);
  std::vector<uint64_t> rc64(nb * 8);
  ZK_HIP(hipMemcpyAsync(bad32.data(), d_bad, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipMemcpyAsync(rc64.data(), d_rc, nb * 64, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));

  std::vector<uint8_t> bad(nb);
  std::vector<zkv::G1> rc(nb);
  std::vector<size_t> idx;
  for (size_t i = 0; i < nb; i++) {
    bad[i] = bad32[i] != 0;
    if (bad[i]) continue;
    rc[i] = zkv::g1_from_canon(rc64.data() + 8 * i);
    idx.push_back(i);
  }
  std::vector<zkv::F12> f(np);
  zkv::VerifyManyIn in = {&vk->vk, nb, n_inputs, inputs, rho.data(), bad.data(), f.data(), rc.data()};
  if (idx.empty()) {  // nothing to pair
    ZK_TRY(timer_flush(ctx));
    return zkv::verify_many_combine(in, nullptr, valid, stats);
  }
  // the three fixed-G2 pairs of the whole batch: lanes nb .. nb+2
  zkv::G1 g[3];
  zkv::verify_many_fixed_g1(in, idx.data(), idx.size(), g);
  uint64_t fixed[3][24];
  for (int k = 0; k < 3; k++) {
    zkv::g1_to_canon(fixed[k], g[k]);
    memcpy(fixed[k] + 8, vk->g2[k], 128);
  }
  ZK_HIP(hipMemcpyAsync(d_pairs + nb * PAIR_WORDS, fixed, sizeof(fixed), hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "verify_miller");
    k_miller<<<(unsigned)((np + VB - 1) / VB), VB, 0, ctx->stream>>>(d_pairs, d_bad, nb, np, d_f);
  }
  ZK_HIP(hipGetLastError());
  std::vector<uint64_t> f64(np * 48);
  ZK_HIP(hipMemcpyAsync(f64.data(), d_f, np * F12_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  ZK_TRY(timer_flush(ctx));
  for (size_t i = 0; i < np; i++) f[i] = zkv::f12_from_canon(f64.data() + 48 * i);
  const zkv::F12 fixed_all = zkv::f12_mul(zkv::f12_mul(f[nb], f[nb + 1]), f[nb + 2]);
  if (stats) stats->pairs = np;
  if (!ctx->verify_probes) return zkv::verify_many_combine(in, &fixed_all, valid, stats);
  // a probe budget: what bisection has not decided when it is spent goes, as
  // ONE sub-batch over the points already uploaded and validated, through the
  // kernels of verify_each
  std::vector<size_t> und;
  ZK_TRY(zkv::verify_many_combine_budget(in, &fixed_all, ctx->verify_probes, valid, stats, &und));
  if (und.empty()) return 0;
  const size_t m = und.size();
  std::vector<uint32_t> sel(m);
  std::vector<uint64_t> sub_in(m * n_inputs * 4);
  for (size_t t = 0; t < m; t++) {
    sel[t] = (uint32_t)und[t];
    if (n_inputs) memcpy(sub_in.data() + t * n_inputs * 4, inputs + und[t] * n_inputs * 4, n_inputs * 32);
  }
  uint32_t* d_sel;
  ZK_TRY(ctx->ws.get("ve_sel", m * 4, (void**)&d_sel));
  ZK_HIP(hipMemcpyAsync(d_sel, sel.data(), m * 4, hipMemcpyHostToDevice, ctx->stream));
  std::vector<uint8_t> sub_valid(m);
  uint64_t gp, ge, gi;
  ZK_TRY(verify_each_run(ctx, vk, m, d_a, d_b, d_c, d_sel, sub_in.data(), sub_valid.data(), &gp, &ge, &gi));
  for (size_t t = 0; t < m; t++) valid[und[t]] = sub_valid[t];
  ctx->verify_last[0] = m;
  ctx->verify_last[1] = gp;
  ctx->verify_last[2] = ge;
  return 0;
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkmi_vk_load(zkmi_ctx* ctx, const uint8_t* bytes, size_t len, zkmi_vk** out) {
  if (!ctx || !bytes || !out) {
    set_error("zkmi_vk_load: null argument");
    return ZKMI_EINVAL;
  }
  zkmi_vk* vk = new zkmi_vk;
  vk->ctx = ctx;
  const char* why = "";
  if (!zkv::vk_decode(bytes, len, &vk->vk, &why)) {
    delete vk;
    set_error("zkmi_vk_load: %s", why);
    return ZKMI_EPOINT;
  }
  zkv::g2_to_canon(vk->g2[0], vk->vk.beta);
  zkv::g2_to_canon(vk->g2[1], vk->vk.gamma);
  zkv::g2_to_canon(vk->g2[2], vk->vk.delta);
  *out = vk;
  return 0;
}
void zkmi_vk_destroy(zkmi_vk* vk) { delete vk; }
int zkmi_vk_info(const zkmi_vk* vk, uint64_t out[1]) {
  if (!vk || !out) {
    set_error("zkmi_vk_info: null argument");
    return ZKMI_EINVAL;
  }
  out[0] = vk->vk.ic.size() - 1;
  return 0;
}

int zkmi_groth16_verify_many(zkmi_ctx* ctx, const zkmi_vk* vk, size_t nb, const uint64_t* inputs, const uint64_t* a,
                             const uint64_t* b, const uint64_t* c, const uint64_t* rho, uint8_t* valid,
                             zkmi_verify_stats* stats) {
  if (!ctx || !vk || vk->ctx != ctx) {
    set_error("zkmi_groth16_verify_many: null context or key, or a key of another context");
    return ZKMI_EINVAL;
  }
  if (stats) memset(stats, 0, sizeof(*stats));
  ctx->verify_last[0] = ctx->verify_last[1] = ctx->verify_last[2] = 0;
  if (nb == 0) return 0;
  if (!a || !b || !c || !valid || (vk->vk.ic.size() > 1 && !inputs)) {
    set_error("zkmi_groth16_verify_many: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return verify_many(ctx, vk, nb, inputs, ProofSrc{a, b, c, 0, nullptr, nullptr}, rho, valid, stats);
}

int zkmi_groth16_verify_each(zkmi_ctx* ctx, const zkmi_vk* vk, size_t nb, const uint64_t* inputs, const uint64_t* a,
                             const uint64_t* b, const uint64_t* c, uint8_t* valid, zkmi_verify_each_stats* stats) {
  if (!ctx || !vk || vk->ctx != ctx) {
    set_error("zkmi_groth16_verify_each: null context or key, or a key of another context");
    return ZKMI_EINVAL;
  }
  if (stats) memset(stats, 0, sizeof(*stats));
  if (nb == 0) return 0;
  if (!a || !b || !c || !valid || (vk->vk.ic.size() > 1 && !inputs)) {
    set_error("zkmi_groth16_verify_each: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return verify_each(ctx, vk, nb, inputs, ProofSrc{a, b, c, 0, nullptr, nullptr}, valid, stats);
}

int zkmi_groth16_verify_many_encoded(zkmi_ctx* ctx, const zkmi_vk* vk, int fmt, size_t nb, const uint8_t* proofs,
                                     const uint64_t* inputs, const uint64_t* rho, uint8_t* valid, uint8_t* malformed,
                                     zkmi_verify_stats* stats) {
  if (!ctx || !vk || vk->ctx != ctx) {
    set_error("zkmi_groth16_verify_many_encoded: null context or key, or a key of another context");
    return ZKMI_EINVAL;
  }
  if (!proof_encoded_len(fmt)) {
    set_error("zkmi_groth16_verify_many_encoded: unknown proof format %d", fmt);
    return ZKMI_EINVAL;
  }
  if (stats) memset(stats, 0, sizeof(*stats));
  ctx->verify_last[0] = ctx->verify_last[1] = ctx->verify_last[2] = 0;
  if (nb == 0) return 0;
  if (!proofs || !valid || (vk->vk.ic.size() > 1 && !inputs)) {
    set_error("zkmi_groth16_verify_many_encoded: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return verify_many(ctx, vk, nb, inputs, ProofSrc{nullptr, nullptr, nullptr, fmt, proofs, malformed}, rho, valid,
                     stats);
}

int zkmi_groth16_verify_each_encoded(zkmi_ctx* ctx, const zkmi_vk* vk, int fmt, size_t nb, const uint8_t* proofs,
                                     const uint64_t* inputs, uint8_t* valid, uint8_t* malformed,
                                     zkmi_verify_each_stats* stats) {
  if (!ctx || !vk || vk->ctx != ctx) {
    set_error("zkmi_groth16_verify_each_encoded: null context or key, or a key of another context");
    return ZKMI_EINVAL;
  }
  if (!proof_encoded_len(fmt)) {
    set_error("zkmi_groth16_verify_each_encoded: unknown proof format %d", fmt);
    return ZKMI_EINVAL;
  }
  if (stats) memset(stats, 0, sizeof(*stats));
  if (nb == 0) return 0;
  if (!proofs || !valid || (vk->vk.ic.size() > 1 && !inputs)) {
    set_error("zkmi_groth16_verify_each_encoded: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return verify_each(ctx, vk, nb, inputs, ProofSrc{nullptr, nullptr, nullptr, fmt, proofs, malformed}, valid, stats);
}

int zkmi_proofs_decode(zkmi_ctx* ctx, int fmt, const uint8_t* proofs, size_t nb, uint64_t* a, uint64_t* b,
                       uint64_t* c, uint8_t* status) {
  if (!ctx) {
    set_error("zkmi_proofs_decode: null context");
    return ZKMI_EINVAL;
  }
  if (!proof_encoded_len(fmt)) {
    set_error("zkmi_proofs_decode: unknown proof format %d", fmt);
    return ZKMI_EINVAL;
  }
  if (nb == 0) return 0;
  if (!proofs || !a || !b || !c || !status) {
    set_error("zkmi_proofs_decode: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  uint32_t *d_in, *d_bad;
  ZK_TRY(ctx->ws.get("vm_in", nb * 68 * 4, (void**)&d_in));
  ZK_TRY(ctx->ws.get("vd_bad", nb * 4, (void**)&d_bad));
  uint32_t *d_a = d_in, *d_b = d_a + nb * 16, *d_c = d_b + nb * 32;
  std::vector<uint8_t> mal(nb);
  ZK_TRY(proofs_to_device(ctx, ProofSrc{nullptr, nullptr, nullptr, fmt, proofs, mal.data()}, nb, d_a, d_b, d_c));
  {
    ScopedKernelTimer tm(ctx, "verify_decode_validate");
    k_proof_validate<<<vblocks(nb), VB, 0, ctx->stream>>>(d_a, d_b, d_c, nb, d_bad);
  }
  ZK_HIP(hipGetLastError());
  std::vector<uint32_t> bad32(nb);
  ZK_HIP(hipMemcpyAsync(bad32.data(), d_bad, nb * 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipMemcpyAsync(a, d_a, nb * 64, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipMemcpyAsync(b, d_b, nb * 128, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipMemcpyAsync(c, d_c, nb * 64, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  ZK_TRY(timer_flush(ctx));
  for (size_t i = 0; i < nb; i++) {
    status[i] = mal[i] ? 1 : bad32[i] ? 2 : 0;
    if (!status[i]) continue;
    memset(a + 8 * i, 0, 64);
    memset(b + 16 * i, 0, 128);
    memset(c + 8 * i, 0, 64);
  }
  return 0;
}

int zkmi_ctx_set_verify_probes(zkmi_ctx* ctx, uint64_t max_probes) {
  if (!ctx) {
    set_error("zkmi_ctx_set_verify_probes: null context");
    return ZKMI_EINVAL;
  }
  ctx->verify_probes = max_probes;
  return 0;
}
uint64_t zkmi_ctx_get_verify_probes(const zkmi_ctx* ctx) { return ctx ? ctx->verify_probes : 0; }
int zkmi_groth16_verify_last(zkmi_ctx* ctx, uint64_t out[3]) {
  if (!ctx || !out) {
    set_error("zkmi_groth16_verify_last: null argument");
    return ZKMI_EINVAL;
  }
  memcpy(out, ctx->verify_last, sizeof(ctx->verify_last));
  return 0;
}

}  // extern "C"
