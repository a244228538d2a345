// pairing.hip — batched Groth16 verification (zkmi_groth16_verify_many,
// DESIGN.md §2.7): two kernels on the context stream,
//   k_verify_prepare  one lane per proof: point validation as
//                     zkmi_groth16_verify's, rho_i A_i and rho_i C_i
//   k_miller          one lane per pair: the Tate Miller loop of pairing.h
// and the host half in verify.cpp (verify_many_combine): one final
// exponentiation for the batch, bisection when the combined check fails.
#include <string.h>
#include <sys/random.h>

#include <vector>

#include "dev_io.h"
#include "pairing.h"
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

// One lane per proof.  bad[i] = 1 when zkmi_groth16_verify would call proof i
// invalid for its points alone: a coordinate >= q, A or C off the curve, B
// off the twist or outside the order-r subgroup ([r] B, the loop of
// k_decode_g2).  The all-zero encoding is the point at infinity (valid).
// Otherwise pairs[i] = (rho_i A_i, B_i) and rc[i] = rho_i C_i.
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
  bool lt = true;
#pragma unroll
  for (int t = 0; t < 2; t++) lt &= v_lt_q(wa + 8 * t) && v_lt_q(wc + 8 * t);
#pragma unroll
  for (int t = 0; t < 4; t++) lt &= v_lt_q(wb + 8 * t);
  if (!lt) return;
  const bool a_inf = v_all_zero(wa, 16), b_inf = v_all_zero(wb, 32), c_inf = v_all_zero(wc, 16);
  const Aff<FqOps> A = {v_fe(wa), v_fe(wa + 8)}, C = {v_fe(wc), v_fe(wc + 8)};
  if (!a_inf && !v_g1_on_curve(A.x, A.y)) return;
  if (!c_inf && !v_g1_on_curve(C.x, C.y)) return;
  if (!b_inf) {
    const Aff<Fq2Ops> B = {{v_fe(wb), v_fe(wb + 8)}, {v_fe(wb + 16), v_fe(wb + 24)}};
    const Fe2 tb = {to_mont<FqP>(ldc_fe(VG2B_C0)), to_mont<FqP>(ldc_fe(VG2B_C1))};
    const Fe2 lhs = f2_sqr(B.y), rhs = f2_add(f2_mul(f2_sqr(B.x), B.x), tb);
    if (!eq<FqP>(lhs.c0, rhs.c0) || !eq<FqP>(lhs.c1, rhs.c1)) return;
    Xyzz<Fq2Ops> acc = xyzz_inf<Fq2Ops>();
    for (int bit = 253; bit >= 0; bit--) {
      acc = xyzz_dbl(acc);
      if ((VR_MOD64[bit >> 6] >> (bit & 63)) & 1) acc = xyzz_madd(acc, B);
    }
    if (!xyzz_is_inf(acc)) return;
  }
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

static int verify_many(zkmi_ctx* ctx, const zkmi_vk* vk, size_t nb, const uint64_t* inputs, const uint64_t* a,
                       const uint64_t* b, const uint64_t* c, const uint64_t* rho_in, uint8_t* valid,
                       zkmi_verify_stats* stats) {
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
  ZK_HIP(hipMemcpyAsync(d_a, a, nb * 64, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_b, b, nb * 128, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_c, c, nb * 64, hipMemcpyHostToDevice, ctx->stream));
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
  return zkv::verify_many_combine(in, &fixed_all, valid, stats);
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
  if (nb == 0) return 0;
  if (!a || !b || !c || !valid || (vk->vk.ic.size() > 1 && !inputs)) {
    set_error("zkmi_groth16_verify_many: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return verify_many(ctx, vk, nb, inputs, a, b, c, rho, valid, stats);
}

}  // extern "C"
