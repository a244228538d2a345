// verify_internal.h — what verify.cpp shares with the batched verifier
// (pairing.hip) and with the stand-alone host checks under tests/host/: the
// host Fq12 (F12), the two halves of the pairing check (Miller value, final
// exponentiation), the decoded verifying key and the G1 helpers, plus the
// combine-and-bisect routine of zkmi_groth16_verify_many and the constants of
// the device final exponentiation.  Host code only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/zkmi.h"
#include "host_field.h"

namespace zkv {

using zkh::F4;
using F2 = zkh::F42;

extern const uint64_t RP[4];  // scalar field r

struct G1 {
  F4 x, y;
  bool inf;
};
struct G2 {
  F2 x, y;
  bool inf;
};
// Fq12 = Fq[w] / (w^12 - 18 w^6 + 82), coefficients of w^0 .. w^11
struct F12 {
  F4 c[12];
};
// arkworks-compressed VerifyingKey<Bn254>, decoded and validated
struct Vk {
  G1 alpha;
  G2 beta, gamma, delta;
  std::vector<G1> ic;
};

bool lt_q(const uint64_t c[4]);
F4 fneg(const F4& a);
bool g1_on_curve(const G1& p);
bool g2_on_curve(const G2& p);
bool g2_in_subgroup(const G2& p);
G1 g1_from_canon(const uint64_t p[8]);
G2 g2_from_canon(const uint64_t p[16]);
void g1_to_canon(uint64_t o[8], const G1& p);
void g2_to_canon(uint64_t o[16], const G2& p);
G1 g1_add(const G1& a, const G1& b);
G1 g1_mul(const G1& p, const uint64_t k[4]);
G1 g1_neg(G1 p);
// sum of pts[i] over idx (one inversion for the whole sum)
G1 g1_sum(const G1* pts, const size_t* idx, size_t n);
bool vk_decode(const uint8_t* b, size_t len, Vk* vk, const char** why);
// One encoded proof (fmt: ZKMI_PROOF_*, in: zkmi_proof_encoded_len(fmt) bytes)
// -> canonical words by the rule of DESIGN.md section 2.9: 0, or 1 when the
// encoding is malformed.  The points are not validated: proof_points_valid
// applies zkmi_groth16_verify's checks (on the curve / twist, B in the
// subgroup) to well-formed words.
int proof_decode_words(int fmt, const uint8_t* in, uint64_t a[8], uint64_t b[16], uint64_t c[8]);
bool proof_points_valid(const uint64_t a[8], const uint64_t b[16], const uint64_t c[8]);

F12 f12_one();
F12 f12_mul(const F12& a, const F12& b);
F12 f12_sqr(const F12& a);
// a * (sparse element with terms cf[t] w^pw[t])
F12 f12_mul_sparse(const F12& a, const int* pw, const F4* cf, int nt);
// 12 canonical coefficients (4 x u64 each) <-> F12
F12 f12_from_canon(const uint64_t c[48]);
void f12_to_canon(uint64_t c[48], const F12& a);

// The pairing check in two halves: prod_k e(P_k, Q_k) = 1 iff
// final_exp_is_one(miller_value(ps, qs)).  Pairs with a point at infinity
// contribute 1.  Miller values of disjoint pair sets multiply (f12_mul).
F12 miller_value(const std::vector<G1>& ps, const std::vector<G2>& qs);
bool final_exp_is_one(const F12& f);
F12 f12_frob2(const F12& a);
// The constants of final_exp_is_one for the device routine of pairing.h:
// zeta^i (w^(q^2) = zeta w; 12 canonical Fq) and the exponent
// (q^4 - q^2 + 1) / r, little-endian.
void final_exp_constants(uint64_t zeta[48], uint64_t hard[12]);
bool pairing_product_is_one(const std::vector<G1>& ps, const std::vector<G2>& qs);

// ------------------------------------------------ batched verification
// zkmi_groth16_verify_many's host half, over values the GPU
// (or a host stand-in) already computed.  For proofs i < nb under vk:
//   bad[i]   != 0: proof i failed point validation (never valid)
//   rho      nb x 2 u64, every 128-bit weight non-zero
//   inputs   nb x n_inputs x 4 u64, every value < r
//   f[i]     Miller value of (rho_i A_i, B_i)   (anything for bad[i])
//   rc[i]    rho_i C_i
struct VerifyManyIn {
  const Vk* vk;
  size_t nb, n_inputs;
  const uint64_t* inputs;
  const uint64_t* rho;
  const uint8_t* bad;
  const F12* f;
  const G1* rc;
};
// ZKMI_EINVAL for a zero weight or an input >= r (checked by the entry point
// before any GPU work, and by verify_many_combine again); rho = NULL checks
// the inputs alone (verify_each has no weights)
int verify_many_check_scalars(size_t nb, size_t n_inputs, const uint64_t* inputs, const uint64_t* rho);
// The G1 sides of a subset's three fixed-G2 pairs:
//   out = { -(sum rho_i) alpha, -sum rho_i X_i, -sum rho_i C_i },  i in idx,
// paired with (beta, gamma, delta).  X_i = IC[0] + sum_j x_ij IC[j+1].
void verify_many_fixed_g1(const VerifyManyIn& in, const size_t* idx, size_t n, G1 out[3]);
// fixed_all: the Miller value of the three fixed pairs of ALL proofs with
// bad[i] == 0 (the GPU's lanes nb .. nb+2 multiplied), or NULL to compute it
// here.  Writes valid[nb]; adds the final exponentiations it ran and the
// number of bad[i] to *st (st may be NULL).  One final exponentiation when
// the combined check holds; otherwise bisection, at most two probes a level.
int verify_many_combine(const VerifyManyIn& in, const F12* fixed_all, uint8_t* valid, zkmi_verify_stats* st);
// The same with a budget of final exponentiations (zkmi_ctx_set_verify_probes):
// max_probes = 0 is verify_many_combine.  With max_probes >= 1 the first
// combined check counts as a probe, no probe runs once max_probes have, and
// the proofs that would have needed one come back in *undecided (ascending
// within a subset; valid[i] = 0 for them until the caller decides them).
// Decided and undecided proofs partition those with bad[i] == 0.
int verify_many_combine_budget(const VerifyManyIn& in, const F12* fixed_all, uint64_t max_probes, uint8_t* valid,
                               zkmi_verify_stats* st, std::vector<size_t>* undecided);

}  // namespace zkv
