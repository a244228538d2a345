// verify_many_check — zkmi_groth16_verify_many's host half (verify.cpp
// verify_many_combine) without a GPU: this program plays the GPU's part with
// the device header (zelana_amd/csrc/pairing.h compiled for the host: one
// Miller loop per pair) and the host G1 arithmetic (rho_i A_i, rho_i C_i),
// then runs the library's combine-and-bisect routine.
//
//   verify_many_check SETS
// SETS: text, "nsets" then per set: "vk_len" + vk bytes (decimal), "n_inputs
// nproofs", per proof n_inputs x 4 + 8 + 16 + 8 u64 (inputs, A, B, C).
// Per set (proofs repeated cyclically to the batch size, fixed weights):
//   nb = 5: all valid -> all 1 with one final exponentiation; each single bad
//   position -> exactly that 0; two bad; all bad; one proof flagged by point
//   validation; nb = 8 with one bad: final_exps <= 1 + 2 ceil(log2 nb);
//   a zero weight is refused.
// Expected verdicts come from zkmi_groth16_verify on each (tampered) proof.
// Prints "ok <sets> <scenarios>".
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zelana_amd/csrc/pairing.h"
#include "../../zelana_amd/csrc/verify_internal.h"

namespace zk {
void set_error(const char*, ...) {}
}  // namespace zk

using namespace zkv;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

static zk::Fe fe_of(const uint64_t c[4]) {
  uint32_t w[8];
  memcpy(w, c, 32);
  return zk::to_mont<zk::FqP>(zk::unpack(w));
}
// k_miller's part: the header's Miller value of one pair
static F12 dev_miller(const G1& P, const G2& Q) {
  if (P.inf || Q.inf) return f12_one();
  uint64_t p[8], q[16], c[48];
  g1_to_canon(p, P);
  g2_to_canon(q, Q);
  zk::F12Reg f[2];
  const zk::Fe2 qx = {fe_of(q), fe_of(q + 4)}, qy = {fe_of(q + 8), fe_of(q + 12)};
  const int k = zk::miller_loop(f[0], f[1], fe_of(p), fe_of(p + 4), qx, qy);
  for (int i = 0; i < 12; i++) {
    uint32_t w[8];
    zk::pack(w, zk::from_mont<zk::FqP>(f[k].c[i]));
    memcpy(c + 4 * i, w, 32);
  }
  return f12_from_canon(c);
}

struct Proof {
  std::vector<uint64_t> in;
  uint64_t a[8], b[16], c[8];
};
struct Set {
  std::vector<uint8_t> vkb;
  Vk vk;
  size_t n_inputs;
  std::vector<Proof> proofs;
};

static uint64_t weight(size_t i, int w) { return 0x9E3779B97F4A7C15ULL * (2 * i + w + 1) + 0x1234567 * (i + 1); }

// one batch: proof i is base proof i % n; tamper[i]: 0 none, 1 C <- 2C, 2 first
// input + 1, 3 flagged by point validation (A off the curve)
static int run(const Set& s, const std::vector<int>& tamper, const std::vector<F12>& f_cache, uint64_t max_exps,
               bool expect_one_exp) {
  const size_t nb = tamper.size();
  std::vector<uint64_t> inputs(nb * s.n_inputs * 4), rho(2 * nb);
  std::vector<uint8_t> bad(nb, 0), valid(nb, 7), expect(nb);
  std::vector<G1> rc(nb);
  std::vector<F12> f(nb);
  for (size_t i = 0; i < nb; i++) {
    Proof p = s.proofs[i % s.proofs.size()];
    if (tamper[i] == 1) {
      G1 C = g1_from_canon(p.c);
      g1_to_canon(p.c, g1_add(C, C));
    }
    if (tamper[i] == 2) p.in[0] += 1;
    if (tamper[i] == 3) p.a[4] ^= 1;
    memcpy(inputs.data() + i * s.n_inputs * 4, p.in.data(), s.n_inputs * 32);
    rho[2 * i] = weight(i, 0);
    rho[2 * i + 1] = weight(i, 1);
    int v = -1;
    CHECK(zkmi_groth16_verify(s.vkb.data(), s.vkb.size(), p.in.data(), s.n_inputs, p.a, p.b, p.c, &v) == 0,
          "zkmi_groth16_verify failed");
    expect[i] = (uint8_t)v;
    // k_verify_prepare's part
    const G1 A = g1_from_canon(p.a), C = g1_from_canon(p.c);
    const G2 B = g2_from_canon(p.b);
    bad[i] = !(g1_on_curve(A) && g1_on_curve(C) && g2_on_curve(B) && g2_in_subgroup(B));
    if (bad[i]) continue;
    const uint64_t k[4] = {rho[2 * i], rho[2 * i + 1], 0, 0};
    rc[i] = g1_mul(C, k);
    f[i] = f_cache[i];  // Miller value of (rho_i A_i, B_i): the tampering above leaves A and B alone
  }
  VerifyManyIn in = {&s.vk, nb, s.n_inputs, inputs.data(), rho.data(), bad.data(), f.data(), rc.data()};
  std::vector<size_t> idx;
  for (size_t i = 0; i < nb; i++)
    if (!bad[i]) idx.push_back(i);
  G1 g[3];
  verify_many_fixed_g1(in, idx.data(), idx.size(), g);
  const F12 fixed = f12_mul(f12_mul(dev_miller(g[0], s.vk.beta), dev_miller(g[1], s.vk.gamma)),
                            dev_miller(g[2], s.vk.delta));
  zkmi_verify_stats st = {0, 0, 0};
  CHECK(verify_many_combine(in, &fixed, valid.data(), &st) == 0, "verify_many_combine failed");
  for (size_t i = 0; i < nb; i++) {
    CHECK(valid[i] == expect[i], "proof %zu of %zu: verdict %d, zkmi_groth16_verify says %d", i, nb, valid[i],
          expect[i]);
    CHECK(expect[i] == (tamper[i] == 0), "proof %zu: the host verifier says %d for tamper %d", i, expect[i], tamper[i]);
  }
  CHECK(st.final_exps <= max_exps, "%llu final exponentiations, at most %llu allowed",
        (unsigned long long)st.final_exps, (unsigned long long)max_exps);
  if (expect_one_exp) CHECK(st.final_exps == 1, "%llu final exponentiations on the all-valid path",
                            (unsigned long long)st.final_exps);
  uint64_t nflag = 0;
  for (size_t i = 0; i < nb; i++) nflag += tamper[i] == 3;
  CHECK(st.invalid_points == nflag, "invalid_points %llu, expected %llu", (unsigned long long)st.invalid_points,
        (unsigned long long)nflag);
  return 0;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: verify_many_check SETS");
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp, "cannot open %s", argv[1]);
  auto rd = [&](uint64_t* v) {
    unsigned long long t;
    if (fscanf(fp, "%llu", &t) != 1) return false;
    *v = t;
    return true;
  };
  uint64_t nsets = 0, v;
  CHECK(rd(&nsets), "bad file");
  int scenarios = 0;
  for (uint64_t si = 0; si < nsets; si++) {
    Set s;
    uint64_t len, np;
    CHECK(rd(&len), "bad set");
    s.vkb.resize(len);
    for (auto& b : s.vkb) {
      CHECK(rd(&v), "bad key");
      b = (uint8_t)v;
    }
    const char* why = "";
    CHECK(vk_decode(s.vkb.data(), s.vkb.size(), &s.vk, &why), "key: %s", why);
    CHECK(rd(&v) && rd(&np) && np > 0, "bad set header");
    s.n_inputs = v;
    CHECK(s.n_inputs >= 1 && s.vk.ic.size() == s.n_inputs + 1, "input count");
    s.proofs.resize(np);
    for (auto& p : s.proofs) {
      p.in.resize(4 * s.n_inputs);
      for (auto& x : p.in) CHECK(rd(&x), "bad proof");
      for (auto& x : p.a) CHECK(rd(&x), "bad proof");
      for (auto& x : p.b) CHECK(rd(&x), "bad proof");
      for (auto& x : p.c) CHECK(rd(&x), "bad proof");
    }
    // the per-proof Miller values for positions 0..7 under the fixed weights
    std::vector<F12> fc(8);
    for (size_t i = 0; i < 8; i++) {
      const Proof& p = s.proofs[i % np];
      const uint64_t k[4] = {weight(i, 0), weight(i, 1), 0, 0};
      fc[i] = dev_miller(g1_mul(g1_from_canon(p.a), k), g2_from_canon(p.b));
    }
    const uint64_t ANY = ~0ULL;
    std::vector<std::vector<int>> five = {{0, 0, 0, 0, 0}};
    for (int p = 0; p < 5; p++) {
      std::vector<int> t(5, 0);
      t[p] = 1 + p % 2;
      five.push_back(t);
    }
    five.push_back({0, 1, 0, 2, 0});
    five.push_back({1, 2, 1, 2, 1});
    five.push_back({0, 0, 3, 0, 0});
    five.push_back({3, 0, 1, 0, 0});
    for (size_t k = 0; k < five.size(); k++) {
      const bool all_ok = k == 0 || k == 8;  // nothing but flagged proofs fails
      if (run(s, five[k], fc, ANY, all_ok)) {
        fprintf(stderr, "set %llu, nb = 5 scenario %zu\n", (unsigned long long)si, k);
        return 1;
      }
      scenarios++;
    }
    // one bad among 8: 1 + 2 ceil(log2 8) = 7 final exponentiations at most
    for (int p : {0, 5, 7}) {
      std::vector<int> t(8, 0);
      t[p] = 1;
      if (run(s, t, fc, 7, false)) {
        fprintf(stderr, "set %llu, nb = 8 bad at %d\n", (unsigned long long)si, p);
        return 1;
      }
      scenarios++;
    }
    // a zero weight is refused
    {
      std::vector<uint64_t> inputs(2 * s.n_inputs * 4, 0), rho = {1, 0, 0, 0};
      std::vector<uint8_t> bad(2, 0), valid(2);
      std::vector<G1> rc(2, G1{F4{{0, 0, 0, 0}}, F4{{0, 0, 0, 0}}, true});
      std::vector<F12> f(2, f12_one());
      VerifyManyIn in = {&s.vk, 2, s.n_inputs, inputs.data(), rho.data(), bad.data(), f.data(), rc.data()};
      CHECK(verify_many_combine(in, nullptr, valid.data(), nullptr) == ZKMI_EINVAL, "a zero weight was accepted");
      CHECK(verify_many_check_scalars(2, s.n_inputs, inputs.data(), rho.data()) == ZKMI_EINVAL, "zero weight");
      memcpy(inputs.data(), RP, 32);
      rho[2] = 5;
      CHECK(verify_many_check_scalars(2, s.n_inputs, inputs.data(), rho.data()) == ZKMI_EINVAL, "input >= r accepted");
      scenarios++;
    }
  }
  fclose(fp);
  printf("ok %llu %d\n", (unsigned long long)nsets, scenarios);
  return 0;
}
