// verify_budget_check — the budgeted combine of zkmi_groth16_verify_many
// (verify.cpp verify_many_combine_budget, zkmi_ctx_set_verify_probes) without
// a GPU, in the style of verify_many_check: this program plays the GPU's part
// with the device header compiled for the host and the host G1 arithmetic.
//
//   verify_budget_check SETS
// SETS: the format of verify_many_check.
// Per set, nb = 8 (proofs repeated cyclically, fixed weights), the batches
//   all valid | one bad | all bad | valid, bad and flagged proofs mixed
// and for each the budgets 1, 2, 5 and unlimited (0):
//   * decided and undecided proofs partition the unflagged ones (an
//     undecided proof has valid = 0 and appears once),
//   * every decided verdict is zkmi_groth16_verify's,
//   * final_exps <= the budget,
//   * unlimited: verdicts, final_exps and invalid_points equal
//     verify_many_combine's, and nothing is undecided.
// Prints "ok <sets> <runs>".
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

static int runs = 0;
// one batch: proof i is base proof i % n; tamper[i]: 0 none, 1 C <- 2C, 2 first
// input + 1, 3 flagged by point validation (A off the curve)
static int run(const Set& s, const std::vector<int>& tamper, const std::vector<F12>& f_cache) {
  const size_t nb = tamper.size();
  std::vector<uint64_t> inputs(nb * s.n_inputs * 4), rho(2 * nb);
  std::vector<uint8_t> bad(nb, 0), expect(nb);
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
    CHECK(expect[i] == (tamper[i] == 0), "proof %zu: the host verifier says %d for tamper %d", i, expect[i], tamper[i]);
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
  std::vector<uint8_t> ref(nb, 7);
  zkmi_verify_stats rst = {0, 0, 0};
  CHECK(verify_many_combine(in, &fixed, ref.data(), &rst) == 0, "verify_many_combine failed");
  for (uint64_t budget : {1ULL, 2ULL, 5ULL, 0ULL}) {
    std::vector<uint8_t> valid(nb, 7);
    std::vector<size_t> und = {99};
    zkmi_verify_stats st = {0, 0, 0};
    CHECK(verify_many_combine_budget(in, &fixed, budget, valid.data(), &st, &und) == 0, "the budgeted combine failed");
    std::vector<int> seen(nb, 0);
    for (size_t i : und) {
      CHECK(i < nb && !bad[i] && !seen[i], "budget %llu: undecided index %zu is flagged, repeated or out of range",
            (unsigned long long)budget, i);
      CHECK(valid[i] == 0, "budget %llu: undecided proof %zu has verdict %d", (unsigned long long)budget, i, valid[i]);
      seen[i] = 1;
    }
    for (size_t i = 0; i < nb; i++) {
      if (seen[i]) continue;
      CHECK(valid[i] == (bad[i] ? 0 : expect[i]), "budget %llu: proof %zu decided %d, zkmi_groth16_verify says %d",
            (unsigned long long)budget, i, valid[i], expect[i]);
    }
    if (budget) {
      CHECK(st.final_exps <= budget, "budget %llu: %llu final exponentiations", (unsigned long long)budget,
            (unsigned long long)st.final_exps);
      CHECK(st.final_exps >= 1 || idx.empty(), "budget %llu: the first combined check did not run",
            (unsigned long long)budget);
      // nothing is left over when bisection would have fitted the budget
      if (rst.final_exps <= budget) CHECK(und.empty() && valid == ref, "budget %llu not needed, yet the result differs",
                                          (unsigned long long)budget);
    } else {
      CHECK(und.empty(), "unlimited: %zu proofs undecided", und.size());
      CHECK(valid == ref, "unlimited: verdicts differ from verify_many_combine's");
      CHECK(st.final_exps == rst.final_exps && st.invalid_points == rst.invalid_points && st.pairs == rst.pairs,
            "unlimited: stats differ from verify_many_combine's (%llu vs %llu final exponentiations)",
            (unsigned long long)st.final_exps, (unsigned long long)rst.final_exps);
    }
    runs++;
  }
  return 0;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: verify_budget_check SETS");
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
    std::vector<F12> fc(8);
    for (size_t i = 0; i < 8; i++) {
      const Proof& p = s.proofs[i % np];
      const uint64_t k[4] = {weight(i, 0), weight(i, 1), 0, 0};
      fc[i] = dev_miller(g1_mul(g1_from_canon(p.a), k), g2_from_canon(p.b));
    }
    const std::vector<std::vector<int>> batches = {
        {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 1, 0, 0}, {1, 2, 1, 2, 1, 2, 1, 2}, {0, 1, 3, 2, 0, 0, 3, 1}};
    for (size_t k = 0; k < batches.size(); k++)
      if (run(s, batches[k], fc)) {
        fprintf(stderr, "set %llu, batch %zu\n", (unsigned long long)si, k);
        return 1;
      }
  }
  fclose(fp);
  printf("ok %llu %d\n", (unsigned long long)nsets, runs);
  return 0;
}
