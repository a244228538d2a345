// final_exp_dev_check — the device header's final exponentiation
// (zelana_amd/csrc/pairing.h final_exp_is_one / f12_frob2, compiled for the
// host with F12Reg) against verify.cpp's.
//
//   final_exp_dev_check CASES
// CASES: the format of pairing_dev_check ("ncases", per case "npairs expected"
// and per pair 24 u64).
// 1. Frobenius^2 on random elements equals verify.cpp's f12_frob2 coefficient
//    by coefficient (the constants come from final_exp_constants).
// 2. the verdict equals verify.cpp's final_exp_is_one on f = 1, f = 0, random
//    elements, elements with even coefficients only, each case's Miller value
//    (where the verdict must also be the case's expected one), and each true
//    case's value multiplied by a random even-coefficient element (still true).
// Prints "ok <random elements> <cases>".
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

static uint64_t rng_state = 0xD1B54A32D192ED03ULL;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static void rnd_canon(uint64_t c[4]) {
  for (int i = 0; i < 4; i++) c[i] = rnd();
  c[3] &= (1ULL << 60) - 1;  // < 2^252 < q
}
static zk::Fe fe_of(const uint64_t c[4]) {
  uint32_t w[8];
  memcpy(w, c, 32);
  return zk::to_mont<zk::FqP>(zk::unpack(w));
}
static void canon_of(uint64_t c[4], const zk::Fe& a) {
  uint32_t w[8];
  zk::pack(w, zk::from_mont<zk::FqP>(a));
  memcpy(c, w, 32);
}
static zk::F12Reg dev_of(const F12& a) {
  uint64_t c[48];
  f12_to_canon(c, a);
  zk::F12Reg r;
  for (int i = 0; i < 12; i++) r.c[i] = fe_of(c + 4 * i);
  return r;
}
static F12 host_of(const zk::F12Reg& a) {
  uint64_t c[48];
  for (int i = 0; i < 12; i++) canon_of(c + 4 * i, a.c[i]);
  return f12_from_canon(c);
}
static bool f12_same(const F12& a, const F12& b) {
  uint64_t x[48], y[48];
  f12_to_canon(x, a);
  f12_to_canon(y, b);
  return memcmp(x, y, sizeof(x)) == 0;
}
// even_only: the odd coefficients are zero (an element of Fq6)
static F12 rnd_f12(bool even_only) {
  uint64_t c[48];
  memset(c, 0, sizeof(c));
  for (int i = 0; i < 12; i += even_only ? 2 : 1) rnd_canon(c + 4 * i);
  return f12_from_canon(c);
}
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

static zk::FinalExpConst FC;
static bool dev_verdict(const F12& f) {
  zk::F12Reg e = dev_of(f), t0, t1;
  return zk::final_exp_is_one(e, t0, t1, FC.zeta, FC.hard);
}

int main(int argc, char** argv) {
  uint64_t zeta[48];
  final_exp_constants(zeta, FC.hard);
  for (int i = 0; i < 12; i++) FC.zeta[i] = fe_of(zeta + 4 * i);
  const int NR = 32;
  for (int t = 0; t < NR; t++) {
    const F12 a = rnd_f12(false);
    zk::F12Reg da = dev_of(a), o;
    zk::f12_frob2(o, da, FC.zeta);
    CHECK(f12_same(host_of(o), f12_frob2(a)), "Frobenius^2 differs at %d", t);
  }
  F12 zero;
  memset(&zero, 0, sizeof(zero));
  CHECK(dev_verdict(f12_one()) && final_exp_is_one(f12_one()), "f = 1 must pass");
  CHECK(!dev_verdict(zero) && !final_exp_is_one(zero), "f = 0 must fail");
  for (int t = 0; t < 3; t++) {
    const F12 a = rnd_f12(false), e = rnd_f12(true);
    CHECK(dev_verdict(a) == final_exp_is_one(a), "random element %d: verdicts differ", t);
    CHECK(dev_verdict(e) == final_exp_is_one(e), "even-coefficient element %d: verdicts differ", t);
    CHECK(final_exp_is_one(e), "an element of Fq6 must pass");
  }
  CHECK(argc > 1, "usage: final_exp_dev_check CASES");
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp, "cannot open %s", argv[1]);
  int ncases = 0;
  CHECK(fscanf(fp, "%d", &ncases) == 1, "bad case file");
  for (int cs = 0; cs < ncases; cs++) {
    int np = 0, expect = 0;
    CHECK(fscanf(fp, "%d %d", &np, &expect) == 2, "bad case header");
    std::vector<G1> ps;
    std::vector<G2> qs;
    for (int k = 0; k < np; k++) {
      uint64_t w[24];
      for (int i = 0; i < 24; i++) {
        unsigned long long v;
        CHECK(fscanf(fp, "%llu", &v) == 1, "bad pair");
        w[i] = v;
      }
      ps.push_back(g1_from_canon(w));
      qs.push_back(g2_from_canon(w + 8));
    }
    const F12 f = miller_value(ps, qs);
    const bool host = final_exp_is_one(f), dev = dev_verdict(f);
    CHECK(host == (expect != 0), "case %d: the host says %d, expected %d", cs, (int)host, expect);
    CHECK(dev == host, "case %d: the header decides %d, the host %d", cs, (int)dev, (int)host);
    const F12 g = f12_mul(f, rnd_f12(true));  // a factor in Fq6 dies in the exponentiation
    CHECK(final_exp_is_one(g) == host && dev_verdict(g) == host, "case %d times an Fq6 element: verdict moved", cs);
  }
  fclose(fp);
  printf("ok %d %d\n", NR, ncases);
  return 0;
}
