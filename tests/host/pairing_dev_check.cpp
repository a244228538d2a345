// pairing_dev_check — the device header's Fq12 arithmetic and Miller loop
// (zelana_amd/csrc/pairing.h, compiled for the host) against verify.cpp's.
//
//   pairing_dev_check CASES
// CASES: text, "ncases" then per case "npairs expected" and per pair 24 u64
// (G1 x, y; G2 x.c0, x.c1, y.c0, y.c1; canonical, all-zero = infinity).
// 1. f12_mul / f12_sqr / the sparse line product on random elements equal
//    verify.cpp's coefficient by coefficient.
// 2. per case: the product of the header's per-pair Miller values, through
//    verify.cpp's final exponentiation, decides as verify.cpp's own Miller
//    value does and as the case expects; a single pair's Miller value equals
//    verify.cpp's coefficient by coefficient.
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
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
static F12 rnd_f12() {
  uint64_t c[48];
  for (int i = 0; i < 12; i++) rnd_canon(c + 4 * i);
  return f12_from_canon(c);
}
#define CHECK(cond, ...)          \
  do {                            \
    if (!(cond)) {                \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");      \
      return 1;                   \
    }                             \
  } while (0)

// the header's Miller value of one pair (1 for a pair with a point at infinity)
static F12 dev_miller(const uint64_t p[8], const uint64_t q[16]) {
  bool pz = true, qz = true;
  for (int i = 0; i < 8; i++) pz &= p[i] == 0;
  for (int i = 0; i < 16; i++) qz &= q[i] == 0;
  if (pz || qz) return f12_one();
  zk::F12Reg f[2];
  const zk::Fe2 qx = {fe_of(q), fe_of(q + 4)}, qy = {fe_of(q + 8), fe_of(q + 12)};
  const int k = zk::miller_loop(f[0], f[1], fe_of(p), fe_of(p + 4), qx, qy);
  return host_of(f[k]);
}

int main(int argc, char** argv) {
  const zk::F12Const K = zk::f12_const();
  const int NR = 64;
  for (int t = 0; t < NR; t++) {
    F12 a = rnd_f12(), b = rnd_f12();
    if (t == 0) a = f12_one();
    if (t == 1) memset(&b, 0, sizeof(b));
    zk::F12Reg da = dev_of(a), db = dev_of(b), o;
    zk::f12_mul(o, da, db, K);
    CHECK(f12_same(host_of(o), f12_mul(a, b)), "f12_mul differs at %d", t);
    zk::f12_sqr(o, da, K);
    CHECK(f12_same(host_of(o), f12_sqr(a)), "f12_sqr differs at %d", t);
    // the line's five terms at powers 0, 2, 3, 8, 9
    const int pw[5] = {0, 2, 3, 8, 9};
    F4 cf[5];
    for (int k = 0; k < 5; k++) cf[k] = b.c[k];
    const zk::Line l = {db.c[0], db.c[1], db.c[2], db.c[3], db.c[4]};
    zk::f12_mul_line(o, da, l, K);
    CHECK(f12_same(host_of(o), f12_mul_sparse(a, pw, cf, 5)), "sparse product differs at %d", t);
  }
  CHECK(argc > 1, "usage: pairing_dev_check CASES");
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp, "cannot open %s", argv[1]);
  int ncases = 0;
  CHECK(fscanf(fp, "%d", &ncases) == 1, "bad case file");
  for (int cs = 0; cs < ncases; cs++) {
    int np = 0, expect = 0;
    CHECK(fscanf(fp, "%d %d", &np, &expect) == 2, "bad case header");
    std::vector<G1> ps;
    std::vector<G2> qs;
    F12 fd = f12_one();
    for (int k = 0; k < np; k++) {
      uint64_t w[24];
      for (int i = 0; i < 24; i++) {
        unsigned long long v;
        CHECK(fscanf(fp, "%llu", &v) == 1, "bad pair");
        w[i] = v;
      }
      ps.push_back(g1_from_canon(w));
      qs.push_back(g2_from_canon(w + 8));
      const F12 one_pair = dev_miller(w, w + 8);
      CHECK(f12_same(one_pair, miller_value({ps.back()}, {qs.back()})), "Miller value of case %d pair %d differs", cs, k);
      fd = f12_mul(fd, one_pair);
    }
    const bool host = final_exp_is_one(miller_value(ps, qs));
    const bool dev = final_exp_is_one(fd);
    CHECK(host == (expect != 0), "case %d: the host pairing says %d, expected %d", cs, (int)host, expect);
    CHECK(dev == host, "case %d: the header's Miller values decide %d, the host's %d", cs, (int)dev, (int)host);
  }
  fclose(fp);
  printf("ok %d %d\n", NR, ncases);
  return 0;
}
