// Host build of the R1CS check's row predicate (zelana_amd/csrc/r1cs_row.h,
// host + device): r1cs_row_bad(a, b, c) on the value-form, < 2r numbers
// k_matvec leaves must say a b != c mod r, whichever of the representatives
// x and x + r each of a, b, c arrives as.  Checked against plain 256-bit
// integer arithmetic (double-and-add product, no Montgomery form).
// Prints "ok <n>".
#include <stdint.h>
#include <stdio.h>

#include "../../zelana_amd/csrc/r1cs_row.h"

using namespace zk;

struct U256 {
  uint64_t v[4];
};
static const U256 RMOD = {{0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull, 0x30644e72e131a029ull}};

static bool geq(const U256& a, const U256& b) {
  for (int i = 3; i >= 0; i--)
    if (a.v[i] != b.v[i]) return a.v[i] > b.v[i];
  return true;
}
static U256 add_raw(const U256& a, const U256& b) {  // (no overflow: operands < 2^255)
  U256 r;
  unsigned __int128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (unsigned __int128)a.v[i] + b.v[i];
    r.v[i] = (uint64_t)c;
    c >>= 64;
  }
  return r;
}
static U256 sub_raw(const U256& a, const U256& b) {
  U256 r;
  uint64_t br = 0;
  for (int i = 0; i < 4; i++) {
    const uint64_t t = a.v[i] - b.v[i], t2 = t - br;
    br = (a.v[i] < b.v[i]) | (t < br);
    r.v[i] = t2;
  }
  return r;
}
static U256 add_mod(const U256& a, const U256& b) {
  U256 r = add_raw(a, b);
  return geq(r, RMOD) ? sub_raw(r, RMOD) : r;
}
static U256 mul_mod(const U256& a, const U256& b) {  // a, b < r
  U256 r = {{0, 0, 0, 0}};
  for (int i = 255; i >= 0; i--) {
    r = add_mod(r, r);
    if ((b.v[i >> 6] >> (i & 63)) & 1) r = add_mod(r, a);
  }
  return r;
}
static Fe to_fe(const U256& x) {  // x < 2r < 2^255
  uint32_t w[8];
  for (int i = 0; i < 4; i++) {
    w[2 * i] = (uint32_t)x.v[i];
    w[2 * i + 1] = (uint32_t)(x.v[i] >> 32);
  }
  return unpack(w);
}

static uint64_t rng = 0x243F6A8885A308D3ull;
static uint64_t next() {
  rng ^= rng << 13;
  rng ^= rng >> 7;
  rng ^= rng << 17;
  return rng;
}
static U256 rand_fr() {
  for (;;) {
    U256 x = {{next(), next(), next(), next() >> 2}};
    if (!geq(x, RMOD)) return x;
  }
}

static long checks = 0;
// every pairing of the representatives {x, x + r} of a, b and c
static bool all_reps(const U256& a, const U256& b, const U256& c, bool want_bad, const char* what) {
  for (int k = 0; k < 8; k++) {
    const U256 ra = (k & 1) ? add_raw(a, RMOD) : a, rb = (k & 2) ? add_raw(b, RMOD) : b,
               rc = (k & 4) ? add_raw(c, RMOD) : c;
    if (r1cs_row_bad(to_fe(ra), to_fe(rb), to_fe(rc)) != want_bad) {
      printf("%s: representatives %d: expected %s\n", what, k, want_bad ? "bad" : "satisfied");
      return false;
    }
    checks++;
  }
  return true;
}
static bool triple(const U256& a, const U256& b, const char* what) {
  const U256 one = {{1, 0, 0, 0}};
  const U256 c = mul_mod(a, b);
  const U256 up = add_mod(c, one), down = add_mod(c, sub_raw(RMOD, one));  // c + 1, c - 1 mod r
  return all_reps(a, b, c, false, what) && all_reps(a, b, up, true, what) && all_reps(a, b, down, true, what);
}

int main() {
  const U256 zero = {{0, 0, 0, 0}}, one = {{1, 0, 0, 0}}, rm1 = sub_raw(RMOD, one);
  const U256 edge[3] = {zero, one, rm1};
  for (const U256& a : edge)
    for (const U256& b : edge)
      if (!triple(a, b, "edge values")) return 1;
  // an edge value against a random one, both ways
  for (int t = 0; t < 30; t++) {
    const U256 x = rand_fr();
    if (!triple(edge[t % 3], x, "edge x random") || !triple(x, edge[t % 3], "random x edge")) return 1;
  }
  for (int t = 0; t < 1000; t++)
    if (!triple(rand_fr(), rand_fr(), "random")) return 1;
  // a product that is congruent to c only modulo 2^256 must not pass, nor one equal in the low limbs
  {
    const U256 a = rand_fr(), b = rand_fr();
    U256 c = mul_mod(a, b);
    c.v[3] ^= 1;
    if (geq(c, RMOD)) c.v[3] ^= 3;
    if (!all_reps(a, b, c, true, "high limb")) return 1;
  }
  printf("ok %ld\n", checks);
  return 0;
}
