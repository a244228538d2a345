// Host check of the batched-MSM epilogue (msm_host.cpp msm_host_batch_combine,
// what zkmi_msm_batch_wait runs on a group job's bit sums): a job of nb x W
// windows -- the batch index as an outer window -- must give, per batch, the
// point of that batch's own W windows, equal to nb separate single-job
// epilogues; it must never Horner-combine across the whole job.  G1 and G2,
// one and two segments per term, a batch whose terms are all at infinity.
// Prints "ok <n>".
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../zelana_amd/csrc/host_field.h"
#include "../../zelana_amd/csrc/zkmi_internal_host.h"

using namespace zkh;
using zk::Xyzz;

static uint64_t rng = 0xD1B54A32D192ED03ull;
static uint64_t next() {
  rng ^= rng << 13;
  rng ^= rng >> 7;
  rng ^= rng << 17;
  return rng;
}
template <class F>
static Xyzz<F> mul(Xyzz<F> p, uint64_t k) {
  Xyzz<F> acc = zk::xyzz_inf<F>();
  for (int b = 63; b >= 0; b--) {
    acc = zk::xyzz_dbl(acc);
    if ((k >> b) & 1) acc = zk::xyzz_add(acc, p);
  }
  return acc;
}
static void put_f(uint32_t* w, const F4& a) {
  uint64_t c[4];
  to_canon(c, a);
  for (int i = 0; i < 4; i++) w[2 * i] = (uint32_t)c[i], w[2 * i + 1] = (uint32_t)(c[i] >> 32);
}
static void put_f(uint32_t* w, const F42& a) {
  put_f(w, a.c0);
  put_f(w + 8, a.c1);
}
template <class F, int CW>
static void put_term(uint32_t* w, const Xyzz<F>& p) {  // canonical packed XYZZ (all-zero = infinity)
  if (zk::xyzz_is_inf(p)) {
    memset(w, 0, 4 * CW * 4);
    return;
  }
  put_f(w, p.x);
  put_f(w + CW, p.y);
  put_f(w + 2 * CW, p.zz);
  put_f(w + 3 * CW, p.zzz);
}

// nb batches of W windows; batch `inf` (or none, -1) has every term at infinity
template <class F, int CW>
static int run(const Xyzz<F>& G, int g2, int c, int W, int sb, int nb, int inf) {
  const int bb = c - 1, XW = 4 * CW, PW = g2 ? 16 : 8;
  const size_t per = (size_t)W * (bb + 1) * sb * XW;  // words of one batch's bit sums
  int bad = 0;
  std::vector<uint32_t> job((size_t)nb * per, 0);
  for (int b = 0; b < nb; b++)
    for (size_t t = 0; t < (size_t)W * (bb + 1) * sb; t++) {
      const Xyzz<F> p = b == inf || next() % 7 == 0 ? zk::xyzz_inf<F>() : mul(G, next() >> 8);
      put_term<F, CW>(job.data() + (size_t)b * per + t * XW, p);
    }
  std::vector<uint64_t> got((size_t)nb * PW, ~0ull);
  zk::msm_host_batch_combine(job.data(), nb, g2, c, W, bb, sb, got.data());
  const int one[1] = {0};
  bool distinct = false;
  for (int b = 0; b < nb; b++) {
    uint64_t want[16];
    // the single-job epilogue over a copy of batch b's bit sums alone
    std::vector<uint32_t> single(job.begin() + (size_t)b * per, job.begin() + (size_t)(b + 1) * per);
    zk::msm_host_assemble_combine(single.data(), per, 0, one, 1, false, g2, c, W, bb, sb, want);
    bad += memcmp(&got[(size_t)b * PW], want, PW * 8) != 0;
    bool zero = true;
    for (int i = 0; i < PW; i++) zero &= got[(size_t)b * PW + i] == 0;
    bad += zero != (b == inf);  // infinity exactly for the all-infinity batch
    if (b && memcmp(&got[(size_t)b * PW], &got[0], PW * 8) != 0) distinct = true;
  }
  bad += !distinct;  // random batches give different points
  // and it is not the Horner pass over all nb * W windows
  uint64_t whole[16];
  zk::msm_host_assemble_combine(job.data(), (size_t)nb * per, 0, one, 1, false, g2, c, nb * W, bb, sb, whole);
  bad += memcmp(whole, &got[0], PW * 8) == 0;
  return bad;
}

int main() {
  const uint64_t g1[8] = {1, 0, 0, 0, 2, 0, 0, 0};
  const uint64_t g2[16] = {0x46debd5cd992f6edULL, 0x674322d4f75edaddULL, 0x426a00665e5c4479ULL, 0x1800deef121f1e76ULL,
                           0x97e485b7aef312c2ULL, 0xf1aa493335a9e712ULL, 0x7260bfb731fb5d25ULL, 0x198e9393920d483aULL,
                           0x4ce6cc0166fa7daaULL, 0xe3d1e7690c43d37bULL, 0x4aab71808dcb408fULL, 0x12c85ea5db8c6debULL,
                           0x55acdadcd122975bULL, 0xbc4b313370b38ef3ULL, 0xec9e99ad690c3395ULL, 0x090689d0585ff075ULL};
  const Xyzz<HFq> G1 = zk::xyzz_from_aff(zk::Aff<HFq>{from_canon(g1), from_canon(g1 + 4)});
  const Xyzz<HFq2> G2 =
      zk::xyzz_from_aff(zk::Aff<HFq2>{{from_canon(g2), from_canon(g2 + 4)}, {from_canon(g2 + 8), from_canon(g2 + 12)}});
  int bad = 0, n = 0;
  for (int sb = 1; sb <= 2; sb++) {
    bad += run<HFq, 8>(G1, 0, 4, 5, sb, 3, -1), n++;
    bad += run<HFq, 8>(G1, 0, 3, 1, sb, 3, 1), n++;  // one window per batch (a full table), batch 1 at infinity
    bad += run<HFq2, 16>(G2, 1, 4, 4, sb, 3, -1), n++;
    bad += run<HFq2, 16>(G2, 1, 4, 2, sb, 3, 2), n++;
  }
  if (bad) {
    printf("FAIL %d of %d\n", bad, n);
    return 1;
  }
  printf("ok %d\n", n);
  return 0;
}
