// msm.hip — Pippenger multi-scalar multiplication over BN254 G1 / G2 for
// gfx950.  Replaces ark-ec 0.5.0 VariableBaseMSM::msm_bigint (SURVEY.md §8a
// a7/a8), called by ark-groth16 for h/l/a/b_g1 (G1) and b_g2 (G2).
//
// Pipeline (one HIP stream, all intermediate data resident in HBM):
//   1. k_msm_digits   signed c-bit digits of every scalar (bases at infinity
//                     get none); with a fixed-base table, window w of copy j.
//   2. k_rs_*         two-pass MSD radix sort of (window, bucket) keys with
//                     LDS-ranked scatters and device-wide scans for offsets.
//   3.                bucket starts come out of the second pass's scan.  Order
//                     inside a bucket is irrelevant: group addition is exact,
//                     so results are bit-identical.
//   4. k_msm_acc0     load balance by construction: every thread owns a fixed
//                     chunk of L sorted entries (not a bucket), accumulating
//                     affine points into an XYZZ register accumulator with
//                     mixed additions; runs that are complete inside the chunk
//                     go straight to their bucket, runs cut by a chunk edge
//                     become head/tail partials.
//   5. k_msm_accN     segmented reduction of the partials (level 1 pairs the
//                     two halves of every cut run; deeper levels only see runs
//                     of heavy buckets, e.g. witness-like scalars in {0,1}).
//   6. k_msm_br_*     bucket reduction without a sequential running sum:
//                     S_w = T_w + sum_j 2^j U_{w,j}, U_{w,j} = sum of buckets
//                     whose index has bit j set, computed as parallel tree sums
//                     over a (high, low) split of the bucket index.
//   7. host Horner    sum_k 2^k V_k over the ~256 bit sums (msm_host.cpp).
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <chrono>

#include "dev_io.h"
#include "ec.h"
#include "zkmi_internal.h"

namespace zk {

// Wave priority of the pipeline's tail kernels (sort, scans, item plan,
// piece sums, bucket reduction).  With several MSM lanes in flight they share
// SIMDs with another lane's accumulation, whose older waves win the
// oldest-first issue arbitration: in a rocprofv3 trace of the 3-lane 2^20
// pipeline the 12-us P1 count took 462 us and the scans 7 -> 48 us, and no
// accumulation ran for 28% of the step.  The tails issue little VALU work, so
// letting them win arbitration costs the accumulation little.  (Measured: the
// P1 count no longer waits, 462 -> 12-28 us; the headline moved within noise,
// because the 1024-thread P1 scatter and the 152-VGPR reductions still wait
// for accumulation waves to retire -- a register / LDS footprint matter,
// DESIGN.md §2.1.)
// (Round 5, with the tails running beside the LDS-capped accumulation: tail
// priority 0 / 1 instead of 3 measured 864-866 / 875-880 vs 869-880 Mpt/s at
// 2-3 lanes and 67.7 / 65.9 vs 65.7 ms at 2^26 -- the sort's slack does not
// buy the accumulation anything.)
#define ZK_TAIL_WAVE() __builtin_amdgcn_s_setprio(3)

// ----------------------------------------------------------------- traits
struct G1T {
  using F = FqOps;
  using P = FqP;                 // product form of the full additions (ff.h pmac)
  static constexpr int CW = 8;   // u32 words per coordinate
  static constexpr int PW = 16;  // u32 words per affine point
};
// G1 for the latency-bound kernels of small MSMs (cut sums, cascade, bucket
// reduction below CUTSUM_COOP_K buckets): same layout, compiler-scheduled
// products, whose split column chains shorten a lone wave's dependent path
struct G1Tn : G1T {
  using P = FqPn;
};
struct G2T {
  using F = Fq2Ops;
  using P = FqPn;
  static constexpr int CW = 16;
  static constexpr int PW = 32;
};

template <class F>
struct Io;
template <>
struct Io<FqOps> {
  static __device__ __forceinline__ Fe ld(const uint32_t* p) { return ld_fe(p); }
  static __device__ __forceinline__ void st(uint32_t* p, const Fe& f) { st_fe(p, f); }
  static __device__ __forceinline__ Fe canon(const Fe& f) { return from_mont<FqP>(f); }
};
template <>
struct Io<Fq2Ops> {
  static __device__ __forceinline__ Fe2 ld(const uint32_t* p) { return {ld_fe(p), ld_fe(p + 8)}; }
  static __device__ __forceinline__ void st(uint32_t* p, const Fe2& f) {
    st_fe(p, f.c0);
    st_fe(p + 8, f.c1);
  }
  static __device__ __forceinline__ Fe2 canon(const Fe2& f) { return {from_mont<FqP>(f.c0), from_mont<FqP>(f.c1)}; }
};

// affine base: x (CW words) || y (CW words); bit 31 of the last word = infinity
template <class G>
__device__ __forceinline__ Aff<typename G::F> ld_aff(const uint32_t* bases, uint32_t idx) {
  const uint32_t* p = bases + (size_t)idx * G::PW;
  Aff<typename G::F> a;
  a.x = Io<typename G::F>::ld(p);
  a.y = Io<typename G::F>::ld(p + G::CW);
  return a;
}
template <class G>
__device__ __forceinline__ Xyzz<typename G::F> ld_xyzz(const uint32_t* p) {
  using F = typename G::F;
  Xyzz<F> r;
  r.x = Io<F>::ld(p);
  r.y = Io<F>::ld(p + G::CW);
  r.zz = Io<F>::ld(p + 2 * G::CW);
  r.zzz = Io<F>::ld(p + 3 * G::CW);
  return r;
}
template <class G>
__device__ __forceinline__ void st_xyzz(uint32_t* p, const Xyzz<typename G::F>& v) {
  using F = typename G::F;
  Io<F>::st(p, v.x);
  Io<F>::st(p + G::CW, v.y);
  Io<F>::st(p + 2 * G::CW, v.zz);
  Io<F>::st(p + 3 * G::CW, v.zzz);
}


// Curve addition of the reductions (piece sums, cascade, bucket reduction).
// (Split-column products for these 1-2 waves/SIMD kernels -- four independent
// accumulators per column -- measured no faster: 2^20 lines kernel 217 -> 195
// us, bit sums 139 -> 143 us; dropped.)
// The lazy-form additions (ec.h xyzz_add_g1/g2) issue ~15-25% fewer VALU
// instructions than the generic xyzz_add.
template <class G>
__device__ __forceinline__ Xyzz<typename G::F> br_add(const Xyzz<typename G::F>& p, const Xyzz<typename G::F>& q) {
  if constexpr (G::CW == 8) return xyzz_add_g1<typename G::P>(p, q);
  else return xyzz_add_g2(p, q);
}

// ----------------------------------------------------------------- digits
__host__ __device__ constexpr int msm_windows(int c) { return (254 + c - 1) / c + ((254 % c) == 0 ? 1 : 0); }

// Window layout of a scalar: W(C) windows.  Uniform (BAL = false): window w
// covers bits [wC, wC + C), the top one only what is left of 254 bits, so its
// digits reach 2^(254 - (W-1)C) buckets at most -- with a full fixed-base
// table that short top window piles a whole copy's n entries onto those few
// buckets (2^20 at c = 20: 2^13 buckets of ~150 entries, split and re-summed
// after the accumulation).  Balanced (BAL, full tables only): the first A
// windows are C bits wide and the rest C - 1, A = 254 - W (C - 1), so every
// copy spreads over 2^(C-2) or 2^(C-1) buckets; the top window (C - 1 bits
// plus the carry) still fits the 2^(C-1) buckets.  (When W (C - 1) >= 254,
// A = 0: every window C - 1 bits, the top one what is left.)  Copy j of the
// table is 2^(offset of window j) P_i (bases_precompute).
template <int C, bool BAL>
struct WinLayout {
  static constexpr int W = msm_windows(C);
  static constexpr int A = BAL ? (254 - W * (C - 1) > 0 ? 254 - W * (C - 1) : 0) : W;  // windows of width C
  static_assert(A >= 0 && A <= W && (!BAL || A < W), "balanced layout");
  static constexpr int width(int w) { return w < A ? C : C - 1; }
  static constexpr int offset(int w) { return w <= A ? w * C : A * C + (w - A) * (C - 1); }
};

template <int C, bool BAL = false>
__device__ __forceinline__ void scalar_digits(const uint32_t* __restrict__ scalars, size_t i, int32_t* d) {
  uint4 a = reinterpret_cast<const uint4*>(scalars)[2 * i];
  uint4 b = reinterpret_cast<const uint4*>(scalars)[2 * i + 1];
  // mask to 254 bits: keeps every digit inside its window's bucket range even
  // for a non-canonical input (documented: scalars must be < r)
  uint32_t s[9] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w & 0x3FFFFFFFu, 0};
  using L = WinLayout<C, BAL>;
  constexpr int W = L::W;
  uint32_t carry = 0;
#pragma unroll
  for (int w = 0; w < W; w++) {
      const int bit = L::offset(w), wi = bit >> 5, sh = bit & 31, wd = L::width(w);
    const uint32_t half = 1u << (wd - 1);
    uint64_t v64 = (((uint64_t)s[wi + 1 < 9 ? wi + 1 : 8]) << 32) | s[wi < 9 ? wi : 8];
    uint32_t v = (uint32_t)(v64 >> sh) & ((1u << wd) - 1);
    v += carry;
    if (w < W - 1 && v > half) {
      d[w] = (int32_t)v - (int32_t)(1u << wd);
      carry = 1;
    } else {
      d[w] = (int32_t)v;
      carry = 0;
    }
  }
}

// Signed digits of every scalar, once per MSM (int32, 0 = nothing to add).
// Window w = j*Wp + w' of the plain recoding is digit w' of table copy j:
// digits[(w' * p + j) * n + i], so the sort sees Wp windows of p*n entries
// (p = 1, Wp = W without a table).  Digits depend on the scalars only (bases
// at infinity are skipped in the accumulation), so MSMs with the same
// scalars over different base sets share one sort (msm_submit_shared).
// blockIdx.y is the scalar vector (batched MSMs, msm_batch_submit; a single
// MSM is a grid of one row): it reads the vector at scalars + y * sstride words
// and writes its Wp * p * n digits after those of the vectors before it, so the
// sort sees nb * Wp windows (the vector index is an outer window).
template <int C, bool BAL>
__global__ void __launch_bounds__(256) k_msm_digits(const uint32_t* __restrict__ scalars, size_t n, int p, int Wp,
                                                    int32_t* __restrict__ digits, size_t sstride) {
  ZK_TAIL_WAVE();
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  scalars += (size_t)blockIdx.y * sstride;
  digits += (size_t)blockIdx.y * (size_t)Wp * p * n;
  constexpr int W = msm_windows(C);
  int32_t d[W];
  scalar_digits<C, BAL>(scalars, i, d);
#pragma unroll
  for (int w = 0; w < W; w++) {
    int j = w / Wp, wq = w - j * Wp;
    digits[((size_t)wq * p + j) * n + i] = d[w];
  }
  for (int w = W; w < p * Wp; w++) {
    int j = w / Wp, wq = w - j * Wp;
    digits[((size_t)wq * p + j) * n + i] = 0;
  }
}

// Bucket sort of the (window, bucket) keys: two-pass MSD radix sort.
//   key = w * B + |digit| - 1  (K = W * B <= 2^21 keys), value = i | sign<<31
//   P1: hi = key >> 8 (NH <= 8192 bins).  Workgroup = chunk of C1 digits; LDS
//       histogram -> count matrix [hi][chunk] -> one device-wide scan gives
//       every (bin, chunk) its output offset; the scatter ranks with LDS
//       atomics on those offsets, so each chunk writes runs of C1/NH entries.
//   P2: lo = key & 255 inside every hi bin.  Tiles of <= C2 entries never
//       cross a bin; count matrix laid out [hi][lo][tile] so the scan yields
//       final positions and the bucket starts directly.
// Only zero digits are dropped; order inside a bucket is irrelevant (group
// addition is exact), so neither pass needs to be stable.
constexpr int RS_THREADS = 256;

// e / ne without a 64-bit integer division (~100 VALU instructions): a
// double-precision estimate (off by at most one for e < 2^52) and a fix-up.
__device__ __forceinline__ void rs_divmod(uint64_t e, uint32_t ne, double inv_ne, uint32_t& w, uint32_t& i) {
  uint64_t q = (uint64_t)((double)e * inv_ne);
  int64_t r = (int64_t)(e - q * ne);
  if (r < 0) {
    q--;
    r += ne;
  } else if (r >= (int64_t)ne) {
    q++;
    r -= ne;
  }
  w = (uint32_t)q;
  i = (uint32_t)r;
}

__device__ __forceinline__ bool rs_key(const int32_t* __restrict__ digits, uint64_t e, uint32_t ne, uint32_t B,
                                       uint32_t& key, uint32_t& val) {
  int32_t d = digits[e];
  if (d == 0) return false;
  uint32_t w, i;
  rs_divmod(e, ne, 1.0 / (double)ne, w, i);
  key = w * B + (uint32_t)(d < 0 ? -d : d) - 1;
  val = i | (d < 0 ? 0x80000000u : 0u);
  return true;
}

__global__ void __launch_bounds__(RS_THREADS) k_rs_p1_count(const int32_t* __restrict__ digits, uint64_t M, uint32_t ne,
                                                            uint32_t B, uint32_t NH, uint32_t lob, uint32_t C1,
                                                            uint32_t nc1, uint32_t* __restrict__ cnt1) {
  ZK_TAIL_WAVE();
  extern __shared__ uint32_t hist[];
  for (uint32_t x = threadIdx.x; x < NH; x += RS_THREADS) hist[x] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * C1;
  const double inv_ne = 1.0 / (double)ne;
  constexpr int U = 8;  // loads in flight per thread
  for (uint32_t k0 = 0; k0 < C1; k0 += U * RS_THREADS) {
    int32_t d[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      uint64_t e = base + k0 + u * RS_THREADS + threadIdx.x;
      d[u] = (k0 + u * RS_THREADS + threadIdx.x < C1 && e < M) ? digits[e] : 0;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      if (d[u] == 0) continue;
      uint32_t w, i;
      rs_divmod(base + k0 + u * RS_THREADS + threadIdx.x, ne, inv_ne, w, i);
      atomicAdd(&hist[(w * B + (uint32_t)(d[u] < 0 ? -d[u] : d[u]) - 1) >> lob], 1u);
    }
  }
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < NH; x += RS_THREADS) cnt1[(size_t)x * nc1 + blockIdx.x] = hist[x];
}


// Exclusive scan of the bin counts hist[0..nb) into lstart, in a
// thread-strided bin order: thread t owns bins t, t + 256, ...  Any bin order
// works (each bin's entries only need to be contiguous in the LDS tile), and
// this one keeps the LDS accesses conflict-free.  Wave scans by shuffles, one
// barrier to combine the 4 waves.  tmp has RS_THREADS / 64 words.
template <int T = RS_THREADS>
__device__ __forceinline__ uint32_t rs_block_scan(const uint32_t* hist, uint32_t* lstart, uint32_t nb, uint32_t* tmp) {
  uint32_t sum = 0;
  for (uint32_t x = threadIdx.x; x < nb; x += T) sum += hist[x];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t inc = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += t;
  }
  if (lane == 63) tmp[wid] = inc;
  __syncthreads();
  uint32_t run = inc - sum, total = 0;
#pragma unroll
  for (int w = 0; w < T / 64; w++) {
    const uint32_t tw = tmp[w];
    if ((uint32_t)w < wid) run += tw;
    total += tw;
  }
  for (uint32_t x = threadIdx.x; x < nb; x += T) {
    lstart[x] = run;
    run += hist[x];
  }
  return total;
}

// Scatter through LDS: each sub-tile of RS_ST entries is first ordered by bin
// in LDS (rank = LDS atomic, bin starts = block scan), then written out so
// that consecutive lanes store consecutive addresses of one bin's run.
// Without this the stores of a wave hit 64 different lines and partially
// written lines get evicted (measured: ~10x slower than the reads).
// LDS layout: hist[nb] | lstart[nb] | gbase[nb] | tmp[4] | skey[RS_ST] | sval[RS_ST]
// Four barriers per sub-tile; hist is zeroed by the caller's first barrier.
template <int PER, class Fill, class Bin, bool WRITE_KEY, int T = RS_THREADS, class KT = uint32_t>
__device__ __forceinline__ void rs_scatter_core(uint32_t nsub, uint32_t nb, uint32_t* lds, Fill fill, Bin bin,
                                                 KT* __restrict__ okey, uint32_t* __restrict__ oval) {
  uint32_t* hist = lds;
  uint32_t* lstart = lds + nb;
  uint32_t* gbase = lds + 2 * nb;
  uint32_t* tmp = lds + 3 * nb;
  uint32_t* skey = tmp + T;
  uint32_t* sval = skey + PER * T;
  for (uint32_t x = threadIdx.x; x < nb; x += T) hist[x] = 0;
  __syncthreads();
  for (uint32_t sub = 0; sub < nsub; sub++) {
    uint32_t key[PER], val[PER], rk[PER];
    bool ok[PER];
    fill(sub, key, val, ok);
#pragma unroll
    for (int k = 0; k < PER; k++)
      if (ok[k]) rk[k] = atomicAdd(&hist[bin(key[k])], 1u);
    __syncthreads();
    const uint32_t total = rs_block_scan<T>(hist, lstart, nb, tmp);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PER; k++) {
      if (ok[k]) {
        uint32_t lp = lstart[bin(key[k])] + rk[k];
        skey[lp] = key[k];
        sval[lp] = val[k];
      }
    }
    __syncthreads();
    for (uint32_t q = threadIdx.x; q < total; q += T) {
      uint32_t kk = skey[q], bn = bin(kk);
      uint32_t g = gbase[bn] + (q - lstart[bn]);
      if (WRITE_KEY) okey[g] = (KT)kk;
      oval[g] = sval[q];
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < nb; x += T) {
      gbase[x] += hist[x];
      hist[x] = 0;
    }
    __syncthreads();
  }
}

// entries e in [0, count) from load(e, key, val), RS_ST per sub-tile
template <int RS_ST, class Load, class Bin, bool WRITE_KEY, int T = RS_THREADS>
__device__ __forceinline__ void rs_scatter_tiles(uint32_t count, uint32_t nb, uint32_t* lds, Load load, Bin bin,
                                                 uint32_t* __restrict__ okey, uint32_t* __restrict__ oval) {
  constexpr int PER = RS_ST / T;
  auto fill = [&](uint32_t sub, uint32_t* key, uint32_t* val, bool* ok) {
#pragma unroll
    for (int k = 0; k < PER; k++) {
      const uint32_t e = sub * RS_ST + k * T + threadIdx.x;
      ok[k] = e < count && load(e, key[k], val[k]);
    }
  };
  rs_scatter_core<PER, decltype(fill), Bin, WRITE_KEY, T>((count + RS_ST - 1) / RS_ST, nb, lds, fill, bin, okey, oval);
}

// entries per LDS sub-tile: 4096 or 8192 (longer runs per bin, fewer resident workgroups)
__host__ __device__ constexpr size_t rs_scatter_lds(uint32_t nb, uint32_t st, uint32_t t = RS_THREADS) {
  return (3 * (size_t)nb + t + 2 * st) * 4;
}

template <int RS_ST>
__global__ void __launch_bounds__(RS_THREADS) k_rs_p1_scatter(const int32_t* __restrict__ digits, uint64_t M,
                                                              uint32_t ne, uint32_t B, uint32_t NH, uint32_t lob,
                                                              uint32_t C1, uint32_t nc1, const uint32_t* __restrict__ offs1,
                                                              uint32_t* __restrict__ okey, uint32_t* __restrict__ oval) {
  ZK_TAIL_WAVE();
  extern __shared__ uint32_t lds[];
  for (uint32_t x = threadIdx.x; x < NH; x += RS_THREADS) lds[2 * NH + x] = offs1[(size_t)x * nc1 + blockIdx.x];
  const uint64_t base = (uint64_t)blockIdx.x * C1;
  const uint32_t count = (uint32_t)std::min<uint64_t>(C1, M - base);
  auto load = [&](uint32_t e, uint32_t& key, uint32_t& val) { return rs_key(digits, base + e, ne, B, key, val); };
  auto bin = [lob](uint32_t key) { return key >> lob; };
  rs_scatter_tiles<RS_ST, decltype(load), decltype(bin), true>(count, NH, lds, load, bin, okey, oval);
}

// P1 straight from the scalars (windows c >= 12, W <= 22): one thread takes
// one scalar and its W signed digits, i.e. entries (w' * p + j) * n + i of the
// digit layout of k_msm_digits (key w' * B + |d| - 1, value (j * n + i) | sign);
// a P1 chunk is CS scalars.  No digits array: its write and two reads go
// (2^26 table MSM: 3.2 GB written + 6.4 GB read).
template <int C, bool BAL>
// wsel (window-sharded MSMs, plain plans): windows [w0, w0 + wn) only, keyed
// from window w0 on (wsel = w0 | wn << 16; 0 = every window)
// kbase: the key of the scalar vector's window 0 (vector index * Wp * B: the
// vector is an outer window; 0 for a single MSM)
__device__ __forceinline__ void rs_scalar_keys(const uint32_t* __restrict__ scalars, size_t i, size_t n, int Wp,
                                               uint32_t B, uint32_t* key, uint32_t* val, bool* ok, uint32_t wsel,
                                               uint32_t kbase) {
  constexpr int W = msm_windows(C);
  int32_t d[W];
  scalar_digits<C, BAL>(scalars, i, d);
  const uint32_t w0 = wsel & 0xFFFFu, wn = wsel >> 16;
  uint32_t j = 0, wq = 0;
#pragma unroll
  for (int w = 0; w < W; w++) {
    const int32_t v = d[w];
    const uint32_t wr = (uint32_t)w - w0;
    ok[w] = v != 0 && (wn == 0 || wr < wn);
    key[w] = kbase + (wn ? wr : wq) * B + (uint32_t)(v < 0 ? -v : v) - 1;
    val[w] = (uint32_t)(j * n + i) | (v < 0 ? 0x80000000u : 0u);
    if (++wq == (uint32_t)Wp) {
      wq = 0;
      j++;
    }
  }
}

// Small sorts (<= SMALL_SORT_MAX entries: the small proofs' MSMs, ~10^5
// entries over a few thousand buckets) are latency-bound: the two-pass radix
// sort's ~11 launches cost ~180 us per MSM there.  Counting sort with global
// atomics instead, in 3 launches: per-bucket counts (a thread per scalar and
// its W digits), one workgroup's exclusive scan (bucket starts + a cursor
// copy), and the scatter, whose positions come from atomics on the cursors.
// Order inside a bucket is then arbitrary, as everywhere (group addition is
// exact).  Contention stays low: ~30 entries per bucket.
constexpr size_t SMALL_SORT_MAX = (size_t)1 << 18;
// blockIdx.y is the scalar vector (one row for a single MSM): its scalars
// start sstride words further per vector and its keys Wp * B further (the
// vector is an outer window); values are unchanged (every vector gathers the
// same table rows).
template <int C, bool BAL>
__global__ void __launch_bounds__(256) k_ss_count(const uint32_t* __restrict__ scalars, size_t n, int Wp, uint32_t B,
                                                  uint32_t wsel, uint32_t* __restrict__ cnt, size_t sstride) {
  ZK_TAIL_WAVE();
  constexpr int W = msm_windows(C);
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t key[W], val[W];
  bool ok[W];
  scalars += (size_t)blockIdx.y * sstride;
  rs_scalar_keys<C, BAL>(scalars, i, n, Wp, B, key, val, ok, wsel, blockIdx.y * (uint32_t)Wp * B);
#pragma unroll
  for (int w = 0; w < W; w++)
    if (ok[w]) atomicAdd(&cnt[key[w]], 1u);
}
// one 1024-thread workgroup: bstart[k] = sum of cnt[< k], bstart[K] = total,
// cursor = a copy of bstart[0..K)
__global__ void __launch_bounds__(1024) k_ss_scan(uint32_t* __restrict__ cnt, uint32_t K,
                                                  uint32_t* __restrict__ bstart, uint32_t* __restrict__ cursor) {
  ZK_TAIL_WAVE();
  __shared__ uint32_t wsum[16];
  const uint32_t per = (K + 1023) / 1024, k0 = threadIdx.x * per, k1 = min(K, k0 + per);
  uint32_t sum = 0;
  for (uint32_t k = k0; k < k1; k++) sum += cnt[k];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t inc = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += t;
  }
  if (lane == 63) wsum[wid] = inc;
  __syncthreads();
  uint32_t run = inc - sum, total = 0;
#pragma unroll
  for (int w = 0; w < 16; w++) {
    const uint32_t tw = wsum[w];
    if ((uint32_t)w < wid) run += tw;
    total += tw;
  }
  for (uint32_t k = k0; k < k1; k++) {
    bstart[k] = run;
    cursor[k] = run;
    run += cnt[k];
    cnt[k] = 0;  // clean for the lane's next counting sort (no memset launch)
  }
  if (threadIdx.x == 0) bstart[K] = total;
}
template <int C, bool BAL>
__global__ void __launch_bounds__(256) k_ss_scatter(const uint32_t* __restrict__ scalars, size_t n, int Wp,
                                                    uint32_t B, uint32_t wsel, uint32_t* __restrict__ cursor,
                                                    uint32_t* __restrict__ sval, size_t sstride) {
  ZK_TAIL_WAVE();
  constexpr int W = msm_windows(C);
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t key[W], val[W];
  bool ok[W];
  scalars += (size_t)blockIdx.y * sstride;
  rs_scalar_keys<C, BAL>(scalars, i, n, Wp, B, key, val, ok, wsel, blockIdx.y * (uint32_t)Wp * B);
#pragma unroll
  for (int w = 0; w < W; w++)
    if (ok[w]) sval[atomicAdd(&cursor[key[w]], 1u)] = val[w];
}

// one workgroup: bin starts and tile starts (tiles of <= C2 entries per bin)
__global__ void __launch_bounds__(1024) k_rs_tiles(const uint32_t* __restrict__ offs1, uint32_t nc1, uint32_t NH,
                                                   const uint32_t* __restrict__ total, uint32_t C2,
                                                   uint32_t* __restrict__ binstart, uint32_t* __restrict__ tstart) {
  ZK_TAIL_WAVE();
  __shared__ uint32_t sh[1024];
  const uint32_t tot = *total;
  uint32_t carry = 0;
  for (uint32_t base = 0; base < NH; base += 1024) {
    uint32_t h = base + threadIdx.x;
    uint32_t nt = 0;
    if (h < NH) {
      uint32_t lo = offs1[(size_t)h * nc1], hi = h + 1 < NH ? offs1[(size_t)(h + 1) * nc1] : tot;
      binstart[h] = lo;
      nt = (hi - lo + C2 - 1) / C2;
    }
    sh[threadIdx.x] = nt;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      uint32_t t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (h < NH) tstart[h] = carry + sh[threadIdx.x] - nt;
    uint32_t blk = sh[1023];
    __syncthreads();
    carry += blk;
  }
  if (threadIdx.x == 0) {
    binstart[NH] = tot;
    tstart[NH] = carry;
  }
}

// tile t -> its bin h (largest h with tstart[h] <= t; bins without tiles skipped)
__device__ __forceinline__ uint32_t rs_tile_bin(const uint32_t* __restrict__ tstart, uint32_t NH, uint32_t t) {
  uint32_t lo = 0, hi = NH;  // tstart[lo] <= t < tstart[hi]
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (tstart[mid] <= t) lo = mid;
    else hi = mid;
  }
  return lo;
}

// P2 tiles of one hi bin run on one XCD (workgroup i lands on XCD i % 8): the
// bin's output range then stays in that XCD's L2 while its tiles scatter
// short runs into it.  Tile of workgroup g: (g % 8) * per + g / 8.
__device__ __forceinline__ uint32_t rs_xcd_tile(uint32_t g, uint32_t T2max) {
  const uint32_t per = (T2max + 7) / 8;
  return (g & 7) * per + (g >> 3);
}

__global__ void __launch_bounds__(RS_THREADS) k_rs_p2_count(const uint32_t* __restrict__ okey,
                                                            const uint32_t* __restrict__ binstart,
                                                            const uint32_t* __restrict__ tstart, uint32_t NH,
                                                            uint32_t lob, uint32_t C2, uint32_t T2max,
                                                            uint32_t* __restrict__ cnt2) {
  ZK_TAIL_WAVE();
  extern __shared__ uint32_t hist[];
  const uint32_t NLO = 1u << lob, mask = NLO - 1;
  const uint32_t t = rs_xcd_tile(blockIdx.x, T2max);
  if (t >= tstart[NH]) return;
  const uint32_t h = rs_tile_bin(tstart, NH, t), q = t - tstart[h], nt = tstart[h + 1] - tstart[h];
  const uint32_t lo = binstart[h] + q * C2, hi = min(lo + C2, binstart[h + 1]);
  for (uint32_t x = threadIdx.x; x < NLO; x += RS_THREADS) hist[x] = 0;
  __syncthreads();
  constexpr int U = 8;  // loads in flight per thread
  for (uint32_t p0 = lo; p0 < hi; p0 += U * RS_THREADS) {
    uint32_t kk[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t p = p0 + u * RS_THREADS + threadIdx.x;
      kk[u] = p < hi ? okey[p] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      if (kk[u] != 0xFFFFFFFFu) atomicAdd(&hist[kk[u] & mask], 1u);
  }
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < NLO; x += RS_THREADS)
    cnt2[((size_t)tstart[h] << lob) + (size_t)x * nt + q] = hist[x];
}

template <int RS_ST, int T = RS_THREADS>
__global__ void __launch_bounds__(T) k_rs_p2_scatter(const uint32_t* __restrict__ okey,
                                                              const uint32_t* __restrict__ oval,
                                                              const uint32_t* __restrict__ binstart,
                                                              const uint32_t* __restrict__ tstart, uint32_t NH,
                                                              uint32_t lob, uint32_t C2, uint32_t T2max,
                                                              const uint32_t* __restrict__ offs2,
                                                              uint32_t* __restrict__ sval) {
  ZK_TAIL_WAVE();
  extern __shared__ uint32_t lds[];
  const uint32_t NLO = 1u << lob, mask = NLO - 1;
  const uint32_t t = rs_xcd_tile(blockIdx.x, T2max);
  if (t >= tstart[NH]) return;
  const uint32_t h = rs_tile_bin(tstart, NH, t), q = t - tstart[h], nt = tstart[h + 1] - tstart[h];
  const uint32_t lo = binstart[h] + q * C2, hi = min(lo + C2, binstart[h + 1]);
  for (uint32_t x = threadIdx.x; x < NLO; x += T)
    lds[2 * NLO + x] = offs2[((size_t)tstart[h] << lob) + (size_t)x * nt + q];
  auto load = [&](uint32_t e, uint32_t& key, uint32_t& val) {
    key = okey[lo + e];
    val = oval[lo + e];
    return true;
  };
  auto bin = [mask](uint32_t key) { return key & mask; };
  rs_scatter_tiles<RS_ST, decltype(load), decltype(bin), false, T>(hi - lo, NLO, lds, load, bin, nullptr, sval);
}

// bucket starts: start of key k = scanned count at (hi, lo, tile 0)
__global__ void __launch_bounds__(256) k_rs_bstart(const uint32_t* __restrict__ offs2,
                                                   const uint32_t* __restrict__ binstart,
                                                   const uint32_t* __restrict__ tstart, uint32_t NH, uint32_t lob,
                                                   uint32_t K, uint32_t* __restrict__ bstart) {
  ZK_TAIL_WAVE();
  uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k > K) return;
  if (k == K) {
    bstart[K] = binstart[NH];
    return;
  }
  uint32_t h = k >> lob, lo = k & ((1u << lob) - 1), nt = tstart[h + 1] - tstart[h];
  bstart[k] = nt ? offs2[((size_t)tstart[h] << lob) + (size_t)lo * nt] : binstart[h];
}

// ------------------------------------------------------------- bin sort
// The sort of every MSM with windows c >= 12 (fused digits): four kernels,
// no device-wide scan, every workgroup 256 threads (one wave per SIMD, so it
// fits beside the accumulation waves of another lane):
//   A k_bs_count    chunk of CS scalars -> LDS histogram of the hi bins (key
//                   >> lob); per (chunk, bin) one atomicAdd on the bin total
//                   and one returning atomicAdd on the (super-chunk, bin)
//                   total, which IS the chunk's offset inside that super-chunk
//                   of the bin (a super-chunk = 1/32 of the scalars).
//   B k_bs_scatter1 the chunk's entries into their bins at binstart (block
//                   prefix of the bin totals) + the earlier super-chunks of
//                   the bin + that offset, LDS-staged runs (rs_scatter_core).
//   C k_bs_count2   tiles of <= C2 entries inside one bin -> LDS histogram of
//                   the lo keys, stored per tile.
//   D k_bs_scatter2 each tile sums its bin's tile histograms (bucket sizes,
//                   and its own offset inside every bucket: the earlier tiles'
//                   counts), prefixes the sizes (bucket starts), scatters;
//                   tile 0 of a bin writes the bin's bstart and, for
//                   one-lane-per-bucket plans, the bin's accumulation items.
// Entries of a bucket therefore stay in scalar order up to 1/32 of the range
// (random only inside a super-chunk).  That order is what the accumulation
// gathers by: at step p every lane of a wave (equal bucket lengths) reads a
// table row of about the same scalar index, so the wave's 64 gathers share a
// few pages per table copy.  (Measured, round 5: with chunk offsets in atomic
// arrival order -- random inside every bucket -- the 2^20 accumulation issued
// 2.6% more VALU instructions but ran 25% longer, 1045 vs 867 us one lane;
// VALU issue 0.75 vs 0.91.)
// Counters: one memset of the bin / super-chunk totals and item counters at
// the sort's start.
// (Replaces the two-pass radix sort's three-launch scans, its tiles / bstart
// kernels and the four-launch item plan: in the r04 3-lane trace the P2 scan
// of a 3.9M-entry [bin][lo][tile] count matrix alone sat ~150 us on the
// critical path between two accumulations.)
constexpr uint32_t BS_NSC = 32;  // super-chunks
// ZK_BS_KEY16: the first scatter writes only the low 16 bits of each key (the
// bin is implied by the position; the second pass needs the low lob <= 11
// bits), so okey is read and written at 2 B per entry instead of 4
// (measured, round 6: 2^26 MSM 63.24-63.30 -> 62.67-62.70 ms, 2^20 2-lane
// loop 916.7-917.9 -> 917.6-920.7 Mpt/s, one box)
#ifndef ZK_BS_KEY16
#define ZK_BS_KEY16 1
#endif
using BsKey = std::conditional_t<ZK_BS_KEY16 != 0, uint16_t, uint32_t>;

// exclusive prefix, in index order, of get(0..nb) into out[0..nb) (LDS) by T
// threads; returns the total.  tmp: T/64 words of LDS.  Ends with a barrier.
template <int T, class Get>
__device__ __forceinline__ uint32_t block_prefix(uint32_t nb, Get get, uint32_t* out, uint32_t* tmp) {
  const uint32_t per = (nb + T - 1) / T, k0 = min(nb, threadIdx.x * per), k1 = min(nb, k0 + per);
  uint32_t sum = 0;
  for (uint32_t k = k0; k < k1; k++) sum += get(k);
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t inc = sum;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t t = __shfl_up(inc, off, 64);
    if (lane >= (unsigned)off) inc += t;
  }
  if (lane == 63) tmp[wid] = inc;
  __syncthreads();
  uint32_t run = inc - sum, total = 0;
#pragma unroll
  for (int w = 0; w < T / 64; w++) {
    const uint32_t tw = tmp[w];
    if ((uint32_t)w < wid) run += tw;
    total += tw;
  }
  for (uint32_t k = k0; k < k1; k++) {
    const uint32_t v = get(k);
    out[k] = run;
    run += v;
  }
  __syncthreads();
  return total;
}

// Grid (chunks per scalar vector, vectors): workgroup (x, y) is chunk x of
// vector y (one row for a single MSM); it reads that vector (sstride words per
// vector) and bases its keys at y * Wp * B.  Chunk offsets, super-chunks and
// the clearing of next_ctr go by the flat chunk index y * gridDim.x + x.
template <int C, bool BAL>
__global__ void __launch_bounds__(256) k_bs_count(const uint32_t* __restrict__ scalars, size_t n, int Wp, uint32_t B,
                                                  uint32_t wsel, uint32_t NH, uint32_t lob, uint32_t CS, uint32_t scs,
                                                  uint32_t* __restrict__ bintot, uint32_t* __restrict__ sctot,
                                                  uint32_t* __restrict__ choff, uint32_t* __restrict__ next_ctr,
                                                  uint32_t ctr_words, size_t sstride) {
  ZK_TAIL_WAVE();
  extern __shared__ uint32_t hist[];
  constexpr int W = msm_windows(C);
  const uint32_t chunk = blockIdx.y * gridDim.x + blockIdx.x;
  // the lane's other counter block, for its next sort
  for (size_t i = (size_t)chunk * 256 + threadIdx.x; i < ctr_words; i += (size_t)gridDim.x * gridDim.y * 256)
    next_ctr[i] = 0;
  for (uint32_t x = threadIdx.x; x < NH; x += 256) hist[x] = 0;
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * CS;
  const uint32_t kbase = blockIdx.y * (uint32_t)Wp * B;
  scalars += (size_t)blockIdx.y * sstride;
  for (uint32_t k = threadIdx.x; k < CS && base + k < n; k += 256) {
    uint32_t key[W], val[W];
    bool ok[W];
    rs_scalar_keys<C, BAL>(scalars, base + k, n, Wp, B, key, val, ok, wsel, kbase);
#pragma unroll
    for (int w = 0; w < W; w++)
      if (ok[w]) atomicAdd(&hist[key[w] >> lob], 1u);
  }
  __syncthreads();
  uint32_t* sc = sctot + (size_t)(chunk >> scs) * NH;
  for (uint32_t x = threadIdx.x; x < NH; x += 256) {
    const uint32_t hx = hist[x];
    uint32_t off = 0;
    if (hx) {
      off = atomicAdd(&sc[x], hx);
      atomicAdd(&bintot[x], hx);
    }
    choff[(size_t)chunk * NH + x] = off;
  }
}

// T threads, sub-tiles of T scalars (T * W entries); the grid of k_bs_count
template <int C, int T, bool BAL>
__global__ void __launch_bounds__(T) k_bs_scatter1(const uint32_t* __restrict__ scalars, size_t n, int Wp, uint32_t B,
                                                   uint32_t wsel, uint32_t NH, uint32_t lob, uint32_t CS, uint32_t scs,
                                                   const uint32_t* __restrict__ bintot,
                                                   const uint32_t* __restrict__ sctot,
                                                   const uint32_t* __restrict__ choff, BsKey* __restrict__ okey,
                                                   uint32_t* __restrict__ oval, size_t sstride) {
  ZK_TAIL_WAVE();
  extern __shared__ uint32_t lds[];
  constexpr int W = msm_windows(C);
  uint32_t* gbase = lds + 2 * NH;
  block_prefix<T>(NH, [&](uint32_t k) { return bintot[k]; }, gbase, lds + 3 * NH);
  const uint32_t chunk = blockIdx.y * gridDim.x + blockIdx.x;
  const uint32_t s0 = chunk >> scs;  // this chunk's super-chunk: the earlier ones come first in every bin
  for (uint32_t x = threadIdx.x; x < NH; x += T) {
    uint32_t g = gbase[x] + choff[(size_t)chunk * NH + x];
    for (uint32_t q = 0; q < s0; q++) g += sctot[(size_t)q * NH + x];
    gbase[x] = g;
  }
  const size_t base = (size_t)blockIdx.x * CS;
  const uint32_t cnt = (uint32_t)std::min<size_t>(CS, n - base);
  const uint32_t kbase = blockIdx.y * (uint32_t)Wp * B;
  scalars += (size_t)blockIdx.y * sstride;
  auto fill = [&](uint32_t sub, uint32_t* key, uint32_t* val, bool* ok) {
    const uint32_t k = sub * T + threadIdx.x;
    if (k < cnt) {
      rs_scalar_keys<C, BAL>(scalars, base + k, n, Wp, B, key, val, ok, wsel, kbase);
    } else {
#pragma unroll
      for (int w = 0; w < W; w++) ok[w] = false;
    }
  };
  auto bin = [lob](uint32_t key) { return key >> lob; };
  rs_scatter_core<W, decltype(fill), decltype(bin), true, T>((cnt + T - 1) / T, NH, lds, fill, bin, okey, oval);
}

// Tile geometry of C / D, recomputed by every workgroup from the bin totals:
// pre[0..NH] bin starts, tst[0..NH] tile starts (every bin has >= 1 tile, so
// tile 0 of every bin exists to write its bstart).  Returns the total tiles.
__device__ __forceinline__ uint32_t bs_tiles(const uint32_t* __restrict__ bintot, uint32_t NH, uint32_t C2,
                                             uint32_t* pre, uint32_t* tst, uint32_t* tmp) {
  const uint32_t M = block_prefix<256>(NH, [&](uint32_t k) { return bintot[k]; }, pre, tmp);
  const uint32_t TT = block_prefix<256>(
      NH, [&](uint32_t k) { return max(1u, (bintot[k] + C2 - 1) / C2); }, tst, tmp);
  if (threadIdx.x == 0) {
    pre[NH] = M;
    tst[NH] = TT;
  }
  __syncthreads();
  return TT;
}

__global__ void __launch_bounds__(256) k_bs_count2(const BsKey* __restrict__ okey,
                                                   const uint32_t* __restrict__ bintot, uint32_t NH, uint32_t lob,
                                                   uint32_t C2, uint32_t T2max, uint32_t* __restrict__ thist) {
  ZK_TAIL_WAVE();
  extern __shared__ uint32_t lds[];
  const uint32_t NLO = 1u << lob, mask = NLO - 1;
  uint32_t* hist = lds;
  uint32_t* pre = lds + NLO;
  uint32_t* tst = pre + NH + 1;
  uint32_t* tmp = tst + NH + 1;
  const uint32_t t = rs_xcd_tile(blockIdx.x, T2max);
  if (t >= T2max) return;  // beyond any tile count (block-uniform)
  const uint32_t TT = bs_tiles(bintot, NH, C2, pre, tst, tmp);
  if (t >= TT) return;
  const uint32_t h = rs_tile_bin(tst, NH, t), q = t - tst[h];
  const uint32_t lo = pre[h] + q * C2, hi = min(lo + C2, pre[h + 1]);
  for (uint32_t x = threadIdx.x; x < NLO; x += 256) hist[x] = 0;
  __syncthreads();
  constexpr int U = 8;  // loads in flight per thread
  for (uint32_t p0 = lo; p0 < hi; p0 += U * 256) {
    uint32_t kk[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const uint32_t p = p0 + u * 256 + threadIdx.x;
      kk[u] = p < hi ? okey[p] : 0xFFFFFFFFu;
    }
#pragma unroll
    for (int u = 0; u < U; u++)
      if (kk[u] != 0xFFFFFFFFu) atomicAdd(&hist[kk[u] & mask], 1u);
  }
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < NLO; x += 256) thist[(size_t)t * NLO + x] = hist[x];
}

// Accumulation items of one-lane-per-bucket plans (k_acc_items_*): tile 0 of
// every bin ranks the bin's buckets by length (pieces capped at `cap`),
// longest first, stages them per bin and adds the bin's class counts to the
// global class histogram; k_items_place then lays the items out class-major
// over all bins (each bin's run of a class contiguous), as round 4's item plan
// did.  Waves then hold buckets of one length, and the items run longest
// first.  That global class order is what the accumulation's speed rests on:
// measured (round 5, one lane, the same sort), the accumulation took 906 us
// with it, 1086 us with the items ranked inside each bin and the bins
// interleaved wave by wave (ranks 64r..64r+63 of bin h per wave), and ~1045-
// 1150 us with one rank of 64 bins per wave -- waves of one class run their
// gathers in step.  A bucket longer than cap keeps its first piece in place;
// pieces 1.. go to the overflow items after the nmain main slots (run first),
// and the bucket to the split list the piece sums read.  A bucket longer than cap keeps its first
// piece in place; pieces 1.. go to the overflow items after the nmain main
// slots (run first), and the bucket to the split list the piece sums read.
// itc: [0] overflow items, [1] partial slots, [2] split buckets.
struct ItemsOut {
  uint4* items;
  uint32_t nmain, cap;
  uint32_t* itc;
  uint4* split;
  uint4* stage;     // [NH][NLO]: a bin's items by class, longest first (k_items_place reads them)
  uint32_t* ghist;  // [cap + 1]: buckets per class over all bins
};

template <int ST, bool ITEMS>
__global__ void __launch_bounds__(256) k_bs_scatter2(const BsKey* __restrict__ okey,
                                                     const uint32_t* __restrict__ oval,
                                                     const uint32_t* __restrict__ bintot, uint32_t NH, uint32_t lob,
                                                     uint32_t C2, uint32_t T2max, uint32_t K,
                                                     const uint32_t* __restrict__ thist,
                                                     uint32_t* __restrict__ sval, uint32_t* __restrict__ bstart,
                                                     ItemsOut io) {
  ZK_TAIL_WAVE();
  constexpr int T = 256;
  extern __shared__ uint32_t lds[];
  const uint32_t NLO = 1u << lob, mask = NLO - 1;
  // rs_scatter_core layout first, then the tile geometry
  uint32_t* lstart = lds + NLO;
  uint32_t* gbase = lds + 2 * NLO;
  uint32_t* tmp = lds + 3 * NLO;
  uint32_t* skey = tmp + T;
  uint32_t* pre = skey + 2 * ST;
  uint32_t* tst = pre + NH + 1;
  const uint32_t t = rs_xcd_tile(blockIdx.x, T2max);
  if (t >= T2max) return;
  const uint32_t TT = bs_tiles(bintot, NH, C2, pre, tst, tmp);
  if (t >= TT) return;
  const uint32_t h = rs_tile_bin(tst, NH, t), q = t - tst[h];
  const uint32_t lo = pre[h] + q * C2, hi = min(lo + C2, pre[h + 1]);
  const uint32_t k0 = h * NLO;  // first key of the bin
  // bucket sizes (all tiles of the bin) and this tile's offset inside every
  // bucket (the earlier tiles' counts: entries keep the bin's order)
  uint32_t* ksz = lds;  // the scatter's hist array, free until rs_scatter_core
  {
    const uint32_t t0 = tst[h], nt = tst[h + 1] - t0;
    for (uint32_t x = threadIdx.x; x < NLO; x += T) {
      uint32_t tot = 0, before = 0;
      for (uint32_t qq = 0; qq < nt; qq++) {
        const uint32_t v = thist[(size_t)(t0 + qq) * NLO + x];
        before += qq < q ? v : 0u;
        tot += v;
      }
      ksz[x] = k0 + x < K ? tot : 0u;
      gbase[x] = before;
    }
    __syncthreads();
  }
  auto ksize = [&](uint32_t x) { return ksz[x]; };
  // bucket starts inside the bin
  block_prefix<T>(NLO, ksize, lstart, tmp);
  if (q == 0) {
    for (uint32_t x = threadIdx.x; x < NLO; x += T)
      if (k0 + x < K) bstart[k0 + x] = pre[h] + lstart[x];
    if (h == NH - 1 && threadIdx.x == 0) bstart[K] = pre[NH];
    if constexpr (ITEMS) {
      // rank the bin's buckets by capped length, longest first (LDS counting
      // sort over the classes 0..cap)
      const uint32_t cap = io.cap;
      uint32_t* ch = skey;         // class histogram [cap + 1]
      uint32_t* cstart = skey + ST;  // descending class starts [cap + 1]
      for (uint32_t c = threadIdx.x; c <= cap; c += T) ch[c] = 0;
      __syncthreads();
      constexpr uint32_t PERX = 2048 / T;  // NLO <= 2048
      uint32_t tk[PERX];
#pragma unroll
      for (uint32_t j = 0; j < PERX; j++) {
        const uint32_t x = j * T + threadIdx.x;
        if (x < NLO) tk[j] = atomicAdd(&ch[min(ksize(x), cap)], 1u);
      }
      __syncthreads();
      block_prefix<T>(cap + 1, [&](uint32_t k) { return ch[cap - k]; }, cstart, tmp);
#pragma unroll
      for (uint32_t j = 0; j < PERX; j++) {
        const uint32_t x = j * T + threadIdx.x;
        if (x >= NLO) continue;
        const uint32_t size = ksize(x), cls = min(size, cap);
        const uint32_t rank = cstart[cap - cls] + tk[j];
        const uint32_t start = pre[h] + lstart[x];
        const uint32_t np = (size + cap - 1) / cap;
        uint32_t slot0 = 0xFFFFFFFFu;  // NOSLOT: no partial slot
        if (np > 1) {
          slot0 = atomicAdd(&io.itc[1], np);
          const uint32_t ov = atomicAdd(&io.itc[0], np - 1);
          io.split[atomicAdd(&io.itc[2], 1u)] = make_uint4(k0 + x, slot0, np, 0);
          for (uint32_t pc = 1; pc < np; pc++)
            io.items[io.nmain + ov + pc - 1] =
                make_uint4(start + pc * cap, min(start + (pc + 1) * cap, start + size), k0 + x, slot0 + pc);
        }
        io.stage[(size_t)h * NLO + rank] = make_uint4(start, start + cls, k0 + x, slot0);
      }
      for (uint32_t c = threadIdx.x; c <= cap; c += T)
        if (ch[c]) atomicAdd(&io.ghist[c], ch[c]);
      __syncthreads();
    }
  }
  for (uint32_t x = threadIdx.x; x < NLO; x += T) gbase[x] += pre[h] + lstart[x];
  auto load = [&](uint32_t e, uint32_t& key, uint32_t& val) {
    key = okey[lo + e];
    val = oval[lo + e];
    return true;
  };
  auto bin = [mask](uint32_t key) { return key & mask; };
  rs_scatter_tiles<ST, decltype(load), decltype(bin), false, T>(hi - lo, NLO, lds, load, bin, nullptr, sval);
}

// ----------------------------------------------------------------- scan
// exclusive scan of counts[K] -> offs[K+1]; 1024 elements per block
__global__ void __launch_bounds__(256) k_scan_blocks(const uint32_t* in, uint32_t K, uint32_t* out,
                                                     uint32_t* __restrict__ block_sums) {
  ZK_TAIL_WAVE();
  __shared__ uint32_t sh[256];
  uint32_t base = blockIdx.x * 1024 + threadIdx.x * 4;
  uint32_t v[4], s = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    v[k] = base + k < K ? in[base + k] : 0;
    s += v[k];
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {
    uint32_t t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
    __syncthreads();
    sh[threadIdx.x] += t;
    __syncthreads();
  }
  uint32_t excl = sh[threadIdx.x] - s;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (base + k < K) out[base + k] = excl;
    excl += v[k];
  }
  if (threadIdx.x == 255) block_sums[blockIdx.x] = sh[255];
}
// single block: exclusive scan of block sums in place (any length)
__global__ void __launch_bounds__(1024) k_scan_top(uint32_t* __restrict__ bs, uint32_t nb, uint32_t* __restrict__ total) {
  ZK_TAIL_WAVE();
  __shared__ uint32_t sh[1024];
  uint32_t carry = 0;
  for (uint32_t base = 0; base < nb; base += 1024) {
    uint32_t i = base + threadIdx.x;
    uint32_t v = i < nb ? bs[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      uint32_t t = threadIdx.x >= (unsigned)off ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nb) bs[i] = sh[threadIdx.x] - v + carry;
    uint32_t blk_total = sh[1023];
    __syncthreads();
    carry += blk_total;
  }
  if (threadIdx.x == 0) *total = carry;
}
__global__ void __launch_bounds__(256) k_scan_add(uint32_t* __restrict__ out, uint32_t K,
                                                  const uint32_t* __restrict__ bs, uint32_t* __restrict__ cursor) {
  ZK_TAIL_WAVE();
  uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K) return;
  uint32_t v = out[i] + bs[i / 1024];
  out[i] = v;
  if (cursor) cursor[i] = v;
}

// ------------------------------------------------------- bucket accumulation
// Partial list layout (size 2*nchunks+1): X[2t+1] = head of chunk t (run
// continuing from the left), X[2t+2] = tail (run continuing to the right).
// Invalid slots carry the key of the chunk's first / last entry so the list
// stays sorted; a run made only of invalid slots is never written.
constexpr uint32_t NOKEY = 0xFFFFFFFFu;

// bucket containing sorted position p: largest k with bstart[k] <= p < bstart[k+1]
__device__ __forceinline__ uint32_t bucket_of(const uint32_t* __restrict__ bstart, uint32_t K, uint32_t p) {
  uint32_t lo = 0, hi = K;  // invariant: bstart[lo] <= p < bstart[hi]
  while (hi - lo > 1) {
    uint32_t mid = (lo + hi) >> 1;
    if (bstart[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// A run cut by chunk edges leaves k = t1 - t0 + 1 partials of bucket b: the
// tail slot of chunk t0 and the head slots of chunks t0+1..t1 (t = chunk of
// its first / last entry).  k_msm_cutsum (one thread per bucket) sums and
// invalidates them for k <= ACC_KMAX, so uniform scalars (a few pieces per
// bucket) finish in one shallow pass; heavier buckets keep valid partials for
// the k_msm_accN cascade.  (Kept out of k_msm_acc0: a second inlined curve
// addition there costs a wave of occupancy.)
constexpr uint32_t ACC_KMAX = 12;

template <class G>
__global__ void __launch_bounds__(256) k_msm_cutsum(const uint32_t* __restrict__ bstart, uint32_t K, uint32_t L,
                                                    uint32_t* __restrict__ buckets, uint32_t* __restrict__ xvalid,
                                                    const uint32_t* __restrict__ xpts,
                                                    uint32_t* __restrict__ open_flag) {
  ZK_TAIL_WAVE();
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= K) return;
  const uint32_t lo = bstart[b], hi = bstart[b + 1];
  if (hi - lo < 2) return;
  const uint32_t t0 = lo / L, t1 = (hi - 1) / L;
  if (t0 == t1) return;  // complete inside one chunk: already in buckets[b]
  if (t1 - t0 + 1 > ACC_KMAX) {
    atomicOr(open_flag, 1u);
    return;
  }
  Xyzz<F> sum = ld_xyzz<G>(xpts + (size_t)(2 * t0 + 2) * XW);
  xvalid[2 * t0 + 2] = 0;
  for (uint32_t t = t0 + 1; t <= t1; t++) {
    sum = br_add<G>(sum, ld_xyzz<G>(xpts + (size_t)(2 * t + 1) * XW));
    xvalid[2 * t + 1] = 0;
  }
  st_xyzz<G>(buckets + (size_t)b * XW, sum);
}

// Small MSMs (K <= 2^16 buckets: the proofs of configs[0]) are latency-
// bound: k_msm_cutsum's one thread per bucket adds up to ACC_KMAX - 1 pieces
// in a dependent chain (~10 curve additions, ~130 us for G1 and ~400 us for
// G2 at a 2^13 domain).  Here 16 lanes share a bucket and add its <= 16
// pieces as a butterfly tree over lane shuffles: 4 dependent additions.
// Same group element per bucket (the XYZZ representative may differ; every
// consumer is representation-independent).
__device__ __forceinline__ Fe shfl_xor_fe(const Fe& a, int m) {
  Fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = (uint32_t)__shfl_xor((int)a.v[i], m, 16);
  return r;
}
__device__ __forceinline__ Fe2 shfl_xor_fe(const Fe2& a, int m) { return {shfl_xor_fe(a.c0, m), shfl_xor_fe(a.c1, m)}; }
template <class F>
__device__ __forceinline__ Xyzz<F> shfl_xor_xyzz(const Xyzz<F>& a, int m) {
  Xyzz<F> r;
  r.x = shfl_xor_fe(a.x, m);
  r.y = shfl_xor_fe(a.y, m);
  r.zz = shfl_xor_fe(a.zz, m);
  r.zzz = shfl_xor_fe(a.zzz, m);
  return r;
}
__device__ __forceinline__ Fe shfl_down_fe(const Fe& a, uint32_t d) {
  Fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = (uint32_t)__shfl_down((int)a.v[i], d, 16);
  return r;
}
__device__ __forceinline__ Fe2 shfl_down_fe(const Fe2& a, uint32_t d) {
  return {shfl_down_fe(a.c0, d), shfl_down_fe(a.c1, d)};
}
template <class F>
__device__ __forceinline__ Xyzz<F> shfl_down_xyzz(const Xyzz<F>& a, uint32_t d) {
  Xyzz<F> r;
  r.x = shfl_down_fe(a.x, d);
  r.y = shfl_down_fe(a.y, d);
  r.zz = shfl_down_fe(a.zz, d);
  r.zzz = shfl_down_fe(a.zzz, d);
  return r;
}
constexpr uint32_t CUTSUM_COOP_K = 1u << 16;  // bucket counts up to which the tree form runs
template <class G>
__global__ void __launch_bounds__(256) k_msm_cutsum_coop(const uint32_t* __restrict__ bstart, uint32_t K, uint32_t L,
                                                         uint32_t* __restrict__ buckets,
                                                         uint32_t* __restrict__ xvalid,
                                                         const uint32_t* __restrict__ xpts,
                                                         uint32_t* __restrict__ open_flag,
                                                         uint4* __restrict__ split = nullptr,
                                                         uint32_t* __restrict__ nsplit = nullptr) {
  ZK_TAIL_WAVE();
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  const uint32_t gt = blockIdx.x * 256 + threadIdx.x;
  const uint32_t b = gt >> 4, r = gt & 15;
  // every lane stays to the end: the shuffles need the whole group
  bool live = b < K;
  uint32_t t0 = 0, k = 0;
  if (live) {
    const uint32_t lo = bstart[b], hi = bstart[b + 1];
    live = hi - lo >= 2;
    if (live) {
      t0 = lo / L;
      k = (hi - 1) / L - t0 + 1;
      live = k > 1;  // else complete inside one chunk: already in buckets[b]
    }
  }
  if (live && k > 16) {  // left to the k_msm_accN cascade, or listed for k_split_combine<G, true>
    if (r == 0) {
      atomicOr(open_flag, 1u);
      if (split) split[atomicAdd(nsplit, 1u)] = make_uint4(b, t0, k, 0);
    }
    live = false;
  }
  bool has = live && r < k;
  Xyzz<F> v = xyzz_inf<F>();
  if (has) {
    const uint32_t slot = r == 0 ? 2 * t0 + 2 : 2 * (t0 + r) + 1;  // tail of chunk t0, heads of t0+1..
    v = ld_xyzz<G>(xpts + (size_t)slot * XW);
    xvalid[slot] = 0;
  }
#pragma unroll 1
  for (int m = 1; m < 16; m <<= 1) {
    const Xyzz<F> o = shfl_xor_xyzz(v, m);
    const bool oh = __shfl_xor((int)has, m, 16) != 0;
    if ((r & m) == 0 && oh) v = has ? br_add<G>(v, o) : o;
    has = has || oh;
  }
  if (live && r == 0) st_xyzz<G>(buckets + (size_t)b * XW, v);
}

// accumulator store: G1 keeps X lazily in [0, 8p) inside the loop
template <class G>
__device__ __forceinline__ void st_acc(uint32_t* p, Xyzz<typename G::F> v) {
  if constexpr (G::CW == 8) v.x = reduce8<FqP>(v.x);
  st_xyzz<G>(p, v);
}

template <class G>
__device__ __forceinline__ void msm_acc0_body(const uint32_t* __restrict__ sval, const uint32_t* __restrict__ bstart,
                                                  uint32_t K, uint32_t L, uint32_t nchunks,
                                                  const uint32_t* __restrict__ bases, uint32_t tn, uint32_t tskip,
                                                  uint32_t* __restrict__ buckets,
                                                  uint32_t* __restrict__ xkey, uint32_t* __restrict__ xvalid,
                                                  uint32_t* __restrict__ xpts, uint32_t* __restrict__ flags) {
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  // the 64-word flag block of the cut sums / cascade that follow on this
  // stream (instead of a memset launch)
  if (flags && t < 64) flags[t] = 0;
  if (t >= nchunks) return;
  const uint32_t M = bstart[K];
  uint32_t start = t * L;
  if (t == 0) {
    xkey[0] = start >= M ? K : bucket_of(bstart, K, start);
    xvalid[0] = 0;
  }
  if (start >= M) {
    // beyond the data: keep the partial list sorted with max-key placeholders
    xkey[2 * t + 1] = K;
    xvalid[2 * t + 1] = 0;
    xkey[2 * t + 2] = K;
    xvalid[2 * t + 2] = 0;
    return;
  }
  uint32_t end = min(start + L, M);
  uint32_t cur = bucket_of(bstart, K, start);
  const uint32_t first_key = cur;
  uint32_t next_b = bstart[cur + 1];
  const bool left_cut = bstart[cur] < start;
  bool head_done = false, tail_done = false;
  Xyzz<F> acc = xyzz_inf<F>();
  bool first_run = true;
  // Software pipeline: the sorted entry two ahead and the base one ahead are
  // in flight while the current mixed addition runs (one gather latency per
  // entry would otherwise be exposed to the few waves a SIMD holds).
  constexpr int PQ = G::PW / 4;  // 16-B words per affine base
  auto row = [&](uint32_t v) {
    uint32_t idx = v & 0x7FFFFFFFu;
    if (tskip) idx += (idx / tn) * tskip;  // entry j*n + i -> table row j*N + i
    return reinterpret_cast<const uint4*>(bases + (size_t)idx * G::PW);
  };
  // (G2 prefetches only the entry: a second 128-B base in flight would cost
  // the second wave per SIMD that 256 VGPRs allow.)
  constexpr bool PF = G::CW == 8;
  uint32_t v_nxt = sval[start];
  uint4 raw[PQ];
  if constexpr (PF) {
    const uint4* q = row(v_nxt);
#pragma unroll
    for (int k = 0; k < PQ; k++) raw[k] = q[k];
  }
  uint32_t v_nn = start + 1 < end ? sval[start + 1] : 0u;
  for (uint32_t p = start; p < end; p++) {
    uint4 cr[PQ];
    const uint32_t v = v_nxt;
    if constexpr (PF) {
#pragma unroll
      for (int k = 0; k < PQ; k++) cr[k] = raw[k];
      if (p + 1 < end) {
        const uint4* q = row(v_nn);
#pragma unroll
        for (int k = 0; k < PQ; k++) raw[k] = q[k];
      }
    } else {
      const uint4* q = row(v);
#pragma unroll
      for (int k = 0; k < PQ; k++) cr[k] = q[k];
    }
    v_nxt = v_nn;
    if (p + 2 < end) v_nn = sval[p + 2];
    if (p == next_b) {
      // run of `cur` ends here (complete on the right)
      if (first_run && left_cut) {
        xkey[2 * t + 1] = cur;
        xvalid[2 * t + 1] = 1;
        st_acc<G>(xpts + (size_t)(2 * t + 1) * XW, acc);
        head_done = true;
      } else {
        st_acc<G>(buckets + (size_t)cur * XW, acc);
      }
      acc = xyzz_inf<F>();
      first_run = false;
      do {
        cur++;
        next_b = bstart[cur + 1];
      } while (next_b == p);  // skip empty buckets
    }
    const uint32_t* w = reinterpret_cast<const uint32_t*>(cr);
    if (w[G::PW - 1] >> 31) continue;  // base at infinity: adds nothing
    Aff<F> P;
    if constexpr (G::CW == 8) {
      P.x = unpack(w);
      P.y = fq_cneg(unpack(w + 8), v >> 31);
      acc = xyzz_madd_g1(acc, P);
    } else {
      P.x = {unpack(w), unpack(w + 8)};
      P.y = {fq_cneg(unpack(w + 16), v >> 31), fq_cneg(unpack(w + 24), v >> 31)};
      acc = xyzz_madd_g2(acc, P);
    }
  }
  const bool left_open = first_run && left_cut;
  const bool right_open = next_b > end;
  if (left_open || right_open) {
    const uint32_t slot = left_open ? 2 * t + 1 : 2 * t + 2;
    xkey[slot] = cur;
    xvalid[slot] = 1;
    st_acc<G>(xpts + (size_t)slot * XW, acc);
    if (left_open) head_done = true;
    else tail_done = true;
  } else {
    st_acc<G>(buckets + (size_t)cur * XW, acc);
  }
  if (!head_done) {
    xkey[2 * t + 1] = first_key;
    xvalid[2 * t + 1] = 0;
  }
  if (!tail_done) {
    xkey[2 * t + 2] = cur;
    xvalid[2 * t + 2] = 0;
  }
}

// G1 bodies fit 128 VGPRs (4 waves per SIMD) only with a minimum-occupancy
// hint; G2 needs ~300 and keeps the default.
#ifndef ZK_ACC0_G2_MINBLK
#define ZK_ACC0_G2_MINBLK 2
#endif
// (Tried: the G1 base prefetch through global_load_lds into LDS instead of 16
// VGPRs, 142 -> 128 VGPRs = 4 waves/SIMD instead of 3: accumulation 1% faster
// isolated, pipelined 2^20 MSM 3% slower; spilling to reach 4-5 waves: +4% /
// +42%.  PMC: 2.6 resident waves/SIMD on average.)
#ifndef ZK_ACC0_G1_MINBLK
#define ZK_ACC0_G1_MINBLK 1
#endif
__global__ void __launch_bounds__(256, ZK_ACC0_G1_MINBLK) k_msm_acc0_g1(const uint32_t* __restrict__ sval, const uint32_t* __restrict__ bstart,
                                                  uint32_t K, uint32_t L, uint32_t nchunks,
                                                  const uint32_t* __restrict__ bases, uint32_t tn, uint32_t tskip,
                                                  uint32_t* __restrict__ buckets,
                                                  uint32_t* __restrict__ xkey, uint32_t* __restrict__ xvalid,
                                                  uint32_t* __restrict__ xpts, uint32_t* __restrict__ flags) { msm_acc0_body<G1T>(sval, bstart, K, L, nchunks, bases, tn, tskip, buckets, xkey, xvalid, xpts, flags); }
__global__ void __launch_bounds__(256, ZK_ACC0_G2_MINBLK) k_msm_acc0_g2(const uint32_t* __restrict__ sval, const uint32_t* __restrict__ bstart,
                                                  uint32_t K, uint32_t L, uint32_t nchunks,
                                                  const uint32_t* __restrict__ bases, uint32_t tn, uint32_t tskip,
                                                  uint32_t* __restrict__ buckets,
                                                  uint32_t* __restrict__ xkey, uint32_t* __restrict__ xvalid,
                                                  uint32_t* __restrict__ xpts, uint32_t* __restrict__ flags) { msm_acc0_body<G2T>(sval, bstart, K, L, nchunks, bases, tn, tskip, buckets, xkey, xvalid, xpts, flags); }
template <class G>
struct Acc0Kernel;
template <>
struct Acc0Kernel<G1T> {
  static constexpr auto fn = k_msm_acc0_g1;
};
template <>
struct Acc0Kernel<G2T> {
  static constexpr auto fn = k_msm_acc0_g2;
};

// ------------------------------------------------ one lane per bucket
// For >= 2^18 buckets (fixed-base tables with c >= 19) the accumulation gives
// each lane a whole bucket: no chunk edges, so no partial sums (except for
// buckets longer than `cap`, split into cap-sized pieces), and no bucket
// boundaries inside a lane's loop.  The items (k_bs_scatter2) are ranked by
// length inside each bin and interleaved over the bins: the 64 lanes of a
// wave get about equal trip counts and the waves that run last are the
// shortest, so the tail is short.  (The chunked path loses ~15% to its tail:
// resident waves of a SIMD finish in age order, the last one alone and
// latency-bound; tools/trace_acc0.py.)
constexpr uint32_t ITEM_CAP_MAX = 1024;
constexpr uint32_t ITEMS_MIN_K = 1u << 18;
constexpr uint32_t NOSLOT = 0xFFFFFFFFu;

// item of lane i: the overflow pieces (full cap-length pieces of split
// buckets) first, then the nmain main slots; empty slots (start == end) are
// buckets without entries.  Returns false when the lane has nothing to add.
__device__ __forceinline__ bool item_of(const uint4* __restrict__ items, uint32_t nover, uint32_t nmain, uint32_t i,
                                        uint4& it) {
  uint32_t idx;
  if (i < nover) {  // (nover <= the grid's npieces by construction)
    idx = nmain + i;
  } else {
    idx = i - nover;
    if (idx >= nmain) return false;
  }
  it = items[idx];
  return it.x != it.y;
}

template <class G>
__device__ __forceinline__ void acc_items_body(const uint4* __restrict__ items, const uint32_t* __restrict__ nover,
                                               uint32_t nmain, const uint32_t* __restrict__ sval,
                                               const uint32_t* __restrict__ bases, uint32_t tn, uint32_t tskip,
                                               uint32_t* __restrict__ buckets, uint32_t* __restrict__ xpts) {
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  constexpr int PQ = G::PW / 4;
  uint4 it;
  if (!item_of(items, *nover, nmain, blockIdx.x * blockDim.x + threadIdx.x, it)) return;
  const uint32_t start = it.x, end = it.y;
  auto row = [&](uint32_t v) {
    uint32_t idx = v & 0x7FFFFFFFu;
    if (tskip) idx += (idx / tn) * tskip;
    const uint32_t* src = bases;
    return reinterpret_cast<const uint4*>(src + (size_t)idx * G::PW);
  };
  constexpr bool PF = G::CW == 8;  // G2: see msm_acc0_body
  Xyzz<F> acc = xyzz_inf<F>();
  bool naff = false;  // acc is one affine point (ZZ = ZZZ = 1)
  uint32_t v_nxt = sval[start];
  uint4 raw[PQ];
  if constexpr (PF) {
    const uint4* q = row(v_nxt);
#pragma unroll
    for (int k = 0; k < PQ; k++) raw[k] = q[k];
  }
  uint32_t v_nn = start + 1 < end ? sval[start + 1] : 0u;
  for (uint32_t p = start; p < end; p++) {
    uint4 cr[PQ];
    const uint32_t v = v_nxt;
    if constexpr (PF) {
#pragma unroll
      for (int k = 0; k < PQ; k++) cr[k] = raw[k];
      if (p + 1 < end) {
        const uint4* q = row(v_nn);
#pragma unroll
        for (int k = 0; k < PQ; k++) raw[k] = q[k];
      }
    } else {
      const uint4* q = row(v);
#pragma unroll
      for (int k = 0; k < PQ; k++) cr[k] = q[k];
    }
    v_nxt = v_nn;
    if (p + 2 < end) v_nn = sval[p + 2];
    const uint32_t* w = reinterpret_cast<const uint32_t*>(cr);
    const bool binf = (w[G::PW - 1] >> 31) != 0;  // base at infinity: mode 3 (no `continue`, see acc_items_g1f)
    Aff<F> P;
    const bool ng = (v >> 31) != 0;  // negative digit: negate y
    if constexpr (G::CW == 8) {
      P.x = unpack(w);
      P.y = unpack(w + 8);
      if (ng) P.y = fq_cneg(P.y, true);
    } else {
      P.x = {unpack(w), unpack(w + 8)};
      P.y = {unpack(w + 16), unpack(w + 24)};
      if (ng) P.y = {fq_cneg(P.y.c0, true), fq_cneg(P.y.c1, true)};
    }
    const int mode = binf ? 3 : xyzz_is_inf(acc) ? 0 : (naff) ? 1 : 2;
    if (mode == 0) {
      acc = xyzz_from_aff(P);
      naff = true;
    } else if (mode == 1) {
      if constexpr (G::CW == 8) acc = xyzz_mmadd_g1({acc.x, acc.y}, P);
      else acc = xyzz_mmadd_g2({acc.x, acc.y}, P);
      naff = false;
    } else if (mode == 2) {
      if constexpr (G::CW == 8) acc = xyzz_madd_g1(acc, P);
      else acc = xyzz_madd_g2(acc, P);
    }
  }
  st_acc<G>(it.w == NOSLOT ? buckets + (size_t)it.z * XW : xpts + (size_t)it.w * XW, acc);
}
// G1 one-lane-per-item accumulation (the dominant kernel of a table MSM):
// rows gathered one entry ahead, the first finite point
// taken as is, the second added by the affine + affine form and every later
// one by xyzz_madd_g1f (subtractions folded into the Montgomery products).  A
// negative digit's y is the borrow form 2p - y (9 subtractions, no carry
// pass).  The rare
// states (a base at infinity, the empty or one-point accumulator after a
// cancellation) branch per lane; lanes of a wave have equal trip counts.
__device__ __forceinline__ void ld_row4(uint4 (&r)[4], const uint4* q) {
  // (Tried, round 6: non-temporal loads here -- every row is read once per
  // MSM -- 2^20 2-lane loop 917 -> 875 Mpt/s, 2^26 63.3 -> 65.3 ms.)
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = q[k];
}
__device__ __forceinline__ void acc_items_g1f(const uint4* __restrict__ items, const uint32_t* __restrict__ nover,
                                              uint32_t nmain, const uint32_t* __restrict__ sval,
                                              const uint32_t* __restrict__ bases, uint32_t tn, uint32_t tskip,
                                              uint32_t* __restrict__ buckets, uint32_t* __restrict__ xpts,
                                              uint32_t i) {
  using F = FqOps;
  constexpr int XW = 32;
  uint4 it;
  if (!item_of(items, *nover, nmain, i, it)) return;
  const uint32_t start = it.x, end = it.y;
  auto row = [&](uint32_t v) {
    uint32_t idx = v & 0x7FFFFFFFu;
    if (tskip) idx += (idx / tn) * tskip;
    const uint32_t* src = bases;
    return reinterpret_cast<const uint4*>(src + (size_t)idx * G1T::PW);
  };
  Xyzz<F> acc = xyzz_inf<F>();
  int phase = 0;  // 0: nothing yet, 1: acc is one affine point, 2: general
  auto step = [&](const uint4 (&r)[4], uint32_t v) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(r);
    // 3: a base at infinity adds nothing.  Folded into the phase switch: a
    // `return` / `continue` here cost the kernel 23 VGPRs (152 -> 129, i.e. 3
    // waves/SIMD with room to spare; 2^20 3-lane 862-870 -> 873-899 Mpt/s)
    const int mode = (w[G1T::PW - 1] >> 31) ? 3 : phase;
    const Fe x2 = unpack(w);
    const Fe y0 = unpack(w + 8);
    const Fe yn = bsub(FqP::B2_1, y0);
    const bool ng = (v >> 31) != 0;
    Fe y2;
#pragma unroll
    for (int k = 0; k < NL; k++) y2.v[k] = ng ? yn.v[k] : y0.v[k];
    if (mode == 2) {
      bool inf;
      acc = xyzz_madd_g1f(acc, x2, y2, &inf);
      if (inf) phase = 0;
    } else if (mode == 1) {
      acc = xyzz_mmadd_g1({acc.x, acc.y}, Aff<F>{x2, reduce_q32<FqP>(y2)});
      phase = xyzz_is_inf(acc) ? 0 : 2;
    } else if (mode == 0) {
      acc = xyzz_from_aff(Aff<F>{x2, reduce_q32<FqP>(y2)});
      phase = 1;
    }
  };
  // one call site of the addition (each inlined copy is ~3.5K instructions):
  // the row of entry p + 1 is in flight while entry p is added.  The loads
  // are unconditional (past the end they re-read the last entry), so the
  // buffer is one loop-carried value with a single copy per entry.  (Round 6:
  // unpacking entry p before reloading the buffer, to drop that copy's 8
  // v_mov_b64, made the compiler keep both buffers live: 127 -> 157 VGPRs,
  // no room left beside three waves for the other lanes' tails.)
  uint4 raw[4];
  const uint32_t last = end - 1;
  uint32_t v_nxt = sval[start];
  ld_row4(raw, row(v_nxt));
  uint32_t v_nn = sval[min(start + 1, last)];
  for (uint32_t p = start; p < end; p++) {
    uint4 cr[4];
    const uint32_t v = v_nxt;
#pragma unroll
    for (int k = 0; k < 4; k++) cr[k] = raw[k];
    ld_row4(raw, row(v_nn));
    v_nxt = v_nn;
    v_nn = sval[min(p + 2, last)];
    step(cr, v);
  }
  if (phase == 0) acc = xyzz_inf<F>();
  st_acc<G1T>(it.w == NOSLOT ? buckets + (size_t)it.z * XW : xpts + (size_t)it.w * XW, acc);
}
// VPAD: the register file padded to 136 VGPRs (three waves per SIMD) instead
// of the launch's LDS reservation (msm_acc_phase) -- for the largest sorts,
// whose scatter workgroups need more LDS than the reservation leaves.
template <bool VPAD>
__global__ void __launch_bounds__(256, ZK_ACC0_G1_MINBLK)
    k_acc_items_g1(const uint4* __restrict__ items, const uint32_t* __restrict__ nover, uint32_t nmain,
                   const uint32_t* __restrict__ sval, const uint32_t* __restrict__ bases, uint32_t tn,
                   uint32_t tskip, uint32_t* __restrict__ buckets, uint32_t* __restrict__ xpts) {
  if constexpr (VPAD) asm volatile("" ::: "v135");
  acc_items_g1f(items, nover, nmain, sval, bases, tn, tskip, buckets, xpts, blockIdx.x * blockDim.x + threadIdx.x);
}
// (Tried for the 3-lane pipeline: rows staged through LDS by
// global_load_lds, and a persistent form with one 768-thread workgroup per CU
// (3 waves/SIMD, the rest of the register file left to other lanes' tails):
// the tails then ran beside the accumulation (95-100% of the step with an
// accumulation running) but the accumulation itself slowed by as much:
// 2^20 3-lane 1.24-1.29 ms/step against 1.17-1.20; dropped.)
__global__ void __launch_bounds__(256, ZK_ACC0_G2_MINBLK)
    k_acc_items_g2(const uint4* __restrict__ items, const uint32_t* __restrict__ nover, uint32_t nmain,
                   const uint32_t* __restrict__ sval, const uint32_t* __restrict__ bases, uint32_t tn,
                   uint32_t tskip, uint32_t* __restrict__ buckets, uint32_t* __restrict__ xpts) {
  acc_items_body<G2T>(items, nover, nmain, sval, bases, tn, tskip, buckets, xpts);
}

// Global class order of the items (one workgroup per bin): class starts from
// the class histogram (longest class first), this bin's offset inside every
// class by one returning atomicAdd per class, then the bin's staged items
// (already class-ordered) copied to their slots.  Items are dense over
// [0, NH * NLO): every bucket has one main item (class 0 = empty, run last).
__global__ void __launch_bounds__(256) k_items_place(const uint4* __restrict__ stage, uint32_t NLO, uint32_t cap,
                                                     const uint32_t* __restrict__ ghist, uint32_t* __restrict__ gcur,
                                                     uint4* __restrict__ items, uint32_t nmain) {
  ZK_TAIL_WAVE();
  __shared__ uint32_t lh[ITEM_CAP_MAX + 1], lstart[ITEM_CAP_MAX + 1], base[ITEM_CAP_MAX + 1], tmp[4];
  const uint32_t h = blockIdx.x;
  const uint4* st = stage + (size_t)h * NLO;
  for (uint32_t c = threadIdx.x; c <= cap; c += 256) lh[c] = 0;
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < NLO; x += 256) {
    const uint4 it = st[x];
    atomicAdd(&lh[min(it.y - it.x, cap)], 1u);
  }
  __syncthreads();
  // the bin's class runs (descending) and the global class starts
  block_prefix<256>(cap + 1, [&](uint32_t k) { return lh[cap - k]; }, lstart, tmp);
  block_prefix<256>(cap + 1, [&](uint32_t k) { return ghist[cap - k]; }, base, tmp);
  for (uint32_t k = threadIdx.x; k <= cap; k += 256) {
    const uint32_t c = cap - k;
    if (lh[c]) base[k] += atomicAdd(&gcur[c], lh[c]);
  }
  __syncthreads();
  for (uint32_t x = threadIdx.x; x < NLO; x += 256) {
    const uint4 it = st[x];
    const uint32_t k = cap - min(it.y - it.x, cap);
    const uint32_t dst = base[k] + (x - lstart[k]);
    if (dst < nmain) items[dst] = it;  // always (the class counts cover exactly nmain items)
  }
}

// Piece sums of the split buckets (k_bs_scatter2's split list: key, first
// partial slot, pieces).  A block takes 4 split buckets: the ones of <= 256
// pieces one wave each (every lane folds its strided share, then a 6-level
// LDS tree), then every larger one with the whole block (256 lanes fold, a
// 6-level tree per wave, 2 levels across the waves).  A witness-like MSM's
// bucket of the digit 1 holds a large share of the entries: zelana_batch's
// ~9K pieces took 137 dependent additions in one wave, ~42 with the block
// (k_split_combine summed to 1.66 ms of a 12 ms proof in the round-5 trace,
// but beside the other lane's work: batch-70 proofs/s measured level, 80.3-
// 82.7 -> 81.2-81.5 resident, 86.5-87.1 -> 87.2-87.3 two in flight).
// One curve-addition call site in one block-uniform step loop (a second
// inlined copy spills G2).  A uniform MSM splits nothing: the launch reads
// the count and exits.
// CHUNKED: the pieces are a chunked accumulation's partials (k_msm_acc0) of a
// bucket cut by chunk edges t0..t0 + np - 1 (split entry: key, t0, np): piece
// 0 is chunk t0's tail slot, piece r >= 1 chunk t0 + r's head slot.
template <class G, bool CHUNKED = false>
__global__ void __launch_bounds__(256) k_split_combine(const uint4* __restrict__ split,
                                                       const uint32_t* __restrict__ nsplit,
                                                       const uint32_t* __restrict__ xpts,
                                                       uint32_t* __restrict__ buckets) {
  ZK_TAIL_WAVE();
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  constexpr uint32_t BIG = 256;  // pieces above which the whole block sums the bucket
  __shared__ Xyzz<F> sh[4][32];
  __shared__ uint4 spl[4];
  const uint32_t ns = *nsplit;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint32_t base = blockIdx.x * 4; base < ns; base += gridDim.x * 4) {  // block-uniform
    if (lane == 0) spl[wave] = base + wave < ns ? split[base + wave] : make_uint4(0, 0, 0, 0);
    __syncthreads();
    // schedule (block-uniform): phase 0 = the small buckets, one per wave;
    // phases 1..4 = the big buckets in wave order, the whole block each
    uint32_t mxs = 0;
    for (int w = 0; w < 4; w++) mxs = max(mxs, spl[w].z <= BIG ? spl[w].z : 0u);
    const uint32_t nload0 = (mxs + 63) / 64;
    uint32_t lev0 = 0;
    while ((1u << lev0) < min(mxs, 64u)) lev0++;
    const uint4 mine = spl[wave];
    const bool small = mine.z <= BIG;
    Xyzz<F> v = xyzz_inf<F>();
    int ph = 0;          // current phase
    uint32_t st0 = 0;    // first step of the phase
    uint32_t nload = nload0, lev = lev0, cross = 0, stride = 64;
    uint4 cur = mine;    // the bucket of this lane's phase
    bool mine_in = small;  // this lane takes part in the phase
    for (uint32_t step = 0;; step++) {
      uint32_t k = step - st0;
      if (k >= nload + lev + cross) {  // phase end (block-uniform): store, next phase
        if (ph == 0) {
          if (small && mine.z && lane == 0) st_xyzz<G>(buckets + (size_t)mine.x * XW, v);
        } else if (threadIdx.x == 0) {
          st_xyzz<G>(buckets + (size_t)cur.x * XW, v);
        }
        v = xyzz_inf<F>();
        int w = ph;  // next big bucket: waves ph.. (phase p >= 1 is wave p - 1's bucket)
        while (w < 4 && spl[w].z <= BIG) w++;
        if (w >= 4) break;
        ph = w + 1;
        cur = spl[w];
        mine_in = true;
        st0 = step;
        k = 0;
        stride = 256;
        nload = (cur.z + 255) / 256;
        lev = 6;
        cross = 2;
      }
      Xyzz<F> q;
      bool act = false;
      if (k < nload) {
        const uint32_t pc = (stride == 64 ? lane : threadIdx.x) + stride * k;
        if (mine_in && pc < cur.z) {
          const uint32_t slot = CHUNKED ? (pc == 0 ? 2 * cur.y + 2 : 2 * (cur.y + pc) + 1) : cur.y + pc;
          q = ld_xyzz<G>(xpts + (size_t)slot * XW);
          act = !xyzz_is_inf(q);
        }
      } else if (k < nload + lev) {  // in-wave tree
        const uint32_t sz = (1u << (lev - 1)) >> (k - nload);
        if (lane >= sz && lane < 2 * sz) sh[wave][lane - sz] = v;
        __syncthreads();
        if (lane < sz) {
          q = sh[wave][lane];
          act = !xyzz_is_inf(q);
        }
      } else {  // across the waves: 4 -> 2 -> 1 (lane 0 of each wave)
        const uint32_t sz = 2u >> (k - nload - lev);
        if (lane == 0 && wave >= sz && wave < 2 * sz) sh[wave - sz][0] = v;
        __syncthreads();
        if (lane == 0 && wave < sz) {
          q = sh[wave][0];
          act = !xyzz_is_inf(q);
        }
      }
      if (act) v = xyzz_is_inf(v) ? q : br_add<G>(v, q);
      if (k >= nload) __syncthreads();
    }
    __syncthreads();  // spl is rewritten by the next iteration
  }
}

template <class G>
__global__ void __launch_bounds__(256) k_msm_accN(const uint32_t* __restrict__ xkey, const uint32_t* __restrict__ xvalid,
                                                  const uint32_t* __restrict__ xpts, uint32_t M, uint32_t L,
                                                  uint32_t nchunks, uint32_t* __restrict__ buckets,
                                                  uint32_t* __restrict__ ykey, uint32_t* __restrict__ yvalid,
                                                  uint32_t* __restrict__ ypts, const uint32_t* __restrict__ prev_open,
                                                  uint32_t* __restrict__ any_open) {
  ZK_TAIL_WAVE();
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nchunks || *prev_open == 0) return;
  uint32_t start = t * L, end = min(start + L, M);
  uint32_t kprev = start > 0 ? xkey[start - 1] : NOKEY;
  uint32_t knext = end < M ? xkey[end] : NOKEY;
  uint32_t first_key = xkey[start], last_key = xkey[end - 1];
  bool head_done = false, tail_done = false;
  Xyzz<F> acc = xyzz_inf<F>();
  uint32_t cur = first_key;
  bool first_run = true, has = false;
  for (uint32_t p = start; p < end; p++) {
    uint32_t k = xkey[p];
    if (k != cur) {
      if (first_run && cur == kprev) {
        ykey[2 * t + 1] = cur;
        yvalid[2 * t + 1] = has;
        if (has) {
          st_xyzz<G>(ypts + (size_t)(2 * t + 1) * XW, acc);
          atomicOr(any_open, 1u);
        }
        head_done = true;
      } else if (has) {
        st_xyzz<G>(buckets + (size_t)cur * XW, acc);
      }
      acc = xyzz_inf<F>();
      has = false;
      cur = k;
      first_run = false;
    }
    if (xvalid[p]) {
      Xyzz<F> q = ld_xyzz<G>(xpts + (size_t)p * XW);
      acc = has ? br_add<G>(acc, q) : q;
      has = true;
    }
  }
  bool left_open = first_run && cur == kprev;
  bool right_open = cur == knext;
  if (left_open || right_open) {
    uint32_t slot = left_open ? 2 * t + 1 : 2 * t + 2;
    ykey[slot] = cur;
    yvalid[slot] = has;
    if (has) {
      st_xyzz<G>(ypts + (size_t)slot * XW, acc);
      atomicOr(any_open, 1u);
    }
    if (left_open) head_done = true;
    else tail_done = true;
  } else if (has) {
    st_xyzz<G>(buckets + (size_t)cur * XW, acc);
  }
  if (!head_done) {
    ykey[2 * t + 1] = first_key;
    yvalid[2 * t + 1] = 0;
  }
  if (!tail_done) {
    ykey[2 * t + 2] = last_key;
    yvalid[2 * t + 2] = 0;
  }
  if (t == 0) {
    ykey[0] = first_key;
    yvalid[0] = 0;
  }
}

// k_msm_accN for small MSMs (K <= CUTSUM_COOP_K, latency-bound): a chunk of
// 16 partials is worked by 16 lanes, one partial each, and its key runs are
// summed by a right-to-left segmented scan over lane shuffles (4 dependent
// additions instead of 15); each run's head lane then writes it exactly as
// the sequential kernel does (complete bucket, or the chunk's head / tail
// slot for the next level).
template <class G>
__global__ void __launch_bounds__(256) k_msm_accN_coop(const uint32_t* __restrict__ xkey,
                                                       const uint32_t* __restrict__ xvalid,
                                                       const uint32_t* __restrict__ xpts, uint32_t M,
                                                       uint32_t nchunks, uint32_t* __restrict__ buckets,
                                                       uint32_t* __restrict__ ykey, uint32_t* __restrict__ yvalid,
                                                       uint32_t* __restrict__ ypts,
                                                       const uint32_t* __restrict__ prev_open,
                                                       uint32_t* __restrict__ any_open) {
  ZK_TAIL_WAVE();
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  constexpr uint32_t L = 16;
  const uint32_t gt = blockIdx.x * 256 + threadIdx.x;
  const uint32_t t = gt / L, r = gt % L;
  if (*prev_open == 0) return;  // uniform over the launch
  const bool chunk = t < nchunks;
  const uint32_t start = t * L, end = chunk ? min(start + L, M) : 0;
  const uint32_t p = start + r;
  const bool in = chunk && p < end;
  const uint32_t key = in ? xkey[p] : NOKEY - 1 - r;  // lanes past the end: distinct keys, no values
  bool has = in && xvalid[p] != 0;
  Xyzz<F> v = xyzz_inf<F>();
  if (has) v = ld_xyzz<G>(xpts + (size_t)p * XW);
#pragma unroll 1
  for (uint32_t sft = 1; sft < L; sft <<= 1) {
    const Xyzz<F> o = shfl_down_xyzz(v, sft);
    const uint32_t ok = (uint32_t)__shfl_down((int)key, sft, L);
    const bool oh = __shfl_down((int)has, sft, L) != 0;
    if (r + sft < L && ok == key && oh) v = has ? br_add<G>(v, o) : o, has = true;
  }
  if (!chunk) return;
  const uint32_t kprev = start > 0 ? xkey[start - 1] : NOKEY;
  const uint32_t knext = end < M ? xkey[end] : NOKEY;
  const uint32_t first_key = xkey[start], last_key = xkey[end - 1];
  const uint32_t left = (uint32_t)__shfl_up((int)key, 1, L);
  const bool head = in && (r == 0 || left != key);
  // slots the chunk's head / tail runs did not fill (the sequential kernel's
  // head_done / tail_done defaults): written first, by lane 0
  const bool first_open = first_key == kprev, last_open = last_key == knext;
  if (r == 0) {
    if (!first_open) {
      ykey[2 * t + 1] = first_key;
      yvalid[2 * t + 1] = 0;
    }
    if (!last_open || (first_key == last_key && first_open)) {
      ykey[2 * t + 2] = last_key;
      yvalid[2 * t + 2] = 0;
    }
    if (t == 0) {
      ykey[0] = first_key;
      yvalid[0] = 0;
    }
  }
  if (!head) return;
  const bool left_open = r == 0 && first_open;
  const bool right_open = key == last_key && last_open;
  if (left_open || right_open) {
    const uint32_t slot = left_open ? 2 * t + 1 : 2 * t + 2;
    ykey[slot] = key;
    yvalid[slot] = has;
    if (has) {
      st_xyzz<G>(ypts + (size_t)slot * XW, v);
      atomicOr(any_open, 1u);
    }
  } else if (has) {
    st_xyzz<G>(buckets + (size_t)key * XW, v);
  }
}

// --------------------------------------------------------- bucket reduction

// Bucket reduction jobs, one per wave (4 per 256-thread workgroup) so that a
// 256-term sum occupies 64 lanes, not 256: every lane folds up to 4 terms,
// then a 6-level LDS tree.  One xyzz_add call site in a uniform loop (a second
// inlined copy doubles VGPRs and spills).
//   FUSED (rows + cols):  job < W*2^hb :  C[w][h] = sum_{l < 2^lb} B[w][(h << lb) + l]
//                         else         :  D[w][l] = sum_{h < 2^hb} B[w][(h << lb) + l]
//   BITS:  job = w*(bb+1) + j:  j < lb : U_j = sum_{l: bit j} D[w][l]
//                               j < bb : U_j = sum_{h: bit j-lb} C[w][h]
//                               j = bb : T   = sum_h C[w][h]      (canonical output)
// Empty buckets were never written (no memset): bstart says which are live.
__device__ __forceinline__ uint32_t insert_bit(uint32_t t, int bit) {
  return (((t >> bit) << (bit + 1)) | (1u << bit) | (t & ((1u << bit) - 1)));
}
#define ZK_BR_WPE 4  // at most 4 waves/SIMD
// minimum waves/SIMD the register allocation must allow (ZK_BR_MINW 4: <= 128
// VGPRs, so a reduction wave fits beside three accumulation waves)
#ifndef ZK_BR_MINW
#define ZK_BR_MINW 1
#endif

template <class G, bool BITS>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ZK_BR_MINW, ZK_BR_WPE))) k_msm_br(const uint32_t* __restrict__ src0, const uint32_t* __restrict__ src1,
                                                const uint32_t* __restrict__ bstart, int lb, int hb, int W, int sr,
                                                int sc, int sb, int segt, uint32_t* __restrict__ out0,
                                                uint32_t* __restrict__ out1) {
  ZK_TAIL_WAVE();
  // Rows and columns are cut into sr / sc segments of <= 256 buckets, one wave
  // each (enough waves for 2^19-bucket windows); C[h][seg], D[l][seg].  Bit
  // sums are cut into sb segments of segt (64..256) terms; the host adds
  // segments.
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  __shared__ Xyzz<F> sh[4][32];
  const int bb = lb + hb;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t job = blockIdx.x * 4 + wave;
  const uint32_t nrow = ((uint32_t)W << hb) * sr, ncol = ((uint32_t)W << lb) * sc;
  const uint32_t njobs = BITS ? (uint32_t)W * (bb + 1) * sb : nrow + ncol;
  const bool live = job < njobs;
  const uint32_t* src = src0;
  uint32_t cnt = 0, stride = 1, bucket0 = 0, t0 = 0;
  int bit = -1, seg = 1;
  uint32_t* dst = nullptr;
  bool canon = false;
  if (live) {
    if (!BITS) {
      if (job < nrow) {  // segment g of row h of window w
        uint32_t rh = job / sr, g = job % sr, w = rh >> hb, h = rh & ((1u << hb) - 1);
        cnt = (1u << lb) / sr;
        bucket0 = (w << bb) + (h << lb) + g * cnt;
        stride = 1;
        dst = out0 + (size_t)job * XW;
      } else {  // segment g of column l of window w
        uint32_t jj = job - nrow, cl = jj / sc, g = jj % sc, w = cl >> lb, l = cl & ((1u << lb) - 1);
        cnt = (1u << hb) / sc;
        bucket0 = (w << bb) + ((g * cnt) << lb) + l;
        stride = 1u << lb;
        dst = out1 + (size_t)jj * XW;
      }
      src = src0 + (size_t)bucket0 * XW;
    } else {
      const uint32_t wj = job / sb;
      t0 = (job % sb) * (uint32_t)segt;  // this job's segment of the term range
      uint32_t w = wj / (bb + 1), j = wj % (bb + 1);
      if ((int)j < lb) {  // U_j over D[l][*] with bit j of l set
        src = src1 + (((size_t)w << lb) * sc) * XW;
        cnt = (1u << (lb - 1)) * sc;
        bit = (int)j;
        seg = sc;
      } else if ((int)j < bb) {  // U_j over C[h][*] with bit j - lb of h set
        src = src0 + (((size_t)w << hb) * sr) * XW;
        cnt = (1u << (hb - 1)) * sr;
        bit = (int)j - lb;
        seg = sr;
      } else {  // T = all C
        src = src0 + (((size_t)w << hb) * sr) * XW;
        cnt = (1u << hb) * sr;
        seg = sr;
      }
      dst = out0 + (size_t)job * XW;
      canon = true;
    }
  }
  // every lane folds its strided share of the job's terms, then a 6-level LDS
  // tree over the wave.  One curve-addition call site in one uniform loop (a
  // second inlined copy spills G2); barriers only in the block-uniform tree
  // steps.
  const uint32_t nload = BITS ? (uint32_t)segt / 64 : 256 / 64;  // block-uniform
  const uint32_t tend = BITS ? min(cnt, t0 + (uint32_t)segt) : cnt;
  Xyzz<F> v = xyzz_inf<F>();
  for (uint32_t step = 0; step < nload + 6; step++) {
    Xyzz<F> q;
    bool act = false;
    if (step < nload) {
      uint32_t t = t0 + lane + 64u * step;
      if (live && t < tend) {
        uint32_t e = BITS ? (bit < 0 ? t : insert_bit(t / seg, bit) * seg + t % seg) : t * stride;
        bool nonempty = BITS ? true : bstart[bucket0 + e + 1] > bstart[bucket0 + e];
        if (nonempty) {
          q = ld_xyzz<G>(src + (size_t)e * XW);
          act = true;
        }
      }
    } else {
      uint32_t sz = 32u >> (step - nload);
      if (lane >= sz && lane < 2 * sz) sh[wave][lane - sz] = v;
      __syncthreads();
      if (lane < sz) {
        q = sh[wave][lane];
        act = !xyzz_is_inf(q);
      }
    }
    if (act) v = xyzz_is_inf(v) ? q : br_add<G>(v, q);
    if (step >= nload) __syncthreads();
  }
  if (live && lane == 0) {
    if (canon) {
      v.x = Io<F>::canon(v.x);
      v.y = Io<F>::canon(v.y);
      v.zz = Io<F>::canon(v.zz);
      v.zzz = Io<F>::canon(v.zzz);
    }
    st_xyzz<G>(dst, v);
  }
}

// Rows / columns in strips (replaces the FUSED pass of k_msm_br when a row or
// column fits one wave): one wave per row h (C[w][h] = sum_l B[w][h, l]) or
// column l (D[w][l] = sum_h B[w][h, l]); lane t folds the contiguous strip
// [t L, (t + 1) L) of its line sequentially, then one 6-level LDS tree.  For
// 2^19-bucket windows this issues ~40% fewer lane-additions than 256-bucket
// jobs (4 folds + 6 levels each), and the bucket reduction runs beside the
// other lane's accumulation, where wasted VALU issue is what it costs.
template <class G>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ZK_BR_MINW, ZK_BR_WPE))) k_msm_br_strip(const uint32_t* __restrict__ buckets,
                                                      const uint32_t* __restrict__ bstart, int lb, int hb, int W,
                                                      int sr, int sc, int mc, uint32_t* __restrict__ outC,
                                                      uint32_t* __restrict__ outD) {
  ZK_TAIL_WAVE();
  // mc = lanes per column line (a power of two <= 64): 64 / mc columns share
  // a wave, so a short column gets the same fold length as a row and a
  // shallower tree (2^19 buckets: 512-bucket columns, mc = 32 -> 16 folds +
  // 5 levels per lane instead of 8 + 6, 25% fewer wave-additions there).
  using F = typename G::F;
  constexpr int XW = 4 * G::CW;
  __shared__ Xyzz<F> sh[4][32];
  const int bb = lb + hb;
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t job = blockIdx.x * 4 + wave;
  const uint32_t nrow = ((uint32_t)W << hb) * sr, ncol = ((uint32_t)W << lb) * sc;
  const uint32_t cpw = 64u / (uint32_t)mc;  // column lines per wave
  const bool row_wave = job < nrow;
  const uint32_t m = row_wave ? 64u : (uint32_t)mc;  // lanes per line (wave-uniform)
  const uint32_t sub = lane & (m - 1), lslot = (lane / m) * (m / 2);
  bool live = false;
  uint32_t len = 0, stride = 1, bucket0 = 0;
  uint32_t* dst = nullptr;
  if (row_wave) {  // segment g of row h of window w (C[h][g], as k_msm_br)
    const uint32_t rh = job / sr, g = job % sr, w = rh >> hb, h = rh & ((1u << hb) - 1);
    live = true;
    len = (1u << lb) / sr;
    bucket0 = (w << bb) + (h << lb) + g * len;
    stride = 1;
    dst = outC + (size_t)job * XW;
  } else {  // segment g of column l of window w
    const uint32_t jj = (job - nrow) * cpw + lane / m;
    if (jj < ncol) {
      const uint32_t cl = jj / sc, g = jj % sc, w = cl >> lb, l = cl & ((1u << lb) - 1);
      live = true;
      len = (1u << hb) / sc;
      bucket0 = (w << bb) + ((g * len) << lb) + l;
      stride = 1u << lb;
      dst = outD + (size_t)jj * XW;
    }
  }
  const uint32_t L = (len + m - 1) / m;  // strip per lane
  const uint32_t Lr = (((1u << lb) / sr) + 63) >> 6, Lc = (((1u << hb) / sc) + mc - 1) / mc;
  const uint32_t Lmax = Lr > Lc ? Lr : Lc;  // block-uniform loop bound
  Xyzz<F> v = xyzz_inf<F>();
  for (uint32_t step = 0; step < Lmax + 6; step++) {
    Xyzz<F> q;
    bool act = false;
    if (step < Lmax) {
      const uint32_t t = sub * L + step;
      if (live && step < L && t < len) {
        const uint32_t b = bucket0 + t * stride;
        if (bstart[b + 1] > bstart[b]) {
          q = ld_xyzz<G>(buckets + (size_t)b * XW);
          act = true;
        }
      }
    } else {  // tree levels 32 .. 1 (block-uniform barriers; levels >= m idle)
      const uint32_t sz = 32u >> (step - Lmax);
      if (sz < m && sub >= sz && sub < 2 * sz) sh[wave][lslot + sub - sz] = v;
      __syncthreads();
      if (sz < m && sub < sz) {
        q = sh[wave][lslot + sub];
        act = !xyzz_is_inf(q);
      }
    }
    if (act) v = xyzz_is_inf(v) ? q : br_add<G>(v, q);
    if (step >= Lmax) __syncthreads();
  }
  if (live && sub == 0) st_xyzz<G>(dst, v);
}

// (Tried: row / column sums as per-strip folds + an LDS-packed line tree
// (issues ~35% fewer wave-additions, 0.38 vs 0.45 ms isolated), and the folds
// + a second in-wave strip pass: level or slower in the pipelined MSM and 2-7%
// slower in the proofs; dropped.)

// ------------------------------------------------------------ base upload
// canonical affine (x||y, all-zero = infinity) -> internal Montgomery packed,
// validated on the curve.  G2's b = 3/(9+u).
__constant__ uint32_t G2B_C0[8] = {0x24a138e5u, 0x3267e6dcu, 0x59dbefa3u, 0xb5b4c5e5u,
                                   0x1be06ac3u, 0x81be1899u, 0xceb8aaaeu, 0x2b149d40u};
__constant__ uint32_t G2B_C1[8] = {0x85c315d2u, 0xe4a2bd06u, 0xe52d1852u, 0xa74fa084u,
                                   0xeed8fdf4u, 0xcd2cafadu, 0x3af0fed4u, 0x009713b0u};

template <class G>
__global__ void __launch_bounds__(256) k_bases_convert(const uint32_t* __restrict__ in, size_t n,
                                                       uint32_t* __restrict__ out, uint32_t* __restrict__ bad) {
  using F = typename G::F;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* p = in + i * G::PW;
  uint32_t o = 0;
  for (int k = 0; k < G::PW; k++) o |= p[k];
  uint32_t* q = out + i * G::PW;
  if (o == 0) {
    for (int k = 0; k < G::PW; k++) q[k] = 0;
    q[G::PW - 1] = 0x80000000u;
    return;
  }
  if constexpr (G::CW == 8) {
    Fe x = to_mont<FqP>(ld_fe(p)), y = to_mont<FqP>(ld_fe(p + 8));
    Fe b = to_mont<FqP>(Fe{{3, 0, 0, 0, 0, 0, 0, 0, 0}});
    Fe lhs = sqr<FqP>(y), rhs = add<FqP>(mul<FqP>(sqr<FqP>(x), x), b);
    if (!eq<FqP>(lhs, rhs)) atomicOr(bad, 1u);
    st_fe(q, reduce<FqP>(x));
    st_fe(q + 8, reduce<FqP>(y));
  } else {
    Fe2 x = {to_mont<FqP>(ld_fe(p)), to_mont<FqP>(ld_fe(p + 8))};
    Fe2 y = {to_mont<FqP>(ld_fe(p + 16)), to_mont<FqP>(ld_fe(p + 24))};
    Fe2 b = {to_mont<FqP>(ld_fe(G2B_C0)), to_mont<FqP>(ld_fe(G2B_C1))};
    Fe2 lhs = f2_sqr(y), rhs = f2_add(f2_mul(f2_sqr(x), x), b);
    if (!(eq<FqP>(lhs.c0, rhs.c0) && eq<FqP>(lhs.c1, rhs.c1))) atomicOr(bad, 1u);
    st_fe(q, reduce<FqP>(x.c0));
    st_fe(q + 8, reduce<FqP>(x.c1));
    st_fe(q + 16, reduce<FqP>(y.c0));
    st_fe(q + 24, reduce<FqP>(y.c1));
  }
}

// ------------------------------------------------ synthetic inputs (bench)
// Deterministic pseudo-random inputs generated where they will live (HBM):
//   scalars: splitmix64 stream per index, 254-bit candidates rejected until < r
//   bases:   P_i = k_i * G with k_i from the same stream (253-bit), G the
//            standard generator (G1: (1, 2); G2: the arkworks/EIP-197 one),
//            normalised to affine (internal Montgomery form)
__device__ __forceinline__ uint64_t splitmix64(uint64_t& x) {
  uint64_t z = (x += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__constant__ uint64_t FR_MOD64[4] = {0x43e1f593f0000001ull, 0x2833e84879b97091ull, 0xb85045b68181585dull,
                                     0x30644e72e131a029ull};
__global__ void __launch_bounds__(256) k_gen_scalars(uint64_t seed, size_t first, size_t n, uint64_t* __restrict__ out) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t gi = first + i;
  uint64_t st = seed * 0x100000001B3ull ^ (gi * 0x9E3779B97F4A7C15ull);
  uint64_t v[4];
  for (;;) {
    for (int k = 0; k < 4; k++) v[k] = splitmix64(st);
    v[3] &= 0x3FFFFFFFFFFFFFFFull;  // 254 bits
    bool lt = false;
    for (int k = 3; k >= 0; k--) {
      if (v[k] != FR_MOD64[k]) {
        lt = v[k] < FR_MOD64[k];
        break;
      }
    }
    if (lt) break;
  }
  for (int k = 0; k < 4; k++) out[i * 4 + k] = v[k];
}
// G2 generator (canonical): x = (x0, x1), y = (y0, y1)
__constant__ uint32_t G2GEN[32] = {
    0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu,
    0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u,
    0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u,
    0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};

__device__ Fe fq_inv(const Fe& a) {
  const uint64_t e[4] = {0x3c208c16d87cfd45ull, 0x97816a916871ca8dull, 0xb85045b68181585dull, 0x30644e72e131a029ull};
  return pow<FqP>(a, e);  // a^(q-2)
}
template <class G>
__global__ void __launch_bounds__(256) k_gen_bases(uint64_t seed, size_t first, size_t n, uint32_t* __restrict__ out) {
  using F = typename G::F;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t gi = first + i;  // element i of the range is global element first + i
  uint64_t st = (seed + 0x51ED270Bull) * 0x100000001B3ull ^ (gi * 0xD1B54A32D192ED03ull);
  uint64_t k[4];
  for (int j = 0; j < 4; j++) k[j] = splitmix64(st);
  k[3] &= 0x1FFFFFFFFFFFFFFFull;  // 253 bits < r
  k[0] |= 1;                       // never zero
  Aff<F> g;
  if constexpr (G::CW == 8) {
    g.x = to_mont<FqP>(Fe{{1, 0, 0, 0, 0, 0, 0, 0, 0}});
    g.y = to_mont<FqP>(Fe{{2, 0, 0, 0, 0, 0, 0, 0, 0}});
  } else {
    g.x = {to_mont<FqP>(ld_fe(G2GEN)), to_mont<FqP>(ld_fe(G2GEN + 8))};
    g.y = {to_mont<FqP>(ld_fe(G2GEN + 16)), to_mont<FqP>(ld_fe(G2GEN + 24))};
  }
  Xyzz<F> acc = xyzz_inf<F>();
  for (int b = 252; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((k[b >> 6] >> (b & 63)) & 1) acc = xyzz_madd(acc, g);
  }
  uint32_t* q = out + i * G::PW;
  if constexpr (G::CW == 8) {
    Fe izz = fq_inv(acc.zz), izzz = fq_inv(acc.zzz);
    st_fe(q, reduce<FqP>(mul<FqP>(acc.x, izz)));
    st_fe(q + 8, reduce<FqP>(mul<FqP>(acc.y, izzz)));
  } else {
    // Fq2 inverse via the norm
    auto inv2 = [](const Fe2& a) {
      Fe nrm = add<FqP>(sqr<FqP>(a.c0), sqr<FqP>(a.c1));
      Fe ni = fq_inv(nrm);
      return Fe2{mul<FqP>(a.c0, ni), neg<FqP>(mul<FqP>(a.c1, ni))};
    };
    Fe2 x = f2_mul(acc.x, inv2(acc.zz)), y = f2_mul(acc.y, inv2(acc.zzz));
    st_fe(q, reduce<FqP>(x.c0));
    st_fe(q + 8, reduce<FqP>(x.c1));
    st_fe(q + 16, reduce<FqP>(y.c0));
    st_fe(q + 24, reduce<FqP>(y.c1));
  }
}
// SURVEY.md §8d point stream: P_i = P0 + i * D (P0, D = the first two
// G1::rand draws of StdRng(seed), drawn on the host), element i of the range
// = global element first + i.  Canonical affine in, internal affine out.
__global__ void __launch_bounds__(256) k_gen_bases_arith(const uint32_t* __restrict__ p0d, size_t first, size_t n,
                                                         uint32_t* __restrict__ out) {
  using F = FqOps;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t gi = first + i;
  Aff<F> p0, d;
  p0.x = to_mont<FqP>(ld_fe(p0d));
  p0.y = to_mont<FqP>(ld_fe(p0d + 8));
  d.x = to_mont<FqP>(ld_fe(p0d + 16));
  d.y = to_mont<FqP>(ld_fe(p0d + 24));
  Xyzz<F> acc = xyzz_inf<F>();
  for (int b = 63; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((gi >> b) & 1) acc = xyzz_madd(acc, d);
  }
  acc = xyzz_madd(acc, p0);
  uint32_t* q = out + i * G1T::PW;
  if (xyzz_is_inf(acc)) {  // P0 + i D = O: stored as the infinity flag
    for (int k = 0; k < G1T::PW; k++) q[k] = 0;
    q[G1T::PW - 1] = 1u << 31;
    return;
  }
  Fe izz = fq_inv(acc.zz), izzz = fq_inv(acc.zzz);
  st_fe(q, reduce<FqP>(mul<FqP>(acc.x, izz)));
  st_fe(q + 8, reduce<FqP>(mul<FqP>(acc.y, izzz)));
}
// Fixed-base table: copy j of point i is 2^(shift) * copy (j-1), in affine
// form (one inversion of ZZ*ZZZ per copy).  Built once per base set (pk load);
// MSMs then trade W windows of n entries for Wp windows of p*n entries, which
// removes (p-1)/p of the bucket-reduction and Horner work and lets c grow.
template <class F>
__device__ __forceinline__ typename F::T inv_any(const typename F::T& a);
template <>
__device__ __forceinline__ Fe inv_any<FqOps>(const Fe& a) {
  return fq_inv(a);
}
template <>
__device__ __forceinline__ Fe2 inv_any<Fq2Ops>(const Fe2& a) {
  Fe nrm = add<FqP>(sqr<FqP>(a.c0), sqr<FqP>(a.c1));
  Fe ni = fq_inv(nrm);
  return Fe2{mul<FqP>(a.c0, ni), neg<FqP>(mul<FqP>(a.c1, ni))};
}
// Copy j >= 1 is copy j-1 doubled `shift` times, or shift - 1 times once
// j - 1 >= wide (balanced window widths, WinLayout; wide = p: uniform).
template <class G>
__global__ void __launch_bounds__(256) k_bases_table(uint32_t* __restrict__ pts, size_t n, int shift, int wide, int p,
                                                     uint32_t* __restrict__ bad) {
  using F = typename G::F;
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool inf = pts[i * G::PW + G::PW - 1] >> 31;
  Aff<F> q = ld_aff<G>(pts, (uint32_t)i);
  for (int j = 1; j < p; j++) {
    uint32_t* o = pts + ((size_t)j * n + i) * G::PW;
    if (inf) {
      for (int k = 0; k < G::PW; k++) o[k] = 0;
      o[G::PW - 1] = 0x80000000u;
      continue;
    }
    Xyzz<F> acc = xyzz_mdbl(q);
    const int dbls = j - 1 < wide ? shift : shift - 1;
    for (int k = 1; k < dbls; k++) acc = xyzz_dbl(acc);
    if (xyzz_is_inf(acc)) {  // impossible without 2-power torsion; refuse
      atomicOr(bad, 1u);
      return;
    }
    auto t = inv_any<F>(F::mul(acc.zz, acc.zzz));
    q.x = F::mul(acc.x, F::mul(t, acc.zzz));
    q.y = F::mul(acc.y, F::mul(t, acc.zz));
    if constexpr (G::CW == 8) {
      q.x = reduce<FqP>(q.x);
      q.y = reduce<FqP>(q.y);
      st_fe(o, q.x);
      st_fe(o + 8, q.y);
    } else {
      q.x = {reduce<FqP>(q.x.c0), reduce<FqP>(q.x.c1)};
      q.y = {reduce<FqP>(q.y.c0), reduce<FqP>(q.y.c1)};
      st_fe(o, q.x.c0);
      st_fe(o + 8, q.x.c1);
      st_fe(o + 16, q.y.c0);
      st_fe(o + 24, q.y.c1);
    }
  }
}

// ------------------------------------------------- fixed-base scalar mult
// k_i * G for a batch of scalars and ONE base (Groth16 setup: every query
// point is a multiple of the G1 / G2 generator, ark-groth16 FixedBase::msm).
// Table: window w (8 bits, 32 windows cover 256 bits) entry d = d 2^(8w) G,
// internal affine.  A scalar then costs <= 32 mixed additions and one
// inversion (of ZZ * ZZZ) to come back to affine.
constexpr int FB_WIN = 8, FB_NW = 32;
template <class G>
__global__ void __launch_bounds__(256) k_fb_table(const uint32_t* __restrict__ gen, uint32_t* __restrict__ tab) {
  using F = typename G::F;
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (uint32_t)FB_NW << FB_WIN) return;
  const uint32_t w = e >> FB_WIN, d = e & ((1u << FB_WIN) - 1);
  uint32_t* o = tab + (size_t)e * G::PW;
  if (d == 0) {
    for (int k = 0; k < G::PW; k++) o[k] = 0;
    o[G::PW - 1] = 0x80000000u;
    return;
  }
  const Aff<F> g = ld_aff<G>(gen, 0);
  Xyzz<F> acc = xyzz_inf<F>();
  for (int b = FB_WIN - 1; b >= 0; b--) {
    acc = xyzz_dbl(acc);
    if ((d >> b) & 1) acc = xyzz_madd(acc, g);
  }
  for (uint32_t k = 0; k < FB_WIN * w; k++) acc = xyzz_dbl(acc);
  auto t = inv_any<F>(F::mul(acc.zz, acc.zzz));
  Aff<F> q;
  q.x = F::mul(acc.x, F::mul(t, acc.zzz));
  q.y = F::mul(acc.y, F::mul(t, acc.zz));
  if constexpr (G::CW == 8) {
    st_fe(o, reduce<FqP>(q.x));
    st_fe(o + 8, reduce<FqP>(q.y));
  } else {
    st_fe(o, reduce<FqP>(q.x.c0));
    st_fe(o + 8, reduce<FqP>(q.x.c1));
    st_fe(o + 16, reduce<FqP>(q.y.c0));
    st_fe(o + 24, reduce<FqP>(q.y.c1));
  }
}
// out[i] = scalars[i] * G, canonical affine (all-zero = infinity); scalars
// canonical packed 8 x u32, < r.
template <class G>
__global__ void __launch_bounds__(256) k_fb_mul(const uint32_t* __restrict__ tab, const uint32_t* __restrict__ sc,
                                                size_t n, uint32_t* __restrict__ out) {
  using F = typename G::F;
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 a = reinterpret_cast<const uint4*>(sc)[2 * i], b = reinterpret_cast<const uint4*>(sc)[2 * i + 1];
  const uint32_t s[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  Xyzz<F> acc = xyzz_inf<F>();
  for (int w = 0; w < FB_NW; w++) {
    const uint32_t d = (s[w >> 2] >> (8 * (w & 3))) & 0xFFu;
    if (d) acc = xyzz_madd(acc, ld_aff<G>(tab, (uint32_t)(w << FB_WIN) + d));
  }
  uint32_t* q = out + i * G::PW;
  if (xyzz_is_inf(acc)) {
    for (int k = 0; k < G::PW; k++) q[k] = 0;
    return;
  }
  auto t = inv_any<F>(F::mul(acc.zz, acc.zzz));
  Aff<F> r;
  r.x = F::mul(acc.x, F::mul(t, acc.zzz));
  r.y = F::mul(acc.y, F::mul(t, acc.zz));
  if constexpr (G::CW == 8) {
    st_fe(q, from_mont<FqP>(r.x));
    st_fe(q + 8, from_mont<FqP>(r.y));
  } else {
    st_fe(q, from_mont<FqP>(r.x.c0));
    st_fe(q + 8, from_mont<FqP>(r.x.c1));
    st_fe(q + 16, from_mont<FqP>(r.y.c0));
    st_fe(q + 24, from_mont<FqP>(r.y.c1));
  }
}

// host: d_out[i] = d_scalars[i] * gen (gen canonical affine on the host)
int fixed_base_mul(zkmi_ctx* ctx, int g2, const uint64_t* gen, const uint32_t* d_scalars, size_t n,
                   uint32_t* d_out) {
  zkmi_bases* gb = nullptr;
  ZK_TRY(bases_upload(ctx, g2, gen, 1, &gb));  // validates the generator (on the curve)
  const int pw = g2 ? 32 : 16;
  uint32_t* tab;
  int rc = ctx->ws.get(g2 ? "fb_table_g2" : "fb_table_g1", (size_t)(FB_NW << FB_WIN) * pw * 4, (void**)&tab);
  if (!rc) {
    const unsigned gt = (unsigned)(((FB_NW << FB_WIN) + 255) / 256), gm = (unsigned)((n + 255) / 256);
    if (g2) k_fb_table<G2T><<<gt, 256, 0, ctx->stream>>>(gb->d_pts, tab);
    else k_fb_table<G1T><<<gt, 256, 0, ctx->stream>>>(gb->d_pts, tab);
    if (n) {
      if (g2) k_fb_mul<G2T><<<gm, 256, 0, ctx->stream>>>(tab, d_scalars, n, d_out);
      else k_fb_mul<G1T><<<gm, 256, 0, ctx->stream>>>(tab, d_scalars, n, d_out);
    }
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
      set_error("fixed_base_mul: kernel failure");
      rc = ZKMI_EHIP;
    }
  }
  zkmi_bases_destroy(gb);
  return rc;
}

// internal -> canonical affine (export for checking)
template <class G>
__global__ void __launch_bounds__(256) k_bases_export(const uint32_t* __restrict__ in, size_t n,
                                                      uint32_t* __restrict__ out) {
  size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t* p = in + i * G::PW;
  uint32_t* q = out + i * G::PW;
  if (p[G::PW - 1] >> 31) {
    for (int k = 0; k < G::PW; k++) q[k] = 0;
    return;
  }
  for (int c = 0; c < G::PW / 8; c++) st_fe(q + 8 * c, from_mont<FqP>(ld_fe(p + 8 * c)));
}

int bases_generate(zkmi_ctx* ctx, int g2, uint64_t seed, size_t first, size_t n, zkmi_bases** out) {
  int pw = g2 ? 32 : 16;
  uint32_t* d_pts = nullptr;
  if (hipMalloc(&d_pts, std::max<size_t>(1, n) * pw * 4) != hipSuccess) {
    (void)hipGetLastError();
    set_error("hipMalloc(%zu) failed for bases", n * pw * 4);
    return ZKMI_ENOMEM;
  }
  if (n) {
    unsigned grid = (unsigned)((n + 255) / 256);
    if (g2) k_gen_bases<G2T><<<grid, 256, 0, ctx->stream>>>(seed, first, n, d_pts);
    else k_gen_bases<G1T><<<grid, 256, 0, ctx->stream>>>(seed, first, n, d_pts);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  zkmi_bases* b = new zkmi_bases;
  b->ctx = ctx;
  b->g2 = g2;
  b->n = n;
  b->d_pts = d_pts;
  *out = b;
  return 0;
}
int bases_generate_arith_g1(zkmi_ctx* ctx, const uint64_t p0[8], const uint64_t d[8], size_t first, size_t n,
                            zkmi_bases** out) {
  uint32_t* d_pts = nullptr;
  uint32_t* d_in = nullptr;
  if (hipMalloc(&d_pts, std::max<size_t>(1, n) * 64) != hipSuccess) {
    (void)hipGetLastError();
    set_error("hipMalloc(%zu) failed for bases", n * 64);
    return ZKMI_ENOMEM;
  }
  ZK_TRY(ctx->ws.get("bases_arith_in", 128, (void**)&d_in));
  uint64_t h[16];
  memcpy(h, p0, 64);
  memcpy(h + 8, d, 64);
  ZK_HIP(hipMemcpyAsync(d_in, h, 128, hipMemcpyHostToDevice, ctx->stream));
  if (n) {
    k_gen_bases_arith<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(d_in, first, n, d_pts);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  zkmi_bases* b = new zkmi_bases;
  b->ctx = ctx;
  b->g2 = 0;
  b->n = n;
  b->d_pts = d_pts;
  *out = b;
  return 0;
}
int bases_export(const zkmi_bases* b, uint64_t* host_out) {
  zkmi_ctx* ctx = b->ctx;
  int pw = b->g2 ? 32 : 16;
  uint32_t* tmp;
  ZK_TRY(ctx->ws.get("bases_export", std::max<size_t>(1, b->n) * pw * 4, (void**)&tmp));
  if (b->n) {
    unsigned grid = (unsigned)((b->n + 255) / 256);
    if (b->g2) k_bases_export<G2T><<<grid, 256, 0, ctx->stream>>>(b->d_pts, b->n, tmp);
    else k_bases_export<G1T><<<grid, 256, 0, ctx->stream>>>(b->d_pts, b->n, tmp);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(host_out, tmp, b->n * pw * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}
int scalars_generate(zkmi_ctx* ctx, uint64_t seed, size_t first, size_t n, void* d_out) {
  if (n) {
    k_gen_scalars<<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(seed, first, n, (uint64_t*)d_out);
    ZK_HIP(hipGetLastError());
  }
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

int bases_from_device_canon(zkmi_ctx* ctx, int g2, const uint32_t* d_canon, size_t n, zkmi_bases** out) {
  int pw = g2 ? 32 : 16;
  uint32_t* d_pts = nullptr;
  if (hipMalloc(&d_pts, std::max<size_t>(1, n) * pw * 4) != hipSuccess) {
    set_error("hipMalloc(%zu) failed for bases", n * pw * 4);
    return ZKMI_ENOMEM;
  }
  uint32_t* d_bad;
  ZK_TRY(ctx->ws.get("bases_bad", 4, (void**)&d_bad));
  ZK_HIP(hipMemsetAsync(d_bad, 0, 4, ctx->stream));
  if (n) {
    unsigned grid = (unsigned)((n + 255) / 256);
    if (g2) k_bases_convert<G2T><<<grid, 256, 0, ctx->stream>>>(d_canon, n, d_pts, d_bad);
    else k_bases_convert<G1T><<<grid, 256, 0, ctx->stream>>>(d_canon, n, d_pts, d_bad);
    ZK_HIP(hipGetLastError());
  }
  uint32_t bad = 0;
  ZK_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  if (bad) {
    hipFree(d_pts);
    set_error("bases: point not on curve");
    return ZKMI_EPOINT;
  }
  zkmi_bases* b = new zkmi_bases;
  b->ctx = ctx;
  b->g2 = g2;
  b->n = n;
  b->d_pts = d_pts;
  *out = b;
  return 0;
}

int bases_upload(zkmi_ctx* ctx, int g2, const uint64_t* host_affine, size_t n, zkmi_bases** out) {
  int pw = g2 ? 32 : 16;
  uint32_t* d_tmp;
  ZK_TRY(ctx->ws.get("bases_stage", std::max<size_t>(1, n) * pw * 4, (void**)&d_tmp));
  if (n) ZK_HIP(hipMemcpyAsync(d_tmp, host_affine, n * pw * 4, hipMemcpyHostToDevice, ctx->stream));
  return bases_from_device_canon(ctx, g2, d_tmp, n, out);
}

// neg[r] = (x, 2p - y) for every table row r (both Fq2 components for G2) --
// exactly the y that fq_cneg produces -- infinity rows copied as they are

int bases_precompute(zkmi_bases* b, int c, int factor) {
  if (c < 4 || c > 22) {
    set_error("bases_precompute: window %d outside [4, 22]", c);
    return ZKMI_EINVAL;
  }
  const int W = msm_windows(c);
  if (factor <= 0 || factor > W) factor = W;
  const int Wp = (W + factor - 1) / factor;
  const int p = (W + Wp - 1) / Wp;  // no copy beyond the last window
  if ((size_t)p * b->n >= (1ull << 31)) {
    set_error("bases_precompute: %d x %zu table rows exceed the 2^31 index space", p, b->n);
    return ZKMI_EINVAL;
  }
  zkmi_ctx* ctx = b->ctx;
  const int pw = b->g2 ? 32 : 16;
  const size_t row = std::max<size_t>(1, b->n) * pw * 4;
  uint32_t* d_tab = nullptr;
  if (hipMalloc(&d_tab, row * p) != hipSuccess) {
    (void)hipGetLastError();
    set_error("hipMalloc(%zu) failed for the fixed-base table", row * p);
    return ZKMI_ENOMEM;
  }
  uint32_t* d_bad;
  int rc = ctx->ws.get("bases_bad", 4, (void**)&d_bad);
  if (rc) {
    hipFree(d_tab);
    return rc;
  }
  hipStream_t st = ctx->stream;
  uint32_t bad = 0;
  hipError_t e = hipMemsetAsync(d_bad, 0, 4, st);
  if (e == hipSuccess && b->n) e = hipMemcpyAsync(d_tab, b->d_pts, b->n * pw * 4, hipMemcpyDeviceToDevice, st);
  // full tables (one window per copy) use the balanced widths (WinLayout):
  // no short top window piling a copy's entries onto a few buckets.
  const bool bal = Wp == 1 && c >= 4;
  const int wide = bal ? std::max(0, 254 - W * (c - 1)) : p;
  if (e == hipSuccess && b->n && p > 1) {
    unsigned grid = (unsigned)((b->n + 255) / 256);
    if (b->g2) k_bases_table<G2T><<<grid, 256, 0, st>>>(d_tab, b->n, c * Wp, wide, p, d_bad);
    else k_bases_table<G1T><<<grid, 256, 0, st>>>(d_tab, b->n, c * Wp, wide, p, d_bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess || bad) {
    hipFree(d_tab);
    if (e != hipSuccess) set_error("bases_precompute: %s", hipGetErrorString(e));
    else set_error("bases_precompute: a base reached infinity under doubling (not in a prime-order group)");
    return e != hipSuccess ? ZKMI_EHIP : ZKMI_EPOINT;
  }
  hipFree(b->d_pts);
  b->d_pts = d_tab;
  b->tc = c;
  b->tp = p;
  b->tw = Wp;
  b->tbal = bal ? 1 : 0;
  // (A negated copy of the table -- gather -P for a negative digit instead of
  // negating y per entry, ~60 instructions -- measured level at 2^20 and 1.3%
  // slower at 2^26 while doubling the table's HBM; dropped.)
  return 0;
}

// Window for a full table over N bases: one window of W(c)*N entries and 2^(c-1)
// buckets; bucket reduction costs ~2.5 additions per bucket.  From 2^18
// buckets on, the accumulation runs one lane per bucket (k_acc_items).
int table_window(size_t N, int g2) {
  // (G2: c = 17 below 2^21 points is faster for a lone MSM, 2^19: 4.45 ->
  // 3.50 ms, but in a prove it splits B1 / B2's shared sort: zelana_batch 66
  // -> 61 proofs/s.  Same window for both groups.)
  (void)g2;
  int best = 8;
  double cost = 1e300;
  // c = 22 (12 copies instead of 13, 2^21 buckets) from 2^25 bases on: 2^26
  // one lane 73.8 -> 72.8 ms, two lanes 914 -> 942 Mpoint/s; below that its
  // latency-bound bucket reduction (~1 ms) costs more than it saves
  const int cmax = N >= (size_t(1) << 25) ? 22 : 20;
  for (int c = 6; c <= cmax; c++) {
    double k = (double)msm_windows(c) * (double)N + 2.5 * (double)(1u << (c - 1));
    if (k < cost) {
      cost = k;
      best = c;
    }
  }
  return best;
}

// ------------------------------------------------------------- driver
static int pick_window(size_t n) {
  if (n < (1u << 10)) return 8;
  if (n < (1u << 14)) return 11;
  if (n < (1u << 17)) return 13;
  if (n < (1u << 19)) return 15;
  if (n < (1u << 22)) return 16;
  return 17;
}

// Calls f(std::integral_constant<int, C>, std::bool_constant<BAL>) for the
// window c in [CMIN, 22] and the layout bal, so only those windows' kernels are
// instantiated; `who` prefixes the error of a window outside the range.
template <int CMIN, class F, int... I>
static bool window_call(int c, bool bal, F& f, std::integer_sequence<int, I...>) {
  return ((c == CMIN + I && (bal ? f(std::integral_constant<int, CMIN + I>{}, std::true_type{})
                                 : f(std::integral_constant<int, CMIN + I>{}, std::false_type{}),
                             true)) ||
          ...);
}
template <int CMIN, class F>
static int dispatch_window(int c, bool bal, const char* who, F f) {
  if (window_call<CMIN>(c, bal, f, std::make_integer_sequence<int, 22 - CMIN + 1>{})) return 0;
  set_error("%sunsupported MSM window %d", who, c);
  return ZKMI_EINVAL;
}

// nb scalar vectors sstride words apart, one grid row each (a single MSM: nb = 1)
static int dispatch_digits(int c, hipStream_t st, const uint32_t* sc, size_t n, int p, int Wp, bool bal,
                           int32_t* dg, uint32_t nb, size_t sstride) {
  const dim3 grid((unsigned)((n + 255) / 256), nb);
  return dispatch_window<4>(c, bal, "", [&](auto C, auto BAL) {
    k_msm_digits<C(), BAL()><<<grid, 256, 0, st>>>(sc, n, p, Wp, dg, sstride);
  });
}

// K covers every vector's windows
static int small_sort(int c, bool bal, hipStream_t st, const uint32_t* sc, size_t n, int Wp, uint32_t B, uint32_t wsel, uint32_t K,
                      uint32_t* cnt, uint32_t* cursor, uint32_t* bstart, uint32_t* sval, uint32_t nb, size_t sstride) {
  const dim3 grid((unsigned)((n + 255) / 256), nb);
  return dispatch_window<12>(c, bal, "small_sort: ", [&](auto C, auto BAL) {
    k_ss_count<C(), BAL()><<<grid, 256, 0, st>>>(sc, n, Wp, B, wsel, cnt, sstride);
    k_ss_scan<<<1, 1024, 0, st>>>(cnt, K, bstart, cursor);
    k_ss_scatter<C(), BAL()><<<grid, 256, 0, st>>>(sc, n, Wp, B, wsel, cursor, sval, sstride);
  });
}

}  // namespace zk

// An MSM in flight: GPU work and the D2H of the bit sums are queued on the
// context stream; the host epilogue runs in zkmi_msm_wait, so a caller can
// overlap it with the next MSM's kernels (submit k+1, then wait k).
struct zkmi_msm_job {
  zkmi_ctx* ctx;
  int g2, c, W, bb;
  uint32_t* host;  // pinned: W*(bb+1)*sb canonical XYZZ
  size_t host_words;
  hipEvent_t done;
  bool empty;
  int sb = 1;                   // segments per bit sum (added on the host)
  hipStream_t st = nullptr;     // lane stream the D2H of `host` is queued on
  zkmi_comm* comm = nullptr;    // sharded MSM: bit sums of every rank are summed
  bool exchanged = false;       // sharded over RCCL: the all-gather is queued
  bool wmode = false;           // window-sharded: each rank's bit sums cover its windows only
  int w0 = 0;                   // (window-sharded) this rank's first window
  bool done_rec = false;        // `done` is recorded after the D2H (msm_job_free waits on it, not on st)
  // sharded over a host transport, failed at submit: msm_wait runs the
  // failure exchange (in wait order, as the peers' exchanges) and returns this
  int fail_rc = 0;
  std::string fail_msg;
  // Batched MSMs (zkmi_msm_batch_submit).  A group job (nbat >= 1) is one
  // launch sequence over nbat scalar vectors: W = nbat x the single plan's
  // windows, the bit sums of vector i in windows [i W / nbat, (i + 1) W / nbat).
  // The job handed to the caller (batch) owns the group jobs of its nb vectors
  // in order; it has no GPU work of its own.
  int nbat = 0;
  bool batch = false;
  size_t nb = 0;
  std::vector<zkmi_msm_job*> parts;
};

namespace zk {

// round-robin MSM lanes, created on first use
static int get_lane(zkmi_ctx* ctx, MsmLane** out) {
  int nl = std::max(1, ctx->msm_lanes);
  int i = ctx->lane_next++ % nl;
  while ((int)ctx->lanes.size() <= i) {
    MsmLane* l = new MsmLane;
    if (hipStreamCreateWithFlags(&l->st, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&l->fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&l->consumed, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&l->acc_done, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError();
      delete l;
      set_error("msm: cannot create a stream / events for an MSM lane");
      return ZKMI_EHIP;
    }
    ctx->lanes.push_back(l);
    ctx->nstreams++;
  }
  *out = ctx->lanes[i];
  return 0;
}

// Window / table plan of one MSM over base set tb.
struct MsmPlan {
  int c, p, W, bb, lb, hb;
  bool bal;  // balanced window widths (full tables built with them, WinLayout)
  size_t ne, Mmax;
  uint32_t B, K;
  // window-sharded plain plans: this rank's windows [w0, w0 + W) of the
  // msm_windows(c) the scalars recode into (wsel as rs_scalar_keys)
  int w0 = 0;
  uint32_t wsel = 0;
  // nb scalar vectors, sstride words apart (a single MSM: 1 and 0; batched:
  // msm_plan_batch), as nb x the single plan's windows: W, K and Mmax cover
  // every vector, ne is still one window's entries
  int nb = 1;
  size_t sstride = 0;
  int Wp() const { return wsel ? msm_windows(c) : W / nb; }  // windows per recoded scalar (per table copy)
};
static MsmPlan msm_plan(const zkmi_ctx* ctx, const zkmi_bases* tb, size_t n) {
  MsmPlan P;
  // a fixed-base table is used when the caller did not pin another window
  const bool table = tb->tc > 0 && (ctx->msm_window == 0 || ctx->msm_window == tb->tc);
  P.c = table ? tb->tc : (ctx->msm_window > 0 ? ctx->msm_window : pick_window(n));
  P.p = table ? tb->tp : 1;
  P.W = table ? tb->tw : msm_windows(P.c);  // windows actually run
  P.bal = table && tb->tbal;
  P.ne = (size_t)P.p * n;                   // entries per window
  P.Mmax = (size_t)P.W * P.ne;
  P.B = 1u << (P.c - 1);
  P.K = (uint32_t)P.W * P.B;
  P.bb = P.c - 1;
  P.lb = (P.bb + 1) / 2;
  P.hb = P.bb - P.lb;
  return P;
}
// The single plan with the batch index as an outer window (key = (batch * W +
// window) * B + ...): nb x the windows, buckets and entries; everything after
// the sort works per key and per window, so it runs unchanged on the larger
// plan and leaves nb independent sets of bit sums.
static MsmPlan msm_plan_batch(const zkmi_ctx* ctx, const zkmi_bases* tb, size_t n, int nb, size_t sstride) {
  MsmPlan P = msm_plan(ctx, tb, n);
  P.nb = nb;
  P.sstride = sstride;
  P.W *= nb;
  P.K *= (uint32_t)nb;
  P.Mmax *= (size_t)nb;
  return P;
}
static bool same_plan(const MsmPlan& a, const MsmPlan& b) {
  return a.c == b.c && a.p == b.p && a.W == b.W && a.bal == b.bal;
}
// one lane per bucket (k_acc_items_*): table plans of >= 2^18 buckets, one or
// two windows (the bin sort makes the items).  (Small table MSMs -- the
// configs[0] proof's ~8K-point MSMs, 2^12 buckets -- on this path with cap 8
// or 16: resident prove 2.95-3.02 / 3.10-3.35 ms against 2.74-2.86 ms on the
// chunked path, round 5; they stay chunked.)
// Plain (multi-window) plans take the items path too when their buckets are
// short (<= 64 entries on average: one lane per bucket keeps its waves in
// step): 2^20 plain MSM (16 windows, ~32 entries per bucket) 508-516 -> 537-538
// Mpt/s; at 2^24 (~512 per bucket) the chunked path stays faster (674-687
// against 653-656 on the items path).
static bool items_plan(const MsmPlan& P) {
  return P.K >= ITEMS_MIN_K && P.c >= 12 && P.c <= 22 && (P.W <= 2 || P.Mmax <= (size_t)64 * P.K);
}
// Piece cap of the items: no lane may run much longer than the kernel's share
// per resident lane (~M / (CUs x 768 lanes)), or its chain becomes the tail;
// buckets above it (witness-like 0/1 scalars, small scalars) are split and
// their pieces summed after (k_split_combine).
static uint32_t item_cap(const zkmi_ctx* ctx, const MsmPlan& P) {
  const size_t share = P.Mmax / ((size_t)ctx->num_cus * 768 * 2);
  // (2^20 tables: 64, 2^26: 1024)
  uint32_t cap = 64;
  while (cap < share && cap < ITEM_CAP_MAX) cap <<= 1;
  return cap;
}
// Bin-sort geometry (k_bs_*): NH bins of NLO = 2^lob keys; A / B chunks of CS
// scalars, super-chunks of 2^scs chunks; C / D tiles of <= C2 entries, T2max
// of them at most.  Counter block: bin totals [NH], item counters [16],
// super-chunk totals [BS_NSC][NH], class histogram and cursors
// [2][ITEM_CAP_MAX + 1].  A lane holds two blocks and alternates them; each
// sort's first kernel clears the other block for the next sort (its last
// readers, the previous MSM's accumulation and piece sums, ran before on the
// same stream), so a sort needs no memset launch.
struct BsGeom {
  uint32_t lob, NLO, NH, CS, nf, scs, C2, T2max;
  uint32_t nfb;  // chunks per scalar vector (nf = nfb x the plan's vectors)
  size_t nmain;  // items: NH * NLO main slots
  size_t ctr_words() const { return (size_t)NH + 16 + (size_t)BS_NSC * NH + 2 * (ITEM_CAP_MAX + 1); }
  uint32_t* ghist(uint32_t* ctr) const { return ctr + NH + 16 + (size_t)BS_NSC * NH; }
};
static BsGeom bs_geom(const MsmPlan& P, size_t n) {
  BsGeom g;
  uint32_t kb = 0;
  while ((1u << kb) < P.K) kb++;
  // lo digit: 11 bits for large key spaces; small ones keep >= 16 bins for P2's
  // parallelism and >= 64 keys per bin (the items' wave-major layout)
  g.lob = kb >= 15 ? std::min(11u, kb) : std::max(6u, kb > 4 ? kb - 4 : 0u);
  g.NLO = 1u << g.lob;
  g.NH = (P.K + g.NLO - 1) >> g.lob;
  g.CS = 1024u * (uint32_t)std::max<size_t>(1, (n + 1024ull * 2048 - 1) / (1024ull * 2048));
  g.nfb = (uint32_t)std::max<size_t>(1, (n + g.CS - 1) / g.CS);
  g.nf = g.nfb * (uint32_t)P.nb;
  g.scs = 0;
  while (((size_t)g.nf + (1u << g.scs) - 1) >> g.scs > BS_NSC) g.scs++;
  const size_t C2B = P.Mmax < ((size_t)1 << 22) ? 4096 : 16384;  // small sorts: more, shorter tiles
  g.C2 = (uint32_t)(C2B * std::max<size_t>(1, (P.Mmax + C2B * C2B - 1) / (C2B * C2B)));
  g.T2max = (uint32_t)((P.Mmax + g.C2 - 1) / g.C2) + g.NH;
  g.nmain = (size_t)g.NH * g.NLO;
  return g;
}
constexpr int BS_ST = 4096;  // k_bs_scatter2 entries per LDS sub-tile
static size_t bs_lds_scatter2(const BsGeom& g) { return rs_scatter_lds(g.NLO, BS_ST, 256) + (2 * (size_t)g.NH + 2) * 4; }

// bin sort pass 1: the count (scatter = false) or the scatter over the (chunks
// per vector, vectors) grid
static int bs_p1(int c, bool bal, hipStream_t st, const uint32_t* sc, size_t n, int Wp, uint32_t B, uint32_t wsel, const BsGeom& g,
                 uint32_t* ctr, uint32_t* next_ctr, uint32_t* choff, uint32_t* okey, uint32_t* oval, bool scatter,
                 uint32_t nb, size_t sstride) {
  uint32_t* bintot = ctr;
  uint32_t* sctot = ctr + g.NH + 16;
  const dim3 grid(g.nfb, nb);
  return dispatch_window<12>(c, bal, "bin sort: ", [&](auto C, auto BAL) {
    if (scatter)
      k_bs_scatter1<C(), 256, BAL()><<<grid, 256, rs_scatter_lds(g.NH, 256 * msm_windows(C()), 256), st>>>(
          sc, n, Wp, B, wsel, g.NH, g.lob, g.CS, g.scs, bintot, sctot, choff, reinterpret_cast<BsKey*>(okey), oval,
          sstride);
    else
      k_bs_count<C(), BAL()><<<grid, 256, g.NH * 4, st>>>(sc, n, Wp, B, wsel, g.NH, g.lob, g.CS, g.scs, bintot, sctot,
                                                         choff, next_ctr, (uint32_t)g.ctr_words(), sstride);
  });
}

// Timing ablation for development only (tools/headline_loop.py): ZKMI_DEBUG_SKIP
// bit 1 re-uses a lane's previous sort and item plan (valid only when every
// MSM on the lane has the same scalars), bit 4 skips the bucket reduction
// (results wrong).  Never set in tests or the bench.
// Compiled in only by a tools-only build (-DZK_DEBUG_ABLATE, tools/build_ab.sh):
// the shipped library ignores the variable.
static int debug_skip() {
#ifdef ZK_DEBUG_ABLATE
  static const int v = [] {
    const char* e = getenv("ZKMI_DEBUG_SKIP");
    return e ? atoi(e) : 0;
  }();
  return v;
#else
  return 0;
#endif
}

// Digits + bucket sort on the lane stream: sval (sorted entries) and bstart
// (K + 1 bucket starts) in the lane workspace.  The context stream waits only
// for the digits pass, the one reader of the scalars.
static int msm_sort_phase(zkmi_ctx* ctx, MsmLane* lane, const MsmPlan& P, const uint32_t* d_scalars, size_t n,
                          uint32_t** out_sval, uint32_t** out_bstart) {
  hipStream_t st = lane->st;
  Workspace& ws = lane->ws;
  // hi digit = top 8 bits of the key (P1: <= 256 bins, long coalesced runs);
  // lo digit = the rest (8..13 bits) inside each hi bin (P2, XCD-local)
  uint32_t kb = 0;
  while ((1u << kb) < P.K) kb++;
  // 21-bit keys (c = 22 tables): 10 hi bits, 11 lo (2^26 with the 1024-thread
  // scatters: sort 10.5 -> 9.4 ms vs 9 + 12, 13.2 ms for 8 + 13; tools/rs_lob.sh)
  const uint32_t lob = kb > 20 ? kb - 10 : kb > 16 ? kb - 8 : 8;
  const uint32_t NH = (P.K + (1u << lob) - 1) >> lob;
  const size_t Mmax = P.Mmax;
  // radix-sort geometry (see k_rs_*): ~2K P1 chunks, ~8K P2 tiles at most
  const uint32_t C1 = 16384u * (uint32_t)std::max<size_t>(1, (Mmax + 16384ull * 2048 - 1) / (16384ull * 2048));
  const uint32_t nc1 = (uint32_t)((Mmax + C1 - 1) / C1);
  const uint32_t C2b = std::max(8192u, 4u << lob);  // >= 4 entries per lo bin per tile
  const uint32_t C2 = C2b * (uint32_t)std::max<size_t>(1, (Mmax + (size_t)C2b * 8192 - 1) / ((size_t)C2b * 8192));
  const uint32_t T2max = (uint32_t)((Mmax + C2 - 1) / C2) + NH;
  const size_t len1 = (size_t)NH * nc1, len2 = (size_t)T2max << lob;
  int32_t* digits;
  uint32_t *bstart, *sval, *cnt1, *okey, *oval, *binstart, *tstart, *cnt2, *bsums, *tot;
  const bool fused = P.c >= 12 && P.c <= 22;  // the sort reads the scalars (k_bs_*, k_ss_*)
  digits = nullptr;
  if (!fused) ZK_TRY(ws.get("msm_digits", Mmax * 4, (void**)&digits));
  ZK_TRY(ws.get("msm_bstart", (size_t)(P.K + 1) * 4, (void**)&bstart));
  ZK_TRY(ws.get("msm_sval", Mmax * 4, (void**)&sval));
  const bool small = fused && Mmax <= SMALL_SORT_MAX && !items_plan(P) && P.K <= (1u << 16);
  if (!small) {
    ZK_TRY(ws.get("msm_okey", Mmax * 4, (void**)&okey));
    ZK_TRY(ws.get("msm_oval", Mmax * 4, (void**)&oval));
  }
  if (ctx->msm_fork) {
    ZK_HIP(hipStreamWaitEvent(st, ctx->msm_fork, 0));
  } else {
    ZK_HIP(hipEventRecord(lane->fork, ctx->stream));
    ZK_HIP(hipStreamWaitEvent(st, lane->fork, 0));
  }
  if ((debug_skip() & 1) && lane->debug_sorted) {
    *out_sval = sval;
    *out_bstart = bstart;
    return 0;
  }
  lane->debug_sorted = 1;
  ScopedKernelTimer tm(ctx, "msm_sort", st);
  if (fused && !small) {
    // bin sort (k_bs_*): five kernels (count, scatter1, count2, scatter2 and,
    // for one-lane-per-bucket plans, the item placement); the counter blocks
    // are cleared by the previous sort's count kernel, so a memset runs only
    // when the blocks are new or a sort was interrupted
    const BsGeom g = bs_geom(P, n);
    const bool items = items_plan(P);
    uint32_t *ctr2, *choff, *thist;
    uint4 *it = nullptr, *split = nullptr, *stage = nullptr;
    const size_t cw = g.ctr_words();
    ZK_TRY(ws.get("msm_bs_ctr", 2 * cw * 4, (void**)&ctr2));
    // a new buffer, another geometry (the blocks' layout moves) or an
    // interrupted sort: both blocks cleared
    if (ctr2 != lane->bs_ctr || cw != lane->bs_ctr_words || lane->bs_dirty) {
      ZK_HIP(hipMemsetAsync(ctr2, 0, 2 * cw * 4, st));
      lane->bs_ctr = ctr2;
      lane->bs_ctr_words = cw;
      lane->bs_parity = 0;
    }
    lane->bs_dirty = true;  // until every kernel of this sort is queued
    uint32_t* ctr = ctr2 + (size_t)lane->bs_parity * cw;
    uint32_t* next_ctr = ctr2 + (size_t)(lane->bs_parity ^ 1) * cw;
    ZK_TRY(ws.get("msm_bs_choff", (size_t)g.nf * g.NH * 4, (void**)&choff));
    ZK_TRY(ws.get("msm_bs_thist", (size_t)g.T2max * g.NLO * 4, (void**)&thist));
    ItemsOut io{nullptr, (uint32_t)g.nmain, 0, ctr + g.NH, nullptr, nullptr, g.ghist(ctr)};
    if (items) {
      io.cap = item_cap(ctx, P);
      ZK_TRY(ws.get("msm_items", (g.nmain + (Mmax + io.cap - 1) / io.cap) * 16, (void**)&it));
      ZK_TRY(ws.get("msm_split", ((Mmax + io.cap - 1) / io.cap + 1) * 16, (void**)&split));
      ZK_TRY(ws.get("msm_items_stage", g.nmain * 16, (void**)&stage));
      io.items = it;
      io.split = split;
      io.stage = stage;
    }
    ZK_TRY(bs_p1(P.c, P.bal, st, d_scalars, n, P.Wp(), P.B, P.wsel, g, ctr, next_ctr, choff, okey, oval, false,
                 (uint32_t)P.nb, P.sstride));
    ZK_TRY(bs_p1(P.c, P.bal, st, d_scalars, n, P.Wp(), P.B, P.wsel, g, ctr, next_ctr, choff, okey, oval, true,
                 (uint32_t)P.nb, P.sstride));
    ZK_HIP(hipEventRecord(lane->consumed, st));
    ZK_HIP(hipStreamWaitEvent(ctx->stream, lane->consumed, 0));
    const uint32_t gt = ((g.T2max + 7) / 8) * 8;  // XCD-mapped grid (rs_xcd_tile)
    k_bs_count2<<<gt, 256, (g.NLO + 2 * g.NH + 2 + 4) * 4, st>>>(reinterpret_cast<BsKey*>(okey), ctr, g.NH, g.lob, g.C2, g.T2max, thist);
    if (items) {
      k_bs_scatter2<BS_ST, true><<<gt, 256, bs_lds_scatter2(g), st>>>(reinterpret_cast<BsKey*>(okey), oval, ctr, g.NH, g.lob, g.C2, g.T2max,
                                                                     P.K, thist, sval, bstart, io);
      k_items_place<<<g.NH, 256, 0, st>>>(stage, g.NLO, io.cap, io.ghist, io.ghist + ITEM_CAP_MAX + 1, it,
                                          (uint32_t)g.nmain);
    } else {
      k_bs_scatter2<BS_ST, false><<<gt, 256, bs_lds_scatter2(g), st>>>(reinterpret_cast<BsKey*>(okey), oval, ctr, g.NH, g.lob, g.C2, g.T2max,
                                                                      P.K, thist, sval, bstart, io);
    }
    lane->bs_cur = ctr;  // the accumulation phases of this sort read its item counters
    lane->bs_parity ^= 1;
    lane->bs_dirty = false;
    ZK_HIP(hipGetLastError());
    *out_sval = sval;
    *out_bstart = bstart;
    return 0;
  }
  if (small) {
    uint32_t *scnt, *scur;
    ZK_TRY(ws.get("msm_ss_cnt", (size_t)P.K * 4, (void**)&scnt));
    ZK_TRY(ws.get("msm_ss_cursor", (size_t)P.K * 4, (void**)&scur));
    // the counts are left zeroed by the previous counting sort's scan on this
    // lane, up to lane->ss_clean_words; a new buffer or a larger K is cleared
    if (scnt != lane->ss_clean || P.K > lane->ss_clean_words) {
      ZK_HIP(hipMemsetAsync(scnt, 0, (size_t)P.K * 4, st));
      lane->ss_clean = scnt;
      lane->ss_clean_words = P.K;
    }
    lane->ss_clean = nullptr;  // until every kernel of this sort is queued
    ZK_TRY(small_sort(P.c, P.bal, st, d_scalars, n, P.Wp(), P.B, P.wsel, P.K, scnt, scur, bstart, sval, (uint32_t)P.nb,
                      P.sstride));
    lane->ss_clean = scnt;
    ZK_HIP(hipEventRecord(lane->consumed, st));
    ZK_HIP(hipStreamWaitEvent(ctx->stream, lane->consumed, 0));
    ZK_HIP(hipGetLastError());
    *out_sval = sval;
    *out_bstart = bstart;
    return 0;
  }
  // windows c < 12: digits array + two-pass radix sort
  ZK_TRY(ws.get("msm_cnt1", len1 * 4, (void**)&cnt1));
  ZK_TRY(ws.get("msm_cnt2", len2 * 4, (void**)&cnt2));
  ZK_TRY(ws.get("msm_binstart", (size_t)(NH + 1) * 4, (void**)&binstart));
  ZK_TRY(ws.get("msm_tstart", (size_t)(NH + 1) * 4, (void**)&tstart));
  ZK_TRY(ws.get("msm_bsums", ((std::max(len1, len2) + 1023) / 1024) * 4 + 16, (void**)&bsums));
  ZK_TRY(ws.get("msm_tot", 64, (void**)&tot));
  {
    // (no wsel here: window-sharded plans have c >= 12, so Wp() is W / nb)
    ZK_TRY(dispatch_digits(P.c, st, d_scalars, n, P.p, P.Wp(), P.bal, digits, (uint32_t)P.nb, P.sstride));
    ZK_HIP(hipEventRecord(lane->consumed, st));
    ZK_HIP(hipStreamWaitEvent(ctx->stream, lane->consumed, 0));
  }
  auto scan = [&](uint32_t* a, size_t len, uint32_t* total) {
    uint32_t nb = (uint32_t)((len + 1023) / 1024);
    k_scan_blocks<<<nb, 256, 0, st>>>(a, (uint32_t)len, a, bsums);
    k_scan_top<<<1, 1024, 0, st>>>(bsums, nb, total);
    k_scan_add<<<(unsigned)((len + 255) / 256), 256, 0, st>>>(a, (uint32_t)len, bsums, nullptr);
  };
  const uint32_t ne = (uint32_t)P.ne;
  k_rs_p1_count<<<nc1, RS_THREADS, NH * 4, st>>>(digits, Mmax, ne, P.B, NH, lob, C1, nc1, cnt1);
  scan(cnt1, len1, &tot[0]);
  k_rs_p1_scatter<4096><<<nc1, RS_THREADS, rs_scatter_lds(NH, 4096), st>>>(digits, Mmax, ne, P.B, NH, lob, C1, nc1,
                                                                           cnt1, okey, oval);
  k_rs_tiles<<<1, 1024, 0, st>>>(cnt1, nc1, NH, &tot[0], C2, binstart, tstart);
  // cnt2 needs no clearing: tiles t < tstart[NH] write all their counts, and
  // the stale tail after them only reaches the (unused) scan total
  const uint32_t g2 = ((T2max + 7) / 8) * 8;  // XCD-mapped grid (rs_xcd_tile)
  k_rs_p2_count<<<g2, RS_THREADS, (1u << lob) * 4, st>>>(okey, binstart, tstart, NH, lob, C2, T2max, cnt2);
  scan(cnt2, len2, &tot[1]);
  k_rs_bstart<<<(P.K + 256) / 256, 256, 0, st>>>(cnt2, binstart, tstart, NH, lob, P.K, bstart);
  const uint32_t NLO = 1u << lob;
  // 1024-thread P2 workgroups over 8192-entry sub-tiles (runs twice as long
  // per lo bin as 4096; 2^20 table MSM, 3 lanes: 1.344 -> 1.297 ms with the
  // 1024-thread P1; tools/rs_ab2.sh)
#define ZK_P2(ST, T) \
  k_rs_p2_scatter<ST, T><<<g2, T, rs_scatter_lds(NLO, ST, T), st>>>(okey, oval, binstart, tstart, NH, lob, C2, T2max, cnt2, sval)
  if (rs_scatter_lds(NLO, 8192, 1024) <= 160 * 1024) ZK_P2(8192, 1024);
  else ZK_P2(4096, 1024);
#undef ZK_P2
  ZK_HIP(hipGetLastError());
  *out_sval = sval;
  *out_bstart = bstart;
  return 0;
}

// Bucket-reduction geometry of a plan.
//   mode 1 (windows with rows / columns of >= 2^9 buckets, i.e. the >= 2^18
//     bucket tables): k_msm_br_strip waves of 8 (G1) / 16 (G2) buckets per
//     lane and a 6-level in-wave tree.  Every level runs at 1-2 waves per
//     SIMD, where one full XYZZ addition takes ~15-20 us (vs ~5.5 us of issue
//     at 4+ waves): the ~19 dependent additions from 2^19 buckets to the bit
//     sums set the isolated time.
//   mode 0 (smaller windows): <= 256-bucket strided wave jobs (k_msm_br).
// Bit sums: sb segments of segt terms each (the longest bit job sums
// max(2^hb * sr, 2^(lb-1) * sc) terms); the host adds the segments.  Shorter
// segments cut the bit kernel's chain of dependent additions (it runs 20-40
// waves on an otherwise idle chip) for a few more host additions.
struct BrGeom {
  int mode;
  int sr, sc, sb, segt;
  int mc = 64;  // mode 1: lanes per column segment (k_msm_br_strip)
};
static BrGeom br_geom(const MsmPlan& P, bool g2, bool pipelined) {
  // buckets folded per lane before the tree: G2 16 (2^20 G2 MSM, 2 lanes:
  // 4.50 -> 4.17 ms).  G1: 8 on one lane, where the reduction's latency is
  // exposed (16 with two 512-bucket columns per wave: 2^20 one lane 1.56 ->
  // 1.62 ms per MSM); 16 when several lanes are in flight, where the
  // reduction runs beside another lane's accumulation and what it costs is
  // its VALU issue -- the in-wave tree's idle lanes -- rather than its latency
  // (22K instead of 29K wave-additions per 2^19-bucket window: 2^20 table
  // MSM, 3 lanes 895-897 -> 906-909 Mpt/s, 2 lanes 886-890 -> 911).  A sharded
  // MSM keeps 8 on every rank: the bit-sum segments are part of the
  // exchanged plan.
#ifndef ZK_BR_FOLD_G1
#define ZK_BR_FOLD_G1 8
#endif
  // (pipelined fold 32 -- 32-bucket column strips, 16 lanes per column --
  // measured level: 887-903 vs 886-900 Mpt/s)
  const int fold = g2 || pipelined ? 16 : ZK_BR_FOLD_G1;
  BrGeom g;
  g.mode = P.hb >= 9 ? 1 : 0;
  g.segt = 256;
  const int segb = g.mode == 1 ? 64 * fold : 256;  // buckets per wave job
  g.sr = (1 << P.lb) > segb ? (1 << P.lb) / segb : 1;
  g.sc = (1 << P.hb) > segb ? (1 << P.hb) / segb : 1;
  // lanes per column segment: as many as keep `fold` buckets per lane
  const int lenc = (1 << P.hb) / g.sc;
  g.mc = 64;
  while (g.mc > 1 && lenc / g.mc < fold) g.mc >>= 1;
  const uint32_t maxterms = std::max((1u << P.hb) * g.sr, (1u << (P.lb - 1)) * g.sc);
  g.sb = (int)((maxterms + g.segt - 1) / g.segt);
  return g;
}

// Sharded MSMs hand over exactly SHARD_PAYLOAD_WORDS u32 per rank: a status
// block [failure flag, plan signature (g2, c, bit sums), segments, windows]
// and the rank's bit sums after it.  The size is the same on every rank
// whatever its plan, inputs or local failure, so every sharded submit is one
// collective of one size on every rank and no rank can wait in a collective
// another rank skips; msm_wait fails on every rank when the plans of the
// non-empty shards differ.  36,864 words hold every table plan (<= 22.5K
// words) and the plain plans of windows <= 20 (<= 34.6K words for G2).
constexpr size_t SHARD_PAYLOAD_WORDS = 36864;
// word 1 of a rank's status block: 0x5A | window-sharded (bit 17) | g2 (bit 16) | c | bit sums
static uint32_t shard_sig0(int g2, int c, int bb, bool wmode = false) {
  return 0x5A000000u | ((uint32_t)wmode << 17) | ((uint32_t)g2 << 16) | ((uint32_t)c << 8) | (uint32_t)bb;
}
__global__ void k_put_words(uint32_t* __restrict__ dst, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3) {
  if (threadIdx.x < 4) dst[threadIdx.x] = threadIdx.x == 0 ? w0 : threadIdx.x == 1 ? w1 : threadIdx.x == 2 ? w2 : w3;
}

// Queue the hand-over of a job's bit sums on stream st (the lane stream):
// d_buf holds a SHARD_STATUS_WORDS status block, then `words` u32 of bit sums
// (W*(bb+1)*sb XYZZ terms; 0 for an empty shard).  Unsharded: the D2H of the
// bit sums into the job's pinned buffer and the job's event.  Sharded: the
// status block first; over RCCL the all-gather of every rank's payload (comm
// stream, ordered after the lane's work) and one strided D2H of every rank's
// status block + bit sums; over a host transport the D2H of this rank's part
// (msm_wait exchanges it).
static int msm_queue_handover(zkmi_ctx* ctx, MsmLane* lane, hipStream_t st, zkmi_msm_job* job, uint32_t* d_buf,
                              size_t words) {
  ZK_HIP(hipEventCreateWithFlags(&job->done, hipEventDisableTiming));
  if (!job->comm) {
    job->host_words = words;
    ZK_TRY(ctx_pinned_get(ctx, words * 4, (void**)&job->host));
    job->st = st;  // from here on the pinned buffer may have a copy in flight
    ZK_HIP(hipMemcpyAsync(job->host, d_buf + SHARD_STATUS_WORDS, words * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipEventRecord(job->done, st));
    job->done_rec = true;
    return 0;
  }
  const int nr = job->comm->nranks;
  const bool empty = words == 0;
  k_put_words<<<1, 64, 0, st>>>(d_buf, 0u, shard_sig0(job->g2, empty ? 0 : job->c, empty ? 0 : job->bb, job->wmode),
                                empty ? 0u : (uint32_t)job->sb,
                                empty ? 0u : (uint32_t)job->W | ((uint32_t)job->w0 << 16));
  ZK_HIP(hipGetLastError());
  // what msm_wait reads of each rank: status + bit sums of this rank's plan
  // (the plan every non-empty point shard must share); everything for an
  // empty shard or a window-sharded MSM (whose ranks hold different counts)
  const size_t width = empty || job->wmode ? SHARD_PAYLOAD_WORDS : SHARD_STATUS_WORDS + words;
  if (job->comm->kind == ZKMI_COMM_RCCL) {
    uint32_t* gathered;
    ZK_TRY(lane->ws.get("msm_gathered", (size_t)nr * SHARD_PAYLOAD_WORDS * 4, (void**)&gathered));
    ZK_TRY(comm_allgather_device(job->comm, st, d_buf, gathered, SHARD_PAYLOAD_WORDS * 4));
    job->exchanged = true;
    job->host_words = width;
    ZK_TRY(ctx_pinned_get(ctx, (size_t)nr * width * 4, (void**)&job->host));
    job->st = st;
    ZK_HIP(hipMemcpy2DAsync(job->host, width * 4, gathered, SHARD_PAYLOAD_WORDS * 4, width * 4, nr,
                            hipMemcpyDeviceToHost, st));
  } else {
    job->host_words = SHARD_PAYLOAD_WORDS;  // the host all-gather sends the whole payload
    ZK_TRY(ctx_pinned_get(ctx, SHARD_PAYLOAD_WORDS * 4, (void**)&job->host));
    job->st = st;
    ZK_HIP(hipMemcpyAsync(job->host, d_buf, width * 4, hipMemcpyDeviceToHost, st));
  }
  ZK_HIP(hipEventRecord(job->done, st));
  job->done_rec = true;
  return 0;
}

// Bucket accumulation + reduction of one base set over a sorted entry list,
// on the lane stream; queues the D2H of the bit sums and the job's event.
template <class G>
static int msm_acc_phase(zkmi_ctx* ctx, MsmLane* lane, const MsmPlan& P, const zkmi_bases* tb, size_t offset,
                         size_t n, const uint32_t* sval, const uint32_t* bstart, zkmi_msm_job* job) {
  constexpr int XW = 4 * G::CW;
  using GS = std::conditional_t<G::CW == 8, G1Tn, G>;  // the small-MSM kernels' trait
  using GB = G;  // (the compiler-scheduled GS products lost here: 3-lane 2^20 862 -> 846-853 Mpt/s)
  hipStream_t st = lane->st;
  Workspace& ws = lane->ws;
  const uint32_t* d_bases = tb->d_pts + offset * G::PW;
  const uint32_t K = P.K;
  const int W = P.W, bb = P.bb, lb = P.lb, hb = P.hb;
  const size_t Mmax = P.Mmax;
  const uint32_t tn = (uint32_t)n, tskip = P.p > 1 ? (uint32_t)(tb->n - n) : 0u;
  uint32_t* buckets;
  ZK_TRY(ws.get("msm_buckets", (size_t)K * XW * 4, (void**)&buckets));
  if (items_plan(P)) {  // table plans (one window of many buckets)
    // one lane per bucket (k_acc_items); the items, the split list and their
    // counters come from the sort (k_bs_scatter2)
    const BsGeom g = bs_geom(P, n);
    const uint32_t cap = item_cap(ctx, P);
    const size_t npieces = (Mmax + cap - 1) / cap;
    const size_t items_max = g.nmain + npieces;
    uint32_t* ctr = lane->bs_cur;  // the counter block of this lane's last sort
    uint32_t* xpts;
    uint4 *items, *split;
    ZK_TRY(ws.get("msm_items", items_max * 16, (void**)&items));
    ZK_TRY(ws.get("msm_split", (npieces + 1) * 16, (void**)&split));
    ZK_TRY(ws.get("msm_xpts", (2 * npieces + 2) * XW * 4, (void**)&xpts));
    const uint32_t* itc = ctr + g.NH;  // [0] overflow items, [1] partial slots, [2] split buckets
    // Table accumulations start in submission order across lanes: this one
    // waits for the previous one (on another lane) to end.  Run together, two
    // accumulations share the CUs and end together, and the lanes' tails and
    // sorts then queue up behind both; chained, the earlier MSM's tail starts
    // a full accumulation sooner.  Measured (interleaved, one box): bench
    // headline 822-825 -> 832-840 Mpt/s, configs[0] resident 2.82-2.86 ->
    // 2.78-2.80 ms, 2^20 / 2^26 loops and the proof legs level.  (Also chaining the bucket
    // reduction, with 256-thread sorts that fit beside the accumulation:
    // 2^26 steady state 64.5 -> 62 ms per MSM, but the accumulation ran 13%
    // longer beside the sort, short runs lost and 2^20 lost 8%.)
    if (ctx->acc_last && ctx->acc_last != lane) ZK_HIP(hipStreamWaitEvent(st, ctx->acc_last->acc_done, 0));
    {
      ScopedKernelTimer tm(ctx, G::CW == 8 ? "msm_acc0_g1" : "msm_acc0_g2", st);
#ifndef ZK_ACC_VPAD_LOG
#define ZK_ACC_VPAD_LOG 27
#endif
      const bool vpad = G::CW == 8 && Mmax >= ((size_t)1 << std::min(ZK_ACC_VPAD_LOG, 63));
      auto kern = G::CW == 8 ? (vpad ? k_acc_items_g1<true> : k_acc_items_g1<false>) : k_acc_items_g2;
#ifndef ZK_ACC_LDS_B
#define ZK_ACC_LDS_B 41984
#endif
      // 41 KB of (unused) LDS per G1 accumulation workgroup caps it at three
      // workgroups per CU -- three of its 127-VGPR waves per SIMD instead of
      // four -- and leaves each SIMD a wave slot the other lanes' sorts and
      // reductions start in at once, instead of waiting for accumulation
      // workgroups to retire.  Measured (2^20 table MSM): one lane level
      // (1.552-1.567 vs 1.557 ms, the accumulation is issue-bound at three
      // waves), 3 lanes 851-861 -> 886-908 Mpt/s, 2 lanes 753-757 -> 879-899.
      // (G2's 252-VGPR waves are two per SIMD either way.)
      const size_t acc_lds = G::CW == 8 && !vpad ? (size_t)ZK_ACC_LDS_B : 0;
      kern<<<(unsigned)((items_max + 255) / 256), 256, acc_lds, st>>>(
          items, &itc[0], (uint32_t)g.nmain, sval, d_bases, tn, tskip, buckets, xpts);
    }
    ZK_HIP(hipEventRecord(lane->acc_done, st));
    ctx->acc_last = lane;
    ScopedKernelTimer tm(ctx, "msm_accN", st);
    auto comb = K <= CUTSUM_COOP_K ? k_split_combine<GS> : k_split_combine<GB>;  // small MSMs: latency-scheduled products
    // one wave per split bucket in one pass up to 4096 of them (a small MSM's
    // buckets at cap 8 are all split); the launch reads the count and exits
    // when there is none
    const size_t maxsplit = std::min<size_t>(K, npieces / 2 + 1);
    comb<<<(unsigned)std::min<size_t>((maxsplit + 3) / 4, 1024), 256, 0, st>>>(split, &itc[2], xpts, buckets);
    ZK_HIP(hipGetLastError());
  } else {
    uint32_t *flags, *xkey, *xvalid, *xpts, *ykey, *yvalid, *ypts;
    ZK_TRY(ws.get("msm_flags", 64 * 4, (void**)&flags));  // zeroed by the accumulation's block 0
    // level 0: fixed-size chunks of the sorted list (sized from the upper bound
    // W*n so no host round-trip is needed; chunks past M exit at once).
    // Threads per CU: measured best at ~1024 for G1 (over-subscribing the
    // resident waves evens out per-thread run lengths).
    const size_t tpc = 1024;
    const size_t acc_threads = (size_t)ctx->num_cus * tpc;
    uint32_t L = (uint32_t)std::max<size_t>(4, (Mmax + acc_threads - 1) / acc_threads);
    uint32_t nch = (uint32_t)((Mmax + L - 1) / L);
    const size_t xl = 2 * (size_t)nch + 1;  // length of the partial list the segmented cascade starts from
    ZK_TRY(ws.get("msm_xkey", xl * 4 + 64, (void**)&xkey));
    ZK_TRY(ws.get("msm_xvalid", xl * 4 + 64, (void**)&xvalid));
    ZK_TRY(ws.get("msm_xpts", (xl + 2) * XW * 4, (void**)&xpts));
    ZK_TRY(ws.get("msm_ykey", xl * 4 + 64, (void**)&ykey));
    ZK_TRY(ws.get("msm_yvalid", xl * 4 + 64, (void**)&yvalid));
    ZK_TRY(ws.get("msm_ypts", (xl + 2) * XW * 4, (void**)&ypts));
    {
      ScopedKernelTimer tm(ctx, G::CW == 8 ? "msm_acc0_g1" : "msm_acc0_g2", st);
      Acc0Kernel<G>::fn<<<(nch + 255) / 256, 256, 0, st>>>(sval, bstart, K, L, nch, d_bases, tn, tskip, buckets, xkey,
                                                            xvalid, xpts, flags);
      ZK_HIP(hipGetLastError());
    }
    ScopedKernelTimer tm(ctx, "msm_accN", st);
    // Small MSMs (ZK_SMALL_SPLIT): the buckets cut by more than 16 chunk edges
    // (a witness MSM's small digits) are listed by the cut sums and summed by
    // k_split_combine in one launch -- a block-wide tree per bucket -- instead
    // of the k_msm_accN cascade's ~7 launches, most of which exit at once.
    // Measured (round 6, one box, 3 interleaved repeats of tools/small_prove.py):
    // configs[0] resident prove 1.754-1.768 -> 1.536-1.579 ms, same proof bytes.
#ifndef ZK_SMALL_SPLIT
#define ZK_SMALL_SPLIT 1
#endif
    if (ZK_SMALL_SPLIT && K <= CUTSUM_COOP_K) {
      const size_t maxsplit = std::min<size_t>(K, nch / 16 + 1);
      uint4* split;
      ZK_TRY(ws.get("msm_small_split", maxsplit * 16, (void**)&split));
      k_msm_cutsum_coop<GS><<<(unsigned)(((size_t)K * 16 + 255) / 256), 256, 0, st>>>(bstart, K, L, buckets, xvalid,
                                                                                   xpts, &flags[0], split, &flags[32]);
      k_split_combine<GS, true><<<(unsigned)std::min<size_t>((maxsplit + 3) / 4, 256), 256, 0, st>>>(split, &flags[32],
                                                                                                  xpts, buckets);
      ZK_HIP(hipGetLastError());
    } else {
    if (K <= CUTSUM_COOP_K)
      k_msm_cutsum_coop<GS><<<(unsigned)(((size_t)K * 16 + 255) / 256), 256, 0, st>>>(bstart, K, L, buckets, xvalid,
                                                                                   xpts, &flags[0]);
    else
      k_msm_cutsum<G><<<(K + 255) / 256, 256, 0, st>>>(bstart, K, L, buckets, xvalid, xpts, &flags[0]);
    // segmented reduction of the remaining partials: level 1 pairs neighbours,
    // deeper levels only carry heavy buckets; each level exits on device when
    // the previous one left nothing open (no host round-trips)
    uint32_t cur_len = (uint32_t)xl;
    for (int level = 1; cur_len > 1; level++) {
      if (level >= 63) {
        set_error("msm: segmented reduction schedule too deep");
        return ZKMI_EINVAL;
      }
      // (a level maps cur_len to 2 ceil(cur_len / Ll) + 1, so Ll >= 5 to shrink)
      const bool coop = level > 1 && K <= CUTSUM_COOP_K;  // small MSMs: 16-lane segmented scans
      uint32_t Ll = level == 1 ? 2 : 16;
      uint32_t nc = (cur_len + Ll - 1) / Ll;
      if (coop)
        k_msm_accN_coop<GS><<<(unsigned)(((size_t)nc * 16 + 255) / 256), 256, 0, st>>>(
            xkey, xvalid, xpts, cur_len, nc, buckets, ykey, yvalid, ypts, &flags[level - 1], &flags[level]);
      else
        k_msm_accN<G><<<(nc + 255) / 256, 256, 0, st>>>(xkey, xvalid, xpts, cur_len, Ll, nc, buckets, ykey, yvalid,
                                                        ypts, &flags[level - 1], &flags[level]);
      std::swap(xkey, ykey);
      std::swap(xvalid, yvalid);
      std::swap(xpts, ypts);
      cur_len = nc == 1 ? 1 : 2 * nc + 1;
    }
    ZK_HIP(hipGetLastError());
    }
  }
  // bucket reduction -> W*(bb+1) canonical bit sums.  (Tried: the reduction
  // and hand-over on a second stream with double-buffered buckets, so the
  // lane goes on to the next sort: 1.31 -> 1.57 ms per 2^20 MSM with a br
  // stream per lane -- more streams than the box's 4 hardware queues -- and
  // 1.37 ms with one shared br stream.)
  hipStream_t brs = st;
  uint32_t *Cb, *Db, *sums;
  const BrGeom bg = br_geom(P, G::CW != 8, ctx->msm_lanes > 1 && !job->comm);
  const int sr = bg.sr, sc = bg.sc, sb = bg.sb;
  ZK_TRY(ws.get("msm_C", (size_t)W * (1u << hb) * sr * XW * 4, (void**)&Cb));
  ZK_TRY(ws.get("msm_D", (size_t)W * (1u << lb) * sc * XW * 4, (void**)&Db));
  // status block (sharded hand-over) + bit sums; a sharded payload is exchanged whole
  const size_t sum_words = (size_t)W * (bb + 1) * sb * XW;
  ZK_TRY(ws.get("msm_sums", std::max(sum_words + SHARD_STATUS_WORDS, job->comm ? SHARD_PAYLOAD_WORDS : 0) * 4,
                (void**)&sums));
  if (!(debug_skip() & 4)) {
    ScopedKernelTimer tm(ctx, "msm_bucket_reduce", brs);
    uint32_t jobs2 = (uint32_t)W * (bb + 1) * sb;
    if (bg.mode == 1) {  // one wave per row segment, 64 / mc column segments per wave
      const uint32_t nrow = (uint32_t)W * ((1u << hb) * sr), ncol = (uint32_t)W * ((1u << lb) * sc);
      const uint32_t cpw = 64u / (uint32_t)bg.mc;
      const uint32_t jobs1 = nrow + (ncol + cpw - 1) / cpw;
      k_msm_br_strip<GB><<<(jobs1 + 3) / 4, 256, 0, brs>>>(buckets, bstart, lb, hb, W, sr, sc, bg.mc, Cb, Db);
    } else {
      uint32_t jobs1 = (uint32_t)W * (((1u << hb) * sr) + ((1u << lb) * sc));
      auto br1 = K <= CUTSUM_COOP_K ? k_msm_br<GS, false> : k_msm_br<G, false>;
      br1<<<(jobs1 + 3) / 4, 256, 0, brs>>>(buckets, nullptr, bstart, lb, hb, W, sr, sc, sb, 256, Cb, Db);
    }
    auto br2 = K <= CUTSUM_COOP_K ? k_msm_br<GS, true> : k_msm_br<GB, true>;
    br2<<<(jobs2 + 3) / 4, 256, 0, brs>>>(Cb, Db, nullptr, lb, hb, W, sr, sc, sb, bg.segt,
                                          sums + SHARD_STATUS_WORDS, nullptr);
    ZK_HIP(hipGetLastError());
  }
  job->sb = sb;
  return msm_queue_handover(ctx, lane, brs, job, sums, sum_words);
}

static int msm_acc_any(zkmi_ctx* ctx, MsmLane* lane, const MsmPlan& P, const zkmi_bases* tb, size_t offset, size_t n,
                       const uint32_t* sval, const uint32_t* bstart, zkmi_msm_job* job) {
  if (ctx->acc_gate && tb == ctx->acc_gate_set) ZK_HIP(hipStreamWaitEvent(lane->st, ctx->acc_gate, 0));
  return tb->g2 ? msm_acc_phase<G2T>(ctx, lane, P, tb, offset, n, sval, bstart, job)
                : msm_acc_phase<G1T>(ctx, lane, P, tb, offset, n, sval, bstart, job);
}

static zkmi_msm_job* new_job(zkmi_ctx* ctx, const zkmi_bases* b, const MsmPlan& P, size_t n) {
  zkmi_msm_job* j = new zkmi_msm_job{ctx, b->g2, P.c, P.W, P.bb, nullptr, 0, nullptr, n == 0};
  j->wmode = P.wsel != 0;
  j->w0 = P.w0;
  return j;
}

static int check_size(const MsmPlan& P, size_t n) {
  if (P.ne >= (1u << 31) || P.Mmax >= (1ull << 32)) {
    set_error("MSM size %zu too large for one call", n);
    return ZKMI_EINVAL;
  }
  return 0;
}

static int check_range(const zkmi_bases* b, size_t offset, size_t n) {
  if (!b || offset > b->n || n > b->n - offset) {
    set_error("msm: range [%zu, %zu) outside base set of %zu", offset, offset + n, b ? b->n : 0);
    return ZKMI_EINVAL;
  }
  return 0;
}

int msm_submit(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const void* d_scalars, size_t n,
               zkmi_msm_job** job) {
  zkmi_msm_job* jobs[1] = {nullptr};
  int rc = msm_submit_shared(ctx, &b, 1, offset, d_scalars, n, jobs);
  *job = jobs[0];
  return rc;
}

// The same nb scalar vectors (n > 0 scalars each, sstride words apart) over k
// base sets: one digits + sort pass on the next lane, then one accumulation
// per set with the same plan; base sets whose window plan differs from the
// first one's get their own sort.  own(j, P) makes set j's job for plan P and
// hands it to whoever frees the jobs, before its accumulation is queued.
template <class Own>
static int msm_sort_acc_shared(zkmi_ctx* ctx, const zkmi_bases* const* bs, int k, size_t offset, const uint32_t* sc,
                               size_t n, int nb, size_t sstride, Own own) {
  std::vector<bool> done(k, false);
  for (int i = 0; i < k; i++) {
    if (done[i]) continue;
    const MsmPlan P = msm_plan_batch(ctx, bs[i], n, nb, sstride);
    ZK_TRY(check_size(P, n));
    MsmLane* lane = nullptr;
    ZK_TRY(get_lane(ctx, &lane));
    uint32_t *sval, *bstart;
    ZK_TRY(msm_sort_phase(ctx, lane, P, sc, n, &sval, &bstart));
    for (int j = i; j < k; j++) {
      if (done[j] || (j > i && !same_plan(P, msm_plan_batch(ctx, bs[j], n, nb, sstride)))) continue;
      zkmi_msm_job* job = own(j, P);
      done[j] = true;
      ZK_TRY(msm_acc_any(ctx, lane, P, bs[j], offset, n, sval, bstart, job));
    }
  }
  return 0;
}

// k MSMs with the same scalars (and range) over k base sets (msm_sort_acc_shared)
int msm_submit_shared(zkmi_ctx* ctx, const zkmi_bases* const* bs, int k, size_t offset, const void* d_scalars,
                      size_t n, zkmi_msm_job** jobs) {
  for (int i = 0; i < k; i++) jobs[i] = nullptr;
  for (int i = 0; i < k; i++) ZK_TRY(check_range(bs[i], offset, n));
  if (n == 0) {
    for (int i = 0; i < k; i++) jobs[i] = new_job(ctx, bs[i], msm_plan(ctx, bs[i], n), n);
    return 0;
  }
  const int rc = msm_sort_acc_shared(ctx, bs, k, offset, (const uint32_t*)d_scalars, n, 1, 0,
                                     [&](int j, const MsmPlan& P) { return jobs[j] = new_job(ctx, bs[j], P, n); });
  if (rc) {
    for (int i = 0; i < k; i++) {
      msm_job_free(jobs[i]);
      jobs[i] = nullptr;
    }
  }
  return rc;
}

// A job freed on an error path may still have the D2H of its bit sums in
// flight into its pinned buffer: wait for the lane before the buffer goes back
// to the pool, or a later MSM that reuses it could have its bit sums
// overwritten by the stale copy.
void msm_job_free(zkmi_msm_job* job) {
  if (!job) return;
  for (zkmi_msm_job* part : job->parts) msm_job_free(part);
  job->parts.clear();
  // (the event, not the stream: a lane released by zkmi_comm_init after its
  // work -- comm.hip stream budget -- may be gone while its jobs are unwaited)
  if (job->host && job->st) {
    if ((job->done_rec ? hipEventSynchronize(job->done) : hipStreamSynchronize(job->st)) != hipSuccess) {
      (void)hipGetLastError();
      job->host = nullptr;  // state unknown: drop the buffer rather than recycle it
    }
  }
  if (job->done) hipEventDestroy(job->done);
  if (job->host) ctx_pinned_put(job->ctx, job->host);
  delete job;
}

int msm_wait(zkmi_msm_job* job, uint64_t* out) {
  if (!job) {
    set_error("msm_wait: null job");
    return ZKMI_EINVAL;
  }
  if (job->batch || job->nbat) {  // the job stays valid
    set_error("msm_wait: a batch job is finished with zkmi_msm_batch_wait");
    return ZKMI_EINVAL;
  }
  zkmi_ctx* ctx = job->ctx;
  ZK_DEVICE_GUARD(ctx);
  int PW = job->g2 ? 32 : 16, XW = 2 * PW;
  if (job->fail_rc) {  // host transport: this rank's failure joins the exchange here, in wait order
    const int frc = job->fail_rc;
    (void)comm_fail_exchange(job->comm, SHARD_PAYLOAD_WORDS);
    set_error("%s", job->fail_msg.c_str());
    msm_job_free(job);
    return frc;
  }
  if (job->empty) {
    memset(out, 0, PW * 4);
    msm_job_free(job);
    return 0;
  }
  hipError_t e = hipEventSynchronize(job->done);
  if (e != hipSuccess) {
    set_error("msm_wait: %s", hipGetErrorString(e));
    // a host-transport peer waits for this rank's bit sums: hand it a failure
    if (job->comm && job->comm->kind == ZKMI_COMM_HOST) (void)comm_fail_exchange(job->comm, job->host_words);
    job->host = nullptr;  // copy state unknown: never recycle the buffer
    msm_job_free(job);
    return ZKMI_EHIP;
  }
  job->st = nullptr;  // the bit-sum copy has landed
  int rc = timer_flush(ctx, false);
  auto th0 = std::chrono::steady_clock::now();
  // Sharded MSM: every rank's status block + bit sums (rank-major, host_words
  // each).  Over RCCL they were all-gathered on the device before the D2H;
  // over a host transport the exchange happens here.
  const int nr = job->comm ? job->comm->nranks : 1;
  const uint32_t* src = job->host;
  std::vector<uint32_t> gathered;
  std::vector<int> live_ranks;  // ranks whose bit sums enter the sum
  if (job->comm && job->comm->kind == ZKMI_COMM_HOST) {
    gathered.resize((size_t)nr * job->host_words);
    const auto tx = std::chrono::steady_clock::now();
    int grc = comm_allgather_host(job->comm, job->host, gathered.data(), job->host_words * 4);
    if (ctx->timer.enabled) {  // per-rank exchange time, as the RCCL path's event timer
      auto& t = ctx->timer.totals["msm_exchange"];
      t.first += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tx).count();
      t.second += 1;
    }
    if (grc) {
      msm_job_free(job);
      return grc;
    }
    src = gathered.data();
  }
  if (job->comm) {  // one failed rank fails the MSM everywhere; non-empty shards must share one plan
    const uint32_t* ref = nullptr;
    for (int r = 0; r < nr; r++) {
      const uint32_t* stw = src + (size_t)r * job->host_words;
      if (stw[0] != 0) {
        set_error("msm_sharded: rank %d failed while running its shard", r);
        msm_job_free(job);
        return ZKMI_EINVAL;
      }
      if ((stw[1] >> 16) != (0x5A00u | ((uint32_t)job->wmode << 1) | (uint32_t)job->g2)) {
        set_error("msm_sharded: rank %d runs a %s MSM (or is out of step)", r, job->g2 ? "G1" : "G2");
        msm_job_free(job);
        return ZKMI_EINVAL;
      }
      if (((stw[1] >> 8) & 0xFF) == 0) continue;  // empty shard
      if (!ref) {
        ref = stw;
      } else if (memcmp(ref + 1, stw + 1, (job->wmode ? 2 : 3) * sizeof(uint32_t)) != 0) {
        set_error("msm_sharded: window plans differ between ranks (c %u/%u, windows %u/%u): use equal shards "
                  "and the same fixed-base table and window setting on every rank",
                  (ref[1] >> 8) & 0xFF, (stw[1] >> 8) & 0xFF, ref[3], stw[3]);
        msm_job_free(job);
        return ZKMI_EINVAL;
      }
      live_ranks.push_back(r);
    }
    if (!ref) {  // every shard empty: the sum is infinity
      memset(out, 0, PW * 4);
      msm_job_free(job);
      return rc;
    }
    job->c = (int)((ref[1] >> 8) & 0xFF);
    job->bb = (int)(ref[1] & 0xFF);
    job->sb = (int)ref[2];
    job->W = job->wmode ? msm_windows(job->c) : (int)(ref[3] & 0xFFFF);
    for (int r : live_ranks) {  // every rank's part fits the payload; window shards tile [0, W) exactly once
      const uint32_t w3 = src[(size_t)r * job->host_words + 3];
      if ((size_t)(w3 & 0xFFFF) * (job->bb + 1) * job->sb * XW + SHARD_STATUS_WORDS > job->host_words) {
        set_error("msm_sharded: the agreed plan does not fit the exchanged payload");
        msm_job_free(job);
        return ZKMI_EINVAL;
      }
    }
    if (job->wmode) {
      std::vector<int> cover(job->W, 0);
      for (int r : live_ranks) {
        const uint32_t w3 = src[(size_t)r * job->host_words + 3];
        for (uint32_t w = w3 >> 16; w < (w3 >> 16) + (w3 & 0xFFFF) && w < (uint32_t)job->W; w++) cover[w]++;
      }
      for (int w = 0; w < job->W; w++)
        if (cover[w] != 1) {
          set_error("msm_window_sharded: window %d is covered by %d ranks (every rank must split the same "
                    "window plan)", w, cover[w]);
          msm_job_free(job);
          return ZKMI_EINVAL;
        }
    }
  } else {
    live_ranks.push_back(0);
  }
  const size_t skip = job->comm ? SHARD_STATUS_WORDS : 0;  // status block before each rank's bit sums
  // terms: V_{c w + j} = U_{w,j} (j < c-1), then T_w at weight 2^{c w}
  // (each term arrives as sb segments per rank, all summed in the combine)
  msm_host_assemble_combine(src, job->host_words, skip, live_ranks.data(), (int)live_ranks.size(), job->wmode,
                            job->g2, job->c, job->W, job->bb, job->sb, out);
  if (ctx->timer.enabled) {
    auto& t = ctx->timer.totals["msm_host_epilogue"];
    t.first += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
    t.second += 1;
  }
  msm_job_free(job);
  return rc;
}

int msm_device(zkmi_ctx* ctx, const zkmi_bases* b, size_t offset, const void* d_scalars, size_t n,
               uint64_t* out_affine) {
  zkmi_msm_job* job;
  ZK_TRY(msm_submit(ctx, b, offset, d_scalars, n, &job));
  return msm_wait(job, out_affine);
}

// ------------------------------------------------------------ batched MSMs
// nb scalar vectors over one base set and range (zkmi_msm_batch_submit): the
// vectors are split into groups of at most G; a group is ONE launch sequence
// over the plan msm_plan_batch makes of it, on the next lane, so groups
// pipeline the way consecutive MSMs do.  A group of one is the single MSM's
// plan and launches.
//
// Group size: zkmi_ctx_set_batch_group, or BATCH_GROUP_AUTO; then the largest
// g <= that for which the batched plan keeps K' <= BATCH_K_MAX buckets and
// Mmax' <= BATCH_M_MAX entries (sort workspace 4 arrays x Mmax' x 4 B <= 1 GB
// per lane, inside check_size's 2^32) and does not take the one-lane-per-bucket
// (items) path: a plan that takes that path alone already fills the part, and
// its item geometry is sized for one or two windows, so such MSMs run as
// pipelined single MSMs (g = 1).
constexpr int BATCH_GROUP_AUTO = 16;
constexpr uint32_t BATCH_K_MAX = 1u << 20;
constexpr size_t BATCH_M_MAX = (size_t)1 << 26;
static int msm_batch_group(const zkmi_ctx* ctx, const zkmi_bases* b, size_t n, size_t nb) {
  int g = ctx->batch_group > 0 ? ctx->batch_group : BATCH_GROUP_AUTO;
  if ((size_t)g > nb) g = (int)nb;
  if (g < 1) g = 1;
  const MsmPlan P1 = msm_plan(ctx, b, n);
  if (items_plan(P1)) return 1;
  for (; g > 1; g--) {
    if ((uint64_t)P1.K * g > BATCH_K_MAX || P1.Mmax * (size_t)g > BATCH_M_MAX) continue;
    if (!items_plan(msm_plan_batch(ctx, b, n, g, 0))) break;
  }
  return g;
}

int msm_batch_submit_shared(zkmi_ctx* ctx, const zkmi_bases* const* bs, int k, size_t offset, const void* d_scalars,
                            size_t n, size_t nb, size_t stride, zkmi_msm_job** jobs) {
  for (int i = 0; i < k; i++) jobs[i] = nullptr;
  for (int i = 0; i < k; i++) ZK_TRY(check_range(bs[i], offset, n));
  if (stride < n * 32 || (stride & 31) || (n && nb && !d_scalars)) {
    set_error("msm_batch: stride %zu must be a multiple of 32 and >= n * 32 = %zu (and the scalars non-null)", stride,
              n * 32);
    return ZKMI_EINVAL;
  }
  for (int i = 0; i < k; i++) {
    const MsmPlan P = msm_plan(ctx, bs[i], n);
    jobs[i] = new zkmi_msm_job{ctx, bs[i]->g2, P.c, P.W, P.bb, nullptr, 0, nullptr, n == 0 || nb == 0};
    jobs[i]->batch = true;
    jobs[i]->nb = nb;
  }
  if (n == 0 || nb == 0) return 0;
  int G = msm_batch_group(ctx, bs[0], n, nb);
  for (int i = 1; i < k; i++) G = std::min(G, msm_batch_group(ctx, bs[i], n, nb));
  const size_t sstride = stride / 4;  // u32 words between two scalar vectors
  int rc = 0;
  for (size_t b0 = 0; b0 < nb && !rc; b0 += (size_t)G) {
    const int gb = (int)std::min<size_t>((size_t)G, nb - b0);
    rc = msm_sort_acc_shared(ctx, bs, k, offset, (const uint32_t*)d_scalars + b0 * sstride, n, gb, sstride,
                             [&](int j, const MsmPlan& P) {
                               zkmi_msm_job* part = new_job(ctx, bs[j], P, n);
                               part->nbat = gb;
                               jobs[j]->parts.push_back(part);  // owned from here on, whatever follows
                               return part;
                             });
  }
  if (rc) {
    for (int i = 0; i < k; i++) {
      msm_job_free(jobs[i]);
      jobs[i] = nullptr;
    }
  }
  return rc;
}

// one group job: the bit sums of its nbat vectors -> nbat points
static int msm_part_wait(zkmi_msm_job* job, uint64_t* out) {
  zkmi_ctx* ctx = job->ctx;
  hipError_t e = hipEventSynchronize(job->done);
  if (e != hipSuccess) {
    set_error("msm_batch_wait: %s", hipGetErrorString(e));
    job->host = nullptr;  // copy state unknown: never recycle the buffer
    msm_job_free(job);
    return ZKMI_EHIP;
  }
  job->st = nullptr;  // the bit-sum copy has landed
  int rc = timer_flush(ctx, false);
  auto th0 = std::chrono::steady_clock::now();
  // each vector's own W windows; never a Horner pass across the whole job
  msm_host_batch_combine(job->host, job->nbat, job->g2, job->c, job->W / job->nbat, job->bb, job->sb, out);
  if (ctx->timer.enabled) {
    auto& t = ctx->timer.totals["msm_host_epilogue"];
    t.first += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - th0).count();
    t.second += 1;
  }
  msm_job_free(job);
  return rc;
}

int msm_batch_wait(zkmi_msm_job* job, uint64_t* out, size_t nb) {
  if (!job || !job->batch || job->nb != nb) {  // the job stays valid
    set_error(!job ? "msm_batch_wait: null job"
                   : !job->batch ? "msm_batch_wait: not a batch job (finish it with zkmi_msm_wait)"
                                 : "msm_batch_wait: the job holds another number of MSMs");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(job->ctx);
  const size_t PW = job->g2 ? 16 : 8;  // u64 per point
  int rc = 0;
  if (job->empty) {
    memset(out, 0, nb * PW * 8);
  } else {
    size_t at = 0;
    for (zkmi_msm_job*& part : job->parts) {
      const size_t cnt = (size_t)part->nbat;
      if (!rc) rc = msm_part_wait(part, out + at * PW);
      else msm_job_free(part);
      part = nullptr;
      at += cnt;
    }
    job->parts.clear();
  }
  msm_job_free(job);
  return rc;
}

// Point-sharded MSM (zkmi.h, multi-GPU): every rank runs its shard through
// the usual pipeline with its own window plan and queues exactly one
// fixed-size exchange (SHARD_PAYLOAD_WORDS per rank: status block + bit sums);
// msm_wait checks the plans and sums the bit sums of every non-empty shard.
// There is no plan-agreement collective: a rank whose plan, shard or local
// checks differ still takes part in the same one exchange (with its failure
// flag or its plan signature), so a mismatch fails msm_wait on every rank and
// no rank can block in a collective the others skip.  (Round 4 agreed the
// plan by a synchronous header all-gather on the first submit and cached it
// per shard state; a rank whose cache missed alone -- its window or table
// changed on that rank only -- entered the header exchange while its peers
// entered the data exchange: a hang over RCCL.)
int msm_submit_sharded(zkmi_comm* comm, const zkmi_bases* b, size_t offset, const void* d_scalars, size_t n,
                       zkmi_msm_job** out, bool windows) {
  *out = nullptr;
  zkmi_ctx* ctx = comm->ctx;
  int rc = check_range(b, offset, n);
  if (!rc && b->ctx != ctx) {
    set_error("msm_sharded: base set belongs to another context than the communicator");
    rc = ZKMI_EINVAL;
  }
  const int XW = b->g2 ? 64 : 32;
  MsmPlan P{};
  if (!rc && windows) {
    // window sharding (north_star's variant): every rank holds every base and
    // scalar and runs windows [r W / N, (r + 1) W / N) of the plain plan (no
    // fixed-base table: a table folds all windows into one)
    // (the automatic choice is clamped to >= 12: the window-sharded plan
    // needs the sort's window filter, which the small-MSM sorts below 12 lack)
    P.c = ctx->msm_window > 0 ? ctx->msm_window : std::max(12, pick_window(n));
    if (P.c < 12 || P.c > 17) {
      set_error("msm_window_sharded: window %d outside 12..17 (zkmi_msm_set_window; 0 = automatic)", P.c);
      rc = ZKMI_EINVAL;
    } else {
      const int Wt = msm_windows(P.c), nr = comm->nranks, r = comm->rank;
      P.w0 = (int)((long)r * Wt / nr);
      P.W = (int)((long)(r + 1) * Wt / nr) - P.w0;
      P.p = 1;
      P.bal = false;
      P.ne = n;
      P.Mmax = (size_t)P.W * n;
      P.B = 1u << (P.c - 1);
      P.K = (uint32_t)P.W * P.B;
      P.bb = P.c - 1;
      P.lb = (P.bb + 1) / 2;
      P.hb = P.bb - P.lb;
      P.wsel = (uint32_t)P.w0 | ((uint32_t)P.W << 16);
      if (P.W == 0) n = 0;  // more ranks than windows: this rank's part is empty
      if (n) rc = check_size(P, n);
    }
  } else if (!rc) {
    P = msm_plan(ctx, b, n);
    if (n) rc = check_size(P, n);
  }
  if (!rc && n) {
    const BrGeom bg = br_geom(P, b->g2 != 0, false);
    if ((size_t)P.W * (P.bb + 1) * bg.sb * XW + SHARD_STATUS_WORDS > SHARD_PAYLOAD_WORDS) {
      set_error("msm_sharded: window %d's bit sums exceed the sharded exchange (use a table or a window <= 20)", P.c);
      rc = ZKMI_EINVAL;
    }
  }
  zkmi_msm_job* job = new_job(ctx, b, P, n);
  job->comm = comm;
  job->wmode = windows;  // (also on a rank left without windows: its status block says so)
  job->empty = false;  // every rank takes part in the exchange, empty shard or not
  MsmLane* lane = nullptr;
  // test hook (tests/host/test_sharded_msm.cpp): ZKMI_DEBUG_SHARD_FAIL=<rank>
  // makes that rank fail before its exchange
  const char* dbg = getenv("ZKMI_DEBUG_SHARD_FAIL");
  if (!rc && dbg && atoi(dbg) == comm->rank) {
    set_error("msm_sharded: injected failure (ZKMI_DEBUG_SHARD_FAIL)");
    rc = ZKMI_EHIP;
  }
  if (!rc && n) {
    uint32_t *sval, *bstart;
    if (!(rc = get_lane(ctx, &lane)) && !(rc = msm_sort_phase(ctx, lane, P, (const uint32_t*)d_scalars, n, &sval,
                                                               &bstart)))
      rc = msm_acc_any(ctx, lane, P, b, offset, n, sval, bstart, job);
  } else if (!rc) {
    // empty shard: the status block alone ("empty", no bit sums)
    uint32_t* buf = nullptr;
    if (!(rc = get_lane(ctx, &lane)) &&
        !(rc = lane->ws.get("msm_empty_shard", SHARD_PAYLOAD_WORDS * 4, (void**)&buf)))
      rc = msm_queue_handover(ctx, lane, lane->st, job, buf, 0);
  }
  if (rc) {
    // The peers are in (or heading for) this job's exchange: join it with a
    // failure status.  Over RCCL every exchange is queued on the
    // communicator's stream in submit order, so the failure exchange goes there
    // now (unless this rank's share is already queued).  Over a host transport
    // the exchanges run in msm_wait, in wait order: a failure exchanged here
    // would pair with the peers' exchange of an earlier job still in flight and
    // shift every later one, so the job is returned marked failed and
    // msm_wait exchanges the failure at its turn.
    const std::string err = zkmi_last_error();
    if (comm->kind == ZKMI_COMM_HOST) {
      if (lane) (void)hipStreamSynchronize(lane->st);  // partly queued work: drained before the buffers recycle
      (void)hipGetLastError();
      if (job->host) ctx_pinned_put(ctx, job->host);
      job->host = nullptr;
      job->st = nullptr;
      job->fail_rc = rc;
      job->fail_msg = err;
      set_error("%s", err.c_str());
      *out = job;
      return 0;
    }
    if (!job->exchanged) (void)comm_fail_exchange(comm, SHARD_PAYLOAD_WORDS);
    set_error("%s", err.c_str());
    msm_job_free(job);
    return rc;
  }
  *out = job;
  return 0;
}

}  // namespace zk
