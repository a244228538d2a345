// lane_util.h — the lane- and block-level pieces the kernels of the resident
// stores and of the witness programs share.  Device only:
// the .hip files include it, the host+device headers do not.  Everything is
// forced inline and every block size is a template constant, so a kernel that
// uses a helper compiles to what it would with the helper written out.
#pragma once
#include "ff.h"

namespace zk {

// x of lane LANE of this lane's quad (a DPP quad broadcast per limb).  All
// four lanes of the quad must be active.
template <int LANE>
__device__ __forceinline__ Fe quad_bcast(const Fe& x) {
  constexpr int ctrl = LANE | (LANE << 2) | (LANE << 4) | (LANE << 6);  // quad_perm [L, L, L, L]
  Fe r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)x.v[i], ctrl, 0xF, 0xF, false);
  return r;
}

// one field element or key of 8 words
__device__ __forceinline__ void copy8(uint32_t* dst, const uint32_t* src) {
#pragma unroll
  for (int w = 0; w < 8; w++) dst[w] = src[w];
}

// A table of n constants into LDS, by the whole block, then a barrier: every
// lane of a wave reads the same constant at the same time afterwards (a
// broadcast read).  All lanes of the block call it.
__device__ __forceinline__ void fe_table_lds(Fe* dst, const Fe* __restrict__ src, uint32_t n) {
  const uint32_t* s = reinterpret_cast<const uint32_t*>(src);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (uint32_t i = threadIdx.x; i < n * NL; i += blockDim.x) d[i] = s[i];
  __syncthreads();
}

// cnt[0 .. nblocks) -> its exclusive prefix sums, in place; *total = their
// sum.  One workgroup of B lanes: a lane sums a run of blocks (the trailing
// lanes an empty one), the lanes' sums are scanned in LDS.  The counts are
// those of the blocks of a flagging kernel; block_rank below consumes the
// offsets in a kernel of the same blocks.
template <int B>
__global__ void __launch_bounds__(B) k_block_offsets(uint32_t* cnt, uint32_t nblocks, uint32_t* total) {
  __shared__ uint32_t sum_s[B];
  const uint32_t per = (nblocks + B - 1) / B;
  const uint32_t lo = threadIdx.x * per < nblocks ? threadIdx.x * per : nblocks;
  const uint32_t hi = lo + per < nblocks ? lo + per : nblocks;
  uint32_t s = 0;
  for (uint32_t b = lo; b < hi; b++) s += cnt[b];
  sum_s[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int i = 0; i < B; i++) {
      const uint32_t v = sum_s[i];
      sum_s[i] = run;
      run += v;
    }
    *total = run;
  }
  __syncthreads();
  uint32_t run = sum_s[threadIdx.x];
  for (uint32_t b = lo; b < hi; b++) {
    const uint32_t v = cnt[b];
    cnt[b] = run;
    run += v;
  }
}

// The rank of a flagged lane among the flagged lanes of the call, in block
// and lane order: *block_off (this block's entry of k_block_offsets' result)
// plus the flagged lanes before it in its block, by ballot and popcount.  ALL
// lanes of a block of B call it (it holds the one barrier); the value is the
// rank for flagged lanes and 0 for the others, which do not read *block_off.
// wave_s: B / 64 words of LDS.
template <int B>
__device__ __forceinline__ uint32_t block_rank(bool flag, const uint32_t* block_off, uint32_t* wave_s) {
  static_assert(B % 64 == 0, "whole waves");
  const unsigned long long m = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) wave_s[wave] = (uint32_t)__popcll(m);
  __syncthreads();
  if (!flag) return 0;
  uint32_t rank = *block_off + (uint32_t)__popcll(m & ((1ull << lane) - 1));
  for (uint32_t w = 0; w < wave; w++) rank += wave_s[w];
  return rank;
}

}  // namespace zk
