// ed25519.hip — batched Ed25519 verification (zkmi.h "Ed25519 verification",
// DESIGN.md §2.16).  The arithmetic is ed25519.h's over note_crypt.h's field;
// this file holds the two kernels' lane mappings, where their tables live, the
// launch sequence and the C entry point.  One lane verifies one signature.
// Everything runs on the context stream, and the call returns with the
// verdicts on the host.
//
//   k_ed_hash    k = SHA-512(R || A || M) mod L.  Lanes differ in the number
//                of blocks they hash; this part is about a tenth of the kernels' time.
//   k_ed_curve   decompress A, range-check s, build the 16 multiples of -A,
//                run [s]B + [k](-A), compress, compare with R.  Every lane
//                runs the same 256 doublings and 128 additions whatever its
//                verdict: a key that does not decompress is replaced by the
//                identity and its verdict set afterwards.
// The table of B (16 cached points, 2560 bytes) is built once per context on
// the host, kept in the workspace and read by every block from LDS.  A lane's
// table of -A (2560 contiguous bytes) lies in the workspace; the curve kernel
// is launched over at most ED_CHUNK signatures at a time, which bounds that
// table whatever n is.
//
// The curve kernel has a second form for tx_auth.hip: keys
// and signatures read from zkmi_signed_tx records where they lie, and an
// optional list of the records to take.  ed_curve_pass launches either.
#include <string.h>

#include <algorithm>

#include "zkmi_internal.h"
#include "ed25519.h"
#include "tx_msg.h"

namespace zk {

constexpr int ED_HASH_B = 256;   // lanes a block of the hash kernel
constexpr int ED_CURVE_B = 64;   // lanes a block of the curve kernel
#ifndef ED_CURVE_WAVES
#define ED_CURVE_WAVES 2         // waves a SIMD the curve kernel's registers are capped for
#endif
constexpr size_t ED_CHUNK = 1u << 18;
constexpr size_t ED_MAX_N = 1u << 26;
static unsigned ed_blocks(size_t n, int b) { return (unsigned)((n + b - 1) / b); }

struct EdGlobalBytes {
  const uint8_t* p;
  __device__ __forceinline__ uint8_t operator()(uint64_t i) const { return p[i]; }
};

__global__ void __launch_bounds__(ED_HASH_B) k_ed_hash(const uint32_t* __restrict__ pk, const uint32_t* __restrict__ sig,
                                                       const uint8_t* __restrict__ msgs,
                                                       const uint64_t* __restrict__ off, uint32_t n,
                                                       uint32_t* __restrict__ k_out) {
  const uint32_t i = blockIdx.x * ED_HASH_B + threadIdx.x;
  if (i >= n) return;
  uint32_t a[8], r[8], k[8];
#pragma unroll
  for (int w = 0; w < 8; w++) a[w] = pk[8 * (size_t)i + w], r[w] = sig[16 * (size_t)i + w];
  const uint64_t at = off[i], len = off[i + 1] - at;
  ed_challenge(k, r, a, len, EdGlobalBytes{msgs + at});
#pragma unroll
  for (int w = 0; w < 8; w++) k_out[8 * (size_t)i + w] = k[w];
}

// A lane's 16 entries are contiguous (2560 bytes), an entry 160 bytes read and
// written as ten 16-byte words: lanes pick different entries, so only whole
// entries keep every sector that moves fully used.
struct EdLaneTable {
  uint4* t;  // this lane's table
  __device__ __forceinline__ void operator()(int j, const EdCached& c) const {
    uint4 q[ED_CACHED_WORDS / 4];
    __builtin_memcpy(q, &c, sizeof c);
#pragma unroll
    for (int x = 0; x < ED_CACHED_WORDS / 4; x++) t[j * (ED_CACHED_WORDS / 4) + x] = q[x];
  }
  __device__ __forceinline__ EdCached operator()(uint32_t j) const {
    uint4 q[ED_CACHED_WORDS / 4];
#pragma unroll
    for (int x = 0; x < ED_CACHED_WORDS / 4; x++) q[x] = t[j * (ED_CACHED_WORDS / 4) + x];
    EdCached c;
    __builtin_memcpy(&c, q, sizeof c);
    return c;
  }
};
struct EdLdsTable {
  const EdCached* t;
  __device__ __forceinline__ const EdCached& operator()(uint32_t j) const { return t[j]; }
};

// signatures [first, first + m); tab: m tables of 640 words.  Two waves a
// SIMD: the register cap of 256 that goes with it costs 60 bytes of scratch a
// lane.  TX: pk is n zkmi_signed_tx records, which
// hold key and signature (sig is not read); lane j of the call takes record
// idx[first + j], or first + j when idx is null.  k and verdict are indexed by
// record either way.
template <bool TX>
__global__ void __launch_bounds__(ED_CURVE_B, ED_CURVE_WAVES) k_ed_curve(const uint32_t* __restrict__ pk,
                                                         const uint32_t* __restrict__ sig,
                                                         const uint32_t* __restrict__ kk,
                                                         const uint32_t* __restrict__ tab_b, uint4* tab,
                                                         const uint32_t* __restrict__ idx, uint32_t first, uint32_t m,
                                                         uint8_t* __restrict__ verdict) {
  __shared__ EdCached tb_s[ED_TABLE];
  {
    uint32_t* d = reinterpret_cast<uint32_t*>(tb_s);
    for (uint32_t x = threadIdx.x; x < ED_TABLE * ED_CACHED_WORDS; x += ED_CURVE_B) d[x] = tab_b[x];
    __syncthreads();
  }
  const uint32_t lane = blockIdx.x * ED_CURVE_B + threadIdx.x;
  if (lane >= m) return;
  const size_t i = TX && idx ? (size_t)idx[first + lane] : (size_t)first + lane;
  const uint32_t* a_at = TX ? pk + TX_REC_WORDS * i + TX_REC_SIGNER : pk + 8 * i;
  const uint32_t* sig_at = TX ? pk + TX_REC_WORDS * i + TX_REC_SIG : sig + 16 * i;
  uint32_t a_bytes[8], r[8], s[8], k[8];
#pragma unroll
  for (int w = 0; w < 8; w++) a_bytes[w] = a_at[w], r[w] = sig_at[w], s[w] = sig_at[8 + w], k[w] = kk[8 * i + w];
  EdPoint a = ed_identity();
  const bool a_ok = ed_decompress(a, a_bytes), s_ok = sc_is_canonical(s);
  const EdLaneTable tq{tab + (size_t)lane * (ED_TABLE * ED_CACHED_WORDS / 4)};
  ed_build_table(ed_neg(a), tq);
  uint32_t got[8];
  ed_compress(got, ed_double_scalar_mul(s, k, EdLdsTable{tb_s}, tq));
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) d |= got[w] ^ r[w];
  verdict[i] = (uint8_t)(!a_ok ? SIG_BAD_PUBKEY : !s_ok ? SIG_BAD_S : d ? SIG_MISMATCH : SIG_OK);
}

// the 16 cached multiples of B, made once per context
static int ed_base_table(zkmi_ctx* ctx, uint32_t** d_tab) {
  const bool have = ctx->ws.bufs.count("ed_base_table") != 0;
  ZK_TRY(ctx->ws.get("ed_base_table", sizeof(EdCached) * ED_TABLE, (void**)d_tab));
  if (have) return 0;
  static_assert(sizeof(EdCached) == 4 * ED_CACHED_WORDS, "a cached point is 40 words");
  EdCached host[ED_TABLE];
  ed_build_table(ed_base(), EdTableArray{host});
  ZK_HIP(hipMemcpyAsync(*d_tab, host, sizeof host, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));  // host[] leaves scope
  return 0;
}

// The curve kernel over n signatures on the context stream, in chunks of at
// most ED_CHUNK, timed under `timer`.  rec null: dense keys and signatures,
// signature i at index i.  rec given: the records of tx_auth.hip, taken by
// idx[0 .. n) (null: records 0 .. n - 1); pk and sig are not read.
int ed_curve_pass(zkmi_ctx* ctx, const char* timer, const uint32_t* pk, const uint32_t* sig, const uint32_t* rec,
                  const uint32_t* idx, const uint32_t* k, size_t n, uint8_t* verdict) {
  const size_t chunk = std::min(n, ED_CHUNK);
  uint32_t *d_tab, *d_tab_b;
  ZK_TRY(ed_base_table(ctx, &d_tab_b));
  ZK_TRY(ctx->ws.get("ed_table", chunk * sizeof(EdCached) * ED_TABLE, (void**)&d_tab));
  {
    ScopedKernelTimer tm(ctx, timer);
    for (size_t first = 0; first < n; first += chunk) {
      const size_t m = std::min(chunk, n - first);
      if (rec)
        k_ed_curve<true><<<ed_blocks(m, ED_CURVE_B), ED_CURVE_B, 0, ctx->stream>>>(rec, rec, k, d_tab_b, (uint4*)d_tab, idx,
                                                                                  (uint32_t)first, (uint32_t)m, verdict);
      else
        k_ed_curve<false><<<ed_blocks(m, ED_CURVE_B), ED_CURVE_B, 0, ctx->stream>>>(pk, sig, k, d_tab_b, (uint4*)d_tab, nullptr,
                                                                                   (uint32_t)first, (uint32_t)m, verdict);
    }
  }
  ZK_HIP(hipGetLastError());
  return 0;
}

// arguments already checked; n >= 1
static int ed_verify_many(zkmi_ctx* ctx, size_t n, const uint8_t* pubkeys, const uint8_t* sigs, const uint8_t* msgs,
                          const uint64_t* off, uint8_t* verdicts) {
  const size_t total = off[n];
  uint32_t *d_pk, *d_sig, *d_k;
  uint64_t* d_off;
  uint8_t *d_msg, *d_verdict;
  ZK_TRY(ctx->ws.get("ed_pk", n * 32, (void**)&d_pk));
  ZK_TRY(ctx->ws.get("ed_sig", n * 64, (void**)&d_sig));
  ZK_TRY(ctx->ws.get("ed_off", (n + 1) * 8, (void**)&d_off));
  ZK_TRY(ctx->ws.get("ed_msg", std::max<size_t>(total, 1), (void**)&d_msg));
  ZK_TRY(ctx->ws.get("ed_k", n * 32, (void**)&d_k));
  ZK_TRY(ctx->ws.get("ed_verdict", n, (void**)&d_verdict));
  ZK_HIP(hipMemcpyAsync(d_pk, pubkeys, n * 32, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_sig, sigs, n * 64, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_off, off, (n + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (total) ZK_HIP(hipMemcpyAsync(d_msg, msgs, total, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "ed25519_hash");
    k_ed_hash<<<ed_blocks(n, ED_HASH_B), ED_HASH_B, 0, ctx->stream>>>(d_pk, d_sig, d_msg, d_off, (uint32_t)n, d_k);
  }
  ZK_HIP(hipGetLastError());
  ZK_TRY(ed_curve_pass(ctx, "ed25519_curve", d_pk, d_sig, nullptr, nullptr, d_k, n, d_verdict));
  ZK_HIP(hipMemcpyAsync(verdicts, d_verdict, n, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return timer_flush(ctx);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkmi_ed25519_verify_many(zkmi_ctx* ctx, size_t n, const uint8_t* pubkeys, const uint8_t* sigs, const uint8_t* msgs,
                             const uint64_t* msg_offsets, uint8_t* verdicts) {
  if (!ctx) {
    set_error("zkmi_ed25519_verify_many: null context");
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  if (!pubkeys || !sigs || !msg_offsets || !verdicts) {
    set_error("zkmi_ed25519_verify_many: null argument");
    return ZKMI_EINVAL;
  }
  if (n > ED_MAX_N) {
    set_error("zkmi_ed25519_verify_many: %zu signatures in a call, at most 2^26", n);
    return ZKMI_EINVAL;
  }
  if (msg_offsets[0] != 0) {
    set_error("zkmi_ed25519_verify_many: msg_offsets[0] is %llu, not 0", (unsigned long long)msg_offsets[0]);
    return ZKMI_EINVAL;
  }
  for (size_t i = 0; i < n; i++)
    if (msg_offsets[i + 1] < msg_offsets[i]) {
      set_error("zkmi_ed25519_verify_many: msg_offsets descend at %zu (%llu after %llu)", i + 1,
                (unsigned long long)msg_offsets[i + 1], (unsigned long long)msg_offsets[i]);
      return ZKMI_EINVAL;
    }
  if (msg_offsets[n] && !msgs) {
    set_error("zkmi_ed25519_verify_many: null messages");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return ed_verify_many(ctx, n, pubkeys, sigs, msgs, msg_offsets, verdicts);
}

}  // extern "C"
