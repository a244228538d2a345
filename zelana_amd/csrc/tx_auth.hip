// tx_auth.hip — the sequencer's authorisation of transfers and withdrawals from
// their fields (zkmi.h "Transaction authorisation"): the
// reference's verify_transfer_signature and verify_withdraw_signature
// (core/src/sequencer/execution/tx_router.rs:668-793) over fixed-width records,
// the messages built on the device by tx_msg.h.  One lane a record, everything
// on the context stream:
//
//   k_tx_format<false>  the readable message of every record into its slot of
//                       TX_MSG_STRIDE bytes, 16 bytes a store, and its length
//   k_tx_hash           k = SHA-512(R || A || M) mod L from the slot
//   k_ed_curve<true>    ed25519.hip's curve kernel, key and signature read
//                       from the record                       -> verdict 1
//   k_tx_compact        the records whose verdict is SIG_MISMATCH into a dense
//                       list (ballot, one atomic add a wave); the count comes
//                       to the host, and a count of zero ends the passes
//   k_tx_format<true>, k_tx_hash, k_ed_curve<true> over the list: the legacy
//                       message                               -> verdict 2
//   k_tx_epilogue       reason and matched format from the two verdicts and
//                       the compare of `from` with the signer
// A key that does not decompress and an s >= L fail under both formats alike
// and are not tried again.
#include <algorithm>

#include "zkmi_internal.h"
#include "ed25519.h"
#include "tx_msg.h"

namespace zk {

constexpr int TX_B = 256;  // lanes a block of every kernel here
constexpr size_t TX_MAX_N = 1u << 26;
static unsigned tx_blocks(size_t n) { return (unsigned)((n + TX_B - 1) / TX_B); }

static_assert(sizeof(zkmi_signed_tx) == 4 * TX_REC_WORDS && offsetof(zkmi_signed_tx, to) == 32 &&
                  offsetof(zkmi_signed_tx, amount) == 64 && offsetof(zkmi_signed_tx, nonce) == 72 &&
                  offsetof(zkmi_signed_tx, chain_id) == 80 && offsetof(zkmi_signed_tx, signer_pubkey) == 4 * TX_REC_SIGNER &&
                  offsetof(zkmi_signed_tx, signature) == 4 * TX_REC_SIG && offsetof(zkmi_signed_tx, kind) == 4 * TX_REC_KIND &&
                  offsetof(zkmi_signed_tx, reserved) == 185,
              "zkmi_signed_tx is 192 bytes without padding, laid out as tx_msg.h reads it");
static_assert(ZKMI_TX_TRANSFER == TX_KIND_TRANSFER && ZKMI_TX_WITHDRAWAL == TX_KIND_WITHDRAWAL, "kinds");
static_assert(ZKMI_SIG_OK == SIG_OK && ZKMI_SIG_BAD_PUBKEY == SIG_BAD_PUBKEY && ZKMI_SIG_MISMATCH == SIG_MISMATCH, "verdicts");

// lane t takes record idx[t], or t when idx is null
__device__ __forceinline__ size_t tx_record_of(const uint32_t* idx, uint32_t t) { return idx ? (size_t)idx[t] : (size_t)t; }

// The message of m records: the fields (the first 96 bytes of a record, and
// its kind) are read as 16-byte words, the message leaves through TxQuadSink.
template <bool LEGACY>
__global__ void __launch_bounds__(TX_B) k_tx_format(const uint4* __restrict__ rec, const uint32_t* __restrict__ idx, uint32_t m,
                                                    uint32_t* __restrict__ slots, uint32_t* __restrict__ lens) {
  const uint32_t t = blockIdx.x * TX_B + threadIdx.x;
  if (t >= m) return;
  const size_t i = tx_record_of(idx, t);
  uint32_t r[TX_REC_WORDS];
#pragma unroll
  for (int q = 0; q < 6; q++) {
    const uint4 v = rec[(TX_REC_WORDS / 4) * i + q];
    r[4 * q] = v.x, r[4 * q + 1] = v.y, r[4 * q + 2] = v.z, r[4 * q + 3] = v.w;
  }
  r[TX_REC_KIND] = reinterpret_cast<const uint32_t*>(rec)[TX_REC_WORDS * i + TX_REC_KIND];
  TxQuadSink sink{slots + (TX_MSG_STRIDE / 4) * i};
  lens[i] = tx_record_message(sink, r, LEGACY);
}

struct TxSlotBytes {
  const uint32_t* w;
  __device__ __forceinline__ uint8_t operator()(uint64_t i) const { return (uint8_t)(w[i >> 2] >> (8 * (i & 3))); }
};

// k of m records from their slots.  Every lane of a pass hashes the same
// number of blocks: three with a readable message, two with a legacy one.
__global__ void __launch_bounds__(TX_B) k_tx_hash(const uint32_t* __restrict__ rec, const uint32_t* __restrict__ slots,
                                                  const uint32_t* __restrict__ lens, const uint32_t* __restrict__ idx, uint32_t m,
                                                  uint32_t* __restrict__ k_out) {
  const uint32_t t = blockIdx.x * TX_B + threadIdx.x;
  if (t >= m) return;
  const size_t i = tx_record_of(idx, t);
  uint32_t a[8], r[8], k[8];
#pragma unroll
  for (int w = 0; w < 8; w++) a[w] = rec[TX_REC_WORDS * i + TX_REC_SIGNER + w], r[w] = rec[TX_REC_WORDS * i + TX_REC_SIG + w];
  ed_challenge(k, r, a, lens[i], TxSlotBytes{slots + (TX_MSG_STRIDE / 4) * i});
#pragma unroll
  for (int w = 0; w < 8; w++) k_out[8 * i + w] = k[w];
}

// The records whose verdict is SIG_MISMATCH, in any order: a wave counts its
// own by ballot, takes its place in the list with one atomic add, and every
// flagged lane writes at its rank.  *count was cleared before the launch.
__global__ void __launch_bounds__(TX_B) k_tx_compact(const uint8_t* __restrict__ verdict, uint32_t n, uint32_t* __restrict__ list,
                                                     uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * TX_B + threadIdx.x;
  const bool flag = i < n && verdict[i] == SIG_MISMATCH;
  const unsigned long long mask = __ballot(flag);
  const uint32_t lane = threadIdx.x & 63;
  uint32_t base = 0;
  if (lane == 0 && mask) base = atomicAdd(count, (uint32_t)__popcll(mask));
  base = __shfl(base, 0);
  if (flag) list[base + (uint32_t)__popcll(mask & ((1ull << lane) - 1))] = i;
}

// v2[i] is read only where v1[i] is SIG_MISMATCH: there the second pass wrote it
__global__ void __launch_bounds__(TX_B) k_tx_epilogue(const uint32_t* __restrict__ rec, const uint8_t* __restrict__ v1,
                                                      const uint8_t* __restrict__ v2, uint32_t n, uint8_t* __restrict__ reasons,
                                                      uint8_t* __restrict__ formats) {
  const uint32_t i = blockIdx.x * TX_B + threadIdx.x;
  if (i >= n) return;
  const uint32_t first = v1[i];
  uint32_t format = ZKMI_TXFMT_NONE;
  if (first == SIG_OK) format = ZKMI_TXFMT_READABLE;
  else if (first == SIG_MISMATCH && v2[i] == SIG_OK) format = ZKMI_TXFMT_LEGACY;
  uint32_t reason = first == SIG_BAD_PUBKEY ? ZKMI_TXAUTH_BAD_PUBKEY : ZKMI_TXAUTH_FAILED;
  if (format != ZKMI_TXFMT_NONE) {
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) d |= rec[TX_REC_WORDS * (size_t)i + w] ^ rec[TX_REC_WORDS * (size_t)i + TX_REC_SIGNER + w];
    reason = d ? ZKMI_TXAUTH_FROM_MISMATCH : ZKMI_TXAUTH_OK;
  }
  reasons[i] = (uint8_t)reason, formats[i] = (uint8_t)format;
}

// arguments already checked; n >= 1
static int tx_auth_many(zkmi_ctx* ctx, size_t n, const zkmi_signed_tx* txs, uint8_t* reasons, uint8_t* formats) {
  uint32_t *d_rec, *d_msg, *d_len, *d_k, *d_list, *d_count;
  uint8_t *d_v1, *d_v2, *d_reason, *d_format;
  ZK_TRY(ctx->ws.get("txauth_rec", n * sizeof(zkmi_signed_tx), (void**)&d_rec));
  ZK_TRY(ctx->ws.get("txauth_msg", n * TX_MSG_STRIDE, (void**)&d_msg));
  ZK_TRY(ctx->ws.get("txauth_len", n * 4, (void**)&d_len));
  ZK_TRY(ctx->ws.get("txauth_k", n * 32, (void**)&d_k));
  ZK_TRY(ctx->ws.get("txauth_list", n * 4, (void**)&d_list));
  ZK_TRY(ctx->ws.get("txauth_count", 4, (void**)&d_count));
  ZK_TRY(ctx->ws.get("txauth_v1", n, (void**)&d_v1));
  ZK_TRY(ctx->ws.get("txauth_v2", n, (void**)&d_v2));
  ZK_TRY(ctx->ws.get("txauth_reason", n, (void**)&d_reason));
  ZK_TRY(ctx->ws.get("txauth_format", n, (void**)&d_format));
  const uint32_t m = (uint32_t)n;
  ZK_HIP(hipMemcpyAsync(d_rec, txs, n * sizeof(zkmi_signed_tx), hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemsetAsync(d_count, 0, 4, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "txauth_format");
    k_tx_format<false><<<tx_blocks(n), TX_B, 0, ctx->stream>>>((const uint4*)d_rec, nullptr, m, d_msg, d_len);
  }
  {
    ScopedKernelTimer tm(ctx, "txauth_hash");
    k_tx_hash<<<tx_blocks(n), TX_B, 0, ctx->stream>>>(d_rec, d_msg, d_len, nullptr, m, d_k);
  }
  ZK_HIP(hipGetLastError());
  ZK_TRY(ed_curve_pass(ctx, "txauth_curve", nullptr, nullptr, d_rec, nullptr, d_k, n, d_v1));
  {
    ScopedKernelTimer tm(ctx, "txauth_compact");
    k_tx_compact<<<tx_blocks(n), TX_B, 0, ctx->stream>>>(d_v1, m, d_list, d_count);
  }
  ZK_HIP(hipGetLastError());
  uint32_t retry = 0;
  ZK_HIP(hipMemcpyAsync(&retry, d_count, 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  if (retry > n) {
    set_error("zkmi_tx_auth_many: %u records to try again among %zu", retry, n);
    return ZKMI_EHIP;
  }
  if (retry) {
    {
      ScopedKernelTimer tm(ctx, "txauth_format_legacy");
      k_tx_format<true><<<tx_blocks(retry), TX_B, 0, ctx->stream>>>((const uint4*)d_rec, d_list, retry, d_msg, d_len);
    }
    {
      ScopedKernelTimer tm(ctx, "txauth_hash_legacy");
      k_tx_hash<<<tx_blocks(retry), TX_B, 0, ctx->stream>>>(d_rec, d_msg, d_len, d_list, retry, d_k);
    }
    ZK_HIP(hipGetLastError());
    ZK_TRY(ed_curve_pass(ctx, "txauth_curve_legacy", nullptr, nullptr, d_rec, d_list, d_k, retry, d_v2));
  }
  {
    ScopedKernelTimer tm(ctx, "txauth_epilogue");
    k_tx_epilogue<<<tx_blocks(n), TX_B, 0, ctx->stream>>>(d_rec, d_v1, d_v2, m, d_reason, d_format);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(reasons, d_reason, n, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipMemcpyAsync(formats, d_format, n, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return timer_flush(ctx);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkmi_tx_auth_many(zkmi_ctx* ctx, size_t n, const zkmi_signed_tx* txs, uint8_t* reasons, uint8_t* formats) {
  if (!ctx) {
    set_error("zkmi_tx_auth_many: null context");
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  if (!txs || !reasons || !formats) {
    set_error("zkmi_tx_auth_many: null argument");
    return ZKMI_EINVAL;
  }
  if (n > TX_MAX_N) {
    set_error("zkmi_tx_auth_many: %zu records in a call, at most 2^26", n);
    return ZKMI_EINVAL;
  }
  for (size_t i = 0; i < n; i++) {
    if (txs[i].kind != ZKMI_TX_TRANSFER && txs[i].kind != ZKMI_TX_WITHDRAWAL) {
      set_error("zkmi_tx_auth_many: record %zu is of kind %u", i, (unsigned)txs[i].kind);
      return ZKMI_EINVAL;
    }
    for (int j = 0; j < 7; j++)
      if (txs[i].reserved[j]) {
        set_error("zkmi_tx_auth_many: record %zu has a reserved byte that is not zero", i);
        return ZKMI_EINVAL;
      }
  }
  ZK_DEVICE_GUARD(ctx);
  return tx_auth_many(ctx, n, txs, reasons, formats);
}

}  // extern "C"
