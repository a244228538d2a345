// nullifier_set.hip — the nullifier set resident in HBM (zkmi.h "nullifier
// set").  The slot function, the probes, the grouping and the
// rules of a round are nullifier_set.h's; this file holds the kernels, the
// launch sequence of a spend and the C entry points.  Everything runs on the
// context stream, and every call returns with its results on the host.
#include <string.h>

#include "lane_util.h"
#include "nullifier_set.h"
#include "zkmi_internal.h"

struct zkmi_nullifier_set {
  zkmi_ctx* ctx = nullptr;
  uint64_t capacity = 0, slots = 0, count = 0;  // count is kept on the host: only spend changes it
  uint32_t* d_log = nullptr;    // capacity x 8 words, insertion order
  uint32_t* d_table = nullptr;  // slots entries: log index + 1, 0 = empty
  ~zkmi_nullifier_set() {
    if (d_log) (void)hipFree(d_log);
    if (d_table) (void)hipFree(d_table);
  }
};

namespace zk {

constexpr int NSB = 256;
// a call of at most NS_ONE_WG transfers runs all its rounds in one launch of one workgroup
constexpr uint32_t NS_ONE_WG = 128;
static unsigned ns_blocks(uint64_t n) { return (unsigned)((n + NSB - 1) / NSB); }

// counters of a call (u32 words)
enum { NS_C_UNDECIDED = 0, NS_C_ACCEPTED = 1, NS_C_ROUNDS = 2, NS_C_GAVE_UP = 3, NS_C_WORDS = 4 };

// out[i] = 1 when keys[i] is stored, one lane per key
__global__ void __launch_bounds__(NSB) k_ns_contains(const uint32_t* __restrict__ table, uint64_t slots,
                                                     const uint32_t* __restrict__ log,
                                                     const uint32_t* __restrict__ keys, uint64_t n,
                                                     uint8_t* __restrict__ out) {
  const uint64_t i = blockIdx.x * (uint64_t)NSB + threadIdx.x;
  if (i >= n) return;
  out[i] = ns_find(table, slots, log, ns_load(keys + 8 * i)) != 0;
}

// Lookup and grouping, one lane per key of an eligible transfer: the key's
// stored / repeated-in-its-transfer bit into flags[t] (zeroed beforehand), and
// its group from the scratch table (zeroed beforehand).  The keys of a skipped
// transfer enter nothing.
__global__ void __launch_bounds__(NSB) k_ns_lookup(const uint32_t* __restrict__ table, uint64_t slots,
                                                   const uint32_t* __restrict__ log, const uint32_t* __restrict__ keys,
                                                   const uint8_t* __restrict__ eligible, uint32_t nkeys,
                                                   uint32_t per_tx, uint32_t* scratch, uint64_t sslots,
                                                   uint32_t* flags, uint32_t* __restrict__ group, uint32_t* ctr) {
  const uint32_t i = blockIdx.x * NSB + threadIdx.x;
  if (i >= nkeys) return;
  const uint32_t t = i / per_tx, k = i % per_tx;
  if (eligible && !eligible[t]) return;
  uint32_t f = ns_dup_flag(keys + 8 * (uint64_t)t * per_tx, k);
  if (ns_find(table, slots, log, ns_load(keys + 8 * (uint64_t)i))) f |= ns_flag_stored(k);
  if (f) atomicOr(flags + t, f);
  const uint32_t g = ns_group(scratch, sslots, keys, i);
  if (g == NS_NONE) atomicOr(ctr + NS_C_GAVE_UP, 1u);
  group[i] = g == NS_NONE ? i : g;
}

// the states the rounds start from, one lane per transfer; counts the undecided
__global__ void __launch_bounds__(NSB) k_ns_init(const uint8_t* __restrict__ eligible,
                                                 const uint32_t* __restrict__ flags, uint32_t ntx,
                                                 uint32_t* __restrict__ state, uint32_t* ctr) {
  const uint32_t t = blockIdx.x * NSB + threadIdx.x;
  const bool active = t < ntx;
  uint32_t st = NS_ST_SKIPPED;
  if (active) state[t] = st = ns_state0(!eligible || eligible[t], flags[t]);
  const int und = __syncthreads_count(st == NS_ST_UNDECIDED);
  if (threadIdx.x == 0 && und) atomicAdd(ctr + NS_C_UNDECIDED, (uint32_t)und);
}

// First half of a round of a call of many transfers, one lane per key: the
// minima of its group over the states as they stand (cand is reset to NS_NONE
// before every round; acc only ever falls, so it is set once).
__global__ void __launch_bounds__(NSB) k_ns_min(const uint32_t* __restrict__ state, const uint32_t* __restrict__ group,
                                                uint32_t nkeys, uint32_t per_tx, uint32_t* cand, uint32_t* acc) {
  const uint32_t i = blockIdx.x * NSB + threadIdx.x;
  if (i >= nkeys) return;
  const uint32_t t = i / per_tx, st = state[t];
  if (st == NS_ST_SKIPPED || st == NS_ST_REJECTED) return;
  const uint32_t g = group[i];
  if (cand) atomicMin(cand + g, t);
  if (st == NS_ST_ACCEPTED) atomicMin(acc + g, t);
}
// Second half, one lane per transfer: ns_decide over the minima.  A lane
// writes its own state only and k_ns_min has ended, so every decision of this
// round reads the states of the round before.
__global__ void __launch_bounds__(NSB) k_ns_decide(uint32_t* state, const uint32_t* __restrict__ group, uint32_t ntx,
                                                   uint32_t per_tx, const uint32_t* __restrict__ cand,
                                                   const uint32_t* __restrict__ acc, uint32_t* ctr) {
  const uint32_t t = blockIdx.x * NSB + threadIdx.x;
  uint32_t st = NS_ST_SKIPPED;
  if (t < ntx && (st = state[t]) == NS_ST_UNDECIDED) {
    uint32_t c[NS_MAX_PER_TX], a[NS_MAX_PER_TX];
    for (uint32_t k = 0; k < per_tx; k++) {
      const uint32_t g = group[(uint64_t)t * per_tx + k];
      c[k] = cand[g], a[k] = acc[g];
    }
    st = ns_decide(t, per_tx, c, a);
    if (st != NS_ST_UNDECIDED) state[t] = st;
  }
  const int und = __syncthreads_count(st == NS_ST_UNDECIDED);
  if (threadIdx.x == 0 && und) atomicAdd(ctr + NS_C_UNDECIDED, (uint32_t)und);
}

// All rounds of a call of at most NS_ONE_WG transfers: one workgroup, a lane
// per transfer, the minima in LDS, a barrier between the halves of a round (as
// account_tree.hip's k_at_levels steps through its levels).  Leaves the final
// states, the final acc of every group and the number of rounds.
__global__ void __launch_bounds__(NS_ONE_WG) k_ns_rounds(uint32_t* state, const uint32_t* __restrict__ group,
                                                         uint32_t ntx, uint32_t per_tx, uint32_t* __restrict__ acc,
                                                         uint32_t* ctr) {
  __shared__ uint32_t cand_s[NS_ONE_WG * NS_MAX_PER_TX], acc_s[NS_ONE_WG * NS_MAX_PER_TX];
  const uint32_t t = threadIdx.x, nkeys = ntx * per_tx;
  uint32_t st = t < ntx ? state[t] : NS_ST_SKIPPED;
  uint32_t g[NS_MAX_PER_TX] = {0, 0, 0, 0};
  if (st != NS_ST_SKIPPED)
    for (uint32_t k = 0; k < per_tx; k++) g[k] = group[t * per_tx + k];
  for (uint32_t i = t; i < nkeys; i += NS_ONE_WG) acc_s[i] = NS_NONE;
  uint32_t rounds = 0;
  for (; rounds < ntx; rounds++) {  // every round decides a transfer: at most ntx rounds
    if (__syncthreads_count(st == NS_ST_UNDECIDED) == 0) break;
    for (uint32_t i = t; i < nkeys; i += NS_ONE_WG) cand_s[i] = NS_NONE;
    __syncthreads();
    if (st == NS_ST_UNDECIDED || st == NS_ST_ACCEPTED)
      for (uint32_t k = 0; k < per_tx; k++) {
        atomicMin(cand_s + g[k], t);
        if (st == NS_ST_ACCEPTED) atomicMin(acc_s + g[k], t);
      }
    __syncthreads();
    if (st == NS_ST_UNDECIDED) {
      uint32_t c[NS_MAX_PER_TX], a[NS_MAX_PER_TX];
      for (uint32_t k = 0; k < per_tx; k++) c[k] = cand_s[g[k]], a[k] = acc_s[g[k]];
      st = ns_decide(t, per_tx, c, a);
    }
  }
  __syncthreads();
  if (st == NS_ST_ACCEPTED)  // the transfers accepted by the last round
    for (uint32_t k = 0; k < per_tx; k++) atomicMin(acc_s + g[k], t);
  const int left = __syncthreads_count(st == NS_ST_UNDECIDED);  // 0: every round decides a transfer
  if (t < ntx) state[t] = st;
  for (uint32_t i = t; i < nkeys; i += NS_ONE_WG) acc[i] = acc_s[i];
  if (t == 0) ctr[NS_C_ROUNDS] = rounds, ctr[NS_C_UNDECIDED] = (uint32_t)left;
}

// Verdicts, one lane per transfer, from the final states and the final acc;
// block_acc[b] = the accepted transfers of block b.
__global__ void __launch_bounds__(NSB) k_ns_reasons(const uint32_t* __restrict__ state,
                                                    const uint32_t* __restrict__ flags,
                                                    const uint32_t* __restrict__ group,
                                                    const uint32_t* __restrict__ acc, uint32_t ntx, uint32_t per_tx,
                                                    uint32_t* __restrict__ verdict, uint32_t* __restrict__ detail,
                                                    uint32_t* __restrict__ block_acc) {
  const uint32_t t = blockIdx.x * NSB + threadIdx.x;
  uint32_t st = NS_ST_SKIPPED;
  if (t < ntx) {
    st = state[t];
    uint32_t v = st == NS_ST_ACCEPTED ? NS_ACCEPTED : NS_SKIPPED, d = 0;
    if (st == NS_ST_REJECTED) {
      uint32_t a[NS_MAX_PER_TX];
      for (uint32_t k = 0; k < per_tx; k++) a[k] = acc[group[(uint64_t)t * per_tx + k]];
      v = ns_reason(t, per_tx, flags[t], a, &d);
    }
    verdict[t] = v;
    detail[t] = d;
  }
  const int n = __syncthreads_count(st == NS_ST_ACCEPTED);
  if (threadIdx.x == 0) block_acc[blockIdx.x] = (uint32_t)n;
}

// Insert, one lane per transfer (the blocks of k_ns_reasons, block_acc turned
// into offsets by k_block_offsets): accepted transfer t, the rank-th accepted
// one of the call, writes its keys to the log at count + rank per_tx + k and
// enters them in the table.  No two inserted keys are equal and none is
// stored, so ns_insert claims without comparing.
__global__ void __launch_bounds__(NSB) k_ns_insert(uint32_t* table, uint64_t slots, uint32_t* log, uint64_t count,
                                                   const uint32_t* __restrict__ keys,
                                                   const uint32_t* __restrict__ state,
                                                   const uint32_t* __restrict__ block_off, uint32_t ntx,
                                                   uint32_t per_tx, uint32_t* ctr) {
  __shared__ uint32_t wave_s[NSB / 64];
  const uint32_t t = blockIdx.x * NSB + threadIdx.x;
  const bool ins = t < ntx && state[t] == NS_ST_ACCEPTED;
  const uint32_t rank = block_rank<NSB>(ins, block_off + blockIdx.x, wave_s);
  if (!ins) return;
  for (uint32_t k = 0; k < per_tx; k++) {
    const NsKey key = ns_load(keys + 8 * ((uint64_t)t * per_tx + k));
    const uint64_t index = count + (uint64_t)rank * per_tx + k;
    ns_put(log + 8 * index, key);
    if (!ns_insert(table, slots, key, (uint32_t)index)) atomicOr(ctr + NS_C_GAVE_UP, 1u);
  }
}

static int ns_contains(zkmi_ctx* ctx, const zkmi_nullifier_set* s, size_t n, const uint8_t* keys, uint8_t* out) {
  uint32_t* d_keys;
  uint8_t* d_out;
  ZK_TRY(ctx->ws.get("ns_keys", n * 32, (void**)&d_keys));
  ZK_TRY(ctx->ws.get("ns_out", n, (void**)&d_out));
  ZK_HIP(hipMemcpyAsync(d_keys, keys, n * 32, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "nullifier_set_contains");
    k_ns_contains<<<ns_blocks(n), NSB, 0, ctx->stream>>>(s->d_table, s->slots, s->d_log, d_keys, n, d_out);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return timer_flush(ctx);
}

// arguments already checked; ntx >= 1
static int ns_spend(zkmi_ctx* ctx, zkmi_nullifier_set* s, uint32_t ntx, uint32_t per_tx, const uint8_t* keys,
                    const uint8_t* eligible, uint32_t* verdict, uint32_t* detail, uint32_t* rounds_out) {
  const uint32_t nkeys = ntx * per_tx, nblocks = ns_blocks(ntx);
  const uint64_t sslots = ns_slots_for(nkeys);
  uint32_t *d_keys, *d_scratch, *d_flags, *d_group, *d_state, *d_cand, *d_acc, *d_verdict, *d_detail, *d_block, *d_ctr;
  uint8_t* d_elig = nullptr;
  ZK_TRY(ctx->ws.get("ns_keys", (size_t)nkeys * 32, (void**)&d_keys));
  ZK_TRY(ctx->ws.get("ns_call_table", sslots * 4, (void**)&d_scratch));
  ZK_TRY(ctx->ws.get("ns_flags", (size_t)ntx * 4, (void**)&d_flags));
  ZK_TRY(ctx->ws.get("ns_group", (size_t)nkeys * 4, (void**)&d_group));
  ZK_TRY(ctx->ws.get("ns_state", (size_t)ntx * 4, (void**)&d_state));
  ZK_TRY(ctx->ws.get("ns_cand", (size_t)nkeys * 4, (void**)&d_cand));
  ZK_TRY(ctx->ws.get("ns_acc", (size_t)nkeys * 4, (void**)&d_acc));
  ZK_TRY(ctx->ws.get("ns_verdict", (size_t)ntx * 4, (void**)&d_verdict));
  ZK_TRY(ctx->ws.get("ns_detail", (size_t)ntx * 4, (void**)&d_detail));
  ZK_TRY(ctx->ws.get("ns_block", (size_t)nblocks * 4, (void**)&d_block));
  ZK_TRY(ctx->ws.get("ns_ctr", NS_C_WORDS * 4, (void**)&d_ctr));
  if (eligible) {
    ZK_TRY(ctx->ws.get("ns_elig", ntx, (void**)&d_elig));
    ZK_HIP(hipMemcpyAsync(d_elig, eligible, ntx, hipMemcpyHostToDevice, ctx->stream));
  }
  ZK_HIP(hipMemcpyAsync(d_keys, keys, (size_t)nkeys * 32, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemsetAsync(d_scratch, 0, sslots * 4, ctx->stream));
  ZK_HIP(hipMemsetAsync(d_flags, 0, (size_t)ntx * 4, ctx->stream));
  ZK_HIP(hipMemsetAsync(d_ctr, 0, NS_C_WORDS * 4, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "nullifier_set_lookup");
    k_ns_lookup<<<ns_blocks(nkeys), NSB, 0, ctx->stream>>>(s->d_table, s->slots, s->d_log, d_keys, d_elig, nkeys,
                                                           per_tx, d_scratch, sslots, d_flags, d_group, d_ctr);
    k_ns_init<<<nblocks, NSB, 0, ctx->stream>>>(d_elig, d_flags, ntx, d_state, d_ctr);
  }
  ZK_HIP(hipGetLastError());
  uint32_t ctr[NS_C_WORDS] = {0, 0, 0, 0};
  uint32_t rounds = 0;
  {
    ScopedKernelTimer tm(ctx, "nullifier_set_rounds");
    if (ntx <= NS_ONE_WG) {
      k_ns_rounds<<<1, NS_ONE_WG, 0, ctx->stream>>>(d_state, d_group, ntx, per_tx, d_acc, d_ctr);
    } else {
      ZK_HIP(hipMemsetAsync(d_acc, 0xFF, (size_t)nkeys * 4, ctx->stream));
      ZK_HIP(hipMemcpyAsync(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, ctx->stream));
      ZK_HIP(hipStreamSynchronize(ctx->stream));
      // every round decides a transfer, so the bound is never what ends the loop
      for (; ctr[NS_C_UNDECIDED] != 0 && rounds < ntx; rounds++) {
        ZK_HIP(hipMemsetAsync(d_cand, 0xFF, (size_t)nkeys * 4, ctx->stream));
        ZK_HIP(hipMemsetAsync(d_ctr + NS_C_UNDECIDED, 0, 4, ctx->stream));
        k_ns_min<<<ns_blocks(nkeys), NSB, 0, ctx->stream>>>(d_state, d_group, nkeys, per_tx, d_cand, d_acc);
        k_ns_decide<<<nblocks, NSB, 0, ctx->stream>>>(d_state, d_group, ntx, per_tx, d_cand, d_acc, d_ctr);
        ZK_HIP(hipGetLastError());
        ZK_HIP(hipMemcpyAsync(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(hipStreamSynchronize(ctx->stream));
      }
      // the transfers accepted by the last round
      k_ns_min<<<ns_blocks(nkeys), NSB, 0, ctx->stream>>>(d_state, d_group, nkeys, per_tx, nullptr, d_acc);
    }
  }
  ZK_HIP(hipGetLastError());
  {
    ScopedKernelTimer tm(ctx, "nullifier_set_reasons");
    k_ns_reasons<<<nblocks, NSB, 0, ctx->stream>>>(d_state, d_flags, d_group, d_acc, ntx, per_tx, d_verdict, d_detail,
                                                   d_block);
    k_block_offsets<NSB><<<1, NSB, 0, ctx->stream>>>(d_block, nblocks, d_ctr + NS_C_ACCEPTED);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  if (ntx <= NS_ONE_WG) rounds = ctr[NS_C_ROUNDS];
  if (ctr[NS_C_GAVE_UP] || ctr[NS_C_UNDECIDED]) {  // cannot happen: the scratch table has 2 slots a key
    set_error("zkmi_nullifier_set_spend: the grouping gave up on a probe, or the rounds did not end");
    return ZKMI_EHIP;
  }
  // nothing of the set has been written so far
  const uint64_t add = (uint64_t)ctr[NS_C_ACCEPTED] * per_tx;
  if (s->count + add > s->capacity) {
    ZK_TRY(timer_flush(ctx));
    set_error("zkmi_nullifier_set_spend: %llu accepted keys beside the %llu held, past the capacity %llu",
              (unsigned long long)add, (unsigned long long)s->count, (unsigned long long)s->capacity);
    return ZKMI_ENOMEM;
  }
  if (add) {
    ScopedKernelTimer tm(ctx, "nullifier_set_insert");
    k_ns_insert<<<nblocks, NSB, 0, ctx->stream>>>(s->d_table, s->slots, s->d_log, s->count, d_keys, d_state, d_block,
                                                  ntx, per_tx, d_ctr);
  }
  // From here on the set may have changed: the stream is synchronised on every
  // path, and the host's count follows the log whenever the insert was queued.
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(verdict, d_verdict, (size_t)ntx * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(detail, d_detail, (size_t)ntx * 4, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(ctr, d_ctr, sizeof ctr, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    set_error("zkmi_nullifier_set_spend: HIP error %s after the insert was launched", hipGetErrorString(e));
    return ZKMI_EHIP;
  }
  s->count += add;
  ZK_TRY(timer_flush(ctx));
  if (ctr[NS_C_GAVE_UP]) {  // cannot happen: slots >= 2 capacity
    set_error("zkmi_nullifier_set_spend: the table gave up on a probe");
    return ZKMI_EHIP;
  }
  if (rounds_out) *rounds_out = rounds;
  return 0;
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkmi_nullifier_set_create(zkmi_ctx* ctx, uint64_t capacity, zkmi_nullifier_set** out) {
  if (!ctx || !out) {
    set_error("zkmi_nullifier_set_create: null argument");
    return ZKMI_EINVAL;
  }
  if (capacity == 0 || capacity > NS_MAX_CAPACITY) {
    set_error("zkmi_nullifier_set_create: capacity %llu outside 1..2^31", (unsigned long long)capacity);
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  zkmi_nullifier_set* s = new zkmi_nullifier_set;
  s->ctx = ctx;
  s->capacity = capacity;
  s->slots = ns_slots_for(capacity);
  if (hipMalloc((void**)&s->d_log, capacity * 32) != hipSuccess ||
      hipMalloc((void**)&s->d_table, s->slots * 4) != hipSuccess) {
    (void)hipGetLastError();
    delete s;
    set_error("zkmi_nullifier_set_create: hipMalloc of a set of %llu keys failed", (unsigned long long)capacity);
    return ZKMI_ENOMEM;
  }
  hipError_t e = hipMemsetAsync(s->d_table, 0, s->slots * 4, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    delete s;
    set_error("zkmi_nullifier_set_create: clearing the table failed (%s)", hipGetErrorString(e));
    return ZKMI_EHIP;
  }
  *out = s;
  return 0;
}
void zkmi_nullifier_set_destroy(zkmi_nullifier_set* s) {
  if (!s) return;
  ZK_DEVICE_GUARD(s->ctx);
  delete s;
}
int zkmi_nullifier_set_info(const zkmi_nullifier_set* s, uint64_t out[3]) {
  if (!s || !out) {
    set_error("zkmi_nullifier_set_info: null argument");
    return ZKMI_EINVAL;
  }
  out[0] = s->capacity;
  out[1] = s->slots;
  out[2] = s->count;
  return 0;
}

int zkmi_nullifier_set_contains(zkmi_ctx* ctx, const zkmi_nullifier_set* s, size_t n, const uint8_t* keys,
                                uint8_t* out) {
  if (!zk_owned("zkmi_nullifier_set_contains", "set", ctx, s ? s->ctx : nullptr)) return ZKMI_EINVAL;
  if (n > NS_MAX_CALL_KEYS) {
    set_error("zkmi_nullifier_set_contains: %zu keys in one call (at most 2^24)", n);
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  if (!keys || !out) {
    set_error("zkmi_nullifier_set_contains: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return ns_contains(ctx, s, n, keys, out);
}

int zkmi_nullifier_set_spend(zkmi_ctx* ctx, zkmi_nullifier_set* s, size_t ntx, uint32_t per_tx, const uint8_t* keys,
                             const uint8_t* eligible, uint32_t* verdict, uint32_t* detail, uint32_t* rounds) {
  if (!zk_owned("zkmi_nullifier_set_spend", "set", ctx, s ? s->ctx : nullptr)) return ZKMI_EINVAL;
  if (per_tx < 1 || per_tx > NS_MAX_PER_TX) {
    set_error("zkmi_nullifier_set_spend: per_tx %u outside 1..%u", per_tx, NS_MAX_PER_TX);
    return ZKMI_EINVAL;
  }
  if (ntx > NS_MAX_CALL_KEYS / per_tx) {
    set_error("zkmi_nullifier_set_spend: %zu transfers of %u keys in one call (at most 2^24 keys)", ntx, per_tx);
    return ZKMI_EINVAL;
  }
  if (ntx == 0) {
    if (rounds) *rounds = 0;
    return 0;
  }
  if (!keys || !verdict || !detail) {
    set_error("zkmi_nullifier_set_spend: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return ns_spend(ctx, s, (uint32_t)ntx, per_tx, keys, eligible, verdict, detail, rounds);
}

int zkmi_nullifier_set_log(zkmi_ctx* ctx, const zkmi_nullifier_set* s, uint64_t first, size_t n, uint8_t* out) {
  if (!zk_owned("zkmi_nullifier_set_log", "set", ctx, s ? s->ctx : nullptr)) return ZKMI_EINVAL;
  if (first > s->count || n > s->count - first) {
    set_error("zkmi_nullifier_set_log: [%llu, +%zu) of a log of %llu keys", (unsigned long long)first, n,
              (unsigned long long)s->count);
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  if (!out) {
    set_error("zkmi_nullifier_set_log: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  ZK_HIP(hipMemcpyAsync(out, s->d_log + 8 * first, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
