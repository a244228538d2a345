// account_tree.hip — batched MiMC hashing and the account tree resident in HBM
// (zkmi.h "MiMC hashing / account tree").  The arithmetic,
// the ordering rule and the node store's probes are mimc_hash.h's; this file
// holds the kernels, the launch sequence of an apply and the C entry points.
// Everything runs on the context stream, and every call returns with its
// results on the host.
#include <string.h>

#include <vector>

#include "hashers.h"
#include "lane_util.h"

struct zkmi_account_tree {
  zkmi_ctx* ctx = nullptr;
  const zkmi_mimc* mh = nullptr;
  uint32_t depth = 0;
  uint64_t max_nodes = 0, count = 0;             // slots of the store; nodes stored
  uint32_t empty[(zk::AT_MAX_DEPTH + 1) * 8];    // e_0 .. e_depth, canonical
  uint64_t root[4];
  uint64_t* d_keys = nullptr;
  uint32_t* d_vals = nullptr;
  uint32_t* d_empty = nullptr;
  unsigned long long* d_counter = nullptr;  // [0] nodes stored, [1] a write-back probe gave up
  ~zkmi_account_tree() {
    if (d_keys) (void)hipFree(d_keys);
    if (d_vals) (void)hipFree(d_vals);
    if (d_empty) (void)hipFree(d_empty);
    if (d_counter) (void)hipFree(d_counter);
  }
};

namespace zk {

constexpr int ATB = 128;
// a call of at most AT_ONE_WG writes steps through all levels in one launch of one workgroup
constexpr uint32_t AT_ONE_WG = ATB;
// positions of the ordering pass go through LDS in tiles of AT_TILE
constexpr uint32_t AT_TILE = 1024;
static unsigned at_blocks(uint64_t n) { return (unsigned)((n + ATB - 1) / ATB); }

// node of level l above `pos` (level 32 of a depth-32 tree is the root, index 0)
__device__ __forceinline__ uint64_t at_ancestor_key(uint32_t pos, uint32_t l) {
  return at_key(l, l >= 32 ? 0u : pos >> l);
}

// out[i] = hash_arity(in[i * arity .. i * arity + arity)), one lane per hash
__global__ void __launch_bounds__(ATB) k_mimc_hash_many(const Fe* __restrict__ tab, const uint32_t* __restrict__ in,
                                                        uint32_t* __restrict__ out, size_t n, uint32_t arity) {
  __shared__ Fe tab_s[MIMC_NTABLE];
  fe_table_lds(tab_s, tab, MIMC_NTABLE);
  const size_t i = blockIdx.x * (size_t)ATB + threadIdx.x;
  if (i >= n) return;
  mimc_hash(in + i * arity * 8, arity, out + i * 8, tab_s);
}

// Ordering pass, one lane per write k, one pass over all j != k with the
// positions tiled through LDS, latest first.  pred[k (depth + 1) + l + 1], l =
// -1 .. depth - 1 (set to -1 = "stored" beforehand): the first j < k met with
// at_hb == l is the latest one; a bit mask of the levels already found stands
// in for a per-level array, so nothing is indexed by level but global memory
// (at most depth + 1 stores a lane).  mlast[k] = m_k, the least at_hb over j > k.
__global__ void __launch_bounds__(ATB) k_at_order(const uint32_t* __restrict__ pos, uint32_t K, uint32_t depth,
                                                  int32_t* __restrict__ pred, int32_t* __restrict__ mlast) {
  __shared__ uint32_t tile[AT_TILE];
  const uint32_t k = blockIdx.x * ATB + threadIdx.x;
  const bool active = k < K;
  const uint32_t pk = active ? pos[k] : 0;
  uint64_t seen = 0;
  int m = (int)depth;
  for (uint32_t t = (K + AT_TILE - 1) / AT_TILE; t-- > 0;) {
    const uint32_t base = t * AT_TILE, cnt = K - base < AT_TILE ? K - base : AT_TILE;
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < cnt; i += ATB) tile[i] = pos[base + i];
    __syncthreads();
    if (!active) continue;
    for (uint32_t i = cnt; i-- > 0;) {
      const uint32_t j = base + i;
      const int h = at_hb(tile[i], pk);
      if (j > k) {
        m = h < m ? h : m;
      } else if (j < k) {
        const uint64_t bit = 1ull << (h + 1);
        if (!(seen & bit)) {
          seen |= bit;
          pred[(size_t)k * (depth + 1) + (uint32_t)(h + 1)] = (int32_t)j;
        }
      }
    }
  }
  if (active) mlast[k] = m;
}

// Stored nodes, one lane per (write, s = 0 .. depth).  s = 0: the leaf's own
// version (the raw value mod r) and, with no earlier write of the same leaf,
// the stored leaf it replaces; s = l + 1: with no predecessor, the stored
// level-l sibling.  ver: level-major, version of write k at level l at
// (l K + k) 8; sib: (k depth + l) 8; old: k 8.
__global__ void __launch_bounds__(ATB) k_at_gather(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                   uint64_t slots, const uint32_t* __restrict__ empty,
                                                   const uint32_t* __restrict__ pos, const uint32_t* __restrict__ raw,
                                                   uint32_t K, uint32_t depth, const int32_t* __restrict__ pred,
                                                   uint32_t* __restrict__ ver, uint32_t* __restrict__ sib,
                                                   uint32_t* __restrict__ old) {
  const uint64_t t = blockIdx.x * (uint64_t)ATB + threadIdx.x;
  if (t >= (uint64_t)K * (depth + 1)) return;
  const uint32_t k = (uint32_t)(t / (depth + 1)), s = (uint32_t)(t % (depth + 1));
  const uint32_t p = pos[k];
  if (s == 0) fr_canon(raw + (size_t)k * 8, ver + (size_t)k * 8);
  if (pred[t] >= 0) return;
  if (s == 0) copy8(old + (size_t)k * 8, at_node(keys, vals, slots, empty, at_key(0, p)));
  else copy8(sib + ((size_t)k * depth + (s - 1)) * 8, at_node(keys, vals, slots, empty, at_sibling_key(p, s - 1)));
}

// One level step of write k: its version at level l + 1 from its version at
// level l and the sibling as it sees it, the predecessor's level-l version or
// the gathered stored node.  The sibling (and at level 0 the replaced leaf)
// taken from a predecessor is written to the outputs here.
__device__ __forceinline__ void at_level_lane(uint32_t k, uint32_t l, const uint32_t* __restrict__ pos, uint32_t K,
                                              uint32_t depth, const int32_t* __restrict__ pred, uint32_t* ver,
                                              uint32_t* sib, uint32_t* old, const Fe* tab) {
  const int32_t* pk = pred + (size_t)k * (depth + 1);
  if (l == 0 && pk[0] >= 0) copy8(old + (size_t)k * 8, ver + (size_t)pk[0] * 8);
  uint32_t* mine = sib + ((size_t)k * depth + l) * 8;
  const int32_t j = pk[l + 1];
  if (j >= 0) copy8(mine, ver + ((size_t)l * K + (uint32_t)j) * 8);
  at_step(ver + ((size_t)l * K + k) * 8, mine, pos[k], l, ver + ((size_t)(l + 1) * K + k) * 8, tab);
}
// one level of a call of many writes
__global__ void __launch_bounds__(ATB) k_at_level(const Fe* __restrict__ tab, const uint32_t* __restrict__ pos,
                                                  uint32_t K, uint32_t depth, uint32_t l,
                                                  const int32_t* __restrict__ pred, uint32_t* ver, uint32_t* sib,
                                                  uint32_t* old) {
  __shared__ Fe tab_s[MIMC_NTABLE];
  fe_table_lds(tab_s, tab, MIMC_NTABLE);
  const uint32_t k = blockIdx.x * ATB + threadIdx.x;
  if (k >= K) return;
  at_level_lane(k, l, pos, K, depth, pred, ver, sib, old, tab_s);
}
// all levels of a call of at most AT_ONE_WG writes: one workgroup, a barrier
// between levels (as note_tree.hip's k_nt_tail steps through its levels)
__global__ void __launch_bounds__(ATB) k_at_levels(const Fe* __restrict__ tab, const uint32_t* __restrict__ pos,
                                                   uint32_t K, uint32_t depth, const int32_t* __restrict__ pred,
                                                   uint32_t* ver, uint32_t* sib, uint32_t* old) {
  __shared__ Fe tab_s[MIMC_NTABLE];
  fe_table_lds(tab_s, tab, MIMC_NTABLE);
  for (uint32_t l = 0; l < depth; l++) {
    if (threadIdx.x < K) at_level_lane(threadIdx.x, l, pos, K, depth, pred, ver, sib, old, tab_s);
    __syncthreads();
  }
}

// Write-back, one lane per (write, level 0 .. depth): write k stores its
// versions of the levels 0 .. m_k.  Every node has one last writer, so no two
// lanes store the same key; lanes that claim new slots at once are kept apart
// by at_claim's compare-and-swap.
__global__ void __launch_bounds__(ATB) k_at_writeback(uint64_t* keys, uint32_t* vals, uint64_t slots,
                                                      const uint32_t* __restrict__ pos,
                                                      const int32_t* __restrict__ mlast, uint32_t K, uint32_t depth,
                                                      const uint32_t* __restrict__ ver, unsigned long long* counter) {
  const uint64_t t = blockIdx.x * (uint64_t)ATB + threadIdx.x;
  if (t >= (uint64_t)K * (depth + 1)) return;
  const uint32_t k = (uint32_t)(t / (depth + 1)), l = (uint32_t)(t % (depth + 1));
  if ((int32_t)l > mlast[k]) return;
  bool fresh;
  const int64_t s = at_claim(keys, slots, at_ancestor_key(pos[k], l), &fresh);
  if (s < 0) {
    atomicOr(counter + 1, 1ull);
    return;
  }
  if (fresh) atomicAdd(counter, 1ull);
  copy8(vals + 8 * s, ver + ((size_t)l * K + k) * 8);
}

// mode 0: out[(i depth + l) 8 ..] = the sibling of positions[i]'s path at level l, lane per (i, l);
// mode 1: out[i 8 ..] = the leaf at positions[i], lane per i
__global__ void __launch_bounds__(ATB) k_at_lookup(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                   uint64_t slots, const uint32_t* __restrict__ empty,
                                                   const uint32_t* __restrict__ pos, uint64_t n, uint32_t depth,
                                                   int mode, uint32_t* __restrict__ out) {
  const uint64_t t = blockIdx.x * (uint64_t)ATB + threadIdx.x;
  const uint32_t per = mode == 0 ? depth : 1;
  if (t >= n * per) return;
  const uint32_t p = pos[t / per], l = (uint32_t)(t % per);
  copy8(out + t * 8, at_node(keys, vals, slots, empty, mode == 0 ? at_sibling_key(p, l) : at_key(0, p)));
}

static int mimc_hash_many(zkmi_ctx* ctx, const zkmi_mimc* mh, size_t n, uint32_t arity, const uint64_t* in,
                          uint64_t* out) {
  return hasher_hash_many(ctx, "mh_in", "mh_out", "mimc_hash_many", n, arity, in, out,
                          [&](const uint32_t* d_in, uint32_t* d_out) {
    k_mimc_hash_many<<<at_blocks(n), ATB, 0, ctx->stream>>>(mh->d_table, d_in, d_out, n, arity);
  });
}

// positions already checked and narrowed; K in 1 .. AT_MAX_WRITES
static int account_tree_apply(zkmi_ctx* ctx, zkmi_account_tree* t, uint32_t K, const uint32_t* pos,
                              const uint64_t* leaves, uint64_t* siblings, uint64_t* old_leaves, uint64_t* roots) {
  const uint32_t depth = t->depth;
  const uint64_t lanes = (uint64_t)K * (depth + 1);
  uint32_t *d_pos, *d_raw, *d_ver, *d_sib, *d_old;
  int32_t *d_pred, *d_mlast;
  ZK_TRY(ctx->ws.get("at_pos", (size_t)K * 4, (void**)&d_pos));
  ZK_TRY(ctx->ws.get("at_raw", (size_t)K * 32, (void**)&d_raw));
  ZK_TRY(ctx->ws.get("at_pred", lanes * 4, (void**)&d_pred));
  ZK_TRY(ctx->ws.get("at_mlast", (size_t)K * 4, (void**)&d_mlast));
  ZK_TRY(ctx->ws.get("at_ver", lanes * 32, (void**)&d_ver));
  ZK_TRY(ctx->ws.get("at_sib", (size_t)K * depth * 32, (void**)&d_sib));
  ZK_TRY(ctx->ws.get("at_old", (size_t)K * 32, (void**)&d_old));
  ZK_HIP(hipMemcpyAsync(d_pos, pos, (size_t)K * 4, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_raw, leaves, (size_t)K * 32, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemsetAsync(d_pred, 0xFF, lanes * 4, ctx->stream));
  const Fe* tab = t->mh->d_table;
  {
    ScopedKernelTimer tm(ctx, "account_tree_order");
    k_at_order<<<at_blocks(K), ATB, 0, ctx->stream>>>(d_pos, K, depth, d_pred, d_mlast);
    k_at_gather<<<at_blocks(lanes), ATB, 0, ctx->stream>>>(t->d_keys, t->d_vals, t->max_nodes, t->d_empty, d_pos,
                                                          d_raw, K, depth, d_pred, d_ver, d_sib, d_old);
  }
  ZK_HIP(hipGetLastError());
  {
    ScopedKernelTimer tm(ctx, "account_tree_levels");
    if (K <= AT_ONE_WG) {
      k_at_levels<<<1, ATB, 0, ctx->stream>>>(tab, d_pos, K, depth, d_pred, d_ver, d_sib, d_old);
    } else {
      for (uint32_t l = 0; l < depth; l++)
        k_at_level<<<at_blocks(K), ATB, 0, ctx->stream>>>(tab, d_pos, K, depth, l, d_pred, d_ver, d_sib, d_old);
    }
  }
  ZK_HIP(hipGetLastError());
  {
    ScopedKernelTimer tm(ctx, "account_tree_writeback");
    k_at_writeback<<<at_blocks(lanes), ATB, 0, ctx->stream>>>(t->d_keys, t->d_vals, t->max_nodes, d_pos, d_mlast, K,
                                                             depth, d_ver, t->d_counter);
  }
  // From here on the table may have changed.  The copies below target this
  // frame (root, counter) and the caller's buffers, so the stream is
  // synchronised on EVERY path before the function returns, and the host's
  // root and node count follow the table whenever they could be read back.
  hipError_t e = hipGetLastError();
  const uint32_t* d_roots = d_ver + (size_t)depth * K * 8;
  unsigned long long counter[2] = {t->count, 0};
  uint64_t root[4];
  memcpy(root, t->root, 32);
  if (e == hipSuccess && siblings)
    e = hipMemcpyAsync(siblings, d_sib, (size_t)K * depth * 32, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && old_leaves)
    e = hipMemcpyAsync(old_leaves, d_old, (size_t)K * 32, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess && roots) e = hipMemcpyAsync(roots, d_roots, (size_t)K * 32, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(root, d_roots + (size_t)(K - 1) * 8, 32, hipMemcpyDeviceToHost, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(counter, t->d_counter, sizeof counter, hipMemcpyDeviceToHost, ctx->stream);
  const hipError_t es = hipStreamSynchronize(ctx->stream);
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) {
    set_error("zkmi_account_tree_apply: HIP error %s after the write-back was launched", hipGetErrorString(e));
    return ZKMI_EHIP;
  }
  t->count = counter[0];
  memcpy(t->root, root, 32);
  ZK_TRY(timer_flush(ctx));
  if (counter[1]) {  // cannot happen after the capacity check; cleared, so that one hit does not fail every later call
    (void)hipMemsetAsync(t->d_counter + 1, 0, sizeof(unsigned long long), ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    set_error("zkmi_account_tree_apply: the node store gave up on a probe");
    return ZKMI_EHIP;
  }
  return 0;
}

// positions (u64, ABI) checked against 2^depth and narrowed; false with the offending entry
static bool at_narrow(const uint64_t* positions, size_t n, uint32_t depth, std::vector<uint32_t>& out, size_t* bad) {
  out.resize(n);
  for (size_t i = 0; i < n; i++) {
    if (positions[i] >> depth) {
      *bad = i;
      return false;
    }
    out[i] = (uint32_t)positions[i];
  }
  return true;
}

static int account_tree_lookup(zkmi_ctx* ctx, const zkmi_account_tree* t, size_t n, const std::vector<uint32_t>& pos,
                               int mode, uint64_t* out) {
  const uint64_t lanes = (uint64_t)n * (mode == 0 ? t->depth : 1);
  uint32_t *d_pos, *d_out;
  ZK_TRY(ctx->ws.get("at_pos", n * 4, (void**)&d_pos));
  ZK_TRY(ctx->ws.get("at_sib", lanes * 32, (void**)&d_out));
  ZK_HIP(hipMemcpyAsync(d_pos, pos.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, mode == 0 ? "account_tree_paths" : "account_tree_leaves");
    k_at_lookup<<<at_blocks(lanes), ATB, 0, ctx->stream>>>(t->d_keys, t->d_vals, t->max_nodes, t->d_empty, d_pos, n,
                                                          t->depth, mode, d_out);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(out, d_out, lanes * 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return timer_flush(ctx);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkmi_mimc_create(zkmi_ctx* ctx, zkmi_mimc** out) {
  if (!ctx || !out) {
    set_error("zkmi_mimc_create: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  zkmi_mimc* mh = new zkmi_mimc;
  mh->ctx = ctx;
  mimc_table(mh->table);
  const int rc = hasher_upload_table("zkmi_mimc_create", ctx, mh->table, MIMC_NTABLE, &mh->d_table);
  if (rc != 0) {
    delete mh;
    return rc;
  }
  *out = mh;
  return 0;
}
void zkmi_mimc_destroy(zkmi_mimc* mh) {
  if (!mh) return;
  ZK_DEVICE_GUARD(mh->ctx);
  delete mh;
}

int zkmi_mimc_hash_many(zkmi_ctx* ctx, const zkmi_mimc* mh, size_t n, uint32_t arity, const uint64_t* in,
                        uint64_t* out) {
  if (!zk_owned("zkmi_mimc_hash_many", "hasher", ctx, mh ? mh->ctx : nullptr)) return ZKMI_EINVAL;
  if (arity < 1 || arity > 4) {
    set_error("zkmi_mimc_hash_many: arity %u outside 1..4", arity);
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  if (!in || !out) {
    set_error("zkmi_mimc_hash_many: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return mimc_hash_many(ctx, mh, n, arity, in, out);
}

int zkmi_account_tree_create(zkmi_ctx* ctx, const zkmi_mimc* mh, uint32_t depth, uint64_t max_nodes,
                             zkmi_account_tree** out) {
  if (!ctx || !mh || mh->ctx != ctx || !out) {
    set_error("zkmi_account_tree_create: null argument, or a hasher of another context");
    return ZKMI_EINVAL;
  }
  if (depth < 1 || depth > AT_MAX_DEPTH) {
    set_error("zkmi_account_tree_create: depth %u outside 1..%u", depth, AT_MAX_DEPTH);
    return ZKMI_EINVAL;
  }
  if (max_nodes == 0 || max_nodes > (1ull << 40)) {
    set_error("zkmi_account_tree_create: max_nodes %llu outside 1..2^40", (unsigned long long)max_nodes);
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  zkmi_account_tree* t = new zkmi_account_tree;
  t->ctx = ctx;
  t->mh = mh;
  t->depth = depth;
  t->max_nodes = max_nodes;
  memset(t->empty, 0, sizeof t->empty);
  for (uint32_t l = 0; l < depth; l++) mimc_pair(t->empty + 8 * l, t->empty + 8 * l, t->empty + 8 * l + 8, mh->table);
  memcpy(t->root, t->empty + 8 * depth, 32);
  const size_t empty_bytes = (depth + 1) * 32;
  if (hipMalloc((void**)&t->d_keys, max_nodes * 8) != hipSuccess ||
      hipMalloc((void**)&t->d_vals, max_nodes * 32) != hipSuccess ||
      hipMalloc((void**)&t->d_empty, empty_bytes) != hipSuccess ||
      hipMalloc((void**)&t->d_counter, 2 * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    delete t;
    set_error("zkmi_account_tree_create: hipMalloc of a store of %llu nodes failed", (unsigned long long)max_nodes);
    return ZKMI_ENOMEM;
  }
  hipError_t e = hipMemsetAsync(t->d_keys, 0xFF, max_nodes * 8, ctx->stream);  // AT_EMPTY_KEY in every slot
  if (e == hipSuccess) e = hipMemsetAsync(t->d_counter, 0, 2 * sizeof(unsigned long long), ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->d_empty, t->empty, empty_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    delete t;
    set_error("zkmi_account_tree_create: upload failed (%s)", hipGetErrorString(e));
    return ZKMI_EHIP;
  }
  *out = t;
  return 0;
}
void zkmi_account_tree_destroy(zkmi_account_tree* t) {
  if (!t) return;
  ZK_DEVICE_GUARD(t->ctx);
  delete t;
}
int zkmi_account_tree_info(const zkmi_account_tree* t, uint64_t out[3]) {
  if (!t || !out) {
    set_error("zkmi_account_tree_info: null argument");
    return ZKMI_EINVAL;
  }
  out[0] = t->depth;
  out[1] = t->max_nodes;
  out[2] = t->count;
  return 0;
}

int zkmi_account_tree_apply(zkmi_ctx* ctx, zkmi_account_tree* t, size_t n, const uint64_t* positions,
                            const uint64_t* leaves, uint64_t* siblings, uint64_t* old_leaves, uint64_t* roots) {
  if (!zk_owned("zkmi_account_tree_apply", "tree", ctx, t ? t->ctx : nullptr)) return ZKMI_EINVAL;
  if (n > AT_MAX_WRITES) {
    set_error("zkmi_account_tree_apply: %zu writes in one call (at most %u)", n, AT_MAX_WRITES);
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  if (!positions || !leaves) {
    set_error("zkmi_account_tree_apply: null argument");
    return ZKMI_EINVAL;
  }
  std::vector<uint32_t> pos;
  size_t bad = 0;
  if (!at_narrow(positions, n, t->depth, pos, &bad)) {
    set_error("zkmi_account_tree_apply: position %llu (entry %zu) of a tree of depth %u",
              (unsigned long long)positions[bad], bad, t->depth);
    return ZKMI_EINVAL;
  }
  if (t->count + at_worst_case_nodes(n, t->depth) > t->max_nodes) {
    set_error("zkmi_account_tree_apply: %zu writes could store %llu nodes beside the %llu held, past max_nodes %llu", n,
              (unsigned long long)at_worst_case_nodes(n, t->depth), (unsigned long long)t->count,
              (unsigned long long)t->max_nodes);
    return ZKMI_ENOMEM;
  }
  ZK_DEVICE_GUARD(ctx);
  return account_tree_apply(ctx, t, (uint32_t)n, pos.data(), leaves, siblings, old_leaves, roots);
}

int zkmi_account_tree_root(zkmi_ctx* ctx, const zkmi_account_tree* t, uint64_t out[4]) {
  if (!ctx || !t || t->ctx != ctx || !out) {
    set_error("zkmi_account_tree_root: null argument, or a tree of another context");
    return ZKMI_EINVAL;
  }
  memcpy(out, t->root, 32);  // kept on the host by every apply
  return 0;
}

static int at_lookup_entry(const char* what, zkmi_ctx* ctx, const zkmi_account_tree* t, size_t n,
                           const uint64_t* positions, int mode, uint64_t* out) {
  if (!zk_owned(what, "tree", ctx, t ? t->ctx : nullptr)) return ZKMI_EINVAL;
  if (n == 0) return 0;
  if (!positions || !out) {
    set_error("%s: null argument", what);
    return ZKMI_EINVAL;
  }
  std::vector<uint32_t> pos;
  size_t bad = 0;
  if (!at_narrow(positions, n, t->depth, pos, &bad)) {
    set_error("%s: position %llu (entry %zu) of a tree of depth %u", what, (unsigned long long)positions[bad], bad,
              t->depth);
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return account_tree_lookup(ctx, t, n, pos, mode, out);
}
int zkmi_account_tree_paths(zkmi_ctx* ctx, const zkmi_account_tree* t, size_t n, const uint64_t* positions,
                            uint64_t* siblings) {
  return at_lookup_entry("zkmi_account_tree_paths", ctx, t, n, positions, 0, siblings);
}
int zkmi_account_tree_leaves(zkmi_ctx* ctx, const zkmi_account_tree* t, size_t n, const uint64_t* positions,
                             uint64_t* out) {
  return at_lookup_entry("zkmi_account_tree_leaves", ctx, t, n, positions, 1, out);
}

}  // extern "C"
