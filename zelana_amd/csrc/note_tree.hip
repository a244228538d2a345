// note_tree.hip — batched Poseidon hashing and the note commitment tree
// resident in HBM (zkmi.h "Poseidon hashing / note commitment tree",
// DESIGN.md §2.11).  The arithmetic is poseidon_hash.h's, one lane per hash;
// this file holds the kernels' lane mappings, the launch sequences and the C
// entry points.  Everything runs on the context stream, and every call
// returns with its results on the host.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "hashers.h"
#include "lane_util.h"

struct zkmi_note_tree {
  zkmi_ctx* ctx = nullptr;
  const zkmi_poseidon* ph = nullptr;
  uint32_t depth = 0;
  uint64_t capacity = 0, next = 0;
  zk::NtGeom geom;
  uint32_t empty[(zk::NT_MAX_DEPTH + 1) * 8];  // e_0 .. e_depth, canonical
  uint64_t root[4];                            // of the leaves [0, next)
  uint32_t* d_tree = nullptr;
  uint32_t* d_empty = nullptr;
  zk::NtGeom* d_geom = nullptr;
  ~zkmi_note_tree() {
    if (d_tree) (void)hipFree(d_tree);
    if (d_empty) (void)hipFree(d_empty);
    if (d_geom) (void)hipFree(d_geom);
  }
};

namespace zk {

constexpr int NTB = 128;
// a level of at most NT_TAIL nodes, and every level above it, is stepped
// through by ONE workgroup in one launch (k_nt_tail)
constexpr uint64_t NT_TAIL = NTB;
// A launch of at most NT_QUAD_MAX hashes runs a quad per hash: 4 x 16384 lanes
// are one wave on each of the 1024 SIMDs, so up to there a hash takes its own
// latency and nothing else, and the quad's is the shorter one.
constexpr uint64_t NT_QUAD_MAX = 16384;
static unsigned nt_blocks(uint64_t n) { return (unsigned)((n + NTB - 1) / NTB); }
static bool nt_quad(const zkmi_poseidon* ph, uint64_t n) { return ph->quad && n <= NT_QUAD_MAX; }

// ------------------------------------------------------------ quad mapping
// One permutation on a quad of lanes, the shape of wprog.hip's poseidon_quad
// without its trace: lane q < 3 holds state element q (lane 3 mirrors lane 2
// and stores nothing), the S-box runs on all lanes in full rounds and on lane
// 0 in partial ones, then every lane forms its MDS row from the three
// elements (DPP quad broadcasts).  A lane then runs ~4.7 field products a
// round where the lane-per-hash mapping runs 18 / 12: a hash finishes ~2.7x
// sooner, on 4x the lanes.  Used wherever the hashes of a launch are too few
// to fill the device (NT_QUAD_MAX), which is where latency is all there is:
// the narrow levels of an append, the per-insertion roots of a short append,
// a short hash_many.  All four lanes of a quad must be active.
// s: this lane's state element; qq = min(lane in quad, 2)
__device__ __forceinline__ void posh_permute_quad(Fe& s, uint32_t qq, const Fe* pc, uint32_t half, uint32_t rounds) {
  const Fe* row = pc + 3 * rounds + 3 * qq;
  for (uint32_t r = 0; r < rounds; r++) {
    Fe u = add<FrP>(s, pc[3 * r + qq]);
    if (qq == 0 || r < half || r >= rounds - half) u = posh_sbox<FrPn>(u);
    const Fe b0 = quad_bcast<0>(u), b1 = quad_bcast<1>(u), b2 = quad_bcast<2>(u);
    s = posh_mul3(row[0], b0, row[1], b1, row[2], b2);
  }
}
// posh_sponge on a quad; lane 1 writes the result
__device__ __forceinline__ void posh_sponge_quad(const uint32_t* in, uint32_t arity, uint32_t* out, uint32_t q,
                                                 const Fe* pc, uint32_t half, uint32_t rounds) {
  const uint32_t qq = q < 3 ? q : 2;
  Fe s = fe_zero();
  for (uint32_t c = 0; c < arity; c += 2) {
    if (qq == 1) s = add<FrP>(s, fr_in(in + 8 * c));
    if (qq == 2 && c + 1 < arity) s = add<FrP>(s, fr_in(in + 8 * c + 8));
    posh_permute_quad(s, qq, pc, half, rounds);
  }
  if (q == 1) fr_out(out, s);
}
// nt_rehash on a quad
__device__ __forceinline__ void nt_rehash_quad(uint32_t* tree, const uint32_t* empty, const NtGeom& g, uint32_t l,
                                               uint64_t p, uint64_t next, uint32_t q, const Fe* pc, uint32_t half,
                                               uint32_t rounds) {
  const uint32_t qq = q < 3 ? q : 2;
  Fe s = fe_zero();
  if (qq == 1) s = fr_in(tree + (g.off[l - 1] + 2 * p) * 8);
  if (qq == 2) s = fr_in(nt_node(tree, empty, g, l - 1, 2 * p + 1, next));
  posh_permute_quad(s, qq, pc, half, rounds);
  if (q == 1) fr_out(tree + (g.off[l] + p) * 8, s);
}
// nt_root_after on a quad: the carried node is broadcast from lane 1 after every level
__device__ __forceinline__ void nt_root_after_quad(const uint32_t* tree, const uint32_t* empty, const NtGeom& g,
                                                   uint64_t k, uint32_t* out, uint32_t q, const Fe* pc,
                                                   uint32_t half, uint32_t rounds) {
  const uint32_t qq = q < 3 ? q : 2;
  Fe cur = fr_in(tree + (g.off[0] + k) * 8);
  uint64_t idx = k;
  for (uint32_t l = 0; l < g.depth; l++, idx >>= 1) {
    Fe s = fe_zero();
    if (idx & 1) {
      if (qq == 1) s = fr_in(tree + (g.off[l] + idx - 1) * 8);
      if (qq == 2) s = cur;
    } else {
      if (qq == 1) s = cur;
      if (qq == 2) s = fr_in(empty + 8 * l);
    }
    posh_permute_quad(s, qq, pc, half, rounds);
    cur = quad_bcast<1>(s);
  }
  if (q == 1) fr_out(out, cur);
}

// ----------------------------------------------------------------- kernels
// QUAD = false: one lane per hash; true: a quad per hash (thread t serves
// item t / 4, so a quad is wholly active or wholly not)

// out[i] = sponge(in[i * arity .. i * arity + arity))
template <bool QUAD>
__global__ void __launch_bounds__(NTB) k_posh_hash_many(const Fe* __restrict__ pc, uint32_t nconst, uint32_t half,
                                                        uint32_t rounds, const uint32_t* __restrict__ in,
                                                        uint32_t* __restrict__ out, size_t n, uint32_t arity) {
  __shared__ Fe pc_s[POSH_MAX_NCONST];
  fe_table_lds(pc_s, pc, nconst);
  const size_t t = blockIdx.x * (size_t)NTB + threadIdx.x, i = QUAD ? t >> 2 : t;
  if (i >= n) return;
  if (QUAD) posh_sponge_quad(in + i * arity * 8, arity, out + i * 8, threadIdx.x & 3, pc_s, half, rounds);
  else posh_sponge(in + i * arity * 8, arity, out + i * 8, pc_s, half, rounds);
}

// leaves [first, first + n) <- the raw values mod r
__global__ void __launch_bounds__(NTB) k_nt_leaves(const uint32_t* __restrict__ raw, uint32_t* __restrict__ level0,
                                                   uint64_t first, uint64_t n) {
  const uint64_t i = blockIdx.x * (uint64_t)NTB + threadIdx.x;
  if (i >= n) return;
  fr_canon(raw + i * 8, level0 + (first + i) * 8);
}

// one wide level: the nodes [lo, lo + cnt) of level l
template <bool QUAD>
__global__ void __launch_bounds__(NTB) k_nt_level(uint32_t* tree, const uint32_t* __restrict__ empty,
                                                  const NtGeom* __restrict__ geom, uint32_t l, uint64_t lo,
                                                  uint64_t cnt, uint64_t next, const Fe* __restrict__ pc,
                                                  uint32_t nconst, uint32_t half, uint32_t rounds) {
  __shared__ Fe pc_s[POSH_MAX_NCONST];
  fe_table_lds(pc_s, pc, nconst);
  const uint64_t t = blockIdx.x * (uint64_t)NTB + threadIdx.x, i = QUAD ? t >> 2 : t;
  if (i >= cnt) return;
  if (QUAD) nt_rehash_quad(tree, empty, *geom, l, lo + i, next, threadIdx.x & 3, pc_s, half, rounds);
  else nt_rehash(tree, empty, *geom, l, lo + i, next, pc_s, half, rounds);
}

// The narrow top, one workgroup: (the leaves, when raw is given,) then the
// touched nodes of the levels l0 .. depth, a barrier between levels (as
// wprog.hip's k_wprog_chain steps through levels).  A level of up to NTB / 4
// nodes runs on quads (QUAD), a wider one (up to NT_TAIL) on lanes.
template <bool QUAD>
__global__ void __launch_bounds__(NTB) k_nt_tail(uint32_t* tree, const uint32_t* __restrict__ empty,
                                                 const NtGeom* __restrict__ geom, uint32_t l0, uint64_t first,
                                                 uint64_t n, uint64_t next, const uint32_t* __restrict__ raw,
                                                 const Fe* __restrict__ pc, uint32_t nconst, uint32_t half,
                                                 uint32_t rounds) {
  __shared__ Fe pc_s[POSH_MAX_NCONST];
  fe_table_lds(pc_s, pc, nconst);
  const uint32_t depth = geom->depth;
  if (raw) {
    for (uint64_t t = threadIdx.x; t < n; t += NTB) fr_canon(raw + t * 8, tree + (geom->off[0] + first + t) * 8);
    __syncthreads();
  }
  for (uint32_t l = l0; l <= depth; l++) {
    uint64_t lo, cnt;
    nt_touched(first, n, l, &lo, &cnt);
    if (QUAD && cnt <= NTB / 4) {
      if ((threadIdx.x >> 2) < cnt)
        nt_rehash_quad(tree, empty, *geom, l, lo + (threadIdx.x >> 2), next, threadIdx.x & 3, pc_s, half, rounds);
    } else {
      for (uint64_t t = threadIdx.x; t < cnt; t += NTB) nt_rehash(tree, empty, *geom, l, lo + t, next, pc_s, half, rounds);
    }
    __syncthreads();
  }
}

// roots[k] = the root after leaf first + k alone was added to the leaves
// before it, over the finished tree
template <bool QUAD>
__global__ void __launch_bounds__(NTB) k_nt_roots(const uint32_t* __restrict__ tree,
                                                  const uint32_t* __restrict__ empty,
                                                  const NtGeom* __restrict__ geom, uint64_t first, uint64_t n,
                                                  uint32_t* __restrict__ roots, const Fe* __restrict__ pc,
                                                  uint32_t nconst, uint32_t half, uint32_t rounds) {
  __shared__ Fe pc_s[POSH_MAX_NCONST];
  fe_table_lds(pc_s, pc, nconst);
  const uint64_t t = blockIdx.x * (uint64_t)NTB + threadIdx.x, k = QUAD ? t >> 2 : t;
  if (k >= n) return;
  if (QUAD) nt_root_after_quad(tree, empty, *geom, first + k, roots + k * 8, threadIdx.x & 3, pc_s, half, rounds);
  else nt_root_after(tree, empty, *geom, first + k, roots + k * 8, pc_s, half, rounds);
}

// sib[(i * depth + l) * 8 ..] = the sibling of positions[i]'s path at level l
__global__ void __launch_bounds__(NTB) k_nt_paths(const uint32_t* __restrict__ tree,
                                                  const uint32_t* __restrict__ empty,
                                                  const NtGeom* __restrict__ geom, const uint64_t* __restrict__ pos,
                                                  uint64_t n, uint64_t next, uint32_t* __restrict__ sib) {
  const uint32_t depth = geom->depth;
  const uint64_t t = blockIdx.x * (uint64_t)NTB + threadIdx.x;
  if (t >= n * depth) return;
  const uint64_t i = t / depth;
  const uint32_t l = (uint32_t)(t % depth);
  copy8(sib + t * 8, nt_sibling(tree, empty, *geom, l, pos[i], next));
}

static int posh_hash_many(zkmi_ctx* ctx, const zkmi_poseidon* ph, size_t n, uint32_t arity, const uint64_t* in,
                          uint64_t* out) {
  return hasher_hash_many(ctx, "ph_in", "ph_out", "poseidon_hash_many", n, arity, in, out,
                          [&](const uint32_t* d_in, uint32_t* d_out) {
    if (nt_quad(ph, n))
      k_posh_hash_many<true><<<nt_blocks(4 * n), NTB, 0, ctx->stream>>>(ph->d_table, ph->nconst, ph->half, ph->rounds,
                                                                       d_in, d_out, n, arity);
    else
      k_posh_hash_many<false><<<nt_blocks(n), NTB, 0, ctx->stream>>>(ph->d_table, ph->nconst, ph->half, ph->rounds,
                                                                    d_in, d_out, n, arity);
  });
}

static int note_tree_append(zkmi_ctx* ctx, zkmi_note_tree* t, size_t n, const uint64_t* leaves, uint64_t* roots) {
  const zkmi_poseidon* ph = t->ph;
  const uint64_t first = t->next, next = first + n;
  uint32_t* d_raw;
  ZK_TRY(ctx->ws.get("nt_raw", n * 32, (void**)&d_raw));
  ZK_HIP(hipMemcpyAsync(d_raw, leaves, n * 32, hipMemcpyHostToDevice, ctx->stream));
  // the first level the single-workgroup tail takes: the touched ranges only
  // narrow going up
  // (level `depth` is one node, so l0 <= depth)
  uint32_t l0 = 1;
  uint64_t lo, cnt;
  for (; l0 < t->depth; l0++) {
    nt_touched(first, n, l0, &lo, &cnt);
    if (cnt <= NT_TAIL) break;
  }
  const bool tail_leaves = l0 == 1;  // a short append is ONE launch: the tail writes the leaves too
  {
    ScopedKernelTimer tm(ctx, "note_tree_append");
    if (!tail_leaves) k_nt_leaves<<<nt_blocks(n), NTB, 0, ctx->stream>>>(d_raw, t->d_tree, first, n);
    for (uint32_t l = 1; l < l0; l++) {
      nt_touched(first, n, l, &lo, &cnt);
      if (nt_quad(ph, cnt))
        k_nt_level<true><<<nt_blocks(4 * cnt), NTB, 0, ctx->stream>>>(t->d_tree, t->d_empty, t->d_geom, l, lo, cnt, next,
                                                                     ph->d_table, ph->nconst, ph->half, ph->rounds);
      else
        k_nt_level<false><<<nt_blocks(cnt), NTB, 0, ctx->stream>>>(t->d_tree, t->d_empty, t->d_geom, l, lo, cnt, next,
                                                                  ph->d_table, ph->nconst, ph->half, ph->rounds);
    }
    const uint32_t* tail_raw = tail_leaves ? d_raw : nullptr;
    if (ph->quad)
      k_nt_tail<true><<<1, NTB, 0, ctx->stream>>>(t->d_tree, t->d_empty, t->d_geom, l0, first, n, next, tail_raw,
                                                  ph->d_table, ph->nconst, ph->half, ph->rounds);
    else
      k_nt_tail<false><<<1, NTB, 0, ctx->stream>>>(t->d_tree, t->d_empty, t->d_geom, l0, first, n, next, tail_raw,
                                                   ph->d_table, ph->nconst, ph->half, ph->rounds);
  }
  ZK_HIP(hipGetLastError());
  if (roots) {
    uint32_t* d_roots;
    ZK_TRY(ctx->ws.get("nt_roots", n * 32, (void**)&d_roots));
    {
      ScopedKernelTimer tm(ctx, "note_tree_roots");
      if (nt_quad(ph, n))
        k_nt_roots<true><<<nt_blocks(4 * n), NTB, 0, ctx->stream>>>(t->d_tree, t->d_empty, t->d_geom, first, n, d_roots,
                                                                   ph->d_table, ph->nconst, ph->half, ph->rounds);
      else
        k_nt_roots<false><<<nt_blocks(n), NTB, 0, ctx->stream>>>(t->d_tree, t->d_empty, t->d_geom, first, n, d_roots,
                                                                ph->d_table, ph->nconst, ph->half, ph->rounds);
    }
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(roots, d_roots, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  }
  uint64_t root[4];
  ZK_HIP(hipMemcpyAsync(root, t->d_tree + t->geom.off[t->depth] * 8, 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  ZK_TRY(timer_flush(ctx));
  memcpy(t->root, root, 32);
  t->next = next;
  return 0;
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkmi_poseidon_create(zkmi_ctx* ctx, uint32_t full_rounds, uint32_t partial_rounds, const uint64_t* consts,
                         zkmi_poseidon** out) {
  if (!ctx || !consts || !out) {
    set_error("zkmi_poseidon_create: null argument");
    return ZKMI_EINVAL;
  }
  if (!posh_rounds_ok(full_rounds, partial_rounds)) {
    set_error("zkmi_poseidon_create: %u full and %u partial rounds (full even and >= 2, at most %d in all)",
              full_rounds, partial_rounds, POSH_MAX_ROUNDS);
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  zkmi_poseidon* ph = new zkmi_poseidon;
  ph->ctx = ctx;
  ph->half = full_rounds / 2;
  ph->rounds = full_rounds + partial_rounds;
  ph->nconst = posh_nconst(full_rounds, partial_rounds);
  const char* no_quad = getenv("ZKMI_DEBUG_NOTE_TREE_NO_QUAD");
  ph->quad = !(no_quad && no_quad[0] == '1');
  ph->table.resize(ph->nconst);
  posh_table(reinterpret_cast<const uint32_t*>(consts), ph->nconst, ph->table.data());
  const int rc = hasher_upload_table("zkmi_poseidon_create", ctx, ph->table.data(), ph->nconst, &ph->d_table);
  if (rc != 0) {
    delete ph;
    return rc;
  }
  *out = ph;
  return 0;
}
void zkmi_poseidon_destroy(zkmi_poseidon* ph) {
  if (!ph) return;
  ZK_DEVICE_GUARD(ph->ctx);
  delete ph;
}

int zkmi_poseidon_hash_many(zkmi_ctx* ctx, const zkmi_poseidon* ph, size_t n, uint32_t arity, const uint64_t* in,
                            uint64_t* out) {
  if (!zk_owned("zkmi_poseidon_hash_many", "hasher", ctx, ph ? ph->ctx : nullptr)) return ZKMI_EINVAL;
  if (arity < 1 || arity > 4) {
    set_error("zkmi_poseidon_hash_many: arity %u outside 1..4", arity);
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  if (!in || !out) {
    set_error("zkmi_poseidon_hash_many: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return posh_hash_many(ctx, ph, n, arity, in, out);
}

int zkmi_note_tree_create(zkmi_ctx* ctx, const zkmi_poseidon* ph, uint32_t depth, uint64_t capacity,
                          const uint64_t empty_leaf[4], zkmi_note_tree** out) {
  if (!ctx || !ph || ph->ctx != ctx || !empty_leaf || !out) {
    set_error("zkmi_note_tree_create: null argument, or a hasher of another context");
    return ZKMI_EINVAL;
  }
  if (depth < 1 || depth > NT_MAX_DEPTH) {
    set_error("zkmi_note_tree_create: depth %u outside 1..%u", depth, NT_MAX_DEPTH);
    return ZKMI_EINVAL;
  }
  if (capacity == 0 || capacity > (1ull << depth)) {
    set_error("zkmi_note_tree_create: capacity %llu outside 1..2^%u", (unsigned long long)capacity, depth);
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  zkmi_note_tree* t = new zkmi_note_tree;
  t->ctx = ctx;
  t->ph = ph;
  t->depth = depth;
  t->capacity = capacity;
  nt_geom(t->geom, depth, capacity);
  fr_canon(reinterpret_cast<const uint32_t*>(empty_leaf), t->empty);
  for (uint32_t l = 0; l < depth; l++)
    posh_pair(t->empty + 8 * l, t->empty + 8 * l, t->empty + 8 * l + 8, ph->table.data(), ph->half, ph->rounds);
  memcpy(t->root, t->empty + 8 * depth, 32);
  const size_t tree_bytes = t->geom.off[depth + 1] * 32, empty_bytes = (depth + 1) * 32;
  if (hipMalloc((void**)&t->d_tree, tree_bytes) != hipSuccess ||
      hipMalloc((void**)&t->d_empty, empty_bytes) != hipSuccess ||
      hipMalloc((void**)&t->d_geom, sizeof(NtGeom)) != hipSuccess) {
    (void)hipGetLastError();
    delete t;
    set_error("zkmi_note_tree_create: hipMalloc of %zu bytes failed", tree_bytes);
    return ZKMI_ENOMEM;
  }
  hipError_t e = hipMemcpyAsync(t->d_empty, t->empty, empty_bytes, hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(t->d_geom, &t->geom, sizeof(NtGeom), hipMemcpyHostToDevice, ctx->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
  if (e != hipSuccess) {
    delete t;
    set_error("zkmi_note_tree_create: upload failed (%s)", hipGetErrorString(e));
    return ZKMI_EHIP;
  }
  *out = t;
  return 0;
}
void zkmi_note_tree_destroy(zkmi_note_tree* t) {
  if (!t) return;
  ZK_DEVICE_GUARD(t->ctx);
  delete t;
}
int zkmi_note_tree_info(const zkmi_note_tree* t, uint64_t out[3]) {
  if (!t || !out) {
    set_error("zkmi_note_tree_info: null argument");
    return ZKMI_EINVAL;
  }
  out[0] = t->depth;
  out[1] = t->capacity;
  out[2] = t->next;
  return 0;
}

int zkmi_note_tree_append(zkmi_ctx* ctx, zkmi_note_tree* t, size_t n, const uint64_t* leaves, uint64_t* first,
                          uint64_t* roots) {
  if (!zk_owned("zkmi_note_tree_append", "tree", ctx, t ? t->ctx : nullptr)) return ZKMI_EINVAL;
  if (n > t->capacity - t->next) {
    set_error("zkmi_note_tree_append: %zu leaves onto %llu of a capacity of %llu", n, (unsigned long long)t->next,
              (unsigned long long)t->capacity);
    return ZKMI_EINVAL;
  }
  if (first) *first = t->next;
  if (n == 0) return 0;
  if (!leaves) {
    set_error("zkmi_note_tree_append: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  return note_tree_append(ctx, t, n, leaves, roots);
}

int zkmi_note_tree_root(zkmi_ctx* ctx, const zkmi_note_tree* t, uint64_t out[4]) {
  if (!ctx || !t || t->ctx != ctx || !out) {
    set_error("zkmi_note_tree_root: null argument, or a tree of another context");
    return ZKMI_EINVAL;
  }
  memcpy(out, t->root, 32);  // kept on the host by every append
  return 0;
}

int zkmi_note_tree_paths(zkmi_ctx* ctx, const zkmi_note_tree* t, size_t n, const uint64_t* positions,
                         uint64_t* siblings) {
  if (!zk_owned("zkmi_note_tree_paths", "tree", ctx, t ? t->ctx : nullptr)) return ZKMI_EINVAL;
  if (n == 0) return 0;
  if (!positions || !siblings) {
    set_error("zkmi_note_tree_paths: null argument");
    return ZKMI_EINVAL;
  }
  for (size_t i = 0; i < n; i++) {
    if (positions[i] >= t->next) {
      set_error("zkmi_note_tree_paths: position %llu (entry %zu) of a tree of %llu leaves",
                (unsigned long long)positions[i], i, (unsigned long long)t->next);
      return ZKMI_EINVAL;
    }
  }
  ZK_DEVICE_GUARD(ctx);
  uint64_t* d_pos;
  uint32_t* d_sib;
  const size_t words = n * t->depth * 8;
  ZK_TRY(ctx->ws.get("nt_pos", n * 8, (void**)&d_pos));
  ZK_TRY(ctx->ws.get("nt_sib", words * 4, (void**)&d_sib));
  ZK_HIP(hipMemcpyAsync(d_pos, positions, n * 8, hipMemcpyHostToDevice, ctx->stream));
  {
    ScopedKernelTimer tm(ctx, "note_tree_paths");
    k_nt_paths<<<nt_blocks((uint64_t)n * t->depth), NTB, 0, ctx->stream>>>(t->d_tree, t->d_empty, t->d_geom, d_pos, n,
                                                                          t->next, d_sib);
  }
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipMemcpyAsync(siblings, d_sib, words * 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return timer_flush(ctx);
}

int zkmi_note_tree_leaves(zkmi_ctx* ctx, const zkmi_note_tree* t, uint64_t first, size_t n, uint64_t* out) {
  if (!zk_owned("zkmi_note_tree_leaves", "tree", ctx, t ? t->ctx : nullptr)) return ZKMI_EINVAL;
  if (n == 0) return 0;
  if (first >= t->next || n > t->next - first) {
    set_error("zkmi_note_tree_leaves: [%llu, +%zu) of a tree of %llu leaves", (unsigned long long)first, n,
              (unsigned long long)t->next);
    return ZKMI_EINVAL;
  }
  if (!out) {
    set_error("zkmi_note_tree_leaves: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  ZK_HIP(hipMemcpyAsync(out, t->d_tree + first * 8, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  return 0;
}

}  // extern "C"
