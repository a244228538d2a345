// note_scan.hip — the encrypted-note store resident in HBM and the batched
// note scan (zkmi.h "encrypted-note store").  The arithmetic
// is note_crypt.h's (X25519, the BLAKE3 key derivation, ChaCha20-Poly1305, the
// plaintext parse) and mimc_hash.h's / poseidon_hash.h's (the commitment
// check); this file holds the store, the kernels' lane mappings, the launch
// sequence of a scan and the C entry points.  Everything runs on the context
// stream, and every call returns with its results on the host.
#include <string.h>

#include <algorithm>
#include <unordered_set>
#include <vector>

#include "hashers.h"
#include "lane_util.h"
#include "note_crypt.h"

// Headers are arrays of their own (a wave reads 64 consecutive entries of
// each); a ciphertext lies at index x stride, stride = max_ct rounded up to 16
// bytes, so its address needs no load and an append needs no prefix sum.
struct zkmi_note_store {
  zkmi_ctx* ctx = nullptr;
  uint64_t capacity = 0, count = 0, ct_bytes = 0;
  uint32_t max_ct = 0, stride_words = 0;
  uint32_t ctx_key[8];               // blake3 derive_key context key of "zelana-note-v1"
  std::vector<uint32_t> positions;   // host mirror, append order: scanned_to and the examined counts
  std::unordered_set<uint32_t> seen; // positions stored (a position is never stored twice)
  uint32_t *d_pos = nullptr, *d_cm = nullptr, *d_epk = nullptr, *d_nonce = nullptr, *d_len = nullptr, *d_ct = nullptr;
  ~zkmi_note_store() {
    for (uint32_t* p : {d_pos, d_cm, d_epk, d_nonce, d_len, d_ct})
      if (p) (void)hipFree(p);
  }
};

namespace zk {

constexpr int NSC_ECDH = 128;  // lanes a block of the ladder kernel
constexpr int NSC_B = 256;     // lanes a block of the others
constexpr uint64_t NSC_MAX_CAPACITY = 1ull << 26;  // nkeys x notes stays below 2^32
constexpr uint32_t NSC_MAX_KEYS = 64, NSC_MAX_LIMIT = 65536;
constexpr uint32_t NSC_REC_WORDS = 16;  // result, position, value[2], randomness[8], memo_len, pair, 2 spare
static unsigned nsc_blocks(uint64_t n, int b) { return (unsigned)((n + b - 1) / b); }

struct NscKey {
  uint32_t w[8];
};

// One lane per (key, note): blockIdx.y is the key, so every lane of a wave
// walks the ladder with the same scalar bits.  key_out[(k n + i) 8 ..] = the
// note key of the pair; notes below from_position take no part.
__global__ void __launch_bounds__(NSC_ECDH) k_scan_ecdh(const uint32_t* __restrict__ dkeys,
                                                        const uint32_t* __restrict__ epk,
                                                        const uint32_t* __restrict__ pos, uint32_t n, uint32_t from,
                                                        NscKey ctx_key, uint32_t* __restrict__ key_out) {
  const uint32_t i = blockIdx.x * NSC_ECDH + threadIdx.x, k = blockIdx.y;
  if (i >= n || pos[i] < from) return;
  uint32_t sc[8], u[8], shared[8], key[8];
#pragma unroll
  for (int w = 0; w < 8; w++) sc[w] = dkeys[8 * k + w], u[w] = epk[8 * (uint64_t)i + w];
  x25519(shared, sc, u);
  note_key(key, ctx_key.w, shared, u);
  copy8(key_out + 8 * ((uint64_t)k * n + i), key);
}

// flag[k n + i] = the tag of note i matches under the pair's key;
// block_cnt[k blocks + b] = the flags of the block
__global__ void __launch_bounds__(NSC_B) k_scan_tag(const uint32_t* __restrict__ keys,
                                                    const uint32_t* __restrict__ nonce,
                                                    const uint32_t* __restrict__ len, const uint32_t* __restrict__ ct,
                                                    uint32_t stride_words, const uint32_t* __restrict__ pos, uint32_t n,
                                                    uint32_t from, uint8_t* __restrict__ flag,
                                                    uint32_t* __restrict__ block_cnt) {
  const uint32_t i = blockIdx.x * NSC_B + threadIdx.x, k = blockIdx.y;
  bool ok = false;
  if (i < n && pos[i] >= from) {
    uint32_t key[8], nc[3];
    copy8(key, keys + 8 * ((uint64_t)k * n + i));
#pragma unroll
    for (int w = 0; w < 3; w++) nc[w] = nonce[4 * (uint64_t)i + w];
    ok = aead_tag_ok(key, nc, ct + (uint64_t)i * stride_words, len[i]);
  }
  if (i < n) flag[(uint64_t)k * n + i] = ok;
  const int c = __syncthreads_count(ok);
  if (threadIdx.x == 0) block_cnt[k * gridDim.x + blockIdx.x] = (uint32_t)c;
}

// list[rank] = k n + i for every flagged pair, in key-major, append order
// (the blocks and lanes of k_scan_tag, block_cnt turned into offsets by
// k_block_offsets)
__global__ void __launch_bounds__(NSC_B) k_scan_compact(const uint8_t* __restrict__ flag, uint32_t n,
                                                        const uint32_t* __restrict__ block_off,
                                                        uint32_t* __restrict__ list) {
  __shared__ uint32_t wave_s[NSC_B / 64];
  const uint32_t i = blockIdx.x * NSC_B + threadIdx.x, k = blockIdx.y;
  const bool f = i < n && flag[(uint64_t)k * n + i];
  const uint32_t rank = block_rank<NSC_B>(f, block_off + (k * gridDim.x + blockIdx.x), wave_s);
  if (!f) return;
  list[rank] = k * n + i;
}

// One lane per flagged pair: the first plaintext block, the parse, the
// commitment of the scheme and its bytewise compare.  SCHEME 0 none, 1 MiMC
// hash_3(owner, value, randomness), 2 the Poseidon sponge over (value,
// randomness, owner).  rec: NSC_REC_WORDS words a pair.
template <int SCHEME>
__global__ void __launch_bounds__(NSC_B) k_scan_open(const uint32_t* __restrict__ list, uint32_t nflag, uint32_t n,
                                                     const uint32_t* __restrict__ keys,
                                                     const uint32_t* __restrict__ nonce,
                                                     const uint32_t* __restrict__ len, const uint32_t* __restrict__ ct,
                                                     uint32_t stride_words, const uint32_t* __restrict__ pos,
                                                     const uint32_t* __restrict__ cm,
                                                     const uint32_t* __restrict__ owner, const Fe* __restrict__ table,
                                                     uint32_t half, uint32_t rounds, uint32_t nconst,
                                                     uint32_t* __restrict__ rec) {
  __shared__ Fe tab_s[SCHEME == 1 ? MIMC_NTABLE : SCHEME == 2 ? POSH_MAX_NCONST : 1];
  if (SCHEME != 0) fe_table_lds(tab_s, table, SCHEME == 1 ? (uint32_t)MIMC_NTABLE : nconst);
  const uint32_t j = blockIdx.x * NSC_B + threadIdx.x;
  if (j >= nflag) return;
  const uint32_t pair = list[j], k = pair / n, i = pair % n;
  uint32_t key[8], nc[3], pt[16];
  copy8(key, keys + 8 * (uint64_t)pair);
#pragma unroll
  for (int w = 0; w < 3; w++) nc[w] = nonce[4 * (uint64_t)i + w];
  const uint32_t body = len[i] - AEAD_TAG;  // flagged: len >= 16
  aead_plain_block(pt, key, nc, ct + (uint64_t)i * stride_words, body, 0);
  NoteHead h;
  uint32_t result = note_parse(pt, body, h) ? SCAN_HIT : SCAN_MALFORMED;
  if (SCHEME != 0 && result == SCAN_HIT) {
    uint32_t in[24], out[8];
#pragma unroll
    for (int w = 0; w < 8; w++) {
      const uint32_t o = owner[8 * k + w], v = w < 2 ? h.value[w] : 0, r = h.randomness[w];
      if (SCHEME == 1)
        in[w] = o, in[8 + w] = v, in[16 + w] = r;
      else
        in[w] = v, in[8 + w] = r, in[16 + w] = o;
    }
    if (SCHEME == 1)
      mimc_hash(in, 3, out, tab_s);
    else
      posh_sponge(in, 3, out, tab_s, half, rounds);
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < 8; w++) d |= out[w] ^ cm[8 * (uint64_t)i + w];
    if (d) result = SCAN_WRONG_COMMITMENT;
  }
  uint32_t* r = rec + (uint64_t)j * NSC_REC_WORDS;
  r[0] = result, r[1] = pos[i], r[2] = h.value[0], r[3] = h.value[1];
  copy8(r + 4, h.randomness);
  r[12] = h.memo_len, r[13] = pair, r[14] = 0, r[15] = 0;
}

// One lane per returned hit that has a memo: sel[2 j] = its pair, sel[2 j + 1]
// = its memo length; the memo's words go to memo_out + j memo_words.
__global__ void __launch_bounds__(NSC_B) k_scan_memo(const uint32_t* __restrict__ sel, uint32_t nsel, uint32_t n,
                                                     const uint32_t* __restrict__ keys,
                                                     const uint32_t* __restrict__ nonce,
                                                     const uint32_t* __restrict__ len, const uint32_t* __restrict__ ct,
                                                     uint32_t stride_words, uint32_t memo_words,
                                                     uint32_t* __restrict__ memo_out) {
  const uint32_t j = blockIdx.x * NSC_B + threadIdx.x;
  if (j >= nsel) return;
  const uint32_t pair = sel[2 * j], memo_len = sel[2 * j + 1], i = pair % n;
  if (note_memo_words(memo_len) > memo_words) return;  // cannot happen: memo_len <= body - 42 <= max_ct - 58
  uint32_t key[8], nc[3];
  copy8(key, keys + 8 * (uint64_t)pair);
#pragma unroll
  for (int w = 0; w < 3; w++) nc[w] = nonce[4 * (uint64_t)i + w];
  note_memo(memo_out + (uint64_t)j * memo_words, key, nc, ct + (uint64_t)i * stride_words, len[i] - AEAD_TAG,
            memo_len);
}

struct ScanOut {
  uint32_t *counts, *scanned_to, *stats, *positions;
  uint64_t* values;
  uint8_t *randomness, *commitments;
  uint32_t* memo_lens;
  uint8_t* memos;
};

// arguments already checked; nkeys >= 1
static int note_scan(zkmi_ctx* ctx, const zkmi_note_store* s, const Fe* table, uint32_t half, uint32_t rounds,
                     uint32_t nconst, uint32_t scheme, uint32_t nkeys, const uint8_t* dkeys, const uint8_t* owner_pks,
                     uint32_t from, uint32_t limit, const ScanOut& o) {
  const uint32_t n = (uint32_t)s->count;
  // what the host knows without the device: the notes examined and the highest position
  uint32_t examined = 0, top = from;
  for (uint32_t p : s->positions)
    if (p >= from) examined++, top = std::max(top, p);
  for (uint32_t k = 0; k < nkeys; k++) {
    o.counts[k] = 0, o.scanned_to[k] = top;
    o.stats[4 * k + SCAN_NOT_MINE] = examined;
    o.stats[4 * k + SCAN_MALFORMED] = o.stats[4 * k + SCAN_WRONG_COMMITMENT] = o.stats[4 * k + SCAN_HIT] = 0;
  }
  if (examined == 0) return 0;
  const uint32_t nblk = nsc_blocks(n, NSC_B), nblocks = nblk * nkeys;
  const uint64_t pairs = (uint64_t)nkeys * n;
  uint32_t *d_dkeys, *d_owner, *d_keys, *d_block, *d_total, *d_list;
  uint8_t* d_flag;
  ZK_TRY(ctx->ws.get("nsc_dkeys", (size_t)nkeys * 32, (void**)&d_dkeys));
  ZK_TRY(ctx->ws.get("nsc_owner", (size_t)nkeys * 32, (void**)&d_owner));
  ZK_TRY(ctx->ws.get("nsc_keys", pairs * 32, (void**)&d_keys));
  ZK_TRY(ctx->ws.get("nsc_flag", pairs, (void**)&d_flag));
  ZK_TRY(ctx->ws.get("nsc_block", (size_t)nblocks * 4, (void**)&d_block));
  ZK_TRY(ctx->ws.get("nsc_total", 4, (void**)&d_total));
  ZK_TRY(ctx->ws.get("nsc_list", pairs * 4, (void**)&d_list));
  ZK_HIP(hipMemcpyAsync(d_dkeys, dkeys, (size_t)nkeys * 32, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(d_owner, owner_pks, (size_t)nkeys * 32, hipMemcpyHostToDevice, ctx->stream));
  NscKey ck;
  memcpy(ck.w, s->ctx_key, 32);
  {
    ScopedKernelTimer tm(ctx, "note_scan_ecdh");
    k_scan_ecdh<<<dim3(nsc_blocks(n, NSC_ECDH), nkeys), NSC_ECDH, 0, ctx->stream>>>(d_dkeys, s->d_epk, s->d_pos, n,
                                                                                    from, ck, d_keys);
  }
  ZK_HIP(hipGetLastError());
  {
    ScopedKernelTimer tm(ctx, "note_scan_tag");
    k_scan_tag<<<dim3(nblk, nkeys), NSC_B, 0, ctx->stream>>>(d_keys, s->d_nonce, s->d_len, s->d_ct, s->stride_words,
                                                             s->d_pos, n, from, d_flag, d_block);
  }
  ZK_HIP(hipGetLastError());
  {
    ScopedKernelTimer tm(ctx, "note_scan_compact");
    k_block_offsets<NSC_B><<<1, NSC_B, 0, ctx->stream>>>(d_block, nblocks, d_total);
    k_scan_compact<<<dim3(nblk, nkeys), NSC_B, 0, ctx->stream>>>(d_flag, n, d_block, d_list);
  }
  ZK_HIP(hipGetLastError());
  uint32_t nflag = 0;
  ZK_HIP(hipMemcpyAsync(&nflag, d_total, 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  if (nflag == 0) return timer_flush(ctx);
  uint32_t* d_rec;
  ZK_TRY(ctx->ws.get("nsc_rec", (size_t)nflag * NSC_REC_WORDS * 4, (void**)&d_rec));
  {
    ScopedKernelTimer tm(ctx, "note_scan_open");
    const dim3 g(nsc_blocks(nflag, NSC_B));
#define NSC_OPEN(S)                                                                                              \
  k_scan_open<S><<<g, NSC_B, 0, ctx->stream>>>(d_list, nflag, n, d_keys, s->d_nonce, s->d_len, s->d_ct,          \
                                               s->stride_words, s->d_pos, s->d_cm, d_owner, table, half, rounds, \
                                               nconst, d_rec)
    if (scheme == 0)
      NSC_OPEN(0);
    else if (scheme == 1)
      NSC_OPEN(1);
    else
      NSC_OPEN(2);
#undef NSC_OPEN
  }
  ZK_HIP(hipGetLastError());
  std::vector<uint32_t> rec((size_t)nflag * NSC_REC_WORDS);
  ZK_HIP(hipMemcpyAsync(rec.data(), d_rec, rec.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  // The hits of a key in ascending position order, cut at limit: an index sort
  // over the flagged pairs (the notes addressed to the scanning keys, few).
  // Records are key-major, so a key's are one run.
  std::vector<uint32_t> sel;  // pair, memo_len of the returned hits that have a memo
  std::vector<uint64_t> sel_slot;
  size_t at = 0;
  for (uint32_t k = 0; k < nkeys; k++) {
    std::vector<uint32_t> hits;
    for (; at < nflag && rec[at * NSC_REC_WORDS + 13] / n == k; at++) {
      const uint32_t result = rec[at * NSC_REC_WORDS];
      o.stats[4 * k + result]++;
      o.stats[4 * k + SCAN_NOT_MINE]--;
      if (result == SCAN_HIT) hits.push_back((uint32_t)at);
    }
    std::sort(hits.begin(), hits.end(),
              [&](size_t a, size_t b) { return rec[a * NSC_REC_WORDS + 1] < rec[b * NSC_REC_WORDS + 1]; });
    if (hits.size() > limit) {
      hits.resize(limit);
      o.scanned_to[k] = rec[(size_t)hits.back() * NSC_REC_WORDS + 1];
    }
    o.counts[k] = (uint32_t)hits.size();
    for (size_t r = 0; r < hits.size(); r++) {
      const uint32_t* h = &rec[(size_t)hits[r] * NSC_REC_WORDS];
      const uint64_t slot = (uint64_t)k * limit + r;
      o.positions[slot] = h[1];
      o.values[slot] = (uint64_t)h[2] | ((uint64_t)h[3] << 32);
      memcpy(o.randomness + 32 * slot, h + 4, 32);
      o.memo_lens[slot] = h[12];
      // the stored commitment: one small copy per returned hit (hits are few)
      ZK_HIP(hipMemcpyAsync(o.commitments + 32 * slot, s->d_cm + 8 * (uint64_t)(h[13] % n), 32, hipMemcpyDeviceToHost,
                            ctx->stream));
      if (o.memos && h[12]) sel.push_back(h[13]), sel.push_back(h[12]), sel_slot.push_back(slot);
    }
  }
  const uint32_t memo_cap = s->max_ct - NOTE_MIN_CT, memo_words = (memo_cap + 3) / 4;
  std::vector<uint32_t> memo_host;
  if (!sel_slot.empty()) {
    const uint32_t nsel = (uint32_t)sel_slot.size();
    uint32_t *d_sel, *d_memo;
    ZK_TRY(ctx->ws.get("nsc_sel", sel.size() * 4, (void**)&d_sel));
    ZK_TRY(ctx->ws.get("nsc_memo", (size_t)nsel * memo_words * 4, (void**)&d_memo));
    ZK_HIP(hipMemcpyAsync(d_sel, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    {
      ScopedKernelTimer tm(ctx, "note_scan_memo");
      k_scan_memo<<<nsc_blocks(nsel, NSC_B), NSC_B, 0, ctx->stream>>>(d_sel, nsel, n, d_keys, s->d_nonce, s->d_len,
                                                                      s->d_ct, s->stride_words, memo_words, d_memo);
    }
    ZK_HIP(hipGetLastError());
    memo_host.resize((size_t)nsel * memo_words);
    ZK_HIP(hipMemcpyAsync(memo_host.data(), d_memo, memo_host.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  }
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  for (size_t j = 0; j < sel_slot.size(); j++)
    memcpy(o.memos + sel_slot[j] * memo_cap, &memo_host[j * memo_words], sel[2 * j + 1]);
  return timer_flush(ctx);
}

}  // namespace zk

using namespace zk;

extern "C" {

int zkmi_note_store_create(zkmi_ctx* ctx, uint64_t capacity, uint32_t max_ct, zkmi_note_store** out) {
  if (!ctx || !out) {
    set_error("zkmi_note_store_create: null argument");
    return ZKMI_EINVAL;
  }
  if (capacity == 0 || capacity > NSC_MAX_CAPACITY || max_ct < NOTE_MIN_CT || max_ct > NOTE_MIN_CT + 65535) {
    set_error("zkmi_note_store_create: capacity %llu outside 1..2^26 or max_ct %u outside 58..65593",
              (unsigned long long)capacity, max_ct);
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  zkmi_note_store* s = new zkmi_note_store;
  s->ctx = ctx;
  s->capacity = capacity;
  s->max_ct = max_ct;
  s->stride_words = (max_ct + 15) / 16 * 4;
  {
    static const char context[] = "zelana-note-v1";
    const uint32_t iv[8] = {0x6A09E667u, 0xBB67AE85u, 0x3C6EF372u, 0xA54FF53Au,
                            0x510E527Fu, 0x9B05688Cu, 0x1F83D9ABu, 0x5BE0CD19u};
    uint32_t block[16] = {0};
    memcpy(block, context, sizeof context - 1);
    blake3_compress8(s->ctx_key, iv, block, 0, sizeof context - 1,
                     B3_CHUNK_START | B3_CHUNK_END | B3_ROOT | B3_DERIVE_KEY_CONTEXT);
  }
  if (hipMalloc((void**)&s->d_pos, capacity * 4) != hipSuccess ||
      hipMalloc((void**)&s->d_cm, capacity * 32) != hipSuccess ||
      hipMalloc((void**)&s->d_epk, capacity * 32) != hipSuccess ||
      hipMalloc((void**)&s->d_nonce, capacity * 16) != hipSuccess ||
      hipMalloc((void**)&s->d_len, capacity * 4) != hipSuccess ||
      hipMalloc((void**)&s->d_ct, capacity * s->stride_words * 4) != hipSuccess) {
    (void)hipGetLastError();
    delete s;
    set_error("zkmi_note_store_create: hipMalloc of a store of %llu notes of %u bytes failed",
              (unsigned long long)capacity, max_ct);
    return ZKMI_ENOMEM;
  }
  *out = s;
  return 0;
}
void zkmi_note_store_destroy(zkmi_note_store* s) {
  if (!s) return;
  ZK_DEVICE_GUARD(s->ctx);
  delete s;
}
int zkmi_note_store_info(const zkmi_note_store* s, uint64_t out[4]) {
  if (!s || !out) {
    set_error("zkmi_note_store_info: null argument");
    return ZKMI_EINVAL;
  }
  out[0] = s->capacity, out[1] = s->max_ct, out[2] = s->count, out[3] = s->ct_bytes;
  return 0;
}

int zkmi_note_store_append(zkmi_ctx* ctx, zkmi_note_store* s, size_t n, const uint32_t* positions,
                           const uint8_t* commitments, const uint8_t* ephemeral_pks, const uint8_t* nonces,
                           const uint32_t* ct_lens, const uint8_t* cts) {
  if (!zk_owned("zkmi_note_store_append", "store", ctx, s ? s->ctx : nullptr)) return ZKMI_EINVAL;
  if (n == 0) return 0;
  if (!positions || !commitments || !ephemeral_pks || !nonces || !ct_lens) {
    set_error("zkmi_note_store_append: null argument");
    return ZKMI_EINVAL;
  }
  if (n > s->capacity - s->count) {
    set_error("zkmi_note_store_append: %zu notes beside the %llu stored, past the capacity %llu", n,
              (unsigned long long)s->count, (unsigned long long)s->capacity);
    return ZKMI_ENOMEM;
  }
  uint64_t total = 0;
  std::unordered_set<uint32_t> fresh;
  for (size_t i = 0; i < n; i++) {
    if (ct_lens[i] > s->max_ct) {
      set_error("zkmi_note_store_append: note %zu has a ciphertext of %u bytes, the store takes %u", i, ct_lens[i],
                s->max_ct);
      return ZKMI_EINVAL;
    }
    if (s->seen.count(positions[i]) || !fresh.insert(positions[i]).second) {
      set_error("zkmi_note_store_append: note %zu repeats position %u", i, positions[i]);
      return ZKMI_EINVAL;
    }
    total += ct_lens[i];
  }
  if (total && !cts) {
    set_error("zkmi_note_store_append: null ciphertexts");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  // nonces at 16 bytes and ciphertexts at their stride, the padding zero
  const size_t stride = (size_t)s->stride_words * 4;
  std::vector<uint8_t> nc(n * 16, 0), ct(n * stride, 0);
  uint64_t at = 0;
  for (size_t i = 0; i < n; i++) {
    memcpy(&nc[16 * i], nonces + 12 * i, 12);
    if (ct_lens[i]) memcpy(&ct[i * stride], cts + at, ct_lens[i]);
    at += ct_lens[i];
  }
  const uint64_t c = s->count;
  ZK_HIP(hipMemcpyAsync(s->d_pos + c, positions, n * 4, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(s->d_cm + 8 * c, commitments, n * 32, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(s->d_epk + 8 * c, ephemeral_pks, n * 32, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(s->d_nonce + 4 * c, nc.data(), n * 16, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(s->d_len + c, ct_lens, n * 4, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipMemcpyAsync(s->d_ct + c * s->stride_words, ct.data(), n * stride, hipMemcpyHostToDevice, ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  // the count moves only after every copy has landed: a failed call leaves the notes before it as they were
  s->positions.insert(s->positions.end(), positions, positions + n);
  s->seen.insert(fresh.begin(), fresh.end());
  s->count += n;
  s->ct_bytes += total;
  return 0;
}

int zkmi_note_store_get(zkmi_ctx* ctx, const zkmi_note_store* s, uint64_t first, size_t n, uint32_t* positions,
                        uint8_t* commitments, uint8_t* ephemeral_pks, uint8_t* nonces, uint32_t* ct_lens,
                        uint8_t* cts) {
  if (!zk_owned("zkmi_note_store_get", "store", ctx, s ? s->ctx : nullptr)) return ZKMI_EINVAL;
  if (first > s->count || n > s->count - first) {
    set_error("zkmi_note_store_get: [%llu, +%zu) of a store of %llu notes", (unsigned long long)first, n,
              (unsigned long long)s->count);
    return ZKMI_EINVAL;
  }
  if (n == 0) return 0;
  ZK_DEVICE_GUARD(ctx);
  const size_t stride = (size_t)s->stride_words * 4;
  std::vector<uint8_t> nc(nonces ? n * 16 : 0), ct(cts ? n * stride : 0);
  std::vector<uint32_t> lens(n);
  if (positions) ZK_HIP(hipMemcpyAsync(positions, s->d_pos + first, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (commitments)
    ZK_HIP(hipMemcpyAsync(commitments, s->d_cm + 8 * first, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (ephemeral_pks)
    ZK_HIP(hipMemcpyAsync(ephemeral_pks, s->d_epk + 8 * first, n * 32, hipMemcpyDeviceToHost, ctx->stream));
  if (nonces) ZK_HIP(hipMemcpyAsync(nc.data(), s->d_nonce + 4 * first, n * 16, hipMemcpyDeviceToHost, ctx->stream));
  ZK_HIP(hipMemcpyAsync(lens.data(), s->d_len + first, n * 4, hipMemcpyDeviceToHost, ctx->stream));
  if (cts)
    ZK_HIP(hipMemcpyAsync(ct.data(), s->d_ct + first * s->stride_words, n * stride, hipMemcpyDeviceToHost,
                          ctx->stream));
  ZK_HIP(hipStreamSynchronize(ctx->stream));
  uint64_t at = 0;
  for (size_t i = 0; i < n; i++) {
    if (nonces) memcpy(nonces + 12 * i, &nc[16 * i], 12);
    if (ct_lens) ct_lens[i] = lens[i];
    if (cts && lens[i]) memcpy(cts + at, &ct[i * stride], lens[i]);
    at += lens[i];
  }
  return 0;
}

int zkmi_note_scan(zkmi_ctx* ctx, const zkmi_note_store* s, const zkmi_mimc* mh, const zkmi_poseidon* ph,
                   uint32_t scheme, size_t nkeys, const uint8_t* decryption_keys, const uint8_t* owner_pks,
                   uint32_t from_position, uint32_t limit, uint32_t* counts, uint32_t* scanned_to, uint32_t* stats,
                   uint32_t* positions, uint64_t* values, uint8_t* randomness, uint8_t* commitments,
                   uint32_t* memo_lens, uint8_t* memos) {
  if (!zk_owned("zkmi_note_scan", "store", ctx, s ? s->ctx : nullptr)) return ZKMI_EINVAL;
  if (scheme > 2 || nkeys > NSC_MAX_KEYS || limit < 1 || limit > NSC_MAX_LIMIT) {
    set_error("zkmi_note_scan: scheme %u (0..2), %zu keys (at most 64) or limit %u (1..65536)", scheme, nkeys, limit);
    return ZKMI_EINVAL;
  }
  const Fe* table = nullptr;
  uint32_t half = 0, rounds = 0, nconst = 0;
  const zkmi_ctx* hctx = ctx;
  if (scheme == 1 && mh) table = mh->d_table, hctx = mh->ctx;
  if (scheme == 2 && ph) table = ph->d_table, half = ph->half, rounds = ph->rounds, nconst = ph->nconst, hctx = ph->ctx;
  if ((scheme != 0 && !table) || hctx != ctx) {
    set_error("zkmi_note_scan: scheme %u needs its hasher, made on this context", scheme);
    return ZKMI_EINVAL;
  }
  if (nkeys == 0) return 0;
  if (!decryption_keys || !owner_pks || !counts || !scanned_to || !stats || !positions || !values || !randomness ||
      !commitments || !memo_lens) {
    set_error("zkmi_note_scan: null argument");
    return ZKMI_EINVAL;
  }
  ZK_DEVICE_GUARD(ctx);
  const ScanOut o = {counts, scanned_to, stats, positions, values, randomness, commitments, memo_lens, memos};
  return note_scan(ctx, s, table, half, rounds, nconst, scheme, (uint32_t)nkeys, decryption_keys, owner_pks,
                   from_position, limit, o);
}

}  // extern "C"
