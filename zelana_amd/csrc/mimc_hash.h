// mimc_hash.h — the MiMC sponge over Fr as a primitive, one lane per hash, and
// the arithmetic of the account tree over it: the ordering rule of a batch of
// ordered leaf writes and the node store.  Host+device like
// poseidon_hash.h: the kernels of account_tree.hip and the stand-alone host
// check (tests/host/account_tree_check.cpp) compile the very same permutation,
// sponge, ordering functions and probes.
//
// The permutation is the reference's (account_tree.rs:47-76, the circuit's
// poseidon.nr, zbatch.mimc_permute, wprog.hip's WP_PERM): 91 rounds of
// x <- (x + c_i)^7, c_i = (i + 1)^3 + (i + 1), key 0.  hash_k(x_1 .. x_k) is
// the sponge over [k, x_1, .., x_k]: state <- P(state + input) from state 0,
// so its first permutation, P(k), is a constant; the table holds the four of
// them and hash_k costs k permutations.
//
// Field elements cross this header as 8 little-endian u32 words.  Inputs may
// be ANY 256-bit value: they are taken mod r by the conversion to Montgomery
// form.  Outputs are canonical (< r).
#pragma once
#include "ff.h"

namespace zk {

constexpr int MIMC_ROUNDS = 91;
// the table: c_0 .. c_90, then P(1) .. P(4); Montgomery form
constexpr int MIMC_NTABLE = MIMC_ROUNDS + 4;

// One round: t = x + c, t^7 = t^4 t^3.  t^3 = t^2 t and t^4 = t^2 t^2 do not
// depend on each other: mul_x2 interleaves their two accumulator chains in one
// instruction stream, so a round is three dependent products deep, not four.
// The square and the last product are compiler-scheduled (ff.h's FrPn): the
// hashes of a level step are few, a lone wave on a SIMD sees the latency of
// every mad of the one-chain form
ZK_HD Fe mimc_round(const Fe& x, const Fe& c) {
  const Fe t = add<FrP>(x, c);
  const Fe t2 = sqr<FrPn>(t);
  Fe t3, t4;
  mul_x2<FrP>(t2, t, t2, t2, t3, t4);
  return mul<FrPn>(t4, t3);
}
// P(x), x in Montgomery form, < 2r
ZK_HD Fe mimc_permute(Fe x, const Fe* tab) {
#pragma unroll 1
  for (int i = 0; i < MIMC_ROUNDS; i++) x = mimc_round(x, tab[i]);
  return x;
}
// the table, made by this header alone
ZK_HD void mimc_table(Fe* tab) {
  for (uint32_t i = 0; i < (uint32_t)MIMC_ROUNDS; i++) {
    const uint64_t c = (uint64_t)(i + 1) * (i + 1) * (i + 1) + (i + 1);
    uint32_t w[8] = {(uint32_t)c, (uint32_t)(c >> 32), 0, 0, 0, 0, 0, 0};
    tab[i] = reduce<FrP>(fr_in(w));
  }
  for (uint32_t k = 1; k <= 4; k++) {
    uint32_t w[8] = {k, 0, 0, 0, 0, 0, 0, 0};
    tab[MIMC_ROUNDS + k - 1] = reduce<FrP>(mimc_permute(fr_in(w), tab));
  }
}
// hash_arity(in[0 .. arity)), arity 1..4; in: arity x 8 words
ZK_HD void mimc_hash(const uint32_t* in, uint32_t arity, uint32_t* out, const Fe* tab) {
  Fe s = tab[MIMC_ROUNDS + arity - 1];
  for (uint32_t i = 0; i < arity; i++) s = mimc_permute(add<FrP>(s, fr_in(in + 8 * i)), tab);
  fr_out(out, s);
}
// hash_2(left, right): the tree's node hash
ZK_HD void mimc_pair(const uint32_t* left, const uint32_t* right, uint32_t* out, const Fe* tab) {
  Fe s = mimc_permute(add<FrP>(tab[MIMC_ROUNDS + 1], fr_in(left)), tab);
  s = mimc_permute(add<FrP>(s, fr_in(right)), tab);
  fr_out(out, s);
}

// ------------------------------------------------------- ordered leaf writes
// A tree of `depth` levels (1..32) over mimc_pair; a position is a u32 below
// 2^depth; level 0 are the leaves, node `index` of level l covers the
// positions index 2^l .. (index + 1) 2^l - 1.  Writes 0 .. K-1 of a call are
// applied in order.  Write k makes a new version of its ancestor at every
// level; the version at level l + 1 is H of the version at level l and the
// level-l sibling as write k sees it: the version made by the latest earlier
// write under that sibling, or what the tree stored before the call.
constexpr uint32_t AT_MAX_DEPTH = 32;
constexpr uint32_t AT_MAX_WRITES = 1u << 16;  // per call

// index of the highest bit in which two positions differ; -1 when they are equal
ZK_HD int at_hb(uint32_t a, uint32_t b) {
  const uint32_t x = a ^ b;
  if (x == 0) return -1;
#if defined(__HIP_DEVICE_COMPILE__)
  return 31 - __clz((int)x);
#else
  return 31 - __builtin_clz(x);
#endif
}
// Write j lies under write k's level-l sibling iff at_hb == l, and wrote the
// same leaf iff at_hb == -1.  The predecessor of (k, l), l = -1 .. depth - 1:
// the latest j < k with at_hb(pos_j, pos_k) == l, or -1 ("stored").  l = -1
// gives the write whose leaf write k replaces.  (Reference loop: the kernels
// find all levels of a write in one pass over j.)
ZK_HD int32_t at_pred(const uint32_t* pos, uint32_t k, int l) {
  for (uint32_t j = k; j-- > 0;)
    if (at_hb(pos[j], pos[k]) == l) return (int32_t)j;
  return -1;
}
// Write k is the last writer of its level-l ancestor iff no j > k has
// at_hb(pos_j, pos_k) < l.  So one number m_k says what write k stores back:
// its versions of the levels 0 .. m_k; m_k = the least at_hb over the later
// writes, `depth` (the root included) when there is none, -1 (nothing) when a
// later write takes the same leaf.  (Reference loop.)
ZK_HD int at_last_level(const uint32_t* pos, uint32_t K, uint32_t k, uint32_t depth) {
  int m = (int)depth;
  for (uint32_t j = k + 1; j < K; j++) {
    const int h = at_hb(pos[j], pos[k]);
    if (h < m) m = h;
  }
  return m;
}
// one level step of one write: the version at level l + 1 from the version at
// level l and the sibling (canonical words).  Left and right are chosen by
// pointer and the pair is hashed ONCE: a branch around two mimc_pair calls
// would leave a wave that holds left and right children (every real call)
// running both arms, four permutations a level instead of two.
ZK_HD void at_step(const uint32_t* cur, const uint32_t* sib, uint32_t pos, uint32_t l, uint32_t* out, const Fe* tab) {
  const bool right = (pos >> l) & 1;
  mimc_pair(right ? sib : cur, right ? cur : sib, out, tab);
}

// ------------------------------------------------------------ the node store
// An open-addressing table of `slots` keys (u64) beside `slots` values of 8
// words.  key = level << 32 | index (level <= 32, so no key is all ones, the
// mark of an empty slot).  Nothing is ever removed, so a lookup may stop at
// the first empty slot.  Every probe sequence is linear from at_slot and at
// most `slots` long.
constexpr uint64_t AT_EMPTY_KEY = ~0ull;
constexpr int64_t AT_ABSENT = -1;  // at_find: the key is not stored
constexpr int64_t AT_FULL = -2;    // at_claim: gave up, every slot holds another key
ZK_HD uint64_t at_key(uint32_t level, uint32_t index) { return ((uint64_t)level << 32) | index; }
// sibling of the path of `pos` at level l
ZK_HD uint64_t at_sibling_key(uint32_t pos, uint32_t l) { return at_key(l, (pos >> l) ^ 1u); }
ZK_HD uint64_t at_slot(uint64_t key, uint64_t slots) {
  uint64_t x = key * 0x9E3779B97F4A7C15ull;  // Fibonacci mix, then fold the high half down
  x ^= x >> 29;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 32;
  return x % slots;
}
// the slot that holds `key`, or AT_ABSENT
ZK_HD int64_t at_find(const uint64_t* keys, uint64_t slots, uint64_t key) {
  uint64_t s = at_slot(key, slots);
  for (uint64_t n = 0; n < slots; n++) {
    const uint64_t have = keys[s];
    if (have == key) return (int64_t)s;
    if (have == AT_EMPTY_KEY) return AT_ABSENT;
    if (++s == slots) s = 0;
  }
  return AT_ABSENT;
}
// The slot that holds `key`, claiming an empty one when it is not stored
// (*fresh = true), or AT_FULL.  The device form claims with a 64-bit
// compare-and-swap, so lanes that claim different keys at once never share a
// slot; the host form is a plain store.
ZK_HD int64_t at_claim(uint64_t* keys, uint64_t slots, uint64_t key, bool* fresh) {
  *fresh = false;
  uint64_t s = at_slot(key, slots);
  for (uint64_t n = 0; n < slots; n++) {
    uint64_t have = keys[s];
    if (have == AT_EMPTY_KEY) {
#if defined(__HIP_DEVICE_COMPILE__)
      have = atomicCAS(reinterpret_cast<unsigned long long*>(keys + s), (unsigned long long)AT_EMPTY_KEY,
                       (unsigned long long)key);
      if (have == AT_EMPTY_KEY) {
        *fresh = true;
        return (int64_t)s;
      }
#else
      keys[s] = key;
      *fresh = true;
      return (int64_t)s;
#endif
    }
    if (have == key) return (int64_t)s;
    if (++s == slots) s = 0;
  }
  return AT_FULL;
}
// node `key` as the store has it: stored, or e_level.  empty: (depth + 1) x 8 words.
ZK_HD const uint32_t* at_node(const uint64_t* keys, const uint32_t* vals, uint64_t slots, const uint32_t* empty,
                              uint64_t key) {
  const int64_t s = at_find(keys, slots, key);
  return s >= 0 ? vals + 8 * s : empty + 8 * (key >> 32);
}
// most nodes K writes can add: every write its leaf and `depth` ancestors
ZK_HD uint64_t at_worst_case_nodes(uint64_t K, uint32_t depth) { return K * (depth + 1); }

}  // namespace zk
