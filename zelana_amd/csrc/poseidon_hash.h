// poseidon_hash.h — the Poseidon sponge over Fr as a primitive, one lane per
// hash, and the index arithmetic of the note commitment tree over it
// (DESIGN.md §2.11).  Host+device like pairing.h / proof_decode.h / fq_sqrt.h:
// the kernels of note_tree.hip and the stand-alone host check
// (tests/host/note_tree_check.cpp) compile the very same permutation, sponge,
// batch rehash and per-insertion fold.
//
// Parameters are runtime values: R_f (even, >= 2) full and R_p partial rounds,
// R_f + R_p <= POSH_MAX_ROUNDS, x^5, width 3 (rate 2, capacity 1).  The
// constant table has the layout of a kind-9 witness-program op (zkmi.h):
// ark[r][i] at 3 r + i, mds[i][j] at 3 (R_f + R_p) + 3 i + j, here as Fe in
// Montgomery form, fully reduced.  Unlike wprog.hip's poseidon_quad (a quad of
// lanes per permutation, every S-box value stored as a witness) a lane here
// holds the whole state (27 limbs) and stores nothing but the result.
//
// Field elements cross this header as 8 little-endian u32 words.  Inputs may
// be ANY 256-bit value: they are taken mod r (Fr::from_le_bytes_mod_order) by
// the conversion to Montgomery form.  Outputs are canonical (< r).
#pragma once
#include "ff.h"

namespace zk {

constexpr int POSH_MAX_ROUNDS = 72;
constexpr int POSH_MAX_NCONST = 3 * POSH_MAX_ROUNDS + 9;
ZK_HD uint32_t posh_nconst(uint32_t rf, uint32_t rp) { return 3 * (rf + rp) + 9; }
ZK_HD bool posh_rounds_ok(uint32_t rf, uint32_t rp) {
  return rf >= 2 && (rf & 1) == 0 && rp <= (uint32_t)POSH_MAX_ROUNDS && rf + rp <= (uint32_t)POSH_MAX_ROUNDS;
}

// (a0 b0 + a1 b1 + a2 b2) 2^-261 mod r with one reduction: an MDS row.  a_k <
// r (the table's constants), b_k < 2r, all limbs normalised: the sum is < 6
// r^2, inside the Montgomery bound (2^261 / r = 169), so the result is < 2r;
// a column holds at most 27 + 9 products of 58 bits, below 2^64.  Plain C (not
// ff.h's one-chain mads): the constants are uniform over a wave, and the
// compiler is free to keep them where it finds them.
ZK_HD Fe posh_mul3(const Fe& a0, const Fe& b0, const Fe& a1, const Fe& b1, const Fe& a2, const Fe& b2) {
  uint32_t m[NL];
  Fe r;
  uint64_t acc = 0;
#pragma unroll
  for (int k = 0; k < NL; k++) {
#pragma unroll
    for (int j = 0; j <= k; j++) {
      acc += (uint64_t)a0.v[j] * b0.v[k - j];
      acc += (uint64_t)a1.v[j] * b1.v[k - j];
      acc += (uint64_t)a2.v[j] * b2.v[k - j];
      if (j < k) acc += (uint64_t)m[j] * FrP::P[k - j];
    }
    m[k] = ((uint32_t)acc * FrP::PINV) & LMASK;
    acc += (uint64_t)m[k] * FrP::P[0];
    acc >>= 29;
  }
#pragma unroll
  for (int k = NL; k < 2 * NL - 1; k++) {
#pragma unroll
    for (int j = k - (NL - 1); j < NL; j++) {
      acc += (uint64_t)a0.v[j] * b0.v[k - j];
      acc += (uint64_t)a1.v[j] * b1.v[k - j];
      acc += (uint64_t)a2.v[j] * b2.v[k - j];
      acc += (uint64_t)m[j] * FrP::P[k - j];
    }
    r.v[k - NL] = (uint32_t)acc & LMASK;
    acc >>= 29;
  }
  r.v[NL - 1] = (uint32_t)acc;
  return r;
}

// x^5.  P = FrP: one-chain mads, for kernels that fill the device; ff.h's
// FrPn: for the latency-bound ones
template <class P = FrP>
ZK_HD Fe posh_sbox(const Fe& t) {
  const Fe x2 = sqr<P>(t);
  return mul<P>(sqr<P>(x2), t);
}

// One permutation of the state s (Montgomery form, < 2r): per round add the
// round constants, x^5 on every element (the first and last half = R_f / 2
// rounds) or on element 0 alone, then the dense MDS product.  18 field
// products a full round, 12 a partial one.
ZK_HD void posh_permute(Fe s[3], const Fe* pc, uint32_t half, uint32_t rounds) {
  const Fe* mds = pc + 3 * rounds;
  for (uint32_t r = 0; r < rounds; r++) {
    Fe t0 = add<FrP>(s[0], pc[3 * r]), t1 = add<FrP>(s[1], pc[3 * r + 1]), t2 = add<FrP>(s[2], pc[3 * r + 2]);
    t0 = posh_sbox(t0);
    if (r < half || r >= rounds - half) {
      t1 = posh_sbox(t1);
      t2 = posh_sbox(t2);
    }
    s[0] = posh_mul3(mds[0], t0, mds[1], t1, mds[2], t2);
    s[1] = posh_mul3(mds[3], t0, mds[4], t1, mds[5], t2);
    s[2] = posh_mul3(mds[6], t0, mds[7], t1, mds[8], t2);
  }
}

// absorb(x_0 .. x_{arity-1}); squeeze_field_elements(1)[0] of the duplex
// sponge, arity 1..4: inputs are added to state[1], state[2]; the sponge
// permutes when the rate is full and before the squeeze, that is once per
// started pair of inputs; the result is state[1].  in: arity x 8 words.
ZK_HD void posh_sponge(const uint32_t* in, uint32_t arity, uint32_t* out, const Fe* pc, uint32_t half,
                       uint32_t rounds) {
  Fe s[3] = {fe_zero(), fe_zero(), fe_zero()};
  for (uint32_t c = 0; c < arity; c += 2) {
    s[1] = add<FrP>(s[1], fr_in(in + 8 * c));
    if (c + 1 < arity) s[2] = add<FrP>(s[2], fr_in(in + 8 * c + 8));
    posh_permute(s, pc, half, rounds);
  }
  fr_out(out, s[1]);
}
// H(left, right): the tree's node hash
ZK_HD void posh_pair(const uint32_t* left, const uint32_t* right, uint32_t* out, const Fe* pc, uint32_t half,
                     uint32_t rounds) {
  Fe s[3] = {fe_zero(), fr_in(left), fr_in(right)};
  posh_permute(s, pc, half, rounds);
  fr_out(out, s[1]);
}
// the table of a parameter set from its canonical constants (n x 8 words)
ZK_HD void posh_table(const uint32_t* canon, uint32_t n, Fe* pc) {
  for (uint32_t i = 0; i < n; i++) pc[i] = reduce<FrP>(fr_in(canon + 8 * i));
}

// ------------------------------------------------------------------ the tree
// An append-only tree of `depth` levels over posh_pair (MerkleTree of the
// reference's sdk/privacy/src/merkle.rs).  Level 0 are the leaves; level l
// stores ceil(capacity / 2^l) nodes (one node once 2^l >= capacity), 8
// canonical words each, level after level in one array.  A node exists once a
// leaf below it does; a node that does not exist reads as e_l, the root of an
// empty subtree of height l (e_0 = the empty leaf, e_{l+1} = H(e_l, e_l)).
constexpr uint32_t NT_MAX_DEPTH = 32;
struct NtGeom {
  uint64_t off[NT_MAX_DEPTH + 2];  // first node of level l; off[depth + 1] = all nodes
  uint32_t depth;
};
// nodes level l stores for a tree of `capacity` leaves (1 .. 2^32)
ZK_HD uint64_t nt_level_nodes(uint64_t capacity, uint32_t l) { return (capacity + ((1ull << l) - 1)) >> l; }
ZK_HD void nt_geom(NtGeom& g, uint32_t depth, uint64_t capacity) {
  g.depth = depth;
  uint64_t at = 0;
  for (uint32_t l = 0; l <= depth; l++) {
    g.off[l] = at;
    at += nt_level_nodes(capacity, l);
  }
  for (uint32_t l = depth + 1; l < NT_MAX_DEPTH + 2; l++) g.off[l] = at;
}
// does node idx of level l exist in a tree holding the leaves [0, next)?
ZK_HD bool nt_present(uint32_t l, uint64_t idx, uint64_t next) { return next != 0 && idx <= ((next - 1) >> l); }
// the nodes of level l above the leaves [first, first + n), n > 0: [*lo, *lo + *cnt)
ZK_HD void nt_touched(uint64_t first, uint64_t n, uint32_t l, uint64_t* lo, uint64_t* cnt) {
  *lo = first >> l;
  *cnt = ((first + n - 1) >> l) - *lo + 1;
}
// node idx of level l as the tree of `next` leaves has it: stored, or e_l.
// empty: (depth + 1) x 8 words.
ZK_HD const uint32_t* nt_node(const uint32_t* tree, const uint32_t* empty, const NtGeom& g, uint32_t l, uint64_t idx,
                              uint64_t next) {
  return nt_present(l, idx, next) ? tree + (g.off[l] + idx) * 8 : empty + 8 * l;
}
// Batch rehash, one node: node p of level l >= 1 from its two children as the
// tree of `next` leaves has them (the left one always exists).  An append of
// [first, first + n) runs this over nt_touched(first, n, l) for l = 1 ..
// depth, a level after the one below it.
ZK_HD void nt_rehash(uint32_t* tree, const uint32_t* empty, const NtGeom& g, uint32_t l, uint64_t p, uint64_t next,
                     const Fe* pc, uint32_t half, uint32_t rounds) {
  const uint32_t* left = tree + (g.off[l - 1] + 2 * p) * 8;
  const uint32_t* right = nt_node(tree, empty, g, l - 1, 2 * p + 1, next);
  posh_pair(left, right, tree + (g.off[l] + p) * 8, pc, half, rounds);
}
// The root after leaf k alone has been added to the leaves before it
// (MerkleTree::insert_at at position k of a tree holding [0, k)), from a tree
// that holds k and any number of later leaves: carry the leaf upward; where
// the carried node is a right child its sibling is the stored left node, whose
// leaves all precede k, so it is final; where it is a left child the sibling
// holds only later leaves and was e_l at the time.
ZK_HD void nt_root_after(const uint32_t* tree, const uint32_t* empty, const NtGeom& g, uint64_t k, uint32_t* out,
                         const Fe* pc, uint32_t half, uint32_t rounds) {
  Fe cur = fr_in(tree + (g.off[0] + k) * 8);
  uint64_t idx = k;
  for (uint32_t l = 0; l < g.depth; l++, idx >>= 1) {
    Fe s[3];
    s[0] = fe_zero();
    if (idx & 1) {
      s[1] = fr_in(tree + (g.off[l] + idx - 1) * 8);
      s[2] = cur;
    } else {
      s[1] = cur;
      s[2] = fr_in(empty + 8 * l);
    }
    posh_permute(s, pc, half, rounds);
    cur = s[1];
  }
  fr_out(out, cur);
}
// sibling of the path of leaf `position` at level l, in a tree of `next` leaves
ZK_HD const uint32_t* nt_sibling(const uint32_t* tree, const uint32_t* empty, const NtGeom& g, uint32_t l,
                                 uint64_t position, uint64_t next) {
  return nt_node(tree, empty, g, l, (position >> l) ^ 1, next);
}

}  // namespace zk
