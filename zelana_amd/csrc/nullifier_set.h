// nullifier_set.h — the arithmetic of the nullifier set: a
// bounded set of 32-byte keys with an ordered, batched "spend".  Host+device
// like mimc_hash.h: the kernels of nullifier_set.hip and the stand-alone host
// check (tests/host/nullifier_set_check.cpp) compile the very same slot
// function, probes, grouping and decision rules.  No HIP call is made here.
//
// A key is 32 raw bytes, 8 little-endian u32 words, compared bytewise: it is
// NOT reduced mod r (the reference keeps a HashSet<[u8; 32]>).
//
// The store has two parts.  The log holds the keys in insertion order,
// capacity x 8 words: what a restart replays.  The table is open addressing
// over `slots` u32 entries, slots a power of two >= 2 capacity; an entry is
// log index + 1, 0 = empty.  Keys are never moved or removed, so a slot is
// claimed with one 32-bit compare-and-swap and equality is decided by reading
// the log; a lookup may stop at the first empty slot.  Every probe sequence is
// linear from ns_slot and at most `slots` long.
//
// The scratch table of one call is the same thing over the call's own key
// array: an entry is item index + 1, equality is decided by reading that
// array.  It gives equal keys of one call one group (the item that claimed the
// entry) without a sort and without trusting a fingerprint.
#pragma once
#include <stdint.h>

#ifndef ZK_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define ZK_HD __host__ __device__ __forceinline__
#else
#define ZK_HD inline
#endif
#endif

namespace zk {

constexpr uint32_t NS_MAX_PER_TX = 4;
constexpr uint64_t NS_MAX_CAPACITY = 1ull << 31;
constexpr uint64_t NS_MAX_CALL_KEYS = 1ull << 24;  // keys of one spend / contains call

// verdicts of a spend (zkmi.h)
constexpr uint32_t NS_ACCEPTED = 0, NS_SKIPPED = 1, NS_SPENT_STORED = 2, NS_SPENT_IN_CALL = 3, NS_DUP_IN_TX = 4;
// state of a transfer while the rounds run
constexpr uint32_t NS_ST_UNDECIDED = 0, NS_ST_ACCEPTED = 1, NS_ST_REJECTED = 2, NS_ST_SKIPPED = 3;
constexpr uint32_t NS_NONE = 0xFFFFFFFFu;  // "no transfer": the start of every minimum

struct NsKey {
  uint32_t w[8];
};
// a key from 16-byte aligned words: two 16-byte loads on the device
ZK_HD NsKey ns_load(const uint32_t* p) {
  NsKey k;
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t v4 __attribute__((ext_vector_type(4)));
  const v4 lo = reinterpret_cast<const v4*>(p)[0], hi = reinterpret_cast<const v4*>(p)[1];
  k.w[0] = lo.x, k.w[1] = lo.y, k.w[2] = lo.z, k.w[3] = lo.w;
  k.w[4] = hi.x, k.w[5] = hi.y, k.w[6] = hi.z, k.w[7] = hi.w;
#else
  for (int i = 0; i < 8; i++) k.w[i] = p[i];
#endif
  return k;
}
ZK_HD void ns_put(uint32_t* p, const NsKey& k) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef uint32_t v4 __attribute__((ext_vector_type(4)));
  v4 lo = {k.w[0], k.w[1], k.w[2], k.w[3]}, hi = {k.w[4], k.w[5], k.w[6], k.w[7]};
  reinterpret_cast<v4*>(p)[0] = lo;
  reinterpret_cast<v4*>(p)[1] = hi;
#else
  for (int i = 0; i < 8; i++) p[i] = k.w[i];
#endif
}
ZK_HD bool ns_eq(const NsKey& a, const NsKey& b) {
  uint32_t d = 0;
  for (int i = 0; i < 8; i++) d |= a.w[i] ^ b.w[i];
  return d == 0;
}

// the smallest power of two >= 2 n (n >= 1)
ZK_HD uint64_t ns_slots_for(uint64_t n) {
  uint64_t s = 2;
  while (s < 2 * n) s <<= 1;
  return s;
}
// Home slot.  Every word goes through a multiply-xorshift step, so keys that
// agree in seven of their words still spread; slots is a power of two.
ZK_HD uint64_t ns_slot(const NsKey& k, uint64_t slots) {
  uint64_t h = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 8; i++) {
    h = (h ^ k.w[i]) * 0xBF58476D1CE4E5B9ull;
    h ^= h >> 29;
  }
  h *= 0x94D049BB133111EBull;
  h ^= h >> 32;
  return h & (slots - 1);
}

// ------------------------------------------------------------------ the store
// log index + 1 of `key`, or 0 when it is not stored
ZK_HD uint32_t ns_find(const uint32_t* table, uint64_t slots, const uint32_t* log, const NsKey& key) {
  uint64_t s = ns_slot(key, slots);
  for (uint64_t n = 0; n < slots; n++) {
    const uint32_t e = table[s];
    if (e == 0) return 0;
    if (ns_eq(ns_load(log + 8 * (uint64_t)(e - 1)), key)) return e;
    s = (s + 1) & (slots - 1);
  }
  return 0;
}
// Enter log index `index` (its key already is, or is being, written to the log)
// under `key`'s probe sequence.  The caller knows that the key is neither
// stored nor entered by anyone else, so no equality probe is made: the first
// empty slot is claimed.  The device form claims with a compare-and-swap, so
// lanes that insert at once never share a slot; the host form is a plain
// store.  false: every slot is taken (cannot happen while count <= capacity).
ZK_HD bool ns_insert(uint32_t* table, uint64_t slots, const NsKey& key, uint32_t index) {
  uint64_t s = ns_slot(key, slots);
  for (uint64_t n = 0; n < slots; n++) {
    if (table[s] == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
      if (atomicCAS(table + s, 0u, index + 1) == 0u) return true;
#else
      table[s] = index + 1;
      return true;
#endif
    }
    s = (s + 1) & (slots - 1);
  }
  return false;
}

// ---------------------------------------------------- the scratch table (call)
// The group of item i of the call's key array `keys`: the item that holds the
// entry of i's key, i itself when it claims the entry.  Equal keys get the same
// group whatever the order in which their lanes arrive; NS_NONE when every slot
// is taken by other keys (cannot happen with sslots >= 2 items).
ZK_HD uint32_t ns_group(uint32_t* scratch, uint64_t sslots, const uint32_t* keys, uint32_t i) {
  const NsKey key = ns_load(keys + 8 * (uint64_t)i);
  uint64_t s = ns_slot(key, sslots);
  for (uint64_t n = 0; n < sslots; n++) {
    uint32_t e = scratch[s];
    if (e == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
      e = atomicCAS(scratch + s, 0u, i + 1);
      if (e == 0) return i;
#else
      scratch[s] = i + 1;
      return i;
#endif
    }
    if (e - 1 == i || ns_eq(ns_load(keys + 8 * (uint64_t)(e - 1)), key)) return e - 1;
    s = (s + 1) & (sslots - 1);
  }
  return NS_NONE;
}

// ------------------------------------------------------- the rules of a spend
// Transfer t holds the keys t per_tx .. t per_tx + per_tx - 1 of the call.
// flags of a transfer: bit k = key k is stored, bit 4 + k = key k equals an
// earlier key of the same transfer.
ZK_HD uint32_t ns_flag_stored(uint32_t k) { return 1u << k; }
ZK_HD uint32_t ns_flag_dup(uint32_t k) { return 16u << k; }
// bit 4 + k when key k of the transfer at `tx_keys` equals one of its keys before it
ZK_HD uint32_t ns_dup_flag(const uint32_t* tx_keys, uint32_t k) {
  const NsKey key = ns_load(tx_keys + 8 * k);
  for (uint32_t j = 0; j < k; j++)
    if (ns_eq(ns_load(tx_keys + 8 * j), key)) return ns_flag_dup(k);
  return 0;
}
// the state the rounds start from
ZK_HD uint32_t ns_state0(bool eligible, uint32_t flags) {
  return !eligible ? NS_ST_SKIPPED : flags ? NS_ST_REJECTED : NS_ST_UNDECIDED;
}
// The decision rule of one round for an UNDECIDED transfer t.  For each of its
// keys, over the states of the round before: cand[k] = the least transfer
// among the holders of the key that are not rejected (t itself is one), acc[k]
// = the least among the accepted holders (NS_NONE when there is none).
//   some acc[k] < t        an earlier transfer spent the key: REJECTED
//   every cand[k] == t     every earlier holder of every key is rejected: ACCEPTED
//   else                   an earlier holder is still undecided: UNDECIDED
// The earliest undecided transfer of a call has no undecided earlier holder,
// so every round decides at least one transfer.
ZK_HD uint32_t ns_decide(uint32_t t, uint32_t per_tx, const uint32_t* cand, const uint32_t* acc) {
  bool first = true;
  for (uint32_t k = 0; k < per_tx; k++) {
    if (acc[k] < t) return NS_ST_REJECTED;
    first = first && cand[k] == t;
  }
  return first ? NS_ST_ACCEPTED : NS_ST_UNDECIDED;
}
// Why a REJECTED transfer t was refused, from the final states: the first key,
// in key order, that fails, and of its failures the first of: stored, spent by
// the accepted earlier transfer acc[k] < t, equal to an earlier key of t.
// Returns the verdict code, *detail = k, acc[k], k.
ZK_HD uint32_t ns_reason(uint32_t t, uint32_t per_tx, uint32_t flags, const uint32_t* acc, uint32_t* detail) {
  for (uint32_t k = 0; k < per_tx; k++) {
    *detail = k;
    if (flags & ns_flag_stored(k)) return NS_SPENT_STORED;
    if (acc[k] < t) {
      *detail = acc[k];
      return NS_SPENT_IN_CALL;
    }
    if (flags & ns_flag_dup(k)) return NS_DUP_IN_TX;
  }
  *detail = 0;
  return NS_ACCEPTED;  // not reached for a rejected transfer
}

}  // namespace zk
