// nullifier_set_check — the device header of the nullifier set
// (zelana_amd/csrc/nullifier_set.h) compiled for the host, alone: the slot
// function, the store's probes in their host form, the scratch grouping and the
// rules of a round, driven serially over plain arrays, step for step as the
// kernels of nullifier_set.hip drive them over device memory.
//
//   nullifier_set_check SCRIPT
// SCRIPT: text, whitespace-separated; a key is 64 hex digits (32 bytes).
//   H slots key                    -> "h <home slot>"
//   N capacity                     a new, empty set -> "n <slots>"
//   S per_tx ntx {eligible key_0 .. key_{per_tx-1}} x ntx
//                                  one spend -> per transfer "v <t> <verdict> <detail>", then
//                                  "s <rounds> <count>"; or "full <count>" when refused (nothing changes)
//   C key                          -> "c <0|1>"
//   L                              -> "l <count> <key> .." the log
//   P key                          -> "p <slots probed by a lookup of key>"
// Nothing here knows an expected value: tests/test_nullifier_set_cpu.py holds
// the output against the sequential model over a Python set.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zelana_amd/csrc/nullifier_set.h"

using namespace zk;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

static bool read_key(FILE* fp, uint32_t w[8]) {
  char hex[80];
  if (fscanf(fp, "%79s", hex) != 1 || strlen(hex) != 64) return false;
  uint8_t b[32];
  for (int i = 0; i < 32; i++) {
    unsigned v;
    if (sscanf(hex + 2 * i, "%2x", &v) != 1) return false;
    b[i] = (uint8_t)v;
  }
  memcpy(w, b, 32);
  return true;
}
static void print_key(const uint32_t* w) {
  uint8_t b[32];
  memcpy(b, w, 32);
  putchar(' ');
  for (int i = 0; i < 32; i++) printf("%02x", b[i]);
}

struct HostSet {
  uint64_t capacity = 0, slots = 0, count = 0;
  std::vector<uint32_t> log, table;
};

// the launch sequence of nullifier_set.hip's spend, on the host; false = refused
static bool spend(HostSet& s, uint32_t ntx, uint32_t per_tx, const std::vector<uint32_t>& keys,
                  const std::vector<uint8_t>& eligible, std::vector<uint32_t>& verdict, std::vector<uint32_t>& detail,
                  uint32_t* rounds_out) {
  const uint32_t nkeys = ntx * per_tx;
  const uint64_t sslots = ns_slots_for(nkeys);
  std::vector<uint32_t> scratch(sslots, 0), flags(ntx, 0), group(nkeys, NS_NONE), state(ntx);
  // lookup and grouping, a "lane" per key of an eligible transfer
  for (uint32_t i = 0; i < nkeys; i++) {
    const uint32_t t = i / per_tx, k = i % per_tx;
    if (!eligible[t]) continue;
    uint32_t f = ns_dup_flag(keys.data() + 8 * (size_t)t * per_tx, k);
    if (ns_find(s.table.data(), s.slots, s.log.data(), ns_load(keys.data() + 8 * (size_t)i))) f |= ns_flag_stored(k);
    flags[t] |= f;
    group[i] = ns_group(scratch.data(), sslots, keys.data(), i);
    if (group[i] == NS_NONE) abort();
  }
  uint32_t undecided = 0;
  for (uint32_t t = 0; t < ntx; t++) {
    state[t] = ns_state0(eligible[t] != 0, flags[t]);
    undecided += state[t] == NS_ST_UNDECIDED;
  }
  // rounds: the minima over the states of the round before, then the decisions
  std::vector<uint32_t> cand(nkeys), acc(nkeys, NS_NONE);
  auto minima = [&](bool with_cand) {
    for (uint32_t i = 0; i < nkeys; i++) {
      const uint32_t t = i / per_tx, st = state[t];
      if (st == NS_ST_SKIPPED || st == NS_ST_REJECTED) continue;
      const uint32_t g = group[i];
      if (with_cand && t < cand[g]) cand[g] = t;
      if (st == NS_ST_ACCEPTED && t < acc[g]) acc[g] = t;
    }
  };
  uint32_t rounds = 0;
  for (; undecided != 0 && rounds < ntx; rounds++) {
    cand.assign(nkeys, NS_NONE);
    minima(true);
    undecided = 0;
    for (uint32_t t = 0; t < ntx; t++) {
      if (state[t] != NS_ST_UNDECIDED) continue;
      uint32_t c[NS_MAX_PER_TX], a[NS_MAX_PER_TX];
      for (uint32_t k = 0; k < per_tx; k++) c[k] = cand[group[t * per_tx + k]], a[k] = acc[group[t * per_tx + k]];
      state[t] = ns_decide(t, per_tx, c, a);  // reads cand / acc only: the states of the round before
      undecided += state[t] == NS_ST_UNDECIDED;
    }
  }
  if (undecided) abort();
  minima(false);
  // reasons
  uint32_t accepted = 0;
  for (uint32_t t = 0; t < ntx; t++) {
    uint32_t v = state[t] == NS_ST_ACCEPTED ? NS_ACCEPTED : NS_SKIPPED, d = 0;
    if (state[t] == NS_ST_REJECTED) {
      uint32_t a[NS_MAX_PER_TX];
      for (uint32_t k = 0; k < per_tx; k++) a[k] = acc[group[t * per_tx + k]];
      v = ns_reason(t, per_tx, flags[t], a, &d);
    }
    verdict[t] = v, detail[t] = d;
    accepted += state[t] == NS_ST_ACCEPTED;
  }
  if (s.count + (uint64_t)accepted * per_tx > s.capacity) return false;
  // insert, in transfer order then key order
  for (uint32_t t = 0; t < ntx; t++) {
    if (state[t] != NS_ST_ACCEPTED) continue;
    for (uint32_t k = 0; k < per_tx; k++) {
      const NsKey key = ns_load(keys.data() + 8 * ((size_t)t * per_tx + k));
      ns_put(s.log.data() + 8 * s.count, key);
      if (!ns_insert(s.table.data(), s.slots, key, (uint32_t)s.count)) abort();
      s.count++;
    }
  }
  *rounds_out = rounds;
  return true;
}

int main(int argc, char** argv) {
  CHECK(argc == 2, "usage: nullifier_set_check SCRIPT");
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp, "cannot open %s", argv[1]);
  HostSet s;
  char cmd[8];
  while (fscanf(fp, "%7s", cmd) == 1) {
    if (!strcmp(cmd, "H")) {
      unsigned long long slots;
      uint32_t w[8];
      CHECK(fscanf(fp, "%llu", &slots) == 1 && slots >= 2 && (slots & (slots - 1)) == 0, "H: slots");
      CHECK(read_key(fp, w), "H: key");
      printf("h %llu\n", (unsigned long long)ns_slot(ns_load(w), slots));
    } else if (!strcmp(cmd, "N")) {
      unsigned long long cap;
      CHECK(fscanf(fp, "%llu", &cap) == 1 && cap >= 1 && cap <= (1ull << 20), "N: capacity");
      s = HostSet();
      s.capacity = cap;
      s.slots = ns_slots_for(cap);
      s.log.assign(cap * 8, 0);
      s.table.assign(s.slots, 0);
      printf("n %llu\n", (unsigned long long)s.slots);
    } else if (!strcmp(cmd, "S")) {
      unsigned per_tx, ntx;
      CHECK(s.capacity, "S: no set");
      CHECK(fscanf(fp, "%u %u", &per_tx, &ntx) == 2 && per_tx >= 1 && per_tx <= NS_MAX_PER_TX && ntx >= 1 &&
                ntx <= (1u << 16),
            "S: per_tx, ntx");
      std::vector<uint32_t> keys((size_t)ntx * per_tx * 8), verdict(ntx), detail(ntx);
      std::vector<uint8_t> eligible(ntx);
      for (unsigned t = 0; t < ntx; t++) {
        unsigned e;
        CHECK(fscanf(fp, "%u", &e) == 1 && e <= 1, "S: eligible");
        eligible[t] = (uint8_t)e;
        for (unsigned k = 0; k < per_tx; k++) CHECK(read_key(fp, keys.data() + 8 * ((size_t)t * per_tx + k)), "S: key");
      }
      uint32_t rounds = 0;
      if (!spend(s, ntx, per_tx, keys, eligible, verdict, detail, &rounds)) {
        printf("full %llu\n", (unsigned long long)s.count);
        continue;
      }
      for (unsigned t = 0; t < ntx; t++) printf("v %u %u %u\n", t, verdict[t], detail[t]);
      printf("s %u %llu\n", rounds, (unsigned long long)s.count);
    } else if (!strcmp(cmd, "C") || !strcmp(cmd, "P")) {
      uint32_t w[8];
      CHECK(s.capacity, "%s: no set", cmd);
      CHECK(read_key(fp, w), "%s: key", cmd);
      const NsKey key = ns_load(w);
      if (cmd[0] == 'C') {
        printf("c %d\n", ns_find(s.table.data(), s.slots, s.log.data(), key) != 0);
      } else {  // the slots a lookup reads, counted by walking as ns_find does
        uint64_t at = ns_slot(key, s.slots), n = 1;
        while (n < s.slots && s.table[at] != 0 && !ns_eq(ns_load(s.log.data() + 8 * (size_t)(s.table[at] - 1)), key))
          at = (at + 1) & (s.slots - 1), n++;
        printf("p %llu\n", (unsigned long long)n);
      }
    } else if (!strcmp(cmd, "L")) {
      CHECK(s.capacity, "L: no set");
      printf("l %llu", (unsigned long long)s.count);
      for (uint64_t i = 0; i < s.count; i++) print_key(s.log.data() + 8 * i);
      printf("\n");
    } else {
      CHECK(false, "unknown command %s", cmd);
    }
  }
  fclose(fp);
  printf("ok\n");
  return 0;
}
