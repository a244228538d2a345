// account_tree_check — the device header of the MiMC hash and the account tree
// (zelana_amd/csrc/mimc_hash.h) compiled for the host, alone: the sponge, the
// empty-subtree chain, the node store's probes in their host form, and a host
// model of an apply that runs the header's ordering rule (at_pred,
// at_last_level), level steps (at_step) and write-back (at_claim) over plain
// arrays, step for step as the kernels of account_tree.hip do over device
// memory.
//
//   account_tree_check SCRIPT
// SCRIPT: text, whitespace-separated; field elements are 64 hex digits, the 32
// bytes little-endian, any 256-bit value; positions and keys are decimal.
//   H arity x_0 .. x_{arity-1}     -> "h <hash>"
//   E depth                        -> "e <e_0> .. <e_depth>"
//   T depth max_nodes              a new, empty tree
//   A K pos_0 leaf_0 .. pos_{K-1} leaf_{K-1}
//                                  K ordered writes -> per write
//                                  "w <k> <replaced leaf> <root after> <sibling_0> .. <sibling_{depth-1}>",
//                                  or "full <nodes stored>" when refused (nothing changes)
//   P pos                          -> "p <pos> <leaf> <sibling_0> .. <sibling_{depth-1}>" (current state)
//   R                              -> "r <nodes stored> <root>"
//   O depth K pos_0 .. pos_{K-1}   -> per write "o <k> <m_k> <pred_-1> .. <pred_{depth-1}>"
//   S slots                        a new, bare store
//   K key                          claim -> "k <slot, or -2> <fresh>"
//   F key                          find  -> "f <slot, or -1>"
// Nothing here knows an expected value: tests/test_mimc_hash_cpu.py holds the
// output against zbatch.mimc_hash and zbatch.SparseTree written one leaf at a time.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../zelana_amd/csrc/mimc_hash.h"

using namespace zk;

#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

static bool read_fe(FILE* fp, uint32_t w[8]) {
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
static void print_fe(const uint32_t* w) {
  uint8_t b[32];
  memcpy(b, w, 32);
  putchar(' ');
  for (int i = 0; i < 32; i++) printf("%02x", b[i]);
}

struct HostTree {
  uint32_t depth = 0;
  uint64_t slots = 0, count = 0;
  std::vector<uint64_t> keys;
  std::vector<uint32_t> vals, empty;
  uint32_t root[8];
};

static uint64_t ancestor_key(uint32_t pos, uint32_t l) { return at_key(l, l >= 32 ? 0u : pos >> l); }

// the launch sequence of account_tree.hip's apply, on the host
static int apply(HostTree& t, const std::vector<uint32_t>& pos, const std::vector<uint32_t>& raw, const Fe* tab) {
  const uint32_t K = (uint32_t)pos.size(), depth = t.depth;
  // ordering pass
  std::vector<int32_t> pred((size_t)K * (depth + 1)), mlast(K);
  for (uint32_t k = 0; k < K; k++) {
    for (int l = -1; l < (int)depth; l++) pred[(size_t)k * (depth + 1) + l + 1] = at_pred(pos.data(), k, l);
    mlast[k] = at_last_level(pos.data(), K, k, depth);
  }
  // stored nodes; 0xA5 wherever a level step has to write first
  std::vector<uint32_t> ver((size_t)K * (depth + 1) * 8, 0xA5A5A5A5u), sib((size_t)K * depth * 8, 0xA5A5A5A5u),
      old((size_t)K * 8, 0xA5A5A5A5u);
  for (uint32_t k = 0; k < K; k++) {
    const int32_t* pk = &pred[(size_t)k * (depth + 1)];
    fr_canon(&raw[(size_t)k * 8], &ver[(size_t)k * 8]);
    if (pk[0] < 0) memcpy(&old[(size_t)k * 8], at_node(t.keys.data(), t.vals.data(), t.slots, t.empty.data(), at_key(0, pos[k])), 32);
    for (uint32_t l = 0; l < depth; l++)
      if (pk[l + 1] < 0)
        memcpy(&sib[((size_t)k * depth + l) * 8],
               at_node(t.keys.data(), t.vals.data(), t.slots, t.empty.data(), at_sibling_key(pos[k], l)), 32);
  }
  // level steps: level l + 1 of every write from level l of this call alone
  for (uint32_t l = 0; l < depth; l++) {
    for (uint32_t k = 0; k < K; k++) {
      const int32_t* pk = &pred[(size_t)k * (depth + 1)];
      if (l == 0 && pk[0] >= 0) memcpy(&old[(size_t)k * 8], &ver[(size_t)pk[0] * 8], 32);
      uint32_t* mine = &sib[((size_t)k * depth + l) * 8];
      if (pk[l + 1] >= 0) memcpy(mine, &ver[((size_t)l * K + pk[l + 1]) * 8], 32);
      at_step(&ver[((size_t)l * K + k) * 8], mine, pos[k], l, &ver[((size_t)(l + 1) * K + k) * 8], tab);
    }
  }
  // write-back
  for (uint32_t k = 0; k < K; k++) {
    for (int l = 0; l <= mlast[k]; l++) {
      bool fresh;
      const int64_t s = at_claim(t.keys.data(), t.slots, ancestor_key(pos[k], (uint32_t)l), &fresh);
      CHECK(s >= 0, "A: the store gave up after the capacity check");
      if (fresh) t.count++;
      memcpy(&t.vals[8 * s], &ver[((size_t)l * K + k) * 8], 32);
    }
  }
  memcpy(t.root, &ver[((size_t)depth * K + K - 1) * 8], 32);
  for (uint32_t k = 0; k < K; k++) {
    printf("w %u", k);
    print_fe(&old[(size_t)k * 8]);
    print_fe(&ver[((size_t)depth * K + k) * 8]);
    for (uint32_t l = 0; l < depth; l++) print_fe(&sib[((size_t)k * depth + l) * 8]);
    printf("\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: account_tree_check SCRIPT");
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp, "cannot open %s", argv[1]);
  std::vector<Fe> tab(MIMC_NTABLE);
  mimc_table(tab.data());
  HostTree t;
  std::vector<uint64_t> store;
  char cmd[8];
  while (fscanf(fp, "%7s", cmd) == 1) {
    CHECK(cmd[1] == 0, "unknown command %s", cmd);
    if (cmd[0] == 'H') {
      unsigned arity;
      CHECK(fscanf(fp, "%u", &arity) == 1 && arity >= 1 && arity <= 4, "H: bad arity");
      uint32_t in[32], out[8];
      for (unsigned i = 0; i < arity; i++) CHECK(read_fe(fp, in + 8 * i), "H: bad input");
      mimc_hash(in, arity, out, tab.data());
      printf("h");
      print_fe(out);
      printf("\n");
    } else if (cmd[0] == 'E' || cmd[0] == 'T') {
      unsigned depth;
      unsigned long long slots = 1;
      CHECK(fscanf(fp, "%u", &depth) == 1 && depth >= 1 && depth <= AT_MAX_DEPTH, "%s: bad depth", cmd);
      if (cmd[0] == 'T') CHECK(fscanf(fp, "%llu", &slots) == 1 && slots >= 1 && slots <= (1ull << 24), "T: bad max_nodes");
      t = HostTree();
      t.depth = depth;
      t.slots = slots;
      t.keys.assign(slots, AT_EMPTY_KEY);
      t.vals.assign(slots * 8, 0xA5A5A5A5u);  // a read of a value never written shows in the output
      t.empty.assign((depth + 1) * 8, 0);
      for (unsigned l = 0; l < depth; l++) mimc_pair(&t.empty[8 * l], &t.empty[8 * l], &t.empty[8 * l + 8], tab.data());
      memcpy(t.root, &t.empty[8 * depth], 32);
      if (cmd[0] == 'E') {
        printf("e");
        for (unsigned l = 0; l <= depth; l++) print_fe(&t.empty[8 * l]);
        printf("\n");
      }
    } else if (cmd[0] == 'A') {
      unsigned long long K;
      CHECK(t.depth, "A before T");
      CHECK(fscanf(fp, "%llu", &K) == 1 && K >= 1 && K <= AT_MAX_WRITES, "A: bad count");
      std::vector<uint32_t> pos(K), raw(K * 8);
      for (uint64_t k = 0; k < K; k++) {
        unsigned long long p;
        CHECK(fscanf(fp, "%llu", &p) == 1 && (p >> t.depth) == 0, "A: bad position");
        pos[k] = (uint32_t)p;
        CHECK(read_fe(fp, &raw[k * 8]), "A: bad leaf");
      }
      if (t.count + at_worst_case_nodes(K, t.depth) > t.slots) {
        printf("full %llu\n", (unsigned long long)t.count);
        continue;
      }
      if (apply(t, pos, raw, tab.data())) return 1;
    } else if (cmd[0] == 'P') {
      unsigned long long p;
      CHECK(t.depth, "P before T");
      CHECK(fscanf(fp, "%llu", &p) == 1 && (p >> t.depth) == 0, "P: bad position");
      printf("p %llu", p);
      print_fe(at_node(t.keys.data(), t.vals.data(), t.slots, t.empty.data(), at_key(0, (uint32_t)p)));
      for (uint32_t l = 0; l < t.depth; l++)
        print_fe(at_node(t.keys.data(), t.vals.data(), t.slots, t.empty.data(), at_sibling_key((uint32_t)p, l)));
      printf("\n");
    } else if (cmd[0] == 'R') {
      CHECK(t.depth, "R before T");
      printf("r %llu", (unsigned long long)t.count);
      print_fe(t.root);
      printf("\n");
    } else if (cmd[0] == 'O') {
      unsigned depth;
      unsigned long long K;
      CHECK(fscanf(fp, "%u %llu", &depth, &K) == 2 && depth >= 1 && depth <= AT_MAX_DEPTH && K >= 1 && K <= AT_MAX_WRITES,
            "O: bad arguments");
      std::vector<uint32_t> pos(K);
      for (uint64_t k = 0; k < K; k++) {
        unsigned long long p;
        CHECK(fscanf(fp, "%llu", &p) == 1 && (p >> depth) == 0, "O: bad position");
        pos[k] = (uint32_t)p;
      }
      for (uint32_t k = 0; k < K; k++) {
        printf("o %u %d", k, at_last_level(pos.data(), (uint32_t)K, k, depth));
        for (int l = -1; l < (int)depth; l++) printf(" %d", at_pred(pos.data(), k, l));
        printf("\n");
      }
    } else if (cmd[0] == 'S') {
      unsigned long long slots;
      CHECK(fscanf(fp, "%llu", &slots) == 1 && slots >= 1 && slots <= (1ull << 24), "S: bad slot count");
      store.assign(slots, AT_EMPTY_KEY);
    } else if (cmd[0] == 'K' || cmd[0] == 'F') {
      unsigned long long key;
      CHECK(!store.empty(), "%s before S", cmd);
      CHECK(fscanf(fp, "%llu", &key) == 1 && key != AT_EMPTY_KEY, "%s: bad key", cmd);
      if (cmd[0] == 'K') {
        bool fresh;
        const int64_t s = at_claim(store.data(), store.size(), key, &fresh);
        printf("k %lld %d\n", (long long)s, fresh ? 1 : 0);
      } else {
        printf("f %lld\n", (long long)at_find(store.data(), store.size(), key));
      }
    } else {
      CHECK(false, "unknown command %s", cmd);
    }
  }
  fclose(fp);
  printf("ok\n");
  return 0;
}
