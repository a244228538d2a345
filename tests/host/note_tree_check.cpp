// note_tree_check — the device header of the Poseidon hash and the note tree
// (zelana_amd/csrc/poseidon_hash.h) compiled for the host, alone: the sponge,
// the empty-subtree chain, and a host model of the tree that runs the header's
// index functions, batch rehash (nt_rehash over nt_touched, level by level)
// and per-insertion fold (nt_root_after) over a plain array, exactly as the
// kernels of note_tree.hip do over device memory.
//
//   note_tree_check SCRIPT
// SCRIPT: text, whitespace-separated; field elements are 64 hex digits, the 32
// bytes little-endian, any 256-bit value.
//   C rf rp c_0 .. c_{3(rf+rp)+8}    the parameter set (first)
//   H arity x_0 .. x_{arity-1}       -> "h <hash>"
//   E depth empty_leaf               -> "e <e_0> .. <e_depth>"
//   T depth capacity empty_leaf      a new, empty tree
//   A n leaf_0 .. leaf_{n-1}         append -> "a <first> <root after leaf 0> .. <final root>"
//                                    (the final root is read from the tree's top node)
//   P                                -> per leaf "p <position> <leaf> <sibling_0> .. <sibling_{depth-1}>"
//   B count arity                    -> "b <hashes per second>": `count` dependent hashes, one thread
// Nothing here knows an expected value: tests/test_poseidon_hash_cpu.py holds
// the output against shielded.sponge_hash and a one-leaf-at-a-time model.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <vector>

#include "../../zelana_amd/csrc/poseidon_hash.h"

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
  NtGeom g;
  uint64_t capacity = 0, next = 0;
  std::vector<uint32_t> nodes, empty;
};

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: note_tree_check SCRIPT");
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp, "cannot open %s", argv[1]);
  std::vector<Fe> pc;
  uint32_t half = 0, rounds = 0;
  HostTree t;
  char cmd[8];
  while (fscanf(fp, "%7s", cmd) == 1) {
    if (cmd[0] == 'C') {
      unsigned rf, rp;
      CHECK(fscanf(fp, "%u %u", &rf, &rp) == 2 && posh_rounds_ok(rf, rp), "C: bad round counts");
      const uint32_t n = posh_nconst(rf, rp);
      std::vector<uint32_t> canon(n * 8);
      for (uint32_t i = 0; i < n; i++) CHECK(read_fe(fp, &canon[8 * i]), "C: bad constant %u", i);
      pc.resize(n);
      posh_table(canon.data(), n, pc.data());
      half = rf / 2;
      rounds = rf + rp;
      continue;
    }
    CHECK(!pc.empty(), "%s before C", cmd);
    if (cmd[0] == 'H') {
      unsigned arity;
      CHECK(fscanf(fp, "%u", &arity) == 1 && arity >= 1 && arity <= 4, "H: bad arity");
      uint32_t in[32], out[8];
      for (unsigned i = 0; i < arity; i++) CHECK(read_fe(fp, in + 8 * i), "H: bad input");
      posh_sponge(in, arity, out, pc.data(), half, rounds);
      printf("h");
      print_fe(out);
      printf("\n");
    } else if (cmd[0] == 'E' || cmd[0] == 'T') {
      unsigned depth;
      unsigned long long cap = 1;
      CHECK(fscanf(fp, "%u", &depth) == 1 && depth >= 1 && depth <= NT_MAX_DEPTH, "%s: bad depth", cmd);
      if (cmd[0] == 'T') CHECK(fscanf(fp, "%llu", &cap) == 1 && cap >= 1 && cap <= (1ull << depth), "T: bad capacity");
      uint32_t leaf[8];
      CHECK(read_fe(fp, leaf), "%s: bad empty leaf", cmd);
      t = HostTree();
      t.capacity = cap;
      nt_geom(t.g, depth, cap);
      t.empty.resize((depth + 1) * 8);
      fr_canon(leaf, t.empty.data());
      for (unsigned l = 0; l < depth; l++)
        posh_pair(&t.empty[8 * l], &t.empty[8 * l], &t.empty[8 * l + 8], pc.data(), half, rounds);
      // 0xA5 in every node never written: a read of one shows in the output
      t.nodes.assign(t.g.off[depth + 1] * 8, 0xA5A5A5A5u);
      if (cmd[0] == 'E') {
        printf("e");
        for (unsigned l = 0; l <= depth; l++) print_fe(&t.empty[8 * l]);
        printf("\n");
      }
    } else if (cmd[0] == 'A') {
      unsigned long long n;
      CHECK(fscanf(fp, "%llu", &n) == 1 && n >= 1 && !t.nodes.empty() && n <= t.capacity - t.next, "A: bad count");
      const uint64_t first = t.next, next = first + n;
      for (uint64_t i = 0; i < n; i++) {
        uint32_t raw[8];
        CHECK(read_fe(fp, raw), "A: bad leaf");
        fr_canon(raw, &t.nodes[(t.g.off[0] + first + i) * 8]);
      }
      for (uint32_t l = 1; l <= t.g.depth; l++) {
        uint64_t lo, cnt;
        nt_touched(first, n, l, &lo, &cnt);
        CHECK(lo + cnt <= nt_level_nodes(t.capacity, l), "A: level %u range past its %llu nodes", l,
              (unsigned long long)nt_level_nodes(t.capacity, l));
        for (uint64_t p = lo; p < lo + cnt; p++)
          nt_rehash(t.nodes.data(), t.empty.data(), t.g, l, p, next, pc.data(), half, rounds);
      }
      t.next = next;
      printf("a %llu", (unsigned long long)first);
      for (uint64_t k = first; k < next; k++) {
        uint32_t r[8];
        nt_root_after(t.nodes.data(), t.empty.data(), t.g, k, r, pc.data(), half, rounds);
        print_fe(r);
      }
      print_fe(&t.nodes[t.g.off[t.g.depth] * 8]);
      printf("\n");
    } else if (cmd[0] == 'P') {
      for (uint64_t pos = 0; pos < t.next; pos++) {
        printf("p %llu", (unsigned long long)pos);
        print_fe(&t.nodes[(t.g.off[0] + pos) * 8]);
        for (uint32_t l = 0; l < t.g.depth; l++) print_fe(nt_sibling(t.nodes.data(), t.empty.data(), t.g, l, pos, t.next));
        printf("\n");
      }
    } else if (cmd[0] == 'B') {
      unsigned long long count;
      unsigned arity;
      CHECK(fscanf(fp, "%llu %u", &count, &arity) == 2 && count && arity >= 1 && arity <= 4, "B: bad arguments");
      uint32_t in[32], out[8];
      for (int i = 0; i < 32; i++) in[i] = 0x01234567u * (i + 1);
      const auto t0 = std::chrono::steady_clock::now();
      for (unsigned long long i = 0; i < count; i++) {
        posh_sponge(in, arity, out, pc.data(), half, rounds);
        memcpy(in, out, 32);  // each hash feeds the next: nothing to hoist
      }
      const double s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      printf("b %.1f", count / s);
      print_fe(out);
      printf("\n");
    } else {
      CHECK(false, "unknown command %s", cmd);
    }
  }
  fclose(fp);
  printf("ok\n");
  return 0;
}
