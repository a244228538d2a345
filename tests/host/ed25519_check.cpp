// ed25519_check — the device header of Ed25519 verification
// (zelana_amd/csrc/ed25519.h) compiled for the host, alone, behind the op
// table of tests/device/ed25519_ops.h.
//
//   ed25519_check [SCRIPT]          (the script is read from stdin when no file is named)
// SCRIPT: one case a line, "<op> <hex>": the op code (decimal) and the input
// words as the hex of their little-endian bytes (a multiple of 8 digits, at
// most ED_IN words; the rest of the input is zero).
//   -> "<hex>" the output words of the case, one line per case, then "ok"
// A line that does not parse, an unknown op, a length that does not fit or a
// point that does not decompress where the op needs one ends the run with
// status 1.  Nothing here knows an expected value: tests/test_ed25519_cpu.py
// holds the output against Python integers, hashlib and the model.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../device/ed25519_ops.h"

using namespace edops;

static int hexval(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

int main(int argc, char** argv) {
  FILE* fp = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!fp) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 1;
  }
  std::vector<char> line(16 + 8 * ED_IN + 8);
  std::vector<uint32_t> in(ED_IN), out(ED_OUT);
  while (fgets(line.data(), (int)line.size(), fp)) {
    char* p = line.data();
    size_t n = strlen(p);
    if (n && p[n - 1] != '\n' && !feof(fp)) {
      fprintf(stderr, "a line is too long\n");
      return 1;
    }
    while (n && (p[n - 1] == '\n' || p[n - 1] == '\r' || p[n - 1] == ' ')) p[--n] = 0;
    if (n == 0) continue;
    char* end;
    const unsigned long op = strtoul(p, &end, 10);
    if (end == p || op < 1 || op > OP_LAST) {
      fprintf(stderr, "bad op in '%.20s'\n", p);
      return 1;
    }
    while (*end == ' ') end++;
    const size_t digits = strlen(end);
    if (digits % 8 || digits / 8 > (size_t)ED_IN) {
      fprintf(stderr, "op %lu: %zu hex digits (whole words, at most %d)\n", op, digits, ED_IN);
      return 1;
    }
    std::fill(in.begin(), in.end(), 0u);
    for (size_t i = 0; i < digits / 2; i++) {
      const int hi = hexval(end[2 * i]), lo = hexval(end[2 * i + 1]);
      if (hi < 0 || lo < 0) {
        fprintf(stderr, "op %lu: not hex\n", op);
        return 1;
      }
      in[i / 4] |= (uint32_t)(hi * 16 + lo) << (8 * (i % 4));
    }
    // the message of a case sits in a buffer of exactly its own size, so a
    // read past its last word is a read past an allocation
    int nout;
    const int len_at = ed_len_at((uint32_t)op);
    if (len_at >= 0) {
      const size_t head = (size_t)len_at + 1;
      const uint32_t len = in[len_at];
      if (len > 4u * (ED_IN - head)) {
        fprintf(stderr, "op %lu: length %u does not fit\n", op, len);
        return 1;
      }
      std::vector<uint32_t> exact(in.begin(), in.begin() + head + (len + 3) / 4);
      nout = ed_apply((uint32_t)op, exact.data(), out.data());
    } else {
      nout = ed_apply((uint32_t)op, in.data(), out.data());
    }
    if (nout < 0) {
      fprintf(stderr, "op %lu failed\n", op);
      return 1;
    }
    for (int i = 0; i < nout; i++)
      printf("%02x%02x%02x%02x", out[i] & 255, (out[i] >> 8) & 255, (out[i] >> 16) & 255, out[i] >> 24);
    printf("\n");
  }
  if (fp != stdin) fclose(fp);
  printf("ok\n");
  return 0;
}
