// proof_decode_check — the device header's proof decoder
// (zelana_amd/csrc/proof_decode.h, compiled for the host) against verify.cpp's
// (proof_decode_words, what zkmi_proof_decode runs).
//
//   proof_decode_check CASES
// CASES: text, "ncases" then per case "fmt expect hex": an encoded proof of
// format fmt (ZKMI_PROOF_*) and whether it is well-formed (0) or malformed (1).
// 1. per case: both decoders say `expect`, and on 0 give the same words.
// 2. per format, a seeded loop of 4096 random byte strings and 4096 more with
//    the flag bytes shaped so that a good share decodes: both decoders agree
//    on malformed / well-formed and on every word; an accepted compressed
//    string re-serializes to itself.
// Prints "ok <cases> <strings per format> <accepted per format x 4>".
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../zelana_amd/csrc/proof_decode.h"
#include "../../zelana_amd/csrc/verify_internal.h"

namespace zk {
void set_error(const char*, ...) {}
void g1_compress(const uint64_t p[8], uint8_t out[32]);
void g2_compress(const uint64_t p[16], uint8_t out[64]);
}  // namespace zk

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      fprintf(stderr, __VA_ARGS__); \
      fprintf(stderr, "\n");        \
      return 1;                     \
    }                               \
  } while (0)

// the header's decoder on one encoded proof: 0, or 1 = malformed
static int dev_decode(int fmt, const uint8_t* in, uint64_t a[8], uint64_t b[16], uint64_t c[8]) {
  uint32_t w[64], oa[16], ob[32], oc[16];
  memcpy(w, in, zk::proof_encoded_len(fmt));
  bool ok;
  switch (fmt) {
    case zk::PROOF_ARK_COMPRESSED:
      ok = zk::pd_g1_compressed(w, oa) && zk::pd_g2_compressed(w + 8, ob) && zk::pd_g1_compressed(w + 24, oc);
      break;
    case zk::PROOF_ARK_UNCOMPRESSED:
      ok = zk::pd_fixed<zk::PROOF_ARK_UNCOMPRESSED>(w, oa, ob, oc);
      break;
    case zk::PROOF_SOLANA_LE:
      ok = zk::pd_fixed<zk::PROOF_SOLANA_LE>(w, oa, ob, oc);
      break;
    default:
      ok = zk::pd_fixed<zk::PROOF_ALT_BN128_BE>(w, oa, ob, oc);
  }
  if (!ok) return 1;
  memcpy(a, oa, 64);
  memcpy(b, ob, 128);
  memcpy(c, oc, 64);
  return 0;
}

// both decoders on one string: -1 on a disagreement, else 0 / 1
static int both(int fmt, const uint8_t* in, const char* what, long idx) {
  uint64_t a[8], b[16], c[8], da[8], db[16], dc[8];
  const int h = zkv::proof_decode_words(fmt, in, a, b, c), d = dev_decode(fmt, in, da, db, dc);
  if (h != d) {
    fprintf(stderr, "%s %ld, format %d: host decoder says %d, the header %d\n", what, idx, fmt, h, d);
    return -1;
  }
  if (h) return 1;
  if (memcmp(a, da, 64) || memcmp(b, db, 128) || memcmp(c, dc, 64)) {
    fprintf(stderr, "%s %ld, format %d: decoded words differ\n", what, idx, fmt);
    return -1;
  }
  if (fmt == zk::PROOF_ARK_COMPRESSED) {
    uint8_t re[128];
    zk::g1_compress(a, re);
    zk::g2_compress(b, re + 32);
    zk::g1_compress(c, re + 96);
    if (memcmp(re, in, 128)) {
      fprintf(stderr, "%s %ld: an accepted compressed string does not re-serialize to itself\n", what, idx);
      return -1;
    }
  }
  return 0;
}

int main(int argc, char** argv) {
  CHECK(argc > 1, "usage: proof_decode_check CASES");
  FILE* fp = fopen(argv[1], "r");
  CHECK(fp, "cannot open %s", argv[1]);
  int ncases = 0;
  CHECK(fscanf(fp, "%d", &ncases) == 1, "bad case file");
  for (int cs = 0; cs < ncases; cs++) {
    int fmt = 0, expect = 0;
    char hex[520];
    CHECK(fscanf(fp, "%d %d %519s", &fmt, &expect, hex) == 3, "bad case %d", cs);
    const size_t len = zk::proof_encoded_len(fmt);
    CHECK(len && strlen(hex) == 2 * len, "case %d: %zu hex digits for format %d", cs, strlen(hex), fmt);
    uint8_t in[256];
    for (size_t i = 0; i < len; i++) {
      unsigned v;
      CHECK(sscanf(hex + 2 * i, "%2x", &v) == 1, "case %d: bad hex", cs);
      in[i] = (uint8_t)v;
    }
    const int got = both(fmt, in, "case", cs);
    CHECK(got >= 0, "case %d failed", cs);
    CHECK(got == expect, "case %d (format %d): decoders say %d, expected %d", cs, fmt, got, expect);
  }
  fclose(fp);
  const int NR = 4096;
  long accepted[4] = {0, 0, 0, 0};
  for (int fmt = 0; fmt < 4; fmt++) {
    const size_t len = zk::proof_encoded_len(fmt);
    for (int t = 0; t < 2 * NR; t++) {
      uint8_t in[256];
      for (size_t i = 0; i < len; i += 8) {
        const uint64_t v = rnd();
        memcpy(in + i, &v, 8);
      }
      if (t >= NR) {
        // shaped: each 32-byte field's most significant byte below 0x40 most of
        // the time (the value then < q with probability 3/4), and SWFlags
        // drawn into the flag positions of the two arkworks formats
        for (size_t f = 0; f < len / 32; f++) {
          const size_t top = fmt == zk::PROOF_ALT_BN128_BE ? 32 * f : 32 * f + 31;
          if (rnd() & 7) in[top] &= 0x3F;
          const bool flag_pos = fmt == zk::PROOF_ARK_COMPRESSED ? (f != 1)
                                : fmt == zk::PROOF_ARK_UNCOMPRESSED ? (f == 1 || f == 5 || f == 7)
                                                                    : false;
          if (!flag_pos) continue;
          const uint64_t r = rnd();
          if ((r & 3) == 0) in[top] |= 0x80;
          if ((r & 60) == 0) {  // 1 in 16: the infinity flag, mostly on an all-zero point
            const size_t p0 = fmt == zk::PROOF_ARK_COMPRESSED ? (f == 0 ? 0 : f == 2 ? 32 : 96)
                                                              : (f == 1 ? 0 : f == 5 ? 64 : 192);
            if (r & 192) memset(in + p0, 0, 32 * f + 32 - p0);
            in[top] |= 0x40;
            if ((r & 0x300) == 0) in[p0 + (r >> 10) % (32 * f + 32 - p0)] |= 1 << ((r >> 20) & 7);  // a stray bit
          }
        }
      }
      const int got = both(fmt, in, "random string", t);
      CHECK(got >= 0, "random string %d of format %d failed", t, fmt);
      accepted[fmt] += got == 0;
    }
  }
  printf("ok %d %d %ld %ld %ld %ld\n", ncases, 2 * NR, accepted[0], accepted[1], accepted[2], accepted[3]);
  return 0;
}
