// ed25519_ops.h — an op table over zelana_amd/csrc/ed25519.h, one call per op,
// compiled twice: for the host by tests/host/ed25519_check.cpp and for the
// device by tests/device/ed25519_probe.hip.  A case is an op code and ED_IN
// input words; it leaves up to ED_OUT output words.  Nothing here knows an
// expected value: tests/ed25519_cases.py holds the outputs against Python
// integers, hashlib and the model (zelana_amd/ed25519.py).
#pragma once
#include "../../zelana_amd/csrc/ed25519.h"

namespace edops {

using namespace zk;

constexpr int ED_IN = 112, ED_OUT = 24;
enum {
  OP_SHA512 = 1,       // len msg[..] -> digest[16]
  OP_SC_REDUCE = 2,    // x[16] -> r[8]
  OP_SC_CANONICAL = 3, // s[8] -> 0 / 1
  OP_DECOMPRESS = 4,   // bytes[8] -> ok, then x[8] y[8] (canonical bytes; Z is 1) and T - x y == 0
  OP_ADD = 5,          // P[8] Q[8] (compressed) -> compress(P + Q)[8], through ed_add
  OP_DBL = 6,          // P[8] -> compress(2 P)[8], through ed_dbl
  OP_COMPRESS = 7,     // X[10] Y[10] Z[10] raw limbs -> bytes[8]
  OP_VERIFY_CORE = 8,  // R[8] A[8] k[8] s[8] -> 1 holds, 0 does not, 2 A does not decompress
  OP_VERIFY = 9,       // pk[8] sig[16] len msg[..] -> SIG_*
  OP_SCALAR_MUL = 10,  // s[8] k[8] Q[8] -> compress([s]B + [k]Q)[8]
  OP_LAST = 10
};
// where an op's length word lies, or -1: the message follows it and ends the input
ZK_HD int ed_len_at(uint32_t op) { return op == OP_SHA512 ? 0 : op == OP_VERIFY ? 24 : -1; }

ZK_HD Fe25 limbs(const uint32_t* w) {
  Fe25 a;
  for (int i = 0; i < 10; i++) a.v[i] = w[i];
  return a;
}

// -> words written to out, or -1 for an unknown op, a length that does not fit
// or a point that does not decompress where the op needs one
ZK_HD int ed_apply(uint32_t op, const uint32_t* in, uint32_t* out) {
  switch (op) {
    case OP_SHA512: {
      if (in[0] > 4u * (ED_IN - 1)) return -1;
      sha512(out, in[0], WordBytes{in + 1});
      return 16;
    }
    case OP_SC_REDUCE: sc_reduce512(out, in); return 8;
    case OP_SC_CANONICAL: out[0] = sc_is_canonical(in) ? 1 : 0; return 1;
    case OP_DECOMPRESS: {
      EdPoint p;
      out[0] = ed_decompress(p, in) ? 1 : 0;
      if (!out[0]) return 1;
      fe25_store(out + 1, p.X);
      fe25_store(out + 9, p.Y);
      out[17] = fe25_is_zero(fe25_sub(fe25_mul(p.T, p.Z), fe25_mul(p.X, p.Y))) ? 1 : 0;
      return 18;
    }
    case OP_ADD: {
      EdPoint p, q;
      if (!ed_decompress(p, in) || !ed_decompress(q, in + 8)) return -1;
      ed_compress(out, ed_add(p, ed_to_cached(q)));
      return 8;
    }
    case OP_DBL: {
      EdPoint p;
      if (!ed_decompress(p, in)) return -1;
      ed_compress(out, ed_dbl(p));
      return 8;
    }
    case OP_COMPRESS: {
      EdPoint p;
      p.X = limbs(in), p.Y = limbs(in + 10), p.Z = limbs(in + 20), p.T = fe25_zero();
      ed_compress(out, p);
      return 8;
    }
    case OP_VERIFY_CORE: out[0] = ed_verify_core(in, in + 8, in + 16, in + 24); return 1;
    case OP_VERIFY: {
      if (in[24] > 4u * (ED_IN - 25)) return -1;
      out[0] = ed_verify(in, in + 8, in[24], WordBytes{in + 25});
      return 1;
    }
    case OP_SCALAR_MUL: {
      EdPoint q;
      if (!ed_decompress(q, in + 16)) return -1;
      EdCached tb[ED_TABLE], tq[ED_TABLE];
      ed_build_table(ed_base(), EdTableArray{tb});
      ed_build_table(q, EdTableArray{tq});
      ed_compress(out, ed_double_scalar_mul(in, in + 8, EdTableArray{tb}, EdTableArray{tq}));
      return 8;
    }
  }
  return -1;
}

}  // namespace edops
