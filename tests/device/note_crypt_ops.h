// note_crypt_ops.h — an op table over zelana_amd/csrc/note_crypt.h, one call
// per op, compiled twice: for the host by tests/host/note_crypt_check.cpp and
// for the device by tests/device/note_crypt_probe.hip.  A case is an op code
// and NC_IN input words; it leaves up to NC_OUT output words.  Nothing here
// knows an expected value: tests/note_crypt_cases.py holds the outputs against
// Python integers and the model (zelana_amd/note_crypt.py).
#pragma once
#include "../../zelana_amd/csrc/note_crypt.h"

namespace ncops {

using namespace zk;

constexpr int NC_IN = 176, NC_OUT = 160;
enum {
  OP_FE_ADD = 1,      // a[10] b[10] -> r[10]          raw limbs in, raw limbs out
  OP_FE_SUB = 2,
  OP_FE_MUL = 3,
  OP_FE_SQR = 4,      // a[10] -> r[10]
  OP_FE_M121665 = 5,
  OP_FE_CSWAP = 6,    // a[10] b[10] bit -> a'[10] b'[10]
  OP_FE_INVERT = 7,
  OP_FE_LOAD = 8,     // bytes as 8 words -> r[10]
  OP_FE_STORE = 9,    // a[10] -> 8 words
  OP_X25519 = 10,     // scalar[8] u[8] -> out[8]
  OP_NOTE_KEY = 11,   // ctx_key[8] shared[8] epk[8] -> key[8]
  OP_CHACHA = 12,     // key[8] counter nonce[3] -> block[16]
  OP_POLY_MAC = 13,   // key[8] len msg[..] -> tag[4]
  OP_AEAD_PLAIN = 14, // key[8] nonce[3] len ct[..] -> ok, then the body's plaintext words when ok
  OP_AEAD_NOTE = 15,  // key[8] nonce[3] len ct[..] -> ok parsed value[2] randomness[8] memo_len memo[..]
  OP_LAST = 15
};

ZK_HD Fe25 limbs(const uint32_t* w) {
  Fe25 a;
  for (int i = 0; i < 10; i++) a.v[i] = w[i];
  return a;
}
ZK_HD void put(uint32_t* w, const Fe25& a) {
  for (int i = 0; i < 10; i++) w[i] = a.v[i];
}

// -> words written to out, or -1 for an unknown op or a length that does not fit
ZK_HD int nc_apply(uint32_t op, const uint32_t* in, uint32_t* out) {
  switch (op) {
    case OP_FE_ADD: put(out, fe25_add(limbs(in), limbs(in + 10))); return 10;
    case OP_FE_SUB: put(out, fe25_sub(limbs(in), limbs(in + 10))); return 10;
    case OP_FE_MUL: put(out, fe25_mul(limbs(in), limbs(in + 10))); return 10;
    case OP_FE_SQR: put(out, fe25_sqr(limbs(in))); return 10;
    case OP_FE_M121665: put(out, fe25_mul121665(limbs(in))); return 10;
    case OP_FE_CSWAP: {
      Fe25 a = limbs(in), b = limbs(in + 10);
      fe25_cswap(a, b, in[20] & 1);
      put(out, a);
      put(out + 10, b);
      return 20;
    }
    case OP_FE_INVERT: put(out, fe25_invert(limbs(in))); return 10;
    case OP_FE_LOAD: put(out, fe25_load(in)); return 10;
    case OP_FE_STORE: fe25_store(out, limbs(in)); return 8;
    case OP_X25519: x25519(out, in, in + 8); return 8;
    case OP_NOTE_KEY: note_key(out, in, in + 8, in + 16); return 8;
    case OP_CHACHA: chacha20_block(out, in, in[8], in + 9); return 16;
    case OP_POLY_MAC: {
      if (in[8] > 4u * (NC_IN - 9)) return -1;
      poly1305_mac(out, in, in + 9, in[8]);
      return 4;
    }
    case OP_AEAD_PLAIN:
    case OP_AEAD_NOTE: {
      const uint32_t len = in[11];
      const uint32_t* ct = in + 12;
      if (len > 4u * (NC_IN - 12)) return -1;
      out[0] = aead_tag_ok(in, in + 8, ct, len) ? 1 : 0;
      if (!out[0]) return 1;
      const uint32_t body = len - AEAD_TAG;
      if (op == OP_AEAD_PLAIN) {
        const uint32_t nw = (body + 3) / 4;
        for (uint32_t b = 0; 16 * b < nw; b++) {
          uint32_t pt[16];
          aead_plain_block(pt, in, in + 8, ct, body, b);
          for (uint32_t i = 0; i < 16; i++)
            if (16 * b + i < nw) out[1 + 16 * b + i] = pt[i];
        }
        return 1 + (int)nw;
      }
      uint32_t pt[16];
      aead_plain_block(pt, in, in + 8, ct, body, 0);
      NoteHead h;
      out[1] = note_parse(pt, body, h) ? 1 : 0;
      if (!out[1]) return 2;
      out[2] = h.value[0], out[3] = h.value[1];
      for (int i = 0; i < 8; i++) out[4 + i] = h.randomness[i];
      out[12] = h.memo_len;
      note_memo(out + 13, in, in + 8, ct, body, h.memo_len);
      return 13 + (int)note_memo_words(h.memo_len);
    }
  }
  return -1;
}

}  // namespace ncops
