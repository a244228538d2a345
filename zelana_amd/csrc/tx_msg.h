// tx_msg.h — the messages the sequencer's transparent path signs, built from a
// transaction's fields.  The reference makes them in
// core/src/sequencer/execution/tx_router.rs:624-666 and 774-779;
// zelana_amd/ed25519.py (transfer_message, withdraw_message, legacy_*) is the
// model, and every builder here agrees with it on every byte.  Host+device
// like ed25519.h and note_crypt.h: the kernels of tx_auth.hip, the device
// probe (tests/device/tx_msg_probe.hip) and the stand-alone host check
// (tests/host/tx_msg_check.cpp) compile the very same functions.  Plain C++,
// no HIP call, no inline assembly.
//
// A 32-byte id crosses this header as 8 little-endian u32 words, as byte
// strings do in ed25519.h.  A builder writes its bytes in order into a sink,
// anything with put(uint8_t), and returns the message length; two sinks are
// given below.  Nothing indexes memory by a data-dependent value: decimal
// digits come from divisions by fixed powers of ten, most significant first,
// and base58 from a fixed 44 rounds of division by 58 whose digits are kept in
// words picked by static indices, the digit count decided afterwards.  A lane
// of a kernel therefore keeps all of it in registers.
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

// ------------------------------------------------------------------- lengths
constexpr uint32_t tx_strlen(const char* s) { return *s ? 1u + tx_strlen(s + 1) : 0u; }
#define TX_T_HEAD "Zelana L2 Transfer\n\nFrom: "
#define TX_T_TO "\nTo: "
#define TX_W_HEAD "Zelana L2 Withdrawal\n\nFrom: "
#define TX_W_TO "\nTo L1: "
#define TX_AMOUNT "\nAmount: "
#define TX_NONCE " lamports\nNonce: "
#define TX_T_CHAIN "\nChain ID: "
#define TX_T_TAIL "\n\nSign to authorize this L2 transfer."
#define TX_W_TAIL "\n\nSign to authorize this withdrawal to Solana L1."
constexpr uint32_t TX_HEX_ID = 64;                     // a 32-byte id in hex
constexpr uint32_t TX_DEC_MIN = 1, TX_DEC_MAX = 20;    // a u64 in decimal: "0" .. "18446744073709551615"
// base58 of 32 bytes: a leading zero byte is one '1', and 32 - z bytes whose
// first is not zero take at least as many digits; 2^256 - 1 < 58^44
constexpr uint32_t TX_B58_MIN = 32, TX_B58_MAX = 44;
constexpr uint32_t TX_TRANSFER_FIXED = tx_strlen(TX_T_HEAD) + TX_HEX_ID + tx_strlen(TX_T_TO) + TX_HEX_ID +
                                       tx_strlen(TX_AMOUNT) + tx_strlen(TX_NONCE) + tx_strlen(TX_T_CHAIN) +
                                       tx_strlen(TX_T_TAIL);
constexpr uint32_t TX_WITHDRAW_FIXED = tx_strlen(TX_W_HEAD) + TX_HEX_ID + tx_strlen(TX_W_TO) + tx_strlen(TX_AMOUNT) +
                                       tx_strlen(TX_NONCE) + tx_strlen(TX_W_TAIL);
constexpr uint32_t TX_TRANSFER_MIN = TX_TRANSFER_FIXED + 3 * TX_DEC_MIN, TX_TRANSFER_MAX = TX_TRANSFER_FIXED + 3 * TX_DEC_MAX;
constexpr uint32_t TX_WITHDRAW_MIN = TX_WITHDRAW_FIXED + TX_B58_MIN + 2 * TX_DEC_MIN;
constexpr uint32_t TX_WITHDRAW_MAX = TX_WITHDRAW_FIXED + TX_B58_MAX + 2 * TX_DEC_MAX;
constexpr uint32_t TX_LEGACY_TRANSFER = 88, TX_LEGACY_WITHDRAW = 80;
constexpr uint32_t TX_MSG_MAX = TX_TRANSFER_MAX > TX_WITHDRAW_MAX ? TX_TRANSFER_MAX : TX_WITHDRAW_MAX;
static_assert(TX_TRANSFER_MIN == 236 && TX_TRANSFER_MAX == 293, "a readable transfer is 236 .. 293 bytes");
static_assert(TX_WITHDRAW_MIN == 209 && TX_WITHDRAW_MAX == 259, "a readable withdrawal is 209 .. 259 bytes");
// A message's slot in a kernel's workspace: whole 16-byte pieces, the longest
// message and the zeros that fill its last piece included.
constexpr uint32_t TX_MSG_STRIDE = 304;
static_assert(TX_MSG_STRIDE % 16 == 0 && TX_MSG_STRIDE >= (TX_MSG_MAX + 15) / 16 * 16, "a slot holds the longest message");

// --------------------------------------------------------------------- sinks
// bytes one after another into memory
struct TxByteSink {
  uint8_t* p;
  uint32_t n = 0;
  ZK_HD void put(uint8_t b) { p[n++] = b; }
  ZK_HD void finish() {}
};
// The same bytes gathered in four words and stored 16 at a time: a lane of a
// kernel writes whole 16-byte pieces of its slot, never single bytes.  The
// words are a shift register (a byte enters at the top, sixteen bytes later it
// is byte 0), so no word is picked by the byte count.  finish() fills the last
// piece with zeros; q must have room for the length rounded up to 16.
struct TxQuadSink {
  uint32_t* q;  // 16-byte aligned
  uint32_t n = 0;
  uint32_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
  ZK_HD void put(uint8_t b) {
    a0 = (a0 >> 8) | (a1 << 24), a1 = (a1 >> 8) | (a2 << 24), a2 = (a2 >> 8) | (a3 << 24);
    a3 = (a3 >> 8) | ((uint32_t)b << 24);
    if ((++n & 15) == 0) {
      uint32_t* d = q + (n / 4 - 4);
#if defined(__HIP_DEVICE_COMPILE__)
      *reinterpret_cast<uint4*>(d) = make_uint4(a0, a1, a2, a3);
#else
      d[0] = a0, d[1] = a1, d[2] = a2, d[3] = a3;
#endif
    }
  }
  ZK_HD void finish() {
    const uint32_t len = n;
    while (n & 15) put(0);
    n = len;
  }
};

// -------------------------------------------------------------------- pieces
template <class Sink, uint32_t N>
ZK_HD void tx_put_text(Sink& s, const char (&text)[N]) {
#pragma unroll
  for (uint32_t i = 0; i + 1 < N; i++) s.put((uint8_t)text[i]);
}
#define TX_PUT(sink, literal) tx_put_text(sink, literal)
// 32 bytes, given as 8 little-endian words, in lower-case hex
template <class Sink>
ZK_HD void tx_put_hex(Sink& s, const uint32_t* id) {
#pragma unroll
  for (int i = 0; i < 32; i++) {
    const uint32_t b = (id[i >> 2] >> (8 * (i & 3))) & 255u;
    const uint32_t hi = b >> 4, lo = b & 15u;
    s.put((uint8_t)(hi < 10 ? '0' + hi : 'a' + hi - 10));
    s.put((uint8_t)(lo < 10 ? '0' + lo : 'a' + lo - 10));
  }
}
ZK_HD uint64_t tx_pow10(int k) {
  uint64_t p = 1;
  for (int i = 0; i < k; i++) p *= 10;
  return p;
}
// a u64 in decimal without leading zeros: twenty divisions by constants
template <class Sink>
ZK_HD void tx_put_dec(Sink& s, uint64_t v) {
  bool started = false;
#pragma unroll
  for (int k = 19; k >= 0; k--) {
    const uint64_t p = tx_pow10(k);
    const uint32_t d = (uint32_t)(v / p);
    v -= d * p;
    started = started || d != 0 || k == 0;
    if (started) s.put((uint8_t)('0' + d));
  }
}
// digit 0 .. 57 -> its character in the Bitcoin alphabet (no 0, I, O, l)
ZK_HD uint8_t tx_b58_char(uint32_t d) {
  return (uint8_t)(d < 9 ? '1' + d : d < 17 ? 'A' + (d - 9) : d < 22 ? 'J' + (d - 17) : d < 33 ? 'P' + (d - 22)
                   : d < 44 ? 'a' + (d - 33) : 'm' + (d - 44));
}
// 32 bytes in base58 (bs58's default alphabet): the bytes are one big-endian
// integer; each leading zero byte becomes a '1', then the integer's digits
// follow, none for zero.  -> the characters written, 32 .. 44.
template <class Sink>
ZK_HD uint32_t tx_put_base58(Sink& s, const uint32_t* id) {
  uint32_t x[8];  // the integer, most significant word first
  uint32_t zeros = 0;
  bool lead = true;
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const uint32_t w = id[j];
    x[j] = (w >> 24) | ((w >> 8) & 0xFF00u) | ((w << 8) & 0xFF0000u) | (w << 24);
#pragma unroll
    for (int b = 0; b < 4; b++) {
      lead = lead && ((w >> (8 * b)) & 255u) == 0;
      zeros += lead ? 1u : 0u;
    }
  }
  // 44 rounds of x, r = divmod(x, 58): round i leaves digit i, the least
  // significant first.  Four digits a word; a finished word is pushed in at
  // g[0], so digit i ends in byte i % 4 of g[10 - i / 4].
  uint32_t g[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
  for (int round = 0; round < 11; round++) {
    uint32_t four = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      uint32_t rem = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint64_t cur = ((uint64_t)rem << 32) | x[j];
        const uint64_t quo = cur / 58u;
        x[j] = (uint32_t)quo;
        rem = (uint32_t)(cur - quo * 58u);
      }
      four |= rem << (8 * t);
    }
#pragma unroll
    for (int k = 10; k > 0; k--) g[k] = g[k - 1];
    g[0] = four;
  }
  uint32_t digits = 0;  // one past the highest digit that is not zero
#pragma unroll
  for (int i = 0; i < 44; i++) digits = ((g[10 - i / 4] >> (8 * (i % 4))) & 255u) ? (uint32_t)(i + 1) : digits;
#pragma unroll 1
  for (uint32_t i = 0; i < zeros; i++) s.put((uint8_t)'1');
#pragma unroll
  for (int i = 43; i >= 0; i--)
    if ((uint32_t)i < digits) s.put(tx_b58_char((g[10 - i / 4] >> (8 * (i % 4))) & 255u));
  return zeros + digits;
}
template <class Sink>
ZK_HD void tx_put_le32(Sink& s, const uint32_t* id) {
#pragma unroll
  for (int i = 0; i < 32; i++) s.put((uint8_t)(id[i >> 2] >> (8 * (i & 3))));
}
template <class Sink>
ZK_HD void tx_put_le64(Sink& s, uint64_t v) {
#pragma unroll
  for (int i = 0; i < 8; i++) s.put((uint8_t)(v >> (8 * i)));
}

// ------------------------------------------------------------------ messages
// tx_router.rs:624-645 build_transfer_message, byte for byte: both blank lines,
// no trailing newline.  -> the length, TX_TRANSFER_MIN .. TX_TRANSFER_MAX
template <class Sink>
ZK_HD uint32_t tx_transfer_message(Sink& s, const uint32_t* from, const uint32_t* to, uint64_t amount, uint64_t nonce,
                                   uint64_t chain_id) {
  TX_PUT(s, TX_T_HEAD);
  tx_put_hex(s, from);
  TX_PUT(s, TX_T_TO);
  tx_put_hex(s, to);
  TX_PUT(s, TX_AMOUNT);
  tx_put_dec(s, amount);
  TX_PUT(s, TX_NONCE);
  tx_put_dec(s, nonce);
  TX_PUT(s, TX_T_CHAIN);
  tx_put_dec(s, chain_id);
  TX_PUT(s, TX_T_TAIL);
  s.finish();
  return s.n;
}
// tx_router.rs:648-666 build_withdraw_message: `from` in hex, the L1 address
// in base58.  -> the length, TX_WITHDRAW_MIN .. TX_WITHDRAW_MAX
template <class Sink>
ZK_HD uint32_t tx_withdraw_message(Sink& s, const uint32_t* from, const uint32_t* to_l1, uint64_t amount, uint64_t nonce) {
  TX_PUT(s, TX_W_HEAD);
  tx_put_hex(s, from);
  TX_PUT(s, TX_W_TO);
  tx_put_base58(s, to_l1);
  TX_PUT(s, TX_AMOUNT);
  tx_put_dec(s, amount);
  TX_PUT(s, TX_NONCE);
  tx_put_dec(s, nonce);
  TX_PUT(s, TX_W_TAIL);
  s.finish();
  return s.n;
}
// The reference's fallback for a transfer, wincode::serialize(&tx.data).
// ASSUMPTION: the wincode crate's source was not at hand; its
// layout of TransactionData is taken to be the fields in declaration order,
// ids raw and integers as fixed-width little-endian u64:
// from || to || amount || nonce || chain_id, 88 bytes.
template <class Sink>
ZK_HD uint32_t tx_legacy_transfer_message(Sink& s, const uint32_t* from, const uint32_t* to, uint64_t amount,
                                          uint64_t nonce, uint64_t chain_id) {
  tx_put_le32(s, from);
  tx_put_le32(s, to);
  tx_put_le64(s, amount);
  tx_put_le64(s, nonce);
  tx_put_le64(s, chain_id);
  s.finish();
  return s.n;
}
// tx_router.rs:774-779: from || to_l1 || amount le64 || nonce le64, 80 bytes,
// under the same assumption of fixed-width little-endian integers
template <class Sink>
ZK_HD uint32_t tx_legacy_withdraw_message(Sink& s, const uint32_t* from, const uint32_t* to_l1, uint64_t amount,
                                          uint64_t nonce) {
  tx_put_le32(s, from);
  tx_put_le32(s, to_l1);
  tx_put_le64(s, amount);
  tx_put_le64(s, nonce);
  s.finish();
  return s.n;
}

// A transaction's fields as they lie in a zkmi_signed_tx (zkmi.h), in words:
// from 0, to 8, amount 16, nonce 18, chain_id 20, signer_pubkey 22,
// signature 30, kind in the low byte of word 46; 48 words a record.
constexpr uint32_t TX_REC_WORDS = 48, TX_REC_SIGNER = 22, TX_REC_SIG = 30, TX_REC_KIND = 46;
constexpr uint32_t TX_KIND_TRANSFER = 0, TX_KIND_WITHDRAWAL = 1;
ZK_HD uint64_t tx_rec_u64(const uint32_t* rec, int word) { return rec[word] | ((uint64_t)rec[word + 1] << 32); }
// the readable (legacy = false) or the legacy message of the record
template <class Sink>
ZK_HD uint32_t tx_record_message(Sink& s, const uint32_t* rec, bool legacy) {
  const uint64_t amount = tx_rec_u64(rec, 16), nonce = tx_rec_u64(rec, 18), chain_id = tx_rec_u64(rec, 20);
  const bool withdrawal = (rec[TX_REC_KIND] & 255u) == TX_KIND_WITHDRAWAL;
  if (legacy)
    return withdrawal ? tx_legacy_withdraw_message(s, rec, rec + 8, amount, nonce)
                      : tx_legacy_transfer_message(s, rec, rec + 8, amount, nonce, chain_id);
  return withdrawal ? tx_withdraw_message(s, rec, rec + 8, amount, nonce)
                    : tx_transfer_message(s, rec, rec + 8, amount, nonce, chain_id);
}

}  // namespace zk
