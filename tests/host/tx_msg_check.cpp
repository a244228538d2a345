// tx_msg_check — the message builders of zelana_amd/csrc/tx_msg.h compiled for
// the host, alone.
//
//   tx_msg_check [RECORDS]          (the records are read from stdin when no file is named)
// RECORDS: one record a line, the hex of its 88 bytes
// from || to || amount le64 || nonce le64 || chain_id le64 (the first 88 bytes
// of a zkmi_signed_tx).
//   -> one line per record: the readable transfer, the readable withdrawal,
//      the legacy transfer and the legacy withdrawal message of these fields,
//      in hex, separated by blanks; then
//      "bounds <transfer min> <max> <withdrawal min> <max> <legacy transfer> <legacy withdrawal> <stride>"
//      as the header declares them, then "ok"
// Every message is built twice, through the byte sink into a buffer of exactly
// the declared maximum and through the 16-byte sink into a buffer of exactly
// the slot it is given on the device, and the two must agree: a write past a
// bound is a write past an allocation.  A line that does not parse, a length
// outside the header's bounds or two sinks that differ end the run with status
// 1.  Nothing here knows an expected byte: tests/test_tx_msg_cpu.py holds the
// output against zelana_amd/ed25519.py.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../zelana_amd/csrc/tx_msg.h"

using namespace zk;

static int hexval(char c) {
  if (c >= '0' && c <= '9') return c - '0';
  if (c >= 'a' && c <= 'f') return c - 'a' + 10;
  return -1;
}

// which: 0 readable transfer, 1 readable withdrawal, 2 legacy transfer, 3 legacy withdrawal
template <class Sink>
static uint32_t build(Sink& s, int which, const uint32_t* rec) {
  const uint64_t amount = tx_rec_u64(rec, 16), nonce = tx_rec_u64(rec, 18), chain_id = tx_rec_u64(rec, 20);
  switch (which) {
    case 0: return tx_transfer_message(s, rec, rec + 8, amount, nonce, chain_id);
    case 1: return tx_withdraw_message(s, rec, rec + 8, amount, nonce);
    case 2: return tx_legacy_transfer_message(s, rec, rec + 8, amount, nonce, chain_id);
    default: return tx_legacy_withdraw_message(s, rec, rec + 8, amount, nonce);
  }
}

int main(int argc, char** argv) {
  FILE* fp = argc > 1 ? fopen(argv[1], "r") : stdin;
  if (!fp) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 1;
  }
  const uint32_t lo[4] = {TX_TRANSFER_MIN, TX_WITHDRAW_MIN, TX_LEGACY_TRANSFER, TX_LEGACY_WITHDRAW};
  const uint32_t hi[4] = {TX_TRANSFER_MAX, TX_WITHDRAW_MAX, TX_LEGACY_TRANSFER, TX_LEGACY_WITHDRAW};
  char line[256];
  while (fgets(line, (int)sizeof line, fp)) {
    size_t n = strlen(line);
    if (n && line[n - 1] != '\n' && !feof(fp)) {
      fprintf(stderr, "a line is too long\n");
      return 1;
    }
    while (n && (line[n - 1] == '\n' || line[n - 1] == '\r' || line[n - 1] == ' ')) line[--n] = 0;
    if (n == 0) continue;
    if (n != 176) {
      fprintf(stderr, "%zu hex digits, not 176\n", n);
      return 1;
    }
    uint32_t rec[22] = {0};
    for (size_t i = 0; i < 88; i++) {
      const int h = hexval(line[2 * i]), l = hexval(line[2 * i + 1]);
      if (h < 0 || l < 0) {
        fprintf(stderr, "not hex\n");
        return 1;
      }
      rec[i / 4] |= (uint32_t)(h * 16 + l) << (8 * (i % 4));
    }
    for (int which = 0; which < 4; which++) {
      std::vector<uint8_t> bytes(hi[which]);
      TxByteSink bs{bytes.data()};
      const uint32_t len = build(bs, which, rec);
      std::vector<uint32_t> slot(TX_MSG_STRIDE / 4, 0xA5A5A5A5u);
      TxQuadSink qs{slot.data()};
      const uint32_t len_q = build(qs, which, rec);
      if (len < lo[which] || len > hi[which] || len_q != len) {
        fprintf(stderr, "message %d: length %u (16-byte sink %u), bounds %u .. %u\n", which, len, len_q, lo[which], hi[which]);
        return 1;
      }
      for (uint32_t i = 0; i < (len + 15) / 16 * 16; i++) {
        const uint8_t got = (uint8_t)(slot[i / 4] >> (8 * (i % 4)));
        if (got != (i < len ? bytes[i] : 0)) {
          fprintf(stderr, "message %d: the sinks differ at byte %u\n", which, i);
          return 1;
        }
      }
      for (uint32_t i = 0; i < len; i++) printf("%02x", bytes[i]);
      printf(which < 3 ? " " : "\n");
    }
  }
  if (fp != stdin) fclose(fp);
  printf("bounds %u %u %u %u %u %u %u\n", TX_TRANSFER_MIN, TX_TRANSFER_MAX, TX_WITHDRAW_MIN, TX_WITHDRAW_MAX,
         TX_LEGACY_TRANSFER, TX_LEGACY_WITHDRAW, TX_MSG_STRIDE);
  printf("ok\n");
  return 0;
}
