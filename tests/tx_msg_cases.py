"""Cases for the message builders of zelana_amd/csrc/tx_msg.h, shared by the
host check (test_tx_msg_cpu.py), the device probe and the end-to-end runs
(test_gpu_tx_auth.py).  A case is (name, from, to, amount, nonce, chain_id);
`to` stands for a transfer's `to` and for a withdrawal's to_l1_address alike,
since every case is built into all four messages.  The expected bytes are
zelana_amd/ed25519.py's."""
import hashlib
import struct

from zelana_amd import ed25519 as E

U64_MAX = 2**64 - 1
EDGE_INTS = [0, 9, 10, 99, 100, 10**19 - 1, 10**19, 2**63, U64_MAX]
for _k in (1, 3, 9, 10, 18):
    EDGE_INTS += [10**_k - 1, 10**_k, 10**_k + 1]
EDGE_INTS = sorted(set(EDGE_INTS))
L1_LEADING_ZEROS = [0, 1, 3, 31, 32]


def rnd(tag: str, n: int = 32) -> bytes:
    out, i = b"", 0
    while len(out) < n:
        out += hashlib.sha256(f"tx-msg/{tag}/{i}".encode()).digest()
        i += 1
    return out[:n]


def be32(v: int) -> bytes:
    return v.to_bytes(32, "big")


def l1_addresses():
    """(name, 32 bytes): the base58 edges"""
    out = []
    for z in L1_LEADING_ZEROS:
        tail = rnd(f"l1/{z}", 32 - z)
        if tail and tail[0] == 0:
            tail = b"\x01" + tail[1:]
        out.append((f"{z} leading zero bytes", bytes(z) + tail))
    # one byte after 31 zeros: one digit up to 57, two from 58 on
    out += [(f"31 zeros then 0x{b:02x}", bytes(31) + bytes([b])) for b in (1, 57, 58, 255)]
    out += [("58^43 - 1", be32(58**43 - 1)), ("58^43", be32(58**43)), ("0xff x 32", b"\xff" * 32),
            ("2^248", be32(2**248)), ("2^248 - 1", be32(2**248 - 1)), ("58^10", be32(58**10))]
    return out


def all_cases():
    ids = [("0x00", bytes(32)), ("0xff", b"\xff" * 32), ("0x0f", b"\x0f" * 32), ("0xf0", b"\xf0" * 32),
           ("random", rnd("id/a"))]
    a, b = rnd("id/from"), rnd("id/to")
    cases = []
    for v in EDGE_INTS:
        cases += [(f"amount {v}", a, b, v, 7, 1), (f"nonce {v}", a, b, 5, v, 1), (f"chain_id {v}", a, b, 5, 7, v),
                  (f"all three {v}", a, b, v, v, v)]
    for nf, f in ids:
        for nt, t in ids:
            cases.append((f"from {nf} to {nt}", f, t, 1234567890123, 42, 1))
    for name, l1 in l1_addresses():
        cases.append((f"to_l1 {name}", a, l1, 1000, 3, 1))
    for i in range(24):
        ints = struct.unpack("<QQQ", rnd(f"rec/ints/{i}", 24))
        # spread the digit counts: a random u64 has 19 or 20 digits nearly always
        ints = tuple(v >> (rnd(f"rec/shift/{i}", 3)[k] % 64) for k, v in enumerate(ints))
        cases.append((f"random record {i}", rnd(f"rec/from/{i}"), rnd(f"rec/to/{i}"), *ints))
    cases += [("shortest of each kind", bytes(32), bytes(32), 0, 0, 0),
              ("longest of each kind", b"\xff" * 32, b"\xff" * 32, U64_MAX, U64_MAX, U64_MAX)]
    return cases


def record88(case) -> bytes:
    """from || to || amount || nonce || chain_id, little-endian: the first 88 bytes of a zkmi_signed_tx"""
    _, f, t, amount, nonce, chain_id = case
    return bytes(f) + bytes(t) + struct.pack("<QQQ", amount, nonce, chain_id)


def expected(case):
    """the four messages by the model: readable transfer and withdrawal, legacy transfer and withdrawal"""
    _, f, t, amount, nonce, chain_id = case
    return (E.transfer_message(f, t, amount, nonce, chain_id), E.withdraw_message(f, t, amount, nonce),
            E.legacy_transfer_message(f, t, amount, nonce, chain_id), E.legacy_withdraw_message(f, t, amount, nonce))


# what the header declares (tx_msg.h TX_*_MIN / MAX, the legacy lengths, TX_MSG_STRIDE)
BOUNDS = (236, 293, 209, 259, 88, 80)
