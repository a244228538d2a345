"""Authorisation of transfers and withdrawals from their fields on the GPU
(tx_auth.hip over tx_msg.h and ed25519.h; gpu.Ed25519Verifier.auth_records,
tx_auth's device path and DeviceAccountState.batches(verifier=) above it).
The oracle throughout is tx_auth._verify over ModelVerifier: the plain-Python
model with the messages built by zelana_amd/ed25519.py.  First the message
builders alone through a probe kernel (tests/device/tx_msg_probe.hip) on the
case list of tx_msg_cases, as the host check runs them on the CPU; then
auth_records at 1, 63, 64, 65 and 257 records of a mixed pile with one record
of every reason and format at the wave's edges; all-readable and all-legacy
piles; a retry list that crosses a wave, and one that crosses the curve
kernel's chunk; the decimal and base58 edges end to
end; the ABI's edges; tx_auth with the messages built on the device and in
Python; and signed batches through the account state."""
import ctypes
import hashlib
import os

import numpy as np
import pytest

import tx_msg_cases as C
from zelana_amd import ed25519 as E
from zelana_amd import tx_auth as T

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257]
DISTINCT = 65  # records signed for the pile; the model signs and verifies a few hundred a second
SECOND_PASS = ["txauth_format_legacy", "txauth_hash_legacy", "txauth_curve_legacy"]
FIRST_PASS = ["txauth_format", "txauth_hash", "txauth_curve", "txauth_compact", "txauth_epilogue"]
NOT_A_POINT = (2).to_bytes(32, "little")  # y = 2 is on no point


@pytest.fixture(scope="module")
def ctx():
    from zelana_amd.gpu import Context
    c = Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def verifier(ctx):
    from zelana_amd.gpu import Ed25519Verifier
    return Ed25519Verifier(ctx)


def _seed(tag):
    return hashlib.sha256(b"tx-auth-device/" + tag.encode()).digest()


SEEDS = [_seed(f"key/{j}") for j in range(8)]
KEYS = [E.public_key(s) for s in SEEDS]


def _model(items):
    """the oracle: reasons and formats by the Python model, messages built in Python"""
    return list(zip(*T._verify(T.ModelVerifier(), items)))


def _device(verifier, items):
    got = list(zip(*T.verify_signed(verifier, items, device_messages=True)))
    # the raw call says the same in the ABI's codes
    r, f = verifier.auth_records(T.pack(items))
    assert r.dtype == np.uint8 and f.dtype == np.uint8 and r.shape == f.shape == (len(items),)
    if all(len(t.signature) == 64 for t in items):
        assert [(T._REASONS[a], T._FORMATS[b]) for a, b in zip(r.tolist(), f.tolist())] == got
    return got


def _timers(ctx, names):
    from zelana_amd._lib import lib
    out = {}
    for k in names:
        ms, cnt = ctypes.c_double(0), ctypes.c_uint64(0)
        if lib().zkmi_profile_get(ctx.h, k.encode(), ctypes.byref(ms), ctypes.byref(cnt)) == 0:
            out[k] = cnt.value
    return out


# ------------------------------------------------------------------- the probe
def test_message_builders_on_the_device():
    here = os.path.dirname(os.path.abspath(__file__))
    L = ctypes.CDLL(os.path.join(here, "..", "zelana_amd", "libzkmi_txprobe.so"))
    stride = L.tx_probe_stride()
    assert stride % 16 == 0 and stride >= max(C.BOUNDS)
    cases = C.all_cases()
    n = len(cases)
    ins = np.frombuffer(b"".join(C.record88(c) for c in cases), np.uint32).reshape(n, 22).copy()
    out, lens = np.zeros((n, 4, stride), np.uint8), np.zeros((n, 4), np.uint32)
    vp = ctypes.c_void_p
    L.tx_probe_run.argtypes = [ctypes.c_int, vp, vp, vp]
    rc = L.tx_probe_run(n, ins.ctypes.data, out.ctypes.data, lens.ctypes.data)
    assert rc == 0, f"HIP error {rc}"
    seen = [[], [], [], []]
    for i, case in enumerate(cases):
        for kind, want in enumerate(C.expected(case)):
            ln = int(lens[i, kind])
            assert ln == len(want), (case[0], kind, ln, len(want))
            assert out[i, kind, :ln].tobytes() == want, (case[0], kind)
            # zeros to the end of the last 16-byte piece, and nothing written after it
            full = (ln + 15) // 16 * 16
            assert not out[i, kind, ln:full].any() and (out[i, kind, full:] == 0xA5).all(), (case[0], kind)
            seen[kind].append(ln)
    assert (min(seen[0]), max(seen[0]), min(seen[1]), max(seen[1]), max(seen[2]), max(seen[3])) == C.BOUNDS


# -------------------------------------------------------------------- the pile
def _make(i, withdrawal, legacy, signer=None, from_=None):
    """record i of the pile, honest: signed by key `signer` (i % 8 by default) over its own fields"""
    j = i % 8 if signer is None else signer
    frm = KEYS[j] if from_ is None else KEYS[from_]
    amount, nonce = 10**(i % 20) + i, i * 977
    if withdrawal:
        l1 = bytes(i % 4) + C.rnd(f"pile/l1/{i}", 32 - i % 4)
        t = T.SignedWithdrawal(frm, l1, amount, nonce, b"", KEYS[j])
    else:
        t = T.SignedTransfer(frm, KEYS[(j + 1 + i % 5) % 8], amount, nonce, 1 + i % 3, b"", KEYS[j])
    t.signature = E.sign(SEEDS[j], t.messages()[1 if legacy else 0])
    return t


class Pile:
    """257 records (65 distinct ones, repeated) and the model's answer on each, made once.  Transfers and
    withdrawals alternate irregularly, one in three is signed over the legacy
    message, and every fifth is spoiled in a way of its own: amount + 1, a
    bit of R, s + L, a key on no point, or a valid signature by a key that is
    not `from`, once in each format.  edge: one record of every reason and
    format, which prefix(n) places at lanes 0, 63, 64 and n - 1."""

    def __init__(self):
        self.base = []
        for i in range(DISTINCT):
            withdrawal, legacy = (i * 7) % 5 in (1, 3) or i % 11 == 0, i % 3 == 2
            t = _make(i, withdrawal, legacy)
            if i % 5 == 4:
                how = (i // 5) % 6
                if how == 0:
                    t.amount += 1
                elif how == 1:
                    t.signature = bytes([t.signature[0] ^ 1]) + t.signature[1:]
                elif how == 2:
                    t.signature = t.signature[:32] + (int.from_bytes(t.signature[32:], "little") + E.L).to_bytes(32, "little")
                elif how == 3:
                    t.signer_pubkey = NOT_A_POINT
                else:
                    t = _make(i, withdrawal, how == 5, signer=(i + 3) % 8, from_=i % 8)
            self.base.append(t)
        self.base_want = _model(self.base)
        self.base = [self.base[i % DISTINCT] for i in range(SIZES[-1])]
        self.base_want = [self.base_want[i % DISTINCT] for i in range(SIZES[-1])]
        g, w = _make(1000, False, False), _make(1001, True, True)
        bad_amount = _make(1002, True, False)
        bad_amount.amount += 1
        big_s = _make(1003, False, True)
        big_s.signature = big_s.signature[:32] + (int.from_bytes(big_s.signature[32:], "little") + E.L).to_bytes(32, "little")
        no_key = _make(1004, False, False)
        no_key.signer_pubkey = no_key.from_ = NOT_A_POINT
        self.edge = [g, w, no_key, bad_amount, big_s, _make(1005, True, False, signer=2, from_=5),
                     _make(1006, False, True, signer=3, from_=6)]
        self.edge_want = _model(self.edge)
        assert self.edge_want == [(T.OK, T.READABLE), (T.OK, T.LEGACY), (T.INVALID_PUBKEY, None),
                                  (T.VERIFICATION_FAILED, None), (T.VERIFICATION_FAILED, None),
                                  (T.FROM_MISMATCH, T.READABLE), (T.FROM_MISMATCH, T.LEGACY)]
        assert set(self.edge_want) <= set(self.base_want)
        kinds = [isinstance(t, T.SignedWithdrawal) for t in self.base]
        assert 80 < sum(kinds) < 180 and any(a == b for a, b in zip(kinds, kinds[1:])) and any(a != b for a, b in zip(kinds, kinds[1:]))

    def prefix(self, n, round_):
        """the first n records with edge records (other ones each round) at lanes 0, 63, 64 and n - 1"""
        items, want = list(self.base[:n]), list(self.base_want[:n])
        for j, lane in enumerate(sorted({0, 63, 64, n - 1})):
            if lane < n:
                e = (4 * round_ + j) % len(self.edge)
                items[lane], want[lane] = self.edge[e], self.edge_want[e]
        return items, want

    def honest(self, fmt):
        return [t for t, w in zip(self.base, self.base_want) if w == (T.OK, fmt)]


@pytest.fixture(scope="module")
def pile():
    return Pile()


def test_auth_records_matches_the_model_at_every_size(verifier, pile):
    for n in SIZES:
        lanes = len({0, 63, 64, n - 1} & set(range(n)))
        for round_ in range(-(-len(pile.edge) // lanes)):  # until every edge record has stood at an edge lane
            items, want = pile.prefix(n, round_)
            got = _device(verifier, items)
            assert got == want, (n, round_, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])


def test_all_readable_runs_no_second_pass(ctx, verifier, pile):
    from zelana_amd._lib import lib
    items = pile.honest(T.READABLE)[:70]
    assert len(items) == 70
    lib().zkmi_profile_reset(ctx.h)
    lib().zkmi_profile_enable(ctx.h, 1)
    try:
        r, f = verifier.auth_records(T.pack(items))
        seen = _timers(ctx, FIRST_PASS + SECOND_PASS)
    finally:
        lib().zkmi_profile_enable(ctx.h, 0)
    assert r.tolist() == [0] * 70 and f.tolist() == [1] * 70  # ZKMI_TXAUTH_OK, ZKMI_TXFMT_READABLE
    assert all(seen.get(k) == 1 for k in FIRST_PASS), seen
    assert not any(seen.get(k) for k in SECOND_PASS), seen


def test_all_legacy_runs_the_second_pass_once(ctx, verifier, pile):
    from zelana_amd._lib import lib
    have = pile.honest(T.LEGACY)
    items = [have[i % len(have)] for i in range(70)]
    lib().zkmi_profile_reset(ctx.h)
    lib().zkmi_profile_enable(ctx.h, 1)
    try:
        r, f = verifier.auth_records(T.pack(items))
        seen = _timers(ctx, FIRST_PASS + SECOND_PASS)
    finally:
        lib().zkmi_profile_enable(ctx.h, 0)
    assert r.tolist() == [0] * 70 and f.tolist() == [2] * 70  # ZKMI_TXFMT_LEGACY
    assert all(seen.get(k) == 1 for k in FIRST_PASS + SECOND_PASS), seen


def test_retry_list_across_a_wave(verifier, pile):
    """257 honest records of which exactly 65 need the second pass: the list
    crosses a wave and a block of the curve kernel.  They lie in the first two
    waves and in the last lanes, so several waves add to the list."""
    readable, legacy = pile.honest(T.READABLE), pile.honest(T.LEGACY)
    where = set(range(0, 66, 2)) | set(range(257 - 32, 257))
    assert len(where) == 65
    items, want, a, b = [], [], 0, 0
    for i in range(257):
        if i in where:
            items.append(legacy[a % len(legacy)])
            want.append((T.OK, T.LEGACY))
            a += 1
        else:
            items.append(readable[b % len(readable)])
            want.append((T.OK, T.READABLE))
            b += 1
    assert _device(verifier, items) == want
    # and 65 that fail both passes beside 192 that pass the first
    spoiled = []
    for i, t in enumerate(items):
        if i in where:
            t = T.SignedTransfer(**vars(t)) if isinstance(t, T.SignedTransfer) else T.SignedWithdrawal(**vars(t))
            t.nonce += 1
        spoiled.append(t)
    want = [(T.VERIFICATION_FAILED, None) if i in where else w for i, w in enumerate(want)]
    assert _device(verifier, spoiled) == want


def test_both_passes_across_the_curve_kernels_chunk(verifier, pile):
    """2^18 + 65 records, the pile's honest legacy ones repeated, so that the
    first pass and the retry list both cross the 2^18 signatures one launch of
    the curve kernel takes; one record of every reason and format on either
    side of the seam and at the end"""
    n, seam = (1 << 18) + 65, 1 << 18
    legacy = T.pack(pile.honest(T.LEGACY))
    rec = np.tile(legacy, -(-n // legacy.size))[:n].copy()
    want_r, want_f = np.zeros(n, np.uint8), np.full(n, 2, np.uint8)  # ZKMI_TXAUTH_OK, ZKMI_TXFMT_LEGACY
    edge = T.pack(pile.edge)
    codes = [(T._REASONS.index(r), T._FORMATS.index(f)) for r, f in pile.edge_want]
    for at in (seam - len(codes), seam, n - len(codes)):
        rec[at:at + len(codes)] = edge
        want_r[at:at + len(codes)], want_f[at:at + len(codes)] = [c[0] for c in codes], [c[1] for c in codes]
    r, f = verifier.auth_records(rec)
    assert np.array_equal(r, want_r), np.flatnonzero(r != want_r)[:8]
    assert np.array_equal(f, want_f), np.flatnonzero(f != want_f)[:8]


def test_decimal_and_base58_edges_end_to_end(verifier):
    """the cases of the CPU list, signed honestly by the model and verified on
    the device, then one digit's worth of a field changed"""
    cases = C.all_cases()
    transfers = [c for c in cases if c[0].startswith(("amount", "all three", "from", "shortest", "longest"))]
    withdrawals = [c for c in cases if c[0].startswith(("to_l1", "shortest", "longest"))] + \
                  [c for c in cases if c[0].startswith("nonce")][::3]
    assert len(transfers) >= 60 and len(withdrawals) >= 20
    honest, changed = [], []
    for i, (_, _, to, amount, nonce, chain_id) in enumerate(transfers):
        t = T.sign_transfer(SEEDS[i % 8], to, amount, nonce, chain_id)
        honest.append(t)
        c = T.SignedTransfer(**vars(t))
        if i % 3 == 0:
            c.amount = amount - 1 if amount else 1
        elif i % 3 == 1:
            c.nonce = nonce + 1 if nonce < C.U64_MAX else nonce - 1
        else:
            c.chain_id = chain_id ^ 1
        changed.append(c)
    for i, (_, _, to, amount, nonce, _) in enumerate(withdrawals):
        w = T.sign_withdrawal(SEEDS[i % 8], to, amount, nonce)
        honest.append(w)
        c = T.SignedWithdrawal(**vars(w))
        if i % 2 == 0:
            c.to_l1_address = to[:31] + bytes([to[31] ^ 1])  # the last base58 digit, or with 32 zeros the digit count
        else:
            c.to_l1_address = bytes([to[0] ^ 1]) + to[1:]    # a leading zero byte made or unmade, or the top digit
        changed.append(c)
    assert _model(honest[:3] + honest[-3:]) == [(T.OK, T.READABLE)] * 6
    assert _device(verifier, honest) == [(T.OK, T.READABLE)] * len(honest)
    got = _device(verifier, changed)
    assert got == [(T.VERIFICATION_FAILED, None)] * len(changed)
    assert got[::7] == _model(changed[::7])


# --------------------------------------------------------------------- the ABI
def test_abi_edges(ctx, verifier, pile):
    from zelana_amd import gpu
    from zelana_amd._lib import ZkmiError, lib, u8p
    assert gpu.SIGNED_TX_DTYPE.itemsize == 192
    assert [gpu.SIGNED_TX_DTYPE.fields[k][1] for k in ("from", "to", "amount", "nonce", "chain_id", "signer_pubkey",
                                                      "signature", "kind", "reserved")] == [0, 32, 64, 72, 80, 88, 120, 184, 185]
    # n = 0 with null arrays does nothing
    assert lib().zkmi_tx_auth_many(ctx.h, 0, None, None, None) == 0
    r, f = verifier.auth_records(np.zeros(0, gpu.SIGNED_TX_DTYPE))
    assert r.shape == f.shape == (0,)
    assert T.verify_signed(verifier, []) == ([], [])
    items, want = pile.prefix(5, 0)
    good = T.pack(items)
    for spoil in ("kind", "reserved first", "reserved last"):
        rec = good.copy()
        if spoil == "kind":
            rec["kind"][3] = 2
        else:
            rec["reserved"][4, 0 if spoil.endswith("first") else 6] = 1
        reasons, formats = np.full(5, 77, np.uint8), np.full(5, 78, np.uint8)
        rc = lib().zkmi_tx_auth_many(ctx.h, 5, rec.ctypes.data, reasons.ctypes.data_as(u8p), formats.ctypes.data_as(u8p))
        assert rc == -1 and reasons.tolist() == [77] * 5 and formats.tolist() == [78] * 5, spoil  # ZKMI_EINVAL, nothing written
        with pytest.raises(ZkmiError):
            verifier.auth_records(rec)
    reasons = np.full(5, 77, np.uint8)
    assert lib().zkmi_tx_auth_many(ctx.h, 5, good.ctypes.data, reasons.ctypes.data_as(u8p), None) == -1
    assert lib().zkmi_tx_auth_many(ctx.h, (1 << 26) + 1, good.ctypes.data, reasons.ctypes.data_as(u8p),
                                   reasons.ctypes.data_as(u8p)) == -1
    assert reasons.tolist() == [77] * 5
    with pytest.raises(ValueError):
        verifier.auth_records(np.zeros(3, np.uint8))
    # a large call, a small one, a large one on one context: the workspace of the larger serves the smaller after it
    big, big_want = pile.prefix(257, 1)
    assert _device(verifier, big) == big_want
    assert _device(verifier, items) == want
    assert _device(verifier, big) == big_want
    # verify_many beside it still answers as before: the two share the tables of -A
    msgs = [t.messages()[0] for t in items]
    assert verifier.verify_many([t.signer_pubkey for t in items], msgs, [t.signature for t in items]).tolist() == \
        [E.verify(t.signer_pubkey, m, t.signature) for t, m in zip(items, msgs)]


# --------------------------------------------------------------------- tx_auth
def _forty_transfers():
    txs, want = [], []
    for i in range(34):
        legacy = i % 3 == 2
        txs.append(T.sign_transfer(SEEDS[i % 8], KEYS[(i + 1) % 8], 1000 + i, i, 1 + i % 2, legacy=legacy))
        want.append((T.OK, T.LEGACY if legacy else T.READABLE))
    g = txs[0]
    txs.append(T.SignedTransfer(NOT_A_POINT, g.to, 5, 0, 1, g.signature[:10], NOT_A_POINT))  # a wrong length beside a bad key
    want.append((T.INVALID_PUBKEY, None))
    txs.append(T.SignedTransfer(g.from_, g.to, g.amount, g.nonce, g.chain_id, g.signature + b"\0", g.signer_pubkey))
    want.append((T.INVALID_SIGNATURE_LENGTH, None))
    txs.append(T.SignedTransfer(g.from_, g.to, g.amount + 1, g.nonce, g.chain_id, g.signature, g.signer_pubkey))
    want.append((T.VERIFICATION_FAILED, None))
    txs.append(T.SignedTransfer(g.from_, g.to, g.amount, g.nonce, g.chain_id, g.signature[:32] + E.L.to_bytes(32, "little"),
                                g.signer_pubkey))
    want.append((T.VERIFICATION_FAILED, None))
    for legacy in (False, True):  # a valid signature by a key that is not `from`
        t = T.SignedTransfer(KEYS[3], KEYS[4], 9, 9, 1, b"", KEYS[5])
        t.signature = E.sign(SEEDS[5], t.messages()[1 if legacy else 0])
        txs.append(t)
        want.append((T.FROM_MISMATCH, T.LEGACY if legacy else T.READABLE))
    return txs, want


def _forty_withdrawals():
    l1s = [bytes(32), bytes(3) + C.rnd("l1/a", 29), C.rnd("l1/b"), b"\xff" * 32]
    reqs, want = [], []
    for i in range(36):
        legacy = i % 4 == 3
        reqs.append(T.sign_withdrawal(SEEDS[i % 5], l1s[i % 4], 2**64 - 1 - i, i, legacy=legacy))
        want.append((T.OK, T.LEGACY if legacy else T.READABLE))
    g = reqs[0]
    reqs.append(T.SignedWithdrawal(NOT_A_POINT, g.to_l1_address, 1, 0, b"", NOT_A_POINT))
    want.append((T.INVALID_PUBKEY, None))
    reqs.append(T.SignedWithdrawal(g.from_, g.to_l1_address, g.amount, g.nonce, b"", g.signer_pubkey))
    want.append((T.INVALID_SIGNATURE_LENGTH, None))
    reqs.append(T.SignedWithdrawal(g.from_, l1s[2], g.amount, g.nonce, g.signature, g.signer_pubkey))
    want.append((T.VERIFICATION_FAILED, None))
    w = T.SignedWithdrawal(KEYS[1], l1s[1], 4, 4, b"", KEYS[2])
    w.signature = E.sign(SEEDS[2], w.messages()[0])
    reqs.append(w)
    want.append((T.FROM_MISMATCH, T.READABLE))
    return reqs, want


def test_device_and_host_messages_give_equal_results(verifier):
    txs, want_t = _forty_transfers()
    reqs, want_w = _forty_withdrawals()
    assert len(txs) == 40 and len(reqs) == 40
    for fn, items, want in ((T.verify_transfers, txs, want_t), (T.verify_withdrawals, reqs, want_w),
                            (T.verify_signed, txs[::2] + reqs[::3] + txs[1::2], None)):
        on_device = fn(verifier, items, device_messages=True)
        on_host = fn(verifier, items, device_messages=False)
        assert on_device == on_host == fn(verifier, items)
        if want is not None:
            assert list(zip(*on_device)) == want
        assert on_device == T._verify(T.ModelVerifier(), items)
    # a wrong-length signature beside a bad key reports the key
    assert want_t[34] == (T.INVALID_PUBKEY, None) and len(txs[34].signature) == 10
    # a verifier without auth_records takes the host path, and cannot be made to take the other
    assert T.verify_transfers(T.ModelVerifier(), txs[:2]) == ([T.OK, T.OK], [T.READABLE, T.READABLE])
    with pytest.raises(ValueError):
        T.verify_transfers(T.ModelVerifier(), txs[:2], device_messages=True)


# ----------------------------------------------------------- the account state
def test_signed_batches_through_the_account_state(ctx, verifier):
    from zelana_amd.account_state import DeviceAccountState
    # four keys with distinct leading bytes: a depth-8 tree places an account by the first byte of its id
    seeds, i = [], 0
    while len(seeds) < 4:
        if E.public_key(_seed(f"acct/{i}"))[0] not in {E.public_key(s)[0] for s in seeds}:
            seeds.append(_seed(f"acct/{i}"))
        i += 1
    ids = [E.public_key(s) for s in seeds]

    def signed_batches(forge: bool):
        b1 = {"batch_id": 7, "transfers": [T.sign_transfer(seeds[0], ids[1], 30, 0, 1),
                                            T.sign_transfer(seeds[1], ids[2], 5, 0, 1, legacy=True)],
              "withdrawals": [T.sign_withdrawal(seeds[2], C.rnd("acct/l1"), 11, 0)]}
        t = T.sign_transfer(seeds[0], ids[3], 8, 1, 1)
        if forge:
            t.amount = 80
        b2 = {"batch_id": 8, "transfers": [T.sign_transfer(seeds[3], ids[0], 2, 0, 1), t],
              "withdrawals": [T.sign_withdrawal(seeds[1], bytes(32), 3, 1, legacy=True)]}
        return [b1, b2]

    def fresh():
        st = DeviceAccountState(ctx, depth=8, max_nodes=1 << 12)
        st.insert_many([(i, 1000 + k, 0) for k, i in enumerate(ids)])
        return st

    class CountingVerifier:
        """the verifier, counting which of its two entries batches() reaches"""

        def __init__(self, inner):
            self.inner, self.records, self.messages = inner, 0, 0

        def auth_records(self, records):
            self.records += len(records)
            return self.inner.auth_records(records)

        def verify_many(self, *a):
            self.messages += len(a[0])
            return self.inner.verify_many(*a)

    honest = signed_batches(False)
    as_tuples = [{"batch_id": b["batch_id"], "transfers": [T.transfer_tuple(t) for t in b["transfers"]],
                  "withdrawals": [T.withdrawal_tuple(w) for w in b["withdrawals"]]} for b in honest]
    a, b = fresh(), fresh()
    try:
        counting = CountingVerifier(verifier)
        want = a.batches(as_tuples)
        got = b.batches(honest, verifier=counting)
        assert got == want
        assert b.root() == a.root() and b.accounts == a.accounts
        assert (counting.records, counting.messages) == (6, 0)  # the device path, all six in one call
        # a forged amount in the second batch: refused before anything changes, in the words of the host path
        root, accounts = b.root(), {k: list(v) for k, v in b.accounts.items()}
        with pytest.raises(ValueError, match=r"batch 8: transfers\[1\] refused: signature verification failed"):
            b.batches(signed_batches(True), verifier=verifier)
        assert b.root() == root and b.accounts == accounts
        with pytest.raises(ValueError, match=r"batch 8: transfers\[1\] refused: signature verification failed"):
            b.batches(signed_batches(True), verifier=T.ModelVerifier())
        assert b.root() == root and b.accounts == accounts
    finally:
        a.close()
        b.close()
