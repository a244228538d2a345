"""The nullifier set's references (no GPU, no native code): the sequential
model of a spend over a Python set (the reference's HashSet<[u8; 32]>, one
transfer at a time), the parallel rounds restated (for the number of rounds a
call takes), nullifier_set.h's slot function restated, and the named case
lists that tests/test_nullifier_set_cpu.py and tests/test_gpu_nullifier_set.py
share."""
import hashlib
import random

ACCEPTED, SKIPPED, SPENT_STORED, SPENT_IN_CALL, DUP_IN_TX = 0, 1, 2, 3, 4
M64 = (1 << 64) - 1


def key(i, tag=b"nf") -> bytes:
    """a 32-byte key that looks like a hash output"""
    return hashlib.sha256(tag + str(i).encode()).digest()


def small_key(i) -> bytes:
    """key number i of a tiny universe (only byte 0 and byte 31 differ between them)"""
    return bytes([i + 1]) + bytes(30) + bytes([0x80 | i])


# ------------------------------------------------------------ sequential model
def spend(stored: set, order: list, keys, per_tx, eligible=None):
    """One call, one transfer at a time.  stored / order (the set and its
    insertion log) are updated in place.  -> (verdicts, details)."""
    assert len(keys) % per_tx == 0
    ntx = len(keys) // per_tx
    before = set(stored)
    owner = {}  # key -> the accepted transfer of this call that spent it
    verdicts, details = [], []
    for t in range(ntx):
        if eligible is not None and not eligible[t]:
            verdicts.append(SKIPPED)
            details.append(0)
            continue
        mine = keys[t * per_tx:(t + 1) * per_tx]
        res = (ACCEPTED, 0)
        for k, x in enumerate(mine):
            if x in before:
                res = (SPENT_STORED, k)
            elif x in owner:
                res = (SPENT_IN_CALL, owner[x])
            elif x in mine[:k]:
                res = (DUP_IN_TX, k)
            else:
                continue
            break
        if res[0] == ACCEPTED:
            for x in mine:
                owner[x] = t
                stored.add(x)
                order.append(x)
        verdicts.append(res[0])
        details.append(res[1])
    return verdicts, details


def spend_or_refuse(stored, order, capacity, keys, per_tx, eligible=None):
    """spend, or None with nothing changed when the accepted keys do not fit"""
    s, o = set(stored), list(order)
    res = spend(s, o, keys, per_tx, eligible)
    if len(o) > capacity:
        return None
    stored |= s
    order[:] = o
    return res


# ---------------------------------------------------------- the parallel form
def rounds(stored: set, keys, per_tx, eligible=None):
    """The rounds as the library runs them (decisions of a round read only the
    states of the round before) -> (accepted flags, number of rounds)."""
    ntx = len(keys) // per_tx
    UND, ACC, REJ, SKIP = 0, 1, 2, 3
    state = []
    for t in range(ntx):
        mine = keys[t * per_tx:(t + 1) * per_tx]
        if eligible is not None and not eligible[t]:
            state.append(SKIP)
        elif any(x in stored for x in mine) or len(set(mine)) != len(mine):
            state.append(REJ)
        else:
            state.append(UND)
    n = 0
    while UND in state:
        cand, acc = {}, {}
        for t in range(ntx):
            if state[t] in (UND, ACC):
                for x in keys[t * per_tx:(t + 1) * per_tx]:
                    cand.setdefault(x, t)
                    if state[t] == ACC:
                        acc.setdefault(x, t)
        new = list(state)
        for t in range(ntx):
            if state[t] != UND:
                continue
            mine = keys[t * per_tx:(t + 1) * per_tx]
            if any(acc.get(x, ntx) < t for x in mine):
                new[t] = REJ
            elif all(cand[x] == t for x in mine):
                new[t] = ACC
        assert new != state, "a round decided nothing"
        state = new
        n += 1
    return [s == ACC for s in state], n


# -------------------------------------------------------------- slot function
def slot(k: bytes, slots: int) -> int:
    """ns_slot of nullifier_set.h"""
    assert len(k) == 32 and slots & (slots - 1) == 0
    h = 0x9E3779B97F4A7C15
    for i in range(8):
        w = int.from_bytes(k[4 * i:4 * i + 4], "little")
        h = ((h ^ w) * 0xBF58476D1CE4E5B9) & M64
        h ^= h >> 29
    h = (h * 0x94D049BB133111EB) & M64
    h ^= h >> 32
    return h & (slots - 1)


def slots_for(capacity: int) -> int:
    s = 2
    while s < 2 * capacity:
        s <<= 1
    return s


def keys_with_home(slots: int, home: int, n: int, tag=b"home") -> list:
    """n keys whose home slot in a table of `slots` is `home`"""
    out, i = [], 0
    while len(out) < n:
        k = key(i, tag)
        if slot(k, slots) == home:
            out.append(k)
        i += 1
    return out


# ----------------------------------------------------------------------- cases
def random_pile(seed, ntx, per_tx, universe=12, p_ineligible=0.2, pool=None):
    """(keys, eligible): ntx transfers over a tiny key universe (or `pool`), so
    conflicts of every kind are dense; some transfers ineligible"""
    rng = random.Random(seed)
    pool = pool or [small_key(i) for i in range(universe)]
    keys = [rng.choice(pool) for _ in range(ntx * per_tx)]
    eligible = [rng.random() >= p_ineligible for _ in range(ntx)]
    return keys, eligible


def mixed_pile(seed, ntx, per_tx, call):
    """(keys, eligible) for the consecutive GPU calls on one set: mostly fresh
    hash-like keys (so most transfers are accepted and the set grows), a share
    drawn from a pool that all calls of a set share (stored by earlier calls,
    repeated within this one), some transfers ineligible"""
    rng = random.Random(seed * 1000 + call)
    shared = [key(i, b"shared") for i in range(ntx + 8)]
    keys = []
    for i in range(ntx * per_tx):
        keys.append(rng.choice(shared) if rng.random() < 0.3 else key((seed, call, i), b"fresh"))
    eligible = [rng.random() >= 0.1 for _ in range(ntx)]
    return keys, eligible


def chain(n, tag=b"chain"):
    """A{n0,n1}, B{n1,n2}, C{n2,n3}, ...: transfer t is decided by round t + 1
    only; verdicts ACCEPTED, SPENT_IN_CALL (t - 1), ACCEPTED, ..."""
    ks = [key(i, tag) for i in range(n + 1)]
    return [k for t in range(n) for k in (ks[t], ks[t + 1])]


def abc(tag=b"abc"):
    """the issue's example: A{n1,n2}, B{n2,n3}, C{n3,n4}"""
    n = [key(i, tag) for i in range(1, 5)]
    return [n[0], n[1], n[1], n[2], n[2], n[3]]


def reasons_pile(tag=b"why"):
    """Transfer 4 = {f, a}: key 0 (f) was spent by transfer 3, which is accepted
    in round 3 only (behind the chain 1, 2, 3); key 1 (a) by transfer 0,
    accepted in round 1.  The rounds refuse transfer 4 for key 1 in round 2;
    the verdict must name key 0's owner: (SPENT_IN_CALL, 3)."""
    a, b, c, d, e, f = (key(i, tag) for i in range(6))
    return [a, b, c, d, d, e, e, f, f, a]


def halves():
    """keys equal in their low 16 bytes, and keys equal in their high 16 bytes"""
    lo, hi = key(0, b"lo")[:16], key(0, b"hi")[16:]
    same_low = [lo + key(i, b"x")[16:] for i in range(3)]
    same_high = [key(i, b"y")[:16] + hi for i in range(3)]
    return same_low, same_high
