"""Shared pieces of the device int64 intern tests (pure numpy, no GPU, no
engine import): the Python restatement of the intern's home-slot hash, a
seeded search for keys with a given home slot, and the `Stream` helper that
turns batches of key INDICES into int64 key values plus the oracle's
expectation computed on the indices.

tests/test_intern_i64_cpu.py pins all three (published hash vectors, the
search's determinism, the helper against tests/pyref.py), so that
tests/test_intern_i64_gpu.py cannot be vacuous.

The hash is the one DESIGN.md documents for the int64 intern:
    home = splitmix64(key as u64) & fp_mask & (P - 1)
with fp_mask = 2^bits - 1 under dz_debug_intern_fp_bits (all ones otherwise).
"""
import numpy as np

from oracle import pyoracle

M64 = (1 << 64) - 1
P_MIN = 65_536            # the smallest intern table (ensure_intern's rule)
INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1
# DESIGN.md "Intern: int64 keys": an EMPTY slot's claim word is 0, so key 0 is
# the one value that cannot be stored as its own claim word; it lives in a
# dedicated cell behind the table.
EMPTY_MARK_KEY = 0
SPECIALS = (0, -1, 1, INT64_MIN, INT64_MIN + 1, INT64_MAX, EMPTY_MARK_KEY)


def splitmix64(x):
    """The engine's splitmix64 device function on Python ints."""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def home_slot(key, P=P_MIN, fp_bits=64):
    """Home slot of one int64 key in a table of P slots."""
    return splitmix64(int(key) & M64) & ((1 << fp_bits) - 1) & (P - 1)


def home_slots(keys, P=P_MIN, fp_bits=64):
    """home_slot over an int64 array (wrapping uint64 arithmetic)."""
    x = np.asarray(keys, np.int64).view(np.uint64).copy()
    with np.errstate(over="ignore"):
        x += np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    mask = np.uint64(((1 << fp_bits) - 1) & (P - 1))
    return (x & mask).astype(np.int64)


def keys_with_home(slots, per_slot, seed, P=P_MIN):
    """{slot: the first `per_slot` distinct non-zero keys of a seeded random
    int64 sequence whose home slot it is}, drawn in blocks until complete."""
    rng = np.random.default_rng(seed)
    found = {s: [] for s in slots}
    while any(len(v) < per_slot for v in found.values()):
        cand = rng.integers(INT64_MIN, INT64_MAX, 1 << 18, dtype=np.int64,
                            endpoint=True)
        home = home_slots(cand, P)
        for s, v in found.items():
            for k in cand[home == s]:
                if len(v) < per_slot and k != 0 and int(k) not in v:
                    v.append(int(k))
    return found


def sparse_values(n, seed):
    """n distinct int64 values spread over the whole range, never a SPECIAL."""
    rng = np.random.default_rng(seed)
    out = []
    seen = set(SPECIALS)
    while len(out) < n:
        for k in rng.integers(INT64_MIN, INT64_MAX, n, dtype=np.int64,
                              endpoint=True):
            if int(k) not in seen and len(out) < n:
                seen.add(int(k))
                out.append(int(k))
    return np.array(out, np.int64)


class Stream:
    """Batches of key indices into `values` (int64), with timestamps, values
    and the oracle's expected output ON THE INDICES, computed once and
    shared (read-only). The expected emitted key column is
    values[exp["key"]]."""

    def __init__(self, values, kid_batches, seed, rows_per_ms=4, len_ms=1000,
                 slide_ms=0):
        self.values = np.asarray(values, np.int64)
        assert len(set(self.values.tolist())) == len(self.values)
        rng = np.random.default_rng(seed)
        self.batches = []
        o = pyoracle.Oracle(len_ms, slide_ms)
        row = 0
        for kid in kid_batches:
            kid = np.asarray(kid, np.int64)
            n = len(kid)
            ts = (1_000_000 + np.arange(row, row + n) // rows_per_ms).astype(
                np.int64)
            row += n
            v = rng.uniform(0, 115, n)
            self.batches.append((ts, kid, self.values[kid], v))
            o.push(ts, kid, v)
        o.finish()
        self.exp = o.fetch()
        o.close()
        for a in self.exp.values():
            a.setflags(write=False)
        assert len(self.exp["key"]) > 0


def growing_batches(n_keys, introduce, n_batches, rows, seed):
    """Random key picks per batch; key k first becomes available in batch
    introduce[k], and every batch's newly available keys do appear in it."""
    rng = np.random.default_rng(seed)
    introduce = np.asarray(introduce)
    out = []
    for b in range(n_batches):
        avail = np.flatnonzero(introduce <= b)
        new = np.flatnonzero(introduce == b)
        kid = avail[rng.integers(0, len(avail), rows)]
        if len(new):
            kid[rng.choice(rows, len(new), replace=False)] = new
        out.append(kid)
    return out
