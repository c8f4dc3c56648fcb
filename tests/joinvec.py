"""Join edge-case vectors: trip ids with a chosen home slot in the build
table, the probe geometry restated, and the match patterns laid over it.
Plain numpy/Python, no GPU: tests/test_joinvec_cpu.py pins the helpers."""
import numpy as np

HASH_MUL = 0x9e3779b97f4a7c15           # kernels.hip jhash / oracle.c oj_find
HASH_INV = pow(HASH_MUL, -1, 2 ** 64)   # the multiplier is odd: invertible
I64_MIN = -2 ** 63
I64_MAX = 2 ** 63 - 1
MIN_SLOTS = 1 << 16                     # smallest table (n_trips_hint <= 16384)


def jhash(trip):
    return ((int(trip) & (2 ** 64 - 1)) * HASH_MUL) % 2 ** 64


def home_slot(trip, slots=MIN_SLOTS):
    return jhash(trip) & (slots - 1)


def _signed(u):
    return u - 2 ** 64 if u >= 2 ** 63 else u


def trips_with_home(slot, count, slots=MIN_SLOTS, first=1):
    """`count` distinct int64 trip ids whose home slot is `slot`: pick hash
    values with the low bits fixed, multiply by the inverse. `first` offsets
    the high bits, so two calls with disjoint ranges give disjoint trips.
    Never returns the reserved id INT64_MIN."""
    assert 0 <= slot < slots and slots & (slots - 1) == 0
    out = []
    j = first
    while len(out) < count:
        t = _signed(((slot + j * slots) * HASH_INV) % 2 ** 64)
        j += 1
        if t != I64_MIN:
            out.append(t)
    return np.array(out, np.int64)


def geometry(n):
    """(C, chunk) of a probe over n rows: one 64-thread block per chunk."""
    C = min(512, max(1, (n + 8191) // 8192))
    return C, (n + C - 1) // C


PATTERNS = ("all", "none", "alternating", "lane0", "lane63", "chunk_ends",
            "runs64")


def pattern(name, n):
    """Boolean match mask over n probe rows. Ballot groups are 64 rows
    counted from each chunk's start, as k_join_emit walks them."""
    C, chunk = geometry(n)
    i = np.arange(n)
    in_chunk = i % chunk
    lane = in_chunk % 64
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "alternating":
        return i % 2 == 0
    if name == "lane0":
        return lane == 0
    if name == "lane63":
        return lane == 63
    if name == "chunk_ends":
        last = np.minimum(n, (i // chunk + 1) * chunk) - 1
        return (in_chunk == 0) | (i == last)
    if name == "runs64":
        return (i // 64) % 2 == 0
    raise ValueError(name)
