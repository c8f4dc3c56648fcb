"""Key-capacity regrow while windows are open, on every packed-close layout.

One stream, host-pushed with KEY_INT64 and n_keys_hint=64 (kcap 512): batch 1
opens state for 64 keys, batch 2 brings 636 new keys into the same windows, so
n_keys passes kcap and every slab the op owns (the main one, the variance /
int64 side slab, the extras' slab) is regrown with open slots to carry over.
In batch 2 keys 0..15 of the old 64 get NULL rows only and keys 16..31 get no
row at all: what batch 1 left for them has to come out untouched. Batch 3
closes everything from a later window.

Each op kind runs through the helpers of its own test file and is compared
with that file's reference, in that file's form: tolerance 0 on every column,
mask, key order and window column (f64 by bits where the helper compares
bits), values read only where the reference's mask says valid."""
import functools

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import intref, medianref, varref
from tests import test_int64_values_gpu as t_int
from tests import test_median_gpu as t_med
from tests import test_multicol_gpu as t_mc
from tests import test_variance_gpu as t_var

pytestmark = pytest.mark.gpu

T0 = 1_000_000
N_OLD, N_ALL = 64, 700
KEYS = (10_000 + 37 * np.arange(N_ALL)).astype(np.int64)
# tumbling: the one window [T0, T0 + 1000) is open across the regrow.
# sliding 1000/200: five windows per row, so nslots passes its initial 4 in
# batch 1 and again, with open state, in batch 2.
SHAPES = {"tumbling": (1000, 0), "sliding": (1000, 200)}
PLAIN = ["count", "min", "max", "sum", "avg"]
FOUR = [("sum", 3, "s3"), ("min", 0, "m0"), ("max", 2, "x2"),
        ("avg", 1, "a1"), ("count", 3, "n3"), ("count", 0, "n0"),
        ("max", 1, "x1"), ("sum", 2, "s2")]


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _with_each(pool, n, rng):
    """n draws from pool, every member at least once, in random order"""
    return rng.permutation(np.r_[pool, rng.choice(pool, n - len(pool))])


@functools.lru_cache(maxsize=None)
def stream():
    """[(ts, keys, cols, valids), ...]: four f64 columns with a mask each
    (column 0 is the single-column ops' value column), plus the int64 values
    in a fifth slot. ts is non-decreasing over the whole stream."""
    rng = np.random.default_rng(1807)
    plan = [(2000, np.arange(N_OLD), 0, 500),
            (3000, np.r_[np.arange(16), np.arange(32, N_ALL)], 500, 1000),
            (5, np.array([3, 20, 650]), 3000, 3100)]
    out = []
    for b, (n, pool, lo, hi) in enumerate(plan):
        ts = (T0 + np.sort(rng.integers(lo, hi, n))).astype(np.int64)
        kid = _with_each(pool, n, rng)
        cols = [rng.uniform(-1e3, 1e3, n) * 10.0 ** j for j in range(4)]
        cols.append(rng.integers(-10**12, 10**12, n))
        valids = [rng.random(n) > 0.2 for _ in range(4)]
        if b == 0:
            valids[0] &= kid != 63    # no valid row until batch 2
        if b == 1:
            for v in valids:
                v &= kid >= 16        # old keys 0..15: NULL rows only
        valids.append(valids[0])
        for a in [ts, kid] + cols + valids:
            a.setflags(write=False)
        out.append((ts, KEYS[kid], cols, valids))
    old = np.isin(out[1][1], KEYS[:32])
    assert old.sum() >= 16 and not out[1][3][0][old].any()
    assert len(np.unique(np.r_[out[0][1], out[1][1]])) == N_ALL > 512
    return out


def single(col=0):
    """the stream as a single-column op takes it: batches and valids"""
    s = stream()
    return ([(ts, k, cols[col]) for ts, k, cols, _ in s],
            [valids[col].astype(np.uint8) for _, _, _, valids in s])


@functools.lru_cache(maxsize=None)
def f64_refs(shape):
    batches, valids = single()
    exp = t_var.run_oracle(*SHAPES[shape], batches, valids)
    return (exp, varref.expected(exp, batches, valids),
            medianref.expected(exp, batches, valids))


@functools.lru_cache(maxsize=None)
def int_ref(shape):
    batches, valids = single(4)
    return intref.run(*SHAPES[shape], batches, valids)


def run_plain(shape):
    batches, valids = single()
    exp, _, _ = f64_refs(shape)
    got = t_var.run_gpu(*SHAPES[shape], batches, PLAIN, valids=valids)
    t_var.assert_rows(got, exp, None, PLAIN)


def run_stddev(shape):
    names = PLAIN + ["stddev"]
    batches, valids = single()
    exp, var, _ = f64_refs(shape)
    got = t_var.run_gpu(*SHAPES[shape], batches, names, valids=valids)
    t_var.assert_rows(got, exp, var, names)


def run_int64(shape, names=t_int.BASE):
    batches, valids = single(4)
    got = t_int.run_gpu("host", *SHAPES[shape], batches, names, valids)
    t_int.assert_rows(got, int_ref(shape), names)


def run_int64_var(shape):
    run_int64(shape, t_int.BASE + ["var_samp"])


def run_columns(shape, aggs):
    batches = [(ts, k, cols[:4], valids[:4]) for ts, k, cols, valids in stream()]
    t_mc._check_host(*SHAPES[shape], batches, aggs)


def run_median_stddev(shape):
    batches, valids = single()
    exp, var, med = f64_refs(shape)
    got = t_med.run_gpu(*SHAPES[shape], batches, t_med.EXAMPLE, valids=valids)
    t_med.assert_rows(got, exp, med, t_med.EXAMPLE)
    vals, msk = var["stddev_samp"]
    assert np.array_equal(got["stddev_valid"], msk)
    m = msk.astype(bool)
    assert np.array_equal(got["stddev"][m], vals[m])


KINDS = {
    "plain": run_plain,
    "stddev": run_stddev,
    "int64": run_int64,
    "int64_var_samp": run_int64_var,
    "two_columns": lambda shape: run_columns(shape, t_mc.TWO),
    "four_columns": lambda shape: run_columns(shape, FOUR),
    "median_stddev": run_median_stddev,
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", list(KINDS))
def test_regrow_with_open_windows(kind, shape):
    KINDS[kind](shape)
