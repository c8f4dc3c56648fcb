"""GPU tests of the fold walk in k_regroup_t's fold modes: a bin's staged
segment is folded in groups of WALK_G records (8; 4 with two or three extra
value columns) whose LDS reads are all issued before the first update, the
last group clamped and masked, nulls through selects, the valid count in 32
bits.

Every case is differential against the CPU oracle (several value columns
against tests/multicolref.py, variance against tests/varref.py) and compared
bit for bit: float columns as their 64-bit patterns, so a flipped sign of
zero fails, with NaN allowed only where the oracle has NaN. Dense ids k * 512
all fall into bucket 0 with kloc = k, so one fold block sees every record and
a key's rows in one window are one bin's segment of one supertile (2,048
records)."""
import numpy as np
import pytest

import __graft_entry__ as graft
from tests import multicolref as mc
from tests import varref
from tests.test_split_supertile_gpu import (BASE, T0, _cat, _drive, run_gpu,
                                            run_oracle)

pytestmark = pytest.mark.gpu

G = (8, 4)  # the group sizes that ship
# 0 (a key absent from the window), 1, G-1, G, G+1, 2G, 2G+1 for both sizes
EDGE_LENS = [1, 3, 4, 5, 7, 8, 9, 16, 17]


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def assert_bits(got, exp, names=BASE):
    assert len(exp["key"]) > 0
    assert np.array_equal(got["key"], exp["key"]), "keys / first-seen order"
    assert np.array_equal(got["window_start"], exp["window_start"])
    assert np.array_equal(got["valid"], exp["valid"]), "validity"
    assert np.array_equal(got["count"], exp["count"]), "count"
    v = exp["valid"].astype(bool)
    for f in names:
        if f == "count":
            continue
        g = np.ascontiguousarray(got[f][v], np.float64)
        e = np.ascontiguousarray(exp[f][v], np.float64)
        nan = np.isnan(e)
        assert np.array_equal(np.isnan(g), nan), f + " NaN positions"
        assert np.array_equal(g[~nan].view(np.uint64),
                              e[~nan].view(np.uint64)), f + " bits"


def check_bits(batches, valids=None, **kw):
    got, _ = run_gpu(1000, 0, batches, valids=valids, **kw)
    exp = run_oracle(1000, 0, batches, valids)
    assert_bits(got, exp)
    return got, exp


def edge_batch(seed, lens=EDGE_LENS, nkeys_extra=1, shuffle=True):
    """One window, one bucket: key j * 512 has lens[j] rows, interleaved in
    a seeded order; key len(lens) * 512 is absent from this window (length
    0) and present in the next one."""
    rng = np.random.default_rng(seed)
    k = np.repeat(np.arange(len(lens)), lens)
    if shuffle:
        rng.shuffle(k)
    n = len(k)
    ts = np.full(n, T0, np.int64)
    # the next window: every key once more, the extra keys for the first time
    k2 = np.arange(len(lens) + nkeys_extra)
    k = np.concatenate([k, k2]) * 512
    ts = np.concatenate([ts, np.full(len(k2), T0 + 1000, np.int64)])
    v = rng.uniform(-50, 115, len(k))
    return ts, k.astype(np.int64), v


NK = 16 * 512


def test_group_edge_lengths():
    b = edge_batch(4101)
    got, exp = check_bits([b], n_keys_hint=NK)
    w0 = exp["window_start"] == exp["window_start"].min()
    assert sorted(exp["count"][w0].tolist()) == sorted(EDGE_LENS)


def _null_cases():
    lens = [8, 8, 16, 17, 9, 24]
    ts, k, v = edge_batch(4102, lens, shuffle=False)
    valid = np.ones(len(k), np.uint8)
    o = np.concatenate([[0], np.cumsum(lens)])
    valid[[o[0], o[0] + 7]] = 0          # first and last record of a group
    valid[o[1]:o[1] + 8] = 0             # a whole segment: touched, count 0
    valid[o[2] + 8:o[2] + 16] = 0        # the second group of two
    valid[o[3]:o[3] + 8] = 0             # the first group, the tail survives
    valid[o[4] + 8] = 0                  # the tail record alone
    valid[o[5] + 4:o[5] + 12] = 0        # across a group boundary
    return (ts, k, v), valid


def test_nulls_at_group_edges():
    b, valid = _null_cases()
    got, exp = check_bits([b], valids=[valid], n_keys_hint=NK)
    r = (got["key"] == 512) & (got["window_start"] == got["window_start"].min())
    assert r.sum() == 1 and got["count"][r][0] == 0 and not got["valid"][r][0]


@pytest.mark.parametrize("case", ["nan_first", "nan_mid", "neg_zero",
                                  "zero_mix_pn", "zero_mix_np"])
def test_nan_and_signed_zero(case):
    lens = [11, 17]
    ts, k, v = edge_batch(4103, lens, shuffle=False)
    valid = np.ones(len(k), np.uint8)
    if case == "nan_first":
        valid[0] = 0      # the NaN is the first VALID value of the bin
        v[1] = np.nan
        v[11] = np.nan
    elif case == "nan_mid":
        v[4] = np.nan     # mid-group
        v[11 + 12] = np.nan
    elif case == "neg_zero":
        v[:11] = -0.0
        v[11:28] = -0.0
    elif case == "zero_mix_pn":
        v[:11] = np.where(np.arange(11) % 2 == 0, 0.0, -0.0)
        v[11:28] = np.where(np.arange(17) % 3 == 0, 0.0, -0.0)
    else:
        v[:11] = np.where(np.arange(11) % 2 == 0, -0.0, 0.0)
        v[11:28] = np.where(np.arange(17) % 3 == 0, -0.0, 0.0)
    check_bits([(ts, k, v)], valids=[valid], n_keys_hint=NK)


@pytest.mark.parametrize("n", [2048, 2049, 4500])
def test_one_bin_across_supertiles(n):
    # one (window, key) takes n records of one bucket: exactly one supertile,
    # one supertile plus a one-record one, and a bin that crosses two
    # boundaries; magnitudes differ enough that any other summation order
    # changes the last bits
    rng = np.random.default_rng(4200 + n)
    ts = np.full(n, T0, np.int64)
    k = np.zeros(n, np.int64)
    v = rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-6, 7, n)
    valid = (rng.random(n) > 0.1).astype(np.uint8)
    valid[2040:2056 if n > 2056 else n] = 1
    check_bits([(ts, k, v)], valids=[valid], n_keys_hint=NK)


def test_late_rows_sum_in_row_order():
    # timestamps out of order inside the batch over two windows: a bin's
    # records are not contiguous in the bucket region
    rng = np.random.default_rng(4301)
    n = 3000
    ts = (T0 + rng.integers(0, 2000, n)).astype(np.int64)
    k = (rng.integers(0, 5, n) * 512).astype(np.int64)
    v = rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-6, 7, n)
    b2 = (np.full(40, T0 + 100, np.int64),  # a late batch into both bins
          (rng.integers(0, 5, 40) * 512).astype(np.int64),
          rng.uniform(-1, 1, 40))
    check_bits([(ts, k, v), b2], n_keys_hint=NK)


def test_two_level_group_edges():
    # 70,000 dense keys select RG_L1 + RG_L2_FOLD (klocs * nw = 137 * 2 >
    # 256, as in test_split_supertile_gpu.test_two_level_fold); keys j * 512
    # (bucket 0, kloc j < 256: one L2 block) carry the group-edge lengths
    rng = np.random.default_rng(4401)
    nk = 70_000
    ek = np.repeat(np.arange(len(EDGE_LENS)), EDGE_LENS) * 512
    rng.shuffle(ek)
    fill = rng.integers(0, nk, 6000)
    fill = fill[(fill & 511) != 0]
    k = np.concatenate([[nk - 1], ek, fill]).astype(np.int64)
    n = len(k)
    ts = (T0 + 990 + np.arange(n) * 20 // n).astype(np.int64)
    ts[1:1 + len(ek)] = T0 + 990        # the edge keys in one window
    v = rng.uniform(-50, 115, n)
    valid = (rng.random(n) > 0.15).astype(np.uint8)
    got, exp = check_bits([(ts, k, v)], valids=[valid], n_keys_hint=nk)
    assert ts[0] // 1000 != ts[-1] // 1000
    assert exp["key"].max() >= 65536


def test_variance_group_edges():
    b, valid = _null_cases()
    e = edge_batch(4501)
    e = (e[0] + 2000, e[1], e[2])  # varref wants non-decreasing timestamps
    batches, valids = [b, e], [valid, None]
    names = ["count", "var_samp", "var_pop", "stddev", "stddev_pop", "avg"]
    got, _ = run_gpu(1000, 0, batches, names=names, valids=valids,
                     n_keys_hint=NK)
    exp = run_oracle(1000, 0, batches, valids)
    assert_bits(got, exp, ["count", "avg"])
    ref = varref.expected(exp, batches, valids)
    for f in names:
        if f in varref.ALIASES:
            vals, msk = ref[varref.ALIASES[f]]
            assert np.array_equal(got[f + "_valid"], msk), f + " mask"
            m = msk.astype(bool)
            assert m.any()
            assert np.array_equal(got[f][m], vals[m]), f + " not bit-exact"


@pytest.mark.parametrize("ncols", [2, 3, 4])
def test_extra_columns_group_edges(ncols):
    # NX = 1 (double-buffered, groups of 8), NX = 2 and 3 (single-buffered,
    # groups of 4); each column has nulls of its own
    from denormalized_amd import WindowOp, _lib
    rng = np.random.default_rng(4600 + ncols)
    mb = []
    for ts, k, v in (edge_batch(4601), _null_cases()[0]):
        cols = [v] + [rng.uniform(-100, 100, len(ts)) * 10.0 ** j
                      for j in range(1, ncols)]
        valids = [rng.random(len(ts)) > 0.3 for _ in range(ncols)]
        mb.append((ts + (0 if not mb else 2000), k, cols, valids))
    aggs = []
    for j in range(ncols):
        aggs += [("count", j, f"n{j}"), ("min", j, f"lo{j}"),
                 ("max", j, f"hi{j}"), ("sum", j, f"sum{j}"),
                 ("avg", j, f"avg{j}")]
    op = WindowOp(length_ms=1000, slide_ms=0,
                  aggs=[(o, 2 + j, a) for o, j, a in aggs],
                  key_kind=_lib.KEY_DENSE_INT64, n_keys_hint=NK)
    order = mc.distinct_cols(aggs)
    outs, _ = _drive(op, [(ts, k, [cols[j] for j in order],
                           [mc.bitmap(valids[j]) for j in order])
                          for ts, k, cols, valids in mb])
    fields = ["key", "valid", "window_start", "window_end"]
    for _o, j, a in aggs:
        fields.append(a)
        if j != order[0]:
            fields.append(a + "_valid")
    got = {f: _cat(outs, f) for f in fields}
    exp = mc.expect(1000, 0, mb, aggs)
    assert len(exp["key"]) > 0
    mc.assert_match(got, exp, aggs)
