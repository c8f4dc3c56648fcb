"""GPU tests of the single-read supertile loop in the tumbling scatter
(k_scatter_t<false>) and in the regroup/fold kernels: every row or record is
held in registers from its one load to its placement, the bin prefix is a wave
scan, and the next supertile's loads are in flight under the current one.

Every case is differential against the CPU oracle (oracle.pyoracle; the
variance columns against tests/varref.py, several value columns against
tests/multicolref.py) with np.array_equal — no tolerance anywhere. Shapes are
the smallest at which the loop can go wrong: wave-quarter and supertile edges
(a supertile is 2,048 rows, a wave's quarter at most 512 = 8 lane-strided
slots), one bucket or one bin taking everything, state carried over supertile
and batch boundaries, validity bits at the seams, each template instantiation,
and the launches that must still take the old scatter."""
import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import pyoracle
from tests import multicolref as mc
from tests import varref

pytestmark = pytest.mark.gpu

BASE = ["count", "min", "max", "sum", "avg"]
T0 = 1_000_000


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _cat(outs, f):
    arrs = [np.asarray(b[f]) for b in outs]
    return np.concatenate(arrs) if arrs else np.zeros(0)


def _drive(op, pushes):
    """Push, poll, finish; an op that reports an error fails the test (push
    and finish raise; finish reads the kernels' bounds-guard cells), and the
    op's error string must be empty afterwards."""
    outs = []
    for args in pushes:
        op.push(*args)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    msg = op._L.dz_last_error(op._h)
    stats = op.kernel_stats()
    op.close()
    assert not msg, msg
    return outs, stats


def run_gpu(len_ms, slide_ms, batches, names=BASE, valids=None, dense=True,
            n_keys_hint=64):
    from denormalized_amd import WindowOp, _lib
    op = WindowOp(length_ms=len_ms, slide_ms=slide_ms,
                  aggs=[(n, 0) for n in names],
                  key_kind=_lib.KEY_DENSE_INT64 if dense else _lib.KEY_INT64,
                  n_keys_hint=n_keys_hint)
    pushes = []
    for bi, (ts, k, v) in enumerate(batches):
        bm = None
        if valids is not None and valids[bi] is not None:
            bm = np.packbits(np.asarray(valids[bi], np.uint8),
                             bitorder="little")
        pushes.append((ts, k, v, bm))
    outs, stats = _drive(op, pushes)
    fields = ["key", "valid", "window_start", "window_end"] + list(names) + \
        [n + "_valid" for n in names if n in varref.ALIASES]
    return {f: _cat(outs, f) for f in fields}, stats


def run_oracle(len_ms, slide_ms, batches, valids=None):
    o = pyoracle.Oracle(len_ms, slide_ms)
    for bi, (ts, k, v) in enumerate(batches):
        vv = valids[bi] if valids is not None else None
        o.push(ts, k, v, None if vv is None else np.asarray(vv, np.uint8))
    o.finish()
    exp = o.fetch()
    o.close()
    return exp


def assert_same(got, exp, names=BASE):
    """Keys and order, windows, the validity mask, and every aggregate where
    the oracle defines it (count everywhere), all exact."""
    assert len(exp["key"]) > 0
    assert np.array_equal(got["key"], exp["key"]), "keys/order"
    assert np.array_equal(got["window_start"], exp["window_start"])
    assert np.array_equal(got["window_end"], exp["window_end"])
    assert np.array_equal(got["valid"], exp["valid"]), "validity"
    v = exp["valid"].astype(bool)
    for f in names:
        if f == "count":
            assert np.array_equal(got[f], exp[f]), f
        elif f in BASE:
            assert np.array_equal(got[f][v], exp[f][v]), f


def check(len_ms, slide_ms, batches, valids=None, **kw):
    got, stats = run_gpu(len_ms, slide_ms, batches, valids=valids, **kw)
    exp = run_oracle(len_ms, slide_ms, batches, valids)
    assert_same(got, exp)
    return got, exp, stats


def stream(seed, nbatches, rows, nkeys, rows_per_ms):
    return [pyoracle.gen(seed, T0, b * rows, rows, nkeys, rows_per_ms)
            for b in range(nbatches)]


# ------------------------------------------- quarter and supertile edges

@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 255, 257, 2047, 2048, 2049,
                               4097, 8193, 16385])
def test_quarter_and_supertile_edges(n):
    # empty wave quarters (n < 4), quarters that are no multiple of 64, a
    # last supertile of one record, exactly one full supertile; 8,193 and
    # 16,385 rows give 2 and 3 scatter chunks whose length is no multiple of
    # 2,048. The rate puts a window boundary inside every batch above 3 rows.
    check(1000, 0, stream(3100 + n, 1, n, 37, max(1, n // 1500)))


# ------------------------------------------------------- bucket extremes

def test_one_key_takes_everything():
    # one bucket, one bin: a single fold block walks 3 supertiles, the other
    # 511 have an empty region
    n = 5000
    ts = (T0 + np.arange(n) // 4).astype(np.int64)
    v = np.random.default_rng(3201).uniform(-50, 115, n)
    check(1000, 0, [(ts, np.full(n, 7, np.int64), v)])


def test_sparse_bins_700_keys():
    # most bins get 0-1 records per supertile; buckets 0..187 hold 2 keys
    rng = np.random.default_rng(3202)
    n = 3000
    ts = (T0 + np.arange(n) // 2).astype(np.int64)
    check(1000, 0, [(ts, rng.integers(0, 700, n), rng.uniform(0, 115, n))],
          n_keys_hint=700)


def test_one_bucket_distinct_bins():
    # dense ids k * 512: every row of every wave shares bucket 0 and differs
    # in kloc, so the scatter's same-bucket ballot is all-ones while the
    # fold's same-bin ballot separates 40 bins
    rng = np.random.default_rng(3203)
    n = 3000
    ts = (T0 + np.arange(n) // 2).astype(np.int64)
    k = (rng.integers(0, 40, n) * 512).astype(np.int64)
    check(1000, 0, [(ts, k, rng.uniform(0, 115, n))], n_keys_hint=40 * 512)


# ------------------------------------------------- prefetch carry-over

@pytest.fixture(scope="module")
def four_batches():
    """4 x 10,000 rows, 37 keys, 8 rows/ms: every batch is 5 supertiles in
    one scatter chunk and spans a window boundary."""
    batches = stream(3301, 4, 10_000, 37, 8)
    for b in batches:
        for a in b:
            a.setflags(write=False)
    return batches, run_oracle(1000, 0, batches)


def test_state_across_supertiles_and_batches(four_batches):
    batches, exp = four_batches
    got, _ = run_gpu(1000, 0, batches)
    # group order is first-seen order: it holds across supertile boundaries
    assert_same(got, exp)
    for ts, _k, _v in batches:
        assert ts[0] // 1000 != ts[-1] // 1000


# --------------------------------------------------------------- validity

def _mask(pattern, k, seed):
    n = len(k)
    valid = np.ones(n, np.uint8)
    if pattern == "third":
        valid[np.random.default_rng(seed).random(n) < 1 / 3] = 0
    elif pattern == "one_key":
        valid[k == 5] = 0
    else:  # the last row of supertile 0 and the first of supertile 1
        valid[2047:2049] = 0
    return valid


@pytest.mark.parametrize("pattern", ["third", "one_key", "seam"])
@pytest.mark.parametrize("n", [2049, 10_000])
def test_validity(n, pattern):
    batches = stream(3400 + n, 1, n, 37, 8)
    valids = [_mask(pattern, batches[0][1], 3401)]
    got, exp, _ = check(1000, 0, batches, valids=valids)
    if pattern == "one_key":  # an all-null group: count 0, everything NULL
        r = got["key"] == 5
        assert r.any() and not got["valid"][r].any()
        assert not got["count"][r].any()
    assert exp["valid"].any()


# ---------------------------------------------------------- instantiations

def test_variance_instantiation(four_batches):
    batches, exp = four_batches
    ref = varref.expected(exp, batches)
    names = ["count", "var_samp", "var_pop", "stddev", "stddev_pop", "avg"]
    got, _ = run_gpu(1000, 0, batches, names=names)
    assert_same(got, exp, names)
    for f in names:
        if f in varref.ALIASES:
            vals, msk = ref[varref.ALIASES[f]]
            assert np.array_equal(got[f + "_valid"], msk), f + " mask"
            m = msk.astype(bool)
            assert m.any()
            assert np.array_equal(got[f][m], vals[m]), f + " not bit-exact"


@pytest.mark.parametrize("ncols", [2, 4])
def test_extra_column_instantiations(four_batches, ncols):
    from denormalized_amd import WindowOp, _lib
    batches, _ = four_batches
    rng = np.random.default_rng(3500 + ncols)
    mb = []
    for ts, k, v in batches:
        cols = [v] + [rng.uniform(-100, 100, len(ts)) * 10.0 ** j
                      for j in range(1, ncols)]
        valids = [rng.random(len(ts)) > 0.2 for _ in range(ncols)]
        mb.append((ts, k, cols, valids))
    aggs = []
    for j in range(ncols):
        aggs += [("count", j, f"n{j}"), ("min", j, f"lo{j}"),
                 ("max", j, f"hi{j}"), ("sum", j, f"sum{j}"),
                 ("avg", j, f"avg{j}")]
    op = WindowOp(length_ms=1000, slide_ms=0,
                  aggs=[(o, 2 + j, a) for o, j, a in aggs],
                  key_kind=_lib.KEY_DENSE_INT64, n_keys_hint=64)
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


def test_two_level_fold():
    # 70,000 dense keys: klocs * nw = 137 * 2 > 256 per batch selects the
    # two-level split (RG_L1 + RG_L2_FOLD); 3 batches of 100,001 rows, 80
    # rows/ms, so every batch spans a window boundary and every segment ends
    # in a partial supertile
    rng = np.random.default_rng(3601)
    nb, rows, nk = 3, 100_001, 70_000
    n = nb * rows
    ts = (T0 + np.arange(n) // 80).astype(np.int64)
    k = rng.integers(0, nk, n)
    k[0] = nk - 1
    v = rng.uniform(0, 115, n)
    batches = [(ts[i * rows:(i + 1) * rows], k[i * rows:(i + 1) * rows],
                v[i * rows:(i + 1) * rows]) for i in range(nb)]
    valids = [(b[1] >= 50).astype(np.uint8) for b in batches]
    got, exp, _ = check(1000, 0, batches, valids=valids, n_keys_hint=nk)
    assert exp["key"].max() >= 65536
    for ts_b, _k, _v in batches:
        assert ts_b[0] // 1000 != ts_b[-1] // 1000


# ------------------------------------------- paths that keep the old scatter

def test_sliding_500_100_keeps_old_scatter():
    rng = np.random.default_rng(3701)
    n, nk = 30_000, 3_000
    ts = (T0 + np.arange(n)).astype(np.int64)  # 30 s: ~305 windows
    batches = [(ts, rng.integers(0, nk, n), rng.uniform(-20, 115, n))]
    got, exp, _ = check(500, 100, batches, dense=False, n_keys_hint=nk)
    assert len(np.unique(exp["window_start"])) > 256


def test_tumbling_subrange_split_keeps_old_scatter():
    # 300 tumbling windows in one batch: more than 256, so the batch is cut
    # into window subranges that run as sliding with slide == length
    rng = np.random.default_rng(3702)
    n, nk = 30_000, 3_000
    ts = (T0 + np.arange(n)).astype(np.int64)
    batches = [(ts, rng.integers(0, nk, n), rng.uniform(-20, 115, n))]
    got, exp, _ = check(100, 0, batches, dense=False, n_keys_hint=nk)
    assert len(np.unique(exp["window_start"])) > 256
