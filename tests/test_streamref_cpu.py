"""tests/streamref.py proved without a GPU: against the C oracle on seeded
fuzz streams with late rows and shuffled batches (count / min / max / sum /
avg bit for bit), against varref.expected and medianref.expected on the
time-sorted streams those helpers accept, against intref.run on int64 streams
with late rows, and against multicolref.expect on a two-column late stream.
CPU-only; every stream stays under 5,000 rows."""
import numpy as np
import pytest

from oracle import pyoracle
from tests import intref, medianref, multicolref, streamref, varref

T0 = 1_000_000
SPECIALS = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0])
# the last four: slide does not divide the snap unit (whole seconds for
# len >= 1000, multiples of len below), so every batch anchors its sliding
# grid at another phase and starts of several residues mod slide interleave
DRIFT = [(1000, 300), (700, 300), (1500, 400), (250, 100)]
SHAPES = [(1000, 0), (2000, 500), (250, 0), (500, 100)] + DRIFT


def fuzz_stream(seed, len_ms, mode, nb=6, n=500, nkeys=9, ints=False):
    """`nb` batches of `n` rows, each covering 1.5 windows and starting 1.2
    windows after the one before. mode "late": sorted batches; in every odd
    batch 5 % of the rows move back to before watermark - len_ms, into
    frames that have closed. mode "shuffled": every batch permuted. 15 %
    NULLs and the last key NULL everywhere; f64 values carry 4 % NaN / inf /
    -inf / +0 / -0."""
    rng = np.random.default_rng(seed)
    batches, valids, wm = [], [], None
    for b in range(nb):
        start = T0 + b * len_ms * 6 // 5
        ts = np.sort(start + rng.integers(0, len_ms * 3 // 2, n))
        if mode == "late" and b % 2 == 1 and wm - len_ms > T0:
            late = rng.random(n) < 0.05
            late[0] = True
            ts[late] = rng.integers(T0, wm - len_ms, int(late.sum()))
        elif mode == "shuffled":
            ts = rng.permutation(ts)
        ts = ts.astype(np.int64)
        keys = rng.integers(0, nkeys, n).astype(np.int64)
        if ints:
            vals = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64,
                                endpoint=True)
            vals[::4] = 2**53 + rng.integers(-5, 6, len(vals[::4]))
        else:
            vals = rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-6, 7, n)
            sp = rng.random(n) < 0.04
            vals[sp] = rng.choice(SPECIALS, int(sp.sum()))
        mn = int(ts.min())
        wm = mn if wm is None or wm <= mn else wm
        batches.append((ts, keys, vals))
        valid = (rng.random(n) > 0.15).astype(np.uint8)
        valid[keys == nkeys - 1] = 0      # one key is NULL everywhere
        valids.append(valid)
    return batches, valids


def run_oracle(len_ms, slide_ms, batches, valids=None):
    o = pyoracle.Oracle(len_ms, slide_ms)
    for bi, (ts, k, v) in enumerate(batches):
        o.push(ts, k, v, None if valids is None else valids[bi])
    o.finish()
    exp = o.fetch()
    o.close()
    return exp


def assert_bits(got, exp, field, mask):
    """f64 columns on their bit patterns where the mask is 1; NaN is compared
    by position."""
    m = mask.astype(bool)
    g = np.ascontiguousarray(got[field][m], np.float64)
    e = np.ascontiguousarray(exp[field][m], np.float64)
    nan = np.isnan(e)
    assert np.array_equal(np.isnan(g), nan), field + " NaN positions"
    assert np.array_equal(g[~nan].view(np.uint64), e[~nan].view(np.uint64)), \
        field + " bits"


# ------------------------------------------------------- against the C oracle

@pytest.mark.parametrize("mode", ["late", "shuffled"])
@pytest.mark.parametrize("len_ms,slide_ms", SHAPES)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_matches_c_oracle(seed, len_ms, slide_ms, mode):
    batches, valids = fuzz_stream(seed * 100 + len_ms % 97, len_ms, mode)
    assert sum(len(b[0]) for b in batches) <= 5000
    exp = run_oracle(len_ms, slide_ms, batches, valids)
    got = streamref.run(len_ms, slide_ms, batches, valids).fetch()
    assert len(exp["key"]) > 0
    for f in ("key", "window_start", "window_end", "count", "valid"):
        assert np.array_equal(got[f], exp[f]), f
    for f in ("min", "max", "sum", "avg"):
        assert_bits(got, exp, f, exp["valid"])
    v = exp["valid"].astype(bool)
    assert (~v).any() and np.isnan(exp["sum"][v]).any()
    assert np.isinf(exp["max"][v]).any()
    if mode == "late":
        # the oracle really re-created a closed frame and emitted it again
        assert len(streamref.twice(exp)) >= 1
    else:
        assert all(np.any(np.diff(b[0]) < 0) for b in batches)


def test_signed_zero_and_leading_nan_pins():
    """sum starts from +0.0, min/max keep the first of two equal zeros, a
    leading NaN sticks in min/max: the oracle's rules, bit for bit."""
    ts = np.full(9, T0, np.int64)
    keys = np.array([0, 0, 1, 1, 2, 2, 2, 3, 3], np.int64)
    vals = np.array([-0.0, 0.0, 0.0, -0.0, np.nan, 1.0, -1.0, -0.0, -0.0])
    exp = run_oracle(1000, 0, [(ts, keys, vals)])
    got = streamref.run(1000, 0, [(ts, keys, vals)]).fetch()
    for f in ("min", "max", "sum", "avg"):
        assert_bits(got, exp, f, exp["valid"])
    assert np.signbit(got["min"][0]) and not np.signbit(got["min"][1])
    assert np.isnan(got["min"][2]) and np.isnan(got["max"][2])
    assert not np.signbit(got["sum"][3])


# ------------------------------------------------- the sliding grid's phase

def test_sliding_grid_phase_drifts_between_batches():
    """A batch's sliding grid is anchored at snap(min_ts - len). For
    (1000, 300) the snap is to whole seconds, which 300 does not divide: two
    batches whose minima lie in different seconds get starts of different
    residues mod 300, and the engine's host window list says the same."""
    import ctypes

    import __graft_entry__ as graft
    from tests.pyref import windows_for_range
    graft.build()
    from denormalized_amd import _lib
    L = _lib.lib()
    ws, we = np.empty(64, np.int64), np.empty(64, np.int64)
    residues = []
    for mn in (T0 + 137, T0 + 1237):
        mx = mn + 1399
        exp = windows_for_range(mn, mx, 1000, 300)
        n = L.dz_debug_windows_for_range(
            mn, mx, 1000, 300, ws.ctypes.data_as(ctypes.c_void_p),
            we.ctypes.data_as(ctypes.c_void_p), 64)
        assert n == len(exp) > 0
        assert ws[:n].tolist() == [s for s, _e in exp]
        assert we[:n].tolist() == [e for _s, e in exp]
        anchor = (mn - 1000) // 1000 * 1000
        assert all((s - anchor) % 300 == 0 for s, _e in exp)
        res = {s % 300 for s, _e in exp}
        assert len(res) == 1
        residues.append(res.pop())
    assert residues[0] != residues[1]


# ------------------------------------------- against varref and medianref

@pytest.mark.parametrize("len_ms,slide_ms", [(1000, 0), (500, 100)] + DRIFT)
def test_matches_varref_and_medianref_on_sorted_streams(len_ms, slide_ms):
    rng = np.random.default_rng(41 + len_ms)
    n = 4500
    ts = T0 + np.sort(rng.integers(0, 4 * len_ms, n)).astype(np.int64)
    keys = rng.integers(0, 11, n).astype(np.int64)
    keys[-3:] = [100, 101, 101]           # one-row, two-row groups
    vals = rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-6, 7, n)
    valid = (rng.random(n) > 0.2).astype(np.uint8)
    valid[-3:] = 1
    valid[keys == 7] = 0                  # a key that is NULL everywhere
    cuts = [0, 1300, 2900, n]
    batches = [(ts[a:b], keys[a:b], vals[a:b])
               for a, b in zip(cuts[:-1], cuts[1:])]
    valids = [valid[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    exp = run_oracle(len_ms, slide_ms, batches, valids)
    got = streamref.run(len_ms, slide_ms, batches, valids).fetch()
    assert np.array_equal(got["key"], exp["key"])
    assert np.array_equal(got["window_start"], exp["window_start"])
    var = varref.expected(exp, batches, valids, slide_ms)
    for name in varref.OPS:
        vals_, msk = var[name]
        assert np.array_equal(got[name + "_valid"], msk), name
        assert 0 < msk.sum() < len(msk), name
        assert np.array_equal(got[name].view(np.uint64),
                              vals_.view(np.uint64)), name
    mvals, mmask = medianref.expected(exp, batches, valids, slide_ms)
    assert np.array_equal(got["valid"], mmask)
    assert np.array_equal(got["median"].view(np.uint64),
                          mvals.view(np.uint64))


def test_median_of_specials_matches_medianref():
    groups = [[-0.0, 0.0], [-np.inf, np.inf], [1e308, 1e308],
              [0.0, -0.0, -0.0], [np.nan, 1.0, 2.0]]
    keys = np.concatenate([np.full(len(g), i) for i, g in enumerate(groups)])
    vals = np.concatenate(groups)
    batches = [(np.full(len(keys), T0, np.int64), keys.astype(np.int64), vals)]
    exp = run_oracle(1000, 0, batches)
    got = streamref.run(1000, 0, batches).fetch()
    mvals, _ = medianref.expected(exp, batches)
    nan = np.isnan(mvals)
    assert nan.sum() == 1 and np.array_equal(np.isnan(got["median"]), nan)
    assert np.array_equal(got["median"][~nan].view(np.uint64),
                          mvals[~nan].view(np.uint64))


# ----------------------------------------------------------- against intref

@pytest.mark.parametrize("mode", ["late", "shuffled"])
@pytest.mark.parametrize("len_ms,slide_ms", [(1000, 0), (500, 100)] + DRIFT)
@pytest.mark.parametrize("no_group", [False, True])
def test_matches_intref_on_int64_streams(len_ms, slide_ms, mode, no_group):
    batches, valids = fuzz_stream(77 + len_ms, len_ms, mode, ints=True)
    ref = intref.run(len_ms, slide_ms, batches, valids, no_group=no_group)
    got = streamref.run(len_ms, slide_ms, batches, valids, dtype="int64",
                        no_group=no_group).fetch()
    assert set(ref) <= set(got) and len(ref["key"]) > 0
    for f, e in ref.items():
        g = got[f]
        assert g.dtype == e.dtype, f
        if e.dtype == np.float64:
            assert np.array_equal(g.view(np.uint64), e.view(np.uint64)), f
        else:
            assert np.array_equal(g, e), f
    if mode == "late":
        assert len(streamref.twice(ref)) >= 1


# ------------------------------------------------------ against multicolref

def test_two_columns_match_multicolref_on_a_late_stream():
    b1, v1 = fuzz_stream(91, 1000, "late")
    b2, v2 = fuzz_stream(92, 1000, "late")   # other values, other NULLs
    mb = [(a[0], a[1], [a[2], b[2]], [va.astype(bool), vb.astype(bool)])
          for a, b, va, vb in zip(b1, b2, v1, v2)]
    aggs = [("count", 0, "n0"), ("min", 0, "lo0"), ("max", 1, "hi1"),
            ("avg", 1, "avg1"), ("sum", 1, "sum1"), ("count", 1, "n1")]
    exp = multicolref.expect(1000, 0, mb, aggs)
    ref = streamref.run(1000, 0, [(t, k, c) for t, k, c, _ in mb],
                        [v for _t, _k, _c, v in mb])
    per = {j: ref.fetch(j) for j in (0, 1)}
    got = {f: per[0][f] for f in ("key", "window_start", "window_end",
                                  "valid")}
    for op, j, alias in aggs:
        got[alias] = per[j][op]
        got[alias + "_valid"] = (np.ones_like(per[j]["valid"])
                                 if op == "count" else per[j]["valid"])
    multicolref.assert_match(got, exp, aggs, nan_payload_free=True)
    assert len(streamref.twice(exp)) >= 1


# ---------------------------------------------------------- the filter helper

def test_filter_helper_null_never_passes():
    ts = np.full(6, T0, np.int64)
    keys = np.array([0, 0, 1, 2, 2, 2], np.int64)
    vals = np.array([1.0, 3.0, 9.0, 5.0, 5.0, 5.0])
    valid = np.array([1, 1, 0, 1, 1, 1], np.uint8)
    cols = streamref.run(1000, 0, [(ts, keys, vals)], [valid]).fetch()
    kept, keep = streamref.filter_rows(cols, "median", "<=", 5.0)
    assert keep.tolist() == [True, False, True]      # key 1 is NULL: 0.0 <= 5
    assert kept["key"].tolist() == [0, 2]
    _, keep = streamref.filter_rows(cols, "stddev_samp", "==", 0.0)
    assert keep.tolist() == [False, False, True]
    _, keep = streamref.filter_rows(cols, "count", "<", 1.0)
    assert keep.tolist() == [False, True, False]     # count is never NULL
