"""CPU-side checks for aggregates over several value columns: the expectation
helper against the independent pure-Python restatement, the shapes
DataStream.window accepts and refuses, and the create-time refusals that need
no device."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import multicolref, pyref


def _small_stream():
    rng = np.random.default_rng(11)
    batches = []
    for b in range(3):
        n = 157
        ts = (1_000_000 + b * 700 + rng.integers(0, 1200, n)).astype(np.int64)
        keys = rng.integers(0, 7, n).astype(np.int64)
        cols = [rng.uniform(-50, 50, n), rng.uniform(0, 1e6, n),
                rng.uniform(-1, 1, n)]
        valids = [rng.random(n) > 0.2, rng.random(n) > 0.6, None]
        # one key NULL throughout in column 1, valid in column 0
        valids[1] &= keys != 3
        valids[0] |= keys == 3
        batches.append((ts, keys, cols, valids))
    return batches


class _PyRefOracle:
    """pyref.PyRef behind the Oracle's push/finish/fetch/close surface."""

    def __init__(self, len_ms, slide_ms):
        self._r = pyref.PyRef(len_ms, slide_ms)

    def push(self, ts, keys, vals, valid=None):
        self._r.push([int(t) for t in ts], [int(k) for k in keys],
                     [float(v) for v in vals],
                     None if valid is None else [bool(x) for x in valid])

    def finish(self):
        self._r.finish()

    def fetch(self):
        rows = self._r.out
        names = ("key", "count", "min", "max", "avg", "sum", "valid",
                 "window_start", "window_end")
        types = (np.int64, np.int64, np.float64, np.float64, np.float64,
                 np.float64, np.uint8, np.int64, np.int64)
        return {nm: np.array([r[i] for r in rows], tp)
                for i, (nm, tp) in enumerate(zip(names, types))}

    def close(self):
        pass


@pytest.mark.parametrize("slide", [0, 250])
def test_helper_matches_pyref(slide):
    graft.build()  # the C oracle
    batches = _small_stream()
    aggs = [("max", 1, "hi"), ("min", 0, "lo"), ("count", 2, "n2"),
            ("avg", 1, "mean1"), ("sum", 0, "tot0"), ("count", 1, "n1")]
    exp = multicolref.expect(1000, slide, batches, aggs)
    ref = multicolref.expect(1000, slide, batches, aggs,
                             make=lambda: _PyRefOracle(1000, slide))
    assert len(exp["key"]) > 10
    assert set(exp) == set(ref)
    for k in exp:
        assert np.array_equal(exp[k], ref[k]), k
    # per-column NULLs really differ: key 3 is NULL in column 1 only
    k3 = exp["key"] == 3
    assert k3.any()
    # (column 1 comes first in aggs, so it is the primary: "valid" is its mask)
    assert not exp["hi_valid"][k3].any() and exp["lo_valid"][k3].all()
    assert np.array_equal(exp["valid"], exp["hi_valid"])
    assert (exp["n1"][k3] == 0).all() and (exp["n2"][k3] > 0).all()
    assert exp["n1_valid"].all()  # count is never NULL


def test_helper_filter_null_never_passes():
    graft.build()
    batches = _small_stream()
    aggs = [("min", 0, "lo"), ("max", 1, "hi")]
    full = multicolref.expect(1000, 0, batches, aggs)
    for cmp in multicolref.CMP:
        f = multicolref.expect(1000, 0, batches, aggs, filt=("hi", cmp, 5e5))
        assert f["hi_valid"].all()
        assert not (f["key"] == 3).any()
        assert len(f["key"]) < len(full["key"])


def _ds():
    import denormalized_amd as dz
    return dz.Context(device=0).from_batches(
        [], ts_col="t", key_col="k", key_kind=dz._lib.KEY_INT64)


def test_window_accepts_several_columns_and_aliases():
    ds = _ds().window(["k"], [("min", "temp"), ("avg", "hum"),
                              ("count", "hum"), ("max", "temp", "tmax")],
                      1000)
    w = ds._window
    assert w["value_cols"] == ["temp", "hum"]
    assert w["names"] == ["min", "avg", "count", "tmax"]
    # one column, no alias: today's shape, untouched
    w1 = _ds().window(["k"], [("min", "v"), ("min", "v")], 1000)._window
    assert w1["value_cols"] == ["v"] and w1["names"] == ["min", "min"]
    # four distinct columns is the limit and is accepted
    _ds().window(["k"], [("min", c) for c in "abcd"][:1] +
                 [("max", "b"), ("sum", "c"), ("avg", "d")], 1000)


def test_window_refuses_alias_collisions():
    with pytest.raises(ValueError, match="collide"):
        _ds().window(["k"], [("min", "a"), ("min", "b")], 1000)
    with pytest.raises(ValueError, match="collide"):
        _ds().window(["k"], [("min", "a", "x"), ("max", "b", "x")], 1000)
    with pytest.raises(ValueError, match="collide"):
        _ds().window(["k"], [("min", "a", "max"), ("max", "a")], 1000)
    # distinct aliases make the same op on two columns legal
    _ds().window(["k"], [("min", "a", "amin"), ("min", "b", "bmin")], 1000)


def test_window_refuses_more_than_four_columns():
    aggs = [("sum", c, "s_" + c) for c in "abcde"]
    with pytest.raises(ValueError, match="at most 4"):
        _ds().window(["k"], aggs, 1000)
    with pytest.raises(ValueError, match=r"\(op, col\)"):
        _ds().window(["k"], [("sum",)], 1000)


def test_filter_names_follow_aliases():
    ds = _ds().window(["k"], [("min", "a", "amin"), ("max", "b", "bmax")],
                      1000).filter("nope", ">", 1.0)
    with pytest.raises((ValueError, RuntimeError)):
        ds._make_op()


def test_create_refusals_need_no_device():
    """More than 4 distinct columns, and variance with 2 columns, are refused
    by dz_window_op_create before it looks for a device, one message each."""
    graft.build()
    from denormalized_amd import _lib
    L = _lib.lib()

    def create(aggs):
        arr = (_lib.DzAggDesc * len(aggs))()
        for i, (op, col) in enumerate(aggs):
            arr[i].op, arr[i].input_col = op, col
        d = _lib.DzWindowDesc(
            window_type=0, length_ms=1000, slide_ms=0, ts_col=0, group_col=1,
            key_kind=_lib.KEY_INT64,
            aggs=ctypes.cast(arr, ctypes.POINTER(_lib.DzAggDesc)),
            n_aggs=len(aggs), n_keys_hint=16, device=0, max_open_windows=0)
        h = L.dz_window_op_create(ctypes.byref(d))
        msg = L.dz_last_error(None)
        if h:
            L.dz_window_op_destroy(h)
        return h, (msg or b"").decode()

    h, msg = create([(_lib.AGG_SUM, c) for c in (2, 3, 4, 5, 6)])
    assert not h and "distinct input columns" in msg
    h, msg = create([(_lib.AGG_VAR_POP, 2), (_lib.AGG_MIN, 3)])
    assert not h and "variance" in msg and "single input column" in msg


def test_merge_global_partials_refuses_multicolumn():
    from denormalized_amd import distributed
    b = {"n_rows": 1, "count": np.array([1]), "min": np.array([1.0]),
         "max": np.array([1.0]), "sum": np.array([1.0]),
         "valid": np.array([1], np.uint8), "window_start": np.array([0]),
         "window_end": np.array([1000]), "hmax": np.array([2.0]),
         "hmax_valid": np.array([1], np.uint8)}
    with pytest.raises(ValueError, match="multi-column"):
        distributed.merge_global_partials([[b]])
