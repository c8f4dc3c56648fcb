"""CPU checks of the int64-value reference (tests/intref.py) and of the ABI /
Python surface of int64 value columns that needs no GPU."""
import os
import random
import re

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import intref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "denormalized_amd.h")
I64_MAX, I64_MIN = 2**63 - 1, -2**63


def _one_group(vals, valid=None):
    """One key, one 1 s window; returns the single emitted row as a dict."""
    n = len(vals)
    r = intref.run(1000, 0, [(np.full(n, 5000, np.int64),
                              np.zeros(n, np.int64),
                              np.array(vals, np.int64))],
                   None if valid is None else [np.array(valid, np.uint8)])
    assert len(r["key"]) == 1
    return {k: v[0] for k, v in r.items()}


# ------------------------------------------------------------ hand vectors

def test_sum_wraps_to_int64_min():
    assert intref.wrap_sum([I64_MAX, 1]) == I64_MIN
    row = _one_group([I64_MAX, 1])
    assert row["sum"] == I64_MIN and row["count"] == 2
    assert row["min"] == 1 and row["max"] == I64_MAX


def test_max_keeps_values_above_2_53_apart():
    row = _one_group([2**53, 2**53 + 1])
    assert row["max"] == 2**53 + 1 and row["min"] == 2**53
    # the f64 cast the default op applies cannot tell them apart
    assert float(2**53) == float(2**53 + 1)


def test_avg_is_cast_then_average():
    want = (float(2**53 + 1) + 1.0) / 2
    assert intref.avg([2**53 + 1, 1]) == want
    assert _one_group([2**53 + 1, 1])["avg"] == want


def test_all_null_group_is_invalid_with_count_zero():
    row = _one_group([7, -7, 9], valid=[0, 0, 0])
    assert row["valid"] == 0 and row["count"] == 0
    assert row["min"] == 0 and row["max"] == 0 and row["sum"] == 0
    for name in intref.VAR_NAMES:
        assert row[name + "_valid"] == 0


def test_variance_null_rules_and_values():
    one = _one_group([5])
    assert one["var_pop_valid"] == 1 and one["var_pop"] == 0.0
    assert one["var_samp_valid"] == 0 and one["stddev_samp_valid"] == 0
    two = _one_group([1, 3])
    assert two["var_samp"] == 2.0 and two["var_pop"] == 1.0
    assert two["stddev_pop"] == 1.0


# ------------------------------------------------------- property checks

def _to_i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >> 63 else x


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_min_max_sum_agree_with_bigint_mod_2_64(seed):
    rng = random.Random(seed)
    n, nk = 3000, 7
    pool = [I64_MAX, I64_MIN, 2**53, 2**53 + 1, -(2**53) - 1, 0, -1, 1]
    vals = [rng.choice(pool) if rng.random() < 0.3
            else rng.randrange(I64_MIN, I64_MAX + 1) for _ in range(n)]
    ts = [1_000_000 + i for i in range(n)]          # 3 windows of 1 s
    keys = [rng.randrange(nk) for _ in range(n)]
    ok = [1 if rng.random() < 0.9 else 0 for _ in range(n)]
    cut = n // 2 + 17                                # state carried over
    batches = [(ts[:cut], keys[:cut], np.array(vals[:cut], np.int64)),
               (ts[cut:], keys[cut:], np.array(vals[cut:], np.int64))]
    r = intref.run(1000, 0, batches, [ok[:cut], ok[cut:]])
    want = {}
    for t, k, v, o in zip(ts, keys, vals, ok):
        g = want.setdefault((t // 1000 * 1000, k), [])
        if o:
            g.append(v)
    assert len(r["key"]) == len(want)
    for i in range(len(r["key"])):
        g = want[(int(r["window_start"][i]), int(r["key"][i]))]
        assert r["count"][i] == len(g)
        if g:
            assert r["min"][i] == min(g) and r["max"][i] == max(g)
            assert r["sum"][i] == _to_i64(sum(g))
            s = 0.0
            for v in g:
                s += float(v)
            assert r["avg"][i] == s / len(g)
        else:
            assert r["valid"][i] == 0


def test_sliding_rows_land_in_every_containing_window():
    ts = np.arange(10_000, 10_600, 7, dtype=np.int64)
    vals = np.arange(len(ts), dtype=np.int64) - 40
    r = intref.run(500, 100, [(ts, np.zeros(len(ts), np.int64), vals)])
    for i in range(len(r["key"])):
        ws, we = int(r["window_start"][i]), int(r["window_end"][i])
        m = (ts >= ws) & (ts < we)
        assert we - ws == 500 and r["count"][i] == m.sum() > 0
        assert r["sum"][i] == int(vals[m].sum())


# ------------------------------------------------- ABI and Python surface

@pytest.fixture(scope="module")
def built():
    graft.build()
    from denormalized_amd import _lib
    return _lib.lib()


def test_setter_is_exported_and_named_in_the_header(built):
    src = open(HEADER).read()
    assert re.search(r"dz_status\s+dz_window_op_set_value_type\s*\(", src)
    assert re.search(r"DZ_VALUE_F64\s*=\s*0", src)
    assert re.search(r"DZ_VALUE_INT64\s*=\s*1", src)
    assert hasattr(built, "dz_window_op_set_value_type")
    from denormalized_amd import _lib
    assert (_lib.VALUE_F64, _lib.VALUE_INT64) == (0, 1)


def _partial(**cols):
    b = {"n_rows": 1, "count": np.array([2]), "valid": np.array([1], np.uint8),
         "window_start": np.array([0]), "window_end": np.array([1000]),
         "min": np.array([1.0]), "max": np.array([2.0]),
         "sum": np.array([3.0])}
    b.update(cols)
    return b


@pytest.mark.parametrize("col", ["min", "max", "sum"])
def test_merge_global_partials_refuses_integer_partials(col):
    from denormalized_amd.distributed import merge_global_partials
    b = _partial(**{col: np.array([2**53 + 1], np.int64)})
    with pytest.raises(ValueError, match="integer-typed.*" + col):
        merge_global_partials([[b]])
    # float partials merge as before
    out = merge_global_partials([[_partial()], [_partial()]])
    assert out[0]["count"] == 4 and out[0]["sum"] == 6.0


def test_int64_push_refuses_a_float_array_before_the_device(built):
    """No GPU here, so no op can be created: the refusal has to come before
    the first call into the engine."""
    from denormalized_amd import WindowOp, _lib
    assert _lib._value_array(np.array([1, 2], np.int32), "int64").dtype == \
        np.int64
    assert _lib._value_array([2**53 + 1], "int64")[0] == 2**53 + 1
    for bad in (np.array([1.0, 2.0]), [1.5], np.array([1, 2], np.float32)):
        with pytest.raises(TypeError, match="int64"):
            _lib._value_array(bad, "int64")
    # the default op casts integers to f64 exactly as before
    assert _lib._value_array(np.array([3], np.int64), "float64").dtype == \
        np.float64

    class _NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"engine call {name} before the type check")

    op = WindowOp.__new__(WindowOp)
    op._L, op._h = _NoEngine(), None
    op._by_col, op.no_group, op.value_dtype = False, False, "int64"
    op.key_kind = _lib.KEY_INT64
    with pytest.raises(TypeError, match="int64"):
        op.push(np.array([1000], np.int64), np.array([1], np.int64),
                np.array([1.0]))


def test_value_dtype_is_validated_before_create():
    from denormalized_amd import WindowOp
    with pytest.raises(ValueError, match="value_dtype"):
        WindowOp(length_ms=1000, value_dtype="int32")
