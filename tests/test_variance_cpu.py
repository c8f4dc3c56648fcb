"""CPU-side checks of the variance-family aggregates: the finalise rule the
engine's emission uses (dz_debug_var_finalize, pure host code) against the
pure-Python reference, and the Python name table."""
import ctypes
import math
import struct

import pytest

import __graft_entry__ as graft
from tests import varref


@pytest.fixture(scope="module")
def L():
    graft.build()
    from denormalized_amd import _lib
    return _lib.lib()


def _bits(x):
    return struct.pack("<d", x)


SUBNORMAL = 5e-324 * 3


@pytest.mark.parametrize("op", [5, 6, 7, 8])
@pytest.mark.parametrize("count", [0, 1, 2, 3])
@pytest.mark.parametrize("m2", [0.0, SUBNORMAL, math.nan, 2.5, math.inf])
def test_finalize_matches_reference(L, op, count, m2):
    out = ctypes.c_double(-1.0)
    ok = L.dz_debug_var_finalize(op, count, m2, ctypes.byref(out))
    exp_v, exp_ok = varref.finalize(op, count, m2)
    assert ok == exp_ok
    if exp_ok:
        if exp_v != exp_v:
            assert out.value != out.value
        else:
            assert _bits(out.value) == _bits(exp_v)


def test_finalize_null_rules(L):
    out = ctypes.c_double()
    # population forms: NULL only for the empty group
    assert L.dz_debug_var_finalize(6, 0, 1.0, ctypes.byref(out)) == 0
    assert L.dz_debug_var_finalize(6, 1, 0.0, ctypes.byref(out)) == 1
    assert out.value == 0.0
    assert L.dz_debug_var_finalize(8, 1, 0.0, ctypes.byref(out)) == 1
    # sample forms: NULL up to one row
    for op in (5, 7):
        assert L.dz_debug_var_finalize(op, 0, 1.0, ctypes.byref(out)) == 0
        assert L.dz_debug_var_finalize(op, 1, 1.0, ctypes.byref(out)) == 0
        assert L.dz_debug_var_finalize(op, 2, 1.0, ctypes.byref(out)) == 1
    assert L.dz_debug_var_finalize(5, 3, 8.0, ctypes.byref(out)) == 1
    assert out.value == 4.0
    assert L.dz_debug_var_finalize(7, 3, 8.0, ctypes.byref(out)) == 1
    assert out.value == 2.0
    assert L.dz_debug_var_finalize(6, 4, 8.0, ctypes.byref(out)) == 1
    assert out.value == 2.0


@pytest.mark.parametrize("op", [-1, 0, 1, 2, 3, 4, 9, 1 << 20])
def test_finalize_rejects_other_ops(L, op):
    out = ctypes.c_double()
    assert L.dz_debug_var_finalize(op, 3, 1.0, ctypes.byref(out)) == -1


def test_agg_by_name_aliases():
    from denormalized_amd import _lib
    for alias, canon in varref.ALIASES.items():
        assert _lib.AGG_BY_NAME[alias] == varref.OPS[canon], alias
    # var / stddev are the SAMPLE forms, as in the reference's functions.py
    assert _lib.AGG_BY_NAME["var"] == 5
    assert _lib.AGG_BY_NAME["stddev"] == 7
    # existing codes unchanged
    assert [_lib.AGG_BY_NAME[n] for n in
            ("count", "min", "max", "sum", "avg", "average")] == \
        [0, 1, 2, 3, 4, 4]


def test_out_batch_layout_appends_one_field():
    from denormalized_amd import _lib
    names = [f[0] for f in _lib.DzOutBatch._fields_]
    assert names[-1] == "agg_valid_cols"
    assert names[:-1] == ["n_rows", "key_i64", "key_offsets", "key_data",
                          "agg_cols", "agg_valid", "window_start_ms",
                          "window_end_ms"]
    assert _lib.DzOutBatch.agg_valid_cols.offset == 64


def test_merge_global_partials_rejects_variance():
    import numpy as np
    from denormalized_amd.distributed import merge_global_partials
    b = {"n_rows": 1, "count": np.array([2]), "valid": np.array([1], np.uint8),
         "window_start": np.array([0]), "window_end": np.array([1000]),
         "min": np.array([1.0]), "max": np.array([2.0]),
         "sum": np.array([3.0]), "var_samp": np.array([0.5]),
         "var_samp_valid": np.array([1], np.uint8)}
    with pytest.raises(ValueError, match="var_samp"):
        merge_global_partials([[b]])


def test_welford_reference_known_values():
    c, mean, m2 = varref.welford([2.0, 4.0, 4.0, 4.0, 5.0, 5.0, 7.0, 9.0])
    assert (c, mean, m2) == (8, 5.0, 32.0)
    assert varref.finalize("stddev_pop", c, m2) == (2.0, 1)
    assert varref.finalize("var_samp", 1, 0.0) == (0.0, 0)
