"""CPU checks of the median reference (tests/medianref.py) and of the Python
surface that needs no GPU: the op code, the merge refusal."""
import math
import random
import statistics
import struct

import numpy as np
import pytest

from tests import medianref


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


NEG_NAN = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
POS_NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]


def test_reference_matches_statistics_median():
    rng = random.Random(5)
    for n in range(1, 65):
        v = [rng.uniform(-1e6, 1e6) for _ in range(n)]
        got, valid = medianref.median(v)
        assert valid == 1
        assert got == statistics.median(v), n


def test_reference_ignores_row_order():
    rng = random.Random(6)
    v = [rng.gauss(0, 1) for _ in range(33)]
    a = medianref.median(v)
    rng.shuffle(v)
    assert medianref.median(v) == a


def test_hand_vectors():
    assert medianref.median([NEG_NAN, 1.0, 2.0]) == (1.0, 1)
    assert medianref.median([POS_NAN, 1.0, 2.0]) == (2.0, 1)
    v, valid = medianref.median([-0.0, 0.0])
    assert valid == 1 and _bits(v) == _bits(0.0)
    v, valid = medianref.median([-math.inf, math.inf])
    assert valid == 1 and math.isnan(v)
    assert medianref.median([1e308, 1e308]) == (math.inf, 1)
    assert medianref.median([]) == (0.0, 0)


def test_total_order_key_orders_the_special_values():
    v = [NEG_NAN, -math.inf, -1.0, -0.0, 0.0, 1.0, math.inf, POS_NAN]
    k = medianref.total_order_key(np.array(v))
    assert np.all(np.diff(k.astype(object)) > 0)


def test_agg_code():
    from denormalized_amd import _lib
    assert _lib.AGG_BY_NAME["median"] == 16
    assert _lib.AGG_MEDIAN == 16
    assert _lib.AGG_MEDIAN not in _lib.VAR_AGGS


def test_merge_global_partials_rejects_median():
    from denormalized_amd.distributed import merge_global_partials
    b = {"n_rows": 1, "count": np.array([2]), "valid": np.array([1], np.uint8),
         "window_start": np.array([0]), "window_end": np.array([1000]),
         "min": np.array([1.0]), "max": np.array([2.0]),
         "avg": np.array([1.5]), "median": np.array([1.5])}
    with pytest.raises(ValueError, match="median"):
        merge_global_partials([[b]])
