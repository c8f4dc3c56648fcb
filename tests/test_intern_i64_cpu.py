"""CPU checks of what tests/test_intern_i64_gpu.py relies on: the Python
restatement of the int64 intern's hash, the home-slot key search, the Stream
helper's expectations, and the Python entry point."""
import numpy as np

from tests import i64vec as iv
from tests.pyref import PyRef

GOLDEN = 0x9E3779B97F4A7C15


def test_splitmix64_published_vectors():
    # the first three outputs of the published SplitMix64 generator seeded
    # with 0 (Steele/Lea/Flood; the xoshiro seeding reference): output n is
    # the mix of n * GOLDEN, i.e. this function applied to (n - 1) * GOLDEN
    assert iv.splitmix64(0) == 0xE220A8397B1DCDAF
    assert iv.splitmix64(GOLDEN) == 0x6E789E6AA1B965F4
    assert iv.splitmix64((2 * GOLDEN) & iv.M64) == 0x06C45D188009454F


def test_home_slot_scalar_and_vector_forms_agree():
    keys = np.concatenate([np.array(iv.SPECIALS, np.int64),
                           iv.sparse_values(500, 3)])
    for P, bits in ((iv.P_MIN, 64), (iv.P_MIN, 4), (iv.P_MIN, 1),
                    (1 << 20, 64)):
        vec = iv.home_slots(keys, P, bits)
        assert vec.tolist() == [iv.home_slot(k, P, bits) for k in keys]
        assert vec.min() >= 0 and vec.max() < min(P, 1 << bits)
    # negative keys hash as their two's-complement u64
    assert iv.home_slot(-1) == iv.splitmix64(iv.M64) & (iv.P_MIN - 1)


def test_home_slot_search_is_deterministic():
    P = iv.P_MIN
    a = iv.keys_with_home((P - 2, P - 1), 3, seed=77)
    b = iv.keys_with_home((P - 2, P - 1), 3, seed=77)
    assert a == b
    for slot in (P - 2, P - 1):
        assert len(a[slot]) == 3 and len(set(a[slot])) == 3
        assert all(iv.home_slot(k, P) == slot for k in a[slot])
        assert 0 not in a[slot]


def test_stream_helper_agrees_with_pyref():
    values = np.concatenate([np.array(iv.SPECIALS[:6], np.int64),
                             iv.sparse_values(6, 5)])
    n = len(values)
    introduce = [b % 3 for b in range(n)]
    s = iv.Stream(values, iv.growing_batches(n, introduce, 3, 700, 6), seed=7,
                  rows_per_ms=1)
    ref = PyRef(1000, 0)
    for ts, _kid, keys, v in s.batches:
        ref.push(ts.tolist(), keys.tolist(), v.tolist())
    ref.finish()
    exp = s.exp
    assert len(ref.out) == len(exp["key"]) > n
    assert [r[0] for r in ref.out] == values[exp["key"]].tolist()
    assert [r[1] for r in ref.out] == exp["count"].tolist()
    for col, name in ((2, "min"), (3, "max"), (4, "avg")):
        assert [r[col] for r in ref.out] == exp[name].tolist(), name
    assert [r[6] for r in ref.out] == exp["valid"].tolist()
    assert [r[7] for r in ref.out] == exp["window_start"].tolist()
    assert [r[8] for r in ref.out] == exp["window_end"].tolist()


def test_python_entry_exists():
    from denormalized_amd import WindowOp
    assert callable(getattr(WindowOp, "push_device_i64"))
