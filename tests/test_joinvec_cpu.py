"""CPU pins for tests/joinvec.py: the home-slot construction really lands on
the slot it names (checked against the hash as kernels.hip and oracle.c
compute it), and the patterns cover what their names say."""
import numpy as np
import pytest

from tests import joinvec as jv
from tests.test_join import PyJoin
from oracle.pyoracle import JoinOracle


def u64_hash(trips):
    """The hash as the device computes it: wrapping uint64 multiply."""
    with np.errstate(over="ignore"):
        return np.asarray(trips, np.int64).view(np.uint64) * np.uint64(jv.HASH_MUL)


def test_inverse_is_an_inverse():
    assert (jv.HASH_MUL * jv.HASH_INV) % 2 ** 64 == 1


@pytest.mark.parametrize("slots", [1 << 16, 1 << 20])
@pytest.mark.parametrize("slot", [0, 1, 1000, 65535])
def test_trips_with_home_land_on_their_slot(slot, slots):
    t = jv.trips_with_home(slot, 300, slots)
    assert t.dtype == np.int64 and len(set(t.tolist())) == 300
    assert jv.I64_MIN not in t.tolist()
    assert np.all(u64_hash(t) & np.uint64(slots - 1) == np.uint64(slot))
    assert all(jv.home_slot(x, slots) == slot for x in t.tolist())
    # disjoint ranges give disjoint trips
    t2 = jv.trips_with_home(slot, 50, slots, first=301)
    assert not set(t.tolist()) & set(t2.tolist())


def test_special_ids_hash_like_the_device():
    for t in (0, -1, jv.I64_MAX, jv.I64_MIN + 1, jv.I64_MIN):
        assert jv.jhash(t) == int(u64_hash([t])[0])


def test_geometry_edges():
    assert jv.geometry(1) == (1, 1)
    assert jv.geometry(8192) == (1, 8192)
    assert jv.geometry(8193) == (2, 4097)       # chunk starts off a 64 edge
    assert jv.geometry(16385) == (3, 5462)
    C, chunk = jv.geometry(512 * 8192 + 513)    # C capped
    assert C == 512 and chunk == 8194 and chunk % 64 != 0


@pytest.mark.parametrize("n", [8193, 3 * 8192 + 65])
def test_patterns(n):
    C, chunk = jv.geometry(n)
    assert jv.pattern("all", n).all() and not jv.pattern("none", n).any()
    ends = jv.pattern("chunk_ends", n)
    assert ends.sum() == 2 * C and ends[0] and ends[n - 1] and ends[chunk - 1]
    assert ends[chunk] and not ends[1]
    l0, l63 = jv.pattern("lane0", n), jv.pattern("lane63", n)
    assert l0[0] and l0[chunk] and l0[chunk + 64] and not (l0 & l63).any()
    assert l63[63] and l63[chunk + 63]
    r = jv.pattern("runs64", n)
    assert r[:64].all() and not r[64:128].any() and r[128]


def test_oracle_never_matches_the_reserved_probe_trip():
    """A probe row with trip INT64_MIN buffers like any absent trip in both
    restatements (the device must agree: tests/test_join_edges_gpu.py)."""
    oj, pj = JoinOracle(), PyJoin()
    for j in (oj, pj):
        j.push_build(np.array([1, 2], np.int64), np.array([7, 8], np.int64))
        j.push_probe(np.array([10, 11, 12], np.int64),
                     np.array([1, jv.I64_MIN, 2], np.int64),
                     np.array([0.5, 1.5, 2.5]))
    ts, drv, _ = oj.fetch()
    assert ts.tolist() == [10, 12] and drv.tolist() == [7, 8]
    assert [(a, d) for a, d, _ in pj.out] == [(10, 7), (12, 8)]
    assert oj.unmatched == 1 and len(pj.un) == 1
    oj.close()
