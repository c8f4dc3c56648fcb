"""Join operator edge cases: dz_join_op vs oracle.c's restatement
(JoinOracle) and, as a second reference, tests/test_join.py::PyJoin, on the
same pushes. After EVERY push: n, ts, kid and value bits of the matches and
the unmatched count are compared bit for bit; no tolerance anywhere. Every
expectation comes from the references, never from the device. The table is
never filled past half in any test."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle.pyoracle import JoinOracle, Oracle
from tests import joinvec as jv
from tests.test_join import PyJoin

pytestmark = pytest.mark.gpu

REFUSALS = ("capacity", "reserved trip id", "driver id outside")
PY_MAX_ROWS = 200_000  # PyJoin is a Python loop: skipped for the one big case


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def d2h(ptr, n, dtype):
    from denormalized_amd import _lib
    out = np.empty(n, dtype)
    if n:
        st = _lib.lib().dz_memcpy_d2h(
            out.ctypes.data_as(ctypes.c_void_p), ptr, out.nbytes)
        if st != 0:
            pytest.exit("d2h of a join output failed, stopping", returncode=3)
    return out


def read_cols(n, pts, pkid, pval):
    return (d2h(pts, n, np.int64), d2h(pkid, n, np.int32),
            d2h(pval, n, np.float64))


def same_cols(a, b):
    return (np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and
            np.array_equal(a[2].view(np.int64), b[2].view(np.int64)))


class Rig:
    """One device join and both references fed the same pushes."""

    def __init__(self, hint, py=True):
        from denormalized_amd import JoinOp
        self.jo = JoinOp(device=0, n_trips_hint=hint)
        self.oj = JoinOracle()
        self.py = PyJoin() if py else None
        self.py_seen = 0

    def _dev(self, a, dt):
        from denormalized_amd import DeviceArray
        a = np.ascontiguousarray(a, dt)
        d = DeviceArray(0, max(8, a.nbytes))
        d.from_host(a)
        return d

    def _call(self, fn, *arrs):
        """Device push. Inputs are free once it returns (pushes end with a
        stream sync). A HIP runtime error (not one of the documented
        refusals) ends the session instead of running more GPU work."""
        try:
            fn(*[a.ptr for a in arrs])
        except RuntimeError as e:
            if not any(m in str(e) for m in REFUSALS):
                pytest.exit(f"device error, stopping: {e}", returncode=3)
            raise
        finally:
            for a in arrs:
                a.free()

    def build_device_only(self, trips, drivers):
        n = len(trips)
        self._call(lambda t, d: self.jo.push_build(n, t, d),
                   self._dev(trips, np.int64), self._dev(drivers, np.int64))

    def build(self, trips, drivers):
        trips = np.asarray(trips, np.int64)
        drivers = np.asarray(drivers, np.int64)
        self.build_device_only(trips, drivers)
        self.refs_build(trips, drivers)
        return self.check()

    def refs_build(self, trips, drivers):
        self.oj.push_build(trips, drivers)
        if self.py:
            self.py.push_build(trips.tolist(), drivers.tolist())

    def probe(self, ts, trips, vals):
        ts = np.asarray(ts, np.int64)
        trips = np.asarray(trips, np.int64)
        vals = np.asarray(vals, np.float64)
        n = len(ts)
        self._call(lambda a, t, v: self.jo.push_probe(n, a, t, v),
                   self._dev(ts, np.int64), self._dev(trips, np.int64),
                   self._dev(vals, np.float64))
        self.oj.push_probe(ts, trips, vals)
        if self.py:
            self.py.push_probe(ts.tolist(), trips.tolist(), vals.tolist())
        return self.check()

    def check(self):
        """Compare the last push's matches and the unmatched count with both
        references; returns the device columns and pointers."""
        n, pts, pkid, pval = self.jo.matches()
        ets, edrv, eval_ = self.oj.fetch()
        assert n == len(ets), (n, len(ets))
        got = read_cols(n, pts, pkid, pval)
        bad = np.flatnonzero(got[0] != ets)
        assert bad.size == 0, ("ts", bad[:5], got[0][bad[:5]], ets[bad[:5]])
        bad = np.flatnonzero(got[1].astype(np.int64) != edrv)
        assert bad.size == 0, ("kid", bad[:5], got[1][bad[:5]], edrv[bad[:5]])
        bad = np.flatnonzero(got[2].view(np.int64) != eval_.view(np.int64))
        assert bad.size == 0, ("val", bad[:5], got[2][bad[:5]], eval_[bad[:5]])
        assert self.jo.unmatched == self.oj.unmatched
        if self.py:
            new = self.py.out[self.py_seen:]
            self.py_seen = len(self.py.out)
            assert len(new) == n
            if n:
                pts_, pdrv, pv = (np.array(c) for c in zip(*new))
                assert np.array_equal(pts_.astype(np.int64), got[0])
                assert np.array_equal(pdrv.astype(np.int64),
                                      got[1].astype(np.int64))
                assert np.array_equal(pv.astype(np.float64).view(np.int64),
                                      got[2].view(np.int64))
            assert self.jo.unmatched == len(self.py.un)
        return got, (n, pts, pkid, pval)

    def close(self):
        self.jo.close()
        self.oj.close()


@pytest.fixture
def rig_factory():
    rigs = []

    def make(hint, py=True):
        rigs.append(Rig(hint, py))
        return rigs[-1]

    yield make
    for r in rigs:
        r.close()


def rows(rng, n, t0=1_000_000):
    return rng.integers(t0, t0 + 50_000, n), rng.uniform(0, 115, n)


# ---- 1. row counts at geometry edges -----------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65, 8191, 8192, 8193, 16385,
                               512 * 8192 + 513])
def test_row_counts_at_geometry_edges(rig_factory, n):
    """C = min(512, ceil(n/8192)), chunk = ceil(n/C), 64-lane ballot groups:
    one row, either side of a ballot group, either side of one chunk, chunks
    that start off a 64 boundary (8193: chunk 4097), three chunks, and the C
    cap with a chunk that is no multiple of 64. About half the rows match;
    the other half is then released by a build, so the re-probe walks the
    same kind of edge at about n/2 rows."""
    rng = np.random.default_rng(n)
    r = rig_factory(1000, py=n <= PY_MAX_ROWS)
    drivers = rng.integers(0, 61, 2000)
    r.build(np.arange(1000), drivers[:1000])
    ts, v = rows(rng, n)
    tr = rng.integers(0, 2000, n)
    (gts, gkid, _), _ = r.probe(ts, tr, v)
    hit = tr < 1000
    if r.py is None:  # second reference for the big case: the same in numpy
        assert np.array_equal(gts, ts[hit])
        assert np.array_equal(gkid.astype(np.int64), drivers[tr[hit]])
    assert r.jo.unmatched == int((~hit).sum())
    (gts, gkid, _), _ = r.build(np.arange(1000, 2000), drivers[1000:])
    if r.py is None:
        assert np.array_equal(gts, ts[~hit])
        assert np.array_equal(gkid.astype(np.int64), drivers[tr[~hit]])
    assert r.jo.unmatched == 0


# ---- 2. match patterns -------------------------------------------------

@pytest.mark.parametrize("n", [8193, 3 * 8192 + 65])
@pytest.mark.parametrize("name", jv.PATTERNS)
def test_match_patterns(rig_factory, name, n):
    """Where in a ballot group and in a chunk the matches sit; the build
    afterwards releases the complement pattern from the buffer."""
    rng = np.random.default_rng(len(name) * 100_003 + n)
    r = rig_factory(1000)
    drivers = rng.integers(0, 61, 2000)
    r.build(np.arange(1000), drivers[:1000])
    hit = jv.pattern(name, n)
    ts, v = rows(rng, n)
    tr = np.where(hit, rng.integers(0, 1000, n), rng.integers(1000, 2000, n))
    (gts, _, _), _ = r.probe(ts, tr, v)
    assert len(gts) == int(hit.sum())
    (gts, _, _), _ = r.build(np.arange(1000, 2000), drivers[1000:])
    assert len(gts) == int((~hit).sum()) and r.jo.unmatched == 0


# ---- 3. unmatched buffer -----------------------------------------------

def test_unmatched_buffer_growth_and_compaction(rig_factory):
    """Appends at a non-zero base, growth while non-empty (the doubling
    copies only the current ping-pong side), three partial releases, a build
    that releases nothing, a probe appended after compaction, and a build
    that releases everything. Order and content follow the oracle at every
    step. Trips 0..499 in five groups of 100; group 0 is built up front."""
    rng = np.random.default_rng(31)
    r = rig_factory(600)
    drv = rng.integers(0, 61, 1000)
    grp = [np.arange(g * 100, (g + 1) * 100) for g in range(5)]
    r.build(grp[0], drv[grp[0]])

    def probe(n):
        ts, v = rows(rng, n)
        return r.probe(ts, rng.integers(0, 500, n), v)

    probe(3000)                         # base 0; capacity becomes 3000
    u1 = r.jo.unmatched
    assert 0 < u1 < 3000
    probe(1000)                         # base u1 > 0, grows while non-empty
    assert r.jo.unmatched > 3000
    probe(9000)                         # two chunks at a non-zero base, grows
    u3 = r.jo.unmatched
    (gts, _, _), _ = r.build(grp[1], drv[grp[1]])       # partial release 1
    assert 0 < len(gts) < u3
    (gts, _, _), _ = r.build(grp[2], drv[grp[2]])       # partial release 2
    assert len(gts) > 0
    before = r.jo.unmatched
    (gts, _, _), _ = r.build(np.arange(900, 1000), drv[900:1000])
    assert len(gts) == 0 and r.jo.unmatched == before   # releases nothing
    probe(5000)                         # append after ping-pong compaction
    (gts, _, _), _ = r.build(grp[3], drv[grp[3]])       # partial release 3
    assert len(gts) > 0 and r.jo.unmatched > 0
    left = r.jo.unmatched
    (gts, _, _), _ = r.build(grp[4], drv[grp[4]])       # releases everything
    assert len(gts) == left and r.jo.unmatched == 0


# ---- 4. probe clusters -------------------------------------------------

def test_probe_clusters_and_extreme_ids(rig_factory):
    """65,536-slot table (n_trips_hint = 1). 300 trips share home slot 1000
    and are claimed concurrently by one build batch; a 40-trip cluster homed
    at slot 65,535 wraps to slot 0, where trip 0 also lives; absent trips
    have their home at the head of, inside, at the tail of and just past
    each cluster. Ids 0, -1, INT64_MAX and INT64_MIN + 1 are ordinary
    trips."""
    rng = np.random.default_rng(41)
    r = rig_factory(1)
    big = jv.trips_with_home(1000, 300)
    wrap = jv.trips_with_home(65535, 40)
    special = np.array([0, -1, jv.I64_MAX, jv.I64_MIN + 1], np.int64)
    present = np.concatenate([big, wrap, special])
    assert len(set(present.tolist())) == len(present)
    absent = np.concatenate(
        [jv.trips_with_home(s, 2, first=1000)
         for s in (1000, 1001, 1150, 1299, 1300, 65535, 0, 5, 39, 40, 41)])
    assert not set(absent.tolist()) & set(present.tolist())
    drv = rng.integers(0, 2 ** 31, len(present))
    r.build(rng.permutation(present), drv)  # any order: oracle keys by trip

    def probe_all(n):
        pool = np.concatenate([present, absent])
        tr = pool[rng.integers(0, len(pool), n)]
        ts, v = rows(rng, n)
        (gts, _, _), _ = r.probe(ts, tr, v)
        assert len(gts) == int(np.isin(tr, present).sum())

    probe_all(3000)
    # update a slice of each cluster in place, then claim the absent trips
    # that sit inside the clusters (they append at the cluster tails)
    upd = np.concatenate([big[100:200], wrap[10:20], special[:2]])
    r.build(upd, rng.integers(0, 2 ** 31, len(upd)))
    probe_all(3000)
    (gts, _, _), _ = r.build(absent[:8], rng.integers(0, 61, 8))
    assert len(gts) > 0
    present = np.concatenate([present, absent[:8]])
    absent = absent[8:]
    probe_all(3000)


# ---- 5. dimension updates ----------------------------------------------

def test_dimension_updates(rig_factory):
    r = rig_factory(16)
    r.build([1, 2, 8, 9], [10, 20, 0, 2 ** 31 - 1])
    (_, kid, _), _ = r.probe([1, 2, 3, 4, 5], [1, 2, 3, 8, 9],
                             [.5, 1.5, 2.5, 3.5, 4.5])
    assert kid.tolist() == [10, 20, 0, 2 ** 31 - 1]  # 0, INT32_MAX round-trip
    (_, kid, _), _ = r.build([1, 6], [11, 60])       # update; releases nothing
    assert len(kid) == 0 and r.jo.unmatched == 1
    (_, kid, _), _ = r.probe([6, 7], [1, 2], [1., 2.])
    assert kid.tolist() == [11, 20]                  # later probes: new driver
    r.build([3], [30])                               # releases the trip-3 row
    r.probe([8], [4], [3.])                          # trip 4: buffered
    r.build([4], [40])
    r.build([4], [41])
    (_, kid, _), _ = r.probe([9], [4], [4.])
    assert kid.tolist() == [41]
    # a buffered row released by an updating batch gets the driver current
    # at release: trip 5 buffered, first built as 50 together with the update
    # of trip 1 to 12
    r.probe([10], [5], [5.])
    (_, kid, _), _ = r.build([1, 5], [12, 50])
    assert kid.tolist() == [50]
    (_, kid, _), _ = r.probe([11, 12], [1, 5], [6., 7.])
    assert kid.tolist() == [12, 50]


def test_duplicates_within_one_build_batch(rig_factory):
    """The winner among duplicates WITHIN one batch is unspecified: the
    emitted driver is one of the candidates, for a probe after the batch and
    for a buffered row the batch releases. The references are then given the
    device's winner, and everything after is exact again."""
    r = rig_factory(16)
    r.probe([1], [7], [1.5])                              # buffered
    r.build_device_only([7, 5, 7, 7], [70, 50, 71, 72])
    n, pts, pkid, pval = r.jo.matches()
    assert n == 1
    ts, kid, val = read_cols(n, pts, pkid, pval)
    assert ts.tolist() == [1] and val.tolist() == [1.5]
    assert int(kid[0]) in (70, 71, 72)
    r.refs_build(np.array([5, 7], np.int64),
                 np.array([50, int(kid[0])], np.int64))
    r.check()
    (_, kid2, _), _ = r.probe([2, 3], [7, 5], [2.5, 3.5])
    assert kid2.tolist() == [int(kid[0]), 50]


# ---- 6. refusals -------------------------------------------------------

def refused(r, trips, drivers, message):
    """Push a build batch that must be refused with `message` and none of
    the other causes; then check that nothing moved: the unmatched count,
    and the previous matches() (count, pointers, content)."""
    n0, *p0 = r.jo.matches()
    cols0 = read_cols(n0, *p0)
    un0 = r.jo.unmatched
    with pytest.raises(RuntimeError) as e:
        r.build_device_only(np.asarray(trips, np.int64),
                            np.asarray(drivers, np.int64))
    assert message in str(e.value), str(e.value)
    assert not any(m in str(e.value) for m in REFUSALS if m != message)
    n1, *p1 = r.jo.matches()
    assert n1 == n0 and [p.value for p in p1] == [p.value for p in p0]
    assert same_cols(read_cols(n1, *p1), cols0)
    assert r.jo.unmatched == un0 == r.oj.unmatched
    return str(e.value)


def test_capacity_refusal_at_half_the_slots(rig_factory):
    """n_trips_hint = 1: 65,536 slots, capacity 32,768 trips. Exactly that
    many distinct trips pass in one push; one more new trip is refused, an
    update of an existing trip still passes, and the handle works on."""
    rng = np.random.default_rng(61)
    r = rig_factory(1)
    trips = rng.permutation(100_000)[:32768].astype(np.int64)
    drv = rng.integers(0, 61, 32768)
    r.build(trips, drv)
    new = np.int64(200_000)
    some = trips[rng.integers(0, 32768, 500)]

    def probe_existing_and_refused():
        tr = np.concatenate([some, [new]])
        ts, v = rows(rng, len(tr))
        (gts, _, _), _ = r.probe(ts, tr, v)
        assert len(gts) == len(some)    # the refused trip stays unmatched

    probe_existing_and_refused()
    assert "n_trips_hint" in refused(r, [new], [5], "capacity")
    probe_existing_and_refused()
    # an update of existing trips passes at the cap, alone ...
    r.build(trips[:100], (drv[:100] + 1) % 61)
    probe_existing_and_refused()
    # ... but not with a new trip riding along: nothing of it is applied
    refused(r, np.concatenate([trips[:50], [new]]), np.full(51, 60), "capacity")
    probe_existing_and_refused()
    assert r.jo.unmatched == 4


@pytest.mark.parametrize("bad_trip,bad_drv,message", [
    (jv.I64_MIN, 5, "reserved trip id"),
    (77, -1, "driver id outside"),
    (77, 2 ** 31, "driver id outside"),
])
def test_reserved_trip_and_driver_range_refusals(rig_factory, bad_trip,
                                                 bad_drv, message):
    """One bad row among valid NEW trips and an update: the whole batch is
    refused before anything is written. The new trips stay unmatched, the
    update is not applied, buffered rows are not released."""
    r = rig_factory(16)
    r.build([1, 2, 3], [10, 20, 30])
    r.probe([1, 2, 3, 4], [1, 2, 50, 77], [1., 2., 3., 4.])  # 2 buffered
    batch_t = [50, 51, 1, bad_trip, 52]
    batch_d = [15, 16, 11, bad_drv, 17]
    refused(r, batch_t, batch_d, message)
    (_, kid, _), _ = r.probe([5, 6, 7, 8], [1, 50, 51, 52], [1., 2., 3., 4.])
    assert kid.tolist() == [10] and r.jo.unmatched == 5
    # the same batch without the bad row is accepted and releases them
    (_, kid, _), _ = r.build([50, 51, 1, 52], [15, 16, 11, 17])
    assert kid.tolist() == [15, 15, 16, 17] and r.jo.unmatched == 1


def test_reserved_trip_on_the_probe_side(rig_factory):
    """Probe rows with trip INT64_MIN never match, whatever the empty slots
    hold: they buffer like absent trips and no build releases them."""
    rng = np.random.default_rng(67)
    r = rig_factory(1000)
    drv = rng.integers(0, 61, 1000)
    r.build(np.arange(500), drv[:500])
    n = 8193
    ts, v = rows(rng, n)
    tr = rng.integers(0, 1000, n)
    res = rng.random(n) < 0.25
    tr[res] = jv.I64_MIN
    (gts, _, _), _ = r.probe(ts, tr, v)
    assert len(gts) == int(((tr >= 0) & (tr < 500)).sum())
    r.build(np.arange(500, 1000), drv[500:])
    assert r.jo.unmatched == int(res.sum())
    (gts, _, _), _ = r.probe(ts[:64], np.full(64, jv.I64_MIN), v[:64])
    assert len(gts) == 0 and r.jo.unmatched == int(res.sum()) + 64


# ---- 7. output lifetime, no window op ----------------------------------

def test_output_survives_growth_and_zero_match_pushes(rig_factory):
    """The columns of a push with matches stay valid and unchanged, at the
    pointers matches() returned, until the push after the next push with
    matches: across growth of the other buffer (probe and build re-probe as
    the growing push) and across pushes that match nothing."""
    rng = np.random.default_rng(71)
    r = rig_factory(2000)
    drv = rng.integers(0, 61, 2000)
    r.build(np.arange(1000), drv[:1000])

    def probe(n, lo, hi):
        ts, v = rows(rng, n)
        return r.probe(ts, rng.integers(lo, hi, n), v)

    probe(300, 0, 1000)                      # both buffers get a small size
    probe(300, 0, 1000)
    a, (na, *pa) = probe(2000, 0, 1000)      # A: grows its own buffer only
    assert na == 2000
    b, (nb, *pb) = probe(50_000, 0, 1000)    # B: larger, grows the other one
    assert nb == 50_000
    assert same_cols(read_cols(na, *pa), a)  # A intact after B's growth
    _, (nz, *_) = probe(60_000, 1000, 2000)  # Z: matches nothing; would have
    assert nz == 0                           # regrown and rewritten A's side
    assert same_cols(read_cols(nb, *pb), b)  # B intact after Z
    c, (nc, *pc) = probe(70_000, 0, 1000)    # C: grows A's old buffer
    assert nc == 70_000 and pc[0].value != pb[0].value
    assert same_cols(read_cols(nb, *pb), b)  # B still intact after C
    # a build re-probe as the growing push: 60,000 buffered rows released
    # into B's old buffer while C is the live output
    d, (nd, *pd) = r.build(np.arange(1000, 2000), drv[1000:])
    assert nd == 60_000
    assert same_cols(read_cols(nc, *pc), c)  # C intact after the re-probe
    # zero-release build and zero-match probe in a row, then a new output
    probe(500, 5000, 6000)
    _, (n0, *_) = r.build([7000], [1])
    assert n0 == 0
    assert same_cols(read_cols(nd, *pd), d)  # D intact across both
    e, (ne, *pe) = probe(80_000, 0, 2000)
    assert ne == 80_000
    assert same_cols(read_cols(nd, *pd), d)  # and after the next output


# ---- 8. borrowed pipeline ----------------------------------------------

def test_borrowed_pipeline_with_varying_batches(rig_factory):
    """join -> WindowOp.push_device(borrowed=True), 1 s tumbling over 61
    drivers, the composition bench.py --cfg5 uses: the window op reads the
    join's own output buffers, with no staging copy, until its next call.
    Probe sizes vary non-monotonically, two probes match nothing (the window
    push is skipped for them), a mid-stream build releases more rows than
    any probe before it produced, and the window op is polled only at some
    steps. The oracle runs join -> window on the same pushes."""
    from denormalized_amd import WindowOp, _lib
    from tests.test_gpu_parity import assert_parity

    rng = np.random.default_rng(81)
    n_trips, n_drivers = 2000, 61
    trips = rng.permutation(n_trips)
    drivers = rng.integers(0, n_drivers, n_trips)
    half = n_trips // 2
    first, second = trips[:half], trips[half:]
    never = np.arange(10_000, 10_500)

    r = rig_factory(n_trips, py=False)
    wop = WindowOp(length_ms=1000, key_kind=_lib.KEY_DENSE_INT64,
                   n_keys_hint=n_drivers, device=0)
    wor = Oracle(1000, 0)
    outs = []
    row0 = [0]

    def feed(got, handle, poll):
        n, pts, pkid, pval = handle
        if n:
            try:
                wop.push_device(n, pts, pkid, pval, borrowed=True)
            except RuntimeError as e:
                pytest.exit(f"device error, stopping: {e}", returncode=3)
            wor.push(got[0], got[1].astype(np.int64), got[2])
        if poll:
            outs.extend(wop.poll_all())
        return n

    def probe(n, pool, poll):
        ts = 1_000_000 + np.arange(row0[0], row0[0] + n) // 40
        row0[0] += n
        tr = pool[rng.integers(0, len(pool), n)]
        return feed(*r.probe(ts, tr, rng.uniform(0, 115, n)), poll)

    r.build(first, drivers[:half])
    assert probe(5_000, trips, poll=False) > 0
    assert probe(40_000, trips, poll=True) > 0
    assert probe(30_000, second, poll=False) == 0       # nothing built yet
    assert probe(12_000, trips, poll=False) > 0
    released = feed(*r.build(second, drivers[half:]), poll=False)
    assert released > 40_000                # larger than every probe before
    assert probe(70_000, trips, poll=True) == 70_000
    assert probe(3_000, never, poll=False) == 0
    assert probe(3_000, trips, poll=False) == 3_000
    assert probe(9_000, trips, poll=False) == 9_000
    wop.finish()
    wor.finish()
    outs.extend(wop.poll_all())
    exp = wor.fetch()
    assert len(exp["key"]) > 0
    assert_parity(outs, exp)
    wop.close()
    wor.close()
