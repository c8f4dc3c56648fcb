"""GPU tests for aggregates over several value columns in one window op.
Every column and every mask is compared bit-exact with tests/multicolref.py
(one oracle per distinct column, zipped)."""
import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import pyoracle
from tests import multicolref as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _op(len_ms, slide_ms, aggs, key_kind=None, n_keys_hint=64, no_group=False,
        **kw):
    from denormalized_amd import WindowOp, _lib
    base = 1 if no_group else 2  # batch: ts, [key,] value columns
    return WindowOp(length_ms=len_ms, slide_ms=slide_ms,
                    aggs=[(op, base + j, alias) for op, j, alias in aggs],
                    key_kind=_lib.KEY_INT64 if key_kind is None else key_kind,
                    n_keys_hint=n_keys_hint, no_group=no_group, **kw)


def _collect(outs, aggs, no_group=False):
    fields = ["valid", "window_start", "window_end"]
    if not no_group:
        fields.append("key")
    order = mc.distinct_cols(aggs)
    for _op_, j, alias in aggs:
        fields.append(alias)
        if j != order[0]:
            fields.append(alias + "_valid")
    got = {}
    for f in fields:
        arrs = [np.asarray(b[f]) for b in outs]
        got[f] = np.concatenate(arrs) if arrs else np.zeros(0)
    return got


def _push_host(op, batch, aggs):
    ts, keys, cols, valids = batch
    order = mc.distinct_cols(aggs)
    op.push(ts, keys, [cols[j] for j in order],
            [mc.bitmap(valids[j]) if valids is not None else None
             for j in order])


def _run_host(len_ms, slide_ms, batches, aggs, filt=None, **kw):
    op = _op(len_ms, slide_ms, aggs, **kw)
    if filt is not None:
        op.set_filter(*filt)
    outs = []
    for b in batches:
        _push_host(op, b, aggs)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    stats = op.kernel_stats()
    op.close()
    return _collect(outs, aggs), stats


def _check_host(len_ms, slide_ms, batches, aggs, filt=None, **kw):
    got, stats = _run_host(len_ms, slide_ms, batches, aggs, filt=filt, **kw)
    exp = mc.expect(len_ms, slide_ms, batches, aggs, filt=filt)
    assert len(exp["key"]) > 0
    mc.assert_match(got, exp, aggs)
    return got, exp, stats


TWO = [("count", 0, "n0"), ("min", 0, "lo0"), ("max", 1, "hi1"),
       ("avg", 1, "avg1"), ("sum", 1, "sum1"), ("count", 1, "n1")]


# ------------------------------------------------ 1/2: seams, per-column NULLs

@pytest.fixture(scope="module")
def seam_batch():
    """3 keys, all = 0 mod 512 (one bucket), 5,003 rows (not a multiple of 8)
    in one tumbling window: several 2,048-record supertiles, wave-quarter
    seams inside each."""
    from denormalized_amd import _lib
    rng = np.random.default_rng(2101)
    n = 5003
    ts = (1_000_000 + np.sort(rng.integers(0, 1000, n))).astype(np.int64)
    keys = (rng.integers(0, 3, n) * 512).astype(np.int64)
    cols = [rng.uniform(-1e3, 1e3, n), rng.uniform(-1e9, 1e9, n)]
    for a in cols:
        a.setflags(write=False)
    return _lib.KEY_DENSE_INT64, (ts, keys, cols)


def test_supertile_and_wave_quarter_seams(seam_batch):
    kind, (ts, keys, cols) = seam_batch
    _check_host(1000, 0, [(ts, keys, cols, None)], TWO, key_kind=kind,
                n_keys_hint=1025)


def test_per_column_nulls(seam_batch):
    kind, (ts, keys, cols) = seam_batch
    rng = np.random.default_rng(2102)
    n = len(ts)
    v0 = rng.random(n) > 0.3
    v1 = rng.random(n) > 0.5
    v1 &= keys != 512   # extra all NULL, primary valid
    v0 |= keys == 512
    v0 &= keys != 1024  # primary all NULL, extra valid
    v1 |= keys == 1024
    got, exp, _ = _check_host(1000, 0, [(ts, keys, cols, [v0, v1])], TWO,
                              key_kind=kind, n_keys_hint=1025)
    i512 = int(np.flatnonzero(got["key"] == 512)[0])
    i1024 = int(np.flatnonzero(got["key"] == 1024)[0])
    assert got["n1"][i512] == 0 and not got["hi1_valid"][i512]
    assert got["valid"][i512] == 1 and got["n0"][i512] > 0
    assert got["n0"][i1024] == 0 and got["valid"][i1024] == 0
    assert got["hi1_valid"][i1024] == 1 and got["n1"][i1024] > 0
    assert got["n1_valid"].all()


# ------------------------------------------------------- 3: aggregate order

def _rand_batches(seed, nb, n, nkeys, ncols, null_p=0.25, span=1500):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(nb):
        ts = (1_000_000 + b * 800 + rng.integers(0, span, n)).astype(np.int64)
        keys = rng.integers(0, nkeys, n).astype(np.int64)
        cols = [rng.uniform(-100, 100, n) * 10.0 ** j for j in range(ncols)]
        valids = [rng.random(n) > null_p * (j + 1) / ncols
                  for j in range(ncols)]
        out.append((ts, keys, cols, valids))
    return out


def test_aggregate_order_primary_is_first_named():
    aggs = [("max", 1, "a"), ("min", 0, "b"), ("count", 2, "c"),
            ("avg", 1, "d"), ("sum", 0, "e")]
    assert mc.distinct_cols(aggs) == [1, 0, 2]
    _check_host(1000, 0, _rand_batches(31, 3, 3001, 41, 3), aggs)


def test_four_columns():
    aggs = [("sum", 3, "s3"), ("min", 0, "m0"), ("max", 2, "x2"),
            ("avg", 1, "a1"), ("count", 3, "n3"), ("count", 0, "n0"),
            ("max", 1, "x1"), ("sum", 2, "s2")]
    _check_host(1000, 0, _rand_batches(32, 3, 3001, 41, 4), aggs)


# ------------------------------------------------ 4: accumulation across pushes

def test_accumulation_across_pushes_is_row_ordered():
    """One window fed by 3 pushes; the f64 sum of 1e16 / 1.0 / -1e16 patterns
    depends on the order of addition, per column."""
    pat0 = np.array([1e16, 1.0, -1e16, 1.0, 1.0])
    pat1 = np.array([1.0, 1e16, 1.0, -1e16, 3.0])
    batches = []
    for b in range(3):
        n = 1001 + b
        ts = (1_000_000 + b * 300 + np.arange(n) % 300).astype(np.int64)
        keys = (np.arange(n) % 5).astype(np.int64)
        cols = [np.roll(np.resize(pat0, n), b), np.roll(np.resize(pat1, n), 2 * b)]
        batches.append((ts, keys, cols, None))
    got, exp, _ = _check_host(1000, 0, batches, TWO)
    assert len(np.unique(exp["window_start"])) == 1


# ------------------------------------------------------------ 5: slot reuse

def test_slot_reuse_does_not_surface_stale_extras():
    """More tumbling windows than slots in use: key 5 has extra values in the
    first two windows only; in every later window (each recycles a slot those
    windows used) its extra column is all NULL."""
    rng = np.random.default_rng(51)
    batches = []
    for w in range(9):
        n = 700
        ts = (1_000_000 + w * 1000 + rng.integers(0, 1000, n)).astype(np.int64)
        keys = rng.integers(0, 9, n).astype(np.int64)
        keys[:3] = 5
        cols = [rng.uniform(0, 10, n), rng.uniform(-999, -900, n)]
        v1 = np.ones(n, bool)
        if w >= 2:
            v1 &= keys != 5
        batches.append((ts, keys, cols, [None, v1]))
    got, exp, _ = _check_host(1000, 0, batches, TWO, max_open_windows=2)
    late = (got["key"] == 5) & (got["window_start"] >= 1_002_000)
    assert late.sum() == 7
    assert (got["n1"][late] == 0).all() and not got["hi1_valid"][late].any()
    assert (got["hi1"][late] == 0.0).all()


# -------------------------------- 6: two-level fold and the 64k-key route

def test_two_level_fold_takes_host_route_above_64k_keys():
    from denormalized_amd import _lib
    rng = np.random.default_rng(61)
    n, nkeys = 300_000, 140_000
    ts = (1_000_000 + rng.integers(0, 1000, n)).astype(np.int64)
    keys = rng.permutation(n) % nkeys
    cols = [rng.uniform(-5, 5, n), rng.uniform(0, 1e6, n)]
    valids = [rng.random(n) > 0.1, rng.random(n) > 0.4]
    got, exp, stats = _check_host(
        1000, 0, [(ts, keys.astype(np.int64), cols, valids)], TWO,
        key_kind=_lib.KEY_DENSE_INT64, n_keys_hint=nkeys)
    assert len(exp["key"]) == nkeys
    assert stats["regroup"]["launches"] >= 1  # RG_L1 ran, so RG_L2_FOLD did
    for name in ("h_emit_group", "h_emit_group_closes", "h_emit_perclose",
                 "h_emit_smallsort"):
        assert stats[name]["launches"] == 0, name


# ------------------------------------------------------- 7/8: sliding, split

def test_sliding_4000_1000():
    rng = np.random.default_rng(71)
    batches = []
    for b in range(2):
        n = 10_000
        ts = (1_000_000 + b * 5000 + np.sort(rng.integers(0, 6000, n))
              ).astype(np.int64)
        keys = rng.integers(0, 50, n).astype(np.int64)
        cols = [rng.uniform(-100, 100, n), rng.uniform(0, 1e4, n)]
        batches.append((ts, keys, cols,
                        [rng.random(n) > 0.2, rng.random(n) > 0.3]))
    _check_host(4000, 1000, batches, TWO)


def test_window_subrange_self_split():
    # the smallest split shape of the single-column parity suite (a batch
    # spanning > 256 sliding windows), with a second column
    rng = np.random.default_rng(4242)
    n = 50_000
    ts = (1_000_000 + np.arange(n) // 25).astype(np.int64)
    keys = rng.integers(0, 600, n).astype(np.int64)
    cols = [rng.uniform(0, 115, n), rng.uniform(-1e5, 1e5, n)]
    valids = [None, rng.random(n) > 0.3]
    _check_host(200, 5, [(ts, keys, cols, valids)], TWO, n_keys_hint=600)


# ---------------------------------------------------------- 9: push kinds

@pytest.fixture(scope="module")
def kinds_batch():
    rng = np.random.default_rng(91)
    n = 4096
    ts = (1_000_000 + rng.integers(0, 2500, n)).astype(np.int64)
    kid = rng.integers(0, 23, n).astype(np.int64)
    cols = [rng.uniform(-10, 10, n), rng.uniform(0, 1e8, n)]
    v1 = rng.random(n) > 0.35
    for a in cols + [ts, kid, v1]:
        a.setflags(write=False)
    return ts, kid, cols, v1


def _dev(arr):
    from denormalized_amd import DeviceArray
    arr = np.ascontiguousarray(arr)
    d = DeviceArray(0, max(arr.nbytes, 8))
    d.from_host(arr)
    return d


def _finish(op, aggs, no_group=False):
    op.finish()
    got = _collect(op.poll_all(), aggs, no_group)
    stats = op.kernel_stats()
    op.close()
    return got, stats


def test_push_kind_host(kinds_batch):
    ts, kid, cols, v1 = kinds_batch
    _check_host(1000, 0, [(ts, kid, cols, [None, v1])], TWO)


@pytest.mark.parametrize("borrowed", [False, True])
def test_push_kind_device_dense(kinds_batch, borrowed):
    from denormalized_amd import _lib
    ts, kid, cols, v1 = kinds_batch
    keep = [_dev(ts), _dev(kid.astype(np.int32)), _dev(cols[0]),
            _dev(cols[1]), _dev(mc.bitmap(v1))]
    op = _op(1000, 0, TWO, key_kind=_lib.KEY_DENSE_INT64, n_keys_hint=32)
    op.set_extra_values(len(ts), [keep[3].ptr], [keep[4].ptr])
    op.push_device(len(ts), keep[0].ptr, keep[1].ptr, keep[2].ptr,
                   borrowed=borrowed)
    got, _ = _finish(op, TWO)
    exp = mc.expect(1000, 0, [(ts, kid, cols, [None, v1])], TWO)
    mc.assert_match(got, exp, TWO)
    for d in keep:
        d.free()


def test_push_kind_device_utf8(kinds_batch):
    from denormalized_amd import _lib
    ts, kid, cols, v1 = kinds_batch
    names = [f"sensor_{int(k)}".encode() for k in kid]
    offs = np.zeros(len(names) + 1, np.int32)
    np.cumsum([len(x) for x in names], out=offs[1:])
    data = np.frombuffer(b"".join(names), np.uint8)
    keep = [_dev(ts), _dev(offs), _dev(data), _dev(cols[0]), _dev(cols[1]),
            _dev(mc.bitmap(v1))]
    op = _op(1000, 0, TWO, key_kind=_lib.KEY_UTF8, n_keys_hint=32)
    op.set_extra_values(len(ts), [keep[4].ptr], [keep[5].ptr])
    op.push_device_utf8(len(ts), keep[0].ptr, keep[1].ptr, keep[2].ptr,
                        keep[3].ptr)
    op.finish()
    outs = op.poll_all()
    op.close()
    exp = mc.expect(1000, 0, [(ts, kid, cols, [None, v1])], TWO)
    keys = [k for b in outs for k in b["key"]]
    assert keys == [f"sensor_{int(k)}" for k in exp["key"]]
    for b in outs:
        b["key"] = np.zeros(b["n_rows"], np.int64)
    got = _collect(outs, TWO)
    got["key"] = exp["key"]
    mc.assert_match(got, exp, TWO)
    for d in keep:
        d.free()


def test_push_kind_device_i64(kinds_batch):
    from denormalized_amd import _lib
    ts, kid, cols, v1 = kinds_batch
    sparse = kid * 1_000_003 - 7_000_000_000  # arbitrary, some negative
    keep = [_dev(ts), _dev(sparse), _dev(cols[0]), _dev(cols[1]),
            _dev(mc.bitmap(v1))]
    op = _op(1000, 0, TWO, key_kind=_lib.KEY_INT64, n_keys_hint=32)
    op.set_extra_values(len(ts), [keep[3].ptr], [keep[4].ptr])
    op.push_device_i64(len(ts), keep[0].ptr, keep[1].ptr, keep[2].ptr)
    got, _ = _finish(op, TWO)
    exp = mc.expect(1000, 0, [(ts, sparse, cols, [None, v1])], TWO)
    mc.assert_match(got, exp, TWO)
    for d in keep:
        d.free()


def test_push_kind_global_no_group(kinds_batch):
    ts, kid, cols, v1 = kinds_batch
    zeros = np.zeros(len(ts), np.int64)
    op = _op(1000, 0, TWO, no_group=True)
    op.push(ts, None, [cols[0], cols[1]], [None, mc.bitmap(v1)])
    got, _ = _finish(op, TWO, no_group=True)
    exp = mc.expect(1000, 0, [(ts, zeros, cols, [None, v1])], TWO)
    got["key"] = exp["key"]  # a global aggregate has no group column
    mc.assert_match(got, exp, TWO)


# ------------------------------------------ 10: filter on an extra aggregate

@pytest.mark.parametrize("cmp", ["<", "<=", ">", ">=", "==", "!="])
def test_filter_on_extra_column_aggregate(cmp):
    batches = _rand_batches(101, 2, 4001, 97, 2, null_p=0.5)
    for ts, keys, cols, valids in batches:
        valids[1] &= keys % 7 != 0  # whole groups NULL in c1
    full = mc.expect(1000, 0, batches, TWO)
    m = full["hi1_valid"].astype(bool)
    assert (~m).any()
    lit = float(np.sort(full["hi1"][m])[m.sum() // 2])  # an attained value
    got, exp, _ = _check_host(1000, 0, batches, TWO, filt=("hi1", cmp, lit))
    assert got["hi1_valid"].all()  # a NULL never passes
    assert 0 < len(exp["key"]) < len(full["key"])


# --------------------------------------------- 11: NaN / +-Inf in an extra

def test_nan_inf_in_extra_column_pinned():
    rng = np.random.default_rng(424)
    n = 20_000
    ts = (1_000_000 + np.arange(n) // 20).astype(np.int64)
    keys = rng.integers(0, 37, n).astype(np.int64)
    c0 = rng.uniform(-10, 115, n)
    c1 = rng.uniform(-10, 115, n)
    sp = rng.integers(0, n, 600)
    c1[sp[:200]] = np.nan
    c1[sp[200:400]] = np.inf
    c1[sp[400:]] = -np.inf
    v1 = rng.random(n) > 0.1
    batches = [(ts, keys, [c0, c1], [None, v1])]
    got, _ = _run_host(1000, 0, batches, TWO)
    exp = mc.expect(1000, 0, batches, TWO)
    assert np.isnan(exp["sum1"]).any() and np.isinf(exp["hi1"]).any()
    mc.assert_match(got, exp, TWO, nan_payload_free=True)


def test_nan_first_sticks_in_extra_column():
    ts = np.array([1_000_000] * 4, np.int64)
    keys = np.zeros(4, np.int64)
    cols = [np.array([1.0, 2.0, 3.0, 4.0]), np.array([np.nan, 1.0, -5.0, 2.0])]
    got, _ = _run_host(1000, 0, [(ts, keys, cols, None)], TWO)
    assert got["n1"][0] == 4 and got["hi1_valid"][0] == 1
    assert np.isnan(got["hi1"][0]) and np.isnan(got["avg1"][0])
    assert got["lo0"][0] == 1.0 and got["n0"][0] == 4


# ------------------------------------------------------------ 12: refusals

def test_refusals_leave_the_handle_usable(kinds_batch):
    from denormalized_amd import WindowOp, _lib
    with pytest.raises(RuntimeError, match="distinct input columns"):
        WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64,
                 aggs=[("sum", 2 + j, f"s{j}") for j in range(5)])
    with pytest.raises(RuntimeError, match="variance"):
        WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64,
                 aggs=[("var_pop", 2, "v"), ("min", 3, "m")])
    ts, kid, cols, v1 = kinds_batch
    n = len(ts)
    keep = [_dev(ts), _dev(kid.astype(np.int32)), _dev(cols[0]),
            _dev(cols[1]), _dev(mc.bitmap(v1))]
    op = _op(1000, 0, TWO, key_kind=_lib.KEY_DENSE_INT64, n_keys_hint=32)
    with pytest.raises(RuntimeError, match="set_extra_values"):
        op.push_device(n, keep[0].ptr, keep[1].ptr, keep[2].ptr)
    op.set_extra_values(n - 1, [keep[3].ptr], [keep[4].ptr])
    with pytest.raises(RuntimeError, match="rows"):
        op.push_device(n, keep[0].ptr, keep[1].ptr, keep[2].ptr)
    # the attachment was consumed by the refused push
    with pytest.raises(RuntimeError, match="set_extra_values"):
        op.push_device(n, keep[0].ptr, keep[1].ptr, keep[2].ptr)
    op.set_extra_values(n, [keep[3].ptr], [keep[4].ptr])
    op.push_device(n, keep[0].ptr, keep[1].ptr, keep[2].ptr)
    got, _ = _finish(op, TWO)
    exp = mc.expect(1000, 0, [(ts, kid, cols, [None, v1])], TWO)
    mc.assert_match(got, exp, TWO)

    single = WindowOp(length_ms=1000, key_kind=_lib.KEY_DENSE_INT64,
                      n_keys_hint=32)
    with pytest.raises(RuntimeError, match="one value column"):
        single.set_extra_values(n, [keep[3].ptr])
    single.push_device(n, keep[0].ptr, keep[1].ptr, keep[2].ptr)
    single.finish()
    outs = single.poll_all()
    single.close()
    o = pyoracle.Oracle(1000, 0)
    o.push(ts, kid, cols[0])
    o.finish()
    e1 = o.fetch()
    o.close()
    assert np.array_equal(np.concatenate([b["key"] for b in outs]), e1["key"])
    assert np.array_equal(np.concatenate([b["avg"] for b in outs]), e1["avg"])
    for d in keep:
        d.free()


# --------------------------------------- 13: single-column ops untouched

def test_single_column_two_tuple_op_unchanged():
    from denormalized_amd import WindowOp, _lib
    rng = np.random.default_rng(131)
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64, n_keys_hint=64,
                  aggs=(("count", 7), ("min", 8), ("max", 9), ("avg", 0),
                        ("sum", 3)))
    assert op.n_value_cols == 1
    o = pyoracle.Oracle(1000, 0)
    outs = []
    for b in range(3):
        n = 5001
        ts = (1_000_000 + b * 900 + rng.integers(0, 1500, n)).astype(np.int64)
        keys = rng.integers(0, 53, n).astype(np.int64)
        vals = rng.uniform(-1e6, 1e6, n)
        valid = rng.random(n) > 0.2
        op.push(ts, keys, vals, mc.bitmap(valid))
        outs += op.poll_all()
        o.push(ts, keys, vals, valid.astype(np.uint8))
    op.finish()
    outs += op.poll_all()
    o.finish()
    exp = o.fetch()
    stats = op.kernel_stats()
    op.close()
    o.close()
    assert not any(k.endswith("_valid") for k in outs[0])
    for f in ("key", "count", "valid", "window_start", "window_end"):
        assert np.array_equal(np.concatenate([b[f] for b in outs]), exp[f]), f
    m = exp["valid"].astype(bool)
    for f in ("min", "max", "avg", "sum"):
        g = np.concatenate([b[f] for b in outs])
        assert np.array_equal(g[m].view(np.int64), exp[f][m].view(np.int64)), f
    assert stats["regfold"]["launches"] >= 3
