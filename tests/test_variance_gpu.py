"""GPU parity of the variance-family aggregates (var_samp / var_pop /
stddev_samp / stddev_pop) against the pure-Python Welford reference
(tests/varref.py) layered on the CPU oracle's rows. The fold presents each
group's rows in stream order and the Welford step is compiled without
contraction, so every value is asserted BIT-EXACT (np.array_equal on the rows
whose per-aggregate mask is 1); masks are compared exactly."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import pyoracle
from tests import varref

pytestmark = pytest.mark.gpu

# output column name -> canonical reference column
VAR4 = {"var_samp": "var_samp", "var_pop": "var_pop",
        "stddev": "stddev_samp", "stddev_pop": "stddev_pop"}
BASE = ("count", "min", "max", "avg")


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _aggs(names):
    return [(n, 0) for n in names]


def _cat(outs, field, dtype=None):
    arrs = [b[field] for b in outs]
    if not arrs:
        return np.zeros(0, dtype or np.float64)
    if isinstance(arrs[0], list):
        return [x for a in arrs for x in a]
    return np.concatenate(arrs)


def run_gpu(len_ms, slide_ms, batches, names, key_kind=None, n_keys_hint=64,
            valids=None, filt=None, **kw):
    """Push `batches` through a WindowOp declaring `names`; returns the
    emitted rows concatenated per column."""
    from denormalized_amd import WindowOp, _lib
    op = WindowOp(length_ms=len_ms, slide_ms=slide_ms, aggs=_aggs(names),
                  key_kind=_lib.KEY_INT64 if key_kind is None else key_kind,
                  n_keys_hint=n_keys_hint, **kw)
    if filt is not None:
        op.set_filter(*filt)
    outs = []
    for bi, (ts, k, v) in enumerate(batches):
        bm = None
        if valids is not None and valids[bi] is not None:
            bm = np.packbits(np.asarray(valids[bi], np.uint8),
                             bitorder="little")
        op.push(ts, k, v, bm)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    op.close()
    fields = ["key", "valid", "window_start", "window_end"] + list(names) + \
        [n + "_valid" for n in names if n in varref.ALIASES]
    return {f: np.asarray(_cat(outs, f)) for f in fields}


def run_oracle(len_ms, slide_ms, batches, valids=None):
    o = pyoracle.Oracle(len_ms, slide_ms)
    for bi, (ts, k, v) in enumerate(batches):
        vv = valids[bi] if valids is not None else None
        o.push(ts, k, v, None if vv is None else np.asarray(vv, np.uint8))
    o.finish()
    exp = o.fetch()
    o.close()
    return exp


def assert_rows(got, exp, ref, names, equal_nan=False):
    """Full parity of one run: row set/order, base columns vs the oracle,
    variance columns + their masks vs the Welford reference."""
    assert len(exp["key"]) > 0
    assert np.array_equal(got["key"], exp["key"]), "keys/order"
    assert np.array_equal(got["window_start"], exp["window_start"])
    assert np.array_equal(got["window_end"], exp["window_end"])
    assert np.array_equal(got["valid"], exp["valid"]), "base validity"
    v = exp["valid"].astype(bool)
    for f in names:
        if f == "count":
            assert np.array_equal(got[f], exp[f]), f
        elif f in BASE or f == "sum":
            assert np.array_equal(got[f][v], exp[f][v], equal_nan=equal_nan), f
        else:
            vals, msk = ref[varref.ALIASES[f]]
            assert np.array_equal(got[f + "_valid"], msk), f + " mask"
            m = msk.astype(bool)
            assert np.array_equal(got[f][m], vals[m], equal_nan=equal_nan), \
                f + " not bit-exact"


def gen_batches(seed, nbatches, rows, nkeys, rows_per_ms, t0=1_000_000):
    return [pyoracle.gen(seed, t0, b * rows, rows, nkeys, rows_per_ms)
            for b in range(nbatches)]


# ------------------------------------------------ 1. direct fold, host emission

@pytest.fixture(scope="module")
def small_stream():
    batches = gen_batches(1, 4, 10_000, 37, 10)
    exp = run_oracle(1000, 0, batches)
    return batches, exp, varref.expected(exp, batches)


def test_direct_fold_host_emission(small_stream):
    batches, exp, ref = small_stream
    names = ["var_samp", "count", "var_pop", "avg", "stddev", "stddev_pop"]
    got = run_gpu(1000, 0, batches, names)
    assert_rows(got, exp, ref, names)


def test_datastream_api_window_and_filter(small_stream):
    import denormalized_amd as dz
    batches, exp, ref = small_stream
    src = [{"occurred_at_ms": ts, "sensor_name": k, "reading": v}
           for ts, k, v in batches]
    lit = float(np.median(ref["stddev_samp"][0]))
    outs = (dz.Context(device=0).from_batches(src)
            .window(["sensor_name"], [("stddev", "reading"),
                                      ("count", "reading")], 1000, None)
            .filter("stddev", ">", lit).collect())
    vals, msk = ref["stddev_samp"]
    keep = msk.astype(bool) & (vals > lit)
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(_cat(outs, "key"), exp["key"][keep])
    assert np.array_equal(_cat(outs, "stddev"), vals[keep])
    assert np.array_equal(_cat(outs, "stddev_valid"),
                          np.ones(keep.sum(), np.uint8))
    assert np.array_equal(_cat(outs, "count"), exp["count"][keep])


# ------------------------------------------- 2. state carried across batches

def test_state_carried_across_batches(small_stream):
    batches, exp, ref = small_stream
    ts, k, v = (np.concatenate([b[i] for b in batches]) for i in range(3))
    names = ["var_samp", "var_pop", "stddev", "stddev_pop", "count"]
    one = run_gpu(1000, 0, [(ts, k, v)], names)
    n = len(ts)
    cuts = [n * i // 8 for i in range(9)]
    eight = run_gpu(1000, 0, [(ts[a:b], k[a:b], v[a:b])
                              for a, b in zip(cuts, cuts[1:])], names)
    for f in one:
        assert np.array_equal(one[f], eight[f]), f
    assert_rows(eight, exp, ref, names)


# --------------------------- 3. two-level fold, >65536 keys (and 9. filters)

@pytest.fixture(scope="module")
def large_stream():
    """70 000 dense keys, 2 x 200 000 rows over 3 windows: klocs * nw =
    137 * 2 > 256 per batch selects RG_L1 + RG_L2_FOLD, and n_keys > 65536 is
    the key count at which ops WITHOUT a variance aggregate emit through the
    device chains."""
    from denormalized_amd import _lib
    rng = np.random.default_rng(7001)
    n, nk = 400_000, 70_000
    ts = (1_000_000 + np.arange(n) // 160).astype(np.int64)  # 2.5 s span
    k = rng.integers(0, nk, n)
    k[0] = nk - 1
    v = rng.uniform(0, 115, n)
    batches = [(ts[:n // 2], k[:n // 2], v[:n // 2]),
               (ts[n // 2:], k[n // 2:], v[n // 2:])]
    # keys < 50 only ever carry null values: all-null groups, the one case
    # in which the population forms are NULL too
    valids = [(b[1] >= 50).astype(np.uint8) for b in batches]
    exp = run_oracle(1000, 0, batches, valids)
    ref = varref.expected(exp, batches, valids)
    names = ["count", "min", "var_samp", "var_pop", "stddev", "stddev_pop"]
    got = run_gpu(1000, 0, batches, names, key_kind=_lib.KEY_DENSE_INT64,
                  n_keys_hint=nk, valids=valids)
    return batches, valids, exp, ref, names, got


def test_two_level_fold_large_keyspace(large_stream):
    batches, _valids, exp, ref, names, got = large_stream
    assert len(np.unique(exp["window_start"])) >= 2
    assert exp["key"].max() >= 65536
    assert_rows(got, exp, ref, names)


# ------------------------------- 4. sliding 500/100, window-subrange split

def test_sliding_500_100_subrange_split():
    # one batch spanning ~305 sliding windows: more than the 50 the shape
    # asks for, because the window-subrange self-split only engages past
    # khigh * nw > 256
    rng = np.random.default_rng(7002)
    n, nk = 30_000, 3_000
    ts = (1_000_000 + np.arange(n)).astype(np.int64)  # 30 s span
    k = rng.integers(0, nk, n)
    v = rng.uniform(-20, 115, n)
    batches = [(ts, k, v)]
    exp = run_oracle(500, 100, batches)
    assert len(np.unique(exp["window_start"])) > 256
    ref = varref.expected(exp, batches)
    names = ["count", "var_samp", "var_pop", "stddev", "stddev_pop", "max"]
    got = run_gpu(500, 100, batches, names, n_keys_hint=nk)
    assert_rows(got, exp, ref, names)


# ------------------------------------------------------------ 5. NULL rules

def test_null_rules():
    rng = np.random.default_rng(7003)
    n = 4_000
    ts = np.full(n, 1_000_200, np.int64)
    k = rng.integers(3, 20, n)
    v = rng.uniform(0, 115, n)
    valid = np.ones(n, np.uint8)
    # key 0: every row null; key 1: one valid row (plus a null one);
    # key 2: two equal values
    k[10:14] = 0
    valid[10:14] = 0
    k[20:22] = 1
    valid[21] = 0
    v[20] = 42.5
    k[30] = k[31] = 2
    v[30] = v[31] = 7.25
    batches, valids = [(ts, k, v)], [valid]
    exp = run_oracle(1000, 0, batches, valids)
    ref = varref.expected(exp, batches, valids)
    names = ["count", "min", "var_samp", "var_pop", "stddev", "stddev_pop"]
    got = run_gpu(1000, 0, batches, names, valids=valids)
    assert_rows(got, exp, ref, names)

    def row(key):
        (i,) = np.flatnonzero(got["key"] == key)
        return i
    r = row(0)   # all-null group: everything NULL
    assert got["count"][r] == 0 and got["valid"][r] == 0
    for f in VAR4:
        assert got[f + "_valid"][r] == 0
    r = row(1)   # one valid row
    assert got["count"][r] == 1 and got["valid"][r] == 1
    assert got["min"][r] == 42.5
    assert got["var_pop_valid"][r] == 1 and got["var_pop"][r] == 0.0
    assert got["stddev_pop_valid"][r] == 1 and got["stddev_pop"][r] == 0.0
    assert got["var_samp_valid"][r] == 0 and got["stddev_valid"][r] == 0
    r = row(2)   # two equal values: exactly zero everywhere
    assert got["count"][r] == 2
    for f in VAR4:
        assert got[f + "_valid"][r] == 1 and got[f][r] == 0.0


# ------------------------------------------------------------ 6. slot reuse

def test_slot_reuse_sees_no_stale_state():
    # 14 tumbling windows pushed one window per batch: at most two windows
    # are ever open, so the op never grows past its initial 4 slots and each
    # slot is recycled 3+ times. Early windows carry huge values, later ones
    # tiny values and FEWER rows per key (some keys get exactly one row), so
    # a stale mean/m2 in a recycled slot would show in bits and in masks.
    rng = np.random.default_rng(7004)
    batches = []
    for w in range(14):
        n = 600 if w < 6 else 40
        ts = np.sort(1_000_000 + w * 1000 + rng.integers(0, 1000, n))
        k = rng.integers(0, 23, n)
        v = rng.uniform(1e6, 1e9, n) if w < 6 else rng.uniform(0, 1e-3, n)
        batches.append((ts.astype(np.int64), k, v))
    exp = run_oracle(1000, 0, batches)
    ref = varref.expected(exp, batches)
    assert (ref["var_samp"][1] == 0).any()  # one-row groups do occur
    names = ["count", "var_samp", "var_pop", "stddev", "stddev_pop"]
    got = run_gpu(1000, 0, batches, names, max_open_windows=4)
    assert_rows(got, exp, ref, names)


# ---------------------------------------------------- 7. contraction sentinel

def _fma(a, b, c):
    """Exact fused multiply-add: one rounding of a*b+c (float(Fraction) is
    correctly rounded)."""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _m2_fused(values):
    count, mean, m2 = 0, 0.0, 0.0
    for v in values:
        count += 1
        d1 = v - mean
        mean = d1 / float(count) + mean
        d2 = v - mean
        m2 = _fma(d1, d2, m2)
    return m2


def test_contraction_sentinel():
    rng = np.random.default_rng(7005)
    vals = rng.uniform(0, 115, 64)          # 64 rows: var_pop = m2 / 2^6 is
    count, _mean, m2 = varref.welford(vals.tolist())   # an exact scaling
    fused = _m2_fused(vals.tolist())
    assert fused != m2, "inputs do not separate fused from unfused m2"
    assert fused / 64.0 != m2 / 64.0
    ts = np.full(64, 1_000_100, np.int64)
    k = np.zeros(64, np.int64)
    got = run_gpu(1000, 0, [(ts, k, vals)], ["var_pop", "count"])
    assert got["count"].tolist() == [64]
    assert got["var_pop_valid"].tolist() == [1]
    assert got["var_pop"][0] == m2 / 64.0, \
        "fused" if got["var_pop"][0] == fused / 64.0 else "neither"


# ------------------------------------------------------------ 8. NaN / ±Inf

def test_nan_inf_propagate():
    rng = np.random.default_rng(7006)
    n = 20_000
    ts = (1_000_000 + np.arange(n) // 10).astype(np.int64)
    k = rng.integers(0, 37, n)
    v = rng.uniform(-10, 115, n)
    sp = rng.choice(n, 30, replace=False)
    v[sp[:10]] = np.nan
    v[sp[10:20]] = np.inf
    v[sp[20:]] = -np.inf
    batches = [(ts, k, v)]
    exp = run_oracle(1000, 0, batches)
    ref = varref.expected(exp, batches)
    fin = np.isfinite(ref["var_pop"][0])
    assert fin.any() and (~fin).any()  # both kinds of group are present
    names = ["count", "var_samp", "var_pop", "stddev", "stddev_pop"]
    got = run_gpu(1000, 0, batches, names)
    # a fresh NaN's sign/payload is ISA-specific; NaN-ness is what is pinned
    assert_rows(got, exp, ref, names, equal_nan=True)


# ---------------------------------------------------------------- 9. filter

def _assert_filtered(full, filt_got, names, field, cmp, lit):
    import operator
    fn = {">": operator.gt, "<=": operator.le}[cmp]
    keep = full[field + "_valid"].astype(bool) & fn(full[field], lit)
    assert 0 < keep.sum() < len(keep)
    assert (full[field + "_valid"] == 0).any()  # NULL rows exist to drop
    for f in filt_got:
        assert np.array_equal(filt_got[f], full[f][keep]), f


@pytest.mark.parametrize("field,cmp,lit", [("stddev", ">", 30.0),
                                           ("var_pop", "<=", 500.0)])
def test_filter_small_keyspace(field, cmp, lit):
    rng = np.random.default_rng(7007)
    n, nk = 12_000, 5_000    # ~2.4 rows per group: plenty of one-row groups
    ts = (1_000_000 + np.arange(n) // 12).astype(np.int64)
    batches = [(ts, rng.integers(0, nk, n), rng.uniform(0, 115, n))]
    valids = [(batches[0][1] >= 50).astype(np.uint8)]  # all-null groups
    names = ["count", "stddev", "var_pop", "min"]
    full = run_gpu(1000, 0, batches, names, n_keys_hint=nk, valids=valids)
    exp = run_oracle(1000, 0, batches, valids)
    assert_rows(full, exp, varref.expected(exp, batches, valids), names)
    got = run_gpu(1000, 0, batches, names, n_keys_hint=nk, valids=valids,
                  filt=(field, cmp, lit))
    _assert_filtered(full, got, names, field, cmp, lit)


@pytest.mark.parametrize("field,cmp,lit", [("stddev", ">", 30.0),
                                           ("var_pop", "<=", 500.0)])
def test_filter_large_keyspace(large_stream, field, cmp, lit):
    from denormalized_amd import _lib
    batches, valids, _exp, _ref, names, full = large_stream
    got = run_gpu(1000, 0, batches, names, key_kind=_lib.KEY_DENSE_INT64,
                  n_keys_hint=70_000, valids=valids, filt=(field, cmp, lit))
    _assert_filtered(full, got, names, field, cmp, lit)


# ------------------------------------- 10. utf8 device intern, global op

def test_device_utf8_intern_push():
    from denormalized_amd import DeviceArray, WindowOp, _lib
    rng = np.random.default_rng(7008)
    n, nk = 4_000, 50
    ts = (1_000_000 + np.arange(n) // 2).astype(np.int64)  # 2 s span
    kid = rng.integers(0, nk, n)
    v = rng.uniform(0, 115, n)
    names_u = [f"sensor_{int(x)}".encode() for x in kid]
    offs = np.zeros(n + 1, np.int32)
    np.cumsum([len(x) for x in names_u], out=offs[1:])
    data = np.frombuffer(b"".join(names_u), np.uint8)
    bufs = []
    for a in (ts, offs, data, v):
        d = DeviceArray(0, a.nbytes)
        d.from_host(a)
        bufs.append(d)
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_UTF8, n_keys_hint=nk,
                  aggs=_aggs(["count", "stddev"]))
    op.push_device_utf8(n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr)
    op.finish()
    outs = op.poll_all()
    op.close()
    for d in bufs:
        d.free()
    batches = [(ts, kid, v)]
    exp = run_oracle(1000, 0, batches)
    vals, msk = varref.expected(exp, batches)["stddev_samp"]
    assert _cat(outs, "key") == [f"sensor_{int(x)}" for x in exp["key"]]
    assert np.array_equal(_cat(outs, "count"), exp["count"])
    assert np.array_equal(_cat(outs, "stddev_valid"), msk)
    m = msk.astype(bool)
    assert m.any()
    assert np.array_equal(_cat(outs, "stddev")[m], vals[m])


def test_global_op_and_merge_refusal():
    from denormalized_amd import WindowOp
    from denormalized_amd.distributed import merge_global_partials
    rng = np.random.default_rng(7009)
    n = 6_000
    ts = (1_000_000 + np.arange(n) // 2).astype(np.int64)  # 3 s span
    v = rng.uniform(-3, 115, n)
    op = WindowOp(length_ms=1000, no_group=True,
                  aggs=_aggs(["count", "min", "max", "sum", "var_samp"]))
    op.push(ts, None, v)
    op.finish()
    outs = op.poll_all()
    op.close()
    batches = [(ts, np.zeros(n, np.int64), v)]
    exp = run_oracle(1000, 0, batches)
    vals, msk = varref.expected(exp, batches)["var_samp"]
    assert all("key" not in b for b in outs)
    assert np.array_equal(_cat(outs, "count"), exp["count"])
    assert np.array_equal(_cat(outs, "var_samp_valid"), msk)
    assert msk.all() and np.array_equal(_cat(outs, "var_samp"), vals)
    with pytest.raises(ValueError, match="var_samp"):
        merge_global_partials([outs])


# --------------------------------------------------------- 11. error contract

def test_unknown_op_code_is_rejected():
    from denormalized_amd import _lib
    L = _lib.lib()
    aggs = (_lib.DzAggDesc * 2)()
    aggs[0].op, aggs[0].input_col = _lib.AGG_COUNT, 2
    aggs[1].op, aggs[1].input_col = 9, 2
    d = _lib.DzWindowDesc(
        window_type=_lib.WINDOW_TUMBLING, length_ms=1000, slide_ms=0,
        ts_col=0, group_col=1, key_kind=_lib.KEY_INT64,
        aggs=ctypes.cast(aggs, ctypes.POINTER(_lib.DzAggDesc)), n_aggs=2,
        n_keys_hint=16, device=0, max_open_windows=0)
    h = L.dz_window_op_create(ctypes.byref(d))
    assert not h
    msg = L.dz_last_error(None)
    assert msg and b"op code 9" in msg
    # every declared code is still accepted
    aggs[1].op = _lib.AGG_STDDEV_POP
    h = L.dz_window_op_create(ctypes.byref(d))
    assert h, L.dz_last_error(None)
    L.dz_window_op_destroy(h)
