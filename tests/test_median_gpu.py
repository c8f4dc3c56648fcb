"""GPU parity of the median aggregate against the numpy restatement
(tests/medianref.py) layered on the CPU oracle's rows. The median does not
depend on row order, so every value is asserted at tolerance 0
(np.array_equal on the rows whose `valid` is 1; equal_nan only where a test
injects NaN). Masks, keys and their order, window columns and the base
aggregates are compared exactly against the oracle. The kernel edges (the
LDS/global split of the select, a value log's first allocation) are read
from dz_debug_median_caps, not hard-coded."""
import struct

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import pyoracle
from tests import medianref, varref

pytestmark = pytest.mark.gpu

T0 = 1_000_000
EXAMPLE = ["count", "min", "max", "avg", "median", "stddev"]
BASE5 = ["count", "min", "max", "avg", "median"]


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


@pytest.fixture(scope="module")
def caps():
    from denormalized_amd import _lib
    return _lib.median_caps()


def _cat(outs, field):
    arrs = [b[field] for b in outs]
    if not arrs:
        return np.zeros(0)
    if isinstance(arrs[0], list):
        return [x for a in arrs for x in a]
    return np.concatenate(arrs)


def _collect(op, names, outs):
    fields = ["valid", "window_start", "window_end"] + list(names)
    if not op.no_group:
        fields.append("key")
    fields += [n + "_valid" for n in names if n in varref.ALIASES]
    return {f: np.asarray(_cat(outs, f)) for f in fields}


def run_gpu(len_ms, slide_ms, batches, names, valids=None, filt=None,
            n_keys_hint=64, stats=None, **kw):
    """Host-push `batches` through a WindowOp declaring `names`."""
    from denormalized_amd import WindowOp, _lib
    kw.setdefault("key_kind", _lib.KEY_INT64)
    op = WindowOp(length_ms=len_ms, slide_ms=slide_ms,
                  aggs=[(n, 0) for n in names], n_keys_hint=n_keys_hint, **kw)
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
    if stats is not None:
        stats.update(op.kernel_stats())
    got = _collect(op, names, outs)
    op.close()
    return got


def run_oracle(len_ms, slide_ms, batches, valids=None):
    o = pyoracle.Oracle(len_ms, slide_ms)
    for bi, (ts, k, v) in enumerate(batches):
        vv = valids[bi] if valids is not None else None
        o.push(ts, k, v, None if vv is None else np.asarray(vv, np.uint8))
    o.finish()
    exp = o.fetch()
    o.close()
    return exp


def assert_rows(got, exp, med, names, equal_nan=False, keep=None,
                has_key=True):
    """Row set/order, window columns, masks and base aggregates vs the
    oracle; the median vs the reference, tolerance 0. keep: expected rows
    that pass a pushed-down filter."""
    mvals, mmask = med
    sel = np.ones(len(exp["valid"]), bool) if keep is None else keep
    assert sel.sum() > 0
    if has_key:
        assert np.array_equal(got["key"], exp["key"][sel]), "keys/order"
    assert np.array_equal(got["window_start"], exp["window_start"][sel])
    assert np.array_equal(got["window_end"], exp["window_end"][sel])
    assert np.array_equal(got["valid"], exp["valid"][sel]), "validity"
    assert np.array_equal(mmask, exp["valid"]), "median NULL-ness is valid's"
    v = exp["valid"][sel].astype(bool)
    for f in names:
        if f == "count":
            assert np.array_equal(got[f], exp[f][sel]), f
        elif f == "median":
            print("median rows", int(v.sum()), "mismatches",
                  int((got[f][v] != mvals[sel][v]).sum()))
            assert np.array_equal(got[f][v], mvals[sel][v],
                                  equal_nan=equal_nan), "median"
        elif f in ("min", "max", "avg", "sum"):
            assert np.array_equal(got[f][v], exp[f][sel][v],
                                  equal_nan=equal_nan), f


def gen_batches(seed, nbatches, rows, nkeys, rows_per_ms, t0=T0):
    return [pyoracle.gen(seed, t0, b * rows, rows, nkeys, rows_per_ms)
            for b in range(nbatches)]


def one_window(groups, rng, t0=T0, span=1000):
    """One batch inside [t0, t0 + span): `groups` is a list of value arrays,
    group g under key g; rows interleaved at random, ts non-decreasing."""
    keys = np.concatenate([np.full(len(g), i, np.int64)
                           for i, g in enumerate(groups)])
    vals = np.concatenate([np.asarray(g, np.float64) for g in groups])
    p = rng.permutation(len(keys))
    ts = t0 + (np.arange(len(keys), dtype=np.int64) * span) // len(keys)
    return ts, keys[p], vals[p]


# ------------------------------------------------ 1. the example as written

@pytest.fixture(scope="module")
def small_stream():
    batches = gen_batches(1, 4, 10_000, 37, 10)
    exp = run_oracle(1000, 0, batches)
    return (batches, exp, medianref.expected(exp, batches),
            varref.expected(exp, batches))


def test_example_as_written(small_stream):
    batches, exp, med, var = small_stream
    got = run_gpu(1000, 0, batches, EXAMPLE)
    assert_rows(got, exp, med, EXAMPLE)
    vals, msk = var["stddev_samp"]
    assert np.array_equal(got["stddev_valid"], msk)
    m = msk.astype(bool)
    assert np.array_equal(got["stddev"][m], vals[m])


def test_example_through_datastream_with_filter(small_stream):
    import denormalized_amd as dz
    batches, exp, med, var = small_stream
    src = [{"occurred_at_ms": ts, "sensor_name": k, "reading": v}
           for ts, k, v in batches]
    lit = float(np.median(exp["max"]))
    outs = (dz.Context(device=0).from_batches(src)
            .window(["sensor_name"], [(n, "reading") for n in EXAMPLE],
                    1000, None)
            .filter("max", ">", lit).collect())
    keep = exp["valid"].astype(bool) & (exp["max"] > lit)
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(_cat(outs, "key"), exp["key"][keep])
    assert np.array_equal(_cat(outs, "count"), exp["count"][keep])
    assert np.array_equal(_cat(outs, "max"), exp["max"][keep])
    assert np.array_equal(_cat(outs, "median"), med[0][keep])
    assert np.array_equal(_cat(outs, "stddev"), var["stddev_samp"][0][keep])
    assert not any("median_valid" in b for b in outs)


# ------------------------------------------------------ 2. small n and ties

def test_small_groups_ties_and_all_null_group():
    rng = np.random.default_rng(2)
    sizes = [1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129]
    groups = [rng.normal(50.0, 10.0, s) for s in sizes]
    groups.append(np.full(10, 7.5))                       # all equal
    groups.append(np.array([3.0] * 9 + [1e9]))            # repeats + outlier
    groups.append(np.array([1.0, 2.0, 3.0, 4.0, 5.0]))    # every row NULL
    null_key = len(groups) - 1
    ts, k, v = one_window(groups, rng)
    valid = (k != null_key).astype(np.uint8)
    batches, valids = [(ts, k, v)], [valid]
    exp = run_oracle(1000, 0, batches, valids)
    med = medianref.expected(exp, batches, valids)
    got = run_gpu(1000, 0, batches, BASE5, valids=valids)
    assert_rows(got, exp, med, BASE5)
    r = int(np.flatnonzero(exp["key"] == null_key)[0])
    assert got["valid"][r] == 0 and got["count"][r] == 0  # emitted, NULL
    assert got["median"][r] == 0.0
    assert med[0][int(np.flatnonzero(exp["key"] == null_key - 1)[0])] == 3.0


# ------------------------------------------------------- 3. path boundary

def test_lds_global_path_boundary(caps):
    L = caps[0]
    rng = np.random.default_rng(3)
    sizes = [L - 1, L, L + 1, 2 * L + 3, 2 * L + 4]
    assert {s % 2 for s in sizes if s <= L} == {0, 1}
    assert {s % 2 for s in sizes if s > L} == {0, 1}
    perm = rng.permutation(sum(sizes)).astype(np.float64)
    groups = np.split(perm, np.cumsum(sizes)[:-1])
    batches = [one_window(groups, rng)]
    exp = run_oracle(1000, 0, batches)
    med = medianref.expected(exp, batches)
    got = run_gpu(1000, 0, batches, BASE5)
    assert_rows(got, exp, med, BASE5)


# --------------------------------------------------------- 4. total order

def _f(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def test_total_order_special_values():
    ninf, inf = -np.inf, np.inf
    nnan, pnan = _f(0xFFF8000000000000), _f(0x7FF8000000000000)
    groups = [
        [nnan, 1.0, 2.0],             # -NaN sorts first: 1
        [pnan, 1.0, 2.0],             # +NaN sorts last: 2
        [-0.0, 0.0],                  # (-0 + +0) / 2 = +0
        [ninf, inf],                  # NaN
        [1e308, 1e308],               # inf
        [-1.0, 0.0, -0.0, 1.0],       # middles are -0.0 then +0.0
        [inf, nnan, 5.0, pnan, ninf],  # 5
        [0.0, -0.0, -0.0],            # -0.0: the second of -0, -0, +0
    ]
    rng = np.random.default_rng(4)
    batches = [one_window([np.array(g) for g in groups], rng)]
    exp = run_oracle(1000, 0, batches)
    med = medianref.expected(exp, batches)
    names = ["count", "median"]
    got = run_gpu(1000, 0, batches, names)
    assert_rows(got, exp, med, names, equal_nan=True)
    by_key = {int(k): got["median"][i] for i, k in enumerate(got["key"])}
    assert by_key[0] == 1.0 and by_key[1] == 2.0 and by_key[6] == 5.0
    assert np.isnan(by_key[3]) and by_key[4] == np.inf
    bits = lambda x: struct.unpack("<Q", struct.pack("<d", x))[0]
    assert bits(by_key[2]) == bits(0.0)
    assert bits(by_key[5]) == bits(0.0)
    assert bits(by_key[7]) == bits(-0.0)
    # non-NaN rows are bit-identical to the reference
    ok = ~np.isnan(med[0])
    assert np.array_equal(got["median"][ok].view(np.uint64),
                          med[0][ok].view(np.uint64))


# ------------------------------------------- 5. log growth and slot reuse

def test_log_growth_and_slot_reuse(caps):
    G = caps[1]
    rng = np.random.default_rng(5)
    batches = []
    t = T0
    for rows in (1, G - 1, 2, 3 * G):       # one window, grown twice
        ts = np.sort(rng.integers(t, t + 200, rows)).astype(np.int64)
        batches.append((ts, rng.integers(0, 3, rows).astype(np.int64),
                        rng.normal(0.0, 1.0, rows)))
        t += 200
    for w, rows in enumerate((900, 700, 500, 300, 100, 7), start=1):
        ts = np.sort(rng.integers(T0 + w * 1000, T0 + (w + 1) * 1000, rows))
        batches.append((ts.astype(np.int64),
                        rng.integers(0, 3, rows).astype(np.int64),
                        rng.normal(float(w), 1.0, rows)))
    exp = run_oracle(1000, 0, batches)
    assert len(set(exp["window_start"].tolist())) == 7
    med = medianref.expected(exp, batches)
    # 7 windows over the operator's 4 initial slots: slots are reused, and a
    # reused slot holds fewer rows than it did
    got = run_gpu(1000, 0, batches, BASE5, max_open_windows=4)
    assert_rows(got, exp, med, BASE5)


# ---------------------------------------------------------------- 6. sliding

def test_sliding_every_window(caps):
    rng = np.random.default_rng(6)
    n = 2100                                  # one row per ms: every window's
    ts_all = T0 + np.arange(n, dtype=np.int64)  # start and end-1 carry a row
    k_all = rng.integers(0, 5, n).astype(np.int64)
    v_all = rng.normal(20.0, 5.0, n)
    cuts = [0, 650, 1430, n]                  # batches straddle window edges
    batches = [(ts_all[a:b], k_all[a:b], v_all[a:b])
               for a, b in zip(cuts[:-1], cuts[1:])]
    exp = run_oracle(500, 100, batches)
    assert int(exp["count"].sum()) == 5 * n   # each row in 5 windows
    med = medianref.expected(exp, batches)
    got = run_gpu(500, 100, batches, BASE5)
    assert_rows(got, exp, med, BASE5)
    assert int(got["count"].sum()) == 5 * n


# ------------------------------------------- 7. many windows in one batch

def test_many_windows_in_one_batch():
    rng = np.random.default_rng(7)
    n = 300 * 40
    ts = T0 + (np.arange(n, dtype=np.int64) * 100) // 40  # 300 x 100 ms
    batches = [(ts, rng.integers(0, 20, n).astype(np.int64),
                rng.normal(0.0, 3.0, n))]
    exp = run_oracle(100, 0, batches)
    assert len(set(exp["window_start"].tolist())) == 300
    med = medianref.expected(exp, batches)
    got = run_gpu(100, 0, batches, BASE5)
    assert_rows(got, exp, med, BASE5)


# ------------------------------------------------------ 8. many small groups

def test_many_small_groups():
    rng = np.random.default_rng(8)
    nk = 70_000
    reps = rng.integers(1, 4, nk)
    keys = np.repeat(np.arange(nk, dtype=np.int64), reps)
    p = rng.permutation(len(keys))
    keys = keys[p]
    n = len(keys)
    ts = T0 + (np.arange(n, dtype=np.int64) * 1000) // n
    batches = [(ts, keys, rng.normal(0.0, 1.0, n))]
    exp = run_oracle(1000, 0, batches)
    assert len(exp["key"]) == nk
    med = medianref.expected(exp, batches)
    stats = {}
    got = run_gpu(1000, 0, batches, BASE5, n_keys_hint=nk, stats=stats)
    assert_rows(got, exp, med, BASE5)
    # emission stays host-built past 65536 keys
    assert stats["h_emit_perclose"]["launches"] == 0
    assert stats["h_emit_group"]["launches"] == 0
    assert stats["med_select"]["launches"] == 1


# ------------------------------------------------------------ 9. device pushes

def _dev(arr):
    from denormalized_amd import DeviceArray
    arr = np.ascontiguousarray(arr)
    d = DeviceArray(0, max(arr.nbytes, 8))
    d.from_host(arr)
    return d


@pytest.fixture(scope="module")
def device_stream():
    batches = gen_batches(9, 3, 3000, 23, 4)
    exp = run_oracle(1000, 0, batches)
    med = medianref.expected(exp, batches)
    host = run_gpu(1000, 0, batches, BASE5)
    assert_rows(host, exp, med, BASE5)
    return batches, host


@pytest.mark.parametrize("kind", ["staged", "borrowed", "utf8", "i64"])
def test_device_pushes_match_host_push(device_stream, kind):
    from denormalized_amd import WindowOp, _lib
    batches, host = device_stream
    kk = {"staged": _lib.KEY_DENSE_INT64, "borrowed": _lib.KEY_DENSE_INT64,
          "utf8": _lib.KEY_UTF8, "i64": _lib.KEY_INT64}[kind]
    op = WindowOp(length_ms=1000, aggs=[(n, 0) for n in BASE5], key_kind=kk,
                  n_keys_hint=64)
    held, outs = [], []
    for ts, k, v in batches:
        n = len(ts)
        d_ts, d_v = _dev(ts), _dev(v)
        held += [d_ts, d_v]
        if kind in ("staged", "borrowed"):
            d_k = _dev(k.astype(np.int32))
            held.append(d_k)
            op.push_device(n, d_ts.ptr, d_k.ptr, d_v.ptr,
                           borrowed=(kind == "borrowed"))
        elif kind == "utf8":
            names = [f"sensor_{int(x)}".encode() for x in k]
            offs = np.zeros(n + 1, np.int32)
            np.cumsum([len(x) for x in names], out=offs[1:])
            d_o = _dev(offs)
            d_d = _dev(np.frombuffer(b"".join(names), np.uint8))
            held += [d_o, d_d]
            op.push_device_utf8(n, d_ts.ptr, d_o.ptr, d_d.ptr, d_v.ptr)
        else:
            d_k = _dev(k * 7919 - 5)
            held.append(d_k)
            op.push_device_i64(n, d_ts.ptr, d_k.ptr, d_v.ptr)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    op.close()
    for d in held:
        d.free()
    key = _cat(outs, "key")
    if kind == "utf8":
        key = np.array([int(s.split("_")[1]) for s in key], np.int64)
    elif kind == "i64":
        key = (np.asarray(key) + 5) // 7919
    assert np.array_equal(key, host["key"])
    for f in ("count", "valid", "window_start", "median", "min", "max", "avg"):
        assert np.array_equal(_cat(outs, f), host[f]), f


# ------------------------------------------------------- 10. global window

def test_global_window_global_memory_path(caps):
    from denormalized_amd.distributed import merge_global_partials
    from denormalized_amd import WindowOp
    L = caps[0]
    raw = gen_batches(10, 3, 8000, 5, 10)
    batches = [(ts, np.zeros(len(ts), np.int64), v) for ts, _k, v in raw]
    exp = run_oracle(1000, 0, batches)
    assert exp["count"].min() > L       # every group takes the global path
    med = medianref.expected(exp, batches)
    op = WindowOp(length_ms=1000, aggs=[(n, 0) for n in BASE5], no_group=True)
    outs = []
    for ts, _k, v in batches:
        op.push(ts, None, v)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    got = _collect(op, BASE5, outs)
    op.close()
    assert_rows(got, exp, med, BASE5, has_key=False)
    with pytest.raises(ValueError, match="median"):
        merge_global_partials([outs])


# ---------------------------------------- 11. filter matrix on the median

@pytest.mark.parametrize("with_stddev", [False, True])
def test_filter_matrix_on_median(small_stream, with_stddev):
    batches, exp, med, _var = small_stream
    mvals, mmask = med
    m = mmask.astype(bool)
    names = BASE5 + (["stddev"] if with_stddev else [])
    cmps = {"<": np.less, "<=": np.less_equal, ">": np.greater,
            ">=": np.greater_equal, "==": np.equal, "!=": np.not_equal}
    # the median of the expected medians, and (so that == selects a row)
    # their upper-middle element
    lits = [medianref.median(mvals[m])[0], float(np.sort(mvals[m])[m.sum() // 2])]
    for lit in lits:
        for cmp, fn in cmps.items():
            keep = m & fn(mvals, lit)
            got = run_gpu(1000, 0, batches, names, filt=("median", cmp, lit))
            if keep.sum() == 0:
                assert len(got["valid"]) == 0, cmp
                continue
            assert_rows(got, exp, med, names, keep=keep)
    assert (m & (mvals == lits[1])).sum() >= 1


# --------------------------------------------------------- 12. error contract

def test_error_contract():
    from denormalized_amd import WindowOp, _lib
    for code in (9, 15, 17):
        with pytest.raises(RuntimeError, match=f"op code {code}"):
            WindowOp(length_ms=1000, aggs=[(code, 0)],
                     key_kind=_lib.KEY_INT64)
    with pytest.raises(RuntimeError, match="median"):
        WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64,
                 aggs=[("median", 2, "m"), ("min", 3, "other_min")])
    # a refused create leaves the library usable
    ts = np.array([T0, T0 + 1, T0 + 2], np.int64)
    got = run_gpu(1000, 0, [(ts, np.zeros(3, np.int64),
                             np.array([3.0, 1.0, 2.0]))], ["median"])
    assert got["median"].tolist() == [2.0]
