"""GPU parity of int64 value columns (dz_window_op_set_value_type /
WindowOp(value_dtype="int64")) against the pure Python reference
tests/intref.py. Tolerance 0 everywhere: integer columns are compared as
integers, f64 columns by their bits; masks and the row set/order exactly."""
import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import pyoracle
from tests import intref

pytestmark = pytest.mark.gpu

I64_MAX, I64_MIN = 2**63 - 1, -2**63
P53 = 2**53
PIN = [P53, P53 + 1, -P53 - 1, I64_MAX, I64_MIN]     # the precision pin
VAR4 = {"var_samp": "var_samp", "var_pop": "var_pop",
        "stddev": "stddev_samp", "stddev_pop": "stddev_pop"}
BASE = ["count", "min", "max", "sum", "avg"]
ALL = BASE + list(VAR4)


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _i64(x):
    return np.array(x, np.int64)


def _bitmap(valid):
    return np.packbits(np.asarray(valid, np.uint8), bitorder="little")


def _dev(arrs):
    from denormalized_amd import DeviceArray
    out = []
    for a in arrs:
        a = np.ascontiguousarray(a)
        d = DeviceArray(0, max(8, a.nbytes))
        if a.nbytes:
            d.from_host(a)
        out.append(d)
    return out


def run_gpu(via, len_ms, slide_ms, batches, names, valids=None, filt=None,
            n_keys_hint=64, value_dtype="int64", stats=None, **kw):
    """Push `batches` [(ts, keys, values), ...] through one op over the push
    path `via`; returns the emitted rows concatenated per column, keys as
    int64 whatever the path's key kind."""
    from denormalized_amd import WindowOp, _lib
    kind = {"host": _lib.KEY_INT64, "dense": _lib.KEY_DENSE_INT64,
            "staged": _lib.KEY_DENSE_INT64, "borrowed": _lib.KEY_DENSE_INT64,
            "utf8": _lib.KEY_UTF8, "i64": _lib.KEY_INT64,
            "global": _lib.KEY_INT64}[via]
    op = WindowOp(length_ms=len_ms, slide_ms=slide_ms,
                  aggs=[(n, 0) for n in names], key_kind=kind,
                  n_keys_hint=n_keys_hint, value_dtype=value_dtype,
                  no_group=(via == "global"), **kw)
    if filt is not None:
        op.set_filter(*filt)
    outs, keep = [], []
    for bi, (ts, k, v) in enumerate(batches):
        ts, n = _i64(ts), len(ts)
        if via in ("host", "dense", "global"):
            bm = None
            if valids is not None and valids[bi] is not None:
                bm = _bitmap(valids[bi])
            op.push(ts, None if via == "global" else _i64(k), v, bm)
        else:
            assert valids is None, "device pushes carry no primary bitmap"
            v = np.ascontiguousarray(
                v, np.int64 if value_dtype == "int64" else np.float64)
            if via in ("staged", "borrowed"):
                d = _dev([ts, np.asarray(k, np.int32), v])
                op.push_device(n, d[0].ptr, d[1].ptr, d[2].ptr,
                               borrowed=(via == "borrowed"))
            elif via == "i64":
                d = _dev([ts, _i64(k), v])
                op.push_device_i64(n, d[0].ptr, d[1].ptr, d[2].ptr)
            else:
                enc = [b"k%d" % int(x) for x in k]
                offs = np.zeros(n + 1, np.int32)
                np.cumsum([len(e) for e in enc], out=offs[1:])
                d = _dev([ts, offs, np.frombuffer(b"".join(enc), np.uint8), v])
                op.push_device_utf8(n, d[0].ptr, d[1].ptr, d[2].ptr, d[3].ptr)
            keep.append(d)   # borrowed until the next call into the op
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    if stats is not None:
        stats.update(op.kernel_stats())
    op.close()
    for d in keep:
        for a in d:
            a.free()
    fields = ["valid", "window_start", "window_end"] + list(names) + \
        [n + "_valid" for n in names if n in VAR4]
    if via != "global":
        fields.append("key")
    got = {}
    for f in fields:
        arrs = [b[f] for b in outs]
        if f == "key" and via == "utf8":
            got[f] = _i64([int(s[1:]) for a in arrs for s in a])
        else:
            got[f] = np.concatenate(arrs) if arrs else np.zeros(0)
    return got


def assert_rows(got, ref, names, keys=True):
    assert len(ref["count"]) > 0
    if keys:
        assert np.array_equal(got["key"], ref["key"]), "keys / order"
    assert np.array_equal(got["window_start"], ref["window_start"])
    assert np.array_equal(got["window_end"], ref["window_end"])
    assert np.array_equal(got["valid"], ref["valid"]), "validity"
    v = ref["valid"].astype(bool)
    for f in names:
        if f == "count":
            assert got[f].dtype == np.int64
            assert np.array_equal(got[f], ref[f]), f
        elif f in ("min", "max", "sum"):
            assert got[f].dtype == np.int64, f + " is not an int64 column"
            assert np.array_equal(got[f][v], ref[f][v]), f
        elif f == "avg":
            assert np.array_equal(_bits(got[f][v]), _bits(ref[f][v])), f
        else:
            r = VAR4[f]
            assert np.array_equal(got[f + "_valid"], ref[r + "_valid"]), f
            m = ref[r + "_valid"].astype(bool)
            assert np.array_equal(_bits(got[f][m]), _bits(ref[r][m])), \
                f + " not bit-exact"


def check(via, len_ms, slide_ms, batches, names=BASE, valids=None, **kw):
    ref = intref.run(len_ms, slide_ms, batches, valids,
                     no_group=(via == "global"))
    got = run_gpu(via, len_ms, slide_ms, batches, names, valids, **kw)
    assert_rows(got, ref, names, keys=(via != "global"))
    return got, ref


# ----------------------------------------------------------- 1. precision pin

def test_precision_pin():
    """Fails on an f64 value column: 2**53 + 1 is not a double."""
    wrap = [I64_MAX, I64_MAX, 5]                      # sums past 2**63 twice
    ts = [5000] * (len(PIN) + len(wrap))
    keys = [1] * len(PIN) + [2] * len(wrap)
    got, ref = check("host", 1000, 0, [(ts, keys, _i64(PIN + wrap))])
    assert got["min"].tolist() == [I64_MIN, 5]
    assert got["max"].tolist() == [I64_MAX, I64_MAX]
    assert got["sum"].tolist() == [P53 - 1, 3]        # both mod 2**64
    want = 0.0
    for v in PIN:
        want += float(v)
    assert _bits([got["avg"][0]])[0] == _bits([want / 5.0])[0]
    # a group where only the integer compare separates max from its neighbour
    got, _ = check("host", 1000, 0, [([5000, 5001], [1, 1],
                                      _i64([P53, P53 + 1]))])
    assert got["max"][0] == P53 + 1 and got["min"][0] == P53


def test_datastream_window_passes_value_dtype():
    import denormalized_amd as dz
    src = [{"occurred_at_ms": _i64([5000] * len(PIN)),
            "sensor_name": _i64([3] * len(PIN)), "reading": _i64(PIN)}]
    aggs = [("min", "reading"), ("max", "reading"), ("sum", "reading")]
    ds = dz.Context(device=0).from_batches(src)
    out = ds.window(["sensor_name"], aggs, 1000, None,
                    value_dtype="int64").collect()
    assert [int(out[0][f][0]) for f in ("min", "max", "sum")] == \
        [I64_MIN, I64_MAX, P53 - 1]
    # no dtype sniffing: the default casts the same integers to f64
    out = ds.window(["sensor_name"], aggs, 1000, None).collect()
    assert out[0]["max"].dtype == np.float64
    assert out[0]["max"][0] == float(I64_MAX)


# --------------------------------------------------------- 2. walk-group edges

def test_walk_group_edges():
    """Groups of 1, 7, 8, 9, 15, 16, 17 valid rows in one supertile (the
    walk reads 8 records at a time), and a NULL as the first, the last and
    the only row of a group. Dense keys that are multiples of 512 share
    bucket 0, so all the groups are bins of one block's one supertile."""
    rng = np.random.default_rng(21)
    keys, valid = [], []
    for k, n in enumerate([1, 7, 8, 9, 15, 16, 17]):
        keys += [k] * n
        valid += [1] * n
    for k, pat in ((10, [0, 1, 1]), (11, [1, 1, 0]), (12, [0]),
                   (13, [0] + [1] * 8), (14, [1] * 8 + [0])):
        keys += [k] * len(pat)
        valid += pat
    perm = rng.permutation(len(keys))     # interleave the groups' rows
    keys, valid = np.array(keys)[perm] * 512, np.array(valid)[perm]
    n = len(keys)
    assert n < 2048
    vals = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    vals[::5] = P53 + rng.integers(-3, 4, len(vals[::5]))
    check("dense", 1000, 0, [(np.full(n, 7000), keys, vals)], ALL,
          valids=[valid], n_keys_hint=15 * 512)


# ----------------------------------------------------------- 3. supertile seam

def test_supertile_seam_and_lazy_seed():
    """One key per row count around ST_RECORDS = 2048 in one batch; a second
    batch continues the same window, so every accumulator (the f64-sum cell
    included) is seeded from the slab."""
    rng = np.random.default_rng(22)
    counts = {0: 2047, 512: 2048, 1024: 2049, 1536: 4097}  # all in bucket 0
    keys = np.concatenate([np.full(c, k) for k, c in counts.items()])
    rng.shuffle(keys)
    n = len(keys)

    def vals(m):
        v = rng.integers(-2**62, 2**62, m, dtype=np.int64)
        v[::3] = P53 + 1 + 2 * rng.integers(0, 1000, len(v[::3]))
        return v
    b1 = (np.full(n, 9000), keys, vals(n))
    b2 = (np.full(300, 9500), keys[:300], vals(300))
    b3 = (np.full(4, 11_000), keys[:4], vals(4))           # closes the window
    check("dense", 1000, 0, [b1, b2, b3], ALL, n_keys_hint=2048)
    check("staged", 1000, 0, [b1, b2, b3], ALL, n_keys_hint=2048)


# ------------------------------------------------ 4. direct vs two-level fold

def _stream(seed, n, nkeys, span_ms, t0=1_000_000):
    rng = np.random.default_rng(seed)
    ts = t0 + (np.arange(n) * span_ms // n).astype(np.int64)
    keys = rng.integers(0, nkeys, n)
    vals = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    vals[::4] = P53 + rng.integers(-5, 6, len(vals[::4]))
    valid = (rng.random(n) < 0.95).astype(np.uint8)
    return ts, keys, vals, valid


def test_direct_fold_three_keys():
    ts, keys, vals, valid = _stream(23, 20_000, 3, 2500)
    h = len(ts) // 2
    st = {}
    check("host", 1000, 0, [(ts[:h], keys[:h], vals[:h]),
                            (ts[h:], keys[h:], vals[h:])], ALL,
          valids=[valid[:h], valid[h:]], stats=st)
    assert st["regfold"]["launches"] > 0
    assert st.get("regroup", {"launches": 0})["launches"] == 0


def test_two_level_fold_large_key_ids():
    """Max key id >= 131,072: klocs * nws > FOLD_GCAP, so the batch goes
    through RG_L1 and the int64 RG_L2_FOLD."""
    nk = 131_073
    ts, keys, vals, valid = _stream(24, 200_000, nk, 1800)
    keys[0] = nk - 1
    h = len(ts) // 2
    st = {}
    _, ref = check("dense", 1000, 0, [(ts[:h], keys[:h], vals[:h]),
                                      (ts[h:], keys[h:], vals[h:])], ALL,
                   valids=[valid[:h], valid[h:]], n_keys_hint=nk, stats=st)
    assert ref["key"].max() >= 131_072
    assert st["regroup"]["launches"] > 0, "the two-level fold was not taken"


def test_sliding_500_100():
    ts, keys, vals, valid = _stream(25, 30_000, 300, 2000)
    t = len(ts) // 3
    cuts = [(0, t), (t, 2 * t), (2 * t, len(ts))]
    check("host", 500, 100, [(ts[a:b], keys[a:b], vals[a:b])
                             for a, b in cuts], ALL,
          valids=[valid[a:b] for a, b in cuts], n_keys_hint=512)


# ------------------------------------------------------------ 5. slot recycling

def test_slot_recycling_shows_no_stale_state():
    """4 open windows at most, 16 windows in the stream: every slot is reused
    three times. Later windows hold strictly larger minima and strictly
    smaller maxima (and f64 sums of another magnitude), so any min / max /
    fsum / Welford cell surviving a recycle would show."""
    nwin, per, nk = 16, 600, 5
    rng = np.random.default_rng(26)
    batches = []
    for w in range(nwin):
        lo, hi = -P53 * 8 + w * 1000, P53 * 8 - w * 1000
        vals = rng.integers(lo, hi, per, dtype=np.int64, endpoint=True)
        vals[:nk], vals[nk:2 * nk] = lo, hi
        keys = np.arange(per) % nk
        batches.append((np.full(per, 50_000 + w * 1000), keys, vals))
    got, _ = check("host", 1000, 0, batches, ALL, max_open_windows=4)
    mins = got["min"].reshape(nwin, nk)
    maxs = got["max"].reshape(nwin, nk)
    assert np.all(np.diff(mins, axis=0) > 0) and np.all(np.diff(maxs, axis=0) < 0)


# ----------------------------------------------------------- 6. every push path

@pytest.fixture(scope="module")
def path_stream():
    ts, keys, vals, _ = _stream(27, 12_000, 40, 2600)
    t = len(ts) // 3
    batches = [(ts[a:b], keys[a:b], vals[a:b])
               for a, b in ((0, t), (t, 2 * t), (2 * t, len(ts)))]
    return batches, intref.run(1000, 0, batches)


@pytest.mark.parametrize("via", ["host", "staged", "borrowed", "utf8", "i64"])
def test_every_push_path(path_stream, via):
    batches, ref = path_stream
    got = run_gpu(via, 1000, 0, batches, ALL, n_keys_hint=64)
    assert_rows(got, ref, ALL)


# ------------------------------------------------- 7. variance family on ints

def test_variance_family_near_2_53_and_small():
    rng = np.random.default_rng(28)
    n = 4000
    keys = rng.integers(0, 6, n)
    vals = np.where(keys < 3, P53 - 50 + rng.integers(0, 100, n),
                    rng.integers(-9, 10, n)).astype(np.int64)
    # one-row groups (the _samp forms are NULL) and an all-NULL group
    keys = np.concatenate([keys, [100, 101, 102]])
    vals = np.concatenate([vals, _i64([P53 + 1, -3, 44])])
    valid = np.ones(len(keys), np.uint8)
    valid[-1] = 0
    ts = np.full(len(keys), 3000)
    names = ["stddev", "count", "var_pop", "var_samp", "stddev_pop", "avg"]
    got, ref = check("host", 1000, 0, [(ts, keys, vals)], names,
                     valids=[valid])
    one = np.isin(ref["key"], [100, 101])
    assert np.all(got["var_samp_valid"][one] == 0)
    assert np.all(got["var_pop_valid"][one] == 1)
    assert got["var_pop_valid"][ref["key"] == 102][0] == 0


# -------------------------------------------------------------------- 8. filter

CMPS = {"<": np.less, "<=": np.less_equal, ">": np.greater,
        ">=": np.greater_equal, "==": np.equal, "!=": np.not_equal}


@pytest.fixture(scope="module")
def filter_stream():
    # key k: max 100 + k, sum 99 + k; key 20: max 2**53 + 2; key 30: all NULL
    keys, vals, valid = [], [], []
    for k in range(8):
        keys += [k, k]
        vals += [-1, 100 + k]
        valid += [1, 1]
    keys += [20, 20, 30]
    vals += [P53 + 2, -5, 7]
    valid += [1, 1, 0]
    batches = [(np.full(len(keys), 4000), _i64(keys), _i64(vals))]
    return batches, [np.array(valid, np.uint8)], \
        intref.run(1000, 0, batches, [valid])


@pytest.mark.parametrize("cmp", list(CMPS))
@pytest.mark.parametrize("field,lit", [
    ("max", 103.5), ("sum", 102.5),          # between two distinct values
    ("max", float(P53 + 2)),                 # exactly (double)v, v > 2**53
    ("max", 103.0), ("sum", 102.0)])         # exactly a small value
def test_filter_on_int_columns(filter_stream, cmp, field, lit):
    batches, valids, ref = filter_stream
    got = run_gpu("host", 1000, 0, batches, BASE, valids, filt=(field, cmp, lit))
    keep = ref["valid"].astype(bool) & CMPS[cmp](
        ref[field].astype(np.float64), lit)
    assert keep.sum() < len(keep)
    assert not keep[ref["key"] == 30][0], "a NULL group passed"
    if not keep.any():    # e.g. == a literal between two values
        assert len(got["count"]) == 0
        return
    ref = {k: v[keep] for k, v in ref.items()}
    assert_rows(got, ref, BASE)


# -------------------------------------------------------------------- 9. global

def test_global_window_over_the_pin():
    ts = [5000 + i for i in range(len(PIN))] + [6100]
    vals = _i64(PIN + [42])
    got, _ = check("global", 1000, 0, [(ts, None, vals)], ALL)
    assert got["max"].tolist() == [I64_MAX, 42]
    assert got["min"].tolist() == [I64_MIN, 42]
    assert got["sum"].tolist() == [P53 - 1, 42]


# ----------------------------------------------------------------- 10. refusals

def _f64_roundtrip(op):
    """the op still aggregates f64 values as before"""
    ts, kid, val = pyoracle.gen(3, 1_000_000, 0, 2000, 9, 4)
    op.push(ts, kid, val)
    op.finish()
    outs = op.poll_all()
    o = pyoracle.Oracle(1000, 0)
    o.push(ts, kid, val)
    o.finish()
    exp = o.fetch()
    o.close()
    assert np.array_equal(np.concatenate([b["key"] for b in outs]), exp["key"])
    assert np.array_equal(np.concatenate([b["count"] for b in outs]),
                          exp["count"])
    got_max = np.concatenate([b["max"] for b in outs])
    assert got_max.dtype == np.float64
    assert np.array_equal(got_max, exp["max"])


def test_setter_refusals_leave_the_op_usable():
    from denormalized_amd import WindowOp, _lib
    aggs = [("count", 0), ("max", 0)]
    seen = set()

    def refused(op, col, vt, pattern):
        with pytest.raises(RuntimeError, match=pattern) as e:
            op.set_value_type(col, vt)
        msg = str(e.value)
        assert msg not in seen, "two causes share a message"
        seen.add(msg)

    op = WindowOp(length_ms=1000, aggs=aggs, key_kind=_lib.KEY_INT64)
    op.set_value_type(0, _lib.VALUE_F64)                 # no-op on a fresh op
    refused(op, 0, 7, "unknown value type")
    refused(op, 1, _lib.VALUE_INT64, "value_col")
    _f64_roundtrip(op)
    refused(op, 0, _lib.VALUE_INT64, "before the operator's first push")
    op.close()

    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64,
                  aggs=[("count", 2, "c"), ("max", 2, "max"),
                        ("max", 3, "m3")])
    refused(op, 0, _lib.VALUE_INT64, "single value column")
    ts = _i64([1000, 1001])
    op.push(ts, _i64([1, 1]), [np.array([1.5, 2.5]), np.array([7.0, 3.0])])
    op.finish()
    b = op.poll_all()[0]
    assert b["max"].tolist() == [2.5] and b["m3"].tolist() == [7.0]
    op.close()

    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64,
                  aggs=[("median", 0), ("max", 0)])
    refused(op, 0, _lib.VALUE_INT64, "median")
    op.push(_i64([1000, 1001, 1002]), _i64([1, 1, 1]), [1.0, 9.0, 2.5])
    op.finish()
    b = op.poll_all()[0]
    assert b["median"].tolist() == [2.5] and b["max"].tolist() == [9.0]
    op.close()
    with pytest.raises(RuntimeError, match="median"):
        WindowOp(length_ms=1000, aggs=[("median", 0)], value_dtype="int64")


# --------------------------------------------------------- 11. non-interference

def test_default_op_still_casts_integers_to_f64(path_stream):
    """A default (f64) op fed the same integer rows rounds them through f64
    exactly as before: it equals the oracle on the f64 cast of the stream."""
    batches, _ = path_stream
    names = ["count", "min", "max", "avg"]
    got = run_gpu("host", 1000, 0, batches, names, value_dtype="float64")
    o = pyoracle.Oracle(1000, 0)
    for ts, k, v in batches:
        o.push(ts, k, v.astype(np.float64))
    o.finish()
    exp = o.fetch()
    o.close()
    assert np.array_equal(got["key"], exp["key"])
    assert np.array_equal(got["count"], exp["count"])
    for f in ("min", "max", "avg"):
        assert got[f].dtype == np.float64
        assert np.array_equal(_bits(got[f]), _bits(exp[f])), f
