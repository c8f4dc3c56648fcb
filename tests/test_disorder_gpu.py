"""GPU tests of late and out-of-order rows through the variance family, the
median, int64 value columns and several value columns.

Two behaviours are pinned for every family: rows may arrive in any timestamp
order and each (window, key) group still folds them in row order, and a row
older than the watermark re-creates its closed frame, which is emitted again
at once holding only the late rows. The expectation is tests/streamref.py (a
row-list model, tied to the C oracle and to varref / medianref / intref by
tests/test_streamref_cpu.py); two value columns go through
tests/multicolref.py. Tolerance 0 everywhere: integer columns and masks with
np.array_equal, f64 columns on their uint64 views where the mask is 1 (NaN by
position), rows in emitted order. Every case asserts its own precondition on
the reference output, so a generator change cannot turn it into a
sorted-stream test."""
import numpy as np
import pytest

import __graft_entry__ as graft
from tests import emitvec, medianref, streamref
from tests import multicolref as mc
from tests.pyref import windows_for_range

pytestmark = pytest.mark.gpu

T0 = 1_000_000
VAR4 = {"var_samp": "var_samp", "var_pop": "var_pop",
        "stddev": "stddev_samp", "stddev_pop": "stddev_pop"}
F64_SIX = ["count", "min", "max", "avg", "median", "stddev"]
F64_VAR = ["count", "min", "max", "sum", "avg"] + list(VAR4)
FAMILIES = {                      # names, value dtype
    "F64_SIX": (F64_SIX, "float64"),
    "F64_VAR": (F64_VAR, "float64"),
    "I64_ALL": (F64_VAR, "int64"),
}
TWO = [("count", 0, "n0"), ("min", 0, "lo0"), ("max", 1, "hi1"),
       ("avg", 1, "avg1"), ("sum", 1, "sum1"), ("count", 1, "n1")]


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


@pytest.fixture(scope="module")
def caps():
    from denormalized_amd import _lib
    L, G = _lib.median_caps()[:2]
    print("median caps: L =", L, "G =", G)
    return L, G


# ------------------------------------------------------------------ plumbing

def _bitmap(valid):
    if valid is None:
        return None
    return np.packbits(np.asarray(valid, np.uint8), bitorder="little")


def _cat(outs, f):
    arrs = [np.asarray(b[f]) for b in outs]
    return np.concatenate(arrs) if arrs else np.zeros(0)


def _fields(names, no_group=False):
    return (["valid", "window_start", "window_end"] + list(names)
            + [n + "_valid" for n in names if n in VAR4]
            + ([] if no_group else ["key"]))


def run_gpu(fam, len_ms, slide_ms, batches, valids=None, filt=None,
            dense=False, no_group=False, n_keys_hint=64, stats=None,
            on_push=None, **kw):
    """Host-push `batches` [(ts, keys, values), ...] through one op of the
    family; the emitted rows concatenated per column, in emitted order.
    on_push(batch index, op) runs after every push."""
    from denormalized_amd import WindowOp, _lib
    names, dtype = FAMILIES[fam]
    op = WindowOp(length_ms=len_ms, slide_ms=slide_ms,
                  aggs=[(n, 0) for n in names],
                  key_kind=_lib.KEY_DENSE_INT64 if dense else _lib.KEY_INT64,
                  n_keys_hint=n_keys_hint, value_dtype=dtype,
                  no_group=no_group, **kw)
    if filt is not None:
        op.set_filter(*filt)
    outs = []
    for bi, (ts, k, v) in enumerate(batches):
        op.push(ts, None if no_group else k, v,
                _bitmap(None if valids is None else valids[bi]))
        if on_push is not None:
            on_push(bi, op)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    msg = op._L.dz_last_error(op._h)
    if stats is not None:
        stats.update(op.kernel_stats())
    op.close()
    assert not msg, msg
    return {f: _cat(outs, f) for f in _fields(names, no_group)}


def reference(fam, len_ms, slide_ms, batches, valids=None, no_group=False):
    """streamref's columns under the engine's names (stddev is
    stddev_samp)."""
    names, dtype = FAMILIES[fam]
    ref = streamref.run(len_ms, slide_ms, batches, valids, dtype=dtype,
                        no_group=no_group).fetch()
    for alias, canon in VAR4.items():
        ref[alias], ref[alias + "_valid"] = ref[canon], ref[canon + "_valid"]
    return ref


def _assert_bits(g, e, what):
    g = np.ascontiguousarray(g, np.float64)
    e = np.ascontiguousarray(e, np.float64)
    nan = np.isnan(e)
    assert np.array_equal(np.isnan(g), nan), what + " NaN positions"
    assert np.array_equal(g[~nan].view(np.uint64), e[~nan].view(np.uint64)), \
        what + " not bit-exact"


def assert_exact(got, ref, fam, no_group=False):
    names, dtype = FAMILIES[fam]
    assert len(ref["count"]) > 0
    if not no_group:
        assert np.array_equal(got["key"], ref["key"]), "keys / order"
    assert np.array_equal(got["window_start"], ref["window_start"])
    assert np.array_equal(got["window_end"], ref["window_end"])
    assert np.array_equal(got["valid"], ref["valid"]), "validity"
    v = ref["valid"].astype(bool)
    for f in names:
        if f == "count":
            assert np.array_equal(got[f], ref[f]), f
        elif f in VAR4:
            assert np.array_equal(got[f + "_valid"], ref[f + "_valid"]), \
                f + " mask"
            m = ref[f + "_valid"].astype(bool)
            _assert_bits(got[f][m], ref[f][m], f)
        elif dtype == "int64" and f in ("min", "max", "sum"):
            assert got[f].dtype == np.int64, f + " is not an int64 column"
            assert np.array_equal(got[f][v], ref[f][v]), f
        else:
            _assert_bits(got[f][v], ref[f][v], f)


def check(fam, len_ms, slide_ms, batches, valids=None, **kw):
    no_group = kw.get("no_group", False)
    ref = reference(fam, len_ms, slide_ms, batches, valids, no_group)
    got = run_gpu(fam, len_ms, slide_ms, batches, valids, **kw)
    assert_exact(got, ref, fam, no_group)
    return got, ref


def values(fam, rng, n, small=False):
    """Magnitudes spread over 13 decades (18 for integers): any other row
    order changes the bits of sum and m2. small: one-digit values."""
    if FAMILIES[fam][1] == "int64":
        if small:
            return rng.integers(-9, 10, n).astype(np.int64)
        return (rng.uniform(-1, 1, n) * 10.0 ** rng.integers(0, 19, n)
                ).astype(np.int64)
    if small:
        return rng.uniform(-9, 9, n)
    return rng.uniform(-1, 1, n) * 10.0 ** rng.integers(-6, 7, n)


def in_window(rng, w, rows, nkeys, fam, len_ms=1000):
    """An in-order batch inside tumbling window `w`."""
    ts = T0 + w * len_ms + np.sort(rng.integers(0, len_ms, rows))
    return (ts.astype(np.int64), rng.integers(0, nkeys, rows).astype(np.int64),
            values(fam, rng, rows))


def late_groups(ref, wstart=T0):
    """{key: (first row, second row)} of the pairs (wstart, key) the
    reference emitted twice."""
    return {g[1]: (rows[0], rows[1])
            for g, rows in streamref.twice(ref).items() if g[0] == wstart}


# ------------------------------------- 1. re-created frame, re-emitted group

LATE_KEYS = np.array([0, 1, 2, 3, 99], np.int64)   # 99 is new to the stream


def case1_stream(fam, seed=1001):
    """Windows 0..2 in order, 40 late rows at T0 + 100 (window 0 has closed)
    over four of its keys and one new key, then window 3."""
    rng = np.random.default_rng(seed)
    batches = [in_window(rng, w, 400, 8, fam) for w in range(3)]
    lk = LATE_KEYS[np.arange(40) % 5]
    rng.shuffle(lk)
    batches.append((np.full(40, T0 + 100, np.int64), lk,
                    values(fam, rng, 40, small=True)))
    batches.append(in_window(rng, 3, 300, 8, fam))
    return batches


def assert_case1_precondition(ref, batches, median=False, count="count"):
    lk, lv = batches[3][1], batches[3][2]
    tw = late_groups(ref)
    assert len(tw) >= 3, "fewer than 3 groups emitted twice"
    assert 99 not in tw and (ref["key"] == 99).sum() == 1
    for k, (r1, r2) in tw.items():
        assert r2 > r1 and ref[count][r1] > ref[count][r2]
        assert ref[count][r2] == (lk == k).sum() == 8, "late rows only"
        if median:
            assert ref["median"][r2] == medianref.median(lv[lk == k])[0]
    print("case 1: groups emitted twice:", len(tw))


@pytest.fixture(scope="module")
def case1_six():
    batches = case1_stream("F64_SIX")
    got, ref = check("F64_SIX", 1000, 0, batches)
    return batches, got, ref


@pytest.mark.parametrize("fam", ["F64_VAR", "I64_ALL"])
def test_recreated_frame_is_reemitted(fam):
    batches = case1_stream(fam)
    _, ref = check(fam, 1000, 0, batches)
    assert_case1_precondition(ref, batches)


def test_recreated_frame_is_reemitted_median(case1_six):
    batches, got, ref = case1_six         # compared inside the fixture
    assert_case1_precondition(ref, batches, median=True)
    for _k, (_r1, r2) in late_groups(ref).items():
        assert got["median"][r2] == ref["median"][r2]


def _two_col_batches(seed=1002):
    rng = np.random.default_rng(seed)
    out = []
    for ts, k, v in case1_stream("F64_VAR"):
        n = len(ts)
        cols = [v, rng.uniform(-1, 1, n) * 10.0 ** rng.integers(0, 9, n)]
        out.append((ts, k, cols, [None, rng.random(n) > 0.3]))
    return out


def test_recreated_frame_is_reemitted_two_columns():
    from denormalized_amd import WindowOp, _lib
    mb = _two_col_batches()
    exp = mc.expect(1000, 0, mb, TWO)
    assert_case1_precondition(
        exp, [(ts, k, c[0]) for ts, k, c, _v in mb], count="n0")
    ref1 = streamref.run(1000, 0, [(t, k, c) for t, k, c, _ in mb],
                         [v for _t, _k, _c, v in mb]).fetch(1)
    assert np.array_equal(ref1["count"], exp["n1"])   # the two references
    op = WindowOp(length_ms=1000, aggs=[(o, 2 + j, a) for o, j, a in TWO],
                  key_kind=_lib.KEY_INT64, n_keys_hint=64)
    outs = []
    for ts, k, cols, valids in mb:
        op.push(ts, k, cols, [_bitmap(v) for v in valids])
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    op.close()
    fields = ["key", "valid", "window_start", "window_end"]
    for _o, j, a in TWO:
        fields += [a] + ([a + "_valid"] if j != 0 else [])
    mc.assert_match({f: _cat(outs, f) for f in fields}, exp, TWO)


# ---------------------------------------------- 2. late, all-NULL re-creation

@pytest.mark.parametrize("fam", list(FAMILIES))
def test_late_all_null_recreation(fam):
    batches = case1_stream(fam, seed=2001)
    valids = [None, None, None, np.zeros(40, np.uint8), None]
    got, ref = check(fam, 1000, 0, batches, valids)
    tw = late_groups(ref)
    assert len(tw) >= 3
    second = [r2 for _r1, r2 in tw.values()]
    second.append(int(np.flatnonzero(ref["key"] == 99)[0]))
    print("case 2: all-NULL groups re-emitted:", len(second))
    for r in second:
        assert got["count"][r] == 0 and got["valid"][r] == 0
        for f in FAMILIES[fam][0]:
            if f in VAR4:
                assert got[f + "_valid"][r] == 0, f
        if "median" in got:
            assert got["median"][r] == 0.0


@pytest.mark.parametrize("fam", ["F64_SIX", "I64_ALL"])
def test_empty_frames_recreated_between_late_and_current_row(fam):
    """One current row (T0 + 5000) and one late row (T0 + 100) in one batch:
    window 0 is re-created for the late row, window 1 re-created empty,
    windows 3 and 4 created empty; the empty ones emit no rows."""
    rng = np.random.default_rng(2002)
    batches = [in_window(rng, w, 300, 6, fam) for w in range(3)]
    batches.append((np.array([T0 + 5000, T0 + 100], np.int64),
                    np.array([2, 4], np.int64), values(fam, rng, 2)))
    batches.append(in_window(rng, 6, 200, 6, fam))
    got, ref = check(fam, 1000, 0, batches)
    starts = ref["window_start"].tolist()
    assert list(late_groups(ref)) == [4]
    assert starts.count(T0) == 7 and starts.count(T0 + 5000) == 1
    assert starts.count(T0 + 1000) == 6          # once, not twice
    assert T0 + 3000 not in starts and T0 + 4000 not in starts
    # emitted order: the late frame, then window 2, 5, 6
    order = [s for i, s in enumerate(starts) if i == 0 or starts[i - 1] != s]
    assert order == [T0, T0 + 1000, T0, T0 + 2000, T0 + 5000, T0 + 6000]


# ------------------------- 3. append and close within one push, both paths

@pytest.mark.parametrize("which", ["select_paths", "log_grows"])
def test_append_and_close_within_one_push(caps, which):
    L, G = caps
    rng = np.random.default_rng(3001)
    na, nb = (L + 1, L - 1) if which == "select_paths" else (G + 1, 0)
    assert na + nb <= 10_000
    batches = [in_window(rng, w, 300, 4, "F64_SIX") for w in range(3)]
    lk = np.repeat(np.array([1, 77], np.int64), [na, nb])
    rng.shuffle(lk)
    batches.append((np.full(na + nb, T0 + 100, np.int64), lk,
                    values("F64_SIX", rng, na + nb)))
    batches.append(in_window(rng, 3, 300, 4, "F64_SIX"))
    stats = {}
    got, ref = check("F64_SIX", 1000, 0, batches, stats=stats)
    # the late frame holds exactly the late rows and closed in their push:
    # it precedes window 2, which the next push closes
    r = int(np.flatnonzero((ref["window_start"] == T0)
                           & (ref["key"] == 1))[1])
    assert ref["count"][r] == na
    assert r < int(np.flatnonzero(ref["window_start"] == T0 + 2000)[0])
    if nb:
        r77 = np.flatnonzero(ref["key"] == 77)
        assert len(r77) == 1 and ref["count"][r77[0]] == nb
        assert na > L >= nb                      # one group per select path
    else:
        assert max(len(b[0]) for b in batches[:3]) < G < na
    assert stats["med_select"]["launches"] >= 1
    print("case 3:", which, "L =", L, "G =", G, "late rows", na, nb)


# --------------------------------------- 4. re-creation into a recycled slot

@pytest.mark.parametrize("fam", list(FAMILIES))
def test_recreation_into_recycled_slot(fam):
    rng = np.random.default_rng(4001)
    ints = FAMILIES[fam][1] == "int64"
    batches = []
    for w, rows in enumerate((900, 900, 500, 300, 100, 50, 20)):
        ts, k, v = in_window(rng, w, rows, 3, fam)
        if w < 2:                 # large magnitudes, many rows per group
            sign = rng.choice([-1, 1], rows)
            v = (sign * (2**62 + rng.integers(0, 1000, rows)) if ints
                 else sign * rng.uniform(1e12, 1e15, rows))
        batches.append((ts, k, v))
    for w, lk in ((0, [0, 2, 2, 0, 2, 0, 2]), (1, [1] * 7)):
        batches.append((np.full(7, T0 + w * 1000 + 100, np.int64),
                        np.array(lk, np.int64),
                        values(fam, rng, 7, small=True)))
    batches.append(in_window(rng, 7, 10, 3, fam))
    got, ref = check(fam, 1000, 0, batches, max_open_windows=4)
    assert len(set(ref["window_start"].tolist())) == 8
    for w, keys in ((0, [0, 2]), (1, [1])):
        tw = late_groups(ref, T0 + w * 1000)
        assert sorted(tw) == keys, "absent keys must not be re-emitted"
        sel = np.flatnonzero(ref["window_start"] == T0 + w * 1000)
        assert len(sel) == 3 + len(keys) and ref["count"][sel[3:]].sum() == 7
        for _r1, r2 in tw.values():
            assert abs(float(got["max"][r2])) < 10
            assert abs(float(got["min"][r2])) < 10
    print("case 4: groups emitted twice:",
          [len(late_groups(ref, T0 + w * 1000)) for w in (0, 1)],
          "in windows 0 and 1")


# ------------------------------- 5. re-creation while key capacity regrows

NEW_KEYS = 600     # with the 10 early keys: past the 512 the slabs start with


@pytest.mark.parametrize("fam", ["F64_SIX", "I64_ALL"])
def test_recreation_while_key_capacity_regrows(fam):
    rng = np.random.default_rng(5001)
    batches = [in_window(rng, w, 300, 10, fam) for w in range(3)]
    ts, k, v = in_window(rng, 3, 600, 10, fam)
    ts = np.sort(T0 + 3000 + rng.integers(0, 2000, 600)).astype(np.int64)
    batches.append((ts, k, v))                    # windows 3 and 4 stay open
    lk = np.concatenate([np.arange(1000, 1000 + NEW_KEYS), np.arange(0, 10)]
                        ).astype(np.int64)
    rng.shuffle(lk)
    batches.append((np.full(len(lk), T0 + 100, np.int64), lk,
                    values(fam, rng, len(lk), small=True)))
    batches.append(in_window(rng, 5, 300, 10, fam))
    # the key capacity is a multiple of 512 and at least 512, whatever the
    # hint: the late batch is the one that takes the key count past it
    before = len(np.unique(np.concatenate([b[1] for b in batches[:4]])))
    after = len(np.unique(np.concatenate([b[1] for b in batches[:5]])))
    assert emitvec.kcap_of(16) == emitvec.kcap_of(before) == 512
    assert before == 10 and after == 10 + NEW_KEYS
    assert emitvec.kcap_of(after) > 512
    got, ref = check(fam, 1000, 0, batches, n_keys_hint=16)
    tw = late_groups(ref)
    late_at = int(np.flatnonzero(ref["key"] >= 1000)[0])
    w0 = ref["window_start"] == T0
    assert len(tw) == 10 and (w0 & (ref["key"] >= 1000)).sum() == NEW_KEYS
    # windows 3 and 4 are open when the late batch regrows the slabs and are
    # emitted after it, from the copied state
    for w in (3, 4):
        first = int(np.flatnonzero(ref["window_start"] == T0 + w * 1000)[0])
        assert first > late_at
    assert (ref["window_start"] == T0 + 3000).sum() == 10
    assert (ref["window_start"] == T0 + 4000).sum() == 10
    print("case 5: groups emitted twice:", len(tw), "distinct keys", before,
          "->", after, "capacity", emitvec.kcap_of(before), "->",
          emitvec.kcap_of(after))


# ------------------------------------------------ 6. fully shuffled batches

def shuffled_batches(fam, seed=6001):
    rng = np.random.default_rng(seed)
    out = []
    for b in range(4):                # 2.5 s each, overlapping by 1 s
        n = 3000
        ts = rng.permutation(T0 + b * 1500 + np.arange(n) * 2500 // n)
        out.append((ts.astype(np.int64),
                    rng.integers(0, 12, n).astype(np.int64),
                    values(fam, rng, n)))
    return out


@pytest.mark.parametrize("len_ms,slide_ms", [(1000, 0), (500, 100)])
@pytest.mark.parametrize("fam", ["F64_VAR", "F64_SIX", "I64_ALL"])
def test_fully_shuffled_batches(fam, len_ms, slide_ms):
    batches = shuffled_batches(fam)
    frames = []
    for ts, _k, _v in batches:
        assert np.any(np.diff(ts) < 0)
        frames.append(len(windows_for_range(int(ts.min()), int(ts.max()),
                                            len_ms, slide_ms)))
    assert min(frames) >= 3
    print("case 6: frames per batch:", frames)
    check(fam, len_ms, slide_ms, batches)


# ------------------------------------ 7. one tile, many windows, shuffled

def test_one_tile_many_windows_shuffled():
    rng = np.random.default_rng(7001)
    n = 2048
    ts = T0 + rng.integers(0, 30_000, n)
    ts[:2] = [T0 + 29_999, T0]
    b1 = (ts.astype(np.int64), rng.integers(0, 20, n).astype(np.int64),
          values("F64_SIX", rng, n))
    b2 = (T0 + 30_000 + np.sort(rng.integers(0, 300, 500)).astype(np.int64),
          rng.integers(0, 20, 500).astype(np.int64),
          values("F64_SIX", rng, 500))
    assert len(windows_for_range(int(ts.min()), int(ts.max()), 100)) == 300
    got, ref = check("F64_SIX", 100, 0, [b1, b2])
    nwin = len(set(ref["window_start"][ref["window_start"] < T0 + 30_000]))
    assert nwin > 290                    # nearly every window holds rows
    print("case 7: non-empty windows of the shuffled tile:", nwin)


# --------------------------- 8. two-level fold, disordered, with variance

@pytest.mark.parametrize("fam", ["F64_VAR", "I64_ALL"])
def test_two_level_fold_disordered(fam):
    rng = np.random.default_rng(8001)
    nk = 70_000
    edge = np.repeat(np.arange(9), [1, 3, 4, 5, 7, 8, 9, 16, 17]) * 512
    fill = rng.integers(0, nk, 8000 - len(edge) - 1)
    k = np.concatenate([[nk - 1], edge, fill]).astype(np.int64)
    rng.shuffle(k)
    n = len(k)
    ts = (T0 + rng.integers(0, 2000, n)).astype(np.int64)
    valid = (rng.random(n) > 0.15).astype(np.uint8)
    assert np.any(np.diff(ts) < 0) and ts.min() < T0 + 1000 <= ts.max()
    stats = {}
    got, ref = check(fam, 1000, 0, [(ts, k, values(fam, rng, n))], [valid],
                     dense=True, n_keys_hint=nk, stats=stats)
    assert stats["regroup"]["launches"] > 0, "the two-level fold was not taken"
    assert ref["key"].max() == nk - 1 and (ref["valid"] == 0).any()
    print("case 8: groups:", len(ref["key"]))


# -------------------------------------- 9. device pushes lag by one batch

def _dev(arr):
    from denormalized_amd import DeviceArray
    arr = np.ascontiguousarray(arr)
    d = DeviceArray(0, max(arr.nbytes, 8))
    d.from_host(arr)
    return d


@pytest.mark.parametrize("kind", ["borrowed", "i64"])
def test_device_pushes_match_host_push(case1_six, kind):
    from denormalized_amd import WindowOp, _lib
    batches, host, ref = case1_six
    kk = _lib.KEY_DENSE_INT64 if kind == "borrowed" else _lib.KEY_INT64
    op = WindowOp(length_ms=1000, aggs=[(n, 0) for n in F64_SIX], key_kind=kk,
                  n_keys_hint=128)
    held, outs = [], []
    for ts, k, v in batches:
        d = [_dev(ts), _dev(k.astype(np.int32) if kind == "borrowed" else k),
             _dev(v)]
        held += d                    # borrowed until the next call on the op
        if kind == "borrowed":
            op.push_device(len(ts), d[0].ptr, d[1].ptr, d[2].ptr,
                           borrowed=True)
        else:
            op.push_device_i64(len(ts), d[0].ptr, d[1].ptr, d[2].ptr)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    op.close()
    for d in held:
        d.free()
    got = {f: _cat(outs, f) for f in _fields(F64_SIX)}
    assert len(late_groups(host)) >= 3           # the re-emission is there
    for f in _fields(F64_SIX):
        assert got[f].dtype == host[f].dtype, f
        if got[f].dtype == np.float64:
            assert np.array_equal(got[f].view(np.uint64),
                                  host[f].view(np.uint64)), f
        else:
            assert np.array_equal(got[f], host[f]), f


# ------------------------------------------ 10. filter on a re-emitted row

@pytest.mark.parametrize("field", ["median", "stddev"])
def test_filter_splits_a_reemitted_group(case1_six, field):
    batches, _got, ref = case1_six
    m = streamref.mask_of(ref, field)
    pick = None
    for k, (r1, r2) in late_groups(ref).items():
        a, b = float(ref[field][r1]), float(ref[field][r2])
        if m[r1] and m[r2] and a != b:
            pick = (k, r1, r2, ">" if a > b else "<", (a + b) / 2.0)
            break
    assert pick is not None
    k, r1, r2, cmp, lit = pick
    exp, keep = streamref.filter_rows(ref, field, cmp, lit)
    assert keep[r1] and not keep[r2] and 0 < keep.sum() < len(keep)
    got = run_gpu("F64_SIX", 1000, 0, batches, filt=(field, cmp, lit))
    assert_exact(got, exp, "F64_SIX")
    w0 = (got["window_start"] == T0) & (got["key"] == k)
    assert w0.sum() == 1
    print("case 10:", field, cmp, lit, "rows kept", int(keep.sum()),
          "of", len(keep))


# ---------------------------------------------------------- 11. global window

def test_global_window_recreated():
    batches = case1_stream("F64_SIX")
    got, ref = check("F64_SIX", 1000, 0, batches, no_group=True)
    tw = late_groups(ref)
    assert list(tw) == [0]
    r1, r2 = tw[0]
    assert ref["count"][r1] == 400 and ref["count"][r2] == 40
    assert ref["median"][r2] == medianref.median(batches[3][2])[0]
    assert ref["window_start"].tolist() == [T0, T0 + 1000, T0, T0 + 2000,
                                            T0 + 3000]
