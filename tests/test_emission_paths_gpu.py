"""Emission-path characterisation: every packed-row route of the engine
(group-batched chain served as views, per-close chain zero-copy, per-close
chain materialising, raw-slab per-close host build) against the CPU oracle,
BIT-EXACT on every column, with the aggregates declared out of canonical
order and with a repeat so a column-mapping or layout-offset mistake cannot
hide behind the default order."""
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import pyoracle
from tests.test_gpu_parity import _CMP_FN, built, cat, make_op  # noqa: F401

pytestmark = pytest.mark.gpu

NK = 70_000          # > 65,536 (device paths) and > 16,384 (zero-copy rows)
RPM = 140            # rows per ms: a 1 s window holds 2 * NK rows
WROWS = 1000 * RPM
T0 = 1_000_000
TAIL_ROWS = 2_000    # window 3
TAIL_KEYS = 1_000

# out of canonical order, `sum` twice. The second sum is declared by its op
# code so the wrapper labels its column "3" instead of overwriting "sum".
AGG_SUM_CODE = 3
AGGS = (("avg", 0), ("sum", 0), ("count", 0), ("max", 0), ("min", 0),
        (AGG_SUM_CODE, 0))
COLS = (("avg", "avg"), ("sum", "sum"), ("count", "count"), ("max", "max"),
        ("min", "min"), (str(AGG_SUM_CODE), "sum"))


@pytest.fixture(scope="module")
def stream():
    """The shared stream, its push cuts and the oracle's (read-only) result,
    plus the per-kind key tables — all built once per module."""
    rng = np.random.default_rng(7070)
    perm = rng.permutation(NK)
    n = 3 * WROWS + TAIL_ROWS
    ts = (T0 + np.arange(n) // RPM).astype(np.int64)
    # windows 0-2: every full window touches all NK keys (twice)
    kid = perm[np.arange(n) % NK].astype(np.int64)
    kid[3 * WROWS:] = perm[np.arange(TAIL_ROWS) % TAIL_KEYS]
    val = rng.uniform(0, 115, n)
    # push 1 = windows 0-1 + first row of window 2 (two closes, one trigger,
    #          cold passer hint: group-batched chain, both slices views)
    # push 2 = rest of window 2 + first row of window 3 (hint now NK:
    #          per-close chain, zero-copy build)
    # push 3 = rest of window 3; finish() closes it (per-close chain,
    #          TAIL_KEYS rows: materialising build)
    cuts = (0, 2 * WROWS + 1, 3 * WROWS + 1, n)
    o = pyoracle.Oracle(1000, 0)
    for lo, hi in zip(cuts, cuts[1:]):
        o.push(ts[lo:hi], kid[lo:hi], val[lo:hi])
    o.finish()
    exp = o.fetch()
    o.close()
    for a in exp.values():
        a.setflags(write=False)
    names = [f"sensor_{i}" for i in range(NK)]
    return SimpleNamespace(
        ts=ts, kid=kid, val=val, cuts=cuts, exp=exp, names=names,
        names_arr=np.array(names, dtype=object),
        # sparse, negative and positive, injective in the dense id
        i64_vals=np.arange(NK, dtype=np.int64) * 1_000_003 - 35_000_000_000)


def _run(st, kind, filt=None):
    """Push the stream through one op of the given key kind, polling after
    every push; returns (batches, kernel_stats)."""
    from denormalized_amd import DeviceArray, _lib
    ts, kid, val, cuts = st.ts, st.kid, st.val, st.cuts
    key_kind = {"dense": _lib.KEY_DENSE_INT64, "int64": _lib.KEY_INT64,
                "utf8": _lib.KEY_UTF8}[kind]
    op = make_op(1000, key_kind=key_kind, n_keys_hint=NK, aggs=AGGS)
    if filt is not None:
        op.set_filter(*filt)
    outs = []
    for lo, hi in zip(cuts, cuts[1:]):
        if kind == "dense":
            bufs = []
            for a in (ts[lo:hi], kid[lo:hi].astype(np.int32), val[lo:hi]):
                d = DeviceArray(0, a.nbytes)
                d.from_host(np.ascontiguousarray(a))
                bufs.append(d)
            op.push_device(hi - lo, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
            outs += op.poll_all()  # drains the deferred push: inputs consumed
            for d in bufs:
                d.free()
        else:
            keys = (st.i64_vals[kid[lo:hi]] if kind == "int64"
                    else st.names_arr[kid[lo:hi]].tolist())
            op.push(ts[lo:hi], keys, val[lo:hi])
            outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    stats = op.kernel_stats()
    op.close()
    return outs, stats


def _assert_all_columns(st, outs, kind, keep=None):
    exp = st.exp
    sel = slice(None) if keep is None else keep
    ek = exp["key"][sel]
    got_key = cat(outs, "key")
    if kind == "utf8":
        assert list(got_key) == [st.names[k] for k in ek]
    elif kind == "int64":
        assert np.array_equal(np.asarray(got_key), st.i64_vals[ek]), "keys/order"
    else:
        assert np.array_equal(np.asarray(got_key), ek), "keys/order"
    for got_name, exp_name in COLS:
        g = cat(outs, got_name)
        e = exp[exp_name][sel]
        assert g.dtype == e.dtype and np.array_equal(g, e), \
            f"column {got_name!r} (oracle {exp_name!r}) not bit-exact"
    assert np.array_equal(cat(outs, "valid"), exp["valid"][sel]), "validity"
    assert np.array_equal(cat(outs, "window_start"), exp["window_start"][sel])
    assert np.array_equal(cat(outs, "window_end"), exp["window_end"][sel])


@pytest.mark.parametrize("kind", ["dense", "int64", "utf8"])
def test_packed_paths_all_columns(stream, kind):
    assert len(stream.exp["key"]) == 3 * NK + TAIL_KEYS
    outs, stats = _run(stream, kind)
    assert [b["n_rows"] for b in outs] == [NK, NK, NK, TAIL_KEYS]
    _assert_all_columns(stream, outs, kind)
    # the engine counts every route: the first trigger's two closes (cold
    # passer hint, NK > the 65,536 group threshold, slices > the 16,384 view
    # threshold) share ONE group-batched chain; windows 2 and 3 each take a
    # per-close chain, whose two builds are counted as well
    assert stats["h_emit_group"]["launches"] == 1
    assert stats["h_emit_group_closes"]["launches"] == 2
    assert stats["h_emit_perclose"]["launches"] == 2
    assert stats["h_emit_smallsort"]["launches"] == 0
    assert stats["h_emit_zc"]["launches"] >= 1
    assert stats["h_emit_copybuild"]["launches"] >= 1


def test_packed_paths_filter_sum_gt_median(stream):
    exp = stream.exp
    q = float(np.quantile(exp["sum"], 0.5))
    keep = _CMP_FN[">"](exp["sum"], q)
    assert 0 < keep.sum() < len(keep)
    outs, _ = _run(stream, "int64", filt=("sum", ">", q))
    _assert_all_columns(stream, outs, "int64", keep)


def test_raw_slab_per_close_host_path():
    # key capacity > 65,536 (no pinned group buffers) while the live key count
    # stays <= 65,536 (no device chain): each close copies its raw slab and
    # the worker sorts, filters and builds on the host.
    rng = np.random.default_rng(5050)
    rows, nwin, nk = 2_000, 3, 50
    n = rows * nwin
    ts = (T0 + (np.arange(n) // rows) * 1000 + (np.arange(n) % rows) // 4
          ).astype(np.int64)
    # keys 0..39 repeat; keys 40..49 appear exactly once per window so that
    # `count >= 2` splits the groups
    j = np.arange(n) % rows
    kid = np.where(j < rows - 10, j % 40, 40 + j - (rows - 10)).astype(np.int64)
    val = rng.uniform(0, 115, n)
    keys = kid * 1_000_003 - 20_000_000
    o = pyoracle.Oracle(1000, 0)
    op = make_op(1000, n_keys_hint=NK, aggs=AGGS)
    op.set_filter("count", ">=", 2.0)
    outs = []
    for w in range(nwin):
        sl = slice(w * rows, (w + 1) * rows)
        op.push(ts[sl], keys[sl], val[sl])
        outs += op.poll_all()
        o.push(ts[sl], kid[sl], val[sl])
    op.finish()
    outs += op.poll_all()
    o.finish()
    exp = o.fetch()
    op.close()
    o.close()
    assert len(exp["key"]) == nwin * nk
    keep = exp["count"] >= 2
    assert 0 < keep.sum() < len(keep)
    assert np.array_equal(np.asarray(cat(outs, "key")),
                          exp["key"][keep] * 1_000_003 - 20_000_000)
    for got_name, exp_name in COLS:
        assert np.array_equal(cat(outs, got_name), exp[exp_name][keep]), got_name
    assert np.array_equal(cat(outs, "valid"), exp["valid"][keep])
    assert np.array_equal(cat(outs, "window_start"), exp["window_start"][keep])
    assert np.array_equal(cat(outs, "window_end"), exp["window_end"][keep])
