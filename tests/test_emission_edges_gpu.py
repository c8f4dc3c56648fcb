"""Device emission chain at its own boundaries: live counts around the radix
block and scan-segment sizes on scratch a larger close left behind, sort keys
on and across the 11-bit digit and the 2^22 pass-count boundaries, group
chains of 1/2/16/16+1 closes with the close index on a digit boundary, the
element-capacity group cap, and the single-block sort. Streams and their
facts come from tests/emitvec.py (pinned on the CPU by
tests/test_emitvec_cpu.py); the reference is the C oracle, every column
BIT-EXACT in emission order; every case asserts through the engine's route
counters that the chain it targets ran, as often as its stream implies."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests import emitvec as ev
from tests.test_emission_paths_gpu import AGGS, _assert_all_columns
from tests.test_emitvec_cpu import built_case
from tests.test_gpu_parity import built, cat, make_op  # noqa: F401

pytestmark = pytest.mark.gpu


def _run(case):
    """Host pushes of dense ids, polling after every push so the passer
    hint is settled before the next trigger; (batches, kernel_stats)."""
    from denormalized_amd import _lib
    op = make_op(case.len_ms, case.slide_ms, key_kind=_lib.KEY_DENSE_INT64,
                 n_keys_hint=case.n_keys_hint, aggs=AGGS)
    if case.filt is not None:
        op.set_filter(*case.filt)
    outs = []
    for ts, kid, val in case.pushes:
        op.push(ts, kid, val)
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    stats = op.kernel_stats()
    op.close()
    return outs, stats


def _launches(stats, name):
    return stats[name]["launches"] if name in stats else 0


def _check(case, outs, stats, small_sort=False):
    f = case.facts
    exp = case.oracle.exp
    # one batch per close, in close order — empty where nothing passes (or
    # nothing was touched), as the host-built path delivers it
    assert [b["n_rows"] for b in outs] == [c.passing for c in f.closes]
    assert [int(b["window_start"][0]) for b in outs if b["n_rows"]] == \
        [c.start for c in f.closes if c.passing]
    keep = exp["count"] >= 2 if case.filt else None
    _assert_all_columns(SimpleNamespace(exp=exp), outs, "dense", keep)
    assert _launches(stats, "h_emit_group") == f.n_group_chains
    assert _launches(stats, "h_emit_group_closes") == f.n_group_closes
    assert _launches(stats, "h_emit_group_max") == f.group_max
    assert _launches(stats, "h_emit_perclose") == f.n_perclose
    assert _launches(stats, "h_emit_smallsort") == \
        (f.n_perclose if small_sort else 0)


@pytest.mark.parametrize("name", ["perclose_counts", "perclose_spans",
                                  "perclose_span22", "group_sizes",
                                  "group_span22", "group_cap"])
def test_emission_edges(built, name):
    case = built_case(name)
    outs, stats = _run(case)
    _check(case, outs, stats)
    if name == "group_cap":
        ws = [int(b["window_start"][0]) for b in outs if b["n_rows"]]
        assert ws == sorted(ws) and len(set(ws)) == len(ws)


def test_zero_passer_close_host_path(built):
    """The host-built path (<= 65,536 keys) delivers one batch per close,
    EMPTY when no group passes — the sequence the device chains are held to
    above."""
    from denormalized_amd import _lib
    op = make_op(1000, key_kind=_lib.KEY_DENSE_INT64, n_keys_hint=64,
                 aggs=AGGS)
    op.set_filter(*ev.FILTER)
    outs = []
    # window 0: three keys, one row each (none passes); window 2: one key
    # twice; window 3: one row, closed by finish()
    for ts, kid in (([0, 1, 2], [5, 6, 7]), ([2000, 2001], [9, 9]),
                    ([3000], [1])):
        op.push(np.array(ts, np.int64) + ev.T0, np.array(kid, np.int64),
                np.ones(len(ts)))
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    stats = op.kernel_stats()
    op.close()
    assert [b["n_rows"] for b in outs] == [0, 1, 0]
    assert _launches(stats, "h_emit_group") == 0
    assert _launches(stats, "h_emit_perclose") == 0


SMALL_CASES = ("small_counts", "perclose_spans")


def _small_sort_child(names, q):
    # the knob is read once per process, at the first per-close chain
    os.environ["DZ_EMIT_SMALL_MAX"] = str(1 << 30)
    for name in names:
        case = built_case(name)
        outs, stats = _run(case)
        _check(case, outs, stats, small_sort=True)
        assert case.facts.n_perclose > 0
        q.put((name, _launches(stats, "h_emit_smallsort")))


@pytest.mark.timeout(240)
def test_small_sort_child_process(built):
    """k_esort_small on (1, 1), (4097, 4097) and the 2^11 span closes (plus
    the 70,000-passer priming closes: "any nt"), in ONE fresh process that
    sets DZ_EMIT_SMALL_MAX; the child asserts the small-sort counter and
    bit-exactness, the parent its exit status."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_small_sort_child, args=(SMALL_CASES, q))
    p.start()
    p.join(200)
    if p.is_alive():
        p.kill()
        p.join(10)
        pytest.fail("small-sort child did not finish")
    assert p.exitcode == 0
    got = dict(q.get(timeout=10) for _ in SMALL_CASES)
    assert got == {n: built_case(n).facts.n_perclose for n in SMALL_CASES}
