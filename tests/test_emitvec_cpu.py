"""The emission-edge streams (tests/emitvec.py) against the C oracle, without
a GPU: every fact a GPU case depends on — touched and passing groups per
closing window, the push that closes it, its row span, the key bit-length,
cshift — is pinned here, together with each case's own claim (which
boundary it sits on)."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import pytest

from oracle import pyoracle
from tests import emitvec as ev


def oracle_run(case):
    """Push the case through the oracle, fetching after every push: the
    concatenated (read-only) output, which push emitted which rows, and the
    open-frame count after each push."""
    o = pyoracle.Oracle(case.len_ms, case.slide_ms)
    parts, open_after = [], []
    for ts, kid, val in case.pushes:
        o.push(ts, kid, val)
        parts.append(o.fetch())
        open_after.append(o.open_frames)
    o.finish()
    parts.append(o.fetch())
    o.close()
    exp = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    for a in exp.values():
        a.setflags(write=False)
    return SimpleNamespace(exp=exp, parts=parts, open_after=open_after)


@lru_cache(maxsize=None)
def built_case(name):
    case = ev.BUILDERS[name]()
    case.oracle = oracle_run(case)
    return case


def _oracle_closes(case):
    """(start, end, touched, passing, close_push) per window the oracle
    emitted, in emission order"""
    out = []
    for p, part in enumerate(case.oracle.parts):
        ws = part["window_start"]
        cut = np.flatnonzero(np.diff(ws)) + 1
        for lo, hi in zip(np.r_[0, cut], np.r_[cut, len(ws)]):
            if hi > lo:
                cnt = part["count"][lo:hi]
                out.append((int(ws[lo]), int(part["window_end"][lo]), hi - lo,
                            int((cnt >= 2).sum()) if case.filt else hi - lo,
                            p))
    return out


@pytest.mark.parametrize("name", sorted(ev.BUILDERS))
def test_facts_match_oracle(name):
    case = built_case(name)
    f = case.facts
    assert f.open_after == case.oracle.open_after
    mine = [(c.start, c.end, c.touched, c.passing, c.close_push)
            for c in f.closes if c.touched]
    assert mine == _oracle_closes(case)
    emitted = set(case.oracle.exp["window_start"].tolist())
    assert all(c.start not in emitted for c in f.closes if not c.touched)
    starts = [c.start for c in f.closes]
    assert len(set(starts)) == len(starts)
    # span: rows pushed from the batch that opened the frame (the oracle's
    # own window enumeration says which) through the batch that closed it
    cum = np.r_[0, np.cumsum([len(p[0]) for p in case.pushes])]
    opened = {}
    for p, (ts, _, _) in enumerate(case.pushes):
        ws, _ = pyoracle.windows_for_range(int(ts.min()), int(ts.max()),
                                           case.len_ms, case.slide_ms)
        for s in ws.tolist():
            opened.setdefault(s, p)
    for c in f.closes:
        hi = cum[min(c.close_push + 1, len(case.pushes))]
        assert c.span == hi - cum[opened[c.start]], c.start
        assert c.bits == int(c.span).bit_length()
    for t in f.triggers:
        assert [c for ch in t.chains for c in ch.closes] == t.closes
        # one trigger closes ascending windows
        ss = [f.closes[i].start for i in t.closes]
        assert ss == sorted(ss)
        for ch in t.chains:
            spans = [f.closes[i].span for i in ch.closes]
            assert ch.cshift == int(max(spans)).bit_length()
            assert all(s < (1 << ch.cshift) for s in spans)
    assert f.n_keys > ev.DEV_KEYS
    assert all(c.route in ("group", "perclose") for c in f.closes)


def _trigger_closes(f, t):
    return [f.closes[i] for i in f.triggers[t].closes]


def test_perclose_counts_claim():
    f = built_case("perclose_counts").facts
    assert ev.scan_bs(f.n_keys) == 2
    pairs = ev.count_pairs()
    assert set(pairs) >= {(1, 0), (1, 1), (4095, 4095), (4096, 4096),
                          (4097, 4097), (4097, 1), (8192, 4096),
                          (8191, 8191), (8192, 8192), (8193, 8193)}
    assert [t.route for t in f.triggers] == ["group", "perclose", "perclose",
                                             "group"]
    prime = _trigger_closes(f, 1)
    assert [c.stream for c in prime] == [0, 1, 2, 3]
    nblk = -(-f.n_keys // ev.RCHUNK)
    assert all(-(-c.passing // ev.RCHUNK) == nblk for c in prime), \
        "priming closes fill every histogram row"
    edge = _trigger_closes(f, 2)
    assert [(c.touched, c.passing) for c in edge] == pairs + [(0, 0), (5, 3)]
    assert len(f.triggers[2].chains) == 1
    seen = {c.stream: c.passing for c in prime}
    for c in edge:  # a larger close ran before it on the same scratch
        assert seen[c.stream] > c.passing
        seen[c.stream] = max(seen[c.stream], c.passing)
    assert f.n_perclose == 4 + len(edge)
    assert (f.n_group_chains, f.n_group_closes, f.group_max) == (2, 2, 1)


def test_perclose_spans_claim():
    f = built_case("perclose_spans").facts
    pc = [c for c in f.closes if c.route == "perclose"]
    assert [c.span for c in pc] == [2047, 2048, 2049, 2051]
    assert [c.bits for c in pc] == [11, 12, 12, 12]
    assert all(ev.radix_passes(c.span) == 2 for c in pc)
    assert [c.max_key for c in pc] == [2044, 2045, 2046, 2048]
    assert [c.max_key >> ev.RDIG for c in pc] == [0, 0, 0, 1]
    assert f.n_perclose == 4 and f.n_group_chains == 2 * 4


def _late_groups(case, push):
    """keys of a big-window push whose first row lies past offset 2^22, and
    every key's first offset within the push"""
    kid = case.pushes[push][1]
    uniq, first = np.unique(kid, return_index=True)
    return uniq[first >= (1 << 22)], dict(zip(uniq.tolist(), first.tolist()))


@pytest.mark.parametrize("name,push", [("perclose_span22", 1),
                                       ("group_span22", 0)])
def test_span22_claim(name, push):
    case = built_case(name)
    f = case.facts
    (big,) = [c for c in f.closes
              if c.start == int(case.pushes[push][0].min())]
    assert (1 << 22) < big.span < (1 << 22) + 200_000
    assert ev.radix_passes((1 << 22) - 1) == 2
    late, first = _late_groups(case, push)
    exp = case.oracle.exp
    sel = exp["window_start"] == big.start
    keys = exp["key"][sel][exp["count"][sel] >= 2]
    assert big.passing == len(keys)
    n_late = int(np.isin(keys, late).sum())
    assert n_late >= 64
    # insertion order puts the late groups last; their low 22 bits do not
    assert np.isin(keys[-n_late:], late).all()
    low = np.array([first[k] & ((1 << 22) - 1) for k in keys.tolist()])
    by_low = keys[np.argsort(low, kind="stable")]
    assert not np.isin(by_low[-n_late:], late).any()
    assert big.max_key >= (1 << 22)
    ch = f.triggers[big.trigger].chains[big.chain]
    if name == "perclose_span22":
        assert big.route == "perclose" and ev.radix_passes(big.span) == 4
    else:
        assert big.route == "group" and big.pos == 0
        assert len(ch.closes) == 3 and ch.cshift == 23 and ch.passes == 4
        assert ch.max_first == big.span
        assert all(f.closes[i].span < 4096 for i in ch.closes[1:])


def test_group_sizes_claim():
    f = built_case("group_sizes").facts
    assert all(t.route == "group" for t in f.triggers)
    sizes = [[len(ch.closes) for ch in t.chains] for t in f.triggers]
    assert [1] in sizes and [2] in sizes and [16] in sizes
    assert [16, 1] in sizes
    two = [ch for t in f.triggers for ch in t.chains if len(ch.closes) == 2]
    assert sorted(ch.cshift for ch in two) == [ev.RDIG, ev.RDIG + 1]
    (g16,) = [ch for t in f.triggers for ch in t.chains
              if len(t.chains) == 1 and len(ch.closes) == 16]
    cl = [f.closes[i] for i in g16.closes]
    assert any(c.touched == 0 for c in cl)
    assert any(c.touched and c.passing == 0 for c in cl)
    assert any(c.passing == 1 < c.touched for c in cl)
    assert any(c.passing == c.touched > 1 for c in cl)
    assert any(c.passing >= ev.VIEW_ROWS for c in cl)
    assert any(c.passing == ev.VIEW_ROWS - 1 for c in cl)
    assert f.n_perclose == 0 and f.group_max == 16


def test_group_cap_claim():
    f = built_case("group_cap").facts
    assert ev.E_GELEMS // f.kcap == 13
    (t,) = [t for t in f.triggers if t.push == 1]
    assert t.route == "group" and len(t.closes) == 20
    assert [len(ch.closes) for ch in t.chains] == [13, 7]
    assert f.rows < 1000
    assert f.group_max == 13 and f.n_perclose == 0
    assert f.n_group_closes == len(f.closes)


def test_small_counts_claim():
    f = built_case("small_counts").facts
    pc = [(c.touched, c.passing) for c in f.closes if c.route == "perclose"]
    assert (4097, 4097) in pc and (1, 1) in pc
