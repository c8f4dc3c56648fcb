"""GPU tests of the sliding scatter (k_scatter_t<true>) at its tile and window
edges.

k_scatter_t<true> serves the sliding launches and the window-subrange splits; the
suite reached it only through workload-shaped streams whose slide divides the
snap unit and whose row counts sit far from any supertile edge. Every case
here is differential against tests/streamref.py (a row-list model, tied to
the C oracle and to varref / medianref / intref by tests/test_streamref_cpu.py,
on phase-drifting grids too), at tolerance 0 with the helpers of
tests/test_disorder_gpu.py: keys and emitted order, window columns, validity,
every aggregate on its bits where its mask is 1, every mask, and an empty
dz_last_error after finish() (the kernels' bounds-guard cell). Values spread
over 13 decades, so a record that moves to a neighbouring group or window, or
a group whose rows are reordered, changes the bits of sum, avg and m2. Every
case asserts its own precondition on the reference, on the window lists or on
kernel_stats(), so a generator change cannot turn it into an easy one.

The structural numbers are derived from len / slide and ST: expand =
ceil(len / slide) + 1 staged records per row at the most (one more than the
true multiplicity, on purpose), st_rows = ST // expand rows per supertile,
split over four wave quarters of ceil(rows / 4)."""
import numpy as np
import pytest

import __graft_entry__ as graft
from tests import multicolref as mc
from tests import streamref
from tests.pyref import windows_for_range
from tests.test_disorder_gpu import (F64_SIX, F64_VAR, T0, TWO, _bitmap, _cat,
                                     _dev, _fields, assert_exact, check,
                                     reference, values)

pytestmark = pytest.mark.gpu

ST = 2048           # dz::ST_RECORDS, denormalized_amd/csrc/dz_internal.h
WAVES = 4           # dz::WAVES_PER_BLOCK
SPLIT_WINDOWS = 256  # a batch list longer than this is cut into subranges


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


# ------------------------------------------------------------------ geometry

def geometry(len_ms, slide_ms):
    """(expand, st_rows) as process_batch derives them."""
    expand = -(-len_ms // slide_ms) + 1
    return expand, max(1, ST // expand)


def quarter_bounds(rows):
    """Row offsets [w0, w1, w2, w3, end] of the wave quarters of a supertile
    of `rows` rows."""
    q = -(-rows // WAVES)
    return [min(rows, w * q) for w in range(WAVES + 1)]


def chunks_of(n):
    """(chunk count, rows per chunk) of an n-row batch (stage_core)."""
    c = min(512, max(1, (n + 8191) // 8192))
    return c, -(-n // c)


def cover_of(ts, len_ms, slide_ms):
    """(starts of the batch's own window list, membership [row, window])."""
    ts = np.asarray(ts, np.int64)
    starts = np.array([s for s, _e in windows_for_range(
        int(ts.min()), int(ts.max()), len_ms, slide_ms)], np.int64)
    return starts, ((ts[:, None] >= starts[None, :])
                    & (ts[:, None] < starts[None, :] + len_ms))


def expected_records(len_ms, slide_ms, batches, valids=None):
    """Valid (row, window) pairs of the stream: what the counts must sum to."""
    tot = 0
    for bi, (ts, _k, _v) in enumerate(batches):
        m = cover_of(ts, len_ms, slide_ms)[1].sum(axis=1)
        ok = 1 if valids is None or valids[bi] is None else valids[bi]
        tot += int((m * ok).sum())
    return tot


def peak_open_frames(len_ms, slide_ms, batches):
    """The largest number of frames the reference holds open at once: the
    open frames plus the batch's new ones, before the batch's trigger."""
    r = streamref.StreamRef(len_ms, slide_ms)
    peak = 0
    for ts, k, v in batches:
        starts = cover_of(ts, len_ms, slide_ms)[0].tolist()
        peak = max(peak, len(set(r.frames) | set(starts)))
        r.push(ts, k, v)
    return peak


def spread(rng, n, base, span):
    """n unsorted timestamps in base + [0, span), both ends present."""
    ts = base + rng.integers(0, span, n)
    ts[0] = base
    if n > 1:
        ts[1] = base + span - 1
    return ts.astype(np.int64)


def window_rows(ref, start):
    return np.flatnonzero(ref["window_start"] == start)


# --------------------------------------------- 1. phase drift across batches

DRIFT_SHAPES = [(1000, 300), (700, 300), (1500, 400), (250, 100),
                (1000, 1000)]


def drift_batches(fam, seed=101):
    """Five in-order batches of 900 rows over 9 keys; batch b covers
    T0 + 137 + b * 1100 + [0, 1400). Neighbours among them overlap in time
    but, for (1000, 300) and (700, 300), never in phase (1100 is no multiple
    of 300), so a sixth batch follows 300 ms after the fifth: same anchor,
    overlapping range, and so starts that both batches reach."""
    rng = np.random.default_rng(seed)
    out = []
    for base in [T0 + 137 + b * 1100 for b in range(5)] + [T0 + 4837]:
        ts = np.sort(spread(rng, 900, base, 1400))
        out.append((ts, rng.integers(0, 9, 900).astype(np.int64),
                    values(fam, rng, 900)))
    return out


def assert_drift_precondition(len_ms, slide_ms, batches):
    lists = [cover_of(ts, len_ms, slide_ms)[0].tolist()
             for ts, _k, _v in batches]
    union = set().union(*lists)
    residues = {s % slide_ms for s in union}
    if slide_ms != len_ms:
        assert len(residues) >= 2, "the grid's phase never moved"
    # a merged frame: one start, rows from two batches
    merged = [s for s in union
              if sum(s in ls and bool(np.any((ts >= s) & (ts < s + len_ms)))
                     for ls, (ts, _k, _v) in zip(lists, batches)) >= 2]
    assert merged, "no start is reached from two batches"
    peak = peak_open_frames(len_ms, slide_ms, batches)
    assert peak <= 64, "more frames open than the default cap"
    print("case 1:", (len_ms, slide_ms), "residues", len(residues),
          "merged starts", len(merged), "peak open frames", peak)


@pytest.mark.parametrize("fam,len_ms,slide_ms",
                         [(f, l, s) for l, s in DRIFT_SHAPES
                          for f in ("F64_VAR", "F64_SIX")]
                         + [("I64_ALL", 1000, 300)])
def test_phase_drift_across_batches(fam, len_ms, slide_ms):
    batches = drift_batches(fam)
    assert_drift_precondition(len_ms, slide_ms, batches)
    _, ref = check(fam, len_ms, slide_ms, batches)
    assert ref["count"].sum() == expected_records(len_ms, slide_ms, batches)


def test_phase_drift_global_window():
    batches = drift_batches("F64_SIX", seed=102)
    assert_drift_precondition(1000, 300, batches)
    _, ref = check("F64_SIX", 1000, 300, batches, no_group=True)
    assert ref["count"].sum() == expected_records(1000, 300, batches)


# ------------------------------------------- 2. supertile and quarter edges

def edge_row_counts(len_ms, slide_ms):
    st = geometry(len_ms, slide_ms)[1]
    return [1, 3, st - 1, st, st + 1, 2 * st, 2 * st + 1, 8192, 8193]


def _supertile_case(len_ms, slide_ms, n):
    rng = np.random.default_rng(200 + n)
    batch = (spread(rng, n, T0 + 137, 700),
             rng.integers(0, 37, n).astype(np.int64),
             values("F64_VAR", rng, n))
    if n > 3:      # a window boundary inside the batch
        cover = cover_of(batch[0], len_ms, slide_ms)[1]
        assert len({c.tobytes() for c in cover}) >= 2
    stats = {}
    _, ref = check("F64_VAR", len_ms, slide_ms, [batch], stats=stats)
    assert stats["hist"]["launches"] >= 1, "not the sliding scatter's path"
    assert ref["count"].sum() == expected_records(len_ms, slide_ms, [batch])


@pytest.mark.parametrize("i", range(9))
def test_supertile_and_quarter_edges(i):
    expand, st = geometry(1000, 300)
    n = edge_row_counts(1000, 300)[i]
    q = quarter_bounds(st)
    sizes = [b - a for a, b in zip(q[:-1], q[1:])]
    assert len(set(sizes)) > 1, "the quarters of a full supertile are equal"
    assert quarter_bounds(1) == [0, 1, 1, 1, 1]        # three empty quarters
    if n == 8193:
        c, chunk = chunks_of(n)
        assert c == 2 and chunk % st != 0
    print("case 2: expand", expand, "st_rows", st, "quarters", sizes,
          "rows", n, "chunks", chunks_of(n))
    _supertile_case(1000, 300, n)


@pytest.mark.parametrize("extra", [0, 1])
def test_supertile_edges_full_quarters(extra):
    expand, st = geometry(1000, 350)
    q = quarter_bounds(st)
    assert expand == 4 and st * expand == ST
    assert len({b - a for a, b in zip(q[:-1], q[1:])}) == 1
    _supertile_case(1000, 350, st + extra)


# ------------------------------- 3. mixed multiplicity inside one wave step

@pytest.mark.parametrize("keys", ["four_keys_two_buckets", "one_key"])
def test_mixed_multiplicity_in_one_wave_step(keys):
    rng = np.random.default_rng(301)
    n = 64 * 5
    assert n < geometry(1000, 300)[1]                  # one supertile
    ts = np.where(np.arange(n) % 2 == 0, T0 + 250, T0 + 350).astype(np.int64)
    m = cover_of(ts, 1000, 300)[1].sum(axis=1)
    assert set(m[:64].tolist()) == {3, 4} == set(m.tolist())
    assert np.all(m[0::2] != m[1::2]), "the multiplicity does not alternate"
    if keys == "one_key":
        k = np.zeros(n, np.int64)
    else:       # dense ids: 0 and 512, 1 and 513 share a bucket (id & 511)
        k = rng.choice(np.array([0, 512, 1, 513], np.int64), n)
        for a in (0, 1):
            same = (k & 511) == a
            assert {3, 4} == set(m[:64][same[:64]].tolist())
    batch = (ts, k, values("F64_VAR", rng, n))
    _, ref = check("F64_VAR", 1000, 300, [batch], dense=True,
                   n_keys_hint=1024)
    assert ref["count"].sum() == int(m.sum())


# -------------------------------------------- 4. window-edge and clamp rows

def edge_batch(len_ms, slide_ms, span, seed):
    """Rows at start, start + len - 1 and start + len of three consecutive
    grid windows, each under a key of its own (100 + 3 * window + edge), one
    row at the batch minimum, one at the maximum, and filler over 5 keys."""
    rng = np.random.default_rng(seed)
    mn, mx = T0 + 137, T0 + 137 + span
    wins = windows_for_range(mn, mx, len_ms, slide_ms)
    inner = [s for s, e in wins if s > mn and e + 1 <= mx]
    assert len(inner) >= 3
    picked = inner[len(inner) // 2 - 1:len(inner) // 2 + 2]
    ts, k = [mn, mx], [0, 1]
    for i, s in enumerate(picked):
        ts += [s, s + len_ms - 1, s + len_ms]
        k += [100 + 3 * i, 101 + 3 * i, 102 + 3 * i]
    fill = rng.integers(mn, mx + 1, 1500)
    ts = np.concatenate([ts, fill]).astype(np.int64)
    k = np.concatenate([k, rng.integers(0, 5, len(fill))]).astype(np.int64)
    p = rng.permutation(len(ts))
    return picked, (ts[p], k[p], values("F64_VAR", rng, len(ts)))


def _groups(ref, start, key):
    return int(((ref["window_start"] == start) & (ref["key"] == key)).sum())


@pytest.mark.parametrize("len_ms,slide_ms,span",
                         [(1000, 300, 2600), (500, 1500, 9000)])
def test_window_edge_and_clamp_rows(len_ms, slide_ms, span):
    picked, batch = edge_batch(len_ms, slide_ms, span, 401)
    starts, cover = cover_of(batch[0], len_ms, slide_ms)
    assert int(batch[0].min()) == T0 + 137
    assert int(batch[0].max()) == T0 + 137 + span
    if slide_ms > len_ms:
        assert (cover.sum(axis=1) == 0).any(), "no row falls in a gap"
    _, ref = check("F64_VAR", len_ms, slide_ms, [batch])
    for i, s in enumerate(picked):
        first, last, past = 100 + 3 * i, 101 + 3 * i, 102 + 3 * i
        # the row at `start` is in its window and not in the next one, the
        # row at start + len - 1 is in it and not in the one before, the row
        # at start + len is out of it
        assert _groups(ref, s, first) == 1
        assert _groups(ref, s + slide_ms, first) == 0
        assert _groups(ref, s, last) == 1
        assert _groups(ref, s - slide_ms, last) == 0
        assert _groups(ref, s, past) == 0
        in_next = s + slide_ms <= s + len_ms < s + slide_ms + len_ms
        assert _groups(ref, s + slide_ms, past) == (1 if in_next else 0)
        if not in_next:
            assert (ref["key"] == past).sum() == 0     # the row is in a gap
    # neighbouring windows hold different row sets
    per_win = [int(ref["count"][window_rows(ref, s)].sum()) for s in picked]
    assert per_win == [int(cover[:, list(starts).index(s)].sum())
                       for s in picked]
    assert ref["count"].sum() == int(cover.sum())
    print("case 4:", (len_ms, slide_ms), "rows per picked window", per_win)


def test_batch_of_gap_rows_and_one_covered_row():
    rng = np.random.default_rng(402)
    gap = np.concatenate([rng.integers(T0 + 600, T0 + 1500, 250),
                          rng.integers(T0 + 2000, T0 + 2900, 250)])
    ts = np.concatenate([[T0 + 600, T0 + 2899, T0 + 1700], gap])
    ts = ts.astype(np.int64)
    p = rng.permutation(len(ts))
    batch = (ts[p], rng.integers(0, 5, len(ts)).astype(np.int64),
             values("F64_VAR", rng, len(ts)))
    m = cover_of(batch[0], 500, 1500)[1].sum(axis=1)
    assert m.sum() == 1 and (m == 0).sum() == len(ts) - 1
    _, ref = check("F64_VAR", 500, 1500, [batch])
    assert len(ref["count"]) == 1 < len(ts) and ref["count"][0] == 1
    assert ref["window_start"][0] == T0 + 1500


# --------------------------------------------------- 5. nulls at the seams

def seam_rows(st, n):
    """Rows st - 1, st, st + 1, the rows around every wave-quarter bound of
    the full supertiles, and the last row."""
    rows = {st - 1, st, st + 1, n - 1}
    for s0 in range(0, n - st + 1, st):
        for b in quarter_bounds(st)[1:-1]:
            rows |= {s0 + b - 1, s0 + b, s0 + b + 1}
    return sorted(r for r in rows if 0 <= r < n)


def null_case(pattern, fam="F64_VAR", seed=501):
    st = geometry(1000, 300)[1]
    n = 2 * st + 1
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 11, n).astype(np.int64)
    valid = np.ones(n, np.uint8)
    if pattern == "every_third":
        valid[::3] = 0
    elif pattern == "one_key":
        valid[k == 4] = 0
    elif pattern == "seams":
        valid[seam_rows(st, n)] = 0
    else:
        assert pattern == "none"
    return (spread(rng, n, T0 + 137, 700), k, values(fam, rng, n)), valid


@pytest.mark.parametrize("fam", ["F64_VAR", "F64_SIX"])
@pytest.mark.parametrize("pattern", ["every_third", "one_key", "seams"])
def test_nulls_at_the_seams(fam, pattern):
    st = geometry(1000, 300)[1]
    batch, valid = null_case(pattern, fam)
    n = len(valid)
    assert n == 2 * st + 1 and n % st == 1      # a last supertile of one row
    if pattern == "seams":
        rows = seam_rows(st, n)
        assert {st - 1, st, st + 1, 2 * st} <= set(rows)
        assert len(rows) == 4 + 2 * 3 * (WAVES - 1) and not valid[rows].any()
        assert valid.sum() == n - len(rows)
    _, ref = check(fam, 1000, 300, [batch], [valid])
    assert ref["count"].sum() == expected_records(1000, 300, [batch], [valid])
    assert ref["count"].sum() < expected_records(1000, 300, [batch])
    if pattern == "one_key":
        g = ref["key"] == 4
        assert g.sum() >= 3 and not ref["valid"][g].any()
        assert not ref["count"][g].any() and ref["valid"][~g].all()


def test_nulls_at_the_seams_two_columns():
    from denormalized_amd import WindowOp, _lib
    st = geometry(1000, 300)[1]
    (ts, k, v0), ok0 = null_case("seams")
    n = len(ts)
    rng = np.random.default_rng(502)
    v1 = rng.uniform(-1, 1, n) * 10.0 ** rng.integers(0, 9, n)
    ok1 = np.ones(n, np.uint8)
    ok1[1::3] = 0
    ok1[[st - 1, st]] = [1, 0]
    assert (ok0 != ok1).any() and not ok0[st] and ok1[st - 1]
    ref = streamref.run(1000, 300, [(ts, k, [v0, v1])], [[ok0, ok1]])
    per = {j: ref.fetch(j) for j in (0, 1)}
    exp = {f: per[0][f] for f in ("key", "window_start", "window_end",
                                  "valid")}
    for o, j, a in TWO:
        exp[a] = per[j][o]
        exp[a + "_valid"] = (np.ones_like(per[j]["valid"]) if o == "count"
                             else per[j]["valid"])
    m = cover_of(ts, 1000, 300)[1].sum(axis=1)
    assert exp["n0"].sum() == (m * ok0).sum() != (m * ok1).sum()
    assert exp["n1"].sum() == (m * ok1).sum()
    op = WindowOp(length_ms=1000, slide_ms=300,
                  aggs=[(o, 2 + j, a) for o, j, a in TWO],
                  key_kind=_lib.KEY_INT64, n_keys_hint=64)
    op.push(ts, k, [v0, v1], [_bitmap(ok0), _bitmap(ok1)])
    outs = op.poll_all()
    op.finish()
    outs += op.poll_all()
    msg = op._L.dz_last_error(op._h)
    op.close()
    assert not msg, msg
    fields = ["key", "valid", "window_start", "window_end"]
    for _o, j, a in TWO:
        fields += [a] + ([a + "_valid"] if j != 0 else [])
    mc.assert_match({f: _cat(outs, f) for f in fields}, exp, TWO)


# ------------------------------------------------ 6. the hop-ratio envelope

@pytest.mark.parametrize("len_ms,rows,span", [(2047, 300, 200),
                                              (1023, 64, 50), (682, 64, 50)])
def test_hop_ratio_envelope(len_ms, rows, span):
    expand, st = geometry(len_ms, 1)
    assert expand == len_ms + 1 <= ST and st == ST // expand
    if len_ms == 2047:
        assert expand == ST and st == 1     # one row fills the staging
    else:
        assert st == 2
    rng = np.random.default_rng(600 + len_ms)
    batch = (spread(rng, rows, T0 + 137, span),
             rng.integers(0, 5, rows).astype(np.int64),
             values("F64_VAR", rng, rows))
    starts, cover = cover_of(batch[0], len_ms, 1)
    # every start from min - len (that window ends at min: listed, empty) to
    # max is a frame, and every row lies in `len` of them
    assert SPLIT_WINDOWS < len(starts) == len_ms + span <= 4096
    assert cover.sum(axis=1).max() == len_ms == cover.sum(axis=1).min()
    stats = {}
    _, ref = check("F64_VAR", len_ms, 1, [batch], stats=stats,
                   max_open_windows=4096)
    assert stats["scatter"]["launches"] == -(-len(starts) // SPLIT_WINDOWS) > 1
    assert ref["count"].sum() == rows * len_ms
    assert len(np.unique(ref["window_start"])) == len(starts) - 1
    print("case 6:", (len_ms, 1), "expand", expand, "st_rows", st, "frames",
          len(starts), "scatter launches", stats["scatter"]["launches"])


def test_hop_ratio_past_the_envelope_is_refused():
    from denormalized_amd import WindowOp, _lib
    assert geometry(2048, 1)[0] == ST + 1
    op = WindowOp(length_ms=2048, slide_ms=1,
                  aggs=[(n, 0) for n in F64_VAR], key_kind=_lib.KEY_INT64,
                  n_keys_hint=64, max_open_windows=4096)
    with pytest.raises(RuntimeError, match="ratio exceeds"):
        op.push(np.array([T0 + 137, T0 + 150], np.int64),
                np.array([1, 2], np.int64), np.array([1.0, 2.0]))
    op.close()                               # still a live, closable handle
    assert op._h is None


# ------------------------------- 7. subrange boundaries under real sliding

@pytest.mark.parametrize("fam", ["F64_VAR", "I64_ALL"])
def test_subrange_boundaries_under_sliding(fam):
    expand, st = geometry(300, 7)
    rng = np.random.default_rng(701)
    b1 = (spread(rng, 2000, T0, 1700),
          rng.integers(0, 600, 2000).astype(np.int64), values(fam, rng, 2000))
    b2 = (spread(rng, 500, T0 + 2500, 400),
          rng.integers(0, 600, 500).astype(np.int64), values(fam, rng, 500))
    assert np.any(np.diff(b1[0]) < 0)
    starts, cover = cover_of(b1[0], 300, 7)
    assert 2 * SPLIT_WINDOWS >= len(starts) > SPLIT_WINDOWS
    assert len({s % 7 for s in starts.tolist()
                + cover_of(b2[0], 300, 7)[0].tolist()}) >= 2    # drift
    straddle = cover[:, SPLIT_WINDOWS - 1] & cover[:, SPLIT_WINDOWS]
    assert straddle.any(), "no row lies on both sides of the subrange cut"
    assert peak_open_frames(300, 7, [b1, b2]) <= 512
    assert int(b2[0].min()) >= int(starts.max()) + 300   # b2 closes b1's
    launches = {}

    def after(bi, op):
        launches[bi] = op.kernel_stats()["scatter"]["launches"]

    _, ref = check(fam, 300, 7, [b1, b2], max_open_windows=512,
                   on_push=after)
    assert launches[0] == 2, "the first batch did not split in two"
    assert launches[1] == 3
    assert ref["count"].sum() == expected_records(300, 7, [b1, b2])
    print("case 7: expand", expand, "st_rows", st, "windows", len(starts),
          "rows across the cut", int(straddle.sum()))


# ------------------------------------------ 8. two-level fold under sliding

@pytest.mark.parametrize("fam", ["F64_VAR", "I64_ALL"])
def test_two_level_fold_under_sliding(fam):
    rng = np.random.default_rng(801)
    nk = 70_000
    counts = [1, 3, 4, 5, 7, 8, 9, 16, 17]
    edge = np.repeat(np.arange(9), counts) * 512
    fill = rng.integers(0, nk, 8000 - len(edge) - 1)
    k = np.concatenate([[nk - 1], edge, fill]).astype(np.int64)
    rng.shuffle(k)
    n = len(k)
    ts = spread(rng, n, T0 + 137, 2000)
    valid = (rng.random(n) > 0.15).astype(np.uint8)
    assert np.any(np.diff(ts) < 0)
    for i, c in enumerate(counts):
        assert (k == i * 512).sum() >= c
    batch = (ts, k, values(fam, rng, n))
    stats = {}
    _, ref = check(fam, 1000, 300, [batch], [valid], dense=True,
                   n_keys_hint=nk, stats=stats)
    assert stats["regroup"]["launches"] > 0, "the two-level fold was not taken"
    assert stats["scatter"]["launches"] == 1
    assert ref["key"].max() == nk - 1 and (ref["valid"] == 0).any()
    assert ref["count"].sum() == expected_records(1000, 300, [batch], [valid])


# ----------------------------------------- 9. late rows into sliding frames

def test_late_rows_into_sliding_frames():
    fam = "F64_SIX"
    rng = np.random.default_rng(901)

    def in_order(b, n=600):
        ts = np.sort(spread(rng, n, T0 + 137 + b * 1100, 1400))
        return (ts, rng.integers(0, 6, n).astype(np.int64),
                values(fam, rng, n))

    batches = [in_order(b) for b in range(3)]
    wm = int(batches[2][0].min())
    late_ts = np.full(7, wm - 2000, np.int64)
    late_k = np.array([0, 1, 2, 0, 1, 2, 0], np.int64)
    batches.append((late_ts, late_k, values(fam, rng, 7, small=True)))
    batches.append(in_order(3))
    starts, cover = cover_of(late_ts, 1000, 300)
    starts = starts[cover.any(axis=0)]               # the frames re-created
    assert len(starts) >= 3
    assert starts.max() + 1000 <= wm                 # every one has closed
    _, ref = check(fam, 1000, 300, batches)
    tw = streamref.twice(ref)
    assert tw, "no group was emitted twice"
    assert set(tw) == {(int(s), int(key)) for s in starts for key in (0, 1, 2)}
    for (_s, key), (r1, r2) in tw.items():
        assert r2 > r1 and ref["count"][r1] > ref["count"][r2]
        assert ref["count"][r2] == (late_k == key).sum(), "late rows only"
    print("case 9: groups emitted twice:", len(tw))


# ------------------------------------------------------- 10. device pushes

def run_device(kind, names, len_ms, slide_ms, batches, **kw):
    """The batches through a device push; rows compared after finish(), as
    device pushes lag one batch."""
    from denormalized_amd import WindowOp, _lib
    kk = _lib.KEY_INT64 if kind == "i64" else _lib.KEY_DENSE_INT64
    op = WindowOp(length_ms=len_ms, slide_ms=slide_ms,
                  aggs=[(n, 0) for n in names], key_kind=kk, n_keys_hint=128,
                  **kw)
    held, outs = [], []
    for ts, k, v in batches:
        d = [_dev(ts), _dev(k if kind == "i64" else k.astype(np.int32)),
             _dev(v)]
        held += d                    # borrowed until the next call on the op
        if kind == "i64":
            op.push_device_i64(len(ts), d[0].ptr, d[1].ptr, d[2].ptr)
        else:
            op.push_device(len(ts), d[0].ptr, d[1].ptr, d[2].ptr,
                           borrowed=kind == "borrowed")
        outs += op.poll_all()
    op.finish()
    outs += op.poll_all()
    msg = op._L.dz_last_error(op._h)
    op.close()
    for d in held:
        d.free()
    assert not msg, msg
    return {f: _cat(outs, f) for f in _fields(names)}


@pytest.mark.parametrize("kind", ["copied", "borrowed"])
def test_device_pushes_of_the_drifting_stream(kind):
    batches = drift_batches("F64_SIX", seed=103)
    assert_drift_precondition(1000, 300, batches)
    ref = reference("F64_SIX", 1000, 300, batches)
    got = run_device(kind, F64_SIX, 1000, 300, batches)
    assert_exact(got, ref, "F64_SIX")


def test_device_push_i64_at_the_supertile_seams():
    st = geometry(1000, 300)[1]
    batch, _valid = null_case("none", "F64_SIX", seed=503)
    assert len(batch[0]) == 2 * st + 1
    ref = reference("F64_SIX", 1000, 300, [batch])
    got = run_device("i64", F64_SIX, 1000, 300, [batch])
    assert_exact(got, ref, "F64_SIX")
    assert ref["count"].sum() == expected_records(1000, 300, [batch])


# ------------------------- 11. runtime supertile length over several chunks

def subrange_multiplicity(ts, len_ms, slide_ms):
    """Per subrange launch of the batch, each row's window count there."""
    cover = cover_of(ts, len_ms, slide_ms)[1]
    return [cover[:, a:a + SPLIT_WINDOWS].sum(axis=1)
            for a in range(0, cover.shape[1], SPLIT_WINDOWS)]


def test_short_last_supertiles_of_two_chunks():
    n = 8193
    expand, st = geometry(500, 100)
    c, chunk = chunks_of(n)
    assert (c, chunk, expand, st) == (2, 4097, 6, 341)
    tail0, tail1 = chunk % st, (n - chunk) % st
    assert (tail0, tail1) == (5, 4)
    q = quarter_bounds(tail0)
    assert [b - a for a, b in zip(q[:-1], q[1:])] == [2, 2, 1, 0]
    rng = np.random.default_rng(1101)
    ts = spread(rng, n, T0 + 137, 30000)
    starts = cover_of(ts, 500, 100)[0]
    assert 2 * SPLIT_WINDOWS >= len(starts) > SPLIT_WINDOWS
    cut = int(starts[SPLIT_WINDOWS])      # the second subrange's first start
    ts[chunk - 5:chunk - 2] = [cut - 50, cut + 50, cut + 450]
    ids = np.array([0, 512, 1024, 1536, 1, 513, 1025], np.int64)
    assert len(set((ids & 511).tolist())) == 2           # 7 keys, two buckets
    k = rng.choice(ids, n)
    m = subrange_multiplicity(ts, 500, 100)
    assert len(m) == 2
    assert {0, 1, 5} <= set(m[1][chunk - tail0:chunk].tolist())
    batch = (ts, k, values("F64_VAR", rng, n))
    stats = {}
    _, ref = check("F64_VAR", 500, 100, [batch], dense=True, n_keys_hint=2048,
                   stats=stats, max_open_windows=512)
    assert stats["scatter"]["launches"] == 2 == stats["hist"]["launches"]
    assert ref["count"].sum() == expected_records(500, 100, [batch])


def test_tumbling_subranges_fill_all_slots():
    n = 8193
    c, chunk = chunks_of(n)
    assert (c, chunk) == (2, 4097)
    st = ST                  # tumbling: expand 1, a supertile of ST rows, and
    assert -(-st // WAVES) == 8 * 64      # 8 wave steps per quarter
    rng = np.random.default_rng(1102)
    ts = spread(rng, n, T0, 300_000)
    starts, cover = cover_of(ts, 1000, 0)
    assert len(starts) == 300
    assert (cover.sum(axis=1) == 1).all()
    first = cover[:, :SPLIT_WINDOWS].any(axis=1)        # m = 1 in subrange 1
    assert 0 < first[:64].sum() < 64, "one wave step, one subrange"
    seams = [s for lo in (0, chunk) for s in range(lo + st, n, st)
             if s < min(n, lo + chunk)]
    assert seams == [2048, 4096, 6145] and seams[2] % 8 != 0
    valid = (rng.random(n) > 0.3).astype(np.uint8)
    for s in seams + [chunk]:
        valid[s - 1:s + 2] = [1, 0, 1]
    batch = (ts, rng.integers(0, 5, n).astype(np.int64),
             values("F64_VAR", rng, n))
    stats = {}
    _, ref = check("F64_VAR", 1000, 0, [batch], [valid], stats=stats,
                   max_open_windows=512)
    # one scatter per subrange; hist counts the ingest's full-range pass too
    assert stats["scatter"]["launches"] == 2 == stats["hist"]["launches"] - 1
    assert ref["count"].sum() == int(valid.sum())


def test_chunk_of_whole_supertiles():
    expand, st = geometry(1000, 500)
    assert (expand, st) == (3, 682)
    n = 2 * 12 * st
    c, chunk = chunks_of(n)
    assert c == 2 and chunk % st == 0 and n < 2 * 8192
    rng = np.random.default_rng(1103)
    k = rng.integers(0, 9, n).astype(np.int64)
    k[chunk - 1], k[chunk] = 100, 101      # the rows either side of the seam
    batch = (spread(rng, n, T0 + 137, 1400), k, values("F64_VAR", rng, n))
    stats = {}
    _, ref = check("F64_VAR", 1000, 500, [batch], stats=stats)
    assert stats["scatter"]["launches"] == 1 == stats["hist"]["launches"]
    m = cover_of(batch[0], 1000, 500)[1].sum(axis=1)
    for key, row in ((100, chunk - 1), (101, chunk)):
        assert ref["count"][ref["key"] == key].sum() == m[row]
    assert ref["count"].sum() == int(m.sum())


def test_one_row_supertiles():
    expand, st = geometry(2047, 1)
    assert (expand, st) == (ST, 1)
    assert quarter_bounds(st) == [0, 1, 1, 1, 1]         # three empty waves
    rows = 70
    assert chunks_of(rows) == (1, rows)
    rng = np.random.default_rng(1104)
    batch = (spread(rng, rows, T0 + 137, 50),
             rng.integers(0, 5, rows).astype(np.int64),
             values("F64_VAR", rng, rows))
    starts = cover_of(batch[0], 2047, 1)[0]
    stats = {}
    _, ref = check("F64_VAR", 2047, 1, [batch], stats=stats,
                   max_open_windows=4096)
    assert stats["scatter"]["launches"] == -(-len(starts) // SPLIT_WINDOWS) > 1
    assert ref["count"].sum() == rows * 2047
