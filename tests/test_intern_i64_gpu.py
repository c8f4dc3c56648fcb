"""Device int64 intern (push_device_i64): every int64 value as a key, row
counts around the wave, block and grid sizes, fresh-key handling, long and
wrapping probe chains, a sliding filtered op, the device emission route,
the capacity contract, the refusals, and a cross-check against the host
dictionary.

Every case pushes raw int64 keys through push_device_i64 and compares with
the CPU oracle on the same rows at tolerance 0, including the emitted key
values and their first-seen order."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import i64vec as iv
from tests.i64vec import Stream, growing_batches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _cat(outs, field):
    arrs = [b[field] for b in outs]
    return np.concatenate(arrs) if arrs else np.zeros(0)


def _device_batch(ts, keys, v):
    from denormalized_amd import DeviceArray
    bufs = []
    for a in (ts, keys, v):
        d = DeviceArray(0, max(8, a.nbytes))
        if a.nbytes:
            d.from_host(np.ascontiguousarray(a))
        bufs.append(d)
    return bufs


def run_engine(stream, fp_bits=None, n_keys_hint=64, slide_ms=0, filt=None,
               via="device", stats=None):
    """Push the stream through one DZ_KEY_INT64 op, polling after every
    push; `via` picks push_device_i64 or the host-dictionary push. A dict
    passed as `stats` receives the op's kernel_stats()."""
    from denormalized_amd import WindowOp, _lib
    op = WindowOp(length_ms=1000, slide_ms=slide_ms, key_kind=_lib.KEY_INT64,
                  n_keys_hint=n_keys_hint)
    if fp_bits is not None:
        op.debug_intern_fp_bits(fp_bits)
    if filt is not None:
        op.set_filter(*filt)
    outs, keep = [], []
    try:
        for ts, _kid, keys, v in stream.batches:
            if via == "host":
                op.push(ts, keys, v)
            else:
                bufs = _device_batch(ts, keys, v)
                keep.append(bufs)  # borrowed until the next call on the op
                op.push_device_i64(len(ts), bufs[0].ptr, bufs[1].ptr,
                                   bufs[2].ptr)
            outs += op.poll_all()
        op.finish()
        outs += op.poll_all()
        if stats is not None:
            stats.update(op.kernel_stats())
    finally:
        op.close()
        for bufs in keep:
            for a in bufs:
                a.free()
    return outs


def assert_exact(outs, stream, keep=None):
    exp = stream.exp
    sel = slice(None) if keep is None else keep
    got_key = _cat(outs, "key")
    assert got_key.dtype == np.int64
    assert np.array_equal(got_key, stream.values[exp["key"][sel]]), \
        "key values / first-seen order"
    assert np.array_equal(_cat(outs, "count"), exp["count"][sel]), "count"
    assert np.array_equal(_cat(outs, "valid"), exp["valid"][sel]), "validity"
    v = exp["valid"][sel].astype(bool)
    for f in ("min", "max", "avg"):
        assert np.array_equal(_cat(outs, f)[v], exp[f][sel][v]), \
            f"{f} not bit-exact"
    assert np.array_equal(_cat(outs, "window_start"), exp["window_start"][sel])
    assert np.array_equal(_cat(outs, "window_end"), exp["window_end"][sel])


# ---------------------------------------------------------- 1. special values

# iv.SPECIALS ends with the value DESIGN.md names as the empty mark's twin
# (key 0, kept in a cell of its own); listed twice on purpose, deduplicated
# here
SPECIALS = list(dict.fromkeys(iv.SPECIALS))


def test_specials_together_in_first_batch():
    assert iv.EMPTY_MARK_KEY in SPECIALS
    values = np.concatenate([np.array(SPECIALS, np.int64),
                             iv.sparse_values(20, 101)])
    n = len(values)
    s = Stream(values, growing_batches(n, [0] * n, 2, 4096, 102), seed=103)
    assert_exact(run_engine(s), s)


@pytest.mark.parametrize("key", SPECIALS)
def test_special_as_only_key(key):
    s = Stream([key], [np.zeros(4096, np.int64), np.zeros(300, np.int64)],
               seed=111)
    assert_exact(run_engine(s), s)


@pytest.mark.parametrize("key", SPECIALS)
def test_special_first_seen_in_third_batch(key):
    values = np.concatenate([[key], iv.sparse_values(30, 121)])
    introduce = [2] + [b % 2 for b in range(30)]
    s = Stream(values, growing_batches(31, introduce, 4, 2048, 122), seed=123)
    assert_exact(run_engine(s), s)


# -------------------------------------------------------------- 2. row counts

def test_row_counts():
    nk = 1000
    values = iv.sparse_values(nk + 1, 201)
    rng = np.random.default_rng(202)
    kid_batches = [np.concatenate([np.arange(nk), rng.integers(0, nk, 1048)])]
    for n in (1, 63, 64, 65, 255, 256, 257, 524_288, 524_289):
        kid_batches.append(rng.integers(0, nk, n))
    # 2048 blocks x 256 threads cover 524,288 rows: row 524,288 is the first
    # one a grid-stride second iteration serves; it carries a new key
    kid_batches[-1][524_288] = nk
    s = Stream(values, kid_batches, seed=203, rows_per_ms=40)
    assert_exact(run_engine(s, n_keys_hint=nk + 1), s)


# ------------------------------------------------------- 3. fresh-key handling

def test_one_new_key_in_every_row_of_a_batch():
    # 4,096 rows race to claim one slot: one id
    values = iv.sparse_values(9, 301)
    rng = np.random.default_rng(302)
    s = Stream(values, [np.zeros(4096, np.int64), rng.integers(0, 9, 4096),
                        np.full(4096, 8)], seed=303)
    assert_exact(run_engine(s), s)


def test_every_row_a_new_distinct_key():
    values = iv.sparse_values(2 * 4096, 311)
    s = Stream(values, [np.arange(4096), np.arange(4096, 2 * 4096),
                        np.arange(2 * 4096)[::-1]], seed=312)
    assert_exact(run_engine(s), s)


def test_batches_without_new_keys_before_and_after_one_with():
    values = iv.sparse_values(41, 321)
    rng = np.random.default_rng(322)
    b1 = np.concatenate([np.arange(40), rng.integers(0, 40, 4056)])
    b2 = rng.integers(0, 40, 4096)           # nothing fresh: passes skipped
    b3 = rng.integers(0, 40, 4096)
    b4 = rng.integers(0, 40, 4096)
    b4[-1] = 40                              # one new key, in the last row
    b5 = rng.integers(0, 41, 4096)           # nothing fresh again
    s = Stream(values, [b1, b2, b3, b4, b5], seed=323)
    assert_exact(run_engine(s), s)


def test_keys_introduced_over_six_batches_with_polls_between():
    # the host mirror grows while earlier windows are being emitted
    nk = 600
    values = iv.sparse_values(nk, 331)
    introduce = np.arange(nk) % 6
    s = Stream(values, growing_batches(nk, introduce, 6, 4096, 332), seed=333)
    assert_exact(run_engine(s), s)


# ------------------------------------------------------------ 4. probe chains

@pytest.mark.parametrize("bits", [1, 4])
def test_long_probe_chains(bits):
    # 2^bits home slots for 300 keys: chains of hundreds, in-batch claims
    # walking past each other and, in the later batches, past assigned slots
    values = iv.sparse_values(300, 401)
    assert len(set(iv.home_slots(values, iv.P_MIN, bits).tolist())) <= 1 << bits
    introduce = [0] * 200 + [1] * 60 + [2] * 40
    s = Stream(values, growing_batches(300, introduce, 3, 4096, 402),
               seed=403)
    assert_exact(run_engine(s, fp_bits=bits), s)


def test_probe_chain_wraps_to_slot_zero():
    P = iv.P_MIN
    found = iv.keys_with_home((P - 2, P - 1, 0), 3, seed=77)
    values = np.array(found[P - 2] + found[P - 1] + found[0], np.int64)
    assert iv.home_slots(values, P).tolist() == [P - 2] * 3 + [P - 1] * 3 + \
        [0] * 3
    # one key of each home slot per batch: the later ones walk over assigned
    # slots P-2, P-1, 0, 1, ... before they claim
    introduce = [0, 1, 2] * 3
    s = Stream(values, growing_batches(9, introduce, 3, 1024, 411), seed=412)
    assert_exact(run_engine(s, n_keys_hint=64), s)  # kcap 512: P = 65,536


# ------------------------------------------------------- 5. sliding and filter

def test_sliding_filtered_op():
    nk = 1000
    values = iv.sparse_values(nk, 501)
    introduce = np.arange(nk) % 3
    s = Stream(values, growing_batches(nk, introduce, 3, 4096, 502), seed=503,
               slide_ms=250)
    keep = s.exp["valid"].astype(bool) & (s.exp["max"] > 100.0)
    assert 0 < keep.sum() < len(keep)
    outs = run_engine(s, n_keys_hint=nk, slide_ms=250,
                      filt=("max", ">", 100.0))
    assert_exact(outs, s, keep)


# ------------------------------------------------------------ 6. large-key route

def test_device_emission_route_above_65536_keys():
    # 50 keys of real data, then 66,000 distinct one-row keys: n_keys passes
    # 65,536 and every later close is emitted by the device chain; a last new
    # key arrives after that
    flood = 66_000
    values = iv.sparse_values(50 + flood + 1, 601)
    rng = np.random.default_rng(602)
    b0 = np.concatenate([np.arange(50), rng.integers(0, 50, 4046)])
    b1 = 50 + np.arange(flood)
    b2 = rng.integers(0, 50, 4096)
    b2[1000] = 50 + flood
    b3 = rng.integers(0, 50 + flood + 1, 4096)
    s = Stream(values, [b0, b1, b2, b3], seed=603, rows_per_ms=40)
    stats = {}
    assert_exact(run_engine(s, n_keys_hint=70_000, stats=stats), s)
    assert stats["intern_i64"]["launches"] == 4
    assert stats["intern_i64"]["bytes_per_launch_alg"] == 12 * len(b3)
    assert (stats["h_emit_group"]["launches"]
            + stats["h_emit_perclose"]["launches"]) >= 1, "no device chain ran"


# ----------------------------------------------------------------- 7. capacity

def test_capacity_overflow_fails_loudly():
    # n_keys_hint 1 -> key capacity 512 -> 4 x 512 < 65,536 slots, the
    # minimum table; ids: half the table = 32,768. One key more is refused
    # through the guard cell; nothing is written out of range.
    from denormalized_amd import WindowOp, _lib
    n = 32_768 + 1
    ts = (1_000_000 + np.arange(n) // 64).astype(np.int64)
    keys = iv.sparse_values(n, 701)
    v = np.ones(n)
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64, n_keys_hint=1)
    bufs = _device_batch(ts, keys, v)
    try:
        op.push_device_i64(n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
        with pytest.raises(RuntimeError, match=r"guard tripped \(cell 3 = "):
            op.finish()
    finally:
        op.close()
        for a in bufs:
            a.free()


# ---------------------------------------------------------------- 8. refusals

@pytest.fixture(scope="module")
def two_batches():
    values = iv.sparse_values(30, 801)
    return Stream(values, growing_batches(30, [b % 2 for b in range(30)], 2,
                                          2048, 802), seed=803)


def _run_with_refusal(s, refused, match, via):
    """Push batch 0, make the refused call (it must raise and change
    nothing), push batch 1, finish: the result must be the stream's."""
    from denormalized_amd import WindowOp, _lib
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_INT64, n_keys_hint=64)
    outs, keep = [], []

    def good(batch):
        ts, _kid, keys, v = batch
        if via == "host":
            op.push(ts, keys, v)
        else:
            bufs = _device_batch(ts, keys, v)
            keep.append(bufs)
            op.push_device_i64(len(ts), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)

    try:
        good(s.batches[0])
        with pytest.raises(RuntimeError, match=match):
            refused(op, s.batches[1], keep)
        good(s.batches[1])
        op.finish()
        outs = op.poll_all()
    finally:
        op.close()
        for bufs in keep:
            for a in bufs:
                a.free()
    assert_exact(outs, s)


def test_refuses_device_push_after_host_push(two_batches):
    def refused(op, batch, keep):
        ts, _kid, keys, v = batch
        bufs = _device_batch(ts, keys, v)
        keep.append(bufs)
        op.push_device_i64(len(ts), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
    _run_with_refusal(two_batches, refused, "cannot mix host int64", "host")


def test_refuses_host_push_after_device_push(two_batches):
    def refused(op, batch, keep):
        ts, _kid, keys, v = batch
        op.push(ts, keys, v)
    _run_with_refusal(two_batches, refused, "cannot mix host int64", "device")


def test_refuses_misaligned_key_column(two_batches):
    def refused(op, batch, keep):
        ts, _kid, keys, v = batch
        bufs = _device_batch(ts, np.concatenate([keys, keys[:1]]), v)
        keep.append(bufs)
        op.push_device_i64(len(ts), bufs[0].ptr,
                           ctypes.c_void_p(bufs[1].ptr.value + 4),
                           bufs[2].ptr)
    _run_with_refusal(two_batches, refused, "8-byte aligned", "device")


def test_refuses_other_key_kinds(two_batches):
    from denormalized_amd import DeviceArray, WindowOp, _lib
    ts, kid, keys, v = two_batches.batches[0]
    bufs = _device_batch(ts, keys, v)
    d_kid = DeviceArray(0, len(kid) * 4)
    d_kid.from_host(kid.astype(np.int32))
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_DENSE_INT64,
                  n_keys_hint=64)
    try:
        with pytest.raises(RuntimeError, match="requires key_kind"):
            op.push_device_i64(len(ts), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr)
        # still usable: the same rows by dense id
        op.push_device(len(ts), bufs[0].ptr, d_kid.ptr, bufs[2].ptr)
        op.finish()
        outs = op.poll_all()
    finally:
        op.close()
        d_kid.free()
        for a in bufs:
            a.free()
    assert _cat(outs, "count").sum() == len(ts)
    assert set(_cat(outs, "key").tolist()) == set(kid.tolist())


# ------------------------------------------------------------- 9. cross-check

def test_host_dictionary_and_device_intern_agree():
    nk = 200
    values = np.concatenate([np.array(SPECIALS, np.int64),
                             iv.sparse_values(nk - len(SPECIALS), 901)])
    introduce = np.arange(nk) % 4
    s = Stream(values, growing_batches(nk, introduce, 4, 4096, 902), seed=903)
    host = run_engine(s, via="host")
    dev = run_engine(s)
    # the device push is pipelined (emission may lag one push), so compare
    # the streams of batches, not what each poll returned
    assert len(host) == len(dev) > 0
    for hb, db in zip(host, dev):
        assert hb.keys() == db.keys()
        for name in hb:
            assert np.array_equal(hb[name], db[name]), name
    assert_exact(dev, s)
