"""Device utf8 intern, slot layout edge cases: keys verified from the bytes
kept in the table slot (up to 16 B), from the pool offset (17..62 B) and
through the id_off/id_len arrays (longer); near-miss keys; row counts around
the wave and grid sizes; unaligned key columns; forced fingerprint
collisions; batches without and with fresh keys.

Every case pushes raw key bytes through push_device_utf8 and compares with
the CPU oracle on the same rows at tolerance 0, including the key strings
and their first-seen emission order."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import pyoracle

pytestmark = pytest.mark.gpu

ROWS_PER_MS = 4  # 4096-row batches span ~1 s: several 1 s windows per stream


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def _cat(outs, field):
    arrs = [b[field] for b in outs]
    if arrs and isinstance(arrs[0], list):
        return [x for a in arrs for x in a]
    return np.concatenate(arrs) if arrs else np.zeros(0)


class Stream:
    """Batches of key indices into `names` (bytes), with timestamps, values
    and the oracle's expected output, computed once and shared."""

    def __init__(self, names, kid_batches, seed, rows_per_ms=ROWS_PER_MS):
        self.names = names
        rng = np.random.default_rng(seed)
        self.batches = []
        o = pyoracle.Oracle(1000, 0)
        row = 0
        for kid in kid_batches:
            kid = np.asarray(kid, np.int64)
            n = len(kid)
            ts = (1_000_000 + np.arange(row, row + n) // rows_per_ms).astype(
                np.int64)
            row += n
            v = rng.uniform(0, 115, n)
            lens = np.array([len(x) for x in names], np.int64)[kid]
            offs = np.zeros(n + 1, np.int32)
            np.cumsum(lens, out=offs[1:])
            data = np.frombuffer(b"".join(names[k] for k in kid), np.uint8)
            self.batches.append((ts, kid, v, offs, data))
            o.push(ts, kid, v)
        o.finish()
        self.exp = o.fetch()
        o.close()
        assert len(self.exp["key"]) > 0


def run_engine(stream, shift=0, fp_bits=None, n_keys_hint=64, finish=True):
    """Push the stream through the device intern; the key column's base
    pointer sits `shift` bytes into an allocation that ends with the last
    key's last byte."""
    from denormalized_amd import DeviceArray, WindowOp, _lib
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_UTF8,
                  n_keys_hint=n_keys_hint)
    if fp_bits is not None:
        op.debug_intern_fp_bits(fp_bits)
    outs, keep = [], []
    try:
        for ts, _kid, v, offs, data in stream.batches:
            n = len(ts)
            d_ts = DeviceArray(0, n * 8); d_ts.from_host(ts)
            d_of = DeviceArray(0, offs.nbytes); d_of.from_host(offs)
            d_da = DeviceArray(0, max(1, data.nbytes + shift))
            if data.nbytes:
                d_da.from_host(np.concatenate(
                    [np.full(shift, 0xEE, np.uint8), data]))
            d_v = DeviceArray(0, n * 8); d_v.from_host(v)
            keep.append((d_ts, d_of, d_da, d_v))  # borrowed until next call
            op.push_device_utf8(n, d_ts.ptr, d_of.ptr,
                                ctypes.c_void_p(d_da.ptr.value + shift),
                                d_v.ptr)
            outs += op.poll_all()
        if finish:
            op.finish()
            outs += op.poll_all()
    finally:
        op.close()
        for bufs in keep:
            for a in bufs:
                a.free()
    return outs


def assert_exact(outs, stream):
    exp = stream.exp
    got_key = _cat(outs, "key")
    assert list(got_key) == [stream.names[k].decode() for k in exp["key"]], \
        "key strings / first-seen order"
    assert np.array_equal(_cat(outs, "count"), exp["count"]), "count"
    assert np.array_equal(_cat(outs, "valid"), exp["valid"]), "validity"
    v = exp["valid"].astype(bool)
    for f in ("min", "max", "avg"):
        assert np.array_equal(_cat(outs, f)[v], exp[f][v]), f"{f} not bit-exact"
    assert np.array_equal(_cat(outs, "window_start"), exp["window_start"])
    assert np.array_equal(_cat(outs, "window_end"), exp["window_end"])


def _growing_batches(n_names, introduce, n_batches, rows, seed):
    """Random key picks per batch; key k first becomes available in batch
    introduce[k], and every batch's newly available keys do appear in it."""
    rng = np.random.default_rng(seed)
    out = []
    for b in range(n_batches):
        avail = np.array([k for k in range(n_names) if introduce[k] <= b])
        new = np.array([k for k in range(n_names) if introduce[k] == b])
        kid = avail[rng.integers(0, len(avail), rows)]
        if len(new):
            kid[rng.choice(rows, len(new), replace=False)] = new
        out.append(kid)
    return out


# ------------------------------------------------------ 1. length boundaries

LENGTHS = (1, 7, 8, 9, 15, 16, 17, 18, 62, 63, 64, 300)


@pytest.fixture(scope="module")
def length_stream():
    names, introduce = [b""], [0]
    for ln in LENGTHS:
        for variant in range(3):  # variant b is new in batch b
            tag = f"{ln}v{variant}-".encode()
            body = (tag + b"abcdefghijklmnopqrstuvwxyz0123456789" * 9)[:ln]
            if ln < len(tag):  # too short for the tag: vary the last byte
                body = body[:-1] + bytes([ord("A") + variant])
            names.append(body)
            introduce.append(variant)
    assert len(set(names)) == len(names)
    assert sorted({len(x) for x in names}) == [0] + list(LENGTHS)
    return Stream(names, _growing_batches(len(names), introduce, 3, 4096, 11),
                  seed=12)


def test_length_boundaries(length_stream):
    assert_exact(run_engine(length_stream), length_stream)


# ------------------------------------------------------------ 2. near-misses

_BASE16 = b"abcdefghijklmnop"
NEAR_PAIRS = [
    (_BASE16 + b"q", _BASE16 + b"r"),              # differ at byte 17
    (_BASE16 + b"q123", _BASE16 + b"r123"),        # same, longer tail
    (b"prefix7", b"prefix7h"),                     # proper prefix 7/8
    (b"prefix_8", b"prefix_8i"),                   # proper prefix 8/9
    (b"prefix_of_15_by", b"prefix_of_15_byt"),     # proper prefix 15/16
    (_BASE16[:15] + b"X", _BASE16[:15] + b"Y"),    # last byte at length 16
    (b"abc", b"abc\x00"),                          # zero padding vs a real NUL
    (b"abcdefgh", b"abcdefgh\x00"),
    (b"", b"\x00"),
]


def test_near_miss_keys():
    assert [len(a) for a, _ in NEAR_PAIRS[2:6]] == [7, 8, 15, 16]
    names, introduce = [], []
    for i, (a, b) in enumerate(NEAR_PAIRS):
        names += [a, b]
        # even pairs: the second key arrives one batch after the first;
        # odd pairs: both new in one batch
        introduce += [0, 1] if i % 2 == 0 else [1, 1]
    names.append(b"late")
    introduce.append(2)
    assert len(set(names)) == len(names)
    s = Stream(names, _growing_batches(len(names), introduce, 3, 4096, 21),
               seed=22)
    assert_exact(run_engine(s), s)


def test_near_miss_keys_share_one_fingerprint():
    # 1-bit fingerprints: every key hashes to 1, so each key is compared
    # against every earlier near-miss in its probe chain — only the length
    # and the bytes tell them apart. One new key per batch (two new keys
    # with one fingerprint in a batch are the documented failure).
    names = [k for pair in NEAR_PAIRS for k in pair]
    n = len(names)
    s = Stream(names, _growing_batches(n, list(range(n)), n, 256, 23),
               seed=24)
    assert_exact(run_engine(s, fp_bits=1), s)


# -------------------------------------------------------------- 3. row counts

def test_row_counts_warm_table():
    names = [f"sensor_{i}".encode() for i in range(50)]
    rng = np.random.default_rng(31)
    kid_batches = [np.concatenate([np.arange(50), rng.integers(0, 50, 462)])]
    for n in (1, 63, 64, 65, 257):
        kid_batches.append(rng.integers(0, 50, n))
    # more rows than the 2048 x 256 launch grid: the grid-stride loop
    kid_batches.append(rng.integers(0, 50, 600_000))
    s = Stream(names, kid_batches, seed=32, rows_per_ms=40)
    assert_exact(run_engine(s), s)


# --------------------------------------------------- 4. unaligned column base

@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_unaligned_key_column(length_stream, shift):
    assert_exact(run_engine(length_stream, shift=shift), length_stream)


# ------------------------------------------------ 5. fingerprint collisions

def _fnv1a64(b):
    h = 1469598103934665603
    for c in b:
        h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _colliding_names(count, bits=3):
    """Keys whose fingerprints agree in the low `bits` bits (the engine
    hashes with 64-bit FNV-1a; should it ever hash differently these keys
    still collide often at 3 bits, and results must be exact either way).
    Short (slot-verified) and long (pool-verified) keys alternate."""
    names, i = [], 0
    while len(names) < count:
        stem = "c%d" if len(names) % 2 == 0 else "collide_with_a_long_key_%d"
        cand = (stem % i).encode()
        i += 1
        if _fnv1a64(cand) & ((1 << bits) - 1) == 5:
            names.append(cand)
    return names


def test_collisions_probe_on():
    # 3-bit fingerprints, one new key per batch for 12 batches after the
    # first: each new key meets assigned slots holding its own fingerprint
    # and must probe on to a slot of its own
    names = _colliding_names(13)
    introduce = list(range(13))
    s = Stream(names, _growing_batches(13, introduce, 13, 512, 41), seed=42)
    assert_exact(run_engine(s, fp_bits=3), s)


def test_two_new_colliding_keys_in_one_batch_fail_loudly():
    # documented limit: two NEW keys with one fingerprint inside one batch
    # cannot be told apart by the claim and are flagged (guard code 6)
    names = _colliding_names(2)
    s = Stream(names, [np.arange(512) % 2], seed=43)
    with pytest.raises(RuntimeError, match=r"guard tripped \(cell 3 = 6\)"):
        run_engine(s, fp_bits=3)


def test_fp_bits_only_before_first_push():
    names = [b"a", b"b"]
    s = Stream(names, [np.arange(64) % 2], seed=44)
    from denormalized_amd import DeviceArray, WindowOp, _lib
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_UTF8, n_keys_hint=8)
    ts, _kid, v, offs, data = s.batches[0]
    bufs = []
    for a in (ts, offs, data, v):
        d = DeviceArray(0, a.nbytes); d.from_host(a); bufs.append(d)
    op.push_device_utf8(len(ts), bufs[0].ptr, bufs[1].ptr, bufs[2].ptr,
                        bufs[3].ptr)
    with pytest.raises(RuntimeError, match="only before the first"):
        op.debug_intern_fp_bits(3)
    op.close()
    for d in bufs:
        d.free()


# ----------------------------------------------------------- 6. flip-pass skip

def test_batch_without_fresh_keys_then_one_in_last_row():
    names = [f"sensor_{i}".encode() for i in range(40)] + [b"sensor_new"]
    rng = np.random.default_rng(51)
    b1 = np.concatenate([np.arange(40), rng.integers(0, 40, 4056)])
    b2 = rng.integers(0, 40, 4096)           # nothing fresh: passes skipped
    b3 = rng.integers(0, 40, 4096)
    b3[-1] = 40                              # one new key, in the last row
    s = Stream(names, [b1, b2, b3], seed=52)
    assert_exact(run_engine(s), s)
