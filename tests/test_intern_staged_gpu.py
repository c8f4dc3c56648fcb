"""Device utf8 intern, tile-cooperative key staging: the claim kernel walks
tiles of 256 consecutive rows, copies a tile's key bytes into LDS with aligned
16 B loads when the tile's span fits the stage (4096 B), and hashes from
there; a tile with a longer span hashes from global memory. Cases sit on the
tile edges, on the stage boundary, on empty keys, on every alignment of the
column base and on bytes >= 0x80.

Every case pushes raw key bytes through push_device_utf8 and compares every
output column with the CPU oracle on the same rows at tolerance 0, including
the key bytes and their first-seen emission order. Keys are compared as bytes
(read from the raw Arrow views), so they need not be valid UTF-8."""
import ctypes

import numpy as np
import pytest

import __graft_entry__ as graft
from oracle import pyoracle

pytestmark = pytest.mark.gpu

TILE = 256
GRID = 2048  # blocks the claim launches at most


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


class Stream:
    """Batches of key indices into `names` (bytes), with timestamps, values
    and the oracle's expected output, computed once."""

    def __init__(self, names, kid_batches, seed, rows_per_ms=4):
        assert len(set(names)) == len(names)
        self.names = names
        rng = np.random.default_rng(seed)
        lens_all = np.array([len(x) for x in names], np.int64)
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
            lens = lens_all[kid]
            data = np.frombuffer(b"".join(names[k] for k in kid), np.uint8)
            self.batches.append((ts, kid, v, lens, data))
            o.push(ts, kid, v)
        o.finish()
        self.exp = o.fetch()
        o.close()
        assert len(self.exp["key"]) > 0


def _collect(op):
    """Every pollable batch, keys as raw bytes."""
    op.drain()
    out = []
    while True:
        b = op.poll(copy=False)
        if b is None:
            return out
        o = b["key_offsets"]
        raw = b["key_data"].tobytes()
        d = {f: np.array(b[f]) for f in ("count", "min", "max", "avg", "valid",
                                         "window_start", "window_end")}
        d["key"] = [raw[o[i]:o[i + 1]] for i in range(b["n_rows"])]
        out.append(d)


def run_engine(stream, shift=0, lead=0, n_keys_hint=64):
    """Push the stream through the device intern. The key column's base
    pointer sits `shift` bytes into an allocation that ends with the last
    key's last byte; the column is a slice whose first offset is `lead`,
    with `lead` junk bytes in front of the first key."""
    from denormalized_amd import DeviceArray, WindowOp, _lib
    op = WindowOp(length_ms=1000, key_kind=_lib.KEY_UTF8,
                  n_keys_hint=n_keys_hint)
    outs, keep = [], []
    try:
        for ts, _kid, v, lens, data in stream.batches:
            n = len(ts)
            offs = np.empty(n + 1, np.int32)
            offs[0] = lead
            offs[1:] = lead + np.cumsum(lens)
            host = np.concatenate([np.full(shift, 0xEE, np.uint8),
                                   np.full(lead, 0xDD, np.uint8), data])
            d_ts = DeviceArray(0, n * 8); d_ts.from_host(ts)
            d_of = DeviceArray(0, offs.nbytes); d_of.from_host(offs)
            d_da = DeviceArray(0, max(1, host.nbytes))
            if host.nbytes:
                d_da.from_host(host)
            d_v = DeviceArray(0, n * 8); d_v.from_host(v)
            keep.append((d_ts, d_of, d_da, d_v))  # borrowed until next call
            op.push_device_utf8(n, d_ts.ptr, d_of.ptr,
                                ctypes.c_void_p(d_da.ptr.value + shift),
                                d_v.ptr)
            outs += _collect(op)
        op.finish()
        outs += _collect(op)
    finally:
        op.close()
        for bufs in keep:
            for a in bufs:
                a.free()
    return outs


def _cat(outs, field):
    arrs = [b[field] for b in outs]
    if field == "key":
        return [x for a in arrs for x in a]
    return np.concatenate(arrs) if arrs else np.zeros(0)


def assert_exact(outs, stream):
    exp = stream.exp
    assert _cat(outs, "key") == [stream.names[k] for k in exp["key"]], \
        "key bytes / first-seen order"
    assert np.array_equal(_cat(outs, "count"), exp["count"]), "count"
    assert np.array_equal(_cat(outs, "valid"), exp["valid"]), "validity"
    v = exp["valid"].astype(bool)
    for f in ("min", "max", "avg"):
        assert np.array_equal(_cat(outs, f)[v], exp[f][v]), f"{f} not bit-exact"
    assert np.array_equal(_cat(outs, "window_start"), exp["window_start"])
    assert np.array_equal(_cat(outs, "window_end"), exp["window_end"])


def _sensor(n):
    return [f"sensor_{i}".encode() for i in range(n)]


def _long(i):
    return (f"long{i:04d}-".encode() + b"0123456789abcdefghijklmnopqrstuv" * 10)[:300]


# ----------------------------------------------------------------- tile edges

EDGE_ROWS = (1, 255, 256, 257, 511, 512, 513)


def test_tile_edges_warm_table():
    names = _sensor(50)
    rng = np.random.default_rng(101)
    kid_batches = [np.concatenate([np.arange(50), rng.integers(0, 50, 206)])]
    kid_batches += [rng.integers(0, 50, n) for n in EDGE_ROWS]
    s = Stream(names, kid_batches, seed=102)
    assert_exact(run_engine(s), s)


def test_tile_edges_cold_table():
    # every row of every batch is a key never seen before: each one is
    # claimed, stashed as ~slot and resolved by the lookup pass
    names, kid_batches = [], []
    for n in EDGE_ROWS:
        kid_batches.append(np.arange(len(names), len(names) + n))
        names += [f"cold{n}_{j}".encode() for j in range(n)]
    s = Stream(names, kid_batches, seed=103)
    assert_exact(run_engine(s, n_keys_hint=4096), s)


def test_grid_stride_wrap_with_ragged_last_tile():
    names = _sensor(50)
    rng = np.random.default_rng(104)
    n = GRID * TILE + TILE + 1
    s = Stream(names, [rng.integers(0, 50, n)], seed=105, rows_per_ms=400)
    assert_exact(run_engine(s), s)


# ------------------------------------------------------------- stage boundary

@pytest.mark.parametrize("length", [8, 15, 16, 17, 24, 32, 33, 64])
def test_uniform_key_length(length):
    # 1024 rows of one key length: per-tile spans of 2 KB .. 16 KB, on both
    # sides of the stage size; first batch cold, second warm
    names = [(f"L{length}k{i:02d}-".encode() + b"abcdefghijklmnopqrstuvwxyz" * 3)
             [:length] for i in range(40)]
    assert {len(x) for x in names} == {length}
    rng = np.random.default_rng(110 + length)
    s = Stream(names, [rng.integers(0, 40, 1024), rng.integers(0, 40, 1024)],
               seed=111)
    assert_exact(run_engine(s), s)


def test_staged_and_fallback_tiles_in_one_launch():
    # four tiles: short keys, 300 B keys, short, 300 B
    names = _sensor(30) + [_long(i) for i in range(30)]
    rng = np.random.default_rng(120)
    kid = np.concatenate([rng.integers(0, 30, TILE), rng.integers(30, 60, TILE),
                          rng.integers(0, 30, TILE), rng.integers(30, 60, TILE)])
    s = Stream(names, [kid, kid[::-1].copy()], seed=121)
    assert_exact(run_engine(s), s)


@pytest.mark.parametrize("pos", [0, 128, 255])
def test_one_long_key_in_a_staged_tile(pos):
    # 255 short keys and one 300 B key: the span still fits the stage, so
    # the long key is hashed from the staged bytes and verified in the pool
    names = _sensor(30) + [_long(0), _long(1)]
    rng = np.random.default_rng(130 + pos)
    batches = []
    for long_id in (30, 31, 30):
        kid = rng.integers(0, 30, TILE)
        kid[pos] = long_id
        batches.append(kid)
    s = Stream(names, batches, seed=131)
    assert_exact(run_engine(s), s)


# ----------------------------------------------------------------- empty keys

def test_empty_keys():
    names = [b""] + _sensor(20)
    rng = np.random.default_rng(140)
    one_among = rng.integers(1, 21, 600)
    one_among[300] = 0
    whole_tile = rng.integers(1, 21, 3 * TILE)
    whole_tile[TILE:2 * TILE] = 0           # tile 1 has span 0
    last_row = rng.integers(1, 21, 700)
    last_row[-1] = 0
    only_empty = np.zeros(TILE, np.int64)   # a batch with no key bytes at all
    s = Stream(names, [one_among, whole_tile, last_row, only_empty], seed=141)
    assert_exact(run_engine(s), s)


def test_empty_key_first_seen_in_last_row():
    names = _sensor(20) + [b""]
    rng = np.random.default_rng(142)
    kid = rng.integers(0, 20, 513)
    kid[-1] = 20
    s = Stream(names, [kid], seed=143)
    assert_exact(run_engine(s), s)


# ------------------------------------------------------------------ alignment

@pytest.fixture(scope="module")
def align_stream():
    # short keys, a 17 B and a 40 B key (staged, pool-verified) and a tile of
    # 300 B keys (fallback), ragged last tile
    names = _sensor(30) + [b"seventeen_bytes_k", b"forty-byte-key-" + b"x" * 25]
    names += [_long(i) for i in range(4)]
    rng = np.random.default_rng(150)
    kid = np.concatenate([rng.integers(0, 32, 2 * TILE),
                          rng.integers(32, 36, TILE),
                          rng.integers(0, 32, 77)])
    return Stream(names, [kid, rng.permutation(kid)], seed=151)


@pytest.mark.parametrize("shift", range(16))
def test_column_base_shifted(align_stream, shift):
    assert_exact(run_engine(align_stream, shift=shift), align_stream)


@pytest.mark.parametrize("shift", [0, 3, 11])
def test_sliced_column_first_offset_5(align_stream, shift):
    assert_exact(run_engine(align_stream, shift=shift, lead=5), align_stream)


# ----------------------------------------------------------------- high bytes

def test_high_bytes_and_top_bit_near_misses():
    names = []
    for ln in (7, 8, 9, 16):
        base = bytes(0x80 + (37 * j + 11 * ln) % 0x80 for j in range(ln))
        assert min(base) >= 0x80
        names.append(base)
        for j in sorted({0, ln // 2, ln - 1}):  # top bit of one byte cleared
            names.append(base[:j] + bytes([base[j] & 0x7F]) + base[j + 1:])
    names.append(b"\xff" * 16)
    names.append(b"\xff" * 15 + b"\x7f")
    names.append(b"\x7f" + b"\xff" * 15)
    nk = len(names)
    rng = np.random.default_rng(160)
    b1 = rng.integers(0, nk // 2, 600)
    b2 = np.concatenate([np.arange(nk), rng.integers(0, nk, 600)])
    b3 = rng.integers(0, nk, 513)
    s = Stream(names, [b1, b2, b3], seed=161)
    assert_exact(run_engine(s), s)
