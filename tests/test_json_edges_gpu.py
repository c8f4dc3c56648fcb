"""JSON decoder edge cases: the device parser vs tests/jsonref.py (a strict
restatement of the documented subset on top of Python's json module) on the
same bytes. Accepts are compared bit for bit; rejects must fail with the
message class jsonref assigns. Every expectation comes from jsonref, never
from the decoder."""
import ctypes
import functools

import numpy as np
import pytest

import __graft_entry__ as graft
from tests import jsonref, jsonvec
from tests.test_json_ingest import decode_all, to_dev

pytestmark = pytest.mark.gpu

CLASS_MSG = {"subset": "exact parse subset", "malformed": "malformed",
             "missing": "missing"}
SHORT = dict(ts_field="t", key_field="k", val_field="v")
SHORT_FIELDS = ("t", "k", "v")


@pytest.fixture(scope="module", autouse=True)
def built():
    graft.build()


def guard(fn, *a, **kw):
    """Run a decode; a HIP runtime error (not one of the decoder's three
    rejections) ends the session instead of running more GPU work."""
    try:
        return fn(*a, **kw)
    except RuntimeError as e:
        if not any(m in str(e) for m in CLASS_MSG.values()):
            pytest.exit(f"device error, stopping: {e}", returncode=3)
        raise


def expect_ok(raw, fields=jsonref.FIELDS):
    rows = jsonref.decode_lines(raw, fields)
    assert all(r[0] == "ok" for r in rows), [r for r in rows if r[0] != "ok"]
    return rows


def assert_rows(got, rows):
    ts, keys, v = got
    assert len(ts) == len(rows)
    exp_ts = np.array([r[1] for r in rows], np.int64)
    exp_v = np.array([r[3] for r in rows], np.float64)
    bad = np.flatnonzero(ts != exp_ts)
    assert bad.size == 0, (bad[:5], ts[bad[:5]], exp_ts[bad[:5]])
    assert [k.encode() for k in keys] == [r[2] for r in rows]
    bad = np.flatnonzero(v.view(np.int64) != exp_v.view(np.int64))
    assert bad.size == 0, (bad[:5], v[bad[:5]], exp_v[bad[:5]])


def assert_accepts(raw, fields=jsonref.FIELDS, **kw):
    rows = expect_ok(raw, fields)
    assert_rows(guard(decode_all, raw, **kw), rows)
    return rows


def assert_rejects(raw, **kw):
    kinds = {r[1] for r in jsonref.decode_lines(raw) if r[0] == "reject"}
    assert len(kinds) == 1, kinds
    (kind,) = kinds
    try:
        got = guard(decode_all, raw, **kw)
    except RuntimeError as e:
        others = [m for k, m in CLASS_MSG.items() if k != kind]
        assert CLASS_MSG[kind] in str(e) and \
            not any(m in str(e) for m in others), (raw, kind, str(e))
        return
    pytest.fail(f"{raw!r}: expected a {kind} rejection, decoded "
                f"ts={list(got[0])} keys={got[1]} v={list(got[2])}")


# ---- a. accepts, bit-exact ---------------------------------------------

def test_value_literal_spellings():
    raw = b"\n".join(jsonvec.rec(ts=str(i), val=v)
                     for i, v in enumerate(jsonvec.VALUE_SPELLINGS))
    rows = assert_accepts(raw)
    assert np.signbit(rows[jsonvec.VALUE_SPELLINGS.index("-0.0")][3])


def test_timestamp_spellings():
    assert_accepts(b"\n".join(jsonvec.rec(ts=t) for t in jsonvec.TS_SPELLINGS)
                   + b"\n")


def test_key_shapes():
    assert_accepts(b"\n".join(jsonvec.rec(key='"' + k + '"')
                              for k in jsonvec.KEYS))


def test_skipped_members_escapes_nesting_duplicates():
    assert_accepts(b"\n".join(jsonvec.SKIPPED_MEMBER_RECORDS) + b"\n")


def test_crlf_and_whitespace_around_every_token():
    assert_accepts(jsonvec.WHITESPACE_PAYLOAD)
    assert_accepts(jsonvec.WHITESPACE_PAYLOAD + b"\n")


# ---- b. rejects: one bad record per decode, message class asserted ------

@pytest.mark.parametrize(
    "i", range(len(jsonvec.REJECTS)),
    ids=[f"{i:02d}-{k}" for i, (_, k) in enumerate(jsonvec.REJECTS)])
def test_reject_message_class(i):
    assert_rejects(jsonvec.REJECTS[i][0])


# ---- c. decoder lifecycle on one handle ---------------------------------

def read_cols(n, pts, pko, pkd, pv):
    from denormalized_amd import _lib
    L = _lib.lib()
    ts = np.empty(n, np.int64)
    ko = np.empty(n + 1, np.int32)
    v = np.empty(n, np.float64)
    L.dz_memcpy_d2h(ts.ctypes.data_as(ctypes.c_void_p), pts, n * 8)
    L.dz_memcpy_d2h(ko.ctypes.data_as(ctypes.c_void_p), pko, (n + 1) * 4)
    L.dz_memcpy_d2h(v.ctypes.data_as(ctypes.c_void_p), pv, n * 8)
    kd = np.empty(max(1, int(ko[-1])), np.uint8)
    L.dz_memcpy_d2h(kd.ctypes.data_as(ctypes.c_void_p), pkd, int(ko[-1]))
    return ts, ko, kd[:int(ko[-1])].tobytes(), v


def assert_cols(cols, rows):
    ts, ko, kd, v = cols
    assert np.array_equal(ts, np.array([r[1] for r in rows], np.int64))
    exp_ko = np.zeros(len(rows) + 1, np.int32)
    np.cumsum([len(r[2]) for r in rows], out=exp_ko[1:])
    assert np.array_equal(ko, exp_ko)  # the whole offsets column
    assert kd == b"".join(r[2] for r in rows)
    assert np.array_equal(v.view(np.int64),
                          np.array([r[3] for r in rows]).view(np.int64))


@pytest.fixture
def handle():
    from denormalized_amd import JsonDecoder
    dec = JsonDecoder(device=0)
    bufs = []

    def decode(raw):
        d = to_dev(raw)
        bufs.append(d)
        return guard(dec.decode, d.ptr, len(raw))

    decode.dec = dec
    yield decode
    dec.close()
    for d in bufs:
        d.free()


def good_batch(n, salt=0):
    return b"".join(jsonvec.rec(ts=str(salt + i), key=f'"s{(salt + i) % 13}"',
                                val=f"{salt + i}.25") + b"\n"
                    for i in range(n))


def test_reject_then_good_batch_on_same_handle(handle):
    with pytest.raises(RuntimeError, match="missing"):
        handle(b'{"occurred_at_ms":1,"sensor_name":"a"}\n')
    assert handle.dec.batch()[0] == 0
    raw = good_batch(40)
    out = handle(raw)
    assert out[0] == 40
    assert_cols(read_cols(*out), expect_ok(raw))
    assert handle.dec.batch()[0] == 40


def test_consecutive_rejects_report_their_own_message(handle):
    seq = [(jsonvec.rec(val="1e23"), "subset"),
           (b'{"occurred_at_ms":1,"sensor_name":"a"}', "missing"),
           (jsonvec.rec() + b"x", "malformed"),
           (jsonvec.rec(ts="5e0"), "subset"),
           (b"{}", "missing")]
    for raw, kind in seq:
        assert jsonref.decode_record(raw) == ("reject", kind)
        with pytest.raises(RuntimeError) as ei:
            handle(raw)
        others = [m for k, m in CLASS_MSG.items() if k != kind]
        assert CLASS_MSG[kind] in str(ei.value) and \
            not any(m in str(ei.value) for m in others), (raw, str(ei.value))
        assert handle.dec.batch()[0] == 0


def test_columns_survive_the_next_decode(handle):
    raw_a, raw_b = good_batch(300), good_batch(299, salt=1000)
    a = handle(raw_a)
    assert_cols(read_cols(*a), expect_ok(raw_a))
    b = handle(raw_b)  # no larger than A
    assert_cols(read_cols(*b), expect_ok(raw_b))
    assert_cols(read_cols(*a), expect_ok(raw_a))  # A still intact
    # a rejected decode in between does not disturb the last good batch
    with pytest.raises(RuntimeError, match="malformed"):
        handle(b"nope\n")
    assert_cols(read_cols(*b), expect_ok(raw_b))


def test_growth_and_empty_buffer(handle):
    small, large = good_batch(3), good_batch(5000, salt=7)
    s = handle(small)
    assert_cols(read_cols(*s), expect_ok(small))
    g = handle(large)  # grows: must not free the columns of the last decode
    assert g[0] == 5000
    assert_cols(read_cols(*g), expect_ok(large))
    assert_cols(read_cols(*s), expect_ok(small))
    larger = good_batch(6000, salt=11)
    h = handle(larger)  # grows the other buffer; `large` stays readable
    assert_cols(read_cols(*h), expect_ok(larger))
    assert_cols(read_cols(*g), expect_ok(large))
    assert handle(b"")[0] == 0
    assert handle.dec.batch()[0] == 0


# ---- d. random literal differential -------------------------------------

def test_random_literal_text_bitwise():
    accepts, _ = jsonvec.literal_corpus()
    assert len(accepts) >= 2000
    raw = b"\n".join(jsonvec.rec(ts=str(i), key=f'"k{i % 7}"', val=t)
                     for i, t in enumerate(accepts))
    rows = expect_ok(raw)
    ts, keys, v = guard(decode_all, raw)
    exp = np.array([r[3] for r in rows])
    bad = np.flatnonzero(v.view(np.int64) != exp.view(np.int64))
    assert bad.size == 0, [(accepts[i], v[i], exp[i]) for i in bad[:8]]
    assert_rows((ts, keys, v), rows)


def test_random_literal_text_rejects():
    _, rejects = jsonvec.literal_corpus()
    assert 0 < len(rejects) <= 60
    wrong = []
    for t in rejects:
        try:
            assert_rejects(jsonvec.rec(val=t))
        except (AssertionError, pytest.fail.Exception) as e:
            wrong.append((t, str(e)[:160]))
    assert not wrong, wrong


# ---- e. record splitting and the offset scan ----------------------------

def short_rec(i):
    return b'{"t":%d,"k":"%s","v":%d}' % (i % 10, b"ab"[:i % 3], (i * 7) % 10)


@pytest.mark.parametrize("tail_newline", [True, False])
def test_newlines_swept_across_the_chunk_seam(tail_newline):
    """~20 KB payloads split into 3 chunks of ceil(n/3) bytes. Growing a
    skipped string in the first record by one byte moves every later newline
    by 1 and the seams by 1/3 and 2/3: over 70 steps the seams slide >= 23
    bytes against the records, which are at most 23 bytes with their
    newline, so every alignment of a newline to a seam occurs."""
    rest = b"\n".join(short_rec(i) for i in range(1, 900))
    rest_rows = expect_ok(rest, SHORT_FIELDS)
    for j in range(70):
        first = b'{"p":"%s","t":0,"k":"F","v":0.5}' % (b"x" * (60 + j))
        raw = first + b"\n" + rest + (b"\n" if tail_newline else b"")
        assert 16384 < len(raw) <= 24576
        rows = expect_ok(first, SHORT_FIELDS) + rest_rows
        assert_rows(guard(decode_all, raw, **SHORT), rows)


def test_buffer_over_4mib_with_odd_byte_count():
    pad = "p" * 150
    lines = [f'{{"occurred_at_ms":{1_000_000 + i},"sensor_name":"sensor_'
             f'{i % 50}","reading":{(i * 37) % 115}.{i % 1000000:06d},'
             f'"pad":"{pad}"}}' for i in range(19500)]
    raw = ("\n".join(lines) + "\n").encode()
    if len(raw) % 2 == 0:
        raw = raw[:-3] + b'x"}\n'  # one more pad byte in the last record
    assert len(raw) > (4 << 20) and len(raw) % 2 == 1
    assert -(-len(raw) // 512) % 64 != 0  # capped chunk, not a multiple of 64
    assert_accepts(raw)


@functools.lru_cache(maxsize=None)
def scan_records():
    recs = [b'{"t":%d,"k":"%s","v":%d.5}' %
            (i, b"0123456789A"[:(i * 7) % 12], i % 97) for i in range(8193)]
    rows = [jsonref.decode_record(r, SHORT_FIELDS) for r in recs]
    assert all(r[0] == "ok" for r in rows)
    assert {len(r[2]) for r in rows} == set(range(12))
    return recs, rows


@pytest.mark.parametrize("n,tail_newline", [
    (1, True), (1, False), (4095, True), (4096, True), (4097, False),
    (8192, False), (8193, True)])
def test_record_counts_at_the_scan_block_edges(n, tail_newline):
    from denormalized_amd import JsonDecoder
    recs, rows = scan_records()
    raw = b"\n".join(recs[:n]) + (b"\n" if tail_newline else b"")
    dec = JsonDecoder(device=0, **SHORT)
    d = to_dev(raw)
    try:
        out = guard(dec.decode, d.ptr, len(raw))
        assert out[0] == n
        assert_cols(read_cols(*out), rows[:n])
    finally:
        dec.close()
        d.free()
