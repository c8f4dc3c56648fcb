"""CPU checks of the strict JSON-subset reference (tests/jsonref.py) and of
the shared edge-case vectors (tests/jsonvec.py) the GPU differential tests
feed to the device decoder: the reference has to be right on its own before
it may judge the kernel."""
import json
import math
import struct

import numpy as np
import pytest

from tests import jsonref, jsonvec


def test_reference_agrees_with_json_loads_on_dumps_output():
    rng = np.random.default_rng(5)
    for i in range(2000):
        ts = int(rng.integers(-(1 << 62), 1 << 62))
        key = "".join(chr(int(c)) for c in rng.integers(0x20, 0x7f, i % 9))
        key = key.replace("\\", "/").replace('"', "'")
        val = round(float(rng.uniform(-1e4, 1e4)), int(rng.integers(0, 8)))
        raw = json.dumps({"occurred_at_ms": ts, "extra": [None, {"k": "\\"}],
                          "sensor_name": key, "reading": val}).encode()
        got = jsonref.decode_record(raw)
        exp = json.loads(raw)
        assert got[0] == "ok", (raw, got)
        assert got[1] == exp["occurred_at_ms"]
        assert got[2] == exp["sensor_name"].encode()
        assert struct.pack("<d", got[3]) == struct.pack("<d", exp["reading"])


def test_custom_field_names_and_last_duplicate():
    raw = b'{"v":1,"t":3,"k":"x","v":2.5,"occurred_at_ms":9}'
    assert jsonref.decode_record(raw, ("t", "k", "v")) == ("ok", 3, b"x", 2.5)
    assert jsonref.decode_record(raw) == ("reject", "missing")


@pytest.mark.parametrize("text,sig,e10", [
    ("0", 1, 0), ("-0.0", 1, -1), ("0.000", 1, -3), ("1.500000", 7, -6),
    ("0.000123456789012345", 15, -18), ("123456789012345e22", 15, 22),
    ("100", 3, 0), ("0.0010", 2, -4), ("1E+5", 1, 5), ("12e-3", 2, -3),
    ("1e4294967297", 1, 4294967297), ("10.01", 4, -2),
])
def test_literal_shape(text, sig, e10):
    assert jsonref.literal_shape(text) == (sig, e10)


def test_accept_vectors_are_inside_the_subset():
    for v in jsonvec.VALUE_SPELLINGS:
        r = jsonref.decode_record(jsonvec.rec(val=v))
        assert r[0] == "ok" and r[3] == float(v), (v, r)
    assert math.copysign(1.0, jsonref.decode_record(
        jsonvec.rec(val="-0.0"))[3]) == -1.0
    for t in jsonvec.TS_SPELLINGS:
        r = jsonref.decode_record(jsonvec.rec(ts=t))
        assert r[0] == "ok" and r[1] == int(t), (t, r)
    assert jsonref.decode_record(
        jsonvec.rec(ts="-9223372036854775808"))[1] == jsonref.INT64_MIN
    for k in jsonvec.KEYS:
        r = jsonref.decode_record(jsonvec.rec(key='"' + k + '"'))
        assert r[0] == "ok" and r[2] == k.encode(), (k, r)
    assert {0, 1, 16, 17, 62, 63, 1024} <= {len(k.encode()) for k in jsonvec.KEYS}
    for raw in jsonvec.SKIPPED_MEMBER_RECORDS:
        r = jsonref.decode_record(raw)
        assert r[0] == "ok", (raw, r)
        assert json.loads(raw)["reading"] == r[3]
    # last duplicate wins
    assert jsonref.decode_record(jsonvec.SKIPPED_MEMBER_RECORDS[-2]) == \
        ("ok", 7, b"y", 2.5)
    assert jsonref.decode_record(jsonvec.SKIPPED_MEMBER_RECORDS[-1]) == \
        ("ok", 0, b"last", -3.25)
    ws = jsonref.decode_lines(jsonvec.WHITESPACE_PAYLOAD)
    assert ws == [("ok", 5, b"a b", 150.0), ("ok", 6, b"bb", -0.25),
                  ("ok", 7, b"", 3.0), ("ok", 8, b"cr-tail", 4.0)]


def test_reject_vectors_match_their_hand_classification():
    assert len(jsonvec.REJECTS) <= 80
    assert len({raw for raw, _ in jsonvec.REJECTS}) == len(jsonvec.REJECTS)
    for raw, kind in jsonvec.REJECTS:
        got = [r for r in jsonref.decode_lines(raw) if r[0] != "ok"]
        assert got == [("reject", kind)], (raw, kind, got)
    assert {k for _, k in jsonvec.REJECTS} == {"malformed", "missing", "subset"}


def test_reference_refuses_what_python_json_alone_would_accept():
    # json.loads takes these; strict JSON (serde_json) does not
    for v in ("NaN", "Infinity", "-Infinity"):
        assert json.loads(jsonvec.rec(val=v))
        assert jsonref.decode_record(jsonvec.rec(val=v)) == \
            ("reject", "malformed")
    # and '\n' is not whitespace inside a record
    assert jsonref.decode_record(b'{"occurred_at_ms":1,\n"sensor_name":"a",'
                                 b'"reading":1}') == ("reject", "malformed")


def test_literal_corpus_coverage():
    accepts, rejects = jsonvec.literal_corpus()
    assert len(accepts) >= 2000
    assert 0 < len(rejects) <= 60
    shapes = [jsonref.literal_shape(t) for t in accepts]
    assert {s for s, _ in shapes} == set(range(1, 16))
    assert {e for _, e in shapes} == set(range(-22, 23))
    rshapes = [jsonref.literal_shape(t) for t in rejects]
    # each boundary is hit by a literal whose ONLY defect is that boundary
    assert {16, 17} <= {s for s, e in rshapes if abs(e) <= 22}
    assert {23, -23} <= {e for s, e in rshapes if s <= 15}
    for t in accepts + rejects:
        # the generator emits JSON-grammar numbers only: json parses them
        json.loads(t)
    # every accept is a plain member of the subset when put in a record,
    # every sampled reject is "subset" and nothing else
    for t in accepts[:300]:
        assert jsonref.decode_record(jsonvec.rec(val=t)) == \
            ("ok", 1, b"a", float(t))
    for t in rejects:
        assert jsonref.decode_record(jsonvec.rec(val=t)) == \
            ("reject", "subset")
    # spellings the kernel has separate code for all occur
    joined = " ".join(accepts)
    for needle in ("e+", "E-", "e0", "0.0", "-0"):
        assert needle in joined, needle
    assert literal_corpus_is_deterministic()


def literal_corpus_is_deterministic():
    return jsonvec.literal_corpus() == jsonvec.literal_corpus()
