"""Edge-case payloads for the JSON decoder, shared by the CPU test (which
checks the hand classification against tests/jsonref.py) and the GPU test
(which feeds the same bytes to the device decoder)."""
import numpy as np


def rec(ts="1", key='"a"', val="1.5", pre="", post=""):
    """One record with raw (already JSON-spelled) member texts."""
    return ('{' + pre + '"occurred_at_ms":' + ts + ',"sensor_name":' + key +
            ',"reading":' + val + post + '}').encode()


# ---- accepts (section a): every group decodes as ONE batch -------------

VALUE_SPELLINGS = [
    "0", "-0.0", "0e0", "1E5", "1e+5", "1.500000", "123456789012345e22",
    "999999999999999e-22", "1e-22", "1e22", "0.000123456789012345",
    "0.000000000000001", "-115.000000", "42", "-0", "0.0e-21", "1e+022",
    "100000000000000", "0.0000000000000000000012", "1.00000000000000E22", "12e22",
]
TS_SPELLINGS = ["0", "-5", "9223372036854775807", "-9223372036854775808",
                "-0", "1000000000000000000"]
KEYS = ["", "k", "s" * 16, "t" * 17, "u" * 62, "v" * 63,
        ("w0123456789abcde" * 64), "{}[],: x", " lead and trail ",
        "temp\u00e9rature_\u00b0C_\u4f20\u611f\u5668_\U0001f321"]

SKIPPED_MEMBER_RECORDS = [
    rec(pre=r'"note":"say \"hi\" \\ \/ \u00e9\n",'),
    rec(pre=r'"na\"me\\":1,"tab\there":"x",'),
    rec(pre=r'"\u0072":2,', post=r',"end\\":"\\"'),
    rec(pre=r'"meta":{"a":[1,{"b":"]}\"{["}],"c":"}","d":{}},"arr":[[],[[]]],'),
    rec(post=r',"m":[{"q":"\\"},"\\\"]"]'),
    rec(pre='"t":true,"f":false,"n":null,"i":-12,"z":0,"x":-1.5e-3,"s":"",'),
    # duplicates of schema fields: the last one wins
    (b'{"reading":1.0,"occurred_at_ms":1,"sensor_name":"x","reading":2.5,'
     b'"sensor_name":"y","occurred_at_ms":7}'),
    b'{"reading":1,"reading":2,"reading":-3.25,"sensor_name":"","occurred_at_ms":0,"sensor_name":"last"}',
]

WHITESPACE_PAYLOAD = (
    b'\t { \t"occurred_at_ms" \t: \t5 \t, \t"sensor_name" : "a b" , '
    b'"reading" \t:\t 1.5e2 \t} \t\r\n'
    b'{"reading":-0.25,"sensor_name":"bb","occurred_at_ms":6}\r\n'
    b' {\r"x" : [ 1 , { "y" : "z" } ] ,\r"occurred_at_ms":7,"sensor_name":"","reading":3 }\r \r\n'
    b'{"occurred_at_ms":8,"sensor_name":"cr-tail","reading":4}\r')

# ---- rejects (section b): (payload, hand classification) ---------------

REJECTS = [
    # empty numeric literals (were decoded as zero)
    (rec(val=""), "malformed"),
    (b'{"reading":,"occurred_at_ms":1,"sensor_name":"a"}', "malformed"),
    (rec(val="-"), "malformed"),
    (b'{"sensor_name":"a","reading":1.5,"occurred_at_ms":}', "malformed"),
    (b'{"sensor_name":"a","reading":1.5,"occurred_at_ms":-}', "malformed"),
    # not the JSON number grammar
    (rec(val="1."), "malformed"),
    (rec(val=".5"), "malformed"),
    (rec(val="1e"), "malformed"),
    (rec(val="1e+"), "malformed"),
    (rec(val="01.5"), "malformed"),
    (rec(val="-01"), "malformed"),
    (rec(val="1.e5"), "malformed"),
    (rec(val="+1"), "malformed"),
    (rec(val="1.5.2"), "malformed"),
    (rec(val="0x10"), "malformed"),
    (rec(val="NaN"), "malformed"),
    (rec(val="Infinity"), "malformed"),
    (rec(val="-Infinity"), "malformed"),
    (rec(ts="5."), "malformed"),
    (rec(ts="007"), "malformed"),
    (rec(pre='"x":1.,'), "malformed"),
    (rec(pre='"x":-,'), "malformed"),
    # exponent without wraparound
    (rec(val="1e4294967297"), "subset"),
    (rec(val="1e-4294967297"), "subset"),
    (rec(val="1e18446744073709551617"), "subset"),
    (rec(val="1e400"), "subset"),
    (rec(val="0e23"), "subset"),
    # timestamp range and literal form
    (rec(ts="9223372036854775808"), "subset"),
    (rec(ts="-9223372036854775809"), "subset"),
    (rec(ts="18446744073709551621"), "subset"),
    (rec(ts="12345678901234567890123"), "subset"),
    (rec(ts="5e0"), "subset"),
    (rec(ts="5.0"), "subset"),
    (rec(ts="1E3"), "subset"),
    # bytes after the closing brace / before the opening one
    (rec() + b"garbage", "malformed"),
    (rec() + rec(), "malformed"),
    (rec() + b" x", "malformed"),
    (rec() + b",", "malformed"),
    (rec() + b"}", "malformed"),
    (b"x" + rec(), "malformed"),
    # comma discipline
    (b'{"occurred_at_ms":1"sensor_name":"a","reading":1.5}', "malformed"),
    (b'{"occurred_at_ms":1 "sensor_name":"a","reading":1.5}', "malformed"),
    (b'{"occurred_at_ms":1,,"sensor_name":"a","reading":1.5}', "malformed"),
    (rec(pre=","), "malformed"),
    (rec(post=","), "malformed"),
    (b'{"occurred_at_ms":1,"sensor_name":"a","reading":1.5 , }', "malformed"),
    # skipped scalars must still be JSON
    (rec(pre='"x":-true,'), "malformed"),
    (rec(pre='"x":tru,'), "malformed"),
    (rec(pre='"x":nulll,'), "malformed"),
    (rec(pre='"x":truefalse,'), "malformed"),
    (rec(post=',"x":fals'), "malformed"),
    # already rejected before this change: pinned with their message class
    (rec(val="1234567890123456"), "subset"),
    (rec(val="0.12345678901234567"), "subset"),
    (rec(val="1.000000000000000e0"), "subset"),
    (rec(val="1e23"), "subset"),
    (rec(val="1e-23"), "subset"),
    (rec(val="1.5e-22"), "subset"),
    (rec(val="0.1e24"), "subset"),
    (rec(key=r'"a\n"'), "subset"),
    (rec(key=r'"\u0061"'), "subset"),
    (b'{"sensor_name":"a","reading":1.5}', "missing"),
    (b'{"occurred_at_ms":1,"reading":1.5}', "missing"),
    (b'{"occurred_at_ms":1,"sensor_name":"a"}', "missing"),
    (b'{}', "missing"),
    (b' { } ', "missing"),
    (rec(val='"1.5"'), "malformed"),
    (rec(ts='"1"'), "malformed"),
    (rec(key="5"), "malformed"),
    (rec(key="null"), "malformed"),
    (rec(key="true"), "malformed"),
    (rec(val="null"), "malformed"),
    (rec(val="[1]"), "malformed"),
    (rec(ts='{"a":1}'), "malformed"),
    (b"\n", "malformed"),
    (rec() + b"\n\n" + rec() + b"\n", "malformed"),  # blank line inside
    (b" \t\r\n", "malformed"),
    (b'{"occurred_at_ms":1,"sensor_name":"a', "malformed"),
    (b'{"occurred_at_ms":1,"sensor_name":"a","reading":1.5', "malformed"),
    (b'{"occurred_at_ms":1,"sensor_name":"a","reading":1.5,"x":[1,2',
     "malformed"),
    (b"not json at all", "malformed"),
]


# ---- random literal text (section d) -----------------------------------

def gen_literal(rng):
    """One JSON-grammar number literal as TEXT: a sign, 1-17 significant
    digits, optional leading zeros and fraction, optional e/E with optional
    sign, e10 (= exponent - fraction digits) drawn from -25..25."""
    nsig = int(rng.integers(1, 18))
    e10 = int(rng.integers(-25, 26))
    if rng.random() < 0.02:
        digits, nsig = "0", 1
    else:
        digits = str(int(rng.integers(1, 10))) + "".join(
            str(int(d)) for d in rng.integers(0, 10, nsig - 1))
    k = int(rng.integers(0, nsig + 1))  # digits before the point
    ipart, fpart = digits[:k], digits[k:]
    if not ipart:  # 0.000ddd: leading zeros on both sides of the point
        ipart = "0"
        fpart = "0" * int(rng.integers(0, 5)) + fpart
    if digits == "0":
        ipart, fpart = "0", ("0" * int(rng.integers(0, 4)))
    exp = e10 + len(fpart)
    text = ("-" if rng.random() < 0.4 else "") + ipart
    if fpart:
        text += "." + fpart
    if exp != 0 or rng.random() < 0.3:
        sign = "-" if exp < 0 else ("+" if rng.random() < 0.4 else "")
        text += ("e" if rng.random() < 0.5 else "E") + sign + \
            ("0" if rng.random() < 0.2 else "") + str(abs(exp))
    return text


def literal_corpus(seed=20251, n=3400, max_rejects=60):
    """(accept literals, sampled reject literals), classified by jsonref.
    The reject sample takes the first literal of each boundary class (16 and
    17 significant digits, e10 = +23 and -23) and then the earliest others."""
    from tests import jsonref
    rng = np.random.default_rng(seed)
    accepts, rejects = [], []
    for _ in range(n):
        t = gen_literal(rng)
        (accepts if jsonref.classify_value(t) is not None else rejects).append(t)
    picked, seen = [], set()
    for t in rejects:
        sig, e10 = jsonref.literal_shape(t)
        # a boundary class is "this defect alone": the other rule holds
        cls = (("sig", sig) if sig in (16, 17) and abs(e10) <= 22 else
               ("e10", e10) if abs(e10) == 23 and sig <= 15 else None)
        if cls and cls not in seen:
            seen.add(cls)
            picked.append(t)
    for t in rejects:
        if len(picked) >= max_rejects:
            break
        if t not in picked:
            picked.append(t)
    return accepts, picked
