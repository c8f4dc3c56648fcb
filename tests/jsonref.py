"""Strict restatement of the JSON decoder's documented subset
(include/denormalized_amd.h, "JSON ingest"), for differential tests.

Python's json module decides validity and structure (it is strict JSON once
NaN/Infinity are refused, like the reference's serde_json::from_slice);
float(literal_text) is the correctly-rounded value. Nothing here is shared
with the device parser: no hand-written tokenizer, no power-of-ten table.

decode_record(raw) -> ("ok", ts, key_bytes, value) | ("reject", kind)
kind: "malformed" (not one strict-JSON object on the line, or a schema field
of the wrong JSON type), "missing" (a schema field is absent), "subset"
(valid JSON outside the documented exact-parse subset).

A record with several defects is classified malformed > subset > missing;
the device parser stops at the first defect it meets, so differential tests
feed records with ONE defect. A duplicated schema field is judged by its
last occurrence only (serde_json Map semantics).
"""
import json
import json.decoder
import json.scanner

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1
MAX_SIG_DIGITS = 15
MAX_ABS_E10 = 22

FIELDS = ("occurred_at_ms", "sensor_name", "reading")


class _Num:
    """A number literal, kept as the text the payload spelled."""
    __slots__ = ("text",)

    def __init__(self, text):
        self.text = text


class _Str(str):
    """A string VALUE, remembering whether its raw spelling held a '\\'."""
    escaped = False


class _Obj:
    __slots__ = ("pairs",)

    def __init__(self, pairs):
        self.pairs = pairs


def _refuse_constant(name):
    raise ValueError(f"{name} is not JSON")


def _scan_string(s, end, strict=True):
    v, nend = json.decoder.scanstring(s, end, strict)
    out = _Str(v)
    out.escaped = "\\" in s[end:nend - 1]
    return out, nend


class _Decoder(json.JSONDecoder):
    def __init__(self):
        super().__init__(object_pairs_hook=_Obj, parse_float=_Num,
                         parse_int=_Num, parse_constant=_refuse_constant)
        # the pure-Python scanner is the one that honours parse_string,
        # which is how a string value's raw spelling is observed
        self.parse_string = _scan_string
        self.scan_once = json.scanner.py_make_scanner(self)


_DECODER = _Decoder()


def literal_shape(text):
    """(significant digits, e10) of a JSON-grammar number literal.

    Significant digits: integer and fraction digits as written, minus the
    zeros before the first non-zero digit (on either side of the point);
    trailing zeros count; an all-zero literal has 1.
    e10 = exponent - number of fraction digits (no wraparound: Python ints).
    """
    t = text[1:] if text.startswith("-") else text
    mant, _, exp = t.replace("E", "e").partition("e")
    ipart, _, fpart = mant.partition(".")
    sig = len((ipart + fpart).lstrip("0")) or 1
    return sig, (int(exp) if exp else 0) - len(fpart)


def classify_value(text):
    sig, e10 = literal_shape(text)
    if sig > MAX_SIG_DIGITS or abs(e10) > MAX_ABS_E10:
        return None
    return float(text)


def classify_ts(text):
    if any(c in text for c in ".eE"):
        return None
    v = int(text)
    return v if INT64_MIN <= v <= INT64_MAX else None


def decode_record(raw, fields=FIELDS):
    ts_f, key_f, val_f = fields
    if b"\n" in raw:
        return ("reject", "malformed")  # one record per line
    try:
        # json's own whitespace set is " \t\n\r"; '\n' is excluded above, so
        # what may surround the object is exactly space, tab and CR
        top = _DECODER.decode(raw.decode("utf-8"))
    except (ValueError, RecursionError):
        return ("reject", "malformed")
    if not isinstance(top, _Obj):
        return ("reject", "malformed")
    members = dict(top.pairs)  # last duplicate wins
    ts, key, val = (members.get(f, members) for f in (ts_f, key_f, val_f))
    for got, want in ((ts, _Num), (key, _Str), (val, _Num)):
        if got is not members and not isinstance(got, want):
            return ("reject", "malformed")  # wrong JSON type
    subset = False
    ts_v = val_v = None
    if ts is not members:
        ts_v = classify_ts(ts.text)
        subset |= ts_v is None
    if val is not members:
        val_v = classify_value(val.text)
        subset |= val_v is None
    if key is not members:
        subset |= key.escaped
    if subset:
        return ("reject", "subset")
    if ts is members or key is members or val is members:
        return ("reject", "missing")
    return ("ok", ts_v, str(key).encode("utf-8"), val_v)


def decode_lines(buf, fields=FIELDS):
    """Split a payload the way the decoder documents it ('\\n'-separated,
    a trailing '\\n' does not open another record) and decode every line."""
    if not buf:
        return []
    lines = buf.split(b"\n")
    if buf.endswith(b"\n"):
        lines.pop()
    return [decode_record(ln, fields) for ln in lines]
