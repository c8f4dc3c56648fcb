"""Expectation helper for windowed aggregates over several value columns.

One oracle.pyoracle.Oracle runs per distinct value column over (ts, keys,
vals_c, valid_c), all on the same push/finish schedule. Group existence, group
order and the window columns do not depend on the values, so the per-column
outputs must agree row for row on (key, window_start, window_end) — asserted
here — and can be zipped: every aggregate reads its own column's output.

Shapes used throughout:
  batches: list of (ts, keys, cols, valids); cols is a list of f64 arrays
           indexed by value-column number j, valids a list of bool arrays or
           None (all valid), same indexing.
  aggs:    list of (op, j, alias), op in count/min/max/sum/avg.
"""
import numpy as np

from oracle import pyoracle

CMP = {
    "<": np.less, "<=": np.less_equal, ">": np.greater,
    ">=": np.greater_equal, "==": np.equal, "!=": np.not_equal,
}


def distinct_cols(aggs):
    """Value-column numbers in order of first appearance: [primary, extras]."""
    order = []
    for _op, j, _alias in aggs:
        if j not in order:
            order.append(j)
    return order


def bitmap(mask):
    """Arrow LSB-first validity bitmap of a bool mask (None stays None)."""
    if mask is None:
        return None
    return np.packbits(np.asarray(mask, bool).astype(np.uint8),
                       bitorder="little")


def per_column(len_ms, slide_ms, batches, cols, finish=True, make=None):
    """{j: oracle fetch dict} for each column number in `cols`."""
    make = make or (lambda: pyoracle.Oracle(len_ms, slide_ms))
    out = {}
    for j in cols:
        o = make()
        for ts, keys, vals, valids in batches:
            vv = valids[j] if valids is not None else None
            o.push(ts, keys, vals[j],
                   None if vv is None else np.asarray(vv, np.uint8))
        if finish:
            o.finish()
        out[j] = o.fetch()
        o.close()
    return out


def expect(len_ms, slide_ms, batches, aggs, filt=None, finish=True, make=None):
    """Expected output columns: key, window_start, window_end, valid (the
    primary column's mask) and, per aggregate, alias and alias + "_valid".
    filt = (alias, cmp, literal): NULL never passes; count is never NULL."""
    order = distinct_cols(aggs)
    per = per_column(len_ms, slide_ms, batches, order, finish, make)
    base = per[order[0]]
    for j in order[1:]:
        for f in ("key", "window_start", "window_end"):
            assert np.array_equal(per[j][f], base[f]), \
                f"column {j} disagrees with the primary on {f}"
    exp = {f: base[f] for f in ("key", "window_start", "window_end")}
    exp["valid"] = base["valid"].astype(np.uint8)
    for op, j, alias in aggs:
        exp[alias] = per[j][op]
        exp[alias + "_valid"] = (
            np.ones(len(base["key"]), np.uint8) if op == "count"
            else per[j]["valid"].astype(np.uint8))
    if filt is not None:
        alias, cmp, lit = filt
        v = exp[alias].astype(np.float64)
        with np.errstate(invalid="ignore"):
            keep = CMP[cmp](v, lit) & exp[alias + "_valid"].astype(bool)
        exp = {k: a[keep] for k, a in exp.items()}
    return exp


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def assert_match(got, exp, aggs, nan_payload_free=False):
    """got: dict of concatenated engine output columns. Every column and mask
    bit-exact; values are compared where their mask says valid. With
    nan_payload_free a NaN matches a NaN of any payload (a fresh NaN's sign
    is ISA-specific); everything else stays bitwise."""
    order = distinct_cols(aggs)
    for f in ("key", "window_start", "window_end", "valid"):
        assert np.array_equal(np.asarray(got[f]), exp[f]), f
    for op, j, alias in aggs:
        own = alias + "_valid"
        if j != order[0]:
            assert np.array_equal(np.asarray(got[own]), exp[own]), own
        m = exp[own].astype(bool)
        g, e = np.asarray(got[alias])[m], exp[alias][m]
        if op == "count":
            assert np.array_equal(np.asarray(got[alias]), exp[alias]), alias
        else:
            same = _bits(g) == _bits(e)
            if nan_payload_free:
                same |= np.isnan(g) & np.isnan(e)
            assert same.all(), f"{alias} not bit-exact"
