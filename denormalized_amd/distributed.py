"""Multi-shard helpers for the windowed-aggregate path.

Grouped pipelines shard by key (each rank owns disjoint groups — no merge
needed). GLOBAL aggregates (no GROUP BY) follow the reference's
Partial/Final two-stage plan (planner/streaming_window.rs:133-153,
FullWindowAggStream streaming_window.rs:640-1051): each shard emits partial
{count,min,max,sum} rows per window; merge_global_partials is the Final
stage, combining shards in rank order (deterministic; the f64 sum order is
rank-major, matching the reference's partition-merge structure rather than
single-stream row order — see DESIGN.md)."""
import numpy as np

from ._lib import AGG_BY_NAME, AGG_MEDIAN, VAR_AGGS

_VAR_NAMES = frozenset(n for n, code in AGG_BY_NAME.items() if code in VAR_AGGS)
_MED_NAMES = frozenset(n for n, code in AGG_BY_NAME.items() if code == AGG_MEDIAN)


def merge_global_partials(per_rank_batches):
    """per_rank_batches: list (rank order) of lists of emitted batches from a
    no-group WindowOp (each batch: one window, one row, with 'count'/'min'/
    'max'/'sum' or 'avg' columns). Returns merged rows keyed by window."""
    for batches in per_rank_batches:
        for b in batches:
            bad = sorted(k for k in b if k in _VAR_NAMES)
            if bad:
                raise ValueError(
                    f"merge_global_partials cannot merge {bad}: combining "
                    "Welford (count, mean, m2) partials needs a different "
                    "formula than count/min/max/sum and is not supported")
            bad = sorted(k for k in b if k in _MED_NAMES)
            if bad:
                raise ValueError(
                    f"merge_global_partials cannot merge {bad}: a median "
                    "does not combine from per-rank partials (it needs every "
                    "value of the window) and is not supported")
            ints = sorted(k for k in ("min", "max", "sum") if k in b
                          and np.asarray(b[k]).dtype.kind in "iu")
            if ints:
                raise ValueError(
                    f"merge_global_partials cannot merge integer-typed "
                    f"{ints} (an int64 value column): its float arithmetic "
                    "would re-round them; merging int64 partials is not "
                    "supported")
            # an aggregate on an extra value column reports its own mask as
            # "<name>_valid": such batches carry several columns' partials
            extra = sorted(k for k in b if k.endswith("_valid")
                           and k[:-len("_valid")] not in _VAR_NAMES)
            if extra:
                raise ValueError(
                    f"merge_global_partials cannot merge batches of a "
                    f"multi-column op ({extra}): it combines one value "
                    "column's count/min/max/sum partials only")
    acc = {}  # (wstart, wend) -> [count, min, max, sum, any_valid]
    order = []
    for batches in per_rank_batches:
        for b in batches:
            for i in range(b["n_rows"]):
                key = (int(b["window_start"][i]), int(b["window_end"][i]))
                cnt = int(b["count"][i])
                valid = bool(b["valid"][i])
                if key not in acc:
                    acc[key] = [0, None, None, 0.0]
                    order.append(key)
                a = acc[key]
                a[0] += cnt
                if valid:
                    mn, mx, sm = float(b["min"][i]), float(b["max"][i]), float(b["sum"][i]) if "sum" in b else cnt * float(b["avg"][i])
                    a[1] = mn if a[1] is None or mn < a[1] else a[1]
                    a[2] = mx if a[2] is None or mx > a[2] else a[2]
                    a[3] += sm
    out = []
    for key in sorted(order):
        cnt, mn, mx, sm = acc[key]
        valid = cnt > 0
        out.append({
            "window_start": key[0], "window_end": key[1], "count": cnt,
            "min": mn if valid else 0.0, "max": mx if valid else 0.0,
            "sum": sm if valid else 0.0,
            "avg": (sm / cnt) if valid else 0.0, "valid": valid,
        })
    return out
