"""ctypes binding over the C ABI (include/denormalized_amd.h).

The HIP engine is REQUIRED for compute: load failures and missing-GPU errors
raise immediately — there is no CPU fallback in the product path.
"""
import ctypes
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
# DZ_ENGINE_SO: A/B hook — point at an alternatively-built engine .so
_SO = os.environ.get("DZ_ENGINE_SO") or os.path.join(_DIR, "_dzengine.so")

DZ_OK = 0

WINDOW_TUMBLING = 0
WINDOW_SLIDING = 1
AGG_COUNT, AGG_MIN, AGG_MAX, AGG_SUM, AGG_AVG = 0, 1, 2, 3, 4
AGG_VAR_SAMP, AGG_VAR_POP, AGG_STDDEV_SAMP, AGG_STDDEV_POP = 5, 6, 7, 8
AGG_MEDIAN = 16
VAR_AGGS = frozenset((AGG_VAR_SAMP, AGG_VAR_POP, AGG_STDDEV_SAMP,
                      AGG_STDDEV_POP))
KEY_UTF8, KEY_INT64, KEY_DENSE_INT64 = 0, 1, 2
VALUE_F64, VALUE_INT64 = 0, 1
VALUE_DTYPES = {"float64": VALUE_F64, "int64": VALUE_INT64}
INT_AGGS = frozenset((AGG_MIN, AGG_MAX, AGG_SUM))  # int64 on an int64 column
CMP = {"<": 0, "<=": 1, ">": 2, ">=": 3, "==": 4, "!=": 5}
AGG_BY_NAME = {"count": AGG_COUNT, "min": AGG_MIN, "max": AGG_MAX,
               "sum": AGG_SUM, "avg": AGG_AVG, "average": AGG_AVG,
               # the reference's functions.py: var/stddev are the sample forms
               "var_samp": AGG_VAR_SAMP, "var_sample": AGG_VAR_SAMP,
               "var": AGG_VAR_SAMP, "var_pop": AGG_VAR_POP,
               "stddev": AGG_STDDEV_SAMP, "stddev_samp": AGG_STDDEV_SAMP,
               "stddev_pop": AGG_STDDEV_POP,
               # exact median: no _valid companion, it follows "valid"
               "median": AGG_MEDIAN}


class DzAggDesc(ctypes.Structure):
    _fields_ = [("op", ctypes.c_int), ("input_col", ctypes.c_int32)]


class DzWindowDesc(ctypes.Structure):
    _fields_ = [
        ("window_type", ctypes.c_int),
        ("length_ms", ctypes.c_int64),
        ("slide_ms", ctypes.c_int64),
        ("ts_col", ctypes.c_int32),
        ("group_col", ctypes.c_int32),
        ("key_kind", ctypes.c_int),
        ("aggs", ctypes.POINTER(DzAggDesc)),
        ("n_aggs", ctypes.c_int32),
        ("n_keys_hint", ctypes.c_int64),
        ("device", ctypes.c_int32),
        ("max_open_windows", ctypes.c_int32),
    ]


class DzColumn(ctypes.Structure):
    _fields_ = [
        ("len", ctypes.c_int64),
        ("validity", ctypes.c_void_p),
        ("offsets", ctypes.c_void_p),
        ("data", ctypes.c_void_p),
    ]


class DzBatch(ctypes.Structure):
    _fields_ = [("n_rows", ctypes.c_int64), ("n_cols", ctypes.c_int32),
                ("cols", ctypes.POINTER(DzColumn))]


class DzOutBatch(ctypes.Structure):
    _fields_ = [
        ("n_rows", ctypes.c_int64),
        ("key_i64", ctypes.POINTER(ctypes.c_int64)),
        ("key_offsets", ctypes.POINTER(ctypes.c_int32)),
        # c_void_p, NOT c_char_p: key bytes are arbitrary (may contain NUL);
        # a c_char_p attribute read returns a NUL-truncated copy, and
        # string_at on that copy could read out of bounds.
        ("key_data", ctypes.c_void_p),
        ("agg_cols", ctypes.POINTER(ctypes.c_void_p)),
        ("agg_valid", ctypes.POINTER(ctypes.c_uint8)),
        ("window_start_ms", ctypes.POINTER(ctypes.c_int64)),
        ("window_end_ms", ctypes.POINTER(ctypes.c_int64)),
        # n_aggs per-aggregate byte masks; NULL entry = follows agg_valid;
        # the pointer itself is NULL for ops without a variance aggregate
        ("agg_valid_cols", ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))),
    ]


class DzKernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", ctypes.c_uint64),
                ("total_ms", ctypes.c_double), ("bytes_per_launch_alg", ctypes.c_double)]


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(
                f"denormalized_amd HIP engine missing: {_SO}. "
                "Run __graft_entry__.build() (hipcc --offload-arch=gfx950).")
        L = ctypes.CDLL(_SO)
        p = ctypes.c_void_p
        i64 = ctypes.c_int64
        L.dz_window_op_create.restype = p
        L.dz_window_op_create.argtypes = [ctypes.POINTER(DzWindowDesc)]
        L.dz_window_op_push.argtypes = [p, ctypes.POINTER(DzBatch)]
        L.dz_window_op_push_device.argtypes = [p, i64, p, p, p]
        try:
            L.dz_window_op_push_device_borrowed.argtypes = [p, i64, p, p, p]
        except AttributeError:  # older engine build (A/B hook)
            pass
        L.dz_window_op_push_device_utf8.argtypes = [p, i64, p, p, p, p]
        L.dz_window_op_push_device_i64.argtypes = [p, i64, p, p, p]
        try:
            L.dz_window_op_set_extra_values.argtypes = [
                p, i64, ctypes.POINTER(p), ctypes.POINTER(p)]
        except AttributeError:  # older engine build (A/B hook)
            pass
        try:
            L.dz_window_op_set_value_type.argtypes = [p, ctypes.c_int32,
                                                      ctypes.c_int]
        except AttributeError:  # older engine build (A/B hook)
            pass
        L.dz_generate_utf8.argtypes = [ctypes.c_int32, ctypes.c_uint64, i64,
                                       i64, i64, p, p, p]
        L.dz_window_op_poll.argtypes = [p, ctypes.POINTER(ctypes.POINTER(DzOutBatch))]
        L.dz_window_op_finish.argtypes = [p]
        L.dz_window_op_drain.argtypes = [p]
        L.dz_window_op_destroy.argtypes = [p]
        L.dz_last_error.restype = ctypes.c_char_p
        L.dz_last_error.argtypes = [p]
        L.dz_window_op_advance_watermark.argtypes = [p, i64]
        L.dz_window_op_watermark.restype = i64
        L.dz_window_op_watermark.argtypes = [p]
        L.dz_window_op_open_windows.restype = i64
        L.dz_window_op_open_windows.argtypes = [p]
        L.dz_window_op_set_filter.argtypes = [p, ctypes.c_int32, ctypes.c_int32,
                                              ctypes.c_double]
        L.dz_window_op_kernel_stats.argtypes = [p, ctypes.POINTER(DzKernelStat),
                                                ctypes.c_int32,
                                                ctypes.POINTER(ctypes.c_int32)]
        L.dz_generate.argtypes = [ctypes.c_int32, ctypes.c_uint64, i64, i64, i64,
                                  i64, i64, p, p, p, p]
        L.dz_device_malloc.argtypes = [ctypes.c_int32, ctypes.c_size_t,
                                       ctypes.POINTER(p)]
        L.dz_device_free.argtypes = [p]
        L.dz_device_synchronize.argtypes = [ctypes.c_int32]
        L.dz_memcpy_d2h.argtypes = [p, p, ctypes.c_size_t]
        L.dz_memcpy_h2d.argtypes = [p, p, ctypes.c_size_t]
        L.dz_join_op_create.restype = p
        L.dz_join_op_create.argtypes = [ctypes.c_int32, i64]
        L.dz_join_op_destroy.argtypes = [p]
        L.dz_join_last_error.restype = ctypes.c_char_p
        L.dz_join_last_error.argtypes = [p]
        L.dz_join_op_push_build.argtypes = [p, i64, p, p]
        L.dz_join_op_push_probe.argtypes = [p, i64, p, p, p]
        L.dz_join_op_matches.argtypes = [p, ctypes.POINTER(i64),
                                         ctypes.POINTER(p), ctypes.POINTER(p),
                                         ctypes.POINTER(p)]
        L.dz_join_op_unmatched.restype = i64
        L.dz_join_op_unmatched.argtypes = [p]
        L.dz_json_decoder_create.restype = p
        L.dz_json_decoder_create.argtypes = [ctypes.c_int32, ctypes.c_char_p,
                                             ctypes.c_char_p, ctypes.c_char_p]
        L.dz_json_decoder_destroy.argtypes = [p]
        L.dz_json_decoder_last_error.restype = ctypes.c_char_p
        L.dz_json_decoder_last_error.argtypes = [p]
        L.dz_json_decode.argtypes = [p, p, i64]
        L.dz_json_decoder_batch.argtypes = [p, ctypes.POINTER(i64),
                                            ctypes.POINTER(p),
                                            ctypes.POINTER(p),
                                            ctypes.POINTER(p),
                                            ctypes.POINTER(p)]
        L.dz_generate_json.argtypes = [ctypes.c_int32, ctypes.c_uint64, i64,
                                       i64, i64, i64, i64, p, p, p]
        L.dz_debug_windows_for_range.restype = i64
        L.dz_debug_windows_for_range.argtypes = [i64, i64, i64, i64, p, p, i64]
        try:
            L.dz_debug_var_finalize.restype = ctypes.c_int32
            L.dz_debug_var_finalize.argtypes = [
                ctypes.c_int32, ctypes.c_uint64, ctypes.c_double,
                ctypes.POINTER(ctypes.c_double)]
        except AttributeError:  # older engine build (A/B hook)
            pass
        try:
            L.dz_debug_median_caps.restype = None
            L.dz_debug_median_caps.argtypes = [
                ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(i64)]
        except AttributeError:  # older engine build (A/B hook)
            pass
        try:
            L.dz_debug_intern_fp_bits.argtypes = [p, ctypes.c_int32]
        except AttributeError:  # older engine build (A/B hook)
            pass
        L.dz_version.restype = ctypes.c_char_p
        _lib = L
    return _lib


def _err(L, h=None):
    m = L.dz_last_error(h)
    return m.decode() if m else "unknown error"


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _value_array(vals, value_dtype):
    """The value column as the op reads it. float64 ops cast whatever they are
    given, as they always have. int64 ops take integers only: a float array
    is a TypeError, never a rounding (np.int64 of 2.0**53 + 1 is already the
    wrong number)."""
    if value_dtype != "int64":
        return np.ascontiguousarray(vals, np.float64)
    a = np.asarray(vals)
    if a.size == 0:
        return np.zeros(0, np.int64)  # an empty list has no dtype to refuse
    if a.dtype.kind not in "iu":
        raise TypeError(
            f"value_dtype='int64' op was pushed {a.dtype} values; pass an "
            "integer array (values are never rounded on the way in)")
    if a.dtype == np.uint64 and a.size and int(a.max()) > np.iinfo(np.int64).max:
        raise TypeError("uint64 values above INT64_MAX do not fit int64")
    return np.ascontiguousarray(a, np.int64)


class WindowOp:
    """Python handle over dz_window_op (one partition's stream).

    aggs entries are (op, col) or (op, col, alias). With 2-tuples only, the
    column half is ignored and every aggregate reads value_col. As soon as
    one entry is a 3-tuple, every entry's col is the batch column index it
    aggregates and alias (default: the op name) names its result column; up
    to 4 distinct columns, numbered in order of first appearance. The first
    is the primary; an aggregate on any other column reports its own mask as
    res[alias + "_valid"].

    value_dtype="int64": the (single) value column is int64. push takes an
    integer array (a float array is a TypeError), the device pushes take
    device pointers to int64 values, and poll returns min/max/sum as
    np.int64 arrays (sum wraps); avg and the variance family are computed on
    (double)v. Not available with several value columns or the median."""

    def __init__(self, length_ms, slide_ms=0, aggs=(("count", 0), ("min", 0),
                 ("max", 0), ("avg", 0)), key_kind=KEY_UTF8, n_keys_hint=1024,
                 device=0, max_open_windows=0, ts_col=0, group_col=1,
                 value_col=2, no_group=False, value_dtype="float64"):
        if value_dtype not in VALUE_DTYPES:
            raise ValueError(f"value_dtype must be one of "
                             f"{sorted(VALUE_DTYPES)}, got {value_dtype!r}")
        self._L = lib()
        self.value_dtype = value_dtype
        self.no_group = no_group
        if no_group:
            group_col = -1
            value_col = 1
        n = len(aggs)
        self._agg_arr = (DzAggDesc * n)()
        self.agg_names = []
        self._var_aggs = []  # indices whose column has its own NULL mask
        self._by_col = any(len(a) == 3 for a in aggs)
        self._dcols = []     # distinct value columns, first-appearance order
        for i, agg in enumerate(aggs):
            name, col = agg[0], agg[1]
            self._agg_arr[i].op = AGG_BY_NAME[name] if isinstance(name, str) else name
            col = int(col) if self._by_col else value_col
            if col not in self._dcols:
                self._dcols.append(col)
            if self._agg_arr[i].op in VAR_AGGS or col != self._dcols[0]:
                self._var_aggs.append(i)
            self._agg_arr[i].input_col = col
            alias = agg[2] if len(agg) == 3 else name
            self.agg_names.append(alias if isinstance(alias, str) else str(alias))
        self.n_value_cols = len(self._dcols)
        self._ts_col, self._group_col = ts_col, group_col
        d = DzWindowDesc(
            window_type=WINDOW_SLIDING if slide_ms else WINDOW_TUMBLING,
            length_ms=length_ms, slide_ms=slide_ms or 0, ts_col=ts_col,
            group_col=group_col, key_kind=key_kind,
            aggs=ctypes.cast(self._agg_arr, ctypes.POINTER(DzAggDesc)),
            n_aggs=n, n_keys_hint=n_keys_hint, device=device,
            max_open_windows=max_open_windows)
        self.key_kind = key_kind
        self._h = self._L.dz_window_op_create(ctypes.byref(d))
        if not self._h:
            raise RuntimeError(f"dz_window_op_create failed: {_err(self._L)}")
        if value_dtype != "float64":
            try:
                self.set_value_type(0, VALUE_DTYPES[value_dtype])
            except Exception:
                self.close()
                raise

    def set_value_type(self, value_col, vtype):
        """dz_window_op_set_value_type: legal only before the first push."""
        self._check(self._L.dz_window_op_set_value_type(
            self._h, value_col, vtype), "set_value_type")
        if value_col == 0:
            self.value_dtype = "int64" if vtype == VALUE_INT64 else "float64"

    def _check(self, st, what):
        if st != DZ_OK:
            raise RuntimeError(f"{what} failed: {_err(self._L, self._h)}")

    def push(self, ts_ms, keys, vals, val_valid_bitmap=None):
        """Host-batch push (the drop-in boundary). keys: np.int64 array, or a
        list of str/bytes for utf8. val_valid_bitmap: LSB-first bitmap bytes."""
        if self._by_col:
            return self._push_by_col(ts_ms, keys, vals, val_valid_bitmap)
        vals = _value_array(vals, self.value_dtype)
        ts_ms = np.ascontiguousarray(ts_ms, np.int64)
        n = len(ts_ms)
        keep = []
        if self.no_group:
            cols = (DzColumn * 2)()
            cols[0] = DzColumn(n, None, None, _np_ptr(ts_ms).value if n else None)
            bm = None
            if val_valid_bitmap is not None:
                bm = np.ascontiguousarray(val_valid_bitmap, np.uint8)
                keep.append(bm)
            cols[1] = DzColumn(n, _np_ptr(bm).value if bm is not None else None,
                               None, _np_ptr(vals).value if n else None)
            batch = DzBatch(n, 2, ctypes.cast(cols, ctypes.POINTER(DzColumn)))
            self._check(self._L.dz_window_op_push(self._h, ctypes.byref(batch)),
                        "push")
            return
        cols = (DzColumn * 3)()
        cols[0] = DzColumn(n, None, None, _np_ptr(ts_ms).value if n else None)
        if self.key_kind == KEY_UTF8:
            data = b"".join(k.encode() if isinstance(k, str) else bytes(k) for k in keys)
            offs = np.zeros(n + 1, np.int32)
            pos = 0
            for i, k in enumerate(keys):
                pos += len(k.encode() if isinstance(k, str) else bytes(k))
                offs[i + 1] = pos
            buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
            keep += [offs, buf]
            cols[1] = DzColumn(n, None, _np_ptr(offs).value, _np_ptr(buf).value)
        else:
            karr = np.ascontiguousarray(keys, np.int64)
            keep.append(karr)
            cols[1] = DzColumn(n, None, None, _np_ptr(karr).value if n else None)
        bm = None
        if val_valid_bitmap is not None:
            bm = np.ascontiguousarray(val_valid_bitmap, np.uint8)
            keep.append(bm)
        cols[2] = DzColumn(n, _np_ptr(bm).value if bm is not None else None, None,
                           _np_ptr(vals).value if n else None)
        batch = DzBatch(n, 3, ctypes.cast(cols, ctypes.POINTER(DzColumn)))
        self._check(self._L.dz_window_op_push(self._h, ctypes.byref(batch)), "push")

    def _push_by_col(self, ts_ms, keys, vals, bitmaps):
        """Host push of an op declared with (op, col, alias): the batch has
        ts at ts_col, keys at group_col and each distinct value column at its
        own index. vals / bitmaps: sequences in distinct-column order (a
        single array / bitmap is accepted for a one-column op)."""
        nv = self.n_value_cols
        if nv == 1 and not isinstance(vals, (list, tuple)):
            vals, bitmaps = [vals], [bitmaps]
        if bitmaps is None:
            bitmaps = [None] * nv
        if len(vals) != nv or len(bitmaps) != nv:
            raise ValueError(f"push needs {nv} value columns (and bitmaps), "
                             f"in distinct-column order")
        ts_ms = np.ascontiguousarray(ts_ms, np.int64)
        n = len(ts_ms)
        used = [self._ts_col] + self._dcols
        if not self.no_group:
            used.append(self._group_col)
        if len(set(used)) != len(used) or min(used) < 0:
            raise ValueError("ts, group and value column indices must be "
                             "distinct and non-negative")
        ncols = max(used) + 1
        cols = (DzColumn * ncols)()
        keep = [ts_ms]
        cols[self._ts_col] = DzColumn(n, None, None,
                                      _np_ptr(ts_ms).value if n else None)
        if self.no_group:
            pass
        elif self.key_kind == KEY_UTF8:
            enc = [k.encode() if isinstance(k, str) else bytes(k) for k in keys]
            offs = np.zeros(n + 1, np.int32)
            np.cumsum([len(k) for k in enc], out=offs[1:])
            data = b"".join(enc)
            buf = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
            keep += [offs, buf]
            cols[self._group_col] = DzColumn(n, None, _np_ptr(offs).value,
                                             _np_ptr(buf).value)
        else:
            karr = np.ascontiguousarray(keys, np.int64)
            keep.append(karr)
            cols[self._group_col] = DzColumn(
                n, None, None, _np_ptr(karr).value if n else None)
        for c, v, bm in zip(self._dcols, vals, bitmaps):
            v = _value_array(v, self.value_dtype)
            if len(v) != n:
                raise ValueError("value column length differs from ts")
            keep.append(v)
            if bm is not None:
                bm = np.ascontiguousarray(bm, np.uint8)
                if len(bm) < (n + 7) // 8:
                    raise ValueError("validity bitmap shorter than the batch")
                keep.append(bm)
            cols[c] = DzColumn(n, _np_ptr(bm).value if bm is not None else None,
                               None, _np_ptr(v).value if n else None)
        batch = DzBatch(n, ncols, ctypes.cast(cols, ctypes.POINTER(DzColumn)))
        self._check(self._L.dz_window_op_push(self._h, ctypes.byref(batch)),
                    "push")

    def set_extra_values(self, n, d_vals_list, d_validity_list=None):
        """Extra value columns (distinct columns 1.., in order) of the NEXT
        device push of any kind: device pointers to f64 columns and, per
        column, an LSB-first validity bitmap or None. Borrowed until the call
        after that push."""
        def as_p(x):
            if x is None:
                return None
            return x.value if isinstance(x, ctypes.c_void_p) else int(x)
        k = len(d_vals_list)
        va = (ctypes.c_void_p * max(k, 1))(*[as_p(x) for x in d_vals_list])
        ba = None
        if d_validity_list is not None:
            if len(d_validity_list) != k:
                raise ValueError("one validity entry per extra column")
            ba = (ctypes.c_void_p * max(k, 1))(
                *[as_p(x) for x in d_validity_list])
        if k != self.n_value_cols - 1 and self.n_value_cols > 1:
            raise ValueError(f"op has {self.n_value_cols - 1} extra columns, "
                             f"got {k}")
        self._check(self._L.dz_window_op_set_extra_values(
            self._h, n, va, ba), "set_extra_values")

    def push_device(self, n, d_ts, d_kid32, d_vals, borrowed=False):
        """borrowed=True: zero-copy — the op reads these buffers until the
        NEXT call on the op; they must stay valid and unmodified until then."""
        fn = (self._L.dz_window_op_push_device_borrowed if borrowed
              else self._L.dz_window_op_push_device)
        self._check(fn(self._h, n, d_ts, d_kid32, d_vals), "push_device")

    def push_device_utf8(self, n, d_ts, d_key_offsets, d_key_data, d_vals):
        """Raw utf8 keys interned ON DEVICE (GroupValues::intern analog).
        Borrowed semantics: all four buffers stay valid until the next call
        on the op. Requires key_kind KEY_UTF8."""
        self._check(self._L.dz_window_op_push_device_utf8(
            self._h, n, d_ts, d_key_offsets, d_key_data, d_vals),
            "push_device_utf8")

    def push_device_i64(self, n, d_ts, d_keys, d_vals):
        """Arbitrary int64 keys interned ON DEVICE; every int64 value is a
        legal key. Borrowed semantics: the three buffers stay valid and
        unmodified until the next call on the op. Requires key_kind
        KEY_INT64 and an 8-byte-aligned d_keys."""
        self._check(self._L.dz_window_op_push_device_i64(
            self._h, n, d_ts, d_keys, d_vals), "push_device_i64")

    def debug_intern_fp_bits(self, bits):
        """Test hook: mask intern fingerprints (utf8) or key hashes (int64)
        to `bits` bits: forces collisions / long probe chains. Only before
        the first push_device_utf8 / push_device_i64."""
        self._check(self._L.dz_debug_intern_fp_bits(self._h, bits),
                    "debug_intern_fp_bits")

    def poll(self, copy=True):
        """Returns a dict of numpy arrays for one emitted batch, or None.
        copy=False returns zero-copy views of the op-owned buffers (valid
        until the next poll on this handle — the C contract's ownership
        rule); copy=True materialises."""
        outp = ctypes.POINTER(DzOutBatch)()
        self._check(self._L.dz_window_op_poll(self._h, ctypes.byref(outp)), "poll")
        if not outp:
            return None

        def mk(p, n, ctype):
            if not n:
                return np.zeros(0, np.int64 if ctype == ctypes.c_int64 else np.float64)
            a = np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), (n,))
            return a.copy() if copy else a
        ob = outp.contents
        n = ob.n_rows
        res = {"n_rows": n}
        if self.no_group:
            pass  # global aggregate: no group column in the output schema
        elif self.key_kind == KEY_UTF8:
            if copy:
                offs = (np.ctypeslib.as_array(ob.key_offsets, (n + 1,)).copy()
                        if n else np.zeros(1, np.int32))
                total = int(offs[-1]) if n else 0
                data = ctypes.string_at(ob.key_data, total) if total else b""
                res["key"] = [data[offs[i]:offs[i + 1]].decode()
                              for i in range(n)]
            else:
                # zero-copy: raw Arrow views (decoding every key into Python
                # strings costs more than the whole GPU step)
                offs = (np.ctypeslib.as_array(ob.key_offsets, (n + 1,))
                        if n else np.zeros(1, np.int32))
                total = int(offs[-1]) if n else 0
                res["key_offsets"] = offs
                res["key_data"] = (np.ctypeslib.as_array(
                    ctypes.cast(ob.key_data, ctypes.POINTER(ctypes.c_uint8)),
                    (total,)) if total else np.zeros(0, np.uint8))
        else:
            res["key"] = mk(ob.key_i64, n, ctypes.c_int64)
        for i, name in enumerate(self.agg_names):
            pt = ob.agg_cols[i]
            if self._agg_arr[i].op == AGG_COUNT or (
                    self.value_dtype == "int64"
                    and self._agg_arr[i].op in INT_AGGS):
                res[name] = mk(pt, n, ctypes.c_int64)
            else:
                res[name] = mk(pt, n, ctypes.c_double)
        if n:
            v = np.ctypeslib.as_array(ob.agg_valid, (n,))
            res["valid"] = v.copy() if copy else v
        else:
            res["valid"] = np.zeros(0, np.uint8)
        for i in self._var_aggs:
            # variance family: own NULL rule (e.g. var_samp of a one-row
            # group); aggregates on an extra value column: that column's
            # NULLs. Both reported per aggregate
            name = self.agg_names[i]
            pm = ob.agg_valid_cols[i] if n and ob.agg_valid_cols else None
            if pm:
                v = np.ctypeslib.as_array(pm, (n,))
                res[name + "_valid"] = v.copy() if copy else v
            elif n:
                raise RuntimeError(
                    f"engine returned no validity mask for {name!r}")
            else:
                res[name + "_valid"] = np.zeros(0, np.uint8)
        res["window_start"] = mk(ob.window_start_ms, n, ctypes.c_int64)
        res["window_end"] = mk(ob.window_end_ms, n, ctypes.c_int64)
        return res

    def drain(self):
        """Wait until every triggered window's batch is pollable (emission is
        pipelined on a worker thread)."""
        self._check(self._L.dz_window_op_drain(self._h), "drain")

    def poll_all(self, drain=True, copy=True):
        """Collect every pollable batch as owned arrays. The C ownership
        contract invalidates a batch's buffers at the next poll on the
        handle, so a LIST of live views is impossible: poll_all always
        materialises (the copy parameter is kept for signature
        compatibility but no longer returns aliased views). Zero-copy
        consumption goes through poll(copy=False) or poll_iter(), reading
        each batch before advancing."""
        del copy
        if drain:
            self.drain()
        out = []
        while True:
            b = self.poll(copy=True)
            if b is None:
                return out
            out.append(b)

    def poll_iter(self, copy=False):
        """Generator form of poll_all: yields one batch at a time; with
        copy=False the yielded views are valid only until the next
        iteration (exactly the single-poll contract)."""
        while True:
            b = self.poll(copy=copy)
            if b is None:
                return
            yield b

    def finish(self):
        self._check(self._L.dz_window_op_finish(self._h), "finish")

    def set_filter(self, agg_name_or_idx, cmp, literal):
        idx = (self.agg_names.index(agg_name_or_idx)
               if isinstance(agg_name_or_idx, str) else agg_name_or_idx)
        self._check(self._L.dz_window_op_set_filter(
            self._h, idx, CMP[cmp] if isinstance(cmp, str) else cmp,
            float(literal)), "set_filter")

    def advance_watermark(self, wm_ms):
        self._check(self._L.dz_window_op_advance_watermark(self._h, wm_ms),
                    "advance_watermark")

    @property
    def watermark(self):
        return self._L.dz_window_op_watermark(self._h)

    @property
    def open_windows(self):
        return self._L.dz_window_op_open_windows(self._h)

    def kernel_stats(self):
        # 32 slots: the stat map currently holds up to 21 entries (6 device
        # kernels + 10 host timers + 5 emission route counters; a median op
        # adds 5 kernels + 1 host timer = 27) — headroom
        # so a new timer can never silently push the roofline's dominant
        # kernel out of the window
        arr = (DzKernelStat * 32)()
        nout = ctypes.c_int32()
        self._check(self._L.dz_window_op_kernel_stats(self._h, arr, 32,
                                                      ctypes.byref(nout)), "stats")
        return {arr[i].name.decode(): {
            "launches": arr[i].launches, "total_ms": arr[i].total_ms,
            "bytes_per_launch_alg": arr[i].bytes_per_launch_alg,
        } for i in range(nout.value)}

    def close(self):
        if getattr(self, "_h", None):
            self._L.dz_window_op_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JsonDecoder:
    """Device JSON decode (from_topic's decode stage): newline-delimited
    records -> (ts, utf8 key column, value) device columns shaped for
    WindowOp.push_device_utf8. See include/denormalized_amd.h for the
    documented subset."""

    def __init__(self, device=0, ts_field="occurred_at_ms",
                 key_field="sensor_name", val_field="reading"):
        self._L = lib()
        self._h = self._L.dz_json_decoder_create(
            device, ts_field.encode(), key_field.encode(), val_field.encode())
        if not self._h:
            m = self._L.dz_json_decoder_last_error(None)
            raise RuntimeError(f"dz_json_decoder_create failed: "
                               f"{m.decode() if m else 'unknown'}")

    def _check(self, st, what):
        if st != DZ_OK:
            m = self._L.dz_json_decoder_last_error(self._h)
            raise RuntimeError(f"{what} failed: "
                               f"{m.decode() if m else 'unknown'}")

    def decode(self, d_bytes, n_bytes):
        self._check(self._L.dz_json_decode(self._h, d_bytes, n_bytes),
                    "json decode")
        return self.batch()

    def batch(self):
        """(n, d_ts, d_key_offsets, d_key_data, d_vals) of the LAST decode
        — device pointers, valid until the second-next decode."""
        n = ctypes.c_int64()
        ts = ctypes.c_void_p()
        ko = ctypes.c_void_p()
        kd = ctypes.c_void_p()
        v = ctypes.c_void_p()
        self._check(self._L.dz_json_decoder_batch(
            self._h, ctypes.byref(n), ctypes.byref(ts), ctypes.byref(ko),
            ctypes.byref(kd), ctypes.byref(v)), "batch")
        return n.value, ts, ko, kd, v

    def close(self):
        if getattr(self, "_h", None):
            self._L.dz_json_decoder_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class JoinOp:
    """Stream inner equi-join on trip_id (BASELINE cfg5): build side
    (trip_id -> driver_id), probe side (ts, trip_id, value). Matches are
    device-resident columns shaped for WindowOp.push_device(borrowed=True)
    — see include/denormalized_amd.h for the emission discipline."""

    def __init__(self, device=0, n_trips_hint=1 << 20):
        self._L = lib()
        self._h = self._L.dz_join_op_create(device, n_trips_hint)
        if not self._h:
            m = self._L.dz_join_last_error(None)
            raise RuntimeError(f"dz_join_op_create failed: "
                               f"{m.decode() if m else 'unknown'}")

    def _check(self, st, what):
        if st != DZ_OK:
            m = self._L.dz_join_last_error(self._h)
            raise RuntimeError(f"{what} failed: "
                               f"{m.decode() if m else 'unknown'}")

    def push_build(self, n, d_trips, d_drivers):
        self._check(self._L.dz_join_op_push_build(self._h, n, d_trips,
                                                  d_drivers), "push_build")

    def push_probe(self, n, d_ts, d_trips, d_vals):
        self._check(self._L.dz_join_op_push_probe(self._h, n, d_ts, d_trips,
                                                  d_vals), "push_probe")

    def matches(self):
        """(n, d_ts, d_kid32, d_vals) of the LAST push (n == 0: no matches).
        The columns of a push with matches stay valid until the push after
        the next push with matches; zero-match pushes recycle nothing."""
        n = ctypes.c_int64()
        ts = ctypes.c_void_p()
        kid = ctypes.c_void_p()
        val = ctypes.c_void_p()
        self._check(self._L.dz_join_op_matches(
            self._h, ctypes.byref(n), ctypes.byref(ts), ctypes.byref(kid),
            ctypes.byref(val)), "matches")
        return n.value, ts, kid, val

    @property
    def unmatched(self):
        return self._L.dz_join_op_unmatched(self._h)

    def close(self):
        if getattr(self, "_h", None):
            self._L.dz_join_op_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceArray:
    """Raw device allocation (no torch types cross the C ABI)."""

    def __init__(self, device, nbytes):
        self._L = lib()
        self.device = device
        self.nbytes = nbytes
        p = ctypes.c_void_p()
        if self._L.dz_device_malloc(device, nbytes, ctypes.byref(p)) != DZ_OK:
            raise RuntimeError("device malloc failed")
        self.ptr = p

    def to_host(self, dtype, count):
        out = np.empty(count, dtype)
        if self._L.dz_memcpy_d2h(_np_ptr(out), self.ptr, out.nbytes) != DZ_OK:
            raise RuntimeError("d2h failed")
        return out

    def from_host(self, arr):
        arr = np.ascontiguousarray(arr)
        if self._L.dz_memcpy_h2d(self.ptr, _np_ptr(arr), arr.nbytes) != DZ_OK:
            raise RuntimeError("h2d failed")

    def free(self):
        if getattr(self, "ptr", None):
            self._L.dz_device_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def generate(device, seed, t0_ms, start_row, n_rows, n_keys, rows_per_ms,
             d_ts=None, d_keys=None, d_kid32=None, d_vals=None):
    L = lib()
    if L.dz_generate(device, seed, t0_ms, start_row, n_rows, n_keys, rows_per_ms,
                     d_ts, d_keys, d_kid32, d_vals) != DZ_OK:
        raise RuntimeError(f"dz_generate failed: {_err(L)}")


def generate_json(device, seed, t0_ms, start_row, n_rows, n_keys,
                  rows_per_ms, d_lens=None, d_offsets=None, d_data=None):
    L = lib()
    if L.dz_generate_json(device, seed, t0_ms, start_row, n_rows, n_keys,
                          rows_per_ms, d_lens, d_offsets, d_data) != DZ_OK:
        raise RuntimeError(f"dz_generate_json failed: {_err(L)}")


def generate_utf8(device, seed, start_row, n_rows, n_keys, d_lens=None,
                  d_offsets=None, d_key_data=None):
    """Synthetic "sensor_{k}" key column: lens pass (host cumsums into
    offsets) and/or fill pass."""
    L = lib()
    if L.dz_generate_utf8(device, seed, start_row, n_rows, n_keys, d_lens,
                          d_offsets, d_key_data) != DZ_OK:
        raise RuntimeError(f"dz_generate_utf8 failed: {_err(L)}")


def median_caps():
    """(lds_vals, log_min_entries) of the median kernels: the largest group
    selected in LDS and a value log's first allocation (test hook)."""
    a, b = ctypes.c_int32(), ctypes.c_int64()
    lib().dz_debug_median_caps(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def synchronize(device=0):
    L = lib()
    if L.dz_device_synchronize(device) != DZ_OK:
        raise RuntimeError("device synchronize failed")
