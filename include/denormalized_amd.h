/* denormalized_amd.h — C ABI of the MI355X-native streaming windowed-aggregate
 * operator (the drop-in replacement for Denormalized's hot path).
 *
 * Boundary contract. Each entry point cites the reference
 * interface it replaces (file:line into /root/reference, the public
 * probably-nothing-labs/denormalized tree @ 2024-12-18). The reference host is
 * Rust; a maintainer binds this library with a plain `extern "C"` FFI block —
 * see INTEGRATION.md for the Rust-side stub. No GPU-runtime types cross this
 * boundary: plain pointers and sizes only.
 */
#ifndef DENORMALIZED_AMD_H
#define DENORMALIZED_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ */
/* Status and descriptors                                              */
/* ------------------------------------------------------------------ */

typedef enum dz_status {
    DZ_OK = 0,
    DZ_ERR = 1,          /* inspect dz_last_error() */
} dz_status;

/* PhysicalStreamingWindowType (crates/core/src/physical_plan/continuous/
 * streaming_window.rs; Session is todo!() in the reference,
 * streaming_window.rs:1062). */
typedef enum dz_window_type {
    DZ_WINDOW_TUMBLING = 0,   /* Tumbling(length) */
    DZ_WINDOW_SLIDING  = 1,   /* Sliding(length, slide) */
} dz_window_type;

/* The aggregate set of the hot path (simple_aggregation.rs:46-52:
 * count/min/max/avg; sum is the avg partial and is also exposed), plus the
 * variance family of the reference's Python example
 * (py-denormalized/python/examples/stream_aggregate.py:52-53). */
typedef enum dz_agg_op {
    DZ_AGG_COUNT = 0,
    DZ_AGG_MIN   = 1,
    DZ_AGG_MAX   = 2,
    DZ_AGG_SUM   = 3,
    DZ_AGG_AVG   = 4,
    /* Welford variance family (the reference's stddev/stddev_pop/var_samp/
     * var_pop, py-denormalized/python/denormalized/datafusion/functions.py):
     * per-group state (count, mean, m2), updated per valid row in row order.
     * NULL when count == 0 (pop) or count <= 1 (samp) — reported through
     * dz_out_batch.agg_valid_cols. */
    DZ_AGG_VAR_SAMP    = 5,
    DZ_AGG_VAR_POP     = 6,
    DZ_AGG_STDDEV_SAMP = 7,
    DZ_AGG_STDDEV_POP  = 8,
    /* Exact median (the reference's median, functions.py:1768; the same
     * example declares it, stream_aggregate.py:52). Codes 9..15 are not
     * assigned and are refused. Per (window, key) group: the column's valid
     * values sorted by IEEE total order (-NaN < -inf < ... < -0.0 < +0.0 <
     * ... < +inf < +NaN; sort key = bits ^ (sign ? ~0 : 1 << 63)); n == 0:
     * NULL; n odd: v[n/2]; n even: (v[n/2-1] + v[n/2]) / 2.0 — one f64 add
     * and one f64 divide, each rounded on its own, so an overflow to +-inf
     * and inf + -inf = NaN come out as they are. Row order does not matter.
     * An f64 column whose NULL-ness is agg_valid's (its agg_valid_cols entry
     * is NULL). A median op may also declare count/min/max/sum/avg and the
     * variance family on the same column; dz_window_op_create refuses it
     * with more than one distinct value column. Median ops build every
     * emitted batch on the host, at every key count.
     * MEMORY: every valid row is kept, per window it belongs to (a sliding
     * row: every window containing it), until that window closes: 12 B per
     * entry of capacity (f64 value + u32 key id); a window's log starts at
     * 4096 entries, grows by 1.5x or to the exact need, whichever is larger,
     * keeps its capacity when the slot is reused, and holds at most 2^31 - 1
     * entries. A failed allocation (or that limit) is DZ_ERR with a message
     * from the push — or from the next call into the op, for the pipelined
     * device pushes — and loses that batch; the op stays usable for poll
     * and destroy. */
    DZ_AGG_MEDIAN = 16,
} dz_agg_op;

typedef enum dz_key_kind {
    DZ_KEY_UTF8        = 0,  /* dictionary-encoded host-side, first-seen ids */
    DZ_KEY_INT64       = 1,  /* arbitrary int64 keys, host dictionary        */
    DZ_KEY_DENSE_INT64 = 2,  /* keys are already dense ids in [0, n_keys)    */
} dz_key_kind;

typedef struct dz_agg_desc {
    dz_agg_op op;
    int32_t input_col;        /* column index in the pushed batch (f64, or
                               * int64 after dz_window_op_set_value_type) */
} dz_agg_desc;

/* The type of a value column (dz_window_op_set_value_type). */
typedef enum dz_value_type {
    DZ_VALUE_F64   = 0,       /* the default */
    DZ_VALUE_INT64 = 1,
} dz_value_type;

/* Construction parameters. Mirrors what the planner hands StreamingWindowExec:
 * (mode, group-by, aggregate exprs, window type) —
 * crates/core/src/planner/streaming_window.rs:133-165 and
 * StreamingWindowExec::new (physical_plan/continuous/streaming_window.rs:201+).
 * This build supports the hot path's shape: one group column, mode Single
 * (grouped), aggregates over up to DZ_MAX_VALUE_COLS distinct f64 value
 * columns (the reference aggregates several columns in one window:
 * examples/examples/kafka_rideshare.rs:73-75).
 *
 * Several value columns. The distinct input_col values are numbered in order
 * of first appearance in aggs: column 0 (aggs[0].input_col) is the primary,
 * columns 1..X the extras. Every column has its own validity bitmap, so
 * count(c) and the NULL-ness of min/max/sum/avg(c) are per column; a group
 * exists as soon as it has a row, whatever is NULL in it. Each column's
 * accumulators see that column's valid rows in row order (bit-exact f64 sum).
 * dz_window_op_create returns NULL for more than DZ_MAX_VALUE_COLS distinct
 * columns, and for a variance-family aggregate together with more than one
 * distinct column: the variance family stays single-column in this version. */
#define DZ_MAX_VALUE_COLS 4
typedef struct dz_window_desc {
    dz_window_type window_type;
    int64_t length_ms;
    int64_t slide_ms;          /* ignored for tumbling */
    int32_t ts_col;            /* Timestamp(ms) column index (the reference's
                                * _streaming_internal_metadata.canonical_timestamp,
                                * crates/common/src/lib.rs:5) */
    int32_t group_col;
    dz_key_kind key_kind;
    const dz_agg_desc* aggs;
    int32_t n_aggs;
    int64_t n_keys_hint;       /* initial key-capacity; grows as needed */
    int32_t device;            /* HIP device ordinal */
    int32_t max_open_windows;  /* 0 => 64 */
} dz_window_desc;

/* ------------------------------------------------------------------ */
/* Batches — Arrow C-data-interface-style buffers                      */
/* (the reference operator consumes/produces Arrow RecordBatches:      */
/*  grouped_window_agg_stream.rs:548-605; caller owns input, the op    */
/*  copies what it keeps; the op owns an output batch until the next   */
/*  poll on the same handle)                                           */
/* ------------------------------------------------------------------ */

typedef struct dz_column {
    int64_t len;
    const uint8_t* validity;   /* Arrow validity bitmap (LSB-first), NULL = all valid */
    const int32_t* offsets;    /* utf8 columns only: len+1 entries */
    const void* data;          /* i64 / f64 values, or utf8 bytes */
} dz_column;

typedef struct dz_batch {
    int64_t n_rows;
    int32_t n_cols;
    const dz_column* cols;
} dz_batch;

/* Emitted window batch. Column order mirrors the reference output schema:
 * group key, aggregates in declaration order, then window_start_time and
 * window_end_time (Timestamp(ms)) — streaming_window.rs:1096-1134 +
 * continuous/mod.rs:42-62. Rows are groups in insertion (first-seen) order
 * per window, windows in ascending start order (GroupValues emits insertion
 * order; trigger iterates the BTreeMap: grouped_window_agg_stream.rs:220-253). */
typedef struct dz_out_batch {
    int64_t n_rows;
    /* group key column (one of): */
    const int64_t* key_i64;        /* key kinds INT64 / DENSE_INT64 */
    const int32_t* key_offsets;    /* key kind UTF8 */
    const char*    key_data;
    /* aggregate columns, one per dz_window_desc.aggs entry:
     * COUNT -> int64; MIN/MAX/SUM of an int64 column -> int64; others ->
     * double */
    const void* const* agg_cols;
    const uint8_t* agg_valid;      /* byte mask (1=valid) for min/max/sum/avg
                                    * (all-null groups); count is never null */
    const int64_t* window_start_ms;
    const int64_t* window_end_ms;
    /* per-aggregate byte masks, n_aggs entries (appended field; everything
     * above keeps its offset and meaning). Entry a is the mask of aggregate
     * a; a NULL entry means that aggregate follows agg_valid. The variance
     * family has its own NULL rule (var_samp of a one-row group is NULL
     * while its min is valid), so its entries are non-NULL. The pointer
     * itself may be NULL for ops that declare no variance aggregate.
     * Multi-column ops: agg_valid is the PRIMARY column's mask; every
     * aggregate on an extra column has a non-NULL entry here (1 while that
     * column has a valid row in the group; all 1 for count, which is never
     * NULL), entries of primary-column aggregates stay NULL. */
    const uint8_t* const* agg_valid_cols;
} dz_out_batch;

/* ------------------------------------------------------------------ */
/* Operator lifecycle                                                  */
/* ------------------------------------------------------------------ */

typedef struct dz_window_op dz_window_op;

/* ExecutionPlan construction + execute(partition) →
 * GroupedWindowAggStream::new (streaming_window.rs:421-482,
 * grouped_window_agg_stream.rs:111-214). One handle = one partition's
 * stream; single-consumer. Returns NULL on error (see dz_last_error(NULL));
 * an aggregate op code outside dz_agg_op is such an error. */
dz_window_op* dz_window_op_create(const dz_window_desc* desc);

/* Declare the type of a value column; the default is DZ_VALUE_F64.
 * value_col is the ordinal of a distinct value column in first-appearance
 * order; only 0 is accepted in this version. After DZ_VALUE_INT64 every push
 * path reads the value buffer as const int64_t*: dz_window_op_push through
 * cols[input_col].data, and the four device pushes through their d_vals
 * argument, which keeps its const double* type — the caller casts the
 * pointer. Validity bitmaps work as before. Per (window, key) group, over the
 * column's valid rows (DataFusion aggregates Int64 on the column's own type:
 * min/max/sum of Int64 yield Int64; avg and the variance family cast each
 * value to Float64 first):
 *   count              unchanged;
 *   min, max           signed int64 compare; the agg_cols entry is
 *                      const int64_t*;
 *   sum                int64 two's-complement wrapping add (add_wrapping);
 *                      the agg_cols entry is const int64_t*;
 *   avg                the f64 sum of (double)v taken in row order, divided
 *                      by (double)count — bit-exact like the f64 sum;
 *   var_*, stddev_*    the Welford step on (double)v, with the NULL rules and
 *                      per-aggregate masks of the f64 column.
 * NULL-ness of min/max/sum/avg is agg_valid's, as for f64. A filter
 * (dz_window_op_set_filter) on an int64 min/max/sum compares (double)value
 * against the literal, which is DataFusion's Int64-vs-Float64 coercion.
 * Int64 ops build every emitted batch on the host, at every key count.
 * Global (no GROUP BY) ops take the same call.
 * Legal only before the op's first push of any kind. Int64 stays single-column
 * and without the median in this version (as the variance family stayed
 * single-column when it arrived). DZ_ERR with one message per cause, the op
 * left as it was and usable, for: a call after a push; an unknown type;
 * value_col != 0; DZ_VALUE_INT64 on an op with more than one distinct value
 * column; DZ_VALUE_INT64 on an op that declares DZ_AGG_MEDIAN. DZ_VALUE_F64
 * on a fresh op changes nothing and returns DZ_OK. */
dz_status dz_window_op_set_value_type(dz_window_op* op, int32_t value_col,
                                      dz_value_type t);

/* One input batch == one poll of the input stream
 * (poll_next_inner: grouped_window_agg_stream.rs:326-420): computes the batch
 * watermark, ensures window frames, routes + aggregates rows, advances the
 * shared watermark, triggers closed windows. Each aggregate reads its values
 * and its validity bitmap from batch->cols[input_col]; the data is int64_t
 * on an op set to DZ_VALUE_INT64. */
dz_status dz_window_op_push(dz_window_op* op, const dz_batch* batch);

/* Extra value columns (distinct input columns 1..X, in order of first
 * appearance in aggs) for the NEXT device push of any kind. d_validity may be
 * NULL, and any entry may be NULL (all valid); bitmaps are Arrow LSB-first.
 * Borrowed: columns and bitmaps stay valid and unmodified until the call
 * AFTER that push, also when the push itself is the staging variant.
 * The attachment is consumed by one push (a refused one included). DZ_ERR
 * with a message, the op left usable, when this is called on a single-column
 * op, when a device push on a multi-column op was not preceded by it, and
 * when its n_rows differs from the push's n_rows (the last two are reported
 * by the push). The primary column of a device push has no validity bitmap.
 * Multi-column ops build every emitted batch on the host (as the variance
 * family does), at every key count. */
dz_status dz_window_op_set_extra_values(dz_window_op* op, int64_t n_rows,
                                        const double* const* d_vals,
                                        const uint8_t* const* d_validity);

/* Device-resident push: same results as dz_window_op_push but the three
 * buffers already live in the op's device HBM (keys as dense int32 ids).
 * This is the bench's timed entry (inputs resident per measurement contract);
 * the host-buffer path above is the reference-shaped boundary.
 * Pipelined: the call stages the inputs (they may be freed once it returns)
 * and enqueues the batch's reduction, then returns; routing/aggregation and
 * any window closes complete at the NEXT call into the op (push/poll/
 * advance_watermark/finish/destroy all flush — poll opportunistically, the
 * rest unconditionally). Emitted batches and the local watermark may
 * therefore lag one device-pushed batch; results are identical.
 * On an op set to DZ_VALUE_INT64, d_vals points at int64_t values (cast). */
dz_status dz_window_op_push_device(dz_window_op* op, int64_t n_rows,
                                   const int64_t* d_ts_ms,
                                   const int32_t* d_key_ids,
                                   const double* d_vals);

/* Zero-copy variant of dz_window_op_push_device: the op reads the caller's
 * device buffers directly instead of staging a copy, so they must remain
 * valid AND unmodified until the NEXT call into the op (when the deferred
 * phase consumes them). Use when the caller owns a resident stream buffer
 * (the bench; an FFI caller holding the RecordBatch across its poll-loop
 * iteration); use the staging variant above when buffer lifetime past the
 * call cannot be guaranteed.
 * On an op set to DZ_VALUE_INT64, d_vals points at int64_t values (cast). */
dz_status dz_window_op_push_device_borrowed(dz_window_op* op, int64_t n_rows,
                                            const int64_t* d_ts_ms,
                                            const int32_t* d_key_ids,
                                            const double* d_vals);

/* Device-resident push with RAW UTF8 KEYS: the per-row string interning the
 * reference pays inside GroupValues::intern (grouped_window_agg_stream.rs:512)
 * runs ON DEVICE (open-address fingerprint table + device string pool), so
 * key materialization is inside the measured path. Borrowed semantics: the
 * offsets/data/ts/vals buffers stay valid and unmodified until the NEXT call
 * into the op. Requires key_kind DZ_KEY_UTF8. Key capacity is sized from
 * n_keys_hint at create (table 4x hint, pool 64 B/key average) and growth
 * past it fails loudly — size the hint for the stream's cardinality.
 * On an op set to DZ_VALUE_INT64, d_vals points at int64_t values (cast). */
dz_status dz_window_op_push_device_utf8(dz_window_op* op, int64_t n_rows,
                                        const int64_t* d_ts_ms,
                                        const int32_t* d_key_offsets,
                                        const char* d_key_data,
                                        const double* d_vals);

/* Device-resident push with ARBITRARY INT64 KEYS (sparse ids, hashes,
 * negative ids): the keys are interned ON DEVICE into dense ids, inside the
 * measured path, and emitted as the original int64 values. Groups exactly as
 * dz_window_op_push does on a DZ_KEY_INT64 op: every value from INT64_MIN to
 * INT64_MAX is a legal key, none is reserved. Borrowed semantics: the
 * ts/keys/vals buffers stay valid and unmodified until the NEXT call into
 * the op. Requires key_kind DZ_KEY_INT64 and an 8-byte-aligned d_keys; an op
 * takes either host pushes or device i64 pushes, never both. Key capacity is
 * sized from n_keys_hint at create (table: the power of two >= 4x hint, at
 * least 65,536 slots; distinct keys: half the table) and growth past it
 * fails loudly — dz_window_op_finish and dz_window_op_kernel_stats return
 * DZ_ERR — so size the hint for the stream's cardinality.
 * On an op set to DZ_VALUE_INT64, d_vals points at int64_t values (cast). */
dz_status dz_window_op_push_device_i64(dz_window_op* op, int64_t n_rows,
                                       const int64_t* d_ts_ms,
                                       const int64_t* d_keys,
                                       const double* d_vals);

/* Retrieve emitted closed windows (the stream's output RecordBatch,
 * trigger_windows :220-253). *out = NULL when nothing is pending.
 * The returned batch stays valid until the next poll/destroy. */
dz_status dz_window_op_poll(dz_window_op* op, const dz_out_batch** out);

/* Close every remaining open window (extension for finite streams; the
 * reference stream is unbounded and only closes on watermark advance). */
dz_status dz_window_op_finish(dz_window_op* op);

/* Emission is pipelined off the push path (a worker thread builds output
 * batches while later pushes compute). Blocks until every window already
 * triggered is available to poll — the synchronous-poll behaviour of the
 * reference stream when a consumer needs it. finish() implies drain. */
dz_status dz_window_op_drain(dz_window_op* op);

void dz_window_op_destroy(dz_window_op* op);

/* DataFusionError-by-value analog (crates/common/src/error/mod.rs:13-44). */
const char* dz_last_error(dz_window_op* op);

/* ------------------------------------------------------------------ */
/* Watermark sharing (the Arc<Mutex<watermark>> shared across partitions:
 * streaming_window.rs:210, grouped_window_agg_stream.rs:255-266). In the
 * multi-GPU plan each shard merges the global watermark (e.g. an RCCL/gloo
 * all-reduce MAX) and injects it here before polling. */
dz_status dz_window_op_advance_watermark(dz_window_op* op, int64_t wm_ms);
int64_t dz_window_op_watermark(dz_window_op* op);   /* INT64_MIN if unset */
int64_t dz_window_op_open_windows(dz_window_op* op);

/* ------------------------------------------------------------------ */
/* Filter pushdown: the pipeline's `.filter(col("max") > lit(113))`
 * (datastream.rs:94-105) evaluates over the window's output; pushing it
 * into the operator's emission keeps the boundary drop-in (output batches
 * are already filtered). cmp: 0 '<', 1 '<=', 2 '>', 3 '>=', 4 '==', 5 '!='.
 * agg_idx indexes dz_window_desc.aggs. NULL aggregate values never pass
 * (for the variance family: the finalised value, under its own NULL rule;
 * for an aggregate on an extra value column: that column's own NULL-ness;
 * for the median: the finalised value, NULL for a group without a valid
 * row; for min/max/sum of an int64 column: (double)value is compared, as
 * DataFusion coerces Int64 against a Float64 literal). */
dz_status dz_window_op_set_filter(dz_window_op* op, int32_t agg_idx,
                                  int32_t cmp, double literal);

/* ------------------------------------------------------------------ */
/* Stream join (BASELINE cfg5): inner equi-join on trip_id feeding the
 * windowed group-by. The reference lowers DataStream::join to DataFusion's
 * inner hash join (crates/core/src/datastream.rs:126-175; its only join
 * example composes two streams, examples/examples/stream_join.rs). The
 * streaming discipline (restated in oracle/oracle.c orc_join_*): build side
 * = (trip_id -> driver_id) dimension table (later duplicates overwrite;
 * the winner among duplicates WITHIN one build batch is unspecified); each
 * probe batch emits its matching rows IN ROW ORDER; unmatched rows buffer
 * in row order and re-emit (original order) when their build row arrives;
 * rows never matched are dropped (inner join). Outputs are device-resident
 * (ts, driver id as a dense int32 key, value) columns shaped for a
 * zero-copy dz_window_op_push_device_borrowed.
 *
 * Capacity: the table has max(65536, pow2 >= 4 * n_trips_hint) slots (at most
 * 2^28) and holds at most HALF of them, so at least 2 * n_trips_hint and
 * never fewer than 32768 distinct trips. A build push is validated before it
 * writes anything and is refused with DZ_ERR, one message per cause, when
 *  - trips held + rows whose trip is new would exceed that capacity (rows
 *    repeating a new trip within the batch each count, so a batch with such
 *    duplicates can be refused slightly early; updates of trips already held
 *    always pass);
 *  - a trip id equals INT64_MIN, which is reserved (the empty-slot mark);
 *  - a driver id lies outside [0, INT32_MAX] (the output kid column is int32).
 * A refused push leaves the table, the unmatched buffer and the last matches
 * exactly as they were; the handle stays usable. A PROBE row whose trip id is
 * INT64_MIN is legal and never matches: it buffers like any absent trip. */

typedef struct dz_join_op dz_join_op;

dz_join_op* dz_join_op_create(int32_t device, int64_t n_trips_hint);
void dz_join_op_destroy(dz_join_op* op);
const char* dz_join_last_error(dz_join_op* op);

/* Device-resident build push (trip_id -> driver_id rows). Also re-probes
 * the unmatched buffer: newly matched rows become this call's matches. */
dz_status dz_join_op_push_build(dz_join_op* op, int64_t n_rows,
                                const int64_t* d_trip_ids,
                                const int64_t* d_driver_ids);

/* Device-resident probe push (event rows). Matching rows become this
 * call's matches; the rest join the unmatched buffer. */
dz_status dz_join_op_push_probe(dz_join_op* op, int64_t n_rows,
                                const int64_t* d_ts_ms,
                                const int64_t* d_trip_ids,
                                const double* d_vals);

/* The LAST push's matched rows; n_out == 0 when it produced none (the
 * pointers then still name the last non-empty output). The device columns of
 * a push that produced matches stay valid and unchanged, at the pointers
 * returned here, until the push AFTER the next push that produces matches:
 * the output is double-buffered, a push with zero matches recycles nothing,
 * and a push that needs more room regrows only the buffer it writes. So
 *     if (n) dz_window_op_push_device_borrowed(...)
 * after every join push always hands the window op live columns for its
 * one-step borrowed lifetime, whatever the batch sizes and however many
 * empty pushes intervene. */
dz_status dz_join_op_matches(dz_join_op* op, int64_t* n_out,
                             const int64_t** d_ts_ms, const int32_t** d_kids,
                             const double** d_vals);
int64_t dz_join_op_unmatched(dz_join_op* op);

/* ------------------------------------------------------------------ */
/* JSON ingest (from_topic's decode stage): the reference decodes Kafka
 * payload bytes on the host with serde_json
 * (crates/core/src/formats/decoders/json.rs:23-46, driven by
 * kafka_stream_read.rs:165-296); here the decode runs ON DEVICE over
 * newline-delimited records, producing (int64 ts, utf8 key column, f64
 * value) device columns shaped for dz_window_op_push_device_utf8 — the
 * on-wire-bytes -> windowed-aggregate pipeline stays in HBM end to end.
 * Input is strict JSON, as serde_json::from_slice takes it, one object per
 * '\n'-separated line (a trailing '\n' opens no further record; a blank
 * line is an error); inside that, a documented subset decodes and anything
 * else fails loudly, with one message class per cause:
 *  - "exact parse subset": valid JSON the exact parse does not cover.
 *    VALUE: a JSON-grammar number with at most 15 significant digits and
 *    |e10| <= 22, where the significant digits are the integer and fraction
 *    digits as written minus the zeros before the first non-zero digit (on
 *    either side of the point; trailing zeros count, an all-zero literal
 *    has 1) and e10 = exponent - number of fraction digits, the exponent
 *    evaluated without wraparound. There the result is (double)digits times
 *    or divided by an exact power of ten: equal to strtod bit for bit.
 *    TIMESTAMP: an integer literal (no fraction, no exponent) within int64;
 *    -9223372036854775808 is INT64_MIN. KEY: a string whose raw bytes hold
 *    no backslash; the empty key is legal.
 *  - "malformed": not strict JSON (number grammar: no empty literal, "1.",
 *    ".5", "1e", "01"; true/false/null spelled exactly; commas exactly
 *    between members; no raw control byte in a string; only space, tab or
 *    CR before '{' and after '}'), or a schema field of the wrong JSON type
 *    (a string for a number, a number/null/nested value for the key).
 *  - "missing": a schema field is absent.
 * The three schema fields are top-level members matched on their raw name
 * bytes (a schema name spelled with escapes is not recognised); when one is
 * duplicated the last occurrence wins. Every other member is skipped and may
 * be any JSON value under any name, escapes included. Not validated: the
 * spelling of escape sequences, UTF-8, and the inside of a skipped nested
 * object/array beyond matching its brackets and quotes. */

typedef struct dz_json_decoder dz_json_decoder;

dz_json_decoder* dz_json_decoder_create(int32_t device, const char* ts_field,
                                        const char* key_field,
                                        const char* val_field);
void dz_json_decoder_destroy(dz_json_decoder* d);
const char* dz_json_decoder_last_error(dz_json_decoder* d);

/* Decode one device-resident byte buffer. Columns are retrieved with
 * dz_json_decoder_batch and stay valid until the SECOND-next decode
 * (double-buffered, covering a utf8 borrowed push across one step; a
 * larger batch regrows only the buffer it writes, so this holds across
 * growth too). A rejected decode (DZ_ERR, message from
 * dz_json_decoder_last_error) leaves n == 0, the last good batch's columns
 * intact and the handle usable. n_bytes == 0 is DZ_OK with n == 0. */
dz_status dz_json_decode(dz_json_decoder* d, const char* d_bytes,
                         int64_t n_bytes);
dz_status dz_json_decoder_batch(dz_json_decoder* d, int64_t* n_out,
                                const int64_t** d_ts_ms,
                                const int32_t** d_key_offsets,
                                const char** d_key_data,
                                const double** d_vals);

/* Synthetic on-wire JSON generator (bench/test input): one newline-
 * delimited record per row of the same seeded sensor stream, reading
 * printed as fixed 6-decimal (inside the decoder's exact subset).
 * Lens pass (host cumsums into int64 offsets) then fill pass. */
dz_status dz_generate_json(int32_t device, uint64_t seed, int64_t t0_ms,
                           int64_t start_row, int64_t n_rows, int64_t n_keys,
                           int64_t rows_per_ms, int32_t* d_lens,
                           const int64_t* d_offsets, char* d_data);

/* ------------------------------------------------------------------ */
/* Synthetic sensor stream generator, on device (bench/test input; spec in
 * DESIGN.md §Generator, bit-identical to oracle orc_gen; mirrors
 * examples/examples/emit_measurements.rs:30-67). Any output pointer may be
 * NULL to skip that column. d_key_ids is the dense int32 form of d_keys. */
dz_status dz_generate(int32_t device, uint64_t seed, int64_t t0_ms,
                      int64_t start_row, int64_t n_rows, int64_t n_keys,
                      int64_t rows_per_ms, int64_t* d_ts_ms,
                      int64_t* d_keys, int32_t* d_key_ids, double* d_vals);

/* Synthetic utf8 key column generator ("sensor_{k}", k from the same seeded
 * draw as dz_generate): pass 1 writes per-row byte lengths to d_lens (host
 * cumsums them into offsets — int32 offsets bound one batch to 2 GiB of key
 * bytes); pass 2 fills d_data at d_offsets. Either pointer pair may be NULL
 * to run one pass. */
dz_status dz_generate_utf8(int32_t device, uint64_t seed, int64_t start_row,
                           int64_t n_rows, int64_t n_keys, int32_t* d_lens,
                           const int32_t* d_offsets, char* d_key_data);

/* Device memory helpers for the bench path (thin wrappers so no HIP types
 * cross the boundary). */
dz_status dz_device_malloc(int32_t device, size_t bytes, void** out);
dz_status dz_device_free(void* ptr);
dz_status dz_device_synchronize(int32_t device);
dz_status dz_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes);
dz_status dz_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes);

/* ------------------------------------------------------------------ */
/* Kernel timing (HIP events recorded on the op's own stream; feeds the
 * bench's roofline line). total_ms covers all completed launches. */
typedef struct dz_kernel_stat {
    char name[32];
    uint64_t launches;
    double total_ms;
    double bytes_per_launch_alg;  /* algorithmic bytes of the LAST launch */
} dz_kernel_stat;

dz_status dz_window_op_kernel_stats(dz_window_op* op, dz_kernel_stat* out,
                                    int32_t cap, int32_t* n_out);

/* ------------------------------------------------------------------ */
/* Pure host logic exported for CPU-only tests (no GPU needed):
 * get_windows_for_watermark + snap_to_window_start
 * (streaming_window.rs:1053-1094; ms generalization for sub-second lengths
 * per SURVEY.md §7). slide_ms == 0 means tumbling. Returns the number of
 * ranges (writes up to cap). */
int64_t dz_debug_windows_for_range(int64_t min_ts, int64_t max_ts,
                                   int64_t len_ms, int64_t slide_ms,
                                   int64_t* starts, int64_t* ends, int64_t cap);

/* Finalise rule of the variance family, shared with emission (which calls
 * this same function): var_pop = m2/count (NULL when count == 0), var_samp =
 * m2/(count-1) (NULL when count <= 1), stddev_* = sqrt of those. Writes the
 * value to *out and returns 1 when valid, 0 when NULL (*out = 0.0), -1 when
 * agg_op is not one of the four variance codes. */
int32_t dz_debug_var_finalize(int32_t agg_op, uint64_t count, double m2,
                              double* out);

/* The median kernels' edges, so tests can aim at them: *lds_vals = the
 * largest group (in values) selected in LDS — a longer one is selected over
 * global memory; *log_min_entries = the first allocation of a window's
 * value log. Either pointer may be NULL. No GPU needed. */
void dz_debug_median_caps(int32_t* lds_vals, int64_t* log_min_entries);

/* Test hook for the device utf8 intern: keep only the low `bits` (1..64)
 * bits of every key fingerprint, so distinct keys collide on demand and the
 * probe-on / byte-verify paths can be exercised. 64 (the default) masks
 * nothing. Legal only before the operator's first device utf8 push; results
 * are unaffected at any setting (verification stays byte-exact), except
 * that two NEW colliding keys inside one batch fail at finish as documented
 * for full 64-bit collisions.
 * On a DZ_KEY_INT64 op (before its first device i64 push) the mask applies
 * to the key's hash before the home slot is taken, so small `bits` forces
 * long probe chains; the key compare stays exact and nothing can fail. */
dz_status dz_debug_intern_fp_bits(dz_window_op* op, int32_t bits);

const char* dz_version(void);

#ifdef __cplusplus
}
#endif

#endif /* DENORMALIZED_AMD_H */
