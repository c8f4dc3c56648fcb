/* dz_internal.h — shared internal declarations between the engine host code
 * (window_op.cpp) and the CDNA4 kernels (kernels.hip). Not part of the C ABI.
 */
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <hip/hip_runtime.h>

namespace dz {

/* Partition geometry. Rows are bucketed by (key_id & (NB-1)): with dense
 * dictionary ids this balances buckets to ±1 key. One wave folds one bucket,
 * so NB also sets fold parallelism (4096 waves = 16 waves/CU on 256 CUs). */
constexpr int NB = 512;
constexpr int LOG_NB = 9;
constexpr int BLOCK = 256;          /* 4 waves */
constexpr int WAVES_PER_BLOCK = BLOCK / 64;
constexpr int MAX_RANGES = 4096;    /* window frames touched by one batch */
constexpr int ST_RECORDS = 2048;    /* scatter staging records per supertile */
/* intern claim: key bytes of one 256-row tile staged in LDS when their span
 * is at most this (16 B/row average; the bench's 8-11 B keys span ~2.8 KB) */
constexpr int INTERN_STAGE_BYTES = 4096;

/* meta word packed per record: kloc (16b) | widx (12b) | valid (1b) */
constexpr uint32_t META_KLOC_MASK = 0xFFFFu;
constexpr int META_WIDX_SHIFT = 16;
constexpr uint32_t META_WIDX_MASK = 0xFFFu;
constexpr int META_VALID_SHIFT = 28;

struct WinParams {
    int64_t s0;          /* first window start of this batch's range list */
    int64_t len_ms;
    int64_t slide_ms;    /* 0 => tumbling */
    int32_t nw;          /* ranges in this batch */
    int32_t is_sliding;
};

struct FoldChunk {
    int32_t w_lo, w_hi;  /* widx range [w_lo, w_hi) this launch folds */
    int32_t k_lo, k_hi;  /* kloc range [k_lo, k_hi) */
    int64_t kcap;        /* state key capacity (multiple of NB) */
    uint64_t row_base;   /* global row id of this batch's row 0: first-seen
                          * = row_base + rowidx, a monotone stream-lifetime
                          * counter (same order as the old batch<<32|row
                          * composite, but window-rebased sort keys stay
                          * small forever — fixed radix pass count) */
    int32_t bin_stride;  /* binoffs/binlens row stride per bucket */
    int32_t tl_nw;       /* two-level mode: windows per batch (0 = off) */
};

/* Extra value columns of a multi-column op (distinct input columns 1..nx, in
 * order of first appearance in aggs), passed to the fold by value: the fold
 * gathers vals[c][row] (and bit `row` of valid[c], LSB-first; null = all
 * valid) by the record's batch row index. slab is the extras' persistent
 * state, [slot][col][{cnt,min,max,sum}][kcap] 8-byte cells (32 B per group
 * per extra), `cells` its size for the bounds guard. nx == 0: unused. */
constexpr int MAX_EXTRA_COLS = 3;
struct FoldExtras {
    const double* vals[MAX_EXTRA_COLS] = {};
    const uint8_t* valid[MAX_EXTRA_COLS] = {};
    uint64_t* slab = nullptr;
    int64_t cells = 0;
    int32_t nx = 0;
};

/* Launch wrappers implemented in kernels.hip. All run on `stream`;
 * n = rows in batch, C = partition chunks (hist/scatter grid). */
void launch_gen(hipStream_t stream, uint64_t seed, int64_t t0, int64_t start_row,
                int64_t n, int64_t nkeys, int64_t rows_per_ms,
                int64_t* d_ts, int64_t* d_keys, int32_t* d_kid, double* d_vals);

/* device utf8 intern (GroupValues::intern analog at device rate) */
void launch_intern(hipStream_t stream, const int32_t* d_offs, const char* d_data,
                   int64_t n,
                   uint4* tab /* 32 B slots {fp, id, lenoff | inline[16]} */,
                   uint32_t* tab_row, uint32_t p_mask, uint32_t* id_off,
                   uint32_t* id_len, char* pool,
                   uint32_t* ctrs /* next id, pool cursor, fresh-batch seq */,
                   uint32_t id_cap, uint32_t pool_cap, int32_t* out_kid,
                   uint32_t seq /* this batch's number, never 0 */,
                   uint64_t fp_mask /* all-ones outside collision tests */,
                   uint32_t* d_dbg);

/* device int64 intern: the same three phases for arbitrary int64 keys */
void launch_intern_i64(hipStream_t stream, const int64_t* d_keys, int64_t n,
                       uint4* tab /* p_mask + 2 16 B slots {key, id, row}:
                                   * the table, then the key-0 cell */,
                       uint32_t p_mask, int64_t* ikeys /* id_cap keys by id */,
                       uint32_t* ctrs /* next id, unused, fresh-batch seq */,
                       uint32_t id_cap, int32_t* out_kid,
                       uint32_t seq /* this batch's number, never 0 */,
                       uint64_t fp_mask /* masks the hash, not the key */,
                       uint32_t* d_dbg);

/* synthetic utf8 key generator ("sensor_{k}"): lens pass and/or fill pass */
void launch_gen_utf8(hipStream_t stream, uint64_t seed, int64_t start_row,
                     int64_t n, int64_t nkeys, int32_t* d_lens,
                     const int32_t* d_offs, char* d_data);

/* d_scalars: [0]=min ts (order-mapped u64), [1]=max ts, [2]=max kid (u64).
 * Host must pre-set [0]=UINT64_MAX, [1]=0, [2]=0. */
void launch_minmax(hipStream_t stream, const int64_t* d_ts, const int32_t* d_kid,
                   int64_t n, uint64_t* d_scalars);

void launch_hist(hipStream_t stream, const int32_t* d_kid, const int64_t* d_ts,
                 int64_t n, int64_t chunk, int C, const WinParams& wp,
                 uint32_t* d_ghist, uint64_t* d_scalars /*fused minmax or null*/);

constexpr int SCAN_SSPLIT = 32; /* d_psum is SCAN_SSPLIT * NB u32 */
void launch_scan(hipStream_t stream, const uint32_t* d_ghist, int C,
                 uint32_t* d_psum, uint32_t* d_bucket_base /*NB+1*/,
                 uint32_t* d_gofs);

/* record payloads are 16 B uint4s: {val lo, val hi, rowidx, meta}; the
 * rowidx word carries the validity bit (bit 31) in FOLD-stage records and
 * .w carries the meta word (kloc|widx|valid) — there is no separate meta
 * array */
void launch_scatter(hipStream_t stream, const int32_t* d_kid, const int64_t* d_ts,
                    const double* d_vals, const uint8_t* d_validity /*bitmap|null*/,
                    int64_t n, int64_t chunk, int C, int32_t st_rows,
                    const WinParams& wp, const uint32_t* d_gofs, uint4* d_grec,
                    uint32_t rec_limit, uint32_t* d_dbg /*bounds-guard cells*/);

constexpr int FOLD_GCAP = 256; /* groups per bucket per fold chunk */

/* value type of the fold (the launches' `ival`): f64, or int64 without / with
 * the variance family's Welford state */
enum { FOLD_F64 = 0, FOLD_INT64 = 1, FOLD_INT64_VAR = 2 };

/* fused stable-split + fold: per-(window,key) bins staged in LDS fold
 * straight into register accumulators seeded from the window-slot slabs —
 * no reordered records in HBM. v_base != null selects the variance-carrying
 * instantiation: the Welford (mean, m2) state lives in a side slab laid out
 * [slot][{mean,m2}][kcap] f64 (vslab_cells = nslots * 2 * kcap), indexed by
 * the same (slot, kloc, bucket) as the main slab and bounds-guarded through
 * d_dbg; null keeps the kernels and the traffic of ops without it.
 * ival != FOLD_F64 selects the int64 instantiations: the records' 8 value
 * bytes are an int64_t, min/max/sum are integers stored bit for bit in the
 * s_min/s_max/s_sum cells, and the side slab (always present then) is
 * [slot][{fsum}][kcap] (FOLD_INT64) or [slot][{fsum, mean, m2}][kcap]
 * (FOLD_INT64_VAR), fsum = the f64 sum of (double)v in row order. */
void launch_regroup_fold(hipStream_t stream, const uint4* d_grec,
                         const uint32_t* d_bucket_base,
                         const FoldChunk& fc, const int32_t* d_slot_of_widx,
                         uint64_t* s_cnt, double* s_min, double* s_max,
                         double* s_sum, uint64_t* s_first, int64_t slab_cells,
                         uint32_t* d_dbg, double* v_base, int64_t vslab_cells,
                         const FoldExtras& fx, int ival = FOLD_F64);

void launch_regroup_l1(hipStream_t stream, const uint4* d_grec,
                       const uint32_t* d_bucket_base,
                       const FoldChunk& fc, uint32_t* d_b1offs,
                       uint32_t* d_b1lens, uint4* d_grec2);

void launch_regroup_l2_fold(hipStream_t stream, const uint4* d_grec2,
                            const uint32_t* d_bucket_base,
                            const FoldChunk& fc, int nb1,
                            const uint32_t* d_b1offs, const uint32_t* d_b1lens,
                            const int32_t* d_slot_of_widx, uint64_t* s_cnt,
                            double* s_min, double* s_max, double* s_sum,
                            uint64_t* s_first, int64_t slab_cells,
                            uint32_t* d_dbg, double* v_base,
                            int64_t vslab_cells, const FoldExtras& fx,
                            int ival = FOLD_F64);

struct EGatherSlots {
    int32_t s[16];
    uint64_t base[16]; /* per-close window-open row base: the sort key is
                        * first - base, bounded by the window's row span */
};

/* Packed close (DESIGN.md §Packed close): what one closing window's state
 * looks like in a pinned group buffer, `fields` columns of kcap 8-byte cells —
 * the main slab's SLAB_FIELDS {cnt, first, min, max, sum}, then fsum (int64
 * values), then m2 (variance family), then the median, or the extras'
 * 4 * nx fields. The one place that derives it, and with it the widths of the
 * two side slabs, from the op's kind; a field index is -1 where absent. */
constexpr int SLAB_FIELDS = 5;
struct CloseLayout {
    int32_t fields = SLAB_FIELDS;   /* columns of a packed close */
    int32_t fsum = -1, m2 = -1, med = -1, x0 = -1; /* packed column index */
    int32_t vfields = 0;            /* v_base: [slot][vfields][kcap] */
    int32_t v_fsum = -1, v_mean = -1, v_m2 = -1;   /* field within v_base */
    int32_t xfields = 0;            /* x_slab: [slot][4 * nx][kcap] */
    bool side() const { return fields > SLAB_FIELDS; }
};
inline CloseLayout close_layout(bool ival, bool has_var, bool has_med, int nx) {
    CloseLayout l;
    if (ival) { l.fsum = l.fields++; l.v_fsum = l.vfields++; }
    if (has_var) {
        l.m2 = l.fields++;
        l.v_mean = l.vfields++;
        l.v_m2 = l.vfields++;
    }
    if (has_med) l.med = l.fields++;
    if (nx > 0) { l.x0 = l.fields; l.xfields = 4 * nx; l.fields += l.xfields; }
    return l;
}

/* The gather's view of a packed close: at most 3 runs of whole columns, each
 * read from one slab at [slot or close][stride] + off and written at column
 * dst of the close. Travels to k_egather_close by value. */
struct GatherSeg {
    const uint64_t* base;
    int64_t stride;   /* cells per slot of the source (per close: by_close) */
    int64_t off;      /* first cell within that */
    int64_t cells;    /* cells copied */
    int64_t dst;      /* first cell within the packed close */
    int32_t by_close; /* source indexed by close number, not by slot */
};
struct GatherDesc {
    GatherSeg seg[3];
    int32_t nseg = 0;
    int64_t close_cells = 0; /* fields * kcap */
};
inline GatherDesc gather_desc(const CloseLayout& l, int64_t kcap,
                              const uint64_t* s_base, const double* v_base,
                              const uint64_t* x_slab, const double* d_med) {
    GatherDesc d;
    d.close_cells = l.fields * kcap;
    auto add = [&](const void* base, int nf, int f0, int nfield, int dst,
                   bool by_close) {
        d.seg[d.nseg++] = {(const uint64_t*)base, nf * kcap, f0 * kcap,
                           nfield * kcap, dst * kcap, by_close ? 1 : 0};
    };
    add(s_base, SLAB_FIELDS, 0, SLAB_FIELDS, 0, false);
    if (l.fsum >= 0) add(v_base, l.vfields, l.v_fsum, 1, l.fsum, false);
    if (l.m2 >= 0) add(v_base, l.vfields, l.v_m2, 1, l.m2, false);
    if (l.med >= 0) add(d_med, 1, 0, 1, l.med, true);
    if (l.x0 >= 0) add(x_slab, l.xfields, 0, l.xfields, l.x0, false);
    return d;
}

struct EmitFilter {
    int32_t on;      /* 0 = no filter */
    int32_t field;   /* 0 cnt, 1 min, 2 max, 3 sum, 4 avg */
    int32_t cmp;     /* 0 < 1 <= 2 > 3 >= 4 == 5 != */
    double lit;
};

/* The pushed-down filter rule, shared by the device chains (k_efilter,
 * k_egf) and the host build: the count compares as a double; every other
 * field is NULL for an empty group, and NULL never passes a comparison.
 * A comparator code outside 0..5 compares as != here (the device chains'
 * long-standing default arm). The host build has always let such a code
 * pass every non-NULL group instead; filter_pass (window_op.cpp) keeps that
 * rule in front of this call — the two are deliberately NOT unified. */
__host__ __device__ inline bool emit_filter_pass(const EmitFilter& ef,
                                                 uint64_t cnt, double mn,
                                                 double mx, double sum) {
    double v;
    if (ef.field == 0) {
        v = (double)cnt;
    } else {
        if (cnt == 0) return false;
        switch (ef.field) {
            case 1: v = mn; break;
            case 2: v = mx; break;
            case 3: v = sum; break;
            default: v = sum / (double)cnt; break;
        }
    }
    switch (ef.cmp) {
        case 0: return v < ef.lit;
        case 1: return v <= ef.lit;
        case 2: return v > ef.lit;
        case 3: return v >= ef.lit;
        case 4: return v == ef.lit;
        default: return v != ef.lit;
    }
}

/* The packed emission row: the device chains' final-order output, pulled D2H
 * as one span and read by the host builders and by poll()'s zero-copy views.
 * Column-major, `stride` rows per column section:
 *   [key i64][cnt u64][min f64][max f64][sum f64][avg f64][kid u32][flags u8]
 * packed_cols() is the ONLY place that spells the section offsets. */
constexpr int PACKED_ROW_BYTES = 53;

template <typename B> /* B = char (writable) or const char (read-only) */
struct PackedColsT {
    template <typename T>
    using P = typename std::conditional<std::is_const<B>::value, const T,
                                        T>::type*;
    P<int64_t> key;
    P<uint64_t> cnt;
    P<double> min, max, sum, avg;
    P<uint32_t> kid;
    P<uint8_t> flags; /* validity, 0/1 */
};
using PackedCols = PackedColsT<const char>;

/* column pointers of a packed span of `stride` rows, advanced to row `off` */
template <typename B>
__host__ __device__ inline PackedColsT<B> packed_cols(B* base, size_t stride,
                                                      size_t off = 0) {
    PackedColsT<B> c;
    c.key = (decltype(c.key))base + off;
    c.cnt = (decltype(c.cnt))(base + stride * 8) + off;
    c.min = (decltype(c.min))(base + stride * 16) + off;
    c.max = (decltype(c.max))(base + stride * 24) + off;
    c.sum = (decltype(c.sum))(base + stride * 32) + off;
    c.avg = (decltype(c.avg))(base + stride * 40) + off;
    c.kid = (decltype(c.kid))(base + stride * 48) + off;
    c.flags = (decltype(c.flags))(base + stride * 52) + off;
    return c;
}

/* device-side emission at window close, two stages on the copy stream:
 * slabread = compact touched groups + gather aggregate columns + filter
 * flags (after which the window slot is reusable); sort = stable radix by
 * first-seen row, leaving the sorted compact-index permutation in `skid`. */
void launch_emission_slabread(hipStream_t stream, const uint64_t* slab_first,
                              const uint64_t* slab_cnt, const double* slab_min,
                              const double* slab_max, const double* slab_sum,
                              uint64_t base, int64_t K, uint64_t* ekeys, uint32_t* ekid,
                              uint64_t* fkeys, uint32_t* fkid, uint32_t* fiota,
                              uint32_t* counter, uint32_t* counter2,
                              const EmitFilter& ef, uint64_t* ocnt, double* omin,
                              double* omax, double* osum, double* oavg,
                              uint8_t* oflags);
void launch_emission_sort(hipStream_t stream, int64_t K, uint64_t* fkeys,
                          uint64_t* skeys, uint32_t* fiota, uint32_t* okid,
                          uint32_t* counter2, uint32_t* rhist, uint32_t* roffs,
                          uint64_t max_key /* host-known bound on `first` */);
/* group-batched device emission (<=16 closes in one chain; see
 * kernels.hip §GROUP-BATCHED): read phase (slot slabs release after it),
 * then sort+pack */
void launch_emission_group_read(hipStream_t stream, const uint64_t* s_base,
                                int64_t stride_u64, const EGatherSlots& slots,
                                int gcount, int64_t K, int64_t kcap,
                                const EmitFilter& ef, int cshift,
                                uint64_t* gkeys, uint32_t* gkid,
                                uint32_t* giota, uint64_t* gcnt_col,
                                double* gmin, double* gmax, double* gsum,
                                double* gavg, uint8_t* gflags, uint32_t* gtot,
                                uint32_t* gcnt);
void launch_emission_group_sort(hipStream_t stream, int64_t elem_cap,
                                int gcount, int cshift, uint64_t max_first,
                                uint64_t* gkeys, uint64_t* gskeys,
                                uint32_t* gkid, uint32_t* gokid,
                                uint32_t* giota, uint64_t* gcnt_col,
                                double* gmin, double* gmax, double* gsum,
                                double* gavg, uint8_t* gflags, uint32_t* gtot,
                                uint32_t* rhist, uint32_t* roffs, char* pout);

void launch_esort_small(hipStream_t stream, uint64_t* fkeys, uint64_t* skeys,
                        uint32_t* fiota, uint32_t* okid, uint32_t* counter2,
                        uint64_t max_key);
constexpr int EMIT_RCHUNK = 4096;
constexpr int EMIT_RBINS = 2048;

void launch_reset_slots(hipStream_t stream, const int32_t* d_slots, int ns,
                        int64_t kcap, uint64_t* s_cnt, uint64_t* s_first);

/* multi-column ops: zero every extra's cnt of the same slots */
void launch_reset_slots_x(hipStream_t stream, const int32_t* d_slots, int ns,
                          int nx, int64_t kcap, uint64_t* x_slab);

/* host-path emission: pack up to 16 closing window slots' state slabs into
 * one contiguous staging area (one launch + ONE big D2H replaces a per-close
 * copy on the push thread; slot ids travel by value in the kernel args) */
void launch_egather_close(hipStream_t stream, const GatherDesc& desc,
                          EGatherSlots slots, int gcount, uint64_t* out);
void launch_arm_scalars(hipStream_t stream, uint64_t* scalars);

/* Median (kernels.hip §MEDIAN). A window slot's value log is SoA — f64 values
 * then u32 dense key ids, 12 B per entry of capacity — grown by the host from
 * exact per-batch counts. MED_LDS_VALS splits k_med_select's two paths: a
 * group of at most that many values is selected in LDS (16 KiB of keys per
 * 256-thread block keeps 8 blocks = 32 waves per CU), a longer one over
 * global memory. MED_LOG_MIN is the first allocation of a log, in entries. */
constexpr int MED_LDS_VALS = 2048;
constexpr int64_t MED_LOG_MIN = 4096;
constexpr int64_t MED_LOG_MAX = (1LL << 31) - 1; /* entries: u32 positions */
struct MedWin {      /* one window of the batch, indexed by widx */
    double* val;     /* the slot's log */
    uint32_t* kid;
    uint32_t base;   /* entries before this batch */
    uint32_t cap;    /* capacity (bounds guard) */
};
/* per-window valid-row counts of the batch into d_wcnt[nw] (pre-zeroed) */
void launch_med_count(hipStream_t stream, const int64_t* d_ts,
                      const uint8_t* d_validity /*bitmap|null*/, int64_t n,
                      const WinParams& wp, uint32_t* d_wcnt);
/* append every valid row to each containing window's log; d_fill[nw] is the
 * batch's per-window cursor (pre-zeroed); overflow flags d_dbg[2] */
void launch_med_append(hipStream_t stream, const int64_t* d_ts,
                       const uint8_t* d_validity, const int32_t* d_kid,
                       const double* d_vals, int64_t n, const WinParams& wp,
                       const MedWin* d_win, uint32_t* d_fill, uint32_t* d_dbg);
/* close chain of one slot: d_seg_off[k] = exclusive scan of d_cnt[0..K),
 * d_fill[0..K) zeroed (d_bsum: ceil(K / 2048) cells of scratch); the log's
 * values scattered into their segments of d_sorted; med[k] per group */
void launch_med_scan(hipStream_t stream, const uint64_t* d_cnt, int64_t K,
                     uint32_t* d_bsum, uint32_t* d_seg_off, uint32_t* d_fill);
void launch_med_place(hipStream_t stream, const uint32_t* d_lkid,
                      const double* d_lval, int64_t len,
                      const uint32_t* d_seg_off, uint32_t* d_fill, int64_t K,
                      double* d_sorted, uint32_t* d_dbg);
void launch_med_select(hipStream_t stream, const uint64_t* d_cnt,
                       const uint32_t* d_seg_off, const double* d_sorted,
                       int64_t len, int64_t K, double* d_med, uint32_t* d_dbg);
void launch_fill_i64(hipStream_t stream, int64_t* d_p, int64_t n, int64_t v);

/* JSON ingest (kernels.hip §JSON ingest): newline count/scan, then
 * emit+parse+key compaction with the record count known host-side */
struct JsonFields {
    char ts_name[32];
    char key_name[32];
    char val_name[32];
    int32_t ts_len, key_len, val_len;
};
void launch_json_count(hipStream_t stream, const char* d_buf, int64_t nbytes,
                       int C, int64_t chunk, int32_t tail_record,
                       uint32_t* d_cnt, uint32_t* d_base, uint32_t* d_tot);
void launch_json_parse(hipStream_t stream, const char* d_buf, int64_t nbytes,
                       int C, int64_t chunk, const JsonFields& jf,
                       const uint32_t* d_base, const uint32_t* d_tot,
                       int64_t* d_recoff, int64_t nrec, int64_t* o_ts,
                       int64_t* o_kbeg, int32_t* o_klen, double* o_val,
                       uint32_t* d_blocksum, uint32_t* d_ktot, int32_t* o_koff,
                       char* o_kdata, uint32_t* d_dbg);
void launch_gen_json(hipStream_t stream, uint64_t seed, int64_t t0,
                     int64_t start_row, int64_t n, int64_t nkeys,
                     int64_t rows_per_ms, int32_t* d_lens,
                     const int64_t* d_offs, char* d_data);

/* stream join (cfg5): open-address trip->driver build table + stable
 * order-preserving probe/emit (kernels.hip §stream join). d_pre is four
 * cells the host zeroes per build push: the pre-pass writes {reserved trip
 * seen, driver id out of int32 range seen, rows whose trip is not in the
 * table (an upper bound: in-batch duplicates each count)}, the build adds
 * the slots it claimed to d_pre[3]. */
void launch_join_precheck(hipStream_t stream, const int64_t* d_trips,
                          const int64_t* d_drivers, int64_t n,
                          const int64_t* tab_trip, uint64_t p_mask,
                          uint32_t* d_pre);
void launch_join_build(hipStream_t stream, const int64_t* d_trips,
                       const int64_t* d_drivers, int64_t n, int64_t* tab_trip,
                       int64_t* tab_drv, uint64_t p_mask, uint32_t* d_dbg,
                       uint32_t* d_pre);
void launch_join_probe(hipStream_t stream, const int64_t* d_ts,
                       const int64_t* d_trips, const double* d_vals, int64_t n,
                       int64_t chunk, int C, const int64_t* tab_trip,
                       const int64_t* tab_drv, uint64_t p_mask,
                       int32_t* d_drvtmp, uint32_t* d_jcnt, uint32_t* d_mbase,
                       uint32_t* d_ubase, uint32_t* d_tot, int64_t* o_ts,
                       int32_t* o_kid, double* o_val, int64_t ubuf_base,
                       int64_t* u_ts, int64_t* u_trip, double* u_val);
void launch_zero_counters(hipStream_t stream, uint32_t* two_u32);
void launch_emission_permute(hipStream_t stream, int64_t K,
                             const uint32_t* counter2, const uint32_t* sidx,
                             const uint32_t* fkid, const uint64_t* ocnt,
                             const double* omin, const double* omax,
                             const double* osum, const double* oavg,
                             const uint8_t* oflags, char* out);

} // namespace dz
