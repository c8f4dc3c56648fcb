/* kernels.hip — hand-written CDNA4 (gfx950) kernels for the streaming
 * windowed aggregate. MI355X-first design, not a translation: the reference
 * computes this path on CPU with arrow-rs compare/filter kernels plus a
 * DataFusion hash table and accumulators over 32-row batches
 * (grouped_window_agg_stream.rs:548-605, :501-537); here the same semantics
 * run as a deterministic stable key-partition + per-group row-order fold over
 * multi-million-row device-resident batches:
 *
 *   k_minmax   batch watermark bounds (time.rs:31-57) + max key id
 *   k_hist     per-chunk bucket histogram (bucket = key_id & (NB-1)),
 *              with per-row window multiplicity (sliding windows expand)
 *   k_scan_*   bucket bases + per-chunk stable offsets
 *   k_scatter_t<MULT>  stable partition: records (meta,rowidx,value) land in
 *              bucket regions IN GLOBAL ROW ORDER, each row read once and
 *              held in registers (MULT: sliding rows expand to one record
 *              per window, weighted intra-wave ranks via readlane)
 *   k_regroup_t<RG_*_FOLD>  one block per bucket (or (bucket,bin1) segment):
 *              stable per-supertile split of the bucket's records into
 *              per-(window,key) bins IN LDS, then each bin's staged segment
 *              folds directly into a per-thread register accumulator IN ROW
 *              ORDER — count/min/max and the f64 sum are bit-identical to
 *              the reference's sequential accumulator updates (update_batch
 *              call order, grouped_window_agg_stream.rs:533). The reordered
 *              records never touch HBM (the unfused regroup+fold pair they
 *              replace moved ~32 B/row of pure materialization traffic).
 *
 * No atomics on the data path (only LDS histogram counts); every kernel is
 * deterministic. Roofline: HBM bandwidth (no contraction => no MFMA).
 */
#include "dz_internal.h"

#include <algorithm>
#include <cassert>

namespace dz {

__device__ __forceinline__ int64_t i64min(int64_t a, int64_t b) { return a < b ? a : b; }

/* ------------------------------------------------------------------ */
/* helpers                                                             */
/* ------------------------------------------------------------------ */

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9e3779b97f4a7c15ULL;
    x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ULL;
    x = (x ^ (x >> 27)) * 0x94d049bb133111ebULL;
    return x ^ (x >> 31);
}

/* snap_to_window_start (streaming_window.rs:1088-1094): whole-second
 * truncation; ms generalization for sub-second lengths. Assumes
 * ts >= 0 (the reference's SystemTime arithmetic asserts the same). */
__device__ __forceinline__ int64_t snap_ms(int64_t ts, int64_t len_ms) {
    int64_t len_s = len_ms / 1000;
    if (len_s == 0) return ts - (ts % len_ms);
    return (ts / 1000) / len_s * len_s * 1000;
}

__device__ __forceinline__ int64_t floordiv(int64_t a, int64_t b) {
    int64_t q = a / b, r = a % b;
    return q - ((r != 0) & ((r < 0) != (b < 0)));
}

/* Window coverage of a row: first widx and count (sliding expands).
 * Mirrors get_windows_for_watermark membership (streaming_window.rs:1053-1086):
 * row t is in window j iff starts[j] <= t < starts[j]+len. */
__device__ __forceinline__ void row_windows(int64_t t, const WinParams& wp,
                                            int32_t* jmin, int32_t* m) {
    if (wp.is_sliding) {
        int64_t lo = floordiv(t - wp.len_ms - wp.s0, wp.slide_ms) + 1; /* start > t-len */
        int64_t hi = floordiv(t - wp.s0, wp.slide_ms);                 /* start <= t    */
        if (lo < 0) lo = 0;
        if (hi > wp.nw - 1) hi = wp.nw - 1;
        *jmin = (int32_t)lo;
        *m = (hi >= lo) ? (int32_t)(hi - lo + 1) : 0;
    } else {
        /* windows are consecutive [s0 + i*len) (streaming_window.rs:1076-1082) */
        *jmin = (int32_t)((t - wp.s0) / wp.len_ms);
        *m = 1;
    }
}

/* ------------------------------------------------------------------ */
/* generator (spec shared with oracle orc_gen)   */
/* ------------------------------------------------------------------ */

__global__ void k_gen(uint64_t seed, int64_t t0, int64_t start_row, int64_t n,
                      int64_t nkeys, int64_t rows_per_ms, int64_t* ts,
                      int64_t* keys, int32_t* kid, double* vals) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        int64_t gi = start_row + i;
        uint64_t r = splitmix64(seed ^ (0x9e3779b97f4a7c15ULL * (uint64_t)(gi + 1)));
        uint64_t k = r % (uint64_t)nkeys;
        if (ts) ts[i] = t0 + gi / rows_per_ms;
        if (keys) keys[i] = (int64_t)k;
        if (kid) kid[i] = (int32_t)k;
        if (vals) vals[i] = (double)(splitmix64(r) >> 11) * (1.0 / 9007199254740992.0) * 115.0;
    }
}

void launch_gen(hipStream_t s, uint64_t seed, int64_t t0, int64_t start_row,
                int64_t n, int64_t nkeys, int64_t rows_per_ms,
                int64_t* d_ts, int64_t* d_keys, int32_t* d_kid, double* d_vals) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_gen, dim3(blocks), dim3(BLOCK), 0, s, seed, t0,
                       start_row, n, nkeys, rows_per_ms, d_ts, d_keys, d_kid, d_vals);
}

/* ------------------------------------------------------------------ */
/* device utf8 intern — GroupValues::intern for string keys            */
/* (grouped_window_agg_stream.rs:512) AT DEVICE RATE: open-address     */
/* claim on a 64-bit FNV fingerprint, byte-verified against a device   */
/* string pool, dense ids from a global counter. Id VALUES are         */
/* schedule-dependent and never surface: bucketing only needs density, */
/* per-group row order (and with it bit-exactness) is preserved by the */
/* partition pipeline, and emission orders groups by first-seen row    */
/* and emits the original bytes from the pool.                         */
/* ------------------------------------------------------------------ */

__device__ __forceinline__ uint64_t fnv1a64(const char* p, int32_t len) {
    /* byte-wise FNV-1a: measured FASTER than a word-at-a-time variant with
     * unaligned dword GLOBAL loads on gfx950 (2.1 ms vs 0.68 ms per 8M-row
     * batch for the whole intern chain). The claim kernel no longer walks
     * global memory here for short-span tiles: it stages a tile's key bytes
     * in LDS and runs this chain against LDS (k_intern_claim). Reading the
     * staged key as aligned dwords funnel-shifted into registers measured
     * the same as the byte walk, so the byte walk stays. */
    uint64_t h = 1469598103934665603ULL;
    for (int32_t i = 0; i < len; i++) {
        h ^= (uint8_t)p[i];
        h *= 1099511628211ULL;
    }
    return h;
}

__device__ __forceinline__ bool bytes_eq(const char* a, const char* b,
                                         int32_t len) {
    for (int32_t i = 0; i < len; i++)
        if (a[i] != b[i]) return false;
    return true;
}

/* table slot: 32 B, 32 B-aligned (never straddles a 128 B line), two uint4s:
 *   [0] {fp lo, fp hi, id, lenoff}   [1] inline[16] (key bytes, zero-padded)
 * fp is the 8 B word the claim CAS works on; everything else is written by
 * k_intern_assign only. ONE cache line serves the probe, the resolve AND
 * the byte-verify of keys up to 16 B (the pool gather they replace was ~11
 * fully divergent byte loads per row). lenoff low 6 bits:
 *   0..62  key length, pool offset (< 2^26) in the upper 26 bits
 *   63     upper bits 0..16: the key's length, its bytes are in inline[]
 *          upper bits all-ones: resolve through the id_off/id_len arrays */
constexpr uint32_t INTERN_INLINE_MAX = 16;

__device__ __forceinline__ uint64_t slot_fp(const uint4& v) {
    return (uint64_t)v.x | ((uint64_t)v.y << 32);
}

/* fingerprint of one key + its first 16 bytes in two registers (lo = bytes
 * 0..7, hi = bytes 8..15; zero for longer keys) for the inline verify. `p` is
 * an LDS address on the staged path and a global one on the fallback path:
 * force-inlined, each call site gets loads of its own address space. */
__device__ __forceinline__ uint64_t key_fp_bytes(const uint8_t* p, int32_t len,
                                                 uint64_t* klo, uint64_t* khi) {
    uint64_t lo = 0, hi = 0, fp = 1469598103934665603ULL;
    if ((uint32_t)len <= INTERN_INLINE_MAX) {
        const int32_t n0 = len < 8 ? len : 8;
        for (int32_t j = 0; j < n0; j++) {
            const uint64_t b = p[j];
            fp = (fp ^ b) * 1099511628211ULL;
            lo |= b << (8 * j);
        }
        for (int32_t j = 8; j < len; j++) {
            const uint64_t b = p[j];
            fp = (fp ^ b) * 1099511628211ULL;
            hi |= b << (8 * (j - 8));
        }
    } else {
        fp = fnv1a64((const char*)p, len);
    }
    *klo = lo;
    *khi = hi;
    return fp;
}

/* stage granules: the span plus up to 15 B each of head and tail alignment */
constexpr int INTERN_STAGE_GRAN = INTERN_STAGE_BYTES / 16 + 2;

__global__ __launch_bounds__(BLOCK) void k_intern_claim(const int32_t* offs,
        const char* data, int64_t n, uint4* tab, uint32_t* tab_row,
        const uint32_t* id_off, const uint32_t* id_len,
        const char* pool, uint32_t p_mask, uint64_t fp_mask, int32_t* out_kid,
        uint32_t* fresh_seq, uint32_t seq, uint32_t* dbg) {
    /* phase 1: every row probes; exactly one row CASes each new
     * fingerprint in, recording itself as the claiming row. No lane ever
     * waits on another (a publish-wait design can cycle across waves).
     * STEADY STATE (slot already has an assigned id from an earlier batch):
     * byte-verify and resolve right here — out_kid = id, final. Rows of
     * keys claimed in THIS batch store ~slot (negative) for the lookup
     * phase and stamp *fresh_seq with this batch's sequence number; assign
     * and lookup return at once when the stamp is not theirs.
     *
     * The block walks tiles of BLOCK consecutive rows (block-uniform loop:
     * the body has barriers). A tile's keys are one contiguous span of the
     * utf8 column: its offsets are read once into LDS, and a span of at most
     * INTERN_STAGE_BYTES is copied into LDS with aligned, coalesced 16 B
     * loads — only granules holding at least one byte of the span, so the
     * copy never leaves a page the column is on. Each lane then hashes its
     * key from LDS. A tile with a longer span hashes from global memory. */
    __shared__ int32_t s_offs[BLOCK + 1];
    __shared__ uint4 s_stage[INTERN_STAGE_GRAN];
    const int t = threadIdx.x;
    const int64_t ntiles = (n + BLOCK - 1) / BLOCK;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * BLOCK;
        const int rows = (int)i64min(BLOCK, n - i0);
        if (t < rows) s_offs[t] = offs[i0 + t];
        if (t == 0) s_offs[rows] = offs[i0 + rows];
        __syncthreads();
        const int32_t o_first = s_offs[0];
        const uint32_t span = (uint32_t)(s_offs[rows] - o_first);
        const bool staged = span <= (uint32_t)INTERN_STAGE_BYTES;
        uint32_t head = 0;
        if (staged) {
            if (span) {
                const char* a0 = data + o_first;
                head = (uint32_t)((uintptr_t)a0 & 15u);
                const uint4* g = (const uint4*)(a0 - head);
                const uint32_t ngran = (head + span + 15u) >> 4;
                for (uint32_t k = t; k < ngran; k += BLOCK) s_stage[k] = g[k];
            }
            __syncthreads();
        }
        const bool active = t < rows;
        const int64_t i = i0 + t;
        int32_t o0 = 0, len = 0;
        uint64_t klo = 0, khi = 0, fp = 0;
        if (active) {
            o0 = s_offs[t];
            len = s_offs[t + 1] - o0;
            if (staged) {
                const uint32_t q = head + (uint32_t)(o0 - o_first);
                fp = key_fp_bytes((const uint8_t*)s_stage + q, len, &klo,
                                  &khi);
            } else {
                fp = key_fp_bytes((const uint8_t*)data + o0, len, &klo, &khi);
            }
        }
        /* every LDS read of this tile is done: the next tile may overwrite
         * the stage while slower lanes are still probing */
        __syncthreads();
        if (!active) continue;
        const char* p = data + o0;
        fp &= fp_mask; /* all-ones outside the collision tests */
        if (!fp) fp = 1; /* 0 marks an empty slot */
        uint32_t slot = (uint32_t)fp & p_mask;
        int32_t out;
        for (uint32_t probes = 0;; slot = (slot + 1) & p_mask) {
            /* both halves of the slot, issued together: one line. A slot
             * whose id is assigned was written whole by an earlier kernel,
             * so none of its words can tear and this load is all the
             * steady state needs. */
            const uint4 a = tab[(size_t)slot * 2];
            const uint4 b = tab[(size_t)slot * 2 + 1];
            const uint32_t cand = a.z;
            const uint32_t lo = a.w;
            const bool assigned = cand != ~0u;
            const bool fpeq = slot_fp(a) == fp;
            /* the whole short-key verdict as ONE predicate (non-short-
             * circuit on purpose: both loads are then needed before the
             * first branch and stay two back-to-back 16 B loads) */
            const uint64_t slo = (uint64_t)b.x | ((uint64_t)b.y << 32);
            const uint64_t shi = (uint64_t)b.z | ((uint64_t)b.w << 32);
            const bool inline_hit = assigned & fpeq &
                ((uint32_t)len <= INTERN_INLINE_MAX) &
                (lo == (((uint32_t)len << 6) | 63u)) & (slo == klo) &
                (shi == khi);
            if (inline_hit) {
                out = (int32_t)cand;
                break;
            }
            if (assigned) {
                const uint32_t clen = lo & 63u;
                const bool is_inline =
                    clen == 63u && (lo >> 6) <= INTERN_INLINE_MAX;
                if (fpeq && !is_inline) { /* same key unless fp64 collides */
                    const bool fits = clen != 63u;
                    const uint32_t co = fits ? (lo >> 6) : id_off[cand];
                    const uint32_t cl = fits ? clen : id_len[cand];
                    if (cl == (uint32_t)len && bytes_eq(pool + co, p, len)) {
                        out = (int32_t)cand;
                        break;
                    }
                }
                /* a different key (fp64 collision or another home slot's
                 * overflow): probe on */
            } else {
                /* empty, or claimed in this batch (assign runs after this
                 * kernel, so an unassigned id stays unassigned throughout):
                 * fp again as an aligned 8 B ATOMIC load (single-copy atomic
                 * vs a concurrent claim CAS — the fp halves of the 16 B
                 * vector load above are not guaranteed tear-free, and a
                 * plain reload could legally be folded into it), then the
                 * CAS */
                uint64_t got = __hip_atomic_load(
                    (const uint64_t*)tab + (size_t)slot * 4, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT);
                if (got == 0)
                    got = (uint64_t)atomicCAS(
                        (unsigned long long*)&tab[(size_t)slot * 2], 0ULL,
                        (unsigned long long)fp);
                if (got == 0 || got == fp) {
                    /* got == 0: claimed, I define the bytes; got == fp:
                     * fresh this batch, lookup decides */
                    if (got == 0) tab_row[slot] = (uint32_t)i;
                    *fresh_seq = seq;
                    out = ~(int32_t)slot;
                    break;
                }
            }
            if (++probes > p_mask) {
                dbg[3] = 4; /* table full */
                *fresh_seq = seq;
                out = ~(int32_t)slot;
                break;
            }
        }
        out_kid[i] = out;
    }
}

__global__ __launch_bounds__(BLOCK) void k_intern_assign(uint4* tab,
        uint32_t* tab_row, uint32_t p_count,
        const int32_t* offs, const char* data, uint32_t* id_off,
        uint32_t* id_len, char* pool, uint32_t* ctrs, uint32_t id_cap,
        uint32_t pool_cap, const uint32_t* fresh_seq, uint32_t seq,
        uint32_t* dbg) {
    /* phase 2 (after claim completes, stream-ordered): one thread per slot;
     * slots claimed this batch (fp set, id still unassigned) get a dense id,
     * their first-seen bytes copied into the persistent pool and — up to
     * 16 B — into the slot itself. The only writer of everything but fp; no
     * reader runs concurrently, so no slot is ever seen half-written. */
    if (*fresh_seq != seq) return; /* nothing was claimed in this batch */
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t sl = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         sl < p_count; sl += stride) {
        uint4 v = tab[(size_t)sl * 2];
        if (slot_fp(v) == 0 || v.z != ~0u) continue;
        const uint32_t r = tab_row[sl];
        const int32_t o0 = offs[r];
        const int32_t len = offs[r + 1] - o0;
        const uint32_t nid = atomicAdd(&ctrs[0], 1u);
        const uint32_t po = atomicAdd(&ctrs[1], (uint32_t)len);
        if (nid >= id_cap || po + (uint32_t)len > pool_cap) {
            dbg[3] = nid >= id_cap ? 1 : 2; /* capacity guard */
            continue;
        }
        uint64_t klo = 0, khi = 0;
        for (int32_t j = 0; j < len; j++) {
            const uint8_t c = (uint8_t)data[o0 + j];
            pool[po + j] = (char)c;
            if (j < 8) klo |= (uint64_t)c << (8 * j);
            else if (j < (int32_t)INTERN_INLINE_MAX)
                khi |= (uint64_t)c << (8 * (j - 8));
        }
        id_off[nid] = po;
        id_len[nid] = (uint32_t)len;
        v.z = nid;
        /* lenoff (slot comment above): inline up to 16 B, pool offset fast
         * path for len<=62 and off<2^26, else the fallback arrays */
        if ((uint32_t)len <= INTERN_INLINE_MAX) {
            v.w = ((uint32_t)len << 6) | 63u;
            tab[(size_t)sl * 2 + 1] = make_uint4((uint32_t)klo,
                (uint32_t)(klo >> 32), (uint32_t)khi, (uint32_t)(khi >> 32));
        } else {
            v.w = (len <= 62 && po < (1u << 26)) ? ((po << 6) | (uint32_t)len)
                                                 : 0xFFFFFFFFu;
        }
        tab[(size_t)sl * 2] = v;
    }
}

__global__ __launch_bounds__(BLOCK) void k_intern_lookup(const int32_t* offs,
        const char* data, int64_t n, const uint4* tab,
        const uint32_t* id_off, const uint32_t* id_len, const char* pool,
        int32_t* out_kid, const uint32_t* fresh_seq, uint32_t seq,
        uint32_t* dbg) {
    /* phase 3 (after assign): resolve each row's slot (stashed as ~slot by
     * the claim phase) to its dense id, byte-verifying against the pool —
     * distinct keys sharing a full 64-bit fingerprint cannot be interned
     * and are FLAGGED (results then fail loudly via the guard cells). In
     * steady state no row is stashed and the whole pass is skipped. */
    if (*fresh_seq != seq) return; /* claim resolved every row */
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const int32_t v = out_kid[i];
        if (v >= 0) continue; /* resolved by the claim phase: final */
        const uint32_t slot = (uint32_t)~v;
        const uint32_t cand = tab[(size_t)slot * 2].z;
        int32_t id = 0;
        if (cand == ~0u) {
            dbg[3] = 5; /* capacity overflow left the slot unassigned */
        } else {
            const int32_t o0 = offs[i];
            const int32_t len = offs[i + 1] - o0;
            const bool eq = id_len[cand] == (uint32_t)len &&
                            bytes_eq(pool + id_off[cand], data + o0, len);
            if (eq) id = (int32_t)cand;
            else dbg[3] = 6; /* fp64 collision between distinct keys */
        }
        out_kid[i] = id;
    }
}

void launch_intern(hipStream_t s, const int32_t* d_offs, const char* d_data,
                   int64_t n, uint4* tab, uint32_t* tab_row, uint32_t p_mask,
                   uint32_t* id_off, uint32_t* id_len, char* pool,
                   uint32_t* ctrs, uint32_t id_cap, uint32_t pool_cap,
                   int32_t* out_kid, uint32_t seq, uint64_t fp_mask,
                   uint32_t* dbg) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    const uint32_t P = p_mask + 1;
    int sblocks = (int)std::min<uint32_t>((P + BLOCK - 1) / BLOCK, 2048);
    uint32_t* fresh_seq = ctrs + 2;
    hipLaunchKernelGGL(k_intern_claim, dim3(blocks), dim3(BLOCK), 0, s, d_offs,
                       d_data, n, tab, tab_row, id_off, id_len,
                       pool, p_mask, fp_mask, out_kid, fresh_seq, seq, dbg);
    hipLaunchKernelGGL(k_intern_assign, dim3(sblocks), dim3(BLOCK), 0, s,
                       tab, tab_row, P, d_offs, d_data, id_off,
                       id_len, pool, ctrs, id_cap, pool_cap, fresh_seq, seq,
                       dbg);
    hipLaunchKernelGGL(k_intern_lookup, dim3(blocks), dim3(BLOCK), 0, s,
                       d_offs, d_data, n, tab, id_off,
                       id_len, pool, out_kid, fresh_seq, seq, dbg);
}

/* ------------------------------------------------------------------ */
/* device int64 intern — the same three stream-ordered phases for      */
/* 8-byte keys. The key is its own identity: the claim word IS the     */
/* key, so there is no fingerprint, no pool and no verify, and no two  */
/* distinct keys can merge.                                            */
/*                                                                     */
/* slot: 16 B, 16 B-aligned, one uint4 = one probe load:               */
/*   {claim lo, claim hi, id (~0 = unassigned), claiming row}          */
/* The claim word is the CAS target, 0 = empty. Key 0 therefore cannot */
/* live in the table: it owns the extra slot tab[P] behind the P table */
/* slots, claimed by its own CAS (0 -> I64_ZERO_CLAIM) and never       */
/* probed past. Every int64 value is a legal key.                      */
/* home slot = splitmix64(key) & fp_mask & p_mask (fp_mask is all-ones */
/* outside dz_debug_intern_fp_bits).                                   */
/* ------------------------------------------------------------------ */

constexpr uint64_t I64_ZERO_CLAIM = 1; /* claim word of the key-0 cell */

__global__ __launch_bounds__(BLOCK) void k_intern_i64_claim(
        const int64_t* keys, int64_t n, uint4* tab, uint32_t p_mask,
        uint64_t fp_mask, int32_t* out_kid, uint32_t* fresh_seq, uint32_t seq,
        uint32_t* dbg) {
    /* phase 1: every row probes; exactly one row CASes each new key in and
     * records itself as the claiming row (the one word of a slot this
     * phase writes besides the claim word; nothing reads it back on
     * device). No lane ever waits on another. A slot whose id is assigned
     * was written whole by an earlier batch's assign: key equal -> out_kid
     * is final. Rows of keys claimed in THIS batch store ~slot and stamp
     * *fresh_seq; assign and lookup return at once otherwise. */
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const uint64_t key = (uint64_t)keys[i];
        const bool zero = key == 0;
        const uint64_t want = zero ? I64_ZERO_CLAIM : key;
        /* the key-0 cell only ever holds 0 or I64_ZERO_CLAIM, so a key-0
         * row leaves the loop in its first iteration */
        uint32_t slot = zero ? p_mask + 1
                             : (uint32_t)(splitmix64(key) & fp_mask) & p_mask;
        int32_t out;
        for (uint32_t probes = 0;; slot = (slot + 1) & p_mask) {
            const uint4 a = tab[slot];
            if (a.z != ~0u) {
                if (slot_fp(a) == want) {
                    out = (int32_t)a.z;
                    break;
                }
                /* another key's slot: probe on */
            } else {
                /* empty, or claimed in this batch (ids are assigned after
                 * this kernel): the claim word again as an aligned 8 B
                 * ATOMIC load — the halves of the 16 B load above may tear
                 * against a concurrent claim CAS — then the CAS */
                uint64_t got = __hip_atomic_load(
                    (const uint64_t*)tab + (size_t)slot * 2, __ATOMIC_RELAXED,
                    __HIP_MEMORY_SCOPE_AGENT);
                if (got == 0)
                    got = (uint64_t)atomicCAS((unsigned long long*)&tab[slot],
                                              0ULL, (unsigned long long)want);
                if (got == 0 || got == want) {
                    if (got == 0) ((uint32_t*)&tab[slot])[3] = (uint32_t)i;
                    *fresh_seq = seq;
                    out = ~(int32_t)slot;
                    break;
                }
            }
            if (++probes > p_mask) {
                dbg[3] = 4; /* table full */
                *fresh_seq = seq;
                out = ~(int32_t)slot;
                break;
            }
        }
        out_kid[i] = out;
    }
}

__global__ __launch_bounds__(BLOCK) void k_intern_i64_assign(uint4* tab,
        uint32_t n_slots, int64_t* ikeys, uint32_t* ctrs, uint32_t id_cap,
        const uint32_t* fresh_seq, uint32_t seq, uint32_t* dbg) {
    /* phase 2: one thread per slot (the key-0 cell is slot n_slots - 1);
     * a slot claimed this batch gets a dense id, its key goes to
     * ikeys[id] for the host mirror, then the slot's id is set. The only
     * writer of ids; no reader runs concurrently. */
    if (*fresh_seq != seq) return; /* nothing was claimed in this batch */
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t sl = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         sl < n_slots; sl += stride) {
        const uint4 v = tab[sl];
        const uint64_t w = slot_fp(v);
        if (w == 0 || v.z != ~0u) continue;
        const uint32_t nid = atomicAdd(&ctrs[0], 1u);
        if (nid >= id_cap) {
            dbg[3] = 1; /* capacity guard */
            continue;
        }
        ikeys[nid] = sl == (int64_t)n_slots - 1 ? 0 : (int64_t)w;
        ((uint32_t*)&tab[sl])[2] = nid;
    }
}

__global__ __launch_bounds__(BLOCK) void k_intern_i64_lookup(int64_t n,
        const uint4* tab, int32_t* out_kid, const uint32_t* fresh_seq,
        uint32_t seq, uint32_t* dbg) {
    /* phase 3: resolve each ~slot stashed by the claim phase to its id */
    if (*fresh_seq != seq) return; /* claim resolved every row */
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const int32_t v = out_kid[i];
        if (v >= 0) continue; /* resolved by the claim phase: final */
        const uint32_t cand = ((const uint32_t*)&tab[(uint32_t)~v])[2];
        int32_t id = 0;
        if (cand == ~0u) dbg[3] = 5; /* capacity overflow: unassigned */
        else id = (int32_t)cand;
        out_kid[i] = id;
    }
}

void launch_intern_i64(hipStream_t s, const int64_t* d_keys, int64_t n,
                       uint4* tab, uint32_t p_mask, int64_t* ikeys,
                       uint32_t* ctrs, uint32_t id_cap, int32_t* out_kid,
                       uint32_t seq, uint64_t fp_mask, uint32_t* dbg) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    const uint32_t n_slots = p_mask + 2; /* the table + the key-0 cell */
    int sblocks = (int)std::min<uint32_t>((n_slots + BLOCK - 1) / BLOCK, 2048);
    uint32_t* fresh_seq = ctrs + 2;
    hipLaunchKernelGGL(k_intern_i64_claim, dim3(blocks), dim3(BLOCK), 0, s,
                       d_keys, n, tab, p_mask, fp_mask, out_kid, fresh_seq,
                       seq, dbg);
    hipLaunchKernelGGL(k_intern_i64_assign, dim3(sblocks), dim3(BLOCK), 0, s,
                       tab, n_slots, ikeys, ctrs, id_cap, fresh_seq, seq, dbg);
    hipLaunchKernelGGL(k_intern_i64_lookup, dim3(blocks), dim3(BLOCK), 0, s,
                       n, tab, out_kid, fresh_seq, seq, dbg);
}

/* synthetic utf8 key generator: "sensor_{k}" with k from the SAME splitmix
 * draw as the dense generator (spec in DESIGN.md §Generator) — lengths
 * first (host cumsums them into offsets), then the bytes */
__device__ __forceinline__ int32_t dec_digits(uint64_t k) {
    int32_t d = 1;
    while (k >= 10) { k /= 10; d++; }
    return d;
}

__global__ void k_gen_keylens(uint64_t seed, int64_t start_row, int64_t n,
                              int64_t nkeys, int32_t* lens) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        uint64_t r = splitmix64(seed ^ (0x9e3779b97f4a7c15ULL *
                                        (uint64_t)(start_row + i + 1)));
        lens[i] = 7 + dec_digits(r % (uint64_t)nkeys);
    }
}

__global__ void k_gen_keyfill(uint64_t seed, int64_t start_row, int64_t n,
                              int64_t nkeys, const int32_t* offs, char* data) {
    const char* pfx = "sensor_";
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        uint64_t r = splitmix64(seed ^ (0x9e3779b97f4a7c15ULL *
                                        (uint64_t)(start_row + i + 1)));
        uint64_t k = r % (uint64_t)nkeys;
        char* p = data + offs[i];
        for (int j = 0; j < 7; j++) p[j] = pfx[j];
        int32_t len = offs[i + 1] - offs[i];
        for (int32_t j = len - 1; j >= 7; j--) {
            p[j] = (char)('0' + (k % 10));
            k /= 10;
        }
    }
}

void launch_gen_utf8(hipStream_t s, uint64_t seed, int64_t start_row, int64_t n,
                     int64_t nkeys, int32_t* d_lens, const int32_t* d_offs,
                     char* d_data) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    if (d_lens)
        hipLaunchKernelGGL(k_gen_keylens, dim3(blocks), dim3(BLOCK), 0, s, seed,
                           start_row, n, nkeys, d_lens);
    if (d_data)
        hipLaunchKernelGGL(k_gen_keyfill, dim3(blocks), dim3(BLOCK), 0, s, seed,
                           start_row, n, nkeys, d_offs, d_data);
}

/* ------------------------------------------------------------------ */
/* batch min/max ts + max kid                                          */
/* ------------------------------------------------------------------ */

__device__ __forceinline__ uint64_t map_i64(int64_t x) {
    return (uint64_t)x ^ 0x8000000000000000ULL; /* order-preserving i64->u64 */
}

__global__ __launch_bounds__(BLOCK) void k_minmax(const int64_t* ts,
        const int32_t* kid, int64_t n, uint64_t* scalars) {
    __shared__ uint64_t red[3][WAVES_PER_BLOCK];
    uint64_t mn = ~0ULL, mx = 0, km = 0;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
        uint64_t t = map_i64(ts[i]);
        mn = min(mn, t);
        mx = max(mx, t);
        if (kid) km = max(km, (uint64_t)(uint32_t)kid[i]);
    }
    /* wave reduce */
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (uint64_t)__shfl_down((unsigned long long)mn, o));
        mx = max(mx, (uint64_t)__shfl_down((unsigned long long)mx, o));
        km = max(km, (uint64_t)__shfl_down((unsigned long long)km, o));
    }
    /* block reduce: one atomic triple per block (device atomics are ~10ns
     * each serialised on a word — keep their count per launch small) */
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        red[0][wave] = mn;
        red[1][wave] = mx;
        red[2][wave] = km;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < WAVES_PER_BLOCK; w++) {
            mn = min(mn, red[0][w]);
            mx = max(mx, red[1][w]);
            km = max(km, red[2][w]);
        }
        atomicMin((unsigned long long*)&scalars[0], (unsigned long long)mn);
        atomicMax((unsigned long long*)&scalars[1], (unsigned long long)mx);
        atomicMax((unsigned long long*)&scalars[2], (unsigned long long)km);
    }
}

void launch_minmax(hipStream_t s, const int64_t* d_ts, const int32_t* d_kid,
                   int64_t n, uint64_t* d_scalars) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 512);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_minmax, dim3(blocks), dim3(BLOCK), 0, s, d_ts, d_kid, n,
                       d_scalars);
}

/* ------------------------------------------------------------------ */
/* histogram                                                           */
/* ------------------------------------------------------------------ */

__global__ __launch_bounds__(BLOCK) void k_hist(const int32_t* kid,
        const int64_t* ts, int64_t n, int64_t chunk, WinParams wp,
        uint32_t* ghist, uint64_t* scalars) {
    /* bucket histogram; when `scalars` is non-null this launch ALSO reduces
     * the batch min/max timestamp + max key id (the tumbling fast path fuses
     * the watermark pass: one 12 B/row read instead of two). Tumbling rows
     * have multiplicity 1, so ts is only read when reducing or sliding. */
    __shared__ uint32_t h[NB];
    __shared__ uint64_t red[3][WAVES_PER_BLOCK];
    for (int t = threadIdx.x; t < NB; t += BLOCK) h[t] = 0;
    __syncthreads();
    int64_t lo = blockIdx.x * chunk;
    int64_t hi = i64min(n, lo + chunk);
    uint64_t mn = ~0ULL, mx = 0, km = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
        uint32_t k = (uint32_t)kid[i];
        uint32_t m = 1;
        if (wp.is_sliding) {
            int32_t jm, mm;
            row_windows(ts[i], wp, &jm, &mm);
            m = (uint32_t)mm;
        }
        if (scalars) {
            uint64_t t = map_i64(ts[i]);
            mn = min(mn, t);
            mx = max(mx, t);
            km = max(km, (uint64_t)k);
        }
        if (m) atomicAdd(&h[k & (NB - 1)], m);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < NB; t += BLOCK)
        ghist[(int64_t)blockIdx.x * NB + t] = h[t];
    if (scalars) {
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (uint64_t)__shfl_down((unsigned long long)mn, o));
            mx = max(mx, (uint64_t)__shfl_down((unsigned long long)mx, o));
            km = max(km, (uint64_t)__shfl_down((unsigned long long)km, o));
        }
        const int wave = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) {
            red[0][wave] = mn;
            red[1][wave] = mx;
            red[2][wave] = km;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < WAVES_PER_BLOCK; w++) {
                mn = min(mn, red[0][w]);
                mx = max(mx, red[1][w]);
                km = max(km, red[2][w]);
            }
            atomicMin((unsigned long long*)&scalars[0], (unsigned long long)mn);
            atomicMax((unsigned long long*)&scalars[1], (unsigned long long)mx);
            atomicMax((unsigned long long*)&scalars[2], (unsigned long long)km);
        }
    }
}

void launch_hist(hipStream_t s, const int32_t* d_kid, const int64_t* d_ts,
                 int64_t n, int64_t chunk, int C, const WinParams& wp,
                 uint32_t* d_ghist, uint64_t* d_scalars) {
    hipLaunchKernelGGL(k_hist, dim3(C), dim3(BLOCK), 0, s, d_kid, d_ts, n, chunk,
                       wp, d_ghist, d_scalars);
}

/* ------------------------------------------------------------------ */
/* scans: bucket totals -> bases; per-chunk stable offsets             */
/* ------------------------------------------------------------------ */

/* Two-level scan over the [C chunks][NB buckets] histogram matrix:
 * SSPLIT chunk-segments give 512+ blocks of parallelism at every stage. */
constexpr int SSPLIT = SCAN_SSPLIT;

/* partial per-segment bucket sums: psum[s][bkt] = sum of ghist over segment s */
__global__ void k_scan_partial(const uint32_t* ghist, int C, int cs,
                               uint32_t* psum) {
    int bkt = blockIdx.x * blockDim.x + threadIdx.x;
    int seg = blockIdx.y;
    if (bkt >= NB) return;
    int c0 = seg * cs, c1 = min(C, c0 + cs);
    uint32_t s = 0;
    for (int c = c0; c < c1; c++) s += ghist[(int64_t)c * NB + bkt];
    psum[(int64_t)seg * NB + bkt] = s;
}

/* single block: bucket totals from psum + exclusive scan -> base[NB+1] */
__global__ __launch_bounds__(NB) void k_scan_base(const uint32_t* psum,
                                                  uint32_t* base) {
    __shared__ uint32_t part[NB];
    const int bkt = threadIdx.x;
    uint32_t t = 0;
    for (int g = 0; g < SSPLIT; g++) t += psum[(int64_t)g * NB + bkt];
    part[bkt] = t;
    __syncthreads();
    /* Hillis-Steele inclusive scan over NB partials */
    for (int o = 1; o < NB; o <<= 1) {
        uint32_t v = (bkt >= o) ? part[bkt - o] : 0;
        __syncthreads();
        part[bkt] += v;
        __syncthreads();
    }
    base[bkt] = bkt ? part[bkt - 1] : 0;
    if (bkt == NB - 1) base[NB] = part[NB - 1];
}

/* per-chunk running offsets within each segment:
 * gofs[c][bkt] = base[bkt] + psum[<seg][bkt] + ghist[[c0,c)][bkt] */
__global__ void k_scan_offsets(const uint32_t* ghist, int C, int cs,
                               const uint32_t* psum, const uint32_t* base,
                               uint32_t* gofs) {
    int bkt = blockIdx.x * blockDim.x + threadIdx.x;
    int seg = blockIdx.y;
    if (bkt >= NB) return;
    uint32_t run = base[bkt];
    for (int g = 0; g < seg; g++) run += psum[(int64_t)g * NB + bkt];
    int c0 = seg * cs, c1 = min(C, c0 + cs);
    for (int c = c0; c < c1; c++) {
        uint32_t t = ghist[(int64_t)c * NB + bkt];
        gofs[(int64_t)c * NB + bkt] = run;
        run += t;
    }
}

void launch_scan(hipStream_t s, const uint32_t* d_ghist, int C,
                 uint32_t* d_psum, uint32_t* d_base, uint32_t* d_gofs) {
    int cs = (C + SSPLIT - 1) / SSPLIT;
    hipLaunchKernelGGL(k_scan_partial, dim3(NB / 256, SSPLIT), dim3(256), 0, s,
                       d_ghist, C, cs, d_psum);
    hipLaunchKernelGGL(k_scan_base, dim3(1), dim3(NB), 0, s, d_psum, d_base);
    hipLaunchKernelGGL(k_scan_offsets, dim3(NB / 256, SSPLIT), dim3(256), 0, s,
                       d_ghist, C, cs, d_psum, d_base, d_gofs);
}

/* ------------------------------------------------------------------ */
/* stable scatter                                                      */
/* ------------------------------------------------------------------ */

/* inclusive scan of one value per lane over the wave, in registers */
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, o);
        if (lane >= o) v += u;
    }
    return v;
}

/* exclusive prefix of one partial per thread over the block, and the block
 * total: a wave scan plus the four wave totals through wtot[] — ONE block
 * barrier (the Hillis-Steele form through LDS took 17). wtot[] must not be
 * written again before another barrier has passed. */
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t s, uint32_t* wtot,
                                                    uint32_t* total) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t incl = wave_scan_incl(s, lane);
    if (lane == 63) wtot[wave] = incl;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
        const uint32_t t = wtot[w];
        if (w < wave) pre += t;
        tot += t;
    }
    *total = tot;
    return pre + incl - s;
}

/* rows (scatter) or records (regroup) one lane holds per supertile: a wave's
 * quarter is at most ST_RECORDS / 4 = 512 = 8 lane-strided iterations */
constexpr int ST_SLOTS = ST_RECORDS / BLOCK;

/* wave-quarter bounds of the supertile [st0, st1) (contiguous: wave order ==
 * row order) */
template <typename T>
__device__ __forceinline__ void wave_quarter(T st0, T st1, int wave, T* w0,
                                             T* w1) {
    const T q = ((st1 - st0) + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    *w0 = st0 + wave * q < st1 ? st0 + wave * q : st1;
    *w1 = *w0 + q < st1 ? *w0 + q : st1;
}

/* rows per supertile: ST_RECORDS, or the launch's st_rows when rows expand */
__device__ __forceinline__ constexpr int64_t st_rows_of() { return ST_RECORDS; }
__device__ __forceinline__ int64_t st_rows_of(int32_t st_rows) { return st_rows; }

template <bool MULT, typename... SR>
__global__ __launch_bounds__(BLOCK) void k_scatter_t(const int32_t* kid,
        const int64_t* ts, const double* vals, const uint8_t* validity,
        int64_t n, int64_t chunk, WinParams wp, const uint32_t* gofs,
        uint4* grec, uint32_t rec_limit, uint32_t* dbg, SR... sr) {
    /* LDS-staged stable partition. Each wave owns a CONTIGUOUS QUARTER of the
     * supertile (wave order == row order), so staging cursors are per-wave
     * private: no cross-wave serialization. Per supertile: wave-quarter
     * counts, bin prefix, ranked placement into LDS, bucket-major flush, so
     * adjacent lanes write adjacent global addresses (the direct form measured
     * 6x write amplification — profiles/hbm_traffic.json). Each row's kid,
     * ts, value and validity bit are read ONCE, into ST_SLOTS register slots
     * per lane, counted and placed from there; the loads of supertile s+1 are
     * issued before supertile s is counted, so their latency runs under its
     * whole chain; and the chain is 4 block barriers (count | wave totals |
     * cursors | placement): the chunk's global cursors live in their owner
     * thread's registers, and each wave re-zeroes its own count row, which
     * nobody else reads until the next prefix.
     * MULT == false is the plain tumbling batch: every row lands in exactly
     * one window, supertiles of ST_RECORDS rows. MULT == true (sliding and
     * window-subrange launches) gives a row a multiplicity m of 0..expand-1:
     * the supertile is st_rows rows (a launch argument that exists only
     * here, so that st_rows * expand records fit the staging), a row counts
     * m, ranks by the m of the lower lanes of its bucket, and stages m
     * records with widx = jmin + jj. Nothing else differs, every difference
     * is an if constexpr, and record order — so every destination in grec —
     * is the same in both: bucket, then row, then window. */
    static_assert(sizeof...(SR) == (MULT ? 1 : 0),
                  "st_rows is passed exactly when MULT");
    __shared__ uint32_t cnt4[WAVES_PER_BLOCK][NB]; /* per-wave-quarter counts,
                                     * converted IN PLACE to per-wave staging
                                     * cursors by the prefix */
    __shared__ uint32_t offs[NB];   /* per-supertile exclusive bin prefix     */
    __shared__ uint32_t dbase[NB];  /* global cursor - offs: dest = dbase + p */
    __shared__ uint4 s_rec[ST_RECORDS];
    __shared__ uint32_t s_wtot[WAVES_PER_BLOCK];
    auto wofs = cnt4;
    constexpr int PER = NB / BLOCK;
    constexpr uint32_t SENT = 0xFFFFFFFFu;

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t lo = blockIdx.x * chunk;
    const int64_t hi = i64min(n, lo + chunk);
    if (lo >= hi) return;
    uint32_t cur[PER]; /* global cursors of this thread's PER bins */
#pragma unroll
    for (int j = 0; j < PER; j++)
        cur[j] = gofs[(int64_t)blockIdx.x * NB + threadIdx.x * PER + j];
    for (int t = lane; t < NB; t += 64) cnt4[wave][t] = 0;
    const int64_t st_rows = st_rows_of(sr...);
    /* MULT is single-buffered: with the next supertile's rows held beside
     * this one's it needs 172 VGPRs, over the 168 that 3 waves/SIMD allow, so
     * it loads each supertile where it takes it over (as NX >= 2 does in
     * k_regroup_t), and only the slots its wave quarter reaches */
    constexpr bool PREFETCH = !MULT;

    /* the supertile's rows as loaded; rows past the quarter's end re-read the
     * chunk's last row (always in bounds) and are masked out below */
    int32_t n_kid[ST_SLOTS];
    int64_t n_ts[ST_SLOTS];
    double n_val[ST_SLOTS];
    uint32_t n_vb[ST_SLOTS];
    auto load_rows = [&](int64_t st0) {
        int64_t w0, w1;
        wave_quarter(st0, i64min(hi, st0 + st_rows), wave, &w0, &w1);
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++) {
            if constexpr (MULT) {
                if (w0 + k * 64 >= w1) break; /* wave-uniform */
            }
            const int64_t i = i64min(w0 + k * 64 + lane, hi - 1);
            n_kid[k] = kid[i];
            n_ts[k] = ts[i];
            n_val[k] = vals[i];
            n_vb[k] = validity ? (uint32_t)validity[i >> 3] : 0xFFu;
        }
    };
    if constexpr (PREFETCH) load_rows(lo);

    for (int64_t st0 = lo; st0 < hi; st0 += st_rows) {
        if constexpr (!PREFETCH) load_rows(st0);
        int64_t w0, w1;
        wave_quarter(st0, i64min(hi, st0 + st_rows), wave, &w0, &w1);
        /* this supertile's rows: bucket (SENT = no row), meta word (of the
         * row's first window), value; MULT: the row's window count */
        uint32_t bk[ST_SLOTS], meta[ST_SLOTS];
        uint64_t vb[ST_SLOTS];
        [[maybe_unused]] uint32_t mult[ST_SLOTS];
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++) {
            if constexpr (MULT) {
                mult[k] = 0;
                if (w0 + k * 64 >= w1) continue; /* wave-uniform: not loaded */
            }
            const int64_t i = w0 + k * 64 + lane;
            const uint32_t kv = (uint32_t)n_kid[k];
            const uint32_t valid = (n_vb[k] >> (i & 7)) & 1u;
            int32_t jmin, m;
            row_windows(n_ts[k], wp, &jmin, &m);
            bk[k] = i < w1 ? (kv & (NB - 1)) : SENT;
            meta[k] = (kv >> LOG_NB) | ((uint32_t)jmin << META_WIDX_SHIFT)
                    | (valid << META_VALID_SHIFT);
            vb[k] = (uint64_t)__double_as_longlong(n_val[k]);
            if constexpr (MULT) mult[k] = i < w1 ? (uint32_t)m : 0u;
        }
        if constexpr (PREFETCH) {
            if (st0 + st_rows < hi) load_rows(st0 + st_rows);
        }
        /* counts per (wave, bucket), from registers */
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++) {
            if constexpr (MULT) {
                if (mult[k]) atomicAdd(&cnt4[wave][bk[k]], mult[k]);
            } else {
                if (bk[k] != SENT) atomicAdd(&cnt4[wave][bk[k]], 1u);
            }
        }
        __syncthreads();
        /* per-supertile prefix: offs (bin-major) + per-wave staging bases */
        uint32_t tot;
        {
            uint32_t excl[PER];
            uint32_t s = 0;
#pragma unroll
            for (int j = 0; j < PER; j++) {
                const int b = threadIdx.x * PER + j;
                uint32_t t = 0;
                for (int w = 0; w < WAVES_PER_BLOCK; w++) t += cnt4[w][b];
                excl[j] = s;
                s += t;
            }
            const uint32_t pre = block_scan_excl(s, s_wtot, &tot);
#pragma unroll
            for (int j = 0; j < PER; j++) {
                const int b = threadIdx.x * PER + j;
                uint32_t run = pre + excl[j];
                offs[b] = run;
                dbase[b] = cur[j] - run;
                for (int w = 0; w < WAVES_PER_BLOCK; w++) {
                    const uint32_t c = cnt4[w][b];
                    wofs[w][b] = run; /* overlays cnt4 */
                    run += c;
                }
                cur[j] += run - (pre + excl[j]); /* the bin's total */
            }
        }
        __syncthreads();
        /* ranked placement from registers, PER-WAVE private cursors, in the
         * row order the counts were taken in */
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++) {
            if (w0 + k * 64 >= w1) break; /* wave-uniform */
            const uint32_t bkt = bk[k];
            /* among the wave step's rows of this bucket: r = records of the
             * lower lanes, wtot = records of all, fl = the lowest lane */
            uint32_t r, wtot;
            int fl;
            if constexpr (MULT) {
                /* weighted by each row's window count */
                r = 0, wtot = 0, fl = lane;
                for (int j = 0; j < 64; j++) {
                    const uint32_t bj =
                        (uint32_t)__builtin_amdgcn_readlane((int)bkt, j);
                    const uint32_t mj =
                        (uint32_t)__builtin_amdgcn_readlane((int)mult[k], j);
                    if (bj == bkt) {
                        if (j < lane) r += mj;
                        wtot += mj;
                        if (j < fl) fl = j;
                    }
                }
            } else {
                /* bit-ballot same-bucket mask (9+1 bits incl SENT) */
                uint64_t same = ~0ULL;
                for (int b = 0; b < 9; b++) {
                    uint64_t bb = __ballot((bkt >> b) & 1);
                    same &= ((bkt >> b) & 1) ? bb : ~bb;
                }
                {
                    uint64_t bb = __ballot(bkt == SENT);
                    same &= (bkt == SENT) ? bb : ~bb;
                }
                const uint64_t below =
                    (lane == 63) ? ~0ULL : ((1ULL << (lane + 1)) - 1);
                r = (uint32_t)__popcll(same & below) - 1;
                wtot = (uint32_t)__popcll(same);
                fl = __ffsll((unsigned long long)same) - 1;
            }
            /* the lowest lane claims the step's records of the bucket */
            uint32_t pre = 0;
            if (lane == fl && bkt != SENT) {
                pre = wofs[wave][bkt];
                wofs[wave][bkt] = pre + wtot;
            }
            pre = (uint32_t)__shfl((int)pre, fl);
            if constexpr (MULT) {
                for (uint32_t jj = 0; jj < mult[k]; jj++)
                    s_rec[pre + r + jj] = make_uint4(
                        (uint32_t)vb[k], (uint32_t)(vb[k] >> 32),
                        (uint32_t)(w0 + k * 64 + lane),
                        meta[k] + (jj << META_WIDX_SHIFT)); /* jmin + jj */
            } else {
                if (bkt != SENT)
                    s_rec[pre + r] = make_uint4(
                        (uint32_t)vb[k], (uint32_t)(vb[k] >> 32),
                        (uint32_t)(w0 + k * 64 + lane), meta[k]);
            }
        }
        /* own count row back to zero for the next supertile (only this wave
         * touches it until the next prefix, two barriers on) */
        for (int t = lane; t < NB; t += 64) cnt4[wave][t] = 0;
        __syncthreads();
        /* flush: bucket-major staging => coalesced run writes; the record's
         * bin (and so its destination) falls out of a binary search over
         * the bin prefix. No barrier after it: nothing it reads is written
         * again before the next supertile's first barrier. */
        for (uint32_t p = threadIdx.x; p < tot; p += BLOCK) {
            uint32_t b = 0;
            for (int stp = NB >> 1; stp; stp >>= 1)
                if (b + stp < NB && offs[b + stp] <= p) b += stp;
            const uint32_t d = dbase[b] + p;
            if (d < rec_limit) grec[d] = s_rec[p];
            else dbg[0] = 1; /* bounds guard: flag, never corrupt */
        }
    }
}

void launch_scatter(hipStream_t s, const int32_t* d_kid, const int64_t* d_ts,
                    const double* d_vals, const uint8_t* d_validity, int64_t n,
                    int64_t chunk, int C, int32_t st_rows, const WinParams& wp,
                    const uint32_t* d_gofs, uint4* d_grec, uint32_t rec_limit,
                    uint32_t* d_dbg) {
    if (!wp.is_sliding) {
        assert(st_rows == ST_RECORDS); /* no expansion without sliding */
        hipLaunchKernelGGL(k_scatter_t<false>, dim3(C), dim3(BLOCK), 0, s,
                           d_kid, d_ts, d_vals, d_validity, n, chunk, wp,
                           d_gofs, d_grec, rec_limit, d_dbg);
    } else {
        hipLaunchKernelGGL((k_scatter_t<true, int32_t>), dim3(C), dim3(BLOCK),
                           0, s, d_kid, d_ts, d_vals, d_validity, n, chunk, wp,
                           d_gofs, d_grec, rec_limit, d_dbg, st_rows);
    }
}

/* ------------------------------------------------------------------ */
/* regroup — one wave per bucket: stable wave-local split of the       */
/* bucket's records into per-(window,key) GROUP segments               */
/* (val 8B + rowidx/valid 4B), so the fold can walk each group's rows  */
/* sequentially. Two passes over the bucket region (second is L2-hot): */
/* count bins (LDS atomics), exclusive prefix, then ranked placement   */
/* (bit-ballot same-group masks + LDS cursors; ranks are row-ordered). */
/* ------------------------------------------------------------------ */

constexpr int GCAP = FOLD_GCAP; /* bins (groups) per bucket per chunk */

/* One templated stable-split kernel, four modes:
 *  DIRECT_FOLD (gtot <= GCAP per chunk): bins = (widx,kloc) groups; each
 *     supertile's LDS-staged bins fold DIRECTLY into per-bin register
 *     accumulators (one thread owns one bin), seeded from / written back to
 *     the persistent window-slot slab. No reordered records ever touch HBM:
 *     the unfused form measured 324 MB regroup write + 159 MB fold read per
 *     8M-row cfg2 launch (profiles/hbm_traffic.json) — pure materialization
 *     round-trip, all of it gone here. Row-order folding is preserved:
 *     supertiles advance in row order and staged records within a bin are
 *     ranked in row order, so each bin's accumulator sees its rows in
 *     exactly the reference's update_batch order (bit-exact f64 sum).
 *  L1 (two-level, first pass): bins = (kloc>>8, widx) <= 256, output FULL
 *     16 B records (meta travels to L2)
 *  L2_FOLD (two-level, second pass): one block per (bucket, bin1) segment
 *     of the L1 output; bins = kloc & 255, folded like DIRECT_FOLD
 * Structure (shared): per-supertile ranked placement (wave-quarters: wave
 * order == row order, private cursors, bit-ballot same-bin masks) into LDS
 * staging; L1 flushes bin-major so writes coalesce, fold modes consume the
 * staging in place. */
enum { RG_L1 = 1, RG_DIRECT_FOLD = 3, RG_L2_FOLD = 4 };

/* One Welford update of the variance family's (mean, m2) state; n is the
 * group's valid-row count INCLUDING this row. Every operation is rounded on
 * its own — the reference accumulator is plain Rust f64 arithmetic, and a
 * fused m2 + d1*d2 differs from it in the last bit — so contraction is
 * switched off for this body (hipcc contracts by default). */
__device__ __forceinline__ void welford_step(double v, uint64_t n,
                                             double& mean, double& m2) {
#pragma clang fp contract(off)
    const double d1 = v - mean;
    const double nmean = d1 / (double)n + mean;
    const double d2 = v - nmean;
    m2 = m2 + d1 * d2;
    mean = nmean;
}

/* VAR: the fold also carries the variance family's (mean, m2) accumulators,
 * persisted in the side slab v_base ([slot][{mean,m2}][kcap] f64). VAR=false
 * compiles to the kernels without them (v_base/vslab_cells unused).
 * NX: extra value columns (0..3) of a multi-column op. The fold gathers each
 * extra's value (and validity bit) by the record's batch row index and keeps
 * {cnt, min, max, sum} per extra in registers, persisted in the side slab
 * fx.slab ([slot][col][{cnt,min,max,sum}][kcap], same (slot, kloc, bucket)
 * cell as the main slab, bounds-guarded through dbg[1]). The FoldExtras
 * argument exists only when NX > 0 (the trailing pack is empty otherwise), so
 * the NX=0 kernels keep their argument block and compile to the code they
 * were before extras existed.
 * IV: the value column is int64 (dz_window_op_set_value_type). The records
 * carry the value as 8 opaque bytes either way; here the walk reads them as
 * int64_t and keeps min/max (signed compare) and sum (wrapping add, on
 * uint64_t) as integers, stored bit for bit in the s_min/s_max/s_sum cells,
 * plus one f64 running sum of (double)v in row order for avg — the
 * reference's cast-then-average. VAR steps Welford on (double)v. The side slab
 * of an int op is [slot][{fsum, mean, m2}][kcap] with VAR and [slot][{fsum}]
 * [kcap] without; fsum is read only behind cnt > 0 like its neighbours, so a
 * recycled slot's stale cell never surfaces and no reset touches it. NX == 0
 * only. IV=false adds no variable and no statement: every branch on it is an
 * if constexpr, and the f64 kernels compile to the code they were. */
__device__ __forceinline__ const FoldExtras& pick_fx(const FoldExtras& f) {
    return f;
}
/* per-extra register accumulators; no members at all when NX == 0 */
template <int N>
struct XAcc {
    uint64_t cnt[N];
    double mn[N], mx[N], sm[N];
};
template <>
struct XAcc<0> {};

template <int MODE, bool VAR = false, int NX = 0, bool IV = false,
          typename... XA>
__global__ __launch_bounds__(BLOCK) void k_regroup_t(const uint4* rrec,
        const uint32_t* bucket_base, FoldChunk fc,
        const uint32_t* b1offs, const uint32_t* b1lens, uint32_t* binoffs,
        uint32_t* binlens, uint4* orec,
        const int32_t* slot_of_widx, uint64_t* s_cnt, double* s_min,
        double* s_max, double* s_sum, uint64_t* s_first, int64_t slab_cells,
        uint32_t* dbg, double* v_base, int64_t vslab_cells, XA... xa) {
    static_assert(sizeof...(XA) == (NX > 0 ? 1 : 0),
                  "FoldExtras is passed exactly when NX > 0");
    static_assert(!VAR || MODE == RG_DIRECT_FOLD || MODE == RG_L2_FOLD,
                  "only the fold modes carry variance state");
    static_assert(NX >= 0 && NX <= MAX_EXTRA_COLS &&
                  (NX == 0 || (!VAR && MODE != RG_L1)),
                  "extras ride the fold modes, without variance state");
    static_assert(!IV || (NX == 0 && MODE != RG_L1),
                  "int64 values ride the fold modes, single-column");
    constexpr bool FOLD = (MODE == RG_DIRECT_FOLD || MODE == RG_L2_FOLD);
    __shared__ uint32_t cnt[GCAP];    /* whole-segment bin counts (L1) */
    __shared__ uint32_t gcur[GCAP];   /* segment-region bin cursors (L1) */
    __shared__ uint32_t stcnt4[WAVES_PER_BLOCK][GCAP]; /* per-wave-quarter */
    __shared__ uint32_t stoffs[GCAP]; /* per-supertile bin prefix */
    __shared__ uint32_t wcur[WAVES_PER_BLOCK][GCAP];   /* per-wave cursors */
    __shared__ uint32_t s_dest[ST_RECORDS]; /* RG_L1 only */
    __shared__ uint4 s_rec[ST_RECORDS];     /* meta travels in .w */
    __shared__ uint32_t s_wtot[WAVES_PER_BLOCK];
    static_assert(GCAP == BLOCK, "parallel bin prefix maps one thread per bin");

    const int bkt = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t bklo = bucket_base[bkt];
    uint32_t lo = bklo, hi = bucket_base[bkt + 1];
    const int nk = fc.k_hi - fc.k_lo;
    int nbins, obase = 0;
    if (MODE == RG_DIRECT_FOLD) {
        nbins = (fc.w_hi - fc.w_lo) * nk;
    } else if (MODE == RG_L1) {
        nbins = ((nk + 255) >> 8) * fc.tl_nw;
        obase = bkt * 256;
    } else { /* RG_L2_FOLD */
        const int bin1 = blockIdx.y;
        nbins = 256;
        lo = bklo + b1offs[bkt * 256 + bin1];
        hi = lo + b1lens[bkt * 256 + bin1];
    }

    auto bin_of = [&](uint32_t ms_) -> uint32_t {
        const int widx = (int)((ms_ >> META_WIDX_SHIFT) & META_WIDX_MASK);
        const int kloc = (int)(ms_ & META_KLOC_MASK);
        if (MODE == RG_DIRECT_FOLD) {
            if (widx < fc.w_lo || widx >= fc.w_hi || kloc < fc.k_lo ||
                kloc >= fc.k_hi)
                return 0x1FFu; /* outside this chunk */
            return (uint32_t)((widx - fc.w_lo) * nk + (kloc - fc.k_lo));
        } else if (MODE == RG_L1) {
            return (uint32_t)((kloc >> 8) * fc.tl_nw + widx);
        } else {
            return (uint32_t)(kloc & 255);
        }
    };

    /* fold modes: thread t owns bin t — accumulator lives in registers,
     * seeded LAZILY from the persistent slab at the bin's first record and
     * written back only if touched: untouched bins cost ZERO state traffic.
     * (Eager seed/writeback of every bin measured ~1 KB/row of pure state
     * traffic on cfg3's sliding 1M-key workload, where each launch covers
     * many windows whose key slots are mostly absent from the batch.) */
    int64_t f_sidx = 0;
    bool f_own = false, f_loaded = false;
    uint64_t f_cnt = 0, f_fst = ~0ULL;
    double f_mn = 0.0, f_mx = 0.0, f_sm = 0.0;
    int64_t f_vidx = 0;               /* VAR: side-slab cell of `mean` */
    double f_mean = 0.0, f_m2 = 0.0;  /* VAR: Welford state */
    /* IV: integer min/max/sum and the f64 sum of (double)v; f_vidx is then
     * the side-slab cell of fsum, with mean and m2 (VAR) kcap and 2 kcap
     * cells behind it */
    [[maybe_unused]] int64_t i_mn = 0, i_mx = 0;
    [[maybe_unused]] uint64_t i_sm = 0;
    [[maybe_unused]] double f_fs = 0.0;
    constexpr int IVF = VAR ? 3 : 1; /* IV: side-slab fields per slot */
    [[maybe_unused]] int64_t f_xidx = 0; /* NX: side-slab cell of extra 0's cnt */
    [[maybe_unused]] XAcc<NX> x;         /* NX: per-extra accumulators */
    if constexpr (NX > 0) {
#pragma unroll
        for (int c = 0; c < NX; c++) {
            x.cnt[c] = 0;
            x.mn[c] = x.mx[c] = x.sm[c] = 0.0;
        }
    }
    if (FOLD) {
        const int g = threadIdx.x;
        int my_widx = 0, my_kloc = 0;
        if (MODE == RG_DIRECT_FOLD) {
            f_own = g < nbins;
            my_widx = fc.w_lo + (f_own ? g / nk : 0);
            my_kloc = fc.k_lo + (f_own ? g % nk : 0);
        } else { /* RG_L2_FOLD: bin1 = (kloc>>8)*nw + widx; bin = kloc&255 */
            const int bin1 = blockIdx.y;
            my_widx = bin1 % fc.tl_nw;
            my_kloc = (bin1 / fc.tl_nw) * 256 + g;
            f_own = my_kloc < nk && my_widx < fc.w_hi;
        }
        if (f_own) {
            int64_t slot = slot_of_widx[my_widx];
            f_sidx = slot * (5 * fc.kcap) + (((int64_t)my_kloc << LOG_NB) | bkt);
            if (slot < 0 || f_sidx < 0 || f_sidx + 4 * fc.kcap >= slab_cells) {
                dbg[1] = 1; /* bounds guard: disown, never corrupt */
                f_own = false;
            }
            if constexpr (IV) {
                f_vidx = slot * ((int64_t)IVF * fc.kcap) +
                         (((int64_t)my_kloc << LOG_NB) | bkt);
                if (slot < 0 || f_vidx < 0 ||
                    f_vidx + (int64_t)(IVF - 1) * fc.kcap >= vslab_cells) {
                    dbg[1] = 1;
                    f_own = false;
                }
            } else if (VAR) {
                /* same (slot, kloc, bucket) indexing, 2 fields per slot;
                 * m2 sits kcap cells after mean */
                f_vidx = slot * (2 * fc.kcap) +
                         (((int64_t)my_kloc << LOG_NB) | bkt);
                if (slot < 0 || f_vidx < 0 ||
                    f_vidx + fc.kcap >= vslab_cells) {
                    dbg[1] = 1;
                    f_own = false;
                }
            }
            if constexpr (NX > 0) {
                const FoldExtras& fx = pick_fx(xa...);
                /* same cell, 4 fields per extra: field f of extra c sits
                 * (4 * c + f) * kcap cells after f_xidx */
                f_xidx = slot * ((int64_t)(4 * NX) * fc.kcap) +
                         (((int64_t)my_kloc << LOG_NB) | bkt);
                if (slot < 0 || f_xidx < 0 ||
                    f_xidx + (int64_t)(4 * NX - 1) * fc.kcap >= fx.cells) {
                    dbg[1] = 1;
                    f_own = false;
                }
            }
        }
    }

    if (MODE == RG_L1) {
        for (int g = threadIdx.x; g < GCAP; g += BLOCK) cnt[g] = 0;
        __syncthreads();
        /* pass 1: whole-segment bin counts (meta rides in each record's
         * .w lane; the supertile passes below re-read the same lines out
         * of L2/MALL) */
        for (uint32_t i = lo + threadIdx.x; i < hi; i += BLOCK) {
            const uint32_t g = bin_of(rrec[i].w);
            if (g != 0x1FFu) atomicAdd(&cnt[g], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) { /* tiny exclusive prefix over <=GCAP bins */
            uint32_t run = 0;
            for (int g = 0; g < GCAP; g++) {
                uint32_t t = cnt[g];
                gcur[g] = run;
                run += t;
            }
        }
        __syncthreads();
        /* publish segment layout for the next stage (offsets are
         * relative to the BUCKET region start) */
        const uint32_t relbase = lo - bklo;
        for (int g = threadIdx.x; g < nbins; g += BLOCK) {
            binoffs[obase + g] = relbase + gcur[g];
            binlens[obase + g] = cnt[g];
        }
    }
    /* Per supertile each record is read ONCE, into ST_SLOTS register slots
     * per lane; bins are counted and records placed from those registers.
     * The next supertile's records are loaded (into nxt) before this one is
     * counted, so their latency runs under its whole chain. 4 block barriers
     * per supertile: count | wave totals | cursors | placement. Each wave
     * re-zeroes its own count row after placing (nobody else reads it until
     * the next prefix), and nothing read after the last barrier is written
     * again before the next supertile's first, so the fold walk (or the L1
     * flush) needs none behind it. */
    /* two or three extra columns' accumulators leave no room for the second
     * register set (179 and 195 VGPRs: past the 168 that 3 waves/SIMD
     * allow): those instantiations load each supertile where it is taken
     * over */
    /* so does the int64 direct fold with variance state (181 VGPRs with the
     * second set); its two-level sibling keeps it (149) */
    constexpr bool PREFETCH =
        NX < 2 && !(IV && VAR && MODE == RG_DIRECT_FOLD);
    /* staged records the fold walk reads ahead of their updates; the group
     * lives in the registers recs[]/bins[] vacate after placement, and the
     * gathered extras of NX >= 2 leave room for half a group */
    constexpr int WALK_G = NX < 2 ? 8 : 4;
    for (int g = lane; g < GCAP; g += 64) stcnt4[wave][g] = 0;
    uint4 nxt[ST_SLOTS];
    /* slots past the quarter's end re-read the segment's last record (always
     * in bounds) and are masked out when the set is taken over */
    auto load_recs = [&](uint32_t st0) {
        uint32_t w0, w1;
        wave_quarter<uint32_t>(st0, min(hi, st0 + (uint32_t)ST_RECORDS), wave,
                               &w0, &w1);
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++)
            nxt[k] = rrec[min(w0 + (uint32_t)(k * 64 + lane), hi - 1)];
    };
    if (PREFETCH && lo < hi) load_recs(lo);
    for (uint32_t st0 = lo; st0 < hi; st0 += ST_RECORDS) {
        uint32_t w0, w1;
        wave_quarter<uint32_t>(st0, min(hi, st0 + (uint32_t)ST_RECORDS), wave,
                               &w0, &w1);
        uint4 recs[ST_SLOTS];
        uint32_t bins[ST_SLOTS];
        if (!PREFETCH) load_recs(st0);
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++) {
            recs[k] = nxt[k];
            uint32_t g = 0x1FFu; /* sentinel above GCAP-1 */
            if (w0 + (uint32_t)(k * 64 + lane) < w1) g = bin_of(recs[k].w);
            /* fold records carry validity in bit 31; L1 passes the
             * raw rowidx through (meta stays in .w) */
            if (MODE != RG_L1 && g != 0x1FFu)
                recs[k].z |= (recs[k].w >> META_VALID_SHIFT) << 31;
            bins[k] = g;
        }
        if (PREFETCH && st0 + (uint32_t)ST_RECORDS < hi &&
            st0 + (uint32_t)ST_RECORDS > st0)
            load_recs(st0 + ST_RECORDS);
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++)
            if (bins[k] != 0x1FFu) atomicAdd(&stcnt4[wave][bins[k]], 1u);
        __syncthreads();
        /* parallel bin prefix (GCAP == BLOCK: one thread per bin) */
        uint32_t tg = 0, s_total;
        for (int w = 0; w < WAVES_PER_BLOCK; w++)
            tg += stcnt4[w][threadIdx.x];
        const uint32_t seg0 = block_scan_excl(tg, s_wtot, &s_total);
        {
            uint32_t run = seg0;
            stoffs[threadIdx.x] = run;
            for (int w = 0; w < WAVES_PER_BLOCK; w++) { /* per-wave bases */
                wcur[w][threadIdx.x] = run;
                run += stcnt4[w][threadIdx.x];
            }
        }
        __syncthreads();
        /* ranked placement into staging, per-wave private cursors */
#pragma unroll
        for (int k = 0; k < ST_SLOTS; k++) {
            if (w0 + (uint32_t)(k * 64) >= w1) break; /* wave-uniform */
            const uint32_t g = bins[k];
            const uint4 rec = recs[k];
            /* same-bin mask via bit-ballots over the 9 bin-id bits */
            uint64_t same = ~0ULL;
            for (int b = 0; b < 9; b++) {
                uint64_t bb = __ballot((g >> b) & 1);
                same &= ((g >> b) & 1) ? bb : ~bb;
            }
            const uint64_t below = (lane == 63) ? ~0ULL : ((1ULL << (lane + 1)) - 1);
            const int rank = (int)__popcll(same & below) - 1;
            const int leader = __ffsll((unsigned long long)same) - 1;
            const uint32_t wtot = (uint32_t)__popcll(same);
            uint32_t pos = 0;
            {
                uint32_t pre = 0;
                if (lane == leader && g != 0x1FFu) {
                    pre = wcur[wave][g];
                    wcur[wave][g] = pre + wtot;
                }
                pre = (uint32_t)__shfl((int)pre, leader);
                pos = pre + (uint32_t)rank;
            }
            if (g != 0x1FFu) {
                s_rec[pos] = rec;
                if (MODE == RG_L1)
                    s_dest[pos] = lo + gcur[g] + (pos - stoffs[g]);
            }
        }
        for (int g = lane; g < GCAP; g += 64) stcnt4[wave][g] = 0;
        __syncthreads();
        if (FOLD) {
            /* consume the staging in place: thread t folds bin t's staged
             * segment (row-ordered) into its register accumulator — the
             * reference's sequential update_batch order, no HBM round-trip */
            const uint32_t seg1 = seg0 + tg;
            if (f_own && seg1 > seg0) {
                if (!f_loaded) { /* lazy seed at the bin's first record */
                    f_loaded = true;
                    f_cnt = s_cnt[f_sidx];
                    f_fst = s_first[f_sidx];
                    if constexpr (IV) {
                        if (f_cnt > 0) {
                            i_mn = (int64_t)__double_as_longlong(s_min[f_sidx]);
                            i_mx = (int64_t)__double_as_longlong(s_max[f_sidx]);
                            i_sm = (uint64_t)__double_as_longlong(s_sum[f_sidx]);
                            f_fs = v_base[f_vidx];
                            if (VAR) {
                                f_mean = v_base[f_vidx + fc.kcap];
                                f_m2 = v_base[f_vidx + 2 * fc.kcap];
                            }
                        }
                    } else if (f_cnt > 0) {
                        f_mn = s_min[f_sidx];
                        f_mx = s_max[f_sidx];
                        f_sm = s_sum[f_sidx];
                        if (VAR) {
                            /* gated on cnt > 0 like min/max/sum: a recycled
                             * slot (cnt reset to 0) starts from (0, 0) in
                             * registers whatever the side slab still holds */
                            f_mean = v_base[f_vidx];
                            f_m2 = v_base[f_vidx + fc.kcap];
                        }
                    }
                    if constexpr (NX > 0) {
                        const FoldExtras& fx = pick_fx(xa...);
#pragma unroll
                        for (int c = 0; c < NX; c++) {
                            /* each extra has its own cnt: min/max/sum are
                             * read only behind it, so whatever a recycled
                             * slot still holds never surfaces */
                            const int64_t xi = f_xidx + (int64_t)(4 * c) * fc.kcap;
                            x.cnt[c] = fx.slab[xi];
                            if (x.cnt[c] > 0) {
                                x.mn[c] = __longlong_as_double(
                                    (long long)fx.slab[xi + fc.kcap]);
                                x.mx[c] = __longlong_as_double(
                                    (long long)fx.slab[xi + 2 * fc.kcap]);
                                x.sm[c] = __longlong_as_double(
                                    (long long)fx.slab[xi + 3 * fc.kcap]);
                            }
                        }
                    }
                }
                if (f_fst == ~0ULL)
                    f_fst = fc.row_base + (s_rec[seg0].z & 0x7FFFFFFFu);
                /* The walk, WALK_G records at a time. The lanes of a wave
                 * walk in lock step and a supertile's records sit in a few
                 * long segments, so a loop that reads one record, waits and
                 * updates pays the LDS round trip once per record of the
                 * longest segment. Here every read of the group (and every
                 * gather of an extra column) is issued before the first
                 * update; the updates then run strictly in record order.
                 * Only the 12 bytes the fold uses are read. The last group
                 * is the same code with its slots past seg1 clamped to the
                 * segment's last record and masked out: a scalar tail would
                 * cost the wave up to WALK_G - 1 round trips again. Null and
                 * masked records go through selects, so the body has no
                 * branch; the valid count runs in 32 bits (a supertile holds
                 * 2,048 records) and joins f_cnt behind the loop. */
                bool fresh = f_cnt == 0;
                uint32_t nv = 0;
                for (uint32_t r = seg0; r < seg1; r += WALK_G) {
                    uint2 gv[WALK_G];
                    uint32_t gz[WALK_G];
                    [[maybe_unused]] double gxv[WALK_G][NX > 0 ? NX : 1];
                    [[maybe_unused]] uint32_t gxb[WALK_G][NX > 0 ? NX : 1];
#pragma unroll
                    for (int i = 0; i < WALK_G; i++) {
                        const uint32_t q = min(r + (uint32_t)i, seg1 - 1);
                        gv[i] = *reinterpret_cast<const uint2*>(&s_rec[q]);
                        gz[i] = s_rec[q].z;
                    }
                    if constexpr (NX > 0) {
                        const FoldExtras& fx = pick_fx(xa...);
                        /* extras: gathered by batch row index (a masked
                         * slot re-reads the last record's row: in bounds) */
#pragma unroll
                        for (int i = 0; i < WALK_G; i++) {
                            const uint32_t row = gz[i] & 0x7FFFFFFFu;
#pragma unroll
                            for (int c = 0; c < NX; c++) {
                                const uint8_t* bm = fx.valid[c];
                                gxb[i][c] = bm ? (uint32_t)bm[row >> 3] : 0xFFu;
                                gxv[i][c] = fx.vals[c][row];
                            }
                        }
                    }
#pragma unroll
                    for (int i = 0; i < WALK_G; i++) {
                        const bool in = r + (uint32_t)i < seg1;
                        const uint64_t vbits =
                            ((uint64_t)gv[i].y << 32) | gv[i].x;
                        double v;
                        if constexpr (IV)
                            v = (double)(int64_t)vbits;
                        else
                            v = __longlong_as_double((long long)vbits);
                        const bool ok = in && (gz[i] >> 31);
                        if constexpr (IV) {
                            const int64_t iv = (int64_t)vbits;
                            i_mn = (ok && (fresh || iv < i_mn)) ? iv : i_mn;
                            i_mx = (ok && (fresh || iv > i_mx)) ? iv : i_mx;
                            i_sm = ok ? i_sm + vbits : i_sm;
                            f_fs = ok ? f_fs + v : f_fs;
                        } else {
                            f_mn = (ok && (fresh || v < f_mn)) ? v : f_mn;
                            f_mx = (ok && (fresh || v > f_mx)) ? v : f_mx;
                            f_sm = ok ? f_sm + v : f_sm;
                        }
                        nv += ok ? 1u : 0u;
                        fresh = fresh && !ok;
                        if (VAR) {
                            double mean = f_mean, m2 = f_m2;
                            welford_step(v, f_cnt + nv, mean, m2);
                            f_mean = ok ? mean : f_mean;
                            f_m2 = ok ? m2 : f_m2;
                        }
                        if constexpr (NX > 0) {
                            /* each extra under its own validity bit,
                             * whatever the primary's is */
                            const uint32_t row = gz[i] & 0x7FFFFFFFu;
#pragma unroll
                            for (int c = 0; c < NX; c++) {
                                const bool xok =
                                    in && ((gxb[i][c] >> (row & 7)) & 1u);
                                const double xv = gxv[i][c];
                                const bool xfresh = x.cnt[c] == 0;
                                x.mn[c] = (xok && (xfresh || xv < x.mn[c]))
                                              ? xv : x.mn[c];
                                x.mx[c] = (xok && (xfresh || xv > x.mx[c]))
                                              ? xv : x.mx[c];
                                x.sm[c] = xok ? x.sm[c] + xv : x.sm[c];
                                x.cnt[c] += xok ? 1u : 0u;
                            }
                        }
                    }
                }
                f_cnt += nv;
            }
        } else {
            /* L1 flush (bin-major staging => coalesced runs); the bin's
             * owner advances its segment cursor, which only the placement
             * phase reads */
            gcur[threadIdx.x] += tg;
            for (uint32_t p = threadIdx.x; p < s_total; p += BLOCK)
                orec[s_dest[p]] = s_rec[p];
        }
    }
    if (FOLD && f_own && f_loaded) { /* untouched bins write nothing */
        s_cnt[f_sidx] = f_cnt;
        s_first[f_sidx] = f_fst;
        if constexpr (IV) {
            s_min[f_sidx] = __longlong_as_double((long long)i_mn);
            s_max[f_sidx] = __longlong_as_double((long long)i_mx);
            s_sum[f_sidx] = __longlong_as_double((long long)i_sm);
            v_base[f_vidx] = f_fs;
            if (VAR) {
                v_base[f_vidx + fc.kcap] = f_mean;
                v_base[f_vidx + 2 * fc.kcap] = f_m2;
            }
        } else {
            s_min[f_sidx] = f_mn;
            s_max[f_sidx] = f_mx;
            s_sum[f_sidx] = f_sm;
            if (VAR) {
                v_base[f_vidx] = f_mean;
                v_base[f_vidx + fc.kcap] = f_m2;
            }
        }
        if constexpr (NX > 0) {
            const FoldExtras& fx = pick_fx(xa...);
#pragma unroll
            for (int c = 0; c < NX; c++) {
                const int64_t xi = f_xidx + (int64_t)(4 * c) * fc.kcap;
                fx.slab[xi] = x.cnt[c];
                fx.slab[xi + fc.kcap] =
                    (uint64_t)__double_as_longlong(x.mn[c]);
                fx.slab[xi + 2 * fc.kcap] =
                    (uint64_t)__double_as_longlong(x.mx[c]);
                fx.slab[xi + 3 * fc.kcap] =
                    (uint64_t)__double_as_longlong(x.sm[c]);
            }
        }
    }
}

/* the fold-mode launch: picks the instantiation from the value type, the
 * variance slab and the number of extra value columns (never two of them,
 * except int64 with variance: create and the setter refuse the rest) */
template <int MODE, typename... A>
static void launch_fold_mode(dim3 grid, hipStream_t s, double* v_base,
                             int ival, const FoldExtras& fx, A... a) {
    if (ival == FOLD_INT64_VAR)
        hipLaunchKernelGGL((k_regroup_t<MODE, true, 0, true>), grid,
                           dim3(BLOCK), 0, s, a...);
    else if (ival == FOLD_INT64)
        hipLaunchKernelGGL((k_regroup_t<MODE, false, 0, true>), grid,
                           dim3(BLOCK), 0, s, a...);
    else if (v_base)
        hipLaunchKernelGGL((k_regroup_t<MODE, true, 0>), grid, dim3(BLOCK), 0,
                           s, a...);
    else if (fx.nx == 1)
        hipLaunchKernelGGL((k_regroup_t<MODE, false, 1, false, FoldExtras>),
                           grid, dim3(BLOCK), 0, s, a..., fx);
    else if (fx.nx == 2)
        hipLaunchKernelGGL((k_regroup_t<MODE, false, 2, false, FoldExtras>),
                           grid, dim3(BLOCK), 0, s, a..., fx);
    else if (fx.nx == 3)
        hipLaunchKernelGGL((k_regroup_t<MODE, false, 3, false, FoldExtras>),
                           grid, dim3(BLOCK), 0, s, a..., fx);
    else
        hipLaunchKernelGGL((k_regroup_t<MODE, false, 0>), grid, dim3(BLOCK), 0,
                           s, a...);
}

void launch_regroup_fold(hipStream_t s, const uint4* d_grec,
                         const uint32_t* d_bucket_base,
                         const FoldChunk& fc, const int32_t* d_slot_of_widx,
                         uint64_t* s_cnt, double* s_min, double* s_max,
                         double* s_sum, uint64_t* s_first, int64_t slab_cells,
                         uint32_t* d_dbg, double* v_base, int64_t vslab_cells,
                         const FoldExtras& fx, int ival) {
    launch_fold_mode<RG_DIRECT_FOLD>(
        dim3(NB), s, v_base, ival, fx, d_grec, d_bucket_base, fc,
        (const uint32_t*)nullptr, (const uint32_t*)nullptr,
        (uint32_t*)nullptr, (uint32_t*)nullptr, (uint4*)nullptr,
        d_slot_of_widx, s_cnt, s_min, s_max, s_sum, s_first, slab_cells,
        d_dbg, v_base, v_base ? vslab_cells : (int64_t)0);
}

void launch_regroup_l1(hipStream_t s, const uint4* d_grec,
                       const uint32_t* d_bucket_base, const FoldChunk& fc,
                       uint32_t* d_b1offs, uint32_t* d_b1lens, uint4* d_grec2) {
    hipLaunchKernelGGL(k_regroup_t<RG_L1>, dim3(NB), dim3(BLOCK), 0, s,
                       d_grec, d_bucket_base, fc, nullptr, nullptr, d_b1offs,
                       d_b1lens, d_grec2, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, 0, nullptr, nullptr, 0);
}

void launch_regroup_l2_fold(hipStream_t s, const uint4* d_grec2,
                            const uint32_t* d_bucket_base,
                            const FoldChunk& fc, int nb1,
                            const uint32_t* d_b1offs, const uint32_t* d_b1lens,
                            const int32_t* d_slot_of_widx, uint64_t* s_cnt,
                            double* s_min, double* s_max, double* s_sum,
                            uint64_t* s_first, int64_t slab_cells,
                            uint32_t* d_dbg, double* v_base,
                            int64_t vslab_cells, const FoldExtras& fx,
                            int ival) {
    launch_fold_mode<RG_L2_FOLD>(
        dim3(NB, nb1), s, v_base, ival, fx, d_grec2, d_bucket_base, fc,
        d_b1offs, d_b1lens, (uint32_t*)nullptr, (uint32_t*)nullptr, (uint4*)nullptr,
        d_slot_of_widx, s_cnt, s_min, s_max, s_sum, s_first, slab_cells,
        d_dbg, v_base, v_base ? vslab_cells : (int64_t)0);
}

/* ------------------------------------------------------------------ */
/* device-side emission: compact touched groups, stable radix sort by  */
/* first-seen row (insertion order), gather aggregate columns + filter */
/* flag. Runs on the op's copy stream at window close; the host worker */
/* only formats the already-sorted columns.                            */
/* ------------------------------------------------------------------ */

constexpr int RDIG = 11;          /* radix digit bits */
constexpr int RBINS = 1 << RDIG;  /* 2048 */
constexpr int RCHUNK = 4096;      /* elements per radix block */
constexpr int RPASSES = 6;        /* 6*11 = 66 >= 64 bits */

/* Block compaction: every thread of a BLOCK-sized block calls this once per
 * round with its `pass` flag; passers get a distinct output position from
 * one `counter` bump per block (a returning per-thread atomic on one word
 * serialises). Rank = wave ballot + per-wave sums in LDS; block-local order
 * is irrelevant pre-sort. `wsum`/`base` are the caller's shared cells; the
 * caller keeps a __syncthreads() between rounds. *tot_out = block passers. */
__device__ __forceinline__ uint32_t block_compact_pos(
        bool pass, uint32_t* counter, uint32_t* wsum /*[WAVES_PER_BLOCK]*/,
        uint32_t* base, uint32_t* tot_out) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(pass);
    const uint64_t below = (lane == 63) ? ~0ULL : ((1ULL << (lane + 1)) - 1);
    const uint32_t wrank = (uint32_t)__popcll(m & below) - (pass ? 1 : 0);
    if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t wbase = 0, tot = 0;
    for (int w = 0; w < WAVES_PER_BLOCK; w++) {
        if (w < wave) wbase += wsum[w];
        tot += wsum[w];
    }
    if (threadIdx.x == 0) *base = tot ? atomicAdd(counter, tot) : 0u;
    __syncthreads();
    *tot_out = tot;
    return *base + wbase + wrank;
}

/* emit_filter_pass straight off a slot slab: the rule reads ONE of the three
 * value columns (field is launch-uniform), so only that one is loaded — the
 * closing slabs are the traffic of these kernels, and most groups fail the
 * filter before any other column is needed. */
__device__ __forceinline__ bool slab_filter_pass(const EmitFilter& ef,
        uint64_t cnt, const double* s_min, const double* s_max,
        const double* s_sum, int64_t k) {
    const double* col = ef.field == 1 ? s_min : ef.field == 2 ? s_max : s_sum;
    const double x = (ef.field != 0 && cnt > 0) ? col[k] : 0.0;
    return emit_filter_pass(ef, cnt, x, x, x);
}

__global__ __launch_bounds__(BLOCK) void k_ecompact(const uint64_t* s_first,
        uint64_t fbase, int64_t K, uint64_t* ekeys, uint32_t* ekid,
        uint32_t* eiota, uint32_t* counter) {
    __shared__ uint32_t base;
    __shared__ uint32_t wsum[WAVES_PER_BLOCK];
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k0 = (int64_t)blockIdx.x * blockDim.x; k0 < K;
         k0 += stride) {
        int64_t k = k0 + threadIdx.x;
        uint64_t f = (k < K) ? s_first[k] : ~0ULL;
        const bool hit = f != ~0ULL;
        uint32_t tot;
        const uint32_t p = block_compact_pos(hit, counter, wsum, &base, &tot);
        if (hit) {
            ekeys[p] = f - fbase; /* window-rebased: small keys, 4 passes */
            ekid[p] = (uint32_t)k;
            eiota[p] = p;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(BLOCK) void k_rhist(const uint64_t* keys,
        const uint32_t* counter, int shift, uint32_t* hist) {
    __shared__ uint32_t h[RBINS];
    const uint32_t nt = *counter;
    const uint32_t lo = blockIdx.x * RCHUNK;
    if (lo >= nt && blockIdx.x > 0) return; /* grids are sized for the full
        keyspace; only ceil(nt/RCHUNK) blocks hold live elements — the rest
        must not even write zeros (every downstream kernel clamps the same
        way), or a filtered close pays full-keyspace scan traffic */
    for (int t = threadIdx.x; t < RBINS; t += BLOCK) h[t] = 0;
    __syncthreads();
    const uint32_t hi = min(nt, lo + (uint32_t)RCHUNK);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += BLOCK)
        atomicAdd(&h[(uint32_t)(keys[i] >> shift) & (RBINS - 1)], 1u);
    __syncthreads();
    for (int t = threadIdx.x; t < RBINS; t += BLOCK)
        hist[(int64_t)blockIdx.x * RBINS + t] = h[t];
}

/* digit-major exclusive offsets: offs[b][d] = base[d] + sum_{b'<b} hist[b'][d]
 * Parallel 3-stage form: the single-block version was 44% of cfg3's GPU time
 * (profiles/r01_kernel_stats_cfg3.csv). */
constexpr int RSEG = 16;

__global__ void k_rscan_a(const uint32_t* hist, int nblk, int bs,
                          uint32_t* psum, const uint32_t* counter) {
    int d = blockIdx.x * blockDim.x + threadIdx.x;
    int seg = blockIdx.y;
    if (d >= RBINS) return;
    const int live = (int)((*counter + RCHUNK - 1) / RCHUNK);
    int b0 = seg * bs, b1 = min(min(nblk, live < 1 ? 1 : live), b0 + bs);
    uint32_t s = 0;
    for (int b = b0; b < b1; b++) s += hist[(int64_t)b * RBINS + d];
    psum[(int64_t)seg * RBINS + d] = s;
}

__global__ __launch_bounds__(1024) void k_rscan_b(const uint32_t* psum,
                                                  uint32_t* dbase) {
    __shared__ uint32_t part[1024];
    constexpr int PER = RBINS / 1024;
    uint32_t loc[PER];
    uint32_t s = 0;
    for (int j = 0; j < PER; j++) {
        int d = threadIdx.x * PER + j;
        uint32_t t = 0;
        for (int g = 0; g < RSEG; g++) t += psum[(int64_t)g * RBINS + d];
        loc[j] = s;
        s += t;
    }
    part[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        uint32_t v = (threadIdx.x >= (unsigned)o) ? part[threadIdx.x - o] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t pre = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (int j = 0; j < PER; j++) dbase[threadIdx.x * PER + j] = pre + loc[j];
}

__global__ void k_rscan_c(const uint32_t* hist, const uint32_t* psum,
                          const uint32_t* dbase, int nblk, int bs,
                          uint32_t* offs, const uint32_t* counter) {
    int d = blockIdx.x * blockDim.x + threadIdx.x;
    int seg = blockIdx.y;
    if (d >= RBINS) return;
    const int live = (int)((*counter + RCHUNK - 1) / RCHUNK);
    uint32_t run = dbase[d];
    for (int g = 0; g < seg; g++) run += psum[(int64_t)g * RBINS + d];
    int b0 = seg * bs, b1 = min(min(nblk, live < 1 ? 1 : live), b0 + bs);
    for (int b = b0; b < b1; b++) {
        uint32_t t = hist[(int64_t)b * RBINS + d];
        offs[(int64_t)b * RBINS + d] = run;
        run += t;
    }
}

__global__ __launch_bounds__(BLOCK) void k_rscatter(const uint64_t* keys,
        const uint32_t* payload, const uint32_t* counter, int shift,
        const uint32_t* offs, uint64_t* okeys, uint32_t* opayload) {
    /* stable per-block scatter: wave-quarters (wave order == element order)
     * with per-(wave,digit) counts -> private cursors */
    __shared__ uint32_t cnt4[WAVES_PER_BLOCK][RBINS]; /* overlaid to cursors */
    const uint32_t nt = *counter;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t lo = blockIdx.x * RCHUNK;
    const uint32_t hi = min(nt, lo + (uint32_t)RCHUNK);
    if (lo >= hi) return;
    for (int t = threadIdx.x; t < RBINS; t += BLOCK)
        for (int w = 0; w < WAVES_PER_BLOCK; w++) cnt4[w][t] = 0;
    __syncthreads();
    const uint32_t n = hi - lo;
    const uint32_t q = (n + WAVES_PER_BLOCK - 1) / WAVES_PER_BLOCK;
    const uint32_t w0 = lo + min(n, (uint32_t)wave * q);
    const uint32_t w1 = lo + min(n, (uint32_t)(wave + 1) * q);
    for (uint32_t i = w0 + lane; i < w1; i += 64)
        atomicAdd(&cnt4[wave][(uint32_t)(keys[i] >> shift) & (RBINS - 1)], 1u);
    __syncthreads();
    {   /* per-digit block totals -> add global offs -> per-wave bases */
        constexpr int PER = RBINS / BLOCK; /* 8 */
        for (int j = 0; j < PER; j++) {
            int d = threadIdx.x * PER + j;
            uint32_t run = offs[(int64_t)blockIdx.x * RBINS + d];
            for (int w = 0; w < WAVES_PER_BLOCK; w++) {
                uint32_t c = cnt4[w][d];
                cnt4[w][d] = run;
                run += c;
            }
        }
    }
    __syncthreads();
    for (uint32_t t0 = w0; t0 < w1; t0 += 64) {
        const uint32_t i = t0 + lane;
        const bool act = i < w1;
        uint64_t key = act ? keys[i] : ~0ULL;
        uint32_t pay = act ? payload[i] : 0;
        uint32_t d = act ? ((uint32_t)(key >> shift) & (RBINS - 1)) : 0xFFFFu;
        uint64_t same = ~0ULL;
        for (int b = 0; b < RDIG; b++) {
            uint64_t bb = __ballot((d >> b) & 1);
            same &= ((d >> b) & 1) ? bb : ~bb;
        }
        {
            uint64_t bb = __ballot(act);
            same &= act ? bb : ~bb;
        }
        const uint64_t below = (lane == 63) ? ~0ULL : ((1ULL << (lane + 1)) - 1);
        const int rank = (int)__popcll(same & below) - 1;
        const int leader = __ffsll((unsigned long long)same) - 1;
        const uint32_t wtot = (uint32_t)__popcll(same);
        uint32_t pos = 0;
        {
            uint32_t pre = 0;
            if (lane == leader && act) {
                pre = cnt4[wave][d];
                cnt4[wave][d] = pre + wtot;
            }
            pre = (uint32_t)__shfl((int)pre, leader);
            pos = pre + (uint32_t)rank;
        }
        if (act) {
            okeys[pos] = key;
            opayload[pos] = pay;
        }
    }
}




/* filter-compact: evaluate the pushed-down predicate on each touched group
 * (straight from the slot slab) and pack the passers:
 * {first, kid, iota} triples for the sort + gather stages. */
__global__ __launch_bounds__(BLOCK) void k_efilter(const uint64_t* ekeys,
        const uint32_t* ekid, const uint32_t* counter, const uint64_t* s_cnt,
        const double* s_min, const double* s_max, const double* s_sum,
        EmitFilter ef, uint64_t* fkeys, uint32_t* fkid, uint32_t* fiota,
        uint32_t* counter2) {
    __shared__ uint32_t base;
    __shared__ uint32_t wsum[WAVES_PER_BLOCK];
    const uint32_t nt = *counter;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x; i0 < nt; i0 += stride) {
        int64_t i = i0 + threadIdx.x;
        const bool act = i < nt;
        const uint32_t kid = act ? ekid[i] : 0;
        bool pass = act;
        if (act && ef.on)
            pass = slab_filter_pass(ef, s_cnt[kid], s_min, s_max, s_sum, kid);
        uint32_t tot;
        const uint32_t p = block_compact_pos(pass, counter2, wsum, &base, &tot);
        if (pass) {
            fkeys[p] = ekeys[i];
            fkid[p] = kid;
            fiota[p] = p;
        }
        __syncthreads();
    }
}

/* gather the passing groups' aggregate columns (by packed order) */
__global__ void k_egather(const uint32_t* fkid, const uint32_t* counter2,
                          const uint64_t* s_cnt, const double* s_min,
                          const double* s_max, const double* s_sum,
                          uint64_t* ocnt, double* omin, double* omax,
                          double* osum, double* oavg, uint8_t* oflags) {
    const uint32_t nt = *counter2;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nt;
         i += stride) {
        const uint32_t kid = fkid[i];
        const uint64_t c = s_cnt[kid];
        const bool valid = c > 0;
        ocnt[i] = c;
        omin[i] = valid ? s_min[kid] : 0.0;
        omax[i] = valid ? s_max[kid] : 0.0;
        osum[i] = valid ? s_sum[kid] : 0.0;
        oavg[i] = valid ? s_sum[kid] / (double)c : 0.0;
        oflags[i] = (uint8_t)((valid ? 1 : 0) | 2);
    }
}

void launch_emission_slabread(hipStream_t s, const uint64_t* slab_first,
                              const uint64_t* slab_cnt, const double* slab_min,
                              const double* slab_max, const double* slab_sum,
                              uint64_t base, int64_t K, uint64_t* ekeys, uint32_t* ekid,
                              uint64_t* fkeys, uint32_t* fkid, uint32_t* fiota,
                              uint32_t* counter, uint32_t* counter2,
                              const EmitFilter& ef, uint64_t* ocnt, double* omin,
                              double* omax, double* osum, double* oavg,
                              uint8_t* oflags) {
    int cblocks = (int)std::min<int64_t>((K + BLOCK - 1) / BLOCK, 2048);
    /* compact touched groups, filter-compact the passers, gather their
     * columns — all reads of the window slot's slab happen HERE, so the
     * slot is reusable right after these launches. */
    hipLaunchKernelGGL(k_ecompact, dim3(cblocks), dim3(BLOCK), 0, s, slab_first,
                       base, K, ekeys, ekid, fiota /*scratch, rewritten below*/,
                       counter);
    hipLaunchKernelGGL(k_efilter, dim3(cblocks), dim3(BLOCK), 0, s, ekeys, ekid,
                       counter, slab_cnt, slab_min, slab_max, slab_sum, ef,
                       fkeys, fkid, fiota, counter2);
    hipLaunchKernelGGL(k_egather, dim3(cblocks), dim3(BLOCK), 0, s, fkid,
                       counter2, slab_cnt, slab_min, slab_max, slab_sum, ocnt,
                       omin, omax, osum, oavg, oflags);
}

void launch_emission_sort(hipStream_t s, int64_t K, uint64_t* fkeys,
                          uint64_t* skeys, uint32_t* fiota, uint32_t* okid,
                          uint32_t* counter2, uint32_t* rhist, uint32_t* roffs,
                          uint64_t max_key) {
    uint64_t* ekeys = fkeys;
    uint32_t* skid = fiota;
    uint32_t* counter = counter2;
    /* sort (first, compact-index) pairs: keys ekeys<->skeys, payload
     * skid<->okid; the pass count covers the HOST-KNOWN key bound
     * (first is window-rebased to the window's open-time global row
     * counter, so the bound is the window's row span — 4 passes at any
     * stream age, not the 66-bit worst case of 6), rounded up to
     * EVEN so the sorted payload lands in skid.
     * (The device path only runs above the 64k-key host-emission cutoff,
     * so the multi-block form is always the right one.) */
    {
        int passes = 0;
        while (passes * RDIG < 64 && (max_key >> (passes * RDIG)) != 0)
            passes++;
        if (passes & 1) passes++;
        if (passes < 2) passes = 2;
        int nblk = (int)((K + RCHUNK - 1) / RCHUNK);
        uint64_t* ka = ekeys;
        uint32_t* pa = skid;
        uint64_t* kb = skeys;
        uint32_t* pb = okid;
        int bs = (nblk + RSEG - 1) / RSEG;
        uint32_t* psum = rhist + (int64_t)nblk * RBINS;  /* scratch tail */
        uint32_t* dbase = psum + (int64_t)RSEG * RBINS;
        for (int p = 0; p < passes; p++) {
            int shift = p * RDIG;
            hipLaunchKernelGGL(k_rhist, dim3(nblk), dim3(BLOCK), 0, s, ka,
                               counter, shift, rhist);
            hipLaunchKernelGGL(k_rscan_a, dim3(RBINS / 256, RSEG), dim3(256), 0,
                               s, rhist, nblk, bs, psum, counter);
            hipLaunchKernelGGL(k_rscan_b, dim3(1), dim3(1024), 0, s, psum, dbase);
            hipLaunchKernelGGL(k_rscan_c, dim3(RBINS / 256, RSEG), dim3(256), 0,
                               s, rhist, psum, dbase, nblk, bs, roffs, counter);
            hipLaunchKernelGGL(k_rscatter, dim3(nblk), dim3(BLOCK), 0, s, ka, pa,
                               counter, shift, roffs, kb, pb);
            std::swap(ka, kb);
            std::swap(pa, pb);
        }
    }
}

/* batched reset of freshly (re)allocated window slots:
 * cnt = 0, first = ~0 for `ns` slots in one launch */
__global__ void k_reset_slots(const int32_t* slots, int ns, int64_t kcap,
                              uint64_t* s_cnt, uint64_t* s_first) {
    int64_t total = (int64_t)ns * kcap;
    int64_t stride5 = 5 * kcap;
    int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += gstride) {
        int64_t si = i / kcap, k = i % kcap;
        int64_t base = slots[si] * stride5 + k;
        s_cnt[base] = 0;
        s_first[base] = ~0ULL;
    }
}

void launch_reset_slots(hipStream_t s, const int32_t* d_slots, int ns,
                        int64_t kcap, uint64_t* s_cnt, uint64_t* s_first) {
    int64_t total = (int64_t)ns * kcap;
    int blocks = (int)std::min<int64_t>((total + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_reset_slots, dim3(blocks), dim3(BLOCK), 0, s, d_slots,
                       ns, kcap, s_cnt, s_first);
}

/* multi-column ops: zero every extra's cnt of the same slots (min/max/sum
 * may stay stale: the fold reads them only behind a non-zero cnt) */
__global__ void k_reset_slots_x(const int32_t* slots, int ns, int nx,
                                int64_t kcap, uint64_t* x_slab) {
    const int64_t per_slot = (int64_t)nx * kcap;
    const int64_t total = (int64_t)ns * per_slot;
    const int64_t gstride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total;
         i += gstride) {
        const int64_t si = i / per_slot, rem = i % per_slot;
        const int64_t c = rem / kcap, k = rem % kcap;
        x_slab[slots[si] * (4 * per_slot) + c * 4 * kcap + k] = 0;
    }
}

void launch_reset_slots_x(hipStream_t s, const int32_t* d_slots, int ns,
                          int nx, int64_t kcap, uint64_t* x_slab) {
    int64_t total = (int64_t)ns * nx * kcap;
    int blocks = (int)std::min<int64_t>((total + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_reset_slots_x, dim3(blocks), dim3(BLOCK), 0, s,
                       d_slots, ns, nx, kcap, x_slab);
}

} // namespace dz

/* ------------------------------------------------------------------ */
/* host-path emission: pack closing slots' slabs into one staging run  */
/* (grid.y = close, grid.z = segment; no per-element division)         */
/* ------------------------------------------------------------------ */

/* One segment (blockIdx.z) of one close (blockIdx.y): a plain grid-stride copy
 * of whole columns, from the closing slot's slab (or, by_close, the close's
 * own row of a per-close buffer) to their place in the packed close. Blocks
 * past a short segment's end fall through the loop. */
__global__ void k_egather_close(dz::GatherDesc d, dz::EGatherSlots slots,
                                uint64_t* __restrict__ out) {
    const int g = blockIdx.y;
    const dz::GatherSeg& sg = d.seg[blockIdx.z];
    const int64_t row = sg.by_close ? g : slots.s[g];
    const uint64_t* __restrict__ src = sg.base + row * sg.stride + sg.off;
    uint64_t* dst = out + (int64_t)g * d.close_cells + sg.dst;
    const int64_t cells = sg.cells;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
         i < cells; i += (int64_t)gridDim.x * blockDim.x)
        dst[i] = src[i];
}

void dz::launch_egather_close(hipStream_t s, const dz::GatherDesc& d,
                              dz::EGatherSlots slots, int gcount,
                              uint64_t* out) {
    int64_t widest = 0;
    for (int i = 0; i < d.nseg; i++)
        widest = std::max(widest, d.seg[i].cells);
    int bx = (int)std::min<int64_t>((widest + dz::BLOCK - 1) / dz::BLOCK, 512);
    dim3 grid(bx, gcount, d.nseg);
    hipLaunchKernelGGL(k_egather_close, grid, dim3(dz::BLOCK), 0, s, d, slots,
                       out);
}

/* arm the per-push scalar block (min=+inf pattern, max/kid=0) in ONE tiny
 * launch: the generic fill kernel costs ~20 us per call on a busy device
 * and two of them sat on the ingest reduction's critical path */
__global__ void k_arm_scalars(uint64_t* __restrict__ s) {
    s[0] = ~0ULL;
    s[1] = 0ULL;
    s[2] = 0ULL;
}

void dz::launch_arm_scalars(hipStream_t st, uint64_t* s) {
    hipLaunchKernelGGL(k_arm_scalars, dim3(1), dim3(1), 0, st, s);
}

__global__ void k_zero2(uint32_t* __restrict__ p) {
    p[0] = 0;
    p[1] = 0;
}

void dz::launch_zero_counters(hipStream_t st, uint32_t* p) {
    hipLaunchKernelGGL(k_zero2, dim3(1), dim3(1), 0, st, p);
}

/* apply the sorted permutation to every output column ON DEVICE, packing
 * the final-order columns into one contiguous block: the worker then pulls
 * ONE span and builds with sequential copies (the host-side gather through
 * sidx over ~1M-row closes was the cfg3 build bottleneck). The layout is
 * dz::packed_cols (dz_internal.h) with stride nt, device-read from counter2.
 * Serves the per-close chain and the group-batched chain alike. */
__global__ void k_epermute(const uint32_t* __restrict__ counter2,
                           const uint32_t* __restrict__ sidx,
                           const uint32_t* __restrict__ fkid,
                           const uint64_t* __restrict__ ocnt,
                           const double* __restrict__ omin,
                           const double* __restrict__ omax,
                           const double* __restrict__ osum,
                           const double* __restrict__ oavg,
                           const uint8_t* __restrict__ oflags,
                           char* __restrict__ out) {
    const uint32_t nt = *counter2;
    const auto o = dz::packed_cols(out, nt);
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nt;
         i += stride) {
        const uint32_t j = sidx[i];
        const uint32_t k = fkid[j];
        o.key[i] = (int64_t)k;
        o.cnt[i] = ocnt[j];
        o.min[i] = omin[j];
        o.max[i] = omax[j];
        o.sum[i] = osum[j];
        o.avg[i] = oavg[j];
        o.kid[i] = k;
        o.flags[i] = oflags[j] & 1; /* packed validity is 0/1 so the host
                                     * build can take it verbatim (k_egather
                                     * sets bit 1 too; k_egf writes 0/1) */
    }
}

void dz::launch_emission_permute(hipStream_t st, int64_t K,
                                 const uint32_t* counter2, const uint32_t* sidx,
                                 const uint32_t* fkid, const uint64_t* ocnt,
                                 const double* omin, const double* omax,
                                 const double* osum, const double* oavg,
                                 const uint8_t* oflags, char* out) {
    int blocks = (int)std::min<int64_t>((K + dz::BLOCK - 1) / dz::BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_epermute, dim3(blocks), dim3(dz::BLOCK), 0, st,
                       counter2, sidx, fkid, ocnt, omin, omax, osum, oavg,
                       oflags, out);
}

/* ------------------------------------------------------------------ */
/* stream join (BASELINE cfg5): inner equi-join on trip_id, build side */
/* (trip -> driver) in an open-address device table; probe batches     */
/* emit matched rows IN ROW ORDER (stable per-chunk compaction) and    */
/* buffer unmatched rows IN ROW ORDER for re-probe on build growth —   */
/* the emission discipline oracle.c::orc_join_* restates.              */
/* ------------------------------------------------------------------ */

namespace dz {

constexpr int64_t JEMPTY = INT64_MIN;

__device__ __forceinline__ uint64_t jhash(int64_t trip) {
    return (uint64_t)trip * 0x9e3779b97f4a7c15ULL;
}

/* build pre-pass (validate BEFORE any write): pre[0] flags a trip equal to
 * the empty-slot sentinel, pre[1] a driver id outside [0, INT32_MAX], and
 * pre[2] counts rows whose trip is not in the table yet. Duplicates of a
 * new trip within the batch each count: the figure is an upper bound on the
 * slots the build will claim, which is what the capacity check needs. */
__global__ void k_join_precheck(const int64_t* trips, const int64_t* drivers,
                                int64_t n, const int64_t* tab_trip,
                                uint64_t p_mask, uint32_t* pre) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t fresh = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const int64_t trip = trips[i];
        const int64_t drv = drivers[i];
        if (trip == JEMPTY) {
            pre[0] = 1;
            continue;
        }
        if (drv < 0 || drv > (int64_t)INT32_MAX) pre[1] = 1;
        uint64_t slot = jhash(trip) & p_mask;
        for (uint64_t probes = 0; probes <= p_mask; ++probes) {
            const int64_t got = tab_trip[slot];
            if (got == JEMPTY) {
                fresh++;
                break;
            }
            if (got == trip) break;
            slot = (slot + 1) & p_mask;
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        fresh += (uint32_t)__shfl_down((int)fresh, o);
    if ((threadIdx.x & 63) == 0 && fresh) atomicAdd(&pre[2], fresh);
}

/* pre[3] receives the number of slots this batch claimed (the op keeps the
 * running total for the capacity check). The host refuses a batch that would
 * fill the table past half before this kernel runs; the probe bound is the
 * second line of defence. */
__global__ void k_join_build(const int64_t* trips, const int64_t* drivers,
                             int64_t n, int64_t* tab_trip, int64_t* tab_drv,
                             uint64_t p_mask, uint32_t* dbg, uint32_t* pre) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    uint32_t claimed = 0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        const int64_t trip = trips[i];
        if (trip == JEMPTY) continue; /* refused by the pre-pass */
        uint64_t slot = jhash(trip) & p_mask;
        for (uint64_t probes = 0;; slot = (slot + 1) & p_mask) {
            int64_t got = tab_trip[slot];
            if (got == JEMPTY) {
                got = (int64_t)atomicCAS((unsigned long long*)&tab_trip[slot],
                                         (unsigned long long)JEMPTY,
                                         (unsigned long long)trip);
                if (got == JEMPTY) {
                    got = trip; /* claimed */
                    claimed++;
                }
            }
            if (got == trip) {
                /* later duplicates overwrite (dimension update); the winner
                 * among duplicates WITHIN one batch is unspecified — same
                 * contract as the oracle documents */
                tab_drv[slot] = drivers[i];
                break;
            }
            if (++probes > p_mask) {
                dbg[3] = 8; /* join table full */
                break;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        claimed += (uint32_t)__shfl_down((int)claimed, o);
    if ((threadIdx.x & 63) == 0 && claimed) atomicAdd(&pre[3], claimed);
}

/* probe pass 1: resolve each row's driver (or -1) into drv_tmp and count
 * matches per chunk (one block per chunk). The empty test comes first, so a
 * probe row whose trip IS the sentinel stops at the first empty slot
 * unmatched instead of "matching" it; the walk is bounded by the table size
 * whatever the table holds. */
__global__ __launch_bounds__(64) void k_join_mark(const int64_t* trips,
        int64_t n, int64_t chunk, const int64_t* tab_trip,
        const int64_t* tab_drv, uint64_t p_mask, int32_t* drv_tmp,
        uint32_t* jcnt) {
    const int64_t lo = blockIdx.x * chunk;
    const int64_t hi = i64min(n, lo + chunk);
    uint32_t m = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 64) {
        const int64_t trip = trips[i];
        uint64_t slot = jhash(trip) & p_mask;
        int32_t drv = -1;
        /* at most 2^28 slots: a 32-bit countdown covers the whole table */
        for (uint32_t left = (uint32_t)p_mask + 1u; left; --left) {
            const int64_t got = tab_trip[slot];
            if (got == JEMPTY) break;
            if (got == trip) {
                drv = (int32_t)tab_drv[slot];
                break;
            }
            slot = (slot + 1) & p_mask;
        }
        drv_tmp[i] = drv;
        m += drv >= 0 ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) m += (uint32_t)__shfl_down((int)m, o);
    if (threadIdx.x == 0) jcnt[blockIdx.x] = m;
}

/* exclusive scan of per-chunk matched counts + complement (single block):
 * mbase/ubase per chunk; totals in tot[0] (matched) / tot[1] (unmatched) */
__global__ __launch_bounds__(1024) void k_join_scan(const uint32_t* jcnt,
        int C, int64_t n, int64_t chunk, uint32_t* mbase, uint32_t* ubase,
        uint32_t* tot) {
    __shared__ uint32_t runm, runu;
    if (threadIdx.x == 0) {
        uint32_t rm = 0, ru = 0;
        for (int c = 0; c < C; c++) {
            const uint32_t rows =
                (uint32_t)(i64min(n, (int64_t)(c + 1) * chunk) -
                           i64min(n, (int64_t)c * chunk));
            mbase[c] = rm;
            ubase[c] = ru;
            rm += jcnt[c];
            ru += rows - jcnt[c];
        }
        runm = rm;
        runu = ru;
        tot[0] = rm;
        tot[1] = ru;
    }
}

/* probe pass 2: stable per-chunk split — matched rows (ts, driver-as-kid,
 * val) to the output block, unmatched (ts, trip, val) appended to the
 * unmatched buffer; one 64-thread block per chunk, wave ballots keep row
 * order */
__global__ __launch_bounds__(64) void k_join_emit(const int64_t* ts,
        const int64_t* trips, const double* vals, const int32_t* drv_tmp,
        int64_t n, int64_t chunk, const uint32_t* mbase, const uint32_t* ubase,
        int64_t* o_ts, int32_t* o_kid, double* o_val, int64_t ubuf_base,
        int64_t* u_ts, int64_t* u_trip, double* u_val) {
    const int64_t lo = blockIdx.x * chunk;
    const int64_t hi = i64min(n, lo + chunk);
    uint32_t mcur = mbase[blockIdx.x];
    uint32_t ucur = ubase[blockIdx.x];
    const int lane = threadIdx.x;
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + lane;
        const bool act = i < hi;
        const int32_t drv = act ? drv_tmp[i] : -1;
        const bool hit = act && drv >= 0;
        const uint64_t mm = __ballot(hit);
        const uint64_t um = __ballot(act && !hit);
        const uint64_t below = (lane == 63) ? ~0ULL : ((1ULL << (lane + 1)) - 1);
        if (hit) {
            const uint32_t p = mcur + (uint32_t)__popcll(mm & below) - 1;
            o_ts[p] = ts[i];
            o_kid[p] = drv;
            o_val[p] = vals[i];
        } else if (act) {
            const int64_t p = ubuf_base + ucur +
                              (uint32_t)__popcll(um & below) - 1;
            u_ts[p] = ts[i];
            u_trip[p] = trips[i];
            u_val[p] = vals[i];
        }
        mcur += (uint32_t)__popcll(mm);
        ucur += (uint32_t)__popcll(um);
    }
}

__global__ void k_fill_i64(int64_t* p, int64_t n, int64_t v) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride)
        p[i] = v;
}

void launch_fill_i64(hipStream_t s, int64_t* d_p, int64_t n, int64_t v) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_fill_i64, dim3(blocks), dim3(BLOCK), 0, s, d_p, n, v);
}

void launch_join_precheck(hipStream_t s, const int64_t* d_trips,
                          const int64_t* d_drivers, int64_t n,
                          const int64_t* tab_trip, uint64_t p_mask,
                          uint32_t* d_pre) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_join_precheck, dim3(blocks), dim3(BLOCK), 0, s,
                       d_trips, d_drivers, n, tab_trip, p_mask, d_pre);
}

void launch_join_build(hipStream_t s, const int64_t* d_trips,
                       const int64_t* d_drivers, int64_t n, int64_t* tab_trip,
                       int64_t* tab_drv, uint64_t p_mask, uint32_t* d_dbg,
                       uint32_t* d_pre) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(k_join_build, dim3(blocks), dim3(BLOCK), 0, s, d_trips,
                       d_drivers, n, tab_trip, tab_drv, p_mask, d_dbg, d_pre);
}

void launch_join_probe(hipStream_t s, const int64_t* d_ts,
                       const int64_t* d_trips, const double* d_vals, int64_t n,
                       int64_t chunk, int C, const int64_t* tab_trip,
                       const int64_t* tab_drv, uint64_t p_mask,
                       int32_t* d_drvtmp, uint32_t* d_jcnt, uint32_t* d_mbase,
                       uint32_t* d_ubase, uint32_t* d_tot, int64_t* o_ts,
                       int32_t* o_kid, double* o_val, int64_t ubuf_base,
                       int64_t* u_ts, int64_t* u_trip, double* u_val) {
    hipLaunchKernelGGL(k_join_mark, dim3(C), dim3(64), 0, s, d_trips, n, chunk,
                       tab_trip, tab_drv, p_mask, d_drvtmp, d_jcnt);
    hipLaunchKernelGGL(k_join_scan, dim3(1), dim3(1024), 0, s, d_jcnt, C, n,
                       chunk, d_mbase, d_ubase, d_tot);
    hipLaunchKernelGGL(k_join_emit, dim3(C), dim3(64), 0, s, d_ts, d_trips,
                       d_vals, d_drvtmp, n, chunk, d_mbase, d_ubase, o_ts,
                       o_kid, o_val, ubuf_base, u_ts, u_trip, u_val);
}

} // namespace dz

/* ------------------------------------------------------------------ */
/* JSON ingest: the reference decodes Kafka payload      */
/* bytes to RecordBatches on the host via serde_json                   */
/* (crates/core/src/formats/decoders/json.rs:23-46 over the stream     */
/* read path kafka_stream_read.rs:165-296). Here the decode runs ON    */
/* DEVICE: newline-split, schema-directed field parse (int64 ts, utf8  */
/* key, f64 reading; other fields of any JSON shape are skipped), and  */
/* a compact Arrow key column — shaped to feed the utf8-intern push.   */
/* Number parsing uses the EXACT Clinger fast path (<=15 significant   */
/* digits and 10^|e|<=22: both factors exactly representable => the    */
/* correctly-rounded double, identical to strtod); longer literals     */
/* flag the debug cell and the decode fails loudly (documented         */
/* subset — the synthetic sensor streams print 6-decimal fixed).       */
/* ------------------------------------------------------------------ */

namespace dz {

__global__ __launch_bounds__(64) void k_json_nl_count(const char* b, int64_t n,
        int64_t chunk, uint32_t* cnt) {
    const int64_t lo = blockIdx.x * chunk;
    const int64_t hi = i64min(n, lo + chunk);
    uint32_t m = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 64)
        m += b[i] == '\n' ? 1 : 0;
    for (int o = 32; o > 0; o >>= 1) m += (uint32_t)__shfl_down((int)m, o);
    if (threadIdx.x == 0) cnt[blockIdx.x] = m;
}

/* exclusive scan over the C chunk counts + total records:
 * rec_total = newlines + (tail bytes after the last newline ? 1 : 0).
 * The tail test needs the LAST byte: done host-side (flag arg). */
__global__ void k_json_nl_scan(const uint32_t* cnt, int C, uint32_t* base,
                               int32_t tail_record, uint32_t* tot) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        uint32_t run = 1; /* record 0 starts at byte 0 */
        for (int c = 0; c < C; c++) {
            base[c] = run;
            run += cnt[c];
        }
        /* run now counts 1 + newlines = candidate starts; the start right
         * after a trailing newline is not a record */
        tot[0] = tail_record ? run : run - 1;
    }
}

/* stable start-offset emission: record i starts at 0 or right after the
 * i-1'th newline */
__global__ __launch_bounds__(64) void k_json_nl_emit(const char* b, int64_t n,
        int64_t chunk, const uint32_t* base, const uint32_t* tot,
        int64_t* rec_off) {
    if (blockIdx.x == 0 && threadIdx.x == 0) rec_off[0] = 0;
    const int64_t lo = blockIdx.x * chunk;
    const int64_t hi = i64min(n, lo + chunk);
    uint32_t cur = base[blockIdx.x];
    const uint32_t nt = tot[0];
    for (int64_t i0 = lo; i0 < hi; i0 += 64) {
        const int64_t i = i0 + threadIdx.x;
        const bool nl = i < hi && b[i] == '\n';
        const uint64_t m = __ballot(nl);
        const uint64_t below =
            (threadIdx.x == 63) ? ~0ULL : ((1ULL << (threadIdx.x + 1)) - 1);
        if (nl) {
            const uint32_t p = cur + (uint32_t)__popcll(m & below) - 1;
            if (p < nt) rec_off[p] = i + 1;
        }
        cur += (uint32_t)__popcll(m);
    }
}

/* schema-directed per-record parse (JsonFields in dz_internal.h) */
__device__ __forceinline__ bool jf_eq(const char* a, int32_t alen,
                                      const char* b, int32_t blen) {
    if (alen != blen) return false;
    for (int32_t i = 0; i < alen; i++)
        if (a[i] != b[i]) return false;
    return true;
}

__device__ __forceinline__ const char* j_ws(const char* p, const char* e) {
    while (p < e && (*p == ' ' || *p == '\t' || *p == '\r')) p++;
    return p;
}

__device__ __forceinline__ bool j_dig(char c) {
    return (unsigned)(c - '0') <= 9u;
}

/* p is just past an opening quote: returns the closing quote's position, or
 * e when the string is unterminated or holds a raw control byte (< 0x20,
 * not JSON). Escape pairs are stepped over (their spelling is not
 * validated); *esc reports that one was seen. */
__device__ __forceinline__ const char* j_str(const char* p, const char* e,
                                             bool* esc) {
    while (p < e && *p != '"') {
        if ((unsigned char)*p < 0x20) return e;
        if (*p == '\\') {
            *esc = true;
            if (++p >= e) return e;
        }
        p++;
    }
    return p;
}

/* length of the literal w (n bytes) if it is spelled at p, else 0 */
__device__ __forceinline__ int32_t j_lit(const char* p, const char* e,
                                         const char* w, int32_t n) {
    if (e - p < n) return 0;
    for (int32_t i = 0; i < n; i++)
        if (p[i] != w[i]) return 0;
    return n;
}

__global__ __launch_bounds__(BLOCK) void k_json_parse(const char* buf,
        const int64_t* rec_off, const uint32_t* tot, int64_t nbytes,
        JsonFields jf, int64_t* o_ts, int64_t* o_kbeg, int32_t* o_klen,
        double* o_val, uint32_t* dbg) {
    const double p10[23] = {1e0, 1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9,
                            1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16, 1e17,
                            1e18, 1e19, 1e20, 1e21, 1e22};
    const uint32_t nt = tot[0];
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nt;
         r += stride) {
        const char* p = buf + rec_off[r];
        const char* e = (r + 1 < nt) ? buf + rec_off[r + 1] - 1 : buf + nbytes;
        while (e > p && (*(e - 1) == '\n' || *(e - 1) == '\r')) e--;
        int64_t ts = 0;
        int64_t kbeg = -1;
        int32_t klen = 0;
        double val = 0.0;
        bool have_ts = false, have_key = false, have_val = false, bad = false;
        bool subset = false; /* valid JSON outside the documented subset */
        bool closed = false;
        p = j_ws(p, e);
        if (p >= e || *p != '{') bad = true;
        if (!bad) {
            p = j_ws(p + 1, e);
            if (p < e && *p == '}') { p++; closed = true; } /* {} */
        }
        while (!bad && !closed) {
            /* one member: "name" : value, then ',' (another member MUST
             * follow) or the closing '}' */
            p = j_ws(p, e);
            if (p >= e || *p != '"') { bad = true; break; }
            const char* name = ++p;
            bool nesc = false;
            p = j_str(p, e, &nesc);
            if (p >= e) { bad = true; break; }
            const int32_t nlen = (int32_t)(p - name);
            p++;
            p = j_ws(p, e);
            if (p >= e || *p != ':') { bad = true; break; }
            p = j_ws(p + 1, e);
            if (p >= e) { bad = true; break; }
            /* names are matched on their raw bytes: a schema name spelled
             * with escapes is not recognised (documented) */
            const bool is_ts = jf_eq(name, nlen, jf.ts_name, jf.ts_len);
            const bool is_key = jf_eq(name, nlen, jf.key_name, jf.key_len);
            const bool is_val = jf_eq(name, nlen, jf.val_name, jf.val_len);
            if (*p == '"') { /* string value */
                const char* s = ++p;
                bool esc = false;
                p = j_str(p, e, &esc);
                if (p >= e) { bad = true; break; }
                if (is_key) {
                    if (esc) { subset = bad = true; break; } /* escaped key */
                    kbeg = (int64_t)(s - buf);
                    klen = (int32_t)(p - s);
                    have_key = true;
                } else if (is_ts || is_val) {
                    bad = true; /* wrong type for a schema field */
                    break;
                }
                p++;
            } else if (*p == '{' || *p == '[') { /* skip nested structure */
                if (is_ts || is_key || is_val) { bad = true; break; }
                int depth = 0;
                bool instr = false;
                while (p < e) {
                    const char c = *p;
                    if (instr) {
                        if (c == '\\' && p + 1 < e) p++;
                        else if (c == '"') instr = false;
                    } else if (c == '"') {
                        instr = true;
                    } else if (c == '{' || c == '[') {
                        depth++;
                    } else if (c == '}' || c == ']') {
                        depth--;
                        if (depth == 0) { p++; break; }
                    }
                    p++;
                }
                if (depth != 0) { bad = true; break; }
            } else if (*p == 't' || *p == 'f' || *p == 'n') {
                /* true / false / null, spelled exactly (what follows is
                 * checked by the separator rule below) */
                if (is_ts || is_key || is_val) { bad = true; break; }
                const int32_t l = *p == 't' ? j_lit(p, e, "true", 4)
                                : *p == 'f' ? j_lit(p, e, "false", 5)
                                            : j_lit(p, e, "null", 4);
                if (!l) { bad = true; break; }
                p += l;
            } else { /* number: -? (0 | [1-9][0-9]*) (. [0-9]+)? ([eE] [+-]? [0-9]+)? */
                bool neg = false;
                if (*p == '-') { neg = true; p++; }
                if (p >= e || !j_dig(*p)) { bad = true; break; }
                /* mant holds the first 19 SIGNIFICANT digits (zeros before
                 * the first non-zero digit are not significant); nsig
                 * saturates at 20, which is all the range checks need */
                uint64_t mant = 0;
                int32_t nsig = 0, exp10 = 0;
                int64_t frac = 0;
                bool isint = true;
                if (*p == '0') {
                    p++;
                    if (p < e && j_dig(*p)) { bad = true; break; } /* 01 */
                } else {
                    while (p < e && j_dig(*p)) {
                        if (nsig < 19) mant = mant * 10 + (uint64_t)(*p - '0');
                        nsig += nsig < 20;
                        p++;
                    }
                }
                if (p < e && *p == '.') {
                    isint = false;
                    p++;
                    if (p >= e || !j_dig(*p)) { bad = true; break; } /* 1. */
                    while (p < e && j_dig(*p)) {
                        if (nsig > 0 || *p != '0') {
                            if (nsig < 19)
                                mant = mant * 10 + (uint64_t)(*p - '0');
                            nsig += nsig < 20;
                        }
                        frac++;
                        p++;
                    }
                }
                if (p < e && (*p == 'e' || *p == 'E')) {
                    isint = false;
                    p++;
                    bool eneg = false;
                    if (p < e && (*p == '+' || *p == '-')) {
                        eneg = *p == '-';
                        p++;
                    }
                    if (p >= e || !j_dig(*p)) { bad = true; break; } /* 1e */
                    int32_t ev = 0; /* saturates far outside +-22 */
                    while (p < e && j_dig(*p)) {
                        if (ev < 100000) ev = ev * 10 + (*p - '0');
                        p++;
                    }
                    exp10 = eneg ? -ev : ev;
                }
                if (is_key) { bad = true; break; } /* wrong type */
                if (is_ts) {
                    /* an integer literal within int64; 19 digits cannot
                     * wrap the u64 mantissa */
                    const uint64_t lim = neg ? (1ULL << 63) : (1ULL << 63) - 1;
                    if (!isint || nsig > 19 || mant > lim) {
                        subset = bad = true;
                        break;
                    }
                    ts = (int64_t)(neg ? 0 - mant : mant);
                    have_ts = true;
                } else if (is_val) {
                    const int64_t e10 = (int64_t)exp10 - frac;
                    if (nsig > 15 || e10 > 22 || e10 < -22) {
                        subset = bad = true; /* outside the exact fast path */
                        break;
                    }
                    double d = (double)mant;
                    d = e10 >= 0 ? d * p10[e10] : d / p10[-e10];
                    val = neg ? -d : d;
                    have_val = true;
                }
            }
            p = j_ws(p, e);
            if (p < e && *p == ',') { p++; continue; }
            if (p < e && *p == '}') { p++; closed = true; break; }
            bad = true;
        }
        /* only space / tab / CR may follow the closing brace */
        if (!bad && j_ws(p, e) != e) bad = true;
        if (bad || !have_ts || !have_key || !have_val) {
            /* 2: outside the subset, 1: malformed, 3: missing schema field */
            dbg[2] = subset ? 2 : (bad ? 1 : 3);
            ts = 0; kbeg = rec_off[r]; klen = 0; val = 0.0;
        }
        o_ts[r] = ts;
        o_kbeg[r] = kbeg;
        o_klen[r] = klen;
        o_val[r] = val;
    }
}

/* generic exclusive scan (u32) for the key-length -> offsets pass:
 * per-block totals, single-block scan of totals, add-back */
constexpr int JS_ELEMS = 4096; /* per block */

__global__ __launch_bounds__(BLOCK) void k_scanu32_a(const int32_t* in,
        int64_t n, uint32_t* blocksum) {
    const int64_t lo = (int64_t)blockIdx.x * JS_ELEMS;
    const int64_t hi = i64min(n, lo + JS_ELEMS);
    uint32_t s = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += BLOCK)
        s += (uint32_t)in[i];
    __shared__ uint32_t red[WAVES_PER_BLOCK];
    for (int o = 32; o > 0; o >>= 1) s += (uint32_t)__shfl_down((int)s, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t t = 0;
        for (int w = 0; w < WAVES_PER_BLOCK; w++) t += red[w];
        blocksum[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(1024) void k_scanu32_b(uint32_t* blocksum,
        int nb, uint32_t* total) {
    /* single block: exclusive scan over nb block sums (loops if nb > 1024) */
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    __shared__ uint32_t buf[1024];
    for (int b0 = 0; b0 < nb; b0 += 1024) {
        const int i = b0 + threadIdx.x;
        uint32_t v = (i < nb) ? blocksum[i] : 0;
        buf[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 1024; o <<= 1) {
            uint32_t t = (threadIdx.x >= (unsigned)o) ? buf[threadIdx.x - o] : 0;
            __syncthreads();
            buf[threadIdx.x] += t;
            __syncthreads();
        }
        if (i < nb)
            blocksum[i] = carry + (threadIdx.x ? buf[threadIdx.x - 1] : 0);
        __syncthreads();
        if (threadIdx.x == 0) carry += buf[1023];
        __syncthreads();
    }
    if (threadIdx.x == 0 && total) total[0] = carry;
}

__global__ __launch_bounds__(BLOCK) void k_scanu32_c(const int32_t* in,
        int64_t n, const uint32_t* blocksum, int32_t* out /* n+1 */) {
    /* per-block local exclusive scan + base add-back */
    __shared__ uint32_t thr[BLOCK];
    const int64_t lo = (int64_t)blockIdx.x * JS_ELEMS;
    const int64_t hi = i64min(n, lo + JS_ELEMS);
    constexpr int PER = JS_ELEMS / BLOCK;
    uint32_t loc[PER];
    uint32_t s = 0;
    for (int j = 0; j < PER; j++) {
        const int64_t i = lo + (int64_t)threadIdx.x * PER + j;
        loc[j] = s;
        if (i < hi) s += (uint32_t)in[i];
    }
    thr[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < BLOCK; o <<= 1) {
        uint32_t t = (threadIdx.x >= (unsigned)o) ? thr[threadIdx.x - o] : 0;
        __syncthreads();
        thr[threadIdx.x] += t;
        __syncthreads();
    }
    const uint32_t base = blocksum[blockIdx.x] +
                          (threadIdx.x ? thr[threadIdx.x - 1] : 0);
    for (int j = 0; j < PER; j++) {
        const int64_t i = lo + (int64_t)threadIdx.x * PER + j;
        if (i < hi) out[i] = (int32_t)(base + loc[j]);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[n] = 0; /* patched below */
}

__global__ void k_scanu32_tail(int64_t n, const uint32_t* total, int32_t* out) {
    out[n] = (int32_t)total[0];
}

/* gather the key bytes into the compact Arrow data buffer */
__global__ __launch_bounds__(BLOCK) void k_json_copykeys(const char* buf,
        const int64_t* kbeg, const int32_t* klen, const int32_t* koff,
        const uint32_t* tot, char* kdata) {
    const uint32_t nt = tot[0];
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < nt;
         r += stride) {
        const char* s = buf + kbeg[r];
        char* d = kdata + koff[r];
        const int32_t l = klen[r];
        for (int32_t j = 0; j < l; j++) d[j] = s[j];
    }
}

void launch_json_count(hipStream_t s, const char* d_buf, int64_t nbytes,
                       int C, int64_t chunk, int32_t tail_record,
                       uint32_t* d_cnt, uint32_t* d_base, uint32_t* d_tot) {
    hipLaunchKernelGGL(k_json_nl_count, dim3(C), dim3(64), 0, s, d_buf, nbytes,
                       chunk, d_cnt);
    hipLaunchKernelGGL(k_json_nl_scan, dim3(1), dim3(64), 0, s, d_cnt, C,
                       d_base, tail_record, d_tot);
}

void launch_json_parse(hipStream_t s, const char* d_buf, int64_t nbytes,
                       int C, int64_t chunk, const JsonFields& jf,
                       const uint32_t* d_base, const uint32_t* d_tot,
                       int64_t* d_recoff, int64_t nrec, int64_t* o_ts,
                       int64_t* o_kbeg, int32_t* o_klen, double* o_val,
                       uint32_t* d_blocksum, uint32_t* d_ktot, int32_t* o_koff,
                       char* o_kdata, uint32_t* d_dbg) {
    hipLaunchKernelGGL(k_json_nl_emit, dim3(C), dim3(64), 0, s, d_buf, nbytes,
                       chunk, d_base, d_tot, d_recoff);
    /* the per-record interpreter is latency/divergence-bound: give it a
     * deep grid so each thread owns ~1 record */
    int pblocks = (int)std::min<int64_t>((nrec + BLOCK - 1) / BLOCK, 32768);
    if (pblocks < 1) pblocks = 1;
    hipLaunchKernelGGL(k_json_parse, dim3(pblocks), dim3(BLOCK), 0, s, d_buf,
                       d_recoff, d_tot, nbytes, jf, o_ts, o_kbeg, o_klen,
                       o_val, d_dbg);
    const int nb = (int)((nrec + JS_ELEMS - 1) / JS_ELEMS);
    hipLaunchKernelGGL(k_scanu32_a, dim3(nb), dim3(BLOCK), 0, s, o_klen,
                       nrec, d_blocksum);
    hipLaunchKernelGGL(k_scanu32_b, dim3(1), dim3(1024), 0, s, d_blocksum, nb,
                       d_ktot);
    hipLaunchKernelGGL(k_scanu32_c, dim3(nb), dim3(BLOCK), 0, s, o_klen,
                       nrec, d_blocksum, o_koff);
    hipLaunchKernelGGL(k_scanu32_tail, dim3(1), dim3(1), 0, s, nrec,
                       d_ktot, o_koff);
    hipLaunchKernelGGL(k_json_copykeys, dim3(pblocks), dim3(BLOCK), 0, s,
                       d_buf, o_kbeg, o_klen, o_koff, d_tot, o_kdata);
}

} // namespace dz

/* synthetic on-wire JSON generator: one newline-delimited record per row of
 * the same seeded sensor stream (emit_measurements.rs shape), reading
 * printed as fixed 6-decimal (inside the decoder's exact parse subset):
 * {"occurred_at_ms":T,"sensor_name":"sensor_K","reading":III.FFFFFF}\n */
namespace dz {

__device__ __forceinline__ void jgen_row(uint64_t seed, int64_t t0,
        int64_t rows_per_ms, int64_t nkeys, int64_t gi, int64_t* ts,
        uint64_t* k, uint64_t* r6) {
    uint64_t r = splitmix64(seed ^ (0x9e3779b97f4a7c15ULL * (uint64_t)(gi + 1)));
    *k = r % (uint64_t)nkeys;
    *ts = t0 + gi / rows_per_ms;
    const double v =
        (double)(splitmix64(r) >> 11) * (1.0 / 9007199254740992.0) * 115.0;
    *r6 = (uint64_t)(v * 1e6 + 0.5);
}

__global__ void k_gen_json_lens(uint64_t seed, int64_t t0, int64_t start_row,
                                int64_t n, int64_t nkeys, int64_t rows_per_ms,
                                int32_t* lens) {
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int64_t ts;
        uint64_t k, r6;
        jgen_row(seed, t0, rows_per_ms, nkeys, start_row + i, &ts, &k, &r6);
        lens[i] = 18 + dec_digits((uint64_t)ts) + 23 + dec_digits(k) + 12 +
                  dec_digits(r6 / 1000000) + 1 + 6 + 2;
    }
}

__device__ __forceinline__ char* jgen_u64(char* p, uint64_t v) {
    const int32_t d = dec_digits(v);
    for (int32_t j = d - 1; j >= 0; j--) {
        p[j] = (char)('0' + (v % 10));
        v /= 10;
    }
    return p + d;
}

__global__ void k_gen_json_fill(uint64_t seed, int64_t t0, int64_t start_row,
                                int64_t n, int64_t nkeys, int64_t rows_per_ms,
                                const int64_t* offs, char* data) {
    const char* A = "{\"occurred_at_ms\":";
    const char* B = ",\"sensor_name\":\"sensor_";
    const char* Cs = "\",\"reading\":";
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n;
         i += stride) {
        int64_t ts;
        uint64_t k, r6;
        jgen_row(seed, t0, rows_per_ms, nkeys, start_row + i, &ts, &k, &r6);
        char* p = data + offs[i];
        for (int j = 0; j < 18; j++) *p++ = A[j];
        p = jgen_u64(p, (uint64_t)ts);
        for (int j = 0; j < 23; j++) *p++ = B[j];
        p = jgen_u64(p, k);
        for (int j = 0; j < 12; j++) *p++ = Cs[j];
        p = jgen_u64(p, r6 / 1000000);
        *p++ = '.';
        uint64_t f = r6 % 1000000;
        for (int32_t j = 5; j >= 0; j--) {
            p[j] = (char)('0' + (f % 10));
            f /= 10;
        }
        p += 6;
        *p++ = '}';
        *p++ = '\n';
    }
}

void launch_gen_json(hipStream_t s, uint64_t seed, int64_t t0,
                     int64_t start_row, int64_t n, int64_t nkeys,
                     int64_t rows_per_ms, int32_t* d_lens,
                     const int64_t* d_offs, char* d_data) {
    int blocks = (int)std::min<int64_t>((n + BLOCK - 1) / BLOCK, 2048);
    if (blocks < 1) blocks = 1;
    if (d_lens)
        hipLaunchKernelGGL(k_gen_json_lens, dim3(blocks), dim3(BLOCK), 0, s,
                           seed, t0, start_row, n, nkeys, rows_per_ms, d_lens);
    if (d_data)
        hipLaunchKernelGGL(k_gen_json_fill, dim3(blocks), dim3(BLOCK), 0, s,
                           seed, t0, start_row, n, nkeys, rows_per_ms, d_offs,
                           d_data);
}

} // namespace dz

/* ------------------------------------------------------------------ */
/* small-N emission sort: ONE launch replacing the ~15-launch          */
/* multi-block radix chain when few groups pass the filter (cfg3's     */
/* sliding closes pass ~1-2% of 1M keys). Single block, in-kernel      */
/* passes, stable: all waves build the digit histogram, wave 0 places  */
/* elements in order (ballot ranks + LDS cursors). Correct for ANY nt  */
/* — just slow when large — so an adaptive host misprediction costs    */
/* time, never correctness.                                            */
/* ------------------------------------------------------------------ */

namespace dz {

__global__ __launch_bounds__(BLOCK) void k_esort_small(uint64_t* ka,
        uint32_t* pa, uint64_t* kb, uint32_t* pb, const uint32_t* counter2,
        int passes /* even */) {
    __shared__ uint32_t hist[RBINS];
    __shared__ uint32_t scanbuf[BLOCK];
    const uint32_t nt = *counter2;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    for (int p = 0; p < passes; p++) {
        const int shift = p * RDIG;
        for (int t = threadIdx.x; t < RBINS; t += BLOCK) hist[t] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nt; i += BLOCK)
            atomicAdd(&hist[(uint32_t)(ka[i] >> shift) & (RBINS - 1)], 1u);
        __syncthreads();
        { /* exclusive scan of 2048 bins: 8 per thread + block scan */
            constexpr int PER = RBINS / BLOCK;
            uint32_t loc[PER];
            uint32_t s = 0;
            for (int j = 0; j < PER; j++) {
                loc[j] = s;
                s += hist[threadIdx.x * PER + j];
            }
            scanbuf[threadIdx.x] = s;
            __syncthreads();
            for (int o = 1; o < BLOCK; o <<= 1) {
                uint32_t v = (threadIdx.x >= (unsigned)o)
                                 ? scanbuf[threadIdx.x - o] : 0;
                __syncthreads();
                scanbuf[threadIdx.x] += v;
                __syncthreads();
            }
            const uint32_t pre = threadIdx.x ? scanbuf[threadIdx.x - 1] : 0;
            for (int j = 0; j < PER; j++)
                hist[threadIdx.x * PER + j] = pre + loc[j];
            __syncthreads();
        }
        /* stable placement by wave 0 (ballot ranks + LDS cursors) */
        if (wave == 0) {
            for (uint32_t i0 = 0; i0 < nt; i0 += 64) {
                const uint32_t i = i0 + lane;
                const bool act = i < nt;
                const uint64_t key = act ? ka[i] : ~0ULL;
                const uint32_t d =
                    act ? ((uint32_t)(key >> shift) & (RBINS - 1)) : 0xFFFFu;
                uint64_t same = ~0ULL;
                for (int b = 0; b < RDIG; b++) {
                    uint64_t bb = __ballot((d >> b) & 1);
                    same &= ((d >> b) & 1) ? bb : ~bb;
                }
                {
                    uint64_t bb = __ballot(act);
                    same &= act ? bb : ~bb;
                }
                const uint64_t below =
                    (lane == 63) ? ~0ULL : ((1ULL << (lane + 1)) - 1);
                const int rank = (int)__popcll(same & below) - 1;
                const int leader = __ffsll((unsigned long long)same) - 1;
                const uint32_t wtot = (uint32_t)__popcll(same);
                uint32_t pos = 0;
                {
                    uint32_t pre = 0;
                    if (lane == leader && act) {
                        pre = hist[d];
                        hist[d] = pre + wtot;
                    }
                    pre = (uint32_t)__shfl((int)pre, leader);
                    pos = pre + (uint32_t)rank;
                }
                if (act) {
                    kb[pos] = key;
                    pb[pos] = pa[i];
                }
            }
        }
        __syncthreads();
        uint64_t* tk = ka; ka = kb; kb = tk;
        uint32_t* tp = pa; pa = pb; pb = tp;
    }
}

void launch_esort_small(hipStream_t s, uint64_t* fkeys, uint64_t* skeys,
                        uint32_t* fiota, uint32_t* okid, uint32_t* counter2,
                        uint64_t max_key) {
    int passes = 0;
    while (passes * RDIG < 64 && (max_key >> (passes * RDIG)) != 0) passes++;
    if (passes & 1) passes++;
    if (passes < 2) passes = 2;
    /* even passes => sorted (key, payload) land back in fkeys/fiota, the
     * same contract as the multi-block chain */
    hipLaunchKernelGGL(k_esort_small, dim3(1), dim3(BLOCK), 0, s, fkeys,
                       fiota, skeys, okid, counter2, passes);
}

} // namespace dz

/* ------------------------------------------------------------------ */
/* GROUP-BATCHED device emission: one chain for a whole trigger group  */
/* of <= 16 closing windows (the per-close chain cost ~17 host         */
/* enqueues; cfg3's sliding steps close ~80 windows, and the push      */
/* thread's enqueue serialization was the wall). Composite sort key =  */
/* close_idx << cshift | first_seen_row, so ONE radix sort yields      */
/* close-major, insertion-ordered rows for every close at once.        */
/* ------------------------------------------------------------------ */

namespace dz {

/* fused compact+filter+gather over all closes of the group: grid.y = close
 * index; element positions come from one global atomic counter (order is
 * irrelevant pre-sort); per-close row counts accumulate in gcnt[] */
__global__ __launch_bounds__(BLOCK) void k_egf(const uint64_t* s_base,
        int64_t stride_u64, EGatherSlots slots, int64_t K, int64_t kcap,
        EmitFilter ef, int cshift, uint64_t* gkeys, uint32_t* gkid,
        uint32_t* giota, uint64_t* gcnt_col, double* gmin, double* gmax,
        double* gsum, double* gavg, uint8_t* gflags, uint32_t* gtot,
        uint32_t* gcnt) {
    const int c = blockIdx.y;
    const uint64_t* sl = s_base + (int64_t)slots.s[c] * stride_u64;
    const uint64_t* f_cnt = sl;
    const uint64_t* f_first = sl + kcap;
    const double* f_min = (const double*)(sl + 2 * kcap);
    const double* f_max = (const double*)(sl + 3 * kcap);
    const double* f_sum = (const double*)(sl + 4 * kcap);
    __shared__ uint32_t base;
    __shared__ uint32_t wsum[WAVES_PER_BLOCK];
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t k0 = (int64_t)blockIdx.x * blockDim.x; k0 < K; k0 += stride) {
        const int64_t k = k0 + threadIdx.x;
        uint64_t f = (k < K) ? f_first[k] : ~0ULL;
        bool pass = f != ~0ULL;
        uint64_t cnt = 0;
        if (pass) {
            cnt = f_cnt[k];
            if (ef.on)
                pass = slab_filter_pass(ef, cnt, f_min, f_max, f_sum, k);
        }
        uint32_t tot;
        const uint32_t p = block_compact_pos(pass, gtot, wsum, &base, &tot);
        if (threadIdx.x == 0 && tot) atomicAdd(&gcnt[c], tot);
        if (pass) {
            const bool valid = cnt > 0;
            gkeys[p] = ((uint64_t)c << cshift) | (f - slots.base[c]);
            gkid[p] = (uint32_t)k;
            giota[p] = p; /* sort payload: identity permutation */
            gcnt_col[p] = cnt;
            gmin[p] = valid ? f_min[k] : 0.0;
            gmax[p] = valid ? f_max[k] : 0.0;
            gsum[p] = valid ? f_sum[k] : 0.0;
            gavg[p] = valid ? f_sum[k] / (double)cnt : 0.0;
            gflags[p] = valid ? 1 : 0;
        }
        __syncthreads();
    }
}

void launch_emission_group_read(hipStream_t s, const uint64_t* s_base,
                                int64_t stride_u64, const EGatherSlots& slots,
                                int gcount, int64_t K, int64_t kcap,
                                const EmitFilter& ef, int cshift,
                                uint64_t* gkeys, uint32_t* gkid,
                                uint32_t* giota, uint64_t* gcnt_col,
                                double* gmin, double* gmax, double* gsum,
                                double* gavg, uint8_t* gflags, uint32_t* gtot,
                                uint32_t* gcnt) {
    int cblocks = (int)std::min<int64_t>((K + BLOCK - 1) / BLOCK, 1024);
    hipLaunchKernelGGL(k_egf, dim3(cblocks, gcount), dim3(BLOCK), 0, s, s_base,
                       stride_u64, slots, K, kcap, ef, cshift, gkeys, gkid,
                       giota, gcnt_col, gmin, gmax, gsum, gavg, gflags, gtot,
                       gcnt);
}

void launch_emission_group_sort(hipStream_t s, int64_t elem_cap, int gcount,
                                int cshift, uint64_t max_first,
                                uint64_t* gkeys, uint64_t* gskeys,
                                uint32_t* gkid, uint32_t* gokid,
                                uint32_t* giota, uint64_t* gcnt_col,
                                double* gmin, double* gmax, double* gsum,
                                double* gavg, uint8_t* gflags, uint32_t* gtot,
                                uint32_t* rhist, uint32_t* roffs, char* pout) {
    /* one multi-block radix chain over the whole group's elements; the
     * key bound covers close_idx << cshift */
    uint64_t max_key = ((uint64_t)gcount << cshift) | max_first;
    launch_emission_sort(s, elem_cap, gkeys, gskeys, giota, gokid, gtot,
                         rhist, roffs, max_key);
    int pb = (int)std::min<int64_t>((elem_cap + BLOCK - 1) / BLOCK, 2048);
    /* pack the sorted group close-major: the per-close permute kernel,
     * keyed off the composite-sorted permutation */
    hipLaunchKernelGGL(k_epermute, dim3(pb), dim3(BLOCK), 0, s, gtot, giota,
                       gkid, gcnt_col, gmin, gmax, gsum, gavg, gflags, pout);
}

/* ------------------------------------------------------------------ */
/* MEDIAN (DZ_AGG_MEDIAN): per-slot value log + order statistic at     */
/* close                                           */
/* ------------------------------------------------------------------ */
/* An exact median cannot fold into registers: every valid value of an open
 * window is appended to its slot's log as (dense key id, value), and at
 * close the log is scattered into per-group segments and one block per
 * group radix-selects the middle order statistic(s). The median does not
 * depend on row order, so placement uses atomics and stays bit-exact. */

constexpr int MED_TILE = 2048;             /* rows per count/append block */
constexpr int MED_RPT = MED_TILE / BLOCK;  /* rows one thread holds */

/* The windows of this block's row tile: each thread's rows keep (first widx,
 * multiplicity) in registers — the same membership rule as k_hist/k_scatter_t
 * (row_windows), multiplicity 0 for NULL rows — and the block's touched
 * widx range [*wlo, *wlo + *span) comes back through s_range. */
__device__ __forceinline__ void med_tile_windows(
        const int64_t* __restrict__ ts, const uint8_t* __restrict__ validity,
        int64_t n, const WinParams& wp, int32_t (&jm)[MED_RPT],
        int32_t (&m)[MED_RPT], int32_t* s_range, int32_t* wlo, int32_t* span) {
    if (threadIdx.x == 0) {
        s_range[0] = INT32_MAX;
        s_range[1] = -1;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * MED_TILE;
    int32_t lo = INT32_MAX, hi = -1;
#pragma unroll
    for (int k = 0; k < MED_RPT; k++) {
        const int64_t i = base + k * BLOCK + threadIdx.x;
        jm[k] = 0;
        m[k] = 0;
        if (i < n && (!validity || ((validity[i >> 3] >> (i & 7)) & 1))) {
            int32_t j, mm;
            row_windows(ts[i], wp, &j, &mm);
            if (mm > 0 && j >= 0 && j + mm <= wp.nw) {
                jm[k] = j;
                m[k] = mm;
                lo = min(lo, j);
                hi = max(hi, j + mm - 1);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_down(lo, o));
        hi = max(hi, __shfl_down(hi, o));
    }
    if ((threadIdx.x & 63) == 0 && hi >= 0) {
        atomicMin(&s_range[0], lo);
        atomicMax(&s_range[1], hi);
    }
    __syncthreads();
    *wlo = s_range[0];
    *span = s_range[1] >= s_range[0] ? s_range[1] - s_range[0] + 1 : 0;
}

/* valid rows of this batch per window: LDS counters over the block's widx
 * range, then ONE global atomic per (block, touched window) */
__global__ __launch_bounds__(BLOCK) void k_med_count(
        const int64_t* __restrict__ ts, const uint8_t* __restrict__ validity,
        int64_t n, WinParams wp, uint32_t* __restrict__ wcnt) {
    __shared__ uint32_t lcnt[MAX_RANGES];
    __shared__ int32_t s_range[2];
    int32_t jm[MED_RPT], m[MED_RPT], wlo, span;
    med_tile_windows(ts, validity, n, wp, jm, m, s_range, &wlo, &span);
    for (int t = threadIdx.x; t < span; t += BLOCK) lcnt[t] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MED_RPT; k++)
        for (int32_t j = 0; j < m[k]; j++)
            atomicAdd(&lcnt[jm[k] - wlo + j], 1u);
    __syncthreads();
    for (int t = threadIdx.x; t < span; t += BLOCK) {
        const uint32_t c = lcnt[t];
        if (c) atomicAdd(&wcnt[wlo + t], c);
    }
}

/* append (key id, value) of every valid row to the log of each window that
 * contains it: the block reserves one range per touched window with a single
 * global atomic on the batch's per-window fill counter; positions inside the
 * range come from LDS atomics. win[w].base is the log length before this
 * batch (host-tracked, exact), win[w].cap its capacity — the bounds guard. */
__global__ __launch_bounds__(BLOCK) void k_med_append(
        const int64_t* __restrict__ ts, const uint8_t* __restrict__ validity,
        const int32_t* __restrict__ kid, const double* __restrict__ vals,
        int64_t n, WinParams wp, const MedWin* __restrict__ win,
        uint32_t* __restrict__ fill, uint32_t* __restrict__ dbg) {
    __shared__ uint32_t lcnt[MAX_RANGES];
    __shared__ int32_t s_range[2];
    int32_t jm[MED_RPT], m[MED_RPT], wlo, span;
    med_tile_windows(ts, validity, n, wp, jm, m, s_range, &wlo, &span);
    for (int t = threadIdx.x; t < span; t += BLOCK) lcnt[t] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < MED_RPT; k++)
        for (int32_t j = 0; j < m[k]; j++)
            atomicAdd(&lcnt[jm[k] - wlo + j], 1u);
    __syncthreads();
    /* the cell turns from the block's count into its reserved start */
    for (int t = threadIdx.x; t < span; t += BLOCK) {
        const uint32_t c = lcnt[t];
        lcnt[t] = c ? atomicAdd(&fill[wlo + t], c) : 0u;
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * MED_TILE;
#pragma unroll
    for (int k = 0; k < MED_RPT; k++) {
        if (m[k] == 0) continue;
        const int64_t i = base + k * BLOCK + threadIdx.x;
        const uint32_t kd = (uint32_t)kid[i];
        const double v = vals[i];
        for (int32_t j = 0; j < m[k]; j++) {
            const int32_t w = jm[k] + j;
            const uint32_t r = atomicAdd(&lcnt[w - wlo], 1u);
            const MedWin mw = win[w];
            const uint64_t pos = (uint64_t)mw.base + r;
            if (pos < mw.cap) {
                mw.kid[pos] = kd;
                mw.val[pos] = v;
            } else {
                dbg[2] = 1; /* bounds guard: flag, never corrupt */
            }
        }
    }
}

void launch_med_count(hipStream_t s, const int64_t* d_ts,
                      const uint8_t* d_validity, int64_t n,
                      const WinParams& wp, uint32_t* d_wcnt) {
    const int grid = (int)((n + MED_TILE - 1) / MED_TILE);
    hipLaunchKernelGGL(k_med_count, dim3(grid), dim3(BLOCK), 0, s, d_ts,
                       d_validity, n, wp, d_wcnt);
}

void launch_med_append(hipStream_t s, const int64_t* d_ts,
                       const uint8_t* d_validity, const int32_t* d_kid,
                       const double* d_vals, int64_t n, const WinParams& wp,
                       const MedWin* d_win, uint32_t* d_fill,
                       uint32_t* d_dbg) {
    const int grid = (int)((n + MED_TILE - 1) / MED_TILE);
    hipLaunchKernelGGL(k_med_append, dim3(grid), dim3(BLOCK), 0, s, d_ts,
                       d_validity, d_kid, d_vals, n, wp, d_win, d_fill, d_dbg);
}

/* segment offsets of a closing slot: exclusive scan of its per-group valid
 * counts (the primary column's s_cnt is exactly each group's segment
 * length). Three kernels, MED_SCAN_ELEMS groups per block: block sums, a
 * single-block scan of those, then the offsets — which also zeroes the
 * per-group fill cursors of k_med_place. */
constexpr int MED_SCAN_ELEMS = 2048;
constexpr int MED_SCAN_PT = MED_SCAN_ELEMS / BLOCK;

__global__ __launch_bounds__(BLOCK) void k_med_scan_a(
        const uint64_t* __restrict__ cnt, int64_t K,
        uint32_t* __restrict__ bsum) {
    __shared__ uint32_t wtot[WAVES_PER_BLOCK];
    const int64_t base =
        (int64_t)blockIdx.x * MED_SCAN_ELEMS + threadIdx.x * MED_SCAN_PT;
    uint32_t s = 0;
#pragma unroll
    for (int e = 0; e < MED_SCAN_PT; e++)
        if (base + e < K) s += (uint32_t)cnt[base + e];
    uint32_t tot;
    block_scan_excl(s, wtot, &tot);
    if (threadIdx.x == 0) bsum[blockIdx.x] = tot;
}

__global__ __launch_bounds__(BLOCK) void k_med_scan_b(
        uint32_t* __restrict__ bsum, int nblk) {
    __shared__ uint32_t wtot[WAVES_PER_BLOCK];
    uint32_t carry = 0;
    for (int b0 = 0; b0 < nblk; b0 += BLOCK) {
        const int b = b0 + threadIdx.x;
        const uint32_t v = b < nblk ? bsum[b] : 0u;
        uint32_t tot;
        const uint32_t ex = block_scan_excl(v, wtot, &tot);
        if (b < nblk) bsum[b] = carry + ex;
        carry += tot;
        __syncthreads(); /* wtot is rewritten by the next round */
    }
}

__global__ __launch_bounds__(BLOCK) void k_med_scan_c(
        const uint64_t* __restrict__ cnt, int64_t K,
        const uint32_t* __restrict__ bsum, uint32_t* __restrict__ seg_off,
        uint32_t* __restrict__ fill) {
    __shared__ uint32_t wtot[WAVES_PER_BLOCK];
    const int64_t base =
        (int64_t)blockIdx.x * MED_SCAN_ELEMS + threadIdx.x * MED_SCAN_PT;
    uint32_t c[MED_SCAN_PT];
    uint32_t s = 0;
#pragma unroll
    for (int e = 0; e < MED_SCAN_PT; e++) {
        c[e] = base + e < K ? (uint32_t)cnt[base + e] : 0u;
        s += c[e];
    }
    uint32_t tot;
    uint32_t ex = block_scan_excl(s, wtot, &tot) + bsum[blockIdx.x];
#pragma unroll
    for (int e = 0; e < MED_SCAN_PT; e++) {
        if (base + e < K) {
            seg_off[base + e] = ex;
            fill[base + e] = 0;
        }
        ex += c[e];
    }
}

void launch_med_scan(hipStream_t s, const uint64_t* d_cnt, int64_t K,
                     uint32_t* d_bsum, uint32_t* d_seg_off, uint32_t* d_fill) {
    const int nblk = (int)((K + MED_SCAN_ELEMS - 1) / MED_SCAN_ELEMS);
    if (nblk < 1) return;
    hipLaunchKernelGGL(k_med_scan_a, dim3(nblk), dim3(BLOCK), 0, s, d_cnt, K,
                       d_bsum);
    hipLaunchKernelGGL(k_med_scan_b, dim3(1), dim3(BLOCK), 0, s, d_bsum, nblk);
    hipLaunchKernelGGL(k_med_scan_c, dim3(nblk), dim3(BLOCK), 0, s, d_cnt, K,
                       d_bsum, d_seg_off, d_fill);
}

/* scatter the log's values into their groups' segments, one thread per
 * entry: destination = seg_off[kid] + atomicAdd(&fill[kid], 1) — the order
 * inside a segment is irrelevant to an order statistic. A wave whose entries
 * all share one key (a global window; long runs of one sensor) reserves its
 * range with one atomic. Guards (dbg[2]): a key id outside [0, K) or a
 * destination outside the slot's `len` entries is skipped and flagged. */
__global__ __launch_bounds__(BLOCK) void k_med_place(
        const uint32_t* __restrict__ lkid, const double* __restrict__ lval,
        uint32_t len, const uint32_t* __restrict__ seg_off,
        uint32_t* __restrict__ fill, uint32_t K, double* __restrict__ sorted,
        uint32_t* __restrict__ dbg) {
    const uint32_t i = blockIdx.x * BLOCK + threadIdx.x;
    const bool act = i < len;
    const uint32_t kd = act ? lkid[i] : 0xFFFFFFFFu;
    const bool ok = act && kd < K;
    if (act && !ok) dbg[2] = 2;
    const uint64_t am = __ballot(ok);
    if (!am) return; /* wave-uniform */
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((long long)am) - 1;
    const uint32_t k0 = (uint32_t)__shfl((int)kd, leader);
    uint32_t r = 0;
    if (__ballot(ok && kd != k0) == 0) {
        uint32_t b = 0;
        if (lane == leader) b = atomicAdd(&fill[k0], (uint32_t)__popcll(am));
        b = (uint32_t)__shfl((int)b, leader);
        r = b + (uint32_t)__popcll(am & ((1ULL << lane) - 1));
    } else if (ok) {
        r = atomicAdd(&fill[kd], 1u);
    }
    if (ok) {
        const uint64_t dst = (uint64_t)seg_off[kd] + r;
        if (dst < len) sorted[dst] = lval[i];
        else dbg[2] = 3;
    }
}

void launch_med_place(hipStream_t s, const uint32_t* d_lkid,
                      const double* d_lval, int64_t len,
                      const uint32_t* d_seg_off, uint32_t* d_fill, int64_t K,
                      double* d_sorted, uint32_t* d_dbg) {
    if (len <= 0) return;
    const int grid = (int)((len + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(k_med_place, dim3(grid), dim3(BLOCK), 0, s, d_lkid,
                       d_lval, (uint32_t)len, d_seg_off, d_fill, (uint32_t)K,
                       d_sorted, d_dbg);
}

/* IEEE total order as an unsigned key (-NaN < -inf < ... < -0 < +0 < ... <
 * +inf < +NaN): bits ^ (sign ? ~0 : 1 << 63), and back */
__device__ __forceinline__ uint64_t med_key(double v) {
    const uint64_t b = (uint64_t)__double_as_longlong(v);
    return b ^ ((b >> 63) ? ~0ULL : 0x8000000000000000ULL);
}
__device__ __forceinline__ double med_unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? (k ^ 0x8000000000000000ULL) : ~k;
    return __longlong_as_double((long long)b);
}

/* One block per group: MSD radix select (8 passes of 8 bits) on the 64-bit
 * total-order key for rank (n-1)/2. Each pass histograms the digit of the
 * candidates that still match the selected prefix, scans the 256 bins across
 * the block and narrows to the bin holding the rank; the running count of
 * keys below the prefix and the final bin's size say, for even n, whether
 * rank n/2 is the same value (ties) — otherwise it is the minimum of the
 * keys above, one more pass. Segments of at most MED_LDS_VALS values are
 * loaded ONCE into LDS as keys and selected there; longer ones run the same
 * passes over global memory. A wave whose candidates all carry one digit
 * (common: the high bytes of same-magnitude readings) adds its count with a
 * single LDS atomic.
 * LDS: 16 KiB keys + 1 KiB bins => 9 blocks/CU by LDS, 8 by the 32-wave
 * cap: full occupancy at BLOCK = 256 (DESIGN.md §Median has the figures). */
static_assert(BLOCK == 256, "k_med_select scans one digit bin per thread");
__global__ __launch_bounds__(BLOCK) void k_med_select(
        const uint64_t* __restrict__ cnt, const uint32_t* __restrict__ seg_off,
        const double* __restrict__ sorted, uint32_t len,
        double* __restrict__ med, uint32_t* __restrict__ dbg) {
    __shared__ uint64_t keys[MED_LDS_VALS];
    __shared__ uint32_t hist[256];
    __shared__ uint32_t wtot[WAVES_PER_BLOCK];
    __shared__ uint32_t s_sel[3]; /* digit, rank inside its bin, bin size */
    __shared__ unsigned long long s_min;
    const uint32_t k = blockIdx.x;
    const uint64_t n64 = cnt[k];
    if (n64 == 0) { /* block-uniform: NULL group, the host emits 0.0 */
        if (threadIdx.x == 0) med[k] = 0.0;
        return;
    }
    const uint32_t off = seg_off[k];
    if ((uint64_t)off + n64 > len) { /* bounds guard: flag, never read past */
        if (threadIdx.x == 0) {
            med[k] = 0.0;
            dbg[2] = 4;
        }
        return;
    }
    const uint32_t n = (uint32_t)n64;
    const double* __restrict__ seg = sorted + off;
    const bool in_lds = n <= (uint32_t)MED_LDS_VALS;
    const int lane = threadIdx.x & 63;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i < n; i += BLOCK)
            keys[i] = med_key(seg[i]);
    }
    if (threadIdx.x == 0) s_min = ~0ULL;
    __syncthreads();
    uint64_t prefix = 0, mask = 0;
    uint32_t r = (n - 1) / 2; /* rank still to find among the candidates */
    uint32_t below = 0;       /* keys strictly below the prefix */
    uint32_t eq = n;          /* candidates matching the prefix */
    for (int shift = 56; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (uint32_t b0 = 0; b0 < n; b0 += BLOCK) {
            const uint32_t i = b0 + threadIdx.x;
            bool hit = false;
            uint32_t d = 0;
            if (i < n) {
                const uint64_t key = in_lds ? keys[i] : med_key(seg[i]);
                hit = (key & mask) == prefix;
                d = (uint32_t)(key >> shift) & 255u;
            }
            const uint64_t hm = __ballot(hit);
            if (hm) {
                const int leader = __ffsll((long long)hm) - 1;
                const uint32_t d0 = (uint32_t)__shfl((int)d, leader);
                if (__ballot(hit && d != d0) == 0) {
                    if (lane == leader)
                        atomicAdd(&hist[d0], (uint32_t)__popcll(hm));
                } else if (hit) {
                    atomicAdd(&hist[d], 1u);
                }
            }
        }
        __syncthreads();
        const uint32_t c = hist[threadIdx.x];
        uint32_t tot;
        const uint32_t ex = block_scan_excl(c, wtot, &tot);
        if (c && ex <= r && r < ex + c) {
            s_sel[0] = threadIdx.x;
            s_sel[1] = r - ex;
            s_sel[2] = c;
        }
        __syncthreads();
        below += r - s_sel[1];
        r = s_sel[1];
        eq = s_sel[2];
        prefix |= (uint64_t)s_sel[0] << shift;
        mask |= 0xFFULL << shift;
    }
    uint64_t hi_key = prefix;
    if ((n & 1) == 0 && below + eq <= n / 2) {
        /* block-uniform: rank n/2 is the smallest key above the selected */
        uint64_t mn = ~0ULL;
        for (uint32_t i = threadIdx.x; i < n; i += BLOCK) {
            const uint64_t key = in_lds ? keys[i] : med_key(seg[i]);
            if (key > prefix && key < mn) mn = key;
        }
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t u =
                (uint64_t)__shfl_down((unsigned long long)mn, o);
            mn = u < mn ? u : mn;
        }
        if (lane == 0) atomicMin(&s_min, (unsigned long long)mn);
        __syncthreads();
        hi_key = s_min;
    }
    if (threadIdx.x == 0) {
        const double lo = med_unkey(prefix);
        /* even n: one f64 add, one f64 divide, each rounded on its own —
         * also when both middles are equal (1e308 + 1e308 overflows) */
        med[k] = (n & 1) ? lo : (lo + med_unkey(hi_key)) / 2.0;
    }
}

void launch_med_select(hipStream_t s, const uint64_t* d_cnt,
                       const uint32_t* d_seg_off, const double* d_sorted,
                       int64_t len, int64_t K, double* d_med,
                       uint32_t* d_dbg) {
    if (K <= 0) return;
    hipLaunchKernelGGL(k_med_select, dim3((uint32_t)K), dim3(BLOCK), 0, s,
                       d_cnt, d_seg_off, d_sorted, (uint32_t)len, d_med, d_dbg);
}

} // namespace dz
