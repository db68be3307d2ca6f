// Internal (host-side) declarations shared by the plan, the device shim and
// the drop-in C-ABI.  Nothing here crosses the public C-ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <vector>

#include "matrix_pack.h"   // MatLayout: the packed matrix block
#include "matrix_route.h"  // kRouteTile, matrix_kp, matrix_route

namespace qi {

// OOR routing: the decode context keeps, per stripe and per tile of
// kRouteTile (matrix_route.h) columns, the marks of the received rows that
// fall in the tile (count + up to kRouteCap entries packed as position << 16
// | column-in-tile).  A count above kRouteCap makes the decode kernel scan
// the OOR buckets.
constexpr int kRouteCap = 15;
constexpr int kRouteStride = kRouteCap + 1;

__host__ __device__ inline long long route_tiles(long long words)
{
    return (words + kRouteTile - 1) / kRouteTile;
}

// Sticky device error bits (qi_gpu_take_error): an OOR bucket held more
// marks than its capacity `cap`, so some marks were lost (encode keeps the
// exact count, decode could not restore every 65536 symbol).
constexpr uint32_t kErrOorTruncated = 1u;
// A decode context was asked for with received ids that are not distinct or
// not below n (the erasure decode's context, which derives the erased set
// from them, checks; the context is then unusable and nothing outside it is
// written).
constexpr uint32_t kErrBadIds = 2u;

// Row source for the matrix kernel: fragment `id` of stripe `s` is at
//   id <  split : base0 + s*ss0 + id*rs0
//   id >= split : base1 + s*ss1 + (id-split)*rs1        (elements of u16)
//   by_pos != 0: row (and OOR slot) of the i-th received fragment is found
//   by its position i instead of its id (compact staging of the block API)
struct RowSrc {
    const uint16_t* base0;
    long long ss0, rs0;
    int split;
    const uint16_t* base1;
    long long ss1, rs1;
    int by_pos;
    int rows0, rows1;  // rows addressable through base0 / base1
};

// Output rows: row t of stripe s at base + s*ss + t*rs
struct RowDst {
    uint16_t* base;
    long long ss, rs;
};

// OOR buckets: counts[s*slots + slot], entries[(s*slots + slot)*cap + e]
struct Oor {
    uint32_t* counts;
    uint32_t* entries;
    int slots;
    int cap;
};

// Per-stripe list of the column tiles whose received-row OOR marks overflowed
// the matrix kernels' LDS list (more than 256 in one tile; adversarial
// data).  Kept in the decode context: word 0 = count, then one word per
// tile (col0 / 64) << 3 | log2(width / 64).  Every kernel tile is a
// power-of-two multiple of kSlowGrain = 64 columns (the narrowest, KS = 16
// matrix-core blocks) starting on a multiple of its width, and each tile is
// pushed at most once per launch, so capacity slow_words(words) - 1 =
// ceil(words / 64) covers every tile of a stripe.  launch_matrix runs
// matrix_redo_kernel over it right after the matrix kernels.
struct SlowList {
    uint32_t* base;  // stripe s at base + s * stride (nullptr: no input marks)
    long long stride;
};

constexpr int kSlowGrain = 64;

__host__ __device__ inline long long slow_words(long long words)
{
    return 1 + (words + kSlowGrain - 1) / kSlowGrain;
}

// A matrix context's lazy-section word (behind its slow-tile list, per
// stripe, cleared by the context builder): the sections a decode fills on
// first use, when the batch's rows keep it off the matrix cores -- bit 0
// the dot2 sections (fill_dot2_sections), bit 1 the NTT engine's context of
// a 256 < k <= 384 plan (ntt_build_ctx_lazy).  Offset from the route table.
constexpr uint32_t kLazyDot2 = 1u, kLazyNtt = 2u;
__host__ __device__ inline long long lazy_word_off(long long words)
{
    return route_tiles(words) * kRouteStride + slow_words(words);
}
// words reserved for it (keeps the following section's alignment)
constexpr int kLazyWords = 4;

// The sections of a matrix context (decode or repair) behind its packed block
// L, for `words` columns, stripes `stride` words apart: the ids as dwords
// (padded to 2 KP), the route table, the slow-tile list, the lazy word.  The
// context builders' kernels write them at these offsets (ctx.hip).
struct MatCtxView {
    int32_t* ctx;
    long long stride;
    long long ids_off, route_off, slow_off, lazy_off;
    MatCtxView(const MatLayout& L, const void* d_ctx, long long stride_, long long words)
        : ctx(static_cast<int32_t*>(const_cast<void*>(d_ctx))), stride(stride_),
          ids_off(static_cast<long long>(L.words())), route_off(ids_off + 2 * L.KP),
          slow_off(route_off + route_tiles(words) * kRouteStride),
          lazy_off(route_off + lazy_word_off(words))
    {
    }
    // words of a stripe's matrix-format context
    long long size() const { return lazy_off + kLazyWords; }
    const int32_t* ids() const { return ctx + ids_off; }
    const uint32_t* route() const { return reinterpret_cast<const uint32_t*>(ctx + route_off); }
    SlowList slow() const { return {reinterpret_cast<uint32_t*>(ctx + slow_off), stride}; }
    uint32_t* lazy() const { return reinterpret_cast<uint32_t*>(ctx + lazy_off); }
};

// Once-per-device setup of a kernel (dynamic-LDS opt-in, cached device
// facts).  `done` is the kernel's own bit per device index below
// kOnceDevices: setup(dev) runs until it has succeeded once on the current
// device (a race only repeats the idempotent calls), and on every call for
// an index of kOnceDevices or above, where nothing can be cached.  Returns
// the device index, or -2 when the device query or the setup fails (the bit
// stays unset).
constexpr int kOnceDevices = 64;
template <class F>
int once_per_device(std::atomic<uint64_t>& done, F&& setup)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return -2;
    const uint64_t bit = dev < kOnceDevices ? 1ull << dev : 0;
    if (!bit || !(done.load(std::memory_order_acquire) & bit)) {
        if (!setup(dev))
            return -2;
        done.fetch_or(bit, std::memory_order_release);
    }
    return dev;
}

// The context builders' kernel by shape, as their block size: launch_decode_ctx
// runs decode_ctx_kernel<1024, true> (the matrix rows in the context itself)
// above k = 128, else decode_ctx_lds_kernel<256 or 128> (2 waves at k <= 32:
// wave 1 routes the marks while wave 0 builds A(x)); launch_repair_ctx runs
// repair_ctx_kernel<64> for at most 16 x 68 words of rows, else <256>.
inline int decode_ctx_threads(int k)
{
    return k > 128 ? 1024 : k > 32 ? 256 : 128;
}
inline int repair_ctx_threads(int k, int R)
{
    return k <= 64 && R <= 16 ? 64 : 256;
}
inline std::string decode_ctx_kernel_name(int k)
{
    const int t = decode_ctx_threads(k);
    return t == 1024 ? "decode_ctx_kernel<1024, true>"
                     : "decode_ctx_lds_kernel<" + std::to_string(t) + ">";
}
inline std::string repair_ctx_kernel_name(int k, int R)
{
    return "repair_ctx_kernel<" + std::to_string(repair_ctx_threads(k, R)) + ">";
}

// the bucket comparison a fused check ends with (launch_verify_marks)
inline std::string verify_marks_kernel_name()
{
    return "verify_marks_kernel";
}

// ---- launchers (kernels.hip) ----
// non-systematic encode by twisted register-resident sub-NTTs
int launch_encode_fnt(int k, int n, int n_out, const int32_t* d_twist,
                      const uint16_t* data, long long dss, long long drs,
                      RowDst out, long long words, int n_stripes, Oor oor,
                      uint32_t* d_err, hipStream_t stream);

// out[t] = sum_i M[t][i] * in[ids[i]]  for t < R
//   mat: per-stripe blocks (mat_stride words apart; 0 = shared)
//   ids: per-stripe kin int32 fragment ids, ids_stride apart (nullptr =
//   identity 0..kin-1)
//   in_oor: restore buckets by slot (nullptr = none); slot_of_id = id -
//     slot_base (ids < slot_base have no bucket)
//   out_oor: record OOR outputs (nullptr = no recording; values stored as 0)
//   rowmap: output row (and OOR slot) of matrix row t (R entries, required;
//   identity for decode matrices)
//   route: per-stripe OOR routing tables (route_stride u32 apart), or null
//   slow: per-stripe slow-tile lists (required when in_oor is given)
//   ver: a fused check instead of a product (see MatVerify); requires out_oor
struct MatVerify;
int launch_matrix(const MatLayout& L, const int32_t* mat, long long mat_stride,
                  const int32_t* ids, long long ids_stride, RowSrc src,
                  RowDst dst, long long words,
                  int n_stripes, const Oor* in_oor, int slot_base,
                  const Oor* out_oor, const int32_t* rowmap, const uint32_t* route,
                  long long route_stride, SlowList slow, uint32_t* d_err,
                  hipStream_t stream, const MatVerify* ver = nullptr);

// A fused check (the _verify kernel forms): matrix row t of stripe s is
// recomputed as in a repair and compared with the stored row of fragment
// checks[s * R + t], addressed in the source regions like the inputs; no row
// is written (dst is not used).  value_mismatch[s * R + t] counts the columns
// whose low 16 bits differ and first[s * R + t] takes the smallest such
// column by an atomic min (both initialised by the caller); the recomputed
// 65536 positions go to out_oor (slot t), for launch_verify_marks.
struct MatVerify {
    const uint16_t* checks;
    uint32_t* value_mismatch;
    uint32_t* first;
};
// counters of S x R checks to 0 / 0 / 0xFFFFFFFF and the work buckets' counts
// to 0
int launch_verify_init(uint32_t* value_mismatch, uint32_t* mark_mismatch, uint32_t* first,
                       uint32_t* work_counts, long long n, hipStream_t stream);
// per (stripe, check row): the stored bucket of fragment checks[s * R + t]
// (slot id - slot_base of `stored`; none for id < slot_base or stored null)
// and the work bucket t as sets; the size of their symmetric difference is
// added to mark_mismatch and its columns go to first by atomic min.  A bucket
// over its capacity raises kErrOorTruncated; stored entries >= words are no
// columns and are ignored
int launch_verify_marks(const uint16_t* checks, int R, int n_stripes, const Oor* stored,
                        int slot_base, const Oor& work, long long words, uint32_t* mark_mismatch,
                        uint32_t* first, uint32_t* d_err, hipStream_t stream);

// per-stripe decode matrices from fragment ids (S x k).
//   mode 0: coefficient extraction (non-systematic: data = poly coefs)
//   mode 1: evaluation at r^t, t < k (systematic: data = P(r^t))
//   d_ctx: per stripe ctx_stride words: the MatLayout block, the k ids as
//   int32 (padded to 2 KP), the OOR route table (route_tiles(words) x
//   kRouteStride u32) built from in_oor, then the slow-tile list
//   (slow_words(words) u32, count cleared), then the lazy-section word
//   (cleared; lazy_word_off)
//   (slot = by_pos ? position : id - slot_base); in_oor may be null.
//   n: the code length (ids < n), r its root of unity
//   dot2: also write the dot2 kernel's sections (packed pairs, `plain`
//   rows); without them only the matrix cores can apply the context
int launch_decode_ctx(int k, int n, uint32_t r, int mode, const MatLayout& L,
                      const uint16_t* d_ids, int n_stripes, int32_t* d_ctx,
                      long long ctx_stride, const Oor* in_oor, int slot_base,
                      int by_pos, long long words, int dot2, uint32_t* d_err,
                      hipStream_t stream);
// per-stripe repair contexts (S x k received ids, S x L.R target ids): the
// L.R x k matrices M[j][i] = L_i(r^{targets[j]}) as complete MatLayout blocks
// (every section written), followed by the sections of a decode context
// (ids as dwords -- data fragments first when sys --, route table, cleared
// slow-tile list, lazy word); k <= 256, L.R <= 64.  code_len = k + m: a
// target must lie below it
int launch_repair_ctx(int k, int n, int code_len, uint32_t r, int sys, const MatLayout& L,
                      const uint16_t* d_ids, const uint16_t* d_targets, int n_stripes,
                      int32_t* d_ctx, long long ctx_stride, const Oor* in_oor, int slot_base,
                      long long words, uint32_t* d_err, hipStream_t stream);
// the dot2 sections of n_stripes contexts built with dot2 = 0 for `words`
// columns, from their operand tiles (before a decode that runs the dot2
// kernel over them); a stripe whose lazy word has kLazyDot2 set is skipped,
// and the bit is set after the fill
int fill_dot2_sections(const MatLayout& L, int32_t* d_ctx, long long ctx_stride, long long words,
                       int n_stripes, hipStream_t stream);

// Whether rows of u16 at base + s * ss + t * rs take the streaming kernels'
// 16-byte form (row_tile.h): the base and both strides multiples of 16 bytes.
// The update asks it of its four regions; the locate and the fingerprint of
// the regions a call can read:
inline bool rows_vec(const void* base, long long ss, long long rs)
{
    return reinterpret_cast<uintptr_t>(base) % 16 == 0 && ss % 8 == 0 && rs % 8 == 0;
}
// the locate reads data rows only below a split
inline bool locate_rows_vec(int split, const void* data, long long dss, long long drs,
                            const void* coded, long long css, long long crs)
{
    return rows_vec(coded, css, crs) && (!split || rows_vec(data, dss, drs));
}
// the fingerprint may hold neither region (null), and its lanes' pieces start
// at multiples of 8 absolute columns
inline bool fingerprint_rows_vec(long long first_col, int split, const void* data, long long dss,
                                 long long drs, const void* coded, long long css, long long crs)
{
    return first_col % 8 == 0 && (!coded || rows_vec(coded, css, crs)) &&
           (!(split && data) || rows_vec(data, dss, drs));
}

// per-stripe delta-update contexts (ctx.hip; S x U data row ids, S x R coded
// slots, d_slots null: slot j = j): update_ctx_words(U, R) words each, the
// R x UP balanced coefficients c(slot, id) of update_coef.h, the slots and the
// ids as dwords.  d_tab: the systematic plan's tables, A(y_j) for j < n_out
// then 1 / A'(x_i) for i < k (null for a non-systematic plan).  Ids not below
// k or repeated and slots not below n_out or repeated raise kErrBadIds and
// enter the context as 0
int launch_update_ctx(int k, int n, int n_out, uint32_t r, int sys, const uint32_t* d_tab,
                      const uint16_t* d_ids, const uint16_t* d_slots, int U, int UP, int R, int S,
                      int32_t* d_ctx, long long ctx_stride, uint32_t* err, hipStream_t st);
// the update itself (update.hip): out[slot] = coded[slot] + sum_u c (new_u -
// old_u) for the R slots of each context; in / outm: the coded rows' buckets
// and the updated rows', by slot (counts null: none); by_pos: rows and
// buckets by the slot's position in the list instead
int launch_update(const int32_t* d_ctx, long long ctx_stride, int U, int UP, int R, int by_pos,
                  const uint16_t* d_old, long long old_ss, long long old_rs,
                  const uint16_t* d_new, long long new_ss, long long new_rs,
                  const uint16_t* d_coded, long long css, long long crs, const Oor& in,
                  uint16_t* d_out, long long oss, long long ors, const Oor& outm, long long words,
                  int n_stripes, uint32_t* d_err, hipStream_t st);
// its kernel, by row count and by whether every base and stride is a
// multiple of 16 bytes
std::string update_kernel_name(int UP, bool vec);
inline std::string update_ctx_kernel_name()
{
    return "update_ctx_kernel";
}

// per-stripe locate contexts (locate.hip; S x (k + R) listed fragment ids):
// locate_ctx_words(k, R) words each (locate_math.h).  Ids not below code_len
// or repeated raise kErrBadIds; an id out of range enters the context as 0
int launch_locate_ctx(int k, int R, int code_len, uint32_t r, const uint16_t* d_ids, int S,
                      int32_t* d_ctx, uint32_t* err, hipStream_t st);
// the locate itself: fragments below `split` are rows of d_data, the others
// rows of d_coded by slot id - split with the buckets `in` (counts null: no
// marks); d_stripes: list position -> stripe of the rows and buckets (null:
// the identity).  Clears the four outputs first
int launch_locate(const int32_t* d_ctx, int k, int R, int split, const uint32_t* d_stripes,
                  const uint16_t* d_data, long long dss, long long drs, const uint16_t* d_coded,
                  long long css, long long crs, const Oor& in, uint32_t* d_located,
                  uint32_t* d_unlocated, uint32_t* d_fix_counts, uint32_t* d_fixes, int fix_cap,
                  long long words, int n_stripes, uint32_t* d_err, hipStream_t st);
// their kernels, by the syndrome count rounded up (locate_rp) and by whether
// every base and stride is a multiple of 16 bytes
std::string locate_ctx_kernel_name(int RP);
std::string locate_kernel_name(int RP, bool vec);
// the multi-fragment locate (locate_multi.hip) over the same contexts: up to t
// bad fragments per column, 1 <= t <= R / 2; launch_locate's arguments and
// d_weights [n_stripes][kLocMaxErrors].  Clears the five outputs first
int launch_locate_multi(const int32_t* d_ctx, int k, int R, int t, int split,
                        const uint32_t* d_stripes, const uint16_t* d_data, long long dss,
                        long long drs, const uint16_t* d_coded, long long css, long long crs,
                        const Oor& in, uint32_t* d_located, uint32_t* d_unlocated,
                        uint32_t* d_weights, uint32_t* d_fix_counts, uint32_t* d_fixes,
                        int fix_cap, long long words, int n_stripes, uint32_t* d_err,
                        hipStream_t st);
std::string locate_multi_kernel_name(int RP, bool vec);

// fragment fingerprints (fingerprint.hip, fingerprint_math.h): F digests of
// each of the N listed rows per stripe; keys: F host triples (they travel as
// kernel arguments), d_work: fp_work_words(S * N, fp_pad(F), words) u32.  An
// id not below code_len, or in a region that is not held (null), raises
// kErrBadIds and gives 0xFFFFFFFF.  The caller checks the ranges
int launch_fingerprint(const uint16_t* d_ids, int N, const uint32_t* keys, int F,
                       long long first_col, int split, int code_len, const uint16_t* d_data,
                       long long dss, long long drs, const uint16_t* d_coded, long long css,
                       long long crs, const Oor& in, uint32_t* d_work, uint32_t* d_fp,
                       long long words, int n_stripes, uint32_t* d_err, hipStream_t st);
// its kernels (rows and strides at multiples of 16 bytes when vec)
std::string fingerprint_kernel_names(int F, bool vec, long long words);

// per-stripe partial-repair contexts (partial.hip, partial_math.h; S x k helper
// ids, S x H positions into them, S x R targets): partial_ctx_words(H, R) words
// each, the H x RP balanced coefficients c(t, held[h]), the targets and the
// held rows' ids.  An id or target not below code_len or repeated, a target
// that is a helper, a position not below k or repeated raise kErrBadIds; the
// offending coefficients are 0
int launch_partial_ctx(int k, int code_len, uint32_t r, const uint16_t* d_ids,
                       const uint16_t* d_held, const uint16_t* d_targets, int H, int R, int S,
                       int32_t* d_ctx, uint32_t* err, hipStream_t st);
// the partial repair itself: out_t = acc_t + sum_h c(t, held[h]) row_h, rows
// and their buckets `in` by position h, the acc rows' and output rows' buckets
// accm / outm by target t (counts null: none); d_acc null: start from 0.  The
// held rows whose id is below `split` are data rows: their bucket is not read
int launch_partial(const int32_t* d_ctx, int H, int R, int split, const uint16_t* d_rows,
                   long long rss, long long rrs, const Oor& in, const uint16_t* d_acc,
                   long long ass, long long ars, const Oor& accm, uint16_t* d_out, long long oss,
                   long long ors, const Oor& outm, long long words, int n_stripes,
                   uint32_t* d_err, hipStream_t st);
// their kernels, by the target count rounded up (partial_rp) and by whether
// every base and stride is a multiple of 16 bytes
std::string partial_ctx_kernel_name();
std::string partial_kernel_name(int RP, bool vec);

// per-stripe syndrome-share contexts (syndrome.hip, syndrome_math.h; S x (k +
// R) listed ids, S x H positions into them): partial_ctx_words(H, R) words
// each in the layout launch_partial reads, the H x RP balanced coefficients
// x^j / w of the held rows, RP filler words and the held rows' ids.  An id not
// below code_len or repeated, a position not below k + R or repeated raise
// kErrBadIds; that row's coefficients are 0.  The share itself is
// launch_partial
int launch_syndrome_ctx(int k, int code_len, uint32_t r, const uint16_t* d_ids,
                        const uint16_t* d_held, int H, int R, int S, int32_t* d_ctx,
                        uint32_t* err, hipStream_t st);
// per-stripe resolve contexts: the k + R ids, points and weights,
// syndrome_locate_ctx_words(k + R) words each
int launch_syndrome_locate_ctx(int k, int R, int code_len, uint32_t r, const uint16_t* d_ids,
                               int S, int32_t* d_ctx, uint32_t* err, hipStream_t st);
// the decision over the R summed syndrome rows (buckets `in` by slot j), bound
// 0 <= t <= R / 2; the five outputs are cleared by the call
int launch_syndrome_locate(const int32_t* d_ctx, int k, int R, int t, const uint16_t* d_syn,
                           long long sss, long long srs, const Oor& in, uint32_t* d_located,
                           uint32_t* d_unlocated, uint32_t* d_weights, uint32_t* d_fix_counts,
                           uint32_t* d_fixes, int fix_cap, long long words, int n_stripes,
                           uint32_t* d_err, hipStream_t st);
std::string syndrome_ctx_kernel_name();
std::string syndrome_locate_ctx_kernel_name();
std::string syndrome_locate_kernel_name(int RP, bool vec);

// the device patch (patch.hip, patch_math.h): the fix lists of n_stripes list
// positions applied to the rows and the coded rows' buckets `marks` (counts
// null: no marks), all or nothing per stripe; d_work: patch_work_words(N,
// n_stripes) u32.  The caller checks the ranges
int launch_patch(int mode, int sys, int k, int code_len, const uint16_t* d_ids, int N,
                 const uint8_t* d_mine, const uint32_t* d_stripes, const uint32_t* d_unlocated,
                 const uint32_t* d_fix_counts, const uint32_t* d_fixes, int fix_cap,
                 uint16_t* d_data, long long dss, long long drs, uint16_t* d_coded, long long css,
                 long long crs, const Oor& marks, uint32_t* d_work, uint32_t* d_status,
                 uint32_t* d_applied, long long words, int n_stripes, uint32_t* d_err,
                 hipStream_t st);
std::string patch_kernel_name();

// whether launch_matrix runs these rows on the matrix cores (whole
// kRouteTile tiles): 8-byte aligned rows inside 31-bit buffer ranges.  The
// kin > 256 layouts have no other kernel, so their callers check this first.
bool matrix_cores_take(const RowSrc& src, const RowDst& dst, int R, long long words);
// names of the kernels launch_matrix runs for L over `words` columns: the
// same matrix_route launch_matrix dispatches on, printed (aligned rows in
// buffer range; diagnostics: qi_gpu_kernels); two: rows from two source
// regions (the systematic decode)
std::string matrix_kernel_names(const MatLayout& L, long long words, bool in_oor, bool two,
                                bool both = false, bool verify = false);
// the register-codelet encode kernel launch_encode_fnt runs (aligned rows)
std::string encode_fnt_kernel_name(int k);

// ---- host math (plan.cpp) ----
// Lagrange matrix for points x_i = r^{ids[i]}:
//   mode 0: M[t][i] = coef_t(L_i), t < k
//   mode 1: M[t][i] = L_i(eval[t]), t < R
std::vector<uint32_t> lagrange_matrix(int k, uint32_t r, const uint32_t* ids,
                                      int mode, const uint32_t* eval, int R);
// pack a canonical R x kin matrix into a MatLayout block
void pack_matrix(const MatLayout& L, const uint32_t* M, int32_t* block);

}  // namespace qi
