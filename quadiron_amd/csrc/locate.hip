// Fragment locate (qi_gpu_locate): which of the N = k + R listed fragments of
// a column is wrong, and what it should hold.  locate_ctx_kernel leaves, per
// stripe, the ids, the points x_i, the dual weights w_i and the N x RP
// syndrome coefficients x_i^j / w_i (locate_math.h); locate_kernel streams the
// N rows once, accumulates the R syndromes of every column and classifies the
// columns whose syndromes are not all 0.  N rows in, no row out.
//
// A block owns one listed stripe and one tile of kLocTile columns, a lane 8
// columns.  It walks the N rows kLocAhead at a time (the loads of a group are
// issued before the first of them is used) and keeps RP x 8 syndrome
// accumulators in registers.  Addressing is flat with 64-bit wave-uniform row
// offsets, as in update.hip: VEC, every base and stride a multiple of 16
// bytes, a lane moves its 8 adjacent columns as one 16-byte piece; otherwise
// lane t takes the columns t, t + 256, ... of the tile symbol by symbol.
// The marks of a row are restored in full through an LDS bitmap of the tile,
// filled from the row's bucket 256 entries at a time.
//
// Ranges (gf65537.h).  A restored symbol y is in [0, 65536] and a coefficient
// c balanced, in [-32768, 32768]: y c reaches 65536 * 32768 = 2^31, which no
// int32 holds.  So the symbol is balanced too, yb = y - q for y > 32768 (the
// mark 65536 becomes -1), yb in [-32768, 32768], and |yb c| <= 2^30 is one
// v_mul_i32_i24 (both operands inside 24 bits).  The accumulator is folded at
// every term, acc <- fold(yb c + acc): with acc in [-16385, 81920] the sum is
// inside +-(2^30 + 81920) < 2^31, its high half in [-16385, 16385], and the
// fold, lo - hi with lo in [0, 65535], is in [-16385, 81920] again.  After
// the last row one conditional + q and one conditional - q make it canonical,
// [0, 65536].  Columns past the row's end read 0: their syndromes are 0.
//
// The epilogue runs only in waves where a ballot finds a non-zero syndrome:
// per bad column one inversion (S_1 / S_0), a scan of the stripe's x_i, a
// reload of the named fragment's symbol (and a scan of its bucket, the symbol
// is 65536 when listed), then atomics on the counters and the fix append.
#include <hip/hip_runtime.h>

#include <string>

#include "gf65537.h"
#include "locate_math.h"
#include "qi_internal.h"

namespace qi {

constexpr int kLocBlock = 256;
constexpr int kLocCols = 8;  // columns per lane: one 16-byte row piece
constexpr int kLocTile = kLocBlock * kLocCols;
constexpr int kLocAhead = 4;  // rows in flight per lane
constexpr int kLocCtxThreads = 256;

typedef uint32_t loc_u32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------
// The context: one block per stripe.  ids that are not below code_len or are
// repeated raise kErrBadIds; an id out of range enters the context as 0, so
// that the locate stays inside the caller's rows (a repeated id has w = 0 and
// all-zero coefficients).  One inversion per listed fragment.
// ---------------------------------------------------------------------------
template <int RP>
__global__ __launch_bounds__(kLocCtxThreads) void locate_ctx_kernel(
    int N, int R, int code_len, uint32_t r, const uint16_t* __restrict__ ids,
    int32_t* __restrict__ ctx, long long ctx_stride, uint32_t* err)
{
    __shared__ uint32_t sx[kLocMaxK + kLocMaxChecks];
    const int s = static_cast<int>(blockIdx.x);
    const int tid = static_cast<int>(threadIdx.x);
    int32_t* c = ctx + static_cast<long long>(s) * ctx_stride;
    const uint16_t* id_s = ids + static_cast<long long>(s) * N;
    bool bad = false;
    for (int i = tid; i < N; i += kLocCtxThreads) {
        uint32_t id = id_s[i];
        if (id >= static_cast<uint32_t>(code_len)) {
            bad = true;
            id = 0;
        }
        const uint32_t x = powmod_c(r, id);
        sx[i] = x;
        c[i] = static_cast<int32_t>(id);
        c[N + i] = static_cast<int32_t>(x);
    }
    __syncthreads();
    for (int i = tid; i < N; i += kLocCtxThreads) {
        const uint32_t w = locate_weight(sx, N, i);
        bad |= w == 0;
        c[2 * N + i] = static_cast<int32_t>(w);
        int32_t co[RP];
        locate_coefs<RP>(sx[i], invmod_c(w), R, co);
#pragma unroll
        for (int j = 0; j < RP; j++)
            c[3 * N + i * RP + j] = co[j];
    }
    if (bad)
        atomicOr(err, kErrBadIds);
}

std::string locate_ctx_kernel_name(int RP)
{
    return "locate_ctx_kernel<" + std::to_string(RP) + ">";
}

int launch_locate_ctx(int k, int R, int code_len, uint32_t r, const uint16_t* d_ids, int S,
                      int32_t* d_ctx, uint32_t* err, hipStream_t st)
{
    if (k < 1 || k > kLocMaxK || R < 2 || R > kLocMaxChecks || S <= 0)
        return -3;
    const int N = k + R;
    const long long cs = locate_ctx_words(k, R);
    const dim3 g(static_cast<unsigned>(S)), b(kLocCtxThreads);
    switch (locate_rp(R)) {
    case 2:
        hipLaunchKernelGGL(locate_ctx_kernel<2>, g, b, 0, st, N, R, code_len, r, d_ids, d_ctx, cs,
                           err);
        break;
    case 4:
        hipLaunchKernelGGL(locate_ctx_kernel<4>, g, b, 0, st, N, R, code_len, r, d_ids, d_ctx, cs,
                           err);
        break;
    default:
        hipLaunchKernelGGL(locate_ctx_kernel<8>, g, b, 0, st, N, R, code_len, r, d_ids, d_ctx, cs,
                           err);
        break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------
// The apply kernel
// ---------------------------------------------------------------------------
struct LocArgs {
    long long ctx_stride;
    const uint32_t* stripes;  // list position -> stripe (null: the identity)
    const uint16_t* data;     // fragments below `split` (systematic data rows)
    long long dss, drs;
    const uint16_t* coded;
    long long css, crs;
    Oor in;  // the coded rows' buckets by slot (counts null: no marks)
    uint32_t* located;
    uint32_t* unlocated;
    uint32_t* fix_counts;
    uint32_t* fixes;
    int fix_cap;
    long long words;
    int N, R, split, tiles;
    uint32_t* err;
};

// column of a lane's element i, relative to the tile
template <bool VEC>
__device__ __forceinline__ int loc_rel(int tid, int i)
{
    return VEC ? tid * kLocCols + i : i * kLocBlock + tid;
}

// a lane's 8 columns of `row` as 4 packed pairs; columns past the row's end
// read 0.  full: the lane's 16-byte piece lies inside the row
template <bool VEC>
__device__ __forceinline__ void loc_load(const uint16_t* row, long long c0, int tid, bool full,
                                         long long words, uint32_t (&w)[4])
{
    if (VEC && full) {
        const loc_u32x4 v = *reinterpret_cast<const loc_u32x4*>(row + c0 + tid * kLocCols);
        w[0] = v[0];
        w[1] = v[1];
        w[2] = v[2];
        w[3] = v[3];
        return;
    }
#pragma unroll
    for (int i = 0; i < kLocCols; i += 2) {
        const long long ca = c0 + loc_rel<VEC>(tid, i), cb = c0 + loc_rel<VEC>(tid, i + 1);
        const uint32_t lo = ca < words ? row[ca] : 0u;
        const uint32_t hi = cb < words ? row[cb] : 0u;
        w[i / 2] = lo | hi << 16;
    }
}

// The marked columns of this tile in bucket bk, as a mask over the lane's 8
// elements: the block scans the bucket's entries 256 at a time into an LDS
// bitmap of the tile (a dense bucket costs entries / 256 steps).  Called by
// the whole block (cnt is the same in every lane).
template <bool VEC>
__device__ __forceinline__ uint32_t loc_marks(uint32_t* bitmap, const Oor& in, long long bk,
                                              uint32_t cnt, long long c0, long long words,
                                              int tid, uint32_t* err)
{
    __syncthreads();  // the previous bitmap has been read
    if (tid < kLocTile / 32)
        bitmap[tid] = 0;
    __syncthreads();
    const uint32_t cap = static_cast<uint32_t>(in.cap);
    if (cnt > cap && tid == 0)
        atomicOr(err, kErrOorTruncated);
    const uint32_t n = cnt < cap ? cnt : cap;
    const uint32_t* e = in.entries + bk * in.cap;
    for (uint32_t x = static_cast<uint32_t>(tid); x < n; x += kLocBlock) {
        const long long col = e[x];
        const long long rel = col - c0;
        if (rel >= 0 && rel < kLocTile && col < words)
            atomicOr(&bitmap[rel >> 5], 1u << (rel & 31));
    }
    __syncthreads();
    uint32_t mk = 0;
#pragma unroll
    for (int i = 0; i < kLocCols; i++) {
        const int rel = loc_rel<VEC>(tid, i);
        mk |= (bitmap[rel >> 5] >> (rel & 31) & 1u) << i;
    }
    return mk;
}

// fragment id -> its row of stripe sr and its bucket (-1: a data row, none)
__device__ __forceinline__ const uint16_t* loc_row(const LocArgs& a, long long sr, int id,
                                                   long long* bk)
{
    if (id < a.split) {
        *bk = -1;
        return a.data + sr * a.dss + id * a.drs;
    }
    const int slot = id - a.split;
    *bk = sr * a.in.slots + slot;
    return a.coded + sr * a.css + slot * a.crs;
}

template <int RP, bool VEC>
__global__ __launch_bounds__(kLocBlock) void locate_kernel(LocArgs a,
                                                           const int32_t* __restrict__ ctx)
{
    __shared__ uint32_t bitmap[kLocTile / 32];
    const int tid = static_cast<int>(threadIdx.x);
    const int tile = static_cast<int>(blockIdx.x) % a.tiles;  // tiles fastest
    const int s = static_cast<int>(blockIdx.x) / a.tiles;
    const long long sr = a.stripes ? a.stripes[s] : s;
    const long long c0 = static_cast<long long>(tile) * kLocTile;
    const bool full = c0 + tid * kLocCols + kLocCols <= a.words;
    const int N = a.N;
    const int32_t* ids = ctx + static_cast<long long>(s) * a.ctx_stride;
    const int32_t* coef = ids + 3 * N;

    int32_t acc[RP][kLocCols];
#pragma unroll
    for (int j = 0; j < RP; j++)
#pragma unroll
        for (int i = 0; i < kLocCols; i++)
            acc[j][i] = 0;

    for (int i0 = 0; i0 < N; i0 += kLocAhead) {
        uint32_t w[kLocAhead][4];
        long long bk[kLocAhead];
        uint32_t cnt[kLocAhead];
#pragma unroll
        for (int q = 0; q < kLocAhead; q++) {
            if (i0 + q < N) {
                const uint16_t* row = loc_row(a, sr, ids[i0 + q], &bk[q]);
                loc_load<VEC>(row, c0, tid, full, a.words, w[q]);
                cnt[q] = bk[q] >= 0 && a.in.counts ? a.in.counts[bk[q]] : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < kLocAhead; q++) {
            if (i0 + q >= N)
                break;
            uint32_t mk = 0;
            if (cnt[q])
                mk = loc_marks<VEC>(bitmap, a.in, bk[q], cnt[q], c0, a.words, tid, a.err);
            const int32_t* c = coef + (i0 + q) * RP;
#pragma unroll
            for (int i = 0; i < kLocCols; i++) {
                const int32_t y = static_cast<int32_t>(w[q][i / 2] >> (i % 2 * 16) & 0xffffu);
                int32_t yb = y > 32768 ? y - kQ : y;
                if (mk)  // a marked symbol is 65536 = -1
                    yb = mk >> i & 1u ? -1 : yb;
#pragma unroll
                for (int j = 0; j < RP; j++)
                    acc[j][i] = fold(__mul24(yb, c[j]) + acc[j][i]);
            }
        }
    }

    // canonical syndromes; nz: the lane's columns with one that is not 0
    uint32_t nz = 0;
#pragma unroll
    for (int i = 0; i < kLocCols; i++) {
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < RP; j++) {
            int32_t v = acc[j][i];
            v = v < 0 ? v + kQ : v;
            v = v >= kQ ? v - kQ : v;
            acc[j][i] = v;
            any |= static_cast<uint32_t>(v);
        }
        nz |= static_cast<uint32_t>(any != 0) << i;
    }
    if (!__ballot(nz != 0))
        return;

    const uint32_t* xs = reinterpret_cast<const uint32_t*>(ids + N);
    const uint32_t* ws = reinterpret_cast<const uint32_t*>(ids + 2 * N);
    while (nz) {
        const int i = __ffs(nz) - 1;
        nz &= nz - 1;
        uint32_t S[RP];
#pragma unroll
        for (int j = 0; j < RP; j++) {
            uint32_t v = 0;
#pragma unroll
            for (int ii = 0; ii < kLocCols; ii++)
                v = i == ii ? static_cast<uint32_t>(acc[j][ii]) : v;
            S[j] = v;
        }
        const long long col = c0 + (VEC ? tid * kLocCols + i : i * kLocBlock + tid);
        int pos = 0;
        bool found = locate_classify<RP>(S, a.R, xs, N, &pos) == kLocFound;
        uint32_t v = 0;
        if (found) {
            // the named fragment's restored symbol at this column
            long long bkp;
            const uint16_t* row = loc_row(a, sr, ids[pos], &bkp);
            uint32_t y = row[col];
            if (bkp >= 0 && a.in.counts) {
                const uint32_t cap = static_cast<uint32_t>(a.in.cap);
                const uint32_t cn = a.in.counts[bkp];
                const uint32_t n = cn < cap ? cn : cap;
                const uint32_t* e = a.in.entries + bkp * a.in.cap;
                for (uint32_t t = 0; t < n; t++)
                    if (e[t] == static_cast<uint32_t>(col))
                        y = 65536u;
            }
            found = locate_fix(y, S[0], ws[pos], bkp < 0, &v);
        }
        if (!found) {
            atomicAdd(&a.unlocated[s], 1u);
            continue;
        }
        atomicAdd(&a.located[static_cast<long long>(s) * N + pos], 1u);
        const uint32_t e = atomicAdd(&a.fix_counts[s], 1u);
        if (e < static_cast<uint32_t>(a.fix_cap)) {
            uint32_t* f = a.fixes + (static_cast<long long>(s) * a.fix_cap + e) * 3;
            f[0] = static_cast<uint32_t>(col);
            f[1] = static_cast<uint32_t>(pos);
            f[2] = v;
        }
    }
}

std::string locate_kernel_name(int RP, bool vec)
{
    return "locate_kernel<" + std::to_string(RP) + ", " + (vec ? "true" : "false") + ">";
}

template <int RP>
static void loc_launch(bool vec, unsigned blocks, const LocArgs& a, const int32_t* ctx,
                       hipStream_t st)
{
    if (vec)
        hipLaunchKernelGGL((locate_kernel<RP, true>), dim3(blocks), dim3(kLocBlock), 0, st, a, ctx);
    else
        hipLaunchKernelGGL((locate_kernel<RP, false>), dim3(blocks), dim3(kLocBlock), 0, st, a,
                           ctx);
}

// The syndromes of n_stripes listed stripes from contexts of locate_ctx_words(k,
// R) words built by launch_locate_ctx.  Fragments below `split` are rows of
// d_data (none: split 0), the others rows of d_coded by slot id - split, with
// the buckets `in` (counts null: no marks).  The four outputs are cleared here.
int launch_locate(const int32_t* d_ctx, int k, int R, int split, const uint32_t* d_stripes,
                  const uint16_t* d_data, long long dss, long long drs, const uint16_t* d_coded,
                  long long css, long long crs, const Oor& in, uint32_t* d_located,
                  uint32_t* d_unlocated, uint32_t* d_fix_counts, uint32_t* d_fixes, int fix_cap,
                  long long words, int n_stripes, uint32_t* d_err, hipStream_t st)
{
    if (k < 1 || k > kLocMaxK || R < 2 || R > kLocMaxChecks || n_stripes <= 0 || words < 0 ||
        fix_cap < 0)
        return -3;
    const int N = k + R;
    const size_t S = static_cast<size_t>(n_stripes);
    if (hipMemsetAsync(d_located, 0, S * N * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(d_unlocated, 0, S * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(d_fix_counts, 0, S * sizeof(uint32_t), st) != hipSuccess)
        return -2;
    if (words == 0)
        return 0;
    const long long tiles = (words + kLocTile - 1) / kLocTile;
    const long long blocks = tiles * n_stripes;
    if (tiles > 0x7fffffffLL || blocks > 0x7fffffffLL)
        return -3;
    LocArgs a{locate_ctx_words(k, R), d_stripes, d_data, dss, drs, d_coded, css, crs, in,
              d_located, d_unlocated, d_fix_counts, d_fixes, fix_cap, words, N, R, split,
              static_cast<int>(tiles), d_err};
    bool vec = reinterpret_cast<uintptr_t>(d_coded) % 16 == 0 && css % kLocCols == 0 &&
               crs % kLocCols == 0;
    if (split)
        vec = vec && reinterpret_cast<uintptr_t>(d_data) % 16 == 0 && dss % kLocCols == 0 &&
              drs % kLocCols == 0;
    const unsigned nb = static_cast<unsigned>(blocks);
    switch (locate_rp(R)) {
    case 2: loc_launch<2>(vec, nb, a, d_ctx, st); break;
    case 4: loc_launch<4>(vec, nb, a, d_ctx, st); break;
    default: loc_launch<8>(vec, nb, a, d_ctx, st); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
