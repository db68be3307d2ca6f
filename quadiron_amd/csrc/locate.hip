// Fragment locate (qi_gpu_locate): which of the N = k + R listed fragments of
// a column is wrong, and what it should hold.  locate_ctx_kernel leaves, per
// stripe, the ids, the points x_i, the dual weights w_i and the N x RP
// syndrome coefficients x_i^j / w_i (locate_math.h); locate_kernel streams the
// N rows once, accumulates the R syndromes of every column and classifies the
// columns whose syndromes are not all 0.  N rows in, no row out.
//
// A block owns one listed stripe and one tile of kTileElems columns, a lane 8
// columns (row_tile.h: the addressing, its two forms VEC and symbol by
// symbol, and the LDS bitmap that restores a row's marks in full).  It walks
// the N rows kLocAhead at a time (the loads of a group are issued before the
// first of them is used) and keeps RP x 8 syndrome accumulators in registers.
// The loop is this file's own text; locate_rows.h says why.
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
#include "locate_rows.h"
#include "qi_internal.h"

namespace qi {

constexpr int kLocCtxThreads = 256;

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
template <int RP, bool VEC>
__global__ __launch_bounds__(kTileBlock) void locate_kernel(LocArgs a,
                                                           const int32_t* __restrict__ ctx)
{
    __shared__ uint32_t bitmap[kTileElems / 32];
    const int tid = static_cast<int>(threadIdx.x);
    const int tile = static_cast<int>(blockIdx.x) % a.tiles;  // tiles fastest
    const int s = static_cast<int>(blockIdx.x) / a.tiles;
    const long long sr = a.stripes ? a.stripes[s] : s;
    const long long c0 = static_cast<long long>(tile) * kTileElems;
    const bool full = c0 + tid * kTileCols + kTileCols <= a.words;
    const int N = a.N;
    const int32_t* ids = ctx + static_cast<long long>(s) * a.ctx_stride;
    const int32_t* coef = ids + 3 * N;

    int32_t acc[RP][kTileCols];
#pragma unroll
    for (int j = 0; j < RP; j++)
#pragma unroll
        for (int i = 0; i < kTileCols; i++)
            acc[j][i] = 0;

    for (int i0 = 0; i0 < N; i0 += kLocAhead) {
        uint32_t w[kLocAhead][4];
        long long bk[kLocAhead];
        uint32_t cnt[kLocAhead];
#pragma unroll
        for (int q = 0; q < kLocAhead; q++) {
            if (i0 + q < N) {
                const uint16_t* row = frag_row(a.rows(), a.in.slots, sr, ids[i0 + q], &bk[q]);
                tile_load<VEC>(row, c0, tid, full, a.words, w[q]);
                cnt[q] = bk[q] >= 0 && a.in.counts ? a.in.counts[bk[q]] : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < kLocAhead; q++) {
            if (i0 + q >= N)
                break;
            uint32_t mk = 0;
            if (cnt[q])
                mk = tile_marks<VEC>(bitmap, a.in, bk[q], cnt[q], c0, a.words, tid, a.err);
            const int32_t* c = coef + (i0 + q) * RP;
#pragma unroll
            for (int i = 0; i < kTileCols; i++) {
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
    for (int i = 0; i < kTileCols; i++) {
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
            for (int ii = 0; ii < kTileCols; ii++)
                v = i == ii ? static_cast<uint32_t>(acc[j][ii]) : v;
            S[j] = v;
        }
        const long long col = c0 + tile_rel<VEC>(tid, i);
        int pos = 0;
        bool found = locate_classify<RP>(S, a.R, xs, N, &pos) == kLocFound;
        uint32_t v = 0;
        if (found) {
            // the named fragment's restored symbol at this column: row_tile.h's
            // tile_symbol in this file's own text (calling it moves registers
            // and adds 6 instructions over the six forms)
            long long bkp;
            const uint16_t* row = frag_row(a.rows(), a.in.slots, sr, ids[pos], &bkp);
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
        hipLaunchKernelGGL((locate_kernel<RP, true>), dim3(blocks), dim3(kTileBlock), 0, st, a,
                           ctx);
    else
        hipLaunchKernelGGL((locate_kernel<RP, false>), dim3(blocks), dim3(kTileBlock), 0, st, a,
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
    LocArgs a;
    unsigned nb;
    bool vec;
    const int rc = loc_prepare(k, R, split, d_stripes, d_data, dss, drs, d_coded, css, crs, in,
                               d_located, d_unlocated, d_fix_counts, d_fixes, fix_cap, words,
                               n_stripes, d_err, st, &a, &nb, &vec);
    if (rc <= 0)
        return rc;
    switch (locate_rp(R)) {
    case 2: loc_launch<2>(vec, nb, a, d_ctx, st); break;
    case 4: loc_launch<4>(vec, nb, a, d_ctx, st); break;
    default: loc_launch<8>(vec, nb, a, d_ctx, st); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
