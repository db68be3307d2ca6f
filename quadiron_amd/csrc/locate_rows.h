// locate_rows.h -- what locate.hip (qi_gpu_locate) and locate_multi.hip
// (qi_gpu_locate_multi) share beyond the tile primitives of row_tile.h: the
// kernels' argument block LocArgs, the host side of a launch (loc_prepare),
// and the row pass loc_syndromes, which walks the N listed rows kLocAhead at a
// time and leaves the RP canonical syndromes of a lane's 8 columns in
// registers.  The layout, the mark bitmap and the range argument are
// described at the top of locate.hip.
//
// locate_multi_kernel calls loc_syndromes.  locate_kernel keeps its own text
// of the same loop: built from the shared pass it takes 4 .. 7 more VGPRs
// (gfx950: <2, true> 56 -> 60, <4, true> 71 -> 75 and 7 -> 6 waves per SIMD,
// <8, true> 103 -> 110).  That cost belongs to the pass as a whole; the
// primitives it is made of (row_tile.h) are shared by both at no cost.
#pragma once

#include <hip/hip_runtime.h>

#include "gf65537.h"
#include "locate_math.h"
#include "qi_internal.h"
#include "row_tile.h"

namespace qi {

constexpr int kLocAhead = 4;  // rows in flight per lane

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
    __host__ __device__ FragRows rows() const { return {data, dss, drs, coded, css, crs, split}; }
};

// The host side both launches share, launch_locate's arguments
// (qi_internal.h): checks them, clears located, unlocated and fix_counts, and
// fills the kernel's arguments, its block count and its form.  Returns 1 when
// there is a kernel to launch, 0 when there is none (no columns), else the
// launch's error
inline int loc_prepare(int k, int R, int split, const uint32_t* d_stripes, const uint16_t* d_data,
                       long long dss, long long drs, const uint16_t* d_coded, long long css,
                       long long crs, const Oor& in, uint32_t* d_located, uint32_t* d_unlocated,
                       uint32_t* d_fix_counts, uint32_t* d_fixes, int fix_cap, long long words,
                       int n_stripes, uint32_t* d_err, hipStream_t st, LocArgs* a,
                       unsigned* blocks, bool* vec)
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
    const long long tiles = (words + kTileElems - 1) / kTileElems;
    const long long nb = tiles * n_stripes;
    if (tiles > 0x7fffffffLL || nb > 0x7fffffffLL)
        return -3;
    *a = LocArgs{locate_ctx_words(k, R), d_stripes, d_data, dss, drs, d_coded, css, crs, in,
                 d_located, d_unlocated, d_fix_counts, d_fixes, fix_cap, words, N, R, split,
                 static_cast<int>(tiles), d_err};
    *blocks = static_cast<unsigned>(nb);
    *vec = locate_rows_vec(split, d_data, dss, drs, d_coded, css, crs);
    return 1;
}

// The row pass: acc[j][i] becomes the canonical syndrome S_j of the lane's
// column i; returns nz, the lane's columns with a syndrome that is not 0.
// ids: the stripe's context (the ids, then x, w and the coefficients)
template <int RP, bool VEC>
__device__ __forceinline__ uint32_t loc_syndromes(const LocArgs& a, const int32_t* ids,
                                                  long long sr, long long c0, int tid,
                                                  uint32_t* bitmap,
                                                  int32_t (&acc)[RP][kTileCols])
{
    const bool full = c0 + tid * kTileCols + kTileCols <= a.words;
    const int N = a.N;
    const int32_t* coef = ids + 3 * N;

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
    return nz;
}

}  // namespace qi
