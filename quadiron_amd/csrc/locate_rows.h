// locate_rows.h -- the row pass of the fragment locate as locate_multi.hip
// (qi_gpu_locate_multi) uses it: a block owns one listed stripe and one tile
// of kLocTile columns, walks the N listed rows kLocAhead at a time and leaves
// the RP canonical syndromes of a lane's 8 columns in registers.  The layout,
// the addressing, the mark bitmap and the range argument are locate.hip's and
// are described at its top.  locate.hip keeps its own text of these steps:
// built from this header its kernels took 4 .. 7 more VGPRs (RP 4, VEC: 7 -> 6
// waves per SIMD), so the two copies live in namespaces of their own.
#pragma once

#include <hip/hip_runtime.h>

#include "gf65537.h"
#include "locate_math.h"
#include "qi_internal.h"

namespace qi {
namespace locrows {

constexpr int kLocBlock = 256;
constexpr int kLocCols = 8;  // columns per lane: one 16-byte row piece
constexpr int kLocTile = kLocBlock * kLocCols;
constexpr int kLocAhead = 4;  // rows in flight per lane

typedef uint32_t loc_u32x4 __attribute__((ext_vector_type(4)));

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

// The row pass: acc[j][i] becomes the canonical syndrome S_j of the lane's
// column i; returns nz, the lane's columns with a syndrome that is not 0.
// ids: the stripe's context (the ids, then x, w and the coefficients)
template <int RP, bool VEC>
__device__ __forceinline__ uint32_t loc_syndromes(const LocArgs& a, const int32_t* ids,
                                                  long long sr, long long c0, int tid,
                                                  uint32_t* bitmap,
                                                  int32_t (&acc)[RP][kLocCols])
{
    const bool full = c0 + tid * kLocCols + kLocCols <= a.words;
    const int N = a.N;
    const int32_t* coef = ids + 3 * N;

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
    return nz;
}

// the restored symbol of fragment position `pos` at column col: the stored
// word, or 65536 when the column is in the row's bucket.  *data_row: whether
// it is a systematic data row (no bucket)
__device__ __forceinline__ uint32_t loc_symbol(const LocArgs& a, const int32_t* ids, long long sr,
                                               int pos, long long col, bool* data_row)
{
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
    *data_row = bkp < 0;
    return y;
}

}  // namespace locrows
}  // namespace qi
