// row_tile.h -- the tile of the streaming row kernels (update.hip, locate.hip,
// locate_multi.hip, fingerprint.hip): a block of kTileBlock lanes owns one
// stripe and one tile of kTileElems columns, a lane kTileCols of them.
// Addressing is flat, with 64-bit wave-uniform row offsets: rows may lie
// anywhere, regions past the 31-bit buffer range and past 4 GiB included.
// VEC (every base and stride a multiple of 16 bytes, rows_vec in
// qi_internal.h): a lane moves its 8 adjacent columns as one 16-byte piece
// (the lane across the end of the row, symbol by symbol).  Otherwise lane t
// takes the columns t, t + 256, ... of the tile symbol by symbol, so that a
// wave's accesses stay adjacent at any alignment.  The marks of a row are
// restored in full through an LDS bitmap of the tile, filled from the row's
// bucket 256 entries at a time.
//
// Only these primitives are shared: every kernel keeps its own row loop (see
// locate_rows.h for what sharing a whole pass cost).  Taking them from here
// leaves the gfx950 instruction stream of all four files as it was with a
// private copy in each, with two exceptions that keep their own text for
// that reason: fingerprint_kernel's row lookup (frag_row) and locate_kernel's
// symbol reload (tile_symbol).
#pragma once

#include <hip/hip_runtime.h>

#include "qi_internal.h"

namespace qi {

constexpr int kTileBlock = 256;
constexpr int kTileCols = 8;  // columns per lane: one 16-byte row piece
constexpr int kTileElems = kTileBlock * kTileCols;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// column of a lane's element i, relative to the tile
template <bool VEC>
__device__ __forceinline__ int tile_rel(int tid, int i)
{
    return VEC ? tid * kTileCols + i : i * kTileBlock + tid;
}

// a lane's 8 columns of `row` as 4 packed pairs; columns past the row's end
// read 0.  full: the lane's 16-byte piece lies inside the row
template <bool VEC>
__device__ __forceinline__ void tile_load(const uint16_t* row, long long c0, int tid, bool full,
                                          long long words, uint32_t (&w)[4])
{
    if (VEC && full) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(row + c0 + tid * kTileCols);
        w[0] = v[0];
        w[1] = v[1];
        w[2] = v[2];
        w[3] = v[3];
        return;
    }
#pragma unroll
    for (int i = 0; i < kTileCols; i += 2) {
        const long long ca = c0 + tile_rel<VEC>(tid, i), cb = c0 + tile_rel<VEC>(tid, i + 1);
        const uint32_t lo = ca < words ? row[ca] : 0u;
        const uint32_t hi = cb < words ? row[cb] : 0u;
        w[i / 2] = lo | hi << 16;
    }
}

// the low 16 bits of y[i] to the lane's 8 columns of `row`; columns past the
// row's end are not written.  NT: the 16-byte piece goes out nontemporal
template <bool VEC, bool NT>
__device__ __forceinline__ void tile_store(uint16_t* row, long long c0, int tid, bool full,
                                           long long words, const uint32_t (&y)[kTileCols])
{
    if (VEC && full) {
        u32x4 v;
#pragma unroll
        for (int i = 0; i < 4; i++)
            v[i] = y[2 * i] | y[2 * i + 1] << 16;
        u32x4* p = reinterpret_cast<u32x4*>(row + c0 + tid * kTileCols);
        if (NT)
            __builtin_nontemporal_store(v, p);
        else
            *p = v;
        return;
    }
#pragma unroll
    for (int i = 0; i < kTileCols; i++) {
        const long long c = c0 + tile_rel<VEC>(tid, i);
        if (c < words)
            row[c] = static_cast<uint16_t>(y[i]);
    }
}

// The marked columns of this tile in bucket bk, as a mask over the lane's 8
// elements: the block scans the bucket's entries 256 at a time into an LDS
// bitmap of the tile (kTileElems / 32 words; a dense bucket costs entries /
// 256 steps, not one per entry).  Called by the whole block (cnt is the same
// in every lane).
template <bool VEC>
__device__ __forceinline__ uint32_t tile_marks(uint32_t* bitmap, const Oor& in, long long bk,
                                               uint32_t cnt, long long c0, long long words,
                                               int tid, uint32_t* err)
{
    __syncthreads();  // the previous bitmap has been read
    if (tid < kTileElems / 32)
        bitmap[tid] = 0;
    __syncthreads();
    const uint32_t cap = static_cast<uint32_t>(in.cap);
    if (cnt > cap && tid == 0)
        atomicOr(err, kErrOorTruncated);
    const uint32_t n = cnt < cap ? cnt : cap;
    const uint32_t* e = in.entries + bk * in.cap;
    for (uint32_t x = static_cast<uint32_t>(tid); x < n; x += kTileBlock) {
        const long long col = e[x];
        const long long rel = col - c0;
        if (rel >= 0 && rel < kTileElems && col < words)
            atomicOr(&bitmap[rel >> 5], 1u << (rel & 31));
    }
    __syncthreads();
    uint32_t mk = 0;
#pragma unroll
    for (int i = 0; i < kTileCols; i++) {
        const int rel = tile_rel<VEC>(tid, i);
        mk |= (bitmap[rel >> 5] >> (rel & 31) & 1u) << i;
    }
    return mk;
}

// Where the fragments live: those below `split` are rows of `data`
// (systematic data rows, no buckets), the others rows of `coded` by slot id -
// split.  Strides in u16 elements: stripe, then row
struct FragRows {
    const uint16_t* data;
    long long dss, drs;
    const uint16_t* coded;
    long long css, crs;
    int split;
};

// fragment id -> its row of stripe sr and its bucket among in_slots per
// stripe (-1: a data row, none)
__device__ __forceinline__ const uint16_t* frag_row(const FragRows& rows, int in_slots,
                                                    long long sr, int id, long long* bk)
{
    if (id < rows.split) {
        *bk = -1;
        return rows.data + sr * rows.dss + id * rows.drs;
    }
    const int slot = id - rows.split;
    *bk = sr * in_slots + slot;
    return rows.coded + sr * rows.css + slot * rows.crs;
}

// the restored symbol of fragment id at column col, by one lane: the stored
// word, or 65536 when the column is in the row's bucket (a scan of the
// bucket).  *data_row: whether it is a systematic data row (no bucket)
__device__ __forceinline__ uint32_t tile_symbol(const FragRows& rows, const Oor& in, long long sr,
                                                int id, long long col, bool* data_row)
{
    long long bk;
    const uint16_t* row = frag_row(rows, in.slots, sr, id, &bk);
    uint32_t y = row[col];
    if (bk >= 0 && in.counts) {
        const uint32_t cap = static_cast<uint32_t>(in.cap);
        const uint32_t cn = in.counts[bk];
        const uint32_t n = cn < cap ? cn : cap;
        const uint32_t* e = in.entries + bk * in.cap;
        for (uint32_t t = 0; t < n; t++)
            if (e[t] == static_cast<uint32_t>(col))
                y = 65536u;
    }
    *data_row = bk < 0;
    return y;
}

// a 65536 written (as 0) at column col of slot `slot` of stripe s, by the
// protocol of qi_gpu_encode's buckets (kernels.hip record_oor): the count
// goes on past cap, entries past it are dropped
__device__ __forceinline__ void tile_record_oor(const Oor& o, int s, int slot, long long col)
{
    const long long bk = static_cast<long long>(s) * o.slots + slot;
    const uint32_t e = atomicAdd(&o.counts[bk], 1u);
    if (e < static_cast<uint32_t>(o.cap))
        o.entries[bk * o.cap + e] = static_cast<uint32_t>(col);
}

}  // namespace qi
