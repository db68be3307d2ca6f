// Syndrome shares (qi_gpu_syndrome, qi_gpu_syndrome_locate): the scrub of a
// stripe whose fragments lie on different nodes, at any k.  The R syndromes of
// the N = k + R listed fragments (locate_math.h),
//   S_j = sum_i y_i x_i^j / w_i,   j < R,
// are linear in the rows, so the holder of H of the N rows forms its share
//   out_j = acc_j + sum_{h<H} c(j, held[h]) row_h   (mod 65537)
// and the shares of any partition of the N positions add up, in any order, to
// the syndromes.  A coordinator that sees only the R summed rows decides every
// column: clean, located in 1 .. t fragments with their errors, or unlocated.
//
// Helper side.  syndrome_ctx_kernel leaves per stripe the H x RP balanced
// coefficients c(j, held[h]) in exactly the layout of a partial repair's
// context (partial_ctx_words(H, R)); the row pass is then partial.hip's
// partial_kernel through launch_partial, unchanged: H (+ R) rows in, R rows
// out, the bucket protocol for 65536.  The context costs O(H N) per stripe:
// one N - 1 term product and one inversion per held row, no host table.
//
// Coordinator side.  syndrome_locate_ctx_kernel leaves the N ids, points x_i
// and weights w_i per stripe: O(N^2) per stripe, spread over ceil(N / 256)
// blocks of one thread per listed position.  syndrome_locate_kernel sits on
// row_tile.h: a block owns one stripe and one tile of kTileElems columns, a
// lane 8 columns.  It reads the R syndrome rows (row j is slot j, the marks
// restored through tile_marks: a syndrome may be 65536), and the waves in
// which a ballot finds a syndrome that is not 0 run the epilogue, the
// bounded-distance decoder of locate_multi_math.h.  A wave takes its lanes'
// columns element by element, every lane with a non-clean column at that
// element decoding it: Berlekamp-Massey in registers, then the root test of
// sigma at the N points.  The walk over the points is the wave's, not the
// lane's: x_p is read from the context at a wave-uniform index, a broadcast
// load (one word for the whole wave, no LDS staging and so no barrier behind
// the ballot), and only the test itself is per lane.  Per root then the value
// E and the error e = E w_p in [1, 65536], and for the whole column one
// atomicAdd of nu on the fix count, so that its entries are adjacent.
//
// The rows themselves are not here: the fix reports the error e, and the true
// symbol is (y_p - e) mod 65537.  Whether that symbol can be stored (65536 on
// a systematic data row cannot) is the holder's decision when it applies the
// fix (fec_stage.h apply_deltas), where qi_gpu_locate_multi makes it in its
// epilogue.
#include <hip/hip_runtime.h>

#include <string>

#include "gf65537.h"
#include "locate_multi_math.h"
#include "qi_internal.h"
#include "row_tile.h"
#include "syndrome_math.h"

namespace qi {

static_assert(kSynMaxChecks == kLocMaxChecks && kSynMaxErrors == kLocMaxErrors,
              "syndrome_math.h and locate_multi_math.h differ");

constexpr int kSynCtxHeld = 256;    // held (listed) positions per context block
constexpr int kSynCtxChunk = 1024;  // points staged in LDS at a time

// The checks both contexts share, by the whole block: the N ids below code_len
// and distinct (a 65536-bit map in LDS, cleared here).  Ends with a barrier
__device__ __forceinline__ bool syn_ids_bad(uint32_t* seen, const uint16_t* id_s, int N,
                                            int code_len, int tid)
{
    bool bad = false;
    for (int i = tid; i < 65536 / 32; i += kSynCtxHeld)
        seen[i] = 0;
    __syncthreads();
    for (int l = tid; l < N; l += kSynCtxHeld) {
        const uint32_t id = id_s[l];
        const uint32_t bit = 1u << (id & 31u);
        if (id >= static_cast<uint32_t>(code_len) || (atomicOr(&seen[id >> 5], bit) & bit))
            bad = true;
    }
    __syncthreads();
    return bad;
}

// w = A'(x) of the thread's point x at list position pos over the N points of
// the stripe, staged through sx kSynCtxChunk at a time (an id out of range
// enters as 0).  Called by the whole block; active: whether the thread has a
// point
__device__ __forceinline__ uint32_t syn_weight(uint32_t* sx, const uint16_t* id_s, int N,
                                               int code_len, uint32_t r, uint32_t x, int pos,
                                               bool active, int tid)
{
    uint32_t prod = 1;
    for (int l0 = 0; l0 < N; l0 += kSynCtxChunk) {
        const int n = min(kSynCtxChunk, N - l0);
        __syncthreads();  // the previous chunk has been read
        for (int l = tid; l < n; l += kSynCtxHeld) {
            const uint32_t id = id_s[l0 + l];
            sx[l] = pm_pow(r, id < static_cast<uint32_t>(code_len) ? id : 0u);
        }
        __syncthreads();
        if (active)
            prod = syndrome_weight(prod, x, sx, n, pos - l0);
    }
    return prod;
}

// ---------------------------------------------------------------------------
// The share context: one block per (stripe, chunk of kSynCtxHeld held
// positions), thread h owns a held position.  Every block checks the whole
// stripe with the map -- the ids, then (the map cleared) the positions below N
// and distinct; a bad one raises kErrBadIds and its row's coefficients are 0
// (a repeated id has w = 0).  Every word is written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kSynCtxHeld) void syndrome_ctx_kernel(
    int N, int code_len, uint32_t r, int H, int R, int RP, const uint16_t* __restrict__ ids,
    const uint16_t* __restrict__ held, int32_t* __restrict__ ctx, long long ctx_stride, int bps,
    uint32_t* err)
{
    __shared__ uint32_t seen[65536 / 32];
    __shared__ uint32_t sx[kSynCtxChunk];
    __shared__ uint32_t s_zero[kSynCtxHeld];
    const int s = static_cast<int>(blockIdx.x) / bps;
    const int cb = static_cast<int>(blockIdx.x) - s * bps;
    const int tid = static_cast<int>(threadIdx.x);
    int32_t* c = ctx + static_cast<long long>(s) * ctx_stride;
    const uint16_t* id_s = ids + static_cast<long long>(s) * N;
    const uint16_t* held_s = held + static_cast<long long>(s) * H;
    const int h = cb * kSynCtxHeld + tid;
    const bool is_held = h < H;

    s_zero[tid] = 0;
    bool bad = syn_ids_bad(seen, id_s, N, code_len, tid);

    // this thread's point and where it sits in the list
    uint32_t x = 0, own_id = 0;
    int pos = -1;
    bool zero = false;
    if (is_held) {
        pos = held_s[h];
        if (pos >= N) {
            zero = true;
            pos = 0;
        }
        own_id = id_s[pos];
        if (own_id >= static_cast<uint32_t>(code_len)) {
            zero = true;
            own_id = 0;
        }
        x = pm_pow(r, own_id);
    }
    bad |= zero;

    // the positions: the map again
    for (int i = tid; i < 65536 / 32; i += kSynCtxHeld)
        seen[i] = 0;
    __syncthreads();
    for (int j = tid; j < H; j += kSynCtxHeld) {
        const uint32_t p = held_s[j];
        const uint32_t bit = 1u << (p & 31u);
        if (p >= static_cast<uint32_t>(N)) {
            bad = true;
        } else if (atomicOr(&seen[p >> 5], bit) & bit) {
            bad = true;
            if (j / kSynCtxHeld == cb)
                s_zero[j - cb * kSynCtxHeld] = 1;
        }
    }
    if (bad)
        atomicOr(err, kErrBadIds);

    const uint32_t w = syn_weight(sx, id_s, N, code_len, r, x, pos, is_held, tid);
    __syncthreads();  // s_zero is complete

    if (is_held) {
        zero |= s_zero[tid] != 0;
        uint32_t v = zero ? 0u : pm_inv(w);
        for (int j = 0; j < RP; j++) {
            c[static_cast<long long>(h) * RP + j] = j < R ? partial_balanced(v) : 0;
            v = pm_mul(v, x);
        }
        c[static_cast<long long>(H) * RP + RP + h] = static_cast<int32_t>(own_id);
    }
    if (cb == 0 && tid < RP)
        c[static_cast<long long>(H) * RP + tid] = 0;
}

std::string syndrome_ctx_kernel_name()
{
    return "syndrome_ctx_kernel";
}

int launch_syndrome_ctx(int k, int code_len, uint32_t r, const uint16_t* d_ids,
                        const uint16_t* d_held, int H, int R, int S, int32_t* d_ctx,
                        uint32_t* err, hipStream_t st)
{
    const int N = k + R;
    if (k < 1 || R < 1 || R > kSynMaxChecks || H < 1 || H > N || N > code_len || S <= 0 ||
        code_len > 65536)
        return -3;
    const int bps = (H + kSynCtxHeld - 1) / kSynCtxHeld;
    const long long blocks = static_cast<long long>(bps) * S;
    if (blocks > 0x7fffffffLL)
        return -3;
    hipLaunchKernelGGL(syndrome_ctx_kernel, dim3(static_cast<unsigned>(blocks)),
                       dim3(kSynCtxHeld), 0, st, N, code_len, r, H, R, partial_rp(R), d_ids,
                       d_held, d_ctx, syndrome_ctx_words(H, R), bps, err);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------
// The resolve context: one block per (stripe, chunk of kSynCtxHeld listed
// positions), thread i owns list position i.  An id that is not below
// code_len or is repeated raises kErrBadIds; it enters as 0 (a repeated id
// has w = 0).  O(N^2) per stripe over ceil(N / 256) blocks.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kSynCtxHeld) void syndrome_locate_ctx_kernel(
    int N, int code_len, uint32_t r, const uint16_t* __restrict__ ids, int32_t* __restrict__ ctx,
    int bps, uint32_t* err)
{
    __shared__ uint32_t seen[65536 / 32];
    __shared__ uint32_t sx[kSynCtxChunk];
    const int s = static_cast<int>(blockIdx.x) / bps;
    const int cb = static_cast<int>(blockIdx.x) - s * bps;
    const int tid = static_cast<int>(threadIdx.x);
    int32_t* c = ctx + static_cast<long long>(s) * syndrome_locate_ctx_words(N);
    const uint16_t* id_s = ids + static_cast<long long>(s) * N;
    const int i = cb * kSynCtxHeld + tid;
    const bool listed = i < N;

    if (syn_ids_bad(seen, id_s, N, code_len, tid))
        atomicOr(err, kErrBadIds);
    uint32_t id = listed ? id_s[i] : 0u;
    if (id >= static_cast<uint32_t>(code_len))
        id = 0;
    const uint32_t x = pm_pow(r, id);
    const uint32_t w = syn_weight(sx, id_s, N, code_len, r, x, i, listed, tid);
    if (listed) {
        c[i] = static_cast<int32_t>(id);
        c[N + i] = static_cast<int32_t>(x);
        c[2 * N + i] = static_cast<int32_t>(w);
    }
}

std::string syndrome_locate_ctx_kernel_name()
{
    return "syndrome_locate_ctx_kernel";
}

int launch_syndrome_locate_ctx(int k, int R, int code_len, uint32_t r, const uint16_t* d_ids,
                               int S, int32_t* d_ctx, uint32_t* err, hipStream_t st)
{
    const int N = k + R;
    if (k < 1 || R < 1 || R > kSynMaxChecks || N > code_len || S <= 0 || code_len > 65536)
        return -3;
    const int bps = (N + kSynCtxHeld - 1) / kSynCtxHeld;
    const long long blocks = static_cast<long long>(bps) * S;
    if (blocks > 0x7fffffffLL)
        return -3;
    hipLaunchKernelGGL(syndrome_locate_ctx_kernel, dim3(static_cast<unsigned>(blocks)),
                       dim3(kSynCtxHeld), 0, st, N, code_len, r, d_ids, d_ctx, bps, err);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------
// The resolve kernel
// ---------------------------------------------------------------------------
struct SynLocArgs {
    const uint16_t* syn;  // syndrome row j of stripe s at syn + s * sss + j * srs
    long long sss, srs;
    Oor in;  // the syndrome rows' buckets, slot j (counts null: no marks)
    uint32_t* located;
    uint32_t* unlocated;
    uint32_t* weights;
    uint32_t* fix_counts;
    uint32_t* fixes;
    int fix_cap;
    long long words;
    int N, R, t, tiles;
    uint32_t* err;
};

// One lane's verdict on its column at element i: the recurrence C of order L
// over the syndromes S and its n roots pos[] among the listed points.  Located
// (n = L >= 1 and every error not 0): the weights, the located counters and
// the nu adjacent fix entries {column, position, e}; else unlocated
template <int RP, bool VEC>
__device__ __forceinline__ void syn_report(const SynLocArgs& a, int s, long long c0, int tid,
                                           int i, const uint32_t (&S)[RP],
                                           const uint32_t (&C)[RP / 2 + 1], int L, int n,
                                           const int (&pos)[RP / 2], const uint32_t* xs,
                                           const uint32_t* ws)
{
    constexpr int TM = RP / 2;
    bool found = L >= 1 && n == L;
    uint32_t v[TM];
    if (found) {
        const auto sel = [&](int j) {
            uint32_t r = 0;
#pragma unroll
            for (int jj = 0; jj < RP; jj++)
                r = j == jj ? S[jj] : r;
            return r;
        };
#pragma unroll
        for (int e = 0; e < TM; e++) {
            v[e] = 0;
            if (e < L) {
                const uint32_t E = lm_value<TM>(C, L, xs[pos[e]], sel);
                v[e] = lm_mul(E, ws[pos[e]]);  // e = E w_p
                found &= v[e] != 0;
            }
        }
    }
    if (!found) {
        atomicAdd(&a.unlocated[s], 1u);
        return;
    }
    const long long col = c0 + tile_rel<VEC>(tid, i);
    atomicAdd(&a.weights[static_cast<long long>(s) * kSynMaxErrors + (L - 1)], 1u);
    const uint32_t e0 = atomicAdd(&a.fix_counts[s], static_cast<uint32_t>(L));
#pragma unroll
    for (int e = 0; e < TM; e++) {
        if (e >= L)
            break;
        atomicAdd(&a.located[static_cast<long long>(s) * a.N + pos[e]], 1u);
        // (64 bits: the count goes on past fix_cap, up to nu per column)
        if (static_cast<unsigned long long>(e0) + e <
            static_cast<unsigned long long>(a.fix_cap)) {
            uint32_t* f = a.fixes + (static_cast<long long>(s) * a.fix_cap + e0 + e) * 3;
            f[0] = static_cast<uint32_t>(col);
            f[1] = static_cast<uint32_t>(pos[e]);
            f[2] = v[e];
        }
    }
}

template <int RP, bool VEC>
__global__ __launch_bounds__(kTileBlock) void syndrome_locate_kernel(
    SynLocArgs a, const int32_t* __restrict__ ctx)
{
    constexpr int TM = RP / 2;  // the largest t this form decodes
    __shared__ uint32_t bitmap[kTileElems / 32];
    const int tid = static_cast<int>(threadIdx.x);
    const int tile = static_cast<int>(blockIdx.x) % a.tiles;  // tiles fastest
    const int s = static_cast<int>(blockIdx.x) / a.tiles;
    const long long c0 = static_cast<long long>(tile) * kTileElems;
    const bool full = c0 + tid * kTileCols + kTileCols <= a.words;
    const int N = a.N;
    const uint32_t* xs =
        reinterpret_cast<const uint32_t*>(ctx) + static_cast<long long>(s) * 3 * N + N;
    const uint32_t* ws = xs + N;

    // the restored syndromes, in [0, 65536]; columns past the row's end read 0
    uint32_t syn[RP][kTileCols];
    uint32_t nz = 0;
#pragma unroll
    for (int j = 0; j < RP; j++) {
        if (j < a.R) {
            uint32_t w[4];
            tile_load<VEC>(a.syn + s * a.sss + j * a.srs, c0, tid, full, a.words, w);
            const long long bk = static_cast<long long>(s) * a.in.slots + j;
            const uint32_t cnt = a.in.counts ? a.in.counts[bk] : 0u;
            uint32_t mk = 0;
            if (cnt)
                mk = tile_marks<VEC>(bitmap, a.in, bk, cnt, c0, a.words, tid, a.err);
#pragma unroll
            for (int i = 0; i < kTileCols; i++) {
                syn[j][i] = mk >> i & 1u ? 65536u : w[i / 2] >> (i % 2 * 16) & 0xffffu;
                nz |= static_cast<uint32_t>(syn[j][i] != 0) << i;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kTileCols; i++)
                syn[j][i] = 0;
        }
    }
    if (!__ballot(nz != 0))
        return;

    // a lane whose column tile_rel(tid, i) lies past the row's end has nz bit
    // i clear: it read 0 and no mark names it (tile_marks drops col >= words)
#pragma nounroll
    for (int i = 0; i < kTileCols; i++) {
        const bool mine = nz >> i & 1u;
        if (!__ballot(mine))
            continue;
        uint32_t S[RP];
#pragma unroll
        for (int j = 0; j < RP; j++) {
            uint32_t v = 0;
#pragma unroll
            for (int ii = 0; ii < kTileCols; ii++)
                v = i == ii ? syn[j][ii] : v;
            S[j] = v;
        }
        uint32_t C[TM + 1];
        int L = -1;
        if (mine && a.t > 0)
            L = lm_berlekamp_massey<RP, TM>(S, a.R, a.t, C);
        int pos[TM];
#pragma unroll
        for (int e = 0; e < TM; e++)
            pos[e] = 0;
        int n = 0;
        if (__ballot(L >= 1)) {
            // the wave walks the points: p and x_p are the same in every lane
            for (int p = 0; p < N; p++) {
                const uint32_t x = xs[p];
                if (L >= 1 && lm_is_root<TM>(C, x)) {
#pragma unroll
                    for (int e = 0; e < TM; e++)
                        pos[e] = n == e ? p : pos[e];
                    n++;
                }
            }
        }
        if (mine)
            syn_report<RP, VEC>(a, s, c0, tid, i, S, C, L, n, pos, xs, ws);
    }
}

std::string syndrome_locate_kernel_name(int RP, bool vec)
{
    return "syndrome_locate_kernel<" + std::to_string(RP) + ", " + (vec ? "true" : "false") + ">";
}

template <int RP>
static void synloc_launch(bool vec, unsigned blocks, const SynLocArgs& a, const int32_t* ctx,
                          hipStream_t st)
{
    if (vec)
        hipLaunchKernelGGL((syndrome_locate_kernel<RP, true>), dim3(blocks), dim3(kTileBlock), 0,
                           st, a, ctx);
    else
        hipLaunchKernelGGL((syndrome_locate_kernel<RP, false>), dim3(blocks), dim3(kTileBlock), 0,
                           st, a, ctx);
}

// The decision over the R summed syndrome rows of n_stripes stripes, from
// contexts of syndrome_locate_ctx_words(k + R) words built by
// launch_syndrome_locate_ctx; `in`: the rows' buckets by slot j (counts null:
// no marks).  0 <= t <= R / 2.  The five outputs are cleared here.
int launch_syndrome_locate(const int32_t* d_ctx, int k, int R, int t, const uint16_t* d_syn,
                           long long sss, long long srs, const Oor& in, uint32_t* d_located,
                           uint32_t* d_unlocated, uint32_t* d_weights, uint32_t* d_fix_counts,
                           uint32_t* d_fixes, int fix_cap, long long words, int n_stripes,
                           uint32_t* d_err, hipStream_t st)
{
    if (k < 1 || R < 1 || R > kSynMaxChecks || t < 0 || 2 * t > R || n_stripes <= 0 ||
        words < 0 || fix_cap < 0)
        return -3;
    const int N = k + R;
    const size_t S = static_cast<size_t>(n_stripes);
    if (hipMemsetAsync(d_located, 0, S * N * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(d_unlocated, 0, S * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(d_weights, 0, S * kSynMaxErrors * sizeof(uint32_t), st) != hipSuccess ||
        hipMemsetAsync(d_fix_counts, 0, S * sizeof(uint32_t), st) != hipSuccess)
        return -2;
    if (words == 0)
        return 0;
    const long long tiles = (words + kTileElems - 1) / kTileElems;
    const long long nb = tiles * n_stripes;
    if (tiles > 0x7fffffffLL || nb > 0x7fffffffLL)
        return -3;
    const SynLocArgs a{d_syn, sss, srs, in, d_located, d_unlocated, d_weights, d_fix_counts,
                       d_fixes, fix_cap, words, N, R, t, static_cast<int>(tiles), d_err};
    const bool vec = rows_vec(d_syn, sss, srs);
    const unsigned blocks = static_cast<unsigned>(nb);
    switch (syndrome_locate_rp(R)) {
    case 2: synloc_launch<2>(vec, blocks, a, d_ctx, st); break;
    case 4: synloc_launch<4>(vec, blocks, a, d_ctx, st); break;
    default: synloc_launch<8>(vec, blocks, a, d_ctx, st); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
