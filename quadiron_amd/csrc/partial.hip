// Partial repair (qi_gpu_partial): the part of a repair's sum that one holder
// of H of the k helper rows can form,
//   out_t = acc_t + sum_{h<H} c(t, held[h]) row_h   (mod 65537),   t < R,
// with the Lagrange weights c of partial_math.h.  The sum is linear, so the
// partials of any partition of the k helpers add up, in any order, to what
// qi_gpu_repair writes.  partial_ctx_kernel leaves, per stripe, the H x RP
// balanced coefficients, the targets and the held rows' ids;
// partial_kernel streams the H rows once past RP x 8 accumulators per lane.
// H (+ R) rows in, R rows out, no matrix cores, no LDS image, any k.
//
// A block owns one stripe and one tile of kTileElems columns, a lane 8 columns
// (row_tile.h: the addressing, its two forms VEC and symbol by symbol, and the
// LDS bitmap that restores a row's marks in full).  It walks the H rows
// kPartAhead at a time: the loads of a group are issued before the first of
// them is used.  The loop is this file's own text; locate_rows.h says why.
// The accumulator column is read by the lane that writes the output column,
// before it writes it: d_out may be d_acc.
//
// Ranges (gf65537.h), as in locate.hip.  A restored symbol y is in [0, 65536]
// and a coefficient c balanced, in [-32768, 32768]: y c reaches 2^31, so the
// symbol is balanced too, yb = y - q for y > 32768 (the mark 65536 becomes
// -1), yb in [-32768, 32768], and |yb c| <= 2^30 is one v_mul_i32_i24.  The
// accumulator starts from the restored acc symbol, in [0, 65536] (or 0), which
// lies inside the loop's invariant [-16385, 81920]; it is folded at every
// term, acc <- fold(yb c + acc): the sum is inside +-(2^30 + 81920) < 2^31,
// its high half in [-16385, 16385], and the fold, lo - hi with lo in [0,
// 65535], is in [-16385, 81920] again.  After the last row one conditional + q
// and one conditional - q make it canonical, [0, 65536]; 65536 is stored as 0
// and recorded.  Columns past the row's end read 0 and compute 0: never
// recorded.
#include <hip/hip_runtime.h>

#include <string>

#include "gf65537.h"
#include "partial_math.h"
#include "qi_internal.h"
#include "row_tile.h"

namespace qi {

constexpr int kPartAhead = 4;       // rows in flight per lane
constexpr int kPartCtxHeld = 256;   // held positions per context block
constexpr int kPartCtxThreads = kPartCtxHeld + 64;  // + one wave for the targets
constexpr int kPartCtxChunk = 1024;  // points staged in LDS at a time
constexpr int kPartMaxTargets = 8;

// ---------------------------------------------------------------------------
// The context: one block per (stripe, chunk of kPartCtxHeld held positions).
// Thread h < 256 owns a held position i and forms A'(x_i), thread 256 + t the
// target t and forms A(y_t); both walk the k points x_l = r^ids[l], staged
// through LDS kPartCtxChunk at a time.  Then a held thread takes one inversion
// per target.  Every block checks the whole stripe with a 65536-bit map in
// LDS -- the ids below code_len and distinct, the targets below code_len,
// distinct and no helper, then (the map cleared) the positions below k and
// distinct; a bad one raises kErrBadIds and its coefficients are 0 (a repeated
// id has A' = 0, a target that is a helper A = 0).  Every word is written.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPartCtxThreads) void partial_ctx_kernel(
    int k, int code_len, uint32_t r, int H, int R, int RP, const uint16_t* __restrict__ ids,
    const uint16_t* __restrict__ held, const uint16_t* __restrict__ targets,
    int32_t* __restrict__ ctx, long long ctx_stride, int bps, uint32_t* err)
{
    __shared__ uint32_t seen[65536 / 32];
    __shared__ uint32_t sx[kPartCtxChunk];
    __shared__ uint32_t s_y[kPartMaxTargets], s_ay[kPartMaxTargets];
    __shared__ uint32_t s_zero[kPartCtxHeld];
    const int s = static_cast<int>(blockIdx.x) / bps;
    const int cb = static_cast<int>(blockIdx.x) - s * bps;
    const int tid = static_cast<int>(threadIdx.x);
    int32_t* c = ctx + static_cast<long long>(s) * ctx_stride;
    const uint16_t* id_s = ids + static_cast<long long>(s) * k;
    const uint16_t* held_s = held + static_cast<long long>(s) * H;
    const uint16_t* tg_s = targets + static_cast<long long>(s) * R;
    const int h = cb * kPartCtxHeld + tid;             // a held thread's row
    const bool is_held = tid < kPartCtxHeld && h < H;
    const int t = tid - kPartCtxHeld;                  // a target thread's target
    const bool is_target = t >= 0 && t < R;
    bool bad = false;

    for (int i = tid; i < 65536 / 32; i += kPartCtxThreads)
        seen[i] = 0;
    if (tid < kPartCtxHeld)
        s_zero[tid] = 0;
    __syncthreads();
    for (int l = tid; l < k; l += kPartCtxThreads) {
        const uint32_t id = id_s[l];
        const uint32_t bit = 1u << (id & 31u);
        if (id >= static_cast<uint32_t>(code_len) || (atomicOr(&seen[id >> 5], bit) & bit))
            bad = true;
    }
    __syncthreads();

    // this thread's point, and where it sits among the helpers (-1: nowhere)
    uint32_t x = 0, own_id = 0;
    int pos = -1;
    bool zero = false;
    if (is_target) {
        uint32_t tg = tg_s[t];
        const uint32_t bit = 1u << (tg & 31u);
        if (tg >= static_cast<uint32_t>(code_len)) {
            zero = true;
            tg = 0;
        } else if (atomicOr(&seen[tg >> 5], bit) & bit) {
            zero = true;  // repeated, or a helper
        }
        own_id = tg;
        x = pm_pow(r, tg);
    } else if (is_held) {
        pos = held_s[h];
        if (pos >= k) {
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
    __syncthreads();

    // the positions: the map again
    for (int i = tid; i < 65536 / 32; i += kPartCtxThreads)
        seen[i] = 0;
    __syncthreads();
    for (int j = tid; j < H; j += kPartCtxThreads) {
        const uint32_t p = held_s[j];
        const uint32_t bit = 1u << (p & 31u);
        if (p >= static_cast<uint32_t>(k)) {
            bad = true;
        } else if (atomicOr(&seen[p >> 5], bit) & bit) {
            bad = true;
            if (j / kPartCtxHeld == cb)
                s_zero[j - cb * kPartCtxHeld] = 1;
        }
    }
    if (bad)
        atomicOr(err, kErrBadIds);

    // A'(x_i) or A(y_t), a chunk of points at a time
    uint32_t prod = 1;
    for (int l0 = 0; l0 < k; l0 += kPartCtxChunk) {
        const int n = min(kPartCtxChunk, k - l0);
        __syncthreads();  // the previous chunk has been read
        for (int l = tid; l < n; l += kPartCtxThreads) {
            const uint32_t id = id_s[l0 + l];
            sx[l] = pm_pow(r, id < static_cast<uint32_t>(code_len) ? id : 0u);
        }
        __syncthreads();
        if (is_held || is_target)
            prod = partial_prod(prod, x, sx, n, pos - l0);
    }
    if (is_target) {
        s_y[t] = x;
        s_ay[t] = zero ? 0u : prod;
    }
    __syncthreads();  // s_zero, s_y and s_ay are complete

    if (is_held) {
        zero |= s_zero[tid] != 0;
        for (int j = 0; j < RP; j++) {
            uint32_t co = 0;
            if (j < R && !zero)
                co = partial_coef(s_ay[j], s_y[j], x, prod);
            c[static_cast<long long>(h) * RP + j] = partial_balanced(co);
        }
        c[static_cast<long long>(H) * RP + RP + h] = static_cast<int32_t>(own_id);
    }
    if (cb == 0 && t >= 0 && t < RP)
        c[static_cast<long long>(H) * RP + t] = is_target ? static_cast<int32_t>(own_id) : 0;
}

std::string partial_ctx_kernel_name()
{
    return "partial_ctx_kernel";
}

int launch_partial_ctx(int k, int code_len, uint32_t r, const uint16_t* d_ids,
                       const uint16_t* d_held, const uint16_t* d_targets, int H, int R, int S,
                       int32_t* d_ctx, uint32_t* err, hipStream_t st)
{
    if (k < 1 || H < 1 || H > k || R < 1 || R > kPartMaxTargets || S <= 0 || code_len > 65536)
        return -3;
    const int bps = (H + kPartCtxHeld - 1) / kPartCtxHeld;
    const long long blocks = static_cast<long long>(bps) * S;
    if (blocks > 0x7fffffffLL)
        return -3;
    hipLaunchKernelGGL(partial_ctx_kernel, dim3(static_cast<unsigned>(blocks)),
                       dim3(kPartCtxThreads), 0, st, k, code_len, r, H, R, partial_rp(R), d_ids,
                       d_held, d_targets, d_ctx, partial_ctx_words(H, R), bps, err);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// ---------------------------------------------------------------------------
// The apply kernel
// ---------------------------------------------------------------------------
struct PartArgs {
    long long ctx_stride;
    const uint16_t* rows;  // held row h of stripe s at rows + s * rss + h * rrs
    long long rss, rrs;
    const uint16_t* acc;  // accumulator row t (null: start from 0)
    long long ass, ars;
    uint16_t* out;
    long long oss, ors;
    Oor in, accm, outm;  // slots H, R, R (counts null: no marks / none recorded)
    long long words;
    int H, R, split, tiles;  // split: helper ids below it are data rows, no bucket
    uint32_t* err;
};

template <int RP, bool VEC>
__global__ __launch_bounds__(kTileBlock) void partial_kernel(PartArgs a,
                                                            const int32_t* __restrict__ ctx)
{
    __shared__ uint32_t bitmap[kTileElems / 32];
    const int tid = static_cast<int>(threadIdx.x);
    const int tile = static_cast<int>(blockIdx.x) % a.tiles;  // tiles fastest
    const int s = static_cast<int>(blockIdx.x) / a.tiles;
    const long long c0 = static_cast<long long>(tile) * kTileElems;
    const bool full = c0 + tid * kTileCols + kTileCols <= a.words;
    const int H = a.H;
    const int32_t* coef = ctx + static_cast<long long>(s) * a.ctx_stride;
    const int32_t* hid = coef + static_cast<long long>(H) * RP + RP;

    // the accumulators: the restored acc rows, in [0, 65536], or 0
    int32_t acc[RP][kTileCols];
#pragma unroll
    for (int j = 0; j < RP; j++) {
        if (a.acc && j < a.R) {
            uint32_t w[4];
            tile_load<VEC>(a.acc + s * a.ass + j * a.ars, c0, tid, full, a.words, w);
            const long long bk = static_cast<long long>(s) * a.accm.slots + j;
            const uint32_t cnt = a.accm.counts ? a.accm.counts[bk] : 0u;
            uint32_t mk = 0;
            if (cnt)
                mk = tile_marks<VEC>(bitmap, a.accm, bk, cnt, c0, a.words, tid, a.err);
#pragma unroll
            for (int i = 0; i < kTileCols; i++)
                acc[j][i] = mk >> i & 1u
                                ? 65536
                                : static_cast<int32_t>(w[i / 2] >> (i % 2 * 16) & 0xffffu);
        } else {
#pragma unroll
            for (int i = 0; i < kTileCols; i++)
                acc[j][i] = 0;
        }
    }

    const uint16_t* rows = a.rows + s * a.rss;
    for (int h0 = 0; h0 < H; h0 += kPartAhead) {
        uint32_t w[kPartAhead][4];
        uint32_t cnt[kPartAhead];
#pragma unroll
        for (int q = 0; q < kPartAhead; q++) {
            if (h0 + q < H) {
                tile_load<VEC>(rows + (h0 + q) * a.rrs, c0, tid, full, a.words, w[q]);
                cnt[q] = a.in.counts && hid[h0 + q] >= a.split
                             ? a.in.counts[static_cast<long long>(s) * a.in.slots + h0 + q]
                             : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < kPartAhead; q++) {
            if (h0 + q >= H)
                break;
            uint32_t mk = 0;
            if (cnt[q])
                mk = tile_marks<VEC>(bitmap, a.in,
                                     static_cast<long long>(s) * a.in.slots + h0 + q, cnt[q], c0,
                                     a.words, tid, a.err);
            const int32_t* c = coef + (h0 + q) * RP;
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

    uint16_t* out = a.out + s * a.oss;
#pragma unroll
    for (int j = 0; j < RP; j++) {
        if (j >= a.R)
            break;
        uint32_t y[kTileCols];
        uint32_t bad = 0;
#pragma unroll
        for (int i = 0; i < kTileCols; i++) {
            int32_t v = acc[j][i];  // [-16385, 81920]
            v = v < 0 ? v + kQ : v;
            v = v >= kQ ? v - kQ : v;
            bad |= static_cast<uint32_t>(v == 65536) << i;
            y[i] = static_cast<uint32_t>(v) & 0xffffu;
        }
        tile_store<VEC, false>(out + j * a.ors, c0, tid, full, a.words, y);
        if (bad && a.outm.counts) {
#pragma unroll
            for (int i = 0; i < kTileCols; i++)
                if (bad >> i & 1u)
                    tile_record_oor(a.outm, s, j, c0 + tile_rel<VEC>(tid, i));
        }
    }
}

std::string partial_kernel_name(int RP, bool vec)
{
    return "partial_kernel<" + std::to_string(RP) + ", " + (vec ? "true" : "false") + ">";
}

template <int RP>
static void part_launch(bool vec, unsigned blocks, const PartArgs& a, const int32_t* ctx,
                        hipStream_t st)
{
    if (vec)
        hipLaunchKernelGGL((partial_kernel<RP, true>), dim3(blocks), dim3(kTileBlock), 0, st, a,
                           ctx);
    else
        hipLaunchKernelGGL((partial_kernel<RP, false>), dim3(blocks), dim3(kTileBlock), 0, st, a,
                           ctx);
}

// out_t = acc_t + sum_h c(t, held[h]) row_h over n_stripes stripes, from
// contexts of partial_ctx_words(H, R) words built by launch_partial_ctx.  in,
// accm, outm: the buckets of the held rows (slot h), of the acc rows and of the
// output rows (slot t); counts null: none.  d_acc null: start from 0
int launch_partial(const int32_t* d_ctx, int H, int R, int split, const uint16_t* d_rows,
                   long long rss, long long rrs, const Oor& in, const uint16_t* d_acc,
                   long long ass, long long ars, const Oor& accm, uint16_t* d_out, long long oss,
                   long long ors, const Oor& outm, long long words, int n_stripes,
                   uint32_t* d_err, hipStream_t st)
{
    if (H < 1 || R < 1 || R > kPartMaxTargets || n_stripes <= 0 || words <= 0)
        return -3;
    const long long tiles = (words + kTileElems - 1) / kTileElems;
    const long long blocks = tiles * n_stripes;
    if (tiles > 0x7fffffffLL || blocks > 0x7fffffffLL)
        return -3;
    const PartArgs a{partial_ctx_words(H, R), d_rows, rss, rrs, d_acc, ass, ars, d_out, oss, ors,
                     in, accm, outm, words, H, R, split, static_cast<int>(tiles), d_err};
    const bool vec = rows_vec(d_rows, rss, rrs) && (!d_acc || rows_vec(d_acc, ass, ars)) &&
                     rows_vec(d_out, oss, ors);
    const unsigned nb = static_cast<unsigned>(blocks);
    switch (partial_rp(R)) {
    case 1: part_launch<1>(vec, nb, a, d_ctx, st); break;
    case 2: part_launch<2>(vec, nb, a, d_ctx, st); break;
    case 4: part_launch<4>(vec, nb, a, d_ctx, st); break;
    default: part_launch<8>(vec, nb, a, d_ctx, st); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
