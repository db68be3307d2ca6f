// Delta update (qi_gpu_update): coded rows follow U changed data rows,
//   out[slot] = coded[slot] + sum_u c(slot, id_u) (new_u - old_u)   (mod 65537)
// with the coefficients update_ctx_kernel (ctx.hip) left in the context.  A
// streaming kernel: 2U + R rows in, R rows out, no matrix cores, no LDS image.
//
// A block owns one stripe, one tile of kTileElems columns and a chunk of the
// listed slots.  It loads the U old and U new rows of its columns once, keeps
// d_u = balanced(new_u - old_u) in registers (8 columns per lane) and walks
// its slots kUpdAhead coded rows at a time: the loads of a group are issued
// before its first store, so they are in flight together.  The coded column
// is read by the lane that writes the output column, before it writes it:
// d_out may be d_coded.
//
// The tile, its flat addressing in the two forms VEC (16-byte pieces) and
// symbol by symbol, and the LDS bitmap of a row's marks are row_tile.h's.
//
// Ranges (gf65537.h): a data symbol is in [0, 65535], so new - old is in
// [-65535, 65535] and its balanced representative d in [-32768, 32768]; the
// coefficients are balanced too, so |c d| <= 2^30 fits v_mul_i32_i24's int32
// result and fold(c d) is in [-16384, 81919] (lo in [0, 65535], hi in
// [-16384, 16384]).  The restored coded symbol is in [0, 65536]; with 8 terms
// acc is in [-131072, 720888], inside (-2^20, 2^20): fold(acc) = lo - hi with
// hi in [-2, 10] is in [-10, 65537], and one conditional +-q each way makes
// it canonical, [0, 65536].  65536 is stored as 0 and recorded.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "gf65537.h"
#include "qi_internal.h"
#include "row_tile.h"

namespace qi {

constexpr int kUpdAhead = 4;  // coded rows in flight per lane
// Blocks wanted before the slots of a stripe tile stay in one block (4 per
// CU of a 256-CU device), and the fewest slots a block takes per changed row
// when they are split: the 2U rows of d are then at most 1 / (1 +
// kUpdSlotsPerRow) of a block's row traffic.
constexpr long long kUpdMinBlocks = 1024;
constexpr int kUpdSlotsPerRow = 4;

// Store policy of the output rows: plain stores, or nontemporal ones
// (-DQI_UPD_NT_STORE=1).  See DESIGN.md 4.13 for what was measured.
#ifndef QI_UPD_NT_STORE
#define QI_UPD_NT_STORE 0
#endif

struct UpdArgs {
    long long ctx_stride;
    const uint16_t* olds;
    long long old_ss, old_rs;
    const uint16_t* news;
    long long new_ss, new_rs;
    const uint16_t* coded;
    long long css, crs;
    uint16_t* out;
    long long oss, ors;
    Oor in, outm;  // counts null: no marks to restore / none recorded
    long long words;
    int R, U, tiles, chunk, chunks;
    int by_pos;  // row and bucket of the j-th listed slot: j instead of the slot
    uint32_t* err;
};

template <int UP, bool VEC>
__global__ __launch_bounds__(kTileBlock) void update_kernel(UpdArgs a,
                                                           const int32_t* __restrict__ ctx)
{
    __shared__ uint32_t bitmap[kTileElems / 32];
    const int tid = static_cast<int>(threadIdx.x);
    // block -> (stripe, slot chunk, tile), tiles fastest
    int b = static_cast<int>(blockIdx.x);
    const int tile = b % a.tiles;
    b /= a.tiles;
    const int ch = b % a.chunks;
    const int s = b / a.chunks;
    const long long c0 = static_cast<long long>(tile) * kTileElems;
    const bool full = c0 + tid * kTileCols + kTileCols <= a.words;
    const int32_t* coef = ctx + static_cast<long long>(s) * a.ctx_stride;
    const int32_t* slot_of = coef + static_cast<long long>(a.R) * UP;

    // d_u = balanced(new_u - old_u), in [-32768, 32768]
    int32_t d[UP][kTileCols];
#pragma unroll
    for (int u = 0; u < UP; u++) {
        if (u < a.U) {
            uint32_t wo[4], wn[4];
            tile_load<VEC>(a.olds + s * a.old_ss + u * a.old_rs, c0, tid, full, a.words, wo);
            tile_load<VEC>(a.news + s * a.new_ss + u * a.new_rs, c0, tid, full, a.words, wn);
#pragma unroll
            for (int i = 0; i < kTileCols; i++) {
                const int32_t o = static_cast<int32_t>(wo[i / 2] >> (i % 2 * 16) & 0xffffu);
                const int32_t n = static_cast<int32_t>(wn[i / 2] >> (i % 2 * 16) & 0xffffu);
                const int32_t x = n - o;
                d[u][i] = x > 32768 ? x - kQ : x < -32768 ? x + kQ : x;
            }
        } else {
#pragma unroll
            for (int i = 0; i < kTileCols; i++)
                d[u][i] = 0;
        }
    }

    const uint16_t* coded = a.coded + s * a.css;
    uint16_t* out = a.out + s * a.oss;
    const int j1 = min(a.R, (ch + 1) * a.chunk);
    for (int j = ch * a.chunk; j < j1; j += kUpdAhead) {
        // a group's rows are all loaded before the first of them is written
        uint32_t w[kUpdAhead][4];
        int slot[kUpdAhead];
        uint32_t cnt[kUpdAhead];
#pragma unroll
        for (int q = 0; q < kUpdAhead; q++) {
            if (j + q < j1) {
                slot[q] = a.by_pos ? j + q : slot_of[j + q];
                tile_load<VEC>(coded + slot[q] * a.crs, c0, tid, full, a.words, w[q]);
                cnt[q] = a.in.counts
                             ? a.in.counts[static_cast<long long>(s) * a.in.slots + slot[q]]
                             : 0u;
            }
        }
#pragma unroll
        for (int q = 0; q < kUpdAhead; q++) {
            if (j + q >= j1)
                break;
            uint32_t mk = 0;
            if (cnt[q])
                mk = tile_marks<VEC>(bitmap, a.in,
                                     static_cast<long long>(s) * a.in.slots + slot[q], cnt[q], c0,
                                     a.words, tid, a.err);
            const int32_t* c = coef + static_cast<long long>(j + q) * UP;
            uint32_t y[kTileCols];
            uint32_t bad = 0;
#pragma unroll
            for (int i = 0; i < kTileCols; i++) {
                // a marked symbol is 65536 (stored as 0)
                int32_t acc = mk >> i & 1u
                                  ? 65536
                                  : static_cast<int32_t>(w[q][i / 2] >> (i % 2 * 16) & 0xffffu);
#pragma unroll
                for (int u = 0; u < UP; u++)
                    acc += fold(__mul24(c[u], d[u][i]));
                int32_t v = fold(acc);  // [-10, 65537]
                v = v < 0 ? v + kQ : v;
                v = v >= kQ ? v - kQ : v;
                bad |= static_cast<uint32_t>(v == 65536) << i;
                y[i] = static_cast<uint32_t>(v) & 0xffffu;
            }
            tile_store<VEC, QI_UPD_NT_STORE != 0>(out + slot[q] * a.ors, c0, tid, full, a.words,
                                                  y);
            // (a column past the row's end computes 0: never recorded)
            if (bad && a.outm.counts) {
#pragma unroll
                for (int i = 0; i < kTileCols; i++)
                    if (bad >> i & 1u)
                        tile_record_oor(a.outm, s, slot[q], c0 + tile_rel<VEC>(tid, i));
            }
        }
    }
}

std::string update_kernel_name(int UP, bool vec)
{
    return "update_kernel<" + std::to_string(UP) + ", " + (vec ? "true" : "false") + ">";
}

template <int UP>
static void upd_launch(bool vec, unsigned blocks, const UpdArgs& a, const int32_t* ctx,
                       hipStream_t st)
{
    if (vec)
        hipLaunchKernelGGL((update_kernel<UP, true>), dim3(blocks), dim3(kTileBlock), 0, st, a,
                           ctx);
    else
        hipLaunchKernelGGL((update_kernel<UP, false>), dim3(blocks), dim3(kTileBlock), 0, st, a,
                           ctx);
}

// out[slot] = coded[slot] + sum_u c (new_u - old_u) over the R listed slots
// of n_stripes stripes, from contexts of update_ctx_words(U, R) words built by
// launch_update_ctx; UP = update_up(U).  in / outm: the coded rows' buckets
// and the updated rows', both by slot (counts null: none); by_pos: rows and
// buckets by the slot's position in the list instead.
int launch_update(const int32_t* d_ctx, long long ctx_stride, int U, int UP, int R, int by_pos,
                  const uint16_t* d_old, long long old_ss, long long old_rs,
                  const uint16_t* d_new, long long new_ss, long long new_rs,
                  const uint16_t* d_coded, long long css, long long crs, const Oor& in,
                  uint16_t* d_out, long long oss, long long ors, const Oor& outm, long long words,
                  int n_stripes, uint32_t* d_err, hipStream_t st)
{
    if (U < 1 || U > UP || R < 1 || n_stripes <= 0 || words <= 0)
        return -3;
    const long long tiles = (words + kTileElems - 1) / kTileElems;
    const long long st_tiles = tiles * n_stripes;
    // slots per block: all of them while that leaves enough blocks, else
    // halved down to kUpdSlotsPerRow per changed row (never below 4)
    const int floor_ = kUpdSlotsPerRow * U;
    int chunk = R;
    while (st_tiles * ((R + chunk - 1) / chunk) < kUpdMinBlocks && chunk > floor_)
        chunk = std::max(floor_, (chunk + 1) / 2);
    const int chunks = (R + chunk - 1) / chunk;
    const long long blocks = st_tiles * chunks;
    if (tiles > 0x7fffffffLL || blocks > 0x7fffffffLL)
        return -3;
    UpdArgs a{ctx_stride, d_old, old_ss, old_rs, d_new, new_ss, new_rs, d_coded, css, crs,
              d_out, oss, ors, in, outm, words, R, U, static_cast<int>(tiles), chunk, chunks,
              by_pos, d_err};
    const bool vec = rows_vec(d_old, old_ss, old_rs) && rows_vec(d_new, new_ss, new_rs) &&
                     rows_vec(d_coded, css, crs) && rows_vec(d_out, oss, ors);
    const unsigned nb = static_cast<unsigned>(blocks);
    switch (UP) {
    case 1: upd_launch<1>(vec, nb, a, d_ctx, st); break;
    case 2: upd_launch<2>(vec, nb, a, d_ctx, st); break;
    case 4: upd_launch<4>(vec, nb, a, d_ctx, st); break;
    case 8: upd_launch<8>(vec, nb, a, d_ctx, st); break;
    default: return -3;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
