// Multi-fragment locate (qi_gpu_locate_multi): up to t = max_errors bad
// fragments per column among the N = k + R listed ones, 2 t <= R.  It reads
// the locate's context (locate.hip's locate_ctx_kernel: ids, x_i, w_i and the
// coefficients) and runs the locate's row pass (locate_rows.h): N rows in, the
// R syndromes of a lane's 8 columns in registers, no row out.  What is new is
// the epilogue, the bounded-distance decoder of locate_multi_math.h.
//
// The epilogue is one lane per column: a lane decodes its own non-clean
// columns one after the other -- Berlekamp-Massey in registers (every index a
// compile-time one), the root test of sigma at the N points x_i, which the
// block stages in LDS (all lanes read the same word: a broadcast), then per
// root the value E, the reload of the named symbol with its bucket scan, the
// storability check, and for the whole column one atomicAdd of nu on the fix
// count, so that its entries are adjacent.  The exit after the row pass is a
// block-wide decision (__syncthreads_or): the staging needs a barrier.
//
// Why not a wave-cooperative drain of a column queue: with a whole fragment
// bad every lane has 8 columns to decode, and the work is columns x (BM + N
// root tests) whichever lanes do it.  Lane per column keeps all 64 lanes busy
// on distinct columns; a drain that decodes one column per wave step would
// run BM 512 times in sequence per wave and only spread the N root tests, 8 x
// (BM + N t) multiplies against 512 x (BM + ceil(N / 64) t) per wave.  The
// price is the sparse case, where one lane walks the N points alone; there
// the epilogue is a vanishing share of the run.
#include <hip/hip_runtime.h>

#include <string>

#include "gf65537.h"
#include "locate_math.h"
#include "locate_multi_math.h"
#include "locate_rows.h"
#include "qi_internal.h"

namespace qi {

template <int RP, bool VEC>
__global__ __launch_bounds__(kTileBlock) void locate_multi_kernel(LocArgs a, uint32_t* weights,
                                                                 int t,
                                                                 const int32_t* __restrict__ ctx)
{
    constexpr int TM = RP / 2;  // the largest t this form decodes
    __shared__ uint32_t bitmap[kTileElems / 32];
    __shared__ uint32_t sx[kLocMaxK + kLocMaxChecks];
    const int tid = static_cast<int>(threadIdx.x);
    const int tile = static_cast<int>(blockIdx.x) % a.tiles;  // tiles fastest
    const int s = static_cast<int>(blockIdx.x) / a.tiles;
    const long long sr = a.stripes ? a.stripes[s] : s;
    const long long c0 = static_cast<long long>(tile) * kTileElems;
    const int N = a.N;
    const int32_t* ids = ctx + static_cast<long long>(s) * a.ctx_stride;

    int32_t acc[RP][kTileCols];
    uint32_t nz = loc_syndromes<RP, VEC>(a, ids, sr, c0, tid, bitmap, acc);
    if (!__syncthreads_or(nz != 0))
        return;

    const uint32_t* xs = reinterpret_cast<const uint32_t*>(ids + N);
    const uint32_t* ws = reinterpret_cast<const uint32_t*>(ids + 2 * N);
    for (int i = tid; i < N; i += kTileBlock)
        sx[i] = xs[i];
    __syncthreads();

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
        uint32_t C[TM + 1];
        const int L = lm_berlekamp_massey<RP, TM>(S, a.R, t, C);
        int pos[TM];
#pragma unroll
        for (int e = 0; e < TM; e++)
            pos[e] = 0;
        int n = 0;
        if (L >= 1) {
            for (int p = 0; p < N; p++) {
                if (lm_is_root<TM>(C, sx[p])) {
#pragma unroll
                    for (int e = 0; e < TM; e++)
                        pos[e] = n == e ? p : pos[e];
                    n++;
                }
            }
        }
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
                    const uint32_t E = lm_value<TM>(C, L, sx[pos[e]], sel);
                    bool data_row;
                    const uint32_t y =
                        tile_symbol(a.rows(), a.in, sr, ids[pos[e]], col, &data_row);
                    found &= locate_fix(y, E, ws[pos[e]], data_row, &v[e]) && E != 0;
                }
            }
        }
        if (!found) {
            atomicAdd(&a.unlocated[s], 1u);
            continue;
        }
        atomicAdd(&weights[static_cast<long long>(s) * kLocMaxErrors + (L - 1)], 1u);
        const uint32_t e0 = atomicAdd(&a.fix_counts[s], static_cast<uint32_t>(L));
#pragma unroll
        for (int e = 0; e < TM; e++) {
            if (e >= L)
                break;
            atomicAdd(&a.located[static_cast<long long>(s) * N + pos[e]], 1u);
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
}

std::string locate_multi_kernel_name(int RP, bool vec)
{
    return "locate_multi_kernel<" + std::to_string(RP) + ", " + (vec ? "true" : "false") + ">";
}

template <int RP>
static void locm_launch(bool vec, unsigned blocks, const LocArgs& a, uint32_t* weights, int t,
                        const int32_t* ctx, hipStream_t st)
{
    if (vec)
        hipLaunchKernelGGL((locate_multi_kernel<RP, true>), dim3(blocks), dim3(kTileBlock), 0, st,
                           a, weights, t, ctx);
    else
        hipLaunchKernelGGL((locate_multi_kernel<RP, false>), dim3(blocks), dim3(kTileBlock), 0, st,
                           a, weights, t, ctx);
}

// launch_locate's arguments (qi_internal.h) with the bound t, 1 <= t <= R / 2,
// and the weights [n_stripes][kLocMaxErrors].  The five outputs are cleared
// here.
int launch_locate_multi(const int32_t* d_ctx, int k, int R, int t, int split,
                        const uint32_t* d_stripes, const uint16_t* d_data, long long dss,
                        long long drs, const uint16_t* d_coded, long long css, long long crs,
                        const Oor& in, uint32_t* d_located, uint32_t* d_unlocated,
                        uint32_t* d_weights, uint32_t* d_fix_counts, uint32_t* d_fixes,
                        int fix_cap, long long words, int n_stripes, uint32_t* d_err,
                        hipStream_t st)
{
    if (t < 1 || 2 * t > R)
        return -3;
    LocArgs a;
    unsigned nb;
    bool vec;
    const int rc = loc_prepare(k, R, split, d_stripes, d_data, dss, drs, d_coded, css, crs, in,
                               d_located, d_unlocated, d_fix_counts, d_fixes, fix_cap, words,
                               n_stripes, d_err, st, &a, &nb, &vec);
    if (rc < 0)
        return rc;
    if (hipMemsetAsync(d_weights, 0, static_cast<size_t>(n_stripes) * kLocMaxErrors *
                                         sizeof(uint32_t), st) != hipSuccess)
        return -2;
    if (rc == 0)
        return 0;
    switch (locate_rp(R)) {
    case 2: locm_launch<2>(vec, nb, a, d_weights, t, d_ctx, st); break;
    case 4: locm_launch<4>(vec, nb, a, d_weights, t, d_ctx, st); break;
    default: locm_launch<8>(vec, nb, a, d_weights, t, d_ctx, st); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
