// Fragment fingerprints (qi_gpu_fingerprint): fp_j = sum_c y_c w_j(first_col +
// c) mod 65537 over the restored symbols of each listed row, F keys per call.
// The definition, the split of the weight and the range argument are at the
// top of fingerprint_math.h.
//
// Three kernels on the caller's stream:
//   fingerprint_tab_kernel     the power tables of the call's keys in the work
//                              buffer: a^x, b^x (x < 256) and d^C2 for the C2
//                              the call's columns meet.  The keys travel as
//                              kernel arguments;
//   fingerprint_kernel<FP, VEC>  a block owns one (stripe, row, chunk of
//                              kFpChunkTiles tiles of kFpTile columns) and
//                              reads the row once;
//   fingerprint_finish_kernel  rows longer than one chunk: adds the chunks'
//                              canonical partials (work buffer) in order.
//
// The row kernel.  The block first multiplies the kFpHi hi weights b^C1 d^C2
// of its chunk out of the tables into LDS, and every lane loads its a^C0.
// VEC (every base and stride a multiple of 16 bytes, first_col of 8 columns):
// a lane loads 16-byte pieces, kFpAhead tiles in flight; its 8 columns share
// H = C >> 8, so a piece is sum_i y_i a^i with the eight a^i wave-uniform
// (kernel arguments), rebalanced and stepped once with the hi weight: one
// mul24 + fold per (symbol, key), the hi step once per 8 symbols.  Otherwise
// the lane's columns are 256 apart (scalar loads, any alignment): they share
// C0, and each symbol is stepped with the hi weight of its own H.  Either way
// the lane's a^C0 is one canonical product per key at the end.  The loads and
// the marks, through the LDS bitmap of the tile (no density limit), are
// row_tile.h's.
// The block sums its lanes' canonical values by wave shuffles, then LDS:
// integer sums, so the result does not depend on the grid.  No floating point,
// no atomics on results.
#include <hip/hip_runtime.h>

#include <string>

#include "fingerprint_math.h"
#include "gf65537.h"
#include "qi_internal.h"
#include "row_tile.h"

namespace qi {

// fingerprint_math.h keeps its own names for the host's index math
static_assert(kFpBlock == kTileBlock && kFpCols == kTileCols,
              "fingerprint_math.h's tile is row_tile.h's");

constexpr int kFpAhead = 4;  // tiles in flight per lane

struct FpKeys {
    uint32_t key[kFpMaxKeys][3];
};
// the balanced a^i, i < 8, of each key
template <int FP>
struct FpPowers {
    int32_t ap[FP][kFpCols];
};

struct FpArgs {
    const uint16_t* ids;  // [S][N]
    const uint16_t* data;  // fragments below `split` (null: none held)
    long long dss, drs;
    const uint16_t* coded;  // the others, by slot id - split (null: none held)
    long long css, crs;
    Oor in;  // the coded rows' buckets by slot (counts null: no marks)
    const uint32_t* tab;  // fp_tab_entry rows of FP keys
    uint32_t* part;  // [S * N][chunks][FP], chunks > 1
    uint32_t* fp;  // [S * N][F]
    long long words, first_col, c2s;
    int N, F, split, code_len, chunks;
    uint32_t* err;
};

__device__ __forceinline__ bool fp_bad_id(const FpArgs& a, int id)
{
    return id >= a.code_len || (id < a.split ? !a.data : !a.coded);
}

__global__ __launch_bounds__(kFpBlock) void fingerprint_tab_kernel(FpKeys k, int FP,
                                                                   long long c2base,
                                                                   long long c2s, uint32_t* tab)
{
    const long long e = static_cast<long long>(blockIdx.x) * kFpBlock + threadIdx.x;
    if (e >= fp_tab_words(c2s, FP))
        return;
    tab[e] = fp_tab_entry(k.key[e % FP], e / FP, c2base);
}

template <int FP, bool VEC>
__global__ __launch_bounds__(kFpBlock) void fingerprint_kernel(FpArgs a, FpPowers<FP> pw)
{
    __shared__ uint32_t bitmap[kFpTile / 32];
    __shared__ int32_t hiw[kFpHi * FP];
    __shared__ uint32_t red[kFpBlock / 64][FP];
    const int tid = static_cast<int>(threadIdx.x);
    const int ch = static_cast<int>(blockIdx.x % static_cast<unsigned>(a.chunks));
    const long long row = blockIdx.x / static_cast<unsigned>(a.chunks);  // s * N + position
    const long long s = row / a.N;
    const int id = a.ids[row];
    if (fp_bad_id(a, id)) {  // nothing is read; chunks > 1: the finish kernel writes
        if (ch == 0 && tid == 0)
            atomicOr(a.err, kErrBadIds);
        if (a.chunks == 1 && tid < a.F)
            a.fp[row * a.F + tid] = 0xFFFFFFFFu;
        return;
    }
    // row_tile.h's frag_row in this file's own text: called from here it
    // reorders the kernel's argument loads (13 more instructions over the forms)
    const uint16_t* rp;
    long long bk = -1;
    if (id < a.split) {
        rp = a.data + s * a.dss + id * a.drs;
    } else {
        const int slot = id - a.split;
        bk = s * a.in.slots + slot;
        rp = a.coded + s * a.css + slot * a.crs;
    }
    const uint32_t cnt = bk >= 0 && a.in.counts ? a.in.counts[bk] : 0u;

    // the chunk's hi weights and the lane's a^C0
    const long long cbeg = ch * kFpChunk;
    const long long abs0 = a.first_col + cbeg;
    for (int e = tid; e < kFpHi * FP; e += kFpBlock)
        hiw[e] = fp_hi_weight(a.tab, FP, e % FP, (abs0 >> 8) + e / FP, a.first_col >> 16, a.c2s);
    const FpLane ln = fp_lane(VEC, static_cast<int>(abs0 & 255), tid);
    uint32_t A[FP];
#pragma unroll
    for (int j = 0; j < FP; j++)
        A[j] = a.tab[ln.a_row * FP + j];
    __syncthreads();

    int32_t acc[FP];
#pragma unroll
    for (int j = 0; j < FP; j++)
        acc[j] = 0;
    const long long left = (a.words - cbeg + kFpTile - 1) / kFpTile;
    const int nt = left < kFpChunkTiles ? static_cast<int>(left) : kFpChunkTiles;
    for (int t0 = 0; t0 < nt; t0 += kFpAhead) {
        uint32_t w[kFpAhead][4];
#pragma unroll
        for (int q = 0; q < kFpAhead; q++) {
            if (t0 + q < nt) {
                const long long c0 = cbeg + static_cast<long long>(t0 + q) * kFpTile;
                tile_load<VEC>(rp, c0, tid, c0 + tid * kFpCols + kFpCols <= a.words, a.words,
                              w[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < kFpAhead; q++) {
            if (t0 + q >= nt)
                break;
            const long long c0 = cbeg + static_cast<long long>(t0 + q) * kFpTile;
            uint32_t mk = 0;
            if (cnt)
                mk = tile_marks<VEC>(bitmap, a.in, bk, cnt, c0, a.words, tid, a.err);
            int32_t y[kFpCols];
#pragma unroll
            for (int i = 0; i < kFpCols; i++)
                y[i] = fp_sym(w[q][i / 2] >> (i % 2 * 16) & 0xffffu, mk >> i & 1u);
            if (VEC) {
                const int32_t* hw = hiw + fp_hi_index(true, t0 + q, ln.hl, 0) * FP;
#pragma unroll
                for (int j = 0; j < FP; j++)
                    acc[j] = fp_step(acc[j], fp_rebalance(fp_piece(y, pw.ap[j])), hw[j]);
            } else {
#pragma unroll
                for (int i = 0; i < kFpCols; i++) {
                    const int32_t* hw = hiw + fp_hi_index(false, t0 + q, ln.hl, i) * FP;
#pragma unroll
                    for (int j = 0; j < FP; j++)
                        acc[j] = fp_step(acc[j], y[i], hw[j]);
                }
            }
        }
    }

    // the lane's a^C0, then the block's sum: 256 canonical values stay below 2^25
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int j = 0; j < FP; j++) {
        uint32_t v = fp_mulmod(fp_canon(acc[j]), A[j]);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1)
            v += __shfl_down(v, d, 64);
        if (lane == 0)
            red[wave][j] = v;
    }
    __syncthreads();
    if (tid < FP) {
        uint32_t v = 0;
#pragma unroll
        for (int wv = 0; wv < kFpBlock / 64; wv++)
            v += red[wv][tid];
        v %= static_cast<uint32_t>(kQ);
        if (a.chunks > 1)
            a.part[(row * a.chunks + ch) * FP + tid] = v;
        else if (tid < a.F)
            a.fp[row * a.F + tid] = v;
    }
}

__global__ __launch_bounds__(kFpBlock) void fingerprint_finish_kernel(FpArgs a, int FP,
                                                                      long long n)
{
    const long long e = static_cast<long long>(blockIdx.x) * kFpBlock + threadIdx.x;
    if (e >= n)
        return;
    const long long row = e / a.F;
    const int j = static_cast<int>(e % a.F);
    if (fp_bad_id(a, a.ids[row])) {
        a.fp[e] = 0xFFFFFFFFu;
        return;
    }
    uint32_t v = 0;
    for (int c = 0; c < a.chunks; c++) {
        v += a.part[(row * a.chunks + c) * FP + j];
        v = v >= static_cast<uint32_t>(kQ) ? v - static_cast<uint32_t>(kQ) : v;
    }
    a.fp[e] = v;
}

std::string fingerprint_kernel_names(int F, bool vec, long long words)
{
    std::string s = "fingerprint_tab_kernel + fingerprint_kernel<" + std::to_string(fp_pad(F)) +
                    ", " + (vec ? "true" : "false") + ">";
    if (fp_chunks(words) > 1)
        s += " + fingerprint_finish_kernel";
    return s;
}

template <int FP>
static void fp_launch(bool vec, unsigned blocks, const FpArgs& a, const uint32_t* keys,
                      hipStream_t st)
{
    FpPowers<FP> pw;
    for (int j = 0; j < FP; j++)
        for (int i = 0; i < kFpCols; i++)
            pw.ap[j][i] = j < a.F ? balanced(fp_powmod(keys[3 * j], static_cast<uint32_t>(i)))
                                  : 1;
    if (vec)
        hipLaunchKernelGGL((fingerprint_kernel<FP, true>), dim3(blocks), dim3(kFpBlock), 0, st, a,
                           pw);
    else
        hipLaunchKernelGGL((fingerprint_kernel<FP, false>), dim3(blocks), dim3(kFpBlock), 0, st,
                           a, pw);
}

// The arguments are qi_gpu_fingerprint's, checked there (keys in range, 1 <= F
// <= 8, 1 <= N, 1 <= words, first_col + words <= 2^32); split / code_len: the
// plan's.  d_work: fp_work_words(S * N, fp_pad(F), words) u32.
int launch_fingerprint(const uint16_t* d_ids, int N, const uint32_t* keys, int F,
                       long long first_col, int split, int code_len, const uint16_t* d_data,
                       long long dss, long long drs, const uint16_t* d_coded, long long css,
                       long long crs, const Oor& in, uint32_t* d_work, uint32_t* d_fp,
                       long long words, int n_stripes, uint32_t* d_err, hipStream_t st)
{
    const int FP = fp_pad(F);
    const long long chunks = fp_chunks(words);
    const long long rows = static_cast<long long>(n_stripes) * N;
    if (chunks > 0x7fffffffLL / rows)
        return -3;
    const long long c2s = fp_c2_count(first_col, words);
    FpKeys k;
    for (int j = 0; j < kFpMaxKeys; j++)
        for (int c = 0; c < 3; c++)
            k.key[j][c] = j < F ? keys[3 * j + c] : 1u;  // a dead key
    const long long tw = fp_tab_words(c2s, FP);
    hipLaunchKernelGGL(fingerprint_tab_kernel, dim3(static_cast<unsigned>((tw + kFpBlock - 1) /
                                                                          kFpBlock)),
                       dim3(kFpBlock), 0, st, k, FP, first_col >> 16, c2s, d_work);
    FpArgs a{d_ids, d_data, dss, drs, d_coded, css, crs, in, d_work,
             d_work + fp_tab_words(fp_c2_max(words), FP), d_fp, words, first_col, c2s, N, F,
             split, code_len, static_cast<int>(chunks), d_err};
    const bool vec = fingerprint_rows_vec(first_col, split, d_data, dss, drs, d_coded, css, crs);
    const unsigned nb = static_cast<unsigned>(rows * chunks);
    switch (FP) {
    case 1: fp_launch<1>(vec, nb, a, keys, st); break;
    case 2: fp_launch<2>(vec, nb, a, keys, st); break;
    case 4: fp_launch<4>(vec, nb, a, keys, st); break;
    default: fp_launch<8>(vec, nb, a, keys, st); break;
    }
    if (chunks > 1) {
        const long long n = rows * F;
        hipLaunchKernelGGL(fingerprint_finish_kernel,
                           dim3(static_cast<unsigned>((n + kFpBlock - 1) / kFpBlock)),
                           dim3(kFpBlock), 0, st, a, FP, n);
    }
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
