// HIP kernels for RS-FNT over GF(65537) on CDNA4 (gfx950).
//
// Layout: every fragment row is a contiguous run of u16 symbols ("words");
// a stripe is the set of rows sharing a column index range.  One lane owns
// COLS adjacent columns of one stripe, so every global access of a wave is a
// contiguous 64*COLS*2-byte segment of one row (coalesced), and every column
// -- an independent RS codeword read "vertically" across the fragments
// (src/fec_base.h:1103-1150) -- is transformed entirely in VGPRs.
//
// Addressing: a stripe's rows are reached through a buffer resource (SGPR
// base + 32-bit extent) with the row offset in an SGPR (soffset) and the
// column offset in one VGPR (voffset), so no per-lane 64-bit address math is
// spent per load/store.  Stripes whose extent does not fit 32 bits use the
// BUF=false instantiation (flat global addressing).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>

#include "fnt_codelets.h"
#include "gf65537.h"
#include "matrix_pack.h"
#include "qi_internal.h"


namespace qi {

constexpr int kBlock = 256;

__device__ __forceinline__ void record_oor(const Oor& o, int s, int slot,
                                           long long col)
{
    const uint32_t e =
        atomicAdd(&o.counts[static_cast<long long>(s) * o.slots + slot], 1u);
    if (e < static_cast<uint32_t>(o.cap))
        o.entries[(static_cast<long long>(s) * o.slots + slot) * o.cap + e] =
            static_cast<uint32_t>(col);
}

// T-range value -> stored u16: 65536 and its alias -1 are stored as 0 (the
// truncation of vec::unpack src/vec_cast.h:133-163).
__device__ __forceinline__ uint32_t fix16(int32_t y)
{
    return static_cast<uint32_t>(y) > 65535u ? 0u : static_cast<uint32_t>(y);
}

// canonical residue of a V-range value [-2, 65537]
__device__ __forceinline__ uint32_t canon_v(int32_t y)
{
    const int32_t c = y < 0 ? y + 65537 : y;
    return static_cast<uint32_t>(c >= 65537 ? c - 65537 : c);
}

constexpr long long kTwLo = -32767, kTwHi = 98303;
static_assert(fold_rng(join(mul_rng(Rng{0, 65535}, 32768),
                            mul_rng(Rng{0, 65535}, -32768))).lo == kTwLo &&
                  fold_rng(join(mul_rng(Rng{0, 65535}, 32768),
                                mul_rng(Rng{0, 65535}, -32768))).hi == kTwHi,
              "twist output range");

// x * c for a T-range x and a balanced row scale |c| <= 32766 as ONE
// v_mul_i32_i24 (written out: the compiler cannot see that the lazily
// reduced x fits 24 bits and emitted the quarter-rate v_mul_lo_u32)
__device__ __forceinline__ int32_t mul_rs(int32_t x, int32_t c)
{
    int32_t r;
    asm("v_mul_i32_i24 %0, %1, %2" : "=v"(r) : "v"(x), "v"(c));
    return r;
}

// pack the low halves of two dwords: [a.lo, b.lo] (one v_perm_b32)
__device__ __forceinline__ uint32_t pack_lo(uint32_t a, uint32_t b)
{
    return __builtin_amdgcn_perm(b, a, 0x05040100u);
}

// A stripe region: buffer resource (BUF) or flat base pointer.
template <bool BUF>
struct Region {
    __amdgpu_buffer_rsrc_t r;
    char* p;
    __device__ __forceinline__ Region(const void* base, uint32_t bytes)
    {
        p = static_cast<char*>(const_cast<void*>(base));
        if constexpr (BUF)
            r = __builtin_amdgcn_make_buffer_rsrc(p, static_cast<short>(0),
                                                  static_cast<int>(bytes),
                                                  0x00020000);
    }
};

// Byte offset of a row inside its stripe region (wave-uniform): 32 bits as
// a buffer op's soffset, 64 bits on the flat path, whose regions are the ones
// that do not fit a 31-bit range (rows of a fragment-major layout lie GiB
// apart)
template <bool BUF>
using roff_t = std::conditional_t<BUF, uint32_t, uint64_t>;
// a row stride in bytes from its halves (the buffer forms take the low one)
template <bool BUF>
__device__ __forceinline__ roff_t<BUF> row_stride(uint32_t lo, uint32_t hi)
{
    if constexpr (BUF)
        return lo;
    else
        return static_cast<uint64_t>(hi) << 32 | lo;
}

// Cache policy of the streamed rows (buffer-op aux bits on gfx950: 1 = sc0,
// 2 = nt, 16 = sc1).  Measured with tools/membw2.hip / membw3.hip on the
// kernels' own shapes (profiles/r1_membw.txt): nt|sc1 stores (device scope,
// written through the XCD's L2) +5 % on both the encode shape (16 rows in,
// 64 out) and the decode shape (16 of 64 rows in, 16 out); nt loads +5 % on
// the decode shape, but slow the encode shape down (its inputs stay plain).
// The matrix-core kernel's whole-line output stores keep nt|sc1 as well:
// default, nt and sc1 alone measured 1-7 % slower
// (profiles/r1_ab_mfma_store_policy.txt).
constexpr int kAuxLd = 2;
constexpr int kAuxSt = 18;
constexpr int kAuxStMf = 18;
// matrix_os_kernel's row loads: default policy (its G row-block groups read
// the same tiles through their XCD's L2; nt measured the same at k200 /
// k256 / cfg3, gpurun_out ab_aux)
constexpr int kAuxLdOs = 0;

// XCD-aware block -> (stripe, tile) map.  Workgroups are dispatched
// round-robin over the 8 XCDs (block b runs on XCD b % 8), so with the plain
// stripe-major order the 8 adjacent tiles of one stripe land on 8 different
// XCDs.  Instead, each group of 8 consecutive stripes is split so that XCD x
// walks all tiles of stripe 8g + x: +4-6 % HBM throughput on both kernel
// shapes (membw3 "ord3").  A trailing partial group (S % 8 stripes) keeps
// the stripe-major order.
__device__ __forceinline__ void block_map(int b, int tiles, int& s, int& tile)
{
    const int n_stripes = static_cast<int>(gridDim.x) / tiles;
    const int grouped = (n_stripes & ~7) * tiles;  // blocks in full groups
    if (b < grouped) {
        const int j = b >> 3;
        const int g = j / tiles;
        s = g * 8 + (b & 7);
        tile = j - g * tiles;
        return;
    }
    s = b / tiles;
    tile = b - s * tiles;
}

// NDW (1 or 2) dwords per lane of the row at byte offset `row`
template <int NDW, bool BUF, int AUX = 0>
__device__ __forceinline__ void ld_dw(const Region<BUF>& g, roff_t<BUF> row,
                                      uint32_t voff, uint32_t (&w)[NDW])
{
    static_assert(NDW == 1 || NDW == 2, "dword count");
    if constexpr (NDW == 1) {
        if constexpr (BUF)
            w[0] = __builtin_amdgcn_raw_buffer_load_b32(
                g.r, static_cast<int>(voff), static_cast<int>(row), AUX);
        else
            w[0] = *reinterpret_cast<const uint32_t*>(g.p + row + voff);
    } else {
        if constexpr (BUF) {
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(
                g.r, static_cast<int>(voff), static_cast<int>(row), AUX);
            w[0] = v[0];
            w[1] = v[1];
        } else {
            const uint2 v = *reinterpret_cast<const uint2*>(g.p + row + voff);
            w[0] = v.x;
            w[1] = v.y;
        }
    }
}

template <int NDW, bool BUF, int AUX = 0>
__device__ __forceinline__ void st_dw(const Region<BUF>& g, roff_t<BUF> row,
                                      uint32_t voff, const uint32_t (&w)[NDW])
{
    static_assert(NDW == 1 || NDW == 2, "dword count");
    if constexpr (NDW == 1) {
        if constexpr (BUF)
            __builtin_amdgcn_raw_buffer_store_b32(w[0], g.r, static_cast<int>(voff),
                                                  static_cast<int>(row), AUX);
        else
            *reinterpret_cast<uint32_t*>(g.p + row + voff) = w[0];
    } else {
        if constexpr (BUF) {
            typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
            u32x2 v;
            v[0] = w[0];
            v[1] = w[1];
            __builtin_amdgcn_raw_buffer_store_b64(v, g.r, static_cast<int>(voff),
                                                  static_cast<int>(row), AUX);
        } else {
            *reinterpret_cast<uint2*>(g.p + row + voff) = make_uint2(w[0], w[1]);
        }
    }
}

// COLS adjacent u16 columns of the row at byte offset `row` (wave-uniform).
// FULL: COLS/2 dwords per lane (COLS 2 or 4); otherwise one u16 per column
// and columns past `avail` are 0.
template <int COLS, bool FULL, bool BUF, int AUX = 0>
__device__ __forceinline__ void ld(const Region<BUF>& g, roff_t<BUF> row,
                                   uint32_t voff, long long avail, int32_t* v)
{
    if constexpr (FULL && COLS % 2 == 0) {
        uint32_t w[COLS / 2];
        ld_dw<COLS / 2, BUF, AUX>(g, row, voff, w);
#pragma unroll
        for (int d = 0; d < COLS / 2; d++) {
            v[2 * d] = w[d] & 0xffff;
            v[2 * d + 1] = w[d] >> 16;
        }
    } else {
#pragma unroll
        for (int c = 0; c < COLS; c++) {
            if (FULL || c < avail) {
                if constexpr (BUF)
                    v[c] = __builtin_amdgcn_raw_buffer_load_b16(
                        g.r, static_cast<int>(voff + 2 * c),
                        static_cast<int>(row), AUX);
                else
                    v[c] = *reinterpret_cast<const uint16_t*>(g.p + row + voff +
                                                              2 * c);
            } else {
                v[c] = 0;
            }
        }
    }
}

template <int COLS, bool FULL, bool BUF, int AUX = 0>
__device__ __forceinline__ void st(const Region<BUF>& g, roff_t<BUF> row,
                                   uint32_t voff, long long avail,
                                   const uint32_t* v)
{
    if constexpr (FULL && COLS % 2 == 0) {
        uint32_t w[COLS / 2];
#pragma unroll
        for (int d = 0; d < COLS / 2; d++)
            w[d] = pack_lo(v[2 * d], v[2 * d + 1]);
        st_dw<COLS / 2, BUF, AUX>(g, row, voff, w);
    } else {
#pragma unroll
        for (int c = 0; c < COLS; c++) {
            if (FULL || c < avail) {
                if constexpr (BUF)
                    __builtin_amdgcn_raw_buffer_store_b16(
                        static_cast<uint16_t>(v[c]), g.r,
                        static_cast<int>(voff + 2 * c), static_cast<int>(row), AUX);
                else
                    *reinterpret_cast<uint16_t*>(g.p + row + voff + 2 * c) =
                        static_cast<uint16_t>(v[c]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Non-systematic encode (src/fec_rs_fnt.h:236-251 NON_SYSTEMATIC branch ==
// Radix2::fft of the zero-padded column, src/fft_2n.h:360-407).
//
// The n-point transform of a column with K = ceil2(k) live inputs is split
// into n/K twisted K-point transforms:
//     out[(n/K) u + v] = sum_{t<K} (d_t w^{vt}) wK^{ut}
// so a lane keeps only 2K values per column live, and pass v writes the K
// output rows {(n/K)u + v}.  All loads of a lane are issued back to back
// (branch-free), outputs are stored as soon as a pass is done, and the rare
// out-of-range outputs (value 65536, src/fec_rs_fnt.h:253-269) are found by
// one OR-reduction per pass and fixed up off the fast path.
// KEQ: k == K (no zero-padded inputs to mask).
// ---------------------------------------------------------------------------
// cfg2 encode passes in store-interleaved pairs (3.675 -> 3.627 ms)
static constexpr bool kEncPair = true;

template <int K, int COLS, bool FULL, bool KEQ, bool BUF>
__device__ __forceinline__ void encode_body(
    int k, int n, int n_out, const int32_t* __restrict__ twist,
    const Region<BUF>& gi, roff_t<BUF> irs, const Region<BUF>& go, roff_t<BUF> ors,
    uint32_t voff, long long col, long long avail, int s, const Oor& oor)
{
    // RELOAD (K = 32): re-read the K input rows every pass (L2 hits after
    // the first) instead of keeping them live next to the pass's outputs:
    // 141 -> 105 VGPRs, 3 -> 4 waves/SIMD.  K = 64 stays resident (its DFT64
    // codelet alone needs ~180 VGPRs, so reloading gains no occupancy).
    // Holding two passes to interleave their stores (the 64 KiB address bit
    // alternating, +7 % on the bare store pattern) measured 3 % slower on
    // the real kernel (16 more VGPRs + unpacks), so passes store alone.
    constexpr bool RELOAD = K == 32;
    const int passes = n / K;

    constexpr bool PAIR_ = kEncPair && K == 16 && COLS == 2 && FULL;
    int32_t x[COLS][K];
    auto load_x = [&](uint32_t vo) {
#pragma unroll
        for (int t = 0; t < K; t++) {
            const int row = KEQ ? t : (t < k ? t : k - 1);  // clamp, then mask
            int32_t v[COLS];
            ld<COLS, FULL, BUF>(gi, static_cast<roff_t<BUF>>(row) * irs, vo, avail, v);
#pragma unroll
            for (int c = 0; c < COLS; c++)
                x[c][t] = (KEQ || t < k) ? v[c] : 0;
        }
    };
    if constexpr (!RELOAD && !PAIR_)
        load_x(voff);

    // pass v: y[c][u] = output row passes*u + v of column c, in V = [-2, 65537]
    auto compute = [&](int v, int32_t (&y)[COLS][K]) {
        if constexpr (RELOAD) {
            uint32_t vo = voff;
            asm volatile("" : "+v"(vo));  // keep the loads inside the loop
            load_x(vo);
        }
        if (v == 0) {
#pragma unroll
            for (int c = 0; c < COLS; c++) {
#pragma unroll
                for (int t = 0; t < K; t++)
                    y[c][t] = x[c][t];
                dft<K, 0, 65535>(y[c]);
            }
        } else {
            // twist by w^{vt}: |x*c| < 2^31 for x < 2^16, |c| <= 2^15, and
            // one fold leaves [-32767, 98303] (kTwLo/kTwHi), which the
            // codelet plan accepts as its input range
            const int32_t* tw = twist + v * K;
#pragma unroll
            for (int t = 0; t < K; t++) {
                const int32_t cb = tw[t];
#pragma unroll
                for (int c = 0; c < COLS; c++)
                    y[c][t] = t == 0 ? x[c][t] : fold(mul_i24_s(x[c][t], cb));
            }
#pragma unroll
            for (int c = 0; c < COLS; c++)
                dft<K, kTwLo, kTwHi>(y[c]);
        }
    };
    // the stored word is the low 16 bits; any output outside [0, 65535] (the
    // true OOR symbol 65536 or a non-canonical alias) sends the pass through
    // the rare fix-up: canonicalise in place, then record the OOR marks from
    // a bitmask (keeps the atomics out of the unrolled code)
    // The wave takes the fix-up when any of its lanes has such an output
    // (about 64 x 2K x 4 / 65537 = 12 % of the passes at K = 16), so the
    // fix-up is per element and wave-uniform: one compare + ballot per
    // output, and only the elements some lane has out of range are
    // canonicalised (the earlier whole-pass canonicalisation with a 64-bit
    // mark mask cost ~400 instructions per taken pass)
    auto fixup = [&](int v, int32_t (&y)[COLS][K]) {
        uint32_t bad = 0;
#pragma unroll
        for (int u = 0; u < K; u++)
#pragma unroll
            for (int c = 0; c < COLS; c++)
                bad |= static_cast<uint32_t>(y[c][u]);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64((bad >> 16) != 0) != 0, 0)) {
#pragma unroll
            for (int u = 0; u < K; u++) {
#pragma unroll
                for (int c = 0; c < COLS; c++) {
                    if (__builtin_amdgcn_ballot_w64(static_cast<uint32_t>(y[c][u]) > 65535u)) {
                        const uint32_t cv = canon_v(y[c][u]);
                        y[c][u] = static_cast<int32_t>(cv & 0xffffu);
                        const int row = passes * u + v;
                        if (cv == 65536u && oor.counts && (FULL || c < avail) && row < n_out)
                            record_oor(oor, s, row, col + c);
                    }
                }
            }
        }
    };
    // CHK: some rows >= n_out are not wanted (uniform per launch; the
    // checks become a scalar branch around every store, so the common
    // all-rows case gets its own branch-free copy)
    auto run = [&](auto chk) {
        for (int v = 0; v < passes; v++) {
            int32_t y[COLS][K];
            compute(v, y);
            fixup(v, y);
#pragma unroll
            for (int u = 0; u < K; u++) {
                const int row = passes * u + v;
                uint32_t o[COLS];
#pragma unroll
                for (int c = 0; c < COLS; c++)
                    o[c] = static_cast<uint32_t>(y[c][u]);
                if (!decltype(chk)::value || row < n_out)
                    st<COLS, FULL, BUF, kAuxSt>(go, static_cast<roff_t<BUF>>(row) * ors,
                                                voff, avail, o);
            }
        }
    };
    // PAIR (K = 16, 2 columns per lane, whole tiles: the cfg2 shape): the
    // passes run in pairs (v, v + 1) and their stores interleave, rows
    // 4u + v, 4u + v + 1, ..., so consecutive 256-byte row stores of a wave
    // alternate the 64 KiB address bit (the pass-order pattern, all 16 rows
    // of a pass in a row, measured 3.61 ms vs 3.34-3.41 ms for row order /
    // pass pairs on the bare store pattern, profiles/r1_membw3.txt,
    // r3_membw4.txt).  The even pass is held packed (16 VGPRs); the inputs
    // stay packed too (16 VGPRs instead of 32: the twist multiplies read a
    // column's 16-bit half with SDWA), so the kernel keeps 4 waves per SIMD.
    auto run_pairs = [&](auto chk) {
        uint32_t xw[K];
#pragma unroll
        for (int t = 0; t < K; t++) {
            const int row = KEQ ? t : (t < k ? t : k - 1);
            uint32_t w[1];
            ld_dw<1, BUF>(gi, static_cast<roff_t<BUF>>(row) * irs, voff, w);
            xw[t] = (KEQ || t < k) ? w[0] : 0u;
        }
        auto compute_p = [&](int v, int32_t (&y)[COLS][K]) {
#pragma unroll
            for (int t = 0; t < K; t++) {
                y[0][t] = static_cast<int32_t>(xw[t] & 0xffffu);
                y[1][t] = static_cast<int32_t>(xw[t] >> 16);
            }
            if (v == 0) {
#pragma unroll
                for (int c = 0; c < COLS; c++)
                    dft<K, 0, 65535>(y[c]);
            } else {
                const int32_t* tw = twist + v * K;
#pragma unroll
                for (int t = 1; t < K; t++) {
                    const int32_t cb = tw[t];
                    y[0][t] = fold(mul_i24_lo16(xw[t], cb));
                    y[1][t] = fold(mul_i24_hi16(xw[t], cb));
                }
#pragma unroll
                for (int c = 0; c < COLS; c++)
                    dft<K, kTwLo, kTwHi>(y[c]);
            }
        };
        auto packed = [&](int v, uint32_t (&o)[K]) {
            int32_t y[COLS][K];
            compute_p(v, y);
            fixup(v, y);
#pragma unroll
            for (int u = 0; u < K; u++)
                o[u] = pack_lo(static_cast<uint32_t>(y[0][u]), static_cast<uint32_t>(y[1][u]));
        };
        auto store = [&](int row, uint32_t o) {
            if (!decltype(chk)::value || row < n_out) {
                const uint32_t w[1] = {o};
                st_dw<1, BUF, kAuxSt>(go, static_cast<roff_t<BUF>>(row) * ors, voff, w);
            }
        };
        int v = 0;
        for (; v + 1 < passes; v += 2) {
            uint32_t o0[K], o1[K];
            packed(v, o0);
            packed(v + 1, o1);
#pragma unroll
            for (int u = 0; u < K; u++) {
                store(passes * u + v, o0[u]);
                store(passes * u + v + 1, o1[u]);
            }
        }
        if (v < passes) {
            uint32_t o0[K];
            packed(v, o0);
#pragma unroll
            for (int u = 0; u < K; u++)
                store(passes * u + v, o0[u]);
        }
    };
    constexpr bool PAIR = kEncPair && K == 16 && COLS == 2 && FULL;
    if constexpr (PAIR) {
        if (n_out >= n)
            run_pairs(std::integral_constant<bool, false>{});
        else
            run_pairs(std::integral_constant<bool, true>{});
    } else {
        if (n_out >= n)
            run(std::integral_constant<bool, false>{});
        else
            run(std::integral_constant<bool, true>{});
    }
}

template <int K, int COLS, bool KEQ, bool BUF>
// 4 waves per SIMD: the K=16, COLS=2 body fits 128 VGPRs without spills or
// extra instructions (3 waves at the compiler's default 130).  K = 64: 2
// waves (3 waves = 168 VGPRs spilled and ran 20 % slower,
// profiles/r1_ab_k64_encode.txt)
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(K >= 64 ? 2 : 4))) void
encode_fnt_kernel(
    int k, int n, int n_out, const int32_t* __restrict__ twist,
    const uint16_t* __restrict__ data, long long dss, uint32_t irs,
    uint32_t iext, uint16_t* __restrict__ out, long long oss, uint32_t ors,
    uint32_t oext, long long words, int tiles, Oor oor)
{
    int s, tile;
    block_map(blockIdx.x, tiles, s, tile);
    const long long col0 = static_cast<long long>(tile) * kBlock * COLS;
    const long long col = col0 + static_cast<long long>(threadIdx.x) * COLS;
    const Region<BUF> gi(data + s * dss, iext);
    const Region<BUF> go(out + s * oss, oext);
    // the flat form has no extents: iext / oext carry the upper halves of its
    // row strides (enc_launch), and the signature stays that of the buffer
    // forms
    const roff_t<BUF> irs_ = row_stride<BUF>(irs, iext), ors_ = row_stride<BUF>(ors, oext);
    const uint32_t voff = static_cast<uint32_t>(col * 2);
    if (col0 + kBlock * COLS <= words) {  // block-uniform
        encode_body<K, COLS, true, KEQ, BUF>(k, n, n_out, twist, gi, irs_, go,
                                             ors_, voff, col, COLS, s, oor);
    } else {
        if (col >= words)
            return;
        encode_body<K, COLS, false, KEQ, BUF>(k, n, n_out, twist, gi, irs_, go,
                                              ors_, voff, col, words - col, s,
                                              oor);
    }
}

// ---------------------------------------------------------------------------
// Matrix apply: out[t] = sum_i M[t][i] * in[i] over GF(65537) with
// v_dot2_i32_i16 (two 16x16 products + accumulate per instruction).
// Used for decode (M = interpolation matrix of the received ids: the linear
// map computed by FecCode::decode_apply, src/fec_base.h:1418-1448, restated
// as one k x k product), systematic decode and systematic encode.
// ---------------------------------------------------------------------------
constexpr int kMaxTileOor = 256;
typedef short qi_short2 __attribute__((ext_vector_type(2)));

// launch geometry of a matrix kernel: byte extents of the stripe regions it
// touches and its first column (a tail launch starts past the columns the
// matrix-core kernel covered)
struct MatExt {
    uint32_t e0, e1, eo;
    long long c0;
};

// everything a matrix launch needs (one kernel argument block)
struct MatArgs {
    MatLayout L;
    const int32_t* mat;  // per-stripe matrix blocks, ms words apart (0: shared)
    long long ms;
    const int32_t* ids;  // per-stripe int32 ids, is apart (nullptr: identity)
    long long is;
    RowSrc src;
    RowDst dst;
    MatExt ext;
    long long words;
    int tiles;
    Oor in_oor;  // input marks (counts nullptr: none)
    int slot_base;
    Oor out_oor;  // output marks recorded (counts nullptr: none)
    // output row of matrix row t (the plan groups a shared generator's
    // row-scaled rows into as few 16-row blocks as possible); identity for
    // decode matrices
    const int32_t* rowmap;
    const uint32_t* route;
    long long rstride;
    SlowList slow;
    uint32_t* err;
};

// The forms a matrix kernel's body file is compiled in (MODE, a constexpr
// set by the including kernel): plain; input and output marks in one launch
// (a repair); and the verify form of a fused check, which is the repair with
// the row store replaced by a load of the stored row and a compare.
enum class MatMode { kPlain, kBoth, kVerify };

// What the verify forms add to a launch (the other forms get an empty one):
// chk[s * R + t] is the fragment id of matrix row t, whose stored row lies in
// the launch's source regions; value mismatches are counted in vmis[s * R +
// t] and the smallest mismatching column goes to first[s * R + t].  The
// recomputed rows' 65536 positions go to the launch's output buckets.
struct VerArgs {
    const uint16_t* chk = nullptr;
    uint32_t* vmis = nullptr;
    uint32_t* first = nullptr;
};

// One row's mismatches of a wave into its counters, by one lane: `mis` is
// this lane's column (lane order = column order), col its column
__device__ __forceinline__ void verify_report_lanes(const VerArgs& v, long long idx, bool mis,
                                                    uint32_t col)
{
    const uint64_t m = __builtin_amdgcn_ballot_w64(mis);
    if (mis && static_cast<int>(threadIdx.x & 63) == __builtin_ctzll(m)) {
        atomicAdd(v.vmis + idx, static_cast<uint32_t>(__builtin_popcountll(m)));
        atomicMin(v.first + idx, col);
    }
}

// Where the OOR marks of the received rows (decode_prepare's restore of
// 65536, src/fec_base.h:1361-1404) come from in a matrix launch.  A tile
// normally takes them from the context's route table or from one scan of
// the buckets into LDS (kMaxTileOor entries); a tile holding more marks
// than that (adversarial data) sets `slow` and every epilogue walks the
// buckets directly -- slower, but with no limit, as the reference has none.
struct OorScan {
    Oor in;
    const int32_t* sid;  // per-stripe ids (nullptr = identity)
    int by_pos, slot_base, kin, s;
    bool slow;
};

// A tile with more than kMaxTileOor marks (adversarial data; the reference
// has no such limit): the matrix kernels applied only the first
// kMaxTileOor of them and appended the tile to its stripe's slow list (in
// the decode context); matrix_redo_kernel, launched right after them on the
// same stream, recomputes every column of the tile that holds a mark from
// scratch -- all marks of the column restored, plain canonical arithmetic
// -- and stores it again.  A decode's outputs are data symbols (< 65536):
// nothing to record.  A repair carries input marks and records output marks
// in the same launch (the BOTH instantiations, chosen by the launchers when
// both kinds of bucket are given): there the first pass records nothing in
// a slow tile -- its outputs came from partly restored inputs -- and the
// redo recomputes every column of the tile, marked or not, and records each
// output equal to 65536 exactly once.  The other instantiations compile to
// what they were before BOTH existed.
// Keeping this out of the hot kernels keeps their registers: inlined at
// their end it held the bucket and row pointers live across the MFMA loop
// (SGPR spills, 2x slower decode).
__device__ __forceinline__ void push_slow_tile(const SlowList& sl, int s, long long col0,
                                               int width)
{
    // width: a power-of-two multiple of kSlowGrain (64 .. 1024 columns)
    uint32_t* l = sl.base + s * sl.stride;
    const uint32_t idx = atomicAdd(l, 1u);
    l[1 + idx] = static_cast<uint32_t>(col0 / kSlowGrain) << 3 |
                 static_cast<uint32_t>(ilog2c(static_cast<uint32_t>(width / kSlowGrain)));
}

// One block per stripe at a time; a slow tile is redone in chunks of
// kRedoCols columns: the chunk's received symbols (u16) and a bitmap of
// their marks staged in LDS (every mark of every received row, from the
// buckets), then lane c of wave wv recomputes column c for the output rows
// wv, wv + 4, ... (the coefficient, read back from the operand tiles by
// mf_entry, is wave-uniform: scalar loads) -- only in columns that hold a
// mark (BOTH: in every column of the tile).  Work per chunk is at most
// R * kin * 64 multiply-adds whatever the mark density (walking the marks
// per (mark, row, input) was quadratic in the density).  The stripe's list
// is emptied afterwards (a context can serve several decodes).
constexpr int kRedoCols = 64;

// Recompute, from scratch, every column of stripe s's columns [t0c, t1c)
// that holds a mark -- BOTH: every column of the range, and record its
// outputs equal to 65536 in a.out_oor -- (all marks of the column restored,
// plain canonical arithmetic) and store it again: NT threads, LDS scratch xs (kin x
// kRedoCols u16), mk (kin x kRedoCols / 32 u32), colmk (kRedoCols / 32 u32).
// The caller has waited for its own stores of these columns.  Only the
// output rows of row blocks gq, gq + G, gq + 2G, ... (16 rows each) are
// recomputed: a block of matrix_os_kernel redoes just the rows it stored
// itself (G row-block groups share a column range), so no two blocks write
// the same outputs; other callers pass gq = 0, G = 1 (every row).
// The verify form compares instead of storing: the stored row of matrix row
// t is fragment v.chk[s * R + t], in the source regions.
template <int NT, MatMode MODE = MatMode::kPlain>
__device__ void redo_columns(const MatArgs& a, int s, long long t0c, long long t1c,
                             uint16_t* xs, uint32_t* mk, uint32_t* colmk, int gq = 0,
                             int G = 1, const VerArgs& v = VerArgs{})
{
    constexpr bool BOTH = MODE != MatMode::kPlain, VERIFY = MODE == MatMode::kVerify;
    const MatLayout L = a.L;
    const int kin = L.kin;
    const RowSrc& src = a.src;
    const RowDst& dst = a.dst;
    const Oor& in = a.in_oor;
    const int tid = threadIdx.x, c = tid & 63, wv = tid >> 6;
    const int32_t* M = a.mat + s * a.ms;
    const int32_t* sid = a.ids ? a.ids + s * a.is : nullptr;
    const int32_t* rscale = M + L.rscale();
    const int32_t* mf = M + L.mf();
    auto id_of = [&](int i) { return src.by_pos ? i : (sid ? sid[i] : i); };
    for (long long c0 = t0c; c0 < t1c; c0 += kRedoCols) {
        for (int j = tid; j < kin * (kRedoCols / 32); j += NT)
            mk[j] = 0;
        if (tid < kRedoCols / 32)
            colmk[tid] = 0;
        // the chunk's received symbols, one row of 64 per wave pass
        for (int i = wv; i < kin; i += NT / 64) {
            const int id = id_of(i);
            const uint16_t* row = id < src.split
                                      ? src.base0 + s * src.ss0 + id * src.rs0
                                      : src.base1 + s * src.ss1 + (id - src.split) * src.rs1;
            xs[i * kRedoCols + c] = c0 + c < t1c ? row[c0 + c] : 0;
        }
        __syncthreads();
        // every mark of every received row inside the chunk
        for (int i = tid; i < kin; i += NT) {
            const int slot = (src.by_pos ? i : id_of(i)) - a.slot_base;
            if (slot < 0)
                continue;  // systematic data row: no marks
            const long long bk = static_cast<long long>(s) * in.slots + slot;
            const uint32_t cnt = min(in.counts[bk], static_cast<uint32_t>(in.cap));
            for (uint32_t f = 0; f < cnt; f++) {
                const long long w = in.entries[bk * in.cap + f];
                if (w >= c0 && w < c0 + kRedoCols && w < t1c) {
                    const int cc = static_cast<int>(w - c0);
                    atomicOr(&mk[i * (kRedoCols / 32) + cc / 32], 1u << (cc % 32));
                    atomicOr(&colmk[cc / 32], 1u << (cc % 32));
                }
            }
        }
        __syncthreads();
        bool redo = (colmk[c / 32] >> (c % 32)) & 1u;
        if constexpr (BOTH)
            redo = redo || c0 + c < t1c;
        if (redo) {
            const int nrows = 16 * ((L.RB() - gq + G - 1) / G);
            for (int it = wv; it < nrows; it += NT / 64) {
                const int t = 16 * (gq + G * (it >> 4)) + (it & 15);
                if (t >= L.R)
                    continue;
                uint64_t acc = 0;
                for (int j = 0; j < kin; j++) {
                    const uint32_t x = (mk[j * (kRedoCols / 32) + c / 32] >> (c % 32)) & 1u
                                           ? 65536u
                                           : xs[j * kRedoCols + c];
                    acc += static_cast<uint64_t>(mf_entry(L, mf, t, j)) * x;
                }
                uint32_t y = static_cast<uint32_t>(acc % 65537u);
                const int32_t rs = rscale[t];
                if (rs != 1)
                    y = static_cast<uint32_t>(static_cast<uint64_t>(y) *
                                              static_cast<uint32_t>(rs < 0 ? rs + kQ : rs) %
                                              65537u);
                if constexpr (VERIFY) {
                    const int id = min(static_cast<int>(v.chk[static_cast<long long>(s) * L.R + t]),
                                       src.rows0 + src.rows1 - 1);
                    const uint16_t* row =
                        id < src.split ? src.base0 + s * src.ss0 + id * src.rs0
                                       : src.base1 + s * src.ss1 + (id - src.split) * src.rs1;
                    verify_report_lanes(v, static_cast<long long>(s) * L.R + t,
                                        (y == 65536u ? 0u : y) != row[c0 + c],
                                        static_cast<uint32_t>(c0 + c));
                } else {
                    dst.base[s * dst.ss + a.rowmap[t] * dst.rs + c0 + c] =
                        static_cast<uint16_t>(y == 65536u ? 0u : y);
                }
                if constexpr (BOTH)
                    if (y == 65536u)
                        record_oor(a.out_oor, s, a.rowmap[t], c0 + c);
            }
        }
        __syncthreads();
    }
}

// A block's slow tiles (see push_slow_tile), redone by the block itself at
// its end, after its waves' stores: the separate redo launch cost 4-5 us per
// decode even with nothing to redo.  Waits for this wave's outstanding
// memory operations (stores included), then the block barrier.
__device__ __forceinline__ void drain_block_stores()
{
    __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) expcnt(0) lgkmcnt(0)
    __syncthreads();
}

// The dot2 kernel's slow tiles (column tails, unaligned rows): kept in the
// context's slow list and redone by this launch after it.  A block checks
// the lists of kRedoSpan stripes at once (one lane each) and walks only the
// stripes holding slow tiles.
constexpr int kRedoSpan = 64;


__global__ __launch_bounds__(kBlock) void matrix_redo_kernel(MatArgs a, int n_stripes)
{
    constexpr MatMode MODE = MatMode::kPlain;
    constexpr VerArgs v{};
#include "matrix_redo_body.h"
}
// input and output marks in one launch (a repair)
__global__ __launch_bounds__(kBlock) void matrix_redo_kernel_both(MatArgs a, int n_stripes)
{
    constexpr MatMode MODE = MatMode::kBoth;
    constexpr VerArgs v{};
#include "matrix_redo_body.h"
}
// a fused check: the slow tiles compared with the stored rows, counted once
__global__ __launch_bounds__(kBlock) void matrix_redo_kernel_verify(MatArgs a, int n_stripes,
                                                                    VerArgs v)
{
    constexpr MatMode MODE = MatMode::kVerify;
#include "matrix_redo_body.h"
}

// the context's routed marks of this tile (count <= kRouteCap, entries
// pos << 16 | column in the kRouteTile tile) into the LDS list (s_i, s_col)
__device__ __forceinline__ void stage_route_marks(const uint32_t* rm, int n_rm,
                                                  long long col0, int* s_i,
                                                  uint32_t* s_col)
{
    if (static_cast<int>(threadIdx.x) < n_rm) {
        const uint32_t v = rm[threadIdx.x];
        s_i[threadIdx.x] = static_cast<int>(v >> 16);
        s_col[threadIdx.x] =
            static_cast<uint32_t>(col0 / kRouteTile * kRouteTile + (v & 0xffffu));
    }
}

// The same from the route-table entry rt (count + kRouteCap entries), the
// count by a scalar load (constant address space).  VEC: the entries by the
// lanes that stage one, with a vector load; otherwise all 16 dwords by
// scalar loads (round 5: a vector load is ordered with the kernel's
// streaming stores and row prefetch in vmcnt, and waiting for it drained
// both every tile).  The callers stage a route tile's list once per mark
// buffer, and only wave 0 issues the vector load; the 16 SGPRs of the
// scalar form had pushed the KS = 4 kernel to ~75 SGPR spills (VEC there:
// cfg3 decode -2 us, k200 / k300 -1 %; at KS = 8 the scalar form measured
// 1.5 % faster, k128).  Returns the count, or -1 when the tile overflowed
// the table (scan the buckets).
template <bool VEC>
__device__ __forceinline__ int stage_route_marks_s(const uint32_t* rt, long long col0, int* s_i,
                                                   uint32_t* s_col)
{
    using CU = const __attribute__((address_space(4))) uint32_t;
    CU* c = (CU*)rt;
    if constexpr (!VEC) {
        uint32_t e[kRouteStride];
#pragma unroll
        for (int i = 0; i < kRouteStride; i++)
            e[i] = c[i];
        const uint32_t rc = e[0];
        if (rc > static_cast<uint32_t>(kRouteCap))
            return -1;
        const int tid = static_cast<int>(threadIdx.x);
        if (tid < static_cast<int>(rc)) {
            uint32_t v = 0;
#pragma unroll
            for (int i = 0; i < kRouteCap; i++)
                v = tid == i ? e[1 + i] : v;
            s_i[tid] = static_cast<int>(v >> 16);
            s_col[tid] = static_cast<uint32_t>(col0 / kRouteTile * kRouteTile + (v & 0xffffu));
        }
        return static_cast<int>(rc);
    }
    const uint32_t rc = c[0];
    if (rc > static_cast<uint32_t>(kRouteCap))
        return -1;
    const int tid = static_cast<int>(threadIdx.x);
    if (tid < static_cast<int>(rc)) {
        const uint32_t v = rt[1 + tid];
        s_i[tid] = static_cast<int>(v >> 16);
        s_col[tid] = static_cast<uint32_t>(col0 / kRouteTile * kRouteTile + (v & 0xffffu));
    }
    return static_cast<int>(rc);
}

// block-wide scan of the buckets into the LDS list (s_i, s_col) of the
// marks inside columns [col0, col1); returns the number of marks found
// (> kMaxTileOor: the list is incomplete, use the slow path)
__device__ __forceinline__ int scan_tile_marks(const OorScan& sc, long long col0,
                                               long long col1, long long words,
                                               int* s_cnt, int* s_i, uint32_t* s_col,
                                               uint32_t* err)
{
    if (threadIdx.x == 0)
        *s_cnt = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < sc.kin; i += blockDim.x) {
        const int id = sc.sid ? sc.sid[i] : i;
        const int slot = (sc.by_pos ? i : id) - sc.slot_base;
        if (slot < 0)
            continue;
        const long long bk = static_cast<long long>(sc.s) * sc.in.slots + slot;
        uint32_t c = sc.in.counts[bk];
        if (c > static_cast<uint32_t>(sc.in.cap)) {
            atomicOr(err, kErrOorTruncated);
            c = static_cast<uint32_t>(sc.in.cap);
        }
        for (uint32_t e = 0; e < c; e++) {
            const uint32_t w = sc.in.entries[bk * sc.in.cap + e];
            if (w >= col0 && w < col1 && w < words) {
                const int p = atomicAdd(s_cnt, 1);
                if (p < kMaxTileOor) {
                    s_i[p] = i;
                    s_col[p] = w;
                }
            }
        }
    }
    __syncthreads();
    return *s_cnt;
}

template <int KP, int COLS, bool FULL, bool BUF, class IdOf>
__device__ __forceinline__ void matrix_load(const IdOf& id_of,
                                            const RowSrc& src,
                                            const Region<BUF>& g0,
                                            const Region<BUF>& g1, uint32_t voff,
                                            long long avail,
                                            int32_t (&xp)[COLS][KP])
{
    // every row pair, branch-free, offset to signed 16 bit (x - 32768) and
    // packed [row 2j, row 2j+1] per column for dot2.  Rows past kin load a
    // valid (clamped) row and need no masking: their packed coefficients are
    // 0 and kcorr sums only the real ones (pack_row).
#pragma unroll
    for (int j = 0; j < KP; j++) {
        Region<BUF> g[2] = {g0, g0};
        roff_t<BUF> off[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int id = id_of(2 * j + h);
            // branch-free source select (uniform s_cselect): a branch here
            // makes the compiler drain vmcnt after every row load
            const bool lo = id < src.split;
            if constexpr (BUF)
                g[h].r = lo ? g0.r : g1.r;
            g[h].p = lo ? g0.p : g1.p;
            off[h] = static_cast<roff_t<BUF>>(lo ? id * src.rs0 * 2
                                              : (id - src.split) * src.rs1 * 2);
        }
        if constexpr (FULL && COLS % 2 == 0) {
            uint32_t w0[COLS / 2], w1[COLS / 2];
            ld_dw<COLS / 2, BUF, kAuxLd>(g[0], off[0], voff, w0);
            ld_dw<COLS / 2, BUF, kAuxLd>(g[1], off[1], voff, w1);
#pragma unroll
            for (int d = 0; d < COLS / 2; d++) {
                xp[2 * d][j] = static_cast<int32_t>(
                    __builtin_amdgcn_perm(w1[d], w0[d], 0x05040100u) ^ 0x80008000u);
                xp[2 * d + 1][j] = static_cast<int32_t>(
                    __builtin_amdgcn_perm(w1[d], w0[d], 0x07060302u) ^ 0x80008000u);
            }
        } else {
            int32_t vv[2][COLS];
            ld<COLS, FULL, BUF, kAuxLd>(g[0], off[0], voff, avail, vv[0]);
            ld<COLS, FULL, BUF, kAuxLd>(g[1], off[1], voff, avail, vv[1]);
#pragma unroll
            for (int c = 0; c < COLS; c++)
                xp[c][j] = static_cast<int32_t>(
                    pack_lo(static_cast<uint32_t>(vv[0][c]),
                            static_cast<uint32_t>(vv[1][c])) ^
                    0x80008000u);
        }
    }
}

template <int KP, int COLS, bool FULL, bool BUF>
__device__ __forceinline__ void matrix_compute(
    const MatLayout& L, const int32_t* __restrict__ M,
    const int32_t (&xp)[COLS][KP], const Region<BUF>& go, roff_t<BUF> ors,
    uint32_t voff, long long col, long long col0, long long avail, int s,
    int n_lm, const int* s_i, const uint32_t* s_col, const Oor& out_oor,
    const int32_t* __restrict__ rowmap)
{
    // M: the per-stripe matrix block (wave-uniform: scalar loads)
    const int kin = L.kin;
    const int32_t* kcorr = M + L.kcorr();
    const int32_t* rscale = M + L.rscale();
    const int32_t* plain = M + L.plain();
    const bool rec = out_oor.counts != nullptr;
    for (int t = 0; t < L.R; t++) {
        const int32_t* mrow = M + t * KP;
        int32_t acc[COLS];
#pragma unroll
        for (int c = 0; c < COLS; c++)
            acc[c] = kcorr[t];
#pragma unroll
        for (int j = 0; j < KP; j++) {
            const qi_short2 m2 = __builtin_bit_cast(qi_short2, mrow[j]);
#pragma unroll
            for (int c = 0; c < COLS; c++)
                acc[c] = fold(__builtin_amdgcn_sdot2(
                    __builtin_bit_cast(qi_short2, xp[c][j]), m2, acc[c], false));
        }
        int32_t y[COLS];
#pragma unroll
        for (int c = 0; c < COLS; c++)
            y[c] = fold(acc[c]);  // T-range
        // restored OOR symbols: 65536 == -1 where the stored word is 0
        for (int e = 0; e < n_lm; e++) {
            const int pos = s_i[e];
            const long long w = s_col[e];
            // branch-free per lane, unconditional load consumed at once (see
            // the matrix-core epilogue: a load under a divergent branch made
            // the compiler drain vmcnt(0) after every row)
            const long long d = w - col;
            const int32_t corr = plain[t * kin + pos];
#pragma unroll
            for (int c = 0; c < COLS; c++) {
                const int32_t yc = fold(fold(y[c] - corr));
                y[c] = d == c ? yc : y[c];
            }
        }
        const int32_t rs = rscale[t];
        if (rs != 1) {
#pragma unroll
            for (int c = 0; c < COLS; c++)
                y[c] = fold(fold(mul_rs(y[c], rs)));
        }
        uint32_t o[COLS];
        uint32_t bad = 0;
#pragma unroll
        for (int c = 0; c < COLS; c++) {
            o[c] = static_cast<uint32_t>(y[c]);
            bad |= o[c];
        }
        if (__builtin_expect((bad >> 16) != 0, 0)) {
#pragma unroll
            for (int c = 0; c < COLS; c++) {
                if (static_cast<uint32_t>(y[c]) > 65535u && rec &&
                    (FULL || c < avail))
                    record_oor(out_oor, s, rowmap[t], col + c);
                o[c] = fix16(y[c]);
            }
        }
        st<COLS, FULL, BUF, kAuxSt>(go, static_cast<roff_t<BUF>>(rowmap[t]) * ors, voff, avail,
                                    o);
    }
}


// The stored rows a verify form compares with: the launch's source regions
// and its VerArgs; skip: a slow tile (counted once, by its redo)
template <bool BUF>
struct VerRows {
    const VerArgs& v;
    const RowSrc& src;
    const Region<BUF>& g0;
    const Region<BUF>& g1;
    bool skip;
};

// matrix_compute in its verify form: the same product, marks and row scale,
// with the row store replaced by a load of the stored row and a compare (a
// copy, not a flag of matrix_compute: the existing forms keep their text and
// their registers)
template <int KP, int COLS, bool FULL, bool BUF>
__device__ __forceinline__ void matrix_compute_verify(
    const MatLayout& L, const int32_t* __restrict__ M,
    const int32_t (&xp)[COLS][KP], const Region<BUF>& go, roff_t<BUF> ors,
    uint32_t voff, long long col, long long col0, long long avail, int s,
    int n_lm, const int* s_i, const uint32_t* s_col, const Oor& out_oor,
    const int32_t* __restrict__ rowmap, const VerRows<BUF>* vr)
{
    // M: the per-stripe matrix block (wave-uniform: scalar loads)
    const int kin = L.kin;
    const int32_t* kcorr = M + L.kcorr();
    const int32_t* rscale = M + L.rscale();
    const int32_t* plain = M + L.plain();
    const bool rec = out_oor.counts != nullptr;
    for (int t = 0; t < L.R; t++) {
        const int32_t* mrow = M + t * KP;
        // the stored row of check t (wave-uniform id), loaded ahead of
        // the products
        int32_t sv[COLS];
        {
            const int id = min(static_cast<int>(vr->v.chk[static_cast<long long>(s) * L.R + t]),
                               vr->src.rows0 + vr->src.rows1 - 1);
            const bool lo = id < vr->src.split;
            Region<BUF> g = vr->g0;
            if constexpr (BUF)
                g.r = lo ? vr->g0.r : vr->g1.r;
            g.p = lo ? vr->g0.p : vr->g1.p;
            const roff_t<BUF> off = static_cast<roff_t<BUF>>(
                lo ? id * vr->src.rs0 * 2 : (id - vr->src.split) * vr->src.rs1 * 2);
            ld<COLS, FULL, BUF, kAuxLd>(g, off, voff, avail, sv);
        }
        int32_t acc[COLS];
#pragma unroll
        for (int c = 0; c < COLS; c++)
            acc[c] = kcorr[t];
#pragma unroll
        for (int j = 0; j < KP; j++) {
            const qi_short2 m2 = __builtin_bit_cast(qi_short2, mrow[j]);
#pragma unroll
            for (int c = 0; c < COLS; c++)
                acc[c] = fold(__builtin_amdgcn_sdot2(
                    __builtin_bit_cast(qi_short2, xp[c][j]), m2, acc[c], false));
        }
        int32_t y[COLS];
#pragma unroll
        for (int c = 0; c < COLS; c++)
            y[c] = fold(acc[c]);  // T-range
        // restored OOR symbols: 65536 == -1 where the stored word is 0
        for (int e = 0; e < n_lm; e++) {
            const int pos = s_i[e];
            const long long w = s_col[e];
            // branch-free per lane, unconditional load consumed at once (see
            // the matrix-core epilogue: a load under a divergent branch made
            // the compiler drain vmcnt(0) after every row)
            const long long d = w - col;
            const int32_t corr = plain[t * kin + pos];
#pragma unroll
            for (int c = 0; c < COLS; c++) {
                const int32_t yc = fold(fold(y[c] - corr));
                y[c] = d == c ? yc : y[c];
            }
        }
        const int32_t rs = rscale[t];
        if (rs != 1) {
#pragma unroll
            for (int c = 0; c < COLS; c++)
                y[c] = fold(fold(mul_rs(y[c], rs)));
        }
        uint32_t o[COLS];
        uint32_t bad = 0;
#pragma unroll
        for (int c = 0; c < COLS; c++) {
            o[c] = static_cast<uint32_t>(y[c]);
            bad |= o[c];
        }
        if (__builtin_expect((bad >> 16) != 0, 0)) {
#pragma unroll
            for (int c = 0; c < COLS; c++) {
                if (static_cast<uint32_t>(y[c]) > 65535u && rec &&
                    (FULL || c < avail))
                    record_oor(out_oor, s, rowmap[t], col + c);
                o[c] = fix16(y[c]);
            }
        }
        {
            // (a mismatch is rare: one ballot per row, the atomics by one lane)
            uint32_t mm = 0;
#pragma unroll
            for (int c = 0; c < COLS; c++)
                mm |= ((FULL || c < avail) && (o[c] & 0xffffu) != static_cast<uint32_t>(sv[c])
                           ? 1u
                           : 0u)
                      << c;
            mm = vr->skip ? 0u : mm;
            const uint64_t any = __builtin_amdgcn_ballot_w64(mm != 0);
            if (__builtin_expect(any != 0, 0)) {
                uint32_t tot = 0;
#pragma unroll
                for (int c = 0; c < COLS; c++)
                    tot += static_cast<uint32_t>(
                        __builtin_popcountll(__builtin_amdgcn_ballot_w64((mm >> c) & 1u)));
                // lane order is column order: the first lane holds the minimum
                if (mm && static_cast<int>(threadIdx.x & 63) == __builtin_ctzll(any)) {
                    const long long idx = static_cast<long long>(s) * L.R + t;
                    atomicAdd(vr->v.vmis + idx, tot);
                    atomicMin(vr->v.first + idx,
                              static_cast<uint32_t>(col) + __builtin_ctz(mm));
                }
            }
        }
    }
}


template <int KP, int COLS, bool BUF>
__global__ __launch_bounds__(kBlock) void matrix_kernel(MatArgs a)
{
    // (An include, not a template flag or a shared inline body: a shared
    // __forceinline__ body changed the register allocation of the plain
    // form -- SGPR spills, VGPRs, once the occupancy.  This way the plain
    // form keeps its text and its resource report; do not fold the two.)
    constexpr MatMode MODE = MatMode::kPlain;
    constexpr VerArgs v{};
#include "matrix_kernel_body.h"
}
// input and output marks in one launch (a repair): see push_slow_tile
template <int KP, int COLS, bool BUF>
__global__ __launch_bounds__(kBlock) void matrix_kernel_both(MatArgs a)
{
    constexpr MatMode MODE = MatMode::kBoth;
    constexpr VerArgs v{};
#include "matrix_kernel_body.h"
}
// a fused check: the repair's product compared with the stored rows
template <int KP, int COLS, bool BUF>
__global__ __launch_bounds__(kBlock) void matrix_kernel_verify(MatArgs a, VerArgs v)
{
    constexpr MatMode MODE = MatMode::kVerify;
#include "matrix_kernel_body.h"
}

// ---------------------------------------------------------------------------
// Matrix apply on the matrix cores (v_mfma_i32_16x16x32_i8 at KS = 1,
// v_mfma_i32_16x16x64_i8 above), kin <= 256.
//
// The product of matrix_kernel, out[t] = sum_i M[t][i] x_i mod q, with the
// u16 inputs and the row-scaled coefficients split into signed bytes:
//   x = 256 h' + l' + 32896        h' = (x >> 8) - 128, l' = (x & 255) - 128
//   c = 256 a + b                  a, b in [-128, 127] (split_i8)
// and 2^16 = -1 (mod q):
//   sum_i c x = 256 D2 + D1 - D0 + 32896 sum_i c
//   D0 = sum a h',  D1 = sum b l',  D2 = sum b h' + a l'
// -- three int8 GEMMs over K = [h' rows ; l' rows] against the per-stripe
// operand tiles [a|0], [0|b], [b|a] (matrix_pack.h pack_mf_dword; D1 starts
// at kmf[t] = 32896 sum c).  |D| <= 2 kin 128^2: up to kin = 128 (2^22)
// 256 D2 + D1 - D0 stays inside int32; at KS = 16 (kin <= 256, |D2| <= 2^23)
// the epilogue folds D2 before the shift.  The dot2 kernel's ~19 VALU
// per (output, column) become ~5 of epilogue, so the decode is HBM-bound
// rather than VALU-bound.
//
// Orientation D^T = X^T M^T: the A operand is the tile's byte planes,
// staged in LDS and read with ds_read_b64_tr_b8 (lane 2q+p of a 16-lane
// group addresses row q, bytes 8p..8p+7 of an 8 x 16-byte block; lane i gets
// column i -- profiles/r1_mfma_probe.txt); the B operand is the coefficient
// tile, pre-swizzled in lane order.  A lane's 4 results are 4 adjacent LDS
// columns of ONE output row t = lane & 15.  The LDS image stores column
// u = 16 g + 4 T + j of every 64-column super tile at byte 4 g + j of 16-byte
// chunk T, so after the 4 chunks of a super tile lane (g, t) holds the 16
// contiguous columns 16 g .. 16 g + 15 of row t: two b128 stores.
// Whole kRouteTile column tiles only; launch_matrix sends the tail to
// matrix_kernel.
// ---------------------------------------------------------------------------
typedef int qi_v4i __attribute__((ext_vector_type(4)));
// (The tall KS = 4 generators -- cfg3's 1024 x 64 -- run gen_mfma_kernel;
// this kernel's super-tile loop is plain.  Round 3's pipelined pair loop for
// them, the next tile's MFMAs interleaved with this one's epilogue, measured
// no gain against a plain loop in round 5: profiles/r5_ab_notes.txt.)
typedef int qi_v2i __attribute__((ext_vector_type(2)));
typedef unsigned int qi_v4u __attribute__((ext_vector_type(4)));

// ---- the verify forms' epilogue on the matrix cores: lane (g, t) holds 16
// adjacent columns of output row t, so it loads the same 32 bytes of the
// stored row (the four lanes of a row read one whole 128-byte line) and
// compares in place; nothing goes through the LDS transpose of the stores.

// This lane's stored row: fragment chk[t] of the stripe in the source
// regions, as a byte offset inside its region and the region (lo: region 0);
// rows past R get an offset past any extent (their loads return 0)
struct VerRow {
    uint32_t off;
    bool lo;
};
__device__ __forceinline__ VerRow verify_row(const VerArgs& v, const RowSrc& src, int s, int R,
                                             int t)
{
    // (an id the context builder refused still addresses a row of the stripe)
    const int id = min(static_cast<int>(v.chk[static_cast<long long>(s) * R + (t < R ? t : R - 1)]),
                       src.rows0 + src.rows1 - 1);
    const bool lo = id < src.split;
    const uint32_t off =
        static_cast<uint32_t>(lo ? id * src.rs0 * 2 : (id - src.split) * src.rs1 * 2);
    return {t < R ? off : 0x80000000u, lo};
}

// 16 columns (32 bytes) of that row from byte cb2 on.  TWO: the rows of a
// wave lie in either region, so each lane loads through both descriptors,
// past the extent in the other one (no memory access, zeros)
template <bool TWO>
__device__ __forceinline__ void verify_load16(const Region<true>& g0, const Region<true>& g1,
                                              const VerRow& vr, uint32_t cb2, qi_v4u (&sv)[2])
{
    constexpr uint32_t kOob = 0x80000000u;
    const bool in = vr.off != kOob;
    const uint32_t o0 = in && (!TWO || vr.lo) ? vr.off + cb2 : kOob;
#pragma unroll
    for (int h = 0; h < 2; h++)
        sv[h] = __builtin_amdgcn_raw_buffer_load_b128(g0.r, static_cast<int>(o0 + 16 * h), 0,
                                                      kAuxLd);
    if constexpr (TWO) {
        const uint32_t o1 = in && !vr.lo ? vr.off + cb2 : kOob;
#pragma unroll
        for (int h = 0; h < 2; h++)
            sv[h] |= __builtin_amdgcn_raw_buffer_load_b128(g1.r, static_cast<int>(o1 + 16 * h), 0,
                                                           kAuxLd);
    }
}

// Compare this lane's 16 stored-form values y (row idx - s R of the stripe,
// columns cb ..) with the loaded words; a row's mismatches are summed over
// its four lanes (g) and reported by the first: one atomic add and one
// atomic min per (wave, row) that saw one.  Every lane of the wave calls it;
// skip (wave-uniform): a slow tile, counted by its redo.
__device__ __forceinline__ void verify_tile16(const VerArgs& v, long long idx, bool trow,
                                              const int32_t (&y)[16], const qi_v4u (&sv)[2],
                                              long long cb, bool skip)
{
    uint32_t mm = 0;
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const uint32_t w = sv[h][d];
            mm |= (static_cast<uint32_t>(y[8 * h + 2 * d]) != (w & 0xffffu) ? 1u : 0u)
                  << (8 * h + 2 * d);
            mm |= (static_cast<uint32_t>(y[8 * h + 2 * d + 1]) != (w >> 16) ? 1u : 0u)
                  << (8 * h + 2 * d + 1);
        }
    mm = trow && !skip ? mm : 0u;
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(mm != 0) != 0, 0)) {
        uint32_t nm = static_cast<uint32_t>(__builtin_popcount(mm));
        uint32_t fm = mm ? static_cast<uint32_t>(cb) + __builtin_ctz(mm) : 0xffffffffu;
#pragma unroll
        for (int o = 16; o < 64; o *= 2) {
            nm += __shfl_xor(nm, o);
            fm = min(fm, static_cast<uint32_t>(__shfl_xor(fm, o)));
        }
        if ((threadIdx.x & 63) < 16 && nm) {
            atomicAdd(v.vmis + idx, nm);
            atomicMin(v.first + idx, fm);
        }
    }
}

// Geometry of a matrix-core block: NST super tiles of 64 columns (the
// block's columns, staged once as the A image), NW waves.  RSPLIT: the waves
// split the row blocks (wave wv takes wv, wv + NW, ...) and each walks every
// super tile, so an operand tile is fetched once per block; otherwise every
// wave takes every row block over its own NST / NW super tiles.
template <int KS, int NST, int NW>
struct MfmaTile {
    static constexpr int kThreads = 64 * NW;
    static constexpr int kCols = 64 * NST;     // columns per block
    static constexpr int kRows = 16 * KS;      // rows per byte plane
    static constexpr int kPitch = kCols + 16;  // LDS row pitch: +4 banks/row
    static constexpr size_t kImg = static_cast<size_t>(2 * kRows) * kPitch;
    // image + OOR scan scratch (s_i, s_col) + s_cnt
    static constexpr size_t kLds = kImg + 2 * 4 * kMaxTileOor + 16;
    // per-wave output staging tile (16 rows x 128 bytes, padded), only
    // allocated when the block has several 16-row output blocks
    static constexpr int kStagePitch = 144;
    static constexpr size_t kStage = 16 * kStagePitch;
    static constexpr size_t kLdsStaged = kLds + NW * kStage;
    // staging loads: CPL columns per lane (b64 or b32), TPR lanes per image
    // row, RG row groups
    // (b64 staging loads at 512-column blocks -- 32 rows per thread
    // instead of 64 -- measured the cfg3 encode 6 % slower, decode equal)
    static constexpr int kCpl = kCols >= 4 * kThreads ? 4 : 2;
    static constexpr int kTpr = kCols / kCpl;
    static constexpr int kRg = kThreads / kTpr;
    static_assert(kRg >= 1 && kThreads % kTpr == 0 && kRows % kRg == 0, "staging");
};


template <int KS, int NST, int NW, bool RSPLIT>
__global__ __launch_bounds__(64 * NW) void matrix_mfma_kernel(MatArgs a)
{
    // (An include, not a template flag or a shared inline body: a shared
    // __forceinline__ body changed the register allocation of the plain
    // form -- SGPR spills, VGPRs, once the occupancy.  This way the plain
    // form keeps its text and its resource report; do not fold the two.)
    constexpr MatMode MODE = MatMode::kPlain;
    constexpr VerArgs v{};
#include "matrix_mfma_body.h"
}
// input and output marks in one launch (a repair): see push_slow_tile
template <int KS, int NST, int NW, bool RSPLIT>
__global__ __launch_bounds__(64 * NW) void matrix_mfma_kernel_both(MatArgs a)
{
    constexpr MatMode MODE = MatMode::kBoth;
    constexpr VerArgs v{};
#include "matrix_mfma_body.h"
}
// a fused check: the repair's product compared with the stored rows
template <int KS, int NST, int NW, bool RSPLIT>
__global__ __launch_bounds__(64 * NW) void matrix_mfma_kernel_verify(MatArgs a, VerArgs v)
{
    constexpr MatMode MODE = MatMode::kVerify;
#include "matrix_mfma_body.h"
}

// ---------------------------------------------------------------------------
// Tall-generator encode at KS = 4 (33 <= k <= 64 and at least 64 output rows:
// cfg3's 1024 x 64 generator).  matrix_mfma_kernel<4, 8, 4, true>'s geometry
// and arithmetic -- a block of 4 waves stages 512 columns of the stripe's k
// data rows as the byte-plane image, wave wv walks row blocks wv, wv + 4, ...
// over all 8 super tiles, each 16 x 64 output tile transposed through the
// wave's LDS tile into whole-line stores -- without what an encode never
// meets: no input marks (no route tables, bucket scans, per-mark epilogue
// loop or slow-tile list), no received ids, one source region.  Its OOR
// outputs (value 65536) go to an LDS list recorded at the end of the block:
// recording one in the epilogue (a returning global atomic) waited for every
// store the wave had in flight.  A row block's operands come one row block
// ahead; the super-tile loop stays plain (the pipelined pair loop measured
// no gain).  The probe ladder of tools/membw7.hip (profiles/r5_ab_notes.txt)
// puts this structure at the store shape's time.
// ---------------------------------------------------------------------------
template <int NST, int NW>
__global__ __launch_bounds__(64 * NW) void gen_mfma_kernel(MatArgs a)
{
    constexpr int KS = 4;
    using G = MfmaTile<KS, NST, NW>;
    constexpr int NCOL = G::kCols, KH = G::kRows, RSB = G::kPitch;
    constexpr int CPL = G::kCpl, RG = G::kRg;
    static_assert(G::kTpr % 64 == 0, "row groups are wave-uniform");
    extern __shared__ __attribute__((aligned(16))) uint8_t qi_lds[];
    uint8_t* img = qi_lds;
    int* s_i = reinterpret_cast<int*>(qi_lds + G::kImg);
    uint32_t* s_col = reinterpret_cast<uint32_t*>(s_i + kMaxTileOor);
    int* s_cnt = reinterpret_cast<int*>(s_col + kMaxTileOor);
    const MatLayout L = a.L;
    const Oor out_oor = a.out_oor;
    const bool rec = out_oor.counts != nullptr;

    int s, tile;
    block_map(blockIdx.x, a.tiles, s, tile);
    const int kin = L.kin;
    const long long col0 = static_cast<long long>(tile) * NCOL;
    const uint32_t cl = (RG == 1 ? threadIdx.x : threadIdx.x % G::kTpr) * CPL;
    const int rg = RG == 1 ? 0 : static_cast<int>(threadIdx.x / G::kTpr);
    const uint32_t voff = static_cast<uint32_t>((col0 + cl) * 2);
    const int32_t* M = a.mat + s * a.ms;
    const Region<true> g0(a.src.base0 + s * a.src.ss0, a.ext.e0);
    const Region<true> go(a.dst.base + s * a.dst.ss, a.ext.eo);
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int g = l >> 4, q = (l & 15) >> 1, p = l & 1, tl = l & 15;
    const int RB = L.RB();
    const int32_t* mf = M + L.mf();
    const int32_t* kmf = M + L.kmf();
    const int32_t* rscale = M + L.rscale_mf();
    const int32_t* __restrict__ rowmap = a.rowmap;

    // a row block's operands: [a|0] over the h' K-steps (b0) and [0|b] over
    // the l' K-steps (b1), as x64 pairs; [b|a] is b1 over the h' half and b0
    // over the l' half, lane for lane (see matrix_mfma_kernel's load_ops)
    struct Ops {
        qi_v4i b0, b1;
        int32_t kt, rs, pr[3];
    };
    auto load_ops = [&](int rb, Ops& o) {
        auto ld2 = [&](int ks, int ty) {
            return *reinterpret_cast<const qi_v2i*>(mf + ((rb * KS + ks) * 3 + ty) * 128 + l * 2);
        };
        const qi_v2i x0 = ld2(0, 0), x1 = ld2(1, 0), y0 = ld2(2, 1), y1 = ld2(3, 1);
        o.b0 = qi_v4i{x0.x, x0.y, x1.x, x1.y};
        o.b1 = qi_v4i{y0.x, y0.y, y1.x, y1.y};
        // unconditional loads of a clamped row, selected after (an
        // exec-masked load leaves the vmcnt count unknown to the compiler)
        const int t = 16 * rb + tl, tc = t < L.R ? t : L.R - 1;
        const int32_t k0 = kmf[tc], r0 = rscale[tc];
        o.kt = t < L.R ? k0 : 0;
        o.rs = t < L.R ? r0 : 1;
        o.pr[0] = rowmap[tc];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int ot = 16 * rb + 8 * h + (l >> 3);
            o.pr[1 + h] = rowmap[ot < L.R ? ot : L.R - 1];
        }
    };
    const int rlast = RB - 1;
    Ops oA, oB;
    load_ops(min(wv, rlast), oA);

    // stage the tile: this thread's CPL columns of every RG-th data row (rows
    // past kin: a clamped row, their operand bytes are 0), all loads first
    uint32_t w[KH / RG][CPL / 2];
    {
        const uint32_t rsb = static_cast<uint32_t>(a.src.rs0 * 2);
#pragma unroll
        for (int r = 0; r < KH / RG; r++) {
            const int i = r * RG + rg;
            ld_dw<CPL / 2, true, kAuxLd>(g0, static_cast<uint32_t>(i < kin ? i : kin - 1) * rsb,
                                         voff, w[r]);
        }
    }
    const uint32_t lpos = 64 * (cl / 64) + 16 * ((cl % 16) / 4) + 4 * ((cl % 64) / 16) + cl % 4;
#pragma unroll
    for (int r = 0; r < KH / RG; r++) {
        const int i = r * RG + rg;
        if constexpr (CPL == 4) {
            const uint32_t hi =
                __builtin_amdgcn_perm(w[r][1], w[r][0], 0x07050301u) ^ 0x80808080u;
            const uint32_t lo =
                __builtin_amdgcn_perm(w[r][1], w[r][0], 0x06040200u) ^ 0x80808080u;
            *reinterpret_cast<uint32_t*>(img + i * RSB + lpos) = hi;
            *reinterpret_cast<uint32_t*>(img + (KH + i) * RSB + lpos) = lo;
        } else {
            const uint32_t hi = __builtin_amdgcn_perm(0u, w[r][0], 0x0c0c0301u) ^ 0x8080u;
            const uint32_t lo = __builtin_amdgcn_perm(0u, w[r][0], 0x0c0c0200u) ^ 0x8080u;
            *reinterpret_cast<uint16_t*>(img + i * RSB + lpos) = static_cast<uint16_t>(hi);
            *reinterpret_cast<uint16_t*>(img + (KH + i) * RSB + lpos) = static_cast<uint16_t>(lo);
        }
    }
    if (threadIdx.x == 0)
        *s_cnt = 0;
    __syncthreads();

    const uint32_t ors = static_cast<uint32_t>(a.dst.rs * 2);
    auto* lds = (__attribute__((address_space(3))) uint8_t*)img;
    const uint32_t abase = static_cast<uint32_t>((8 * g + q) * RSB + 8 * p);
    uint8_t* stg = qi_lds + G::kLds + wv * G::kStage;

    auto rb_body = [&](int rb, const Ops& o) {
        const int t = 16 * rb + tl;
        const bool trow = t < L.R;
        const qi_v4i ktv{o.kt, o.kt, o.kt, o.kt};
#pragma unroll 1
        for (int st = 0; st < NST; st++) {
            qi_v4i acc[4][3];
#pragma unroll
            for (int T = 0; T < 4; T++) {
                auto rd = [&](int ks) {
                    auto* pa = (__attribute__((address_space(3))) qi_v2i*)(
                        lds + abase + 32 * ks * RSB + (4 * st + T) * 16);
                    return __builtin_amdgcn_ds_read_tr8_b64_v2i32(pa);
                };
                const qi_v2i h0 = rd(0), h1 = rd(1), l0 = rd(2), l1 = rd(3);
                const qi_v4i ah{h0.x, h0.y, h1.x, h1.y}, al{l0.x, l0.y, l1.x, l1.y};
                acc[T][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, o.b0, qi_v4i{0, 0, 0, 0},
                                                                  0, 0, 0);
                acc[T][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, o.b1, ktv, 0, 0, 0);
                acc[T][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, o.b1, qi_v4i{0, 0, 0, 0},
                                                                  0, 0, 0);
                acc[T][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, o.b0, acc[T][2], 0, 0, 0);
            }
            // lane (g, t) holds row t, columns cb .. cb + 15 (the image's
            // column order): y = 256 D2 + D1 - D0, kt in D1
            const long long cb = col0 + 64 * st + 16 * g;
            int32_t y[16];
#pragma unroll
            for (int T = 0; T < 4; T++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    y[4 * T + j] = fold(fold((acc[T][2][j] << 8) + acc[T][1][j] - acc[T][0][j]));
            if (__builtin_amdgcn_ballot_w64(o.rs != 1)) {
#pragma unroll
                for (int c = 0; c < 16; c++)
                    y[c] = fold(fold(mul_rs(y[c], o.rs)));
            }
            uint32_t bad = 0;
#pragma unroll
            for (int c = 0; c < 16; c++)
                bad |= static_cast<uint32_t>(y[c]);
            if (__builtin_expect(__builtin_amdgcn_ballot_w64((bad >> 16) != 0) != 0, 0)) {
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    if (static_cast<uint32_t>(y[c]) > 65535u) {
                        if (rec && trow) {
                            // LDS atomic: no wait on the stores in flight
                            const int e = atomicAdd(s_cnt, 1);
                            if (e < kMaxTileOor) {
                                s_i[e] = o.pr[0];
                                s_col[e] = static_cast<uint32_t>(cb + c);
                            } else {
                                record_oor(out_oor, s, o.pr[0], cb + c);
                            }
                        }
                        y[c] = 0;  // 65536 (or its alias -1) is stored as 0
                    }
                }
            }
            qi_v4u o0, o1;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                o0[c] = pack_lo(static_cast<uint32_t>(y[2 * c]), static_cast<uint32_t>(y[2 * c + 1]));
                o1[c] = pack_lo(static_cast<uint32_t>(y[8 + 2 * c]),
                                static_cast<uint32_t>(y[8 + 2 * c + 1]));
            }
            *reinterpret_cast<qi_v4u*>(stg + tl * G::kStagePitch + 32 * g) = o0;
            *reinterpret_cast<qi_v4u*>(stg + tl * G::kStagePitch + 32 * g + 16) = o1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int orow = 8 * h + (l >> 3), c = l & 7;
                const qi_v4u v =
                    *reinterpret_cast<const qi_v4u*>(stg + orow * G::kStagePitch + 16 * c);
                // rows >= R: an offset past the extent (< 2^31), dropped
                const int ot = 16 * rb + orow;
                const uint32_t vo =
                    ot < L.R ? static_cast<uint32_t>(o.pr[1 + h]) * ors +
                                   static_cast<uint32_t>((col0 + 64 * st + 8 * c) * 2)
                             : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b128(v, go.r, static_cast<int>(vo), 0, kAuxStMf);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    };
    // row blocks in ping-pong over two operand sets, each prefetched one row
    // block ahead and unconditional (a clamped row block past the end)
    for (int rb = wv; rb < RB; rb += 2 * NW) {
        load_ops(min(rb + NW, rlast), oB);
        rb_body(rb, oA);
        if (rb + NW >= RB)
            break;
        load_ops(min(rb + 2 * NW, rlast), oA);
        rb_body(rb + NW, oB);
    }
    // the block's OOR outputs into their buckets
    __syncthreads();
    const int n = min(*s_cnt, kMaxTileOor);
    for (int e = threadIdx.x; e < n; e += 64 * NW)
        record_oor(out_oor, s, s_i[e], s_col[e]);
}

// ---------------------------------------------------------------------------
// Operand-stationary matrix-core kernel (KS = 4, 8, 16: 32 < kin <= 256; the
// decodes of k = 33 .. 256 and the generators of those codes).
//
// matrix_mfma_kernel stages one column block, computes it and exits: every
// block re-fetches the operand tiles of every row block it covers from L2
// (16 KB of non-zero i8 tiles per 16 output rows at KS = 16, ~8x the HBM
// data stream at k = 200), and its load and compute phases run one after
// the other (two blocks per CU in lock step).  Here a block of 8 waves
// stays on one stripe for a range of column tiles:
//   - wave w owns RPW row blocks (slot w % WR) for the block's whole life:
//     their operand tiles stay in registers (KS / 2 + KS / 2 v4i each: 64
//     VGPRs at KS = 16), with kmf / rscale / rowmap;
//   - a tile is 64 NSTT columns, NSTT = 8 / WR super tiles of 64 columns
//     (wave w takes super tile w / WR), staged as the byte-plane image of
//     matrix_mfma_kernel in one of two LDS buffers: the next tile's rows are
//     loaded into registers while this one is on the matrix cores;
//   - a matrix with more than WR RPW row blocks runs G blocks per column
//     range (group gq takes rb = gq WR RPW + slot + WR j); they read the same
//     input tiles, and the XCD-aware map puts them on one XCD (shared L2).
// The arithmetic, operand tiles, epilogue and OOR handling are
// matrix_mfma_kernel's (byte split, 2^16 = -1, D2 folded first at KS = 16).
// ---------------------------------------------------------------------------
// Coefficient M[t][pos] of this lane's output row t (lane (g, t & 15) of a
// 16-row block) from the block's [b | a] operand tile held in registers:
// pick(2 ks + dw) returns this lane's dword dw of K-step ks (lane 16 g + t:
// bytes K = 32 ks + 8 g + 4 dw + 0..3; b at K = pos, a at K = 16 KS + pos,
// pack_mf_dword's layout).  Returns the row-scaled entry as 256 a + b
// (balanced), the value of mf_entry / the `plain` section; pos is
// wave-uniform, and each byte comes from the lane holding it by ds_bpermute
// -- no memory load (waiting for one drains the stores and prefetches).
template <int KS, class Pick>
__device__ __forceinline__ int32_t coef_from_tiles(const Pick& pick, int pos, int lane)
{
    constexpr int KH = 16 * KS;
    auto byte_at = [&](int K) {
        const int ks = K >> 5, g = (K & 31) >> 3, dw = (K >> 2) & 1, sh = 8 * (K & 3);
        const int32_t x = __shfl(pick(2 * ks + dw), 16 * g + (lane & 15));
        return (x << (24 - sh)) >> 24;
    };
    return 256 * byte_at(KH + pos) + byte_at(pos);
}

// uniform-index selection among a wave's operand dwords (a v_cndmask chain)
template <int NP>
__device__ __forceinline__ int32_t pick_v4(const qi_v4i (&v)[NP], int idx)
{
    int32_t r = 0;
#pragma unroll
    for (int i = 0; i < NP; i++)
#pragma unroll
        for (int e = 0; e < 4; e++)
            r = idx == 4 * i + e ? v[i][e] : r;
    return r;
}

// K chunks of the operand-stationary kernel: KS = 40 (384 < k <= 640) stages
// its image in two chunks of 20 K-steps (the received rows [0, 320) and
// [320, 640)), double-buffered over (tile, chunk) items, the accumulators
// held across the chunks of a tile: a whole KS = 40 image (2 x 640 rows of
// 80 bytes, 102 KB) could not be double-buffered in LDS
template <int KS>
struct OsK {
    static constexpr int NCH = KS > 24 ? 2 : 1;  // K chunks per tile
    static constexpr int KC = KS / NCH;          // K-steps per chunk
};

template <int KS, int WR>
struct OsTile {
    static constexpr int kWaves = 8;
    static constexpr int kThreads = 64 * kWaves;
    static constexpr int kNst = kWaves / WR;   // super tiles per tile
    static constexpr int kCols = 64 * kNst;    // columns per tile
    static constexpr int kRows = 16 * KS;      // rows per byte plane (KH)
    static constexpr int kPitch = kCols + 16;  // LDS row pitch: +4 banks/row
    static constexpr size_t kImg = static_cast<size_t>(2 * kRows) * kPitch;
    static constexpr int kStagePitch = 144;
    static constexpr size_t kStage = 16 * kStagePitch;
    static constexpr size_t kStageOff = 2 * kImg;
    static constexpr size_t kMarkOff = kStageOff + kWaves * kStage;
    // two mark lists (s_i, s_col) + two counts
    static constexpr size_t kLds = kMarkOff + 2 * 2 * 4 * kMaxTileOor + 16;
    // staging: 4 columns (b64) per lane, kTpr lanes per image row
    static constexpr int kTpr = kCols / 4;
    static constexpr int kRpp = kThreads / kTpr;  // rows per pass
    static constexpr int kRpt = kRows / kRpp;     // rows per thread
    static_assert(kRpt >= 1 && kRows % kRpp == 0, "staging");
};


template <int KS, int WR, int RPW, bool TWO>
__global__ __launch_bounds__(512) void matrix_os_kernel(MatArgs a, int G, int C, int TS)
{
    // (An include, not a template flag or a shared inline body: a shared
    // __forceinline__ body changed the register allocation of the plain
    // form -- SGPR spills, VGPRs, once the occupancy.  This way the plain
    // form keeps its text and its resource report; do not fold the two.)
    constexpr MatMode MODE = MatMode::kPlain;
    constexpr VerArgs v{};
#include "matrix_os_body.h"
}
// input and output marks in one launch (a repair): see push_slow_tile
template <int KS, int WR, int RPW, bool TWO>
__global__ __launch_bounds__(512) void matrix_os_kernel_both(MatArgs a, int G, int C, int TS)
{
    constexpr MatMode MODE = MatMode::kBoth;
    constexpr VerArgs v{};
#include "matrix_os_body.h"
}
// a fused check: the repair's product compared with the stored rows
template <int KS, int WR, int RPW, bool TWO>
__global__ __launch_bounds__(512) void matrix_os_kernel_verify(MatArgs a, int G, int C, int TS,
                                                               VerArgs v)
{
    constexpr MatMode MODE = MatMode::kVerify;
#include "matrix_os_body.h"
}


// ---------------------------------------------------------------------------
// Fused check, the marks: the _verify forms left every recomputed 65536 of
// check row t in work bucket t; the stored row's own bucket must hold exactly
// those columns.  One block per (stripe, check row) takes the two buckets as
// sets and counts their symmetric difference by comparing all pairs (a bucket
// holds about words / 65537 entries; the cost is quadratic, but no entry is
// ever dropped): entry i counts when the other bucket lacks its column and no
// earlier entry of its own bucket repeats it.  Stored entries that are no
// column of the row (>= words) are ignored.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void verify_marks_kernel(
    const uint16_t* __restrict__ checks, int R, Oor stored, int slot_base, Oor work,
    long long words, uint32_t* __restrict__ mark_mismatch, uint32_t* __restrict__ first,
    uint32_t* err)
{
    __shared__ uint32_t s_n, s_min;
    const int s = blockIdx.x / R, t = blockIdx.x - s * R;
    const long long idx = static_cast<long long>(s) * R + t;
    if (threadIdx.x == 0) {
        s_n = 0;
        s_min = 0xffffffffu;
    }
    __syncthreads();
    const int slot = static_cast<int>(checks[idx]) - slot_base;
    const bool has = stored.counts != nullptr && slot >= 0 && slot < stored.slots;
    const long long ab = static_cast<long long>(s) * stored.slots + slot;
    uint32_t na = has ? stored.counts[ab] : 0u, nb = work.counts[idx];
    if (na > static_cast<uint32_t>(stored.cap) || nb > static_cast<uint32_t>(work.cap)) {
        if (threadIdx.x == 0)
            atomicOr(err, kErrOorTruncated);
        na = min(na, static_cast<uint32_t>(stored.cap));
        nb = min(nb, static_cast<uint32_t>(work.cap));
    }
    const uint32_t* A = has ? stored.entries + ab * stored.cap : nullptr;
    const uint32_t* B = work.entries + idx * work.cap;
    uint32_t n = 0, mn = 0xffffffffu;
    for (uint32_t i = threadIdx.x; i < na + nb; i += kBlock) {
        const bool in_a = i < na;
        const uint32_t* own = in_a ? A : B;
        const uint32_t* other = in_a ? B : A;
        const uint32_t io = in_a ? i : i - na, n_other = in_a ? nb : na;
        const uint32_t c = own[io];
        bool count = !in_a || c < words;
        for (uint32_t j = 0; count && j < io; j++)
            count = own[j] != c;
        for (uint32_t j = 0; count && j < n_other; j++)
            count = other[j] != c;
        if (count) {
            n++;
            mn = min(mn, c);
        }
    }
    if (n) {
        atomicAdd(&s_n, n);
        atomicMin(&s_min, mn);
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_n) {
        atomicAdd(mark_mismatch + idx, s_n);
        atomicMin(first + idx, s_min);
    }
}

__global__ __launch_bounds__(kBlock) void verify_init_kernel(uint32_t* value_mismatch,
                                                             uint32_t* mark_mismatch,
                                                             uint32_t* first,
                                                             uint32_t* work_counts, long long n)
{
    const long long i = static_cast<long long>(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) {
        value_mismatch[i] = 0u;
        mark_mismatch[i] = 0u;
        first[i] = 0xffffffffu;
        work_counts[i] = 0u;
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
int launch_verify_init(uint32_t* value_mismatch, uint32_t* mark_mismatch, uint32_t* first,
                       uint32_t* work_counts, long long n, hipStream_t st)
{
    if (n <= 0)
        return 0;
    const long long grid = (n + kBlock - 1) / kBlock;
    if (grid > 0x7fffffffLL)
        return -1;
    hipLaunchKernelGGL(verify_init_kernel, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0, st,
                       value_mismatch, mark_mismatch, first, work_counts, n);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

int launch_verify_marks(const uint16_t* checks, int R, int S, const Oor* stored, int slot_base,
                        const Oor& work, long long words, uint32_t* mark_mismatch,
                        uint32_t* first, uint32_t* err, hipStream_t st)
{
    const long long grid = static_cast<long long>(S) * R;
    if (grid <= 0)
        return 0;
    if (grid > 0x7fffffffLL)
        return -1;
    const Oor none{nullptr, nullptr, 0, 0};
    hipLaunchKernelGGL(verify_marks_kernel, dim3(static_cast<unsigned>(grid)), dim3(kBlock), 0, st,
                       checks, R, stored ? *stored : none, slot_base, work, words, mark_mismatch,
                       first, err);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

static int grid_for(long long words, int cols, int n_stripes, int* tiles)
{
    const long long per = static_cast<long long>(kBlock) * cols;
    const long long t = (words + per - 1) / per;
    if (t <= 0 || t * n_stripes > 0x7fffffffLL)
        return -1;
    *tiles = static_cast<int>(t);
    return 0;
}

template <int K, int COLS, bool KEQ, bool BUF>
static int enc_launch(int k, int n, int n_out, const int32_t* tw,
                      const uint16_t* data, long long dss, long long drs,
                      uint32_t iext, RowDst out, uint32_t oext, long long words,
                      int S, Oor oor, hipStream_t st)
{
    int tiles;
    if (grid_for(words, COLS, S, &tiles))
        return -1;
    // (flat: the row strides' upper halves in the extents' place)
    const unsigned long long ib = static_cast<unsigned long long>(drs) * 2,
                             ob = static_cast<unsigned long long>(out.rs) * 2;
    if constexpr (!BUF) {
        iext = static_cast<uint32_t>(ib >> 32);
        oext = static_cast<uint32_t>(ob >> 32);
    }
    hipLaunchKernelGGL((encode_fnt_kernel<K, COLS, KEQ, BUF>), dim3(tiles * S),
                       dim3(kBlock), 0, st, k, n, n_out, tw, data, dss,
                       static_cast<uint32_t>(ib), iext, out.base, out.ss,
                       static_cast<uint32_t>(ob), oext, words, tiles,
                       oor);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

static bool aligned_for(int cols, const void* p, long long a, long long b,
                        long long c, long long d)
{
    const long long m = cols;
    return (reinterpret_cast<uintptr_t>(p) % (2 * cols)) == 0 && a % m == 0 &&
           b % m == 0 && c % m == 0 && d % m == 0;
}

int launch_encode_fnt(int k, int n, int n_out, const int32_t* d_twist,
                      const uint16_t* data, long long dss, long long drs,
                      RowDst out, long long words, int S, Oor oor,
                      uint32_t* /*d_err*/, hipStream_t st)
{
    const int K = static_cast<int>(ceil2(static_cast<uint32_t>(k)));
    const bool a2 = aligned_for(2, data, dss, drs, out.ss, out.rs) &&
                    (reinterpret_cast<uintptr_t>(out.base) % 4) == 0;
    const uint32_t ie = row_extent(k, drs, words), oe = row_extent(n_out, out.rs, words);
    if (!ie || !oe) {
        // stripes wider than a 31-bit buffer range: flat addressing
        switch (K) {
#define QI_ENC_FLAT(KK)                                                        \
    case KK:                                                                   \
        return enc_launch<KK, 1, false, false>(k, n, n_out, d_twist, data, dss, \
                                               drs, 0, out, 0, words, S, oor,  \
                                               st);
            QI_ENC_FLAT(1)
            QI_ENC_FLAT(2)
            QI_ENC_FLAT(4)
            QI_ENC_FLAT(8)
            QI_ENC_FLAT(16)
            QI_ENC_FLAT(32)
            QI_ENC_FLAT(64)
#undef QI_ENC_FLAT
        default:
            return -3;
        }
    }
#define QI_ENC(KK, C2)                                                         \
    if (K == KK) {                                                             \
        if (a2 && k == KK)                                                     \
            return enc_launch<KK, C2, true, true>(k, n, n_out, d_twist, data,  \
                                                  dss, drs, ie, out, oe,       \
                                                  words, S, oor, st);          \
        if (a2)                                                                \
            return enc_launch<KK, C2, false, true>(k, n, n_out, d_twist, data, \
                                                   dss, drs, ie, out, oe,      \
                                                   words, S, oor, st);         \
        return enc_launch<KK, 1, false, true>(k, n, n_out, d_twist, data, dss, \
                                              drs, ie, out, oe, words, S, oor, \
                                              st);                             \
    }
    QI_ENC(1, 2)
    QI_ENC(2, 2)
    QI_ENC(4, 2)
    QI_ENC(8, 2)
    QI_ENC(16, 2)
    QI_ENC(32, 1)
    QI_ENC(64, 1)
#undef QI_ENC
    return -3;  // K > 64: caller uses the matrix path
}

// The launchers below run what matrix_route (matrix_route.h) chose: each
// takes its template parameters and the runtime forms (`both`, `two`) from
// the route and decides only its grid.

// dynamic LDS above the default limit needs opting in per kernel
static bool lds_opt_in(const void* fn, size_t bytes)
{
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(bytes)) == hipSuccess;
}

template <int KP, int COLS, bool BUF>
static int mat_launch(MatArgs a, const MatRoute& r, int S, hipStream_t st, const VerArgs& v)
{
    if (grid_for(a.words - a.ext.c0, COLS, S, &a.tiles))
        return -1;
    if (r.verify) {
        hipLaunchKernelGGL((matrix_kernel_verify<KP, COLS, BUF>), dim3(a.tiles * S), dim3(kBlock),
                           0, st, a, v);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    const auto fn = r.both ? &matrix_kernel_both<KP, COLS, BUF> : &matrix_kernel<KP, COLS, BUF>;
    hipLaunchKernelGGL(fn, dim3(a.tiles * S), dim3(kBlock), 0, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int KS, int NST, int NW, bool RSPLIT>
static int mfma_launch(MatArgs a, const MatRoute& r, int S, hipStream_t st, const VerArgs& v)
{
    using G = MfmaTile<KS, NST, NW>;
    using Fn = void (*)(MatArgs);
    const Fn one = &matrix_mfma_kernel<KS, NST, NW, RSPLIT>;
    // input and output marks together (a repair: at most 4 row blocks; KS >=
    // 4 runs the operand-stationary kernel)
    Fn both = nullptr;
    if constexpr (mfma_has_both(KS))
        both = &matrix_mfma_kernel_both<KS, NST, NW, RSPLIT>;
    const Fn run = r.both ? both : one;
    const long long t = r.wfull / G::kCols;
    if (!run || t <= 0 || t * S > 0x7fffffffLL)
        return -1;
    a.tiles = static_cast<int>(t);
    const size_t lds = a.L.RB() > 1 ? G::kLdsStaged : G::kLds;
    static std::atomic<uint64_t> attr_done{0};
    if (G::kLdsStaged > 65536 && once_per_device(attr_done, [&](int) {
            return lds_opt_in(reinterpret_cast<const void*>(one), G::kLdsStaged) &&
                   (!both || lds_opt_in(reinterpret_cast<const void*>(both), G::kLdsStaged));
        }) < 0)
        return -2;
    if (r.verify) {
        // (the shapes of the _both form; at most 4 row blocks: under 64 KiB)
        if constexpr (mfma_has_both(KS)) {
            static_assert(G::kLdsStaged <= 65536, "verify form without the LDS opt-in");
            hipLaunchKernelGGL((matrix_mfma_kernel_verify<KS, NST, NW, RSPLIT>), dim3(t * S),
                               dim3(G::kThreads), lds, st, a, v);
            return hipGetLastError() == hipSuccess ? 0 : -2;
        }
        return -1;
    }
    hipLaunchKernelGGL(run, dim3(t * S), dim3(G::kThreads), lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int NST, int NW>
static int gen_launch(MatArgs a, const MatRoute& r, int S, hipStream_t st)
{
    using G = MfmaTile<4, NST, NW>;
    const long long t = r.wfull / G::kCols;
    if (t <= 0 || t * S > 0x7fffffffLL)
        return -1;
    a.tiles = static_cast<int>(t);
    static std::atomic<uint64_t> attr_done{0};
    if (once_per_device(attr_done, [](int) {
            return lds_opt_in(reinterpret_cast<const void*>(&gen_mfma_kernel<NST, NW>),
                              G::kLdsStaged);
        }) < 0)
        return -2;
    hipLaunchKernelGGL((gen_mfma_kernel<NST, NW>), dim3(t * S), dim3(G::kThreads),
                       G::kLdsStaged, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

template <int KS, int WR, int RPW>
static int os_launch(MatArgs a, const MatRoute& r, int S, hipStream_t st, const VerArgs& v)
{
    using O = OsTile<OsK<KS>::KC, WR>;
    // the forms the library has (matrix_route.h), indexed by two + 2 * both
    void (*fns[4])(MatArgs, int, int, int) = {&matrix_os_kernel<KS, WR, RPW, false>};
    if constexpr (os_has_two(KS, RPW))
        fns[1] = &matrix_os_kernel<KS, WR, RPW, true>;
    if constexpr (os_has_both(KS, WR, RPW)) {
        fns[2] = &matrix_os_kernel_both<KS, WR, RPW, false>;
        fns[3] = &matrix_os_kernel_both<KS, WR, RPW, true>;
    }
    // the verify forms, indexed by two (the shapes of the _both forms)
    void (*vfns[2])(MatArgs, int, int, int, VerArgs) = {nullptr, nullptr};
    if constexpr (os_has_both(KS, WR, RPW)) {
        vfns[0] = &matrix_os_kernel_verify<KS, WR, RPW, false>;
        vfns[1] = &matrix_os_kernel_verify<KS, WR, RPW, true>;
    }
    const long long TS = r.wfull / O::kCols;
    if (TS <= 0 || TS > 0x7fffffffLL)
        return -1;
    const int RB = a.L.RB();
    const int G = (RB + WR * RPW - 1) / (WR * RPW);
    constexpr size_t lds = O::kLds + kOsMaxTiles / 8;
    // per device, once: the dynamic-LDS attribute and the number of blocks
    // the device holds at once (CUs x blocks per CU)
    static std::atomic<uint64_t> attr_done{0};
    static std::atomic<int> slots_of[kOnceDevices];
    const int dev = once_per_device(attr_done, [&](int d) {
        for (const auto fn : fns)
            if (fn && lds > 65536 && !lds_opt_in(reinterpret_cast<const void*>(fn), lds))
                return false;
        for (const auto fn : vfns)
            if (fn && lds > 65536 && !lds_opt_in(reinterpret_cast<const void*>(fn), lds))
                return false;
        int per_cu = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(
                &per_cu, reinterpret_cast<const void*>(fns[0]), O::kThreads, lds) != hipSuccess ||
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess)
            return false;
        if (d < kOnceDevices)
            slots_of[d].store(std::max(1, per_cu) * std::max(1, cus), std::memory_order_relaxed);
        return true;
    });
    if (dev < 0)
        return -2;
    const long long slots =
        dev < kOnceDevices ? slots_of[dev].load(std::memory_order_relaxed) : 256;
    // blocks wanted over the launch: ~2 per CU, or ~8 for the short KS = 4
    // decodes (cfg3: two column ranges per stripe, 0.168 -> 0.158 ms; the
    // KS >= 8 decodes and generators lose at 2048, gpurun_out ab_x4)
    constexpr long long kTarget = KS == 4 ? 2048 : 512;
    const long long SG = static_cast<long long>(S) * G;
    const long long cmax = std::max(1LL, TS / 4);
    long long C = (kTarget + SG - 1) / SG;
    C = std::max(1LL, std::min(C, cmax));
    // the blocks are equal: a launch of B blocks takes ceil(B / slots)
    // rounds, so among C .. 2C - 1 take the column-range count whose last
    // round is fullest (k300 / k384: 576 blocks on 256 one-block CUs ran
    // three rounds, the last a quarter full; 768 fill them), then let the
    // XCD map have S * C a multiple of 8
    {
        long long best = C;
        double best_eff = 0.0;
        for (long long c = C; c < 2 * C && c <= cmax; c++) {
            const long long B = SG * c;
            const double eff = static_cast<double>(B) / (((B + slots - 1) / slots) * slots);
            if (eff > best_eff + 1e-9) {
                best_eff = eff;
                best = c;
            }
        }
        C = best;
    }
    while ((S * C) % 8 != 0 && C < TS / 2)
        C++;
    // at most kOsMaxTiles tiles per block (the LDS bitmask of its slow
    // tiles)
    C = std::max(C, (TS + kOsMaxTiles - 1) / kOsMaxTiles);
    const long long blocks = SG * C;
    if (blocks > 0x7fffffffLL)
        return -1;
    a.tiles = static_cast<int>(TS);
    if (r.verify) {
        const auto vfn = vfns[r.two ? 1 : 0];
        if (!vfn)
            return -1;
        hipLaunchKernelGGL(vfn, dim3(static_cast<unsigned>(blocks)), dim3(O::kThreads), lds, st,
                           a, G, static_cast<int>(C), static_cast<int>(TS), v);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    const auto fn = fns[(r.two ? 1 : 0) + (r.both ? 2 : 0)];
    if (!fn)
        return -1;  // (matrix_route reports these as errors)
    hipLaunchKernelGGL(fn, dim3(static_cast<unsigned>(blocks)), dim3(O::kThreads), lds, st, a, G,
                       static_cast<int>(C), static_cast<int>(TS));
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

// The one map from a route to its instantiation: every matrix kernel of the
// library appears here, and nothing else launches one (the redo launch,
// which has no parameters, is launch_matrix's).
static int launch_route(const MatRoute& r, MatArgs a, int S, hipStream_t st,
                        const VerArgs& v = VerArgs{})
{
    if (r.err == -1)
        return -1;
#define QI_OS(KS_, WR_, RPW_)                                  \
    if (r.KS == KS_ && r.WR == WR_ && r.RPW == RPW_)           \
        rc = os_launch<KS_, WR_, RPW_>(a, r, S, st, v);
#define QI_MFMA(KS_, NST_, NW_, RS_)                                          \
    if (r.KS == KS_ && r.NST == NST_ && r.NW == NW_ && r.RSPLIT == RS_)       \
        rc = mfma_launch<KS_, NST_, NW_, RS_>(a, r, S, st, v);
    if (r.core != MatCore::kNone) {
        int rc = -1;
        if (r.core == MatCore::kGen) {
            if (r.NST == 8 && r.NW == 4)
                rc = gen_launch<8, 4>(a, r, S, st);
        } else if (r.core == MatCore::kOs) {
            QI_OS(4, 4, 1) QI_OS(4, 8, 1) QI_OS(8, 8, 1) QI_OS(16, 8, 1) QI_OS(16, 8, 2)
            QI_OS(20, 8, 1) QI_OS(20, 8, 2) QI_OS(24, 8, 1) QI_OS(24, 8, 2) QI_OS(40, 8, 1)
        } else {
            QI_MFMA(1, 16, 4, false) QI_MFMA(1, 16, 4, true) QI_MFMA(2, 8, 4, false)
            QI_MFMA(2, 8, 4, true) QI_MFMA(4, 8, 4, false) QI_MFMA(4, 8, 4, true)
            QI_MFMA(8, 4, 4, true) QI_MFMA(16, 1, 4, true)
        }
        if (rc || !r.tail)
            return rc;
        a.ext.c0 = r.wfull;
    }
#undef QI_OS
#undef QI_MFMA
#define QI_TAIL(KP_, COLS_, BUF_)                                \
    if (r.KP == KP_ && r.COLS == COLS_ && r.BUF == BUF_)         \
        return mat_launch<KP_, COLS_, BUF_>(a, r, S, st, v);
    QI_TAIL(2, 1, false) QI_TAIL(2, 1, true) QI_TAIL(2, 2, true) QI_TAIL(2, 4, true)
    QI_TAIL(4, 1, false) QI_TAIL(4, 1, true) QI_TAIL(4, 2, true) QI_TAIL(4, 4, true)
    QI_TAIL(8, 1, false) QI_TAIL(8, 1, true) QI_TAIL(8, 2, true) QI_TAIL(8, 4, true)
    QI_TAIL(16, 1, false) QI_TAIL(16, 1, true) QI_TAIL(16, 2, true)
    QI_TAIL(32, 1, false) QI_TAIL(32, 1, true)
    QI_TAIL(64, 1, false) QI_TAIL(64, 1, true)
    QI_TAIL(128, 1, false) QI_TAIL(128, 1, true)
#undef QI_TAIL
    return -3;
}

// rows at `cols`-word aligned offsets (source regions and destination)
static bool rows_aligned(int cols, const RowSrc& src, const RowDst& dst)
{
    return aligned_for(cols, src.base0, src.ss0, src.rs0, dst.ss, dst.rs) &&
           (src.base1 == nullptr || aligned_for(cols, src.base1, src.ss1, src.rs1, 0, 0)) &&
           (reinterpret_cast<uintptr_t>(dst.base) % (2 * cols)) == 0;
}

static MatExt mat_ext(const RowSrc& src, int R, const RowDst& dst, long long words)
{
    return MatExt{row_extent(src.rows0, src.rs0, words), row_extent(src.rows1, src.rs1, words),
                  row_extent(R, dst.rs, words), 0};
}

// what matrix_route reads of a launch
static MatRouteIn route_in(const MatArgs& a, bool verify = false)
{
    const bool buf = a.ext.e0 && a.ext.eo && (!a.src.base1 || a.ext.e1);
    const int align = !rows_aligned(2, a.src, a.dst) ? 1 : rows_aligned(4, a.src, a.dst) ? 4 : 2;
    return MatRouteIn{a.L, a.words, buf, align, a.in_oor.counts != nullptr,
                      a.out_oor.counts != nullptr, a.ids != nullptr, a.route != nullptr,
                      a.src.base1 != nullptr, verify};
}

bool matrix_cores_take(const RowSrc& src, const RowDst& dst, int R, long long words)
{
    MatArgs a{};
    a.src = src;
    a.dst = dst;
    a.ext = mat_ext(src, R, dst, words);
    const MatRouteIn in = route_in(a);
    return in.buf && in.align == 4 && words >= kRouteTile;
}

// for aligned rows in buffer range; a decode's ids and route table come with
// its input marks.  both: input and output marks in one launch (a repair)
std::string matrix_kernel_names(const MatLayout& L, long long words, bool in_oor, bool two,
                                bool both, bool verify)
{
    return to_string(
        matrix_route(MatRouteIn{L, words, true, 4, in_oor, both, in_oor, in_oor, two, verify}));
}

std::string encode_fnt_kernel_name(int k)
{
    const int K = static_cast<int>(ceil2(static_cast<uint32_t>(k)));
    return "encode_fnt_kernel<" + std::to_string(K) + ", " + std::to_string(K <= 16 ? 2 : 1) +
           ", " + (k == K ? "true" : "false") + ", true>";
}

int launch_matrix(const MatLayout& L, const int32_t* mat, long long ms,
                  const int32_t* ids, long long is, RowSrc src, RowDst dst,
                  long long words, int S, const Oor* in_oor, int slot_base,
                  const Oor* out_oor, const int32_t* rowmap, const uint32_t* route,
                  long long rstride, SlowList slow, uint32_t* err, hipStream_t st,
                  const MatVerify* ver)
{
    if (!rowmap)
        return -1;
    if (L.KP != matrix_kp(L.kin))
        return -4;
    if (in_oor && !slow.base)
        return -1;  // input marks need the slow-tile lists
    const Oor none{nullptr, nullptr, 0, 0};
    // no input buckets: no marks.  The route table goes with them: the
    // operand-stationary kernel and the NTT engine restore nothing without
    // the buckets, so the kernels that read the table alone must not either
    // (qi_gpu.h, qi_gpu_decode)
    if (!in_oor)
        route = nullptr;
    MatArgs a{L, mat, ms, ids, is, src, dst, mat_ext(src, L.R, dst, words), words, 0, in_oor ? *in_oor : none, slot_base, out_oor ? *out_oor : none,
              rowmap, route, rstride, in_oor ? slow : SlowList{nullptr, 0}, err};
    // a fused check (ver): the stored rows are the source regions', nothing
    // is written through dst, and the output buckets take the recomputed
    // rows' 65536 positions
    const VerArgs v = ver ? VerArgs{ver->checks, ver->value_mismatch, ver->first} : VerArgs{};
    if (ver && (!ver->checks || !ver->value_mismatch || !ver->first || !out_oor))
        return -1;
    const MatRoute r = matrix_route(route_in(a, ver != nullptr));
    const int rc = launch_route(r, a, S, st, v);
    if (rc || !r.redo)
        return rc;
    // the dot2 kernel's tiles with more marks than its LDS list (the matrix
    // cores redo theirs themselves): see push_slow_tile
    const int grid = (S + kRedoSpan - 1) / kRedoSpan;
    if (r.verify) {
        hipLaunchKernelGGL(matrix_redo_kernel_verify, dim3(grid), dim3(kBlock), 0, st, a, S, v);
        return hipGetLastError() == hipSuccess ? 0 : -2;
    }
    const auto redo = r.both ? &matrix_redo_kernel_both : &matrix_redo_kernel;
    hipLaunchKernelGGL(redo, dim3(grid), dim3(kBlock), 0, st, a, S);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
