// Which kernels a matrix launch runs (host only, no HIP: plain g++ compiles
// it, tests/host/test_matrix_route.cpp).  matrix_route is the one decision:
// launch_matrix dispatches on its result and matrix_kernel_names prints it,
// so the names a plan reports are the kernels that run.
#pragma once

#include <stdint.h>

#include <string>

#include "matrix_pack.h"  // MatLayout

namespace qi {

// columns per OOR route tile: a multiple of every block width (256*COLS);
// the matrix cores take whole tiles, the dot2 kernel the tail
constexpr int kRouteTile = 1024;

// Byte extent of a stripe's row region: `rows` rows of `words` u16 at row
// stride rs (elements), as a buffer resource takes it; 0 when the region does
// not fit a 31-bit range (or has no rows), which sends the launch to the flat
// kernels.  In 128 bits: a product past 2^63 must not wrap into the range
inline uint32_t row_extent(long long rows, long long rs, long long words)
{
    if (rows <= 0)
        return 0;
    const __int128 e = (static_cast<__int128>(rows - 1) * rs + words) * 2;
    return e > 0 && e < 0x7fffffffLL ? static_cast<uint32_t>(e) : 0;
}

// pair columns (KP) of the dot2 kernel's packed rows for kin inputs
inline int matrix_kp(int kin)
{
    const int pairs = (kin + 1) / 2;
    for (int kp = 2; kp <= 128; kp *= 2)
        if (pairs <= kp)
            return kp;
    if (2 * pairs <= kMatGenMaxKin + 1)
        return 256;  // 256 < k <= 384: matrix cores only (no dot2 tails)
    if (2 * pairs <= kMatMaxKin + 1)
        return 320;  // 384 < k <= 640: (the context layout's unused section)
    return -1;  // larger k runs the NTT path (ntt.hip)
}

// Block geometry by matrix shape (kRouteTile = 1024 must be a multiple of
// the block width):
//  - short matrices (RB < 4: decodes, k x k): 4 waves, each on its own super
//    tiles; 1024 columns at KS = 1 (35 KB LDS), 512 at KS = 2, 4 (one u16
//    column per lane at KS = 4 -- 256 columns -- slowed the cfg3 decode,
//    profiles/r1_ab_mfma_cols1.txt);
//  - tall ones (RB >= 4: encode generators): the waves split the row blocks
//    over the whole image.  8 waves over 256 columns (54 KB LDS: 2 blocks =
//    4 waves per SIMD instead of 2) measured slower on the 1024 x 64 cfg3
//    generator (1.37 vs 1.22 ms, gpurun_out r2f), so the block stays at 4
//    waves.

// operand-stationary kernel (KS >= 4): G row-block groups of 8 waves, C
// column ranges per stripe; about two blocks per CU over the launch
constexpr bool kMmOs = true;
constexpr long long kOsMaxTiles = 4096;  // tiles per block (slow-tile bitmask)

// operand-stationary geometry by shape: (WR row-block slots, RPW row blocks
// per wave); 0 = the per-launch kernel
struct OsGeom {
    int wr, rpw;
};
inline OsGeom os_geom(int KS, int RB, bool two)
{
    if (!kMmOs)
        return {0, 0};
    // KS = 16, 20, 24 with more than one block of 8 row blocks, one source
    // region: two row blocks per wave, so one group (k200, k256) or two
    // (k300, k384) stage each input tile instead of two or three (k200
    // decode 0.757 -> 0.66 ms, k300 0.704 -> 0.653, k256 0.30 -> 0.278,
    // k384 0.88 -> 0.83; encodes ~10 % faster).  The systematic decodes'
    // two regions too since their rows load once (round 6), but not at KS =
    // 24 (28 bytes of scratch); not at KS = 8 (k128 encode 0.725 -> 0.757
    // ms; gpurun_out/ab_r5k, ab_r5l)
    if ((KS == 16 || KS == 20 || (KS == 24 && !two)) && RB > 8)
        return {8, 2};
    // KS = 40 (384 < k <= 640, K chunks): one row block per wave (80
    // operand VGPRs), one or two source regions
    if (KS >= 8)
        return {8, 1};
    // KS = 4: the short decode matrices (2 super tiles per 128-column tile)
    // and up to 8 row blocks; the tall generators (RB = 64 at cfg3) stay on
    // matrix_mfma_kernel (os at 1 or 4 row blocks per wave: 1.48 / 1.37 vs
    // 1.05 ms, gpurun_out ab_os2 / ab_os3)
    if (KS == 4 && RB <= 8)
        return RB <= 4 ? OsGeom{4, 1} : OsGeom{8, 1};
    return {0, 0};
}

// The forms each family is built in (the launchers instantiate by these,
// matrix_route refuses by them).  Two source regions (the systematic
// decodes): not at KS = 24 with two row blocks per wave (28 bytes of scratch)
constexpr bool os_has_two(int KS, int RPW)
{
    return !(KS >= 24 && RPW == 2);
}
// input and output marks in one launch: what a repair reaches (at most 4 row
// blocks, k <= 256); the verify forms (the stored rows compared, not
// written) exist for the same shapes
constexpr bool os_has_both(int KS, int WR, int RPW)
{
    return (KS == 4 && WR == 4) || KS == 8 || (KS == 16 && RPW == 1);
}
constexpr bool mfma_has_both(int KS)
{
    return KS <= 2;
}

// every fact the choice reads
struct MatRouteIn {
    MatLayout L;
    long long words;
    bool buf;    // every row region inside a 31-bit buffer range
    int align;   // rows at offsets that are multiples of 4, 2 or 1 words
    bool in_marks, out_marks;  // OOR marks to restore / to record
    bool ids, route;           // per-stripe fragment ids / route tables
    bool two;                  // rows from two source regions
    bool verify = false;       // compare with the stored rows, store nothing
};

enum class MatCore { kNone, kOs, kGen, kMfma };

struct MatRoute {
    // whole kRouteTile tiles (the first wfull columns) on the matrix cores:
    // matrix_os_kernel<KS, WR, RPW, two>, gen_mfma_kernel<NST, NW> or
    // matrix_mfma_kernel<KS, NST, NW, RSPLIT>
    MatCore core = MatCore::kNone;
    int KS = 0, WR = 0, RPW = 0, NST = 0, NW = 0;
    bool two = false, RSPLIT = false;
    long long wfull = 0;
    // the _both forms (input and output marks), of every kernel of the route
    bool both = false;
    // matrix_kernel<KP, COLS, BUF> over the other columns, then
    // matrix_redo_kernel over its slow tiles
    bool tail = false;
    int KP = 0, COLS = 0;
    bool BUF = false;
    bool redo = false;
    // the _verify forms, of every kernel of the route (a fused check: the
    // shapes of `both`)
    bool verify = false;
    // -1: the library has no such matrix-core kernel (nothing is launched);
    // -3: none for the tail (the matrix cores, if any, still run first)
    int err = 0;
};

inline MatRoute matrix_route(const MatRouteIn& in)
{
    MatRoute r;
    const int KS = in.L.KS(), RB = in.L.RB();
    r.verify = in.verify;
    r.both = !in.verify && in.in_marks && in.out_marks;
    const bool marks2 = r.both || r.verify;  // the forms of os_has_both
    r.wfull = in.words / kRouteTile * kRouteTile;
    if (KS > 0 && in.buf && in.align == 4 && r.wfull > 0) {
        r.KS = KS;
        const OsGeom og = os_geom(KS, RB, in.two);
        if (og.wr) {
            r.core = MatCore::kOs;
            r.WR = og.wr;
            r.RPW = og.rpw;
            r.two = in.two;
            if ((marks2 && !os_has_both(KS, og.wr, og.rpw)) || (in.two && !os_has_two(KS, og.rpw)))
                r.err = -1;
        } else if (KS == 4 && RB >= 4 && !in.in_marks && !in.route && !in.ids && !in.two &&
                   !in.verify) {
            // a tall generator over one source region (every encode): the
            // lean generator kernel
            r.core = MatCore::kGen;
            r.NST = 8;
            r.NW = 4;
        } else {
            // KS = 16: a 512-row byte-plane image of 64 columns (41 KB); 8
            // waves over 128 columns (94 KB) measured the same at k200 / k256
            // (profiles/r2_ab_round2b.txt).  KS = 8: a 256-row image of 256
            // columns, the waves always splitting the row blocks (81 KB with
            // the staging tiles; 128 columns measured 5 % slower at k128)
            r.core = MatCore::kMfma;
            r.NST = KS == 1 ? 16 : KS == 8 ? 4 : KS == 16 ? 1 : 8;
            r.NW = 4;
            r.RSPLIT = KS == 8 || KS == 16 || RB >= 4;
            // only the operand-stationary kernel takes kin > 256
            if (KS > 16 || (marks2 && !mfma_has_both(KS)))
                r.err = -1;
        }
    } else {
        r.wfull = 0;
    }
    // the tail, and everything the matrix cores do not take, on the dot2
    // kernel.  Columns per lane: 4 (b64 row loads) while the packed rows fit
    // in registers, 2 up to KP 16, else 1; 1 is also the flat path
    r.tail = r.wfull < in.words;
    if (r.tail) {
        r.KP = in.L.KP;
        r.BUF = in.buf;
        r.COLS = !in.buf ? 1 : r.KP <= 8 && in.align == 4 ? 4 : r.KP <= 16 && in.align >= 2 ? 2 : 1;
        // its slow tiles (the matrix cores redo their own)
        r.redo = in.in_marks;
        if (!r.err && (r.KP < 2 || r.KP > 128 || (r.KP & (r.KP - 1))))
            r.err = -3;
    }
    return r;
}

// spelled as the demangler (and rocprofv3) spells the instantiations
inline std::string to_string(const MatRoute& r)
{
    const std::string sfx = r.verify ? "_verify" : r.both ? "_both" : "";
    auto tf = [](bool b) { return std::string(b ? "true" : "false"); };
    auto n = [](int v) { return std::to_string(v); };
    std::string s;
    if (r.core == MatCore::kOs)
        s = "matrix_os_kernel" + sfx + "<" + n(r.KS) + ", " + n(r.WR) + ", " + n(r.RPW) + ", " +
            tf(r.two) + ">";
    else if (r.core == MatCore::kGen)
        s = "gen_mfma_kernel<" + n(r.NST) + ", " + n(r.NW) + ">";
    else if (r.core == MatCore::kMfma)
        s = "matrix_mfma_kernel" + sfx + "<" + n(r.KS) + ", " + n(r.NST) + ", " + n(r.NW) + ", " +
            tf(r.RSPLIT) + ">";
    if (r.tail) {
        s += std::string(s.empty() ? "" : " + ") + "matrix_kernel" + sfx + "<" + n(r.KP) + ", " +
             n(r.COLS) + ", " + tf(r.BUF) + "> (tail)";
        if (r.redo)
            s += " + matrix_redo_kernel" + sfx;
    }
    return s;
}

}  // namespace qi
