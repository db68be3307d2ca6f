// Geometry of the LDS-resident NTT engine (ntt.hip: ntt_lds_kernel and
// ntt_eras_kernel), host only apart from prow: the pass plan of a transform,
// where its twiddle tables sit, the LDS bytes of a tile and the tile width
// chosen from them (plain g++ compiles it, tests/host/test_ntt_geom.cpp).
// The launchers size their launches by lds_geom / eras_geom and
// ntt_kernel_names prints the same result, so the instantiation a plan
// reports is the one that runs.
#pragma once

#include <stddef.h>

#include <algorithm>

#include "gf65537.h"  // QI_HD

namespace qi {

constexpr int kLdsMaxN = 2048;   // largest transform of the LDS engine
constexpr int kLdsMaxPasses = 6;
constexpr int kErasMax = 64;     // most erasures of the erasure decode
constexpr size_t kLdsCap = 160 * 1024;  // LDS per CU

struct XfPlan {
    int N, np;
    int lgr[kLdsMaxPasses];  // log2 radix of pass q
    int sh[kLdsMaxPasses];   // log2 s_q = log2(N / (R_0 ... R_q))
    int tw[kLdsMaxPasses];   // pass q's twiddles in the LDS table: entry
                             // j R_q + u = w_{L_q}^{+-j u}, j < s_q
};

// Image row of transform position p: one empty row after every 32.  A
// wave holds 64 / T tasks of a pass; in the short-stride passes (the unit
// pass: 32 consecutive positions per task) those tasks sat 32 T words
// apart, i.e. on the same banks (k1000 encode: 72 % of the LDS cycles were
// bank conflicts); one row per 32 moves task tt by tt T banks.  A pass
// task's positions b + j + q s (b a multiple of 32 or the task inside one
// aligned 32-block, j < s) never carry into bit 5, so
// prow(b + j + q s) = prow(b + j) + prow(q s): a per-task base plus a
// per-q uniform offset, as before.
QI_HD int prow(int p)
{
    return p + (p >> 5);
}

inline int ilog2i(long long v)
{
    int l = 0;
    while ((1LL << l) < v)
        l++;
    return l;
}

// radices <= 32 for the LDS passes, as even as possible (fewest twiddled
// passes; 2048: 16, 16, 8).  Round 6 tried the radix-32 unit pass the
// image's row padding keeps conflict-free (2048: 8, 8, 32; the k600 encode
// had 58 % of its LDS cycles in bank conflicts): 2.06-2.09 -> 2.17-2.26 ms,
// the radix-8 passes cost more than the conflicts
// (profiles/r6_ab_notes.txt), so the plan stays
inline XfPlan xf_plan(int N)
{
    XfPlan P{};
    P.N = N;
    const int bits = ilog2i(N);
    P.np = std::max(1, (bits + 4) / 5);
    int left = bits, sh = bits;
    for (int q = 0; q < P.np; q++) {
        const int b = (left + (P.np - q) - 1) / (P.np - q);
        P.lgr[q] = b;
        sh -= b;
        P.sh[q] = sh;
        left -= b;
    }
    return P;
}

enum : int { kLdsEnc = 0, kLdsSysEnc = 1, kLdsDec = 2, kLdsSysDec = 3 };

inline int lds_mode(bool sys, bool decode)
{
    return decode ? (sys ? kLdsSysDec : kLdsDec) : (sys ? kLdsSysEnc : kLdsEnc);
}

// The four transforms' pass twiddle tables, back to back (offsets kept 4-
// aligned for the vector LDS reads): pass q of a length-N transform holds
// w_{L_q}^{+-j u} at j R_q + u, L_q = R_q s_q.  Order INTT_n, NTT_2k,
// INTT_2k, NTT_n (NTT_2k / INTT_2k as h = len_2k / 2 point transforms): a
// decode stages the first three, a non-systematic encode the last one,
// systematic codes all four.  Before NTT_n's, the decode's twist w2k^t, then
// w2k^-t (t < h); behind everything w_32^-x, x < 32 (the erasure decode's
// inverse roots).  ntt.hip's lds_tables fills the table by this layout
enum : int { kTwPni = 0, kTwP2f = 1, kTwP2i = 2, kTwPnf = 3 };

struct LdsTables {
    XfPlan pl[4];
    int twist, rinv, words;
};

inline LdsTables lds_table_layout(int n, int len2k)
{
    LdsTables L{};
    const int h = len2k / 2;
    const int Ns[4] = {n, h, h, n};
    int off = 0;
    for (int t = 0; t < 4; t++) {
        if (t == kTwPnf) {
            L.twist = off;
            off += (2 * h + 3) & ~3;
        }
        L.pl[t] = xf_plan(Ns[t]);
        for (int q = 0; q < L.pl[t].np; q++) {
            L.pl[t].tw[q] = off;
            off += ((1 << (L.pl[t].lgr[q] + L.pl[t].sh[q])) + 3) & ~3;
        }
    }
    L.rinv = off;
    L.words = off + 32;
    return L;
}

// the table range [lo, hi) a mode of ntt_lds_kernel stages
inline void lds_table_range(int n, int len2k, int mode, int* lo, int* hi)
{
    const LdsTables L = lds_table_layout(n, len2k);
    *lo = mode == kLdsEnc ? L.pl[kTwPnf].tw[0] : 0;
    *hi = mode == kLdsDec ? L.pl[kTwPnf].tw[0] : L.words;
}

// ntt_lds_kernel's side arrays behind the image (int32 words): inv_A and the
// ids, and unless twg the pass tables and C
inline int lds_side_words(int tw_words, int k, int len2k, bool twg)
{
    return twg ? 2 * k : tw_words + 2 * k + len2k;
}

// the image has nmax = max(n, len_2k) rows in every mode
inline size_t lds_bytes(int k, int n, int len2k, int lgT, int tw_words, bool twg)
{
    return ((static_cast<size_t>(prow(std::max(n, len2k))) << lgT) +
            lds_side_words(tw_words, k, len2k, twg)) *
           4;
}

// What a launch of either kernel is sized by.  lgT: log2 of the tile's
// columns, -1 when not even 8 columns fit a CU; two: two workgroups fit a CU;
// twg (ntt_lds_kernel): the tables and C are read from global memory; c2
// (ntt_eras_kernel): the two-pass completion
struct LdsGeom {
    int lgT;
    bool two, twg, c2;
    int tw_lo, tw_words;  // the staged range of the tables
    size_t bytes;
};

// columns per workgroup: the widest tile (<= 64 columns) that leaves room
// for two workgroups per CU with the tables staged, else with the tables
// read from global memory, else one workgroup per CU (at least 8 columns)
inline LdsGeom lds_geom(int k, int n, int len2k, int mode)
{
    LdsGeom g{};
    int hi;
    lds_table_range(n, len2k, mode, &g.tw_lo, &hi);
    g.tw_words = hi - g.tw_lo;
    for (int twg = 0; twg < 2; twg++)
        for (int lg = 6; lg >= 3; lg--) {
            g.bytes = lds_bytes(k, n, len2k, lg, g.tw_words, twg == 1);
            if (g.bytes <= kLdsCap / 2) {
                g.lgT = lg;
                g.two = true;
                g.twg = twg == 1;
                return g;
            }
        }
    g.bytes = lds_bytes(k, n, len2k, 3, g.tw_words, false);
    g.lgT = g.bytes <= kLdsCap ? 3 : -1;
    return g;
}

inline bool lds_engine(int k, int n, int len2k)
{
    // (the systematic decode stages the largest set)
    return std::max(n, len2k) <= kLdsMaxN && lds_geom(k, n, len2k, kLdsSysDec).lgT >= 0;
}

// ---- erasure decode (ntt_eras_kernel) ----
inline bool eras_shape(int k, int n)
{
    return n <= kLdsMaxN && n - k <= kErasMax;
}

// image n x T, INTT_n's tables, ids, the position map (c2: the e x T
// syndromes in its place), E, B, c_E (e x T) and w_32^-x
inline size_t eras_bytes(int k, int n, int lgT, int tw_words, bool c2)
{
    const size_t e = static_cast<size_t>(n - k);
    const size_t posw = c2 ? e << lgT : static_cast<size_t>(n);
    return ((static_cast<size_t>(prow(n)) << lgT) + tw_words + k + posw + e + e * e +
            (e << lgT) + 32) *
           4;
}

// Tile width at two workgroups per CU, else one.  dec: a non-systematic
// decode, which takes the two-pass completion (ntt_eras_kernel<true>) when
// INTT_n has two passes: it reads no position map.  The tables (INTT_n's
// only: [0, NTT_h's first table)) are always staged: wherever they keep a
// second workgroup off the CU (n = 2048), the rest alone does too
// (tests/host/test_ntt_geom.cpp checks every erasure shape)
inline LdsGeom eras_geom(int k, int n, int len2k, bool dec)
{
    const LdsTables L = lds_table_layout(n, len2k);
    LdsGeom g{};
    g.tw_words = L.pl[kTwP2f].tw[0];
    g.c2 = dec && L.pl[kTwPni].np == 2;
    for (int lg = 6; lg >= 3; lg--) {
        g.bytes = eras_bytes(k, n, lg, g.tw_words, g.c2);
        if (g.bytes <= kLdsCap / 2) {
            g.lgT = lg;
            g.two = true;
            return g;
        }
    }
    g.lgT = g.bytes <= kLdsCap ? 3 : -1;
    return g;
}

}  // namespace qi
