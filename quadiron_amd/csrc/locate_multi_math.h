// locate_multi_math.h -- the bounded-distance decoder of the multi-fragment
// locate (qi_gpu_locate_multi), on top of locate_math.h: from the R canonical
// syndromes of a column and the bound t it finds the nu <= t bad listed
// fragments and their errors.  No HIP is needed: tests/host/
// test_locate_multi_math.cpp compiles it on its own; under hipcc the same
// functions are host and device code.
//
// With nu bad fragments at the list positions p_a, off by e_a != 0, the
// syndromes are S_j = sum_a E_a x_(p_a)^j, E_a = e_a / w_(p_a): a linear
// recurrence of order nu whose characteristic polynomial is the locator
// sigma(z) = prod_a (z - x_(p_a)).  Berlekamp-Massey over all R syndromes
// gives the shortest recurrence, of order L.  L > t is rejected (L never
// shrinks, so at the step that raises it past t).  With L <= t, 2 L <= R: the
// recurrence reproduces every syndrome, so the R - 2 L surplus syndromes are
// guards with no code of their own, and it is the only one of its order.  The
// column is located when sigma has L distinct roots among the listed points:
// the x_i are distinct and not 0, so the S_j are then sum_a E_a x_a^j for all
// j < R with the E_a of lm_value, none of them 0 (a zero E_a would make a
// shorter recurrence).  Anything else is unlocated.
//
// b bad fragments, b <= t: located exactly.  t < b <= R - t: a recurrence of
// order <= t and the true one of order b would agree on R >= b + t terms, so
// they would be the same: always unlocated.  b > R - t: may be miscorrected.
//
// The update is the inverse-free one, C <- b C - d x^m B, so sigma comes out
// scaled by a non-zero constant c = C[0]: sigma(z) c = sum_i C[i] z^(L - i).
// Neither the root test nor the values need it monic: the values are a
// quotient in which c cancels, and the only inversion of a column is that
// quotient's (none at all for L = 1, where E = S_0).
#pragma once

#include <stdint.h>

#include "gf65537.h"
#include "locate_math.h"

namespace qi {

constexpr int kLocMaxErrors = 4;  // QI_LOCATE_MAX_ERRORS = kLocMaxChecks / 2

// a b mod q for canonical a, b in [0, 65536] through the balanced
// representatives: |ab bb| <= 2^30 is one 24-bit multiply, its fold is in
// [-16384, 81919], and one conditional + q and one - q make it canonical
QI_HD uint32_t lm_mul(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    int32_t v = fold(__mul24(balanced(a), balanced(b)));
#else
    int32_t v = fold(balanced(a) * balanced(b));
#endif
    v = v < 0 ? v + kQ : v;
    v = v >= kQ ? v - kQ : v;
    return static_cast<uint32_t>(v);
}

QI_HD uint32_t lm_add(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;
    return s >= 65537u ? s - 65537u : s;
}

// Berlekamp-Massey over S[0 .. R) with the order bounded by t <= TM: the order
// L of the shortest recurrence and its connection polynomial C[0 .. TM] (C[0]
// != 0, C[i] = 0 for i > L), sum_i C[i] S[n - i] = 0 for L <= n < R; -1 when
// L > t.  B is kept multiplied by x^m (shifted once per step): with L <= TM no
// coefficient of C or x^m B past TM is ever used, so TM + 1 words hold each,
// and every index below is a compile-time one.
template <int RP, int TM>
QI_HD int lm_berlekamp_massey(const uint32_t (&S)[RP], int R, int t, uint32_t (&C)[TM + 1])
{
    uint32_t B[TM + 1];
#pragma unroll
    for (int i = 0; i <= TM; i++)
        C[i] = B[i] = i == 0 ? 1u : 0u;
    uint32_t b = 1;
    int L = 0;
#pragma unroll
    for (int n = 0; n < RP; n++) {
        if (n >= R)
            break;
#pragma unroll
        for (int i = TM; i > 0; i--)
            B[i] = B[i - 1];
        B[0] = 0;
        uint32_t d = 0;
#pragma unroll
        for (int i = 0; i <= TM; i++)
            if (i <= n)
                d = lm_add(d, lm_mul(C[i], S[n - i]));
        if (d == 0)
            continue;
        const bool grow = 2 * L <= n;
        if (grow && n + 1 - L > t)
            return -1;
        const uint32_t nd = 65537u - d;  // d != 0
#pragma unroll
        for (int i = 0; i <= TM; i++) {
            const uint32_t c = C[i];
            C[i] = lm_add(lm_mul(b, c), lm_mul(nd, B[i]));
            B[i] = grow ? c : B[i];
        }
        if (grow) {
            L = n + 1 - L;
            b = d;
        }
    }
    return L;
}

// whether the listed point x is a root of sigma: Horner over all TM + 1
// coefficients gives x^(TM - L) sigma(x) c, and x is not 0
template <int TM>
QI_HD bool lm_is_root(const uint32_t (&C)[TM + 1], uint32_t x)
{
    uint32_t v = C[0];
#pragma unroll
    for (int i = 1; i <= TM; i++)
        v = lm_add(lm_mul(v, x), C[i]);
    return v == 0;
}

// E of the root x of sigma (order L >= 1).  g = sigma c / (z - x) by synthetic
// division, g(z) = sum_(i < L) g_i z^(L - 1 - i); sum_j S_j [z^j] g = sum_a
// E_a g(x_a) = E g(x), the other roots being roots of g.  sel(j) returns S[j]
// (the caller's choice of how to index its syndromes)
template <int TM, typename Sel>
QI_HD uint32_t lm_value(const uint32_t (&C)[TM + 1], int L, uint32_t x, Sel sel)
{
    if (L == 1)
        return sel(0);
    uint32_t g = 0, num = 0, den = 0;
#pragma unroll
    for (int i = 0; i < TM; i++) {
        if (i < L) {
            g = lm_add(lm_mul(g, x), C[i]);
            num = lm_add(num, lm_mul(g, sel(L - 1 - i)));
            den = lm_add(lm_mul(den, x), g);
        }
    }
    return lm_mul(num, invmod_c(den));  // den = g(x) != 0: the roots are distinct
}

// One column on the host (and the model of the kernel's epilogue): the
// syndromes S, the N listed points x and weights w, the restored symbols
// through y(i), data_row(i) whether position i is a systematic data row.
// kLocClean, kLocNone, or kLocFound with *nu positions pos[] (ascending) and
// corrected symbols v[]
template <int RP, typename Y, typename D>
inline LocClass lm_decode_column(const uint32_t (&S)[RP], int R, int t, const uint32_t* x,
                                 const uint32_t* w, int N, Y y, D data_row, int* nu,
                                 int (&pos)[kLocMaxErrors], uint32_t (&v)[kLocMaxErrors])
{
    constexpr int TM = RP / 2;
    uint32_t any = 0;
    for (int j = 0; j < RP; j++)
        any |= S[j];
    *nu = 0;
    if (!any)
        return kLocClean;
    uint32_t C[TM + 1];
    const int L = lm_berlekamp_massey<RP, TM>(S, R, t, C);
    if (L < 1)
        return kLocNone;
    int n = 0;
    for (int i = 0; i < N; i++)
        if (lm_is_root<TM>(C, x[i])) {
            if (n < kLocMaxErrors)
                pos[n] = i;
            n++;
        }
    if (n != L)
        return kLocNone;
    for (int a = 0; a < L; a++) {
        const uint32_t E = lm_value<TM>(C, L, x[pos[a]], [&](int j) { return S[j]; });
        if (E == 0 || !locate_fix(y(pos[a]), E, w[pos[a]], data_row(pos[a]), &v[a]))
            return kLocNone;
    }
    *nu = L;
    return kLocFound;
}

}  // namespace qi
