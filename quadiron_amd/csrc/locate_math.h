// locate_math.h -- the field arithmetic of the fragment locate (qi_gpu_locate):
// the dual weights, the syndrome coefficients and the classify step, shared by
// the context kernel, the apply kernel (locate.hip) and the host.  No HIP is
// needed: tests/host/test_locate_math.cpp compiles it on its own; under hipcc
// the same functions are host and device code (gf65537.h's constexpr
// arithmetic is both).
//
// Fragment f of a column is P(r^f) with deg P < k in both code types.  For
// N = k + R distinct listed fragments with points x_i = r^(f_i) and the dual
// weights w_i = prod_{l != i} (x_i - x_l) = A'(x_i), the syndromes of a
// received column y are
//   S_j = sum_i y_i x_i^j / w_i,   j < R.
// sum_i g(x_i) / w_i is the coefficient of x^(N-1) of the interpolant of g
// through the N points, and g = x^j P has degree j + k - 1 <= N - 2: all R
// syndromes of a codeword are 0.  One fragment p off by e != 0 gives S_j =
// (e / w_p) x_p^j: S_0 != 0, S_1 / S_0 = x_p names the fragment, S_0 w_p = e
// is the error, and S_j = x_p S_(j-1), 2 <= j < R, are R - 2 guard equations.
// The code over the N listed points has minimum distance R + 1, so a column
// with 2 .. R - 1 bad fragments is never within distance 1 of another
// codeword: it fails a guard (or names no listed point) and is unlocated,
// never misattributed.  R = 2 has no guard: two bad fragments may pass as one.
#pragma once

#include <stdint.h>

#include "gf65537.h"

namespace qi {

constexpr int kLocMaxChecks = 8;  // QI_LOCATE_MAX_CHECKS
constexpr int kLocMaxK = 256;

// R rounded up to the syndrome counts the apply kernel is built for
QI_HD int locate_rp(int n_checks)
{
    return n_checks <= 2 ? 2 : n_checks <= 4 ? 4 : 8;
}

// int32 words of one stripe's locate context, N = k + R listed fragments: the
// N ids, the N points x_i, the N weights w_i (canonical), then N x RP balanced
// coefficients x_i^j / w_i, fragment-major (the rows j >= R are 0)
QI_HD long long locate_ctx_words(int k, int n_checks)
{
    const long long N = static_cast<long long>(k) + n_checks;
    return N * (3 + locate_rp(n_checks));
}

QI_HD uint32_t locate_sub(uint32_t a, uint32_t b)
{
    return a >= b ? a - b : a + 65537u - b;
}

// w_i = prod_{l != i} (x_i - x_l) over the N canonical points x; 0 exactly
// when x_i is repeated
QI_HD uint32_t locate_weight(const uint32_t* x, int N, int i)
{
    uint32_t w = 1;
    const uint32_t xi = x[i];
    for (int l = 0; l < N; l++)
        if (l != i)
            w = mulmod_c(w, locate_sub(xi, x[l]));
    return w;
}

// the RP coefficients of fragment i, c[j] = balanced(x_i^j / w_i) for j < R
// and 0 above; iw = 1 / w_i
template <int RP>
QI_HD void locate_coefs(uint32_t xi, uint32_t iw, int R, int32_t (&c)[RP])
{
    uint32_t v = iw;
#pragma unroll
    for (int j = 0; j < RP; j++) {
        c[j] = j < R ? balanced(v) : 0;
        v = mulmod_c(v, xi);
    }
}

enum LocClass { kLocClean = 0, kLocFound = 1, kLocNone = 2 };

// The syndromes S (canonical, S[j] = 0 for j >= R) of one column against the
// N listed points x: clean, one bad fragment (*pos its position in the list)
// or unlocated.  A found column still has to pass locate_fix.
template <int RP>
QI_HD LocClass locate_classify(const uint32_t (&S)[RP], int R, const uint32_t* x, int N, int* pos)
{
    uint32_t any = 0;
#pragma unroll
    for (int j = 0; j < RP; j++)
        any |= S[j];
    if (!any)
        return kLocClean;
    if (S[0] == 0)
        return kLocNone;
    const uint32_t xr = mulmod_c(S[1], invmod_c(S[0]));
    bool ok = true;
#pragma unroll
    for (int j = 2; j < RP; j++)
        if (j < R && S[j] != mulmod_c(xr, S[j - 1]))
            ok = false;
    if (!ok)
        return kLocNone;
    for (int i = 0; i < N; i++)
        if (x[i] == xr) {
            *pos = i;
            return kLocFound;
        }
    return kLocNone;
}

// The corrected symbol v = y - S_0 w_p in [0, 65536] of the found fragment,
// from its restored symbol y; false when it cannot be stored: 65536 on a
// systematic data row, which carries no marks
QI_HD bool locate_fix(uint32_t y, uint32_t S0, uint32_t wp, bool data_row, uint32_t* v)
{
    *v = locate_sub(y % 65537u, mulmod_c(S0, wp));
    return !(data_row && *v == 65536u);
}

}  // namespace qi
