// syndrome_math.h -- the field formulas of the syndrome shares
// (qi_gpu_syndrome, qi_gpu_syndrome_locate), constexpr and shared by host and
// device on top of partial_math.h: no HIP, so
// tests/host/test_syndrome_math.cpp compiles it on its own.
//
// For the N = k + R listed fragments with points x_i = r^ids[i] and the dual
// weights w_i = prod_{l != i, l < N} (x_i - x_l) = A'(x_i) the syndromes of a
// received column y are (locate_math.h)
//   S_j = sum_i y_i x_i^j / w_i,   j < R,
// all 0 for a codeword.  They are linear in the rows: the holder of H of the N
// fragments forms sum_{h<H} c(j, held[h]) y_h with
//   c(j, i) = x_i^j / w_i,
// and the shares of any partition of the N positions add up modulo 65537 to
// the syndromes.  Only the weights of the held rows are needed: one N - 1 term
// product and one inversion per held position, then R - 1 multiplies by x_i --
// O(H N) for H held rows.  The resolve side (qi_gpu_syndrome_locate) needs all
// N points and weights, O(N^2), and no coefficient.
//
// Everything here is canonical, in [0, 65536].  A repeated id makes w_i = 0;
// the inverse of 0 is taken as 0, so every coefficient of such a row is 0.
#pragma once

#include <stdint.h>

#include "partial_math.h"

namespace qi {

constexpr int kSynMaxChecks = 8;  // QI_SYNDROME_MAX_CHECKS
constexpr int kSynMaxErrors = 4;  // QI_SYNDROME_MAX_ERRORS = kSynMaxChecks / 2

// prod * prod_{l < n, l != skip} (x - xs[l]): a stretch of w_skip = A'(x).
// Both context kernels call it once per staged chunk of points
constexpr uint32_t syndrome_weight(uint32_t prod, uint32_t x, const uint32_t* xs, int n, int skip)
{
    return partial_prod(prod, x, xs, n, skip);
}

// the rp coefficients of a held row at the point x with weight w: c[j] =
// balanced(x^j / w) for j < R, 0 above (and all 0 for w = 0)
constexpr void syndrome_coefs(uint32_t x, uint32_t w, int R, int rp, int32_t* c)
{
    uint32_t v = pm_inv(w);
    for (int j = 0; j < rp; j++) {
        c[j] = j < R ? partial_balanced(v) : 0;
        v = pm_mul(v, x);
    }
}

// int32 words of one stripe's share context: partial_ctx_words(H, R), the
// layout partial_kernel reads -- H x RP balanced coefficients (row h: c(j,
// held[h]), j < RP, the pad columns 0), RP filler words (0; a partial repair
// keeps its targets there), and the H fragment ids of the held rows (a
// systematic plan's data rows, id < k, have no bucket)
constexpr long long syndrome_ctx_words(int n_held, int n_checks)
{
    return partial_ctx_words(n_held, n_checks);
}

// R rounded up to the syndrome counts the resolve kernel is built for (the
// decoder of locate_multi_math.h takes RP / 2 as its largest bound)
constexpr int syndrome_locate_rp(int n_checks)
{
    return n_checks <= 2 ? 2 : n_checks <= 4 ? 4 : 8;
}

// int32 words of one stripe's resolve context: the N ids, the N points x_i
// and the N weights w_i (canonical) -- 12 N bytes
constexpr long long syndrome_locate_ctx_words(int n_listed)
{
    return 3LL * n_listed;
}

}  // namespace qi
