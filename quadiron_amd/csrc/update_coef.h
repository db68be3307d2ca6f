// update_coef.h -- the coefficients of a delta update (qi_gpu_update), host
// only: no HIP, so tests/host/test_update_coef.cpp compiles it on its own.
//
// Both code types are linear: when data row i moves by d = new - old, coded
// slot `slot` moves by c(slot, i) * d with
//   non-systematic  c = r^(slot * i)              (fragment f = sum_t d_t r^(f t))
//   systematic      c = l_i(y_j),  y_j = r^(k+j)  (l_i: Lagrange basis over
//                   x_l = r^l, l < k; slot j is parity j)
//                     = A(y_j) / ((y_j - x_i) A'(x_i)),  A(x) = prod_{l<k} (x - x_l)
// The systematic form needs two per-plan tables, A(y_j) for j < m and
// 1 / A'(x_i) for i < k.  Consecutive points differ by a factor r, which
// shifts the product by one term:
//   A(y_{j+1})  = r^k     A(y_j)  (y_j - r^-1) / (y_j - r^(k-1))
//   A'(x_{i+1}) = r^(k-1) A'(x_i) (x_i - r^-1) / (x_i - r^(k-1))
// so each table is one k-term product and then one step per entry.  Every
// divisor is a difference of two powers of r with distinct exponents below n
// (j + 1 < m <= n - k, i + 1 < k), so none is zero; the builder checks.
#pragma once

#include <stdint.h>

#include <vector>

#include "gf65537.h"

namespace qi {

inline uint32_t submod_c(uint32_t a, uint32_t b)
{
    return a >= b ? a - b : a + 65537u - b;
}

struct UpdateTables {
    std::vector<uint32_t> ay;   // A(y_j), j < m
    std::vector<uint32_t> iap;  // 1 / A'(x_i), i < k
};

// The tables of the systematic code (k, m) with root r of order n >= k + m.
// false when a divisor is zero (no valid code reaches that).
inline bool update_tables(int k, int m, uint32_t r, UpdateTables& t)
{
    const uint32_t rinv = invmod_c(r);
    const uint32_t rk1 = powmod_c(r, static_cast<uint32_t>(k - 1));  // r^(k-1) = x_{k-1}
    const uint32_t rk = mulmod_c(rk1, r);                            // r^k = y_0
    t.ay.assign(static_cast<size_t>(m), 0);
    t.iap.assign(static_cast<size_t>(k), 0);
    // A(y_0) and A'(x_0) term by term
    uint32_t a = 1, ap = 1, xl = 1;
    for (int l = 0; l < k; l++, xl = mulmod_c(xl, r)) {
        a = mulmod_c(a, submod_c(rk, xl));
        if (l)
            ap = mulmod_c(ap, submod_c(1u, xl));
    }
    uint32_t y = rk;
    for (int j = 0; j < m; j++, y = mulmod_c(y, r)) {
        t.ay[static_cast<size_t>(j)] = a;
        if (j + 1 == m)
            break;
        const uint32_t den = submod_c(y, rk1);
        if (den == 0)
            return false;
        a = mulmod_c(mulmod_c(a, rk), mulmod_c(submod_c(y, rinv), invmod_c(den)));
    }
    uint32_t x = 1;
    for (int i = 0; i < k; i++, x = mulmod_c(x, r)) {
        if (ap == 0)
            return false;
        t.iap[static_cast<size_t>(i)] = invmod_c(ap);
        if (i + 1 == k)
            break;
        const uint32_t den = submod_c(x, rk1);
        if (den == 0)
            return false;
        ap = mulmod_c(mulmod_c(ap, rk1), mulmod_c(submod_c(x, rinv), invmod_c(den)));
    }
    return true;
}

// c(slot, id), canonical, as update_ctx_kernel computes it on the device
inline uint32_t update_coef_sys(const UpdateTables& t, int k, uint32_t r, int slot, int id)
{
    const uint32_t y = powmod_c(r, static_cast<uint32_t>(k + slot));
    const uint32_t x = powmod_c(r, static_cast<uint32_t>(id));
    return mulmod_c(mulmod_c(t.ay[static_cast<size_t>(slot)], invmod_c(submod_c(y, x))),
                    t.iap[static_cast<size_t>(id)]);
}

inline uint32_t update_coef_nonsys(uint32_t r, int n, int slot, int id)
{
    const uint64_t e = static_cast<uint64_t>(slot) * static_cast<uint64_t>(id);
    return powmod_c(r, static_cast<uint32_t>(e % static_cast<uint64_t>(n)));
}

// U rounded up to the row counts the update kernel is built for
inline int update_up(int n_rows)
{
    return n_rows <= 1 ? 1 : n_rows <= 2 ? 2 : n_rows <= 4 ? 4 : 8;
}

// int32 words of one stripe's update context: R x UP balanced coefficients,
// the R slots, the UP ids (padded with 0)
inline long long update_ctx_words(int n_rows, int n_slots)
{
    const long long up = update_up(n_rows);
    return static_cast<long long>(n_slots) * up + n_slots + up;
}

}  // namespace qi
