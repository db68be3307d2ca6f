// partial_math.h -- the field formulas of a partial repair (qi_gpu_partial),
// constexpr and shared by host and device: no HIP, so
// tests/host/test_partial_math.cpp compiles it on its own.
//
// A repair from the k helpers x_l = r^ids[l] rebuilds target y_t = r^targets[t]
// as sum_i c(t, i) in[i] with the Lagrange weights
//   c(t, i) = A(y_t) / ((y_t - x_i) A'(x_i)),   A(x) = prod_{l<k} (x - x_l),
//   A'(x_i) = prod_{l != i} (x_i - x_l).
// Only the weights of the rows a call holds are needed: one k - 1 term product
// per held position, one k term product per target, one inversion per
// coefficient -- O((H + R) k) for H held rows and R targets, where the whole
// R x k matrix costs O(k^2).
//
// Everything here is canonical, in [0, 65536].  A repeated helper makes
// A'(x_i) = 0 and a target among the helpers A(y_t) = 0; the inverse of 0 is
// taken as 0 (0^65535), so such a coefficient is 0.
#pragma once

#include <stdint.h>

namespace qi {

// a b mod q for canonical a, b: with 2^16 = -1 and 2^32 = 1 the product p0 +
// p1 2^16 + p2 2^32 (p2 is 1 only for 65536 * 65536) reduces to p0 - p1 + p2
constexpr uint32_t pm_mul(uint32_t a, uint32_t b)
{
    const uint64_t p = static_cast<uint64_t>(a) * b;
    const int32_t v = static_cast<int32_t>(p & 0xffffu) -
                      static_cast<int32_t>((p >> 16) & 0xffffu) +
                      static_cast<int32_t>(p >> 32);  // [-65535, 65536]
    return static_cast<uint32_t>(v < 0 ? v + 65537 : v);
}

constexpr uint32_t pm_sub(uint32_t a, uint32_t b)
{
    return a >= b ? a - b : a + 65537u - b;
}

constexpr uint32_t pm_pow(uint32_t a, uint32_t e)
{
    uint32_t r = 1;
    while (e) {
        if (e & 1u)
            r = pm_mul(r, a);
        a = pm_mul(a, a);
        e >>= 1;
    }
    return r;
}

// 1 / a (0 for a = 0)
constexpr uint32_t pm_inv(uint32_t a)
{
    return pm_pow(a, 65535u);
}

// prod * prod_{l < n, l != skip} (x - xs[l]): a stretch of A(x) (skip < 0) or
// of A'(x_skip).  The context kernel calls it once per staged chunk of points
constexpr uint32_t partial_prod(uint32_t prod, uint32_t x, const uint32_t* xs, int n, int skip)
{
    for (int l = 0; l < n; l++)
        if (l != skip)
            prod = pm_mul(prod, pm_sub(x, xs[l]));
    return prod;
}

// c(t, i) from A(y_t), y_t, x_i and A'(x_i)
constexpr uint32_t partial_coef(uint32_t ay, uint32_t y, uint32_t x, uint32_t apx)
{
    return pm_mul(ay, pm_inv(pm_mul(pm_sub(y, x), apx)));
}

// balanced representative of a canonical residue, in [-32768, 32768]
constexpr int32_t partial_balanced(uint32_t c)
{
    return c > 32768u ? static_cast<int32_t>(c) - 65537 : static_cast<int32_t>(c);
}

// R rounded up to the target counts the kernel is built for
constexpr int partial_rp(int n_targets)
{
    return n_targets <= 1 ? 1 : n_targets <= 2 ? 2 : n_targets <= 4 ? 4 : 8;
}

// int32 words of one stripe's context: H x RP balanced coefficients (row h:
// the RP coefficients of held row h, the pad columns 0), the RP targets (pad
// 0), and the H helper ids of the held rows (a systematic plan's data rows,
// id < k, have no bucket)
constexpr long long partial_ctx_words(int n_held, int n_targets)
{
    const long long rp = partial_rp(n_targets);
    return static_cast<long long>(n_held) * rp + rp + n_held;
}

}  // namespace qi
