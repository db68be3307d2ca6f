// Host program for tests/test_partial_host.py: the partial repair's
// coefficients c(t, i) from quadiron_amd/csrc/partial_math.h alone (no HIP, no
// library), formed the way partial_ctx_kernel forms them -- A'(x_i) and A(y_t)
// as products over the k points taken in chunks, one inversion per
// coefficient -- and checked here against a brute-force Lagrange product in
// plain 64-bit arithmetic, and by interpolation: the sum over all k positions
// of c(t, i) P(x_i) must be P(y_t) for a polynomial P of degree below k.
//   test_partial_math <k> <m> <n_targets> <targets...> <ids... (k of them)>
// prints, per target, one line "C <target> <c(t, 0)> ... <c(t, k - 1)>", then
// "W ..." (context sizes) and "OK".  Exit status 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadiron_amd/csrc/partial_math.h"

namespace {

constexpr uint64_t Q = 65537;

uint64_t mpow(uint64_t a, uint64_t e)
{
    uint64_t r = 1;
    for (a %= Q; e; e >>= 1, a = a * a % Q)
        if (e & 1)
            r = r * a % Q;
    return r;
}

uint32_t ceil2(uint32_t n)
{
    uint32_t x = 1;
    while (x < n)
        x <<= 1;
    return x;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc < 4)
        return 2;
    int a = 1;
    const int k = std::atoi(argv[a++]), m = std::atoi(argv[a++]), R = std::atoi(argv[a++]);
    if (k < 1 || m < 1 || R < 1 || argc != a + R + k)
        return 2;
    std::vector<uint32_t> targets, ids;
    for (int t = 0; t < R; t++)
        targets.push_back(static_cast<uint32_t>(std::atoi(argv[a++])));
    for (int i = 0; i < k; i++)
        ids.push_back(static_cast<uint32_t>(std::atoi(argv[a++])));
    const uint32_t n = ceil2(static_cast<uint32_t>(k + m));
    const uint32_t r = static_cast<uint32_t>(mpow(3, 65536 / n));

    // the field primitives against plain arithmetic, at the edges
    const uint32_t edge[] = {0, 1, 2, 255, 256, 32767, 32768, 32769, 65535, 65536};
    for (uint32_t x : edge)
        for (uint32_t y : edge) {
            if (qi::pm_mul(x, y) != static_cast<uint64_t>(x) * y % Q ||
                qi::pm_sub(x, y) != (x + Q - y) % Q) {
                std::fprintf(stderr, "pm_mul / pm_sub at %u, %u\n", x, y);
                return 1;
            }
        }
    for (uint32_t x : edge)
        if (qi::pm_inv(x) != mpow(x, Q - 2) || qi::pm_pow(r, x) != mpow(r, x) ||
            qi::partial_balanced(x) != (x > 32768 ? static_cast<int>(x) - 65537 : static_cast<int>(x))) {
            std::fprintf(stderr, "pm_inv / pm_pow / balanced at %u\n", x);
            return 1;
        }

    std::vector<uint32_t> xs(static_cast<size_t>(k));
    for (int i = 0; i < k; i++)
        xs[static_cast<size_t>(i)] = qi::pm_pow(r, ids[static_cast<size_t>(i)]);
    // A'(x_i) and A(y_t) in chunks of 7 points, as the context kernel stages them
    constexpr int kChunk = 7;
    const auto product = [&](uint32_t x, int skip) {
        uint32_t prod = 1;
        for (int l0 = 0; l0 < k; l0 += kChunk)
            prod = qi::partial_prod(prod, x, xs.data() + l0, k - l0 < kChunk ? k - l0 : kChunk,
                                    skip - l0);
        return prod;
    };
    std::vector<uint32_t> apx(static_cast<size_t>(k));
    for (int i = 0; i < k; i++)
        apx[static_cast<size_t>(i)] = product(xs[static_cast<size_t>(i)], i);
    // P: coefficients from a fixed generator
    std::vector<uint64_t> pc(static_cast<size_t>(k));
    uint64_t seed = 12345;
    for (auto& c : pc) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        c = (seed >> 33) % Q;
    }
    const auto eval = [&](uint64_t x) {
        uint64_t v = 0;
        for (int j = k - 1; j >= 0; j--)
            v = (v * x + pc[static_cast<size_t>(j)]) % Q;
        return v;
    };
    for (int t = 0; t < R; t++) {
        const uint32_t y = qi::pm_pow(r, targets[static_cast<size_t>(t)]);
        const uint32_t ay = product(y, -1);
        std::printf("C %u", targets[static_cast<size_t>(t)]);
        uint64_t sum = 0;
        for (int i = 0; i < k; i++) {
            const uint32_t xi = xs[static_cast<size_t>(i)];
            const uint32_t c = qi::partial_coef(ay, y, xi, apx[static_cast<size_t>(i)]);
            // brute force: prod_{l != i} (y - x_l) / (x_i - x_l)
            uint64_t num = 1, den = 1;
            for (int l = 0; l < k; l++) {
                if (l == i)
                    continue;
                num = num * ((y + Q - xs[static_cast<size_t>(l)]) % Q) % Q;
                den = den * ((xi + Q - xs[static_cast<size_t>(l)]) % Q) % Q;
            }
            const uint64_t brute = num * mpow(den, Q - 2) % Q;
            if (c != brute) {
                std::fprintf(stderr, "c(%d, %d) = %u, brute force %llu\n", t, i, c,
                             static_cast<unsigned long long>(brute));
                return 1;
            }
            sum = (sum + static_cast<uint64_t>(c) * eval(xi)) % Q;
            std::printf(" %u", c);
        }
        std::printf("\n");
        if (sum != eval(y)) {
            std::fprintf(stderr, "target %d: sum %llu, P(y) %llu\n", t,
                         static_cast<unsigned long long>(sum),
                         static_cast<unsigned long long>(eval(y)));
            return 1;
        }
    }
    std::printf("W %lld %lld %lld %lld\n", qi::partial_ctx_words(1, 1), qi::partial_ctx_words(5, 3),
                qi::partial_ctx_words(16, 8), qi::partial_ctx_words(k, 2));
    std::printf("OK\n");
    return 0;
}
