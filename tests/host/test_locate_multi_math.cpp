// Host program for tests/test_locate_multi_host.py: the multi-fragment
// locate's decoder from quadiron_amd/csrc/locate_multi_math.h alone (no HIP,
// no library), in the form the kernel uses (RP = locate_rp(R), TM = RP / 2).
//   test_locate_multi_math <sys> <k> <m> <R> <t> <N> <ids...>   < columns
// stdin: one received column per line, the N restored symbols y_i in [0,
// 65536] in list order.  Per column one line
//   <class> <nu> <p0> <v0> <p1> <v1> <p2> <v2> <p3> <v3>  <class1> <pos1> <v1>
// class 0 clean, 1 located (nu positions, ascending, and corrected symbols;
// unused pairs -1 0), 2 unlocated; then locate_math.h's single-fragment
// verdict on the same column (locate_classify + locate_fix).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadiron_amd/csrc/locate_multi_math.h"

template <int RP>
static int run(int sys, int k, int R, int t, int N, const std::vector<int>& ids,
               const std::vector<uint32_t>& x, const std::vector<uint32_t>& w)
{
    std::vector<int32_t> coef(static_cast<size_t>(N) * RP);
    for (int i = 0; i < N; i++) {
        int32_t c[RP];
        qi::locate_coefs<RP>(x[i], qi::invmod_c(w[i]), R, c);
        for (int j = 0; j < RP; j++)
            coef[static_cast<size_t>(i) * RP + j] = c[j];
    }
    std::vector<uint32_t> y(N);
    for (;;) {
        for (int i = 0; i < N; i++)
            if (std::scanf("%u", &y[i]) != 1)
                return i == 0 ? 0 : 2;
        uint32_t S[RP];
        for (int j = 0; j < RP; j++) {
            int64_t acc = 0;
            for (int i = 0; i < N; i++)
                acc += static_cast<int64_t>(y[i]) * coef[static_cast<size_t>(i) * RP + j];
            S[j] = qi::canon(acc);
        }
        int nu = 0, pos[qi::kLocMaxErrors] = {-1, -1, -1, -1};
        uint32_t v[qi::kLocMaxErrors] = {0, 0, 0, 0};
        const int cls = qi::lm_decode_column<RP>(
            S, R, t, x.data(), w.data(), N, [&](int i) { return y[i]; },
            [&](int i) { return sys && ids[i] < k; }, &nu, pos, v);
        std::printf("%d %d", cls, cls == qi::kLocFound ? nu : 0);
        for (int a = 0; a < qi::kLocMaxErrors; a++)
            if (cls == qi::kLocFound && a < nu)
                std::printf(" %d %u", pos[a], v[a]);
            else
                std::printf(" -1 0");
        int p1 = -1;
        uint32_t v1 = 0;
        int c1 = qi::locate_classify<RP>(S, R, x.data(), N, &p1);
        if (c1 == qi::kLocFound && !qi::locate_fix(y[p1], S[0], w[p1], sys && ids[p1] < k, &v1))
            c1 = qi::kLocNone;
        if (c1 != qi::kLocFound) {
            p1 = -1;
            v1 = 0;
        }
        std::printf(" %d %d %u\n", c1, p1, v1);
    }
}

int main(int argc, char** argv)
{
    if (argc < 7)
        return 2;
    int a = 1;
    const int sys = std::atoi(argv[a++]), k = std::atoi(argv[a++]), m = std::atoi(argv[a++]);
    const int R = std::atoi(argv[a++]), t = std::atoi(argv[a++]), N = std::atoi(argv[a++]);
    if (N != k + R || argc < a + N || R < 2 || R > qi::kLocMaxChecks || t < 1 || 2 * t > R)
        return 2;
    std::vector<int> ids;
    for (int i = 0; i < N; i++)
        ids.push_back(std::atoi(argv[a++]));
    const uint32_t n = qi::ceil2(static_cast<uint32_t>(k + m));
    const uint32_t r = qi::root_of_unity(n);
    std::vector<uint32_t> x(N), w(N);
    for (int i = 0; i < N; i++)
        x[i] = qi::powmod_c(r, static_cast<uint32_t>(ids[i]));
    for (int i = 0; i < N; i++) {
        w[i] = qi::locate_weight(x.data(), N, i);
        if (w[i] == 0) {
            std::fprintf(stderr, "repeated point\n");
            return 1;
        }
    }
    switch (qi::locate_rp(R)) {
    case 2: return run<2>(sys, k, R, t, N, ids, x, w);
    case 4: return run<4>(sys, k, R, t, N, ids, x, w);
    default: return run<8>(sys, k, R, t, N, ids, x, w);
    }
}
