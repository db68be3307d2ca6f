// Host program for tests/test_locate_host.py: the fragment locate's field
// arithmetic from quadiron_amd/csrc/locate_math.h alone (no HIP, no library).
//   test_locate_math <sys> <k> <m> <R> <N> <ids...>   < columns
// stdin: one received column per line, the N restored symbols y_i in [0,
// 65536] in list order.  Prints "W <context words>" and per column one line
// "<class> <pos> <v>": class 0 clean, 1 located (position and corrected
// symbol), 2 unlocated (pos -1, v 0).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadiron_amd/csrc/locate_math.h"

int main(int argc, char** argv)
{
    if (argc < 6)
        return 2;
    int a = 1;
    const int sys = std::atoi(argv[a++]), k = std::atoi(argv[a++]), m = std::atoi(argv[a++]);
    const int R = std::atoi(argv[a++]), N = std::atoi(argv[a++]);
    if (N != k + R || argc < a + N)
        return 2;
    std::vector<int> ids;
    for (int i = 0; i < N; i++)
        ids.push_back(std::atoi(argv[a++]));
    const uint32_t n = qi::ceil2(static_cast<uint32_t>(k + m));
    const uint32_t r = qi::root_of_unity(n);
    std::vector<uint32_t> x(N), w(N);
    std::vector<int32_t> coef(static_cast<size_t>(N) * 8);
    for (int i = 0; i < N; i++)
        x[i] = qi::powmod_c(r, static_cast<uint32_t>(ids[i]));
    for (int i = 0; i < N; i++) {
        w[i] = qi::locate_weight(x.data(), N, i);
        if (w[i] == 0) {
            std::fprintf(stderr, "repeated point\n");
            return 1;
        }
        int32_t c[8];
        qi::locate_coefs<8>(x[i], qi::invmod_c(w[i]), R, c);
        for (int j = 0; j < 8; j++)
            coef[static_cast<size_t>(i) * 8 + j] = c[j];
    }
    std::printf("W %lld\n", qi::locate_ctx_words(k, R));
    std::vector<uint32_t> y(N);
    for (;;) {
        for (int i = 0; i < N; i++)
            if (std::scanf("%u", &y[i]) != 1)
                return i == 0 ? 0 : 2;
        uint32_t S[8];
        for (int j = 0; j < 8; j++) {
            int64_t acc = 0;
            for (int i = 0; i < N; i++)
                acc += static_cast<int64_t>(y[i]) * coef[static_cast<size_t>(i) * 8 + j];
            S[j] = qi::canon(acc);
        }
        int pos = -1;
        uint32_t v = 0;
        int cls = qi::locate_classify<8>(S, R, x.data(), N, &pos);
        if (cls == qi::kLocFound &&
            !qi::locate_fix(y[pos], S[0], w[pos], sys && ids[pos] < k, &v))
            cls = qi::kLocNone;
        if (cls != qi::kLocFound) {
            pos = -1;
            v = 0;
        }
        std::printf("%d %d %u\n", cls, pos, v);
    }
}
