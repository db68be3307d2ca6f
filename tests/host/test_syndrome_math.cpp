// Host program for tests/test_syndrome_host.py: the syndrome shares' host
// side, from quadiron_amd/csrc/syndrome_math.h and fec_stage.h alone (no HIP,
// no library).
//   test_syndrome_math <k> <m> <R>
// lists N = k + R fragments of a code of k + m drawn by a fixed generator and
// forms the coefficients c(j, i) = x_i^j / w_i the way syndrome_ctx_kernel
// forms them -- w_i as a product over the N points taken in chunks, one
// inversion per row, then multiplies by x_i -- and checks them against a
// brute-force product in plain 64-bit arithmetic, and as a parity check: sum_i
// c(j, i) P(x_i) = 0 for random polynomials P of degree below k.  Then
// stage::apply_deltas against a direct model: a delta that makes a coded
// symbol 65536 inserts a mark, one that leaves 65536 removes it, a data row
// that would reach 65536 and a mark list past its capacity refuse the whole
// patch.  Prints "OK"; exit status 1 on a mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../quadiron_amd/csrc/fec_stage.h"
#include "../../quadiron_amd/csrc/syndrome_math.h"

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

uint64_t g_seed = 12345;
uint64_t rnd()
{
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return g_seed >> 33;
}

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            std::fprintf(stderr, "line %d: %s\n", __LINE__, #c);   \
            return 1;                                              \
        }                                                          \
    } while (0)

using qi::Properties;
using qi::fec::FecType;
using qi::fec::LocateFix;
using qi::fec::stage::FragMap;

// a holder's rows as u16 words and as the byte rows apply_deltas takes
struct Holder {
    std::vector<int> ids;
    std::vector<std::vector<uint8_t>> mem;
    std::vector<uint8_t*> rows;
    std::vector<Properties> props;
    Holder(const std::vector<int>& f, size_t words) : ids(f), props(f.size())
    {
        for (size_t h = 0; h < f.size(); h++) {
            mem.emplace_back(words * 2);
            for (auto& b : mem.back())
                b = static_cast<uint8_t>(rnd());
        }
        for (auto& m : mem)
            rows.push_back(m.data());
    }
    uint32_t word(size_t h, size_t c) const { return mem[h][2 * c] | mem[h][2 * c + 1] << 8; }
    void set(size_t h, size_t c, uint32_t w)
    {
        mem[h][2 * c] = static_cast<uint8_t>(w & 0xff);
        mem[h][2 * c + 1] = static_cast<uint8_t>(w >> 8);
    }
    std::vector<size_t> marks(size_t h) const
    {
        std::vector<size_t> v;
        for (auto const& it : props[h].get_map())
            v.push_back(it.first);
        return v;
    }
};

int test_apply_deltas()
{
    const size_t words = 64;
    const FragMap sys(FecType::SYSTEMATIC, 4, 4), nsys(FecType::NON_SYSTEMATIC, 4, 16);
    // 1. a coded symbol becomes 65536 (a mark is inserted, the word is 0), one
    //    leaves 65536 (its mark is removed), a plain one changes; fixes for
    //    fragments held elsewhere are skipped
    {
        Holder hd({5, 1, 7}, words);  // parity 1, data row 1, parity 3
        hd.set(0, 10, 100);           // y = 100, e = 101 -> 65536
        hd.set(0, 20, 0);             // marked: y = 65536, e = 65536 -> 0
        hd.props[0].add(20, qi::OOR_MARK);
        hd.props[0].add(40, qi::OOR_MARK);  // stays
        hd.set(1, 3, 7);                    // data row: y = 7, e = 65530 -> 14
        hd.set(2, 63, 65535);               // y = 65535, e = 1 -> 65534
        const Holder before = hd;
        const std::vector<LocateFix> fx = {{10, 5, 101}, {20, 5, 65536}, {3, 1, 65530},
                                           {63, 7, 1},   {5, 6, 9},      {5, 0, 9}};
        CHECK(qi::fec::stage::apply_deltas(sys, hd.ids, hd.rows, hd.props, fx, 8) == 4);
        CHECK(hd.word(0, 10) == 0 && hd.word(0, 20) == 0 && hd.word(1, 3) == 14 &&
              hd.word(2, 63) == 65534);
        CHECK((hd.marks(0) == std::vector<size_t>{10, 40}));
        CHECK(hd.marks(1).empty() && hd.marks(2).empty());
        // nothing else moved
        for (size_t h = 0; h < 3; h++)
            for (size_t c = 0; c < words; c++) {
                const bool named = (h == 0 && (c == 10 || c == 20)) || (h == 1 && c == 3) ||
                                   (h == 2 && c == 63);
                CHECK(named || hd.word(h, c) == before.word(h, c));
            }
    }
    // 2. a data row reaching 65536 refuses the whole patch
    {
        Holder hd({2, 6}, words);
        hd.set(0, 9, 5);  // data row 2: y = 5, e = 6 -> 65536
        hd.set(1, 9, 5);
        const Holder before = hd;
        const std::vector<LocateFix> fx = {{9, 6, 1}, {9, 2, 6}};
        CHECK(qi::fec::stage::apply_deltas(sys, hd.ids, hd.rows, hd.props, fx, 8) == -1);
        CHECK(hd.mem == before.mem && hd.marks(0).empty() && hd.marks(1).empty());
    }
    // 3. a mark list past its capacity refuses the whole patch; at the
    //    capacity it goes through
    {
        Holder hd({3, 0}, words);  // non-systematic: both coded
        hd.props[0].add(1, qi::OOR_MARK);
        hd.set(0, 1, 0);
        hd.set(0, 2, 50);  // e = 51 -> 65536: a second mark
        hd.set(1, 2, 50);
        const Holder before = hd;
        const std::vector<LocateFix> fx = {{2, 0, 3}, {2, 3, 51}};
        CHECK(qi::fec::stage::apply_deltas(nsys, hd.ids, hd.rows, hd.props, fx, 1) == -1);
        CHECK(hd.mem == before.mem && hd.marks(0) == std::vector<size_t>{1} &&
              hd.marks(1).empty());
        CHECK(qi::fec::stage::apply_deltas(nsys, hd.ids, hd.rows, hd.props, fx, 2) == 2);
        CHECK((hd.marks(0) == std::vector<size_t>{1, 2}) && hd.word(0, 2) == 0 &&
              hd.word(1, 2) == 47);
    }
    // 4. random deltas against the model (y - e) mod q, marks as a set
    for (int round = 0; round < 50; round++) {
        Holder hd({9, 4, 11, 2}, words);
        std::vector<std::vector<uint32_t>> y(4, std::vector<uint32_t>(words));
        for (size_t h = 0; h < 4; h++) {
            for (size_t c = 0; c < words; c++)
                y[h][c] = hd.word(h, c);
            for (size_t c = h; c < words; c += 7 + h) {
                hd.set(h, c, 0);
                hd.props[h].add(c, qi::OOR_MARK);
                y[h][c] = 65536;
            }
        }
        std::vector<LocateFix> fx;
        for (size_t c = 0; c < words; c += 3) {
            const size_t h = rnd() % 4;
            // every third delta lands on 65536
            const uint32_t e = rnd() % 3 == 0 ? (y[h][c] + 1) % Q : 1 + rnd() % 65536;
            if (e == 0)
                continue;
            fx.push_back({static_cast<uint32_t>(c), hd.ids[h], e});
            y[h][c] = static_cast<uint32_t>((y[h][c] + Q - e) % Q);
        }
        CHECK(qi::fec::stage::apply_deltas(nsys, hd.ids, hd.rows, hd.props, fx, words) ==
              static_cast<long long>(fx.size()));
        for (size_t h = 0; h < 4; h++) {
            std::vector<size_t> want;
            for (size_t c = 0; c < words; c++) {
                CHECK(hd.word(h, c) == (y[h][c] & 0xffffu));
                if (y[h][c] == 65536)
                    want.push_back(c);
            }
            CHECK(hd.marks(h) == want);
        }
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    if (argc != 4)
        return 2;
    const int k = std::atoi(argv[1]), m = std::atoi(argv[2]), R = std::atoi(argv[3]);
    if (k < 1 || m < 1 || R < 1 || R > m || R > qi::kSynMaxChecks)
        return 2;
    const int N = k + R;
    const uint32_t n = ceil2(static_cast<uint32_t>(k + m));
    const uint32_t r = static_cast<uint32_t>(mpow(3, 65536 / n));

    // the N listed fragments: the head of a shuffle of 0 .. k + m
    std::vector<uint32_t> ids(static_cast<size_t>(k + m));
    for (size_t i = 0; i < ids.size(); i++)
        ids[i] = static_cast<uint32_t>(i);
    for (size_t i = ids.size() - 1; i > 0; i--)
        std::swap(ids[i], ids[rnd() % (i + 1)]);
    ids.resize(static_cast<size_t>(N));
    std::vector<uint32_t> xs(ids.size());
    for (size_t i = 0; i < ids.size(); i++)
        xs[i] = qi::pm_pow(r, ids[i]);

    // w_i in chunks of 1024 points, as the context kernels stage them
    constexpr int kChunk = 1024;
    const int rp = qi::partial_rp(R);
    std::vector<int32_t> coef(static_cast<size_t>(N) * rp);
    for (int i = 0; i < N; i++) {
        uint32_t w = 1;
        for (int l0 = 0; l0 < N; l0 += kChunk)
            w = qi::syndrome_weight(w, xs[i], xs.data() + l0, N - l0 < kChunk ? N - l0 : kChunk,
                                    i - l0);
        qi::syndrome_coefs(xs[i], w, R, rp, coef.data() + static_cast<size_t>(i) * rp);
        // brute force
        uint64_t den = 1;
        for (int l = 0; l < N; l++)
            if (l != i)
                den = den * ((xs[i] + Q - xs[l]) % Q) % Q;
        CHECK(den != 0 && den == w);
        const uint64_t iw = mpow(den, Q - 2);
        for (int j = 0; j < rp; j++) {
            const uint64_t want = j < R ? iw * mpow(xs[i], j) % Q : 0;
            const int32_t c = coef[static_cast<size_t>(i) * rp + j];
            CHECK(c >= -32768 && c <= 32768 && (c + static_cast<int64_t>(Q)) % Q == want);
        }
    }
    // a repeated point has weight 0 and all-zero coefficients
    {
        int32_t c[8];
        qi::syndrome_coefs(xs[0], 0, R, rp, c);
        for (int j = 0; j < rp; j++)
            CHECK(c[j] == 0);
    }
    // codewords: sum_i c(j, i) P(x_i) = 0 for deg P < k; and a polynomial of
    // degree k is no codeword for syndrome R - 1
    for (int round = 0; round < 3; round++) {
        std::vector<uint64_t> pc(static_cast<size_t>(k) + (round == 2 ? 1 : 0));
        for (auto& c : pc)
            c = 1 + rnd() % (Q - 1);
        std::vector<uint64_t> S(static_cast<size_t>(R), 0);
        for (int i = 0; i < N; i++) {
            uint64_t v = 0;
            for (size_t d = pc.size(); d-- > 0;)
                v = (v * xs[i] + pc[d]) % Q;
            for (int j = 0; j < R; j++) {
                const int64_t c = coef[static_cast<size_t>(i) * rp + j];
                S[j] = (S[j] + static_cast<uint64_t>((c + static_cast<int64_t>(Q)) % Q) * v) % Q;
            }
        }
        for (int j = 0; j < R; j++)
            CHECK(round == 2 ? (j < R - 1 ? S[j] == 0 : S[j] != 0) : S[j] == 0);
    }
    std::printf("W %lld %lld %lld %lld\n", qi::syndrome_ctx_words(1, 1), qi::syndrome_ctx_words(5, 3),
                qi::syndrome_ctx_words(N, R), qi::syndrome_locate_ctx_words(N));
    if (test_apply_deltas())
        return 1;
    std::printf("OK\n");
    return 0;
}
