// Host program for tests/test_fingerprint_host.py: the fragment fingerprint's
// arithmetic from quadiron_amd/csrc/fingerprint_math.h alone (no HIP, no
// device).  It runs a row three ways -- the header's 64-bit reference, and the
// steps of fingerprint.hip's lanes in both forms (columns 256 apart; 16-byte
// pieces of 8 adjacent columns), chunk by chunk, tile by tile and lane by lane
// as the kernel walks them, from the same tables -- and prints the F values of
// each.  Built with -fsanitize=undefined -DQI_HOST_CHECK: the header's range
// assertions are live.
//   test_fingerprint_math <words> <first_col> <F> <a b d>...   < symbols
// stdin: `words` little-endian u32 restored symbols in [0, 65536].
// stdout: "ref v..", "scalar v..", "vec v.." ("vec -" when first_col is no
// multiple of 8: the launcher never takes that form then).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadiron_amd/csrc/fingerprint_math.h"

using namespace qi;

static std::vector<uint32_t> run_lanes(bool vec, const std::vector<uint32_t>& y, long long first_col,
                                       const uint32_t* keys, int F)
{
    const int FP = fp_pad(F);
    const long long words = static_cast<long long>(y.size());
    const long long c2base = first_col >> 16, c2s = fp_c2_count(first_col, words);
    if (c2s > fp_c2_max(words))
        abort();
    // fingerprint_tab_kernel (dead keys 1, 1, 1) and the balanced a^i
    std::vector<uint32_t> key(3 * FP, 1u);
    for (int e = 0; e < 3 * F; e++)
        key[e] = keys[e];
    std::vector<uint32_t> tab(fp_tab_words(c2s, FP));
    for (long long e = 0; e < static_cast<long long>(tab.size()); e++)
        tab[e] = fp_tab_entry(&key[3 * (e % FP)], e / FP, c2base);
    std::vector<int32_t> ap(FP * kFpCols);
    for (int j = 0; j < FP; j++)
        for (int i = 0; i < kFpCols; i++)
            ap[j * kFpCols + i] = balanced(fp_powmod(key[3 * j], i));
    std::vector<uint32_t> out(F, 0);
    for (long long ch = 0; ch < fp_chunks(words); ch++) {
        const long long cbeg = ch * kFpChunk, abs0 = first_col + cbeg;
        std::vector<int32_t> hiw(kFpHi * FP);
        for (int e = 0; e < kFpHi * FP; e++)
            hiw[e] = fp_hi_weight(tab.data(), FP, e % FP, (abs0 >> 8) + e / FP, c2base, c2s);
        const long long left = (words - cbeg + kFpTile - 1) / kFpTile;
        const int nt = left < kFpChunkTiles ? static_cast<int>(left) : kFpChunkTiles;
        std::vector<uint64_t> sum(FP, 0);
        for (int tid = 0; tid < kFpBlock; tid++) {
            const FpLane ln = fp_lane(vec, static_cast<int>(abs0 & 255), tid);
            std::vector<int32_t> acc(FP, 0);
            for (int t = 0; t < nt; t++) {
                int32_t s[kFpCols];
                for (int i = 0; i < kFpCols; i++) {
                    const long long c = cbeg + static_cast<long long>(t) * kFpTile +
                                        (vec ? tid * kFpCols + i : i * kFpBlock + tid);
                    const uint32_t v = c < words ? y[c] : 0u;
                    s[i] = fp_sym(v & 0xffffu, v == 65536u);
                }
                for (int j = 0; j < FP; j++) {
                    if (vec) {
                        const int h = fp_hi_index(true, t, ln.hl, 0);
                        acc[j] = fp_step(acc[j], fp_rebalance(fp_piece(s, &ap[j * kFpCols])),
                                         hiw[h * FP + j]);
                    } else {
                        for (int i = 0; i < kFpCols; i++)
                            acc[j] = fp_step(acc[j], s[i],
                                             hiw[fp_hi_index(false, t, ln.hl, i) * FP + j]);
                    }
                }
            }
            for (int j = 0; j < FP; j++)
                sum[j] += fp_mulmod(fp_canon(acc[j]), tab[ln.a_row * FP + j]);
        }
        for (int j = 0; j < F; j++)
            out[j] = static_cast<uint32_t>((out[j] + sum[j]) % 65537u);
    }
    return out;
}

int main(int argc, char** argv)
{
    if (argc < 4)
        return 2;
    const long long words = atoll(argv[1]), first_col = atoll(argv[2]);
    const int F = atoi(argv[3]);
    if (F < 1 || F > kFpMaxKeys || argc != 4 + 3 * F || words < 1)
        return 2;
    uint32_t keys[3 * kFpMaxKeys];
    for (int e = 0; e < 3 * F; e++)
        keys[e] = static_cast<uint32_t>(atoll(argv[4 + e]));
    std::vector<uint32_t> y(words);
    if (fread(y.data(), 4, y.size(), stdin) != y.size())
        return 3;
    printf("ref");
    for (int j = 0; j < F; j++)
        printf(" %u", fingerprint_row([&](long long c) { return y[c]; }, words, first_col,
                                      keys + 3 * j));
    printf("\nscalar");
    for (uint32_t v : run_lanes(false, y, first_col, keys, F))
        printf(" %u", v);
    printf("\nvec");
    if (first_col % kFpCols == 0)
        for (uint32_t v : run_lanes(true, y, first_col, keys, F))
            printf(" %u", v);
    else
        printf(" -");
    printf("\n");
    return 0;
}
