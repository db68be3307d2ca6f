// Host-only driver for tests/test_ntt_geom.py: the LDS engine's launch
// geometry (quadiron_amd/csrc/ntt_geom.h, compiled by plain g++) over every
// code the engine takes.  Exits nonzero at the first shape that breaks a rule;
// prints the (kernel, TWG, C2) forms that occur, one per line, then the
// number of geometries checked.
#include <algorithm>
#include <cstdio>
#include <set>
#include <string>

#include "../../quadiron_amd/csrc/ntt_geom.h"

using namespace qi;

static int bad(const char* what, int k, int n, int mode)
{
    std::fprintf(stderr, "%s: k=%d n=%d mode=%d\n", what, k, n, mode);
    return 1;
}

// radices <= 32 whose product is N, strides and table offsets consistent
static bool plan_ok(const XfPlan& P, int N)
{
    int bits = 0;
    for (int q = 0; q < P.np; q++) {
        if (P.lgr[q] < 1 || P.lgr[q] > 5)
            return false;
        bits += P.lgr[q];
        if (P.sh[q] != ilog2i(N) - bits)
            return false;
    }
    return P.N == N && P.np >= 1 && P.np <= kLdsMaxPasses && (1 << bits) == N;
}

// The LDS bytes of a launch, counted again from the kernels' own carving of
// the dynamic LDS (ntt.hip), not through lds_bytes / eras_bytes or the table
// layout.  Pass tables of an N-point transform: pass q holds L_q = N / (R_0
// ... R_{q-1}) words, each table padded to 4
static size_t table_words(int N)
{
    const int bits = ilog2i(N), np = std::max(1, (bits + 4) / 5);
    size_t w = 0;
    for (int q = 0, left = bits; q < np; q++) {
        w += ((size_t{1} << left) + 3) & ~size_t{3};
        left -= (left + (np - q) - 1) / (np - q);
    }
    return w;
}

static size_t image_words(int rows, int lgT)
{
    return static_cast<size_t>(rows + rows / 32) << lgT;  // one empty row after every 32
}

// ntt_lds_kernel: image nmax x T | tables | inv_A[k] | ids[k] | C[len_2k];
// twg: no tables, no C.  A decode stages INTT_n, NTT_h, INTT_h and the twist
// (2 h words), an encode NTT_n and the 32 inverse roots, systematic modes all
static size_t lds_bytes_again(int k, int n, int len2k, int mode, int lgT, bool twg)
{
    const int h = len2k / 2;
    const size_t dec = table_words(n) + 2 * table_words(h) + ((2 * h + 3) & ~3);
    const size_t enc = table_words(n) + 32;
    const size_t tw = mode == kLdsEnc ? enc : mode == kLdsDec ? dec : dec + enc;
    return 4 * (image_words(std::max(n, len2k), lgT) + 2 * k + (twg ? 0 : tw + len2k));
}

// ntt_eras_kernel: image n x T | INTT_n's tables | ids[k] | position map[n]
// (c2: e x T syndromes) | E[e] | B[e x e] | c_E[e x T] | 32 inverse roots
static size_t eras_bytes_again(int k, int n, int lgT, bool c2)
{
    const size_t e = n - k, T = size_t{1} << lgT;
    return 4 * (image_words(n, lgT) + table_words(n) + k + (c2 ? e * T : n) + e + e * e + e * T +
                32);
}

// again(lgT): the bytes of the reported form at another tile width
template <class Again>
static int check(const LdsGeom& g, int k, int n, int mode, Again again)
{
    if (g.lgT < 0)
        return bad("no geometry", k, n, mode);
    if (g.lgT < 3 || g.lgT > 6)
        return bad("tile width", k, n, mode);
    if (g.bytes != again(g.lgT))
        return bad("byte count", k, n, mode);
    if (g.bytes > kLdsCap)
        return bad("over a CU's LDS", k, n, mode);
    if ((g.bytes <= kLdsCap / 2) != g.two)
        return bad("two-workgroup form", k, n, mode);
    // the widest tile that fits: one column more per lane group would not
    if (g.two ? g.lgT < 6 && again(g.lgT + 1) <= kLdsCap / 2 : g.lgT != 3)
        return bad("not the widest tile", k, n, mode);
    return 0;
}

int main()
{
    std::set<std::string> forms;
    long checked = 0;
    auto form = [&](const char* kern, bool twg, bool c2) {
        forms.insert(std::string(kern) + " " + (twg ? "1" : "0") + " " + (c2 ? "1" : "0"));
    };
    for (int n = 512; n <= 2048; n *= 2)
        for (int k = 257; k < n; k++) {
            int len2k = 1;
            while (len2k < 2 * k)
                len2k *= 2;
            const LdsTables L = lds_table_layout(n, len2k);
            const int Ns[4] = {n, len2k / 2, len2k / 2, n};
            for (int t = 0; t < 4; t++)
                if (!plan_ok(L.pl[t], Ns[t]))
                    return bad("xf_plan", k, n, t);
            if (std::max(n, len2k) <= kLdsMaxN) {
                if (!lds_engine(k, n, len2k))
                    return bad("lds_engine", k, n, -1);
                for (int mode = kLdsEnc; mode <= kLdsSysDec; mode++) {
                    const LdsGeom g = lds_geom(k, n, len2k, mode);
                    if (check(g, k, n, mode, [&](int lg) {
                            return lds_bytes_again(k, n, len2k, mode, lg, g.twg);
                        }))
                        return 1;
                    // global tables only where the staged ones leave no
                    // room for a second workgroup even at 8 columns
                    if (g.twg && lds_bytes_again(k, n, len2k, mode, 3, false) <= kLdsCap / 2)
                        return bad("global tables although the staged ones fit", k, n, mode);
                    if (g.twg && !g.two)
                        return bad("global tables without a second workgroup", k, n, mode);
                    form("ntt_lds_kernel", g.twg, false);
                    checked++;
                }
            }
            if (eras_shape(k, n))
                for (int dec = 0; dec < 2; dec++) {
                    const LdsGeom g = eras_geom(k, n, len2k, dec == 1);
                    if (check(g, k, n, 4 + dec,
                              [&](int lg) { return eras_bytes_again(k, n, lg, g.c2); }))
                        return 1;
                    if (g.c2 != (dec == 1 && n <= 1024))
                        return bad("two-pass completion", k, n, 4 + dec);
                    // why ntt_eras_kernel has no global-table form: it would
                    // never gain the second workgroup
                    if (!g.two &&
                        eras_bytes_again(k, n, 3, g.c2) - 4 * table_words(n) <= kLdsCap / 2)
                        return bad("global tables would fit two workgroups", k, n, 4 + dec);
                    form("ntt_eras_kernel", false, g.c2);
                    checked++;
                }
        }
    for (const std::string& f : forms)
        std::printf("%s\n", f.c_str());
    std::printf("checked %ld\n", checked);
    return 0;
}
