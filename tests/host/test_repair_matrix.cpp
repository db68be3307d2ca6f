// Host-only driver for tests/test_repair_host.py: the repair matrix of a
// stripe from the library's own host math (lagrange_matrix, mode 1, eval =
// r^target), then packed by pack_row / pack_mf_dword and read back through
// mf_entry.  No GPU call.
//   usage: test_repair_matrix k n r R id_0 .. id_{k-1} target_0 .. target_{R-1}
//   prints R rows "M <k entries>", then per row "S <scale> <rscale> <rscale_mf>"
//   and "P <k entries read back from the operand tiles>"
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadiron_amd/csrc/matrix_pack.h"

namespace qi {
std::vector<uint32_t> lagrange_matrix(int k, uint32_t r, const uint32_t* ids, int mode,
                                      const uint32_t* eval, int R);
}

int main(int argc, char** argv)
{
    if (argc < 5)
        return 2;
    const int k = std::atoi(argv[1]);
    const uint32_t r = static_cast<uint32_t>(std::atoi(argv[3]));
    const int R = std::atoi(argv[4]);
    if (argc != 5 + k + R)
        return 2;
    std::vector<uint32_t> ids(k), ev(R);
    for (int i = 0; i < k; i++)
        ids[i] = static_cast<uint32_t>(std::atoi(argv[5 + i]));
    for (int j = 0; j < R; j++)
        ev[j] = qi::powmod_c(r, static_cast<uint32_t>(std::atoi(argv[5 + k + j])));
    const std::vector<uint32_t> M = qi::lagrange_matrix(k, r, ids.data(), 1, ev.data(), R);
    for (int j = 0; j < R; j++) {
        std::printf("M");
        for (int i = 0; i < k; i++)
            std::printf(" %u", M[static_cast<size_t>(j) * k + i]);
        std::printf("\n");
    }
    // the packing of a repair context: KP as matrix_kp(k) (matrix_route.h)
    int kp = 2;
    while (2 * kp < k)
        kp *= 2;
    const qi::MatLayout L{R, k, kp};
    std::vector<int32_t> blk(L.words(), 0);
    std::vector<uint32_t> scale(R);
    for (int j = 0; j < R; j++)
        scale[j] = qi::pack_row(M.data() + static_cast<size_t>(j) * k, L, j, blk.data());
    for (size_t d = 0; d < L.mf_words(); d++)
        blk[L.mf() + d] = qi::pack_mf_dword(L, blk.data() + L.plain(), d);
    for (int j = 0; j < R; j++) {
        std::printf("S %u %d %d\n", scale[j], blk[L.rscale() + j], blk[L.rscale_mf() + j]);
        std::printf("P");
        for (int i = 0; i < k; i++)
            std::printf(" %u", qi::mf_entry(L, blk.data() + L.mf(), j, i));
        std::printf("\n");
    }
    return 0;
}
