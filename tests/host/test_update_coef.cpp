// Host program for tests/test_update_host.py: the delta update's
// coefficients c(slot, id) from quadiron_amd/csrc/update_coef.h alone (no
// HIP, no library), printed for the test to compare with the oracle's
// generator.
//   test_update_coef <sys> <k> <m> <n_ids> <ids...> <n_slots> <slots...>
// prints, per slot, one line "C <slot> <c(slot, ids[0])> <c(slot, ids[1])> ...",
// and for a systematic code "T <m> <k>" after the tables were built.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadiron_amd/csrc/update_coef.h"

int main(int argc, char** argv)
{
    if (argc < 6)
        return 2;
    int a = 1;
    const int sys = std::atoi(argv[a++]), k = std::atoi(argv[a++]), m = std::atoi(argv[a++]);
    const int nid = std::atoi(argv[a++]);
    if (argc < a + nid + 1)
        return 2;
    std::vector<int> ids;
    for (int i = 0; i < nid; i++)
        ids.push_back(std::atoi(argv[a++]));
    const int ns = std::atoi(argv[a++]);
    if (argc < a + ns)
        return 2;
    std::vector<int> slots;
    for (int i = 0; i < ns; i++)
        slots.push_back(std::atoi(argv[a++]));
    const int n = static_cast<int>(qi::ceil2(static_cast<uint32_t>(k + m)));
    const uint32_t r = qi::root_of_unity(static_cast<uint32_t>(n));
    qi::UpdateTables t;
    if (sys) {
        if (!qi::update_tables(k, m, r, t)) {
            std::fprintf(stderr, "update_tables: zero divisor\n");
            return 1;
        }
        std::printf("T %zu %zu\n", t.ay.size(), t.iap.size());
    }
    for (int s : slots) {
        std::printf("C %d", s);
        for (int i : ids)
            std::printf(" %u", sys ? qi::update_coef_sys(t, k, r, s, i)
                                   : qi::update_coef_nonsys(r, n, s, i));
        std::printf("\n");
    }
    // the context sizes the device layer derives from the same header
    std::printf("W %lld %lld %lld %lld\n", qi::update_ctx_words(1, 1), qi::update_ctx_words(3, 5),
                qi::update_ctx_words(5, 7), qi::update_ctx_words(8, m));
    return 0;
}
