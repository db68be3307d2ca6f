// Host check of stage::apply_fixes (quadiron_amd/csrc/fec_stage.h) with the
// fix lists of a multi-fragment locate: two and three fixes in one column, at
// different fragments, across data and coded rows; one fix adds a mark, one
// removes a mark, and a list that would pass the capacity refuses the whole
// patch.  Stand-alone (run by tests/test_apply_fixes_multi.py).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../quadiron_amd/csrc/fec_stage.h"

using namespace qi;
using namespace qi::fec;
using namespace qi::fec::stage;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static uint16_t word(const std::vector<uint8_t>& row, size_t c)
{
    return static_cast<uint16_t>(row[2 * c] | row[2 * c + 1] << 8);
}

static std::vector<size_t> marks(const Properties& p)
{
    std::vector<size_t> v;
    for (auto const& it : p.get_map())
        v.push_back(it.first);
    return v;
}

int main()
{
    const unsigned k = 3, m = 3, P = 8;
    const FragMap map(FecType::SYSTEMATIC, k, m);
    using Rows = std::vector<std::vector<uint8_t>>;
    const Rows data0(k, std::vector<uint8_t>(2 * P, 0x11)), coded0(m, std::vector<uint8_t>(2 * P, 0x22));
    const auto ptrs = [](Rows& r) {
        std::vector<uint8_t*> p;
        for (auto& v : r)
            p.push_back(v.data());
        return p;
    };
    // parity 0 has a mark at column 5, parity 1 at 2 and 6, parity 2 none
    const auto props0 = [] {
        std::vector<Properties> p(3);
        p[0].add(5, OOR_MARK);
        p[1].add(2, OOR_MARK);
        p[1].add(6, OOR_MARK);
        return p;
    };
    // column 5: three fixes -- data row 1, parity 0 (the mark goes: 65536 ->
    // 0x0a0b) and parity 2 (a mark comes: -> 65536); column 2: two fixes --
    // data row 0 and parity 1 under its mark (stays 65536: the mark stays)
    const std::vector<LocateFix> fixes = {
        {5, 1, 0x0102}, {5, 3, 0x0a0b}, {5, 5, 65536}, {2, 0, 0xffff}, {2, 4, 65536}};
    {
        Rows data = data0, coded = coded0;
        std::vector<Properties> props = props0();
        CHECK(apply_fixes(map, fixes, ptrs(data), ptrs(coded), props, 2));
        CHECK(word(data[1], 5) == 0x0102 && word(data[0], 2) == 0xffff);
        CHECK(word(coded[0], 5) == 0x0a0b && word(coded[2], 5) == 0 && word(coded[1], 2) == 0);
        CHECK(marks(props[0]).empty());
        CHECK((marks(props[1]) == std::vector<size_t>{2, 6}));
        CHECK((marks(props[2]) == std::vector<size_t>{5}));
        // nothing else moved
        for (unsigned c = 0; c < P; c++) {
            CHECK(c == 2 || word(data[0], c) == 0x1111);
            CHECK(c == 5 || word(data[1], c) == 0x1111);
            CHECK(word(data[2], c) == 0x1111);
            CHECK(c == 5 || word(coded[0], c) == 0x2222);
            CHECK(c == 2 || word(coded[1], c) == 0x2222);
            CHECK(c == 5 || word(coded[2], c) == 0x2222);
        }
    }
    {
        // capacity 0: parity 2's list would grow from 0 to 1 -- the whole
        // patch is refused, the other fixes of its column included
        Rows data = data0, coded = coded0;
        std::vector<Properties> props = props0();
        CHECK(!apply_fixes(map, fixes, ptrs(data), ptrs(coded), props, 0));
        CHECK(data == data0 && coded == coded0);
        CHECK((marks(props[0]) == std::vector<size_t>{5}));
        CHECK((marks(props[1]) == std::vector<size_t>{2, 6}) && marks(props[2]).empty());
    }
    {
        // a data row cannot hold 65536: refused as a whole
        Rows data = data0, coded = coded0;
        std::vector<Properties> props = props0();
        const std::vector<LocateFix> bad = {{5, 3, 7}, {5, 1, 65536}};
        CHECK(!apply_fixes(map, bad, ptrs(data), ptrs(coded), props, 8));
        CHECK(data == data0 && coded == coded0 && (marks(props[0]) == std::vector<size_t>{5}));
    }
    std::printf("ALL OK\n");
    return 0;
}
