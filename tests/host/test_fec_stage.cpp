// Host check of quadiron_amd/csrc/fec_stage.h, the host facade's staging
// steps that need no device, against values written out here.  Stand-alone:
// links nothing of the library (run by tests/test_fec_stage.py under ASan +
// UBSan).
#include <cstdio>
#include <cstdlib>
#include <utility>
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

using V = std::vector<int>;
using U = std::vector<uint32_t>;
using Marks = std::vector<std::pair<size_t, uint32_t>>;

static Properties props_at(std::initializer_list<size_t> locs)
{
    Properties p;
    for (size_t l : locs)
        p.add(l, OOR_MARK);
    return p;
}

static void test_fragment_map()
{
    const unsigned k = 4, m = 4;
    const FragMap sys(FecType::SYSTEMATIC, k, m), non(FecType::NON_SYSTEMATIC, k, k + m);
    CHECK(sys.code_len() == 8 && non.code_len() == 8);
    CHECK(sys.data_rows() == 4 && non.data_rows() == 0);
    // slots at ids 0, k - 1, k, k + m - 1
    const unsigned ids[4] = {0, k - 1, k, k + m - 1};
    const bool sys_data[4] = {true, true, false, false};
    const unsigned sys_slot[4] = {0, 3, 0, 3}, non_slot[4] = {0, 3, 4, 7};
    for (int i = 0; i < 4; i++) {
        CHECK(sys.slot(ids[i]).is_data == sys_data[i] && sys.slot(ids[i]).slot == sys_slot[i]);
        CHECK(!non.slot(ids[i]).is_data && non.slot(ids[i]).slot == non_slot[i]);
    }
    CHECK(sys.coded_id(3) == 7 && non.coded_id(3) == 3);
    const V data{10, 11, 12, 13}, coded{20, 21, 22, 23, 24, 25, 26, 27};
    CHECK(sys.pick(2, data, coded) == 12 && sys.pick(5, data, coded) == 21);
    CHECK(non.pick(2, data, coded) == 22 && non.pick(5, data, coded) == 25);
    // present from missing flags; a data row and a parity missing
    const V missing{0, 1, 0, 0, 0, 1, 0, 0};
    const V present{1, 0, 1, 1, 1, 0, 1, 1};
    CHECK(sys.present(missing) == present && non.present(missing) == present);
    V sel;
    CHECK(sys.select(present, sel) && sel == (V{0, 2, 3, 4}));   // data first, then parity 0
    CHECK(non.select(present, sel) && sel == (V{0, 2, 3, 4}));   // the first k coded rows
    CHECK(!sys.data_in_clear(present) && !non.data_in_clear(present));
    // only parities missing: systematic data is in the clear
    const V par_gone{1, 1, 1, 1, 0, 1, 0, 1};
    CHECK(sys.data_in_clear(par_gone) && !non.data_in_clear(par_gone));
    CHECK(sys.select(par_gone, sel) && sel == (V{0, 1, 2, 3}));
    CHECK(non.select(par_gone, sel) && sel == (V{0, 1, 2, 3}));
    // exactly k present, and k - 1
    const V exact{0, 1, 0, 0, 1, 1, 0, 1}, short1{0, 1, 0, 0, 1, 1, 0, 0};
    CHECK(sys.select(exact, sel) && sel == (V{1, 4, 5, 7}));
    CHECK(non.select(exact, sel) && sel == (V{1, 4, 5, 7}));
    CHECK(!sys.select(short1, sel) && !non.select(short1, sel));
    // present from null-ness predicates: data by row, coded by slot
    const bool has_d[4] = {false, true, false, false};
    const bool has_c[8] = {true, true, false, true, false, false, false, true};
    CHECK(sys.present([&](unsigned i) { return has_d[i]; },
                      [&](unsigned i) { return has_c[i]; }) == exact);
    CHECK(non.present([&](unsigned i) { return has_d[i]; },
                      [&](unsigned i) { return has_c[i]; }) == (V{1, 1, 0, 1, 0, 0, 0, 1}));
}

static void test_pack_marks()
{
    // window [100, 150): marks at offset - 1, offset, offset + words - 1 and
    // offset + words; a row without Properties; an empty row
    const Properties edge = props_at({99, 100, 149, 150}), none;
    const std::vector<const Properties*> rows{&edge, nullptr, &none};
    PackedMarks pm = pack_marks(rows, 100, 50);
    CHECK(pm.cap == 2 && pm.counts == (U{2, 0, 0}) && pm.entries == (U{0, 49, 0, 0, 0, 0}));
    // every row empty: cap 1, one zero entry per row
    pm = pack_marks(rows, 200, 50);
    CHECK(pm.cap == 1 && pm.counts == (U{0, 0, 0}) && pm.entries == (U{0, 0, 0}));
    pm = pack_marks({}, 0, 50);
    CHECK(pm.cap == 1 && pm.counts.empty() && pm.entries.empty());
    // the widest row sets cap; the others are zero padded
    const Properties a = props_at({3, 7, 49, 50, 51, 120}), b = props_at({0, 99, 100, 149});
    const std::vector<const Properties*> two{&a, nullptr, &b};
    pm = pack_marks(two, 0, 50);
    CHECK(pm.cap == 3 && pm.counts == (U{3, 0, 1}));
    CHECK(pm.entries == (U{3, 7, 49, 0, 0, 0, 0, 0, 0}));
    // a chunked walk over three windows equals three one-shot packings
    std::vector<size_t> cursor(3, 0);
    const U want_counts[3] = {{3, 0, 1}, {2, 0, 1}, {1, 0, 2}};
    const U want_entries[3] = {{3, 7, 49, 0, 0, 0, 0, 0, 0}, {0, 1, 0, 0, 49, 0},
                               {20, 0, 0, 0, 0, 49}};
    for (size_t w = 0; w < 3; w++) {
        const PackedMarks one = pack_marks(two, 50 * w, 50);
        const PackedMarks walk = pack_marks(two, 50 * w, 50, &cursor);
        CHECK(one.counts == want_counts[w] && one.entries == want_entries[w]);
        CHECK(walk.cap == one.cap && walk.counts == one.counts && walk.entries == one.entries);
    }
    CHECK(cursor == (std::vector<size_t>{5, 0, 2}));  // each mark passed once
}

static void test_layout()
{
    // the forms it replaces: counts | entries | tail, and ids | counts | entries
    for (size_t no : {1, 16, 17})
        for (size_t cap : {1, 65}) {
            const size_t R = 3;
            const size_t ent_off = 64 * ((no * 4 + 63) / 64);
            const size_t oc_off = ent_off + 64 * ((no * cap * 4 + 63) / 64);
            const auto off = layout({no * 4, no * cap * 4, R * 4});
            CHECK(off[0] == 0 && off[1] == ent_off && off[2] == oc_off &&
                  off[3] == oc_off + R * 4);
            const size_t ids_b = round64(no * 2), cnt_b = round64(no * 4);
            const size_t ent_b = round64(no * cap * 4);
            const auto pipe = layout({no * 2, no * 4, ent_b});
            CHECK(pipe[1] == ids_b && pipe[2] == ids_b + cnt_b &&
                  pipe[3] == ids_b + cnt_b + ent_b);
        }
    const auto off = layout({size_t{68}, size_t{260}, size_t{12}});
    CHECK(off[1] == 128 && off[2] == 448 && off[3] == 460);
    CHECK(round64(0) == 0 && round64(1) == 64 && round64(64) == 64 && round64(65) == 128);
}

static void test_retry()
{
    std::vector<size_t> caps;
    int reads = 0, between = 0;
    // fits: one attempt
    size_t cap = run_with_retry(
        65, [&](size_t c) { caps.push_back(c); }, [&] { reads++; return size_t{65}; },
        [&] { between++; });
    CHECK(cap == 65 && caps == (std::vector<size_t>{65}) && reads == 1 && between == 0);
    // overflows: a second attempt with the exact maximum, read back again
    caps.clear();
    reads = 0;
    cap = run_with_retry(
        65, [&](size_t c) { caps.push_back(c); }, [&] { reads++; return size_t{100}; },
        [&] { between++; });
    CHECK(cap == 100 && caps == (std::vector<size_t>{65, 100}) && reads == 2 && between == 1);
    // never a third attempt
    caps.clear();
    size_t mx = 100;
    cap = run_with_retry(
        65, [&](size_t c) { caps.push_back(c); }, [&] { return mx += 10; }, [] {});
    CHECK(cap == 110 && caps == (std::vector<size_t>{65, 110}));
}

static void test_entries_and_flat()
{
    // a bucket's first `count` entries, ascending, at offset + e
    uint32_t bucket[5] = {9, 2, 5, 1, 0};
    Properties p;
    add_sorted(p, bucket, 3, 1000);
    CHECK(p.get_map() == (Marks{{1002, 1}, {1005, 1}, {1009, 1}}));
    CHECK(bucket[3] == 1 && bucket[4] == 0);
    // flat -> Properties: a count above cap is clamped; a null count: none
    const uint32_t cap = 3;
    const uint32_t oor[6] = {4, 8, 15, 16, 23, 42}, cnt[2] = {2, 7};
    std::vector<Properties> pr(2);
    props_from_flat(pr, oor, nullptr, cnt, cap);
    CHECK(pr[0].get_map() == (Marks{{4, 1}, {8, 1}}));
    CHECK(pr[1].get_map() == (Marks{{16, 1}, {23, 1}, {42, 1}}));
    std::vector<Properties> empty(2);
    props_from_flat(empty, oor, nullptr, nullptr, cap);
    CHECK(empty[0].get_map().empty() && empty[1].get_map().empty());
    // Properties -> flat: the count is exact, only cap entries are written
    pr[1].add(77, OOR_MARK);
    uint32_t out[6] = {9, 9, 9, 9, 9, 9}, oc[2] = {9, 9};
    props_to_flat(pr, out, nullptr, oc, cap);
    CHECK(oc[0] == 2 && oc[1] == 4);
    CHECK(out[0] == 4 && out[1] == 8 && out[2] == 9 && out[3] == 16 && out[4] == 23 &&
          out[5] == 42);
    // a round trip with flags
    const uint32_t floc[4] = {1, 6, 0, 0}, fl[4] = {0x3, 0x8, 0, 0}, fc[2] = {2, 0};
    std::vector<Properties> fp(2);
    props_from_flat(fp, floc, fl, fc, 2);
    CHECK(fp[0].get_map() == (Marks{{1, 0x3}, {6, 0x8}}) && fp[1].get_map().empty());
    uint32_t rloc[4] = {0, 0, 0, 0}, rfl[4] = {0, 0, 0, 0}, rc[2] = {5, 5};
    props_to_flat(fp, rloc, rfl, rc, 2);
    for (int i = 0; i < 4; i++)
        CHECK(rloc[i] == floc[i] && rfl[i] == fl[i]);
    CHECK(rc[0] == 2 && rc[1] == 0);
}

static void test_held_positions()
{
    using H = std::vector<uint16_t>;
    const unsigned code_len = 8;
    const V listed{5, 0, 7, 2};
    H pos{9};
    // positions in list order of the held ids; targets are the ids not listed
    CHECK(held_positions(code_len, listed, {1, 6}, {2, 5}, pos) == HeldCheck::ok);
    CHECK(pos == (H{3, 0}));
    CHECK(held_positions(code_len, listed, {}, {7, 2, 0, 5}, pos) == HeldCheck::ok);
    CHECK(pos == (H{2, 3, 1, 0}));
    CHECK(held_positions(code_len, listed, {}, {}, pos) == HeldCheck::ok && pos.empty());
    // a listed id: repeated, == code_len, negative
    CHECK(held_positions(code_len, {5, 0, 5, 2}, {}, {0}, pos) == HeldCheck::bad_id);
    CHECK(held_positions(code_len, {5, 0, 8, 2}, {}, {0}, pos) == HeldCheck::bad_id);
    CHECK(held_positions(code_len, {5, 0, -1, 2}, {}, {0}, pos) == HeldCheck::bad_id);
    // a target: listed, repeated, == code_len
    CHECK(held_positions(code_len, listed, {1, 7}, {0}, pos) == HeldCheck::bad_target);
    CHECK(held_positions(code_len, listed, {1, 1}, {0}, pos) == HeldCheck::bad_target);
    CHECK(held_positions(code_len, listed, {8}, {0}, pos) == HeldCheck::bad_target);
    // a held id: not listed, repeated, == code_len, a target
    CHECK(held_positions(code_len, listed, {}, {3}, pos) == HeldCheck::bad_held);
    CHECK(held_positions(code_len, listed, {}, {0, 2, 0}, pos) == HeldCheck::bad_held);
    CHECK(held_positions(code_len, listed, {}, {8}, pos) == HeldCheck::bad_held);
    CHECK(held_positions(code_len, listed, {1, 6}, {0, 6}, pos) == HeldCheck::bad_held);
    // the first failing check is the one reported
    CHECK(held_positions(code_len, {5, 5}, {5}, {3}, pos) == HeldCheck::bad_id);
    CHECK(held_positions(code_len, listed, {0}, {3}, pos) == HeldCheck::bad_target);
}

static void test_locate_results()
{
    using LL = std::vector<long long>;
    // N = 3 listed fragments of a code of 6: located[3], unlocated, nfix, weights[t]
    const V ids{4, 0, 3};
    const uint32_t res[3 + 2 + 4] = {7, 0, 2, 5, 2, 6, 1, 99, 99};
    const uint32_t fx[6] = {10, 2, 65536, 11, 0, 0};
    LocateResult r;
    r.located = {1, 2};
    r.unlocated = 9;
    r.fixes.push_back(LocateFix{1, 1, 1});
    r.weights = {3};
    reset_locate(r, 6, 2);
    CHECK(r.located == (LL{-1, -1, -1, -1, -1, -1}) && r.unlocated == 0 && r.fixes.empty() &&
          r.weights == (LL{0, 0}));
    fill_locate(r, ids, res, fx, 2);
    CHECK(r.located == (LL{0, -1, -1, 2, 7, -1}) && r.unlocated == 5 && r.weights == (LL{6, 1}));
    // positions 2 and 0 of the list are fragments 3 and 4
    CHECK(r.fixes.size() == 2 && r.fixes[0].column == 10 && r.fixes[0].fragment == 3 &&
          r.fixes[0].symbol == 65536 && r.fixes[1].column == 11 && r.fixes[1].fragment == 4 &&
          r.fixes[1].symbol == 0);
    long long flat[10];
    for (auto& v : flat)
        v = 77;
    locate_to_flat(r, flat);
    CHECK((LL(flat, flat + 10)) == (LL{0, -1, -1, 2, 7, -1, 5, 6, 1, 77}));
    // t = 0: no weight is read or written; nfix = 0: no fix, a null list
    reset_locate(r, 6, 0);
    fill_locate(r, ids, res, nullptr, 0);
    CHECK(r.located == (LL{0, -1, -1, 2, 7, -1}) && r.unlocated == 5 && r.weights.empty() &&
          r.fixes.empty());
    for (auto& v : flat)
        v = 77;
    locate_to_flat(r, flat);
    CHECK((LL(flat, flat + 10)) == (LL{0, -1, -1, 2, 7, -1, 5, 77, 77, 77}));
    // t = 0 on exactly N + 2 words (what the single locate reads back)
    const uint32_t short_res[5] = {1, 2, 3, 4, 0};
    reset_locate(r, 6, 0);
    fill_locate(r, ids, short_res, nullptr, 0);
    CHECK(r.located == (LL{2, -1, -1, 3, 1, -1}) && r.unlocated == 4);
}

static void test_nf4_marks()
{
    // 4 lanes per word: lanes 0, 1 -> word 0 mask 0b0011; 5 -> word 1 mask
    // 0b0010; 8, 11 -> word 2 mask 0b1001
    const Properties lanes = props_at({0, 1, 5, 8, 11});
    Properties words, back;
    words.add(99, 1);  // cleared first
    marks_from_lanes(lanes, 4, words);
    CHECK(words.get_map() == (Marks{{0, 0x3}, {1, 0x2}, {2, 0x9}}));
    marks_to_lanes(words, 4, back);
    CHECK(back.get_map() == lanes.get_map());
    // one lane per word: the marks themselves
    marks_from_lanes(lanes, 1, words);
    CHECK(words.get_map() == lanes.get_map());
    marks_from_lanes(Properties(), 2, words);
    CHECK(words.get_map().empty());
}

int main()
{
    test_fragment_map();
    test_pack_marks();
    test_layout();
    test_retry();
    test_entries_and_flat();
    test_held_positions();
    test_locate_results();
    test_nf4_marks();
    std::printf("ALL OK\n");
    return 0;
}
