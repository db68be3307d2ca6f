// Host test of quadiron_amd/csrc/patch_math.h, the per-fix decisions of the
// device patch (qi_gpu_patch): a plain C++ loop with the kernel's phases
// (classify everything, decide, write the symbols, edit the unordered
// buckets: removals first, insertions at the end) is driven over random fix
// lists and compared with the project's host rule, stage::apply_fixes and
// stage::apply_deltas of fec_stage.h.  Rows, marks, the number of fixes
// applied and the refusal must agree exactly; the one documented difference
// is the finer status: the host's single "refused" is code 5 or 6 here.
// Built by tests/test_patch_host.py with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../quadiron_amd/csrc/fec_stage.h"
#include "../../quadiron_amd/csrc/patch_math.h"

using namespace qi;
using namespace qi::fec;

namespace {

struct Stripe {
    bool sys;
    unsigned k, code_len, n_outputs, words, cap;
    std::vector<std::vector<uint16_t>> data, coded;  // rows
    std::vector<std::vector<uint32_t>> bucket;       // unordered, per coded slot
};

struct Fix {
    uint32_t col, p, w;
};

struct Result {
    uint32_t status, applied;
};

// the kernel's phases over one stripe (patch.hip), on host buffers
Result model_patch(int mode, Stripe& s, const std::vector<unsigned>& ids,
                   const std::vector<uint8_t>& mine, const std::vector<Fix>& fixes)
{
    const size_t F = fixes.size(), N = ids.size();
    std::vector<char> ins(F, 0);
    std::vector<uint32_t> n_ins(N, 0), n_rem(N, 0);
    uint32_t worst = kPatchOk, applied = 0;
    const auto row_of = [&](const Fix& f) { return patch_row(s.sys, s.k, ids[f.p]); };
    const auto present_in = [&](const PatchRow& r, uint32_t col) {
        if (r.is_data)
            return false;
        auto const& b = s.bucket[r.slot];
        return std::find(b.begin(), b.end(), col) != b.end();
    };
    const auto word_of = [&](const PatchRow& r, uint32_t col) -> uint16_t& {
        return r.is_data ? s.data[r.slot][col] : s.coded[r.slot][col];
    };
    // 1: classify
    for (size_t e = 0; e < F; e++) {
        const Fix& f = fixes[e];
        uint32_t c = kPatchBadFix;
        if (f.p < N) {
            if (!mine[f.p])
                continue;
            c = patch_entry_code(mode, s.words, s.code_len, f.col, ids[f.p], f.w);
        }
        if (c == kPatchOk) {
            const PatchRow r = row_of(f);
            const bool over = !r.is_data && s.bucket[r.slot].size() > s.cap;
            const bool present = !over && present_in(r, f.col);
            const PatchFix pf =
                patch_fix(mode, r.is_data, over, present, over ? 0 : word_of(r, f.col), f.w);
            c = pf.code;
            if (c == kPatchOk) {
                applied++;
                if (pf.dir > 0) {
                    n_ins[f.p]++;
                    ins[e] = 1;
                } else if (pf.dir < 0) {
                    n_rem[f.p]++;
                }
            }
        }
        worst = std::min(worst, c);
    }
    // 2: decide
    if (worst == kPatchOk)
        for (size_t e = 0; e < F; e++) {
            const Fix& f = fixes[e];
            if (!mine[f.p] || row_of(f).is_data)
                continue;
            if (patch_bucket_full(static_cast<uint32_t>(s.bucket[row_of(f).slot].size()),
                                  n_ins[f.p], n_rem[f.p], s.cap))
                worst = kPatchBucketFull;
        }
    if (worst != kPatchOk)
        return {worst, 0};
    if (!applied)
        return {kPatchNone, 0};
    // 3: the symbols
    for (size_t e = 0; e < F; e++) {
        const Fix& f = fixes[e];
        if (!mine[f.p])
            continue;
        const PatchRow r = row_of(f);
        uint32_t v = 65536u;
        if (!ins[e])
            v = patch_fix(mode, r.is_data, false, mode == kPatchDelta && present_in(r, f.col),
                          word_of(r, f.col), f.w)
                    .v;
        word_of(r, f.col) = patch_stored(v);
    }
    // 4: the buckets, removals first (the last entry moves into the gap)
    for (size_t p = 0; p < N; p++) {
        if (!mine[p] || patch_row(s.sys, s.k, ids[p]).is_data)
            continue;
        auto& b = s.bucket[patch_row(s.sys, s.k, ids[p]).slot];
        for (size_t e = 0; e < F; e++) {
            const Fix& f = fixes[e];
            if (f.p != p || ins[e] || (mode == kPatchAbsolute && f.w == 65536u))
                continue;
            auto at = std::find(b.begin(), b.end(), f.col);
            if (at != b.end()) {
                *at = b.back();
                b.pop_back();
            }
        }
        for (size_t e = 0; e < F; e++)
            if (fixes[e].p == p && ins[e] && b.size() < s.cap)
                b.push_back(fixes[e].col);
    }
    return {kPatchDone, applied};
}

int failures = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAIL line %d: %s (trial %d)\n", __LINE__, #cond, trial); \
            failures++;                                                   \
        }                                                                 \
    } while (0)

}  // namespace

int main()
{
    std::mt19937 rng(20240611);
    const auto rnd = [&](unsigned n) { return static_cast<unsigned>(rng() % n); };
    int seen[8] = {0};
    int transitions[4] = {0};
    for (int trial = 0; trial < 4000; trial++) {
        const int mode = trial & 1;
        Stripe s;
        s.sys = (trial >> 1) & 1;
        s.k = 2 + rnd(4);
        const unsigned m = 2 + rnd(5);
        s.code_len = s.k + m;
        s.n_outputs = s.sys ? m : s.code_len;
        s.words = 8 + rnd(40);
        s.cap = rnd(4) == 0 ? rnd(4) : 4 + rnd(s.words);
        s.data.assign(s.sys ? s.k : 0, std::vector<uint16_t>(s.words));
        s.coded.assign(s.n_outputs, std::vector<uint16_t>(s.words));
        s.bucket.assign(s.n_outputs, {});
        for (auto& r : s.data)
            for (auto& w : r)
                w = static_cast<uint16_t>(rnd(4) ? rnd(65536) : rnd(3));
        for (unsigned j = 0; j < s.n_outputs; j++) {
            for (auto& w : s.coded[j])
                w = static_cast<uint16_t>(rnd(4) ? rnd(65536) : rnd(3));
            const unsigned want = std::min(s.cap, rnd(3) ? rnd(6) : s.cap);
            std::set<uint32_t> cols;
            while (cols.size() < std::min(want, s.words))
                cols.insert(rnd(s.words));
            s.bucket[j].assign(cols.begin(), cols.end());
            std::shuffle(s.bucket[j].begin(), s.bucket[j].end(), rng);
        }
        // the listed fragments and which of them are held here
        std::vector<unsigned> all(s.code_len);
        for (unsigned i = 0; i < s.code_len; i++)
            all[i] = i;
        std::shuffle(all.begin(), all.end(), rng);
        const unsigned N = 1 + rnd(s.code_len);
        std::vector<unsigned> ids(all.begin(), all.begin() + N);
        std::vector<uint8_t> mine(N, 1);
        if (mode == kPatchDelta && rnd(2))
            for (auto& h : mine)
                h = rnd(3) != 0;
        // a random list of distinct (position, column) pairs
        std::vector<Fix> fixes;
        std::set<std::pair<unsigned, unsigned>> named;
        const unsigned n_fix = rnd(4) ? rnd(24) : 0;
        for (unsigned e = 0; e < n_fix; e++) {
            const unsigned p = rnd(N), col = rnd(s.words);
            if (!named.insert({p, col}).second)
                continue;
            const PatchRow r = patch_row(s.sys, s.k, ids[p]);
            const bool present = !r.is_data && std::count(s.bucket[r.slot].begin(),
                                                          s.bucket[r.slot].end(), col);
            const uint32_t y =
                present ? 65536u : (r.is_data ? s.data[r.slot][col] : s.coded[r.slot][col]);
            // the wanted symbol: 65536 often on coded rows, rarely on data rows
            const bool to_mark = r.is_data ? rnd(40) == 0 : rnd(3) == 0;
            uint32_t v = to_mark ? 65536u : rnd(65536);
            if (mode == kPatchDelta && v == y)
                v = (v + 1) % 65536u;
            const uint32_t w = mode == kPatchAbsolute ? v : (y + 65537u - v) % 65537u;
            fixes.push_back({col, p, w});
        }
        // ---- the host rule, on copies
        const stage::FragMap map(s.sys ? FecType::SYSTEMATIC : FecType::NON_SYSTEMATIC, s.k,
                                 s.n_outputs);
        std::vector<std::vector<uint16_t>> h_data = s.data, h_coded = s.coded;
        std::vector<Properties> props(s.n_outputs);
        for (unsigned j = 0; j < s.n_outputs; j++) {
            std::vector<uint32_t> asc = s.bucket[j];
            std::sort(asc.begin(), asc.end());
            for (uint32_t c : asc)
                props[j].add(c, OOR_MARK);
        }
        bool refused;
        long long h_applied = 0;
        if (mode == kPatchAbsolute) {
            std::vector<LocateFix> lf;
            for (auto const& f : fixes)
                lf.push_back({f.col, static_cast<int>(ids[f.p]), f.w});
            std::vector<uint8_t*> db, cb;
            for (auto& r : h_data)
                db.push_back(reinterpret_cast<uint8_t*>(r.data()));
            for (auto& r : h_coded)
                cb.push_back(reinterpret_cast<uint8_t*>(r.data()));
            refused = !stage::apply_fixes(map, lf, db, cb, props, s.cap);
            h_applied = static_cast<long long>(lf.size());
        } else {
            std::vector<int> held;
            std::vector<uint8_t*> rows;
            std::vector<Properties> hp;
            for (unsigned p = 0; p < N; p++) {
                if (!mine[p])
                    continue;
                held.push_back(static_cast<int>(ids[p]));
                const auto fs = map.slot(ids[p]);
                rows.push_back(reinterpret_cast<uint8_t*>(
                    fs.is_data ? h_data[fs.slot].data() : h_coded[fs.slot].data()));
                hp.push_back(fs.is_data ? Properties() : props[fs.slot]);
            }
            std::vector<LocateFix> lf;
            for (auto const& f : fixes)
                lf.push_back({f.col, static_cast<int>(ids[f.p]), f.w});
            h_applied = stage::apply_deltas(map, held, rows, hp, lf, s.cap);
            refused = h_applied < 0;
            for (size_t h = 0; h < held.size(); h++) {
                const auto fs = map.slot(static_cast<unsigned>(held[h]));
                if (!fs.is_data)
                    props[fs.slot] = hp[h];
            }
        }
        // ---- the model
        const Stripe before = s;
        const Result r = model_patch(mode, s, ids, mine, fixes);
        seen[r.status]++;
        if (refused) {
            CHECK(r.status == kPatchDataMark || r.status == kPatchBucketFull);
            CHECK(r.applied == 0);
            CHECK(s.data == before.data && s.coded == before.coded && s.bucket == before.bucket);
        } else {
            CHECK(r.status == (h_applied ? kPatchDone : kPatchNone));
            CHECK(r.applied == h_applied);
        }
        // (a refused host call touched nothing either)
        CHECK(s.data == h_data);
        CHECK(s.coded == h_coded);
        for (unsigned j = 0; j < s.n_outputs; j++) {
            std::vector<uint32_t> got = s.bucket[j], want;
            std::sort(got.begin(), got.end());
            for (auto const& it : props[j].get_map())
                want.push_back(static_cast<uint32_t>(it.first));
            CHECK(got == want);
            CHECK(std::adjacent_find(got.begin(), got.end()) == got.end());
            CHECK(got.size() <= std::max<size_t>(s.cap, before.bucket[j].size()));
        }
        if (!refused)
            for (auto const& f : fixes) {
                if (!mine[f.p])
                    continue;
                const PatchRow pr = patch_row(s.sys, s.k, ids[f.p]);
                if (pr.is_data)
                    continue;
                const bool was = std::count(before.bucket[pr.slot].begin(),
                                            before.bucket[pr.slot].end(), f.col);
                const bool is = std::count(s.bucket[pr.slot].begin(), s.bucket[pr.slot].end(),
                                           f.col);
                transitions[2 * was + is]++;
            }
    }
    // what the device adds to the host rule: the entry checks
    {
        const int trial = -1;
        CHECK(patch_entry_code(kPatchAbsolute, 10, 8, 10, 0, 0) == kPatchBadFix);   // column
        CHECK(patch_entry_code(kPatchAbsolute, 10, 8, 9, 8, 0) == kPatchBadFix);    // id
        CHECK(patch_entry_code(kPatchAbsolute, 10, 8, 9, 7, 65537) == kPatchBadFix);
        CHECK(patch_entry_code(kPatchAbsolute, 10, 8, 9, 7, 65536) == kPatchOk);
        CHECK(patch_entry_code(kPatchDelta, 10, 8, 9, 7, 0) == kPatchBadFix);
        CHECK(patch_entry_code(kPatchDelta, 10, 8, 9, 7, 65536) == kPatchOk);
        CHECK(patch_entry_code(kPatchDelta, 1ull << 32, 65536, 0xffffffffu, 65535, 1) == kPatchOk);
        CHECK(patch_fix(kPatchAbsolute, false, true, false, 0, 1).code == kPatchBadFix);
        CHECK(patch_fix(kPatchDelta, true, false, false, 4, 5).code == kPatchDataMark);
        CHECK(patch_fix(kPatchDelta, false, false, true, 7, 65536).v == 0);
        CHECK(patch_bucket_full(4, 1, 1, 4) == false);
        CHECK(patch_bucket_full(4, 2, 1, 4) == true);
        CHECK(patch_bucket_full(0, 1, 0, 0) == true);
        // every status and every transition occurred
        CHECK(seen[kPatchNone] > 50 && seen[kPatchDone] > 500);
        CHECK(seen[kPatchDataMark] > 20 && seen[kPatchBucketFull] > 50);
        for (int t = 0; t < 4; t++)
            CHECK(transitions[t] > 100 || (t == 3 && transitions[t] > 20));
    }
    std::printf("none %d done %d data_mark %d bucket_full %d; transitions %d %d %d %d\n",
                seen[kPatchNone], seen[kPatchDone], seen[kPatchDataMark], seen[kPatchBucketFull],
                transitions[0], transitions[1], transitions[2], transitions[3]);
    if (failures)
        return 1;
    std::printf("ALL OK\n");
    return 0;
}
