// fec_stage.h -- the host facade's staging steps that need no device: which
// fragments a decode uses and where each one lives, OOR marks packed into the
// device's counts + entries[cap] form, the layout of the small device buffer,
// the bounded capacity retry, the held ids of a share as list positions, a
// locate's result words, and the flat C arrays <-> Properties.  No HIP,
// no plan: fec.cpp and quadiron_c.cpp build on it, and
// tests/host/test_fec_stage.cpp checks it on the CPU.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/qi_fec.hpp"

namespace qi {
namespace fec {
namespace stage {

// ---- fragment map -------------------------------------------------------
// Fragment ids are the decode's id space: systematic f < k is data row f and
// f >= k coded slot (parity) f - k; non-systematic f is coded slot f.
struct FragMap {
    bool sys;
    unsigned k, n_outputs;
    FragMap(FecType t, unsigned n_data, unsigned outputs)
        : sys(t == FecType::SYSTEMATIC), k(n_data), n_outputs(outputs)
    {
    }
    struct Slot {
        bool is_data;
        unsigned slot;
    };
    unsigned code_len() const { return sys ? k + n_outputs : n_outputs; }
    unsigned data_rows() const { return sys ? k : 0; }
    Slot slot(unsigned id) const
    {
        return sys && id < k ? Slot{true, id} : Slot{false, sys ? id - k : id};
    }
    unsigned coded_id(unsigned slot) const { return sys ? k + slot : slot; }
    // the entry of fragment `id` in the caller's data / coded arrays
    template <typename A, typename B>
    auto pick(unsigned id, const A& data, const B& coded) const
    {
        const Slot s = slot(id);
        return s.is_data ? data[s.slot] : coded[s.slot];
    }
    std::vector<int> present(const std::vector<int>& missing_idxs) const
    {
        std::vector<int> p(code_len());
        for (unsigned i = 0; i < code_len(); i++)
            p[i] = missing_idxs[i] ? 0 : 1;
        return p;
    }
    // has_data(i) / has_coded(slot): whether the caller holds that fragment
    template <typename D, typename C>
    std::vector<int> present(D has_data, C has_coded) const
    {
        std::vector<int> p(code_len(), 0);
        for (unsigned i = 0; i < data_rows(); i++)
            p[i] = has_data(i) ? 1 : 0;
        for (unsigned i = 0; i < n_outputs; i++)
            p[coded_id(i)] = has_coded(i) ? 1 : 0;
        return p;
    }
    // systematic with every data row present: nothing to decode
    // (src/fec_base.h:1208-1211)
    bool data_in_clear(const std::vector<int>& present) const
    {
        if (!sys)
            return false;
        for (unsigned i = 0; i < k; i++)
            if (!present[i])
                return false;
        return true;
    }
    // first k present, data before parities: src/fec_base.h:1199-1236
    bool select(const std::vector<int>& present, std::vector<int>& ids) const
    {
        ids.clear();
        for (unsigned i = 0; i < data_rows(); i++)
            if (present[i])
                ids.push_back(static_cast<int>(i));
        for (unsigned i = 0; i < n_outputs && ids.size() < k; i++)
            if (present[coded_id(i)])
                ids.push_back(static_cast<int>(coded_id(i)));
        return ids.size() == k;
    }
    // the first min(present, limit) present fragments in the same order (data
    // before parities): what a locate lists
    std::vector<int> select_upto(const std::vector<int>& present, size_t limit) const
    {
        std::vector<int> ids;
        for (unsigned i = 0; i < data_rows() && ids.size() < limit; i++)
            if (present[i])
                ids.push_back(static_cast<int>(i));
        for (unsigned i = 0; i < n_outputs && ids.size() < limit; i++)
            if (present[coded_id(i)])
                ids.push_back(static_cast<int>(coded_id(i)));
        return ids;
    }
};

// ---- mark packing -------------------------------------------------------
// rows.size() buckets of `cap` entries each: the marks of rows[i] (null: no
// marks) inside [offset, offset + words), relative to offset, in list order;
// cap is the largest count, at least 1
struct PackedMarks {
    std::vector<uint32_t> counts, entries;
    size_t cap = 1;
};

// With a cursor (one position per row, zero before the first window) the
// lists must ascend and the windows move forward: every mark is then taken
// once and skipped once over the whole walk.
inline PackedMarks pack_marks(const std::vector<const Properties*>& rows, size_t offset,
                              size_t words, std::vector<size_t>* cursor = nullptr)
{
    const size_t n = rows.size();
    std::vector<std::vector<uint32_t>> in(n);
    PackedMarks pm;
    for (size_t i = 0; i < n; i++) {
        if (!rows[i])
            continue;
        auto const& mk = rows[i]->get_map();
        size_t b = 0;
        if (cursor) {
            size_t& c = (*cursor)[i];
            while (c < mk.size() && mk[c].first < offset)
                c++;
            b = c;
        }
        for (size_t e = b; e < mk.size(); e++) {
            if (mk[e].first >= offset + words) {
                if (cursor)
                    break;
                continue;
            }
            if (mk[e].first >= offset)
                in[i].push_back(static_cast<uint32_t>(mk[e].first - offset));
        }
        pm.cap = std::max(pm.cap, in[i].size());
    }
    pm.counts.resize(n);
    pm.entries.assign(n * pm.cap, 0);
    for (size_t i = 0; i < n; i++) {
        pm.counts[i] = static_cast<uint32_t>(in[i].size());
        std::copy(in[i].begin(), in[i].end(), pm.entries.begin() + i * pm.cap);
    }
    return pm;
}

// ---- small-buffer layout ------------------------------------------------
inline size_t round64(size_t n)
{
    return (n + 63) / 64 * 64;
}

// consecutive sections of the given byte sizes, each starting on a 64-byte
// boundary: off[i] is the start of section i, off[N] the end of the last one
template <size_t N>
std::array<size_t, N + 1> layout(const size_t (&bytes)[N])
{
    std::array<size_t, N + 1> off{};
    for (size_t i = 0; i < N; i++) {
        off[i] = i ? round64(off[i]) : 0;
        off[i + 1] = off[i] + bytes[i];
    }
    return off;
}

// ---- capacity retry -----------------------------------------------------
// launch(cap), then read_max() -- the largest bucket count the launch
// reported.  A count above cap (adversarial data) means entries were dropped:
// between() and one more launch with the exact capacity, read back again.
// At most two attempts; returns the capacity of the last one.
template <typename Launch, typename ReadMax, typename Between>
size_t run_with_retry(size_t cap, Launch launch, ReadMax read_max, Between between)
{
    launch(cap);
    const size_t mx = read_max();
    if (mx <= cap)
        return cap;
    between();
    launch(mx);
    (void)read_max();
    return mx;
}

// ---- entries -> Properties ----------------------------------------------
// a device bucket is unordered: its first `count` entries, ascending, become
// marks at offset + entry
inline void add_sorted(Properties& p, uint32_t* bucket, uint32_t count, size_t offset)
{
    std::sort(bucket, bucket + count);
    for (uint32_t e = 0; e < count; e++)
        p.add(offset + bucket[e], OOR_MARK);
}

// ---- locate fixes -> the caller's buffers -----------------------------------
// Writes the corrected symbols into the rows (u16 words; 65536 is stored as 0)
// and keeps the coded fragments' ascending mark lists in step: a mark is
// inserted where the symbol becomes 65536 and removed where it stops being
// one.  Nothing is touched, and false returned, when a list would grow past
// max_marks or a data row would need a mark.
inline bool apply_fixes(const FragMap& map, const std::vector<LocateFix>& fixes,
                        const std::vector<uint8_t*>& data_bufs,
                        const std::vector<uint8_t*>& coded_bufs, std::vector<Properties>& props,
                        size_t max_marks)
{
    std::vector<std::vector<size_t>> marks(map.n_outputs);
    std::vector<char> touched(map.n_outputs, 0);
    for (auto const& f : fixes) {
        const auto fs = map.slot(static_cast<unsigned>(f.fragment));
        if (fs.is_data) {
            if (f.symbol > 65535u)
                return false;
            continue;
        }
        auto& mk = marks[fs.slot];
        if (!touched[fs.slot]) {
            touched[fs.slot] = 1;
            for (auto const& it : props[fs.slot].get_map())
                mk.push_back(it.first);
            std::sort(mk.begin(), mk.end());
        }
        const auto at = std::lower_bound(mk.begin(), mk.end(), static_cast<size_t>(f.column));
        const bool has = at != mk.end() && *at == f.column;
        if (f.symbol == 65536u && !has)
            mk.insert(at, f.column);
        else if (f.symbol != 65536u && has)
            mk.erase(at);
    }
    for (unsigned j = 0; j < map.n_outputs; j++)
        if (touched[j] && marks[j].size() > max_marks &&
            marks[j].size() > props[j].get_map().size())
            return false;
    for (auto const& f : fixes) {
        uint8_t* row = map.pick(static_cast<unsigned>(f.fragment), data_bufs, coded_bufs);
        const uint16_t w = static_cast<uint16_t>(f.symbol & 0xffffu);
        row[2 * static_cast<size_t>(f.column)] = static_cast<uint8_t>(w & 0xff);
        row[2 * static_cast<size_t>(f.column) + 1] = static_cast<uint8_t>(w >> 8);
    }
    for (unsigned j = 0; j < map.n_outputs; j++) {
        if (!touched[j])
            continue;
        props[j].clear();
        for (size_t c : marks[j])
            props[j].add(c, OOR_MARK);
    }
    return true;
}

// ---- syndrome deltas -> a holder's rows --------------------------------------
// A syndrome resolve (qi_gpu_syndrome_locate) reports what a fragment is off
// by, not what it should hold: LocateFix::symbol is the error e in [1, 65536]
// and the true symbol (y - e) mod 65537, with y the restored symbol of the row
// (65536 where its ascending mark list names the column).  The holder of the
// fragments `fragment_ids` (rows[h], props[h]; a systematic data row has no
// marks) applies the deltas that name one of them and skips the others.
// Nothing is touched, and -1 returned, when a data row would have to hold
// 65536 or a mark list would grow past max_marks (apply_fixes' rule); else the
// number of deltas applied.  A (fragment, column) pair is named at most once.
inline long long apply_deltas(const FragMap& map, const std::vector<int>& fragment_ids,
                              const std::vector<uint8_t*>& rows, std::vector<Properties>& props,
                              const std::vector<LocateFix>& deltas, size_t max_marks)
{
    std::vector<int> where(map.code_len(), -1);
    std::vector<uint8_t*> data_bufs(map.data_rows(), nullptr), coded_bufs(map.n_outputs, nullptr);
    std::vector<Properties> coded_props(map.n_outputs);
    std::vector<std::vector<size_t>> marks(map.n_outputs);  // ascending
    for (size_t h = 0; h < fragment_ids.size(); h++) {
        const int f = fragment_ids[h];
        if (f < 0 || static_cast<unsigned>(f) >= map.code_len() || where[f] >= 0)
            return -1;
        where[f] = static_cast<int>(h);
        const auto fs = map.slot(static_cast<unsigned>(f));
        if (fs.is_data) {
            data_bufs[fs.slot] = rows[h];
        } else {
            coded_bufs[fs.slot] = rows[h];
            coded_props[fs.slot] = props[h];
            for (auto const& it : props[h].get_map())
                marks[fs.slot].push_back(it.first);
            std::sort(marks[fs.slot].begin(), marks[fs.slot].end());
        }
    }
    std::vector<LocateFix> fixes;
    for (auto const& d : deltas) {
        if (d.fragment < 0 || static_cast<unsigned>(d.fragment) >= map.code_len() ||
            where[d.fragment] < 0)
            continue;
        const auto fs = map.slot(static_cast<unsigned>(d.fragment));
        const uint8_t* row = rows[where[d.fragment]];
        uint32_t y = static_cast<uint32_t>(row[2 * static_cast<size_t>(d.column)]) |
                     static_cast<uint32_t>(row[2 * static_cast<size_t>(d.column) + 1]) << 8;
        if (!fs.is_data && std::binary_search(marks[fs.slot].begin(), marks[fs.slot].end(),
                                              static_cast<size_t>(d.column)))
            y = 65536u;
        const uint32_t e = d.symbol % 65537u;
        const uint32_t v = y >= e ? y - e : y + 65537u - e;
        if (fs.is_data && v == 65536u)
            return -1;
        fixes.push_back(LocateFix{d.column, d.fragment, v});
    }
    if (!apply_fixes(map, fixes, data_bufs, coded_bufs, coded_props, max_marks))
        return -1;
    for (size_t h = 0; h < fragment_ids.size(); h++) {
        const auto fs = map.slot(static_cast<unsigned>(fragment_ids[h]));
        if (!fs.is_data)
            props[h] = coded_props[fs.slot];
    }
    return static_cast<long long>(fixes.size());
}

// ---- held ids -> list positions ----------------------------------------------
// A share (partial repair, syndrome) names the fragments its context lists,
// the fragments to rebuild and the fragments the caller holds.  Checked in
// this order, the first failure reported: every listed id is below code_len
// and listed once (bad_id); every target is below code_len, not listed and
// named once (bad_target); every held id is listed and held once (bad_held).
// pos[h]: the position of held[h] in `listed`.
enum class HeldCheck { ok, bad_id, bad_target, bad_held };

inline HeldCheck held_positions(unsigned code_len, const std::vector<int>& listed,
                                const std::vector<int>& targets, const std::vector<int>& held,
                                std::vector<uint16_t>& pos)
{
    const auto in_range = [&](int f) { return f >= 0 && static_cast<unsigned>(f) < code_len; };
    std::vector<int> where(code_len, -1);  // fragment id -> position in listed, -2: a target
    for (size_t i = 0; i < listed.size(); i++) {
        if (!in_range(listed[i]) || where[listed[i]] != -1)
            return HeldCheck::bad_id;
        where[listed[i]] = static_cast<int>(i);
    }
    for (int t : targets) {
        if (!in_range(t) || where[t] != -1)
            return HeldCheck::bad_target;
        where[t] = -2;
    }
    pos.clear();
    std::vector<char> taken(listed.size(), 0);
    for (int f : held) {
        if (!in_range(f) || where[f] < 0 || taken[where[f]])
            return HeldCheck::bad_held;
        taken[where[f]] = 1;
        pos.push_back(static_cast<uint16_t>(where[f]));
    }
    return HeldCheck::ok;
}

// ---- locate results -----------------------------------------------------------
// What a locate starts from: no fragment listed, nothing found, t weights.
inline void reset_locate(LocateResult& r, unsigned code_len, int t)
{
    r.located.assign(code_len, -1);
    r.unlocated = 0;
    r.fixes.clear();
    r.weights.assign(t, 0);
}

// The device's result words over the N = ids.size() listed fragments --
// located[N], unlocated, the fix count, then the weights -- and its nfix fix
// triples {column, list position, symbol} into a reset LocateResult of t
// weights: positions become fragment ids through `ids`.
inline void fill_locate(LocateResult& r, const std::vector<int>& ids, const uint32_t* res,
                        const uint32_t* fx, size_t nfix)
{
    const size_t N = ids.size();
    for (size_t i = 0; i < N; i++)
        r.located[ids[i]] = static_cast<long long>(res[i]);
    r.unlocated = static_cast<long long>(res[N]);
    for (size_t nu = 0; nu < r.weights.size(); nu++)
        r.weights[nu] = static_cast<long long>(res[N + 2 + nu]);
    for (size_t e = 0; e < nfix; e++)
        r.fixes.push_back(LocateFix{fx[3 * e], ids[fx[3 * e + 1]], fx[3 * e + 2]});
}

// LocateResult -> the C views' result words: located per fragment id,
// unlocated, then the weights
inline void locate_to_flat(const LocateResult& r, long long* result)
{
    long long* at = std::copy(r.located.begin(), r.located.end(), result);
    *at++ = r.unlocated;
    std::copy(r.weights.begin(), r.weights.end(), at);
}

// ---- flat C arrays <-> Properties ---------------------------------------
// (oor, flags, count, cap): props.size() rows of cap locations (and markers;
// flags null: OOR_MARK) with a count each.  A count above cap is clamped on
// the way in; on the way out the count is exact and only cap entries are
// written.  count null on the way in: no marks.
inline void props_from_flat(std::vector<Properties>& props, const uint32_t* oor,
                            const uint32_t* flags, const uint32_t* count, uint32_t cap)
{
    for (size_t i = 0; i < props.size(); i++) {
        const uint32_t c = !count ? 0 : std::min(count[i], cap);
        for (uint32_t e = 0; e < c; e++)
            props[i].add(oor[i * cap + e], flags ? flags[i * cap + e] : OOR_MARK);
    }
}

inline void props_to_flat(const std::vector<Properties>& props, uint32_t* oor, uint32_t* flags,
                          uint32_t* count, uint32_t cap)
{
    for (size_t i = 0; i < props.size(); i++) {
        uint32_t c = 0;
        for (auto const& it : props[i].get_map()) {
            if (c < cap) {
                oor[i * cap + c] = static_cast<uint32_t>(it.first);
                if (flags)
                    flags[i * cap + c] = it.second;
            }
            c++;
        }
        count[i] = c;
    }
}

// ---- RS-NF4 marks -------------------------------------------------------
// (16-bit lane, OOR_MARK) marks <-> (word, component mask) marks of g lanes
// per word; lane marks ascend
inline void marks_from_lanes(const Properties& lanes, unsigned g, Properties& words)
{
    // encode_post_process (src/fec_rs_nf4.h:271-289): one mark per word,
    // bit c set when component c was 65536 (NF4::unpack, gf_nf4.h:421-446)
    words.clear();
    size_t cur = 0;
    uint32_t mask = 0;
    for (auto const& it : lanes.get_map()) {
        const size_t w = it.first / g;
        if (mask && w != cur) {
            words.add(cur, mask);
            mask = 0;
        }
        cur = w;
        mask |= 1u << (it.first % g);
    }
    if (mask)
        words.add(cur, mask);
}

inline void marks_to_lanes(const Properties& words, unsigned g, Properties& lanes)
{
    // decode_prepare (src/fec_rs_nf4.h:291-317): NF4::pack(a, flag) sets the
    // flagged components to 65536 (gf_nf4.h:372-383)
    lanes.clear();
    for (auto const& it : words.get_map())
        for (unsigned c = 0; c < g; c++)
            if ((it.second >> c) & 1u)
                lanes.add(it.first * g + c, OOR_MARK);
}

}  // namespace stage
}  // namespace fec
}  // namespace qi
