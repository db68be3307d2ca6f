// C++ FecCode-style API (include/qi_fec.hpp) on top of the device engine.
//
// The block/stream methods keep the reference's observable behaviour
// (fragment selection, tail handling, OOR side channel, offsets) while the
// per-packet loop of src/fec_base.h:1103-1150 becomes ONE device call over
// the whole block: outputs do not depend on the packet size.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <arpa/inet.h>
#include <chrono>
#include <memory>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>

#include "../../include/qi_fec.hpp"
#include "../../include/qi_gpu.h"
#include "fec_stage.h"
#include "qi_internal.h"
#include "qi_plan.h"

namespace qi {

// ------------------------------------------------------------- Properties

void Properties::sort()
{
    std::sort(props.begin(), props.end());
}

int Properties::fnt_serialize(uint32_t* dwords, unsigned n_dwords) const
{
    // src/property.h:104-118 (the last dword is left untouched)
    if ((2 + props.size()) > n_dwords)
        return -1;
    dwords[0] = htonl(FNT1);
    unsigned i = 2;
    for (auto const& it : props)
        dwords[i++] = htonl(static_cast<uint32_t>(it.first));
    dwords[1] = htonl(i - 2);
    for (unsigned d = i; d + 1 < n_dwords; d++)
        dwords[d] = 0;
    return 0;
}

int Properties::fnt_deserialize(const uint32_t* dwords, unsigned n_dwords)
{
    // src/property.h:125-142
    if (n_dwords < 2)
        return -1;
    if (ntohl(dwords[0]) != FNT1)
        return -1;
    const uint32_t n = ntohl(dwords[1]);
    if ((2 + static_cast<uint64_t>(n)) > n_dwords)
        return -1;
    for (uint32_t i = 0; i < n; i++)
        add(static_cast<size_t>(ntohl(dwords[i + 2])), OOR_MARK);
    return 0;
}

// text form of ec_driver's .props files (src/property.cpp:37-78)
std::istream& operator>>(std::istream& is, Properties& p)
{
    std::string line;
    while (std::getline(is, line)) {
        auto b = line.find_first_not_of(" \f\t\v");
        if (b == std::string::npos)
            continue;
        if (line[b] == '#' || line[b] == ';')
            continue;
        auto e = line.find('=', b);
        std::string key = line.substr(b, e - b);
        key.erase(key.find_last_not_of(" \f\t\v") + 1);
        if (key.empty())
            continue;
        b = line.find_first_not_of(" \f\n\r\t\v", e + 1);
        e = line.find_last_not_of(" \f\n\r\t\v") + 1;
        p.add(std::stoul(key), static_cast<uint32_t>(std::stoul(line.substr(b, e - b))));
    }
    return is;
}

std::ostream& operator<<(std::ostream& os, const Properties& p)
{
    for (auto const& it : p.get_map())
        os << it.first << " = " << it.second << '\n';
    return os;
}

namespace fec {

namespace {

constexpr size_t kAlign = 64;  // row stride granule (u16 words)

size_t pad_words(size_t w)
{
    return std::max<size_t>(kAlign, (w + kAlign - 1) / kAlign * kAlign);
}

void check(hipError_t e, const char* what)
{
    if (e != hipSuccess)
        throw std::runtime_error(std::string("HIP error in ") + what + ": " +
                                 hipGetErrorString(e));
}

void check_rc(int rc, const char* what)
{
    if (rc != 0)
        throw std::runtime_error(std::string(what) + " failed: " +
                                 std::to_string(rc));
}

void reserve(DevBuf& b, size_t bytes)
{
    if (!b.reserve(bytes))
        throw std::runtime_error("RsFnt: device allocation failed");
}

void h2d(void* dst, const void* src, size_t bytes, hipStream_t s)
{
    check(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), "H2D");
}

void d2h(void* dst, const void* src, size_t bytes, hipStream_t s)
{
    check(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s), "D2H");
}

// the bucket counts back from the device (synchronises s): the largest
size_t read_max(std::vector<uint32_t>& cnt, const void* dcnt, hipStream_t s)
{
    d2h(cnt.data(), dcnt, cnt.size() * 4, s);
    check(hipStreamSynchronize(s), "sync");
    return *std::max_element(cnt.begin(), cnt.end());
}

void upload_marks(const stage::PackedMarks& pm, uint32_t* dcnt, uint32_t* dent, hipStream_t s)
{
    h2d(dcnt, pm.counts.data(), pm.counts.size() * 4, s);
    h2d(dent, pm.entries.data(), pm.entries.size() * 4, s);
}

stage::FragMap frag_map(const RsFnt& f)
{
    return stage::FragMap(f.type, f.n_data, f.n_outputs);
}

struct Timer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    uint64_t usec() const
    {
        return static_cast<uint64_t>(
            std::chrono::duration_cast<std::chrono::microseconds>(
                std::chrono::steady_clock::now() - t0)
                .count());
    }
};

}  // namespace

RsFnt::RsFnt(FecType t, unsigned ws, unsigned k, unsigned m, size_t pkt)
    : type(t), word_size(ws), n_data(k), n_parities(m), code_len(k + m),
      n_outputs(t == FecType::SYSTEMATIC ? m : k + m), pkt_size(pkt),
      buf_size(pkt * ws), n(0)
{
    if (ws != 2)
        throw std::invalid_argument(
            "RsFnt: only word_size 2 (GF(65537)) is supported");
    if (k < 1 || m < 1 || pkt < 1)
        throw std::invalid_argument("RsFnt: bad parameters");
    plan_ = qi_plan_create(static_cast<int>(k), static_cast<int>(m),
                           t == FecType::SYSTEMATIC ? 1 : 0);
    if (!plan_)
        throw std::runtime_error(
            "RsFnt: cannot create the GPU plan (no HIP device)");
    n = static_cast<unsigned>(qi_plan_n(plan_));
    const hipError_t e =
        hipStreamCreateWithFlags(&plan_->host.stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        // the destructor does not run for a throwing constructor
        qi_plan_destroy(plan_);
        plan_ = nullptr;
        check(e, "hipStreamCreate");
    }
}

RsFnt::~RsFnt()
{
    pipe_.reset();
    qi_plan_destroy(hplan_);
    qi_plan_destroy(plan_);
}

qi_plan* RsFnt::hplan()
{
    if (hplan_)
        return hplan_;
    qi_plan* p = qi_plan_create(static_cast<int>(n_data), static_cast<int>(n - n_data), 0);
    if (!p)
        throw std::runtime_error("RsFnt: cannot create the GPU plan");
    const hipError_t e = hipStreamCreateWithFlags(&p->host.stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        qi_plan_destroy(p);
        check(e, "hipStreamCreate");
    }
    hplan_ = p;
    return p;
}

int RsFnt::get_n_outputs() const
{
    // src/fec_rs_fnt.h:165-168
    return type == FecType::SYSTEMATIC ? static_cast<int>(n_parities)
                                       : static_cast<int>(n);
}

void RsFnt::encode_columns(qi_plan* pl, const uint8_t* const* data, uint8_t* const* outputs,
                           size_t words, std::vector<Properties>& props,
                           size_t offset)
{
    if (words == 0)
        return;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    const size_t P = pad_words(words);
    const size_t no = static_cast<size_t>(pl->n_outputs);
    reserve(h.in, static_cast<size_t>(pl->k) * P * 2);
    reserve(h.out, no * P * 2);
    reserve(h.counts, no * 4);
    uint16_t* din = static_cast<uint16_t*>(h.in.p);
    uint16_t* dout = static_cast<uint16_t*>(h.out.p);
    uint32_t* dcnt = static_cast<uint32_t*>(h.counts.p);
    for (int t = 0; t < pl->k; t++)
        h2d(din + t * P, data[t], words * 2, s);
    std::vector<uint32_t> cnt(no);
    const size_t cap = stage::run_with_retry(
        64 + words / 512,
        [&](size_t c) {
            reserve(h.entries, no * c * 4);
            check_rc(qi_gpu_oor_clear(dcnt, no, s), "oor_clear");
            check_rc(qi_gpu_encode(pl, din, 0, static_cast<long long>(P), dout, 0,
                                   static_cast<long long>(P), static_cast<long long>(words), 1,
                                   dcnt, static_cast<uint32_t*>(h.entries.p),
                                   static_cast<int>(c), s),
                     "qi_gpu_encode");
        },
        [&] { return read_max(cnt, dcnt, s); }, [] {});
    std::vector<uint32_t> ent(no * cap);
    d2h(ent.data(), h.entries.p, no * cap * 4, s);
    for (size_t i = 0; i < no; i++)
        if (outputs[i])
            d2h(outputs[i], dout + i * P, words * 2, s);
    check(hipStreamSynchronize(s), "sync");
    for (size_t i = 0; i < no; i++)
        stage::add_sorted(props[i], ent.data() + i * cap, cnt[i], offset);
}

void RsFnt::decode_columns(qi_plan* pl, const std::vector<int>& ids,
                           const std::vector<const uint8_t*>& rows,
                           const std::vector<const Properties*>& props,
                           uint8_t* const* outputs, size_t words,
                           size_t offset)
{
    if (words == 0)
        return;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    const size_t P = pad_words(words);
    const int k = pl->k;
    // OOR marks of the received coded rows inside [offset, offset+words)
    const stage::PackedMarks pm = stage::pack_marks(props, offset, words);
    const size_t cap = pm.cap;
    std::vector<uint16_t> hids(ids.begin(), ids.end());
    const size_t ctx_bytes =
        qi_gpu_decode_ctx_bytes(pl, 1, static_cast<long long>(words));
    // counts buffer: counts, entries
    const auto off = stage::layout({size_t(k) * 4, pm.entries.size() * 4});
    reserve(h.in, static_cast<size_t>(k) * P * 2);
    reserve(h.out, static_cast<size_t>(k) * P * 2);
    reserve(h.counts, off[2]);
    reserve(h.ids, k * 2);
    reserve(h.ctx, ctx_bytes);
    uint16_t* din = static_cast<uint16_t*>(h.in.p);
    uint16_t* dout = static_cast<uint16_t*>(h.out.p);
    // received rows staged by position; OOR buckets by position
    uint32_t* dcnt = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(h.counts.p) + off[0]);
    uint32_t* dent = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(h.counts.p) + off[1]);
    for (int i = 0; i < k; i++)
        h2d(din + i * P, rows[i], words * 2, s);
    upload_marks(pm, dcnt, dent, s);
    h2d(h.ids.p, hids.data(), k * 2, s);
    check_rc(qi_gpu_decode_ctx_packed(pl, static_cast<uint16_t*>(h.ids.p), hids.data(), 1,
                                      dcnt, dent, static_cast<int>(cap),
                                      static_cast<long long>(words), h.ctx.p, s),
             "decode context");
    check_rc(qi_gpu_decode_packed(pl, h.ctx.p, din, 0, static_cast<long long>(P), dcnt,
                                  dent, static_cast<int>(cap), dout, 0,
                                  static_cast<long long>(P), static_cast<long long>(words), 1,
                                  s),
             "decode");
    for (int t = 0; t < k; t++)
        if (outputs[t])
            d2h(outputs[t], dout + t * P, words * 2, s);
    check(hipStreamSynchronize(s), "sync");
    if (qi_gpu_take_error(pl))
        throw std::runtime_error("RsFnt: OOR marks lost (bucket capacity)");
}

void RsFnt::encode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                   std::vector<uint8_t*>& parities_bufs,
                                   std::vector<Properties>& parities_props,
                                   std::vector<bool>& wanted_idxs,
                                   size_t block_size_bytes)
{
    // src/fec_base.h:1066-1151
    for (auto& p : parities_props)
        p.clear();
    reset_stats_enc();
    const size_t words = block_size_bytes / word_size;
    std::vector<uint8_t*> outs(n_outputs, nullptr);
    for (unsigned i = 0; i < n_outputs; i++)
        if (wanted_idxs[i])
            outs[i] = parities_bufs[i];
    Timer tm;
    if (!encode_blocks_pipe(data_bufs, outs, parities_props, words)) {
        encode_columns(plan_, data_bufs.data(), outs.data(), words, parities_props, 0);
        n_encode_ops++;
    }
    total_enc_usec += tm.usec();
}

namespace {

// the k selected fragments by position: where each one comes from (`data`
// or `coded`, by slot) and, for a coded one, its marks
template <typename T, typename R>
void selected_rows(const stage::FragMap& map, const std::vector<int>& ids,
                   const std::vector<T>& data, const std::vector<T>& coded,
                   std::vector<Properties>& coded_props, std::vector<R>& rows,
                   std::vector<const Properties*>& props)
{
    for (size_t i = 0; i < ids.size(); i++) {
        const auto fs = map.slot(ids[i]);
        rows[i] = map.pick(ids[i], data, coded);
        props[i] = fs.is_data ? nullptr : &coded_props[fs.slot];
    }
}

}  // namespace

bool RsFnt::decode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                   std::vector<uint8_t*>& parities_bufs,
                                   std::vector<Properties>& parities_props,
                                   std::vector<int>& missing_idxs,
                                   std::vector<bool>& wanted_idxs,
                                   size_t block_size_bytes)
{
    // src/fec_base.h:1177-1321
    const stage::FragMap map = frag_map(*this);
    const std::vector<int> present = map.present(missing_idxs);
    if (map.data_in_clear(present))
        return true;
    std::vector<int> ids;
    if (!map.select(present, ids))
        return false;
    // DecodeContext sorts every input property list (src/fec_context.h:93-97)
    for (auto& p : parities_props)
        p.sort();
    reset_stats_dec();
    std::vector<const uint8_t*> rows(n_data);
    std::vector<const Properties*> props(n_data, nullptr);
    selected_rows(map, ids, data_bufs, parities_bufs, parities_props, rows, props);
    std::vector<uint8_t*> outs(n_data, nullptr);
    for (unsigned t = 0; t < n_data; t++)
        if (wanted_idxs[t])
            outs[t] = data_bufs[t];
    Timer tm;
    const size_t words = block_size_bytes / word_size;
    if (!decode_blocks_pipe(ids, rows, props, outs, words)) {
        decode_columns(plan_, ids, rows, props, outs.data(), words, 0);
        n_decode_ops++;
    }
    total_dec_usec += tm.usec();
    return true;
}

namespace {

size_t chunk_bytes(size_t buf_size)
{
    const size_t target = 4u << 20;
    return buf_size * std::max<size_t>(1, target / buf_size);
}

// read up to `len` bytes; returns bytes read (short = end of stream)
size_t read_full(std::istream* is, uint8_t* p, size_t len)
{
    is->read(reinterpret_cast<char*>(p), static_cast<std::streamsize>(len));
    return static_cast<size_t>(is->gcount());
}

}  // namespace

// ---- fused repair and verify (single chunk; qi_gpu_repair_ctx, then
// qi_gpu_repair / qi_gpu_verify) ----
bool RsFnt::repair_supported(size_t n_targets, size_t block_size_bytes) const
{
    const size_t words = block_size_bytes / word_size;
    if (n_data > 256 || n_targets < 1 || n_targets > std::min<size_t>(64, n - n_data))
        return false;
    if (words == 0 || words > chunk_bytes(buf_size) / 2)
        return false;  // wider blocks go through the chunk pipeline
    // every fragment of the code has a row slot on the device (the context
    // addresses rows by fragment id)
    return static_cast<size_t>(code_len) * pad_words(words) * 2 <= (size_t{256} << 20);
}

namespace {

// What a repair and a verify stage alike: the fragments `upload` in their own
// row slots of h.in (row = fragment id: the data rows first when systematic,
// then the coded rows), the coded ones' OOR buckets by slot at the head of
// h.counts, followed by `tail_bytes` for the caller's own results; h.ids and
// h.ctx reserved.  offset: the first column staged (marks relative to it).
struct Staged {
    size_t P;
    uint16_t *din, *dcoded;
    uint32_t *dcnt, *dent, *dtail;
    stage::PackedMarks pm;  // host side of the buckets: alive until the sync
};

Staged stage_fragments(qi_plan* pl, const stage::FragMap& map, const std::vector<int>& upload,
                       const std::vector<uint8_t*>& data_bufs,
                       const std::vector<uint8_t*>& parities_bufs,
                       const std::vector<Properties>& parities_props, size_t words,
                       size_t tail_bytes, size_t n_ids, size_t ctx_bytes, size_t offset = 0)
{
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    Staged st;
    const size_t P = st.P = pad_words(words), no = map.n_outputs;
    std::vector<const Properties*> marked(no, nullptr);
    for (int id : upload) {
        const auto fs = map.slot(id);
        if (!fs.is_data)
            marked[fs.slot] = &parities_props[fs.slot];
    }
    st.pm = stage::pack_marks(marked, offset, words);
    const auto off = stage::layout({no * 4, st.pm.entries.size() * 4, tail_bytes});
    reserve(h.in, (map.data_rows() + no) * P * 2);
    reserve(h.counts, off[3]);
    reserve(h.ids, n_ids * 2);
    reserve(h.ctx, ctx_bytes);
    uint8_t* dcb = static_cast<uint8_t*>(h.counts.p);
    st.din = static_cast<uint16_t*>(h.in.p);
    st.dcoded = st.din + map.data_rows() * P;
    st.dcnt = reinterpret_cast<uint32_t*>(dcb + off[0]);
    st.dent = reinterpret_cast<uint32_t*>(dcb + off[1]);
    st.dtail = reinterpret_cast<uint32_t*>(dcb + off[2]);
    for (int id : upload)
        h2d(st.din + id * P, map.pick(id, data_bufs, parities_bufs) + offset * 2, words * 2, s);
    upload_marks(st.pm, st.dcnt, st.dent, s);
    return st;
}

// The compact sibling, for the calls that address rows by position (update,
// the shares, the syndrome locate): `n_rows` row slots in h.in, of which the
// rows `up` are uploaded, in that order, to the slots they name; the M mark
// groups' buckets (counts, then entries, per group) at the head of h.counts,
// followed by `tail_bytes`; h.ids holds `hids`; h.ctx is reserved.  Uploads:
// the rows, the marks, the ids.
struct RowUpload {
    const uint8_t* src;
    size_t row;
};

template <size_t M>
struct StagedRows {
    size_t P;
    uint16_t* din;
    uint32_t *dcnt[M], *dent[M], *dtail;
    const uint16_t* dids;
    stage::PackedMarks pm[M];  // host side of the buckets: alive until the sync
};

template <size_t M>
StagedRows<M> stage_rows(qi_plan* pl, size_t n_rows, const std::vector<RowUpload>& up,
                         const std::vector<const Properties*> (&marks)[M], size_t words,
                         size_t tail_bytes, const std::vector<uint16_t>& hids, size_t ctx_bytes)
{
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    StagedRows<M> st;
    const size_t P = st.P = pad_words(words);
    size_t bytes[2 * M + 1];
    for (size_t g = 0; g < M; g++) {
        st.pm[g] = stage::pack_marks(marks[g], 0, words);
        bytes[2 * g] = marks[g].size() * 4;
        bytes[2 * g + 1] = st.pm[g].entries.size() * 4;
    }
    bytes[2 * M] = tail_bytes;
    const auto off = stage::layout(bytes);
    reserve(h.in, n_rows * P * 2);
    reserve(h.counts, off[2 * M + 1]);
    reserve(h.ids, hids.size() * 2);
    reserve(h.ctx, ctx_bytes);
    uint8_t* dcb = static_cast<uint8_t*>(h.counts.p);
    st.din = static_cast<uint16_t*>(h.in.p);
    for (size_t g = 0; g < M; g++) {
        st.dcnt[g] = reinterpret_cast<uint32_t*>(dcb + off[2 * g]);
        st.dent[g] = reinterpret_cast<uint32_t*>(dcb + off[2 * g + 1]);
    }
    st.dtail = reinterpret_cast<uint32_t*>(dcb + off[2 * M]);
    st.dids = static_cast<uint16_t*>(h.ids.p);
    for (auto const& u : up)
        h2d(st.din + u.row * P, u.src, words * 2, s);
    for (size_t g = 0; g < M; g++)
        upload_marks(st.pm[g], st.dcnt[g], st.dent[g], s);
    h2d(h.ids.p, hids.data(), hids.size() * 2, s);
    return st;
}

// The tail of every call that leaves R marked rows (repair, update, the
// shares): launch(entries, cap) into the cleared counts `docnt`, first with
// 64 + words / 512 entries per row and, if a row has more marks, once more
// with the exact capacity after between() has put back what the first attempt
// overwrote.  No error drain between the attempts: the sticky error is read
// once, after the rows drows[j * P] are back in rows_out[j] (null: not
// wanted).  Returns the R ascending mark lists.
template <typename Launch, typename Between>
std::vector<Properties> finish_marked_rows(qi_plan* pl, size_t R, size_t words, uint32_t* docnt,
                                           Launch launch, Between between,
                                           const uint16_t* drows, size_t P,
                                           uint8_t* const* rows_out, const char* what)
{
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    std::vector<uint32_t> ocnt(R);
    const size_t ocap = stage::run_with_retry(
        64 + words / 512,
        [&](size_t c) {
            reserve(h.entries, R * c * 4);
            check_rc(qi_gpu_oor_clear(docnt, R, s), "oor_clear");
            launch(static_cast<uint32_t*>(h.entries.p), static_cast<int>(c));
        },
        [&] { return read_max(ocnt, docnt, s); }, between);
    std::vector<uint32_t> ent(R * ocap);
    d2h(ent.data(), h.entries.p, R * ocap * 4, s);
    for (size_t j = 0; j < R; j++)
        if (rows_out[j])
            d2h(rows_out[j], drows + j * P, words * 2, s);
    check(hipStreamSynchronize(s), "sync");
    if (qi_gpu_take_error(pl))
        throw std::runtime_error(std::string("RsFnt: ") + what +
                                 " failed (bad ids or OOR bucket capacity)");
    std::vector<Properties> marks(R);
    for (size_t j = 0; j < R; j++)
        stage::add_sorted(marks[j], ent.data() + j * ocap, ocnt[j], 0);
    return marks;
}

// The tail of the two locates: launch(fixes, cap) leaves located[N],
// unlocated, the fix count and the weights in `dres`, of which T_read words
// are read back (the read synchronises).  A fix list longer than the capacity
// is run again with the exact one; an overflowing fix list raises no error, so
// there is nothing to drain.  Fills the reset `result`: fix positions become
// fragment ids through `ids`.
template <typename Launch>
void finish_fix_list(qi_plan* pl, size_t words, size_t T_read, const uint32_t* dres,
                     Launch launch, const std::vector<int>& ids, LocateResult& result,
                     const char* what)
{
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    const size_t N = ids.size();
    std::vector<uint32_t> res(T_read);
    const size_t fcap = stage::run_with_retry(
        64 + words / 512,
        [&](size_t c) {
            reserve(h.entries, c * 3 * 4);
            launch(static_cast<uint32_t*>(h.entries.p), static_cast<int>(c));
        },
        [&] {
            d2h(res.data(), dres, T_read * 4, s);
            check(hipStreamSynchronize(s), "sync");
            return static_cast<size_t>(res[N + 1]);
        },
        [] {});
    const size_t nfix = res[N + 1];
    if (nfix > fcap)
        throw std::runtime_error(std::string("RsFnt: ") + what + " fix list overflowed twice");
    std::vector<uint32_t> fx(nfix * 3);
    if (nfix)
        d2h(fx.data(), h.entries.p, nfix * 3 * 4, s);
    check(hipStreamSynchronize(s), "sync");
    if (qi_gpu_take_error(pl))
        throw std::runtime_error(std::string("RsFnt: ") + what +
                                 " failed (bad ids or OOR bucket capacity)");
    stage::fill_locate(result, ids, res.data(), fx.data(), nfix);
}

}  // namespace

bool RsFnt::repair_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                   std::vector<uint8_t*>& parities_bufs,
                                   std::vector<Properties>& parities_props,
                                   std::vector<int>& missing_idxs,
                                   const std::vector<int>& targets,
                                   std::vector<uint8_t*>& out_bufs,
                                   std::vector<Properties>& out_props,
                                   size_t block_size_bytes)
{
    // validate
    const stage::FragMap map = frag_map(*this);
    const size_t R = targets.size();
    if (!repair_supported(R, block_size_bytes))
        throw std::invalid_argument("RsFnt::repair_blocks_vertical: unsupported shape");
    if (out_bufs.size() < R)
        throw std::invalid_argument("RsFnt::repair_blocks_vertical: out_bufs");
    const std::vector<int> present = map.present(missing_idxs);
    for (int t : targets)
        if (t < 0 || t >= static_cast<int>(code_len) || present[t])
            throw std::invalid_argument("RsFnt::repair_blocks_vertical: target not missing");
    std::vector<int> ids;
    if (!map.select(present, ids))
        return false;
    for (auto& p : parities_props)
        p.sort();
    out_props.assign(R, Properties());
    const size_t words = block_size_bytes / word_size;
    const int k = static_cast<int>(n_data);
    qi_plan* pl = plan_;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    const size_t ctx_bytes = qi_gpu_repair_ctx_bytes(pl, static_cast<int>(R), 1,
                                                     static_cast<long long>(words));
    if (ctx_bytes == 0)
        throw std::invalid_argument("RsFnt::repair_blocks_vertical: unsupported shape");
    // stage: the k selected rows, their buckets, then the output counts
    reserve(h.out, R * pad_words(words) * 2);
    const Staged st = stage_fragments(pl, map, ids, data_bufs, parities_bufs, parities_props,
                                      words, R * 4, k + R, ctx_bytes);
    const long long P = static_cast<long long>(st.P);
    const int cap = static_cast<int>(st.pm.cap);
    uint16_t* dout = static_cast<uint16_t*>(h.out.p);
    uint32_t* docnt = st.dtail;
    std::vector<uint16_t> hids(ids.begin(), ids.end());
    hids.insert(hids.end(), targets.begin(), targets.end());
    h2d(h.ids.p, hids.data(), (k + R) * 2, s);
    const uint16_t* dids = static_cast<uint16_t*>(h.ids.p);
    check_rc(qi_gpu_repair_ctx(pl, dids, dids + k, static_cast<int>(R), 1, st.dcnt, st.dent, cap,
                               static_cast<long long>(words), h.ctx.p, s),
             "repair context");
    // launch and collect (a null out_bufs[j] is a row not wanted)
    out_props = finish_marked_rows(
        pl, R, words, docnt,
        [&](uint32_t* oent, int ocap) {
            check_rc(qi_gpu_repair(pl, h.ctx.p, static_cast<int>(R), st.din, 0, P, st.dcoded, 0,
                                   P, st.dcnt, st.dent, cap, dout, 0, P, docnt, oent, ocap,
                                   static_cast<long long>(words), 1, s),
                     "repair");
        },
        [] {}, dout, st.P, out_bufs.data(), "repair");
    return true;
}

bool RsFnt::verify_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                   std::vector<uint8_t*>& parities_bufs,
                                   std::vector<Properties>& parities_props,
                                   std::vector<int>& missing_idxs,
                                   std::vector<VerifyResult>& result, size_t block_size_bytes)
{
    // validate (the staging of a repair; the group size is checked per group)
    const stage::FragMap map = frag_map(*this);
    if (!repair_supported(1, block_size_bytes))
        throw std::invalid_argument("RsFnt::verify_blocks_vertical: unsupported shape");
    const std::vector<int> present = map.present(missing_idxs);
    result.assign(code_len, VerifyResult{-1, -1, -1});
    std::vector<int> ids;
    if (!map.select(present, ids))
        return false;
    const int k = static_cast<int>(n_data);
    std::vector<char> basis(code_len, 0);
    for (int id : ids)
        basis[id] = 1;
    std::vector<int> held, checks;
    for (unsigned f = 0; f < code_len; f++) {
        if (present[f])
            held.push_back(static_cast<int>(f));
        if (present[f] && !basis[f])
            checks.push_back(static_cast<int>(f));
    }
    if (checks.empty())
        return false;  // fewer than n_data + 1 fragments: nothing to check against
    for (auto& p : parities_props)
        p.sort();
    const size_t words = block_size_bytes / word_size;
    qi_plan* pl = plan_;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    const size_t Rmax = std::min<size_t>({size_t{64}, checks.size(), code_len - n_data});
    const size_t ctx_bytes = qi_gpu_repair_ctx_bytes(pl, static_cast<int>(Rmax), 1,
                                                     static_cast<long long>(words));
    if (ctx_bytes == 0)
        throw std::invalid_argument("RsFnt::verify_blocks_vertical: unsupported shape");
    // stage: every present fragment, the buckets, then the three results
    const Staged st = stage_fragments(pl, map, held, data_bufs, parities_bufs, parities_props,
                                      words, 3 * Rmax * 4, k + Rmax, ctx_bytes);
    const long long P = static_cast<long long>(st.P);
    const int cap = static_cast<int>(st.pm.cap);
    uint32_t* dres = st.dtail;
    const uint16_t* dids = static_cast<uint16_t*>(h.ids.p);
    std::vector<uint16_t> hids(ids.begin(), ids.end());
    hids.resize(k + Rmax);
    std::vector<uint32_t> res(3 * Rmax);
    size_t wcap = 64 + words / 512;
    // launch: groups of at most 64 checks over the same staged rows
    for (size_t g0 = 0; g0 < checks.size(); g0 += Rmax) {
        const size_t R = std::min(Rmax, checks.size() - g0);
        for (size_t j = 0; j < R; j++)
            hids[k + j] = static_cast<uint16_t>(checks[g0 + j]);
        // (the previous group's kernels read the ids: ordered on the stream,
        // and the host copy is synchronous with respect to hids below)
        h2d(h.ids.p, hids.data(), (k + R) * 2, s);
        check_rc(qi_gpu_repair_ctx(pl, dids, dids + k, static_cast<int>(R), 1, st.dcnt, st.dent,
                                   cap, static_cast<long long>(words), h.ctx.p, s),
                 "verify context");
        std::vector<uint32_t> wc(R);
        // adversarial data: more recomputed 65536 values than the work
        // buckets hold; the error that attempt raised is drained before the
        // next one, and a capacity that grew is kept for the later groups
        wcap = stage::run_with_retry(
            wcap,
            [&](size_t c) {
                const size_t wb = qi_gpu_verify_work_bytes(pl, static_cast<int>(R), 1,
                                                           static_cast<int>(c));
                if (!wb)
                    throw std::runtime_error("RsFnt: device allocation failed");
                reserve(h.entries, wb);
                check_rc(qi_gpu_verify(pl, h.ctx.p, static_cast<int>(R), dids + k, st.din, 0, P,
                                       st.dcoded, 0, P, st.dcnt, st.dent, cap, h.entries.p,
                                       static_cast<int>(c), dres, dres + R, dres + 2 * R,
                                       static_cast<long long>(words), 1, s),
                         "verify");
            },
            [&] {
                d2h(res.data(), dres, 3 * R * 4, s);
                return read_max(wc, h.entries.p, s);
            },
            [&] { (void)qi_gpu_take_error(pl); });
        if (qi_gpu_take_error(pl))
            throw std::runtime_error("RsFnt: verify failed (bad ids or OOR bucket capacity)");
        // collect
        for (size_t j = 0; j < R; j++)
            result[checks[g0 + j]] = VerifyResult{static_cast<long long>(res[j]),
                                                  static_cast<long long>(res[R + j]),
                                                  static_cast<long long>(res[2 * R + j])};
    }
    return true;
}

// ---- fragment locate (single chunk; qi_gpu_locate_ctx, then qi_gpu_locate
// over the staged rows) ----
bool RsFnt::locate_supported(size_t block_size_bytes) const
{
    return code_len - n_data >= 2 && repair_supported(1, block_size_bytes);
}

int RsFnt::locate_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                  std::vector<uint8_t*>& parities_bufs,
                                  std::vector<Properties>& parities_props,
                                  std::vector<int>& missing_idxs, LocateResult& result,
                                  bool correct, size_t block_size_bytes, size_t max_marks)
{
    return locate_run(data_bufs, parities_bufs, parities_props, missing_idxs, result, 0, correct,
                      block_size_bytes, max_marks);
}

int RsFnt::locate_multi_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                        std::vector<uint8_t*>& parities_bufs,
                                        std::vector<Properties>& parities_props,
                                        std::vector<int>& missing_idxs, LocateResult& result,
                                        int max_errors, bool correct, size_t block_size_bytes,
                                        size_t max_marks)
{
    if (max_errors < 1 || max_errors > QI_LOCATE_MAX_ERRORS)
        throw std::invalid_argument("RsFnt::locate_multi_blocks_vertical: max_errors");
    return locate_run(data_bufs, parities_bufs, parities_props, missing_idxs, result, max_errors,
                      correct, block_size_bytes, max_marks);
}

// max_errors = t: 0 runs qi_gpu_locate, 1 .. 4 qi_gpu_locate_multi, whose
// weights follow the fix count in the tail
int RsFnt::locate_run(std::vector<uint8_t*>& data_bufs, std::vector<uint8_t*>& parities_bufs,
                      std::vector<Properties>& parities_props, std::vector<int>& missing_idxs,
                      LocateResult& result, int t, bool correct, size_t block_size_bytes,
                      size_t max_marks)
{
    // validate
    const stage::FragMap map = frag_map(*this);
    if (!locate_supported(block_size_bytes))
        throw std::invalid_argument("RsFnt::locate_blocks_vertical: unsupported shape");
    const std::vector<int> present = map.present(missing_idxs);
    stage::reset_locate(result, code_len, t);
    const std::vector<int> ids = map.select_upto(present, n_data + QI_LOCATE_MAX_CHECKS);
    if (ids.size() < n_data + 2)
        return 0;
    const size_t N = ids.size();
    const int R = static_cast<int>(N - n_data);
    if (R < 2 * t)
        return 0;
    for (auto& p : parities_props)
        p.sort();
    const size_t words = block_size_bytes / word_size;
    qi_plan* pl = plan_;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    const size_t ctx_bytes = qi_gpu_locate_ctx_bytes(pl, R, 1);
    if (ctx_bytes == 0)
        throw std::invalid_argument("RsFnt::locate_blocks_vertical: unsupported shape");
    // stage: the listed rows, their buckets, then located[N], unlocated, the
    // fix count and the weights
    const size_t T = N + 2 + QI_LOCATE_MAX_ERRORS;
    const Staged st = stage_fragments(pl, map, ids, data_bufs, parities_bufs, parities_props,
                                      words, T * 4, N, ctx_bytes);
    const long long P = static_cast<long long>(st.P);
    const int cap = static_cast<int>(st.pm.cap);
    uint32_t* dres = st.dtail;
    const std::vector<uint16_t> hids(ids.begin(), ids.end());
    h2d(h.ids.p, hids.data(), N * 2, s);
    check_rc(qi_gpu_locate_ctx(pl, static_cast<uint16_t*>(h.ids.p), R, 1, h.ctx.p, s),
             "locate context");
    // launch and collect (the single locate writes no weights: N + 2 words)
    finish_fix_list(
        pl, words, t ? T : N + 2, dres,
        [&](uint32_t* fixes, int fcap) {
            const long long w = static_cast<long long>(words);
            if (t == 0)
                check_rc(qi_gpu_locate(pl, h.ctx.p, R, nullptr, st.din, 0, P, st.dcoded, 0, P,
                                       st.dcnt, st.dent, cap, dres, dres + N, dres + N + 1, fixes,
                                       fcap, w, 1, s),
                         "locate");
            else
                check_rc(qi_gpu_locate_multi(pl, h.ctx.p, R, t, nullptr, st.din, 0, P, st.dcoded,
                                             0, P, st.dcnt, st.dent, cap, dres, dres + N,
                                             dres + N + 2, dres + N + 1, fixes, fcap, w, 1, s),
                         "locate");
        },
        ids, result, "locate");
    if (!correct || result.fixes.empty() || result.unlocated != 0)
        return 1;
    if (!stage::apply_fixes(map, result.fixes, data_bufs, parities_bufs, parities_props,
                            max_marks))
        throw std::length_error("RsFnt::locate_blocks_vertical: mark list capacity");
    return 2;
}

// ---- fragment fingerprints (qi_gpu_fingerprint over the staged rows, in
// column chunks that fit the staging) ----
void RsFnt::fingerprint_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                        std::vector<uint8_t*>& parities_bufs,
                                        std::vector<Properties>& parities_props,
                                        std::vector<int>& missing_idxs, const uint32_t* keys,
                                        int n_keys, std::vector<long long>& result,
                                        size_t block_size_bytes)
{
    // validate
    if (!keys || n_keys < 1 || n_keys > QI_FINGERPRINT_MAX_KEYS)
        throw std::invalid_argument("RsFnt::fingerprint_blocks_vertical: n_keys");
    for (int e = 0; e < 3 * n_keys; e++)
        if (keys[e] < 1 || keys[e] > 65536)
            throw std::invalid_argument("RsFnt::fingerprint_blocks_vertical: key out of range");
    const size_t F = static_cast<size_t>(n_keys);
    const size_t words = block_size_bytes / word_size;
    if (words == 0 || words > (size_t{1} << 32))
        throw std::invalid_argument("RsFnt::fingerprint_blocks_vertical: block size");
    const stage::FragMap map = frag_map(*this);
    const std::vector<int> present = map.present(missing_idxs);
    result.assign(code_len * F, -1);
    std::vector<int> held;
    for (unsigned f = 0; f < code_len; f++)
        if (present[f])
            held.push_back(static_cast<int>(f));
    if (held.empty())
        return;
    const size_t N = held.size();
    for (auto& p : parities_props)
        p.sort();
    // the chunk: every fragment of the code has a row slot on the device (at
    // most 256 MiB of rows), rows of whole kAlign granules
    const size_t slots = map.data_rows() + map.n_outputs;
    size_t chunk = std::max<size_t>(kAlign, (size_t{256} << 20) / (2 * slots) / kAlign * kAlign);
    chunk = std::min(chunk, chunk_bytes(buf_size) / 2);
    if (const char* env = std::getenv("QI_FINGERPRINT_CHUNK_WORDS")) {
        const long long v = std::atoll(env);
        if (v > 0)
            chunk = std::min(chunk, static_cast<size_t>(v));
    }
    qi_plan* pl = plan_;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    const std::vector<uint16_t> hids(held.begin(), held.end());
    std::vector<uint32_t> sum(N * F, 0), res(N * F);
    for (size_t c0 = 0; c0 < words; c0 += chunk) {
        const size_t w = std::min(chunk, words - c0);
        // stage: the present rows' columns [c0, c0 + w), their buckets, then
        // the fingerprints
        const Staged st = stage_fragments(pl, map, held, data_bufs, parities_bufs, parities_props,
                                          w, N * F * 4, N, 0, c0);
        const size_t wb = qi_gpu_fingerprint_work_bytes(pl, static_cast<int>(N), n_keys, 1,
                                                        static_cast<long long>(w));
        if (!wb)
            throw std::runtime_error("RsFnt: fingerprint work size");
        reserve(h.entries, wb);
        h2d(h.ids.p, hids.data(), N * 2, s);
        const long long P = static_cast<long long>(st.P);
        // launch
        check_rc(qi_gpu_fingerprint(pl, static_cast<uint16_t*>(h.ids.p), static_cast<int>(N),
                                    keys, n_keys, static_cast<long long>(c0), st.din, 0, P,
                                    st.dcoded, 0, P, st.dcnt, st.dent,
                                    static_cast<int>(st.pm.cap), h.entries.p, st.dtail,
                                    static_cast<long long>(w), 1, s),
                 "fingerprint");
        // collect
        d2h(res.data(), st.dtail, N * F * 4, s);
        check(hipStreamSynchronize(s), "sync");
        if (qi_gpu_take_error(pl))
            throw std::runtime_error("RsFnt: fingerprint failed (bad ids or OOR bucket capacity)");
        for (size_t e = 0; e < N * F; e++)
            sum[e] = (sum[e] + res[e]) % 65537u;
    }
    for (size_t i = 0; i < N; i++)
        for (size_t j = 0; j < F; j++)
            result[held[i] * F + j] = static_cast<long long>(sum[i * F + j]);
}

// ---- delta update (single chunk; qi_gpu_update_ctx, then the update in
// place on the staged rows) ----
bool RsFnt::update_supported(size_t n_rows, size_t n_held, size_t block_size_bytes) const
{
    const size_t words = block_size_bytes / word_size;
    if (n_rows < 1 || n_rows > std::min<size_t>(QI_UPDATE_MAX_ROWS, n_data) || n_held < 1 ||
        n_held > n_outputs)
        return false;
    if (words == 0 || words > chunk_bytes(buf_size) / 2)
        return false;
    // the old and the new rows and the held coded rows, back to back
    return (2 * n_rows + n_held) * pad_words(words) * 2 <= (size_t{256} << 20);
}

void RsFnt::update_blocks_vertical(const std::vector<int>& ids, std::vector<uint8_t*>& old_bufs,
                                   std::vector<uint8_t*>& new_bufs,
                                   std::vector<uint8_t*>& parities_bufs,
                                   std::vector<Properties>& parities_props,
                                   size_t block_size_bytes)
{
    // validate
    const size_t U = ids.size();
    std::vector<uint16_t> held;  // the slots held here, ascending
    for (size_t j = 0; j < n_outputs && j < parities_bufs.size(); j++)
        if (parities_bufs[j])
            held.push_back(static_cast<uint16_t>(j));
    const size_t R = held.size();
    if (!update_supported(U, R, block_size_bytes))
        throw std::invalid_argument("RsFnt::update_blocks_vertical: unsupported shape");
    if (old_bufs.size() < U || new_bufs.size() < U || parities_props.size() < n_outputs)
        throw std::invalid_argument("RsFnt::update_blocks_vertical: buffers");
    for (size_t u = 0; u < U; u++) {
        if (ids[u] < 0 || ids[u] >= static_cast<int>(n_data) || !old_bufs[u] || !new_bufs[u])
            throw std::invalid_argument("RsFnt::update_blocks_vertical: id out of range");
        for (size_t v = 0; v < u; v++)
            if (ids[v] == ids[u])
                throw std::invalid_argument("RsFnt::update_blocks_vertical: id repeated");
    }
    const size_t words = block_size_bytes / word_size;
    qi_plan* pl = plan_;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    // stage: U old rows, U new rows, the R held rows (row j = held[j]: the
    // compact addressing of update_rows), their buckets, the output counts
    std::vector<const Properties*> marked[1] = {std::vector<const Properties*>(R)};
    std::vector<uint8_t*> coded(R);
    std::vector<RowUpload> up;
    for (size_t u = 0; u < U; u++) {
        up.push_back({old_bufs[u], u});
        up.push_back({new_bufs[u], U + u});
    }
    for (size_t j = 0; j < R; j++) {
        parities_props[held[j]].sort();
        marked[0][j] = &parities_props[held[j]];
        coded[j] = parities_bufs[held[j]];
        up.push_back({coded[j], 2 * U + j});
    }
    std::vector<uint16_t> hids(ids.begin(), ids.end());
    hids.insert(hids.end(), held.begin(), held.end());
    const size_t ctx_bytes =
        qi_gpu_update_ctx_bytes(pl, static_cast<int>(U), static_cast<int>(R), 1);
    const StagedRows<1> st = stage_rows(pl, 2 * U + R, up, marked, words, R * 4, hids, ctx_bytes);
    uint16_t* dold = st.din;
    uint16_t* dnew = dold + U * st.P;
    uint16_t* dcoded = dnew + U * st.P;
    uint32_t* docnt = st.dtail;
    check_rc(qi_gpu_update_ctx(pl, st.dids, st.dids + U, static_cast<int>(U),
                               static_cast<int>(R), 1, h.ctx.p, s),
             "update context");
    // launch in place; a second attempt starts from the rows as they were
    const long long Pl = static_cast<long long>(st.P);
    const std::vector<Properties> marks = finish_marked_rows(
        pl, R, words, docnt,
        [&](uint32_t* oent, int ocap) {
            check_rc(update_rows(pl, h.ctx.p, static_cast<int>(U), static_cast<int>(R), 1, dold,
                                 0, Pl, dnew, 0, Pl, dcoded, 0, Pl, st.dcnt[0], st.dent[0],
                                 static_cast<int>(st.pm[0].cap), dcoded, 0, Pl, docnt, oent, ocap,
                                 static_cast<long long>(words), 1, s),
                     "update");
        },
        [&] {
            for (size_t j = 0; j < R; j++)
                h2d(dcoded + j * st.P, coded[j], words * 2, s);
        },
        dcoded, st.P, coded.data(), "update");
    for (size_t j = 0; j < R; j++)
        parities_props[held[j]] = marks[j];
}

// ---- accumulating shares: partial repair and syndrome shares (single chunk;
// the share's context call, then the row call in place on the staged acc
// rows) ----
namespace {

// what tells the two shares apart
struct ShareKind {
    const char* fn;        // the public function: named by invalid_argument
    const char* what;      // named by the runtime errors
    const char* null_out;  // what a null out row is reported as
    const char *ctx_name, *rows_name;
    decltype(&qi_gpu_partial_ctx_bytes) ctx_bytes;
    // the context from the device ids: `listed` ids, the H held positions,
    // then the targets
    int (*ctx)(qi_plan*, const uint16_t* dids, size_t listed, int H, int R, void* dctx,
               hipStream_t s);
    decltype(&qi_gpu_partial) rows;
};

const ShareKind kPartialShare = {
    "RsFnt::partial_repair_blocks_vertical", "partial repair", "bad target", "partial context",
    "partial", qi_gpu_partial_ctx_bytes,
    [](qi_plan* pl, const uint16_t* dids, size_t listed, int H, int R, void* dctx,
       hipStream_t s) {
        return qi_gpu_partial_ctx(pl, dids, dids + listed, dids + listed + H, H, R, 1, dctx, s);
    },
    qi_gpu_partial};

const ShareKind kSyndromeShare = {
    "RsFnt::syndrome_blocks_vertical", "syndrome share", "buffers", "syndrome context",
    "syndrome", qi_gpu_syndrome_ctx_bytes,
    [](qi_plan* pl, const uint16_t* dids, size_t listed, int H, int R, void* dctx,
       hipStream_t s) { return qi_gpu_syndrome_ctx(pl, dids, dids + listed, H, R, 1, dctx, s); },
    qi_gpu_syndrome};

// The share of the R output rows (the targets of a partial repair: then
// `targets` names them; the checks of a syndrome share) that the holder of
// `held_ids`, each one of `listed`, can form: added to out_bufs / out_props
// when acc, else started from 0.  Shapes and buffer counts are the caller's
// to check.
void share_rows(qi_plan* pl, const stage::FragMap& map, const ShareKind& kind,
                const std::vector<int>& listed, const std::vector<int>& held_ids,
                std::vector<uint8_t*>& held_bufs, std::vector<Properties>& held_props,
                const std::vector<int>& targets, size_t R, bool acc,
                std::vector<uint8_t*>& out_bufs, std::vector<Properties>& out_props, size_t words)
{
    // validate; held fragment ids -> positions into listed
    const auto bad = [&](const char* why) {
        return std::invalid_argument(std::string(kind.fn) + ": " + why);
    };
    const size_t H = held_ids.size();
    std::vector<uint16_t> pos;
    const auto hc = stage::held_positions(map.code_len(), listed, targets, held_ids, pos);
    if (hc == stage::HeldCheck::bad_id)
        throw bad("bad id");
    if (hc == stage::HeldCheck::bad_target ||
        std::find(out_bufs.begin(), out_bufs.begin() + R, nullptr) != out_bufs.begin() + R)
        throw bad(kind.null_out);
    if (hc == stage::HeldCheck::bad_held ||
        std::find(held_bufs.begin(), held_bufs.begin() + H, nullptr) != held_bufs.begin() + H)
        throw bad("bad held id");
    std::vector<uint16_t> hids(listed.begin(), listed.end());
    hids.insert(hids.end(), pos.begin(), pos.end());
    hids.insert(hids.end(), targets.begin(), targets.end());
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    // stage: the H held rows, the R output rows, the buckets of both, the
    // output counts
    std::vector<const Properties*> marked[2] = {std::vector<const Properties*>(H, nullptr),
                                                std::vector<const Properties*>(R, nullptr)};
    std::vector<RowUpload> up;
    for (size_t hh = 0; hh < H; hh++) {
        up.push_back({held_bufs[hh], hh});
        if (map.slot(static_cast<unsigned>(held_ids[hh])).is_data)
            continue;
        held_props[hh].sort();
        marked[0][hh] = &held_props[hh];
    }
    for (size_t j = 0; acc && j < R; j++) {
        up.push_back({out_bufs[j], H + j});
        out_props[j].sort();
        marked[1][j] = &out_props[j];
    }
    const size_t ctx_bytes = kind.ctx_bytes(pl, static_cast<int>(H), static_cast<int>(R), 1);
    const StagedRows<2> st = stage_rows(pl, H + R, up, marked, words, R * 4, hids, ctx_bytes);
    uint16_t* dacc = st.din + H * st.P;
    uint32_t* docnt = st.dtail;
    check_rc(kind.ctx(pl, st.dids, listed.size(), static_cast<int>(H), static_cast<int>(R),
                      h.ctx.p, s),
             kind.ctx_name);
    // launch in place; a second attempt starts from the acc rows as they were
    const long long Pl = static_cast<long long>(st.P);
    out_props = finish_marked_rows(
        pl, R, words, docnt,
        [&](uint32_t* oent, int ocap) {
            check_rc(kind.rows(pl, h.ctx.p, static_cast<int>(H), static_cast<int>(R), st.din, 0,
                               Pl, st.dcnt[0], st.dent[0], static_cast<int>(st.pm[0].cap),
                               acc ? dacc : nullptr, 0, Pl, st.dcnt[1], st.dent[1],
                               static_cast<int>(st.pm[1].cap), dacc, 0, Pl, docnt, oent, ocap,
                               static_cast<long long>(words), 1, s),
                     kind.rows_name);
        },
        [&] {
            for (size_t j = 0; acc && j < R; j++)
                h2d(dacc + j * st.P, out_bufs[j], words * 2, s);
        },
        dacc, st.P, out_bufs.data(), kind.what);
}

}  // namespace

// ---- partial repair ----
bool RsFnt::partial_supported(size_t n_held, size_t n_targets, size_t block_size_bytes) const
{
    const size_t words = block_size_bytes / word_size;
    if (n_held < 1 || n_held > n_data || n_targets < 1 ||
        n_targets > std::min<size_t>(QI_PARTIAL_MAX_TARGETS, n_parities))
        return false;
    if (words == 0 || words > chunk_bytes(buf_size) / 2)
        return false;
    // the held rows and the partial rows, back to back
    return (n_held + n_targets) * pad_words(words) * 2 <= (size_t{256} << 20);
}

void RsFnt::partial_repair_blocks_vertical(const std::vector<int>& ids,
                                           const std::vector<int>& held_ids,
                                           std::vector<uint8_t*>& held_bufs,
                                           std::vector<Properties>& held_props,
                                           const std::vector<int>& targets, bool acc,
                                           std::vector<uint8_t*>& out_bufs,
                                           std::vector<Properties>& out_props,
                                           size_t block_size_bytes)
{
    const size_t k = n_data, H = held_ids.size(), R = targets.size();
    if (!partial_supported(H, R, block_size_bytes))
        throw std::invalid_argument("RsFnt::partial_repair_blocks_vertical: unsupported shape");
    if (ids.size() != k || held_bufs.size() < H || held_props.size() < H || out_bufs.size() < R ||
        (acc && out_props.size() < R))
        throw std::invalid_argument("RsFnt::partial_repair_blocks_vertical: buffers");
    share_rows(plan_, frag_map(*this), kPartialShare, ids, held_ids, held_bufs, held_props,
               targets, R, acc, out_bufs, out_props, block_size_bytes / word_size);
}

// ---- syndrome shares, and qi_gpu_syndrome_locate over the summed rows ----
bool RsFnt::syndrome_supported(size_t n_held, size_t n_checks, size_t block_size_bytes) const
{
    const size_t words = block_size_bytes / word_size;
    if (n_checks < 1 || n_checks > std::min<size_t>(QI_SYNDROME_MAX_CHECKS, code_len - n_data) ||
        n_held < 1 || n_held > n_data + n_checks)
        return false;
    if (words == 0 || words > chunk_bytes(buf_size) / 2)
        return false;
    // the held rows and the syndrome rows, back to back
    return (n_held + n_checks) * pad_words(words) * 2 <= (size_t{256} << 20);
}

void RsFnt::syndrome_blocks_vertical(const std::vector<int>& listed_ids,
                                     const std::vector<int>& held_ids,
                                     std::vector<uint8_t*>& held_bufs,
                                     std::vector<Properties>& held_props, int n_checks, bool acc,
                                     std::vector<uint8_t*>& out_bufs,
                                     std::vector<Properties>& out_props, size_t block_size_bytes)
{
    const size_t H = held_ids.size(), R = n_checks < 0 ? 0 : static_cast<size_t>(n_checks);
    if (!syndrome_supported(H, R, block_size_bytes))
        throw std::invalid_argument("RsFnt::syndrome_blocks_vertical: unsupported shape");
    if (listed_ids.size() != n_data + R || held_bufs.size() < H || held_props.size() < H ||
        out_bufs.size() < R || (acc && out_props.size() < R))
        throw std::invalid_argument("RsFnt::syndrome_blocks_vertical: buffers");
    share_rows(plan_, frag_map(*this), kSyndromeShare, listed_ids, held_ids, held_bufs, held_props,
               {}, R, acc, out_bufs, out_props, block_size_bytes / word_size);
}

void RsFnt::locate_syndromes(const std::vector<int>& listed_ids, std::vector<uint8_t*>& syn_bufs,
                             std::vector<Properties>& syn_props, int max_errors,
                             LocateResult& result, size_t block_size_bytes)
{
    // validate
    const size_t N = listed_ids.size();
    const size_t R = N > n_data ? N - n_data : 0;
    const int t = max_errors;
    if (!syndrome_supported(1, R, block_size_bytes) || t < 0 || 2 * static_cast<size_t>(t) > R)
        throw std::invalid_argument("RsFnt::locate_syndromes: unsupported shape");
    if (syn_bufs.size() < R || syn_props.size() < R)
        throw std::invalid_argument("RsFnt::locate_syndromes: buffers");
    std::vector<char> seen(code_len, 0);
    for (int f : listed_ids) {
        if (f < 0 || f >= static_cast<int>(code_len) || seen[f])
            throw std::invalid_argument("RsFnt::locate_syndromes: bad id");
        seen[f] = 1;
    }
    stage::reset_locate(result, code_len, t);
    const size_t words = block_size_bytes / word_size;
    qi_plan* pl = plan_;
    HostState& h = pl->host;
    hipStream_t s = h.stream;
    // stage: the R syndrome rows, their buckets, then located[N], unlocated,
    // the fix count and the weights
    std::vector<const Properties*> marked[1] = {std::vector<const Properties*>(R, nullptr)};
    std::vector<RowUpload> up;
    for (size_t j = 0; j < R; j++) {
        if (!syn_bufs[j])
            throw std::invalid_argument("RsFnt::locate_syndromes: buffers");
        syn_props[j].sort();
        marked[0][j] = &syn_props[j];
        up.push_back({syn_bufs[j], j});
    }
    const size_t T = N + 2 + QI_SYNDROME_MAX_ERRORS;
    const std::vector<uint16_t> hids(listed_ids.begin(), listed_ids.end());
    const size_t ctx_bytes = qi_gpu_syndrome_locate_ctx_bytes(pl, static_cast<int>(R), 1);
    const StagedRows<1> st = stage_rows(pl, R, up, marked, words, T * 4, hids, ctx_bytes);
    uint32_t* dres = st.dtail;
    check_rc(qi_gpu_syndrome_locate_ctx(pl, st.dids, static_cast<int>(R), 1, h.ctx.p, s),
             "syndrome locate context");
    // launch and collect
    finish_fix_list(
        pl, words, T, dres,
        [&](uint32_t* fixes, int fcap) {
            check_rc(qi_gpu_syndrome_locate(pl, h.ctx.p, static_cast<int>(R), t, st.din, 0,
                                            static_cast<long long>(st.P), st.dcnt[0], st.dent[0],
                                            static_cast<int>(st.pm[0].cap), dres, dres + N,
                                            dres + N + 2, dres + N + 1, fixes, fcap,
                                            static_cast<long long>(words), 1, s),
                     "syndrome locate");
        },
        listed_ids, result, "syndrome locate");
}

long long RsFnt::apply_deltas(const std::vector<int>& fragment_ids, std::vector<uint8_t*>& bufs,
                              std::vector<Properties>& props,
                              const std::vector<LocateFix>& deltas, size_t block_size_bytes,
                              size_t max_marks) const
{
    if (bufs.size() < fragment_ids.size() || props.size() < fragment_ids.size())
        throw std::invalid_argument("RsFnt::apply_deltas: buffers");
    const size_t words = block_size_bytes / word_size;
    for (auto const& d : deltas)
        if (d.column >= words || d.symbol < 1 || d.symbol > 65536)
            throw std::invalid_argument("RsFnt::apply_deltas: bad fix");
    for (size_t hh = 0; hh < fragment_ids.size(); hh++)
        if (!bufs[hh])
            throw std::invalid_argument("RsFnt::apply_deltas: buffers");
    return stage::apply_deltas(frag_map(*this), fragment_ids, bufs, props, deltas, max_marks);
}

int RsFnt::scrub_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                 std::vector<uint8_t*>& parities_bufs,
                                 std::vector<Properties>& parities_props,
                                 std::vector<int>& missing_idxs, LocateResult& result,
                                 int max_errors, bool correct, size_t block_size_bytes,
                                 size_t max_marks)
{
    if (max_errors < 0 || max_errors > QI_SYNDROME_MAX_ERRORS)
        throw std::invalid_argument("RsFnt::scrub_blocks_vertical: max_errors");
    const stage::FragMap map = frag_map(*this);
    const std::vector<int> present = map.present(missing_idxs);
    stage::reset_locate(result, code_len, max_errors);
    const std::vector<int> ids = map.select_upto(present, n_data + QI_SYNDROME_MAX_CHECKS);
    if (ids.size() < n_data + std::max(1, 2 * max_errors))
        return 0;
    const size_t N = ids.size(), R = N - n_data;
    if (!syndrome_supported(N, R, block_size_bytes))
        throw std::invalid_argument("RsFnt::scrub_blocks_vertical: unsupported shape");
    // the share of a holder of every listed fragment, then the decision
    std::vector<uint8_t*> rows(N);
    std::vector<Properties> props(N);
    for (size_t i = 0; i < N; i++) {
        const auto fs = map.slot(static_cast<unsigned>(ids[i]));
        rows[i] = fs.is_data ? data_bufs[fs.slot] : parities_bufs[fs.slot];
        if (!fs.is_data)
            props[i] = parities_props[fs.slot];
    }
    std::vector<std::vector<uint8_t>> syn(R, std::vector<uint8_t>(block_size_bytes));
    std::vector<uint8_t*> syn_bufs(R);
    for (size_t j = 0; j < R; j++)
        syn_bufs[j] = syn[j].data();
    std::vector<Properties> syn_props;
    syndrome_blocks_vertical(ids, ids, rows, props, static_cast<int>(R), false, syn_bufs,
                             syn_props, block_size_bytes);
    locate_syndromes(ids, syn_bufs, syn_props, max_errors, result, block_size_bytes);
    if (!correct || result.fixes.empty() || result.unlocated != 0)
        return 1;
    if (apply_deltas(ids, rows, props, result.fixes, block_size_bytes, max_marks) < 0)
        throw std::length_error("RsFnt::scrub_blocks_vertical: patch refused");
    for (size_t i = 0; i < N; i++) {
        const auto fs = map.slot(static_cast<unsigned>(ids[i]));
        if (!fs.is_data)
            parities_props[fs.slot] = props[i];
    }
    return 2;
}

namespace {

// One stage of the pipelined stream API: pinned host staging, device
// buffers and a HIP stream.  Chunk i runs in slot i % 2, so reading chunk i
// from the input streams and writing chunk i-2 to the output streams overlap
// the transfers and kernels of chunk i-1.
struct StreamSlot {
    hipStream_t st = nullptr;
    uint8_t* host = nullptr;
    size_t host_bytes = 0;
    DevBuf in, out, small, ctx;
    size_t got = 0, offset = 0;
    bool busy = false;
    StreamSlot()
    {
        check(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate");
    }
    ~StreamSlot()
    {
        (void)hipStreamSynchronize(st);
        if (host)
            (void)hipHostFree(host);
        in.release();
        out.release();
        small.release();
        ctx.release();
        (void)hipStreamDestroy(st);
    }
    StreamSlot(const StreamSlot&) = delete;
    StreamSlot& operator=(const StreamSlot&) = delete;
    uint8_t* pinned(size_t n)
    {
        if (n > host_bytes) {
            if (host)
                (void)hipHostFree(host);
            host = nullptr;
            host_bytes = 0;
            check(hipHostMalloc(reinterpret_cast<void**>(&host), n,
                                hipHostMallocDefault),
                  "hipHostMalloc");
            host_bytes = n;
        }
        return host;
    }
};

// fn(i) for i < n on up to 16 threads: the fragments are independent
// streams (shard files, sockets), so they are read and written in parallel
template <typename F>
void parallel_for(size_t n, F fn)
{
    const size_t hw = std::max(1u, std::thread::hardware_concurrency());
    const size_t nt = std::min<size_t>({n, hw, 16});
    if (nt <= 1) {
        for (size_t i = 0; i < n; i++)
            fn(i);
        return;
    }
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nt; t++)
        pool.emplace_back([&, t] {
            for (size_t i = t; i < n; i += nt)
                fn(i);
        });
    for (auto& th : pool)
        th.join();
}

// read `k` streams into rows `pitch` bytes apart: bytes read by every
// stream (short = end of stream), the tail of each row zeroed
size_t read_rows(const std::vector<std::istream*>& src, uint8_t* rows,
                 size_t pitch, bool& cont)
{
    std::vector<size_t> r(src.size());
    parallel_for(src.size(),
                 [&](size_t i) { r[i] = read_full(src[i], rows + i * pitch, pitch); });
    size_t got = pitch;
    for (size_t i = 0; i < src.size(); i++) {
        if (r[i] < pitch) {
            got = std::min(got, r[i]);
            cont = false;
        }
    }
    for (size_t i = 0; i < src.size(); i++)
        std::memset(rows + i * pitch + got, 0, pitch - got);
    return got;
}

// write `got` bytes of each of the n rows at hout to its stream (null: not
// wanted)
template <typename S>
void write_rows(const std::vector<S*>& dst, size_t n, const uint8_t* hout, size_t pitch,
                size_t got)
{
    parallel_for(n, [&](size_t i) {
        if (dst[i])
            dst[i]->write(reinterpret_cast<const char*>(hout + i * pitch),
                          static_cast<std::streamsize>(got));
    });
}

// the reader and writer of a block in caller memory, chunk by chunk: n rows
// of `total` bytes in, n rows out at the chunk's byte offset (null: not
// wanted)
auto mem_reader(const uint8_t* const* rows, size_t n, size_t total)
{
    return [=, pos = size_t{0}](uint8_t* h, size_t pitch, bool& cont) mutable {
        const size_t got = std::min(pitch, total - pos);
        parallel_for(n, [&](size_t i) {
            std::memcpy(h + i * pitch, rows[i] + pos, got);
            std::memset(h + i * pitch + got, 0, pitch - got);
        });
        pos += got;
        cont = pos < total;
        return got;
    };
}

auto mem_writer(uint8_t* const* outs, size_t n)
{
    return [=](const uint8_t* hout, size_t pitch, size_t got, size_t off) {
        parallel_for(n, [&](size_t i) {
            if (outs[i])
                std::memcpy(outs[i] + off, hout + i * pitch, got);
        });
    };
}

// The two-slot loop under both pipes: chunks of whole packets (CH bytes per
// row) alternate between two slots (pinned staging, device buffers, a HIP
// stream each): while one chunk is in H2D -> kernels -> D2H, the host fills
// the other slot with the next chunk and finishes the previous one.
//   pinned_bytes(offset)                  the chunk's pinned staging size
//   submit(slot, host, got, words, offset)  enqueue the filled chunk on slot.st
//   finish(slot)                          the chunk has left the device
// offset counts words; `ops` counts the chunks; chunks finish in order.
template <typename Reader, typename Bytes, typename Submit, typename Finish>
void two_slot_pipe(StreamSlot* slot, size_t CH, const Reader& read, uint64_t& ops,
                   Bytes pinned_bytes, Submit submit, Finish finish)
{
    auto done = [&](StreamSlot& sl) {
        check(hipStreamSynchronize(sl.st), "sync");
        sl.busy = false;
        finish(sl);
    };
    size_t offset = 0;
    unsigned it = 0;
    bool cont = true;
    while (cont) {
        StreamSlot& sl = slot[it & 1];
        if (sl.busy)
            done(sl);
        uint8_t* h = sl.pinned(pinned_bytes(offset));
        const size_t got = read(h, CH, cont);
        if (got == 0)
            break;
        submit(sl, h, got, (got + 1) / 2, offset);
        sl.got = got;
        sl.offset = offset;
        sl.busy = true;
        offset += got / 2;
        ops++;
        it++;
    }
    // drain in chunk order: the older pending chunk sits in slot it % 2
    if (slot[it & 1].busy)
        done(slot[it & 1]);
    if (slot[(it + 1) & 1].busy)
        done(slot[(it + 1) & 1]);
}

}  // namespace

struct RsFnt::StreamPipe {
    StreamSlot slot[2];
};

void RsFnt::encode_streams_vertical(
    const std::vector<std::istream*>& input_data_bufs,
    std::vector<std::ostream*>& output_parities_bufs,
    std::vector<Properties>& output_parities_props)
{
    // src/fec_base.h:463-542: packets of buf_size bytes, zero padded tail,
    // `read_bytes` of every output written for the last packet.  Here whole
    // chunks of packets go through the two-slot pinned pipeline.
    reset_stats_enc();
    Timer tm;
    encode_pipe(
        [&](uint8_t* h, size_t pitch, bool& cont) {
            return read_rows(input_data_bufs, h, pitch, cont);
        },
        [&](const uint8_t* hout, size_t pitch, size_t got, size_t) {
            write_rows(output_parities_bufs, n_outputs, hout, pitch, got);
        },
        output_parities_props);
    total_enc_usec += tm.usec();
}

void RsFnt::encode_pipe(const RowReader& read, const RowWriter& write,
                        std::vector<Properties>& output_parities_props)
{
    for (auto& p : output_parities_props)
        p.clear();
    const size_t CH = chunk_bytes(buf_size);  // a multiple of 128 bytes
    const size_t P = CH / 2, k = n_data, no = n_outputs;
    const uint32_t cap = static_cast<uint32_t>(64 + P / 512);
    // pinned: k input rows, no output rows, then (as on the device) OOR
    // counts, OOR entries
    const size_t in_b = k * CH, out_b = no * CH;
    const auto small = stage::layout({no * 4, no * cap * 4});
    if (!pipe_)
        pipe_.reset(new StreamPipe);
    two_slot_pipe(
        pipe_->slot, CH, read, n_encode_ops,
        [&](size_t) { return in_b + out_b + small[2]; },
        [&](StreamSlot& sl, uint8_t* h, size_t, size_t words, size_t) {
            reserve(sl.in, in_b);
            reserve(sl.out, out_b);
            reserve(sl.small, small[2]);
            uint8_t* ds = static_cast<uint8_t*>(sl.small.p);
            uint32_t* dcnt = reinterpret_cast<uint32_t*>(ds + small[0]);
            uint32_t* dent = reinterpret_cast<uint32_t*>(ds + small[1]);
            h2d(sl.in.p, h, k * CH, sl.st);
            check_rc(qi_gpu_oor_clear(dcnt, no, sl.st), "oor_clear");
            check_rc(qi_gpu_encode(plan_, static_cast<uint16_t*>(sl.in.p), 0,
                                   static_cast<long long>(P), static_cast<uint16_t*>(sl.out.p),
                                   0, static_cast<long long>(P), static_cast<long long>(words),
                                   1, dcnt, dent, static_cast<int>(cap), sl.st),
                     "qi_gpu_encode");
            d2h(h + in_b, sl.out.p, out_b, sl.st);
            d2h(h + in_b + out_b, sl.small.p, small[2], sl.st);
        },
        [&](StreamSlot& sl) {
            uint8_t* hout = sl.host + in_b;
            const uint32_t* cnt = reinterpret_cast<const uint32_t*>(hout + out_b + small[0]);
            uint32_t* ent = reinterpret_cast<uint32_t*>(hout + out_b + small[1]);
            if (*std::max_element(cnt, cnt + no) > cap) {
                // adversarial data: redo this chunk synchronously, exact capacity
                std::vector<const uint8_t*> dp(k);
                std::vector<uint8_t*> op(no);
                for (size_t i = 0; i < k; i++)
                    dp[i] = sl.host + i * CH;
                for (size_t i = 0; i < no; i++)
                    op[i] = hout + i * CH;
                encode_columns(plan_, dp.data(), op.data(), (sl.got + 1) / 2,
                               output_parities_props, sl.offset);
            } else {
                for (size_t i = 0; i < no; i++)
                    stage::add_sorted(output_parities_props[i], ent + i * cap, cnt[i],
                                      sl.offset);
            }
            write(hout, CH, sl.got, 2 * sl.offset);
        });
}

bool RsFnt::decode_streams_vertical(
    const std::vector<std::istream*>& input_data_bufs,
    const std::vector<std::istream*>& input_parities_bufs,
    std::vector<Properties>& input_parities_props,
    std::vector<std::ostream*>& output_data_bufs)
{
    // src/fec_base.h:898-1048, through the two-slot pipeline: the k received
    // rows of a chunk are staged back to back (packed decode)
    const stage::FragMap map = frag_map(*this);
    const std::vector<int> present =
        map.present([&](unsigned i) { return input_data_bufs[i] != nullptr; },
                    [&](unsigned i) { return input_parities_bufs[i] != nullptr; });
    if (map.data_in_clear(present))
        return true;
    std::vector<int> ids;
    if (!map.select(present, ids))
        return false;
    for (auto& p : input_parities_props)
        p.sort();
    reset_stats_dec();
    const size_t k = n_data;
    std::vector<std::istream*> src(k);
    std::vector<const Properties*> props(k, nullptr);
    selected_rows(map, ids, input_data_bufs, input_parities_bufs, input_parities_props, src,
                  props);
    Timer tm;
    decode_pipe(
        ids, props,
        [&](uint8_t* h, size_t pitch, bool& cont) { return read_rows(src, h, pitch, cont); },
        [&](const uint8_t* hout, size_t pitch, size_t got, size_t) {
            write_rows(output_data_bufs, k, hout, pitch, got);
        });
    total_dec_usec += tm.usec();
    return true;
}

void RsFnt::decode_pipe(const std::vector<int>& ids, const std::vector<const Properties*>& props,
                        const RowReader& read, const RowWriter& write)
{
    const size_t k = n_data;
    const size_t CH = chunk_bytes(buf_size);
    const size_t P = CH / 2;
    const size_t io_b = k * CH;
    // OOR marks of each received row (ascending), consumed chunk by chunk;
    // pinned behind the rows, as on the device: ids, counts, entries
    std::vector<size_t> cursor(k, 0);
    stage::PackedMarks pm;
    std::array<size_t, 4> small{};
    if (!pipe_)
        pipe_.reset(new StreamPipe);
    two_slot_pipe(
        pipe_->slot, CH, read, n_decode_ops,
        [&](size_t offset) {
            // the chunk's marks per received row (positions relative to it)
            pm = stage::pack_marks(props, offset, P, &cursor);
            small = stage::layout({k * 2, k * 4, stage::round64(k * pm.cap * 4)});
            return 2 * io_b + small[3];
        },
        [&](StreamSlot& sl, uint8_t* h, size_t, size_t words, size_t) {
            const size_t cap = pm.cap;
            uint8_t* hs = h + 2 * io_b;
            uint16_t* hids = reinterpret_cast<uint16_t*>(hs + small[0]);
            std::copy(ids.begin(), ids.end(), hids);
            std::copy(pm.counts.begin(), pm.counts.end(),
                      reinterpret_cast<uint32_t*>(hs + small[1]));
            std::copy(pm.entries.begin(), pm.entries.end(),
                      reinterpret_cast<uint32_t*>(hs + small[2]));
            // the context's size follows this chunk's width (a 256 < k <= 384
            // context is larger at whole-tile widths than at ragged ones)
            reserve(sl.in, io_b);
            reserve(sl.out, io_b);
            reserve(sl.small, small[3]);
            reserve(sl.ctx, qi_gpu_decode_ctx_bytes(plan_, 1, static_cast<long long>(words)));
            uint8_t* ds = static_cast<uint8_t*>(sl.small.p);
            const uint16_t* dids = reinterpret_cast<const uint16_t*>(ds + small[0]);
            const uint32_t* dcnt = reinterpret_cast<const uint32_t*>(ds + small[1]);
            const uint32_t* dent = reinterpret_cast<const uint32_t*>(ds + small[2]);
            h2d(sl.in.p, h, io_b, sl.st);
            h2d(sl.small.p, hs, small[3], sl.st);
            check_rc(qi_gpu_decode_ctx_packed(plan_, dids, hids, 1, dcnt, dent,
                                              static_cast<int>(cap),
                                              static_cast<long long>(words), sl.ctx.p, sl.st),
                     "decode context");
            check_rc(qi_gpu_decode_packed(plan_, sl.ctx.p, static_cast<uint16_t*>(sl.in.p), 0,
                                          static_cast<long long>(P), dcnt, dent,
                                          static_cast<int>(cap),
                                          static_cast<uint16_t*>(sl.out.p), 0,
                                          static_cast<long long>(P),
                                          static_cast<long long>(words), 1, sl.st),
                     "decode");
            d2h(h + io_b, sl.out.p, io_b, sl.st);
        },
        [&](StreamSlot& sl) {
            if (qi_gpu_take_error(plan_))
                throw std::runtime_error("RsFnt: OOR marks lost (bucket capacity)");
            write(sl.host + io_b, CH, sl.got, 2 * sl.offset);
        });
}

// Blocks wider than one pipeline chunk (quadiron_fnt32_encode / _decode on
// multi-MiB fragments) go through the same two-slot pinned pipeline as the
// streams: the caller's rows are copied chunk by chunk into pinned staging
// (parallel over the fragments) while the previous chunk is on the device,
// so H2D, kernels, D2H and the host copies overlap.  Returns false for
// blocks of one chunk or less (one synchronous device call).
bool RsFnt::encode_blocks_pipe(const std::vector<uint8_t*>& data_bufs,
                               const std::vector<uint8_t*>& outs,
                               std::vector<Properties>& props, size_t words)
{
    if (words <= chunk_bytes(buf_size) / 2)
        return false;
    // one operation per block call, as the reference counts it
    // (src/fec_base.h:1136); the pipe counts its chunks
    const uint64_t ops = n_encode_ops;
    encode_pipe(mem_reader(data_bufs.data(), n_data, 2 * words),
                mem_writer(outs.data(), n_outputs), props);
    n_encode_ops = ops + 1;
    return true;
}

bool RsFnt::decode_blocks_pipe(const std::vector<int>& ids,
                               const std::vector<const uint8_t*>& rows,
                               const std::vector<const Properties*>& props,
                               const std::vector<uint8_t*>& outs, size_t words)
{
    if (words <= chunk_bytes(buf_size) / 2)
        return false;
    const uint64_t ops = n_decode_ops;  // one per block call (src/fec_base.h:1304)
    decode_pipe(ids, props, mem_reader(rows.data(), n_data, 2 * words),
                mem_writer(outs.data(), n_data));
    n_decode_ops = ops + 1;
    return true;
}

// ---------------------------------------------------- horizontal API

namespace {

std::vector<unsigned> id_order(const vec::Vector& ids, unsigned k)
{
    std::vector<unsigned> ord(k);
    for (unsigned i = 0; i < k; i++)
        ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](unsigned a, unsigned b) { return ids[a] < ids[b]; });
    for (unsigned i = 1; i < k; i++)
        if (ids[ord[i]] == ids[ord[i - 1]])
            throw std::invalid_argument("RsFnt::decode: repeated fragment id");
    return ord;
}

bool marked_at(const Properties& p, size_t loc)
{
    for (auto const& it : p.get_map())
        if (it.first == loc && it.second == OOR_MARK)
            return true;
    return false;
}

}  // namespace

void RsFnt::encode(vec::Vector& output, std::vector<Properties>& props, off_t offset,
                   const vec::Vector& words)
{
    // src/fec_rs_fnt.h:178-201: fft->fft(output, words) -- the n-point NTT of
    // the zero-padded data whatever the type -- then encode_post_process: an
    // output i < n_outputs equal to 65536 is marked at `offset` and set to 0
    if (words.size() < n_data || output.size() < n || props.size() < n_outputs)
        throw std::invalid_argument("RsFnt::encode: vector sizes");
    std::vector<uint16_t> in(n_data), out(n);
    for (unsigned i = 0; i < n_data; i++) {
        if (words[i] > 65535u)
            throw std::invalid_argument("RsFnt::encode: data symbol >= 65536");
        in[i] = static_cast<uint16_t>(words[i]);
    }
    std::vector<const uint8_t*> dp(n_data);
    std::vector<uint8_t*> op(n);
    for (unsigned i = 0; i < n_data; i++)
        dp[i] = reinterpret_cast<const uint8_t*>(&in[i]);
    for (unsigned i = 0; i < n; i++)
        op[i] = reinterpret_cast<uint8_t*>(&out[i]);
    std::vector<Properties> marks(n);
    encode_columns(hplan(), dp.data(), op.data(), 1, marks, 0);
    for (unsigned i = 0; i < n; i++)
        output[i] = marks[i].get_map().empty() ? out[i] : 65536u;
    for (unsigned i = 0; i < n_outputs; i++) {
        if (output[i] == 65536u) {
            props[i].add(static_cast<size_t>(offset), OOR_MARK);
            output[i] = 0;
        }
    }
    n_encode_ops++;
}

void RsFnt::encode(vec::Buffers& output, std::vector<Properties>& props, off_t offset,
                   const vec::Buffers& words)
{
    // src/fec_rs_fnt.h:231-270: systematic -> the m parities (interpolation
    // + NTT), otherwise the n outputs of the NTT; encode_post_process marks
    // every 65536 of the first n_outputs rows at offset + j (the value stays)
    const bool sys = type == FecType::SYSTEMATIC;
    qi_plan* pl = sys ? plan_ : hplan();
    const unsigned rows = sys ? n_parities : n;
    const size_t size = words.get_size();
    if (words.get_n() < static_cast<int>(n_data) || output.get_n() < static_cast<int>(rows) ||
        output.get_size() < size || props.size() < n_outputs)
        throw std::invalid_argument("RsFnt::encode: buffer sizes");
    std::vector<std::vector<uint16_t>> in(n_data, std::vector<uint16_t>(size));
    std::vector<std::vector<uint16_t>> out(rows, std::vector<uint16_t>(size));
    for (unsigned i = 0; i < n_data; i++)
        for (size_t j = 0; j < size; j++) {
            const uint32_t v = words.get(static_cast<int>(i))[j];
            if (v > 65535u)
                throw std::invalid_argument("RsFnt::encode: data symbol >= 65536");
            in[i][j] = static_cast<uint16_t>(v);
        }
    std::vector<const uint8_t*> dp(n_data);
    std::vector<uint8_t*> op(rows);
    for (unsigned i = 0; i < n_data; i++)
        dp[i] = reinterpret_cast<const uint8_t*>(in[i].data());
    for (unsigned i = 0; i < rows; i++)
        op[i] = reinterpret_cast<uint8_t*>(out[i].data());
    std::vector<Properties> marks(rows);
    encode_columns(pl, dp.data(), op.data(), size, marks, 0);
    for (unsigned i = 0; i < rows; i++) {
        uint32_t* o = output.get(static_cast<int>(i));
        for (size_t j = 0; j < size; j++)
            o[j] = out[i][j];
        for (auto const& it : marks[i].get_map()) {
            o[it.first] = 65536u;
            if (i < n_outputs)
                props[i].add(static_cast<size_t>(offset) + it.first, OOR_MARK);
        }
    }
    n_encode_ops++;
}

std::unique_ptr<DecodeContext> RsFnt::init_context_dec(const vec::Vector& fragments_ids,
                                                       std::vector<Properties>& input_props,
                                                       size_t size)
{
    // src/fec_base.h:758-793 (the props are read by each decode call)
    (void)input_props;
    if (fragments_ids.size() < n_data)
        throw std::invalid_argument("RsFnt::init_context_dec: need n_data ids");
    vec::Vector ids(fragments_ids.begin(), fragments_ids.begin() + n_data);
    for (uint32_t id : ids)
        if (id >= n)
            throw std::invalid_argument("RsFnt::init_context_dec: fragment id >= n");
    return std::make_unique<DecodeContext>(ids, size);
}

void RsFnt::decode(DecodeContext& context, vec::Vector& output,
                   const std::vector<Properties>& props, off_t offset, vec::Vector& words)
{
    // decode_prepare (src/fec_base.h:799-820): a mark at `offset` on fragment
    // ids[i] restores words[i] = 65536; decode_apply (:829-878) interpolates
    // the n-point code: output = the k coefficients
    const vec::Vector& ids = context.get_fragments_id();
    if (words.size() < n_data || output.size() < n_data)
        throw std::invalid_argument("RsFnt::decode: vector sizes");
    std::vector<int> id(n_data);
    std::vector<uint16_t> in(n_data), out(n_data);
    std::vector<Properties> marks(n_data);
    std::vector<const uint8_t*> rows(n_data);
    std::vector<const Properties*> mp(n_data);
    std::vector<uint8_t*> op(n_data);
    // the device takes the received fragments in ascending id order (the
    // interpolation does not depend on the order)
    const std::vector<unsigned> ord = id_order(ids, n_data);
    for (unsigned i = 0; i < n_data; i++) {
        const unsigned r = ord[i];
        if (ids[r] < props.size() && marked_at(props[ids[r]], static_cast<size_t>(offset)))
            words[r] = 65536u;
    }
    for (unsigned i = 0; i < n_data; i++) {
        const unsigned r = ord[i];
        id[i] = static_cast<int>(ids[r]);
        in[i] = static_cast<uint16_t>(words[r] & 0xffffu);
        if (words[r] == 65536u)
            marks[i].add(0, OOR_MARK);
        rows[i] = reinterpret_cast<const uint8_t*>(&in[i]);
        mp[i] = &marks[i];
        op[i] = reinterpret_cast<uint8_t*>(&out[i]);
    }
    decode_columns(hplan(), id, rows, mp, op.data(), 1, 0);
    for (unsigned i = 0; i < n_data; i++)
        output[i] = out[i];
    n_decode_ops++;
}

void RsFnt::decode(DecodeContext& context, vec::Buffers& output,
                   const std::vector<Properties>& props, off_t offset, vec::Buffers& words)
{
    // decode_prepare (src/fec_base.h:1361-1404): the marks of the received
    // coded fragments (props by parity index) inside [offset, offset + size)
    // restore 65536; decode_apply (:1418-1448) + for systematic codes the
    // evaluation at r^t (:1336-1355): output = the k data rows
    const stage::FragMap map = frag_map(*this);
    const vec::Vector& ids = context.get_fragments_id();
    const size_t size = words.get_size();
    if (words.get_n() < static_cast<int>(n_data) || output.get_n() < static_cast<int>(n_data) ||
        output.get_size() < size)
        throw std::invalid_argument("RsFnt::decode: buffer sizes");
    std::vector<int> id(n_data);
    std::vector<std::vector<uint16_t>> in(n_data, std::vector<uint16_t>(size)),
        out(n_data, std::vector<uint16_t>(size));
    std::vector<Properties> marks(n_data);
    std::vector<const uint8_t*> rows(n_data);
    std::vector<const Properties*> mp(n_data);
    std::vector<uint8_t*> op(n_data);
    const std::vector<unsigned> ord = id_order(ids, n_data);
    for (unsigned i = 0; i < n_data; i++) {
        const unsigned r = ord[i];
        id[i] = static_cast<int>(ids[r]);
        uint32_t* w = words.get(static_cast<int>(r));
        const auto fs = map.slot(ids[r]);
        if (!fs.is_data && fs.slot < props.size())
            // decode_prepare restores the marks in [offset, offset +
            // pkt_size) (src/fec_base.h:1372), which equals the Buffers'
            // size on the reference's own paths; here the window is the
            // Buffers' size: a Buffers wider than pkt_size keeps every
            // mark (the reference would drop those past pkt_size) and a
            // narrower one is never written past its end (deliberate
            // deviation)
            for (auto const& it : props[fs.slot].get_map())
                if (it.second == OOR_MARK && it.first >= static_cast<size_t>(offset) &&
                    it.first < static_cast<size_t>(offset) + size)
                    w[it.first - static_cast<size_t>(offset)] = 65536u;
        for (size_t j = 0; j < size; j++) {
            in[i][j] = static_cast<uint16_t>(w[j] & 0xffffu);
            if (w[j] == 65536u)
                marks[i].add(j, OOR_MARK);
        }
        rows[i] = reinterpret_cast<const uint8_t*>(in[i].data());
        mp[i] = &marks[i];
        op[i] = reinterpret_cast<uint8_t*>(out[i].data());
    }
    decode_columns(plan_, id, rows, mp, op.data(), size, 0);
    for (unsigned i = 0; i < n_data; i++) {
        uint32_t* o = output.get(static_cast<int>(i));
        for (size_t j = 0; j < size; j++)
            o[j] = out[i][j];
    }
    n_decode_ops++;
}

// ----------------------------------------------------------------- RS-NF4

void nf4_marks_from_lanes(const Properties& lanes, unsigned g, Properties& words)
{
    stage::marks_from_lanes(lanes, g, words);
}

void nf4_marks_to_lanes(const Properties& words, unsigned g, Properties& lanes)
{
    stage::marks_to_lanes(words, g, lanes);
}

namespace {

unsigned nf4_word_size(unsigned ws)
{
    if (ws != 2 && ws != 4 && ws != 8)
        throw std::invalid_argument("RsNf4: word_size must be 2, 4 or 8");
    return ws;
}

}  // namespace

RsNf4::RsNf4(unsigned ws, unsigned k, unsigned m, size_t pkt)
    : word_size(nf4_word_size(ws)), n_data(k), n_parities(m), code_len(k + m),
      n_outputs(k + m), gf_n(ws / 2), pkt_size(pkt), buf_size(pkt * ws), n(0),
      lanes_(FecType::NON_SYSTEMATIC, 2, k, m, pkt * (ws / 2))
{
    n = lanes_.n;
}

void RsNf4::encode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                   std::vector<uint8_t*>& parities_bufs,
                                   std::vector<Properties>& parities_props,
                                   std::vector<bool>& wanted_idxs,
                                   size_t block_size_bytes)
{
    std::vector<Properties> lp(n_outputs);
    lanes_.encode_blocks_vertical(data_bufs, parities_bufs, lp, wanted_idxs,
                                  block_size_bytes / word_size * word_size);
    for (unsigned i = 0; i < n_outputs; i++)
        nf4_marks_from_lanes(lp[i], gf_n, parities_props[i]);
}

bool RsNf4::decode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                   std::vector<uint8_t*>& parities_bufs,
                                   std::vector<Properties>& parities_props,
                                   std::vector<int>& missing_idxs,
                                   std::vector<bool>& wanted_idxs,
                                   size_t block_size_bytes)
{
    std::vector<Properties> lp(n_outputs);
    for (unsigned i = 0; i < n_outputs; i++) {
        parities_props[i].sort();  // as DecodeContext (src/fec_context.h:93-97)
        nf4_marks_to_lanes(parities_props[i], gf_n, lp[i]);
    }
    return lanes_.decode_blocks_vertical(data_bufs, parities_bufs, lp,
                                         missing_idxs, wanted_idxs,
                                         block_size_bytes / word_size * word_size);
}

void RsNf4::encode_streams_vertical(
    const std::vector<std::istream*>& input_data_bufs,
    std::vector<std::ostream*>& output_parities_bufs,
    std::vector<Properties>& output_parities_props)
{
    std::vector<Properties> lp(n_outputs);
    lanes_.encode_streams_vertical(input_data_bufs, output_parities_bufs, lp);
    for (unsigned i = 0; i < n_outputs; i++)
        nf4_marks_from_lanes(lp[i], gf_n, output_parities_props[i]);
}

bool RsNf4::decode_streams_vertical(
    const std::vector<std::istream*>& input_data_bufs,
    const std::vector<std::istream*>& input_parities_bufs,
    std::vector<Properties>& input_parities_props,
    std::vector<std::ostream*>& output_data_bufs)
{
    std::vector<Properties> lp(n_outputs);
    for (unsigned i = 0; i < n_outputs; i++) {
        input_parities_props[i].sort();
        nf4_marks_to_lanes(input_parities_props[i], gf_n, lp[i]);
    }
    return lanes_.decode_streams_vertical(input_data_bufs, input_parities_bufs,
                                          lp, output_data_bufs);
}

}  // namespace fec
}  // namespace qi

// ---------------------------------------------------------------- C view

struct qi_fec {
    qi::fec::RsFnt* f;
};

struct qi_nf4 {
    qi::fec::RsNf4* f;
};

namespace {

namespace stage = qi::fec::stage;

// the block calls of both classes on flat (oor, flags, oor_count, cap)
// arrays; flags null: RS-FNT's plain marks
template <typename F>
int encode_blocks_flat(F& f, uint8_t** data, uint8_t** outputs, size_t block_bytes,
                       uint32_t* oor, uint32_t* flags, uint32_t* oor_count, uint32_t cap)
{
    std::vector<uint8_t*> dv(data, data + f.n_data);
    std::vector<uint8_t*> pv(outputs, outputs + f.n_outputs);
    std::vector<qi::Properties> props(f.n_outputs);
    std::vector<bool> wanted(f.n_outputs);
    for (unsigned i = 0; i < f.n_outputs; i++)
        wanted[i] = outputs[i] != nullptr;
    f.encode_blocks_vertical(dv, pv, props, wanted, block_bytes);
    stage::props_to_flat(props, oor, flags, oor_count, cap);
    return 0;
}

template <typename F>
int decode_blocks_flat(F& f, uint8_t** data, uint8_t** parities, const uint32_t* oor,
                       const uint32_t* flags, const uint32_t* oor_count, uint32_t cap,
                       const int* missing, const int* wanted, size_t block_bytes)
{
    std::vector<uint8_t*> dv(data, data + f.n_data);
    std::vector<uint8_t*> pv(parities, parities + f.n_outputs);
    std::vector<qi::Properties> props(f.n_outputs);
    stage::props_from_flat(props, oor, flags, oor_count, cap);
    std::vector<int> miss(missing, missing + f.code_len);
    std::vector<bool> want(f.n_data);
    for (unsigned i = 0; i < f.n_data; i++)
        want[i] = wanted[i] != 0;
    return f.decode_blocks_vertical(dv, pv, props, miss, want, block_bytes) ? 1 : 0;
}

// data rows (null: none, as for a non-systematic code) and coded rows with
// their marks, as repair and verify take them
struct FlatFragments {
    std::vector<uint8_t*> dv, pv;
    std::vector<qi::Properties> props;
    std::vector<int> miss;
    FlatFragments(const qi::fec::RsFnt& f, uint8_t** data, uint8_t** parities,
                  const uint32_t* oor, const uint32_t* oor_count, uint32_t cap,
                  const int* missing)
        : dv(f.n_data, nullptr), pv(parities, parities + f.n_outputs), props(f.n_outputs),
          miss(missing, missing + f.code_len)
    {
        if (data)
            dv.assign(data, data + f.n_data);
        stage::props_from_flat(props, oor, nullptr, oor_count, cap);
    }
};

// the two shares on flat arrays: n_listed listed ids, n_held held rows with
// their marks (oor_count null: none), n_out output rows whose marks are read
// first when acc; share(listed, held, rows, marks, out rows, out marks)
template <typename Share>
int share_blocks_flat(const int* listed, size_t n_listed, const int* held_ids, int n_held,
                      uint8_t** rows, const uint32_t* oor, const uint32_t* oor_count, uint32_t cap,
                      int n_out, int acc, uint8_t** out, uint32_t* out_oor, uint32_t* out_count,
                      uint32_t out_cap, Share share)
{
    std::vector<int> iv(listed, listed + n_listed), hv(held_ids, held_ids + n_held);
    std::vector<uint8_t*> rv(rows, rows + n_held), ov(out, out + n_out);
    std::vector<qi::Properties> hp(static_cast<size_t>(n_held)), op(static_cast<size_t>(n_out));
    stage::props_from_flat(hp, oor, nullptr, oor_count, cap);
    if (acc)
        stage::props_from_flat(op, out_oor, nullptr, out_count, out_cap);
    share(iv, hv, rv, hp, ov, op);
    stage::props_to_flat(op, out_oor, nullptr, out_count, out_cap);
    return 1;
}

}  // namespace

extern "C" {

qi_fec* qi_fec_new(int systematic, int k, int m)
{
    try {
        auto* h = new qi_fec;
        h->f = new qi::fec::RsFnt(systematic ? qi::fec::FecType::SYSTEMATIC
                                             : qi::fec::FecType::NON_SYSTEMATIC,
                                  2, static_cast<unsigned>(k),
                                  static_cast<unsigned>(m), 1024);
        return h;
    } catch (...) {
        return nullptr;
    }
}

void qi_fec_delete(qi_fec* h)
{
    if (h) {
        delete h->f;
        delete h;
    }
}

int qi_fec_n_outputs(const qi_fec* h)
{
    return h ? static_cast<int>(h->f->n_outputs) : -1;
}

int qi_fec_encode_blocks(qi_fec* h, uint8_t** data, uint8_t** outputs,
                         size_t block_bytes, uint32_t* oor, uint32_t* oor_count,
                         uint32_t cap)
{
    try {
        return encode_blocks_flat(*h->f, data, outputs, block_bytes, oor, nullptr, oor_count,
                                  cap);
    } catch (...) {
        return -1;
    }
}

int qi_fec_decode_blocks(qi_fec* h, uint8_t** data, uint8_t** parities,
                         const uint32_t* oor, const uint32_t* oor_count,
                         uint32_t cap, const int* missing, const int* wanted,
                         size_t block_bytes)
{
    try {
        return decode_blocks_flat(*h->f, data, parities, oor, nullptr, oor_count, cap, missing,
                                  wanted, block_bytes);
    } catch (...) {
        return -1;
    }
}

int qi_fec_repair_blocks(qi_fec* h, uint8_t** data, uint8_t** parities, const uint32_t* oor,
                         const uint32_t* oor_count, uint32_t cap, const int* missing,
                         const int* targets, int n_targets, uint8_t** out, uint32_t* out_oor,
                         uint32_t* out_count, uint32_t out_cap, size_t block_bytes)
{
    try {
        if (!h || n_targets < 0)
            return -1;
        qi::fec::RsFnt& f = *h->f;
        if (!f.repair_supported(static_cast<size_t>(n_targets), block_bytes))
            return -2;
        FlatFragments fr(f, data, parities, oor, oor_count, cap, missing);
        std::vector<int> tg(targets, targets + n_targets);
        std::vector<uint8_t*> ov(out, out + n_targets);
        std::vector<qi::Properties> oprops;
        if (!f.repair_blocks_vertical(fr.dv, fr.pv, fr.props, fr.miss, tg, ov, oprops,
                                      block_bytes))
            return 0;
        stage::props_to_flat(oprops, out_oor, nullptr, out_count, out_cap);
        return 1;
    } catch (...) {
        return -1;
    }
}

int qi_fec_verify_blocks(qi_fec* h, uint8_t** data, uint8_t** parities, const uint32_t* oor,
                         const uint32_t* oor_count, uint32_t cap, const int* missing,
                         long long* result, size_t block_bytes)
{
    try {
        if (!h || !parities || !missing || !result)
            return -1;
        qi::fec::RsFnt& f = *h->f;
        if (!f.repair_supported(1, block_bytes))
            return -2;
        // (oor_count null: no marks)
        FlatFragments fr(f, data, parities, oor, oor_count, cap, missing);
        std::vector<qi::fec::VerifyResult> res;
        const bool ok = f.verify_blocks_vertical(fr.dv, fr.pv, fr.props, fr.miss, res,
                                                 block_bytes);
        for (unsigned i = 0; i < f.code_len; i++) {
            result[3 * i] = res[i].value_mismatch;
            result[3 * i + 1] = res[i].mark_mismatch;
            result[3 * i + 2] = res[i].first;
        }
        return ok ? 1 : 0;
    } catch (...) {
        return -1;
    }
}

int qi_fec_locate_blocks(qi_fec* h, uint8_t** data, uint8_t** parities, uint32_t* oor,
                         uint32_t* oor_count, uint32_t cap, const int* missing,
                         long long* result, int correct, size_t block_bytes)
{
    try {
        if (!h || !parities || !missing || !result)
            return -1;
        qi::fec::RsFnt& f = *h->f;
        if (!f.locate_supported(block_bytes))
            return -2;
        // (oor_count null: no marks, and none can be written)
        FlatFragments fr(f, data, parities, oor, oor_count, cap, missing);
        qi::fec::LocateResult res;
        const int rc = f.locate_blocks_vertical(fr.dv, fr.pv, fr.props, fr.miss, res,
                                                correct != 0, block_bytes,
                                                oor_count ? cap : 0);
        stage::locate_to_flat(res, result);
        if (rc == 2 && oor_count)
            stage::props_to_flat(fr.props, oor, nullptr, oor_count, cap);
        return rc;
    } catch (...) {
        return -1;
    }
}

int qi_fec_locate_multi_blocks(qi_fec* h, uint8_t** data, uint8_t** parities, uint32_t* oor,
                               uint32_t* oor_count, uint32_t cap, const int* missing,
                               int max_errors, long long* result, int correct,
                               size_t block_bytes)
{
    try {
        if (!h || !parities || !missing || !result || max_errors < 1 ||
            max_errors > QI_LOCATE_MAX_ERRORS)
            return -1;
        qi::fec::RsFnt& f = *h->f;
        if (!f.locate_supported(block_bytes))
            return -2;
        // (oor_count null: no marks, and none can be written)
        FlatFragments fr(f, data, parities, oor, oor_count, cap, missing);
        qi::fec::LocateResult res;
        const int rc = f.locate_multi_blocks_vertical(fr.dv, fr.pv, fr.props, fr.miss, res,
                                                      max_errors, correct != 0, block_bytes,
                                                      oor_count ? cap : 0);
        stage::locate_to_flat(res, result);
        if (rc == 2 && oor_count)
            stage::props_to_flat(fr.props, oor, nullptr, oor_count, cap);
        return rc;
    } catch (...) {
        return -1;
    }
}

int qi_fec_fingerprint_blocks(qi_fec* h, uint8_t** data, uint8_t** parities, const uint32_t* oor,
                              const uint32_t* oor_count, uint32_t cap, const int* missing,
                              const uint32_t* keys, int n_keys, long long* result,
                              size_t block_bytes)
{
    try {
        if (!keys || n_keys < 1 || n_keys > QI_FINGERPRINT_MAX_KEYS)
            return -1;
        for (int e = 0; e < 3 * n_keys; e++)
            if (keys[e] < 1 || keys[e] > 65536)
                return -1;
        if (!h || !parities || !missing || !result)
            return -1;
        qi::fec::RsFnt& f = *h->f;
        // (oor_count null: no marks)
        FlatFragments fr(f, data, parities, oor, oor_count, cap, missing);
        std::vector<long long> res;
        f.fingerprint_blocks_vertical(fr.dv, fr.pv, fr.props, fr.miss, keys, n_keys, res,
                                      block_bytes);
        std::copy(res.begin(), res.end(), result);
        return 1;
    } catch (...) {
        return -1;
    }
}

int qi_fec_update_blocks(qi_fec* h, const int* ids, int n_rows, uint8_t** old_rows,
                         uint8_t** new_rows, uint8_t** parities, uint32_t* oor,
                         uint32_t* oor_count, uint32_t cap, size_t block_bytes)
{
    try {
        if (!h || !ids || !old_rows || !new_rows || !parities || n_rows < 0)
            return -1;
        qi::fec::RsFnt& f = *h->f;
        size_t held = 0;
        for (unsigned j = 0; j < f.n_outputs; j++)
            held += parities[j] != nullptr;
        if (held == 0)
            return -1;
        if (!f.update_supported(static_cast<size_t>(n_rows), held, block_bytes))
            return -2;
        std::vector<int> iv(ids, ids + n_rows);
        std::vector<uint8_t*> ov(old_rows, old_rows + n_rows), nv(new_rows, new_rows + n_rows);
        std::vector<uint8_t*> pv(parities, parities + f.n_outputs);
        // the held fragments' marks only (oor_count null: none)
        std::vector<qi::Properties> props(f.n_outputs);
        for (unsigned j = 0; j < f.n_outputs; j++)
            for (uint32_t e = 0; pv[j] && oor_count && e < std::min(oor_count[j], cap); e++)
                props[j].add(oor[static_cast<size_t>(j) * cap + e], qi::OOR_MARK);
        f.update_blocks_vertical(iv, ov, nv, pv, props, block_bytes);
        for (unsigned j = 0; j < f.n_outputs; j++) {
            if (!pv[j] || !oor_count)
                continue;
            uint32_t c = 0;
            for (auto const& it : props[j].get_map()) {
                if (c < cap)
                    oor[static_cast<size_t>(j) * cap + c] = static_cast<uint32_t>(it.first);
                c++;
            }
            oor_count[j] = c;
        }
        return 1;
    } catch (...) {
        return -1;
    }
}

int qi_fec_partial_repair_blocks(qi_fec* h, const int* ids, const int* held_ids, int n_held,
                                 uint8_t** rows, const uint32_t* oor, const uint32_t* oor_count,
                                 uint32_t cap, const int* targets, int n_targets, int acc,
                                 uint8_t** out, uint32_t* out_oor, uint32_t* out_count,
                                 uint32_t out_cap, size_t block_bytes)
{
    try {
        if (!h || !ids || !held_ids || !rows || !targets || !out || !out_count || n_held < 0 ||
            n_targets < 0 || (out_cap > 0 && !out_oor))
            return -1;
        qi::fec::RsFnt& f = *h->f;
        if (!f.partial_supported(static_cast<size_t>(n_held), static_cast<size_t>(n_targets),
                                 block_bytes))
            return -2;
        const std::vector<int> tv(targets, targets + n_targets);
        return share_blocks_flat(
            ids, f.n_data, held_ids, n_held, rows, oor, oor_count, cap, n_targets, acc, out,
            out_oor, out_count, out_cap,
            [&](auto& iv, auto& hv, auto& rv, auto& hp, auto& ov, auto& op) {
                f.partial_repair_blocks_vertical(iv, hv, rv, hp, tv, acc != 0, ov, op,
                                                 block_bytes);
            });
    } catch (...) {
        return -1;
    }
}

int qi_fec_syndrome_blocks(qi_fec* h, const int* listed_ids, int n_listed, const int* held_ids,
                           int n_held, uint8_t** rows, const uint32_t* oor,
                           const uint32_t* oor_count, uint32_t cap, int n_checks, int acc,
                           uint8_t** out, uint32_t* out_oor, uint32_t* out_count,
                           uint32_t out_cap, size_t block_bytes)
{
    try {
        if (!h || !listed_ids || !held_ids || !rows || !out || !out_count || n_held < 0 ||
            n_checks < 0 || n_listed < 0 || (out_cap > 0 && !out_oor))
            return -1;
        qi::fec::RsFnt& f = *h->f;
        if (!f.syndrome_supported(static_cast<size_t>(n_held), static_cast<size_t>(n_checks),
                                  block_bytes) ||
            static_cast<size_t>(n_listed) != f.n_data + static_cast<size_t>(n_checks))
            return -2;
        return share_blocks_flat(
            listed_ids, n_listed, held_ids, n_held, rows, oor, oor_count, cap, n_checks, acc, out,
            out_oor, out_count, out_cap,
            [&](auto& iv, auto& hv, auto& rv, auto& hp, auto& ov, auto& op) {
                f.syndrome_blocks_vertical(iv, hv, rv, hp, n_checks, acc != 0, ov, op,
                                           block_bytes);
            });
    } catch (...) {
        return -1;
    }
}

int qi_fec_locate_syndromes(qi_fec* h, const int* listed_ids, int n_listed, uint8_t** rows,
                            const uint32_t* oor, const uint32_t* oor_count, uint32_t cap,
                            int max_errors, long long* result, uint32_t* fixes, uint32_t fix_cap,
                            uint32_t* n_fixes, size_t block_bytes)
{
    try {
        if (!h || !listed_ids || !rows || !result || !n_fixes || n_listed < 0 ||
            (fix_cap > 0 && !fixes))
            return -1;
        qi::fec::RsFnt& f = *h->f;
        const size_t R = static_cast<size_t>(n_listed) > f.n_data ? n_listed - f.n_data : 0;
        if (!f.syndrome_supported(1, R, block_bytes) || max_errors < 0 ||
            2 * static_cast<size_t>(max_errors) > R)
            return -2;
        std::vector<int> iv(listed_ids, listed_ids + n_listed);
        std::vector<uint8_t*> rv(rows, rows + R);
        std::vector<qi::Properties> sp(R);
        qi::fec::stage::props_from_flat(sp, oor, nullptr, oor_count, cap);
        qi::fec::LocateResult res;
        f.locate_syndromes(iv, rv, sp, max_errors, res, block_bytes);
        stage::locate_to_flat(res, result);
        *n_fixes = static_cast<uint32_t>(res.fixes.size());
        for (size_t e = 0; e < res.fixes.size() && e < fix_cap; e++) {
            fixes[3 * e] = res.fixes[e].column;
            fixes[3 * e + 1] = static_cast<uint32_t>(res.fixes[e].fragment);
            fixes[3 * e + 2] = res.fixes[e].symbol;
        }
        return 1;
    } catch (...) {
        return -1;
    }
}

int qi_fec_apply_deltas(qi_fec* h, const int* fragment_ids, int n_rows, uint8_t** rows,
                        uint32_t* oor, uint32_t* oor_count, uint32_t cap, const uint32_t* fixes,
                        uint32_t n_fixes, size_t block_bytes)
{
    try {
        if (!h || !fragment_ids || !rows || n_rows < 0 || (n_fixes > 0 && !fixes) ||
            (oor_count && cap > 0 && !oor))
            return -1;
        qi::fec::RsFnt& f = *h->f;
        std::vector<int> iv(fragment_ids, fragment_ids + n_rows);
        std::vector<uint8_t*> rv(rows, rows + n_rows);
        std::vector<qi::Properties> props(static_cast<size_t>(n_rows));
        qi::fec::stage::props_from_flat(props, oor, nullptr, oor_count, cap);
        std::vector<qi::fec::LocateFix> dl;
        for (uint32_t e = 0; e < n_fixes; e++)
            dl.push_back(qi::fec::LocateFix{fixes[3 * e], static_cast<int>(fixes[3 * e + 1]),
                                            fixes[3 * e + 2]});
        const long long n = f.apply_deltas(iv, rv, props, dl, block_bytes, oor_count ? cap : 0);
        if (n < 0)
            return -3;
        if (oor_count)
            qi::fec::stage::props_to_flat(props, oor, nullptr, oor_count, cap);
        return static_cast<int>(n);
    } catch (...) {
        return -1;
    }
}

int qi_fec_scrub_blocks(qi_fec* h, uint8_t** data, uint8_t** parities, uint32_t* oor,
                        uint32_t* oor_count, uint32_t cap, const int* missing, int max_errors,
                        long long* result, int correct, size_t block_bytes)
{
    try {
        if (!h || !parities || !missing || !result || max_errors < 0 ||
            max_errors > QI_SYNDROME_MAX_ERRORS)
            return -1;
        qi::fec::RsFnt& f = *h->f;
        if (!f.syndrome_supported(1, 1, block_bytes))
            return -2;
        // (oor_count null: no marks, and none can be written)
        FlatFragments fr(f, data, parities, oor, oor_count, cap, missing);
        qi::fec::LocateResult res;
        const int rc = f.scrub_blocks_vertical(fr.dv, fr.pv, fr.props, fr.miss, res, max_errors,
                                               correct != 0, block_bytes, oor_count ? cap : 0);
        stage::locate_to_flat(res, result);
        if (rc == 2 && oor_count)
            stage::props_to_flat(fr.props, oor, nullptr, oor_count, cap);
        return rc;
    } catch (const std::invalid_argument&) {
        return -2;
    } catch (...) {
        return -1;
    }
}

}  // extern "C"

namespace {

// std::streambuf over caller memory (no copies of its own) for the C view
// of the stream API
struct MemIn : std::streambuf {
    MemIn(const uint8_t* p, size_t n)
    {
        char* b = reinterpret_cast<char*>(const_cast<uint8_t*>(p));
        setg(b, b, b + n);
    }
};
struct MemOut : std::streambuf {
    MemOut(uint8_t* p, size_t n)
    {
        char* b = reinterpret_cast<char*>(p);
        setp(b, b + n);
    }
};

struct MemStreams {
    std::vector<std::unique_ptr<std::streambuf>> bufs;
    std::vector<std::unique_ptr<std::iostream>> streams;
    std::iostream* in(const uint8_t* p, size_t n)
    {
        if (!p)
            return nullptr;
        bufs.emplace_back(new MemIn(p, n));
        streams.emplace_back(new std::iostream(bufs.back().get()));
        return streams.back().get();
    }
    std::iostream* out(uint8_t* p, size_t n)
    {
        if (!p)
            return nullptr;
        bufs.emplace_back(new MemOut(p, n));
        streams.emplace_back(new std::iostream(bufs.back().get()));
        return streams.back().get();
    }
};

}  // namespace

extern "C" {

int qi_fec_encode_streams(qi_fec* h, const uint8_t** data, size_t bytes,
                          uint8_t** outputs, uint32_t* oor, uint32_t* oor_count,
                          uint32_t cap)
{
    try {
        qi::fec::RsFnt& f = *h->f;
        MemStreams ms;
        std::vector<std::istream*> in(f.n_data);
        std::vector<std::ostream*> out(f.n_outputs);
        for (unsigned i = 0; i < f.n_data; i++)
            if (!(in[i] = ms.in(data[i], bytes)))
                return -1;
        for (unsigned i = 0; i < f.n_outputs; i++)
            if (!(out[i] = ms.out(outputs[i], bytes)))
                return -1;
        std::vector<qi::Properties> props(f.n_outputs);
        f.encode_streams_vertical(in, out, props);
        stage::props_to_flat(props, oor, nullptr, oor_count, cap);
        return 0;
    } catch (...) {
        return -1;
    }
}

int qi_fec_decode_streams(qi_fec* h, const uint8_t** data,
                          const uint8_t** parities, size_t bytes,
                          const uint32_t* oor, const uint32_t* oor_count,
                          uint32_t cap, uint8_t** out_data)
{
    try {
        qi::fec::RsFnt& f = *h->f;
        MemStreams ms;
        std::vector<std::istream*> din(f.n_data), pin(f.n_outputs);
        std::vector<std::ostream*> dout(f.n_data);
        for (unsigned i = 0; i < f.n_data; i++) {
            din[i] = ms.in(data ? data[i] : nullptr, bytes);
            dout[i] = ms.out(out_data[i], bytes);
        }
        for (unsigned i = 0; i < f.n_outputs; i++)
            pin[i] = ms.in(parities[i], bytes);
        std::vector<qi::Properties> props(f.n_outputs);
        stage::props_from_flat(props, oor, nullptr, oor_count, cap);
        return f.decode_streams_vertical(din, pin, props, dout) ? 1 : 0;
    } catch (...) {
        return -1;
    }
}

qi_nf4* qi_nf4_new(int word_size, int k, int m)
{
    try {
        if (word_size < 0 || k < 1 || m < 1)
            return nullptr;
        auto* h = new qi_nf4;
        try {
            h->f = new qi::fec::RsNf4(static_cast<unsigned>(word_size),
                                      static_cast<unsigned>(k),
                                      static_cast<unsigned>(m), 1024);
        } catch (...) {
            delete h;
            return nullptr;
        }
        return h;
    } catch (...) {
        return nullptr;
    }
}

void qi_nf4_delete(qi_nf4* h)
{
    if (h) {
        delete h->f;
        delete h;
    }
}

int qi_nf4_n_outputs(const qi_nf4* h)
{
    return h ? static_cast<int>(h->f->n_outputs) : -1;
}

int qi_nf4_encode_blocks(qi_nf4* h, uint8_t** data, uint8_t** outputs,
                         size_t block_bytes, uint32_t* oor, uint32_t* flags,
                         uint32_t* oor_count, uint32_t cap)
{
    try {
        return encode_blocks_flat(*h->f, data, outputs, block_bytes, oor, flags, oor_count, cap);
    } catch (...) {
        return -1;
    }
}

int qi_nf4_decode_blocks(qi_nf4* h, uint8_t** data, uint8_t** parities,
                         const uint32_t* oor, const uint32_t* flags,
                         const uint32_t* oor_count, uint32_t cap,
                         const int* missing, const int* wanted,
                         size_t block_bytes)
{
    try {
        return decode_blocks_flat(*h->f, data, parities, oor, flags, oor_count, cap, missing,
                                  wanted, block_bytes);
    } catch (...) {
        return -1;
    }
}

}  // extern "C"
