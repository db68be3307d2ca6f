// qi_fec.hpp -- C++ FecCode-style API of the MI355X RS-FNT engine.
//
// Mirrors the part of QuadIron's C++ surface that the C-ABI, the benchmark and
// ec_driver use (src/fec_base.h:93-294, src/fec_rs_fnt.h:51-270,
// src/property.h:61-198): RsFnt<uint32_t>(type, word_size, k, m, pkt_size)
// with the vertical block and stream APIs and the OOR Properties side channel.
// Every transform runs on the GPU through include/qi_gpu.h; there is no CPU
// compute path.  word_size 2 (GF(65537)) only.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <istream>
#include <memory>
#include <ostream>
#include <utility>
#include <vector>

#include <sys/types.h>

struct qi_plan;

namespace qi {

static constexpr unsigned OOR_MARK = 1;  // src/property.h:49

// Sparse (location, marker) list of out-of-range symbols of one fragment.
class Properties {
  public:
    enum { FNT1 = 0x464E5431 };
    void add(size_t location, uint32_t marker)
    {
        props.emplace_back(location, marker);
    }
    void clear() { props.clear(); }
    void sort();
    const std::vector<std::pair<size_t, uint32_t>>& get_map() const
    {
        return props;
    }
    // FNT1 header (src/property.h:104-142): 0 on success, -1 on error
    int fnt_serialize(uint32_t* dwords, unsigned n_dwords) const;
    int fnt_deserialize(const uint32_t* dwords, unsigned n_dwords);

    friend std::istream& operator>>(std::istream& is, Properties& p);
    friend std::ostream& operator<<(std::ostream& os, const Properties& p);

  private:
    std::vector<std::pair<size_t, uint32_t>> props;
};

namespace vec {

// Containers of the horizontal API (QuadIron's vec::Vector<T> /
// vec::Buffers<T>, src/vec_vector.h, src/vec_buffers.h, with T = uint32_t):
// GF(65537) symbols 0 .. 65536 held in 32 bits.
using Vector = std::vector<uint32_t>;

class Buffers {
  public:
    Buffers(int n, size_t size)
        : n_(n), size_(size), mem_(static_cast<size_t>(n) * size, 0u)
    {
    }
    int get_n() const { return n_; }
    size_t get_size() const { return size_; }
    uint32_t* get(int i) { return mem_.data() + static_cast<size_t>(i) * size_; }
    const uint32_t* get(int i) const { return mem_.data() + static_cast<size_t>(i) * size_; }

  private:
    int n_;
    size_t size_;
    std::vector<uint32_t> mem_;
};

}  // namespace vec

namespace fec {

enum class FecType { SYSTEMATIC, NON_SYSTEMATIC };

// What FecCode::init_context_dec returns (src/fec_base.h:758-793,
// src/fec_context.h:66-274): the fragment ids a decode uses.  The
// per-pattern constants themselves are built on the device by every decode
// call, together with that call's OOR marks (decode_prepare).
class DecodeContext {
  public:
    explicit DecodeContext(const vec::Vector& ids, size_t size) : ids_(ids), size_(size) {}
    const vec::Vector& get_fragments_id() const { return ids_; }
    size_t get_size() const { return size_; }

  private:
    vec::Vector ids_;
    size_t size_;
};

// What RsFnt::verify_blocks_vertical reports per fragment: the columns whose
// stored word / OOR mark differ from the recomputed symbol and the smallest
// such column (0xFFFFFFFF: none); all -1 for a fragment that was not checked
struct VerifyResult {
    long long value_mismatch, mark_mismatch, first;
};

// What RsFnt::locate_blocks_vertical reports: per fragment id the number of
// columns in which that fragment alone was wrong (-1 for a fragment that is
// missing or was not listed), the number of bad columns that could not be
// attributed, and per located column the fragment and the symbol (0 .. 65536)
// it should hold there
struct LocateFix {
    uint32_t column;
    int fragment;
    uint32_t symbol;
};
struct LocateResult {
    std::vector<long long> located;
    long long unlocated = 0;
    std::vector<LocateFix> fixes;
    // locate_multi_blocks_vertical only: weights[nu - 1] is the number of
    // columns located with nu fragments, nu = 1 .. max_errors
    std::vector<long long> weights;
};

class RsFnt {
  public:
    // throws std::invalid_argument (bad parameters / word_size != 2) or
    // std::runtime_error (no HIP device)
    RsFnt(FecType type, unsigned word_size, unsigned n_data,
          unsigned n_parities, size_t pkt_size = 8);
    ~RsFnt();
    RsFnt(const RsFnt&) = delete;
    RsFnt& operator=(const RsFnt&) = delete;

    FecType type;
    unsigned word_size, n_data, n_parities, code_len, n_outputs;
    size_t pkt_size, buf_size;
    unsigned n;

    uint64_t n_encode_ops = 0, n_decode_ops = 0;
    uint64_t total_enc_usec = 0, total_dec_usec = 0;

    int get_n_outputs() const;  // n (non-systematic) or m (systematic)

    void encode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                std::vector<uint8_t*>& parities_bufs,
                                std::vector<Properties>& parities_props,
                                std::vector<bool>& wanted_idxs,
                                size_t block_size_bytes);

    bool decode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                std::vector<uint8_t*>& parities_bufs,
                                std::vector<Properties>& parities_props,
                                std::vector<int>& missing_idxs,
                                std::vector<bool>& wanted_idxs,
                                size_t block_size_bytes);

    // Fused repair: rebuild the fragments `targets` (ids in the decode's id
    // space: systematic f < n_data is data row f, otherwise parity
    // f - n_data; non-systematic: coded row f) straight from the first
    // n_data present fragments, chosen as decode_blocks_vertical chooses
    // them, in one pass on the device (qi_gpu_repair).  out_bufs[j]
    // receives target j (block_size_bytes each) and out_props[j] its marks
    // (ascending, counts exact; none for a data row).  Every target must be
    // flagged missing.  Returns false when fewer than n_data fragments are
    // present.  Throws std::invalid_argument where repair_supported() is
    // false, or a target is present or out of range.
    bool repair_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                std::vector<uint8_t*>& parities_bufs,
                                std::vector<Properties>& parities_props,
                                std::vector<int>& missing_idxs,
                                const std::vector<int>& targets,
                                std::vector<uint8_t*>& out_bufs,
                                std::vector<Properties>& out_props,
                                size_t block_size_bytes);
    // n_data <= 256, 1 <= n_targets <= min(64, n_parities), and a block that
    // fits the single-chunk device staging with every fragment row of the
    // code in its own slot (at most 256 MiB of rows)
    bool repair_supported(size_t n_targets, size_t block_size_bytes) const;

    // Delta update (qi_gpu_update): data rows ids[u] (below n_data, distinct)
    // go from old_bufs[u] to new_bufs[u]; the coded fragments held here
    // (parities_bufs[j] != nullptr, n_outputs entries) follow in place, and
    // their parities_props[j] are replaced by the marks of the updated rows
    // (ascending).  Only those 2 ids.size() + held rows are staged: the other
    // data rows of the stripe are not needed.  A bucket overflow on the
    // device is retried once with the exact capacity, as by the other block
    // calls.  Throws std::invalid_argument where update_supported() is false,
    // or an id is out of range or repeated, or no fragment is held.
    void update_blocks_vertical(const std::vector<int>& ids, std::vector<uint8_t*>& old_bufs,
                                std::vector<uint8_t*>& new_bufs,
                                std::vector<uint8_t*>& parities_bufs,
                                std::vector<Properties>& parities_props,
                                size_t block_size_bytes);
    // 1 <= n_rows <= min(8, n_data), 1 <= n_held <= n_outputs, and a block
    // whose 2 n_rows + n_held rows fit the single-chunk device staging (at
    // most 256 MiB of rows)
    bool update_supported(size_t n_rows, size_t n_held, size_t block_size_bytes) const;

    // Partial repair (qi_gpu_partial): the share of a repair of `targets`
    // from the n_data helper fragments `ids` (decode's id space, distinct)
    // that the holder of the fragments `held_ids` (each one of `ids`,
    // distinct) can form.  held_bufs[h] is fragment held_ids[h] and
    // held_props[h] its marks (a systematic data row has none).  With acc:
    // out_bufs[j] / out_props[j] hold the partial rows and marks so far and
    // are updated in place on the device (chain and tree aggregation); else
    // the sum starts from 0.  out_props[j] become the marks of the new
    // partial rows (ascending, counts exact) -- a partial row of a data-row
    // target may carry marks too; only the complete sum is free of them.
    // Summed over any partition of `ids`, in any order, the rows and marks
    // are those of repair_blocks_vertical, at any n_data.  Only the held and
    // the partial rows are staged.  A bucket overflow on the device is
    // retried once with the exact capacity, from the acc rows as they were.
    // Throws std::invalid_argument where partial_supported() is false, or an
    // id, a held id or a target is out of range, repeated or misplaced.
    void partial_repair_blocks_vertical(const std::vector<int>& ids,
                                        const std::vector<int>& held_ids,
                                        std::vector<uint8_t*>& held_bufs,
                                        std::vector<Properties>& held_props,
                                        const std::vector<int>& targets, bool acc,
                                        std::vector<uint8_t*>& out_bufs,
                                        std::vector<Properties>& out_props,
                                        size_t block_size_bytes);
    // 1 <= n_held <= n_data, 1 <= n_targets <= min(8, n_parities), and a
    // block whose n_held + n_targets rows fit the single-chunk device staging
    // (at most 256 MiB of rows)
    bool partial_supported(size_t n_held, size_t n_targets, size_t block_size_bytes) const;

    // Syndrome share (qi_gpu_syndrome): the share of the n_checks syndrome
    // rows of the n_data + n_checks listed fragments `listed_ids` (decode's
    // id space, distinct) that the holder of the fragments `held_ids` (each
    // one of `listed_ids`, distinct) can form.  held_bufs, held_props, acc,
    // out_bufs and out_props as in partial_repair_blocks_vertical, with
    // n_checks rows out.  Summed over any partition of `listed_ids`, in any
    // order, the rows and marks are the syndromes of the stripe: all 0,
    // without marks, when every listed fragment is intact.  Any n_data.
    // Throws std::invalid_argument where syndrome_supported() is false, or an
    // id or a held id is out of range, repeated or not listed.
    void syndrome_blocks_vertical(const std::vector<int>& listed_ids,
                                  const std::vector<int>& held_ids,
                                  std::vector<uint8_t*>& held_bufs,
                                  std::vector<Properties>& held_props, int n_checks, bool acc,
                                  std::vector<uint8_t*>& out_bufs,
                                  std::vector<Properties>& out_props, size_t block_size_bytes);
    // 1 <= n_checks <= min(8, n_parities), 1 <= n_held <= n_data + n_checks,
    // and a block whose n_held + n_checks rows fit the single-chunk device
    // staging (at most 256 MiB of rows)
    bool syndrome_supported(size_t n_held, size_t n_checks, size_t block_size_bytes) const;

    // The coordinator's decision (qi_gpu_syndrome_locate) over the complete
    // sums syn_bufs[j] / syn_props[j], j < n_checks = listed_ids.size() -
    // n_data: locate_multi_blocks_vertical's result at any n_data, from the
    // syndrome rows alone.  0 <= max_errors <= n_checks / 2; 0 only detects
    // (every bad column is unlocated).  result.located is by fragment id (-1:
    // not listed); result.fixes[e].symbol is the *error* of that fragment in
    // that column, in 1 .. 65536: the true symbol is (y - error) mod 65537
    // (apply_deltas).  A fix list longer than the first attempt's capacity is
    // run again with the exact one.  Throws std::invalid_argument for counts
    // out of range or ids out of range or repeated.
    void locate_syndromes(const std::vector<int>& listed_ids, std::vector<uint8_t*>& syn_bufs,
                          std::vector<Properties>& syn_props, int max_errors,
                          LocateResult& result, size_t block_size_bytes);

    // The holder's step, without the device: applies the deltas of
    // locate_syndromes that name one of `fragment_ids` to bufs[h] / props[h]
    // (a systematic data row has no marks) and skips the others.  Returns the
    // number applied, or -1 with nothing touched when a data row would have
    // to hold 65536 or a mark list would grow beyond max_marks.
    long long apply_deltas(const std::vector<int>& fragment_ids, std::vector<uint8_t*>& bufs,
                           std::vector<Properties>& props, const std::vector<LocateFix>& deltas,
                           size_t block_size_bytes,
                           size_t max_marks = static_cast<size_t>(-1)) const;

    // Scrub at any n_data: locate_multi_blocks_vertical's listing, result,
    // `correct`, max_marks and return values, composed of the three calls
    // above with every listed fragment held here.  0 <= max_errors <= 4 (0:
    // detection only, with at least n_data + 1 fragments listed).  Returns 0
    // when fewer than n_data + max(1, 2 max_errors) fragments are listed.
    // Throws std::length_error (nothing patched) when apply_deltas refuses.
    int scrub_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                              std::vector<uint8_t*>& parities_bufs,
                              std::vector<Properties>& parities_props,
                              std::vector<int>& missing_idxs, LocateResult& result,
                              int max_errors, bool correct, size_t block_size_bytes,
                              size_t max_marks = static_cast<size_t>(-1));

    // Fused verify (scrubbing): check the present fragments against each
    // other on the device without rebuilding a row (qi_gpu_verify).  The
    // basis is the first n_data present fragments, chosen as
    // decode_blocks_vertical chooses them; every other present fragment is
    // recomputed from the basis and compared with its buffer and its marks
    // (more than 64 of them: in groups of at most 64 over the same staged
    // rows).  result gets one entry per fragment id (code_len): {-1, -1, -1}
    // for a missing or a basis fragment, otherwise the number of columns
    // whose stored word differs, the number whose OOR mark differs, and the
    // smallest such column (0xFFFFFFFF: none).  A corrupt basis fragment
    // shows in every checked fragment at its column.  Returns false with
    // fewer than n_data + 1 fragments present.  Throws std::invalid_argument
    // where repair_supported(1, block_size_bytes) is false.
    bool verify_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                std::vector<uint8_t*>& parities_bufs,
                                std::vector<Properties>& parities_props,
                                std::vector<int>& missing_idxs,
                                std::vector<VerifyResult>& result, size_t block_size_bytes);

    // Fragment locate (scrubbing, after a verify flagged the stripe): which
    // fragment is wrong in which column, and what it should hold there
    // (qi_gpu_locate).  The first min(present, n_data + 8) present fragments
    // are listed, chosen as decode_blocks_vertical chooses them; R = listed -
    // n_data syndromes tell a single bad fragment of a column and its
    // correction.  With R >= 3 a column with 2 .. R - 1 bad fragments is
    // counted as unlocated, never attributed; with R = 2 (exactly n_data + 2
    // present) two bad fragments of a column may be attributed to a third.
    // Returns 0 with fewer than n_data + 2 fragments present (nothing to
    // locate with), 1 when the result was filled, and with `correct`, when
    // there are fixes and no column is unlocated, 2 after the fixes were
    // written into the caller's buffers and parities_props (a mark inserted
    // where the symbol becomes 65536, removed where it stops being one; lists
    // ascending).  A fix list longer than the first attempt's capacity is run
    // again with the exact one.  Throws std::invalid_argument where
    // locate_supported() is false, std::length_error (nothing patched) when a
    // patched mark list would grow beyond max_marks.
    int locate_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                               std::vector<uint8_t*>& parities_bufs,
                               std::vector<Properties>& parities_props,
                               std::vector<int>& missing_idxs, LocateResult& result,
                               bool correct, size_t block_size_bytes,
                               size_t max_marks = static_cast<size_t>(-1));
    // n_data <= 256, at least 2 parities, and a block within the single-chunk
    // staging of repair_supported
    bool locate_supported(size_t block_size_bytes) const;

    // The same with up to max_errors bad fragments per column
    // (qi_gpu_locate_multi): a column is located when 1 .. max_errors listed
    // fragments explain all R syndromes, and then counts in each of them; its
    // fixes are adjacent in result.fixes, result.weights[nu - 1] counts the
    // columns located with nu fragments.  A column with more than max_errors
    // and at most R - max_errors bad fragments is always unlocated.  Listing,
    // return values, `correct`, max_marks and the exceptions are
    // locate_blocks_vertical's; 0 is also returned when R < 2 max_errors.
    // Throws std::invalid_argument for max_errors outside 1 .. 4.
    int locate_multi_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                     std::vector<uint8_t*>& parities_bufs,
                                     std::vector<Properties>& parities_props,
                                     std::vector<int>& missing_idxs, LocateResult& result,
                                     int max_errors, bool correct, size_t block_size_bytes,
                                     size_t max_marks = static_cast<size_t>(-1));

    // Fragment fingerprints (qi_gpu_fingerprint, include/qi_gpu.h): keys holds
    // n_keys triples (a, b, d), each component in 1 .. 65536, 1 <= n_keys <=
    // 8.  result gets code_len * n_keys values: per fragment id its n_keys
    // fingerprints in [0, 65536], or -1 for a missing fragment.  Every present
    // fragment is covered, at any n_data; a block wider than the device
    // staging goes through in column chunks (first_col) whose results are
    // added modulo 65537 here.  QI_FINGERPRINT_CHUNK_WORDS in the environment,
    // read at call time, caps the chunk width (a test switch).  Throws
    // std::invalid_argument for keys out of range.
    void fingerprint_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                     std::vector<uint8_t*>& parities_bufs,
                                     std::vector<Properties>& parities_props,
                                     std::vector<int>& missing_idxs, const uint32_t* keys,
                                     int n_keys, std::vector<long long>& result,
                                     size_t block_size_bytes);

    void encode_streams_vertical(
        const std::vector<std::istream*>& input_data_bufs,
        std::vector<std::ostream*>& output_parities_bufs,
        std::vector<Properties>& output_parities_props);

    bool decode_streams_vertical(
        const std::vector<std::istream*>& input_data_bufs,
        const std::vector<std::istream*>& input_parities_bufs,
        std::vector<Properties>& input_parities_props,
        std::vector<std::ostream*>& output_data_bufs);

    // Horizontal API (src/fec_base.h:129-178, 409-460, 740-878,
    // src/fec_rs_fnt.h:178-270): one codeword per Vector call, get_size()
    // codewords (columns) per Buffers call, all on the device.  As in the
    // reference, the Vector calls use the non-systematic code of length n
    // for both types (RsFnt::encode(Vector) is fft(output, words) then the
    // post-process over n_outputs; decode(Vector) returns the polynomial's
    // coefficients), and props are indexed by fragment id; the Buffers calls
    // follow the type (systematic: m parities out, the data rows decoded)
    // with props indexed by output / parity.  Data symbols must be < 65536
    // (16-bit input; std::invalid_argument otherwise).
    void encode(vec::Vector& output, std::vector<Properties>& props, off_t offset,
                const vec::Vector& words);
    void encode(vec::Buffers& output, std::vector<Properties>& props, off_t offset,
                const vec::Buffers& words);
    std::unique_ptr<DecodeContext> init_context_dec(const vec::Vector& fragments_ids,
                                                    std::vector<Properties>& input_props,
                                                    size_t size = 0);
    void decode(DecodeContext& context, vec::Vector& output,
                const std::vector<Properties>& props, off_t offset, vec::Vector& words);
    void decode(DecodeContext& context, vec::Buffers& output,
                const std::vector<Properties>& props, off_t offset, vec::Buffers& words);

    void reset_stats_enc()
    {
        n_encode_ops = 0;
        total_enc_usec = 0;
    }
    void reset_stats_dec()
    {
        n_decode_ops = 0;
        total_dec_usec = 0;
    }

    qi_plan* plan() const { return plan_; }

  private:
    // both locates: max_errors 0 is qi_gpu_locate, 1 .. 4 qi_gpu_locate_multi
    int locate_run(std::vector<uint8_t*>& data_bufs, std::vector<uint8_t*>& parities_bufs,
                   std::vector<Properties>& parities_props, std::vector<int>& missing_idxs,
                   LocateResult& result, int max_errors, bool correct, size_t block_size_bytes,
                   size_t max_marks);
    // device encode of `words` columns on plan pl; outputs[i] NULL = not
    // wanted (pl's n_outputs of them)
    void encode_columns(qi_plan* pl, const uint8_t* const* data, uint8_t* const* outputs,
                        size_t words, std::vector<Properties>& props,
                        size_t offset);
    // device decode of `words` columns from the k selected fragments
    void decode_columns(qi_plan* pl, const std::vector<int>& ids,
                        const std::vector<const uint8_t*>& rows,
                        const std::vector<const Properties*>& props,
                        uint8_t* const* outputs, size_t words, size_t offset);
    // the two-slot pinned pipeline behind the stream API and the blocks
    // wider than one chunk: read(h, pitch, cont) fills the next chunk's
    // input rows (pitch bytes apart) and returns the bytes per row (0: no
    // more); write(h, pitch, got, byte_offset) takes a finished chunk's
    // output rows, in chunk order
    using RowReader = std::function<size_t(uint8_t*, size_t, bool&)>;
    using RowWriter = std::function<void(const uint8_t*, size_t, size_t, size_t)>;
    void encode_pipe(const RowReader& read, const RowWriter& write,
                     std::vector<Properties>& props);
    void decode_pipe(const std::vector<int>& ids, const std::vector<const Properties*>& props,
                     const RowReader& read, const RowWriter& write);
    bool encode_blocks_pipe(const std::vector<uint8_t*>& data_bufs,
                            const std::vector<uint8_t*>& outs, std::vector<Properties>& props,
                            size_t words);
    bool decode_blocks_pipe(const std::vector<int>& ids, const std::vector<const uint8_t*>& rows,
                            const std::vector<const Properties*>& props,
                            const std::vector<uint8_t*>& outs, size_t words);

    // the non-systematic plan of length n behind the Vector calls (created
    // on first use)
    qi_plan* hplan();
    qi_plan* plan_ = nullptr;
    qi_plan* hplan_ = nullptr;
    // pinned two-slot pipeline of the stream API, kept across calls
    struct StreamPipe;
    std::unique_ptr<StreamPipe> pipe_;
};

// RS-NF4 (src/fec_rs_nf4.h:46-334, src/gf_nf4.h).  A word of word_size bytes
// packs gf_n = word_size / 2 GF(65537) components that are coded
// independently with RS-FNT's root and transform (NF4::get_nth_root
// replicates the prime-field root, gf_nf4.h:450-455; Radix2 as RsFnt,
// fec_rs_nf4.h:78-96).  So every 16-bit lane of the byte stream is one
// RS-FNT codeword and the device path is RS-FNT's.  Non-systematic only.
// OOR marks are (word offset, component bitmask) pairs (NF4::unpack,
// gf_nf4.h:391-446; restored by NF4::pack(a, flag), :372-383).  word_size 2,
// 4 or 8: the reference benchmark's T = uint32 / uint64 / __uint128_t
// (benchmark/benchmark.cpp:283-306, 696-718).
class RsNf4 {
  public:
    // throws std::invalid_argument (bad parameters / word_size) or
    // std::runtime_error (no HIP device)
    RsNf4(unsigned word_size, unsigned n_data, unsigned n_parities,
          size_t pkt_size = 8);
    RsNf4(const RsNf4&) = delete;
    RsNf4& operator=(const RsNf4&) = delete;

    unsigned word_size, n_data, n_parities, code_len, n_outputs, gf_n;
    size_t pkt_size, buf_size;
    unsigned n;

    int get_n_outputs() const { return static_cast<int>(n); }  // :115-118

    // only whole words are coded (block_size = bytes / word_size,
    // src/fec_base.h:1083); trailing bytes of a partial word are untouched
    void encode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                std::vector<uint8_t*>& parities_bufs,
                                std::vector<Properties>& parities_props,
                                std::vector<bool>& wanted_idxs,
                                size_t block_size_bytes);
    bool decode_blocks_vertical(std::vector<uint8_t*>& data_bufs,
                                std::vector<uint8_t*>& parities_bufs,
                                std::vector<Properties>& parities_props,
                                std::vector<int>& missing_idxs,
                                std::vector<bool>& wanted_idxs,
                                size_t block_size_bytes);
    void encode_streams_vertical(
        const std::vector<std::istream*>& input_data_bufs,
        std::vector<std::ostream*>& output_parities_bufs,
        std::vector<Properties>& output_parities_props);
    bool decode_streams_vertical(
        const std::vector<std::istream*>& input_data_bufs,
        const std::vector<std::istream*>& input_parities_bufs,
        std::vector<Properties>& input_parities_props,
        std::vector<std::ostream*>& output_data_bufs);

    const RsFnt& lanes() const { return lanes_; }

  private:
    RsFnt lanes_;  // the 16-bit lane code (RsFnt NON_SYSTEMATIC, word_size 2)
};

// (16-bit lane, OOR_MARK) marks <-> (word, component mask) marks of gf_n
// lanes per word; lane marks must be ascending (as the encoders emit them)
void nf4_marks_from_lanes(const Properties& lanes, unsigned gf_n,
                          Properties& words);
void nf4_marks_to_lanes(const Properties& words, unsigned gf_n,
                        Properties& lanes);

}  // namespace fec
}  // namespace qi
