// Device-level C-ABI (include/qi_gpu.h): batch encode / decode on
// device-resident stripes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/qi_gpu.h"
#include "fingerprint_math.h"
#include "gf65537.h"
#include "locate_math.h"
#include "locate_multi_math.h"
#include "partial_math.h"
#include "patch_math.h"
#include "qi_internal.h"
#include "qi_plan.h"
#include "syndrome_math.h"
#include "update_coef.h"

using namespace qi;

namespace {

MatLayout ctx_layout(const qi_plan* p)
{
    return MatLayout{p->k, p->k, matrix_kp(p->k)};
}


hipStream_t st(void* s)
{
    return static_cast<hipStream_t>(s);
}

// The decode-context format for this batch width: matrix contexts for
// every k <= 256, and for 256 < k <= 384 (mbig) when the columns tile into
// whole 1024-column blocks (the operand-stationary kernel has no column tail
// there); otherwise the NTT engine's.  A context is valid only for the
// `words` it was built with.
bool use_matrix(const qi_plan* p, long long words)
{
    return !p->ntt || (p->mbig && words % kRouteTile == 0);
}

// the R x k matrices of a repair
MatLayout repair_layout(const qi_plan* p, int R)
{
    return MatLayout{R, p->k, matrix_kp(p->k)};
}

// the matrix-format part of a context: packed block, ids, route table,
// slow-tile list, lazy-section word
long long mat_ctx_words(const MatLayout& L, long long words)
{
    return MatCtxView(L, nullptr, 0, words).size();
}

// the plan's fragment rows: a systematic code's data fragments (ids below
// k; in the coded region's place when the caller holds none) and its coded
// ones, or the n coded fragments
RowSrc plan_src(const qi_plan* p, const uint16_t* d_data, long long dss, long long drs,
                const uint16_t* d_coded, long long css, long long crs)
{
    if (p->sys)
        return RowSrc{d_data ? d_data : d_coded, dss, drs, p->k, d_coded, css, crs, 0,
                      p->k, p->n_outputs};
    return RowSrc{d_coded, css, crs, 1 << 30, nullptr, 0, 0, 0, p->n_outputs, 0};
}

// apply the matrices of the contexts `v` (decode or repair) to the rows
int apply_ctx(const qi_plan* p, const MatLayout& L, const MatCtxView& v, const RowSrc& src,
              const RowDst& out, long long words, int S, const Oor* in, int slot_base,
              const Oor* out_marks, hipStream_t s, const MatVerify* ver = nullptr)
{
    // output row t = matrix row t (d_rowid: the identity, at least
    // QI_REPAIR_MAX_TARGETS entries)
    return launch_matrix(L, v.ctx, v.stride, v.ids(), v.stride, src, out, words, S, in, slot_base,
                         out_marks, p->d_rowid, v.route(), v.stride, v.slow(), p->d_err, s, ver);
}

// The decode of qi_gpu_decode and qi_gpu_decode_packed, which differ in the
// rows (src, by id or by position) and in the marks' slots (`slots` per
// stripe, slot = position or id - slot_base).
// A context built for a whole-tile width carries only the matrix-core
// form.  Rows the matrix cores cannot address send every column to the dot2
// kernel (k <= 256), whose sections are filled from the tiles by the first
// such decode, or to the NTT engine (256 < k <= 384), whose context is built
// by the first such decode from the ids the matrix context holds; the
// context's lazy word records both, so each is filled once (qi_gpu.h: a
// decode may write its context)
int decode_rows(qi_plan* p, const void* d_ctx, const RowSrc& src, const uint32_t* d_counts,
                const uint32_t* d_entries, int slots, int cap, int slot_base, const RowDst& out,
                long long words, int S, hipStream_t s)
{
    const Oor marks{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries), slots, cap};
    const Oor* in = d_counts ? &marks : nullptr;
    const long long cs = ctx_stride(p, words);
    if (!use_matrix(p, words))
        return ntt_decode(p, static_cast<const int32_t*>(d_ctx), cs, src, in, slot_base, out,
                          words, S, s);
    const MatLayout L = ctx_layout(p);
    const MatCtxView v(L, d_ctx, cs, words);
    // (a context with a column tail was built with every section)
    if (!matrix_cores_take(src, out, L.R, words) && words % kRouteTile == 0) {
        if (!p->mbig) {
            if (int rc = fill_dot2_sections(L, v.ctx, cs, words, S, s))
                return rc;
        } else {
            if (int rc = ntt_build_ctx_lazy(p, v.ids(), S, v.ctx + v.size(), cs, v.lazy(), s))
                return rc;
            return ntt_decode(p, v.ctx + v.size(), cs, src, in, slot_base, out, words, S, s);
        }
    }
    return apply_ctx(p, L, v, src, out, words, S, in, slot_base, nullptr, s);
}

}  // namespace

namespace qi {

long long ctx_stride(const qi_plan* p, long long words)
{
    if (!use_matrix(p, words))
        return ntt_ctx_words(p);
    // 256 < k <= 384: the NTT engine's context follows the matrix one, for
    // rows the matrix cores cannot address (matrix_cores_take)
    return mat_ctx_words(ctx_layout(p), words) + (p->mbig ? ntt_ctx_words(p) : 0);
}

// Decode contexts for n_stripes stripes, built on the device inside the
// caller's stream: the matrix paths (k <= 256; 256 < k <= 384 at whole-tile
// widths), interpolation matrices + OOR route tables (decode_ctx_kernel);
// otherwise the NTT decode's per-pattern constants (ntt_ctx_kernel or
// eras_ctx_kernel; its decode reads the OOR buckets directly).
int build_ctx(qi_plan* p, const uint16_t* d_ids, int n_stripes, const Oor* in,
              int slot_base, int by_pos, long long words, void* d_ctx, hipStream_t s)
{
    if (n_stripes == 0)
        return 0;
    if (!d_ids)
        return -1;
    const long long cs = ctx_stride(p, words);
    if (!use_matrix(p, words))
        return ntt_build_ctx(p, d_ids, n_stripes, static_cast<int32_t*>(d_ctx), cs, s);
    const MatLayout L = ctx_layout(p);
    // (256 < k <= 384: the NTT engine's half only when a decode needs it,
    // decode_rows)
    // the dot2 sections only for widths with a column tail (below 256 < k:
    // no dot2 kernel at all); a whole-tile decode that needs them after all
    // fills them from the tiles (qi_gpu_decode)
    const int dot2 = !p->mbig && words % kRouteTile != 0;
    return launch_decode_ctx(p->k, p->n, p->r, p->sys ? 1 : 0, L, d_ids, n_stripes,
                             static_cast<int32_t*>(d_ctx), cs, in, slot_base, by_pos,
                             words, dot2, p->d_err, s);
}

static bool update_ok(const qi_plan* p, int U, int R)
{
    return U >= 1 && U <= std::min(QI_UPDATE_MAX_ROWS, p->k) && R >= 1 && R <= p->n_outputs;
}

// qi_gpu_update; by_pos: the coded / output row and both buckets of the j-th
// listed slot are found by its position j (rows and slots = R: the compact
// staging of the block API) instead of by the slot
int update_rows(qi_plan* p, const void* d_ctx, int U, int R, int by_pos, const uint16_t* d_old,
                long long old_ss, long long old_rs, const uint16_t* d_new, long long new_ss,
                long long new_rs, const uint16_t* d_coded, long long css, long long crs,
                const uint32_t* d_in_counts, const uint32_t* d_in_entries, int in_cap,
                uint16_t* d_out, long long oss, long long ors, uint32_t* d_out_counts,
                uint32_t* d_out_entries, int out_cap, long long words, int n_stripes,
                hipStream_t s)
{
    if (!d_ctx || !d_old || !d_new || !d_coded || !d_out || n_stripes < 0 || words < 0)
        return -1;
    if (!update_ok(p, U, R))
        return -1;
    if (n_stripes == 0 || words == 0)
        return 0;
    const int slots = by_pos ? R : p->n_outputs;
    const Oor in{const_cast<uint32_t*>(d_in_counts), const_cast<uint32_t*>(d_in_entries), slots,
                 in_cap};
    const Oor outm{d_out_counts, d_out_entries, slots, out_cap};
    return launch_update(static_cast<const int32_t*>(d_ctx), update_ctx_words(U, R), U,
                         update_up(U), R, by_pos, d_old, old_ss, old_rs, d_new, new_ss, new_rs,
                         d_coded, css, crs, in, d_out, oss, ors, outm, words, n_stripes, p->d_err,
                         s);
}

}  // namespace qi

extern "C" {

int qi_gpu_oor_clear(uint32_t* d_counts, size_t n, void* stream)
{
    if (!d_counts || n == 0)
        return 0;
    return hipMemsetAsync(d_counts, 0, n * sizeof(uint32_t), st(stream)) ==
                   hipSuccess
               ? 0
               : -2;
}

int qi_gpu_encode(qi_plan* p, const uint16_t* d_data, long long dss,
                  long long drs, uint16_t* d_out, long long oss, long long ors,
                  long long words, int n_stripes, uint32_t* d_counts,
                  uint32_t* d_entries, int cap, void* stream)
{
    if (!p || !d_data || !d_out || n_stripes < 0 || words < 0)
        return -1;
    if (n_stripes == 0 || words == 0)
        return 0;
    Oor oor{d_counts, d_entries, p->n_outputs, cap};
    RowDst out{d_out, oss, ors};
    RowSrc src{d_data, dss, drs, 1 << 30, nullptr, 0, 0, 0, p->k, 0};
    // k > 256: the NTT engine, unless the matrix cores take the batch (mbig
    // plans with a generator, whole tiles, addressable rows)
    if (p->ntt && !(p->d_gen && use_matrix(p, words) &&
                    matrix_cores_take(src, out, p->gen.R, words)))
        return ntt_encode(p, d_data, dss, drs, out, words, n_stripes,
                          d_counts ? &oor : nullptr, st(stream));
    if (!p->d_gen)
        return launch_encode_fnt(p->k, p->n, p->n_outputs, p->d_twist, d_data,
                                 dss, drs, out, words, n_stripes, oor,
                                 p->d_err, st(stream));
    return launch_matrix(p->gen, p->d_gen, 0, nullptr, 0, src, out, words,
                         n_stripes, nullptr, 0, d_counts ? &oor : nullptr, p->d_rowmap,
                         nullptr, 0, SlowList{nullptr, 0}, p->d_err, st(stream));
}

size_t qi_gpu_decode_ctx_bytes(const qi_plan* p, int n_stripes,
                               long long words)
{
    if (!p || n_stripes < 0 || words < 0)
        return 0;
    // an upper bound for every width up to `words` (the format, and so the
    // stride, of a 256 < k <= 384 context depends on the width: a caller
    // sizing for its widest batch may build narrower ones in the buffer)
    long long w = ctx_stride(p, words);
    if (p->mbig && words >= kRouteTile)
        w = std::max(w, ctx_stride(p, words / kRouteTile * kRouteTile));
    return static_cast<size_t>(w) * sizeof(int32_t) * static_cast<size_t>(n_stripes);
}

int qi_gpu_decode_ctx(qi_plan* p, const uint16_t* d_ids, const uint16_t* h_ids,
                      int n_stripes, const uint32_t* d_counts,
                      const uint32_t* d_entries, int cap, long long words,
                      void* d_ctx, void* stream)
{
    if (!p || !d_ctx || n_stripes < 0 || words < 0)
        return -1;
    Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries),
           p->n_outputs, cap};
    (void)h_ids;  // contexts are built on the device for every k
    return qi::build_ctx(p, d_ids, n_stripes, d_counts ? &in : nullptr,
                         p->sys ? p->k : 0, 0, words, d_ctx, st(stream));
}

int qi_gpu_decode(qi_plan* p, const void* d_ctx, const uint16_t* d_ids,
                  const uint16_t* d_data, long long dss, long long drs,
                  const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_counts, const uint32_t* d_entries, int cap,
                  uint16_t* d_out, long long oss, long long ors,
                  long long words, int n_stripes, void* stream)
{
    if (!p || !d_ctx || !d_ids || !d_out || !d_coded || n_stripes < 0 || words < 0)
        return -1;
    if (n_stripes == 0 || words == 0)
        return 0;
    // (the context carries the ids, as dwords)
    return decode_rows(p, d_ctx, plan_src(p, d_data, dss, drs, d_coded, css, crs), d_counts,
                       d_entries, p->n_outputs, cap, p->sys ? p->k : 0, RowDst{d_out, oss, ors},
                       words, n_stripes, st(stream));
}

int qi_gpu_decode_ctx_packed(qi_plan* p, const uint16_t* d_ids,
                             const uint16_t* h_ids, int n_stripes,
                             const uint32_t* d_counts, const uint32_t* d_entries,
                             int cap, long long words, void* d_ctx, void* stream)
{
    if (!p || !d_ctx || n_stripes < 0 || words < 0)
        return -1;
    Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries),
           p->k, cap};
    (void)h_ids;
    return qi::build_ctx(p, d_ids, n_stripes, d_counts ? &in : nullptr, 0, 1, words,
                         d_ctx, st(stream));
}

int qi_gpu_decode_packed(qi_plan* p, const void* d_ctx, const uint16_t* d_recv,
                         long long rss, long long rrs, const uint32_t* d_counts,
                         const uint32_t* d_entries, int cap, uint16_t* d_out,
                         long long oss, long long ors, long long words,
                         int n_stripes, void* stream)
{
    if (!p || !d_ctx || !d_recv || !d_out || n_stripes < 0 || words < 0)
        return -1;
    if (n_stripes == 0 || words == 0)
        return 0;
    return decode_rows(p, d_ctx, RowSrc{d_recv, rss, rrs, 1 << 30, nullptr, 0, 0, 1, p->k, 0},
                       d_counts, d_entries, p->k, cap, 0, RowDst{d_out, oss, ors}, words,
                       n_stripes, st(stream));
}

// ---- fused repair (k <= 256): R x k Lagrange matrices applied by
// launch_matrix with input marks (the received rows') and output marks (the
// rebuilt rows') in one launch; per stripe the packed R x k block, then the
// sections of a matrix decode context ----
static bool repair_ok(const qi_plan* p, int R)
{
    return R >= 1 && R <= std::min(QI_REPAIR_MAX_TARGETS, p->code_len - p->k);
}

size_t qi_gpu_repair_ctx_bytes(const qi_plan* p, int n_targets, int n_stripes, long long words)
{
    if (!p || p->ntt || n_stripes < 0 || words < 0 || !repair_ok(p, n_targets))
        return 0;
    return static_cast<size_t>(mat_ctx_words(repair_layout(p, n_targets), words)) *
           sizeof(int32_t) * static_cast<size_t>(n_stripes);
}

int qi_gpu_repair_ctx(qi_plan* p, const uint16_t* d_ids, const uint16_t* d_targets, int R,
                      int n_stripes, const uint32_t* d_counts, const uint32_t* d_entries,
                      int cap, long long words, void* d_ctx, void* stream)
{
    if (!p || !d_ctx || n_stripes < 0 || words < 0)
        return -1;
    if (p->ntt)
        return QI_ERR_UNSUPPORTED;
    if (!repair_ok(p, R))
        return -1;
    if (n_stripes == 0)
        return 0;
    if (!d_ids || !d_targets)
        return -1;
    const MatLayout L = repair_layout(p, R);
    Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries), p->n_outputs, cap};
    return launch_repair_ctx(p->k, p->n, p->code_len, p->r, p->sys, L, d_ids, d_targets,
                             n_stripes, static_cast<int32_t*>(d_ctx), mat_ctx_words(L, words),
                             d_counts ? &in : nullptr, p->sys ? p->k : 0, words, p->d_err,
                             st(stream));
}

int qi_gpu_repair(qi_plan* p, const void* d_ctx, int R, const uint16_t* d_data, long long dss,
                  long long drs, const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_in_counts, const uint32_t* d_in_entries, int in_cap,
                  uint16_t* d_out, long long oss, long long ors, uint32_t* d_out_counts,
                  uint32_t* d_out_entries, int out_cap, long long words, int n_stripes,
                  void* stream)
{
    if (!p || !d_ctx || !d_out || !d_coded || n_stripes < 0 || words < 0)
        return -1;
    if (p->ntt)
        return QI_ERR_UNSUPPORTED;
    if (!repair_ok(p, R))
        return -1;
    if (n_stripes == 0 || words == 0)
        return 0;
    const MatLayout L = repair_layout(p, R);
    Oor in{const_cast<uint32_t*>(d_in_counts), const_cast<uint32_t*>(d_in_entries),
           p->n_outputs, in_cap};
    Oor outm{d_out_counts, d_out_entries, R, out_cap};  // output slot j = target j
    return apply_ctx(p, L, MatCtxView(L, d_ctx, mat_ctx_words(L, words), words),
                     plan_src(p, d_data, dss, drs, d_coded, css, crs), RowDst{d_out, oss, ors},
                     words, n_stripes, d_in_counts ? &in : nullptr, p->sys ? p->k : 0,
                     d_out_counts ? &outm : nullptr, st(stream));
}

const char* qi_gpu_repair_kernels(const qi_plan* p, int R, long long words)
{
    static thread_local std::string names;
    if (!p || p->ntt || words <= 0 || !repair_ok(p, R))
        return "";
    names = "repair=" + repair_ctx_kernel_name(p->k, R) + " + " +
            matrix_kernel_names(repair_layout(p, R), words, true, p->sys != 0, true);
    return names.c_str();
}

// ---- fused verify (k <= 256): the repair's launch in its _verify forms --
// the check rows recomputed from the basis rows and compared with the stored
// ones in the epilogue, their 65536 positions recorded in the work buckets --
// then verify_marks_kernel over the stored and the work buckets ----
size_t qi_gpu_verify_work_bytes(const qi_plan* p, int n_checks, int n_stripes, int work_cap)
{
    if (!p || p->ntt || n_stripes < 0 || work_cap < 0 || !repair_ok(p, n_checks))
        return 0;
    // per (stripe, check row): a count and work_cap entries
    return static_cast<size_t>(n_stripes) * n_checks * (1 + static_cast<size_t>(work_cap)) *
           sizeof(uint32_t);
}

int qi_gpu_verify(qi_plan* p, const void* d_ctx, int R, const uint16_t* d_checks,
                  const uint16_t* d_data, long long dss, long long drs, const uint16_t* d_coded,
                  long long css, long long crs, const uint32_t* d_counts,
                  const uint32_t* d_entries, int cap, void* d_work, int work_cap,
                  uint32_t* d_value_mismatch, uint32_t* d_mark_mismatch, uint32_t* d_first,
                  long long words, int n_stripes, void* stream)
{
    if (!p || !d_ctx || !d_coded || !d_checks || !d_work || !d_value_mismatch ||
        !d_mark_mismatch || !d_first || n_stripes < 0 || words < 0 || work_cap < 0)
        return -1;
    if (p->ntt)
        return QI_ERR_UNSUPPORTED;
    if (!repair_ok(p, R))
        return -1;
    if (n_stripes == 0)
        return 0;
    const long long n = static_cast<long long>(n_stripes) * R;
    uint32_t* wc = static_cast<uint32_t*>(d_work);
    if (int rc = launch_verify_init(d_value_mismatch, d_mark_mismatch, d_first, wc, n, st(stream)))
        return rc;
    if (words == 0)
        return 0;
    const MatLayout L = repair_layout(p, R);
    Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries), p->n_outputs, cap};
    Oor work{wc, wc + n, R, work_cap};  // work slot j = check row j
    const MatVerify ver{d_checks, d_value_mismatch, d_first};
    const int slot_base = p->sys ? p->k : 0;
    if (int rc = apply_ctx(p, L, MatCtxView(L, d_ctx, mat_ctx_words(L, words), words),
                           plan_src(p, d_data, dss, drs, d_coded, css, crs),
                           RowDst{nullptr, 0, 0}, words, n_stripes, d_counts ? &in : nullptr,
                           slot_base, &work, st(stream), &ver))
        return rc;
    return launch_verify_marks(d_checks, R, n_stripes, d_counts ? &in : nullptr, slot_base, work,
                               words, d_mark_mismatch, d_first, p->d_err, st(stream));
}

const char* qi_gpu_verify_kernels(const qi_plan* p, int R, long long words)
{
    static thread_local std::string names;
    if (!p || p->ntt || words <= 0 || !repair_ok(p, R))
        return "";
    names = "verify=" + repair_ctx_kernel_name(p->k, R) + " + " +
            matrix_kernel_names(repair_layout(p, R), words, true, p->sys != 0, false, true) +
            " + " + verify_marks_kernel_name();
    return names.c_str();
}

// ---- delta update (any k): update_ctx_kernel leaves the R x UP coefficients
// c(slot, id) per stripe, update_kernel streams the R coded rows past the U
// row differences ----
// the systematic plan's coefficient tables, built on the host and uploaded
// once (the copy is complete when hipMemcpy returns, so every stream sees it)
static int update_tables_ready(qi_plan* p)
{
    if (!p->sys)
        return 0;
    std::lock_guard<std::mutex> lock(p->upd_mu);
    if (p->d_upd_tab)
        return 0;
    UpdateTables t;
    if (!update_tables(p->k, p->m, p->r, t))
        return -3;
    t.ay.insert(t.ay.end(), t.iap.begin(), t.iap.end());
    uint32_t* d = nullptr;
    if (hipMalloc(&d, t.ay.size() * 4) != hipSuccess)
        return -2;
    if (hipMemcpy(d, t.ay.data(), t.ay.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(d);
        return -2;
    }
    p->d_upd_tab = d;
    return 0;
}

size_t qi_gpu_update_ctx_bytes(const qi_plan* p, int U, int R, int n_stripes)
{
    if (!p || n_stripes < 0 || !update_ok(p, U, R))
        return 0;
    return static_cast<size_t>(update_ctx_words(U, R)) * sizeof(int32_t) *
           static_cast<size_t>(n_stripes);
}

int qi_gpu_update_ctx(qi_plan* p, const uint16_t* d_ids, const uint16_t* d_slots, int U, int R,
                      int n_stripes, void* d_ctx, void* stream)
{
    if (!p || !d_ctx || n_stripes < 0)
        return -1;
    if (!update_ok(p, U, R) || (!d_slots && R != p->n_outputs))
        return -1;
    if (n_stripes == 0)
        return 0;
    if (!d_ids)
        return -1;
    if (int rc = update_tables_ready(p))
        return rc;
    return launch_update_ctx(p->k, p->n, p->n_outputs, p->r, p->sys, p->d_upd_tab, d_ids, d_slots,
                             U, update_up(U), R, n_stripes, static_cast<int32_t*>(d_ctx),
                             update_ctx_words(U, R), p->d_err, st(stream));
}

int qi_gpu_update(qi_plan* p, const void* d_ctx, int U, int R, const uint16_t* d_old,
                  long long old_ss, long long old_rs, const uint16_t* d_new, long long new_ss,
                  long long new_rs, const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_in_counts, const uint32_t* d_in_entries, int in_cap,
                  uint16_t* d_out, long long oss, long long ors, uint32_t* d_out_counts,
                  uint32_t* d_out_entries, int out_cap, long long words, int n_stripes,
                  void* stream)
{
    if (!p)
        return -1;
    return qi::update_rows(p, d_ctx, U, R, 0, d_old, old_ss, old_rs, d_new, new_ss, new_rs,
                           d_coded, css, crs, d_in_counts, d_in_entries, in_cap, d_out, oss, ors,
                           d_out_counts, d_out_entries, out_cap, words, n_stripes, st(stream));
}

const char* qi_gpu_update_kernels(const qi_plan* p, int U, int R, long long words)
{
    static thread_local std::string names;
    if (!p || words <= 0 || !update_ok(p, U, R))
        return "";
    names = "update=" + update_ctx_kernel_name() + " + " + update_kernel_name(update_up(U), true);
    return names.c_str();
}

// ---- fragment locate (k <= 256): locate_ctx_kernel leaves the points, the
// dual weights and the syndrome coefficients of the k + R listed fragments
// per stripe, locate_kernel streams their rows once and classifies the
// columns whose R syndromes are not all 0 (locate.hip, locate_math.h) ----
static bool locate_ok(const qi_plan* p, int R)
{
    return R >= 2 && R <= std::min(QI_LOCATE_MAX_CHECKS, p->code_len - p->k);
}

size_t qi_gpu_locate_ctx_bytes(const qi_plan* p, int R, int n_stripes)
{
    if (!p || p->k > kLocMaxK || n_stripes < 0 || !locate_ok(p, R))
        return 0;
    return static_cast<size_t>(locate_ctx_words(p->k, R)) * sizeof(int32_t) *
           static_cast<size_t>(n_stripes);
}

int qi_gpu_locate_ctx(qi_plan* p, const uint16_t* d_ids, int R, int n_stripes, void* d_ctx,
                      void* stream)
{
    if (!p || !d_ctx || n_stripes < 0)
        return -1;
    if (p->k > kLocMaxK)
        return QI_ERR_UNSUPPORTED;
    if (!locate_ok(p, R))
        return -1;
    if (n_stripes == 0)
        return 0;
    if (!d_ids)
        return -1;
    return launch_locate_ctx(p->k, R, p->code_len, p->r, d_ids, n_stripes,
                             static_cast<int32_t*>(d_ctx), p->d_err, st(stream));
}

int qi_gpu_locate(qi_plan* p, const void* d_ctx, int R, const uint32_t* d_stripes,
                  const uint16_t* d_data, long long dss, long long drs, const uint16_t* d_coded,
                  long long css, long long crs, const uint32_t* d_counts,
                  const uint32_t* d_entries, int cap, uint32_t* d_located, uint32_t* d_unlocated,
                  uint32_t* d_fix_counts, uint32_t* d_fixes, int fix_cap, long long words,
                  int n_stripes, void* stream)
{
    if (!p || !d_ctx || !d_coded || !d_located || !d_unlocated || !d_fix_counts ||
        n_stripes < 0 || words < 0 || fix_cap < 0 || (fix_cap > 0 && !d_fixes) ||
        (d_counts && cap > 0 && !d_entries))
        return -1;
    if (p->k > kLocMaxK)
        return QI_ERR_UNSUPPORTED;
    if (!locate_ok(p, R) || (p->sys && !d_data))
        return -1;
    if (n_stripes == 0)
        return 0;
    const Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries), p->n_outputs,
                 cap};
    return launch_locate(static_cast<const int32_t*>(d_ctx), p->k, R, p->sys ? p->k : 0,
                         d_stripes, d_data, dss, drs, d_coded, css, crs, in, d_located,
                         d_unlocated, d_fix_counts, d_fixes, fix_cap, words, n_stripes, p->d_err,
                         st(stream));
}

const char* qi_gpu_locate_kernels(const qi_plan* p, int R, long long words)
{
    static thread_local std::string names;
    if (!p || p->k > kLocMaxK || words <= 0 || !locate_ok(p, R))
        return "";
    names = "locate=" + locate_ctx_kernel_name(locate_rp(R)) + " + " +
            locate_kernel_name(locate_rp(R), true);
    return names.c_str();
}

// ---- multi-fragment locate: the same contexts and row pass, a bounded-
// distance decoder behind them (locate_multi.hip, locate_multi_math.h) ----
static_assert(QI_LOCATE_MAX_ERRORS == kLocMaxErrors, "qi_gpu.h and locate_multi_math.h differ");

int qi_gpu_locate_multi(qi_plan* p, const void* d_ctx, int R, int t, const uint32_t* d_stripes,
                        const uint16_t* d_data, long long dss, long long drs,
                        const uint16_t* d_coded, long long css, long long crs,
                        const uint32_t* d_counts, const uint32_t* d_entries, int cap,
                        uint32_t* d_located, uint32_t* d_unlocated, uint32_t* d_weights,
                        uint32_t* d_fix_counts, uint32_t* d_fixes, int fix_cap, long long words,
                        int n_stripes, void* stream)
{
    if (!p || !d_ctx || !d_coded || !d_located || !d_unlocated || !d_weights || !d_fix_counts ||
        n_stripes < 0 || words < 0 || fix_cap < 0 || (fix_cap > 0 && !d_fixes) ||
        (d_counts && cap > 0 && !d_entries))
        return -1;
    if (p->k > kLocMaxK)
        return QI_ERR_UNSUPPORTED;
    if (!locate_ok(p, R) || t < 1 || 2 * t > R || (p->sys && !d_data))
        return -1;
    if (n_stripes == 0)
        return 0;
    const Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries), p->n_outputs,
                 cap};
    return launch_locate_multi(static_cast<const int32_t*>(d_ctx), p->k, R, t, p->sys ? p->k : 0,
                               d_stripes, d_data, dss, drs, d_coded, css, crs, in, d_located,
                               d_unlocated, d_weights, d_fix_counts, d_fixes, fix_cap, words,
                               n_stripes, p->d_err, st(stream));
}

const char* qi_gpu_locate_multi_kernels(const qi_plan* p, int R, int t, long long words)
{
    static thread_local std::string names;
    if (!p || p->k > kLocMaxK || words <= 0 || !locate_ok(p, R) || t < 1 || 2 * t > R)
        return "";
    names = "locate_multi=" + locate_ctx_kernel_name(locate_rp(R)) + " + " +
            locate_multi_kernel_name(locate_rp(R), true);
    return names.c_str();
}

// ---- fragment fingerprints: F keyed digests of each listed row, homomorphic
// under the code (fingerprint.hip, fingerprint_math.h).  Any plan: no context
// is built ----
static_assert(QI_FINGERPRINT_MAX_KEYS == kFpMaxKeys, "qi_gpu.h and fingerprint_math.h differ");

static bool fingerprint_ok(const qi_plan* p, int N, int F, long long words)
{
    return p && F >= 1 && F <= kFpMaxKeys && N >= 1 && N <= p->code_len && words >= 1 &&
           words <= (1LL << 32);
}

size_t qi_gpu_fingerprint_work_bytes(const qi_plan* p, int N, int F, int n_stripes,
                                     long long words)
{
    if (!fingerprint_ok(p, N, F, words) || n_stripes < 0)
        return 0;
    return static_cast<size_t>(fp_work_words(static_cast<long long>(n_stripes) * N, fp_pad(F),
                                             words)) *
           sizeof(uint32_t);
}

int qi_gpu_fingerprint(qi_plan* p, const uint16_t* d_ids, int N, const uint32_t* h_keys, int F,
                       long long first_col, const uint16_t* d_data, long long dss, long long drs,
                       const uint16_t* d_coded, long long css, long long crs,
                       const uint32_t* d_counts, const uint32_t* d_entries, int cap, void* d_work,
                       uint32_t* d_fp, long long words, int n_stripes, void* stream)
{
    if (!fingerprint_ok(p, N, F, words) || !h_keys || first_col < 0 ||
        first_col > (1LL << 32) - words || n_stripes < 0 || cap < 0 ||
        (d_counts && cap > 0 && !d_entries))
        return -1;
    for (int e = 0; e < 3 * F; e++)
        if (h_keys[e] < 1u || h_keys[e] > 65536u)
            return -1;
    if (n_stripes == 0)
        return 0;
    if (!d_ids || !d_work || !d_fp || (!d_data && !d_coded) || (!p->sys && !d_coded) ||
        (d_data && (dss < 0 || drs < 0)) || (d_coded && (css < 0 || crs < 0)))
        return -1;
    const Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries), p->n_outputs,
                 cap};
    return launch_fingerprint(d_ids, N, h_keys, F, first_col, p->sys ? p->k : 0, p->code_len,
                              p->sys ? d_data : nullptr, dss, drs, d_coded, css, crs, in,
                              static_cast<uint32_t*>(d_work), d_fp, words, n_stripes, p->d_err,
                              st(stream));
}

const char* qi_gpu_fingerprint_kernels(const qi_plan* p, int N, int F, long long words)
{
    static thread_local std::string names;
    if (!fingerprint_ok(p, N, F, words))
        return "";
    names = "fingerprint=" + fingerprint_kernel_names(F, true, words);
    return names.c_str();
}

// ---- partial repair (any k): partial_ctx_kernel leaves the H x RP Lagrange
// weights of the held rows per stripe, partial_kernel streams the H rows past
// the R accumulators (partial.hip, partial_math.h) ----
static bool partial_ok(const qi_plan* p, int H, int R)
{
    return H >= 1 && H <= p->k && R >= 1 &&
           R <= std::min(QI_PARTIAL_MAX_TARGETS, p->code_len - p->k);
}

size_t qi_gpu_partial_ctx_bytes(const qi_plan* p, int H, int R, int n_stripes)
{
    if (!p || n_stripes < 0 || !partial_ok(p, H, R))
        return 0;
    return static_cast<size_t>(partial_ctx_words(H, R)) * sizeof(int32_t) *
           static_cast<size_t>(n_stripes);
}

int qi_gpu_partial_ctx(qi_plan* p, const uint16_t* d_ids, const uint16_t* d_held,
                       const uint16_t* d_targets, int H, int R, int n_stripes, void* d_ctx,
                       void* stream)
{
    if (!p || !d_ctx || n_stripes < 0)
        return -1;
    if (!partial_ok(p, H, R))
        return -1;
    if (n_stripes == 0)
        return 0;
    if (!d_ids || !d_held || !d_targets)
        return -1;
    return launch_partial_ctx(p->k, p->code_len, p->r, d_ids, d_held, d_targets, H, R, n_stripes,
                              static_cast<int32_t*>(d_ctx), p->d_err, st(stream));
}

// the accumulating row call of a partial repair and of a syndrome share: they
// differ in which counts `ok` admits
static int accumulate_rows(bool (*ok)(const qi_plan*, int, int), qi_plan* p, const void* d_ctx,
                           int H, int R, const uint16_t* d_rows, long long rss, long long rrs,
                           const uint32_t* d_in_counts, const uint32_t* d_in_entries, int in_cap,
                           const uint16_t* d_acc, long long ass, long long ars,
                           const uint32_t* d_acc_counts, const uint32_t* d_acc_entries,
                           int acc_cap, uint16_t* d_out, long long oss, long long ors,
                           uint32_t* d_out_counts, uint32_t* d_out_entries, int out_cap,
                           long long words, int n_stripes, void* stream)
{
    if (!p || !d_ctx || !d_rows || !d_out || n_stripes < 0 || words < 0 || in_cap < 0 ||
        acc_cap < 0 || out_cap < 0 || (d_in_counts && in_cap > 0 && !d_in_entries) ||
        (d_acc_counts && acc_cap > 0 && !d_acc_entries) ||
        (d_out_counts && out_cap > 0 && !d_out_entries))
        return -1;
    if (!ok(p, H, R))
        return -1;
    if (n_stripes == 0 || words == 0)
        return 0;
    const Oor in{const_cast<uint32_t*>(d_in_counts), const_cast<uint32_t*>(d_in_entries), H,
                 in_cap};
    // (no acc rows: no acc marks)
    const Oor accm{d_acc ? const_cast<uint32_t*>(d_acc_counts) : nullptr,
                   const_cast<uint32_t*>(d_acc_entries), R, acc_cap};
    const Oor outm{d_out_counts, d_out_entries, R, out_cap};
    return launch_partial(static_cast<const int32_t*>(d_ctx), H, R, p->sys ? p->k : 0, d_rows, rss,
                          rrs, in, d_acc, ass, ars, accm, d_out, oss, ors, outm, words, n_stripes,
                          p->d_err, st(stream));
}

int qi_gpu_partial(qi_plan* p, const void* d_ctx, int H, int R, const uint16_t* d_rows,
                   long long rss, long long rrs, const uint32_t* d_in_counts,
                   const uint32_t* d_in_entries, int in_cap, const uint16_t* d_acc, long long ass,
                   long long ars, const uint32_t* d_acc_counts, const uint32_t* d_acc_entries,
                   int acc_cap, uint16_t* d_out, long long oss, long long ors,
                   uint32_t* d_out_counts, uint32_t* d_out_entries, int out_cap, long long words,
                   int n_stripes, void* stream)
{
    return accumulate_rows(partial_ok, p, d_ctx, H, R, d_rows, rss, rrs, d_in_counts, d_in_entries,
                           in_cap, d_acc, ass, ars, d_acc_counts, d_acc_entries, acc_cap, d_out,
                           oss, ors, d_out_counts, d_out_entries, out_cap, words, n_stripes,
                           stream);
}

const char* qi_gpu_partial_kernels(const qi_plan* p, int H, int R, long long words)
{
    static thread_local std::string names;
    if (!p || words <= 0 || !partial_ok(p, H, R))
        return "";
    names = "partial=" + partial_ctx_kernel_name() + " + " +
            partial_kernel_name(partial_rp(R), true);
    return names.c_str();
}

// ---- syndrome shares (any k): syndrome_ctx_kernel leaves the H x RP syndrome
// coefficients of the held rows in a partial repair's context layout and the
// share is launch_partial; syndrome_locate_ctx_kernel and
// syndrome_locate_kernel decide the columns from the R summed rows
// (syndrome.hip, syndrome_math.h) ----
static_assert(QI_SYNDROME_MAX_CHECKS == kSynMaxChecks && QI_SYNDROME_MAX_ERRORS == kSynMaxErrors,
              "qi_gpu.h and syndrome_math.h differ");

static bool syndrome_checks_ok(const qi_plan* p, int R)
{
    return R >= 1 && R <= std::min(QI_SYNDROME_MAX_CHECKS, p->code_len - p->k);
}

static bool syndrome_ok(const qi_plan* p, int H, int R)
{
    return syndrome_checks_ok(p, R) && H >= 1 && H <= p->k + R;
}

size_t qi_gpu_syndrome_ctx_bytes(const qi_plan* p, int H, int R, int n_stripes)
{
    if (!p || n_stripes < 0 || !syndrome_ok(p, H, R))
        return 0;
    return static_cast<size_t>(syndrome_ctx_words(H, R)) * sizeof(int32_t) *
           static_cast<size_t>(n_stripes);
}

int qi_gpu_syndrome_ctx(qi_plan* p, const uint16_t* d_ids, const uint16_t* d_held, int H, int R,
                        int n_stripes, void* d_ctx, void* stream)
{
    if (!p || !d_ctx || n_stripes < 0)
        return -1;
    if (!syndrome_ok(p, H, R))
        return -1;
    if (n_stripes == 0)
        return 0;
    if (!d_ids || !d_held)
        return -1;
    return launch_syndrome_ctx(p->k, p->code_len, p->r, d_ids, d_held, H, R, n_stripes,
                               static_cast<int32_t*>(d_ctx), p->d_err, st(stream));
}

int qi_gpu_syndrome(qi_plan* p, const void* d_ctx, int H, int R, const uint16_t* d_rows,
                    long long rss, long long rrs, const uint32_t* d_in_counts,
                    const uint32_t* d_in_entries, int in_cap, const uint16_t* d_acc,
                    long long ass, long long ars, const uint32_t* d_acc_counts,
                    const uint32_t* d_acc_entries, int acc_cap, uint16_t* d_out, long long oss,
                    long long ors, uint32_t* d_out_counts, uint32_t* d_out_entries, int out_cap,
                    long long words, int n_stripes, void* stream)
{
    return accumulate_rows(syndrome_ok, p, d_ctx, H, R, d_rows, rss, rrs, d_in_counts,
                           d_in_entries, in_cap, d_acc, ass, ars, d_acc_counts, d_acc_entries,
                           acc_cap, d_out, oss, ors, d_out_counts, d_out_entries, out_cap, words,
                           n_stripes, stream);
}

const char* qi_gpu_syndrome_kernels(const qi_plan* p, int H, int R, long long words)
{
    static thread_local std::string names;
    if (!p || words <= 0 || !syndrome_ok(p, H, R))
        return "";
    names = "syndrome=" + syndrome_ctx_kernel_name() + " + " +
            partial_kernel_name(partial_rp(R), true);
    return names.c_str();
}

size_t qi_gpu_syndrome_locate_ctx_bytes(const qi_plan* p, int R, int n_stripes)
{
    if (!p || n_stripes < 0 || !syndrome_checks_ok(p, R))
        return 0;
    return static_cast<size_t>(syndrome_locate_ctx_words(p->k + R)) * sizeof(int32_t) *
           static_cast<size_t>(n_stripes);
}

int qi_gpu_syndrome_locate_ctx(qi_plan* p, const uint16_t* d_ids, int R, int n_stripes,
                               void* d_ctx, void* stream)
{
    if (!p || !d_ctx || n_stripes < 0)
        return -1;
    if (!syndrome_checks_ok(p, R))
        return -1;
    if (n_stripes == 0)
        return 0;
    if (!d_ids)
        return -1;
    return launch_syndrome_locate_ctx(p->k, R, p->code_len, p->r, d_ids, n_stripes,
                                      static_cast<int32_t*>(d_ctx), p->d_err, st(stream));
}

int qi_gpu_syndrome_locate(qi_plan* p, const void* d_ctx, int R, int t, const uint16_t* d_syn,
                           long long sss, long long srs, const uint32_t* d_counts,
                           const uint32_t* d_entries, int cap, uint32_t* d_located,
                           uint32_t* d_unlocated, uint32_t* d_weights, uint32_t* d_fix_counts,
                           uint32_t* d_fixes, int fix_cap, long long words, int n_stripes,
                           void* stream)
{
    if (!p || !d_ctx || !d_syn || !d_located || !d_unlocated || !d_weights || !d_fix_counts ||
        n_stripes < 0 || words < 0 || cap < 0 || fix_cap < 0 || (fix_cap > 0 && !d_fixes) ||
        (d_counts && cap > 0 && !d_entries))
        return -1;
    if (!syndrome_checks_ok(p, R) || t < 0 || 2 * t > R)
        return -1;
    if (n_stripes == 0)
        return 0;
    const Oor in{const_cast<uint32_t*>(d_counts), const_cast<uint32_t*>(d_entries), R, cap};
    return launch_syndrome_locate(static_cast<const int32_t*>(d_ctx), p->k, R, t, d_syn, sss, srs,
                                  in, d_located, d_unlocated, d_weights, d_fix_counts, d_fixes,
                                  fix_cap, words, n_stripes, p->d_err, st(stream));
}

const char* qi_gpu_syndrome_locate_kernels(const qi_plan* p, int R, int t, long long words)
{
    static thread_local std::string names;
    if (!p || words <= 0 || !syndrome_checks_ok(p, R) || t < 0 || 2 * t > R)
        return "";
    names = "syndrome_locate=" + syndrome_locate_ctx_kernel_name() + " + " +
            syndrome_locate_kernel_name(syndrome_locate_rp(R), true);
    return names.c_str();
}

// ---- device patch: patch_kernel applies the fix lists of a locate to the rows
// and the buckets, one block per list position (patch.hip, patch_math.h) ----
static_assert(QI_PATCH_ABSOLUTE == kPatchAbsolute && QI_PATCH_DELTA == kPatchDelta &&
                  QI_PATCH_NONE == kPatchNone && QI_PATCH_DONE == kPatchDone &&
                  QI_PATCH_UNLOCATED == kPatchUnlocated && QI_PATCH_TRUNCATED == kPatchTruncated &&
                  QI_PATCH_BAD_FIX == kPatchBadFix && QI_PATCH_DATA_MARK == kPatchDataMark &&
                  QI_PATCH_BUCKET_FULL == kPatchBucketFull &&
                  QI_PATCH_MAX_FIXES == kPatchMaxFixes,
              "qi_gpu.h and patch_math.h differ");

static bool patch_ok(const qi_plan* p, int N)
{
    return p && N >= 1 && N <= p->code_len;
}

size_t qi_gpu_patch_work_bytes(const qi_plan* p, int N, int n_stripes)
{
    if (!patch_ok(p, N) || n_stripes < 1)
        return 0;
    return static_cast<size_t>(patch_work_words(N, n_stripes)) * sizeof(uint32_t);
}

int qi_gpu_patch(qi_plan* p, int mode, const uint16_t* d_ids, int N, const uint8_t* d_mine,
                 const uint32_t* d_stripes, const uint32_t* d_unlocated,
                 const uint32_t* d_fix_counts, const uint32_t* d_fixes, int fix_cap,
                 uint16_t* d_data, long long dss, long long drs, uint16_t* d_coded, long long css,
                 long long crs, uint32_t* d_counts, uint32_t* d_entries, int cap, void* d_work,
                 uint32_t* d_status, uint32_t* d_applied, long long words, int n_stripes,
                 void* stream)
{
    if (!patch_ok(p, N) || (mode != QI_PATCH_ABSOLUTE && mode != QI_PATCH_DELTA) || fix_cap < 0 ||
        words < 1 || words > (1LL << 32) || n_stripes < 1)
        return -1;
    if (!d_ids || !d_fix_counts || (fix_cap > 0 && !d_fixes) || !d_work || !d_status ||
        !d_applied || cap < 0 || (d_counts && cap > 0 && !d_entries) ||
        (d_data && (dss < 0 || drs < 0)) || (d_coded && (css < 0 || crs < 0)))
        return -1;
    const Oor marks{d_counts, d_entries, p->n_outputs, cap};
    return launch_patch(mode, p->sys, p->k, p->code_len, d_ids, N, d_mine, d_stripes, d_unlocated,
                        d_fix_counts, d_fixes, fix_cap, p->sys ? d_data : nullptr, dss, drs,
                        d_coded, css, crs, marks, static_cast<uint32_t*>(d_work), d_status,
                        d_applied, words, n_stripes, p->d_err, st(stream));
}

const char* qi_gpu_patch_kernels(const qi_plan* p, int N, int mode, long long words)
{
    static thread_local std::string names;
    if (!patch_ok(p, N) || (mode != QI_PATCH_ABSOLUTE && mode != QI_PATCH_DELTA) || words < 1 ||
        words > (1LL << 32))
        return "";
    names = "patch=" + patch_kernel_name();
    return names.c_str();
}

const char* qi_gpu_kernels(const qi_plan* p, long long words)
{
    static thread_local std::string names;
    if (!p || words <= 0)
        return "";
    std::string enc, dec;
    if (!use_matrix(p, words)) {
        enc = ntt_kernel_names(p, false);
        dec = ntt_kernel_names(p, true);
    } else {
        if (p->ntt && !p->d_gen)
            enc = ntt_kernel_names(p, false);
        else if (!p->d_gen)
            enc = encode_fnt_kernel_name(p->k);
        else
            enc = matrix_kernel_names(p->gen, words, false, false);
        dec = decode_ctx_kernel_name(p->k) + " + " +
              matrix_kernel_names(ctx_layout(p), words, true, p->sys != 0);
    }
    names = "encode=" + enc + "; decode=" + dec;
    return names.c_str();
}

// git describe of the tree the library was built from + a hash of its
// sources (quadiron_amd/csrc/Makefile writes QI_BUILD_ID), so a run's
// record ties the loaded binary to a commit
const char* qi_build_id(void)
{
#ifdef QI_BUILD_ID
    return QI_BUILD_ID;
#else
    return "unknown";
#endif
}

int qi_gpu_take_error(qi_plan* p)
{
    if (!p)
        return -1;
    uint32_t e = 0;
    if (hipMemcpy(&e, p->d_err, 4, hipMemcpyDeviceToHost) != hipSuccess)
        return -2;
    if (e)
        (void)hipMemset(p->d_err, 0, 4);
    return static_cast<int>(e);
}

}  // extern "C"
