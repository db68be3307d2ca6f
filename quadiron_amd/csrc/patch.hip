// Device patch (qi_gpu_patch): the fix lists a locate leaves in device memory
// -- {column, list position, symbol} of qi_gpu_locate / qi_gpu_locate_multi,
// {column, list position, error} of qi_gpu_syndrome_locate -- applied to the
// rows and to the unordered OOR buckets without leaving the stream.  The rule
// is fec_stage.h's apply_fixes / apply_deltas, per stripe and all or nothing;
// the per-fix decisions are patch_math.h's.
//
// The work is list-driven: one block of kPatchBlock lanes per list position
// walks the stripe's fix list kPatchBlock entries at a time, in phases
// separated by block barriers.  No block looks at another stripe, so nothing
// is handed over between blocks.
//
//   0  the stripe's own refusals (unlocated, truncated); the counters in
//      d_work of the positions the list names are reset.
//   1  every fix is validated and classified against the untouched rows and
//      buckets: is the column in the row's bucket (a linear scan: buckets are
//      unordered), the symbol v, the mark transition.  Per position the marks
//      inserted and removed are counted in d_work, and the smallest index of
//      a fix that edits the position's bucket becomes its owner.  A fix that
//      inserts a mark sets its bit in LDS: once its word is written nothing
//      else tells it from a fix that wrote a plain 0 (in delta mode v is gone
//      with the old word).  The bits are the block's dynamic LDS, sized by
//      the launch for min(fix_cap, kPatchMaxFixes) entries; a longer list is
//      refused as truncated.
//   2  old + inserted - removed against oor_cap per touched bucket; the
//      status is the smallest code found.  A refused stripe ends here: nothing
//      has been written.
//   3  the symbols, one 2-byte store per fix (two fixes may share a dword).
//      Delta mode reads the word and scans the bucket once more: nothing has
//      edited either.
//   4  the buckets, behind a barrier: every scan of phases 1 and 3 is over.
//      The owner lane of a position edits its bucket alone and in order:
//      first the removals, each by moving the last entry into the gap, then
//      the insertions at the end, never at or past oor_cap; then the count.
//      Old + inserted may exceed oor_cap where old + inserted - removed does
//      not, hence removals first.
//
// Cost: phases 1 and 3 are O(count) per fix over all lanes; phase 4 is one
// lane per touched bucket, O(fixes) to pick its entries plus O(count) per
// removal.  A full bucket with a list of similar length is quadratic, and in
// phase 4 serial.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "patch_math.h"
#include "qi_internal.h"

namespace qi {

constexpr int kPatchBlock = 256;

struct PatchArgs {
    int mode, sys, k, code_len, N;
    const uint16_t* ids;        // [S][N]
    const uint8_t* mine;        // [S][N] or null
    const uint32_t* stripes;    // [S] or null
    const uint32_t* unlocated;  // [S] or null
    const uint32_t* fix_counts;
    const uint32_t* fixes;
    int fix_cap;
    uint16_t* data;
    long long dss, drs;
    uint16_t* coded;
    long long css, crs;
    Oor m;  // the coded rows' buckets by slot (counts null: no marks)
    uint32_t* work;
    uint32_t* status;
    uint32_t* applied;
    unsigned long long words;
    uint32_t* err;
};

// a fix entry against the call's arguments: where it points
struct PatchSite {
    uint32_t code;  // kPatchOk, or kPatchBadFix
    bool skip;      // not held here
    uint32_t col, p, w;
    bool is_data;
    uint16_t* word;   // the row's word
    uint32_t* count;  // the row's bucket (null: a data row, or no buckets)
    uint32_t* ent;
    uint32_t n;  // its count
};

// what a block keeps of the call: its list position's lists and the bases of
// its stripe's rows and buckets
struct PatchStripe {
    int mode, sys, k, code_len, N;
    unsigned long long words;
    const uint32_t* fx;
    const uint16_t* ids;
    const uint8_t* mine;  // null: everything is held here
    uint16_t* data;       // null: region not passed
    uint16_t* coded;
    long long drs, crs;
    uint32_t* counts;  // null: no marks
    uint32_t* entries;
    uint32_t cap;  // 0 without counts
};

__device__ __forceinline__ PatchSite patch_site(const PatchStripe& a, uint32_t e)
{
    PatchSite t{};
    t.col = a.fx[3 * static_cast<long long>(e)];
    t.p = a.fx[3 * static_cast<long long>(e) + 1];
    t.w = a.fx[3 * static_cast<long long>(e) + 2];
    t.code = kPatchBadFix;
    if (t.p >= static_cast<uint32_t>(a.N))
        return t;
    if (a.mine && !a.mine[t.p]) {
        t.code = kPatchOk;
        t.skip = true;
        return t;
    }
    const uint32_t id = a.ids[t.p];
    if (patch_entry_code(a.mode, a.words, static_cast<uint32_t>(a.code_len), t.col, id, t.w) !=
        kPatchOk)
        return t;
    const PatchRow r = patch_row(a.sys != 0, static_cast<uint32_t>(a.k), id);
    t.is_data = r.is_data;
    uint16_t* base = r.is_data ? a.data : a.coded;
    if (!base)
        return t;
    t.word = base + static_cast<long long>(r.slot) * (r.is_data ? a.drs : a.crs) + t.col;
    if (!r.is_data && a.counts) {
        t.count = a.counts + r.slot;
        t.ent = a.entries + static_cast<long long>(r.slot) * a.cap;
        t.n = *t.count;
    }
    t.code = kPatchOk;
    return t;
}

// the index of col among the first n entries, or -1
__device__ __forceinline__ long long patch_find(const uint32_t* ent, uint32_t n, uint32_t col)
{
    for (uint32_t i = 0; i < n; i++)
        if (ent[i] == col)
            return i;
    return -1;
}

// d_work's words are touched by atomics only: they bypass the lanes' cache
__device__ __forceinline__ uint32_t patch_work_load(uint32_t* w)
{
    return __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kPatchBlock) void patch_kernel(PatchArgs a)
{
    extern __shared__ uint32_t s_ins[];  // one bit per fix: the fixes that insert a mark
    __shared__ uint32_t s_code, s_applied;
    const int s = static_cast<int>(blockIdx.x);
    const uint32_t tid = threadIdx.x;

    // ---- 0: the stripe's own refusals
    const uint32_t F = a.fix_counts[s];
    uint32_t code = kPatchOk;
    if (a.unlocated && a.unlocated[s])
        code = kPatchUnlocated;
    else if (F > static_cast<uint32_t>(a.fix_cap) || F > static_cast<uint32_t>(kPatchMaxFixes))
        code = kPatchTruncated;
    if (code != kPatchOk || F == 0) {
        if (tid == 0) {
            a.status[s] = code != kPatchOk ? code : kPatchNone;
            a.applied[s] = 0;
        }
        return;
    }
    const long long st = a.stripes ? static_cast<long long>(a.stripes[s]) : s;
    const uint32_t cap = a.m.counts ? static_cast<uint32_t>(a.m.cap) : 0u;
    const uint32_t* fx = a.fixes + static_cast<long long>(s) * a.fix_cap * 3;
    const PatchStripe ps{a.mode, a.sys, a.k, a.code_len, a.N, a.words, fx,
                         a.ids + static_cast<long long>(s) * a.N,
                         a.mine ? a.mine + static_cast<long long>(s) * a.N : nullptr,
                         a.data ? a.data + st * a.dss : nullptr,
                         a.coded ? a.coded + st * a.css : nullptr, a.drs, a.crs,
                         a.m.counts ? a.m.counts + st * a.m.slots : nullptr,
                         a.m.counts ? a.m.entries + st * a.m.slots * a.m.cap : nullptr, cap};
    uint32_t* work_s = a.work + static_cast<long long>(s) * a.N * kPatchWorkWords;

    for (uint32_t i = tid; i < (F + 31) / 32; i += kPatchBlock)
        s_ins[i] = 0;
    if (tid == 0) {
        s_code = kPatchOk;
        s_applied = 0;
    }
    for (uint32_t e = tid; e < F; e += kPatchBlock) {
        const uint32_t p = fx[3 * static_cast<long long>(e) + 1];
        if (p < static_cast<uint32_t>(a.N)) {
            uint32_t* w = work_s + static_cast<long long>(p) * kPatchWorkWords;
            atomicExch(w, 0u);
            atomicExch(w + 1, 0u);
            atomicExch(w + 2, 0xffffffffu);
        }
    }
    __syncthreads();

    // ---- 1: validate and classify; no write to a row or a bucket
    uint32_t worst = kPatchOk, n_ok = 0;
    for (uint32_t e = tid; e < F; e += kPatchBlock) {
        const PatchSite t = patch_site(ps, e);
        uint32_t c = t.code;
        if (c == kPatchOk && !t.skip) {
            const bool over = t.count && t.n > cap;
            if (over)
                atomicOr(a.err, kErrOorTruncated);
            bool present = false;
            uint32_t stored = 0;
            if (!over) {
                present = t.count && patch_find(t.ent, t.n, t.col) >= 0;
                stored = *t.word;
            }
            const PatchFix r = patch_fix(a.mode, t.is_data, over, present, stored, t.w);
            c = r.code;
            if (c == kPatchOk) {
                n_ok++;
                if (r.dir) {
                    uint32_t* w = work_s + static_cast<long long>(t.p) * kPatchWorkWords;
                    atomicAdd(w + (r.dir > 0 ? 0 : 1), 1u);
                    atomicMin(w + 2, e);
                    if (r.dir > 0)
                        atomicOr(&s_ins[e >> 5], 1u << (e & 31u));
                }
            }
        }
        worst = min(worst, c);
    }
    if (worst != kPatchOk)
        atomicMin(&s_code, worst);
    if (n_ok)
        atomicAdd(&s_applied, n_ok);
    __syncthreads();

    // ---- 2: the buckets' new counts (only over a list that is valid)
    const bool valid = s_code == kPatchOk;
    __syncthreads();
    if (valid) {
        bool full = false;
        for (uint32_t e = tid; e < F; e += kPatchBlock) {
            const PatchSite t = patch_site(ps, e);
            if (t.skip || t.is_data)
                continue;
            uint32_t* w = work_s + static_cast<long long>(t.p) * kPatchWorkWords;
            full |= patch_bucket_full(t.n, patch_work_load(w), patch_work_load(w + 1), cap);
        }
        if (full)
            atomicMin(&s_code, kPatchBucketFull);
    }
    __syncthreads();
    code = s_code;
    const uint32_t n_applied = s_applied;
    if (code != kPatchOk || n_applied == 0) {
        if (tid == 0) {
            a.status[s] = code != kPatchOk ? code : kPatchNone;
            a.applied[s] = 0;
        }
        return;
    }

    // ---- 3: the symbols
    for (uint32_t e = tid; e < F; e += kPatchBlock) {
        const PatchSite t = patch_site(ps, e);
        if (t.skip)
            continue;
        uint32_t v = 65536u;
        if (!(s_ins[e >> 5] >> (e & 31u) & 1u)) {
            const bool present =
                a.mode == kPatchDelta && t.count && patch_find(t.ent, t.n, t.col) >= 0;
            v = patch_fix(a.mode, t.is_data, false, present, *t.word, t.w).v;
        }
        *t.word = patch_stored(v);
    }
    __syncthreads();  // every scan is over

    // ---- 4: the buckets, each by its owner lane
    for (uint32_t e = tid; e < F; e += kPatchBlock) {
        const PatchSite t = patch_site(ps, e);
        if (t.skip || !t.count)
            continue;
        if (patch_work_load(work_s + static_cast<long long>(t.p) * kPatchWorkWords + 2) != e)
            continue;
        uint32_t cur = t.n;
        // a column leaves the bucket where it is there and the new symbol is
        // not 65536 (a delta never leaves 65536 in place)
        for (uint32_t e2 = 0; e2 < F; e2++) {
            const uint32_t* f2 = fx + 3 * static_cast<long long>(e2);
            if (f2[1] != t.p || (s_ins[e2 >> 5] >> (e2 & 31u) & 1u) ||
                (a.mode == kPatchAbsolute && f2[2] == 65536u))
                continue;
            const long long i = patch_find(t.ent, cur, f2[0]);
            if (i >= 0) {
                cur--;
                t.ent[i] = t.ent[cur];
            }
        }
        for (uint32_t e2 = 0; e2 < F; e2++) {
            const uint32_t* f2 = fx + 3 * static_cast<long long>(e2);
            if (f2[1] == t.p && (s_ins[e2 >> 5] >> (e2 & 31u) & 1u) && cur < cap)
                t.ent[cur++] = f2[0];
        }
        *t.count = cur;
    }
    if (tid == 0) {
        a.status[s] = kPatchDone;
        a.applied[s] = n_applied;
    }
}

std::string patch_kernel_name()
{
    return "patch_kernel";
}

int launch_patch(int mode, int sys, int k, int code_len, const uint16_t* d_ids, int N,
                 const uint8_t* d_mine, const uint32_t* d_stripes, const uint32_t* d_unlocated,
                 const uint32_t* d_fix_counts, const uint32_t* d_fixes, int fix_cap,
                 uint16_t* d_data, long long dss, long long drs, uint16_t* d_coded, long long css,
                 long long crs, const Oor& marks, uint32_t* d_work, uint32_t* d_status,
                 uint32_t* d_applied, long long words, int n_stripes, uint32_t* d_err,
                 hipStream_t st)
{
    if ((mode != kPatchAbsolute && mode != kPatchDelta) || N < 1 || N > code_len ||
        code_len > 65536 || fix_cap < 0 || words < 1 ||
        words > (1LL << 32) || n_stripes < 1)
        return -3;
    const PatchArgs a{mode, sys, k, code_len, N, d_ids, d_mine, d_stripes, d_unlocated,
                      d_fix_counts, d_fixes, fix_cap, d_data, dss, drs, d_coded, css, crs, marks,
                      d_work, d_status, d_applied, static_cast<unsigned long long>(words), d_err};
    // the bits of the longest list a stripe can have (at most 32 KiB)
    const size_t lds = static_cast<size_t>((std::min(fix_cap, kPatchMaxFixes) + 31) / 32) * 4;
    hipLaunchKernelGGL(patch_kernel, dim3(static_cast<unsigned>(n_stripes)), dim3(kPatchBlock),
                       lds, st, a);
    return hipGetLastError() == hipSuccess ? 0 : -2;
}

}  // namespace qi
