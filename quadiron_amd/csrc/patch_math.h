// patch_math.h -- the per-fix decisions of the device patch (qi_gpu_patch,
// patch.hip): where the fragment at a list position lives, whether a fix
// entry is valid, the symbol it asks for in both modes, and what that does to
// the row's mark.  It is apply_fixes / apply_deltas of fec_stage.h, one fix at
// a time.  No HIP here (constexpr functions compile for both sides): the
// kernel and tests/host/test_patch_math.cpp share it.
#pragma once

#include <stdint.h>

namespace qi {

constexpr int kPatchAbsolute = 0;  // third word: the symbol v in [0, 65536]
constexpr int kPatchDelta = 1;     // third word: the error e in [1, 65536]

// per-stripe status (QI_PATCH_* of qi_gpu.h); a stripe reports the smallest
// code from kPatchUnlocated on that applies
constexpr uint32_t kPatchNone = 0, kPatchDone = 1, kPatchUnlocated = 2, kPatchTruncated = 3,
                   kPatchBadFix = 4, kPatchDataMark = 5, kPatchBucketFull = 6;
// "no refusal": above every code
constexpr uint32_t kPatchOk = 7;

// The longest list a stripe may have: the kernel keeps one bit per entry in
// LDS (the entries that insert a mark), 32 KiB at this length
constexpr int kPatchMaxFixes = 1 << 18;

// Fragment ids are the decode's id space: systematic f < k is data row f (no
// bucket), f >= k coded slot f - k; non-systematic f is coded slot f
struct PatchRow {
    bool is_data;
    uint32_t slot;
};

constexpr PatchRow patch_row(bool sys, uint32_t k, uint32_t id)
{
    return sys && id < k ? PatchRow{true, id} : PatchRow{false, sys ? id - k : id};
}

// the third word's range
constexpr bool patch_word_ok(int mode, uint32_t w)
{
    return mode == kPatchDelta ? w >= 1u && w <= 65536u : w <= 65536u;
}

// the symbol the fix asks for, from the restored symbol y of the row (65536
// where the column is in the row's bucket, else the stored word)
constexpr uint32_t patch_symbol(int mode, uint32_t y, uint32_t w)
{
    return mode == kPatchDelta ? (y >= w ? y - w : y + 65537u - w) : w;
}

// what a row stores for v
constexpr uint16_t patch_stored(uint32_t v)
{
    return static_cast<uint16_t>(v & 0xffffu);
}

// the mark transition: +1 the column enters the bucket, -1 it leaves it, 0
// the bucket stays as it is
constexpr int patch_transition(bool present, uint32_t v)
{
    return v == 65536u ? (present ? 0 : 1) : (present ? -1 : 0);
}

// One fix that is not skipped, against its row: the refusal it causes
// (kPatchOk: none), its symbol and its transition.  have_region: the row's
// region was passed (not NULL); marks: the call has buckets (counts not NULL);
// over_cap: the row's bucket count is above its capacity; present: the column
// is in the bucket; stored: the row's word.  The caller has checked the
// position; nothing of the row is looked at unless the entry is valid
struct PatchFix {
    uint32_t code;
    uint32_t v;
    int dir;
};

constexpr uint32_t patch_entry_code(int mode, unsigned long long words, uint32_t code_len,
                                    uint32_t col, uint32_t id, uint32_t w)
{
    return col >= words || !patch_word_ok(mode, w) || id >= code_len ? kPatchBadFix : kPatchOk;
}

constexpr PatchFix patch_fix(int mode, bool is_data, bool over_cap, bool present,
                             uint32_t stored, uint32_t w)
{
    if (!is_data && over_cap)
        return PatchFix{kPatchBadFix, 0, 0};
    const uint32_t y = !is_data && present ? 65536u : stored;
    const uint32_t v = patch_symbol(mode, y, w);
    if (is_data)
        return PatchFix{v == 65536u ? kPatchDataMark : kPatchOk, v, 0};
    return PatchFix{kPatchOk, v, patch_transition(present, v)};
}

// a bucket of `count` marks that gains ins and loses rem of them
constexpr bool patch_bucket_full(uint32_t count, uint32_t ins, uint32_t rem, uint32_t cap)
{
    return static_cast<unsigned long long>(count) + ins - rem > cap;
}

// d_work: three words per (stripe, list position) -- marks inserted, marks
// removed, and the smallest fix index that edits the position's bucket
constexpr int kPatchWorkWords = 3;

constexpr unsigned long long patch_work_words(int n_listed, int n_stripes)
{
    return static_cast<unsigned long long>(n_listed) * n_stripes * kPatchWorkWords;
}

}  // namespace qi
