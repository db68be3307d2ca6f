// fingerprint_math.h -- the arithmetic of the fragment fingerprint
// (qi_gpu_fingerprint, include/qi_gpu.h), host + device: the weight digits,
// the power tables, the lazy-reduction steps of fingerprint.hip's lanes and a
// plain 64-bit reference.  No HIP: tests/host/test_fingerprint_math.cpp
// compiles it alone.
//
// Definition.  Column C = first_col + c of a row has the base-256 digits
//   C0 = C & 255, C1 = (C >> 8) & 255, C2 = C >> 16
// and under the key (a, b, d), each in [1, 65536], the weight
//   w(C) = a^C0 b^C1 d^C2  (mod 65537),
// never 0.  fp = sum_c y_c w(first_col + c) over the restored symbols y_c in
// [0, 65536], canonical in [0, 65536].
//
// How a lane computes it.  The weight splits into a^C0, which a lane keeps as
// one constant per key (its columns are 256 apart, or 8 adjacent ones whose
// a^i, i < 8, are the same in every lane), and the "hi" weight b^C1 d^C2 of
// H = C >> 8, which the block keeps for the kFpHi values of H its chunk of
// columns can meet.  All three come from tables a setup kernel leaves in the
// work buffer (fp_tab_entry): a^x and b^x for x < 256, d^(C2base + x).
//
// Ranges (gf65537.h: |x| < 2^31 -> fold(x) in [-32767, 98303]; x in [-98305,
// 163840] -> fold(x) in [-2, 65537]):
//   - a stored u16 (<= 65535) times a balanced weight (|c| <= 32768) stays
//     below 2^31, but leaves no room for an accumulator.  The lanes therefore
//     balance the symbol first (fp_sym: |y| <= 32768, a marked symbol is
//     65536 = -1), so that |y c| <= 2^30;
//   - acc = fold(mul24(y, c) + acc) (fp_step) then keeps acc in [-32767,
//     98303]: |y c + acc| <= 2^30 + 98303 < 2^31, as in locate_rows.h;
//   - a lane piece (fp_piece) is 8 such steps from 0; one more fold and a
//     balance (fp_rebalance: [-32767, 98303] -> [-2, 65537] -> [-32768,
//     32768]) make it a symbol again for the step with the hi weight;
//   - fp_canon brings [-32767, 98303] to [0, 65536] with one correction each
//     way, and the lane's a^C0 is one canonical product (fp_mulmod) at the
//     end of a chunk.
#pragma once

#include <stdint.h>

#include "gf65537.h"

namespace qi {

constexpr int kFpMaxKeys = 8;
constexpr int kFpBlock = 256;
constexpr int kFpCols = 8;  // columns per lane and tile: one 16-byte row piece
constexpr int kFpTile = kFpBlock * kFpCols;
constexpr int kFpChunkTiles = 8;  // whole tiles a block owns
constexpr long long kFpChunk = static_cast<long long>(kFpTile) * kFpChunkTiles;
// values of H = C >> 8 a chunk meets: kFpChunk / 256, one more when first_col
// is no multiple of 256
constexpr int kFpHi = static_cast<int>(kFpChunk / 256) + 1;
// table rows in front of the d powers: a^x, then b^x, x < 256
constexpr int kFpTabHead = 512;

// keys per kernel form: 1, 2, 4 or 8 (a smaller F is padded with dead keys)
constexpr int fp_pad(int F)
{
    return F <= 1 ? 1 : F <= 2 ? 2 : F <= 4 ? 4 : 8;
}
constexpr long long fp_chunks(long long words)
{
    return (words + kFpChunk - 1) / kFpChunk;
}
// d powers a call over `words` columns needs: the values of C2 it meets
constexpr long long fp_c2_count(long long first_col, long long words)
{
    return ((first_col + words - 1) >> 16) - (first_col >> 16) + 1;
}
// ... at most this many, whatever first_col
constexpr long long fp_c2_max(long long words)
{
    return (words >> 16) + 2;
}
// u32 words of the tables / of the work buffer (partials only for rows longer
// than one chunk)
constexpr long long fp_tab_words(long long c2s, int FP)
{
    return (kFpTabHead + c2s) * FP;
}
constexpr long long fp_work_words(long long rows, int FP, long long words)
{
    return fp_tab_words(fp_c2_max(words), FP) +
           (fp_chunks(words) > 1 ? rows * fp_chunks(words) * FP : 0);
}

// a b mod q for canonical a, b in [0, 65536]: 2^16 = -1, 2^32 = 1
QI_HD uint32_t fp_mulmod(uint32_t a, uint32_t b)
{
    const uint64_t p = static_cast<uint64_t>(a) * b;  // <= 2^32
    const int32_t v = static_cast<int32_t>(p & 0xffffu) -
                      static_cast<int32_t>((p >> 16) & 0xffffu) +
                      static_cast<int32_t>(p >> 32);  // [-65535, 65535]
    return static_cast<uint32_t>(v < 0 ? v + kQ : v);
}

QI_HD uint32_t fp_powmod(uint32_t a, uint32_t e)
{
    uint32_t r = 1;
    while (e) {
        if (e & 1u)
            r = fp_mulmod(r, a);
        a = fp_mulmod(a, a);
        e >>= 1;
    }
    return r;
}

// w(C) of key (a, b, d), canonical; 0 <= C < 2^32
QI_HD uint32_t fp_weight(const uint32_t* key, long long C)
{
    const uint32_t c0 = static_cast<uint32_t>(C & 255), c1 = static_cast<uint32_t>(C >> 8 & 255),
                   c2 = static_cast<uint32_t>(C >> 16);
    return fp_mulmod(fp_mulmod(fp_powmod(key[0], c0), fp_powmod(key[1], c1)),
                     fp_powmod(key[2], c2));
}

// row x of the tables for key (a, b, d): a^x, b^(x - 256), d^(c2base + x - 512)
QI_HD uint32_t fp_tab_entry(const uint32_t* key, long long x, long long c2base)
{
    if (x < 256)
        return fp_powmod(key[0], static_cast<uint32_t>(x));
    if (x < kFpTabHead)
        return fp_powmod(key[1], static_cast<uint32_t>(x - 256));
    return fp_powmod(key[2], static_cast<uint32_t>(c2base + x - kFpTabHead));
}

// the balanced hi weight b^C1 d^C2 of H = C >> 8 from the tables (tab: rows of
// FP keys); c2s: the d rows there are (a chunk's last H may lie past the row's
// end: no column uses it, 0)
QI_HD int32_t fp_hi_weight(const uint32_t* tab, int FP, int j, long long H, long long c2base,
                           long long c2s)
{
    const long long x = (H >> 8) - c2base;
    if (x >= c2s)
        return 0;
    return balanced(fp_mulmod(tab[(256 + (H & 255)) * FP + j], tab[(kFpTabHead + x) * FP + j]));
}

// A lane's place in its chunk.  vec: the lane holds 8 adjacent columns of a
// tile (first_col a multiple of 8, so that they share H), otherwise columns
// 256 apart.  lo = (first_col + chunk start) & 255, the same for every tile of
// the chunk.  a_row: the row of its a^C0 in the tables (vec: of its first
// column); hl: its H relative to the tile's first one
struct FpLane {
    int a_row, hl;
};
QI_HD FpLane fp_lane(bool vec, int lo, int tid)
{
    const int c = lo + (vec ? tid * kFpCols : tid);
    return FpLane{c & 255, c >> 8};
}
// index into the chunk's hi weights of element i of tile t
QI_HD int fp_hi_index(bool vec, int t, int hl, int i)
{
    return (kFpTile / 256) * t + hl + (vec ? 0 : i);
}

// x * c for |x|, |c| <= 32768 as one v_mul_i32_i24
QI_HD int32_t fp_mul24(int32_t x, int32_t c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __mul24(x, c);
#else
    QI_ASSERT24(x);
    QI_ASSERT24(c);
    return x * c;
#endif
}

// restored symbol -> balanced: a stored u16 or, marked, 65536 = -1
QI_HD int32_t fp_sym(uint32_t y16, bool marked)
{
    const int32_t y = static_cast<int32_t>(y16);
    return marked ? -1 : y > 32768 ? y - kQ : y;
}

// acc in [-32767, 98303], |y|, |c| <= 32768 -> the same range
QI_HD int32_t fp_step(int32_t acc, int32_t y, int32_t c)
{
#if defined(QI_HOST_CHECK) && !defined(__HIP_DEVICE_COMPILE__)
    assert(acc >= -32767 && acc <= 98303 && y >= -32768 && y <= 32768 && c >= -32768 &&
           c <= 32768);
#endif
    return fold(fp_mul24(y, c) + acc);
}

// a value in [-32767, 98303] as a balanced symbol again
QI_HD int32_t fp_rebalance(int32_t q)
{
    const int32_t v = fold(q);  // [-2, 65537]
    return v > 32768 ? v - kQ : v;
}

// sum_i y[i] ap[i] of a lane piece (ap: the balanced a^i), in [-32767, 98303]
QI_HD int32_t fp_piece(const int32_t (&y)[kFpCols], const int32_t* ap)
{
    int32_t q = 0;
    for (int i = 0; i < kFpCols; i++)
        q = fp_step(q, y[i], ap[i]);
    return q;
}

// [-32767, 98303] -> canonical
QI_HD uint32_t fp_canon(int32_t v)
{
    v = v < 0 ? v + kQ : v;
    v = v >= kQ ? v - kQ : v;
    return static_cast<uint32_t>(v);
}

// The plain reference: sym(c) in [0, 65536] is the restored symbol of column
// c < words; 64-bit arithmetic, one modulo per column.
template <class Sym>
inline uint32_t fingerprint_row(Sym sym, long long words, long long first_col,
                                const uint32_t* key)
{
    uint64_t sum = 0;
    for (long long c = 0; c < words; c++)
        sum = (sum + static_cast<uint64_t>(sym(c)) * fp_weight(key, first_col + c)) % 65537u;
    return static_cast<uint32_t>(sum);
}

}  // namespace qi
