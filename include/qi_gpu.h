/*
 * qi_gpu.h -- device-level C-ABI of the MI355X RS-FNT engine.
 *
 * This is the "thin C-ABI shim" below the drop-in quadiron_c.h boundary: plain
 * pointers and sizes, no C++ or torch types.  Device pointers are HIP device
 * memory; `stream` is a hipStream_t passed as void* (NULL = default stream).
 * All calls are asynchronous on `stream` unless stated.  Errors are negative
 * ints.
 *
 * Semantics follow QuadIron's RsFnt<uint32_t> with word_size 2
 * (src/fec_rs_fnt.h:51-270): GF(65537), n = ceil2(k+m), root r = 3^(65536/n).
 *   - NON-SYSTEMATIC encode: outputs 0..k+m-1 = evaluations of the data
 *     polynomial at r^i (the zero-padded n-point NTT, src/fft_2n.h:360-407).
 *   - SYSTEMATIC encode: outputs = the m parities (codeword rows k..k+m-1).
 *   - An output symbol equal to 65536 is stored as 0 and recorded as an
 *     out-of-range (OOR) mark (src/fec_rs_fnt.h:253-269).
 *
 * Device layout: a *stripe* is a set of fragment rows of `words` u16 symbols.
 * Row t of stripe s lives at base + s*stripe_stride + t*row_stride (strides in
 * u16 elements).  One call processes n_stripes stripes; every column of every
 * stripe is an independent codeword.
 *
 * Supported layouts: a unit stride between the words of a row, and any
 * positive row and stripe strides for which no two rows overlap; every tensor
 * of a call has its own.  Fragment-major is one example (each fragment holds
 * all its stripes back to back: stripe_stride = words, row_stride = n_stripes
 * * words), stripe-major [stripe][row][word] the other.  While every stripe's
 * row region, (rows - 1) * row_stride + words elements, stays inside a 31-bit
 * byte range (below 2^31 - 1 bytes), the kernels named under qi_plan_create
 * run.  Once one region of a call is larger -- rows GiB apart, as in a large
 * fragment-major batch -- the whole call runs the flat-addressing forms of
 * the dot2 and register-codelet kernels (k <= 256, 64-bit row offsets) or the
 * NTT engine (k > 256) instead of the matrix cores.  That path is tested bit
 * for bit against the reference, regions past 4 GiB included, but nobody has
 * timed it: expect it to be slower, by an unmeasured amount.  (qi_gpu_update
 * has one kernel for every layout: it addresses its rows flat, with 64-bit
 * row offsets, whatever the size of the regions.)
 *
 * OOR marks are kept in *buckets*: counts[s*slots + slot] (u32) and
 * entries[(s*slots + slot)*cap + e] (u32 word offset within the row).  Encode
 * zeroes nothing: callers clear counts (qi_gpu_oor_clear) before encoding.
 * Entries inside a bucket are unordered; encode keeps counting past cap (the
 * caller detects the overflow from the count and re-runs with a larger
 * cap); a decode reading such a bucket raises qi_gpu_take_error.
 */
#ifndef QI_GPU_H
#define QI_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qi_plan qi_plan;

/* Number of visible HIP devices (0 when none). */
int qi_gpu_device_count(void);

/* Create an RS-FNT plan (word_size 2 only).  Returns NULL on bad
 * parameters (k < 1, m < 1, k+m > 65536) or when no device is present.
 * Kernels by k:
 *   - k <= 256: the register codelets (non-systematic encode, k <= 32) and
 *     the matrix cores (every decode; the systematic encode; the
 *     non-systematic encode for 32 < k <= 256), dot2 kernels for column
 *     tails;
 *   - 256 < k <= 384: the matrix cores for batches whose width is a
 *     multiple of 1024 columns and whose rows are 8-byte aligned inside
 *     31-bit buffer ranges (the encode only while the generator stays small:
 *     k * n_outputs <= 2^21, 2^18 systematic); the NTT engine otherwise;
 *   - 384 < k <= 640, n - k > 64: the decode as above on the matrix cores
 *     (k x k contexts, two K chunks), and the systematic encode while its
 *     generator stays small (k * m <= 2^20); the non-systematic encode, and
 *     every other batch, on the NTT engine;
 *   - k > 384 otherwise: the NTT engine (column-batched NTT passes in LDS or
 *     HBM; the erasure decode when n - k <= 64). */
qi_plan* qi_plan_create(int k, int m, int systematic);
/* The same with flags: QI_PLAN_ENC_MATRIX / QI_PLAN_ENC_CODELETS force the
 * matrix-core or the register-codelet non-systematic encode for k <= 64
 * (both bit-exact; the default picks the faster: codelets up to k = 32).
 * NULL on unknown or contradictory flags. */
#define QI_PLAN_ENC_MATRIX 1
#define QI_PLAN_ENC_CODELETS 2
qi_plan* qi_plan_create_ex(int k, int m, int systematic, int flags);
void qi_plan_destroy(qi_plan* plan);
/* n (FFT length) and n_outputs (m if systematic, k+m otherwise) */
int qi_plan_n(const qi_plan* plan);
int qi_plan_n_outputs(const qi_plan* plan);

/* Zero n u32 OOR counters. */
int qi_gpu_oor_clear(uint32_t* d_counts, size_t n, void* stream);

/* Batch encode (device resident).  data: k rows per stripe.  out: n_outputs
 * rows per stripe.  OOR buckets: slots = n_outputs, slot = output index.
 * Pass d_oor_counts = NULL to skip OOR recording. */
int qi_gpu_encode(qi_plan* plan, const uint16_t* d_data,
                  long long data_stripe_stride, long long data_row_stride,
                  uint16_t* d_out, long long out_stripe_stride,
                  long long out_row_stride, long long words, int n_stripes,
                  uint32_t* d_oor_counts, uint32_t* d_oor_entries, int oor_cap,
                  void* stream);

/* Bytes of device workspace for n_stripes decode contexts of `words`
 * columns each -- enough for any width up to `words`.  A context is valid
 * only for the `words` it was built with (its format and per-stripe stride
 * follow the width: for 256 < k <= 384 (and the non-systematic 384 < k <=
 * 640 codes with n - k > 64), matrix contexts at multiples of 1024 columns,
 * the NTT engine's otherwise). */
size_t qi_gpu_decode_ctx_bytes(const qi_plan* plan, int n_stripes,
                               long long words);

/* Build per-stripe decode contexts from the received fragment ids:
 * d_ids[s*k + i] (u16, distinct, < k+m; ascending as the reference passes
 * them, any order accepted) -- the k fragments the decoder uses
 * (FecCode::decode_blocks_vertical picks the first k present,
 * src/fec_base.h:1199-1236; a systematic context lists them data fragments
 * first, so that the matrix kernel reads each of its two source regions in
 * one run) -- and route the OOR marks of those fragments
 * (buckets as produced by qi_gpu_encode) into per-tile tables.  With NULL
 * counts the context is built from the ids alone (init_context_dec,
 * src/fec_base.h:758-793: before the fragments' data and marks exist, e.g.
 * on another stream while they are produced); a decode given buckets then
 * reads the marks from them directly (slightly slower per tile than routed
 * tables).  Built on the device, asynchronously on `stream`, for every k:
 * matrix contexts (the interpolation matrix, up to ~780 KB per stripe at
 * k = 256) for k <= 256, and for 256 < k <= 640 at widths that are a
 * multiple of 1024 columns (then followed by the NTT engine's context, used
 * when the decode's rows are not addressable by the matrix cores); the NTT
 * decode's per-pattern constants (src/fec_context.h:232-274, whose decode
 * reads the OOR buckets directly) otherwise; for 256 < k <= 640 the NTT
 * engine's half is built by the first decode that needs it.  h_ids is
 * unused (kept for ABI stability; may be NULL). */
int qi_gpu_decode_ctx(qi_plan* plan, const uint16_t* d_ids,
                      const uint16_t* h_ids, int n_stripes,
                      const uint32_t* d_oor_counts,
                      const uint32_t* d_oor_entries, int oor_cap,
                      long long words, void* d_ctx, void* stream);

/* Batch decode.  Received fragment id f of stripe s is read from
 *   f <  k (systematic data rows):  d_data + s*dss + f*drs
 *   otherwise (coded row / parity): d_coded + s*css + slot*crs
 * with slot = f - k (systematic) or f (non-systematic).
 * OOR buckets of the coded rows are indexed by the same slot (slots =
 * n_outputs); pass NULL counts when there are none.  Output: k data rows.
 * NULL counts mean "no marks" whatever the context was built with: the
 * decode is then the interpolation of the stored symbols (a result of 65536
 * is stored as 0), on every kernel path, and marks routed into the context
 * by qi_gpu_decode_ctx are NOT restored.  Rows that carry marks need their
 * buckets at decode time; giving them to the context builder as well only
 * makes that decode faster.  (Only the matrix contexts hold routed marks; an
 * NTT context holds none, so "restore what the context holds" could not be
 * kept for every k, and neither could a check.)  The same holds for
 * qi_gpu_decode_packed, qi_gpu_repair and qi_gpu_verify and their contexts.
 * The context is not const in effect: a decode whose rows the matrix cores
 * cannot address fills the context's lazily built sections (the dot2
 * kernel's packed rows for k <= 256, the NTT engine's half for 256 < k <=
 * 640) the first time, on `stream`, and records that in the context.  Every
 * word such a fill writes gets the value it already holds when the section
 * was filled before, so a context may serve any number of decodes, on one
 * stream or on several at once (two decodes may then both fill it), once
 * the qi_gpu_decode_ctx call that built it is ordered before them. */
int qi_gpu_decode(qi_plan* plan, const void* d_ctx, const uint16_t* d_ids,
                  const uint16_t* d_data, long long dss, long long drs,
                  const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_oor_counts, const uint32_t* d_oor_entries,
                  int oor_cap, uint16_t* d_out, long long out_stripe_stride,
                  long long out_row_stride, long long words, int n_stripes,
                  void* stream);

/* Packed-row decode (the staging layout of a host pipeline, where the k
 * received fragments of a stripe are copied back to back): row i of stripe s
 * is read from d_recv + s*rss + i*rrs and holds fragment d_ids[s*k + i].  The
 * OOR buckets are indexed by that position i (slots = k).  Contexts for this
 * layout come from qi_gpu_decode_ctx_packed (same size as
 * qi_gpu_decode_ctx_bytes). */
int qi_gpu_decode_ctx_packed(qi_plan* plan, const uint16_t* d_ids,
                             const uint16_t* h_ids, int n_stripes,
                             const uint32_t* d_oor_counts,
                             const uint32_t* d_oor_entries, int oor_cap,
                             long long words, void* d_ctx, void* stream);
int qi_gpu_decode_packed(qi_plan* plan, const void* d_ctx,
                         const uint16_t* d_recv, long long rss, long long rrs,
                         const uint32_t* d_oor_counts,
                         const uint32_t* d_oor_entries, int oor_cap,
                         uint16_t* d_out, long long out_stripe_stride,
                         long long out_row_stride, long long words,
                         int n_stripes, void* stream);

/* Non-zero if an OOR bucket read by a decode context or a decode held more
 * marks than its capacity (oor_cap), i.e. some out-of-range symbols could
 * not be restored and the affected stripes are wrong (bit 1), or if a decode
 * context was built from ids that were not distinct or not below n (bit 2;
 * every context builder checks: a repeated id makes A'(x_i) = 0, and the
 * erasure decode of k > 384, n - k <= 64, derives its erased set from the
 * ids).  Sticky per plan; reset by
 * reading.  Synchronous.  Tiles with many marks need no capacity of their
 * own: they are decoded by a slower path, never refused. */
int qi_gpu_take_error(qi_plan* plan);

/* Names of the kernels an encode and a decode of `words` columns launch on
 * this plan (rows at 8-byte aligned offsets), as
 * "encode=<kernels>; decode=<kernels>" -- diagnostics for bench lines and
 * profiles.  The string is per calling thread, valid until its next call. */
const char* qi_gpu_kernels(const qi_plan* plan, long long words);

/* ---- Fused fragment repair: rebuild lost fragments straight from k
 * received ones, in one pass (a decode followed by an encode writes the k
 * data rows to memory and reads them back to compute every output).
 * Fragment f of a column is P(r^f) in both code types, so target t is the
 * Lagrange evaluation out_t = sum_i L_i(r^t) in[ids[i]]: one R x k matrix
 * per stripe (R = n_targets), applied by the kernels of the decode.
 *
 * Ids and targets are fragment ids in the decode's id space (systematic:
 * f < k is data row f, otherwise parity f - k; non-systematic: coded row f),
 * and the received rows and their OOR buckets are addressed exactly as
 * qi_gpu_decode addresses them.  1 <= n_targets <= min(64, m)
 * (QI_REPAIR_MAX_TARGETS), the same count for every stripe of a call; the
 * targets themselves may differ per stripe.  Output row j of a stripe is target j
 * (d_out + s*oss + j*ors), and its marks go to bucket slot j (slots =
 * n_targets): a rebuilt coded symbol equal to 65536 is stored as 0 and
 * recorded, as by qi_gpu_encode; rebuilt data rows never hold one.  Clear
 * d_out_counts first (qi_gpu_oor_clear); NULL skips the recording.
 *
 * Supported for plans with k <= 256, at any width and row alignment (the
 * matrix cores take the whole 1024-column tiles of addressable rows, the
 * dot2 kernel the tail and everything else).  For k > 256
 * qi_gpu_repair_ctx_bytes returns 0 and the two calls return
 * QI_ERR_UNSUPPORTED; n_targets out of range returns -1 (nothing is
 * launched).  A context is valid for the `words` and n_targets it was built
 * with.  Bad ids raise bit 2 of qi_gpu_take_error and leave the stripe's
 * context unusable: received ids repeated or not below n, a target not
 * below k + m, a repeated target, or a target that is also a received id.
 * An input bucket over its capacity raises bit 1, as for a decode.  With
 * NULL counts at context time the marks are read from the buckets given to
 * qi_gpu_repair. */
#define QI_REPAIR_MAX_TARGETS 64
#define QI_ERR_UNSUPPORTED (-5)
size_t qi_gpu_repair_ctx_bytes(const qi_plan* plan, int n_targets, int n_stripes,
                               long long words);
int qi_gpu_repair_ctx(qi_plan* plan, const uint16_t* d_ids /*[S][k]*/,
                      const uint16_t* d_targets /*[S][R]*/, int n_targets,
                      int n_stripes, const uint32_t* d_oor_counts,
                      const uint32_t* d_oor_entries, int oor_cap,
                      long long words, void* d_ctx, void* stream);
int qi_gpu_repair(qi_plan* plan, const void* d_ctx, int n_targets,
                  const uint16_t* d_data, long long dss, long long drs,
                  const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_in_counts, const uint32_t* d_in_entries,
                  int in_cap, uint16_t* d_out, long long oss, long long ors,
                  uint32_t* d_out_counts, uint32_t* d_out_entries, int out_cap,
                  long long words, int n_stripes, void* stream);
/* Names of the kernels a repair of n_targets fragments over `words` columns
 * launches (rows at 8-byte aligned offsets), as "repair=<kernels>"; "" when
 * unsupported.  Per calling thread, valid until its next call. */
const char* qi_gpu_repair_kernels(const qi_plan* plan, int n_targets, long long words);

/* ---- Fused fragment verify (scrubbing): check stored fragments against
 * each other on the device, in one pass and without writing a row.  Take k
 * *basis* fragments and n_checks *check* fragments of a stripe, all present
 * and distinct.  Each check fragment j is recomputed from the basis rows
 * (their OOR marks restored) exactly as qi_gpu_repair would rebuild it, and
 * compared with the stored row j and that row's OOR bucket where it is
 * computed: a repair into scratch rows followed by a compare writes n_checks
 * rows and reads 2 n_checks rows that this call never touches.
 *
 * The context IS a repair context with targets = the check ids: build it
 * with qi_gpu_repair_ctx(plan, d_basis_ids, d_checks, n_checks, ...), sized
 * by qi_gpu_repair_ctx_bytes, with the same limits (k <= 256, 1 <= n_checks
 * <= min(64, m), ids below k + m; a check id that is also a basis id raises
 * bit 2 of qi_gpu_take_error).  d_checks is the [S][n_checks] u16 array given
 * to that call.  Basis rows AND check rows are addressed by fragment id as
 * qi_gpu_decode addresses received rows (d_data / d_coded), their buckets by
 * the same slot.
 *
 * At column c the canonical recomputed value is v in [0, 65536]:
 *   value mismatch: (v & 0xffff) != stored[c]
 *   mark mismatch:  (v == 65536) != (c is in the stored row's bucket); a
 *                   systematic data row has no bucket, so any v == 65536
 *                   there is one (as is every one when d_oor_counts is NULL).
 * Per (stripe s, check j), at index s * n_checks + j, the call writes
 *   d_value_mismatch: the number of value mismatches,
 *   d_mark_mismatch:  the number of mark mismatches,
 *   d_first:          the smallest column with either kind, or 0xFFFFFFFF.
 * It initialises all three itself.  A corrupt *basis* fragment shows up as a
 * mismatch in every check row at that column (each recomputed symbol depends
 * on every basis symbol of its column); which fragment of a stripe is the
 * corrupt one, and what it should hold, is qi_gpu_locate's answer (below).
 *
 * d_work: qi_gpu_verify_work_bytes bytes of scratch for the recomputed rows'
 * 65536 positions, work_cap per (stripe, check) -- about words / 65537 are
 * expected; it holds no rows (its size does not depend on the width).  More
 * recomputed 65536 values than work_cap, or a stored bucket over oor_cap,
 * raise bit 1 of qi_gpu_take_error (the mark counts are then lower bounds).
 * Returns QI_ERR_UNSUPPORTED for k > 256 (qi_gpu_verify_work_bytes: 0), -1
 * for n_checks out of range (nothing is launched). */
size_t qi_gpu_verify_work_bytes(const qi_plan* plan, int n_checks, int n_stripes,
                                int work_cap);
int qi_gpu_verify(qi_plan* plan, const void* d_ctx, int n_checks,
                  const uint16_t* d_checks /*[S][R], as given to repair_ctx*/,
                  const uint16_t* d_data, long long dss, long long drs,
                  const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_oor_counts, const uint32_t* d_oor_entries,
                  int oor_cap, void* d_work, int work_cap,
                  uint32_t* d_value_mismatch, uint32_t* d_mark_mismatch,
                  uint32_t* d_first, long long words, int n_stripes, void* stream);
/* Names of the kernels such a check launches (rows at 8-byte aligned
 * offsets), as "verify=<kernels>": the repair's, in their _verify forms, and
 * the bucket comparison; "" when unsupported.  Per calling thread, valid
 * until its next call. */
const char* qi_gpu_verify_kernels(const qi_plan* plan, int n_checks, long long words);

/* ---- Delta update: some data rows of a stripe change and the coded rows
 * must follow.  Both code types are linear, so when data row i goes from old
 * to new, coded slot f moves by a constant times the difference,
 *   out_f = coded_f + c(f, i) (new_i - old_i)   (mod 65537)
 *   c(f, i) = r^(f i)      non-systematic (fragment f = sum_t d_t r^(f t))
 *   c(f, i) = l_i(r^(k+f)) systematic (l_i: the Lagrange basis over r^0 ..
 *                          r^(k-1); slot f is parity f)
 * and an update of U rows reads 2 U + R rows and writes R: no other data row
 * of the stripe is needed, and the cost does not depend on k.  (A full
 * qi_gpu_encode reads k rows and writes n_outputs: by bytes the update wins
 * when 2 U + 2 R < k + n_outputs for R = n_outputs.  At k = 16, m = 48 it
 * moves MORE bytes than the encode -- it is then still the only way for a
 * node that does not hold the other 15 rows.)
 *
 * Supported on every plan qi_plan_create accepts (any k, both code types),
 * for 1 <= n_rows <= min(QI_UPDATE_MAX_ROWS, k) changed rows and 1 <= n_slots
 * <= n_outputs coded rows, the same counts for every stripe of a call; the
 * ids and slots themselves may differ per stripe.  A count out of range
 * returns -1 (qi_gpu_update_ctx_bytes: 0) and launches nothing.
 *
 * Slots are the encode's output indices (parity j of a systematic plan, coded
 * row j otherwise).  The coded rows, the output rows and both bucket sets are
 * addressed by slot (slots = n_outputs), exactly as qi_gpu_encode wrote them;
 * rows and buckets of slots not listed are not touched.  d_slots = NULL means
 * all of them, slot j = j, and needs n_slots = n_outputs.  Row u of d_old /
 * d_new (n_rows rows per stripe) holds the old / new contents of data row
 * d_ids[s * n_rows + u].
 *
 * In place: d_out == d_coded with equal strides is allowed and is the
 * expected use (every column is read before it is written, by the lane that
 * writes it); any other overlap between the tensors of a call is undefined.
 * The two bucket sets must be distinct.  Clear the out counts of the listed
 * slots first (qi_gpu_oor_clear); NULL out counts skip the recording (65536
 * is still stored as 0).  After an in-place update the out buckets are the
 * rows' marks: swap the two bucket sets for the next call.
 *
 * Marks: an input symbol listed in its slot's in-bucket is 65536 (stored as
 * 0), as qi_gpu_encode records it; an updated symbol equal to 65536 is stored
 * as 0 and recorded, the count going on past out_cap as in the encode.  Data
 * rows carry no marks.  No mark is refused: a bucket with count <= in_cap is
 * restored in full however dense; a count above in_cap raises bit 1 of
 * qi_gpu_take_error.  NULL in counts: no marks.
 *
 * Bad ids -- an id not below k, a repeated id, a slot not below n_outputs, a
 * repeated slot -- raise bit 2 of qi_gpu_take_error when the context is
 * built; the update of such a stripe is then unspecified, but stays inside
 * the caller's rows.
 *
 * The context holds, per stripe, the n_slots x n_rows coefficients, the slots
 * and the ids (it does not depend on the width).  For a systematic plan the
 * first qi_gpu_update_ctx builds two per-plan tables on the host (O(k + m)
 * field operations, under a lock) and uploads them with a blocking copy;
 * everything else is asynchronous on `stream`.  Any positive strides with a
 * unit inner stride, per tensor, at any alignment (rows and strides that are
 * all multiples of 16 bytes move as 16-byte pieces per lane). */
#define QI_UPDATE_MAX_ROWS 8
size_t qi_gpu_update_ctx_bytes(const qi_plan* plan, int n_rows, int n_slots, int n_stripes);
int qi_gpu_update_ctx(qi_plan* plan, const uint16_t* d_ids /*[S][U] data row ids, < k*/,
                      const uint16_t* d_slots /*[S][R] coded-row slots, or NULL*/,
                      int n_rows, int n_slots, int n_stripes, void* d_ctx, void* stream);
int qi_gpu_update(qi_plan* plan, const void* d_ctx, int n_rows, int n_slots,
                  const uint16_t* d_old, long long old_ss, long long old_rs,
                  const uint16_t* d_new, long long new_ss, long long new_rs,
                  const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_in_counts, const uint32_t* d_in_entries, int in_cap,
                  uint16_t* d_out, long long oss, long long ors,
                  uint32_t* d_out_counts, uint32_t* d_out_entries, int out_cap,
                  long long words, int n_stripes, void* stream);
/* Names of the kernels such an update launches (rows and strides at
 * multiples of 16 bytes), as "update=<context kernel> + <kernel>"; "" for
 * counts out of range.  Per calling thread, valid until its next call. */
const char* qi_gpu_update_kernels(const qi_plan* plan, int n_rows, int n_slots, long long words);

/* ---- Fragment locate: qi_gpu_verify says that the fragments of a stripe
 * disagree; this call says which one is wrong and what it should hold, in one
 * pass over the rows and without writing one.  Fragment f of a column is
 * P(r^f), deg P < k, in both code types.  List N = k + n_checks distinct
 * present fragments f_0 .. f_(N-1) of a stripe (ids in the decode's id space,
 * as for qi_gpu_repair), let x_i = r^(f_i) and w_i = prod_{l != i} (x_i - x_l).
 * For the received column y (y_i the restored symbol: 65536 where the column
 * is in the row's OOR bucket, the stored u16 otherwise) the syndromes are
 *   S_j = sum_i y_i x_i^j / w_i   (mod 65537),  j < n_checks = R,
 * all 0 for a codeword.  One fragment p off by e != 0 gives S_j = (e / w_p)
 * x_p^j, and a column is
 *   clean      every S_j = 0;
 *   located    at position p of the list: S_0 != 0, S_1 / S_0 = x_p, S_j = x_p
 *              S_(j-1) for 2 <= j < R, and the corrected symbol v = y_p - S_0
 *              w_p can be stored: v in [0, 65536], and v != 65536 when p is a
 *              systematic data row (data rows carry no marks);
 *   unlocated  anything else.
 * The code over the listed points has minimum distance R + 1: a column with
 * 2 .. R - 1 bad fragments is always unlocated, never attributed to a wrong
 * fragment.  R = 2 has no guard equation: there a column with two bad
 * fragments MAY be attributed to a third one, with a wrong correction.  Use
 * R >= 3 where more than one fragment of a column can be bad.
 *
 * Supported for k <= 256 (as qi_gpu_verify) and 2 <= n_checks <= min(
 * QI_LOCATE_MAX_CHECKS, m): a larger k returns QI_ERR_UNSUPPORTED (the bytes
 * call 0, the kernels call ""), an n_checks out of range -1 (0, ""), and
 * nothing is launched.
 *
 * Rows and buckets are addressed by fragment id exactly as qi_gpu_decode
 * addresses received rows (d_data for f < k of a systematic plan, d_coded by
 * slot otherwise; d_data may be NULL for a non-systematic plan), with any
 * positive strides and a unit inner stride at any alignment (rows and strides
 * that are all multiples of 16 bytes move as 16-byte pieces per lane).
 * d_stripes = NULL: list position s is stripe s.  Otherwise list position s
 * takes the rows and buckets of stripe d_stripes[s], so that only the stripes
 * a verify flagged need be listed; the context, the ids and all four outputs
 * are indexed by list position.
 *
 * Outputs, all initialised by the call: d_located[s * N + i] counts the
 * columns attributed to listed fragment i, d_unlocated[s] the unlocated
 * columns.  Each located column appends {column, position i, corrected
 * symbol v in [0, 65536]} to the stripe's fix list d_fixes[s][fix_cap][3], in
 * no particular order; d_fix_counts[s] goes on past fix_cap and entries past
 * it are dropped (the OOR bucket protocol).  fix_cap = 0: counts only (d_fixes
 * may be NULL).  No row and no bucket is written.
 *
 * Ids repeated or not below k + m raise bit 2 of qi_gpu_take_error when the
 * context is built; the result of such a stripe is unspecified, but the call
 * stays inside the caller's buffers.  A bucket over oor_cap raises bit 1.
 * NULL d_oor_counts: no marks.  A bucket with count <= oor_cap is restored in
 * full however dense.  The context holds, per stripe, the ids, x_i, w_i and
 * the R x N coefficients (it does not depend on the width). */
#define QI_LOCATE_MAX_CHECKS 8
size_t qi_gpu_locate_ctx_bytes(const qi_plan* plan, int n_checks, int n_stripes);
int qi_gpu_locate_ctx(qi_plan* plan, const uint16_t* d_ids /*[S][k+R]*/, int n_checks,
                      int n_stripes, void* d_ctx, void* stream);
int qi_gpu_locate(qi_plan* plan, const void* d_ctx, int n_checks,
                  const uint32_t* d_stripes /*[S] or NULL*/,
                  const uint16_t* d_data, long long dss, long long drs,
                  const uint16_t* d_coded, long long css, long long crs,
                  const uint32_t* d_oor_counts, const uint32_t* d_oor_entries, int oor_cap,
                  uint32_t* d_located /*[S][k+R]*/, uint32_t* d_unlocated /*[S]*/,
                  uint32_t* d_fix_counts /*[S]*/, uint32_t* d_fixes /*[S][fix_cap][3]*/,
                  int fix_cap, long long words, int n_stripes, void* stream);
/* Names of the kernels a locate launches (rows and strides at multiples of
 * 16 bytes), as "locate=<context kernel> + <kernel>"; "" when unsupported.
 * Per calling thread, valid until its next call. */
const char* qi_gpu_locate_kernels(const qi_plan* plan, int n_checks, long long words);

/* ---- Multi-fragment locate: qi_gpu_locate solves with two of its R
 * syndromes and keeps the others as guards, so a column with two bad
 * fragments is always unlocated.  This call decodes up to max_errors = t bad
 * fragments per column, 1 <= t <= floor(R / 2) <= QI_LOCATE_MAX_ERRORS, from
 * the same context (qi_gpu_locate_ctx) and the same single pass over the rows.
 * With the notation above a column is
 *   clean      every S_j = 0;
 *   located    with nu fragments, 1 <= nu <= t: there are distinct list
 *              positions p_1 .. p_nu and non-zero E_1 .. E_nu with S_j = sum_a
 *              E_a x_(p_a)^j for ALL j < R, and every corrected symbol v_a =
 *              y_(p_a) - E_a w_(p_a) can be stored (v_a in [0, 65536], and not
 *              65536 on a systematic data row).  As 2 nu <= R such a set is
 *              unique when it exists;
 *   unlocated  anything else.  One v_a that cannot be stored makes the whole
 *              column unlocated: no partial fix is emitted.
 * With b bad listed fragments in a column:
 *   b <= t          located exactly, each fix is the original symbol;
 *   t < b <= R - t  always unlocated, never attributed;
 *   b > R - t       may be miscorrected.
 * With t = 1 every output equals qi_gpu_locate's on the same input (R = 2
 * included).  A t below floor(R / 2) buys a wider guard zone.
 *
 * Rows, buckets, d_stripes, limits and errors are exactly qi_gpu_locate's:
 * k > 256 returns QI_ERR_UNSUPPORTED (the kernels call ""); n_checks outside
 * 2 .. min(QI_LOCATE_MAX_CHECKS, m) or max_errors outside 1 .. n_checks / 2
 * returns -1 and launches nothing; a bucket over oor_cap raises bit 1; bad
 * ids are the context's business (bit 2).
 *
 * Outputs, all initialised by the call: a located column adds 1 to each of
 * its nu d_located[s * N + p_a] and 1 to d_weights[s * QI_LOCATE_MAX_ERRORS +
 * nu - 1], an unlocated one 1 to d_unlocated[s].  A located column reserves
 * its nu fix entries {column, position, v} with one addition of nu to
 * d_fix_counts[s], so they are adjacent in d_fixes[s][fix_cap][3]; entries at
 * or past fix_cap are dropped one by one and the count goes on (the OOR bucket
 * protocol).  fix_cap = 0: counts only (d_fixes may be NULL).  No row and no
 * bucket is written. */
#define QI_LOCATE_MAX_ERRORS 4
int qi_gpu_locate_multi(qi_plan* plan, const void* d_ctx, int n_checks, int max_errors,
                        const uint32_t* d_stripes /*[S] or NULL*/,
                        const uint16_t* d_data, long long dss, long long drs,
                        const uint16_t* d_coded, long long css, long long crs,
                        const uint32_t* d_oor_counts, const uint32_t* d_oor_entries,
                        int oor_cap, uint32_t* d_located /*[S][k+R]*/,
                        uint32_t* d_unlocated /*[S]*/,
                        uint32_t* d_weights /*[S][QI_LOCATE_MAX_ERRORS]*/,
                        uint32_t* d_fix_counts /*[S]*/, uint32_t* d_fixes /*[S][fix_cap][3]*/,
                        int fix_cap, long long words, int n_stripes, void* stream);
/* "locate_multi=<context kernel> + <kernel>" (rows and strides at multiples
 * of 16 bytes); "" when unsupported or max_errors is out of range.  Per
 * calling thread, valid until its next call. */
const char* qi_gpu_locate_multi_kernels(const qi_plan* plan, int n_checks, int max_errors,
                                        long long words);

/* ---- Fragment fingerprints: keyed digests of the rows that are homomorphic
 * under the code, so that a stripe can be scrubbed from a few symbols per
 * fragment instead of the fragments themselves.
 *
 * Symbols.  y_c in [0, 65536] is the restored symbol of a row: 65536 where
 * column c is listed in the row's OOR bucket, the stored u16 otherwise (a
 * systematic data row has no bucket) -- exactly how qi_gpu_locate reads rows.
 *
 * Keys and weights.  A key is a triple (a, b, d), each in [1, 65536]; F keys
 * per call, 1 <= F <= QI_FINGERPRINT_MAX_KEYS, passed from the host as
 * h_keys[F][3].  They travel as kernel arguments: no upload, no blocking copy.
 * For the absolute column C = first_col + c take the base-256 digits C0 = C &
 * 255, C1 = (C >> 8) & 255, C2 = C >> 16.  Then
 *   w_j(C) = a_j^C0 b_j^C1 d_j^C2                      (mod 65537)
 *   fp_j   = sum_{c < words} y_c w_j(first_col + c)    (mod 65537),
 * canonical in [0, 65536].  Weights are never 0: one changed symbol changes
 * every fp_j.  Every column of a stripe is a codeword P_c(r^f), so the
 * fingerprints of a stripe's fragments are a codeword again, h_f = P_h(r^f)
 * with P_h = sum_c w(c) P_c, in both code types: qi_gpu_verify, qi_gpu_locate
 * and qi_gpu_locate_multi run unchanged on a stripe of F columns whose rows
 * are the fragments' fingerprints (65536 as a mark), and the encode of the k
 * data rows' fingerprints gives the fingerprints of all n outputs.
 *
 * Collision bound.  Three variables because the field has 65537 elements and
 * rows are longer: a single power z^C would alias columns 65536 apart.  With
 * base-256 digits two different rows of total width W collide under one
 * uniformly random key with probability at most (510 + floor((W - 1) / 65536))
 * / 65536 (Schwartz-Zippel: the difference is a non-zero polynomial of total
 * degree at most 255 + 255 + floor((W - 1) / 65536)), under 0.8 % per key at
 * 32768 words; keys are independent.  This is an error-detection digest, not
 * a cryptographic one: keys must be random and kept from whoever may tamper
 * with the data.
 *
 * first_col (chunking).  Bucket columns and `words` are relative to the row
 * pointers given; only the weights see first_col, so the fingerprints of
 * adjacent column slices of a row add modulo 65537 to the fingerprint of the
 * whole row.  first_col >= 0 and first_col + words <= 2^32.
 *
 * The call.  Any plan qi_plan_create accepts, at any k, both code types; no
 * context.  d_ids[s * N + i] are fragment ids in the decode's id space, 1 <=
 * N <= k + m, and an id may repeat within a stripe.  Rows and buckets are
 * addressed exactly as qi_gpu_decode addresses received rows (d_data for f <
 * k of a systematic plan, d_coded by slot otherwise), with any positive
 * strides and a unit inner stride at any 2-byte alignment (rows and strides
 * that are all multiples of 16 bytes, with first_col a multiple of 8, move as
 * 16-byte pieces per lane).  d_data may be NULL for a non-systematic plan; a
 * systematic plan may pass NULL for the region it holds no row of, not both.
 * NULL d_oor_counts: no marks.  A bucket with count <= oor_cap is restored in
 * full however dense; a count above oor_cap raises bit 1 of
 * qi_gpu_take_error, and bucket entries >= words are no columns.  An id not
 * below k + m, or one in a region passed as NULL, raises bit 2: its F outputs
 * are 0xFFFFFFFF and nothing is read for it.
 * Arguments out of range -- NULL plan; n_keys, n_rows, words (1 .. 2^32) or
 * first_col out of range; a key component outside 1 .. 65536 -- return -1
 * (the kernels call "", the bytes call 0) and launch nothing.  For valid
 * arguments the bytes call returns at least 4.
 * d_fp[s][i][j] is written in full by the call (no clearing needed).  Results
 * are exact and deterministic: the same bits whatever the grid.  d_work holds
 * the call's power tables and, for rows longer than one block's share, the
 * blocks' partial sums: one call at a time per work buffer.  Everything runs
 * on `stream`. */
#define QI_FINGERPRINT_MAX_KEYS 8
size_t qi_gpu_fingerprint_work_bytes(const qi_plan* plan, int n_rows, int n_keys,
                                     int n_stripes, long long words);
int qi_gpu_fingerprint(qi_plan* plan, const uint16_t* d_ids /*[S][N] fragment ids*/, int n_rows,
                       const uint32_t* h_keys /*[F][3], host*/, int n_keys, long long first_col,
                       const uint16_t* d_data, long long dss, long long drs,
                       const uint16_t* d_coded, long long css, long long crs,
                       const uint32_t* d_oor_counts, const uint32_t* d_oor_entries, int oor_cap,
                       void* d_work, uint32_t* d_fp /*[S][N][F]*/,
                       long long words, int n_stripes, void* stream);
/* "fingerprint=<table kernel> + <kernel>[ + <finish kernel>]" (rows and
 * strides at multiples of 16 bytes, first_col 0); "" for arguments out of
 * range.  Per calling thread, valid until its next call. */
const char* qi_gpu_fingerprint_kernels(const qi_plan* plan, int n_rows, int n_keys,
                                       long long words);

/* ---- Partial repair: the share of a repair that one holder of some of the k
 * helper fragments can form.  qi_gpu_repair rebuilds a fragment as a sum over
 * all k helpers, which must all be in one device's memory, and is limited to
 * k <= 256.  The sum is linear: a node can form it over just the rows it
 * holds, and the partial sums of different nodes add modulo 65537
 * (partial-parallel repair: a helper ships n_targets partial rows instead of
 * its held rows, and aggregators add as they forward).  With n_held = k and
 * no accumulator it is a one-pass streaming repair for any k.
 *
 * For one stripe:
 *   ids[0 .. k)     the k helper fragments of the repair: distinct, below
 *                   k + m, in the decode's id space;
 *   targets[0 .. R) the fragments to rebuild: distinct, below k + m, none of
 *                   them in ids;
 *   held[0 .. H)    *positions* into ids (each < k, distinct): the helpers
 *                   whose rows this call has.
 * With x_l = r^ids[l], y_t = r^targets[t] and A(x) = prod_{l<k} (x - x_l) the
 * coefficient is
 *   c(t, i) = A(y_t) / ((y_t - x_i) A'(x_i)),
 * entry (t, i) of the matrix of qi_gpu_repair.  The call computes, per column,
 *   out_t = canon(acc_t + sum_{h<H} c(t, held[h]) y_h),   in [0, 65536],
 * where y_h is the restored symbol of held row h -- 65536 where the column is
 * in that row's bucket; a systematic data row (id < k) carries no marks and
 * its bucket is not read -- and acc_t the restored symbol of accumulator row t
 * (its bucket is always read), or 0 when d_acc is NULL.  A result of 65536 is
 * stored as 0 and recorded in the out bucket of slot t by the encode's bucket
 * protocol (the count goes on past out_cap).  This holds for data-row targets
 * too: only the *complete* sum of a valid stripe is guaranteed storable there,
 * a partial is not.  Summed over any partition of the k positions, in any
 * order, the result is bit for bit what qi_gpu_repair writes, rows and marks
 * both.
 *
 * Supported on every plan qi_plan_create accepts (any k, both code types), for
 * 1 <= n_held <= k and 1 <= n_targets <= min(QI_PARTIAL_MAX_TARGETS, m), the
 * same counts for every stripe of a call; ids, held and targets may differ per
 * stripe.  Counts out of range return -1 (qi_gpu_partial_ctx_bytes: 0,
 * qi_gpu_partial_kernels: "") and launch nothing.
 *
 * Rows are positional, as in qi_gpu_decode_packed: row h of stripe s is d_rows
 * + s * rss + h * rrs, its bucket slot h of n_held; a node passes only what it
 * holds.  Accumulator and output row t are slot t of n_targets.  Any positive
 * strides with a unit inner stride, at any 2-byte alignment; rows and strides
 * that are all multiples of 16 bytes move as 16-byte pieces per lane.
 *
 * In place: d_out == d_acc with equal strides is allowed and is the expected
 * use (chain aggregation: every column is read before it is written, by the
 * lane that writes it); any other overlap is undefined.  The acc and out
 * bucket sets must be distinct.  Clear the out counts first
 * (qi_gpu_oor_clear); NULL out counts skip the recording.
 *
 * Errors: an id not below k + m, a repeated id, a position not below k or
 * repeated, a target not below k + m, a repeated target, or a target that is
 * also a helper raise bit 2 of qi_gpu_take_error when the context is built;
 * the offending coefficients enter as 0, and the call stays inside the
 * caller's rows.  An in or acc bucket over its capacity raises bit 1; a bucket
 * within its capacity is restored in full however dense.
 *
 * The context holds, per stripe, the n_targets x n_held balanced coefficients,
 * the targets and the held rows' ids; it does not depend on the width.  It
 * costs O((n_held + n_targets) k) field operations per stripe (only the held
 * rows' Lagrange weights are needed), where the k x R matrix of
 * qi_gpu_repair_ctx costs O(k^2).  Everything is asynchronous on `stream`: no
 * host tables, no blocking copy. */
#define QI_PARTIAL_MAX_TARGETS 8
size_t qi_gpu_partial_ctx_bytes(const qi_plan* plan, int n_held, int n_targets, int n_stripes);
int qi_gpu_partial_ctx(qi_plan* plan, const uint16_t* d_ids /*[S][k]*/,
                       const uint16_t* d_held /*[S][H] positions into ids*/,
                       const uint16_t* d_targets /*[S][R]*/, int n_held, int n_targets,
                       int n_stripes, void* d_ctx, void* stream);
int qi_gpu_partial(qi_plan* plan, const void* d_ctx, int n_held, int n_targets,
                   const uint16_t* d_rows, long long rss, long long rrs,
                   const uint32_t* d_in_counts, const uint32_t* d_in_entries, int in_cap,
                   const uint16_t* d_acc, long long ass, long long ars,
                   const uint32_t* d_acc_counts, const uint32_t* d_acc_entries, int acc_cap,
                   uint16_t* d_out, long long oss, long long ors,
                   uint32_t* d_out_counts, uint32_t* d_out_entries, int out_cap,
                   long long words, int n_stripes, void* stream);
/* Names of the kernels such a partial repair launches (rows and strides at
 * multiples of 16 bytes), as "partial=<context kernel> + <kernel>"; "" for
 * counts out of range.  Per calling thread, valid until its next call. */
const char* qi_gpu_partial_kernels(const qi_plan* plan, int n_held, int n_targets,
                                   long long words);

/* ---- Syndrome shares: locate bad fragments at any k from per-node sums.
 * For one stripe, ids[0 .. N) are the N = k + R listed fragments (decode's id
 * space, distinct, below k + m), R = n_checks, 1 <= R <=
 * min(QI_SYNDROME_MAX_CHECKS, m).  With x_i = r^ids[i] and the dual weights
 * w_i = prod_{l != i, l < N} (x_i - x_l), the syndromes of the received
 * symbols y_i of a column are S_j = sum_i y_i x_i^j / w_i, j < R: all 0 for a
 * codeword, and linear in the rows.
 *
 * Helper side (qi_gpu_syndrome_ctx, qi_gpu_syndrome).  held[0 .. H) are
 * distinct positions into ids, 1 <= H <= N: the listed fragments whose rows
 * this call has.  Per column it computes
 *   out_j = canon(acc_j + sum_{h<H} (x_held[h]^j / w_held[h]) y_h),  j < R,
 * in [0, 65536].  Every other convention is qi_gpu_partial's: rows are
 * positional (row h of stripe s at d_rows + s * rss + h * rrs, its bucket
 * slot h of n_held), accumulator and output row j are slot j of n_checks; y_h
 * is the restored symbol (65536 where the column is in the row's bucket; a
 * systematic data row, id < k, carries no marks and its bucket is not read);
 * d_acc NULL starts from 0; a result of 65536 is stored as 0 and recorded in
 * the out bucket of slot j (the count goes on past out_cap; clear the out
 * counts first, NULL out counts skip the recording); d_out == d_acc with equal
 * strides is allowed and is the expected use, with distinct acc and out
 * bucket sets.  Any positive strides at any 2-byte alignment; rows and
 * strides that are all multiples of 16 bytes move as 16-byte pieces per lane.
 * The shares of any partition of the N positions, added in any order, are bit
 * for bit the result of one call with H = N, rows and marks both: the R
 * syndrome rows.  For an intact stripe those are all 0 with empty buckets.
 *
 * The share context is a partial repair's (n_checks in the place of
 * n_targets): per stripe the n_held x n_checks balanced coefficients and the
 * held rows' ids; the row pass is the partial repair's kernel.  It costs
 * O(n_held N) field operations per stripe, one inversion per held row.
 * Everything is asynchronous on `stream`: no host tables, no blocking copy.
 *
 * Errors: an id not below k + m or repeated, a position not below N or
 * repeated raise bit 2 of qi_gpu_take_error when the context is built; that
 * row's coefficients are 0 and the call stays inside the caller's rows.  An in
 * or acc bucket over its capacity raises bit 1.  n_checks outside 1 .. min(8,
 * m) or n_held outside 1 .. N return -1 (qi_gpu_syndrome_ctx_bytes: 0,
 * qi_gpu_syndrome_kernels: "") and launch nothing. */
#define QI_SYNDROME_MAX_CHECKS 8
#define QI_SYNDROME_MAX_ERRORS 4
size_t qi_gpu_syndrome_ctx_bytes(const qi_plan* plan, int n_held, int n_checks, int n_stripes);
int qi_gpu_syndrome_ctx(qi_plan* plan, const uint16_t* d_ids /*[S][k + R]*/,
                        const uint16_t* d_held /*[S][H] positions into ids*/, int n_held,
                        int n_checks, int n_stripes, void* d_ctx, void* stream);
int qi_gpu_syndrome(qi_plan* plan, const void* d_ctx, int n_held, int n_checks,
                    const uint16_t* d_rows, long long rss, long long rrs,
                    const uint32_t* d_in_counts, const uint32_t* d_in_entries, int in_cap,
                    const uint16_t* d_acc, long long ass, long long ars,
                    const uint32_t* d_acc_counts, const uint32_t* d_acc_entries, int acc_cap,
                    uint16_t* d_out, long long oss, long long ors,
                    uint32_t* d_out_counts, uint32_t* d_out_entries, int out_cap,
                    long long words, int n_stripes, void* stream);
/* "syndrome=<context kernel> + <partial kernel form>" (rows and strides at
 * multiples of 16 bytes); "" for counts out of range.  Per calling thread,
 * valid until its next call. */
const char* qi_gpu_syndrome_kernels(const qi_plan* plan, int n_held, int n_checks,
                                    long long words);

/* Coordinator side (qi_gpu_syndrome_locate_ctx, qi_gpu_syndrome_locate): the
 * decision of qi_gpu_locate_multi from the R summed syndrome rows alone, at
 * any k.  d_syn row j of stripe s is at d_syn + s * sss + j * srs, its marks
 * (a syndrome of 65536) in bucket slot j of n_checks (d_counts NULL: none; a
 * bucket over its capacity raises bit 1).  max_errors = t, 0 <= t <=
 * floor(R / 2) <= QI_SYNDROME_MAX_ERRORS.  A column whose R syndromes are all
 * 0 is clean.  Any other column is located when 1 <= nu <= t listed fragments
 * explain all R syndromes with errors that are not 0, else unlocated: b <= t
 * bad fragments are located exactly, t < b <= R - t bad fragments are always
 * unlocated, more may be miscorrected.  t = 0 is detection only: every column
 * that is not clean counts as unlocated (a verify at any k).
 *
 * Outputs, initialised by the call, as qi_gpu_locate_multi's: d_located[s * N
 * + p] the located columns fragment position p takes part in, d_unlocated[s],
 * d_weights[s * QI_SYNDROME_MAX_ERRORS + nu - 1] the columns located with nu
 * fragments, d_fix_counts[s] the fix entries of stripe s (the count goes on
 * past fix_cap; entries past it are dropped), d_fixes[(s * fix_cap + e) * 3
 * ..] = {column, list position p, error e}.  The nu entries of a column are
 * adjacent.  No row is written.
 *
 * The fix is a delta: e = E w_p in [1, 65536] is what fragment p is off by,
 * and the true symbol is (y_p - e) mod 65537 -- the coordinator does not hold
 * y_p.  Unlike qi_gpu_locate_multi, which drops a column whose corrected
 * symbol cannot be stored (65536 on a systematic data row), this call cannot
 * tell: the holder decides when it applies the fix (qi_fec_apply_deltas).
 *
 * The context holds per stripe the N ids, points and weights, 12 N bytes; it
 * costs O(N^2) field operations per stripe, spread over ceil(N / 256) blocks.
 * Ids not below k + m or repeated raise bit 2 when it is built.  n_checks
 * outside 1 .. min(8, m) or max_errors outside 0 .. n_checks / 2 return -1
 * (qi_gpu_syndrome_locate_ctx_bytes: 0, qi_gpu_syndrome_locate_kernels: "")
 * and launch nothing. */
size_t qi_gpu_syndrome_locate_ctx_bytes(const qi_plan* plan, int n_checks, int n_stripes);
int qi_gpu_syndrome_locate_ctx(qi_plan* plan, const uint16_t* d_ids /*[S][k + R]*/, int n_checks,
                               int n_stripes, void* d_ctx, void* stream);
int qi_gpu_syndrome_locate(qi_plan* plan, const void* d_ctx, int n_checks, int max_errors,
                           const uint16_t* d_syn, long long sss, long long srs,
                           const uint32_t* d_counts, const uint32_t* d_entries, int cap,
                           uint32_t* d_located /*[S][k + R]*/, uint32_t* d_unlocated /*[S]*/,
                           uint32_t* d_weights /*[S][QI_SYNDROME_MAX_ERRORS]*/,
                           uint32_t* d_fix_counts /*[S]*/, uint32_t* d_fixes /*[S][fix_cap][3]*/,
                           int fix_cap, long long words, int n_stripes, void* stream);
/* "syndrome_locate=<context kernel> + <kernel>"; "" when out of range. */
const char* qi_gpu_syndrome_locate_kernels(const qi_plan* plan, int n_checks, int max_errors,
                                           long long words);

/* ---- Device patch: apply the fix lists of a locate to the rows and their
 * marks.  qi_gpu_locate, qi_gpu_locate_multi and qi_gpu_syndrome_locate leave
 * per list position a fix count and d_fixes[s][fix_cap][3]; this call consumes
 * them on the device, so that verify -> locate -> patch -> decode / repair is
 * a chain of asynchronous calls on one stream.  The rule is that of the host
 * facade (qi_fec_locate_multi_blocks with `correct`, qi_fec_apply_deltas), per
 * stripe, over the unordered device buckets.
 *
 * Any plan qi_plan_create accepts (any k, both code types); there is no
 * context.  d_ids are the n_listed = N ids that were given to the locate's
 * context, 1 <= N <= k + m.
 *
 * List position s owns d_ids[s * N ..], d_mine[s * N ..], d_unlocated[s],
 * d_fix_counts[s], d_fixes[s], d_status[s] and d_applied[s], and patches the
 * rows and buckets of stripe d_stripes[s] (d_stripes NULL: of stripe s).  Two
 * list positions that name the same stripe in one call are undefined, and so
 * is an id that d_ids[s * N ..] holds twice (two positions would share one row
 * and one bucket); both stay inside the caller's rows and inside each bucket's
 * oor_cap entries.  Rows and buckets are addressed by fragment id exactly as
 * qi_gpu_decode addresses received rows: d_data for f < k of a systematic
 * plan, d_coded by slot otherwise, the buckets with slots = n_outputs.  d_data
 * may be NULL for a non-systematic plan; a systematic plan may pass NULL for a
 * region none of its applied fixes touches.  Any positive strides with a unit
 * inner stride, at any 2-byte alignment.
 *
 * The fixes of a stripe are its first min(d_fix_counts[s], fix_cap) entries
 * {column, position p, third word}.  A fix with d_mine[s * N + p] == 0 is
 * skipped (the holder's rule of qi_fec_apply_deltas: another node holds that
 * fragment): only p < N is checked of it, and it is not counted.  For every
 * other fix let y be the restored symbol of the row at the column: 65536
 * where the column is in the row's bucket, else the stored word (a systematic
 * data row has no bucket; with NULL counts nothing is marked).  Then
 *   QI_PATCH_ABSOLUTE  v = the third word, valid in [0, 65536];
 *   QI_PATCH_DELTA     e = the third word, valid in [1, 65536], and
 *                      v = (y - e) mod 65537.
 * The row's word becomes v & 0xffff and the column is in the row's bucket
 * afterwards iff v == 65536: inserted if it was absent, removed if it was
 * present and v != 65536, the bucket untouched otherwise.  Buckets stay
 * unordered, their counts exact, without duplicates.  Rows, words and buckets
 * that no applied fix names are not written.
 *
 * All or nothing per stripe.  d_status[s] is the smallest of these codes that
 * applies; a stripe with one of them is left byte for byte as it was, rows
 * and buckets, with d_applied[s] = 0:
 *   QI_PATCH_UNLOCATED    d_unlocated is not NULL and d_unlocated[s] != 0;
 *   QI_PATCH_TRUNCATED    d_fix_counts[s] > fix_cap: entries were dropped; or
 *                         d_fix_counts[s] > QI_PATCH_MAX_FIXES, the longest
 *                         list one call applies to a stripe, whatever fix_cap;
 *   QI_PATCH_BAD_FIX      a position >= N; in a fix that is not skipped a
 *                         column >= words, a third word out of range, an id
 *                         >= k + m or an id in a region passed as NULL; a
 *                         touched bucket whose count is already above oor_cap
 *                         (this also raises bit 1 of qi_gpu_take_error);
 *   QI_PATCH_DATA_MARK    a systematic data row would have to hold 65536;
 *   QI_PATCH_BUCKET_FULL  a touched bucket's new count would exceed oor_cap
 *                         (NULL counts: any v == 65536 on a coded row).
 * Otherwise d_status[s] = QI_PATCH_DONE and d_applied[s] is the number of
 * fixes applied, or QI_PATCH_NONE when that number is 0 (an empty list, or
 * every fix skipped).  A (position, column) pair named twice in one list
 * leaves that stripe unspecified, but the call stays inside the caller's rows
 * and inside each bucket's oor_cap entries.  The new count is what decides:
 * a bucket at oor_cap that loses one mark and gains one in the same list is
 * patched, and no entry is ever written at or past oor_cap.
 *
 * A NULL plan, a mode that is not one of the two, n_listed outside 1 .. k + m,
 * fix_cap < 0, words outside 1 .. 2^32 or n_stripes < 1 return -1 and launch
 * nothing (the bytes call 0, the kernels call "").  So do, as in the sibling
 * calls, a NULL d_ids, d_fix_counts, d_work, d_status or d_applied, NULL
 * d_fixes with fix_cap > 0, oor_cap < 0, counts without entries at oor_cap >
 * 0, and a negative stride of a region that is passed.  fix_cap == 0: every
 * stripe gets QI_PATCH_NONE, or QI_PATCH_TRUNCATED where its count is not 0;
 * d_fixes may then be NULL.
 *
 * Everything is asynchronous on `stream`: no host tables, no blocking copy.
 * d_work is scratch of qi_gpu_patch_work_bytes bytes (per stripe and position
 * the marks inserted and removed and the bucket's editing lane); it needs no
 * clearing, and only one call at a time may use a given work buffer.
 *
 * Decode and repair contexts hold the marks of the buckets they were built
 * from (the route tables): after a patch that changed a bucket they are stale
 * and must be rebuilt before the healed rows are decoded. */
#define QI_PATCH_ABSOLUTE 0   /* fixes {column, position, v}: qi_gpu_locate, qi_gpu_locate_multi */
#define QI_PATCH_DELTA    1   /* fixes {column, position, e}: qi_gpu_syndrome_locate              */

/* per-stripe status */
#define QI_PATCH_NONE            0  /* nothing to apply                                   */
#define QI_PATCH_DONE            1
#define QI_PATCH_UNLOCATED       2  /* d_unlocated[s] != 0                                */
#define QI_PATCH_TRUNCATED       3  /* d_fix_counts[s] > fix_cap (entries were dropped), or
                                     * > QI_PATCH_MAX_FIXES                                */
#define QI_PATCH_BAD_FIX         4  /* see above                                          */
#define QI_PATCH_DATA_MARK       5  /* a systematic data row would have to hold 65536     */
#define QI_PATCH_BUCKET_FULL     6  /* a bucket would grow past oor_cap (NULL counts: past 0) */

/* the longest list one call applies to a stripe (one bit of a block's LDS per entry);
 * fix_cap itself, the stride of d_fixes, is not bounded */
#define QI_PATCH_MAX_FIXES 262144

size_t qi_gpu_patch_work_bytes(const qi_plan* plan, int n_listed, int n_stripes);
int qi_gpu_patch(qi_plan* plan, int mode,
                 const uint16_t* d_ids /*[S][N] as given to the locate context*/, int n_listed,
                 const uint8_t* d_mine /*[S][N] or NULL: 0 = not held here, skip*/,
                 const uint32_t* d_stripes /*[S] or NULL, as qi_gpu_locate*/,
                 const uint32_t* d_unlocated /*[S] or NULL*/,
                 const uint32_t* d_fix_counts /*[S]*/, const uint32_t* d_fixes /*[S][fix_cap][3]*/,
                 int fix_cap,
                 uint16_t* d_data, long long dss, long long drs,
                 uint16_t* d_coded, long long css, long long crs,
                 uint32_t* d_oor_counts, uint32_t* d_oor_entries, int oor_cap,
                 void* d_work, uint32_t* d_status /*[S]*/, uint32_t* d_applied /*[S]*/,
                 long long words, int n_stripes, void* stream);
/* "patch=<kernel>"; "" for arguments out of range.  Per calling thread, valid
 * until its next call. */
const char* qi_gpu_patch_kernels(const qi_plan* plan, int n_listed, int mode, long long words);

/* Build identification: "<git describe>+src:<hash of the library sources>". */
const char* qi_build_id(void);


/* ---- Block API over host buffers (C view of qi::fec::RsFnt, see
 * include/qi_fec.hpp; semantics of FecCode::encode_blocks_vertical /
 * decode_blocks_vertical, src/fec_base.h:1066-1321).  OOR marks are returned
 * as per-output ascending offset lists of capacity oor_cap (counts exact). */
typedef struct qi_fec qi_fec;
qi_fec* qi_fec_new(int systematic, int k, int m);
void qi_fec_delete(qi_fec* f);
int qi_fec_n_outputs(const qi_fec* f);
/* outputs: n_outputs pointers (NULL = not wanted). 0 or -1 */
int qi_fec_encode_blocks(qi_fec* f, uint8_t** data, uint8_t** outputs,
                         size_t block_bytes, uint32_t* oor, uint32_t* oor_count,
                         uint32_t oor_cap);
/* returns 1 decoded, 0 fewer than k fragments, -1 error */
int qi_fec_decode_blocks(qi_fec* f, uint8_t** data, uint8_t** parities,
                         const uint32_t* oor, const uint32_t* oor_count,
                         uint32_t oor_cap, const int* missing,
                         const int* wanted, size_t block_bytes);

/* Fused repair of n_targets missing fragments (RsFnt::repair_blocks_vertical,
 * include/qi_fec.hpp): `targets` are fragment ids in the decode's id space
 * (systematic: f < k data row f, else parity f - k; non-systematic: coded row
 * f), each flagged in `missing`; the first k present fragments are used, as
 * by qi_fec_decode_blocks.  out[j] receives target j (block_bytes), its marks
 * ascending in out_oor[j * out_cap ..] with the exact count in out_count[j].
 * `data` may be NULL for non-systematic codes.  Returns 1 rebuilt, 0 fewer
 * than k fragments, -1 error (a target present or out of range), -2 shape not
 * supported (k > 256, n_targets outside 1 .. min(64, m), or a block wider
 * than the single-chunk staging): decode and encode instead. */
int qi_fec_repair_blocks(qi_fec* f, uint8_t** data, uint8_t** parities,
                         const uint32_t* oor, const uint32_t* oor_count,
                         uint32_t oor_cap, const int* missing, const int* targets,
                         int n_targets, uint8_t** out, uint32_t* out_oor,
                         uint32_t* out_count, uint32_t out_cap, size_t block_bytes);

/* Fused verify of the present fragments (RsFnt::verify_blocks_vertical,
 * include/qi_fec.hpp): the first k present fragments are the basis, every
 * other present one is recomputed from them and compared with its buffer and
 * its marks.  result: 3 * (k + m) values, per fragment id {value mismatches,
 * mark mismatches, first mismatching column or 0xFFFFFFFF}, or {-1, -1, -1}
 * for a missing or a basis fragment.  `data` may be NULL for non-systematic
 * codes, oor_count NULL when no row has marks.  Returns 1 verified, 0 fewer
 * than k + 1 fragments present, -1 error, -2 shape not supported (k > 256 or
 * a block wider than the single-chunk staging). */
int qi_fec_verify_blocks(qi_fec* f, uint8_t** data, uint8_t** parities,
                         const uint32_t* oor, const uint32_t* oor_count,
                         uint32_t oor_cap, const int* missing, long long* result,
                         size_t block_bytes);

/* Fragment locate over the present fragments (RsFnt::locate_blocks_vertical,
 * include/qi_fec.hpp): the first min(present, k + 8) present fragments are
 * listed, as qi_fec_decode_blocks chooses them, and each bad column is
 * attributed to the one listed fragment that is wrong there.  result: k + m + 1
 * values, per fragment id the number of columns located in it (-1 for a
 * fragment that is missing or not listed), then the number of bad columns
 * that could not be attributed.  With exactly k + 2 present (two syndromes)
 * two bad fragments of a column may be attributed to a third; from k + 3 on
 * such a column is counted as unlocated.
 * correct != 0: when there are located columns and none is unlocated, the
 * corrected symbols are written into the caller's buffers and the ascending
 * mark lists (oor / oor_count, oor_cap entries per coded fragment) follow: a
 * mark is inserted where the symbol becomes 65536 and removed where it stops
 * being one.  If a list would grow beyond oor_cap (oor_count NULL: beyond 0)
 * nothing is patched and -1 returned.
 * Returns 1 located (result filled), 2 located and patched, 0 fewer than k + 2
 * fragments present, -1 error, -2 shape not supported (k > 256, m < 2, or a
 * block wider than the single-chunk staging). */
int qi_fec_locate_blocks(qi_fec* f, uint8_t** data, uint8_t** parities, uint32_t* oor,
                         uint32_t* oor_count, uint32_t oor_cap, const int* missing,
                         long long* result, int correct, size_t block_bytes);

/* The same with up to max_errors bad fragments per column
 * (RsFnt::locate_multi_blocks_vertical, qi_gpu_locate_multi), 1 <= max_errors
 * <= QI_LOCATE_MAX_ERRORS (else -1).  Listing as above, R = listed - k; 0 is
 * also returned when R < 2 max_errors.  result: the k + m + 1 values of
 * qi_fec_locate_blocks (a located column counts in each of its fragments),
 * then max_errors values: the columns located with 1 .. max_errors fragments.
 * `correct` patches all fixes of all columns or, with a column unlocated or a
 * mark list past oor_cap, nothing.  Return values as qi_fec_locate_blocks. */
int qi_fec_locate_multi_blocks(qi_fec* f, uint8_t** data, uint8_t** parities, uint32_t* oor,
                               uint32_t* oor_count, uint32_t oor_cap, const int* missing,
                               int max_errors, long long* result, int correct,
                               size_t block_bytes);

/* Fingerprints of every present fragment (RsFnt::fingerprint_blocks_vertical,
 * qi_gpu_fingerprint): keys[n_keys][3], each component in 1 .. 65536, 1 <=
 * n_keys <= QI_FINGERPRINT_MAX_KEYS.  result: (k + m) * n_keys values, per
 * fragment id its n_keys fingerprints in [0, 65536], or -1 for a missing
 * fragment.  Any k and any block width: blocks wider than the staging go
 * through in column chunks and the chunk results are added modulo 65537.
 * `data` may be NULL for non-systematic codes, oor_count NULL when no row has
 * marks.  Returns 1 done, -1 error (a key or n_keys out of range, a NULL
 * handle; nothing is staged). */
int qi_fec_fingerprint_blocks(qi_fec* f, uint8_t** data, uint8_t** parities, const uint32_t* oor,
                              const uint32_t* oor_count, uint32_t oor_cap, const int* missing,
                              const uint32_t* keys, int n_keys, long long* result,
                              size_t block_bytes);

/* Delta update of the held coded fragments (RsFnt::update_blocks_vertical,
 * include/qi_fec.hpp): data rows ids[0 .. n_rows) go from old_rows[u] to
 * new_rows[u] (block_bytes each); parities[j] != NULL are the coded fragments
 * held here, updated in place, their marks (oor / oor_count, oor_cap entries
 * per fragment, as qi_fec_encode_blocks returned them) replaced by the new
 * ones, ascending, with exact counts (a count above oor_cap: only oor_cap
 * entries were written).  Returns 1 updated, -1 error (an id out of range or
 * repeated, no fragment held), -2 shape not supported (n_rows outside 1 ..
 * min(8, k), or 2 n_rows + held rows wider than the single-chunk staging):
 * encode again instead. */
int qi_fec_update_blocks(qi_fec* f, const int* ids, int n_rows, uint8_t** old_rows,
                         uint8_t** new_rows, uint8_t** parities, uint32_t* oor,
                         uint32_t* oor_count, uint32_t oor_cap, size_t block_bytes);

/* Partial repair (RsFnt::partial_repair_blocks_vertical, qi_gpu_partial):
 * the share of the repair of targets[0 .. n_targets) from the k helper
 * fragments ids[0 .. k) (decode's id space) that the holder of the fragments
 * held_ids[0 .. n_held) can form; each held id is one of ids (it is mapped to
 * its position here).  rows[h] is fragment held_ids[h] (block_bytes), its
 * marks oor[h * oor_cap ..] with the count oor_count[h] (oor_count NULL: no
 * marks; a systematic data row has none).  acc != 0: out[j], out_oor and
 * out_count hold the partial rows and marks so far and are added to; else the
 * sum starts from 0.  out[j] receives partial row j, its marks ascending in
 * out_oor[j * out_cap ..] with the exact count in out_count[j] (a count above
 * out_cap: only out_cap entries were written, and the list is not a valid acc
 * for another call).  Returns 1 done, -1 error (an id, a held id or a target
 * out of range, repeated or misplaced), -2 shape not supported (n_held
 * outside 1 .. k, n_targets outside 1 .. min(8, m), or n_held + n_targets
 * rows wider than the single-chunk staging). */
int qi_fec_partial_repair_blocks(qi_fec* f, const int* ids, const int* held_ids, int n_held,
                                 uint8_t** rows, const uint32_t* oor, const uint32_t* oor_count,
                                 uint32_t oor_cap, const int* targets, int n_targets, int acc,
                                 uint8_t** out, uint32_t* out_oor, uint32_t* out_count,
                                 uint32_t out_cap, size_t block_bytes);

/* Syndrome share (RsFnt::syndrome_blocks_vertical, qi_gpu_syndrome): the
 * share of the n_checks syndrome rows of the n_listed = k + n_checks listed
 * fragments listed_ids (decode's id space) that the holder of the fragments
 * held_ids[0 .. n_held) can form; each held id is one of listed_ids.  rows,
 * oor, oor_count, oor_cap, acc, out, out_oor, out_count and out_cap as for
 * qi_fec_partial_repair_blocks, with n_checks rows out.  Any k.  Returns 1
 * done, -1 error (an id or a held id out of range, repeated or not listed),
 * -2 shape not supported (n_checks outside 1 .. min(8, m), n_listed != k +
 * n_checks, n_held outside 1 .. n_listed, or n_held + n_checks rows wider
 * than the single-chunk staging). */
int qi_fec_syndrome_blocks(qi_fec* f, const int* listed_ids, int n_listed, const int* held_ids,
                           int n_held, uint8_t** rows, const uint32_t* oor,
                           const uint32_t* oor_count, uint32_t oor_cap, int n_checks, int acc,
                           uint8_t** out, uint32_t* out_oor, uint32_t* out_count,
                           uint32_t out_cap, size_t block_bytes);

/* The coordinator's decision over summed syndrome rows
 * (RsFnt::locate_syndromes, qi_gpu_syndrome_locate): rows[j], j < n_checks =
 * n_listed - k, are the complete sums of qi_fec_syndrome_blocks over all
 * n_listed fragments, with their marks (oor_count NULL: none).  0 <=
 * max_errors <= n_checks / 2.  result: k + m + 1 + max_errors values, per
 * fragment id the located columns it takes part in (-1: not listed), the
 * unlocated columns, then the columns located with 1 .. max_errors fragments.
 * fixes: up to fix_cap triples {column, fragment id, error e in 1 .. 65536},
 * the fixes of a column adjacent; *n_fixes their exact number (above fix_cap:
 * only fix_cap were written; call again with that capacity).  The true symbol
 * is (y - e) mod 65537 (qi_fec_apply_deltas).  Returns 1 done, -1 error, -2
 * shape not supported (n_checks outside 1 .. min(8, m), max_errors out of
 * range, or a block wider than the single-chunk staging). */
int qi_fec_locate_syndromes(qi_fec* f, const int* listed_ids, int n_listed, uint8_t** rows,
                            const uint32_t* oor, const uint32_t* oor_count, uint32_t oor_cap,
                            int max_errors, long long* result, uint32_t* fixes, uint32_t fix_cap,
                            uint32_t* n_fixes, size_t block_bytes);

/* The holder's step (RsFnt::apply_deltas; no device): for every fix {column,
 * fragment id, e} that names one of fragment_ids[0 .. n_rows), the restored
 * symbol y of rows[h] at that column (65536 where oor lists it) becomes (y -
 * e) mod 65537, and the ascending mark list of the row follows (oor[h *
 * oor_cap ..], oor_count[h]; a systematic data row has none).  Fixes for
 * other fragments are skipped.  The whole patch is refused, and nothing
 * touched, when a data row would have to hold 65536 or a mark list would grow
 * beyond oor_cap (oor_count NULL: beyond 0).  Returns the number of fixes
 * applied (0 included), -1 error, -3 refused. */
int qi_fec_apply_deltas(qi_fec* f, const int* fragment_ids, int n_rows, uint8_t** rows,
                        uint32_t* oor, uint32_t* oor_count, uint32_t oor_cap,
                        const uint32_t* fixes, uint32_t n_fixes, size_t block_bytes);

/* Scrub at any k (RsFnt::scrub_blocks_vertical): qi_fec_locate_multi_blocks
 * without its k <= 256 limit, composed of the three calls above with every
 * listed fragment held here.  The first min(present, k + 8) present fragments
 * are listed, R = listed - k; 0 <= max_errors <= 4, max_errors = 0 only
 * detects.  result, `correct` and the return values as
 * qi_fec_locate_multi_blocks (0: fewer than k + max(1, 2 max_errors)
 * fragments listed); a patch that qi_fec_apply_deltas refuses returns -1 with
 * nothing patched.  -2: a block wider than the single-chunk staging. */
int qi_fec_scrub_blocks(qi_fec* f, uint8_t** data, uint8_t** parities, uint32_t* oor,
                        uint32_t* oor_count, uint32_t oor_cap, const int* missing,
                        int max_errors, long long* result, int correct, size_t block_bytes);

/* Stream API (encode_streams_vertical / decode_streams_vertical,
 * src/fec_base.h:463-542, 898-1048) over caller memory: each fragment is a
 * stream of `bytes` bytes.  The streams go through the two-slot pinned
 * pipeline of qi::fec::RsFnt (chunks of whole packets, host reads/writes
 * overlapping the transfers and kernels).  Encode: all outputs required;
 * 0 or -1.  Decode: data[i] / parities[i] NULL = missing (data may be NULL
 * as a whole for non-systematic codes), out_data[i] NULL = not wanted;
 * 1 decoded, 0 fewer than k fragments, -1 error. */
int qi_fec_encode_streams(qi_fec* f, const uint8_t** data, size_t bytes,
                          uint8_t** outputs, uint32_t* oor, uint32_t* oor_count,
                          uint32_t oor_cap);
int qi_fec_decode_streams(qi_fec* f, const uint8_t** data,
                          const uint8_t** parities, size_t bytes,
                          const uint32_t* oor, const uint32_t* oor_count,
                          uint32_t oor_cap, uint8_t** out_data);

/* ---- RS-NF4 block API (C view of qi::fec::RsNf4; RsNf4<T>,
 * src/fec_rs_nf4.h:46-334).  word_size 2, 4 or 8 (NULL otherwise): every
 * word packs word_size/2 GF(65537) components, each coded like an RS-FNT
 * column on the device.  Non-systematic: n_outputs = k + m.  OOR marks per
 * output: ascending word offsets in `oor` with the component bitmask in
 * `flags` (oor_cap entries each, counts exact).  Whole words only. */
typedef struct qi_nf4 qi_nf4;
qi_nf4* qi_nf4_new(int word_size, int k, int m);
void qi_nf4_delete(qi_nf4* f);
int qi_nf4_n_outputs(const qi_nf4* f);
/* 0 or -1 */
int qi_nf4_encode_blocks(qi_nf4* f, uint8_t** data, uint8_t** outputs,
                         size_t block_bytes, uint32_t* oor, uint32_t* flags,
                         uint32_t* oor_count, uint32_t oor_cap);
/* missing: k + m flags.  1 decoded, 0 fewer than k fragments, -1 error */
int qi_nf4_decode_blocks(qi_nf4* f, uint8_t** data, uint8_t** parities,
                         const uint32_t* oor, const uint32_t* flags,
                         const uint32_t* oor_count, uint32_t oor_cap,
                         const int* missing, const int* wanted,
                         size_t block_bytes);

#ifdef __cplusplus
}
#endif

#endif
