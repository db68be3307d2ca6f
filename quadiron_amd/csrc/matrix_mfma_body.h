// Body of a kernel of kernels.hip, included once per form: MODE (a
// constexpr MatMode set by the including kernel, next to its VerArgs v)
// selects the plain form, the form for input and output marks in one launch
// (BOTH: a repair) or the verify form (VERIFY: a repair that compares with
// the stored row instead of storing); in the plain form the text is the
// kernel as it was before the others existed.  Not a stand-alone header.
    [[maybe_unused]] constexpr bool BOTH = MODE != MatMode::kPlain,
                                    VERIFY = MODE == MatMode::kVerify;
    const MatLayout L = a.L;
    const int32_t* __restrict__ mat = a.mat;
    const long long mat_stride = a.ms;
    const int32_t* __restrict__ ids = a.ids;
    const long long ids_stride = a.is;
    const RowSrc src = a.src;
    const RowDst dst = a.dst;
    const MatExt ext = a.ext;
    const long long words = a.words;
    const int tiles = a.tiles;
    const Oor in_oor = a.in_oor;
    const int slot_base = a.slot_base;
    const Oor out_oor = a.out_oor;
    const uint32_t* __restrict__ route = a.route;
    const long long route_stride = a.rstride;
    uint32_t* err = a.err;
    using G = MfmaTile<KS, NST, NW>;
    constexpr int NCOL = G::kCols, KH = G::kRows, RSB = G::kPitch;
    constexpr int CPL = G::kCpl, RG = G::kRg;
    // one dynamic region (16-byte aligned base: no static LDS in front)
    extern __shared__ __attribute__((aligned(16))) uint8_t qi_lds[];
    uint8_t* img = qi_lds;
    int* s_i = reinterpret_cast<int*>(qi_lds + G::kImg);
    uint32_t* s_col = reinterpret_cast<uint32_t*>(s_i + kMaxTileOor);
    int* s_cnt = reinterpret_cast<int*>(s_col + kMaxTileOor);

    int s, tile;
    block_map(blockIdx.x, tiles, s, tile);
    const int kin = L.kin;
    const long long col0 = static_cast<long long>(tile) * NCOL;
    const long long col1 = col0 + NCOL;
    // staging: this thread's first column and its row group
    const uint32_t cl = (RG == 1 ? threadIdx.x : threadIdx.x % G::kTpr) * CPL;
    const int rg = RG == 1 ? 0 : static_cast<int>(threadIdx.x / G::kTpr);
    const uint32_t voff = static_cast<uint32_t>((col0 + cl) * 2);
    const int32_t* M = mat + s * mat_stride;
    const int32_t* sid = ids ? ids + s * ids_stride : nullptr;
    const Region<true> g0(src.base0 + s * src.ss0, ext.e0);
    const Region<true> g1(src.base1 ? src.base1 + s * src.ss1 : src.base0,
                          ext.e1);
    const Region<true> go(dst.base + s * dst.ss, ext.eo);

    // OOR marks of the received rows in this tile: route table (scalar
    // loads) or bucket scan, as matrix_kernel
    int n_rm = 0;
    const uint32_t* rm = nullptr;
    bool scan = in_oor.counts != nullptr;
    if (route) {
        const uint32_t* rt =
            route + s * route_stride + (col0 / kRouteTile) * kRouteStride;
        const uint32_t rc = rt[0];
        if (rc <= static_cast<uint32_t>(kRouteCap)) {
            n_rm = static_cast<int>(rc);
            rm = rt + 1;
            scan = false;
        }
    }

    // operand tiles of output block 0 (per-lane loads; issued before the row
    // loads so their latency hides behind the staging)
    const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int g = l >> 4, q = (l & 15) >> 1, p = l & 1, tl = l & 15;
    const int RB = L.RB();
    const int32_t* mf = M + L.mf();
    const int32_t* kmf = M + L.kmf();
    const int32_t* rscale = M + L.rscale_mf();
    const int32_t* __restrict__ rowmap = a.rowmap;
    auto load_ops = [&](int rb, qi_v2i (&b)[KS][3], int32_t& kt, int32_t& rs, int32_t (&pr)[3]) {
        // [b | a] is [0 | b] of the l' half over the h' K-steps and [a | 0]
        // of the h' half over the l' K-steps, lane for lane (the same K
        // offset within the half): from those registers at KS >= 2 (the
        // contexts do not store it); at KS = 1 the halves share a K-step
        // and sit in other lanes, so it is loaded
#pragma unroll
        for (int ks = 0; ks < KS; ks++)
#pragma unroll
            for (int ty = 0; ty < (KS >= 2 ? 2 : 3); ty++)
                b[ks][ty] = *reinterpret_cast<const qi_v2i*>(
                    mf + ((rb * KS + ks) * 3 + ty) * 128 + l * 2);
        if constexpr (KS >= 2) {
#pragma unroll
            for (int ks = 0; ks < KS; ks++)
                b[ks][2] = ks < KS / 2 ? b[ks + KS / 2][1] : b[ks - KS / 2][0];
        }
        // unconditional loads (a clamped row), selected after: an exec-masked
        // load leaves the compiler unsure how many vector-memory ops are in
        // flight, and it then drains vmcnt further than needed
        const int t = 16 * rb + tl, tc = t < L.R ? t : L.R - 1;
        const int32_t k0 = kmf[tc], r0 = rscale[tc];
        kt = t < L.R ? k0 : 0;
        rs = t < L.R ? r0 : 1;
        // output rows: this lane's epilogue row and its two store rows
        pr[0] = rowmap[tc];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int ot = 16 * rb + 8 * h + (l >> 3);
            pr[1 + h] = rowmap[ot < L.R ? ot : L.R - 1];
        }
    };
    // tall matrices (RSPLIT, the encode generators): wave wv takes row
    // blocks wv, wv + NW, ... over all the block's super tiles, so each wave
    // fetches only its own operand tiles (NW x fewer L2 operand reads than
    // every wave walking every row block); otherwise every wave takes every
    // row block over its own super tiles
    constexpr bool rsplit = RSPLIT;
    const int rb0 = rsplit ? wv : 0, rbs = rsplit ? NW : 1;
    constexpr int nst = rsplit ? NST : NST / NW;
    static_assert(rsplit || NST % NW == 0, "super tiles per wave");

    // the first row block's operands, issued ahead of the row loads
    qi_v2i bA[KS][3], bB[KS][3];
    int32_t ktA, rsA, ktB, rsB, prA[3], prB[3];
    const int rlast = RB - 1;
    const bool single = rb0 + rbs >= RB;
    load_ops(min(rb0, rlast), bA, ktA, rsA, prA);

    // stage the tile as byte planes h' (rows 0..KH-1) and l' (rows KH..):
    // this thread's CPL columns of every RG-th row, all row loads issued back
    // to back; rows past kin load a clamped row (their operand bytes are 0)
    uint32_t w[KH / RG][CPL / 2];
    if constexpr (G::kTpr % 64 == 0) {
        // the row group is wave-uniform: every id of the thread's rows in
        // SGPRs first (the scalar loads issue together; loading each id
        // next to its row load made a chain of KH dependent scalar loads,
        // one lgkmcnt(0) per row), then the row loads back to back -- with
        // one source region (every decode but the systematic one, and the
        // encode) a row offset is one scalar multiply
        int idv[KH / RG];
        if (sid && !src.by_pos) {
#pragma unroll
            for (int r = 0; r < KH / RG; r++) {
                const int i = r * RG + rg;
                idv[r] = sid[i < kin ? i : kin - 1];
            }
        } else {
#pragma unroll
            for (int r = 0; r < KH / RG; r++) {
                const int i = r * RG + rg;
                idv[r] = i < kin ? i : kin - 1;
            }
        }
        if (!src.base1) {
            const uint32_t rsb = static_cast<uint32_t>(src.rs0 * 2);
#pragma unroll
            for (int r = 0; r < KH / RG; r++)
                ld_dw<CPL / 2, true, kAuxLd>(g0, static_cast<uint32_t>(idv[r]) * rsb, voff,
                                             w[r]);
        } else {
#pragma unroll
            for (int r = 0; r < KH / RG; r++) {
                const int id = idv[r];
                const bool lo = id < src.split;
                Region<true> g = g0;
                g.r = lo ? g0.r : g1.r;
                const uint32_t off = static_cast<uint32_t>(
                    lo ? id * src.rs0 * 2 : (id - src.split) * src.rs1 * 2);
                ld_dw<CPL / 2, true, kAuxLd>(g, off, voff, w[r]);
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < KH / RG; r++) {
            const int i = r * RG + rg;
            const int ii = i < kin ? i : kin - 1;
            const int id = src.by_pos ? ii : (sid ? sid[ii] : ii);
            const bool lo = id < src.split;
            Region<true> g = g0;
            g.r = lo ? g0.r : g1.r;
            const uint32_t off = static_cast<uint32_t>(
                lo ? id * src.rs0 * 2 : (id - src.split) * src.rs1 * 2);
            ld_dw<CPL / 2, true, kAuxLd>(g, off, voff, w[r]);
        }
    }
    const uint32_t lpos = 64 * (cl / 64) + 16 * ((cl % 16) / 4) +
                          4 * ((cl % 64) / 16) + cl % 4;
#pragma unroll
    for (int r = 0; r < KH / RG; r++) {
        const int i = r * RG + rg;
        if constexpr (CPL == 4) {
            // [c0 lo, c0 hi, c1 lo, c1 hi] [c2 lo, ...] -> hi / lo planes
            const uint32_t hi =
                __builtin_amdgcn_perm(w[r][1], w[r][0], 0x07050301u) ^ 0x80808080u;
            const uint32_t lo =
                __builtin_amdgcn_perm(w[r][1], w[r][0], 0x06040200u) ^ 0x80808080u;
            *reinterpret_cast<uint32_t*>(img + i * RSB + lpos) = hi;
            *reinterpret_cast<uint32_t*>(img + (KH + i) * RSB + lpos) = lo;
        } else {
            const uint32_t hi =
                __builtin_amdgcn_perm(0u, w[r][0], 0x0c0c0301u) ^ 0x8080u;
            const uint32_t lo =
                __builtin_amdgcn_perm(0u, w[r][0], 0x0c0c0200u) ^ 0x8080u;
            *reinterpret_cast<uint16_t*>(img + i * RSB + lpos) =
                static_cast<uint16_t>(hi);
            *reinterpret_cast<uint16_t*>(img + (KH + i) * RSB + lpos) =
                static_cast<uint16_t>(lo);
        }
    }
    OorScan sc{in_oor, sid, src.by_pos, slot_base, kin, s, false};
    int n_lm = 0;
    if (scan) {  // block-uniform; the scan's barriers also publish the image
        const int cnt = scan_tile_marks(sc, col0, col1, words, s_cnt, s_i, s_col, err);
        sc.slow = cnt > kMaxTileOor;
        n_lm = min(cnt, kMaxTileOor);
    } else {
        // the routed marks into the same LDS list: the epilogue then reads
        // only LDS (no memory loads in the hot loop)
        stage_route_marks(rm, n_rm, col0, s_i, s_col);
        __syncthreads();
        n_lm = n_rm;
    }

    // matrix cores: wave wv covers nst super tiles of 64 columns, for each
    // block of 16 output rows in turn (the next block's operands prefetched)
    // (BOTH: a slow tile records its output marks in the redo below)
    const bool rec = out_oor.counts != nullptr && !(BOTH && sc.slow);
    const uint32_t ors = static_cast<uint32_t>(dst.rs * 2);
    // generic -> LDS address space (C-style cast: reinterpret_cast cannot
    // change the address space)
    auto* lds = (__attribute__((address_space(3))) uint8_t*)img;
    const uint32_t abase = static_cast<uint32_t>((8 * g + q) * RSB + 8 * p);
    // One row block: every super tile's MFMAs, epilogue and stores, with
    // the block's operand tiles b / kt / rs.
    auto rb_body = [&](int rb, const qi_v2i (&bop)[KS][3], const int32_t kt,
                       const int32_t rs, const int32_t (&pr)[3]) {
        const int t = 16 * rb + tl;
        const bool trow = t < L.R;
        // VERIFY: this lane's stored row, and its 16 columns of the super
        // tile (loaded ahead of the tile's MFMAs)
        [[maybe_unused]] VerRow vrow{};
        [[maybe_unused]] qi_v4u sv[2];
        if constexpr (VERIFY)
            vrow = verify_row(v, src, s, L.R, t);
        // MFMAs of super tile ST into acc
        auto tile_mfma = [&](const int ST, qi_v4i (&acc)[4][3]) {
#pragma unroll
            for (int T = 0; T < 4; T++) {
                acc[T][0] = qi_v4i{0, 0, 0, 0};
                acc[T][1] = qi_v4i{kt, kt, kt, kt};
                acc[T][2] = qi_v4i{0, 0, 0, 0};
                auto rd_a = [&](int ks) {
                    auto* pa = (__attribute__((address_space(3))) qi_v2i*)(
                        lds + abase + 32 * ks * RSB + (4 * ST + T) * 16);
                    return __builtin_amdgcn_ds_read_tr8_b64_v2i32(pa);
                };
                if constexpr (KS == 1) {
                    const long a = __builtin_bit_cast(long, rd_a(0));
#pragma unroll
                    for (int ty = 0; ty < 3; ty++)
                        acc[T][ty] = __builtin_amdgcn_mfma_i32_16x16x32_i8(
                            a, __builtin_bit_cast(long, bop[0][ty]), acc[T][ty], 0,
                            0, 0);
                } else {
                    // two K-steps per v_mfma_i32_16x16x64_i8 (CDNA4: the
                    // cycles of 16x16x32_i8 at twice the K).  Lane l holds
                    // the 8 A bytes of steps ks and ks + 1 (and the same
                    // two B halves): A and B share their lane/byte -> K
                    // map, so the 64-K product is the sum of the two
                    // 32-K products whatever that map is
#pragma unroll
                    for (int ks = 0; ks < KS; ks += 2) {
                        const qi_v2i a0 = rd_a(ks), a1 = rd_a(ks + 1);
                        const qi_v4i a{a0.x, a0.y, a1.x, a1.y};
#pragma unroll
                        for (int ty = 0; ty < 3; ty++) {
                            // [a | 0] is zero over the l' half of K and
                            // [0 | b] over the h' half: skip the pairs
                            // that lie in a zero half (KS = 4)
                            if ((ty == 0 && ks >= KS / 2) ||
                                (ty == 1 && ks + 1 < KS / 2))
                                continue;
                            const qi_v4i b{bop[ks][ty].x, bop[ks][ty].y,
                                           bop[ks + 1][ty].x, bop[ks + 1][ty].y};
                            acc[T][ty] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                                a, b, acc[T][ty], 0, 0, 0);
                        }
                    }
                }
            }
        };
        // epilogue element math of one super tile: lane (g, t) holds row t,
        // columns 16 g .. 16 g + 15 of the super tile; result j of chunk T is
        // LDS byte 4 g + j = column 16 g + 4 T + j (straight-line VALU, so
        // it can share a scheduling region with the next tile's MFMAs)
        auto tile_y = [&](const qi_v4i (&acc)[4][3], int32_t (&y)[16]) {
#pragma unroll
            for (int T = 0; T < 4; T++)
#pragma unroll
                for (int j = 0; j < 4; j++)
                    y[4 * T + j] =
                        fold(fold(((KS >= 16 ? fold(acc[T][2][j]) : acc[T][2][j]) << 8) +
                                  acc[T][1][j] - acc[T][0][j]));
        };
        // the rest of the epilogue + stores of super tile ST
        auto tile_fin = [&](const int ST, int32_t (&y)[16]) {
            const long long cb = col0 + 64 * ST + 16 * g;
            // restored OOR symbols of the received rows: 65536 == -1 where
            // the stored word is 0 (decode_prepare, src/fec_base.h:1361-1404)
            // Branch-free per lane: the marks come from LDS and the
            // coefficient load is unconditional and consumed at once.  A gather load under a lane-divergent branch left a
            // possibly pending load into a reused VGPR at the loop exit,
            // and the compiler then drained vmcnt(0) -- every outstanding
            // store and operand prefetch -- after every super tile, with or
            // without marks (cfg3 encode: wait_any 34 % of wave cycles).
            // (One loop body, no lambda: as a lambda the compiler indexed
            // y[] dynamically and moved it to scratch memory.)
            // Only the marks inside this super tile's 64 columns are applied
            // (a wave-uniform test on the LDS list: the list holds the route
            // tile's marks, 1024 columns, so without it every super tile
            // paid 80 VALU per mark of its whole route tile).
            const uint32_t st0 = static_cast<uint32_t>(col0 + 64 * ST);
            for (int e = 0; e < n_lm; e++) {
                const uint32_t wcu = __builtin_amdgcn_readfirstlane(s_col[e]);
                if (wcu - st0 >= 64u)
                    continue;
                const int pos = __builtin_amdgcn_readfirstlane(s_i[e]);
                const long long wc = wcu;
                const long long d = wc - cb;
                // from the operand tile in registers (bop[ks][2] = [b | a])
                const int32_t corr = coef_from_tiles<KS>(
                    [&](int idx) {
                        int32_t r = 0;
#pragma unroll
                        for (int q = 0; q < 2 * KS; q++)
                            r = idx == q ? bop[q >> 1][2][q & 1] : r;
                        return r;
                    },
                    pos, l);
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    const int32_t yc = fold(fold(y[c] - corr));
                    y[c] = (trow && d == c) ? yc : y[c];
                }
            }
            if (__builtin_amdgcn_ballot_w64(rs != 1)) {
                // every lane (rs = 1 keeps its value's residue: y is in
                // [-1, 65536] either way): no per-element exec masking
#pragma unroll
                for (int c = 0; c < 16; c++)
                    y[c] = fold(fold(mul_rs(y[c], rs)));
            }
            uint32_t bad = 0;
#pragma unroll
            for (int c = 0; c < 16; c++)
                bad |= static_cast<uint32_t>(y[c]);
            if (__builtin_expect(__builtin_amdgcn_ballot_w64((bad >> 16) != 0) != 0, 0)) {
#pragma unroll
                for (int c = 0; c < 16; c++) {
                    if (static_cast<uint32_t>(y[c]) > 65535u) {
                        if (rec && trow)
                            record_oor(out_oor, s, pr[0], cb + c);
                        y[c] = 0;  // 65536 (or its alias -1) is stored as 0
                    }
                }
            }
            if constexpr (VERIFY) {
                // compared where it lies: no transpose, no store
                verify_tile16(v, static_cast<long long>(s) * L.R + t, trow, y, sv, cb, sc.slow);
                return;
            }
            qi_v4u o0, o1;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                o0[c] = pack_lo(static_cast<uint32_t>(y[2 * c]),
                                static_cast<uint32_t>(y[2 * c + 1]));
                o1[c] = pack_lo(static_cast<uint32_t>(y[8 + 2 * c]),
                                static_cast<uint32_t>(y[8 + 2 * c + 1]));
            }
            // the 16 x 64 output tile is transposed through LDS and stored
            // as 8 whole 128-byte lines per instruction, which can stream
            // (nt|sc1).  One block of output rows: through this super
            // tile's input bytes, dead once its MFMAs are done (row t at
            // image rows 2t, 2t+1, bytes 64 ST..); several: through the
            // wave's own staging tile behind the image (144-byte rows).
            uint8_t* stg;
            int pitch, half;
            if (RB == 1) {
                stg = img + 64 * ST;
                pitch = 2 * RSB;
                half = RSB - 64;  // bytes 64..127 of a row sit one image row down
            } else {
                stg = qi_lds + G::kLds + wv * G::kStage;
                pitch = G::kStagePitch;
                half = 0;
            }
            auto at = [&](int row, int byte) {
                return stg + row * pitch + byte + (byte >= 64 ? half : 0);
            };
            *reinterpret_cast<qi_v4u*>(at(tl, 32 * g)) = o0;
            *reinterpret_cast<qi_v4u*>(at(tl, 32 * g + 16)) = o1;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const int orow = 8 * h + (l >> 3), c = l & 7;
                const qi_v4u v = *reinterpret_cast<const qi_v4u*>(at(orow, 16 * c));
                // rows >= R get an offset past the buffer resource's extent
                // (< 2^31): the hardware drops those stores.  Unconditional,
                // so the compiler keeps an exact count of the stores in flight
                const int ot = 16 * rb + orow;
                const uint32_t vo =
                    ot < L.R ? static_cast<uint32_t>(pr[1 + h]) * ors +
                                   static_cast<uint32_t>((col0 + 64 * ST + 8 * c) * 2)
                             : 0x80000000u;
                __builtin_amdgcn_raw_buffer_store_b128(v, go.r, static_cast<int>(vo), 0,
                                                       kAuxStMf);
            }
            // the staging tile is rewritten by the next (ST, rb): keep this
            // iteration's reads ahead of those writes
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        };
        auto st_of = [&](int st) { return rsplit ? st : wv * nst + st; };
#pragma unroll 1
        for (int st = 0; st < nst; st++) {
            qi_v4i acc[4][3];
            int32_t y[16];
            if constexpr (VERIFY) {
                const uint32_t cb2 = static_cast<uint32_t>((col0 + 64 * st_of(st) + 16 * g) * 2);
                if (src.base1)  // (block-uniform)
                    verify_load16<true>(g0, g1, vrow, cb2, sv);
                else
                    verify_load16<false>(g0, g1, vrow, cb2, sv);
            }
            tile_mfma(st_of(st), acc);
            tile_y(acc, y);
            tile_fin(st_of(st), y);
        }
    };
    // Row blocks in ping-pong over two operand buffers, each prefetch one row
    // block ahead and unconditional (a clamped row block past the end).  On
    // gfx9 loads and stores share the in-order vmcnt: copying a prefetched
    // buffer (or a conditional prefetch) made the compiler drain vmcnt(0) at
    // every row block -- i.e. wait for all the previous block's streaming
    // stores before the next MFMA could issue.
    if (single) {
        // one row block for this wave (every decode up to k = 64): its
        // operands were loaded before the row loads, nothing to prefetch
        if (rb0 < RB)
            rb_body(rb0, bA, ktA, rsA, prA);
    } else {
        for (int rb = rb0; rb < RB; rb += 2 * rbs) {
            load_ops(min(rb + rbs, rlast), bB, ktB, rsB, prB);
            rb_body(rb, bA, ktA, rsA, prA);
            if (rb + rbs >= RB)
                break;
            load_ops(min(rb + 2 * rbs, rlast), bA, ktA, rsA, prA);
            rb_body(rb + rbs, bB, ktB, rsB, prB);
        }
    }
    if (sc.slow) {
        // rare (block-uniform): more marks than the LDS list held; this
        // block redoes its columns once its stores are done, with the image
        // as scratch (kin x 136 bytes <= the image)
        drain_block_stores();
        redo_columns<64 * NW, MODE>(a, s, col0, col1, reinterpret_cast<uint16_t*>(qi_lds),
                              reinterpret_cast<uint32_t*>(qi_lds + kin * 2 * kRedoCols),
                              reinterpret_cast<uint32_t*>(qi_lds + kin * (2 * kRedoCols + 8)), 0, 1,
                              v);
    }
