// Body of a kernel of kernels.hip, included once per form: MODE (a
// constexpr MatMode set by the including kernel, next to its VerArgs v)
// selects the plain form, the form for input and output marks in one launch
// (BOTH: a repair) or the verify form (VERIFY: a repair that compares with
// the stored row instead of storing); in the plain form the text is the
// kernel as it was before the others existed.  Not a stand-alone header.
    [[maybe_unused]] constexpr bool BOTH = MODE != MatMode::kPlain,
                                    VERIFY = MODE == MatMode::kVerify;
    constexpr int NCH = OsK<KS>::NCH, KC = OsK<KS>::KC;
    using O = OsTile<KC, WR>;  // one chunk's image (the whole K when NCH = 1)
    constexpr int KH = O::kRows, RSB = O::kPitch, RPT = O::kRpt, NCOL = O::kCols;
    static_assert(KS % 4 == 0 && KC % 4 == 0, "x64 pairs with zero halves");
    static_assert(NCH == 1 || RPW == 1, "K chunks: one row block per wave");
    extern __shared__ __attribute__((aligned(16))) uint8_t qi_lds[];
    const MatLayout L = a.L;
    const RowSrc src = a.src;
    const RowDst dst = a.dst;
    const MatExt ext = a.ext;
    const Oor in_oor = a.in_oor;
    const Oor out_oor = a.out_oor;
    const int kin = L.kin;
    const int tid = threadIdx.x, wv = tid >> 6, l = tid & 63;
    const int g = l >> 4, q = (l & 15) >> 1, p = l & 1, tl = l & 15;

    // block -> (stripe, row-block group, column range); every block of one
    // stripe on the same XCD (block b runs on XCD b % 8), consecutive in its
    // dispatch order, when the stripes tile the 8 XCDs: the stripe's context
    // tiles (256 KB per stripe at k = 256, 4 KiB packets: a quarter of its
    // data bytes) and the input tiles its G groups share are read from HBM
    // once and hit that XCD's L2 after (round 6: the C column ranges had
    // landed on different XCDs, k256 decode reads 1.23x algorithmic);
    // otherwise the G groups of one (stripe, range) on one XCD
    int s, gq, cr;
    {
        const int L0 = blockIdx.x;
        int unit;
        const int S = static_cast<int>(gridDim.x) / (G * C);
        if ((S & 7) == 0) {
            const int x = L0 & 7, j = L0 >> 3, per = G * C;
            const int sg = j / per, rem = j - sg * per;
            s = sg * 8 + x;
            cr = rem / G;
            gq = rem - cr * G;
            unit = s * C + cr;
        } else if (((S * C) & 7) == 0) {
            const int x = L0 & 7, j = L0 >> 3;
            gq = j % G;
            unit = (j / G) * 8 + x;
        } else {
            gq = L0 % G;
            unit = L0 / G;
        }
        s = unit / C;
        cr = unit - s * C;
    }
    const int t0 = static_cast<int>(static_cast<long long>(cr) * TS / C);
    const int t1 = static_cast<int>(static_cast<long long>(cr + 1) * TS / C);
    // one bit per tile of the block (<= kOsMaxTiles, os_launch), behind the
    // other LDS sections; cleared before the first mark scan's barrier
    uint32_t* slow_bits = reinterpret_cast<uint32_t*>(qi_lds + O::kLds);
    for (int wd = tid; wd <= (t1 - t0 - 1) >> 5; wd += 512)
        slow_bits[wd] = 0u;

    const int RB = L.RB();
    const int slot = wv % WR, st = wv / WR;  // row-block slot, super tile
    const int32_t* M = a.mat + s * a.ms;
    const int32_t* mf = M + L.mf();
    const int32_t* kmf = M + L.kmf();
    const int32_t* rscale = M + L.rscale_mf();
    const int32_t* __restrict__ rowmap = a.rowmap;
    const int32_t* sid = a.ids ? a.ids + s * a.is : nullptr;

    // this wave's row blocks and their operand tiles, for the block's whole
    // life: [a|0] over the h' K-steps, [0|b] over the l' K-steps (x64
    // pairs); [b|a] over the h' half is b1 and over the l' half b0, lane for
    // lane (see matrix_mfma_kernel's load_ops), so it is neither stored in
    // the context nor held twice
    int rbj[RPW];
    bool act[RPW];
    qi_v4i b0[RPW][KS / 4], b1[RPW][KS / 4];
    int32_t kt[RPW], rs[RPW], pr[RPW][3];
    // VERIFY: this lane's stored row per row block, and its 16 columns of
    // the tile in hand (loaded ahead of the tile's MFMAs)
    [[maybe_unused]] VerRow vrow[RPW];
    [[maybe_unused]] qi_v4u sv[2];
#pragma unroll
    for (int j = 0; j < RPW; j++) {
        // row blocks dealt round-robin over the G groups (their counts
        // differ by at most one): a group with fewer busy waves ran ahead of
        // the others, and the input tiles it had fetched were evicted from
        // L2 before they came by (k300: 1.88x the input bytes read)
        const int rb = gq + G * (slot + WR * j);
        act[j] = rb < RB;  // wave-uniform
        const int rbc = act[j] ? rb : RB - 1;
        rbj[j] = rbc;
        auto ld2 = [&](int ks, int ty) {
            return *reinterpret_cast<const qi_v2i*>(mf + ((rbc * KS + ks) * 3 + ty) * 128 + l * 2);
        };
#pragma unroll
        for (int i = 0; i < KS / 4; i++) {
            const qi_v2i x0 = ld2(2 * i, 0), x1 = ld2(2 * i + 1, 0);
            b0[j][i] = qi_v4i{x0.x, x0.y, x1.x, x1.y};
            const qi_v2i y0 = ld2(KS / 2 + 2 * i, 1), y1 = ld2(KS / 2 + 2 * i + 1, 1);
            b1[j][i] = qi_v4i{y0.x, y0.y, y1.x, y1.y};
        }
        const int t = 16 * rbc + tl;
        const int tcl = t < L.R ? t : L.R - 1;
        const int32_t k0 = kmf[tcl], r0 = rscale[tcl];
        kt[j] = t < L.R ? k0 : 0;
        rs[j] = t < L.R ? r0 : 1;
        pr[j][0] = rowmap[tcl];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int ot = 16 * rbc + 8 * h + (l >> 3);
            pr[j][1 + h] = rowmap[ot < L.R ? ot : L.R - 1];
        }
        if constexpr (VERIFY)
            vrow[j] = verify_row(v, src, s, L.R, act[j] ? t : L.R);
    }

    // staging: lane (rowgrp, cl) loads 4 columns (b64) of rows kRpp r +
    // rowgrp; per-lane row offsets fixed for the block (rows past kin
    // clamped: their operand bytes are 0); chunk c stages the received rows
    // KH c .. KH c + KH - 1.
    //   TWO (two source regions, the systematic decodes): one offset per
    // row, in its own region.  The context lists the received rows region by
    // region (order_ids, ctx.hip), so a wave's load of pass (c, r) reads one
    // region, through that region's descriptor (bit c RPT + r of sel), but
    // for at most one pass (xcr) that straddles the boundary: its region-1
    // lanes take an extra load (wx, one per item, past the extent in every
    // other item: zeros), ORed into that row when it is written to LDS.
    // (Each row loaded through both descriptors, past the extent in the
    // other region, took the k600 systematic decode 1.11 -> 1.92 ms:
    // twice the load instructions, gpurun_out/r6l.)
    const Region<true> g0(src.base0 + s * src.ss0, ext.e0);
    const Region<true> g1(src.base1 ? src.base1 + s * src.ss1 : src.base0, ext.e1);
    const Region<true> go(dst.base + s * dst.ss, ext.eo);
    const int rowgrp = tid / O::kTpr, cl = (tid % O::kTpr) * 4;
    constexpr uint32_t kOob = 0x80000000u;  // past any extent (< 2^31)
    static_assert(NCH * RPT <= 32, "pass bits");
    uint32_t off0[NCH][RPT];
    uint32_t sel = 0, offx = kOob;  // sel: wave-uniform
    int xcr = -1;                   // wave-uniform: c RPT + r of the straddling pass
#pragma unroll
    for (int c = 0; c < NCH; c++)
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            const int i = KH * c + O::kRpp * r + rowgrp;
            const int ii = i < kin ? i : kin - 1;
            const int id = src.by_pos ? ii : (sid ? sid[ii] : ii);
            const uint32_t lane = static_cast<uint32_t>(cl * 2);
            if constexpr (TWO) {
                const bool lo = id < src.split;
                off0[c][r] = (lo ? static_cast<uint32_t>(id * src.rs0 * 2)
                                 : static_cast<uint32_t>((id - src.split) * src.rs1 * 2)) +
                             lane;
                const uint64_t b1 = __ballot(!lo);
                if (b1 == ~0ull) {
                    sel |= 1u << (c * RPT + r);
                } else if (b1 != 0ull) {
                    if (xcr >= 0 && a.err && l == 0)
                        atomicOr(a.err, kErrBadIds);  // rows not in region order
                    xcr = c * RPT + r;
                    offx = lo ? kOob : off0[c][r];
                }
            } else {
                off0[c][r] = static_cast<uint32_t>(id * src.rs0 * 2) + lane;
            }
        }
    sel = __builtin_amdgcn_readfirstlane(sel);
    xcr = __builtin_amdgcn_readfirstlane(xcr);
    const int xc = xcr >= 0 ? xcr / RPT : -1, xr = xcr >= 0 ? xcr % RPT : -1;
    // DEEP (KS = 4, the short decodes): ND tiles of rows in flight per
    // block (a ring of ND register sets, 8 VGPRs each) -- with one, a CU
    // kept ~32 KB of loads in flight and the cfg3 decode was bound by the
    // load latency; three measured the same as two, four slower (125 / 133
    // VGPRs: cfg3 decode 0.143 / 0.168 ms, profiles/r5_ab_notes.txt)
    constexpr int ND = KS == 4 ? 2 : 1;
    constexpr bool DEEP = ND >= 2;
    uint32_t w[RPT][2], wring[DEEP ? ND : 1][DEEP ? RPT : 1][2];
    uint32_t wx[2], wxring[DEEP ? ND : 1][2];  // TWO: the straddling pass's region-1 lanes
    // rows of `tile` into wr; an invalid tile (past the block's range) loads
    // from past the buffer's extent (no memory access, zeros), so the number
    // of loads in flight is the same on every path
    auto issue_rows_to = [&](int tile, bool valid, auto& wr, auto& wxr, auto cc) {
        constexpr int c = decltype(cc)::value;  // K chunk
        const int so = valid ? tile * NCOL * 2 : 0;  // byte offset of the tile's first column
        const uint32_t oob = valid ? 0u : kOob;
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            uint32_t o = off0[c][r] | oob;
            auto rsrc = g0.r;
            if constexpr (TWO) {
                // (the straddling pass: its region-1 lanes through wx)
                o = c * RPT + r == xcr && offx != kOob ? kOob : o;
                rsrc = (sel >> (c * RPT + r)) & 1u ? g1.r : g0.r;
            }
            const auto v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, static_cast<int>(o), so,
                                                                kAuxLdOs);
            wr[r][0] = v[0];
            wr[r][1] = v[1];
        }
        if constexpr (TWO) {
            const auto u = __builtin_amdgcn_raw_buffer_load_b64(
                g1.r, static_cast<int>(c == xc ? offx | oob : kOob), so, kAuxLdOs);
            wxr[0] = u[0];
            wxr[1] = u[1];
        }
    };
    using C0 = std::integral_constant<int, 0>;
    auto issue_rows = [&](int tile, auto cc) { issue_rows_to(tile, true, w, wx, cc); };
    const uint32_t lpos = 64 * (cl / 64) + 16 * ((cl % 16) / 4) + 4 * ((cl % 64) / 16);
    auto write_rows_from = [&](uint8_t* img, const auto& w, const auto& wxr) {
#pragma unroll
        for (int r = 0; r < RPT; r++) {
            const int i = O::kRpp * r + rowgrp;
            uint32_t w0 = w[r][0], w1 = w[r][1];
            if constexpr (TWO) {
                // (zeros unless this item's chunk holds the straddling pass)
                w0 |= r == xr ? wxr[0] : 0u;
                w1 |= r == xr ? wxr[1] : 0u;
            }
            const uint32_t hi = __builtin_amdgcn_perm(w1, w0, 0x07050301u) ^ 0x80808080u;
            const uint32_t lo = __builtin_amdgcn_perm(w1, w0, 0x06040200u) ^ 0x80808080u;
            *reinterpret_cast<uint32_t*>(img + i * RSB + lpos) = hi;
            *reinterpret_cast<uint32_t*>(img + (KH + i) * RSB + lpos) = lo;
        }
    };
    auto write_rows = [&](uint8_t* img) { write_rows_from(img, w, wx); };

    // OOR marks of the received rows in a tile (route table or bucket
    // scan) into mark list mb; returns the count (all threads)
    auto s_i = [&](int mb) {
        return reinterpret_cast<int*>(qi_lds + O::kMarkOff) + mb * 2 * kMaxTileOor;
    };
    auto s_col = [&](int mb) { return reinterpret_cast<uint32_t*>(s_i(mb) + kMaxTileOor); };
    auto s_cnt = [&](int mb) {
        return reinterpret_cast<int*>(qi_lds + O::kMarkOff + 2 * 2 * 4 * kMaxTileOor) + mb;
    };
    const bool marks_in = in_oor.counts != nullptr;
    // the route-table list each mark buffer holds (block-uniform): the tiles
    // of one kRouteTile-column route tile share its list (the epilogue keeps
    // the marks in its own columns), so a buffer that already holds it is not
    // staged again.  (Staging it every tile cost the cfg3 decode ~8 us: the
    // wait for the scalar load also drained the LDS accesses in flight,
    // tools/ab/probe_os_nomarks.patch)
    // (not at KS = 8, whose kernel measured faster staging every tile from
    // scalar loads: k128 decode 1.5 %)
    constexpr bool kOnce = KS != 8;
    int srt0 = -1, srt1 = -1, scnt0 = 0, scnt1 = 0;
    auto stage_marks = [&](int tile, int mb) -> int {
        if (!marks_in)
            return 0;
        const long long col0 = static_cast<long long>(tile) * NCOL;
        if (a.route) {
            const int rti = static_cast<int>(col0 / kRouteTile);
            if (kOnce && (mb ? srt1 : srt0) == rti)
                return mb ? scnt1 : scnt0;
            const int rc = stage_route_marks_s<kOnce>(
                a.route + s * a.rstride + static_cast<long long>(rti) * kRouteStride, col0,
                s_i(mb), s_col(mb));
            if (rc >= 0) {
                if constexpr (kOnce) {
                    if (mb) {
                        srt1 = rti;
                        scnt1 = rc;
                    } else {
                        srt0 = rti;
                        scnt0 = rc;
                    }
                }
                return rc;
            }
        }
        if constexpr (kOnce) {
            if (mb)  // this buffer now holds a bucket scan of one tile
                srt1 = -1;
            else
                srt0 = -1;
        }
        OorScan sc{in_oor, sid, src.by_pos, a.slot_base, kin, s, false};
        const int cnt = scan_tile_marks(sc, col0, col0 + NCOL, a.words, s_cnt(mb), s_i(mb),
                                        s_col(mb), a.err);
        if (cnt > kMaxTileOor && tid == 0)  // rare: redone at the block's end
            atomicOr(&slow_bits[(tile - t0) >> 5], 1u << ((tile - t0) & 31));
        return min(cnt, kMaxTileOor);
    };
    // the block's slow tiles (bits over [t0, t1)), redone by the block once
    // its stores are done, with the images as scratch
    auto finish = [&]() {
        if (!marks_in)
            return;
        bool any = false;
        for (int wd = 0; wd <= (t1 - t0 - 1) >> 5; wd++)
            any |= slow_bits[wd] != 0u;
        if (!any)
            return;  // block-uniform
        drain_block_stores();
        for (int wd = 0; wd <= (t1 - t0 - 1) >> 5; wd++) {
            uint32_t bits = slow_bits[wd];
            while (bits) {
                const int tile = t0 + 32 * wd + __builtin_ctz(bits);
                bits &= bits - 1;
                const long long c0 = static_cast<long long>(tile) * NCOL;
                // this group's row blocks only: the G blocks of a column
                // range each redo (and earlier stored) disjoint rows
                redo_columns<512, MODE>(a, s, c0, c0 + NCOL, reinterpret_cast<uint16_t*>(qi_lds),
                                  reinterpret_cast<uint32_t*>(qi_lds + kin * 2 * kRedoCols),
                                  reinterpret_cast<uint32_t*>(qi_lds + kin * (2 * kRedoCols + 8)),
                                  gq, G, v);
            }
        }
    };

    const bool rec = out_oor.counts != nullptr;
    const uint32_t ors = static_cast<uint32_t>(dst.rs * 2);
    const uint32_t abase = static_cast<uint32_t>((8 * g + q) * RSB + 8 * p + 64 * st);
    uint8_t* stg = qi_lds + O::kStageOff + wv * O::kStage;

    // row block j of this wave over its super tile (columns col0 ..
    // col0 + 63) from image img
    // row block j's accumulators: D0 = 0, D1 = kmf (the byte offsets'
    // correction), D2 = 0
    auto init_acc = [&](qi_v4i (&acc)[4][3], auto jc) {
        constexpr int j = decltype(jc)::value;
#pragma unroll
        for (int T = 0; T < 4; T++) {
            acc[T][0] = qi_v4i{0, 0, 0, 0};
            acc[T][1] = qi_v4i{kt[j], kt[j], kt[j], kt[j]};
            acc[T][2] = qi_v4i{0, 0, 0, 0};
        }
    };
    // K chunk cc of row block j over this wave's super tile of image img,
    // accumulated into acc: the chunk's h' half of K (its pairs: [a|0] and
    // [b|a]), then its l' half ([0|b] and [b|a]), KC / 4 A pairs live at a
    // time; operand pair c KC / 4 + i of the row block's registers
    auto mma = [&](const uint8_t* img, qi_v4i (&acc)[4][3], auto jc, auto cc) {
        constexpr int j = decltype(jc)::value, c = decltype(cc)::value;
        auto* lds = (__attribute__((address_space(3))) const uint8_t*)img;
#pragma unroll
        for (int T = 0; T < 4; T++) {
#pragma unroll
            for (int hf = 0; hf < 2; hf++) {
                qi_v4i av[KC / 4];
#pragma unroll
                for (int i = 0; i < KC / 4; i++) {
                    auto rd = [&](int ks) {
                        auto* pa = (__attribute__((address_space(3))) qi_v2i*)(
                            lds + abase + 32 * ks * RSB + T * 16);
                        return __builtin_amdgcn_ds_read_tr8_b64_v2i32(pa);
                    };
                    const int pi = hf * (KC / 4) + i;
                    const qi_v2i x0 = rd(2 * pi), x1 = rd(2 * pi + 1);
                    av[i] = qi_v4i{x0.x, x0.y, x1.x, x1.y};
                }
#pragma unroll
                for (int i = 0; i < KC / 4; i++) {
                    constexpr int o = c * (KC / 4);
                    if (hf == 0)
                        acc[T][0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[i], b0[j][o + i],
                                                                          acc[T][0], 0, 0, 0);
                    else
                        acc[T][1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[i], b1[j][o + i],
                                                                          acc[T][1], 0, 0, 0);
                    acc[T][2] = __builtin_amdgcn_mfma_i32_16x16x64_i8(
                        av[i], hf == 0 ? b1[j][o + i] : b0[j][o + i], acc[T][2], 0, 0, 0);
                }
            }
        }
    };
    auto epilogue = [&](const qi_v4i (&acc)[4][3], long long col0, int n_lm, const int* mi,
                        const uint32_t* mc, auto jc, auto&& before_stores) {
        constexpr int j = decltype(jc)::value;
        const int t = 16 * rbj[j] + tl;
        const bool trow = act[j] && t < L.R;
        // epilogue: lane (g, t) holds row t, columns cb .. cb + 15
        const long long cb = col0 + 16 * g;
        int32_t y[16];
#pragma unroll
        for (int T = 0; T < 4; T++)
#pragma unroll
            for (int jj = 0; jj < 4; jj++)
                y[4 * T + jj] =
                    fold(fold(((KS >= 16 ? fold(acc[T][2][jj]) : acc[T][2][jj]) << 8) +
                              acc[T][1][jj] - acc[T][0][jj]));
        // restored OOR symbols of the received rows (decode_prepare,
        // src/fec_base.h:1361-1404): 65536 == -1 where the stored word is 0
        const uint32_t st0 = static_cast<uint32_t>(col0);
        for (int e = 0; e < n_lm; e++) {
            const uint32_t wcu = __builtin_amdgcn_readfirstlane(mc[e]);
            if (wcu - st0 >= 64u)
                continue;
            const int pos = __builtin_amdgcn_readfirstlane(mi[e]);
            const long long d = static_cast<long long>(wcu) - cb;
            // the coefficient from the wave's own operand tiles (no memory
            // load: waiting for one drained the stores and the prefetch)
            const int32_t corr = coef_from_tiles<KS>(
                [&](int idx) {
                    // [b | a]'s dword idx: b1 over the h' pairs, b0 over the l'
                    return idx < KS ? pick_v4(b1[j], idx) : pick_v4(b0[j], idx - KS);
                },
                pos, l);
#pragma unroll
            for (int c = 0; c < 16; c++) {
                const int32_t yc = fold(fold(y[c] - corr));
                y[c] = (trow && d == c) ? yc : y[c];
            }
        }
        if (__builtin_amdgcn_ballot_w64(rs[j] != 1)) {
#pragma unroll
            for (int c = 0; c < 16; c++)
                y[c] = fold(fold(mul_rs(y[c], rs[j])));
        }
        uint32_t bad = 0;
#pragma unroll
        for (int c = 0; c < 16; c++)
            bad |= static_cast<uint32_t>(y[c]);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64((bad >> 16) != 0) != 0, 0)) {
#pragma unroll
            for (int c = 0; c < 16; c++) {
                if (static_cast<uint32_t>(y[c]) > 65535u) {
                    bool rnow = rec && trow;
                    if constexpr (BOTH) {
                        // a slow tile records its output marks in its redo
                        const int tb = static_cast<int>(col0 / NCOL) - t0;
                        rnow = rnow && !((slow_bits[tb >> 5] >> (tb & 31)) & 1u);
                    }
                    if (rnow)
                        record_oor(out_oor, s, pr[j][0], cb + c);
                    y[c] = 0;  // 65536 (or its alias -1) is stored as 0
                }
            }
        }
        if constexpr (VERIFY) {
            // compared where it lies (no transpose, no store); a slow tile is
            // counted by its redo
            const int tb = static_cast<int>(col0 / NCOL) - t0;
            verify_tile16(v, static_cast<long long>(s) * L.R + t, trow, y, sv, cb,
                          (slow_bits[tb >> 5] >> (tb & 31)) & 1u);
            if constexpr (j == RPW - 1)
                before_stores();
            return;
        }
        qi_v4u o0, o1;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            o0[c] = pack_lo(static_cast<uint32_t>(y[2 * c]), static_cast<uint32_t>(y[2 * c + 1]));
            o1[c] = pack_lo(static_cast<uint32_t>(y[8 + 2 * c]),
                            static_cast<uint32_t>(y[8 + 2 * c + 1]));
        }
        // transposed through the wave's staging tile into whole-line stores
        *reinterpret_cast<qi_v4u*>(stg + tl * O::kStagePitch + 32 * g) = o0;
        *reinterpret_cast<qi_v4u*>(stg + tl * O::kStagePitch + 32 * g + 16) = o1;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        qi_v4u v2[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int orow = 8 * h + (l >> 3), c = l & 7;
            v2[h] = *reinterpret_cast<const qi_v4u*>(stg + orow * O::kStagePitch + 16 * c);
        }
        if constexpr (j == RPW - 1)
            before_stores();
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int orow = 8 * h + (l >> 3), c = l & 7;
            const qi_v4u v = v2[h];
            const int ot = 16 * rbj[j] + orow;
            const uint32_t vo = (act[j] && ot < L.R)
                                    ? static_cast<uint32_t>(pr[j][1 + h]) * ors +
                                          static_cast<uint32_t>((col0 + 8 * c) * 2)
                                    : 0x80000000u;
            __builtin_amdgcn_raw_buffer_store_b128(v, go.r, static_cast<int>(vo), 0, kAuxStMf);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    // the whole K in one image (NCH = 1)
    auto compute = [&](const uint8_t* img, long long col0, int n_lm, const int* mi,
                       const uint32_t* mc, auto jc, auto&& before_stores) {
        qi_v4i acc[4][3];
        if constexpr (VERIFY)
            verify_load16<TWO>(g0, g1, vrow[decltype(jc)::value],
                               static_cast<uint32_t>((col0 + 16 * g) * 2), sv);
        init_acc(acc, jc);
        mma(img, acc, jc, C0{});
        epilogue(acc, col0, n_lm, mi, mc, jc, before_stores);
    };

    auto idle_stores = [&]() {
        if constexpr (VERIFY)
            return;  // (the verify forms store nothing)
#pragma unroll
        for (int h = 0; h < 2; h++)
            __builtin_amdgcn_raw_buffer_store_b128(qi_v4u{0u, 0u, 0u, 0u}, go.r,
                                                   static_cast<int>(0x80000000u + 16 * h), 0,
                                                   kAuxStMf);
    };

    if (t0 >= t1)
        return;
    auto img = [&](int b) { return qi_lds + b * O::kImg; };
    if constexpr (DEEP) {
        // tiles t0 .. t0 + ND - 1 in flight, the first one into image 0
#pragma unroll
        for (int d = 0; d < ND; d++)
            issue_rows_to(t0 + d, t0 + d < t1, wring[d], wxring[d], C0{});
        write_rows_from(img(0), wring[0], wxring[0]);
        int nl[2];
        nl[0] = stage_marks(t0, 0);
        nl[1] = 0;
        __syncthreads();
        // tile's rows are in image b; set J (tile's, already written) takes
        // tile + ND's, set J + 1 holds tile + 1's (in flight)
        auto body = [&](int tile, auto jc) {
            constexpr int J = decltype(jc)::value;
            const int b = (tile - t0) & 1;
            const bool more = tile + 1 < t1;  // block-uniform
            issue_rows_to(tile + ND, tile + ND < t1, wring[J], wxring[J], C0{});
            const long long col0 = static_cast<long long>(tile) * NCOL + 64 * st;
            auto none = [] {};
            [&]<int... R>(std::integer_sequence<int, R...>) {
                ((act[R] ? compute(img(b), col0, nl[b], s_i(b), s_col(b),
                                   std::integral_constant<int, R>{}, none)
                         : idle_stores()),
                 ...);
            }(std::make_integer_sequence<int, RPW>{});
            // unconditional, so every path waits for the next set's loads
            // here (a skipped write left them pending on one path, and the
            // compiler then drained vmcnt(0) before reusing the registers);
            // past the last tile it writes the invalid tile's zeros into an
            // image no wave reads again
            write_rows_from(img(b ^ 1), wring[(J + 1) % ND], wxring[(J + 1) % ND]);
            if (more)
                nl[b ^ 1] = stage_marks(tile + 1, b ^ 1);
            __syncthreads();
        };
#pragma unroll 1
        for (int tile = t0; tile < t1; tile += ND) {
            bool done = false;
            [&]<int... J>(std::integer_sequence<int, J...>) {
                ((done = done || tile + J >= t1, done ? void() : body(tile + J,
                                                                     std::integral_constant<int, J>{})),
                 ...);
            }(std::make_integer_sequence<int, ND>{});
            if (done)
                break;
        }
        finish();
        return;
    }
    issue_rows(t0, C0{});
    write_rows(img(0));
    int nl[2];
    nl[0] = stage_marks(t0, 0);
    nl[1] = 0;
    __syncthreads();
    if constexpr (NCH > 1) {
        // (tile, chunk) items, double-buffered: item q's rows in image q & 1
        // while item q + 1's are in flight; a tile's accumulators live over
        // its chunks, its epilogue (marks, stores) after the last one
        static_assert(NCH == 2, "two K chunks");
        constexpr bool rows_first = true;
        int ib = 0;
#pragma unroll 1
        for (int tile = t0; tile < t1; tile++) {
            const int mb = (tile - t0) & 1;
            const bool more = tile + 1 < t1;  // block-uniform
            const long long col0 = static_cast<long long>(tile) * NCOL + 64 * st;
            qi_v4i acc[4][3];
            using J0 = std::integral_constant<int, 0>;
            // chunk 0; chunk 1's rows in flight, staged right after
            issue_rows(tile, std::integral_constant<int, 1>{});
            init_acc(acc, J0{});
            if (act[0])
                mma(img(ib), acc, J0{}, C0{});
            write_rows(img(ib ^ 1));
            __syncthreads();
            ib ^= 1;
            // chunk 1, then the epilogue; the next tile's chunk 0 in flight
            if (more)
                issue_rows(tile + 1, C0{});
            if (act[0])
                mma(img(ib), acc, J0{}, std::integral_constant<int, 1>{});
            auto stage_next = [&]() {
                if (rows_first && more)
                    write_rows(img(ib ^ 1));
            };
            if (act[0])
                epilogue(acc, col0, nl[mb], s_i(mb), s_col(mb), J0{}, stage_next);
            else {
                stage_next();
                idle_stores();
            }
            if (more)
                nl[mb ^ 1] = stage_marks(tile + 1, mb ^ 1);
            __syncthreads();
            ib ^= 1;
        }
        finish();
        return;
    }
#pragma unroll 1
    for (int tile = t0; tile < t1; tile++) {
        const int b = (tile - t0) & 1;
        const bool more = tile + 1 < t1;  // block-uniform
        if (more)
            issue_rows(tile + 1, C0{});
        const long long col0 = static_cast<long long>(tile) * NCOL + 64 * st;
        // an idle wave (row block past RB) issues the same two stores, past
        // the buffer's extent (dropped): with the store count equal on both
        // sides of the branch, the compiler's vmcnt wait for the next tile's
        // rows stays behind them instead of draining this tile's stores
        // (vmcnt(0) on the merged path)
        // the next tile's rows go to LDS before this tile's stores issue: on
        // gfx9 loads and stores share vmcnt, so waiting for the rows after
        // the stores drained the stores too (the whole store latency per
        // tile); here the wait covers the rows (issued at the top of the
        // iteration) and the previous tile's stores
        // (KS >= 8: k128 encode 0.985 -> 0.917 ms, k200 0.70 -> 0.67 ms; the
        // short KS = 4 decodes keep the rows after the stores: cfg3 decode
        // 0.186 vs 0.192 ms, gpurun_out ab_ws)
        constexpr bool rows_first = KS >= 8;
        auto stage_next = [&]() {
            if (rows_first && more)
                write_rows(img(b ^ 1));
        };
        [&]<int... J>(std::integer_sequence<int, J...>) {
            ((act[J] ? compute(img(b), col0, nl[b], s_i(b), s_col(b),
                               std::integral_constant<int, J>{}, stage_next)
                     : (J == RPW - 1 ? (stage_next(), idle_stores()) : idle_stores())),
             ...);
        }(std::make_integer_sequence<int, RPW>{});
        if (!rows_first && more)
            write_rows(img(b ^ 1));
        if (more)
            nl[b ^ 1] = stage_marks(tile + 1, b ^ 1);
        __syncthreads();
    }
    finish();
