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
    const SlowList slow = a.slow;
    uint32_t* err = a.err;
    __shared__ int s_cnt;
    __shared__ int s_i[kMaxTileOor];
    __shared__ uint32_t s_col[kMaxTileOor];

    int s, tile;
    block_map(blockIdx.x, tiles, s, tile);
    const int kin = L.kin;
    const long long col0 = ext.c0 + static_cast<long long>(tile) * kBlock * COLS;
    const long long col1 = col0 + kBlock * COLS;
    const long long col = col0 + static_cast<long long>(threadIdx.x) * COLS;
    const uint32_t voff = static_cast<uint32_t>(col * 2);
    const int32_t* M = mat + s * mat_stride;
    // fragment ids as dwords (scalar loads; a u16 array would need vector
    // loads + readfirstlane, draining vmcnt between the row loads)
    const int32_t* sid = ids ? ids + s * ids_stride : nullptr;
    const bool full = col1 <= words;  // block-uniform
    const Region<BUF> g0(src.base0 + s * src.ss0, ext.e0);
    const Region<BUF> g1(src.base1 ? src.base1 + s * src.ss1 : src.base0,
                         ext.e1);
    const Region<BUF> go(dst.base + s * dst.ss, ext.eo);

    // the OOR marks of the received rows in this tile (decode_prepare,
    // src/fec_base.h:1361-1404): from the context's route table (scalar
    // loads, issued with the row loads), or -- when the table overflowed or
    // is absent -- by scanning the OOR buckets
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

    // source row of input i: its position (by_pos) or its fragment id; rows
    // past kin are clamped to a valid row (their coefficients are 0).
    // KP <= 32: all ids up front in SGPRs (2*KP dwords, the context pads
    // past kin), so the scalar loads batch into a few s_load_dwordxN.
    // KP >= 64 (the column tails of k > 64): 128-256 ids do not fit the
    // SGPRs (they spilled to VGPR lanes and scratch), so lane c of
    // idl[i / 64] holds id i and the row loads read it with v_readlane.
    // (VERIFY: from KP = 32 on -- its row addressing needs the SGPRs the 64
    // ids took, and the flat form spilled to scratch)
    constexpr int kIdLanes = VERIFY ? 32 : 64;
    constexpr int NIL = KP >= kIdLanes ? (2 * KP + 63) / 64 : 1;
    constexpr int NIV = KP >= kIdLanes ? 1 : 2 * KP;
    int idl[NIL];
    int idv[NIV];
    if constexpr (KP >= kIdLanes) {
        const int ln = static_cast<int>(threadIdx.x & 63);
#pragma unroll
        for (int c = 0; c < NIL; c++) {
            const int i = 64 * c + ln;
            const int ii = i < kin ? i : kin - 1;
            idl[c] = src.by_pos ? ii : (sid ? sid[i < kin ? i : 0] : (i < kin ? i : 0));
        }
        (void)idv;
    } else {
        (void)idl;
        if (sid) {
#pragma unroll
            for (int i = 0; i < 2 * KP; i++)
                idv[i] = sid[i];
        } else {
#pragma unroll
            for (int i = 0; i < 2 * KP; i++)
                idv[i] = i;
        }
#pragma unroll
        for (int i = 0; i < 2 * KP; i++) {
            const int ii = i < kin ? i : kin - 1;
            idv[i] = src.by_pos ? ii : (i < kin ? idv[i] : idv[0]);
        }
    }
    auto id_of = [&](int i) {
        if constexpr (KP >= kIdLanes)
            return __builtin_amdgcn_readlane(idl[i / 64], i % 64);
        else
            return idv[i];
    };
    int32_t xp[COLS][KP];
    if (full) {
        matrix_load<KP, COLS, true, BUF>(id_of, src, g0, g1, voff, COLS, xp);
    } else if (col < words) {
        matrix_load<KP, COLS, false, BUF>(id_of, src, g0, g1, voff,
                                          words - col, xp);
    }
    OorScan sc{in_oor, sid, src.by_pos, slot_base, kin, s, false};
    int n_lm = 0;
    if (scan) {  // block-uniform
        const int cnt = scan_tile_marks(sc, col0, col1, words, &s_cnt, s_i, s_col, err);
        sc.slow = cnt > kMaxTileOor;
        n_lm = min(cnt, kMaxTileOor);
    } else if (n_rm > 0) {  // block-uniform: the routed marks into the same list
        stage_route_marks(rm, n_rm, col0, s_i, s_col);
        __syncthreads();
        n_lm = n_rm;
    }
    const roff_t<BUF> ors = static_cast<roff_t<BUF>>(dst.rs * 2);
    if constexpr (BOTH) {
        // a slow tile records no output marks here, matrix_redo_kernel_both
        // does, from fully restored inputs (block-uniform)
        const Oor out_rec = sc.slow ? Oor{nullptr, nullptr, 0, 0} : out_oor;
        if constexpr (VERIFY) {
            // the same, comparing with the stored rows (a slow tile is
            // counted by the redo alone)
            const VerRows<BUF> vrows{v, src, g0, g1, sc.slow};
            if (full) {
                matrix_compute_verify<KP, COLS, true, BUF>(L, M, xp, go, ors, voff, col, col0,
                                                           COLS, s, n_lm, s_i, s_col, out_rec,
                                                           a.rowmap, &vrows);
            } else if (col < words) {
                matrix_compute_verify<KP, COLS, false, BUF>(L, M, xp, go, ors, voff, col, col0,
                                                            words - col, s, n_lm, s_i, s_col,
                                                            out_rec, a.rowmap, &vrows);
            }
        } else if (full) {
            matrix_compute<KP, COLS, true, BUF>(L, M, xp, go, ors, voff, col, col0, COLS, s,
                                                n_lm, s_i, s_col, out_rec, a.rowmap);
        } else if (col < words) {
            matrix_compute<KP, COLS, false, BUF>(L, M, xp, go, ors, voff, col, col0,
                                                 words - col, s, n_lm, s_i, s_col, out_rec,
                                                 a.rowmap);
        }
    } else if (full) {
        matrix_compute<KP, COLS, true, BUF>(L, M, xp, go, ors, voff, col, col0,
                                            COLS, s, n_lm, s_i, s_col, out_oor,
                                            a.rowmap);
    } else if (col < words) {
        matrix_compute<KP, COLS, false, BUF>(L, M, xp, go, ors, voff, col, col0,
                                             words - col, s, n_lm, s_i, s_col,
                                             out_oor, a.rowmap);
    }
    if (sc.slow && threadIdx.x == 0)  // rare: see matrix_redo_kernel
        push_slow_tile(slow, s, col0, kBlock * COLS);
