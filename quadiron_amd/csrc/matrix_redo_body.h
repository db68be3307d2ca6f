// Body of a kernel of kernels.hip, included once per form: MODE (a
// constexpr MatMode set by the including kernel, next to its VerArgs v)
// selects the plain form, the form for input and output marks in one launch
// (BOTH: a repair) or the verify form (VERIFY: a repair that compares with
// the stored row instead of storing); in the plain form the text is the
// kernel as it was before the others existed.  Not a stand-alone header.
    [[maybe_unused]] constexpr bool BOTH = MODE != MatMode::kPlain,
                                    VERIFY = MODE == MatMode::kVerify;
    // (the dot2 tails' slow tiles: k <= 256; the operand-stationary kernel
    // redoes its own in its dynamic LDS)
    __shared__ uint16_t xs[kMatGenMaxKin * kRedoCols];  // [input i][column]
    __shared__ uint32_t mk[kMatGenMaxKin * (kRedoCols / 32)];
    __shared__ uint32_t colmk[kRedoCols / 32];
    const int tid = threadIdx.x, c = tid & 63, wv = tid >> 6;
    // this block's stripes with a non-empty list (wave 0, one lane each;
    // broadcast to the block through LDS)
    __shared__ uint64_t todo;
    const int s0 = blockIdx.x * kRedoSpan;
    if (wv == 0) {
        const int sl = s0 + c;
        const uint32_t nl = sl < n_stripes
                                ? __hip_atomic_load(a.slow.base + sl * a.slow.stride,
                                                    __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                : 0u;
        const uint64_t m = __builtin_amdgcn_ballot_w64(nl != 0);
        if (c == 0)
            todo = m;
    }
    __syncthreads();
    uint64_t pend = todo;
    while (pend) {
        const int s = s0 + __builtin_ctzll(pend);  // block-uniform
        pend &= pend - 1;
        uint32_t* l = a.slow.base + s * a.slow.stride;
        const uint32_t n = *l;
        for (uint32_t e = 0; e < n; e++) {
            const uint32_t code = l[1 + e];
            const long long t0 = static_cast<long long>(code >> 3) * kSlowGrain;
            const long long t1 = min(t0 + (static_cast<long long>(kSlowGrain) << (code & 7)),
                                     a.words);
            redo_columns<kBlock, MODE>(a, s, t0, t1, xs, mk, colmk, 0, 1, v);
        }
        __syncthreads();
        if (tid == 0)
            *l = 0;
    }
