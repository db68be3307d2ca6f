"""quadiron_amd -- MI355X-native RS-FNT erasure coding (Reed-Solomon over
GF(65537) via the Fermat Number Transform), a drop-in for QuadIron's RS-FNT
path.

The product is the native library ``quadiron_amd/libquadiron_amd.so`` (HIP
kernels for gfx950 + C++ host layer) exporting:

* the drop-in C-ABI ``quadiron_fnt32_*`` (include/quadiron_c.h),
* the device-level C-ABI ``qi_plan_* / qi_gpu_*`` (include/qi_gpu.h),
* the C view of the block API ``qi_fec_*`` (include/qi_gpu.h).

This module only loads it with ctypes and wraps those entry points for
Python callers (tests, bench).  There is no Python or CPU compute path: if
the library or a HIP device is missing, calls fail loudly.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# QI_LIB_PATH: load another build of the same library (A/B timing of kernel
# variants built by tools/ab_build.sh); the default is the in-tree product
LIB_PATH = os.environ.get("QI_LIB_PATH") or os.path.join(HERE,
                                                         "libquadiron_amd.so")

_lib = None

c_u8p = C.POINTER(C.c_uint8)
c_u8pp = C.POINTER(c_u8p)


def _declare(lib):
    V, I, LL, SZ, U32 = C.c_void_p, C.c_int, C.c_longlong, C.c_size_t, C.c_uint32
    sig = {
        # include/quadiron_c.h
        "quadiron_fnt32_new": (V, [I, I, I, I]),
        "quadiron_fnt32_delete": (None, [V]),
        "quadiron_fnt32_get_metadata_size": (I, [V, SZ]),
        "quadiron_fnt32_encode": (I, [V, c_u8pp, c_u8pp, V, SZ]),
        "quadiron_fnt32_decode": (I, [V, c_u8pp, c_u8pp, V, SZ]),
        "quadiron_fnt32_reconstruct": (I, [V, c_u8pp, c_u8pp, V, C.c_uint, SZ]),
        "quadiron_hex_dump": (None, [V, SZ]),
        # include/qi_gpu.h
        "qi_gpu_device_count": (I, []),
        "qi_plan_create": (V, [I, I, I]),
        "qi_plan_create_ex": (V, [I, I, I, I]),
        "qi_plan_destroy": (None, [V]),
        "qi_plan_n": (I, [V]),
        "qi_plan_n_outputs": (I, [V]),
        "qi_gpu_oor_clear": (I, [V, SZ, V]),
        "qi_gpu_encode": (I, [V, V, LL, LL, V, LL, LL, LL, I, V, V, I, V]),
        "qi_gpu_decode_ctx_bytes": (SZ, [V, I, LL]),
        "qi_gpu_decode_ctx": (I, [V, V, V, I, V, V, I, LL, V, V]),
        "qi_gpu_decode": (I, [V, V, V, V, LL, LL, V, LL, LL, V, V, I, V, LL,
                              LL, LL, I, V]),
        "qi_gpu_decode_ctx_packed": (I, [V, V, V, I, V, V, I, LL, V, V]),
        "qi_gpu_decode_packed": (I, [V, V, V, LL, LL, V, V, I, V, LL, LL, LL,
                                     I, V]),
        "qi_gpu_repair_ctx_bytes": (SZ, [V, I, I, LL]),
        "qi_gpu_repair_ctx": (I, [V, V, V, I, I, V, V, I, LL, V, V]),
        "qi_gpu_repair": (I, [V, V, I, V, LL, LL, V, LL, LL, V, V, I, V, LL,
                              LL, V, V, I, LL, I, V]),
        "qi_gpu_repair_kernels": (C.c_char_p, [V, I, LL]),
        "qi_gpu_verify_work_bytes": (SZ, [V, I, I, I]),
        "qi_gpu_verify": (I, [V, V, I, V, V, LL, LL, V, LL, LL, V, V, I, V, I,
                              V, V, V, LL, I, V]),
        "qi_gpu_verify_kernels": (C.c_char_p, [V, I, LL]),
        "qi_gpu_update_ctx_bytes": (SZ, [V, I, I, I]),
        "qi_gpu_update_ctx": (I, [V, V, V, I, I, I, V, V]),
        "qi_gpu_update": (I, [V, V, I, I, V, LL, LL, V, LL, LL, V, LL, LL, V, V, I,
                              V, LL, LL, V, V, I, LL, I, V]),
        "qi_gpu_update_kernels": (C.c_char_p, [V, I, I, LL]),
        "qi_gpu_locate_ctx_bytes": (SZ, [V, I, I]),
        "qi_gpu_locate_ctx": (I, [V, V, I, I, V, V]),
        "qi_gpu_locate": (I, [V, V, I, V, V, LL, LL, V, LL, LL, V, V, I, V, V, V, V, I,
                              LL, I, V]),
        "qi_gpu_locate_kernels": (C.c_char_p, [V, I, LL]),
        "qi_gpu_locate_multi": (I, [V, V, I, I, V, V, LL, LL, V, LL, LL, V, V, I, V, V, V,
                                    V, V, I, LL, I, V]),
        "qi_gpu_locate_multi_kernels": (C.c_char_p, [V, I, I, LL]),
        "qi_gpu_fingerprint_work_bytes": (SZ, [V, I, I, I, LL]),
        "qi_gpu_fingerprint": (I, [V, V, I, V, I, LL, V, LL, LL, V, LL, LL, V, V, I, V, V,
                                   LL, I, V]),
        "qi_gpu_fingerprint_kernels": (C.c_char_p, [V, I, I, LL]),
        "qi_gpu_partial_ctx_bytes": (SZ, [V, I, I, I]),
        "qi_gpu_partial_ctx": (I, [V, V, V, V, I, I, I, V, V]),
        "qi_gpu_partial": (I, [V, V, I, I, V, LL, LL, V, V, I, V, LL, LL, V, V, I,
                               V, LL, LL, V, V, I, LL, I, V]),
        "qi_gpu_partial_kernels": (C.c_char_p, [V, I, I, LL]),
        "qi_gpu_syndrome_ctx_bytes": (SZ, [V, I, I, I]),
        "qi_gpu_syndrome_ctx": (I, [V, V, V, I, I, I, V, V]),
        "qi_gpu_syndrome": (I, [V, V, I, I, V, LL, LL, V, V, I, V, LL, LL, V, V, I,
                                V, LL, LL, V, V, I, LL, I, V]),
        "qi_gpu_syndrome_kernels": (C.c_char_p, [V, I, I, LL]),
        "qi_gpu_syndrome_locate_ctx_bytes": (SZ, [V, I, I]),
        "qi_gpu_syndrome_locate_ctx": (I, [V, V, I, I, V, V]),
        "qi_gpu_syndrome_locate": (I, [V, V, I, I, V, LL, LL, V, V, I, V, V, V, V, V, I,
                                       LL, I, V]),
        "qi_gpu_syndrome_locate_kernels": (C.c_char_p, [V, I, I, LL]),
        "qi_gpu_patch_work_bytes": (SZ, [V, I, I]),
        "qi_gpu_patch": (I, [V, I, V, I, V, V, V, V, V, I, V, LL, LL, V, LL, LL, V, V, I, V, V, V,
                             LL, I, V]),
        "qi_gpu_patch_kernels": (C.c_char_p, [V, I, I, LL]),
        "qi_gpu_take_error": (I, [V]),
        "qi_build_id": (C.c_char_p, []),
        "qi_gpu_kernels": (C.c_char_p, [V, LL]),
        "qi_fec_new": (V, [I, I, I]),
        "qi_fec_delete": (None, [V]),
        "qi_fec_n_outputs": (I, [V]),
        "qi_fec_encode_blocks": (I, [V, c_u8pp, c_u8pp, SZ, V, V, U32]),
        "qi_fec_decode_blocks": (I, [V, c_u8pp, c_u8pp, V, V, U32, V, V, SZ]),
        "qi_fec_repair_blocks": (I, [V, c_u8pp, c_u8pp, V, V, U32, V, V, I, c_u8pp, V,
                                     V, U32, SZ]),
        "qi_fec_verify_blocks": (I, [V, c_u8pp, c_u8pp, V, V, U32, V, V, SZ]),
        "qi_fec_locate_blocks": (I, [V, c_u8pp, c_u8pp, V, V, U32, V, V, I, SZ]),
        "qi_fec_locate_multi_blocks": (I, [V, c_u8pp, c_u8pp, V, V, U32, V, I, V, I, SZ]),
        "qi_fec_fingerprint_blocks": (I, [V, c_u8pp, c_u8pp, V, V, U32, V, V, I, V, SZ]),
        "qi_fec_update_blocks": (I, [V, V, I, c_u8pp, c_u8pp, c_u8pp, V, V, U32, SZ]),
        "qi_fec_partial_repair_blocks": (I, [V, V, V, I, c_u8pp, V, V, U32, V, I, I, c_u8pp,
                                             V, V, U32, SZ]),
        "qi_fec_syndrome_blocks": (I, [V, V, I, V, I, c_u8pp, V, V, U32, I, I, c_u8pp, V, V,
                                       U32, SZ]),
        "qi_fec_locate_syndromes": (I, [V, V, I, c_u8pp, V, V, U32, I, V, V, U32, V, SZ]),
        "qi_fec_apply_deltas": (I, [V, V, I, c_u8pp, V, V, U32, V, U32, SZ]),
        "qi_fec_scrub_blocks": (I, [V, c_u8pp, c_u8pp, V, V, U32, V, I, V, I, SZ]),
        "qi_fec_encode_streams": (I, [V, c_u8pp, SZ, c_u8pp, V, V, U32]),
        "qi_fec_decode_streams": (I, [V, c_u8pp, c_u8pp, SZ, V, V, U32,
                                      c_u8pp]),
        "qi_nf4_new": (V, [I, I, I]),
        "qi_nf4_delete": (None, [V]),
        "qi_nf4_n_outputs": (I, [V]),
        "qi_nf4_encode_blocks": (I, [V, c_u8pp, c_u8pp, SZ, V, V, V, U32]),
        "qi_nf4_decode_blocks": (I, [V, c_u8pp, c_u8pp, V, V, V, U32, V, V,
                                     SZ]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib


def lib():
    """Load the native library (raises if it was not built)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} missing: build it with "
                "`python -c 'import __graft_entry__ as g; g.build()'` or "
                "`make -C quadiron_amd/csrc`")
        # torch-rocm bundles its own libamdhip64 with the same SONAME
        # (libamdhip64.so.7): load torch first so the process keeps ONE HIP
        # runtime (ours then binds to it) and torch streams/pointers are
        # valid in our launches.  C-ABI users without torch get /opt/rocm's.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        _lib = _declare(C.CDLL(LIB_PATH))
    return _lib


def build_id():
    """'<git describe>+src:<source hash>' baked into the loaded library."""
    return lib().qi_build_id().decode()


def _rows(t, name, rows=None, stripes=None):
    """Check a [S, rows, P] u16 row tensor before its pointer and strides go
    to the device C-ABI: a wrong dtype, device, shape or a non-unit inner
    stride would become out-of-bounds device accesses."""
    import torch
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name}: expected a HIP (cuda) tensor")
    if t.dtype not in (torch.int16, torch.uint16):
        raise TypeError(f"{name}: expected int16/uint16, got {t.dtype}")
    if t.dim() != 3 or t.stride(-1) != 1:
        raise ValueError(f"{name}: expected [S, rows, P] with unit inner stride")
    if rows is not None and t.shape[1] != rows:
        raise ValueError(f"{name}: expected {rows} rows, got {t.shape[1]}")
    if stripes is not None and t.shape[0] != stripes:
        raise ValueError(f"{name}: expected {stripes} stripes, got {t.shape[0]}")


def _flat(t, name, n, dtypes):
    """A device buffer of at least n elements of one of `dtypes`."""
    if t is None:
        return
    if not t.is_cuda or t.dtype not in dtypes or not t.is_contiguous():
        raise TypeError(f"{name}: expected a contiguous HIP tensor of {dtypes}")
    if t.numel() < n:
        raise ValueError(f"{name}: {t.numel()} elements, need {n}")


def _oor(counts, entries, cap, S, slots):
    import torch
    if counts is None:
        return
    if entries is None or cap < 1:
        raise ValueError("OOR buckets need counts, entries and cap >= 1")
    _flat(counts, "counts", S * slots, (torch.int32,))
    _flat(entries, "entries", S * slots * cap, (torch.int32,))


def _ptr(t):
    """The device pointer of an optional tensor (None -> NULL)."""
    return t.data_ptr() if t is not None else None


def _row_args(t):
    """(pointer, stripe stride, row stride) of an optional row tensor."""
    return (t.data_ptr(), t.stride(0), t.stride(1)) if t is not None else (None, 0, 0)


def _need(need, S, unsupported):
    """a context size, or the ValueError of a shape whose size is 0"""
    if need == 0 and S > 0:
        raise ValueError(unsupported)
    return need


def require_device():
    n = lib().qi_gpu_device_count()
    if n < 1:
        raise RuntimeError("quadiron_amd: no HIP device visible")
    return n


def ptr_array(arrs):
    """uint8_t** from a list of numpy uint8 arrays (None -> NULL)."""
    p = (c_u8p * len(arrs))()
    for i, a in enumerate(arrs):
        p[i] = a.ctypes.data_as(c_u8p) if a is not None else None
    return p


class Plan:
    """Device plan (include/qi_gpu.h) for RS-FNT(k, m)."""

    ENCODERS = {None: 0, "matrix": 1, "codelets": 2}  # QI_PLAN_ENC_* flags

    def __init__(self, k, m, systematic=False, encoder=None):
        """encoder: None (the library's choice), "matrix" or "codelets"
        (force the non-systematic encode kernel for k <= 64)."""
        require_device()
        if encoder not in self.ENCODERS:
            raise ValueError(f"encoder must be one of {list(self.ENCODERS)}")
        self.k, self.m, self.sys = k, m, bool(systematic)
        self.h = lib().qi_plan_create_ex(k, m, int(systematic),
                                         self.ENCODERS[encoder])
        if not self.h:
            raise ValueError(f"qi_plan_create({k}, {m}, {systematic}) failed")
        self.n = lib().qi_plan_n(self.h)
        self.n_outputs = lib().qi_plan_n_outputs(self.h)

    def kernels(self, words):
        """'encode=<kernels>; decode=<kernels>' this plan launches over
        `words` columns (qi_gpu_kernels)."""
        return lib().qi_gpu_kernels(self.h, words).decode()

    def close(self):
        if self.h:
            lib().qi_plan_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _stream(stream):
        return stream if stream is not None else None

    def encode(self, data, out, counts=None, entries=None, cap=0, stream=None):
        """data: int16/uint16 tensor [S, k, P] on cuda; out: [S, n_out, P]."""
        _rows(data, "data", self.k)
        S, k, P = data.shape
        _rows(out, "out", self.n_outputs, S)
        if out.shape[2] < P:
            raise ValueError("out: fewer columns than data")
        _oor(counts, entries, cap, S, self.n_outputs)
        rc = lib().qi_gpu_encode(
            self.h, data.data_ptr(), data.stride(0), data.stride(1),
            out.data_ptr(), out.stride(0), out.stride(1), P, S,
            _ptr(counts), _ptr(entries), int(cap),
            self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_encode failed: {rc}")

    def ctx_bytes(self, n_stripes, words):
        return lib().qi_gpu_decode_ctx_bytes(self.h, n_stripes, words)

    def decode_ctx(self, ids, ctx, words, counts=None, entries=None, cap=0,
                   h_ids=None, stream=None):
        """ids: int16 tensor [S, k] on cuda (fragment ids); OOR buckets of
        the coded rows as produced by encode (routed into the contexts)."""
        import torch
        S = ids.shape[0]
        _flat(ids, "ids", S * self.k, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", self.ctx_bytes(S, words), (torch.uint8,))
        _oor(counts, entries, cap, S, self.n_outputs)
        rc = lib().qi_gpu_decode_ctx(
            self.h, ids.data_ptr(),
            h_ids.ctypes.data_as(C.c_void_p) if h_ids is not None else None,
            ids.shape[0],
            _ptr(counts), _ptr(entries), int(cap),
            words, ctx.data_ptr(), self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_decode_ctx failed: {rc}")

    def decode(self, ctx, ids, coded, out, data=None, counts=None,
               entries=None, cap=0, stream=None, check=True):
        """coded: [S, n_out, P] (fragment slot rows); out: [S, k, P].
        check: synchronise and return the sticky OOR-overflow flag
        (qi_gpu_take_error); with check=False the call stays asynchronous
        and returns 0 -- call take_error() later."""
        import torch
        _rows(out, "out", self.k)
        S, _, P = out.shape
        _rows(coded, "coded", self.n_outputs, S)
        if data is not None:
            _rows(data, "data", self.k, S)
        _flat(ids, "ids", S * self.k, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", self.ctx_bytes(S, P), (torch.uint8,))
        _oor(counts, entries, cap, S, self.n_outputs)
        d = data if data is not None else coded
        rc = lib().qi_gpu_decode(
            self.h, ctx.data_ptr(), ids.data_ptr(), d.data_ptr(), d.stride(0),
            d.stride(1), coded.data_ptr(), coded.stride(0), coded.stride(1),
            _ptr(counts), _ptr(entries), int(cap),
            out.data_ptr(), out.stride(0), out.stride(1), P, S,
            self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_decode failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    def decode_ctx_packed(self, ids, ctx, words, counts=None, entries=None,
                          cap=0, h_ids=None, stream=None):
        """Contexts for decode_packed: OOR buckets indexed by the position
        of the received row (slots = k)."""
        import torch
        S = ids.shape[0]
        _flat(ids, "ids", S * self.k, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", self.ctx_bytes(S, words), (torch.uint8,))
        _oor(counts, entries, cap, S, self.k)
        rc = lib().qi_gpu_decode_ctx_packed(
            self.h, ids.data_ptr(),
            h_ids.ctypes.data_as(C.c_void_p) if h_ids is not None else None,
            ids.shape[0],
            _ptr(counts), _ptr(entries), int(cap),
            words, ctx.data_ptr(), self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_decode_ctx_packed failed: {rc}")

    def decode_packed(self, ctx, recv, out, counts=None, entries=None, cap=0,
                      stream=None, check=True):
        """recv: [S, k, P] received rows in id order; out: [S, k, P]."""
        import torch
        _rows(out, "out", self.k)
        S, _, P = out.shape
        _rows(recv, "recv", self.k, S)
        _flat(ctx, "ctx", self.ctx_bytes(S, P), (torch.uint8,))
        _oor(counts, entries, cap, S, self.k)
        rc = lib().qi_gpu_decode_packed(
            self.h, ctx.data_ptr(), recv.data_ptr(), recv.stride(0),
            recv.stride(1),
            _ptr(counts), _ptr(entries), int(cap),
            out.data_ptr(), out.stride(0), out.stride(1), P, S,
            self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_decode_packed failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    ERR_UNSUPPORTED = -5  # QI_ERR_UNSUPPORTED

    def repair_kernels(self, n_targets, words):
        """'repair=<kernels>' a repair of n_targets fragments launches over
        `words` columns (qi_gpu_repair_kernels); '' when unsupported."""
        return lib().qi_gpu_repair_kernels(self.h, n_targets, words).decode()

    def repair_ctx_bytes(self, n_targets, n_stripes, words):
        """0 when the plan (k > 256) or n_targets is not supported."""
        return lib().qi_gpu_repair_ctx_bytes(self.h, n_targets, n_stripes,
                                             words)

    def _repair_need(self, what, R, S, words):
        """repair_ctx_bytes, or the error of a "repair" / "check" of R
        fragments that the plan does not support."""
        noun = "targets" if what == "repair" else "fragments"
        return _need(self.repair_ctx_bytes(R, S, words), S,
                     f"{what} of {R} {noun} is not supported on "
                     f"this plan (k <= 256, 1 <= R <= min(64, m))")

    def repair_ctx(self, ids, targets, ctx, words, counts=None, entries=None,
                   cap=0, stream=None):
        """ids: int16 tensor [S, k] (received fragment ids); targets: int16
        tensor [S, R] (the fragments to rebuild); OOR buckets of the coded
        rows as produced by encode (routed into the contexts)."""
        import torch
        if ids.dim() != 2 or targets.dim() != 2 or ids.shape[0] != targets.shape[0]:
            raise ValueError("ids: expected [S, k], targets: [S, R]")
        S, R = targets.shape
        need = self._repair_need("repair", R, S, words)
        _flat(ids, "ids", S * self.k, (torch.int16, torch.uint16))
        _flat(targets, "targets", S * R, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", need, (torch.uint8,))
        _oor(counts, entries, cap, S, self.n_outputs)
        rc = lib().qi_gpu_repair_ctx(
            self.h, ids.data_ptr(), targets.data_ptr(), R, S,
            _ptr(counts), _ptr(entries), int(cap),
            words, ctx.data_ptr(), self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_repair_ctx failed: {rc}")

    def repair(self, ctx, coded, out, data=None, counts=None, entries=None,
               cap=0, out_counts=None, out_entries=None, out_cap=0,
               stream=None, check=True):
        """coded: [S, n_out, P] (fragment slot rows, with their OOR buckets
        counts / entries); out: [S, R, P], row j = target j of the context,
        its marks in out_counts / out_entries (slots = R; cleared by the
        caller).  Returns the sticky error flags when check."""
        _rows(out, "out")
        S, R, P = out.shape
        _rows(coded, "coded", self.n_outputs, S)
        if data is not None:
            _rows(data, "data", self.k, S)
        need = self._repair_need("repair", R, S, P)
        import torch
        _flat(ctx, "ctx", need, (torch.uint8,))
        _oor(counts, entries, cap, S, self.n_outputs)
        _oor(out_counts, out_entries, out_cap, S, R)
        d = data if data is not None else coded
        rc = lib().qi_gpu_repair(
            self.h, ctx.data_ptr(), R, d.data_ptr(), d.stride(0), d.stride(1),
            coded.data_ptr(), coded.stride(0), coded.stride(1),
            _ptr(counts), _ptr(entries), int(cap),
            out.data_ptr(), out.stride(0), out.stride(1),
            _ptr(out_counts), _ptr(out_entries), int(out_cap), P, S, self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_repair failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    def verify_kernels(self, n_checks, words):
        """'verify=<kernels>' a check of n_checks fragments launches over
        `words` columns (qi_gpu_verify_kernels); '' when unsupported."""
        return lib().qi_gpu_verify_kernels(self.h, n_checks, words).decode()

    def verify_work_bytes(self, n_checks, n_stripes, work_cap):
        """Scratch for the recomputed rows' 65536 positions (no rows: no
        width); 0 when the plan (k > 256) or n_checks is not supported."""
        return lib().qi_gpu_verify_work_bytes(self.h, n_checks, n_stripes,
                                              work_cap)

    def verify(self, ctx, checks, coded, work, work_cap, value_mismatch,
               mark_mismatch, first, data=None, counts=None, entries=None,
               cap=0, stream=None, check=True):
        """Fused check (qi_gpu_verify).  ctx: a repair context built by
        repair_ctx(basis ids, checks, ...); checks: int16 tensor [S, R], the
        same as given there; coded: [S, n_out, P] (fragment slot rows, with
        their OOR buckets counts / entries), data: [S, k, P] for systematic
        codes; work: uint8 scratch of verify_work_bytes(R, S, work_cap).
        value_mismatch, mark_mismatch, first: int32 tensors of S * R
        elements, written (and initialised) by the call.  Returns the sticky
        error flags when check."""
        import torch
        if checks.dim() != 2:
            raise ValueError("checks: expected [S, R]")
        S, R = checks.shape
        _rows(coded, "coded", self.n_outputs, S)
        P = coded.shape[2]
        if data is not None:
            _rows(data, "data", self.k, S)
            if data.shape[2] != P:
                raise ValueError("data and coded differ in width")
        need = self._repair_need("check", R, S, P)
        _flat(checks, "checks", S * R, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", need, (torch.uint8,))
        _flat(work, "work", self.verify_work_bytes(R, S, work_cap), (torch.uint8,))
        for t, name in ((value_mismatch, "value_mismatch"),
                        (mark_mismatch, "mark_mismatch"), (first, "first")):
            if t is None:
                raise ValueError(f"{name} is required")
            _flat(t, name, S * R, (torch.int32, torch.uint32))
        _oor(counts, entries, cap, S, self.n_outputs)
        d = data if data is not None else coded
        rc = lib().qi_gpu_verify(
            self.h, ctx.data_ptr(), R, checks.data_ptr(), d.data_ptr(),
            d.stride(0), d.stride(1), coded.data_ptr(), coded.stride(0),
            coded.stride(1),
            _ptr(counts), _ptr(entries), int(cap),
            work.data_ptr(), int(work_cap), value_mismatch.data_ptr(),
            mark_mismatch.data_ptr(), first.data_ptr(), P, S,
            self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_verify failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    UPDATE_MAX_ROWS = 8  # QI_UPDATE_MAX_ROWS

    def update_kernels(self, n_rows, n_slots, words):
        """'update=<context kernel> + <kernel>' an update of n_rows data rows
        and n_slots coded rows launches (qi_gpu_update_kernels); '' for
        counts out of range."""
        return lib().qi_gpu_update_kernels(self.h, n_rows, n_slots, words).decode()

    def update_ctx_bytes(self, n_rows, n_slots, n_stripes):
        """0 when n_rows is outside 1 .. min(8, k) or n_slots outside
        1 .. n_outputs."""
        return lib().qi_gpu_update_ctx_bytes(self.h, n_rows, n_slots, n_stripes)

    def update_ctx(self, ids, slots, ctx, stream=None):
        """ids: int16 tensor [S, U] (the changed data rows); slots: int16
        tensor [S, R] (the coded rows to update, by encode output index) or
        None for all n_outputs of them."""
        import torch
        if ids.dim() != 2 or (slots is not None and (
                slots.dim() != 2 or slots.shape[0] != ids.shape[0])):
            raise ValueError("ids: expected [S, U], slots: [S, R] or None")
        S, U = ids.shape
        R = slots.shape[1] if slots is not None else self.n_outputs
        need = self.update_ctx_bytes(U, R, S)
        if need == 0 and S > 0:
            raise ValueError(f"update of {U} rows into {R} slots is not supported "
                             f"(1 <= U <= min(8, k), 1 <= R <= n_outputs)")
        _flat(ids, "ids", S * U, (torch.int16, torch.uint16))
        _flat(slots, "slots", S * R, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", need, (torch.uint8,))
        rc = lib().qi_gpu_update_ctx(
            self.h, ids.data_ptr(), _ptr(slots), U, R, S, ctx.data_ptr(), self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_update_ctx failed: {rc}")

    def update(self, ctx, n_slots, old, new, coded, out=None, counts=None,
               entries=None, cap=0, out_counts=None, out_entries=None,
               out_cap=0, stream=None, check=True):
        """old, new: [S, U, P], row u the old / new contents of data row
        ids[s][u] of the context; coded: [S, n_out, P] (rows by slot, with
        their OOR buckets counts / entries); out: the same shape, None for
        in place; the updated rows' marks go to out_counts / out_entries
        (slots = n_outputs, cleared by the caller, distinct from counts /
        entries).  n_slots: the R the context was built with.  Returns the
        sticky error flags when check."""
        import torch
        _rows(old, "old")
        S, U, P = old.shape
        _rows(new, "new", U, S)
        _rows(coded, "coded", self.n_outputs, S)
        out = coded if out is None else out
        _rows(out, "out", self.n_outputs, S)
        if not new.shape[2] == coded.shape[2] == out.shape[2] == P:
            raise ValueError("old, new, coded and out differ in width")
        need = self.update_ctx_bytes(U, n_slots, S)
        if need == 0 and S > 0:
            raise ValueError(f"update of {U} rows into {n_slots} slots is not supported "
                             f"(1 <= U <= min(8, k), 1 <= R <= n_outputs)")
        _flat(ctx, "ctx", need, (torch.uint8,))
        _oor(counts, entries, cap, S, self.n_outputs)
        _oor(out_counts, out_entries, out_cap, S, self.n_outputs)
        rc = lib().qi_gpu_update(
            self.h, ctx.data_ptr(), U, n_slots,
            old.data_ptr(), old.stride(0), old.stride(1),
            new.data_ptr(), new.stride(0), new.stride(1),
            coded.data_ptr(), coded.stride(0), coded.stride(1),
            _ptr(counts), _ptr(entries), int(cap),
            out.data_ptr(), out.stride(0), out.stride(1),
            _ptr(out_counts), _ptr(out_entries), int(out_cap), P, S, self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_update failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    PARTIAL_MAX_TARGETS = 8  # QI_PARTIAL_MAX_TARGETS

    def partial_kernels(self, n_held, n_targets, words):
        """'partial=<context kernel> + <kernel>' a partial repair of n_targets
        fragments from n_held held rows launches (qi_gpu_partial_kernels); ''
        for counts out of range."""
        return lib().qi_gpu_partial_kernels(self.h, n_held, n_targets, words).decode()

    def partial_ctx_bytes(self, n_held, n_targets, n_stripes):
        """0 when n_held is outside 1 .. k or n_targets outside
        1 .. min(8, m)."""
        return lib().qi_gpu_partial_ctx_bytes(self.h, n_held, n_targets, n_stripes)

    def _partial_need(self, H, R, S):
        return _need(self.partial_ctx_bytes(H, R, S), S,
                     f"partial repair of {R} targets from {H} held rows is not "
                     f"supported (1 <= H <= k, 1 <= R <= min(8, m))")

    def partial_ctx(self, ids, held, targets, ctx, stream=None):
        """ids: int16 tensor [S, k] (the k helper fragments of the repair);
        held: int16 tensor [S, H], positions into ids (the helpers whose rows
        the call has); targets: int16 tensor [S, R] (the fragments to
        rebuild)."""
        import torch
        if (ids.dim() != 2 or held.dim() != 2 or targets.dim() != 2 or
                not ids.shape[0] == held.shape[0] == targets.shape[0] or
                ids.shape[1] != self.k):
            raise ValueError("ids: expected [S, k], held: [S, H], targets: [S, R]")
        S, H = held.shape
        R = targets.shape[1]
        need = self._partial_need(H, R, S)
        for t, name, n in ((ids, "ids", S * self.k), (held, "held", S * H),
                           (targets, "targets", S * R)):
            _flat(t, name, n, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", need, (torch.uint8,))
        rc = lib().qi_gpu_partial_ctx(
            self.h, ids.data_ptr(), held.data_ptr(), targets.data_ptr(), H, R, S,
            ctx.data_ptr(), self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_partial_ctx failed: {rc}")

    def partial(self, ctx, rows, out, acc=None, counts=None, entries=None, cap=0,
                acc_counts=None, acc_entries=None, acc_cap=0, out_counts=None,
                out_entries=None, out_cap=0, stream=None, check=True):
        """rows: [S, H, P], row h the helper at position held[s][h] of the
        context, with its OOR bucket in slot h of counts / entries (slots =
        H); acc: [S, R, P] partial rows to start from (None: 0) with their
        buckets acc_counts / acc_entries (slots = R); out: [S, R, P], row t =
        target t, may be acc itself; its marks go to out_counts / out_entries
        (slots = R, cleared by the caller, distinct from the acc buckets).
        Returns the sticky error flags when check."""
        return self._share(lib().qi_gpu_partial, "qi_gpu_partial", self._partial_need, ctx, rows,
                           out, acc, counts, entries, cap, acc_counts, acc_entries, acc_cap,
                           out_counts, out_entries, out_cap, stream, check)

    def _share(self, fn, name, need_of, ctx, rows, out, acc, counts, entries, cap, acc_counts,
               acc_entries, acc_cap, out_counts, out_entries, out_cap, stream, check):
        """the accumulating row call of partial and syndrome"""
        import torch
        _rows(rows, "rows")
        S, H, P = rows.shape
        _rows(out, "out", None, S)
        R = out.shape[1]
        if acc is not None:
            _rows(acc, "acc", R, S)
        if out.shape[2] != P or (acc is not None and acc.shape[2] != P):
            raise ValueError("rows, acc and out differ in width")
        need = need_of(H, R, S)
        _flat(ctx, "ctx", need, (torch.uint8,))
        _oor(counts, entries, cap, S, H)
        _oor(acc_counts, acc_entries, acc_cap, S, R)
        _oor(out_counts, out_entries, out_cap, S, R)
        rc = fn(
            self.h, ctx.data_ptr(), H, R,
            rows.data_ptr(), rows.stride(0), rows.stride(1),
            _ptr(counts), _ptr(entries), int(cap),
            *_row_args(acc), _ptr(acc_counts), _ptr(acc_entries), int(acc_cap),
            out.data_ptr(), out.stride(0), out.stride(1),
            _ptr(out_counts), _ptr(out_entries), int(out_cap), P, S, self._stream(stream))
        if rc:
            raise RuntimeError(f"{name} failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    SYNDROME_MAX_CHECKS = 8  # QI_SYNDROME_MAX_CHECKS
    SYNDROME_MAX_ERRORS = 4  # QI_SYNDROME_MAX_ERRORS

    def syndrome_kernels(self, n_held, n_checks, words):
        """'syndrome=<context kernel> + <partial kernel form>' a syndrome share
        of n_held rows with n_checks syndromes launches
        (qi_gpu_syndrome_kernels); '' for counts out of range."""
        return lib().qi_gpu_syndrome_kernels(self.h, n_held, n_checks, words).decode()

    def syndrome_ctx_bytes(self, n_held, n_checks, n_stripes):
        """0 when n_checks is outside 1 .. min(8, m) or n_held outside
        1 .. k + n_checks."""
        return lib().qi_gpu_syndrome_ctx_bytes(self.h, n_held, n_checks, n_stripes)

    def _syndrome_need(self, H, R, S):
        return _need(self.syndrome_ctx_bytes(H, R, S), S,
                     f"a syndrome share of {H} held rows with {R} checks is not "
                     f"supported (1 <= R <= min(8, m), 1 <= H <= k + R)")

    def syndrome_ctx(self, ids, held, ctx, stream=None):
        """ids: int16 tensor [S, k + R] (the listed fragments; R = n_checks
        follows from the shape); held: int16 tensor [S, H], positions into ids
        (the listed fragments whose rows the call has)."""
        import torch
        if ids.dim() != 2 or held.dim() != 2 or ids.shape[0] != held.shape[0]:
            raise ValueError("ids: expected [S, k + R], held: [S, H]")
        S, H = held.shape
        R = ids.shape[1] - self.k
        need = self._syndrome_need(H, R, S)
        _flat(ids, "ids", S * (self.k + R), (torch.int16, torch.uint16))
        _flat(held, "held", S * H, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", need, (torch.uint8,))
        rc = lib().qi_gpu_syndrome_ctx(self.h, ids.data_ptr(), held.data_ptr(), H, R, S,
                                       ctx.data_ptr(), self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_syndrome_ctx failed: {rc}")

    def syndrome(self, ctx, rows, out, acc=None, counts=None, entries=None, cap=0,
                 acc_counts=None, acc_entries=None, acc_cap=0, out_counts=None,
                 out_entries=None, out_cap=0, stream=None, check=True):
        """Syndrome share (qi_gpu_syndrome).  Arguments as partial: rows
        [S, H, P], row h the listed fragment at position held[s][h]; acc and
        out [S, R, P], row j = syndrome j, out may be acc itself.  Returns the
        sticky error flags when check."""
        return self._share(lib().qi_gpu_syndrome, "qi_gpu_syndrome", self._syndrome_need, ctx,
                           rows, out, acc, counts, entries, cap, acc_counts, acc_entries, acc_cap,
                           out_counts, out_entries, out_cap, stream, check)

    def syndrome_locate_kernels(self, n_checks, max_errors, words):
        """'syndrome_locate=<context kernel> + <kernel>'
        (qi_gpu_syndrome_locate_kernels); '' when n_checks is outside
        1 .. min(8, m) or max_errors outside 0 .. n_checks // 2."""
        return lib().qi_gpu_syndrome_locate_kernels(self.h, n_checks, max_errors,
                                                    words).decode()

    def syndrome_locate_ctx_bytes(self, n_checks, n_stripes):
        """12 (k + n_checks) bytes per stripe; 0 when n_checks is outside
        1 .. min(8, m)."""
        return lib().qi_gpu_syndrome_locate_ctx_bytes(self.h, n_checks, n_stripes)

    def _syndrome_locate_need(self, R, S):
        return _need(self.syndrome_locate_ctx_bytes(R, S), S,
                     f"a syndrome locate with {R} checks is not supported "
                     f"(1 <= R <= min(8, m))")

    def syndrome_locate_ctx(self, ids, ctx, stream=None):
        """ids: int16 tensor [S, k + R], the listed fragments; R = n_checks
        follows from the shape."""
        import torch
        if ids.dim() != 2:
            raise ValueError("ids: expected [S, k + R]")
        S, N = ids.shape
        R = N - self.k
        need = self._syndrome_locate_need(R, S)
        _flat(ids, "ids", S * N, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", need, (torch.uint8,))
        rc = lib().qi_gpu_syndrome_locate_ctx(self.h, ids.data_ptr(), R, S, ctx.data_ptr(),
                                              self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_syndrome_locate_ctx failed: {rc}")

    def syndrome_locate(self, ctx, max_errors, syn, located, unlocated, weights, fix_counts,
                        fixes=None, fix_cap=0, counts=None, entries=None, cap=0, stream=None,
                        check=True):
        """The decision over summed syndrome rows (qi_gpu_syndrome_locate).
        syn: [S, R, P], row j = syndrome j, with its marks in slot j of counts
        / entries (slots = R).  0 <= max_errors <= R // 2.  Outputs, int32,
        initialised by the call: located [S, k + R], unlocated [S], weights
        [S, 4], fix_counts [S], fixes [S, fix_cap, 3] of {column, position,
        error e}: the true symbol is (y - e) mod 65537.  Returns the sticky
        error flags when check."""
        import torch
        _rows(syn, "syn")
        S, R, P = syn.shape
        need = self._syndrome_locate_need(R, S)
        t = int(max_errors)
        if not 0 <= 2 * t <= R:
            raise ValueError("syndrome_locate: max_errors must be 0 .. R // 2")
        _flat(ctx, "ctx", need, (torch.uint8,))
        _oor(counts, entries, cap, S, R)
        for tn, name, n in ((located, "located", self.k + R), (unlocated, "unlocated", 1),
                            (weights, "weights", self.SYNDROME_MAX_ERRORS),
                            (fix_counts, "fix_counts", 1)):
            if tn is None:
                raise ValueError(f"{name}: required")
            _flat(tn, name, S * n, (torch.int32,))
        if fix_cap < 0 or (fix_cap > 0 and fixes is None):
            raise ValueError("fix_cap > 0 needs fixes")
        _flat(fixes, "fixes", S * fix_cap * 3, (torch.int32,))
        rc = lib().qi_gpu_syndrome_locate(
            self.h, ctx.data_ptr(), R, t, syn.data_ptr(), syn.stride(0), syn.stride(1),
            _ptr(counts), _ptr(entries), int(cap), located.data_ptr(), unlocated.data_ptr(),
            weights.data_ptr(), fix_counts.data_ptr(), _ptr(fixes), int(fix_cap), P, S,
            self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_syndrome_locate failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    LOCATE_MAX_CHECKS = 8  # QI_LOCATE_MAX_CHECKS

    def locate_kernels(self, n_checks, words):
        """'locate=<context kernel> + <kernel>' a locate with n_checks
        syndromes launches (qi_gpu_locate_kernels); '' when unsupported."""
        return lib().qi_gpu_locate_kernels(self.h, n_checks, words).decode()

    def locate_ctx_bytes(self, n_checks, n_stripes):
        """0 when k > 256 or n_checks is outside 2 .. min(8, m)."""
        return lib().qi_gpu_locate_ctx_bytes(self.h, n_checks, n_stripes)

    def locate_ctx(self, ids, ctx, stream=None):
        """ids: int16 tensor [S, k + R], the listed present fragments of each
        list position (decode id space); R = n_checks follows from the
        shape."""
        import torch
        if ids.dim() != 2:
            raise ValueError("ids: expected [S, k + R]")
        S, N = ids.shape
        R = N - self.k
        need = self.locate_ctx_bytes(R, S)
        if need == 0 and S > 0:
            raise ValueError(f"locate with {R} checks is not supported on this "
                             f"plan (k <= 256, 2 <= R <= min(8, m))")
        _flat(ids, "ids", S * N, (torch.int16, torch.uint16))
        _flat(ctx, "ctx", need, (torch.uint8,))
        rc = lib().qi_gpu_locate_ctx(self.h, ids.data_ptr(), R, S, ctx.data_ptr(),
                                     self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_locate_ctx failed: {rc}")

    def _locate_args(self, ctx, n_checks, coded, outputs, fixes, fix_cap, data,
                     counts, entries, cap, stripes, check):
        """The checks locate and locate_multi share.  outputs: the call's
        required (tensor, name, elements per list position).  Returns the
        argument runs in front of and behind the C call's outputs: (stripes,
        data rows, coded rows, buckets) and (fixes, fix_cap, P, S)."""
        import torch
        _rows(coded, "coded", self.n_outputs)
        S_all, _, P = coded.shape
        if data is not None:
            _rows(data, "data", self.k, S_all)
            if data.shape[2] != P:
                raise ValueError("data and coded differ in width")
        elif self.sys:
            raise ValueError("a systematic plan needs the data rows")
        if stripes is not None:
            _flat(stripes, "stripes", 0, (torch.int32,))
            S = stripes.numel()
            # every listed stripe must exist (checked here unless check=False:
            # reading the values back waits for the device)
            if check and S > 0 and not (0 <= int(stripes.min()) and
                                        int(stripes.max()) < S_all):
                raise ValueError(f"stripes: values must lie in [0, {S_all})")
        else:
            S = S_all
        need = self.locate_ctx_bytes(n_checks, S)
        if need == 0 and S > 0:
            raise ValueError(f"locate with {n_checks} checks is not supported on "
                             f"this plan (k <= 256, 2 <= R <= min(8, m))")
        _flat(ctx, "ctx", need, (torch.uint8,))
        _oor(counts, entries, cap, S_all, self.n_outputs)
        for t, name, n in outputs:
            if t is None:
                raise ValueError(f"{name}: required")
            _flat(t, name, S * n, (torch.int32,))
        if fix_cap < 0 or (fix_cap > 0 and fixes is None):
            raise ValueError("fix_cap > 0 needs fixes")
        _flat(fixes, "fixes", S * fix_cap * 3, (torch.int32,))
        return ((_ptr(stripes), *_row_args(data), *_row_args(coded), _ptr(counts),
                 _ptr(entries), int(cap)),
                (_ptr(fixes), int(fix_cap), P, S))

    def locate(self, ctx, n_checks, coded, located, unlocated, fix_counts,
               fixes=None, fix_cap=0, data=None, counts=None, entries=None,
               cap=0, stripes=None, stream=None, check=True):
        """Fragment locate (qi_gpu_locate).  ctx: built by locate_ctx; coded:
        [S_all, n_out, P] (fragment slot rows, with their OOR buckets counts /
        entries), data: [S_all, k, P] for systematic codes.  stripes: int32
        tensor of the stripes to look at (list position -> stripe), None for
        all S_all in order.  Outputs by list position, int32, initialised by
        the call: located [S, k + R], unlocated [S], fix_counts [S], fixes
        [S, fix_cap, 3] of {column, position, corrected symbol}.  Returns the
        sticky error flags when check."""
        rows, tail = self._locate_args(
            ctx, n_checks, coded,
            ((located, "located", self.k + n_checks), (unlocated, "unlocated", 1),
             (fix_counts, "fix_counts", 1)),
            fixes, fix_cap, data, counts, entries, cap, stripes, check)
        rc = lib().qi_gpu_locate(
            self.h, ctx.data_ptr(), n_checks, *rows, located.data_ptr(),
            unlocated.data_ptr(), fix_counts.data_ptr(), *tail, self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_locate failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    LOCATE_MAX_ERRORS = 4  # QI_LOCATE_MAX_ERRORS

    def locate_multi_kernels(self, n_checks, max_errors, words):
        """'locate_multi=<context kernel> + <kernel>' a multi-fragment locate
        launches (qi_gpu_locate_multi_kernels); '' when unsupported or
        max_errors is outside 1 .. n_checks // 2."""
        return lib().qi_gpu_locate_multi_kernels(self.h, n_checks, max_errors,
                                                 words).decode()

    def locate_multi(self, ctx, n_checks, max_errors, coded, located, unlocated,
                     weights, fix_counts, fixes=None, fix_cap=0, data=None,
                     counts=None, entries=None, cap=0, stripes=None, stream=None,
                     check=True):
        """Multi-fragment locate (qi_gpu_locate_multi): up to max_errors bad
        fragments per column, 1 <= max_errors <= n_checks // 2.  Arguments as
        locate, and weights: int32 [S, 4], weights[s, nu - 1] the columns of
        list position s located with nu fragments.  A located column adds 1
        to each of its fragments' located counters and its nu fix entries are
        adjacent.  Returns the sticky error flags when check."""
        rows, tail = self._locate_args(
            ctx, n_checks, coded,
            ((located, "located", self.k + n_checks), (unlocated, "unlocated", 1),
             (weights, "weights", self.LOCATE_MAX_ERRORS), (fix_counts, "fix_counts", 1)),
            fixes, fix_cap, data, counts, entries, cap, stripes, check)
        rc = lib().qi_gpu_locate_multi(
            self.h, ctx.data_ptr(), n_checks, int(max_errors), *rows, located.data_ptr(),
            unlocated.data_ptr(), weights.data_ptr(), fix_counts.data_ptr(), *tail,
            self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_locate_multi failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    FINGERPRINT_MAX_KEYS = 8  # QI_FINGERPRINT_MAX_KEYS

    def fingerprint_kernels(self, n_rows, n_keys, words):
        """'fingerprint=<table kernel> + <kernel>[ + <finish kernel>]' a
        fingerprint of n_rows rows under n_keys keys launches
        (qi_gpu_fingerprint_kernels); '' for arguments out of range."""
        return lib().qi_gpu_fingerprint_kernels(self.h, n_rows, n_keys, words).decode()

    def fingerprint_work_bytes(self, n_rows, n_keys, n_stripes, words):
        """Bytes of the work buffer of such a call (0: arguments out of
        range)."""
        return lib().qi_gpu_fingerprint_work_bytes(self.h, n_rows, n_keys, n_stripes,
                                                   words)

    @staticmethod
    def _keys(keys):
        import numpy as np
        kk = np.ascontiguousarray(keys, np.int64)
        if kk.ndim != 2 or kk.shape[1] != 3 or not 1 <= kk.shape[0] <= Plan.FINGERPRINT_MAX_KEYS:
            raise ValueError("keys: expected 1 .. 8 triples (a, b, d)")
        if kk.min() < 1 or kk.max() > 65536:
            raise ValueError("keys: every component must lie in 1 .. 65536")
        return np.ascontiguousarray(kk, np.uint32)

    def fingerprint(self, ids, keys, fp, work, coded=None, data=None, counts=None,
                    entries=None, cap=0, first_col=0, words=None, stream=None, check=True):
        """Fragment fingerprints (qi_gpu_fingerprint).  ids: int16 tensor
        [S, N] of fragment ids (decode id space; an id may repeat); keys: F
        host triples (a, b, d), each in 1 .. 65536; coded: [S, n_out, P] with
        its OOR buckets counts / entries, data: [S, k, P] for systematic codes
        (either may be None when no listed row lives there); fp: int32 [S, N,
        F], written in full; work: uint8 tensor of fingerprint_work_bytes(N,
        F, S, words).  words: the columns to digest (default P); first_col:
        the absolute column of column 0, for slices of a wider row.  Returns
        the sticky error flags when check."""
        import torch
        if ids.dim() != 2:
            raise ValueError("ids: expected [S, N]")
        S, N = ids.shape
        kk = self._keys(keys)
        F = kk.shape[0]
        P = None
        for t, name, rows in ((coded, "coded", self.n_outputs), (data, "data", self.k)):
            if t is None:
                continue
            _rows(t, name, rows, S)
            if P is not None and t.shape[2] != P:
                raise ValueError("data and coded differ in width")
            P = t.shape[2]
        if P is None or (coded is None and not self.sys):
            raise ValueError("no rows given")
        if data is not None and not self.sys:
            data = None
        words = P if words is None else int(words)
        if not 1 <= words <= P:
            raise ValueError("words: expected 1 .. P")
        need = self.fingerprint_work_bytes(N, F, S, words)
        if need == 0:
            raise ValueError("fingerprint: n_rows out of range (1 .. k + m)")
        _flat(ids, "ids", S * N, (torch.int16, torch.uint16))
        _flat(work, "work", need, (torch.uint8,))
        _flat(fp, "fp", S * N * F, (torch.int32,))
        _oor(counts, entries, cap, S, self.n_outputs)
        rc = lib().qi_gpu_fingerprint(
            self.h, ids.data_ptr(), N, kk.ctypes.data_as(C.c_void_p), F, int(first_col),
            *_row_args(data), *_row_args(coded),
            _ptr(counts), _ptr(entries), int(cap),
            work.data_ptr(), fp.data_ptr(), words, S, self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_fingerprint failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    PATCH_ABSOLUTE, PATCH_DELTA = 0, 1  # QI_PATCH_ABSOLUTE, QI_PATCH_DELTA
    # QI_PATCH_* per-stripe status
    (PATCH_NONE, PATCH_DONE, PATCH_UNLOCATED, PATCH_TRUNCATED, PATCH_BAD_FIX, PATCH_DATA_MARK,
     PATCH_BUCKET_FULL) = range(7)
    PATCH_MAX_FIXES = 262144  # QI_PATCH_MAX_FIXES

    def patch_kernels(self, n_listed, mode, words):
        """'patch=<kernel>' (qi_gpu_patch_kernels); '' for arguments out of
        range."""
        return lib().qi_gpu_patch_kernels(self.h, n_listed, mode, words).decode()

    def patch_work_bytes(self, n_listed, n_stripes):
        """Bytes of the work buffer of a patch (0: arguments out of range)."""
        return lib().qi_gpu_patch_work_bytes(self.h, n_listed, n_stripes)

    def patch(self, mode, ids, fix_counts, fixes, fix_cap, coded, status, applied, work,
              data=None, mine=None, stripes=None, unlocated=None, counts=None, entries=None,
              cap=0, stream=None, check=True):
        """Apply a locate's fix lists to the rows and buckets (qi_gpu_patch).
        mode: PATCH_ABSOLUTE for the lists of locate / locate_multi,
        PATCH_DELTA for syndrome_locate's.  ids: int16 [S, N], the ids given
        to the locate's context; fix_counts [S], fixes [S, fix_cap, 3] and
        unlocated [S] as the locate left them; mine: uint8 [S, N], 0 = that
        fragment is not held here.  coded: [S_all, n_out, P] with its buckets
        counts / entries, data: [S_all, k, P] for systematic codes (either may
        be None when no applied fix lives there); stripes as for locate.
        status and applied: int32 [S], written by the call; work: uint8 of
        patch_work_bytes(N, S).  All or nothing per stripe.  Returns the
        sticky error flags when check."""
        import torch
        if mode not in (self.PATCH_ABSOLUTE, self.PATCH_DELTA):
            raise ValueError("patch: mode must be PATCH_ABSOLUTE or PATCH_DELTA")
        if ids.dim() != 2:
            raise ValueError("ids: expected [S, N]")
        S, N = ids.shape
        S_all = P = None
        for t, name, rows in ((coded, "coded", self.n_outputs), (data, "data", self.k)):
            if t is None:
                continue
            _rows(t, name, rows, S_all)
            if P is not None and t.shape[2] != P:
                raise ValueError("data and coded differ in width")
            S_all, P = t.shape[0], t.shape[2]
        if P is None or (coded is None and not self.sys):
            raise ValueError("no rows given")
        if data is not None and not self.sys:
            data = None
        if stripes is not None:
            _flat(stripes, "stripes", S, (torch.int32,))
            if stripes.numel() != S:
                raise ValueError(f"stripes: expected {S} list positions")
            if check and S > 0 and not (0 <= int(stripes.min()) and int(stripes.max()) < S_all):
                raise ValueError(f"stripes: values must lie in [0, {S_all})")
        elif S != S_all:
            raise ValueError(f"ids: expected {S_all} stripes, got {S}")
        need = self.patch_work_bytes(N, S)
        if need == 0:
            raise ValueError("patch: n_listed out of range (1 .. k + m), or no stripe")
        if fix_cap < 0 or (fix_cap > 0 and fixes is None):
            raise ValueError("fix_cap > 0 needs fixes")
        _flat(ids, "ids", S * N, (torch.int16, torch.uint16))
        _flat(mine, "mine", S * N, (torch.uint8,))
        _flat(unlocated, "unlocated", S, (torch.int32,))
        for t, name in ((fix_counts, "fix_counts"), (status, "status"), (applied, "applied")):
            if t is None:
                raise ValueError(f"{name}: required")
            _flat(t, name, S, (torch.int32,))
        _flat(fixes, "fixes", S * fix_cap * 3, (torch.int32,))
        if work is None:
            raise ValueError("work: required")
        _flat(work, "work", need, (torch.uint8,))
        _oor(counts, entries, cap, S_all, self.n_outputs)
        rc = lib().qi_gpu_patch(
            self.h, int(mode), ids.data_ptr(), N, _ptr(mine), _ptr(stripes), _ptr(unlocated),
            fix_counts.data_ptr(), _ptr(fixes), int(fix_cap), *_row_args(data),
            *_row_args(coded), _ptr(counts), _ptr(entries), int(cap), work.data_ptr(),
            status.data_ptr(), applied.data_ptr(), P, S, self._stream(stream))
        if rc:
            raise RuntimeError(f"qi_gpu_patch failed: {rc}")
        return lib().qi_gpu_take_error(self.h) if check else 0

    def take_error(self):
        return lib().qi_gpu_take_error(self.h)


class Fec:
    """Block API (qi::fec::RsFnt via the qi_fec_* C view)."""

    def __init__(self, k, m, systematic=False):
        require_device()
        self.k, self.m, self.sys = k, m, bool(systematic)
        self.h = lib().qi_fec_new(int(systematic), k, m)
        if not self.h:
            raise ValueError("qi_fec_new failed")
        self.n_outputs = lib().qi_fec_n_outputs(self.h)

    def repair_blocks(self, data, parities, oor, counts, missing, targets,
                      out_cap=64):
        """Rebuild the missing fragments `targets` (fragment ids) from the
        first k present ones in one pass (qi_fec_repair_blocks).  data: k
        uint8 rows or None entries (None as a whole for non-systematic
        codes); parities: n_outputs rows or None; oor (n_outputs, cap) uint32
        and counts (n_outputs,) uint32: the coded rows' marks; missing: k + m
        flags.  Returns (rows, out_oor, out_counts): the rebuilt uint8 rows,
        their ascending marks (len(targets), out_cap) and exact counts; None
        when fewer than k fragments are present.  Raises ValueError for an
        unsupported shape (k > 256, more than min(64, m) targets, a block
        wider than one staging chunk)."""
        import numpy as np
        rows = [r for r in list(data or []) + list(parities) if r is not None]
        B = len(rows[0])
        tg = np.ascontiguousarray(targets, np.int32)
        miss = np.ascontiguousarray(missing, np.int32)
        oor = np.ascontiguousarray(oor, np.uint32)
        counts = np.ascontiguousarray(counts, np.uint32)
        outs = [np.zeros(B, np.uint8) for _ in range(len(tg))]
        o_oor = np.zeros((len(tg), out_cap), np.uint32)
        o_cnt = np.zeros(len(tg), np.uint32)
        rc = lib().qi_fec_repair_blocks(
            self.h, ptr_array(list(data)) if data is not None else None,
            ptr_array(list(parities)), oor.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p), oor.shape[1],
            miss.ctypes.data_as(C.c_void_p), tg.ctypes.data_as(C.c_void_p),
            len(tg), ptr_array(outs), o_oor.ctypes.data_as(C.c_void_p),
            o_cnt.ctypes.data_as(C.c_void_p), out_cap, B)
        if rc == -2:
            raise ValueError("repair_blocks: shape not supported")
        if rc < 0:
            raise RuntimeError(f"qi_fec_repair_blocks failed: {rc}")
        return (outs, o_oor, o_cnt) if rc == 1 else None

    def verify_blocks(self, data, parities, oor, counts, missing):
        """Check the present fragments against each other in one pass on the
        device (qi_fec_verify_blocks): the first k present ones are the
        basis, every other present one is recomputed and compared with its
        row and its marks.  Arguments as repair_blocks.  Returns an int64
        array (k + m, 3): per fragment id [value mismatches, mark
        mismatches, first mismatching column or 0xFFFFFFFF], or [-1, -1, -1]
        for a missing or a basis fragment; None when fewer than k + 1
        fragments are present.  Raises ValueError for an unsupported shape
        (k > 256, a block wider than one staging chunk)."""
        import numpy as np
        rows = [r for r in list(data or []) + list(parities) if r is not None]
        B = len(rows[0])
        miss = np.ascontiguousarray(missing, np.int32)
        oor = np.ascontiguousarray(oor, np.uint32)
        counts = np.ascontiguousarray(counts, np.uint32)
        res = np.full((self.k + self.m, 3), -1, np.int64)
        rc = lib().qi_fec_verify_blocks(
            self.h, ptr_array(list(data)) if data is not None else None,
            ptr_array(list(parities)), oor.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p), oor.shape[1],
            miss.ctypes.data_as(C.c_void_p), res.ctypes.data_as(C.c_void_p), B)
        if rc == -2:
            raise ValueError("verify_blocks: shape not supported")
        if rc < 0:
            raise RuntimeError(f"qi_fec_verify_blocks failed: {rc}")
        return res if rc == 1 else None

    def locate_blocks(self, data, parities, oor, counts, missing, correct=False,
                      max_errors=None):
        """Which fragment is wrong in which columns (qi_fec_locate_blocks):
        the first min(present, k + 8) present fragments are listed.  Arguments
        as verify_blocks; oor (n_outputs, cap) and counts (n_outputs,) must be
        contiguous uint32 arrays (counts None: no marks).  Returns an int64
        array of k + m + 1 values: per fragment id the number of columns
        located in it (-1: missing or not listed), then the number of bad
        columns that could not be attributed; None when fewer than k + 2
        fragments are present.  correct=True returns (that array, patched):
        when there are located columns and none is unlocated, the rows (uint8
        numpy arrays, written in place), oor and counts are corrected and
        patched is True.  Raises ValueError for an unsupported shape (k > 256,
        m < 2, a block wider than one staging chunk).
        max_errors=t (1 .. 4) decodes up to t bad fragments per column
        (qi_fec_locate_multi_blocks): a located column counts in each of its
        fragments, the array has t more values, the columns located with
        1 .. t fragments, and None is also returned when fewer than k + 2 t
        fragments are listed.  None keeps the single-fragment call."""
        import numpy as np
        rows = [r for r in list(data or []) + list(parities) if r is not None]
        B = len(rows[0])
        miss = np.ascontiguousarray(missing, np.int32)
        for a in (oor, counts):
            if a is not None and (a.dtype != np.uint32 or not a.flags.c_contiguous):
                raise TypeError("oor, counts: expected contiguous uint32 arrays")
        if max_errors is not None:
            t = int(max_errors)
            if not 1 <= t <= Plan.LOCATE_MAX_ERRORS:
                raise ValueError("locate_blocks: max_errors must be 1 .. 4")
            res = np.full(self.k + self.m + 1 + t, -1, np.int64)
            rc = lib().qi_fec_locate_multi_blocks(
                self.h, ptr_array(list(data)) if data is not None else None,
                ptr_array(list(parities)), oor.ctypes.data_as(C.c_void_p),
                counts.ctypes.data_as(C.c_void_p) if counts is not None else None,
                oor.shape[1], miss.ctypes.data_as(C.c_void_p), t,
                res.ctypes.data_as(C.c_void_p), int(bool(correct)), B)
            if rc == -2:
                raise ValueError("locate_blocks: shape not supported")
            if rc < 0:
                raise RuntimeError(f"qi_fec_locate_multi_blocks failed: {rc}")
            if rc == 0:
                return None
            return (res, rc == 2) if correct else res
        res = np.full(self.k + self.m + 1, -1, np.int64)
        rc = lib().qi_fec_locate_blocks(
            self.h, ptr_array(list(data)) if data is not None else None,
            ptr_array(list(parities)), oor.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p) if counts is not None else None,
            oor.shape[1], miss.ctypes.data_as(C.c_void_p),
            res.ctypes.data_as(C.c_void_p), int(bool(correct)), B)
        if rc == -2:
            raise ValueError("locate_blocks: shape not supported")
        if rc < 0:
            raise RuntimeError(f"qi_fec_locate_blocks failed: {rc}")
        if rc == 0:
            return None
        return (res, rc == 2) if correct else res

    def fingerprint_blocks(self, data, parities, oor, counts, missing, keys):
        """Fingerprints of every present fragment (qi_fec_fingerprint_blocks):
        arguments as verify_blocks (counts None: no marks), keys: F triples
        (a, b, d), each in 1 .. 65536.  Returns an int64 array (k + m, F): per
        fragment id its F fingerprints in [0, 65536], -1 for a missing
        fragment.  Any k and any block width."""
        import numpy as np
        kk = Plan._keys(keys)
        rows = [r for r in list(data or []) + list(parities) if r is not None]
        B = len(rows[0])
        miss = np.ascontiguousarray(missing, np.int32)
        for a in (oor, counts):
            if a is not None and (a.dtype != np.uint32 or not a.flags.c_contiguous):
                raise TypeError("oor, counts: expected contiguous uint32 arrays")
        res = np.full((self.k + self.m, kk.shape[0]), -1, np.int64)
        rc = lib().qi_fec_fingerprint_blocks(
            self.h, ptr_array(list(data)) if data is not None else None,
            ptr_array(list(parities)),
            oor.ctypes.data_as(C.c_void_p) if oor is not None else None,
            counts.ctypes.data_as(C.c_void_p) if counts is not None else None,
            oor.shape[1] if oor is not None else 0, miss.ctypes.data_as(C.c_void_p),
            kk.ctypes.data_as(C.c_void_p), kk.shape[0], res.ctypes.data_as(C.c_void_p), B)
        if rc != 1:
            raise RuntimeError(f"qi_fec_fingerprint_blocks failed: {rc}")
        return res

    def check_fingerprints(self, fp, missing, max_errors=1):
        """The coordinator's half of a scrub by fingerprints: fp is the
        (k + m, F) table of the fragments' fingerprints under the same F keys
        (fingerprint_blocks, or gathered from the nodes; rows of missing
        fragments are ignored).  The fingerprints of a stripe's fragments are
        a codeword in each of the F columns, so the present ones are laid out
        as blocks of F words, a value of 65536 as a mark, and handed to
        locate_blocks (max_errors 1: the single-fragment locate, 2 .. 4: up to
        that many bad fragments).  Returns that call's array: per fragment id
        the number of the F columns located in it (-1: missing or not
        listed), then the unlocated columns (then, max_errors > 1, the columns
        located with 1 .. max_errors fragments); None when too few fragments
        are present.  Locate's limits hold: k <= 256 and at least k + 2
        fragments present (ValueError otherwise).  A systematic data
        fragment's fingerprint equal to 65536 cannot be stored in a data row:
        ValueError -- draw another key (probability 1 / 65537 per data
        fragment and key)."""
        import numpy as np
        fp = np.asarray(fp, np.int64)
        n = self.k + self.m
        if fp.ndim != 2 or fp.shape[0] != n or fp.shape[1] < 1:
            raise ValueError("fp: expected a (k + m, F) table")
        F = fp.shape[1]
        miss = np.ascontiguousarray(missing, np.int32)
        first = self.k if self.sys else 0
        rows = [None] * n
        oor = np.zeros((self.n_outputs, F), np.uint32)
        counts = np.zeros(self.n_outputs, np.uint32)
        for f in range(n):
            if miss[f]:
                continue
            v = fp[f]
            if v.min() < 0 or v.max() > 65536:
                raise ValueError(f"fp: fragment {f} holds no fingerprints")
            marks = np.flatnonzero(v == 65536)
            if len(marks) and f < first:
                raise ValueError(f"data fragment {f} has a fingerprint of 65536: "
                                 "draw another key")
            if f >= first:
                counts[f - first] = len(marks)
                oor[f - first, :len(marks)] = marks
            rows[f] = np.ascontiguousarray((v & 0xffff).astype(np.uint16)).view(np.uint8)
        return self.locate_blocks(rows[:first] if self.sys else None, rows[first:], oor,
                                  counts, miss,
                                  max_errors=None if max_errors == 1 else max_errors)

    def update_blocks(self, ids, old_rows, new_rows, parities, oor, counts):
        """Delta update (qi_fec_update_blocks): data rows `ids` go from
        old_rows[u] to new_rows[u] (uint8 rows); parities: n_outputs uint8
        rows, None where the fragment is not held -- the held ones are updated
        in place.  oor (n_outputs, cap) uint32 and counts (n_outputs,) uint32
        hold their marks and are replaced, for the held rows, by the new marks
        (ascending, counts exact).  Raises ValueError for an unsupported shape
        (more than min(8, k) rows, a block wider than one staging chunk)."""
        import numpy as np
        idv = np.ascontiguousarray(ids, np.int32)
        if oor.dtype != np.uint32 or counts.dtype != np.uint32 or not (
                oor.flags.c_contiguous and counts.flags.c_contiguous):
            raise TypeError("oor, counts: expected contiguous uint32 arrays")
        rc = lib().qi_fec_update_blocks(
            self.h, idv.ctypes.data_as(C.c_void_p), len(idv),
            ptr_array(list(old_rows)), ptr_array(list(new_rows)),
            ptr_array(list(parities)), oor.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p), oor.shape[1], len(old_rows[0]))
        if rc == -2:
            raise ValueError("update_blocks: shape not supported")
        if rc != 1:
            raise RuntimeError(f"qi_fec_update_blocks failed: {rc}")

    def partial_repair_blocks(self, ids, held_ids, rows, oor, counts, targets, acc=None,
                              out_cap=64):
        """Partial repair (qi_fec_partial_repair_blocks): the share of the
        repair of `targets` from the k helper fragments `ids` that the holder
        of the fragments `held_ids` (each one of ids) can form.  rows[h]:
        fragment held_ids[h] (uint8 rows); oor (len(held_ids), cap) uint32 and
        counts uint32: their marks by position h (None: no marks).  acc: the
        (rows, out_oor, out_counts) another call returned, to add to (None:
        start from 0).  Returns (rows, out_oor, out_counts): the len(targets)
        partial rows, their ascending marks (len(targets), cap') and exact
        counts; summed over any partition of ids they are the rebuilt
        fragments.  Raises ValueError for an unsupported shape (no or more
        than k held rows, more than min(8, m) targets, a block wider than one
        staging chunk)."""
        import numpy as np
        idv = np.ascontiguousarray(ids, np.int32)
        hv = np.ascontiguousarray(held_ids, np.int32)
        tg = np.ascontiguousarray(targets, np.int32)
        if len(idv) != self.k or len(rows) != len(hv):
            raise ValueError("partial_repair_blocks: k ids and one row per held id")
        if len(hv) == 0:
            raise ValueError("partial_repair_blocks: shape not supported")
        return self._share_blocks(
            "partial_repair_blocks", "target", hv, rows, oor, counts, len(tg), acc, out_cap,
            lambda held, out: lib().qi_fec_partial_repair_blocks(
                self.h, idv.ctypes.data_as(C.c_void_p), *held, tg.ctypes.data_as(C.c_void_p),
                len(tg), *out))

    def _share_blocks(self, name, noun, hv, rows, oor, counts, R, acc, out_cap, call):
        """The staging of partial_repair_blocks and syndrome_blocks: the held
        rows and their marks, R output rows started from acc, and the call
        again with the exact capacity when a mark list did not fit.
        call(held, out): the C call, given its held-row and its output
        arguments."""
        import numpy as np
        B = len(rows[0])
        if oor is not None:
            oor = np.ascontiguousarray(oor, np.uint32).reshape(len(hv), -1)
            counts = np.ascontiguousarray(counts, np.uint32)
        if acc is not None:
            a_rows, a_oor, a_cnt = acc
            if len(a_rows) != R or int(np.max(a_cnt, initial=0)) > a_oor.shape[1]:
                raise ValueError(f"{name}: acc needs one row per {noun} "
                                 "and complete mark lists")
            out_cap = max(out_cap, a_oor.shape[1])
        while True:
            outs = [np.zeros(B, np.uint8) for _ in range(R)]
            o_oor = np.zeros((R, out_cap), np.uint32)
            o_cnt = np.zeros(R, np.uint32)
            if acc is not None:
                for j in range(R):
                    outs[j][:] = a_rows[j]
                o_oor[:, :a_oor.shape[1]] = a_oor
                o_cnt[:] = a_cnt
            rc = call(
                (hv.ctypes.data_as(C.c_void_p), len(hv), ptr_array(list(rows)),
                 oor.ctypes.data_as(C.c_void_p) if oor is not None else None,
                 counts.ctypes.data_as(C.c_void_p) if oor is not None else None,
                 oor.shape[1] if oor is not None else 0),
                (int(acc is not None), ptr_array(outs), o_oor.ctypes.data_as(C.c_void_p),
                 o_cnt.ctypes.data_as(C.c_void_p), out_cap, B))
            if rc == -2:
                raise ValueError(f"{name}: shape not supported")
            if rc != 1:
                raise RuntimeError(f"qi_fec_{name} failed: {rc}")
            if o_cnt.max(initial=0) <= out_cap:
                return outs, o_oor, o_cnt
            out_cap = int(o_cnt.max())   # the list did not fit: once more

    def syndrome_blocks(self, listed_ids, held_ids, rows, oor, counts, n_checks, acc=None,
                        out_cap=64):
        """Syndrome share (qi_fec_syndrome_blocks): the share of the n_checks
        syndrome rows of the k + n_checks listed fragments `listed_ids` that
        the holder of the fragments `held_ids` (each one of listed_ids) can
        form, at any k.  rows, oor, counts and acc as partial_repair_blocks.
        Returns (rows, out_oor, out_counts): the n_checks partial syndrome
        rows, their ascending marks and exact counts; summed over any
        partition of listed_ids they are the stripe's syndromes (all 0 when it
        is intact).  Raises ValueError for an unsupported shape."""
        import numpy as np
        idv = np.ascontiguousarray(listed_ids, np.int32)
        hv = np.ascontiguousarray(held_ids, np.int32)
        R = int(n_checks)
        if len(rows) != len(hv):
            raise ValueError("syndrome_blocks: one row per held id")
        if len(hv) == 0 or R < 1 or len(idv) != self.k + R:
            raise ValueError("syndrome_blocks: shape not supported")
        return self._share_blocks(
            "syndrome_blocks", "check", hv, rows, oor, counts, R, acc, out_cap,
            lambda held, out: lib().qi_fec_syndrome_blocks(
                self.h, idv.ctypes.data_as(C.c_void_p), len(idv), *held, R, *out))

    def locate_syndromes(self, listed_ids, rows, oor, counts, max_errors=1, fix_cap=256):
        """The coordinator's decision over the complete syndrome sums
        (qi_fec_locate_syndromes): rows, oor, counts as syndrome_blocks
        returned them, R = len(listed_ids) - k of them.  0 <= max_errors <=
        R // 2.  Returns (result, fixes): result an int64 array of k + m + 1 +
        max_errors values -- per fragment id the located columns it takes part
        in (-1: not listed), the unlocated columns, the columns located with
        1 .. max_errors fragments -- and fixes an int64 array (n, 3) of
        (column, fragment id, e): that fragment is off by e there, its true
        symbol is (y - e) mod 65537 (apply_deltas)."""
        import numpy as np
        idv = np.ascontiguousarray(listed_ids, np.int32)
        t = int(max_errors)
        B = len(rows[0])
        if oor is not None:
            oor = np.ascontiguousarray(oor, np.uint32).reshape(len(rows), -1)
            counts = np.ascontiguousarray(counts, np.uint32)
        res = np.full(self.k + self.m + 1 + max(t, 0), -1, np.int64)
        n = C.c_uint32(0)
        while True:
            fx = np.zeros((max(fix_cap, 1), 3), np.uint32)
            rc = lib().qi_fec_locate_syndromes(
                self.h, idv.ctypes.data_as(C.c_void_p), len(idv), ptr_array(list(rows)),
                oor.ctypes.data_as(C.c_void_p) if oor is not None else None,
                counts.ctypes.data_as(C.c_void_p) if oor is not None else None,
                oor.shape[1] if oor is not None else 0, t,
                res.ctypes.data_as(C.c_void_p), fx.ctypes.data_as(C.c_void_p), fix_cap,
                C.byref(n), B)
            if rc == -2:
                raise ValueError("locate_syndromes: shape not supported")
            if rc != 1:
                raise RuntimeError(f"qi_fec_locate_syndromes failed: {rc}")
            if n.value <= fix_cap:
                return res, fx[:n.value].astype(np.int64)
            fix_cap = n.value

    def apply_deltas(self, fragment_ids, rows, oor, counts, fixes):
        """The holder's step (qi_fec_apply_deltas, no device): applies the
        fixes of locate_syndromes that name one of `fragment_ids` to rows[h]
        (uint8 numpy arrays, written in place) and to their ascending mark
        lists oor (len(fragment_ids), cap) / counts (contiguous uint32 arrays,
        updated in place; None: no marks, and none can be written); fixes for
        other fragments are skipped.  Returns the number applied, or None with
        nothing touched when the patch is refused: a data row would have to
        hold 65536, or a mark list would outgrow cap."""
        import numpy as np
        fv = np.ascontiguousarray(fragment_ids, np.int32)
        for a in (oor, counts):
            if a is not None and (a.dtype != np.uint32 or not a.flags.c_contiguous):
                raise TypeError("oor, counts: expected contiguous uint32 arrays")
        fx = np.ascontiguousarray(fixes, np.uint32).reshape(-1, 3)
        if len(rows) != len(fv):
            raise ValueError("apply_deltas: one row per fragment id")
        rc = lib().qi_fec_apply_deltas(
            self.h, fv.ctypes.data_as(C.c_void_p), len(fv), ptr_array(list(rows)),
            oor.ctypes.data_as(C.c_void_p) if oor is not None else None,
            counts.ctypes.data_as(C.c_void_p) if counts is not None else None,
            oor.shape[1] if oor is not None else 0, fx.ctypes.data_as(C.c_void_p), len(fx),
            len(rows[0]) if len(rows) else 0)
        if rc == -3:
            return None
        if rc < 0:
            raise RuntimeError(f"qi_fec_apply_deltas failed: {rc}")
        return rc

    def scrub_blocks(self, data, parities, oor, counts, missing, max_errors=1, correct=False):
        """locate_blocks(max_errors=...) at any k (qi_fec_scrub_blocks): the
        first min(present, k + 8) present fragments are listed, their syndrome
        rows formed on the device and decided from those alone.  Arguments and
        results as locate_blocks with max_errors; max_errors = 0 only detects
        (every bad column is unlocated).  None when fewer than k + max(1, 2
        max_errors) fragments are listed."""
        import numpy as np
        rows = [r for r in list(data or []) + list(parities) if r is not None]
        B = len(rows[0])
        miss = np.ascontiguousarray(missing, np.int32)
        for a in (oor, counts):
            if a is not None and (a.dtype != np.uint32 or not a.flags.c_contiguous):
                raise TypeError("oor, counts: expected contiguous uint32 arrays")
        t = int(max_errors)
        if not 0 <= t <= Plan.SYNDROME_MAX_ERRORS:
            raise ValueError("scrub_blocks: max_errors must be 0 .. 4")
        res = np.full(self.k + self.m + 1 + t, -1, np.int64)
        rc = lib().qi_fec_scrub_blocks(
            self.h, ptr_array(list(data)) if data is not None else None,
            ptr_array(list(parities)), oor.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p) if counts is not None else None,
            oor.shape[1], miss.ctypes.data_as(C.c_void_p), t,
            res.ctypes.data_as(C.c_void_p), int(bool(correct)), B)
        if rc == -2:
            raise ValueError("scrub_blocks: shape not supported")
        if rc < 0:
            raise RuntimeError(f"qi_fec_scrub_blocks failed: {rc}")
        if rc == 0:
            return None
        return (res, rc == 2) if correct else res

    def close(self):
        if self.h:
            lib().qi_fec_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Nf4:
    """RS-NF4 block API (qi::fec::RsNf4 via the qi_nf4_* C view)."""

    def __init__(self, word_size, k, m):
        require_device()
        self.ws, self.k, self.m = word_size, k, m
        self.h = lib().qi_nf4_new(word_size, k, m)
        if not self.h:
            raise ValueError(f"qi_nf4_new({word_size}, {k}, {m}) failed")
        self.n_outputs = lib().qi_nf4_n_outputs(self.h)

    def encode(self, data, outputs, oor, flags, counts):
        """data: k uint8 rows; outputs: n_outputs rows (None = unwanted);
        oor/flags: (n_outputs, cap) uint32; counts: (n_outputs,) uint32."""
        rc = lib().qi_nf4_encode_blocks(
            self.h, ptr_array(data), ptr_array(outputs), len(data[0]),
            oor.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p), oor.shape[1])
        if rc:
            raise RuntimeError(f"qi_nf4_encode_blocks failed: {rc}")

    def decode(self, data, parities, oor, flags, counts, missing, wanted):
        """Returns 1 (decoded) or 0 (fewer than k fragments)."""
        rc = lib().qi_nf4_decode_blocks(
            self.h, ptr_array(data), ptr_array(parities),
            oor.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p),
            counts.ctypes.data_as(C.c_void_p), oor.shape[1],
            missing.ctypes.data_as(C.c_void_p),
            wanted.ctypes.data_as(C.c_void_p), len(data[0]))
        if rc < 0:
            raise RuntimeError(f"qi_nf4_decode_blocks failed: {rc}")
        return rc

    def close(self):
        if self.h:
            lib().qi_nf4_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class QuadironFnt32:
    """The drop-in C-ABI handle (include/quadiron_c.h)."""

    def __init__(self, word_size, n_data, n_parities, systematic):
        self.h = lib().quadiron_fnt32_new(word_size, n_data, n_parities,
                                          int(systematic))
        if not self.h:
            raise ValueError("quadiron_fnt32_new returned NULL")
        self.k, self.m, self.sys = n_data, n_parities, bool(systematic)

    def metadata_size(self, block_size):
        return lib().quadiron_fnt32_get_metadata_size(self.h, block_size)

    def encode(self, data, parity, wanted, block_size):
        return lib().quadiron_fnt32_encode(
            self.h, ptr_array(data), ptr_array(parity),
            wanted.ctypes.data_as(C.c_void_p), block_size)

    def decode(self, data, parity, missing, block_size):
        return lib().quadiron_fnt32_decode(
            self.h, ptr_array(data), ptr_array(parity),
            missing.ctypes.data_as(C.c_void_p), block_size)

    def reconstruct(self, data, parity, missing, dest, block_size):
        return lib().quadiron_fnt32_reconstruct(
            self.h, ptr_array(data), ptr_array(parity),
            missing.ctypes.data_as(C.c_void_p), dest, block_size)

    def close(self):
        if self.h:
            lib().quadiron_fnt32_delete(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
