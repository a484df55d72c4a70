"""ppals — ctypes binding of libppals.so (include/ppals.h), the MI355X-native ALS sweep engine.

This is plumbing for tests/ and bench.py; the product is the C-ABI library and the C++ `test_ALS`
driver. There is no CPU fallback: creating a Context without a HIP device raises PpalsError.

Names follow the reference (LinjianMa/pairwise-perturbation): `alsCP_DT`, `alsCP_PP`, `hosvd`,
`alsTucker_DT` take the same arguments in the same order as als_CP.h:30-32,105-108 and
als_Tucker.h:14-15,46-48, minus the CTF `World` (the Context) and the always-zero `F`.

Array conventions: tensors are Fortran-ordered numpy fp64 arrays (first index fastest, like CTF);
factor matrices are (s_i, R) Fortran-ordered.
"""
import ctypes as C
import os
import weakref

import numpy as np

F32, F64 = 0, 1
F16, BF16 = 2, 3  # F16: a device view only; BF16: a view, or the tensor's storage (CP only)
U8 = 4  # a mask view only (CP / Tucker.impute_device): one byte per element, 0 = missing
_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.environ.get("PPALS_LIB", os.path.join(os.path.dirname(_HERE), "lib", "libppals.so"))
_lib = None

c_dp = C.POINTER(C.c_double)


class PpalsError(RuntimeError):
    pass


class _Opts(C.Structure):
    _fields_ = [("tol", C.c_double), ("timelimit", C.c_double), ("maxiter", C.c_int),
                ("lambda_", C.c_double), ("resprint", C.c_int), ("bench", C.c_int),
                ("tol_init", C.c_double), ("ratio_step", C.c_double), ("csv_path", C.c_char_p),
                ("csv_append", C.c_int), ("verbose", C.c_int),
                ("update_percentage", C.c_double)]


EXPORTS = [
    "ppals_last_error", "ppals_version", "ppals_preload_eigensolver", "ppals_ctx_create",
    "ppals_ctx_destroy",
    "ppals_get_unique_id", "ppals_ctx_init_comm", "ppals_ctx_rank", "ppals_ctx_nranks",
    "ppals_ctx_sync", "ppals_profile_enable", "ppals_profile_read", "ppals_profile_reset",
    "ppals_tensor_create", "ppals_tensor_destroy", "ppals_tensor_local_rows",
    "ppals_tensor_fill_cp", "ppals_tensor_fill_uniform", "ppals_tensor_upload",
    "ppals_tensor_download", "ppals_tensor_import_device", "ppals_tensor_export_device",
    "ppals_tensor_check_device_view",
    "ppals_tensor_fill_laplacian", "ppals_tensor_fill_collinear", "ppals_collinear_factors",
    "ppals_tensor_norm", "ppals_fill_uniform_host", "ppals_tree_node", "ppals_mttkrp",
    "ppals_pp_operator", "ppals_cp_residual", "ppals_cp_gram_system", "ppals_cp_create",
    "ppals_cp_destroy", "ppals_cp_set_factors", "ppals_cp_get_factors", "ppals_cp_sweeps_dt",
    "ppals_cp_gradnorm", "ppals_cp_dt", "ppals_cp_pp", "ppals_cp_pp_partupdate",
    "ppals_cpd_als", "ppals_cpd_als_lr", "ppals_cp_set_schedule", "ppals_cp_get_schedule", "ppals_cp_placement_report", "ppals_cp_pp_build_stats",
    "ppals_tucker_create",
    "ppals_tucker_destroy", "ppals_tucker_set_factors", "ppals_tucker_get_factors",
    "ppals_tucker_set_core",
    "ppals_tucker_hosvd", "ppals_tucker_ttmc", "ppals_tucker_sweeps_dt", "ppals_tucker_dt",
    "ppals_tucker_pp", "ppals_cp_export_model_device", "ppals_tucker_export_model_device",
    "ppals_cp_multi_create", "ppals_cp_multi_destroy", "ppals_cp_multi_set_factors",
    "ppals_cp_multi_get_factors", "ppals_cp_multi_set_schedule", "ppals_cp_multi_sweeps",
    "ppals_cp_multi_residuals", "ppals_cp_multi_gradnorms", "ppals_cp_multi_run",
    "ppals_cp_multi_take", "ppals_cp_impute_device", "ppals_cp_em", "ppals_cp_wls_device", "ppals_cp_wls",
    "ppals_cp_huber_device", "ppals_cp_robust", "ppals_cp_abs_residual_quantile",
    "ppals_cp_set_nonneg", "ppals_cp_get_nonneg",
    "ppals_cp_multi_set_nonneg", "ppals_cp_multi_get_nonneg",
    "ppals_cp_multi_create_ranks", "ppals_cp_multi_ranks",
    "ppals_cp_core_consistency", "ppals_cp_multi_core_consistency", "ppals_cp_multi_core",
    "ppals_tucker_impute_device", "ppals_tucker_em",
    "ppals_match_columns", "ppals_cp_congruence", "ppals_cp_fms", "ppals_cp_multi_congruence",
    "ppals_cp_multi_fms", "ppals_cp_multi_fms_between",
    "ppals_cp_slice_residuals", "ppals_cp_leverages",
    "ppals_tucker_residual", "ppals_tucker_slice_residuals", "ppals_tucker_leverages",
    "ppals_cp_multi_set_holdout", "ppals_cp_multi_get_holdout", "ppals_cp_multi_heldout_scores",
    "ppals_cp_multi_take_predicted",
    "ppals_cp_set_mode_constraints", "ppals_cp_get_mode_constraints",
    "ppals_cp_multi_set_mode_constraints", "ppals_cp_multi_get_mode_constraints",
    "ppals_cp_set_mode_shapes", "ppals_cp_get_mode_shapes",
    "ppals_cp_multi_set_mode_shapes", "ppals_cp_multi_get_mode_shapes",
    "ppals_tensor_center", "ppals_tensor_shift", "ppals_tensor_slice_sumsq", "ppals_tensor_scale",
    "ppals_tensor_rescale",
    "ppals_parafac2_create", "ppals_parafac2_destroy", "ppals_parafac2_cp", "ppals_parafac2_tensor",
    "ppals_parafac2_step_device",
    "ppals_parafac2_run", "ppals_parafac2_projections", "ppals_parafac2_projections_device",
    "ppals_parafac2_create_ragged", "ppals_parafac2_rows", "ppals_parafac2_step_ragged_device",
    "ppals_parafac2_run_ragged",
    "ppals_npls_fit", "ppals_npls_destroy", "ppals_npls_dims", "ppals_npls_get", "ppals_npls_predict",
    "ppals_tensor_contract_mode", "ppals_tensor_slice_inner",
    "ppals_tensor_contract_columns", "ppals_tensor_slice_inner_columns", "ppals_npls_crossval",
]
HOST, DEVICE = 0, 1  # PPALS_HOST / PPALS_DEVICE: where the offsets of Tensor.center / Tensor.shift lie
MODE_FREE, MODE_NONNEG, MODE_FIXED, MODE_ORTHO = 0, 1, 2, 3  # PPALS_MODE_*
MODE_KINDS = ("free", "nonneg", "fixed", "ortho")
SHAPE_NONE, SHAPE_UNIMODAL, SHAPE_INCREASING, SHAPE_DECREASING = 0, 1, 2, 3  # PPALS_SHAPE_*
SHAPE_KINDS = ("none", "unimodal", "increasing", "decreasing")
MODEL, RESIDUAL = 0, 1  # PPALS_MODEL / PPALS_RESIDUAL
FMS_WEIGHTS = 1  # PPALS_FMS_WEIGHTS


def _kinds(kinds, n):
    """a kind per mode, as ints or as the strings of MODE_KINDS, into a C array of n ints"""
    kinds = list(kinds)
    if len(kinds) != n:
        raise ValueError(f"one kind per mode: {n} expected, {len(kinds)} given")
    return (C.c_int * n)(*[MODE_KINDS.index(k) if isinstance(k, str) else int(k) for k in kinds])


def _shapes(shapes, n):
    """a shape per mode, as ints or as the strings of SHAPE_KINDS, into a C array of n ints"""
    shapes = list(shapes)
    if len(shapes) != n:
        raise ValueError(f"one shape per mode: {n} expected, {len(shapes)} given")
    return (C.c_int * n)(*[SHAPE_KINDS.index(k) if isinstance(k, str) else int(k) for k in shapes])


def lib(path=None):
    """load libppals.so; raises (loudly) when it has not been built"""
    global _lib
    if _lib is None:
        p = path or _LIBPATH
        if not os.path.exists(p):
            raise PpalsError(f"{p} not found: build it with `make -C pairwise-perturbation_amd` "
                             "(there is no pure-Python or CPU fallback)")
        _lib = C.CDLL(p)
        _lib.ppals_last_error.restype = C.c_char_p
        _lib.ppals_version.restype = C.c_char_p
        # the product binding only ever drives the HIP build; the host stand-in of tests/hostsim is
        # reachable solely through tests/hostsim_util.py, which loads this file under another name
        if __name__ == "ppals" and b"TEST INFRASTRUCTURE" in _lib.ppals_version():
            _lib = None
            raise PpalsError(f"{p} is the test stand-in, not the HIP engine (no CPU fallback)")
    return _lib


def _check(rc, allow_bool=False):
    if rc < 0:
        raise PpalsError(f"ppals error {rc}: {lib().ppals_last_error().decode()}")
    return rc


def _dp(a):
    return a.ctypes.data_as(c_dp)


def _torch():
    """torch, imported on first use only: `import ppals` works without it. It must have been imported
    before libppals was loaded for the two to share one HIP runtime (and so one view of pointers)."""
    import torch
    return torch


def flat(Ws):
    return np.concatenate([np.asfortranarray(W, dtype=np.float64).ravel(order="F") for W in Ws])


def unflat(wflat, lens, ranks):
    out, p = [], 0
    for s, r in zip(lens, ranks):
        out.append(wflat[p:p + s * r].reshape((s, r), order="F").copy(order="F"))
        p += s * r
    return out


def fill_uniform_host(n, seed, offset=0, lo=0.0, hi=1.0):
    out = np.empty(int(n), dtype=np.float64)
    lib().ppals_fill_uniform_host(_dp(out), C.c_int64(int(n)), C.c_uint64(seed),
                                  C.c_uint64(offset), C.c_double(lo), C.c_double(hi))
    return out


def init_factors(lens, R, seed):
    """W_i[e] = u01(seed + i, e): the deterministic stand-in for CTF's W[i].fill_random(0,1)"""
    return [fill_uniform_host(s * R, seed + i).reshape((s, R), order="F")
            for i, s in enumerate(lens)]


def collinear_factors(lens, R, col_min=0.5, col_max=0.9, seed=0):
    """the factor vectors of `-tensor c` (Gen_collinearity, common.cxx:361-423), lambda in mode 0"""
    wf = np.empty(sum(int(s) * R for s in lens))
    arr = (C.c_int64 * len(lens))(*[int(x) for x in lens])
    _check(lib().ppals_collinear_factors(len(lens), arr, R, C.c_double(col_min),
                                         C.c_double(col_max), C.c_uint64(seed), _dp(wf)))
    return unflat(wf, lens, [R] * len(lens))


def match_columns(score):
    """ppals_match_columns: the exact optimum of the rectangular assignment problem on score (ra, rb):
    (perm, total), perm[p] the column matched to row p or -1 (ra > rb), total the sum of the min(ra, rb)
    matched entries. Host only: needs no context and no device."""
    sc = np.asfortranarray(score, dtype=np.float64)
    if sc.ndim != 2:
        raise PpalsError("match_columns: score must be a matrix")
    ra, rb = sc.shape
    perm = (C.c_int * max(ra, 1))()
    total = C.c_double(0)
    _check(lib().ppals_match_columns(_dp(sc), ra, rb, ra, perm, C.byref(total)))
    return np.array(perm[:ra], dtype=np.int64), total.value


def _skip(skip_mode):
    return -1 if skip_mode is None else int(skip_mode)


def preload_eigensolver():
    """load rocBLAS / rocSOLVER now — call before anything initialises the HIP runtime in this
    process when a Tucker session with a mode extent > 64 will follow (include/ppals.h)"""
    _check(lib().ppals_preload_eigensolver())


class Context:
    """replaces CTF::World (test_ALS.cxx:200): one per process, one GPU"""

    def __init__(self, device=0):
        self.device = device
        self._h = C.c_void_p()
        self._children = weakref.WeakSet()  # tensors / sessions that must die before the context
        _check(lib().ppals_ctx_create(C.byref(self._h), device))

    def init_comm(self, rank, nranks, unique_id):
        _check(lib().ppals_ctx_init_comm(self._h, rank, nranks, unique_id))

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(lib().ppals_get_unique_id(buf))
        return buf.raw

    @property
    def rank(self):
        return lib().ppals_ctx_rank(self._h)

    @property
    def nranks(self):
        return lib().ppals_ctx_nranks(self._h)

    def sync(self):
        _check(lib().ppals_ctx_sync(self._h))

    def profile_enable(self, level=1):
        """0 off, 1 tensor scans only, 2 scans + the other bracketed kernels"""
        _check(lib().ppals_profile_enable(self._h, int(level)))

    def profile_reset(self):
        _check(lib().ppals_profile_reset(self._h))

    def profile_read(self, which=0):
        n, ms, by = C.c_int64(0), C.c_double(0), C.c_double(0)
        _check(lib().ppals_profile_read(self._h, which, C.byref(n), C.byref(ms), C.byref(by)))
        return n.value, ms.value, by.value

    def close(self):
        if self._h:
            for ch in sorted(list(self._children), key=lambda c: isinstance(c, Tensor)):
                ch.close()  # sessions first, then tensors
            lib().ppals_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tensor:
    """replaces CTF::Tensor<> V: dense, block-partitioned along the leading mode"""

    def __init__(self, ctx, lens, dtype=F32):
        self.ctx = ctx
        self.lens = [int(x) for x in lens]
        self.dtype = dtype
        self._h = C.c_void_p()
        arr = (C.c_int64 * len(lens))(*self.lens)
        _check(lib().ppals_tensor_create(ctx._h, len(lens), arr, dtype, C.byref(self._h)))
        ctx._children.add(self)

    def local_rows(self):
        lo, n = C.c_int64(0), C.c_int64(0)
        _check(lib().ppals_tensor_local_rows(self._h, C.byref(lo), C.byref(n)))
        return lo.value, n.value

    def fill_cp(self, Wtrue):
        wf = flat(Wtrue)
        _check(lib().ppals_tensor_fill_cp(self._h, Wtrue[0].shape[1], _dp(wf)))
        return self

    def fill_uniform(self, seed, lo=0.5, hi=1.0):
        _check(lib().ppals_tensor_fill_uniform(self._h, C.c_uint64(seed), C.c_double(lo),
                                               C.c_double(hi)))
        return self

    def fill_laplacian(self, ndigits, s):
        _check(lib().ppals_tensor_fill_laplacian(self._h, ndigits, s))
        return self

    def fill_collinear(self, R, col_min=0.5, col_max=0.9, ratio_noise=0.01, seed=0):
        _check(lib().ppals_tensor_fill_collinear(self._h, R, C.c_double(col_min),
                                                 C.c_double(col_max), C.c_double(ratio_noise),
                                                 C.c_uint64(seed)))
        return self

    def upload(self, V):
        Vf = np.asfortranarray(V, dtype=np.float64)
        assert list(Vf.shape) == self.lens
        _check(lib().ppals_tensor_upload(self._h, _dp(Vf)))
        return self

    def download(self):
        """the tensor as fp64, first index fastest (this rank's rows; zeros elsewhere)"""
        out = np.zeros(self.lens, dtype=np.float64, order="F")
        _check(lib().ppals_tensor_download(self._h, _dp(out)))
        return out

    # ---- device views: torch tensors (or any device pointer) in and out, no host round trip ----
    def _box(self, shape, lo):
        n = len(self.lens)
        if len(shape) != n:
            raise PpalsError(f"the view has {len(shape)} modes, the tensor {n}")
        lo = [0] * n if lo is None else [int(x) for x in lo]
        return (C.c_int64 * n)(*lo), (C.c_int64 * n)(*[int(x) for x in shape])

    def check_view(self, direction, ptr, dtype, shape, strides, lo=None):
        """ppals_tensor_check_device_view: PPALS_OK (0) or the error code the copy would return; the
        message is ppals_last_error(). direction 0 = import, 1 = export."""
        blo, blen = self._box(shape, lo)
        st = (C.c_int64 * len(self.lens))(*[int(x) for x in strides])
        return lib().ppals_tensor_check_device_view(self._h, int(direction), C.c_void_p(int(ptr)),
                                                    int(dtype), blo, blen, st)

    def import_device(self, ptr, dtype, shape, strides, lo=None, stream=0):
        """raw ppals_tensor_import_device: element (j_0, ...) of the box at lo is at
        ptr + sum_i j_i * strides[i] elements of type dtype (F32 / F64 / F16 / BF16)"""
        blo, blen = self._box(shape, lo)
        st = (C.c_int64 * len(self.lens))(*[int(x) for x in strides])
        _check(lib().ppals_tensor_import_device(self._h, C.c_void_p(int(ptr)), int(dtype), blo, blen,
                                                st, C.c_void_p(int(stream or 0))))
        return self

    def export_device(self, ptr, dtype, shape, strides, lo=None, stream=0):
        """raw ppals_tensor_export_device: this rank's rows of the box into the view (F32 / F64)"""
        blo, blen = self._box(shape, lo)
        st = (C.c_int64 * len(self.lens))(*[int(x) for x in strides])
        _check(lib().ppals_tensor_export_device(self._h, C.c_void_p(int(ptr)), int(dtype), blo, blen,
                                                st, C.c_void_p(int(stream or 0))))
        return self

    def _torch_view(self, x, dtypes):
        torch = _torch()
        if x.dtype not in dtypes:
            raise PpalsError(f"torch dtype {x.dtype} is not one of {sorted(map(str, dtypes))}")
        if x.device.type != "cuda" or x.device.index != self.ctx.device:
            raise PpalsError(f"the torch tensor is on {x.device}, the context on cuda:{self.ctx.device}")
        code = {torch.float32: F32, torch.float64: F64, torch.float16: F16, torch.bfloat16: BF16}
        return x.data_ptr(), code[x.dtype], tuple(x.shape), x.stride()

    @staticmethod
    def _stream(stream):
        if stream is None:
            return _torch().cuda.current_stream().cuda_stream
        return getattr(stream, "cuda_stream", stream)

    @classmethod
    def from_torch(cls, ctx, x, dtype=None):
        """a tensor with lens = x.shape (mode i = dim i) holding x: stored as F64 for a float64 x,
        as F32 otherwise (a bfloat16 x too), unless dtype says (BF16: a bfloat16 x is copied bit for
        bit, wider types are rounded as x.to(torch.bfloat16) rounds them). Under P > 1 ranks each
        rank copies its own rows of x."""
        torch = _torch()
        if dtype is None:
            dtype = F64 if x.dtype == torch.float64 else F32
        return cls(ctx, list(x.shape), dtype).import_torch(x)

    def import_torch(self, x, lo=None, stream=None):
        """copy the torch tensor x (any strides, f16 / bf16 / f32 / f64, on the context's device) into
        the box of the tensor at lo (default: the origin), ordered on `stream` (default: torch's
        current stream); the host does not wait"""
        torch = _torch()
        ptr, code, shape, strides = self._torch_view(
            x, (torch.float32, torch.float64, torch.float16, torch.bfloat16))
        return self.import_device(ptr, code, shape, strides, lo, self._stream(stream))

    def export_torch(self, out, lo=None, stream=None):
        """this rank's rows of the box at lo (shape out.shape) into the torch tensor out (f32 / f64,
        any strides that do not overlap); other elements of out are left alone"""
        torch = _torch()
        ptr, code, shape, strides = self._torch_view(out, (torch.float32, torch.float64))
        return self.export_device(ptr, code, shape, strides, lo, self._stream(stream))

    def to_torch(self, dtype=None):
        """the tensor as a new torch tensor on the context's device (this rank's rows; zeros
        elsewhere), ordered on torch's current stream"""
        torch = _torch()
        out = torch.zeros(self.lens, dtype=dtype or torch.float32, device=f"cuda:{self.ctx.device}")
        self.export_torch(out)
        return out

    def norm(self):
        out = C.c_double(0)
        _check(lib().ppals_tensor_norm(self._h, C.byref(out)))
        return out.value

    # ---- centring and scaling in place (include/ppals.h, "PARAFAC preprocessing") ----
    def _prep_shape(self, mode):
        """(L, J, T) around `mode`, and the offsets' shape: the tensor's with shape[mode] = 1. A mode out of
        range gives sizes of 1: the library is the one that refuses it."""
        n = len(self.lens)
        if not 0 <= mode < n:
            return 1, 1, 1, [1] * n
        L = int(np.prod(self.lens[:mode], dtype=np.int64))
        T = int(np.prod(self.lens[mode + 1:], dtype=np.int64))
        return L, self.lens[mode], T, self.lens[:mode] + [1] + self.lens[mode + 1:]

    def center(self, mode, offsets=None, stream=None):
        """V <- V - its mean over `mode`, fibre by fibre. offsets: None (nothing is returned and the host does
        not wait), "numpy" (the means as an fp64 array of the tensor's shape with shape[mode] = 1) or "torch"
        (the same as a float64 torch tensor on the context's device, ordered on `stream`, default torch's
        current stream; the host does not wait)."""
        mode = int(mode)
        L, _, T, shape = self._prep_shape(mode)
        if offsets is None:
            _check(lib().ppals_tensor_center(self._h, mode, None, HOST, None))
            return None
        if offsets == "numpy":
            out = np.empty(L * T, dtype=np.float64)
            _check(lib().ppals_tensor_center(self._h, mode, _dp(out), HOST, None))
            return out.reshape(shape, order="F")
        if offsets == "torch":
            torch = _torch()
            buf = torch.empty(L * T, dtype=torch.float64, device=f"cuda:{self.ctx.device}")
            _check(lib().ppals_tensor_center(self._h, mode, C.c_void_p(buf.data_ptr()), DEVICE,
                                             C.c_void_p(int(self._stream(stream) or 0))))
            n = len(shape)  # element l + L t of buf is element (i_0, ..) of the result, first index fastest
            return buf.view(*reversed(shape)).permute(*reversed(range(n)))
        raise ValueError('offsets must be None, "numpy" or "torch"')

    def shift(self, mode, offsets, alpha=1.0, stream=None):
        """V <- V + alpha * offsets, the offsets (numpy, or a float64 torch tensor on the context's device) of
        the tensor's shape with shape[mode] = 1, as center returns them: alpha = 1 undoes a centring, alpha = -1
        applies a calibration set's means to new data. A torch tensor is read in place when it already lies first
        index fastest; the call is then ordered on `stream` and the host does not wait."""
        mode = int(mode)
        L, _, T, shape = self._prep_shape(mode)
        if type(offsets).__module__.split(".")[0] == "torch":
            torch = _torch()
            if offsets.dtype != torch.float64:
                raise PpalsError(f"the offsets must be float64, not {offsets.dtype}")
            if offsets.device.type != "cuda" or offsets.device.index != self.ctx.device:
                raise PpalsError(f"the offsets are on {offsets.device}, the context on cuda:{self.ctx.device}")
            if list(offsets.shape) != shape:
                raise PpalsError(f"the offsets have shape {list(offsets.shape)}, expected {shape}")
            flat_ = offsets.permute(*reversed(range(len(shape)))).contiguous().view(-1)
            _check(lib().ppals_tensor_shift(self._h, mode, C.c_void_p(flat_.data_ptr()), DEVICE,
                                            C.c_double(alpha), C.c_void_p(int(self._stream(stream) or 0))))
            return self
        o = np.asarray(offsets, dtype=np.float64)
        if list(o.shape) != shape and 0 <= mode < len(self.lens):
            raise PpalsError(f"the offsets have shape {list(o.shape)}, expected {shape}")
        o = np.ascontiguousarray(o.ravel(order="F"))
        _check(lib().ppals_tensor_shift(self._h, mode, _dp(o), HOST, C.c_double(alpha), None))
        return self

    def slice_sumsq(self, mode):
        """ss[x] = the sum of V^2 over slice x of `mode` (fp64; the tensor is only read)"""
        mode = int(mode)
        out = np.empty(self._prep_shape(mode)[1], dtype=np.float64)
        _check(lib().ppals_tensor_slice_sumsq(self._h, mode, _dp(out)))
        return out

    def scale(self, mode):
        """every slice of `mode` divided by its root mean square; returns the rms values (a slice whose rms is
        not a positive finite number stays as it is)"""
        mode = int(mode)
        out = np.empty(self._prep_shape(mode)[1], dtype=np.float64)
        _check(lib().ppals_tensor_scale(self._h, mode, _dp(out)))
        return out

    def rescale(self, mode, factors):
        """slice x of `mode` multiplied by factors[x]"""
        mode = int(mode)
        f = np.ascontiguousarray(np.asarray(factors, dtype=np.float64).ravel())
        J = self._prep_shape(mode)[1]
        if f.size != J and 0 <= mode < len(self.lens):
            raise PpalsError(f"{f.size} factors for {J} slices")
        _check(lib().ppals_tensor_rescale(self._h, mode, _dp(f)))
        return self

    # ---- the two tensor passes of N-PLS (include/ppals.h, "N-PLS regression"): the tensor is only read ----
    def contract_mode(self, mode, U):
        """Z[..., c] = sum_i X[.., i, ..] U[i, c]: the tensor contracted over `mode` with the columns of U
        (lens[mode] x C, or a vector). Returns an fp64 array of the tensor's shape without `mode`, C last."""
        mode = int(mode)
        L, I, T, _ = self._prep_shape(mode)
        U2 = np.asfortranarray(np.asarray(U, dtype=np.float64).reshape(I, -1, order="F"))
        Cn = U2.shape[1]
        Z = np.empty(L * T * Cn, dtype=np.float64)
        _check(lib().ppals_tensor_contract_mode(self._h, mode, _dp(U2), Cn, _dp(Z)))
        return Z.reshape(self.lens[:mode] + self.lens[mode + 1:] + [Cn], order="F")

    def slice_inner(self, mode, W):
        """S[i, c] = <slice i of `mode`, W[..., c]>: W has the tensor's shape without `mode`, optionally with
        C columns last. Returns lens[mode] x C (fp64)."""
        mode = int(mode)
        L, I, T, _ = self._prep_shape(mode)
        W2 = np.asfortranarray(np.asarray(W, dtype=np.float64).reshape(L * T, -1, order="F"))
        Cn = W2.shape[1]
        S = np.empty((I, Cn), dtype=np.float64, order="F")
        _check(lib().ppals_tensor_slice_inner(self._h, mode, _dp(W2), Cn, _dp(S)))
        return S

    # ---- the same passes for many columns: up to 64 a read of the tensor, on the fp64 matrix cores; deterministic and
    # within the same error bounds as the two above, not bit-equal to them ----
    def contract_columns(self, mode, U):
        """contract_mode(mode, U) through the wide-column pass"""
        mode = int(mode)
        L, I, T, _ = self._prep_shape(mode)
        U2 = np.asfortranarray(np.asarray(U, dtype=np.float64).reshape(I, -1, order="F"))
        Cn = U2.shape[1]
        Z = np.empty(L * T * Cn, dtype=np.float64)
        _check(lib().ppals_tensor_contract_columns(self._h, mode, _dp(U2), Cn, _dp(Z)))
        return Z.reshape(self.lens[:mode] + self.lens[mode + 1:] + [Cn], order="F")

    def slice_inner_columns(self, mode, W):
        """slice_inner(mode, W) through the wide-column pass"""
        mode = int(mode)
        L, I, T, _ = self._prep_shape(mode)
        W2 = np.asfortranarray(np.asarray(W, dtype=np.float64).reshape(L * T, -1, order="F"))
        Cn = W2.shape[1]
        S = np.empty((I, Cn), dtype=np.float64, order="F")
        _check(lib().ppals_tensor_slice_inner_columns(self._h, mode, _dp(W2), Cn, _dp(S)))
        return S

    def close(self):
        if self._h:
            lib().ppals_tensor_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _opts(tol=0.0, timelimit=5e3, maxiter=0, lam=0.0, resprint=10, bench=0, tol_init=1e-2,
          ratio_step=1.0, csv=None, csv_append=0, verbose=0, update_percentage=1.0):
    return _Opts(tol, timelimit, maxiter, lam, resprint, bench, tol_init, ratio_step,
                 csv.encode() if csv else None, csv_append, verbose, update_percentage)



def _usable_rms(rms):
    """the rms values Tensor.scale divided by: 1 where a slice was left alone (rms not positive finite)"""
    rms = np.asarray(rms, dtype=np.float64)
    return np.where(np.isfinite(rms) & (rms > 0), rms, 1.0)


class Preprocessing:
    """What ppals.preprocess did to a tensor, in order: ("center", mode, offsets) and ("scale", mode, rms)
    steps, the arrays as Tensor.center(mode, "numpy") and Tensor.scale(mode) returned them."""

    def __init__(self, lens):
        self.lens = [int(x) for x in lens]
        self.steps = []

    def apply(self, other):
        """the same offsets and factors on new data (a tensor of the same extents): the calibration set's
        preprocessing applied to a test set"""
        if list(other.lens) != self.lens:
            raise PpalsError(f"the tensor has extents {other.lens}, the preprocessing {self.lens}")
        for kind, mode, a in self.steps:
            if kind == "center":
                other.shift(mode, a, -1.0)
            else:
                other.rescale(mode, 1.0 / _usable_rms(a))
        return other

    def undo(self, tensor):
        """back to the raw data (up to the roundings of the storage type): the steps inverted, last first"""
        if list(tensor.lens) != self.lens:
            raise PpalsError(f"the tensor has extents {tensor.lens}, the preprocessing {self.lens}")
        for kind, mode, a in reversed(self.steps):
            if kind == "center":
                tensor.shift(mode, a, 1.0)
            else:
                tensor.rescale(mode, _usable_rms(a))
        return tensor

    def unscale_factors(self, Ws):
        """factors of a model of the scaled tensor -> factors of the model of the unscaled (still centred) one:
        the rows of W_mode multiplied by the rms of every scaling of that mode"""
        out = [np.array(W, dtype=np.float64, order="F") for W in Ws]
        for kind, mode, a in self.steps:
            if kind == "scale":
                out[mode] *= _usable_rms(a)[:, None]
        return out


def preprocess(tensor, center=(), scale=(), scale_iters=1):
    """Centre `tensor` across every mode of `center`, then scale it within every mode of `scale` (the whole list
    scale_iters times over: scaling within several modes at once is iterative), in place; returns the
    Preprocessing record. A mode in both lists is refused: scaling within a mode destroys centring across it
    (Bro & Smilde 2003)."""
    center, scale = [int(m) for m in center], [int(m) for m in scale]
    both = sorted(set(center) & set(scale))
    if both:
        raise ValueError(f"modes {both} are both centred across and scaled within: the scaling would destroy "
                         "the centring")
    rec = Preprocessing(tensor.lens)
    for m in center:
        rec.steps.append(("center", m, tensor.center(m, "numpy")))
    for _ in range(int(scale_iters)):
        for m in scale:
            rec.steps.append(("scale", m, tensor.scale(m)))
    return rec


class _ModelExport:
    """the fitted model (or V - model) into device memory; the session's class names the entry point"""
    _export_fn = None

    def export_model_device(self, ptr, dtype, shape, strides, lo=None, residual=False, stream=0):
        """raw ppals_*_export_model_device: this rank's rows of the box at lo of the model (residual:
        V - model) into the view at ptr (F32 / F64, strides in elements)"""
        blo, blen = Tensor._box(self, shape, lo)
        st = (C.c_int64 * len(self.lens))(*[int(x) for x in strides])
        _check(getattr(lib(), self._export_fn)(self._h, RESIDUAL if residual else MODEL,
                                               C.c_void_p(int(ptr)), int(dtype), blo, blen, st,
                                               C.c_void_p(int(stream or 0))))
        return self

    def export_model_torch(self, out, residual=False, lo=None, stream=None):
        """the model (residual: V - model) of the box at lo (shape out.shape) into the torch tensor out
        (f32 / f64, any strides that do not overlap), this rank's rows, ordered on `stream` (default:
        torch's current stream); other elements of out are left alone and the host does not wait"""
        torch = _torch()
        ptr, code, shape, strides = self.V._torch_view(out, (torch.float32, torch.float64))
        return self.export_model_device(ptr, code, shape, strides, lo, residual, Tensor._stream(stream))

    def model_to_torch(self, dtype=None, residual=False):
        """the model (residual: V - model) as a new torch tensor on the context's device (this rank's
        rows; zeros elsewhere), ordered on torch's current stream"""
        torch = _torch()
        out = torch.zeros(self.lens, dtype=dtype or torch.float32, device=f"cuda:{self.ctx.device}")
        self.export_model_torch(out, residual=residual)
        return out


class _Impute:
    """missing entries under a mask of one byte per element, 0 = missing; the session's class names the
    entry points"""
    _impute_fn = None
    _em_fn = None

    def _mask_view(self, shape, strides, lo):
        blo, blen = Tensor._box(self, shape, lo)
        return blo, blen, (C.c_int64 * len(self.lens))(*[int(x) for x in strides])

    def impute_device(self, ptr, shape, strides, lo=None, stream=0, want_residual=False):
        """raw ppals_*_impute_device: the tensor's elements whose mask byte (at ptr + sum_i j_i *
        strides[i], box at lo) is 0 become the current model, the others stay bit for bit. Returns the
        observed residual norm sqrt(sum over the observed elements of (V - model)^2) if want_residual
        (the call then waits for it), else None (a CP session's host does not wait; a Tucker session
        settles its eigen-steps first and may)."""
        blo, blen, st = self._mask_view(shape, strides, lo)
        sq = C.c_double(0)
        _check(getattr(lib(), self._impute_fn)(self._h, C.c_void_p(int(ptr)), blo, blen, st,
                                               C.c_void_p(int(stream or 0)),
                                               C.byref(sq) if want_residual else None))
        return float(np.sqrt(sq.value)) if want_residual else None

    def _torch_mask(self, mask):
        torch = _torch()
        if mask.dtype not in (torch.bool, torch.uint8):   # the C ABI takes bytes: nothing there to refuse it
            raise TypeError(f"the mask's torch dtype {mask.dtype} is not torch.bool or torch.uint8 "
                            "(one byte per element)")
        if mask.device.type != "cuda" or mask.device.index != self.ctx.device:
            raise PpalsError(f"the mask is on {mask.device}, the context on cuda:{self.ctx.device}")
        return mask.data_ptr(), tuple(mask.shape), mask.stride()

    def impute_torch(self, mask, lo=None, stream=None, want_residual=False):
        """impute_device with a torch.bool / torch.uint8 mask on the context's device (any strides, 0
        included: an expanded mask marks whole fibres), False / 0 = missing; the box at lo has the
        mask's shape. Ordered on `stream` (default: torch's current stream)."""
        ptr, shape, strides = self._torch_mask(mask)
        return self.impute_device(ptr, shape, strides, lo, Tensor._stream(stream), want_residual)

    def run_em(self, mask, inner_sweeps=1, lo=None, stream=None, **opts):
        """ppals_cp_em / ppals_tucker_em: repeat { impute; inner_sweeps exact sweeps } until maxiter
        iterations, timelimit or an observed residual <= tol (looked at every resprint iterations); uses
        tol, timelimit, maxiter, resprint and (CP) lam. Returns (stopped on tol, iterations, observed
        residual norm); the tensor's missing entries then hold the model of the returned factors. A
        Tucker session starts from the factors and core it holds: usually hosvd() of the zero-filled tensor."""
        ptr, shape, strides = self._torch_mask(mask)
        blo, blen, st = self._mask_view(shape, strides, lo)
        o = _opts(**opts)
        it, res = C.c_int(0), C.c_double(0)
        rc = _check(getattr(lib(), self._em_fn)(self._h, C.c_void_p(int(ptr)), blo, blen, st,
                                                C.c_void_p(int(Tensor._stream(stream) or 0)), C.byref(o),
                                                int(inner_sweeps), C.byref(it), C.byref(res)))
        return rc, it.value, res.value


def weights_from_std(std):
    """element weights for CP.wls_torch / run_wls from a noise standard deviation per element (a numpy array or
    a torch tensor, any shape that broadcasts against the data): std.min()**2 / std**2, which lies in (0, 1]
    as Kiers' majorization wants, with 0 where std is inf or NaN (such an element is missing)."""
    if isinstance(std, np.ndarray) or not hasattr(std, "device"):
        std = np.asarray(std, dtype=np.float64)
        ok = np.isfinite(std)
        lo = std[ok].min() if ok.any() else 1.0
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(ok, (lo / std) ** 2, 0.0)
    torch = _torch()
    ok = torch.isfinite(std)
    lo = std[ok].min() if bool(ok.any()) else torch.ones((), dtype=std.dtype, device=std.device)
    return torch.where(ok, (lo / std) ** 2, torch.zeros((), dtype=std.dtype, device=std.device))


class _Wls:
    """element weights (ppals_cp_wls_device / ppals_cp_wls): Kiers' majorization step and its driver"""

    def _wls_views(self, shape, data_strides, weight_strides, lo):
        blo, blen = Tensor._box(self, shape, lo)
        n = len(self.lens)
        return (blo, blen, (C.c_int64 * n)(*[int(x) for x in data_strides]),
                (C.c_int64 * n)(*[int(x) for x in weight_strides]))

    def wls_device(self, data_ptr, weights_ptr, dtype, shape, data_strides, weight_strides, lo=None, stream=0,
                   want_loss=False):
        """raw ppals_cp_wls_device: every element of the box at lo becomes x (weight h >= 1), the current model
        m (h <= 0 or NaN) or fma(h, x - m, m), x and h read from the two views (F32 or F64, strides in
        elements, 0 broadcasts). Returns the weighted loss sum h (x - m)^2 if want_loss (the call then waits
        for it), else None (the host does not wait)."""
        blo, blen, ds, ws = self._wls_views(shape, data_strides, weight_strides, lo)
        sq = C.c_double(0)
        _check(lib().ppals_cp_wls_device(self._h, C.c_void_p(int(data_ptr)), C.c_void_p(int(weights_ptr)), int(dtype),
                                         blo, blen, ds, ws, C.c_void_p(int(stream or 0)),
                                         C.byref(sq) if want_loss else None))
        return float(sq.value) if want_loss else None

    def _torch_wls(self, data, weights):
        torch = _torch()
        if data.dtype != weights.dtype:
            raise TypeError(f"data is {data.dtype} and weights {weights.dtype}: the two views share one dtype")
        if data.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"the torch dtype {data.dtype} of data and weights is not torch.float32 or torch.float64")
        if tuple(weights.shape) != tuple(data.shape):
            weights = weights.expand(data.shape)   # stride 0 where it broadcasts: no copy
        dptr, code, shape, dstr = self.V._torch_view(data, (torch.float32, torch.float64))
        wptr, _, _, wstr = self.V._torch_view(weights, (torch.float32, torch.float64))
        return dptr, wptr, code, shape, dstr, wstr

    def wls_torch(self, data, weights, lo=None, stream=None, want_loss=False):
        """wls_device with torch tensors on the context's device (f32 or f64, the same dtype, any strides);
        `weights` is expanded to data.shape when it broadcasts (a per-variable vector costs its own length).
        The box at lo has data's shape. Ordered on `stream` (default: torch's current stream)."""
        dptr, wptr, code, shape, dstr, wstr = self._torch_wls(data, weights)
        return self.wls_device(dptr, wptr, code, shape, dstr, wstr, lo, Tensor._stream(stream), want_loss)

    def run_wls(self, data, weights, inner_sweeps=1, rel_change=0.0, lo=None, stream=None, **opts):
        """ppals_cp_wls: repeat { majorization step; inner_sweeps exact sweeps } until maxiter iterations,
        timelimit, a weighted residual <= tol (rc 1) or, from the second look on, a fall of no more than
        rel_change of the residual at the look before (rc 2); looks every resprint iterations. Uses tol,
        timelimit, maxiter, resprint and lam. Returns (rc, iterations, weighted residual sqrt(sum h (x - m)^2))."""
        dptr, wptr, code, shape, dstr, wstr = self._torch_wls(data, weights)
        blo, blen, ds, ws = self._wls_views(shape, dstr, wstr, lo)
        o = _opts(**opts)
        it, res = C.c_int(0), C.c_double(0)
        rc = _check(lib().ppals_cp_wls(self._h, C.c_void_p(int(dptr)), C.c_void_p(int(wptr)), int(code), blo, blen,
                                       ds, ws, C.c_void_p(int(Tensor._stream(stream) or 0)), C.byref(o),
                                       int(inner_sweeps), C.c_double(float(rel_change)), C.byref(it), C.byref(res)))
        return rc, it.value, res.value


class _Robust:
    """robust CP (ppals_cp_huber_device / ppals_cp_robust / ppals_cp_abs_residual_quantile): Huber's loss by
    majorization, and the residual quantile its threshold is chosen from"""

    def _robust_views(self, data, weights):
        """(data ptr, weights ptr or None, dtype code, shape, data strides, weights strides) of torch tensors"""
        torch = _torch()
        if weights is not None:
            return self._torch_wls(data, weights)
        if data.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"the torch dtype {data.dtype} of data is not torch.float32 or torch.float64")
        dptr, code, shape, dstr = self.V._torch_view(data, (torch.float32, torch.float64))
        return dptr, None, code, shape, dstr, dstr

    def huber_device(self, data_ptr, weights_ptr, dtype, shape, data_strides, weight_strides, c, lo=None, stream=0,
                     want_loss=False):
        """raw ppals_cp_huber_device: wls_device with the residual clipped to [-c, c] (c > 0; inf: wls_device's
        bits); weights_ptr None or 0: weight 1 everywhere (weight_strides is then ignored). Returns
        (Huber loss, number of clipped elements) if want_loss (the call then waits), else None."""
        blo, blen, ds, ws = self._wls_views(shape, data_strides, weight_strides or data_strides, lo)
        loss, clipped = C.c_double(0), C.c_int64(0)
        _check(lib().ppals_cp_huber_device(self._h, C.c_void_p(int(data_ptr)),
                                           C.c_void_p(int(weights_ptr)) if weights_ptr else None, int(dtype), blo, blen,
                                           ds, ws, C.c_double(float(c)), C.c_void_p(int(stream or 0)),
                                           C.byref(loss) if want_loss else None,
                                           C.byref(clipped) if want_loss else None))
        return (float(loss.value), int(clipped.value)) if want_loss else None

    def huber_torch(self, data, c, weights=None, lo=None, stream=None, want_loss=False):
        """huber_device with torch tensors on the context's device (f32 or f64, the same dtype, any strides;
        `weights` is expanded when it broadcasts, None: weight 1 everywhere, which reads one view less). Every
        element of the box at lo becomes m + h clip(x - m, -c, c), m the current model. Returns None, or
        (loss, clipped) when want_loss is set."""
        dptr, wptr, code, shape, dstr, wstr = self._robust_views(data, weights)
        return self.huber_device(dptr, wptr, code, shape, dstr, wstr, c, lo, Tensor._stream(stream), want_loss)

    def abs_residual_quantile_torch(self, data, p=0.5, weights=None, lo=None, stream=None):
        """ppals_cp_abs_residual_quantile: (value, count), count the elements of the box with weight > 0 (all
        without weights) and value the k-th smallest (float)|x - m| among them, k = min(count - 1,
        max(0, ceil(p count) - 1)), NaN last; (nan, 0) if there are none. Exact; reads no tensor (any storage)."""
        dptr, wptr, code, shape, dstr, wstr = self._robust_views(data, weights)
        blo, blen, ds, ws = self._wls_views(shape, dstr, wstr, lo)
        val, cnt = C.c_double(0), C.c_int64(0)
        _check(lib().ppals_cp_abs_residual_quantile(self._h, C.c_void_p(int(dptr)),
                                                    C.c_void_p(int(wptr)) if wptr else None, int(code), blo, blen,
                                                    ds, ws, C.c_void_p(int(Tensor._stream(stream) or 0)),
                                                    C.c_double(float(p)), C.byref(val), C.byref(cnt)))
        return float(val.value), int(cnt.value)

    def robust_scale(self, data, weights=None, lo=None, stream=None):
        """1.4826 x the median of |x - m|: the MAD scale of the current residuals (a consistent estimate of the
        noise's standard deviation under Gaussian noise, whatever a minority of outliers does)"""
        return 1.4826 * self.abs_residual_quantile_torch(data, 0.5, weights, lo, stream)[0]

    def run_robust(self, data, c=None, weights=None, tune=1.345, inner_sweeps=1, rel_change=0.0, lo=None,
                   stream=None, **opts):
        """ppals_cp_robust: repeat { Huber step at the fixed threshold c; inner_sweeps exact sweeps } with the
        looks and stop rules of run_wls. c=None: tune x robust_scale(...), taken ONCE from the factors the
        session holds (1.345: 95 % efficiency under Gaussian noise). Returns (rc, iterations, sqrt(Huber loss), c).

        The intended staging, from a random start: the scale of a poor fit is large, so estimate it twice,

            cp.sweeps_dt(20)                                   # some plain sweeps
            rc, it, res, c1 = cp.run_robust(x, maxiter=100)    # c from the plain fit's residuals
            rc, it, res, c2 = cp.run_robust(x, maxiter=100)    # c again, from the robust fit: the noise's scale

        (c is never re-estimated inside a call: the loss of a call falls monotonically only at a fixed c.)"""
        if c is None:
            c = float(tune) * self.robust_scale(data, weights, lo, stream)
        dptr, wptr, code, shape, dstr, wstr = self._robust_views(data, weights)
        blo, blen, ds, ws = self._wls_views(shape, dstr, wstr, lo)
        o = _opts(**opts)
        it, res = C.c_int(0), C.c_double(0)
        rc = _check(lib().ppals_cp_robust(self._h, C.c_void_p(int(dptr)), C.c_void_p(int(wptr)) if wptr else None,
                                          int(code), blo, blen, ds, ws, C.c_void_p(int(Tensor._stream(stream) or 0)),
                                          C.c_double(float(c)), C.byref(o), int(inner_sweeps),
                                          C.c_double(float(rel_change)), C.byref(it), C.byref(res)))
        return rc, it.value, res.value, float(c)


class CP(_ModelExport, _Impute, _Wls, _Robust):
    """a CP-ALS session: factors, Grams and dimension-tree caches resident in HBM"""
    _export_fn = "ppals_cp_export_model_device"
    _impute_fn, _em_fn = "ppals_cp_impute_device", "ppals_cp_em"

    def __init__(self, ctx, V, R):
        self.ctx, self.V, self.R = ctx, V, R
        self.lens = V.lens
        self._h = C.c_void_p()
        _check(lib().ppals_cp_create(ctx._h, V._h, R, C.byref(self._h)))
        ctx._children.add(self)

    def set_factors(self, Ws, gradWs=None):
        wf = flat(Ws)
        gf = flat(gradWs) if gradWs is not None else None
        _check(lib().ppals_cp_set_factors(self._h, _dp(wf), _dp(gf) if gf is not None else None))

    def get_factors(self, with_grad=False):
        n = sum(s * self.R for s in self.lens)
        wf = np.empty(n)
        gf = np.empty(n) if with_grad else None
        _check(lib().ppals_cp_get_factors(self._h, _dp(wf), _dp(gf) if with_grad else None))
        W = unflat(wf, self.lens, [self.R] * len(self.lens))
        if with_grad:
            return W, unflat(gf, self.lens, [self.R] * len(self.lens))
        return W

    def set_schedule(self, schedule):
        """"dt" (two first-level nodes, alsCP_DT) or "msdt" (multi-sweep tree, the default)"""
        code = {"dt": 0, "msdt": 1}[schedule] if isinstance(schedule, str) else int(schedule)
        _check(lib().ppals_cp_set_schedule(self._h, code))

    @property
    def schedule(self):
        return {0: "dt", 1: "msdt"}[_check(lib().ppals_cp_get_schedule(self._h))]

    def set_nonneg(self, on=True):
        """non-negative CP: every mode update becomes one HALS pass (entries >= PPALS_NN_FLOOR).
        Exact sweeps, run_dt, cpd_als and run_em work on top; PP, the low-rank optimizers, CPMulti.take
        from an unconstrained multi-start session, more than one rank and R > 64 are refused, as are
        factors with a negative or non-finite entry."""
        _check(lib().ppals_cp_set_nonneg(self._h, 1 if on else 0))

    @property
    def nonneg(self):
        return bool(_check(lib().ppals_cp_get_nonneg(self._h)))

    def set_mode_constraints(self, kinds):
        """one kind per mode, ints (MODE_*) or "free" | "nonneg" | "fixed" | "ortho": the solve, the HALS pass
        of set_nonneg, no update at all, or orthonormal columns (the polar factor of the mode's MTTKRP). With
        a fixed or orthonormal mode the sweeps end without Normalize. PP, the low-rank optimizers, more than
        one rank, and non-negative or orthonormal modes at R > 64 are refused."""
        _check(lib().ppals_cp_set_mode_constraints(self._h, _kinds(kinds, len(self.lens))))

    @property
    def mode_constraints(self):
        out = (C.c_int * len(self.lens))()
        _check(lib().ppals_cp_get_mode_constraints(self._h, out))
        return [MODE_KINDS[k] for k in out]

    def set_mode_shapes(self, shapes):
        """one shape per mode, ints (SHAPE_*) or "none" | "unimodal" | "increasing" | "decreasing", on modes of
        kind "nonneg" only: every column of a shaped mode's factor is, update by update, the least-squares
        projection of its HALS target onto the non-negative sequences with one peak, or that never fall, or
        that never rise. All "none" is the session as it was. Changing a mode's kind away from "nonneg"
        clears its shape."""
        _check(lib().ppals_cp_set_mode_shapes(self._h, _shapes(shapes, len(self.lens))))

    @property
    def mode_shapes(self):
        out = (C.c_int * len(self.lens))()
        _check(lib().ppals_cp_get_mode_shapes(self._h, out))
        return [SHAPE_KINDS[k] for k in out]

    def placement_report(self):
        """where the online placement choice put each root's first-level intermediate (dict)"""
        import json
        buf = C.create_string_buffer(8192)
        _check(lib().ppals_cp_placement_report(self._h, buf, 8192))
        return json.loads(buf.value.decode())

    def pp_build_stats(self, mode=0):
        """(number, seconds) of the PP operator builds since the last reset; mode +1 / -1: reset and
        turn their timing on / off"""
        n, sec = C.c_int64(0), C.c_double(0)
        _check(lib().ppals_cp_pp_build_stats(self._h, mode, C.byref(n), C.byref(sec)))
        return n.value, sec.value

    def sweeps_dt(self, n, lam=0.0):
        _check(lib().ppals_cp_sweeps_dt(self._h, n, C.c_double(lam)))

    def gradnorm(self):
        out = C.c_double(0)
        _check(lib().ppals_cp_gradnorm(self._h, C.byref(out)))
        return out.value

    def residual(self):
        out = C.c_double(0)
        _check(lib().ppals_cp_residual(self._h, C.byref(out)))
        return out.value

    def core_consistency(self, return_core=False):
        """the core consistency diagnostic (Bro & Kiers 2003) of the current factors, in per cent, not
        clamped; NaN when a factor has no pseudo-inverse. return_core: (cc, core), the core of shape
        (R,) * order. Reads the session and changes nothing of it."""
        cc, n = C.c_double(0), C.c_int64(0)
        if not return_core:
            _check(lib().ppals_cp_core_consistency(self._h, C.byref(cc), None, C.byref(n)))
            return cc.value
        core = np.empty(int(self.R) ** len(self.lens))
        _check(lib().ppals_cp_core_consistency(self._h, C.byref(cc), _dp(core), C.byref(n)))
        return cc.value, core.reshape((self.R,) * len(self.lens), order="F")

    def congruence(self, other, skip_mode=None):
        """Phi (R, other.R): the signed product over the compared modes (all, or all but skip_mode) of the
        cosines between this session's columns and other's (ppals_cp_congruence); 0 in the row / column of
        a column without a positive finite norm. Reads both sessions and changes nothing of them."""
        out = np.empty((self.R, other.R), order="F")
        n = C.c_int64(0)
        _check(lib().ppals_cp_congruence(self._h, other._h, _skip(skip_mode), _dp(out), C.byref(n)))
        return out

    def fms(self, other, skip_mode=None, weights=False, return_perm=False):
        """the factor match score against other (ppals_cp_fms): the mean congruence of the optimally
        matched min(R, other.R) column pairs; weights: each pair scaled by 1 - |w - w'| / max(w, w') of
        the components' norm products. return_perm: (fms, perm), perm[p] the matched column of other or -1."""
        out = C.c_double(0)
        perm = (C.c_int * self.R)()
        _check(lib().ppals_cp_fms(self._h, other._h, _skip(skip_mode), FMS_WEIGHTS if weights else 0,
                                  C.byref(out), perm if return_perm else None))
        return (out.value, np.array(perm[:], dtype=np.int64)) if return_perm else out.value

    def _per_mode(self, flat_vec):
        cuts = np.cumsum(self.lens)[:-1]
        return [v.copy() for v in np.split(flat_vec, cuts)]

    def slice_residuals(self, return_total=False):
        """the residual side of the influence plot (ppals_cp_slice_residuals): a list of N vectors, entry x
        of vector i the sum of (V - model)^2 over the slice x of mode i — one pass over the tensor, nothing
        materialised. return_total: (list, total), total = residual()**2 up to rounding. Reads the session
        and changes nothing of it."""
        out = np.empty(sum(self.lens))
        total = C.c_double(0)
        _check(lib().ppals_cp_slice_residuals(self._h, _dp(out), C.byref(total)))
        ss = self._per_mode(out)
        return (ss, total.value) if return_total else ss

    def leverages(self):
        """the leverage side (ppals_cp_leverages): a list of N vectors, entry x of vector i the x-th diagonal
        entry of the projector onto the columns of W_i; all NaN when a factor has no pseudo-inverse. Never
        reads the tensor."""
        out = np.empty(sum(self.lens))
        _check(lib().ppals_cp_leverages(self._h, _dp(out)))
        return self._per_mode(out)

    def tree_node(self, key, shape=None):
        n = C.c_int64(0)
        _check(lib().ppals_tree_node(self._h, key.encode(), None, C.byref(n)))
        out = np.empty(n.value)
        _check(lib().ppals_tree_node(self._h, key.encode(), _dp(out), C.byref(n)))
        return out.reshape(shape, order="F") if shape else out

    def mttkrp(self, mode):
        M = np.empty(self.lens[mode] * self.R)
        _check(lib().ppals_mttkrp(self._h, mode, _dp(M)))
        return M.reshape((self.lens[mode], self.R), order="F")

    def pp_operator(self, contracted, shape=None):
        n = C.c_int64(0)
        _check(lib().ppals_pp_operator(self._h, contracted.encode(), None, C.byref(n)))
        out = np.empty(n.value)
        _check(lib().ppals_pp_operator(self._h, contracted.encode(), _dp(out), C.byref(n)))
        return out.reshape(shape, order="F") if shape else out

    def gram_system(self, mode, lam=0.0):
        S = np.empty(self.R * self.R)
        Si = np.empty(self.R * self.R)
        _check(lib().ppals_cp_gram_system(self._h, mode, C.c_double(lam), _dp(S), _dp(Si)))
        return S.reshape((self.R, self.R), order="F"), Si.reshape((self.R, self.R), order="F")

    def run_dt(self, **kw):
        o = _opts(**kw)
        it = C.c_int(0)
        rc = _check(lib().ppals_cp_dt(self._h, C.byref(o), C.byref(it)))
        return rc, it.value

    def run_pp(self, **kw):
        o = _opts(**kw)
        it = C.c_int(0)
        rc = _check(lib().ppals_cp_pp(self._h, C.byref(o), C.byref(it)))
        return rc, it.value

    def cpd_als(self, optimizer, **kw):
        """CPD<dtype, Optimizer>::als (src/CP.cxx:100-186); maxiter= is maxsweep.
        Returns (rc, sweeps, iters)."""
        o = _opts(**kw)
        it = C.c_int(0)
        sw = C.c_double(0)
        rc = _check(lib().ppals_cpd_als(self._h, int(optimizer), C.byref(o), C.byref(sw),
                                        C.byref(it)))
        return rc, sw.value, it.value

    def cpd_als_lr(self, optimizer, update_rank, randomsvd=0, **kw):
        """CPD<dtype, CPDTLROptimizer / CPMSDTLROptimizer>::als (optimizer 3 / 4); randomsvd as
        run.cxx's flag. Returns (rc, sweeps, iters)."""
        o = _opts(**kw)
        it = C.c_int(0)
        sw = C.c_double(0)
        rc = _check(lib().ppals_cpd_als_lr(self._h, int(optimizer), int(update_rank), int(randomsvd),
                                           C.byref(o), C.byref(sw), C.byref(it)))
        return rc, sw.value, it.value

    def run_pp_partupdate(self, **kw):
        o = _opts(**kw)
        it = C.c_int(0)
        rc = _check(lib().ppals_cp_pp_partupdate(self._h, C.byref(o), C.byref(it)))
        return rc, it.value

    def close(self):
        if self._h:
            lib().ppals_cp_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedCP(CP):
    """the inner session of a Parafac2: a CP on the compressed tensor; closing it does nothing
    (ppals_parafac2_destroy destroys the session)"""

    def __init__(self, owner, handle, lens, R):
        self.ctx, self.V, self.R = owner.ctx, None, R
        self.lens = list(lens)
        self._owner = owner  # keeps the owner alive while the session is in use
        self._h = handle

    def close(self):
        self._h = C.c_void_p()


class _BorrowedTensor(Tensor):
    """the compressed tensor of a Parafac2 (R x J x K): download, export and norm; closing it does nothing"""

    def __init__(self, owner, handle, lens, dtype):
        self.ctx, self.lens, self.dtype, self._owner, self._h = owner.ctx, list(lens), dtype, owner, handle

    def close(self):
        self._h = C.c_void_p()


class Parafac2:
    """PARAFAC2 by direct fitting (ppals_parafac2_*): X_k ~ P_k B diag(C[k, :]) A^T for the slices X_k = X[:, :, k]
    of an I x J x K torch tensor on the context's device, P_k^T P_k = I. `.cp` is the rank-R CP session on the
    compressed tensor (R x J x K; factors [B, A, C]): constraints, shapes, schedule and diagnostics are set there;
    mode 0 (B) must stay free.

    Parafac2.ragged(ctx, rows, J, R) is the model on K = len(rows) slices of unequal length, slice k rows[k] x J
    (`is_ragged`, `I` is None): step_torch / run / loss then take a list of K torch matrices or one flat buffer
    with offsets and column strides, and projections() / profiles() return lists."""

    def __init__(self, ctx, I, J, K, R, dtype=F64):
        self.ctx, self.I, self.J, self.K, self.R, self.dtype = ctx, int(I), int(J), int(K), int(R), dtype
        self.is_ragged = False
        self._h = C.c_void_p()
        _check(lib().ppals_parafac2_create(ctx._h, C.c_int64(self.I), C.c_int64(self.J), C.c_int64(self.K), self.R,
                                           int(dtype), C.byref(self._h)))
        self._attach()

    @classmethod
    def ragged(cls, ctx, rows, J, R, dtype=F64):
        """ppals_parafac2_create_ragged: slice k is rows[k] x J"""
        self = cls.__new__(cls)
        rows = [int(r) for r in rows]
        self.ctx, self.I, self.J, self.K, self.R, self.dtype = ctx, None, int(J), len(rows), int(R), dtype
        self.is_ragged = True
        self._pack = None      # a list input's packed device copy: (key, the tensors, the buffer)
        self._h = C.c_void_p()
        _check(lib().ppals_parafac2_create_ragged(ctx._h, C.c_int64(self.K), (C.c_int64 * max(self.K, 1))(*rows),
                                                  C.c_int64(self.J), self.R, int(dtype), C.byref(self._h)))
        self._attach()
        return self

    def _attach(self):
        ctx, dtype = self.ctx, self.dtype
        lib().ppals_parafac2_cp.restype = C.c_void_p
        self.cp = _BorrowedCP(self, C.c_void_p(lib().ppals_parafac2_cp(self._h)), [self.R, self.J, self.K], self.R)
        lib().ppals_parafac2_tensor.restype = C.c_void_p
        self.Y = _BorrowedTensor(self, C.c_void_p(lib().ppals_parafac2_tensor(self._h)), [self.R, self.J, self.K], dtype)
        self.cp.V = self.Y
        ctx._children.add(self)

    @property
    def rows(self):
        """the slice lengths (ppals_parafac2_rows): I for every slice of an equal-length object"""
        out = (C.c_int64 * self.K)()
        _check(lib().ppals_parafac2_rows(self._h, out, None))
        return [int(r) for r in out]

    def _view(self, X):
        torch = _torch()
        if X.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"the torch dtype {X.dtype} of X is not torch.float32 or torch.float64")
        if X.device.type != "cuda" or X.device.index != self.ctx.device:
            raise PpalsError(f"the torch tensor is on {X.device}, the context on cuda:{self.ctx.device}")
        if tuple(X.shape) != (self.I, self.J, self.K):
            raise PpalsError(f"X has shape {tuple(X.shape)}, the model {(self.I, self.J, self.K)}")
        return X.data_ptr(), (F64 if X.dtype == torch.float64 else F32), (C.c_int64 * 3)(*X.stride())

    def step_device(self, ptr, dtype, strides=None, stream=0, want=True):
        """raw ppals_parafac2_step_device; strides in elements (None: dense, first index fastest). Returns
        (lost_sq, failed) if want (the call then waits), else None."""
        st = (C.c_int64 * 3)(*[int(x) for x in strides]) if strides is not None else None
        lost, failed = C.c_double(0), C.c_int(0)
        _check(lib().ppals_parafac2_step_device(self._h, C.c_void_p(int(ptr)), int(dtype), st,
                                                C.c_void_p(int(stream or 0)), C.byref(lost) if want else None,
                                                C.byref(failed) if want else None))
        return (float(lost.value), int(failed.value)) if want else None

    def _i64(self, v):
        if v is None:
            return None
        v = [int(x) for x in v]
        if len(v) != self.K:
            raise PpalsError(f"{len(v)} entries for {self.K} slices")
        return (C.c_int64 * self.K)(*v)

    def step_slices_device(self, ptr, dtype, offsets=None, col_strides=None, stream=0, want=True):
        """raw ppals_parafac2_step_ragged_device: X_k[i, j] = data[offsets[k] + i + col_strides[k] j] in elements
        (offsets None: packed one after another; col_strides None: rows[k]). Returns (lost_sq, failed) if want
        (the call then waits), else None."""
        lost, failed = C.c_double(0), C.c_int(0)
        _check(lib().ppals_parafac2_step_ragged_device(self._h, C.c_void_p(int(ptr)), int(dtype), self._i64(offsets),
                                                       self._i64(col_strides), C.c_void_p(int(stream or 0)),
                                                       C.byref(lost) if want else None,
                                                       C.byref(failed) if want else None))
        return (float(lost.value), int(failed.value)) if want else None

    def _slices_view(self, X, offsets, col_strides, stream):
        """a ragged object's input as (pointer, dtype code, offsets, col_strides): a flat 1-D torch buffer with its
        offsets and column strides, or a list of K matrices rows[k] x J, packed (each slice column-major, one after
        another) into a buffer the object keeps. The buffer is refilled, on `stream`, when the list holds other
        tensors than last time or one of them has been written to since."""
        torch = _torch()
        if not isinstance(X, (list, tuple)):
            if X.dim() != 1:
                raise PpalsError(f"a ragged model takes a list of K matrices or a 1-D buffer, not shape {tuple(X.shape)}")
            if X.stride(0) != 1:
                raise PpalsError("the flat buffer needs unit stride")
            self._check_torch(X)
            return X.data_ptr(), (F64 if X.dtype == torch.float64 else F32), offsets, col_strides
        if offsets is not None or col_strides is not None:
            raise PpalsError("offsets and col_strides go with a flat buffer, not with a list of matrices")
        rows = self.rows
        if len(X) != self.K:
            raise PpalsError(f"{len(X)} matrices for {self.K} slices")
        for k, x in enumerate(X):
            self._check_torch(x)
            if tuple(x.shape) != (rows[k], self.J) or x.dtype != X[0].dtype:
                raise PpalsError(f"slice {k} has shape {tuple(x.shape)} and dtype {x.dtype}, the model "
                                 f"{(rows[k], self.J)} and the first slice {X[0].dtype}")
        key = tuple((id(x), x.data_ptr(), x._version) for x in X)
        if self._pack is None or self._pack[0] != key:
            buf = self._pack[2] if self._pack is not None and self._pack[2].dtype == X[0].dtype else \
                torch.empty(sum(rows) * self.J, dtype=X[0].dtype, device=X[0].device)
            s = stream if stream is not None else torch.cuda.current_stream()
            with torch.cuda.stream(s if hasattr(s, "cuda_stream") else torch.cuda.ExternalStream(int(s))):
                o = 0
                for k, x in enumerate(X):          # column-major rows[k] x J = row-major J x rows[k]
                    buf[o:o + rows[k] * self.J].view(self.J, rows[k]).copy_(x.t())
                    o += rows[k] * self.J
            self._pack = (key, list(X), buf)       # (the tensors stay referenced: their ids stay theirs)
        buf = self._pack[2]
        return buf.data_ptr(), (F64 if buf.dtype == torch.float64 else F32), None, None

    def _check_torch(self, X):
        torch = _torch()
        if X.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"the torch dtype {X.dtype} of X is not torch.float32 or torch.float64")
        if X.device.type != "cuda" or X.device.index != self.ctx.device:
            raise PpalsError(f"the torch tensor is on {X.device}, the context on cuda:{self.ctx.device}")

    def step_torch(self, X, stream=None, want=True, offsets=None, col_strides=None):
        """one projection step from the session's current factors: new P_k where Q_k has a polar factor, Y = P^T X
        into the compressed tensor. X: float32 or float64 with X.stride(0) == 1 (e.g. made by
        x.permute(2, 1, 0).contiguous().permute(2, 1, 0)); on a ragged object a list of K matrices rows[k] x J, or
        a flat 1-D buffer with `offsets` and `col_strides` (step_slices_device). Returns (lost_sq, failed), or None
        if not want."""
        if self.is_ragged:
            ptr, code, off, cs = self._slices_view(X, offsets, col_strides, stream)
            return self.step_slices_device(ptr, code, off, cs, Tensor._stream(stream), want)
        ptr, code, st = self._view(X)
        return self.step_device(ptr, code, st, Tensor._stream(stream), want)

    def run(self, X, inner_sweeps=1, rel_change=0.0, stream=None, offsets=None, col_strides=None, **opts):
        """ppals_parafac2_run (ppals_parafac2_run_ragged on a ragged object, X as step_torch takes it): repeat
        { step; inner_sweeps exact sweeps } with the looks and stop rules of CP.run_wls. Returns
        (rc, iterations, ||X - model||)."""
        o = _opts(**opts)
        it, res = C.c_int(0), C.c_double(0)
        if self.is_ragged:
            ptr, code, off, cs = self._slices_view(X, offsets, col_strides, stream)
            rc = _check(lib().ppals_parafac2_run_ragged(self._h, C.c_void_p(int(ptr)), int(code), self._i64(off),
                                                        self._i64(cs), C.c_void_p(int(Tensor._stream(stream) or 0)),
                                                        C.byref(o), int(inner_sweeps), C.c_double(float(rel_change)),
                                                        C.byref(it), C.byref(res)))
            return rc, it.value, res.value
        ptr, code, st = self._view(X)
        rc = _check(lib().ppals_parafac2_run(self._h, C.c_void_p(int(ptr)), int(code), st,
                                             C.c_void_p(int(Tensor._stream(stream) or 0)), C.byref(o),
                                             int(inner_sweeps), C.c_double(float(rel_change)), C.byref(it),
                                             C.byref(res)))
        return rc, it.value, res.value

    def loss(self, X, stream=None, offsets=None, col_strides=None):
        """||X - model||^2 of the session's current factors with the P_k that are best for them: takes a step
        (which can only lower the loss), then lost_sq + the inner residual squared"""
        if self.is_ragged:
            lost, _ = self.step_torch(X, stream, offsets=offsets, col_strides=col_strides)
        else:
            lost, _ = self.step_torch(X, stream)
        return max(lost, 0.0) + self.cp.residual() ** 2

    def projections(self):
        """the P_k as a K x I x R numpy array; of a ragged object as a list of K arrays rows[k] x R"""
        if self.is_ragged:
            rows = self.rows
            flat_p = np.empty(sum(rows) * self.R)
            _check(lib().ppals_parafac2_projections(self._h, _dp(flat_p)))
            out, o = [], 0
            for n in rows:
                out.append(np.ascontiguousarray(flat_p[o:o + n * self.R].reshape((n, self.R), order="F")))
                o += n * self.R
            return out
        out = np.empty((self.I, self.R, self.K), order="F")
        _check(lib().ppals_parafac2_projections(self._h, _dp(out)))
        return np.ascontiguousarray(out.transpose(2, 0, 1))

    def projections_device(self):
        """the device pointer of P (I x R x K doubles, first index fastest), the object's"""
        ptr = c_dp()
        _check(lib().ppals_parafac2_projections_device(self._h, C.byref(ptr)))
        return C.cast(ptr, C.c_void_p).value

    def profiles(self):
        """the slice profiles P_k B as a K x I x R numpy array; of a ragged object as a list of rows[k] x R arrays"""
        B = self.cp.get_factors()[0]
        if self.is_ragged:
            return [P @ B for P in self.projections()]
        return self.projections() @ B

    def close(self):
        if self._h:
            self.cp.close()
            self.Y.close()
            lib().ppals_parafac2_destroy(self._h)
            self._h = C.c_void_p()
            self._pack = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def parafac2(X, R, n_iter=100, nonneg_modes=(), inner_sweeps=1, rel_change=0.0, dtype=F64, ctx=None, A0=None):
    """PARAFAC2 of a torch tensor X (I x J x K on a GPU, float32 or float64; mode 0 shifts, mode 2 are the slices).
    nonneg_modes: which of the modes 1 (A) and 2 (C) are non-negative. Looks at the loss at every iteration.
    X may also be a list or tuple of K torch matrices rows[k] x J, slices of unequal length (Parafac2.ragged).
    Returns a dict: B, A, C, projections (K x I x R), profiles (K x I x R), losses (||X - model||^2 per
    iteration, the final one last), iterations, rc; for a list input projections and profiles are lists of K
    arrays rows[k] x R."""
    slices = isinstance(X, (list, tuple))
    if slices:
        X = list(X)
        dev, (J, K) = X[0].device, (X[0].shape[1], len(X))
    else:
        if X.stride(0) != 1:
            X = X.permute(2, 1, 0).contiguous().permute(2, 1, 0)
        dev = X.device
    own = ctx is None
    ctx = ctx or Context(dev.index or 0)
    if slices:
        p2 = Parafac2.ragged(ctx, [x.shape[0] for x in X], J, R, dtype)
    else:
        I, J, K = X.shape
        p2 = Parafac2(ctx, I, J, K, R, dtype)
    try:
        if A0 is not None:
            p2.cp.set_factors([np.eye(R), np.asarray(A0, dtype=np.float64), np.ones((K, R))])
        if nonneg_modes:
            if 0 in nonneg_modes:
                raise ValueError("mode 0 (B) must stay free in PARAFAC2")
            p2.cp.set_mode_constraints(["nonneg" if m in nonneg_modes else "free" for m in range(3)])
        losses, rc, it = [], 0, 0
        for it in range(int(n_iter)):
            losses.append(p2.loss(X))
            if rel_change > 0 and it > 0 and losses[-2] - losses[-1] <= rel_change * losses[-2]:
                rc = 2
                break
            p2.cp.sweeps_dt(inner_sweeps)
        else:
            it = int(n_iter)
            losses.append(p2.loss(X))
        B, A, Cm = p2.cp.get_factors()
        return dict(B=B, A=A, C=Cm, projections=p2.projections(), profiles=p2.profiles(), losses=losses,
                    iterations=it, rc=rc)
    finally:
        p2.close()
        if own:
            ctx.close()


class _NplsOpts(C.Structure):
    _fields_ = [("hopm_tol", C.c_double), ("hopm_max", C.c_int), ("inner_tol", C.c_double), ("inner_max", C.c_int)]


NPLS_T, NPLS_U, NPLS_Q, NPLS_B, NPLS_SSX, NPLS_SSY, NPLS_STATUS, NPLS_W = 0, 1, 2, 3, 4, 5, 6, 16  # PPALS_NPLS_*


def _host_matrix(Y):
    """numpy, or a torch tensor on any device, as an fp64 Fortran-ordered I x M array on the host"""
    if type(Y).__module__.split(".")[0] == "torch":
        Y = Y.detach().cpu().numpy()
    Y = np.asarray(Y, dtype=np.float64)
    return np.asfortranarray(Y.reshape(Y.shape[0], -1) if Y.ndim != 2 else Y)


class NPLS:
    """N-PLS regression (multilinear PLS, Bro 1996) of Y (I x M) on the resident tensor, `mode` its sample mode;
    both centred by the caller (Tensor.center). The tensor is only read: no copy, no deflation, live sessions are
    undisturbed. After fit: scores (I x F), y_scores (I x F), weights (a lens x F matrix for every mode off the
    sample mode), y_loadings (M x F), inner (F x F, upper triangular), ssx, ssy (cumulative explained variation) and
    status (bit 0: the power iterations hit their cap, bit 1: the loop over q did). F may be smaller than ncomp:
    the fit ends where nothing is left to explain."""

    def __init__(self, hopm_tol=1e-12, hopm_max=500, inner_tol=1e-12, inner_max=200):
        self._opts = _NplsOpts(hopm_tol, hopm_max, inner_tol, inner_max)
        self._h = C.c_void_p()

    def _opts_tuple(self):
        o = self._opts
        return o.hopm_tol, o.hopm_max, o.inner_tol, o.inner_max

    def _get(self, what, shape):
        n = C.c_int64(0)
        _check(lib().ppals_npls_get(self._h, what, None, C.byref(n)))
        out = np.empty(n.value, dtype=np.float64)
        _check(lib().ppals_npls_get(self._h, what, _dp(out), C.byref(n)))
        return out.reshape(shape, order="F")

    def fit(self, tensor, Y, ncomp, mode=0):
        self.close()
        Yh = _host_matrix(Y)
        mode = int(mode)
        I = tensor.lens[mode] if 0 <= mode < len(tensor.lens) else Yh.shape[0]
        if Yh.shape[0] != I:
            raise PpalsError(f"Y has {Yh.shape[0]} rows, the sample mode {I}")
        M = Yh.shape[1]
        _check(lib().ppals_npls_fit(tensor._h, mode, _dp(Yh), M, int(ncomp), C.byref(self._opts), C.byref(self._h)))
        fitted = C.c_int(0)
        _check(lib().ppals_npls_dims(self._h, None, None, None, None, None, C.byref(fitted)))
        F = fitted.value
        self.mode, self.lens, self.ncomp, self.M = mode, list(tensor.lens), F, M
        self.scores = self._get(NPLS_T, (I, F))
        self.y_scores = self._get(NPLS_U, (I, F))
        self.y_loadings = self._get(NPLS_Q, (M, F))
        self.inner = self._get(NPLS_B, (F, F))
        self.ssx, self.ssy = self._get(NPLS_SSX, (F,)), self._get(NPLS_SSY, (F,))
        self.status = self._get(NPLS_STATUS, (F,)).astype(np.int64)
        off = [n for i, n in enumerate(tensor.lens) if i != mode]
        self.weights = [self._get(NPLS_W + k, (n, F)) for k, n in enumerate(off)]
        return self

    def predict(self, tensor, ncomp=None, return_scores=False):
        """Yhat (I_new x M, numpy) for a tensor with the training extents off the sample mode, from the first ncomp
        components (default: all): one pass over the tensor. return_scores: (Yhat, T_new)."""
        k = self.ncomp if ncomp is None else int(ncomp)
        I = tensor.lens[self.mode] if self.mode < len(tensor.lens) else 1
        Yhat = np.empty((I, self.M), dtype=np.float64, order="F")
        Tn = np.empty((I, max(k, 0)), dtype=np.float64, order="F")
        _check(lib().ppals_npls_predict(self._h, tensor._h, k, _dp(Yhat), _dp(Tn)))
        return (Yhat, Tn) if return_scores else Yhat

    def close(self):
        if self._h:
            lib().ppals_npls_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def npls(tensor, Y, ncomp, mode=0, **opts):
    """NPLS(**opts).fit(tensor, Y, ncomp, mode)"""
    return NPLS(**opts).fit(tensor, Y, ncomp, mode)


class NplsCrossval:
    """The record of npls_crossval: Ycv (I x M x F, the prediction of sample i from the first f + 1 components of the
    fit without its segment), press (F x M), rmsecv = sqrt(press / I), best_ncomp (1-based: the first minimum of PRESS
    summed over the responses), fitted (S: the components each resampled fit reached), status (S x F), x_passes (how
    often the tensor was read) and segments (the I labels used)."""

    def __init__(self, Ycv, press, fitted, status, x_passes, segments):
        self.Ycv, self.press, self.fitted, self.status, self.x_passes, self.segments = Ycv, press, fitted, status, x_passes, segments
        self.rmsecv = np.sqrt(press / Ycv.shape[0])
        self.best_ncomp = int(np.argmin(press.sum(axis=1))) + 1


def npls_crossval(tensor, Y, ncomp, mode=0, segments=7, center=True, split="interleave", **opts):
    """Leave-segments-out cross-validation of N-PLS with 1 .. ncomp components on the resident tensor (ppals.h, "N-PLS
    cross-validation"): all resampled fits share every pass over the tensor, which is neither written nor copied.
    segments: a count (labels from holdout_segments(I, segments, split)) or an array of I labels in [0, S), S their
    largest + 1. center: every fit centres X and Y on its own training samples (pass the tensor as it is). opts: those
    of NPLS. Returns an NplsCrossval."""
    Yh = _host_matrix(Y)
    mode = int(mode)
    I = tensor.lens[mode] if 0 <= mode < len(tensor.lens) else Yh.shape[0]
    if Yh.shape[0] != I:
        raise PpalsError(f"Y has {Yh.shape[0]} rows, the sample mode {I}")
    if np.ndim(segments) == 0:
        S = int(segments)
        seg = np.argmin(holdout_segments(I, S, split), axis=0)
    else:
        seg = np.asarray(segments).ravel()
        if seg.size != I:
            raise PpalsError(f"{seg.size} segment labels for {I} samples")
        S = int(seg.max()) + 1
    seg = np.ascontiguousarray(seg, dtype=np.int32)
    M, F = Yh.shape[1], int(ncomp)
    o = _NplsOpts(*NPLS(**opts)._opts_tuple())
    Ycv = np.zeros((I, M, max(F, 0)), dtype=np.float64, order="F")
    press = np.zeros((max(F, 0), M), dtype=np.float64, order="F")
    fitted, status = np.zeros(max(S, 0), dtype=np.int32), np.zeros((max(S, 0), max(F, 0)), dtype=np.int32, order="F")
    passes = C.c_int64(0)
    _check(lib().ppals_npls_crossval(tensor._h, mode, _dp(Yh), M, F, seg.ctypes.data_as(C.POINTER(C.c_int32)), S,
                                     int(bool(center)), C.byref(o), _dp(Ycv), _dp(press),
                                     fitted.ctypes.data_as(C.POINTER(C.c_int)), status.ctypes.data_as(C.POINTER(C.c_int)),
                                     C.byref(passes)))
    return NplsCrossval(Ycv, press, fitted.astype(np.int64), status.astype(np.int64), int(passes.value), seg.astype(np.int64))


class CPMulti:
    """K independent rank-R CP-ALS starts of one tensor that share every tensor scan (ppals_cp_multi):
    start b evolves as an ordinary CP session does under cpd_als(0, ...) from the same factors. No
    Normalize, PP or drivers here: take() the winner into a CP session and go on there.
    CPMulti.with_ranks(ctx, V, ranks) is a rank sweep: start b is a rank-ranks[b] model
    (ppals_cp_multi_create_ranks). `ranks` lists every start's rank, [R] * nstarts here."""

    def __init__(self, ctx, V, R, nstarts):
        self.ctx, self.V, self.R, self.nstarts = ctx, V, int(R), int(nstarts)
        self.lens = V.lens
        self._h = C.c_void_p()
        _check(lib().ppals_cp_multi_create(ctx._h, V._h, int(R), int(nstarts), C.byref(self._h)))
        self.ranks = self._read_ranks()
        ctx._children.add(self)

    @classmethod
    def with_ranks(cls, ctx, V, ranks):
        """a session whose starts have their own ranks; R is the common rank, None when they differ"""
        self = cls.__new__(cls)
        ranks = [int(r) for r in ranks]
        self.ctx, self.V, self.nstarts, self.lens = ctx, V, len(ranks), V.lens
        self.R = ranks[0] if ranks and len(set(ranks)) == 1 else None
        self._h = C.c_void_p()
        arr = (C.c_int * max(len(ranks), 1))(*ranks)
        _check(lib().ppals_cp_multi_create_ranks(ctx._h, V._h, len(ranks), arr, C.byref(self._h)))
        self.ranks = self._read_ranks()
        ctx._children.add(self)
        return self

    def _read_ranks(self):
        k = C.c_int(0)
        _check(lib().ppals_cp_multi_ranks(self._h, C.byref(k), None))
        arr = (C.c_int * k.value)()
        _check(lib().ppals_cp_multi_ranks(self._h, C.byref(k), arr))
        return list(arr)

    def _n(self, b):
        return sum(s * self.ranks[b] for s in self.lens)

    def set_factors(self, start, Ws, gradWs=None):
        """one start's factors (list of (s_i, R) arrays); start = -1: Ws (and gradWs) are lists of
        nstarts such lists"""
        if start == -1:
            wf = np.concatenate([flat(W) for W in Ws])
            gf = np.concatenate([flat(G) for G in gradWs]) if gradWs is not None else None
        else:
            wf = flat(Ws)
            gf = flat(gradWs) if gradWs is not None else None
        _check(lib().ppals_cp_multi_set_factors(self._h, int(start), _dp(wf),
                                                _dp(gf) if gf is not None else None))

    def get_factors(self, start, with_grad=False):
        starts = list(range(self.nstarts)) if start == -1 else [int(start)]
        starts = [b for b in starts if 0 <= b < self.nstarts]  # (a bad start: the library refuses)
        at = np.concatenate([[0], np.cumsum([self._n(b) for b in starts])]).astype(int)
        wf = np.empty(at[-1])
        gf = np.empty(at[-1]) if with_grad else None
        _check(lib().ppals_cp_multi_get_factors(self._h, int(start), _dp(wf),
                                                _dp(gf) if with_grad else None))
        cut = lambda f: [unflat(f[at[k]:at[k + 1]], self.lens, [self.ranks[b]] * len(self.lens))
                         for k, b in enumerate(starts)]
        W = cut(wf)
        G = cut(gf) if with_grad else None
        if start != -1:
            W, G = W[0], (G[0] if with_grad else None)
        return (W, G) if with_grad else W

    def set_schedule(self, schedule):
        code = {"dt": 0, "msdt": 1}[schedule] if isinstance(schedule, str) else int(schedule)
        _check(lib().ppals_cp_multi_set_schedule(self._h, code))

    def set_nonneg(self, on=True):
        """non-negative multi-start: every start updates by the HALS pass of CP.set_nonneg, all starts in
        one batched update per mode. Factors of any start with a negative or non-finite entry are refused."""
        _check(lib().ppals_cp_multi_set_nonneg(self._h, 1 if on else 0))

    @property
    def nonneg(self):
        return bool(_check(lib().ppals_cp_multi_get_nonneg(self._h)))

    def set_mode_constraints(self, kinds):
        """CP.set_mode_constraints for every start: one kind per mode, shared by all starts"""
        _check(lib().ppals_cp_multi_set_mode_constraints(self._h, _kinds(kinds, len(self.lens))))

    @property
    def mode_constraints(self):
        out = (C.c_int * len(self.lens))()
        _check(lib().ppals_cp_multi_get_mode_constraints(self._h, out))
        return [MODE_KINDS[k] for k in out]

    def set_mode_shapes(self, shapes):
        """CP.set_mode_shapes for every start: one shape per mode, shared by all starts (not on the hold-out
        mode)"""
        _check(lib().ppals_cp_multi_set_mode_shapes(self._h, _shapes(shapes, len(self.lens))))

    @property
    def mode_shapes(self):
        out = (C.c_int * len(self.lens))()
        _check(lib().ppals_cp_multi_get_mode_shapes(self._h, out))
        return [SHAPE_KINDS[k] for k in out]

    def sweeps(self, n, lam=0.0):
        _check(lib().ppals_cp_multi_sweeps(self._h, int(n), C.c_double(lam)))

    def residuals(self):
        out = np.empty(self.nstarts)
        _check(lib().ppals_cp_multi_residuals(self._h, _dp(out)))
        return out

    def gradnorms(self):
        out = np.empty(self.nstarts)
        _check(lib().ppals_cp_multi_gradnorms(self._h, _dp(out)))
        return out

    def core_consistencies(self):
        """the core consistency of every start (CP.core_consistency), all starts on ONE tensor scan; NaN
        for a start one of whose factors has no pseudo-inverse"""
        out = np.empty(self.nstarts)
        _check(lib().ppals_cp_multi_core_consistency(self._h, _dp(out)))
        return out

    def core(self, start):
        """start's core, shape (ranks[start],) * order (all NaN where core_consistencies gives NaN)"""
        n = C.c_int64(0)
        _check(lib().ppals_cp_multi_core(self._h, int(start), None, C.byref(n)))
        out = np.empty(n.value)
        _check(lib().ppals_cp_multi_core(self._h, int(start), _dp(out), C.byref(n)))
        return out.reshape((self.ranks[int(start)],) * len(self.lens), order="F")

    def congruence(self, other=None, skip_mode=None):
        """Phi (C, C'): all columns of all starts against those of other (None: this session itself), start
        b owning rows / columns [sum(ranks[:b]), sum(ranks[:b + 1])) (ppals_cp_multi_congruence)"""
        o = self if other is None else other
        out = np.empty((sum(self.ranks), sum(o.ranks)), order="F")
        n = C.c_int64(0)
        _check(lib().ppals_cp_multi_congruence(self._h, None if other is None else other._h,
                                               _skip(skip_mode), _dp(out), C.byref(n)))
        return out

    def fms(self, skip_mode=None, weights=False):
        """(nstarts, nstarts): the factor match score of every pair of starts, each with its own rank, from
        one congruence of all columns (ppals_cp_multi_fms)"""
        out = np.empty((self.nstarts, self.nstarts), order="F")
        _check(lib().ppals_cp_multi_fms(self._h, _skip(skip_mode), FMS_WEIGHTS if weights else 0, _dp(out)))
        return out

    def fms_between(self, other, skip_mode=None, weights=False):
        """(nstarts,): start k against start k of other, a session with as many starts (their ranks and,
        in skip_mode, the extents may differ): the split-half comparison (ppals_cp_multi_fms_between)"""
        out = np.empty(self.nstarts)
        _check(lib().ppals_cp_multi_fms_between(self._h, other._h, _skip(skip_mode),
                                                FMS_WEIGHTS if weights else 0, _dp(out)))
        return out

    def run(self, **kw):
        """returns (rc, sweeps, best): rc 1 if it stopped on tol / timelimit before maxiter sweeps"""
        o = _opts(**kw)
        sw, best = C.c_int(0), C.c_int(0)
        rc = _check(lib().ppals_cp_multi_run(self._h, C.byref(o), C.byref(sw), C.byref(best)))
        return rc, sw.value, best.value

    def take(self, start, dst):
        """start's factors and gradients into the CP session dst (same tensor, the start's rank), on the device"""
        _check(lib().ppals_cp_multi_take(self._h, int(start), dst._h))
        return dst

    # ---- hold-out rows per start (ppals_cp_multi_set_holdout): resampled fits on the shared scans ----
    def set_holdout(self, mode, keep):
        """keep: (nstarts, s_mode) bool array, False = start b holds sample x of `mode` out — start b then
        evolves as a session on the tensor without those slices does, and heldout_scores(b) carries the
        held-out samples' predicted scores. None clears the hold-out (mode is ignored)."""
        if keep is None:
            _check(lib().ppals_cp_multi_set_holdout(self._h, -1, None))
            return
        mode = int(mode)
        n = self.lens[mode] if 0 <= mode < len(self.lens) else -1   # (a bad mode: the library refuses)
        k = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
        if n >= 0 and k.shape != (self.nstarts, n):
            raise PpalsError(f"set_holdout: keep has shape {k.shape}, not {(self.nstarts, n)}")
        _check(lib().ppals_cp_multi_set_holdout(self._h, mode, k.ctypes.data_as(C.POINTER(C.c_uint8))))

    @property
    def holdout(self):
        """(mode, keep) of the hold-out, keep an (nstarts, s_mode) bool array; None without one"""
        mode = C.c_int(-1)
        _check(lib().ppals_cp_multi_get_holdout(self._h, C.byref(mode), None))
        if mode.value < 0:
            return None
        k = np.zeros((self.nstarts, self.lens[mode.value]), dtype=np.uint8)
        _check(lib().ppals_cp_multi_get_holdout(self._h, C.byref(mode), k.ctypes.data_as(C.POINTER(C.c_uint8))))
        return mode.value, k != 0

    def heldout_scores(self, start):
        """(s_mode, ranks[start]): the held-out samples' rows from the sample mode's most recent update
        (before any: the rows the caller set); rows of kept samples are 0"""
        b = int(start)
        h = self.holdout
        if h is None or not 0 <= b < self.nstarts:   # (the library refuses both, with its message)
            _check(lib().ppals_cp_multi_heldout_scores(self._h, b, _dp(np.empty(1))))
            raise PpalsError("heldout_scores: no hold-out, or start out of range")
        out = np.empty((self.lens[h[0]], self.ranks[b]), order="F")
        _check(lib().ppals_cp_multi_heldout_scores(self._h, b, _dp(out)))
        return out

    def take_predicted(self, start, dst):
        """take() with the sample-mode factor carrying the predicted scores in the held-out rows (W + scores)"""
        _check(lib().ppals_cp_multi_take_predicted(self._h, int(start), dst._h))
        return dst

    def sample_residuals(self, start, dst):
        """take_predicted(start, dst), then dst.slice_residuals()[mode]: per sample of the hold-out mode the
        sum of (V - model)^2 over its slice — the fit of a kept sample, the prediction error of a held-out one"""
        self.take_predicted(start, dst)
        return dst.slice_residuals()[self.holdout[0]]

    def close(self):
        if self._h:
            lib().ppals_cp_multi_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Tucker(_ModelExport, _Impute):
    _export_fn = "ppals_tucker_export_model_device"
    _impute_fn, _em_fn = "ppals_tucker_impute_device", "ppals_tucker_em"

    def __init__(self, ctx, V, ranks):
        self.ctx, self.V = ctx, V
        self.lens, self.ranks = V.lens, [int(r) for r in ranks]
        self._h = C.c_void_p()
        arr = (C.c_int * len(ranks))(*self.ranks)
        _check(lib().ppals_tucker_create(ctx._h, V._h, arr, C.byref(self._h)))
        ctx._children.add(self)

    def set_factors(self, Ws):
        wf = flat(Ws)
        _check(lib().ppals_tucker_set_factors(self._h, _dp(wf)))

    def set_core(self, core=None):
        """the `core` argument of alsTucker_DT/_PP; None: recompute it from V and the factors"""
        if core is None:
            _check(lib().ppals_tucker_set_core(self._h, None))
        else:
            cf = np.asfortranarray(core, dtype=np.float64).ravel(order="F").copy()
            _check(lib().ppals_tucker_set_core(self._h, _dp(cf)))

    def get_factors(self):
        wf = np.empty(sum(s * r for s, r in zip(self.lens, self.ranks)))
        core = np.empty(int(np.prod(self.ranks)))
        _check(lib().ppals_tucker_get_factors(self._h, _dp(wf), _dp(core)))
        return unflat(wf, self.lens, self.ranks), core.reshape(self.ranks, order="F")

    def hosvd(self):
        _check(lib().ppals_tucker_hosvd(self._h))

    def ttmc(self, skip):
        n = C.c_int64(0)
        shape = [self.lens[i] if i == skip else self.ranks[i] for i in range(len(self.lens))]
        Y = np.empty(int(np.prod(shape)))
        _check(lib().ppals_tucker_ttmc(self._h, skip, _dp(Y), C.byref(n)))
        return Y.reshape(shape, order="F")

    def sweeps_dt(self, n):
        _check(lib().ppals_tucker_sweeps_dt(self._h, n))

    def run_dt(self, **kw):
        o = _opts(**kw)
        it = C.c_int(0)
        rc = _check(lib().ppals_tucker_dt(self._h, C.byref(o), C.byref(it)))
        return rc, it.value

    def run_pp(self, **kw):
        o = _opts(**kw)
        it = C.c_int(0)
        rc = _check(lib().ppals_tucker_pp(self._h, C.byref(o), C.byref(it)))
        return rc, it.value

    def residual(self):
        """||V - core x_i W_i||_F of the factors and core get_factors would return now (ppals_tucker_residual)"""
        out = C.c_double(0)
        _check(lib().ppals_tucker_residual(self._h, C.byref(out)))
        return out.value

    _per_mode = CP._per_mode

    def slice_residuals(self, return_total=False):
        """the residual side of the influence plot (ppals_tucker_slice_residuals): a list of N vectors, entry x
        of vector i the sum of (V - model)^2 over the slice x of mode i — one pass over the tensor, nothing
        materialised. return_total: (list, total), total = residual()**2 up to rounding. Changes nothing of
        the session beyond the settle of get_factors."""
        out = np.empty(sum(self.lens))
        total = C.c_double(0)
        _check(lib().ppals_tucker_slice_residuals(self._h, _dp(out), C.byref(total)))
        ss = self._per_mode(out)
        return (ss, total.value) if return_total else ss

    def leverages(self):
        """the leverage side (ppals_tucker_leverages): a list of N vectors, entry x of vector i the x-th
        diagonal entry of the projector onto the columns of W_i (the row's sum of squares for the orthonormal
        factors a sweep leaves); all NaN when a factor is rank deficient. Never reads the tensor."""
        out = np.empty(sum(self.lens))
        _check(lib().ppals_tucker_leverages(self._h, _dp(out)))
        return self._per_mode(out)

    def explained(self):
        """core**2 / ||V||**2, shaped like the core: the share of the tensor's variation each core entry
        explains. Meaningful for ORTHONORMAL factors (what hosvd and every sweep leave): the entries then sum
        to 1 - residual()**2 / ||V||**2. A host helper on get_factors."""
        core = self.get_factors()[1]
        return core ** 2 / self.V.norm() ** 2

    def close(self):
        if self._h:
            lib().ppals_tucker_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def project(ctx, V, mode, W, lam=0.0):
    """The calibration step: the least-squares scores of the slices of the Tensor V along `mode` under given
    loadings. W lists one (s_i, R) factor per mode with None at `mode`. A session with every other mode FIXED
    and zeros in `mode` runs one sweep of cpd_als(0): the MTTKRP of `mode` and the solve of its normal
    equations (+ lam I), nothing else. Returns the (s_mode, R) scores; closes what it opened."""
    N = len(V.lens)
    if len(W) != N or W[mode] is not None or any(w is None for i, w in enumerate(W) if i != mode):
        raise ValueError("W lists one factor per mode, None at `mode` and only there")
    R = int(np.shape(W[(mode + 1) % N])[1])
    s = CP(ctx, V, R)
    try:
        s.set_mode_constraints([MODE_FREE if i == mode else MODE_FIXED for i in range(N)])
        s.set_factors([np.zeros((V.lens[mode], R)) if i == mode else w for i, w in enumerate(W)])
        s.cpd_als(0, maxiter=0, tol=0.0, lam=lam, resprint=1 << 30)
        return s.get_factors()[mode]
    finally:
        s.close()


def split_half(ctx, x, mode, ranks, sweeps, seed=0, dtype=F32, split="interleave"):
    """Split-half validation (Harshman) of a torch tensor x in HBM: the two halves of x along `mode` —
    "interleave": the even and the odd indices, "blocks": [0, s // 2) and [s // 2, s) — are imported as
    strided views (Tensor.from_torch: no copy on the torch side), a CPMulti.with_ranks(ranks) session is
    created on each, its factors drawn with numpy.random.default_rng(seed).random((s_i, r)) in the order
    half 0 then half 1, start by start, mode by mode, and swept `sweeps` times. Returns
    (fms, residuals of half 0, residuals of half 1), fms[k] = the factor match score of the rank-ranks[k]
    models of the two halves over all modes but `mode` (CPMulti.fms_between)."""
    mode = int(mode)
    s = x.shape[mode]
    if split == "interleave":
        idx = (slice(0, s, 2), slice(1, s, 2))
    elif split == "blocks":
        idx = (slice(0, s // 2), slice(s // 2, s))
    else:
        raise PpalsError(f"split_half: split must be 'interleave' or 'blocks', not {split!r}")
    rng = np.random.default_rng(seed)
    tensors, sessions = [], []
    try:
        for sl in idx:
            half = x[(slice(None),) * mode + (sl,)]
            t = Tensor.from_torch(ctx, half, dtype)
            tensors.append(t)
            m = CPMulti.with_ranks(ctx, t, ranks)
            sessions.append(m)
            m.set_factors(-1, [[rng.random((n, r)) for n in t.lens] for r in m.ranks])
            m.sweeps(sweeps)
        fms = sessions[0].fms_between(sessions[1], skip_mode=mode)
        return fms, sessions[0].residuals(), sessions[1].residuals()
    finally:
        for h in sessions + tensors:
            h.close()


def holdout_segments(n, K, split="interleave"):
    """(K, n) bool keep masks of a segmented leave-samples-out scheme over n samples: segment g leaves out
    the samples x with x % K == g ("interleave") or the g-th of K contiguous blocks ("blocks", sizes as
    numpy.array_split). Every sample is left out by exactly one segment. Rows for CPMulti.set_holdout."""
    n, K = int(n), int(K)
    if K < 1 or K > n:
        raise PpalsError(f"holdout_segments: K must be in [1, {n}], not {K}")
    if split == "interleave":
        seg = np.arange(n) % K
    elif split == "blocks":
        seg = np.concatenate([np.full(len(c), g) for g, c in enumerate(np.array_split(np.arange(n), K))])
    else:
        raise PpalsError(f"holdout_segments: split must be 'interleave' or 'blocks', not {split!r}")
    return seg[None, :] != np.arange(K)[:, None]


def jackknife(ctx, V, mode, R, segments, sweeps, W0=None, seed=0, split="interleave"):
    """The segmented jackknife of a rank-R PARAFAC model over the samples of `mode` (Riu & Bro 2003) in ONE
    multi-start session on the tensor V: start 0 keeps every sample (the reference fit), start g leaves out
    segment g - 1 of holdout_segments(s_mode, segments, split); all `segments + 1` fits share every tensor
    scan of the `sweeps` sweeps. All starts begin from the same W0 — a list of (s_i, R) arrays, by default
    numpy.random.default_rng(seed).random((s_i, R)) mode by mode; a list of segments + 1 such lists gives
    every start its own. Refused when segments + 1 > 32 or (segments + 1) * R > 128 (CPMulti's limits).

    Each start is then aligned to start 0: its columns are matched to the reference's (match_columns on the
    absolute congruence over all modes but `mode`), and in each mode other than `mode` each column is scaled
    to unit norm and given the sign of its dot product with the matched reference column; the product of
    those signs and norms goes into the sample mode and the predicted scores, so the model is unchanged.
    Returns a dict:
      loadings[i]  (segments, s_i, R): the aligned factors (in `mode`: zero rows where a sample was left out)
      se[i]        (s_i, R), i != mode: the jackknife standard error sqrt((K - 1) / K * sum_g (a_g - mean)^2),
                   K = segments; None for `mode`
      reference    start 0's factors in the same normalisation
      scores       (s_mode, R): each sample's predicted score from the start that left it out
      fms          (segments,): the factor match score of each start against the reference, `mode` skipped: the
                   mean absolute congruence of the matched columns (the skipped mode can carry a sign)
      press        (s_mode,): each sample's prediction error (CPMulti.sample_residuals) from that start
    Leave-samples-out PRESS projects a sample with its own data and so falls with the rank: it is an outlier
    diagnostic, not a rank selector. Element-wise cross-validation is what run_em with a mask is for."""
    mode, R, K = int(mode), int(R), int(segments)
    N = len(V.lens)
    if not 0 <= mode < N:
        raise PpalsError(f"jackknife: mode must be in [0, {N}), not {mode}")
    if K < 2:
        raise PpalsError("jackknife: at least 2 segments")
    if K + 1 > 32 or (K + 1) * R > 128:
        raise PpalsError(f"jackknife: segments + 1 = {K + 1} starts of rank {R} exceed a multi-start session "
                         "(32 starts, 128 columns)")
    n = V.lens[mode]
    keep = np.vstack([np.ones((1, n), dtype=bool), holdout_segments(n, K, split)])
    if W0 is None:
        rng = np.random.default_rng(seed)
        W0 = [rng.random((s, R)) for s in V.lens]
    per_start = list(W0) if isinstance(W0[0], (list, tuple)) else [W0] * (K + 1)
    if len(per_start) != K + 1:
        raise PpalsError(f"jackknife: W0 lists {len(per_start)} starts, not {K + 1}")
    m = dst = None
    try:
        m = CPMulti(ctx, V, R, K + 1)
        m.set_holdout(mode, keep)
        m.set_factors(-1, per_start)
        m.sweeps(int(sweeps))
        Ws = m.get_factors(-1)
        phi = np.abs(m.congruence(skip_mode=mode))
        held = [m.heldout_scores(g) for g in range(K + 1)]
        dst = CP(ctx, V, R)
        press = np.zeros(n)
        for g in range(1, K + 1):
            press[~keep[g]] = m.sample_residuals(g, dst)[~keep[g]]
    finally:
        for h in (dst, m):
            if h is not None:
                h.close()

    def normalised(W, sc, ref):
        """modes != mode to unit norm (and the sign of <column, ref column> if ref), the rest into `mode`"""
        W = [w.copy() for w in W]
        f = np.ones(R)
        for i in range(N):
            if i == mode:
                continue
            c = np.linalg.norm(W[i], axis=0)
            if ref is not None:
                c = c * np.where(np.sum(W[i] * ref[i], axis=0) < 0, -1.0, 1.0)
            W[i] = W[i] / c
            f = f * c
        W[mode] = W[mode] * f
        return W, sc * f

    ref_raw = Ws[0]
    loadings = [np.empty((K, s, R)) for s in V.lens]
    scores, fms = np.zeros((n, R)), np.empty(K)
    for g in range(1, K + 1):
        perm, total = match_columns(phi[g * R:(g + 1) * R, :R])   # column p of start g <-> column perm[p] of start 0
        fms[g - 1] = total / R
        inv = np.argsort(perm)
        Wg, sg = normalised([w[:, inv] for w in Ws[g]], held[g][:, inv], ref_raw)
        for i in range(N):
            loadings[i][g - 1] = Wg[i]
        scores[~keep[g]] = sg[~keep[g]]
    se = [None if i == mode else
          np.sqrt((K - 1) / K * np.sum((loadings[i] - loadings[i].mean(axis=0)) ** 2, axis=0)) for i in range(N)]
    reference, _ = normalised(ref_raw, np.zeros((n, R)), None)
    return dict(loadings=loadings, se=se, reference=reference, scores=scores, fms=fms, press=press)


# ---- reference-named entry points (als_CP.h / als_Tucker.h), argument order preserved ----
def alsCP_DT(V, W, grad_W, tol, timelimit, maxiter, lambda_, Plot_File, resprint, bench, dw):
    """alsCP_DT(V, W, grad_W, F, tol, timelimit, maxiter, lambda, Plot_File, resprint, bench, dw)
    (als_CP.h:30-32) — F is always zero in the reference and is dropped. W/grad_W are updated in
    place (lists of numpy arrays). Returns the reference's bool."""
    s = CP(dw, V, W[0].shape[1])
    s.set_factors(W, grad_W)
    rc, _ = s.run_dt(tol=tol, timelimit=timelimit, maxiter=maxiter, lam=lambda_, csv=Plot_File,
                     resprint=resprint, bench=int(bench))
    Wn, Gn = s.get_factors(with_grad=True)
    for a, b in zip(W, Wn):
        a[...] = b
    for a, b in zip(grad_W, Gn):
        a[...] = b
    s.close()
    return bool(rc)


def alsCP_PP(V, W, grad_W, tol, tol_init, timelimit, maxiter, lambda_, ratio_step, Plot_File,
             resprint, bench, dw):
    """alsCP_PP (als_CP.h:105-108), F dropped"""
    s = CP(dw, V, W[0].shape[1])
    s.set_factors(W, grad_W)
    rc, _ = s.run_pp(tol=tol, tol_init=tol_init, timelimit=timelimit, maxiter=maxiter,
                     lam=lambda_, ratio_step=ratio_step, csv=Plot_File, resprint=resprint,
                     bench=int(bench))
    Wn, Gn = s.get_factors(with_grad=True)
    for a, b in zip(W, Wn):
        a[...] = b
    for a, b in zip(grad_W, Gn):
        a[...] = b
    s.close()
    return bool(rc)
