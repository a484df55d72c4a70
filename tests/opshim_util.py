"""Loads tests/opshim (TEST INFRASTRUCTURE: a C surface over ppals::Ops, see ops_shim.cpp) through ctypes:
kind "hip" is the product's Ops over the HIP kernels of libppals.so, kind "host" the host stand-in. Neither
needs torch; the library is built on first use, as hipsim_util.load does."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "opshim")
F32, F64, BF16 = 0, 1, 3
_libs = {}

_P, _I64, _I, _U, _D, _U64 = C.c_void_p, C.c_int64, C.c_int, C.c_uint, C.c_double, C.c_uint64
_SIGS = {
    "shim_alloc": [_P, C.c_size_t, C.POINTER(_P)],
    "shim_free": [_P, _P],
    "shim_h2d": [_P, _P, _P, C.c_size_t],
    "shim_d2h": [_P, _P, _P, C.c_size_t],
    "shim_sync": [_P],
    "shim_scan_store_mode": [_P, _I],
    "shim_scan_contract": [_P, _P, _I, _I64, _I64, _I64, C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I64), _I, _I,
                           _P, _I, _I64, _I64, _I64, _I64],
    "shim_mttv": [_P, _P, _I, _I64, _I64, _I64, C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I64), _I, _I, _P, _I64,
                  _I, _P],
    "shim_ttm_keep": [_P, _P, _I, _I64, _I64, _I64, _P, _I64, _I, _P],
    "shim_ttm_lead_front": [_P, _P, _I, _I64, _I64, _I64, _P, _I64, _I, _P, C.POINTER(_I)],
    "shim_pp_correct": [_P, _P, _I64, _I, C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I), C.POINTER(_P),
                        C.POINTER(_I64), _I, _P],
    "shim_arm_gram_system": [_P, _P, _I, _I, _I, C.c_double, _P, _P],
    "shim_gram": [_P, _P, _I64, _I64, _I, _P],
    "shim_gram_batched": [_P, _P, _I64, _I64, _I, _I, _P, _I64],
    "shim_gram_system": [_P, _P, _I, _I, _I, _D, _P, _P],
    "shim_cp_update": [_P, _P, _I64, _P, _I64, _P, _I64, _P, _I64, _I64, _I, _P, _P, _P, _P, _I64, _P, _I64, _D],
    "shim_cp_mode_update": [_P, _P, _I, _I, _I, _D, _P, _I64, _P, _I64, _P, _I64, _I64, _P, _P, _I64, _P, _I64, _D,
                            _P, _P, _P],
    "shim_cp_mode_update_batched": [_P, _P, _I, _I, _I, _I, _D, _P, _I64, _P, _I64, _P, _I64, _I64, _P, _P, _P],
    "shim_cp_mode_update_blocked": [_P, _P, _I, _I, _I, _D, _P, _I64, _I, _P, _P, _I64, _P, _I64, _I64, _P, _P, _I64,
                                    _P, _I64, _D, _P, _P],
    "shim_arm_normalize": [_P, C.POINTER(_P), C.POINTER(_I64), _I, _I, _P, _I, _P, _P, C.POINTER(_U), _U, _U,
                           C.POINTER(_I)],
    "shim_normalize": [_P, C.POINTER(_P), C.POINTER(_I64), _I, _I, _P],
    "shim_normalize_ms": [_P, C.POINTER(_P), C.POINTER(_I64), _I, _I, _P, _P, C.POINTER(_U), _U, _U, _P],
    "shim_normalize_scales": [_P, C.POINTER(_P)],
    "shim_diff_norms": [_P, C.POINTER(_P), C.POINTER(_P), C.POINTER(_I64), _I, _I, C.POINTER(_P), _I, _P],
    "shim_pack_blocks": [_P, _P, _I64, _I64, _I, _I64, _I, _P],
    "shim_unpack_blocks": [_P, _P, _I64, _I64, _I, _I64, _I, _P],
    "shim_sumsq": [_P, _P, _I64, _P],
    "shim_scale_update": [_P, _P, _P, _U, _I],
    "shim_scale_update_many": [_P, _P, _P, C.POINTER(_U), _U, _U],
    "shim_d2d": [_P, _P, _P, C.c_size_t],
    "shim_unfold_gram": [_P, _P, _I, _I64, _I64, _I64, _P],
    "shim_top_eigvecs": [_P, _P, _I64, _I, _P],
    "shim_top_eigvecs_warm": [_P, _P, _I64, _I, _P, _I],
    "shim_eig_lazy": [_P, _I, _I],
    "shim_eig_defer": [_P, _I, _I],
    "shim_eig_gram": [_P, _I, _I64, C.POINTER(_P)],
    "shim_eig_deferred": [_P, _I, C.POINTER(_I)],
    "shim_eig_verify": [_P, _I, _I, C.POINTER(_I)],
    "shim_eig_pending_rotation": [_P, _I, C.POINTER(_P)],
    "shim_eig_rotation_done": [_P, _I],
    "shim_eig_session_new": [_P, C.POINTER(_I)],
    "shim_eig_session_free": [_P, _I],
    "shim_orthonormalize": [_P, _P, _I64, _I, C.POINTER(_I)],
    "shim_sign_align": [_P, _P, _P, _I64, _I],
    "shim_rows_times_small": [_P, _P, _I64, _I, _P, _I, _P, _P],
    "shim_lowrank_accumulate": [_P, _P, _I, _I64, _I, _P, _I, _P],
    "shim_add_inplace": [_P, _P, _P, _I64],
    "shim_transpose2d": [_P, _P, _I, _I64, _I64, _P],
    "shim_transpose_batched": [_P, _P, _I, _I64, _I64, _I64, _P],
    "shim_fill_uniform": [_P, _P, _I, _I64, _I64, _I64, _I64, _U64, _D, _D],
    "shim_fill_laplacian": [_P, _P, _I, _I64, _I64, _I64, _I64, _I, _I],
    "shim_add_uniform_noise": [_P, _P, _I, _I64, _I64, _I64, _I64, _U64, _D, _D, _D],
    "shim_uniform_sumsq": [_P, _I64, _I64, _I64, _I64, _U64, _D, _D, _P],
    "shim_fill_rank": [_P, _P, _I, _I64, _I64, _P, _P, _I],
    "shim_residual_sq": [_P, _P, _I, _I64, _I64, _P, _P, _I, _P],
    "shim_upload_shard": [_P, _P, _I, _P, _I64, _I64, _I64, _I64],
    "shim_download_shard": [_P, _P, _I, _P, _I64, _I64, _I64, _I64],
    "shim_pad_layout": [_P, _P, _I, _I64, _I64, _I64, _I64, _P],
    "shim_unpack_shards": [_P, _P, _I, _I64, _I64, _I64, _I, _I64, _P],
    "shim_krp": [_P, _P, C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I64), _I, _I, _I],
    "shim_cp_mode_update_ragged": [_P, _P, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _D, _P, _I64, _P, _I64, _P, _I64,
                                   _I64, _P, _P, _P],
    "shim_gram_ragged": [_P, _P, _I64, _I64, _I, C.POINTER(_I), C.POINTER(_I), _I, _I, _P],
    "shim_cp_mode_update_nn": [_P, _P, _I, _I, _I, _D, _P, _I64, _P, _I64, _P, _I64, _I64, _P, _P],
    "shim_cp_mode_update_nn_batched": [_P, _P, _I, _I, _I, _I, _D, _P, _I64, _P, _I64, _P, _I64, _I64, _P, _P],
    "shim_cp_mode_update_nn_ragged": [_P, _P, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), _D, _P, _I64, _P, _I64, _P,
                                      _I64, _I64, _P, _P],
    "shim_cp_hold_rows": [_P, _P, _I64, _P, _I64, _P, _I64, _I64, _I, C.POINTER(_I), C.POINTER(_I), _P, _U, _P, _I, _I,
                          _P],
    "shim_cp_pinv_ragged": [_P, _P, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_P), C.POINTER(_I64),
                            C.POINTER(_P), _P],
    "shim_core_score": [_P, _P, _I, _I, _P, _P],
    "shim_factor_congruence_work": [_P, _I, C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I64), _I, C.POINTER(_P),
                                    C.POINTER(_I64), C.POINTER(_I64), _I, C.POINTER(_I64)],
    "shim_factor_congruence": [_P, _I, C.POINTER(_P), C.POINTER(_I64), C.POINTER(_I64), _I, C.POINTER(_P),
                               C.POINTER(_I64), C.POINTER(_I64), _I, _U, _P, _P, _P, _P],
    "shim_row_dots": [_P, _P, _P, _I64, _I, _I64, _P],
    "shim_fold_slice_sums": [_P, _P, C.POINTER(_I64), _I, _P],
}


def load(kind, make=True):
    if kind not in _libs:
        path = os.path.join(DIR, "build", f"libopshim_{kind}.so")
        if make or not os.path.exists(path):
            subprocess.check_call(["make", "-s", "-C", DIR, kind])
        lib = C.CDLL(path)
        for name, args in _SIGS.items():
            f = getattr(lib, name)
            f.argtypes, f.restype = args, _I
        lib.shim_create.argtypes, lib.shim_create.restype = [_I], _P
        lib.shim_destroy.argtypes, lib.shim_destroy.restype = [_P], None
        lib.shim_route_attach.argtypes, lib.shim_route_attach.restype = [_P, _I], None
        lib.shim_route_clear.argtypes, lib.shim_route_clear.restype = [_P], None
        for name in ("shim_error", "shim_route_read"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [_P], C.c_char_p
        for name in ("shim_backend", "shim_create_error"):
            getattr(lib, name).argtypes, getattr(lib, name).restype = [], C.c_char_p
        _libs[kind] = lib
    return _libs[kind]


class ShimError(RuntimeError):
    """an exception of the back end, caught in the shim"""


def _arr(ctype, vals):
    return (ctype * max(1, len(vals)))(*vals)


class Shim:
    """One Ops of the back end `kind`, with its route log attached."""

    def __init__(self, kind, device=0):
        self.kind, self.lib = kind, load(kind)
        self.h = self.lib.shim_create(device)
        if not self.h:
            raise ShimError(self.lib.shim_create_error().decode())
        self.lib.shim_route_attach(self.h, 1)

    def close(self):
        if self.h:
            self.lib.shim_destroy(self.h)
            self.h = None

    def _ck(self, rc):
        if rc != 0:
            raise ShimError(self.lib.shim_error(self.h).decode())

    # ---- memory: device pointers are plain integers
    def alloc(self, nbytes):
        p = _P()
        self._ck(self.lib.shim_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, p):
        self._ck(self.lib.shim_free(self.h, p))

    def h2d(self, dst, a):
        a = np.ascontiguousarray(a)
        self._ck(self.lib.shim_h2d(self.h, dst, a.ctypes.data, a.nbytes))

    def d2h(self, src, nbytes):
        out = np.empty(nbytes, np.uint8)
        self._ck(self.lib.shim_d2h(self.h, out.ctypes.data, src, nbytes))
        return out

    def sync(self):
        self._ck(self.lib.shim_sync(self.h))

    # ---- the route log
    def route_take(self):
        tags = self.lib.shim_route_read(self.h).decode()
        self.lib.shim_route_clear(self.h)
        return tags.split("\n") if tags else []

    # ---- the ops; factors: list of (device pointer, rows, ld)
    def scan_store_mode(self, mode):
        self._ck(self.lib.shim_scan_store_mode(self.h, mode))

    @staticmethod
    def _factors(factors):
        return (_arr(_P, [f[0] for f in factors]), _arr(_I64, [f[1] for f in factors]),
                _arr(_I64, [f[2] for f in factors]), len(factors))

    def scan_contract(self, V, dt, L, J, T, factors, R, out, out_dt, ts, rs, pad=(0, 0)):
        self._ck(self.lib.shim_scan_contract(self.h, V, dt, L, J, T, *self._factors(factors), R, out, out_dt, ts, rs,
                                             pad[0], pad[1]))

    def mttv(self, X, xdt, L, J, T, factors, R, out, rs, accumulate, out_scale):
        self._ck(self.lib.shim_mttv(self.h, X, xdt, L, J, T, *self._factors(factors), R, out, rs, accumulate,
                                    out_scale))

    def ttm_keep(self, X, dt, L, J, T, W, ldw, Kc, out):
        self._ck(self.lib.shim_ttm_keep(self.h, X, dt, L, J, T, W, ldw, Kc, out))

    def ttm_lead_front(self, X, dt, J, S, T, W, ldw, Kc, out):
        taken = _I(0)
        self._ck(self.lib.shim_ttm_lead_front(self.h, X, dt, J, S, T, W, ldw, Kc, out, C.byref(taken)))
        return bool(taken.value)

    def pp_correct(self, M0, rows, R, terms, M):
        """terms: list of (T pointer, ny, keep_first, dW pointer, lddw)"""
        self._ck(self.lib.shim_pp_correct(self.h, M0, rows, R, _arr(_P, [t[0] for t in terms]),
                                          _arr(_I64, [t[1] for t in terms]), _arr(_I, [t[2] for t in terms]),
                                          _arr(_P, [t[3] for t in terms]), _arr(_I64, [t[4] for t in terms]),
                                          len(terms), M))

    def arm_gram_system(self, Gall, N, mode, R, lam, S, Sinv):
        self._ck(self.lib.shim_arm_gram_system(self.h, Gall, N, mode, R, lam, S, Sinv))

    # ---- the mode-update, Normalize and factor-side ops (0 / None: a null pointer)
    def gram(self, W, rows, ld, R, G):
        self._ck(self.lib.shim_gram(self.h, W, rows, ld, R, G))

    def gram_batched(self, W, rows, ld, R, nstarts, G, gstride):
        self._ck(self.lib.shim_gram_batched(self.h, W, rows, ld, R, nstarts, G, gstride))

    def gram_system(self, Gall, N, mode, R, lam, S, Sinv):
        self._ck(self.lib.shim_gram_system(self.h, Gall, N, mode, R, lam, S, Sinv))

    def cp_update(self, M, ldm, Wold, ldw, Wnew, ldn, grad, ldg, rows, R, S, Sinv, gradsq, Winit, ldi, dW, ldd,
                  ratio):
        self._ck(self.lib.shim_cp_update(self.h, M, ldm, Wold, ldw, Wnew, ldn, grad, ldg, rows, R, S, Sinv, gradsq,
                                         Winit, ldi, dW, ldd, ratio))

    def cp_mode_update(self, Gall, N, mode, R, lam, M, ldm, W, ldw, grad, ldg, rows, gradsq, Winit, ldi, dW, ldd,
                       ratio, S, Sinv, dwsq):
        self._ck(self.lib.shim_cp_mode_update(self.h, Gall, N, mode, R, lam, M, ldm, W, ldw, grad, ldg, rows, gradsq,
                                              Winit, ldi, dW, ldd, ratio, S, Sinv, dwsq))

    def cp_mode_update_batched(self, Gall, N, mode, R, nstarts, lam, M, ldm, W, ldw, grad, ldg, rows, gradsq, S,
                               Sinv):
        self._ck(self.lib.shim_cp_mode_update_batched(self.h, Gall, N, mode, R, nstarts, lam, M, ldm, W, ldw, grad,
                                                      ldg, rows, gradsq, S, Sinv))

    def cp_mode_update_blocked(self, Gall, N, mode, R, lam, Mblk, blk, P, scratch, W, ldw, grad, ldg, rows, gradsq,
                               Winit, ldi, dW, ldd, ratio, S, Sinv):
        self._ck(self.lib.shim_cp_mode_update_blocked(self.h, Gall, N, mode, R, lam, Mblk, blk, P, scratch, W, ldw,
                                                      grad, ldg, rows, gradsq, Winit, ldi, dW, ldd, ratio, S, Sinv))

    @staticmethod
    def _masks(masks):
        return _arr(_U, list(masks) + [0] * (32 - len(masks))) if masks is not None else None

    def arm_normalize(self, W, rows, R, Gall, mode, wsq, ms_dst=None, masks=None, active=0, fresh=0):
        taken = _I(0)
        self._ck(self.lib.shim_arm_normalize(self.h, _arr(_P, W), _arr(_I64, rows), len(W), R, Gall, mode, wsq,
                                             ms_dst, self._masks(masks), active, fresh, C.byref(taken)))
        return bool(taken.value)

    def normalize(self, W, rows, R, Gall):
        self._ck(self.lib.shim_normalize(self.h, _arr(_P, W), _arr(_I64, rows), len(W), R, Gall))

    def normalize_ms(self, W, rows, R, Gall, ms_dst, masks, active, fresh, wsq):
        self._ck(self.lib.shim_normalize_ms(self.h, _arr(_P, W), _arr(_I64, rows), len(W), R, Gall, ms_dst,
                                            self._masks(masks), active, fresh, wsq))

    def normalize_scales(self):
        p = _P()
        self._ck(self.lib.shim_normalize_scales(self.h, C.byref(p)))
        return p.value

    def diff_norms(self, A, B, n, store_diff, D, update_prev, out):
        """A, B, D: lists of device pointers (B, D may be None: a null array; an entry may be 0)"""
        arr = lambda v: _arr(_P, v) if v is not None else None
        self._ck(self.lib.shim_diff_norms(self.h, arr(A), arr(B), _arr(_I64, n), len(A), store_diff, arr(D),
                                          update_prev, out))

    def pack_blocks(self, nat, rows, ld, R, blk, P, blocked):
        self._ck(self.lib.shim_pack_blocks(self.h, nat, rows, ld, R, blk, P, blocked))

    def unpack_blocks(self, blocked, rows, ld, R, blk, P, nat):
        self._ck(self.lib.shim_unpack_blocks(self.h, blocked, rows, ld, R, blk, P, nat))

    def sumsq(self, x, n, out):
        self._ck(self.lib.shim_sumsq(self.h, x, n, out))

    def scale_update(self, dst, scales, mask, set_one):
        self._ck(self.lib.shim_scale_update(self.h, dst, scales, mask, set_one))

    def scale_update_many(self, dst, scales, masks, active, fresh):
        self._ck(self.lib.shim_scale_update_many(self.h, dst, scales, self._masks(masks), active, fresh))

    # ---- the Tucker eigen side and the low-rank factor ops (tests/tucker_ops_cases.py)
    def d2d(self, dst, src, nbytes):
        self._ck(self.lib.shim_d2d(self.h, dst, src, nbytes))

    def unfold_gram(self, X, dt, L, J, T, G):
        self._ck(self.lib.shim_unfold_gram(self.h, X, dt, L, J, T, G))

    def top_eigvecs(self, G, J, rank, U):
        self._ck(self.lib.shim_top_eigvecs(self.h, G, J, rank, U))

    def top_eigvecs_warm(self, G, J, rank, U, slot):
        self._ck(self.lib.shim_top_eigvecs_warm(self.h, G, J, rank, U, slot))

    def eig_lazy(self, slot, on):
        self._ck(self.lib.shim_eig_lazy(self.h, slot, int(on)))

    def eig_defer(self, slot, on):
        self._ck(self.lib.shim_eig_defer(self.h, slot, int(on)))

    def _int_out(self, f, *args):
        v = _I(0)
        self._ck(f(self.h, *args, C.byref(v)))
        return v.value

    def _ptr_out(self, f, *args):
        p = _P()
        self._ck(f(self.h, *args, C.byref(p)))
        return p.value

    def eig_gram(self, slot, J):
        return self._ptr_out(self.lib.shim_eig_gram, slot, J)

    def eig_deferred(self, slot):
        return bool(self._int_out(self.lib.shim_eig_deferred, slot))

    def eig_verify(self, slot, discard=False):
        return self._int_out(self.lib.shim_eig_verify, slot, int(discard))

    def eig_pending_rotation(self, slot):
        return self._ptr_out(self.lib.shim_eig_pending_rotation, slot)

    def eig_rotation_done(self, slot):
        self._ck(self.lib.shim_eig_rotation_done(self.h, slot))

    def eig_session_new(self):
        return self._int_out(self.lib.shim_eig_session_new)

    def eig_session_free(self, base):
        self._ck(self.lib.shim_eig_session_free(self.h, base))

    def orthonormalize(self, U, rows, r):
        return bool(self._int_out(self.lib.shim_orthonormalize, U, rows, r))

    def sign_align(self, W, Wref, rows, r):
        self._ck(self.lib.shim_sign_align(self.h, W, Wref, rows, r))

    def rows_times_small(self, A, rows, K, B, Cc, D, out):
        self._ck(self.lib.shim_rows_times_small(self.h, A, rows, K, B, Cc, D, out))

    def lowrank_accumulate(self, X, xdt, n, R, T, r, VT):
        self._ck(self.lib.shim_lowrank_accumulate(self.h, X, xdt, n, R, T, r, VT))

    def add_inplace(self, dst, src, n):
        self._ck(self.lib.shim_add_inplace(self.h, dst, src, n))

    def transpose2d(self, src, dt, rows, cols, dst):
        self._ck(self.lib.shim_transpose2d(self.h, src, dt, rows, cols, dst))

    def transpose_batched(self, src, dt, rows, cols, batch, dst):
        self._ck(self.lib.shim_transpose_batched(self.h, src, dt, rows, cols, batch, dst))

    # ---- the tensor streams: generation, residual, layouts and shards (tests/stream_cases.py)
    def fill_uniform(self, V, dt, l0, g0, row0, rest, seed, lo, hi):
        self._ck(self.lib.shim_fill_uniform(self.h, V, dt, l0, g0, row0, rest, seed, lo, hi))

    def fill_laplacian(self, V, dt, l0, g0, row0, rest, ndigits, s):
        self._ck(self.lib.shim_fill_laplacian(self.h, V, dt, l0, g0, row0, rest, ndigits, s))

    def add_uniform_noise(self, V, dt, l0, g0, row0, rest, seed, lo, hi, alpha):
        self._ck(self.lib.shim_add_uniform_noise(self.h, V, dt, l0, g0, row0, rest, seed, lo, hi, alpha))

    def uniform_sumsq(self, l0, g0, row0, rest, seed, lo, hi, out):
        self._ck(self.lib.shim_uniform_sumsq(self.h, l0, g0, row0, rest, seed, lo, hi, out))

    def fill_rank(self, V, dt, M, K, Q, P, R):
        self._ck(self.lib.shim_fill_rank(self.h, V, dt, M, K, Q, P, R))

    def residual_sq(self, V, dt, M, K, Q, P, R, out):
        self._ck(self.lib.shim_residual_sq(self.h, V, dt, M, K, Q, P, R, out))

    def upload_shard(self, V, dt, host_full, l0, g0, row0, rest):
        """host_full: a contiguous float64 numpy array, the full tensor"""
        assert host_full.dtype == np.float64 and host_full.flags.c_contiguous and host_full.size == g0 * rest
        self._ck(self.lib.shim_upload_shard(self.h, V, dt, host_full.ctypes.data, l0, g0, row0, rest))

    def download_shard(self, V, dt, host_full, l0, g0, row0, rest):
        assert host_full.dtype == np.float64 and host_full.flags.c_contiguous and host_full.size == g0 * rest
        self._ck(self.lib.shim_download_shard(self.h, V, dt, host_full.ctypes.data, l0, g0, row0, rest))

    def pad_layout(self, src, dt, rows, cols, blk, ld, dst):
        self._ck(self.lib.shim_pad_layout(self.h, src, dt, rows, cols, blk, ld, dst))

    def unpack_shards(self, stage, dt, s0, rest, blk, P, chunk_bytes, full):
        self._ck(self.lib.shim_unpack_shards(self.h, stage, dt, s0, rest, blk, P, chunk_bytes, full))

    def krp(self, out, factors, col0, ncols):
        self._ck(self.lib.shim_krp(self.h, out, *self._factors(factors), col0, ncols))

    # ---- the multi-start, constraint and diagnostic ops (tests/multistart_ops_cases.py)
    # table: (nstarts, col, sq), handed on as given; side: (list of pointers, list of ld, list of rows, cols)
    @staticmethod
    def _table(t):
        return t[0], _arr(_I, list(t[1])), _arr(_I, list(t[2]))

    def cp_mode_update_ragged(self, Gall, N, mode, t, lam, M, ldm, W, ldw, grad, ldg, rows, gradsq, S, Sinv):
        self._ck(self.lib.shim_cp_mode_update_ragged(self.h, Gall, N, mode, *self._table(t), lam, M, ldm, W, ldw, grad,
                                                     ldg, rows, gradsq, S, Sinv))

    def gram_ragged(self, W, rows, ld, t, N, mode, Gall):
        self._ck(self.lib.shim_gram_ragged(self.h, W, rows, ld, *self._table(t), N, mode, Gall))

    def cp_mode_update_nn(self, Gall, N, mode, R, lam, M, ldm, W, ldw, grad, ldg, rows, gradsq, S):
        self._ck(self.lib.shim_cp_mode_update_nn(self.h, Gall, N, mode, R, lam, M, ldm, W, ldw, grad, ldg, rows,
                                                 gradsq, S))

    def cp_mode_update_nn_batched(self, Gall, N, mode, R, nstarts, lam, M, ldm, W, ldw, grad, ldg, rows, gradsq, S):
        self._ck(self.lib.shim_cp_mode_update_nn_batched(self.h, Gall, N, mode, R, nstarts, lam, M, ldm, W, ldw, grad,
                                                         ldg, rows, gradsq, S))

    def cp_mode_update_nn_ragged(self, Gall, N, mode, t, lam, M, ldm, W, ldw, grad, ldg, rows, gradsq, S):
        self._ck(self.lib.shim_cp_mode_update_nn_ragged(self.h, Gall, N, mode, *self._table(t), lam, M, ldm, W, ldw,
                                                        grad, ldg, rows, gradsq, S))

    def cp_hold_rows(self, W, ldw, grad, ldg, scores, lds, rows, t, keep, holds, Gall, N, mode, gradsq):
        self._ck(self.lib.shim_cp_hold_rows(self.h, W, ldw, grad, ldg, scores, lds, rows, *self._table(t), keep, holds,
                                            Gall, N, mode, gradsq))

    def cp_pinv_ragged(self, Gall, N, t, W, rows, P, bad):
        self._ck(self.lib.shim_cp_pinv_ragged(self.h, Gall, N, *self._table(t), _arr(_P, W), _arr(_I64, rows),
                                              _arr(_P, P), bad))

    def core_score(self, core, R, N, bad, cc):
        self._ck(self.lib.shim_core_score(self.h, core, R, N, bad, cc))

    @staticmethod
    def _side(s):
        return _arr(_P, s[0]), _arr(_I64, s[1]), _arr(_I64, s[2]), s[3]

    def factor_congruence_work(self, N, a, b):
        n = _I64(0)
        self._ck(self.lib.shim_factor_congruence_work(self.h, N, *self._side(a), *self._side(b), C.byref(n)))
        return n.value

    def factor_congruence(self, N, a, b, mask, work, Phi, wa, wb):
        self._ck(self.lib.shim_factor_congruence(self.h, N, *self._side(a), *self._side(b), mask, work, Phi, wa, wb))

    def row_dots(self, P, W, rows, R, ld, out):
        self._ck(self.lib.shim_row_dots(self.h, P, W, rows, R, ld, out))

    def fold_slice_sums(self, src, lens, out):
        self._ck(self.lib.shim_fold_slice_sums(self.h, src, _arr(_I64, list(lens)), len(lens), out))


def compute_units():
    """The compute-unit count of the first GPU in the KFD topology (what the launchers' device-dependent
    rules see as multiProcessorCount), or None where there is no such node."""
    for path in sorted(glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties")):
        try:
            with open(path) as f:
                props = dict(line.split()[:2] for line in f if len(line.split()) >= 2)
            simd, per = int(props.get("simd_count", 0)), int(props.get("simd_per_cu", 0))
        except (OSError, ValueError):
            continue
        if simd > 0 and per > 0:
            return simd // per
    return None
