"""spmv_amd — Python host mirror of the MI355X SpMV suite's C-ABI.

The product is C/HIP: ``lib/libspmv_hip.so`` (gfx950 kernels behind the
``extern "C"`` entry points of ``include/spmv.h``) and ``lib/libspmv_host.so``
(Matrix Market reader, format builders, generators, CPU loops; declared in
``include/spmv_host.h``).  This module binds both with ctypes so tests and
``bench.py`` drive exactly the calls the C drivers make.  PyTorch is used
only as plumbing: device memory (CUDA tensors on ROCm), the current HIP
stream and ``torch.distributed``.

There is no fallback: if ``libspmv_hip.so`` is missing or a HIP call fails,
``SpmvError`` is raised.  The five formats mirror the reference's five
programs (reference coo.c, csr.c, ell.c, sigma_c.c, cmrs.c) and kernels
(reference kernels/{Coo,Csr,Ell,Sigma_C,Cmrs}.cl).
"""
from __future__ import annotations

import ctypes
import os
import sys
from dataclasses import dataclass, field
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
LIB_DIR = PKG_DIR / "lib"
REPO_DIR = PKG_DIR.parent

FORMATS = ("coo", "csr", "ell", "sell", "cmrs")  # the reference's five
# §8f row 4: CSR with 16-bit column offsets; ELL + COO tail; CSR with fp32 values;
# SELL-C-σ with 16-bit column offsets; column-grouped CSR (gather-bound rows)
EXTRA_FORMATS = ("csr16", "hyb", "csrf32", "sell16", "csrg")
ALL_FORMATS = FORMATS + EXTRA_FORMATS
# block formats: their own tuple, so the per-format sweeps over ALL_FORMATS stay what they were
BLOCK_FORMATS = ("bsr",)
HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)

# The reference's ReturnCode values (reference inc/enums.h:4-11).
SUCCESS, DEVICE_ERROR, PROGRAM_ERROR, FILE_ERROR, OTHER_ERROR = range(5)


class SpmvError(RuntimeError):
    """A C-ABI call returned a non-zero spmv_rc code."""

    def __init__(self, rc: int, what: str, detail: str = ""):
        super().__init__(f"{what} failed: rc={rc} {detail}".strip())
        self.rc = rc


# --------------------------------------------------------------- loading
_c_i64 = ctypes.c_int64
_c_i32 = ctypes.c_int32
_vp = ctypes.c_void_p


class Dims(ctypes.Structure):
    """``spmv_dims`` (include/spmv.h)."""

    _fields_ = [
        ("n_rows", _c_i64),
        ("n_cols", _c_i64),
        ("nnz", _c_i64),
        ("device", ctypes.c_int),
        ("stream", _vp),
    ]


class MtxInfo(ctypes.Structure):
    """``spmv_mtx_info`` (include/spmv_host.h)."""

    _fields_ = [
        ("n_rows", _c_i64),
        ("n_cols", _c_i64),
        ("nnz", _c_i64),
        ("symmetric", ctypes.c_int),
        ("pattern", ctypes.c_int),
        ("integer", ctypes.c_int),
    ]


class PlanOpts(ctypes.Structure):
    """``spmv_plan_opts`` (include/spmv.h)."""

    _fields_ = [
        ("lanes", _c_i32),
        ("variant", _c_i32),
        ("xwin", _c_i32),
        ("xwin_rows", _c_i32),
        ("head", _c_i32),
        ("index16", _c_i32),
        ("coo_pass", _c_i32),
        ("split", _c_i32),
        ("bigplan", _c_i32),
        ("reserved", _c_i32),
        ("H", _c_i64),
    ]


class PlanInfo(ctypes.Structure):
    """``spmv_plan_info`` (include/spmv.h)."""

    _fields_ = [(k, _c_i32) for k in ("format", "path", "lanes", "variant", "ki", "xcap", "xwin", "head", "single_pass",
                                      "index16", "split_T", "reserved")] + \
               [(k, _c_i64) for k in ("n_chunks", "big_tiles", "head_bytes", "ws_bytes", "owned_bytes", "H")] + \
               [("kernel", ctypes.c_char * 64), ("desc", ctypes.c_char * 320)]


class TransposeInfo(ctypes.Structure):
    """``spmv_transpose_info`` (include/spmv.h)."""

    _fields_ = [("mode", _c_i32), ("cap", _c_i32)] + \
               [(k, _c_i64) for k in ("blocks", "lds_blocks", "flush_entries", "owned_bytes")] + \
               [("kernel", ctypes.c_char * 64)]


class TransposeMultiInfo(ctypes.Structure):
    """``spmv_transpose_multi_info`` (include/spmv.h)."""

    _fields_ = [("mode", _c_i32), ("reserved", _c_i32), ("cap_cols", _c_i32 * 4), ("lds_blocks", _c_i64 * 4),
                ("kernel", ctypes.c_char * 64)]


TRANSPOSE_MODES = {None: 0, "scatter": 1, "copy": 2}  # enum spmv_transpose_mode
_TRANSPOSE_MODE_NAMES = {v: k for k, v in TRANSPOSE_MODES.items()}


class SymmetricInfo(ctypes.Structure):
    """``spmv_symmetric_info`` (include/spmv.h)."""

    _fields_ = [("mode", _c_i32), ("cap", _c_i32)] + \
               [(k, _c_i64) for k in ("blocks", "window_blocks", "flush_entries", "nnz_expanded", "owned_bytes")] + \
               [("kernel", ctypes.c_char * 64)]


SYMMETRIC_MODES = {None: 0, "fused": 1, "expand": 2}  # enum spmv_symmetric_mode
_SYMMETRIC_MODE_NAMES = {v: k for k, v in SYMMETRIC_MODES.items()}


class SymmetricMultiInfo(ctypes.Structure):
    """``spmv_symmetric_multi_info`` (include/spmv.h)."""

    _fields_ = [("mode", _c_i32), ("reserved", _c_i32), ("cap_cols", _c_i32 * 4), ("window_blocks", _c_i64 * 4),
                ("flush_entries", _c_i64 * 4), ("long_rows", _c_i64), ("segments", _c_i64),
                ("multi_owned_bytes", _c_i64), ("kernel", ctypes.c_char * 64)]


class MultiOpts(ctypes.Structure):
    """``spmv_multi_opts`` (include/spmv.h); -1 = the library's rule."""

    _fields_ = [("long_len", _c_i32), ("seg_len", _c_i32)]


class MultiInfo(ctypes.Structure):
    """``spmv_multi_info`` (include/spmv.h)."""

    _fields_ = [(k, _c_i32) for k in ("mode", "long_len", "seg_len", "reserved")] + \
               [(k, _c_i64) for k in ("long_rows", "segments", "slots", "long_entries", "owned_bytes", "t_long_rows",
                                      "t_segments", "t_owned_bytes")] + \
               [("kernel", ctypes.c_char * 64)]


MULTI_MODES = {None: 0, "balanced": 1}  # enum spmv_multi_mode
_MULTI_MODE_NAMES = {v: k for k, v in MULTI_MODES.items()}


class BjacobiInfo(ctypes.Structure):
    """``spmv_bjacobi_info`` (include/spmv_ext.h)."""

    _fields_ = [("bs", _c_i32), ("symmetric_half", _c_i32)] + \
               [(k, _c_i64) for k in ("n", "n_blocks", "singular_blocks", "col_base", "owned_bytes")] + \
               [("kernel", ctypes.c_char * 64)]


_PP = ctypes.POINTER(_vp)
_PO = ctypes.POINTER(PlanOpts)

# name -> (restype, argtypes)
HIP_SYMBOLS = {
    "spmv_plan_opts_init": (None, [_PO]),
    "spmv_plan_coo": (ctypes.c_int, [Dims, _vp, _vp, _vp, _PO, _PP]),
    "spmv_plan_csr": (ctypes.c_int, [Dims, _vp, _vp, _vp, _PO, _PP]),
    "spmv_plan_ell": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, _PO, _PP]),
    "spmv_plan_sell": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _PO, _PP]),
    "spmv_plan_cmrs": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _PO, _PP]),
    "spmv_bsr_auto_lanes": (ctypes.c_int, [_c_i64, _c_i64]),
    "spmv_plan_bsr": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _PO, _PP]),
    "spmv_bsr_run": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_plan_run": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_plan_run_multi": (ctypes.c_int, [_vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp]),
    "spmv_plan_multi_supported": (ctypes.c_int, [_vp]),
    "spmv_multi_opts_init": (None, [ctypes.POINTER(MultiOpts)]),
    "spmv_plan_prepare_multi": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(MultiOpts)]),
    "spmv_plan_get_multi_info": (ctypes.c_int, [_vp, ctypes.POINTER(MultiInfo)]),
    "spmv_plan_transpose_supported": (ctypes.c_int, [_vp]),
    "spmv_plan_prepare_transpose": (ctypes.c_int, [_vp, ctypes.c_int]),
    "spmv_plan_get_transpose_info": (ctypes.c_int, [_vp, ctypes.POINTER(TransposeInfo)]),
    "spmv_plan_run_t": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_plan_run_t_multi": (ctypes.c_int, [_vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp]),
    "spmv_plan_get_transpose_multi_info": (ctypes.c_int, [_vp, ctypes.POINTER(TransposeMultiInfo)]),
    "spmv_plan_symmetric_supported": (ctypes.c_int, [_vp]),
    "spmv_plan_prepare_symmetric": (ctypes.c_int, [_vp, ctypes.c_int]),
    "spmv_plan_get_symmetric_info": (ctypes.c_int, [_vp, ctypes.POINTER(SymmetricInfo)]),
    "spmv_plan_run_sym": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "spmv_plan_get_symmetric_arrays": (ctypes.c_int, [_vp, _PP, _PP, _PP, ctypes.POINTER(_c_i64)]),
    "spmv_plan_run_sym_multi": (ctypes.c_int, [_vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp]),
    "spmv_plan_get_symmetric_multi_info": (ctypes.c_int, [_vp, ctypes.POINTER(SymmetricMultiInfo)]),
    "spmv_plan_get_info": (ctypes.c_int, [_vp, ctypes.POINTER(PlanInfo)]),
    "spmv_plan_destroy": (ctypes.c_int, [_vp]),
    "spmv_set_option": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
    "spmv_get_option": (ctypes.c_int, [ctypes.c_int]),
    "spmv_coo_ws_bytes": (ctypes.c_size_t, [_c_i64]),
    "spmv_coo_run": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t]),
    "spmv_coo_tail_bytes": (ctypes.c_size_t, [_c_i64]),
    "spmv_coo_tail_build": (ctypes.c_int, [Dims, _vp, _vp, ctypes.c_size_t]),
    "spmv_coo_run_tail": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_csr_auto_lanes": (ctypes.c_int, [_c_i64, _c_i64]),
    "spmv_csr_run": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_csr_run_variant": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int]),
    "spmv_csr_tiled_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "spmv_csr_run_tiled": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t]),
    "spmv_csr_hot_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i64, _c_i64]),
    "spmv_csr_f32v_run_xwin": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _c_i32, _vp, _c_i32]),
    "spmv_csr_f32v_run_tiled_hot": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp,
                                                   ctypes.c_size_t]),
    "spmv_csr_run_tiled_hot": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp,
                                              ctypes.c_size_t]),
    "spmv_csr_tiled_plan_len": (_c_i64, [_c_i64]),
    "spmv_csr_tiled_plan": (ctypes.c_int, [Dims, _vp, _vp]),
    "spmv_csr_tiled_tile": (_c_i64, [_c_i64, _c_i64]),
    "spmv_csr_run_tiled_plan": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, _vp, _c_i64,
                                               _c_i64, _vp, ctypes.c_size_t]),
    "spmv_csrg_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "spmv_csrg_run": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     ctypes.c_size_t]),
    "spmv_csr16_run": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_csr16_run_xwin": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _c_i32, _vp,
                                           _c_i32]),
    "spmv_hyb_ws_bytes": (ctypes.c_size_t, [_c_i64]),
    "spmv_hyb_run": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                    ctypes.c_size_t]),
    "spmv_hyb_run_tail": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp,
                                         _vp]),
    "spmv_hyb_run_tail_xwin": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp, _c_i32]),
    "spmv_csr_xwin_bytes": (ctypes.c_size_t, [_c_i64, _c_i64, ctypes.c_int, _c_i32]),
    "spmv_csr_xwin_build": (ctypes.c_int, [Dims, _vp, _vp, ctypes.c_int, _c_i32, _vp, ctypes.c_size_t,
                                           ctypes.POINTER(_c_i32)]),
    "spmv_csr_run_xwin": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, _c_i32, _vp, _c_i32]),
    "spmv_ell_run": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, _vp, _vp]),
    "spmv_ell_xwin_bytes": (ctypes.c_size_t, [_c_i64]),
    "spmv_ell_xwin_build": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, ctypes.c_size_t,
                                           ctypes.POINTER(_c_i32)]),
    "spmv_ell_run_xwin": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, _vp, _vp, _vp, _c_i32]),
    "spmv_sell_xwin_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i32]),
    "spmv_sell_auto_ki": (ctypes.c_int, [_c_i64, _c_i32]),
    "spmv_sell_xwin_build": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, ctypes.c_size_t,
                                            ctypes.POINTER(_c_i32)]),
    "spmv_sell_run_xwin": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                          _vp, _c_i32]),
    "spmv_sell_run": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_sell16_fill": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp]),
    "spmv_sell16_run": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _c_i32, _vp]),
    "spmv_sell16_head_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i32]),
    "spmv_sell_head_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i32]),
    "spmv_sell_head_fill": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp,
                                           ctypes.c_size_t]),
    "spmv_sell_run_xwin_head": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp,
                                               _vp, _c_i32, _vp]),
    "spmv_sell16_head_fill": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp,
                                             ctypes.c_size_t]),
    "spmv_cmrs_run": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_coo_xwin_bytes": (ctypes.c_size_t, [_c_i64]),
    "spmv_coo_xwin_build": (ctypes.c_int, [Dims, _vp, _vp, ctypes.c_size_t, ctypes.POINTER(_c_i32)]),
    "spmv_coo_run_xwin": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t, _vp, _c_i32]),
    "spmv_cmrs_xwin_bytes": (ctypes.c_size_t, [Dims, _c_i32, _c_i64]),
    "spmv_cmrs_xwin_build": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, ctypes.c_size_t,
                                            ctypes.POINTER(_c_i32)]),
    "spmv_cmrs_run_xwin": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c_i32]),
    "spmv_coo_hot_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "spmv_coo_run_hot": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp, ctypes.c_size_t]),
    "spmv_cmrs_hot_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i64, _c_i32, _c_i64]),
    "spmv_cmrs_run_tiled_hot": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _vp,
                                               ctypes.c_size_t]),
    "spmv_cmrs_tiled_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i64, _c_i32]),
    "spmv_cmrs_run_tiled": (ctypes.c_int, [Dims, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_size_t]),
    "spmv_sell_split_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "spmv_sell_hot_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i32, _c_i64]),
    "spmv_hyb_hot_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i64]),
    "spmv_hyb_run_hot": (ctypes.c_int, [Dims, _c_i32, _c_i64, _c_i32, _vp, _vp, _c_i64, _vp, _vp, _vp, _vp, _vp,
                                        _c_i64, _vp, _vp, ctypes.c_size_t]),
    "spmv_sell_run_hot": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _c_i32,
                                         _c_i64, _vp, _vp, _c_i64, _vp, _vp, ctypes.c_size_t]),
    "spmv_sell_run_split": (ctypes.c_int, [Dims, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                           _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, ctypes.c_size_t]),
    "spmv_gen_banded_device": (ctypes.c_int, [_c_i64, ctypes.c_uint64, _c_i64, _c_i64, ctypes.c_int, _c_i32,
                                              _c_i32, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "spmv_dev_csr_from_coo": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_dev_csr_transpose": (ctypes.c_int, [Dims, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_dev_ell_plan": (ctypes.c_int, [Dims, _vp, _c_i32, ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i64)]),
    "spmv_dev_ell_fill": (ctypes.c_int, [Dims, _vp, _vp, _vp, _c_i32, _c_i64, _c_i32, _vp, _vp]),
    "spmv_dev_sell_plan": (ctypes.c_int, [Dims, _vp, _vp, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp,
                                          ctypes.POINTER(_c_i64)]),
    "spmv_dev_sell_fill": (ctypes.c_int, [Dims, _vp, _vp, _vp, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp]),
    "spmv_dev_cmrs_build": (ctypes.c_int, [Dims, _vp, _c_i32, _vp, _vp]),
    "spmv_dot_ws_bytes": (ctypes.c_size_t, [_c_i64]),
    "spmv_dot": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "spmv_axpy_ratio": (ctypes.c_int, [_c_i64, _vp, _vp, ctypes.c_double, _vp, _vp, ctypes.c_int, _vp]),
    "spmv_xpay_ratio": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "spmv_scale_rsqrt": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "spmv_dot_multi_ws_bytes": (ctypes.c_size_t, [_c_i64, ctypes.c_int32]),
    "spmv_dot_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _c_i64, _vp, _c_i64, _vp, _vp, ctypes.c_size_t,
                                      ctypes.c_int, _vp]),
    "spmv_axpy_ratio_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _vp, ctypes.c_double, _vp, _c_i64, _vp,
                                             _c_i64, ctypes.c_int, _vp]),
    "spmv_xpay_ratio_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _vp, _vp, _c_i64, _vp, _c_i64,
                                             ctypes.c_int, _vp]),
    "spmv_dot2_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _vp,
                                       ctypes.c_size_t, ctypes.c_int, _vp]),
    "spmv_bicgstab_update_dot_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp,
                                                      _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp,
                                                      _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "spmv_bicgstab_dir_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64,
                                               _vp, _c_i64, ctypes.c_int, _vp]),
    "spmv_gram_multi_ws_bytes": (ctypes.c_size_t, [_c_i64, ctypes.c_int32, ctypes.c_int32]),
    "spmv_gram_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _c_i64, ctypes.c_int32, _vp, _c_i64, _vp, _vp,
                                       ctypes.c_size_t, ctypes.c_int, _vp]),
    "spmv_block_combine_multi": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, ctypes.c_int32, _vp, _c_i64,
                                                ctypes.c_int32, _vp, _c_i64, ctypes.c_int32, _vp, _c_i64, _vp, _c_i64,
                                                ctypes.c_int, _vp]),
    "spmv_krylov_project_dot": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _c_i64, _vp,
                                               _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "spmv_krylov_combine": (ctypes.c_int, [_c_i64, ctypes.c_int32, _vp, _c_i64, _vp, _vp, _c_i64, ctypes.c_int, _vp]),
    "spmv_krylov_normalize": (ctypes.c_int, [_c_i64, _vp, _vp, _c_i64, _vp, _c_i64, _vp, ctypes.c_int, _vp]),
    "spmv_bjacobi_create": (ctypes.c_int, [Dims, _vp, _vp, _vp, _c_i32, _c_i64, _c_i32, _PP]),
    "spmv_bjacobi_get_info": (ctypes.c_int, [_vp, ctypes.POINTER(BjacobiInfo)]),
    "spmv_bjacobi_inverse": (ctypes.c_int, [_vp, _PP]),
    "spmv_bjacobi_apply_multi": (ctypes.c_int, [_vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp]),
    "spmv_bjacobi_ws_bytes": (ctypes.c_size_t, [_c_i64, _c_i32]),
    "spmv_bjacobi_apply_dot_multi": (ctypes.c_int, [_vp, _c_i32, _vp, _c_i64, _vp, _c_i64, _vp, _vp, ctypes.c_size_t,
                                                    _vp]),
    "spmv_bjacobi_cheb_step_multi": (ctypes.c_int, [_vp, _c_i32, ctypes.c_double, ctypes.c_double, _vp, _c_i64, _vp,
                                                    _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp]),
    "spmv_bjacobi_cheb_step_dot_multi": (ctypes.c_int, [_vp, _c_i32, ctypes.c_double, ctypes.c_double, _vp, _c_i64,
                                                        _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _vp,
                                                        ctypes.c_size_t, _vp]),
    "spmv_bjacobi_destroy": (ctypes.c_int, [_vp]),
    "spmv_gather": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, ctypes.c_int, _vp]),
    "spmv_device_count": (ctypes.c_int, [ctypes.POINTER(ctypes.c_int)]),
    "spmv_set_device": (ctypes.c_int, [ctypes.c_int]),
    "spmv_device_name": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "spmv_malloc": (ctypes.c_int, [ctypes.POINTER(_vp), ctypes.c_size_t]),
    "spmv_free": (ctypes.c_int, [_vp]),
    "spmv_memset": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_size_t, _vp]),
    "spmv_upload": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
    "spmv_download": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp]),
    "spmv_stream_create": (ctypes.c_int, [ctypes.POINTER(_vp)]),
    "spmv_stream_destroy": (ctypes.c_int, [_vp]),
    "spmv_sync": (ctypes.c_int, [_vp]),
    "spmv_flush_cache": (ctypes.c_int, [_vp, ctypes.c_size_t]),
    "spmv_flush_cache_read": (ctypes.c_int, [_vp, ctypes.c_size_t]),
    "spmv_event_create": (ctypes.c_int, [ctypes.POINTER(_vp)]),
    "spmv_event_destroy": (ctypes.c_int, [_vp]),
    "spmv_event_record": (ctypes.c_int, [_vp, _vp]),
    "spmv_event_elapsed": (ctypes.c_int, [_vp, _vp, ctypes.POINTER(ctypes.c_double)]),
    "spmv_time_launch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.POINTER(ctypes.c_double)]),
    "spmv_release": (ctypes.c_int, []),
    "spmv_multi_init": (ctypes.c_int, [ctypes.c_int, _vp, _vp]),
    "spmv_multi_free": (ctypes.c_int, [_vp]),
    "spmv_multi_size": (ctypes.c_int, [_vp]),
    "spmv_multi_device": (ctypes.c_int, [_vp, ctypes.c_int]),
    "spmv_multi_stream": (_vp, [_vp, ctypes.c_int]),
    "spmv_multi_allgatherv": (ctypes.c_int, [_vp, _vp, _vp]),
    "spmv_multi_sync": (ctypes.c_int, [_vp]),
    "spmv_multi_time": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_int, _vp]),
    "spmv_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "spmv_last_error": (ctypes.c_char_p, []),
    "spmv_version": (ctypes.c_char_p, []),
}

HOST_SYMBOLS = {
    "spmv_mtx_read_info": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(MtxInfo)]),
    "spmv_mtx_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(MtxInfo), _vp, _vp, _vp]),
    "spmv_mtx_write": (ctypes.c_int, [ctypes.c_char_p, _c_i64, _c_i64, _c_i64, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_bin_write": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(MtxInfo), _vp, _vp, _vp]),
    "spmv_bin_read_info": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(MtxInfo)]),
    "spmv_bin_read": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(MtxInfo), _vp, _vp, _vp]),
    "spmv_coo_sort_by_row": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_csr_from_coo": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_csr_transpose": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "spmv_coo_symmetrize": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, ctypes.POINTER(_c_i64), _vp, _vp, _vp]),
    "spmv_cpu_csr_sym": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _vp, _vp]),
    "spmv_cpu_csr_sym_multi": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _c_i32, _vp, _c_i64, _vp, _c_i64]),
    "spmv_bjacobi_build": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _c_i32, _c_i64, _c_i32, _vp, ctypes.POINTER(_c_i64)]),
    "spmv_cpu_bjacobi_apply_multi": (ctypes.c_int, [_c_i64, _c_i32, _vp, _c_i32, _vp, _c_i64, _vp, _c_i64]),
    "spmv_cpu_bjacobi_cheb_step_multi": (ctypes.c_int, [_c_i64, _c_i32, _vp, _c_i32, ctypes.c_double, ctypes.c_double,
                                                        _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp, _c_i64, _vp,
                                                        _c_i64]),
    "spmv_cpu_bicgstab_update_multi": (ctypes.c_int, [_c_i64, _c_i32, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp,
                                                      _c_i64, _vp, _c_i64, _vp, _c_i64]),
    "spmv_cpu_bicgstab_dir_multi": (ctypes.c_int, [_c_i64, _c_i32, _vp, _vp, _vp, _vp, _vp, _c_i64, _vp, _c_i64, _vp,
                                                   _c_i64]),
    "spmv_cpu_block_combine_multi": (ctypes.c_int, [_c_i64, _c_i32, _vp, _c_i32, _vp, _c_i64, _c_i32, _vp, _c_i64,
                                                    _c_i32, _vp, _c_i64, _vp, _c_i64]),
    "spmv_cpu_krylov_project": (ctypes.c_int, [_c_i64, _c_i32, _vp, _c_i64, _vp, _vp, _c_i64, _vp, _c_i64]),
    "spmv_cpu_krylov_combine": (ctypes.c_int, [_c_i64, _c_i32, _vp, _c_i64, _vp, _vp, _c_i64]),
    "spmv_cpu_krylov_normalize": (ctypes.c_int, [_c_i64, _vp, _vp, _c_i64, _vp, _c_i64, _vp]),
    "spmv_csr_sort_rows": (ctypes.c_int, [_c_i64, _vp, _vp, _vp]),
    "spmv_csr_row_stats": (ctypes.c_int, [_c_i64, _vp, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), ctypes.POINTER(ctypes.c_double)]),
    "spmv_csr_pick_variant": (ctypes.c_int, [_c_i64, _vp]),
    "spmv_csr_variant_rule": (ctypes.c_int, [_c_i64, _c_i64, _c_i64]),
    "spmv_cmrs_variant_rule": (ctypes.c_int, [_c_i64, _c_i64, _c_i64]),
    "spmv_hot_columns_possible": (ctypes.c_int, [_c_i64, _c_i64]),
    "spmv_hot_columns": (_c_i64, [_c_i64, _c_i64, _vp, _c_i64, _vp, _vp]),
    "spmv_column_relabel": (_c_i64, [_c_i64, _c_i64, _vp, _vp, _vp, _vp]),
    "spmv_column_relabel_ex": (_c_i64, [_c_i64, _c_i64, _vp, _vp, _vp, _vp, _c_i32]),
    "spmv_csr_tiled_bigplan": (_c_i64, [_c_i64, _vp, _c_i64, _c_i32, _vp]),
    "spmv_csr_multi_plan": (ctypes.c_int, [_c_i64, _vp, _c_i32, _c_i32, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64),
                                           ctypes.POINTER(_c_i64), _vp, _vp, _vp, _vp, _vp]),
    "spmv_ell_plan": (ctypes.c_int, [_c_i64, _vp, _c_i32, ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i64)]),
    "spmv_ell_fill": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _c_i32, _c_i64, _c_i32, _vp, _vp]),
    "spmv_sell_plan": (ctypes.c_int, [_c_i64, _vp, _c_i32, _c_i32, _c_i32, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "spmv_sell_fill": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _c_i32, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp]),
    "spmv_cmrs_build": (ctypes.c_int, [_c_i64, _vp, _c_i32, _vp, _vp]),
    "spmv_cmrs_pick_variant": (ctypes.c_int, [_c_i64, _vp]),
    "spmv_sell_split_auto": (_c_i32, [_c_i64, _vp, _c_i32, _c_i32]),
    "spmv_sell_split_plan": (_c_i64, [_c_i64, _vp, _c_i32, _c_i32, _vp, _vp]),
    "spmv_partition_rows": (ctypes.c_int, [_c_i64, _vp, ctypes.c_int, _c_i64, _vp]),
    "spmv_coo_row_shard": (_c_i64, [_c_i64, _vp, _vp, _vp, _c_i64, _c_i64, _vp, _vp, _vp]),
    "spmv_partition_rows_weighted": (ctypes.c_int, [_c_i64, _vp, ctypes.c_int, _c_i64, ctypes.c_double, _vp]),
    "spmv_partition_rows_calibrated": (ctypes.c_int, [_c_i64, _vp, ctypes.c_int, _c_i64, ctypes.c_double, ctypes.c_int,
                                                      _vp, _vp, _vp]),
    "spmv_csr16_plan": (ctypes.c_int, [_c_i64, _vp, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "spmv_hyb_plan": (ctypes.c_int, [_c_i64, _vp, _c_i32, _c_i32, ctypes.POINTER(_c_i32), ctypes.POINTER(_c_i64),
                                     ctypes.POINTER(_c_i64)]),
    "spmv_hyb_fill": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _c_i32, _c_i64, _c_i32, _vp, _vp, _vp, _vp, _vp]),
    "spmv_csr16_fill": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _vp]),
    "spmv_csrg_group": (_c_i32, [_c_i32, _c_i32]),
    "spmv_csrg_block_rows": (_c_i32, []),
    "spmv_csrg_plan": (ctypes.c_int, [_c_i64, _vp, _vp, _c_i32, ctypes.POINTER(_c_i64)]),
    "spmv_csrg_fill": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _c_i32, _vp, _vp, _vp, _vp, _vp]),
    "spmv_bsr_plan": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _c_i32, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64)]),
    "spmv_bsr_fill": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _c_i32, _vp, _vp, _vp]),
    "spmv_cpu_bsr": (ctypes.c_int, [_c_i64, _c_i64, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp]),
    "spmv_cpu_coo": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_cpu_csr": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_cpu_csr_multi": (ctypes.c_int, [_c_i64, _vp, _vp, _vp, _c_i32, _vp, _c_i64, _vp, _c_i64]),
    "spmv_cpu_csr_t": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp]),
    "spmv_cpu_csr_t_multi": (ctypes.c_int, [_c_i64, _c_i64, _vp, _vp, _vp, _c_i32, _vp, _c_i64, _vp, _c_i64]),
    "spmv_cpu_ell": (ctypes.c_int, [_c_i64, _c_i32, _c_i64, _c_i32, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_cpu_sell": (ctypes.c_int, [_c_i64, _c_i32, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_cpu_cmrs": (ctypes.c_int, [_c_i64, _c_i32, _c_i64, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    "spmv_cpu_threads": (ctypes.c_int, []),
    "spmv_check": (_c_i64, [_c_i64, _c_i64, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, ctypes.c_double, ctypes.POINTER(_c_i64), ctypes.POINTER(ctypes.c_double)]),
    "spmv_gen_cantlike": (ctypes.c_int, [ctypes.c_int, _c_i64, ctypes.POINTER(_c_i64), ctypes.POINTER(_c_i64), _vp, _vp, _vp]),
    "spmv_gen_rmat": (ctypes.c_int, [_c_i64, _c_i64, ctypes.c_int, ctypes.c_uint64, _vp, _vp, _vp]),
    "spmv_gen_banded_csr": (ctypes.c_int, [_c_i64, ctypes.c_uint64, _c_i64, _c_i64, _vp, _vp, _vp]),
    "spmv_gen_random": (ctypes.c_int, [_c_i64, _c_i64, _c_i64, _c_i64, ctypes.c_uint64, ctypes.POINTER(_c_i64), _vp, _vp, _vp]),
    "spmv_splitmix64": (ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]),
}

_LAUNCH_FN = ctypes.CFUNCTYPE(ctypes.c_int, _vp)

_hip = None
_host = None


def _bind(lib: ctypes.CDLL, table: dict) -> ctypes.CDLL:
    for name, (res, args) in table.items():
        fn = getattr(lib, name)  # AttributeError = symbol missing: loud
        fn.restype = res
        fn.argtypes = args
    return lib


def hip_lib() -> ctypes.CDLL:
    """libspmv_hip.so — raises if it was not built (no CPU fallback)."""
    global _hip
    if _hip is None:
        host_lib()  # its plans call the host rules: loaded first (RTLD_GLOBAL, soname libspmv_host.so)
        path = Path(os.environ.get("SPMV_HIP_LIB") or LIB_DIR / "libspmv_hip.so")  # override: A/B runs
        if not path.exists():
            raise SpmvError(PROGRAM_ERROR, "load libspmv_hip.so", f"{path} missing: run `make lib`")
        _hip = _bind(ctypes.CDLL(str(path), mode=ctypes.RTLD_GLOBAL), HIP_SYMBOLS)
    return _hip


def host_lib() -> ctypes.CDLL:
    global _host
    if _host is None:
        path = Path(os.environ.get("SPMV_HOST_LIB", LIB_DIR / "libspmv_host.so"))  # `make test-san` build
        if not path.exists():
            raise SpmvError(PROGRAM_ERROR, "load libspmv_host.so", f"{path} missing: run `make lib`")
        _host = _bind(ctypes.CDLL(str(path), mode=ctypes.RTLD_GLOBAL), HOST_SYMBOLS)
    return _host


def _ptr(a) -> int | None:
    """Raw address of a numpy array or torch tensor (None for empty)."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return a.data_ptr()


def _check(rc: int, what: str) -> None:
    if rc != SUCCESS:
        detail = hip_lib().spmv_last_error().decode() if _hip is not None else ""
        raise SpmvError(rc, what, detail)


# --------------------------------------------------------- host: inputs
@dataclass
class Coo:
    """Entries in FILE order (the order check_result accumulates in)."""

    n_rows: int
    n_cols: int
    row: np.ndarray
    col: np.ndarray
    val: np.ndarray
    symmetric: bool = False
    label: str = ""

    @property
    def nnz(self) -> int:
        return int(self.row.shape[0])


def read_mtx(path: str | os.PathLike) -> Coo:
    """Matrix Market reader with the reference's acceptance rules
    (reference inc/helper_functions.h:134-165, csr.c:77-91)."""
    lib = host_lib()
    info = MtxInfo()
    p = str(path).encode()
    rc = lib.spmv_mtx_read_info(p, ctypes.byref(info))
    if rc != SUCCESS:
        raise SpmvError(rc, f"read {path}")
    z = info.nnz
    row = np.empty(z, np.int32)
    col = np.empty(z, np.int32)
    val = np.empty(z, np.float64)
    _check_host(lib.spmv_mtx_read(p, ctypes.byref(info), _ptr(row), _ptr(col), _ptr(val)), f"read {path}")
    return Coo(info.n_rows, info.n_cols, row, col, val, bool(info.symmetric), str(path))


def _check_host(rc: int, what: str) -> None:
    if rc != SUCCESS:
        raise SpmvError(rc, what)


def write_mtx(path, m: Coo) -> None:
    _check_host(host_lib().spmv_mtx_write(str(path).encode(), m.n_rows, m.n_cols, m.nnz,
                                          _ptr(m.row), _ptr(m.col), _ptr(m.val), int(m.symmetric)),
                f"write {path}")


def gen_cantlike(mode: int = 0, copies: int = 1) -> Coo:
    """cant-like stand-in (include/spmv_host.h: spmv_gen_cantlike)."""
    lib = host_lib()
    n = _c_i64()
    z = _c_i64()
    _check_host(lib.spmv_gen_cantlike(mode, copies, ctypes.byref(n), ctypes.byref(z), None, None, None), "gen_cantlike")
    row = np.empty(z.value, np.int32)
    col = np.empty(z.value, np.int32)
    val = np.empty(z.value, np.float64)
    _check_host(lib.spmv_gen_cantlike(mode, copies, ctypes.byref(n), ctypes.byref(z), _ptr(row), _ptr(col), _ptr(val)), "gen_cantlike")
    label = f"cant-like stand-in (synthetic, mode {mode}, x{copies})"
    return Coo(n.value, n.value, row, col, val, mode == 2, label)


def gen_rmat(n: int = 10_000_000, nnz: int = 100_000_000, scale: int = 24, seed: int = 1) -> Coo:
    lib = host_lib()
    row = np.empty(nnz, np.int32)
    col = np.empty(nnz, np.int32)
    val = np.empty(nnz, np.float64)
    _check_host(lib.spmv_gen_rmat(n, nnz, scale, seed, _ptr(row), _ptr(col), _ptr(val)), "gen_rmat")
    return Coo(n, n, row, col, val, False, f"R-MAT {n} rows {nnz} entries (synthetic)")


def gen_random(n_rows: int, n_cols: int, min_len: int, max_len: int, seed: int = 1) -> Coo:
    lib = host_lib()
    z = _c_i64()
    _check_host(lib.spmv_gen_random(n_rows, n_cols, min_len, max_len, seed, ctypes.byref(z), None, None, None), "gen_random")
    row = np.empty(z.value, np.int32)
    col = np.empty(z.value, np.int32)
    val = np.empty(z.value, np.float64)
    _check_host(lib.spmv_gen_random(n_rows, n_cols, min_len, max_len, seed, ctypes.byref(z), _ptr(row), _ptr(col), _ptr(val)), "gen_random")
    return Coo(n_rows, n_cols, row, col, val, False, f"random {n_rows}x{n_cols} len {min_len}..{max_len}")


def gen_banded_csr(n: int, row_begin: int = 0, row_end: int | None = None, seed: int = 2):
    """Banded rows [row_begin,row_end) in CSR form (local row_ptr)."""
    row_end = n if row_end is None else row_end
    m = row_end - row_begin
    ptr = np.empty(m + 1, np.int64)
    col = np.empty(16 * m, np.int32)
    val = np.empty(16 * m, np.float64)
    _check_host(host_lib().spmv_gen_banded_csr(n, seed, row_begin, row_end, _ptr(ptr), _ptr(col), _ptr(val)), "gen_banded")
    return ptr, col, val


def ramp_x(n_cols: int) -> np.ndarray:
    """x[j] = j, the reference's input vector (reference csr.c:95-99)."""
    return np.arange(n_cols, dtype=np.float64)


# ------------------------------------------------------- host: formats
def csr_from_coo(m: Coo):
    ptr = np.empty(m.n_rows + 1, np.int64)
    col = np.empty(m.nnz, np.int32)
    val = np.empty(m.nnz, np.float64)
    _check_host(host_lib().spmv_csr_from_coo(m.n_rows, m.nnz, _ptr(m.row), _ptr(m.col), _ptr(m.val),
                                             _ptr(ptr), _ptr(col), _ptr(val)), "csr_from_coo")
    return ptr, col, val


def csr_transpose(n_rows: int, n_cols: int, ptr, col, val):
    """A^T as CSR (spmv_csr_transpose) -> (t_ptr[n_cols+1], t_col, t_val): a
    stable counting sort by column, t_col the row ids of A."""
    nnz = int(ptr[n_rows])
    t_ptr = np.empty(n_cols + 1, np.int64)
    t_col = np.empty(nnz, np.int32)
    t_val = np.empty(nnz, np.float64)
    _check_host(host_lib().spmv_csr_transpose(n_rows, n_cols, _ptr(ptr), _ptr(col), _ptr(val), _ptr(t_ptr),
                                              _ptr(t_col), _ptr(t_val)), "csr_transpose")
    return t_ptr, t_col, t_val


# The host statements hand raw addresses and strides of numpy arrays to C:
# these two checks are all that stands between a caller's array and a loop
# that trusts them.  Each array is checked completely before the next one.
_F64 = np.dtype(np.float64)  # made once: comparing a dtype with the type np.float64 makes one every time


def _host_vectors(what: str, *pairs) -> None:
    """pairs of (array, least length): contiguous 1-D float64 vectors."""
    for a, n in pairs:
        if not isinstance(a, np.ndarray) or a.dtype != _F64 or a.ndim != 1 or not a.flags.c_contiguous:
            raise SpmvError(OTHER_ERROR, what, "x and y must be contiguous 1-D float64 arrays")
        if a.size < n:
            raise SpmvError(OTHER_ERROR, what, "x or y too short")


def _host_blocks(what: str, pairs, k=None, names=("X and Y", "X and Y", "X or Y")):
    """pairs of (array, least rows): 2-D float64 blocks with unit inner stride
    and a row stride of whole doubles, k columns (default: the first block's
    width) in each; k = 0 for blocks without a common width.  names: what the
    messages call all of them (their kind, their strides) and any one.
    Returns (k, ld), ld(a, w=k) the leading dimension C is given."""
    for a, n in pairs:
        if not isinstance(a, np.ndarray) or a.dtype != _F64 or a.ndim != 2:
            raise SpmvError(OTHER_ERROR, what, f"{names[0]} must be 2-D float64 arrays")
        if a.shape[1] > 1 and a.strides[1] != 8 or a.strides[0] % 8:
            raise SpmvError(OTHER_ERROR, what, f"{names[1]} need unit inner stride")
        if a.shape[0] < n:
            raise SpmvError(OTHER_ERROR, what, f"{names[2]} has too few rows")
    k = pairs[0][0].shape[1] if k is None else int(k)
    for a, _ in pairs:
        if k > a.shape[1]:
            raise SpmvError(OTHER_ERROR, what, f"{names[2]} has fewer than k columns")
    return k, lambda a, w=k: a.strides[0] // 8 if a.shape[0] > 1 else w  # one row: its stride is never used


def cpu_csr_t(n_rows: int, n_cols: int, ptr, col, val, x: np.ndarray, y: np.ndarray) -> None:
    """Host y = A^T x (spmv_cpu_csr_t): x has n_rows entries; y[:n_cols] is
    overwritten, nothing past it."""
    _host_vectors("cpu_csr_t", (x, n_rows), (y, n_cols))
    _check_host(host_lib().spmv_cpu_csr_t(n_rows, n_cols, _ptr(ptr), _ptr(col), _ptr(val), _ptr(x), _ptr(y)),
                "spmv_cpu_csr_t")


def expand_symmetric(m: Coo) -> Coo:
    """The matrix a half-stored symmetric COO describes, A = S + S^T - diag S
    (spmv_coo_symmetrize): m's entries in their order, then the mirror of every
    off-diagonal one.  The result has symmetric = False: nothing is left to
    mirror."""
    if m.n_rows != m.n_cols:
        raise SpmvError(OTHER_ERROR, "expand_symmetric", "the matrix is not square")
    lib = host_lib()
    z = _c_i64()
    _check_host(lib.spmv_coo_symmetrize(m.n_rows, m.nnz, _ptr(m.row), _ptr(m.col), _ptr(m.val), ctypes.byref(z),
                                        None, None, None), "spmv_coo_symmetrize")
    row = np.empty(z.value, np.int32)
    col = np.empty(z.value, np.int32)
    val = np.empty(z.value, np.float64)
    _check_host(lib.spmv_coo_symmetrize(m.n_rows, m.nnz, _ptr(m.row), _ptr(m.col), _ptr(m.val), ctypes.byref(z),
                                        _ptr(row), _ptr(col), _ptr(val)), "spmv_coo_symmetrize")
    return Coo(m.n_rows, m.n_cols, row, col, val, False, (m.label + " (symmetric, expanded)").strip())


def cpu_csr_sym(n: int, ptr, col, val, x: np.ndarray, y: np.ndarray) -> None:
    """Host y = (S + S^T - diag S) x on the half storage (spmv_cpu_csr_sym):
    x has n entries; y[:n] is overwritten, nothing past it."""
    _host_vectors("cpu_csr_sym", (x, n), (y, n))
    _check_host(host_lib().spmv_cpu_csr_sym(n, _ptr(ptr), _ptr(col), _ptr(val), _ptr(x), _ptr(y)), "spmv_cpu_csr_sym")


def cpu_csr_sym_multi(n: int, ptr, col, val, X: np.ndarray, Y: np.ndarray, k: int | None = None) -> None:
    """Host Y = (S + S^T - diag S) X on the half storage
    (spmv_cpu_csr_sym_multi): X and Y (>= n rows) are 2-D float64 arrays with
    unit inner stride whose row strides are ldx and ldy; k defaults to X's
    width.  Only Y[:n, :k] is written."""
    k, ld = _host_blocks("cpu_csr_sym_multi", ((X, n), (Y, n)), k)
    rc = host_lib().spmv_cpu_csr_sym_multi(n, _ptr(ptr), _ptr(col), _ptr(val), k, _ptr(X), ld(X), _ptr(Y), ld(Y))
    _check_host(rc, "spmv_cpu_csr_sym_multi")


def bjacobi_build_host(n: int, ptr, col, val, bs: int, col_base: int = 0, symmetric_half: bool = False):
    """The host statement of the block-Jacobi preconditioner
    (spmv_bjacobi_build) on a CSR with n rows -> (inv, singular): inv is
    (ceil(n / bs) * bs, bs), row q*bs + r holding row r of D_q^-1; singular
    counts the blocks replaced by the identity."""
    if not 1 <= bs <= 16:  # before inv is sized
        raise SpmvError(OTHER_ERROR, "bjacobi_build_host", f"bs must be 1..16, not {bs}")
    n_blocks = (max(n, 0) + bs - 1) // bs
    inv = np.empty((n_blocks * bs, bs), np.float64)
    singular = _c_i64()
    ptr, col, val = (np.ascontiguousarray(a, t) for a, t in ((ptr, np.int64), (col, np.int32), (val, np.float64)))
    _check_host(host_lib().spmv_bjacobi_build(n, _ptr(ptr), _ptr(col), _ptr(val), bs, col_base, int(symmetric_half),
                                              _ptr(inv), ctypes.byref(singular)), "spmv_bjacobi_build")
    return inv, int(singular.value)


def cpu_bjacobi_apply_multi(n: int, bs: int, inv: np.ndarray, R: np.ndarray, Z: np.ndarray, k: int | None = None) -> None:
    """Host Z = M^-1 R (spmv_cpu_bjacobi_apply_multi) with inv from
    bjacobi_build_host: R and Z (>= n rows) are 2-D float64 arrays with unit
    inner stride; k defaults to R's width.  Only Z[:n, :k] is written."""
    k, ld = _host_blocks("cpu_bjacobi_apply_multi", ((R, n), (Z, n)), k, ("R and Z", "R and Z", "R or Z"))
    inv = np.ascontiguousarray(inv, np.float64)
    if 1 <= bs <= 16 and inv.size < (max(n, 0) + bs - 1) // bs * bs * bs:
        raise SpmvError(OTHER_ERROR, "cpu_bjacobi_apply_multi", "inv is too short")
    _check_host(host_lib().spmv_cpu_bjacobi_apply_multi(n, bs, _ptr(inv), k, _ptr(R), ld(R), _ptr(Z), ld(Z)),
                "spmv_cpu_bjacobi_apply_multi")


def cpu_bjacobi_cheb_step_multi(n: int, bs: int, inv: np.ndarray, a: float, b: float, R: np.ndarray, AZ, D: np.ndarray,
                                Zin, Zout: np.ndarray, k: int | None = None) -> None:
    """One host step of the Chebyshev recurrence over M^-1
    (spmv_cpu_bjacobi_cheb_step_multi) with inv from bjacobi_build_host.
    AZ = None is step 0 (Zin may then be None as well); every array given
    (>= n rows) is a 2-D float64 array with unit inner stride; k defaults to
    R's width.  Zout may be Zin itself.  Only D[:n, :k] and Zout[:n, :k] are
    written."""
    what = "cpu_bjacobi_cheb_step_multi"
    if AZ is None:
        Zin = None
    elif Zin is None:
        raise SpmvError(OTHER_ERROR, what, "a general step (AZ given) needs Zin")
    k, ld = _host_blocks(what, [(t, n) for t in (R, AZ, D, Zin, Zout) if t is not None], k,
                         ("R, AZ, D, Zin and Zout", "the arrays", "an array"))
    inv = np.ascontiguousarray(inv, np.float64)
    if 1 <= bs <= 16 and inv.size < (max(n, 0) + bs - 1) // bs * bs * bs:
        raise SpmvError(OTHER_ERROR, what, "inv is too short")
    args = []
    for t in (R, AZ, D, Zin, Zout):
        args += [None, 0] if t is None else [_ptr(t), ld(t)]
    _check_host(host_lib().spmv_cpu_bjacobi_cheb_step_multi(n, bs, _ptr(inv), k, float(a), float(b), *args),
                "spmv_cpu_bjacobi_cheb_step_multi")


_BLOCK_NAMES = ("the blocks", "the blocks", "a block")


def _bicgstab_blocks(what: str, n: int, k, blocks, scalars):
    """The checks of the two BiCGSTAB host statements: 2-D float64 blocks with
    unit inner stride and >= n rows, k (default: the first block's width)
    columns in each, float64 arrays of >= k scalars.  Returns (k, ld(block))."""
    k, ld = _host_blocks(what, [(t, n) for t in blocks], k, _BLOCK_NAMES)
    for c in scalars:
        if not isinstance(c, np.ndarray) or c.dtype != np.float64 or c.ndim != 1 or c.size < k or \
                (c.size > 1 and c.strides[0] != 8):
            raise SpmvError(OTHER_ERROR, what, "the scalars must be contiguous float64 arrays of k entries")
    return k, ld


def cpu_bicgstab_update_multi(n: int, a_num, a_den, w_num, w_den, Ph, Sh, T, X, R, k: int | None = None) -> None:
    """Host statement of BiCGSTAB's fused update (spmv_cpu_bicgstab_update_multi):
    with alpha_j = a_num[j] / a_den[j] and omega_j = w_num[j] / w_den[j] (0 for
    a zero denominator), X = fma(omega, Sh, fma(alpha, Ph, X)) and
    R = fma(-omega, T, R) on 2-D float64 blocks (>= n rows, unit inner stride);
    Sh may be R itself.  Only X[:n, :k] and R[:n, :k] are written."""
    k, ld = _bicgstab_blocks("cpu_bicgstab_update_multi", n, k, (Ph, Sh, T, X, R), (a_num, a_den, w_num, w_den))
    _check_host(host_lib().spmv_cpu_bicgstab_update_multi(n, k, _ptr(a_num), _ptr(a_den), _ptr(w_num), _ptr(w_den),
                                                          _ptr(Ph), ld(Ph), _ptr(Sh), ld(Sh), _ptr(T), ld(T), _ptr(X),
                                                          ld(X), _ptr(R), ld(R)), "spmv_cpu_bicgstab_update_multi")


def cpu_bicgstab_dir_multi(n: int, rho_new, rv, tt, ts, V, R, P, k: int | None = None) -> None:
    """Host statement of BiCGSTAB's direction update (spmv_cpu_bicgstab_dir_multi):
    P = fma(beta, fma(-omega, V, P), R) with beta_j = (rho_new[j] / rv[j]) *
    (tt[j] / ts[j]) and omega_j = ts[j] / tt[j] (0 for a zero denominator).
    Only P[:n, :k] is written."""
    k, ld = _bicgstab_blocks("cpu_bicgstab_dir_multi", n, k, (V, R, P), (rho_new, rv, tt, ts))
    _check_host(host_lib().spmv_cpu_bicgstab_dir_multi(n, k, _ptr(rho_new), _ptr(rv), _ptr(tt), _ptr(ts), _ptr(V),
                                                       ld(V), _ptr(R), ld(R), _ptr(P), ld(P)),
                "spmv_cpu_bicgstab_dir_multi")


def combine_matrix(C, blocks, who: str):
    """The checks that spmv_block_combine_multi's callers share: 1 to 3 blocks
    of 1..8 columns each, C a (sum of their widths, kc) matrix with kc in 1..8.
    Returns (C as a contiguous float64 array, kc)."""
    if not 1 <= len(blocks) <= 3:
        raise SpmvError(OTHER_ERROR, who, "1 to 3 operand blocks")
    widths = [int(t.shape[1]) for t in blocks]
    if any(not 1 <= w <= 8 for w in widths):
        raise SpmvError(OTHER_ERROR, who, f"every operand has 1..8 columns, not {widths}")
    C = np.ascontiguousarray(C, np.float64)
    if C.ndim != 2 or C.shape[0] != sum(widths) or not 1 <= C.shape[1] <= 8:
        raise SpmvError(OTHER_ERROR, who, f"C must be ({sum(widths)}, kc in 1..8), not {C.shape}")
    return C, int(C.shape[1])


def cpu_block_combine_multi(n: int, C, blocks, Y: np.ndarray) -> None:
    """Host statement of the block combine (spmv_cpu_block_combine_multi):
    Y[:n, :kc] = [blocks[0] blocks[1] blocks[2]] C, every element the fma chain
    s = 0; s = fma(S[i][r], C[r][c], s) in the order of r.  blocks: 1 to 3 2-D
    float64 arrays (>= n rows, unit inner stride, 1..8 columns each); C: (sum of
    their widths, kc <= 8); Y (>= n rows, >= kc columns) must not overlap them.
    Only Y[:n, :kc] is written."""
    what = "cpu_block_combine_multi"
    _, ld = _host_blocks(what, [(t, n) for t in (*blocks, Y)], 0, _BLOCK_NAMES)  # every block has its own width
    C, kc = combine_matrix(C, blocks, what)
    if Y.shape[1] < kc:
        raise SpmvError(OTHER_ERROR, what, "Y has fewer than kc columns")
    args = []
    for q in range(3):
        t = blocks[q] if q < len(blocks) else None
        args += [0, None, 0] if t is None else [t.shape[1], _ptr(t), ld(t, t.shape[1])]
    _check_host(host_lib().spmv_cpu_block_combine_multi(n, kc, _ptr(C), *args, _ptr(Y), ld(Y, kc)),
                "spmv_cpu_block_combine_multi")


KRYLOV_MAX_COLS = 32  # SPMV_KRYLOV_MAX_COLS (spmv_ext.h): the widest GMRES basis
_COLUMN_NAMES = ("the vectors", "the vectors", "a vector")


def _krylov_operands(what: str, n: int, V, c, columns, coef=None):
    """The checks of the three GMRES host statements: V a 2-D float64 block
    (>= n rows, unit inner stride) of which c columns (default: all, 1..32) are
    read; every vector in `columns` a 2-D float64 (>= n rows, 1) array, which
    may be a column view of a block; coef (h or y) a contiguous float64 array
    of >= c entries.  Returns (c, ld)."""
    if V is not None:
        c, ld = _host_blocks(what, [(V, n)], c, _BLOCK_NAMES)
        if not 1 <= c <= KRYLOV_MAX_COLS:
            raise SpmvError(OTHER_ERROR, what, f"the basis has 1..{KRYLOV_MAX_COLS} columns, not {c}")
    _, ld = _host_blocks(what, [(t, n) for t in columns], 1, _COLUMN_NAMES)
    if coef is not None:
        _host_vectors(what, (coef, c))
    return c, ld


def cpu_krylov_project(n: int, V, h, w, w_out, c: int | None = None) -> None:
    """Host statement of one Gram-Schmidt pass (spmv_cpu_krylov_project):
    w_out[i] = the chain s = w[i]; s = fma(-h[j], V[i][j], s), j < c.  V: a 2-D
    float64 block (>= n rows, unit inner stride), c defaults to its width
    (1..32); h: >= c float64 scalars; w and w_out: (>= n rows, 1) float64 arrays,
    possibly column views; w_out may be w.  Only w_out[:n] is written."""
    what = "cpu_krylov_project"
    c, ld = _krylov_operands(what, n, V, c, (w, w_out), h)
    _check_host(host_lib().spmv_cpu_krylov_project(n, c, _ptr(V), ld(V, c), _ptr(h), _ptr(w), ld(w), _ptr(w_out),
                                                   ld(w_out)), "spmv_cpu_krylov_project")


def cpu_krylov_combine(n: int, V, y, t, c: int | None = None) -> None:
    """Host statement of t = V y (spmv_cpu_krylov_combine): t[i] = the chain
    s = 0; s = fma(V[i][j], y[j], s), j < c.  Operands as cpu_krylov_project;
    t must not overlap the columns read.  Only t[:n] is written."""
    what = "cpu_krylov_combine"
    c, ld = _krylov_operands(what, n, V, c, (t,), y)
    _check_host(host_lib().spmv_cpu_krylov_combine(n, c, _ptr(V), ld(V, c), _ptr(y), _ptr(t), ld(t)),
                "spmv_cpu_krylov_combine")


def cpu_krylov_normalize(n: int, s, w, v, copy=None) -> None:
    """Host statement of v = w / sqrt(s[0]) (spmv_cpu_krylov_normalize), v = 0
    when s[0] <= 0.  s: one float64 scalar in an array; w and v: (>= n rows, 1)
    float64 arrays, possibly column views, v may be w; copy: None or a contiguous
    float64 vector of >= n entries that receives the same values."""
    what = "cpu_krylov_normalize"
    _, ld = _krylov_operands(what, n, None, None, (w, v))
    _host_vectors(what, (s, 1), *(() if copy is None else ((copy, n),)))
    _check_host(host_lib().spmv_cpu_krylov_normalize(n, _ptr(s), _ptr(w), ld(w), _ptr(v), ld(v), _ptr(copy)),
                "spmv_cpu_krylov_normalize")


def csr_sort_rows(n_rows: int, ptr, col, val) -> None:
    """Sort every row's entries by column, in place (spmv_csr_sort_rows)."""
    _check_host(host_lib().spmv_csr_sort_rows(n_rows, _ptr(ptr), _ptr(col), _ptr(val)), "csr_sort_rows")


def coo_sort_by_row(m: Coo):
    row = np.empty(m.nnz, np.int32)
    col = np.empty(m.nnz, np.int32)
    val = np.empty(m.nnz, np.float64)
    _check_host(host_lib().spmv_coo_sort_by_row(m.n_rows, m.nnz, _ptr(m.row), _ptr(m.col), _ptr(m.val),
                                                _ptr(row), _ptr(col), _ptr(val)), "coo_sort_by_row")
    return row, col, val


def row_stats(n_rows: int, ptr: np.ndarray):
    mn, mx, mean = _c_i64(), _c_i64(), ctypes.c_double()
    host_lib().spmv_csr_row_stats(n_rows, _ptr(ptr), ctypes.byref(mn), ctypes.byref(mx), ctypes.byref(mean))
    return mn.value, mx.value, mean.value


def ell_build(n_rows: int, ptr, col, val, ki: int = 2, max_padding: float | None = None):
    lib = host_lib()
    K, ld = _c_i32(), _c_i64()
    _check_host(lib.spmv_ell_plan(n_rows, _ptr(ptr), ki, ctypes.byref(K), ctypes.byref(ld)), "ell_plan")
    stored = K.value * ld.value
    nnz = int(ptr[-1]) if n_rows > 0 else 0
    if max_padding is not None and nnz > 0 and stored / nnz > max_padding:
        raise SpmvError(OTHER_ERROR, "ell_build", f"padding factor {stored / nnz:.1f} > {max_padding}")
    ecol = np.empty(max(stored, 1), np.int32)
    evalv = np.empty(max(stored, 1), np.float64)
    _check_host(lib.spmv_ell_fill(n_rows, _ptr(ptr), _ptr(col), _ptr(val), K.value, ld.value, ki,
                                  _ptr(ecol), _ptr(evalv)), "ell_fill")
    return dict(K=K.value, ld=ld.value, ki=ki, col=ecol, val=evalv, stored=stored)


def sell_build(n_rows: int, ptr, col, val, C: int = 64, sigma: int = 1024, ki: int = 2):
    lib = host_lib()
    ns, stored = _c_i64(), _c_i64()
    _check_host(lib.spmv_sell_plan(n_rows, _ptr(ptr), C, sigma, ki, ctypes.byref(ns), ctypes.byref(stored)), "sell_plan")
    sp = np.empty(ns.value + 1, np.int64)
    perm = np.empty(max(ns.value * C, 1), np.int32)
    scol = np.empty(max(stored.value, 1), np.int32)
    sval = np.empty(max(stored.value, 1), np.float64)
    _check_host(lib.spmv_sell_fill(n_rows, _ptr(ptr), _ptr(col), _ptr(val), C, sigma, ki, ns.value,
                                   _ptr(sp), _ptr(perm), _ptr(scol), _ptr(sval)), "sell_fill")
    return dict(C=C, sigma=sigma, ki=ki, n_slices=ns.value, slice_ptr=sp, perm=perm, col=scol,
                val=sval, stored=stored.value)


def sell_split_plan(s: dict, T: int | None = None):
    """Wide-slice split plan of a sell_build result: (T, chunk_slice,
    chunk_k0); T None = the library rule (0: no split)."""
    hl = host_lib()
    sp = np.ascontiguousarray(s["slice_ptr"], dtype=np.int64)
    if T is None:
        T = hl.spmv_sell_split_auto(s["n_slices"], _ptr(sp), s["C"], s["ki"])
    if T <= 0:
        return 0, np.zeros(0, np.int32), np.zeros(0, np.int32)
    n = hl.spmv_sell_split_plan(s["n_slices"], _ptr(sp), s["C"], T, None, None)
    if n < 0:
        raise SpmvError(OTHER_ERROR, "spmv_sell_split_plan", "bad plan arguments")
    cs, ck = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    hl.spmv_sell_split_plan(s["n_slices"], _ptr(sp), s["C"], T, _ptr(cs), _ptr(ck))
    return T, cs[:n], ck[:n]


def hot_columns(n_cols: int, col, H: int = 0):
    """spmv_hot_columns: (H, hot[H], col_hot) — the H most frequent columns
    and col with them renumbered n_cols + rank (H = 0: the library rule)."""
    col = np.ascontiguousarray(col, dtype=np.int32)
    hot = np.empty(max(H, 1 << 19), np.int32)
    out = np.empty(max(col.size, 1), np.int32)
    n = host_lib().spmv_hot_columns(n_cols, col.size, _ptr(col), H, _ptr(hot), _ptr(out))
    if n < 0:
        raise SpmvError(OTHER_ERROR, "spmv_hot_columns", "bad arguments")
    return int(n), hot[:n].copy(), out[: col.size]


def column_relabel(n_cols: int, col, ties: str = "id"):
    """spmv_column_relabel(_ex): (order, newid, col') — columns ranked by
    decreasing entry count, ties by column id or (ties="first") by first
    appearance in col; x' = x[order] is the input of the relabelled matrix,
    whose y is the original's, row for row."""
    if ties not in ("id", "first"):
        raise SpmvError(OTHER_ERROR, "spmv_column_relabel", f"ties must be 'id' or 'first', not {ties!r}")
    col = np.ascontiguousarray(col, dtype=np.int32)
    order = np.empty(n_cols, np.int32)
    newid = np.empty(n_cols, np.int32)
    out = np.empty(max(col.size, 1), np.int32)
    n = host_lib().spmv_column_relabel_ex(n_cols, col.size, _ptr(col), _ptr(order), _ptr(newid), _ptr(out),
                                          0 if ties == "id" else 1)
    if n < 0:
        raise SpmvError(OTHER_ERROR, "spmv_column_relabel", "bad arguments")
    return order, newid, out[: col.size]


TILED_ROW_CAP = 1024  # rows a tiled-CSR tile stages offsets for (staged.hip kTiledRowCap)


def csr_tiled_bigplan(n_rows: int, ptr: np.ndarray, nnz: int, cap: int = TILED_ROW_CAP):
    """spmv_csr_tiled_bigplan for the tile the library runs this matrix
    with (spmv_csr_tiled_tile): int32 plan, or None when no tile owns more
    than `cap` rows."""
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    tile = int(hip_lib().spmv_csr_tiled_tile(n_rows, nnz))
    n = host_lib().spmv_csr_tiled_bigplan(n_rows, _ptr(ptr), tile, cap, None)
    if n < 0:
        raise SpmvError(OTHER_ERROR, "spmv_csr_tiled_bigplan", "bad arguments")
    plan = np.empty(max(n, 1), np.int32)
    host_lib().spmv_csr_tiled_bigplan(n_rows, _ptr(ptr), tile, cap, _ptr(plan))
    tiles = (nnz + tile - 1) // tile
    return plan if tiles > 0 and np.any(plan[:tiles] >= 0) else None


def csr_multi_plan(n_rows: int, ptr: np.ndarray, long_len: int, seg_len: int, counts_only: bool = False) -> dict:
    """spmv_csr_multi_plan: the long-row plan of the balanced multi-vector
    run -> {"n_long", "n_seg", "n_slots"} and, unless counts_only, the tables
    seg_beg[n_seg] (int64), seg_cnt / seg_dest[n_seg], long_row /
    long_first[n_long + 1] (int32)."""
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    if ptr.size != n_rows + 1:
        raise SpmvError(OTHER_ERROR, "csr_multi_plan", "row_ptr must hold n_rows + 1 offsets")
    f = host_lib().spmv_csr_multi_plan
    nl, ns, nsl = _c_i64(0), _c_i64(0), _c_i64(0)
    refs = (ctypes.byref(nl), ctypes.byref(ns), ctypes.byref(nsl))
    _check_host(f(n_rows, ptr.ctypes.data, long_len, seg_len, *refs, None, None, None, None, None), "csr_multi_plan")
    out = {"n_long": nl.value, "n_seg": ns.value, "n_slots": nsl.value}
    if counts_only:
        return out
    t = {"seg_beg": np.empty(max(ns.value, 1), np.int64), "seg_cnt": np.empty(max(ns.value, 1), np.int32),
         "seg_dest": np.empty(max(ns.value, 1), np.int32), "long_row": np.empty(nl.value + 1, np.int32),
         "long_first": np.empty(nl.value + 1, np.int32)}
    _check_host(f(n_rows, ptr.ctypes.data, long_len, seg_len, *refs, *(a.ctypes.data for a in t.values())),
                "csr_multi_plan")
    assert (nl.value, ns.value, nsl.value) == (out["n_long"], out["n_seg"], out["n_slots"])
    for k in ("seg_beg", "seg_cnt", "seg_dest"):
        t[k] = t[k][: ns.value]
    return {**out, **t}


def relabel_columns(m: Coo):
    """(m', order): m with its columns relabelled hot-first (same rows, same
    entry order); run m' on x[order]."""
    order, _, c2 = column_relabel(m.n_cols, m.col)
    return Coo(m.n_rows, m.n_cols, m.row, c2, m.val, False, f"{m.label} (columns relabelled by degree)"), order


def gather_x(order, x, out=None, stream=None):
    """out[k] = x[order[k]] on the device (spmv_gather): the x a
    column-relabelled matrix takes.  order: int32 device tensor."""
    torch = _torch()
    if out is None:
        out = torch.empty(order.numel(), dtype=torch.float64, device=x.device)
    s = stream if stream is not None else torch.cuda.current_stream(x.device)
    _check(hip_lib().spmv_gather(order.numel(), _ptr(order), _ptr(x), _ptr(out), x.device.index or 0, s.cuda_stream),
           "spmv_gather")
    return out


def cmrs_build(n_rows: int, ptr, h: int = 8):
    ns = (n_rows + h - 1) // h
    sp = np.empty(ns + 1, np.int64)
    rin = np.empty(max(int(ptr[-1]), 1), np.uint8)
    _check_host(host_lib().spmv_cmrs_build(n_rows, _ptr(ptr), h, _ptr(sp), _ptr(rin)), "cmrs_build")
    return dict(h=h, n_strips=ns, strip_ptr=sp, row_in_strip=rin)


def hyb_build(n_rows: int, ptr, col, val, ki: int = 2, K: int = 0):
    """ELL part (first K entries per row) + row-sorted COO tail (§8f row 4)."""
    Kc, ld, tail = _c_i32(0), _c_i64(0), _c_i64(0)
    _check_host(host_lib().spmv_hyb_plan(n_rows, _ptr(ptr), ki, K, ctypes.byref(Kc), ctypes.byref(ld),
                                         ctypes.byref(tail)), "hyb_plan")
    stored = Kc.value * ld.value
    ec, ev = np.empty(max(stored, 1), np.int32), np.empty(max(stored, 1), np.float64)
    tr, tc = np.empty(max(tail.value, 1), np.int32), np.empty(max(tail.value, 1), np.int32)
    tv = np.empty(max(tail.value, 1), np.float64)
    _check_host(host_lib().spmv_hyb_fill(n_rows, _ptr(ptr), _ptr(col), _ptr(val), Kc.value, ld.value, ki, _ptr(ec),
                                         _ptr(ev), _ptr(tr), _ptr(tc), _ptr(tv)), "hyb_fill")
    return dict(K=Kc.value, ld=ld.value, ki=ki, stored=stored, tail_nnz=tail.value, ell_col=ec, ell_val=ev,
                tail_row=tr, tail_col=tc, tail_val=tv)


def csr16_build(col: np.ndarray):
    """16-bit column offsets per 64-entry block."""
    nnz = int(col.shape[0])
    nb, ne = _c_i64(0), _c_i64(0)
    _check_host(host_lib().spmv_csr16_plan(nnz, _ptr(col), ctypes.byref(nb), ctypes.byref(ne)), "csr16_plan")
    base = np.empty(max(nb.value, 1), np.int32)
    off = np.empty(max(nnz, 2), np.uint16)
    esc = np.empty(max(ne.value * 64, 1), np.int32)
    _check_host(host_lib().spmv_csr16_fill(nnz, _ptr(col), _ptr(base), _ptr(off), _ptr(esc)), "csr16_fill")
    return dict(n_blocks=nb.value, n_esc=ne.value, blk_base=base, col_off=off, col_esc=esc)


def csrg_build(n_rows: int, ptr, col, val, groups: int = 4):
    """Column-grouped CSR (spmv_host.h spmv_csrg_plan/fill): the entries
    group after group of 128-B x lines, as a CSR over (row, group) pairs,
    plus the per-row-block pair ranges of the reduce."""
    lib = host_lib()
    npairs = _c_i64(0)
    _check_host(lib.spmv_csrg_plan(n_rows, _ptr(ptr), _ptr(col), groups, ctypes.byref(npairs)), "csrg_plan")
    n = npairs.value
    nnz = int(ptr[n_rows])
    rows = int(host_lib().spmv_csrg_block_rows())  # SPMV_CSRG_ROWS as built into the host fill
    nb = (n_rows + rows - 1) // rows
    pair_ptr = np.empty(n + 1, np.int64)
    col_g = np.empty(max(nnz, 1), np.int32)
    val_g = np.empty(max(nnz, 1), np.float64)
    blk_off = np.empty(groups * (nb + 1), np.int32)
    pair_row = np.empty(max(n, 1), np.uint16)
    _check_host(lib.spmv_csrg_fill(n_rows, _ptr(ptr), _ptr(col), _ptr(val), groups, _ptr(pair_ptr), _ptr(col_g),
                                   _ptr(val_g), _ptr(blk_off), _ptr(pair_row)), "csrg_fill")
    return dict(groups=groups, n_pairs=n, nb=nb, pair_ptr=pair_ptr, col_g=col_g, val_g=val_g, blk_off=blk_off,
                pair_row=pair_row)


BSR_MAX_B = 8  # SPMV_BSR_MAX_B (spmv_host.h): the host builder's block sizes; the device runs 2, 3 and 4


def bsr_build(n_rows: int, n_cols: int, ptr, col, val, b: int):
    """Block CSR with b x b blocks from a CSR (spmv_bsr_plan / spmv_bsr_fill,
    spmv_host.h, which states the layout and the fill-in rule): brow_ptr
    (n_brows + 1, int64), bcol (n_blocks, int32, ascending inside a block row),
    bval (n_blocks * b * b, float64, scipy's data[blk, r, c]); fill = stored
    values / entries (0.0 for an empty matrix)."""
    lib = host_lib()
    nbr, nbl = _c_i64(0), _c_i64(0)
    _check_host(lib.spmv_bsr_plan(n_rows, n_cols, _ptr(ptr), _ptr(col), b, ctypes.byref(nbr), ctypes.byref(nbl)),
                "bsr_plan")
    brow_ptr = np.empty(nbr.value + 1, np.int64)
    bcol = np.empty(nbl.value, np.int32)
    bval = np.empty(nbl.value * b * b, np.float64)
    _check_host(lib.spmv_bsr_fill(n_rows, n_cols, _ptr(ptr), _ptr(col), _ptr(val), b, _ptr(brow_ptr), _ptr(bcol),
                                  _ptr(bval)), "bsr_fill")
    nnz = int(ptr[n_rows]) - int(ptr[0]) if n_rows > 0 else 0
    return dict(b=b, n_brows=nbr.value, n_blocks=nbl.value, brow_ptr=brow_ptr, bcol=bcol, bval=bval,
                fill=nbl.value * b * b / nnz if nnz else 0.0)


def bsr_stored_bytes(s: dict) -> int:
    """Bytes of the three BSR arrays of bsr_build's dict."""
    return 8 * s["n_blocks"] * s["b"] ** 2 + 4 * s["n_blocks"] + 8 * (s["n_brows"] + 1)


def bsr_check_fill(n_rows: int, nnz: int, s: dict, bsr_max_fill: float | None = None) -> None:
    """to_device's acceptance rule for bsr_build's dict `s`: None raises
    SpmvError when the BSR arrays are not smaller than CSR's
    12 nnz + 8 (n_rows + 1) bytes (a derived break-even, not a measured one); a
    float raises when fill exceeds it (float("inf"): never)."""
    b, stored, csr_bytes = s["b"], bsr_stored_bytes(s), 12 * nnz + 8 * (n_rows + 1)
    if bsr_max_fill is None and stored >= csr_bytes:
        raise SpmvError(OTHER_ERROR, "bsr_build", f"{b}x{b} blocks store {stored} bytes (fill {s['fill']:.3f}), "
                        f"not fewer than CSR's {csr_bytes}")
    if bsr_max_fill is not None and s["fill"] > float(bsr_max_fill):
        raise SpmvError(OTHER_ERROR, "bsr_build", f"{b}x{b} blocks: fill {s['fill']:.3f} > {float(bsr_max_fill)}")


def cpu_bsr(n_rows: int, n_cols: int, b: int, brow_ptr, bcol, bval, x: np.ndarray, y: np.ndarray) -> None:
    """y = A x from the BSR arrays on the CPU (spmv_cpu_bsr: the plain loop,
    the host statement of a BSR plan's run).  x float64 (>= n_cols), y
    float64 (>= n_rows), both C-contiguous; y[:n_rows] is overwritten."""
    for a, n, what in ((x, n_cols, "x"), (y, n_rows, "y")):
        if not isinstance(a, np.ndarray) or a.dtype != np.float64 or a.ndim != 1 or not a.flags.c_contiguous:
            raise SpmvError(OTHER_ERROR, "cpu_bsr", f"{what} must be a contiguous 1-D float64 array")
        if a.shape[0] < n:
            raise SpmvError(OTHER_ERROR, "cpu_bsr", f"{what} is too short")
    _check_host(host_lib().spmv_cpu_bsr(n_rows, n_cols, b, int(brow_ptr.shape[0]) - 1, _ptr(brow_ptr), _ptr(bcol),
                                        _ptr(bval), _ptr(x), _ptr(y)), "cpu_bsr")


def partition_rows(n_rows: int, ptr: np.ndarray, parts: int, align: int = 1024,
                   row_weight: float = 0.0) -> np.ndarray:
    """Contiguous row ranges with ~nnz/parts entries each;
    row_weight > 0 balances entries + row_weight per row instead."""
    bounds = np.empty(parts + 1, np.int64)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    if row_weight:
        rc = host_lib().spmv_partition_rows_weighted(n_rows, _ptr(ptr), parts, align, float(row_weight), _ptr(bounds))
    else:
        rc = host_lib().spmv_partition_rows(n_rows, _ptr(ptr), parts, align, _ptr(bounds))
    _check_host(rc, "partition_rows")
    return bounds


def partition_rows_calibrated(n_rows: int, ptr: np.ndarray, parts: int, old_bounds, old_ms, align: int = 1024,
                              row_weight: float = 0.0) -> np.ndarray:
    """Re-cut rows into `parts` ranges of equal measured cost: each row
    costs its old shard's time per (entries + row_weight * rows) unit
    (spmv_partition_rows_calibrated)."""
    bounds = np.empty(parts + 1, np.int64)
    ptr = np.ascontiguousarray(ptr, dtype=np.int64)
    ob = np.ascontiguousarray(old_bounds, dtype=np.int64)
    ms = np.ascontiguousarray(old_ms, dtype=np.float64)
    if ms.size + 1 != ob.size:
        raise SpmvError(OTHER_ERROR, "partition_rows_calibrated", "one time per old shard")
    _check_host(host_lib().spmv_partition_rows_calibrated(n_rows, _ptr(ptr), parts, align, float(row_weight),
                                                          ms.size, _ptr(ob), _ptr(ms), _ptr(bounds)),
                "partition_rows_calibrated")
    return bounds


def partition_rows_damped(n_rows: int, old_bounds, new_bounds, damp: float = 0.5, align: int = 1024) -> np.ndarray:
    """Move every cut point of old_bounds the fraction `damp` of the way to
    new_bounds (aligned, monotone, ends kept).  Cold shard times are not
    linear in a shard's rows and entries (a flushed shard also re-reads x
    and its row offsets), so a full profile-guided re-cut overshoots; half
    steps settle instead."""
    ob = np.asarray(old_bounds, dtype=np.float64)
    nb = np.asarray(new_bounds, dtype=np.float64)
    if ob.shape != nb.shape or ob[0] != 0 or nb[0] != 0 or ob[-1] != n_rows or nb[-1] != n_rows:
        raise SpmvError(OTHER_ERROR, "partition_rows_damped", "bounds must share size and ends")
    b = np.rint((ob + damp * (nb - ob)) / align).astype(np.int64) * align
    b[0], b[-1] = 0, n_rows
    b = np.minimum(np.maximum.accumulate(b), n_rows)
    return b


def shard(m: Coo, lo: int, hi: int) -> Coo:
    """Rows [lo, hi) of m as a local matrix (row ids rebased, columns kept:
    x stays replicated)."""
    sel = (m.row >= lo) & (m.row < hi)
    return Coo(hi - lo, m.n_cols, (m.row[sel] - lo).astype(np.int32), m.col[sel], m.val[sel], m.symmetric,
               f"{m.label} rows [{lo},{hi})")


def bytes_alg(n_rows: int, n_cols: int, nnz: int) -> int:
    """Algorithmic bytes of one SpMV: fp64 values + int32
    columns + int32 row offsets + x read once + y written once."""
    return 12 * nnz + 4 * (n_rows + 1) + 8 * n_cols + 8 * n_rows


def bytes_alg_multi(n_rows: int, n_cols: int, nnz: int, k: int) -> int:
    """Algorithmic bytes of one multi-vector run Y = A X with k vectors: the
    matrix once, k vectors read and k written (k = 1: bytes_alg)."""
    return 12 * nnz + 4 * (n_rows + 1) + 8 * k * (n_cols + n_rows)


def cpu_csr_multi(n_rows: int, ptr, col, val, X: np.ndarray, Y: np.ndarray, k: int | None = None) -> None:
    """Host Y = A X (spmv_cpu_csr_multi): X and Y (>= n_rows rows) are 2-D
    float64 arrays with unit inner stride whose row strides are ldx and ldy; k
    defaults to X's width.  Only Y[:n_rows, :k] is written."""
    k, ld = _host_blocks("cpu_csr_multi", ((X, 0), (Y, n_rows)), k)  # no n_cols here: X's rows go unchecked
    rc = host_lib().spmv_cpu_csr_multi(n_rows, _ptr(ptr), _ptr(col), _ptr(val), k, _ptr(X), ld(X), _ptr(Y), ld(Y))
    _check_host(rc, "spmv_cpu_csr_multi")


def cpu_csr_t_multi(n_rows: int, n_cols: int, ptr, col, val, X: np.ndarray, Y: np.ndarray, k: int | None = None) -> None:
    """Host Y = A^T X (spmv_cpu_csr_t_multi): X (>= n_rows rows) and Y
    (>= n_cols rows) are 2-D float64 arrays with unit inner stride whose row
    strides are ldx and ldy; k defaults to X's width.  Only Y[:n_cols, :k] is
    written."""
    k, ld = _host_blocks("cpu_csr_t_multi", ((X, n_rows), (Y, n_cols)), k)
    rc = host_lib().spmv_cpu_csr_t_multi(n_rows, n_cols, _ptr(ptr), _ptr(col), _ptr(val), k, _ptr(X), ld(X),
                                         _ptr(Y), ld(Y))
    _check_host(rc, "spmv_cpu_csr_t_multi")


def check(m: Coo, x: np.ndarray, y: np.ndarray, rel_tol: float = 1e-6, abs_tol: float = 0.0):
    """Host check_result (reference inc/helper_functions.h:184-236)
    -> (bad_rows, first_bad)."""
    first = _c_i64()
    ref = ctypes.c_double()
    bad = host_lib().spmv_check(m.n_rows, m.nnz, _ptr(m.row), _ptr(m.col), _ptr(m.val), _ptr(x), _ptr(y),
                                abs_tol, rel_tol, ctypes.byref(first), ctypes.byref(ref))
    return int(bad), int(first.value)


# ------------------------------------------------------------- device
def _torch():
    import torch

    return torch


def _dev_tensor(arr: np.ndarray, device):
    torch = _torch()
    return torch.from_numpy(np.ascontiguousarray(arr)).to(device)


# Raw data_ptr()s and strides go to the C-ABI: a tensor of another dtype, a
# strided view or a tensor on another device would give a wrong y or a GPU
# fault, not an exception.  The two checks below are the only thing between a
# caller's tensors and a kernel; they are in front of every launch, so they
# look torch, the dtype and the device up once, not per tensor.
def _ld(t, k: int) -> int:
    """Leading dimension of a row-major (rows, k) block (one row: its stride is never used)."""
    return t.stride(0) if t.shape[0] > 1 else k


def _on_device(t, here) -> bool:
    """t is on the torch.device `here`, an index-less device being its device
    0 (the one dims() names); equal devices are the quick way out."""
    d = t.device
    return d == here or (d.type == here.type and (d.index or 0) == (here.index or 0))


def _check_vectors(what: str, x, x_len: int, y, y_len: int, device, *, types="x and y must be float64 tensors",
                   refuse=None) -> None:
    """x and y are contiguous float64 tensors of >= x_len and >= y_len entries
    on `device`, or SpmvError(OTHER_ERROR, what, ..).  types: the wording of
    the first refusal (run's differs).  refuse: a refusal of the caller's own
    that stands between the type checks and the sizes."""
    torch = _torch()
    tensor, f64 = torch.Tensor, torch.float64
    for t in (x, y):
        if not isinstance(t, tensor) or t.dtype != f64:
            raise SpmvError(OTHER_ERROR, what, types)
    if refuse:
        raise SpmvError(OTHER_ERROR, what, refuse)
    if x.numel() < x_len or y.numel() < y_len:
        raise SpmvError(OTHER_ERROR, what, "x or y too short")
    if not (x.is_contiguous() and y.is_contiguous()):
        raise SpmvError(OTHER_ERROR, what, "x and y must be contiguous")
    here = torch.device(device)
    if not (_on_device(x, here) and _on_device(y, here)):
        raise SpmvError(OTHER_ERROR, what, f"x and y must be on {here.type}:{here.index or 0}")


def _check_blocks(what: str, X, x_rows: int, Y, y_rows: int, device, *, refuse=None):
    """X and Y are row-major float64 blocks on `device` of >= x_rows and
    >= y_rows rows and the same k >= 1 columns: rows of k contiguous values, row
    stride >= k, so column slices of wider tensors pass.  Returns (k, ldx,
    ldy), or SpmvError(OTHER_ERROR, what, ..); refuse as in _check_vectors."""
    torch = _torch()
    tensor, f64 = torch.Tensor, torch.float64
    for t in (X, Y):
        if not isinstance(t, tensor) or t.dtype != f64:
            raise SpmvError(OTHER_ERROR, what, "X and Y must be float64 tensors")
        if t.dim() != 2:
            raise SpmvError(OTHER_ERROR, what, "X and Y must be 2-D (rows, k)")
    if refuse:
        raise SpmvError(OTHER_ERROR, what, refuse)
    (xr, k), (yr, yk) = X.shape, Y.shape
    if k < 1 or yk != k:
        raise SpmvError(OTHER_ERROR, what, "X and Y must have the same number k >= 1 of columns")
    if xr < x_rows or yr < y_rows:
        raise SpmvError(OTHER_ERROR, what, "X or Y has too few rows")
    for rows, (row_stride, inner) in ((xr, X.stride()), (yr, Y.stride())):
        if (k > 1 and inner != 1) or (rows > 1 and row_stride < k):
            raise SpmvError(OTHER_ERROR, what, "X and Y need inner stride 1 and a row stride >= k")
    here = torch.device(device)
    if not (_on_device(X, here) and _on_device(Y, here)):
        raise SpmvError(OTHER_ERROR, what, f"X and Y must be on {here.type}:{here.index or 0}")
    return k, _ld(X, k), _ld(Y, k)


def _stream_handle(stream, device) -> int:
    """The HIP stream of `stream` (None: torch's current stream on `device`)."""
    st = stream if stream is not None else _torch().cuda.current_stream(device)
    return st.cuda_stream


@dataclass
class DeviceMatrix:
    """One format resident in HBM, ready for repeated SpMV launches.

    The reference's five formats run through a C plan (spmv_plan_<fmt>,
    include/spmv.h): the library chooses and prepares the kernel path once,
    exactly as ./bin/<fmt> does, and run() is spmv_plan_run.  `arrays`
    holds the format's device arrays (torch tensors, owned here; the plan
    keeps pointers to them), `params` the plan's choices (spmv_plan_info).
    The §8f extra formats (csr16, csrf32, hyb, csrg) call their entry
    points of include/spmv_ext.h directly."""

    fmt: str
    n_rows: int
    n_cols: int
    nnz: int
    device: object
    arrays: dict = field(default_factory=dict)
    params: dict = field(default_factory=dict)
    stored_bytes: int = 0
    plan: object = None  # ctypes.c_void_p of an spmv_plan, or None

    def __del__(self):
        plan, self.plan = self.plan, None
        if plan is not None and _hip is not None and not sys.is_finalizing():
            _hip.spmv_plan_destroy(plan)

    @property
    def bytes_alg(self) -> int:
        return bytes_alg(self.n_rows, self.n_cols, self.nnz)

    @property
    def kernel(self) -> str:
        """The dominant kernel the plan launches (rocprofv3 name, no template args)."""
        return self.params.get("kernel", "")

    def dims(self, stream=None) -> Dims:
        torch = _torch()
        dev = torch.device(self.device)
        if stream is None:
            stream = torch.cuda.current_stream(dev)
        return Dims(self.n_rows, self.n_cols, self.nnz, dev.index or 0, stream.cuda_stream)

    def run(self, x, y, stream=None) -> None:
        """y = A x on `stream` (default: torch's current stream)."""
        _check_vectors("run", x, self.n_cols, y, self.n_rows, self.device, types="x and y must be float64")
        lib = hip_lib()
        if self.plan is not None:
            _check(lib.spmv_plan_run(self.plan, _ptr(x), _ptr(y), _stream_handle(stream, self.device)),
                   f"spmv_plan_run ({self.fmt})")
            return
        a = self.arrays
        p = self.params
        d = self.dims(stream)
        if self.fmt == "csrf32" and p.get("variant") == 4:
            rc = lib.spmv_csr_f32v_run_tiled_hot(d, _ptr(a["row_ptr"]), _ptr(a["col"]), _ptr(a["val"]), _ptr(x),
                                                 _ptr(y), p["H"], _ptr(a.get("hot")), _ptr(a.get("own_lo")),
                                                 _ptr(a["ws"]), a["ws"].numel())
        elif self.fmt == "csrf32":
            rc = lib.spmv_csr_f32v_run_xwin(d, _ptr(a["row_ptr"]), _ptr(a["col"]), _ptr(a["val"]), _ptr(x), _ptr(y),
                                            p["lanes"], p.get("xwin_rows", 0), _ptr(a["win"]), p["xcap"])
        elif self.fmt == "csr16" and "win" in a:
            rc = lib.spmv_csr16_run_xwin(d, _ptr(a["row_ptr"]), _ptr(a["blk_base"]), _ptr(a["col_off"]),
                                         _ptr(a["col_esc"]), _ptr(a["val"]), _ptr(x), _ptr(y), p["lanes"],
                                         p.get("xwin_rows", 0), _ptr(a["win"]), p["xcap"])
        elif self.fmt == "csr16":
            rc = lib.spmv_csr16_run(d, _ptr(a["row_ptr"]), _ptr(a["blk_base"]), _ptr(a["col_off"]),
                                    _ptr(a["col_esc"]), _ptr(a["val"]), _ptr(x), _ptr(y), p["lanes"])
        elif self.fmt == "hyb" and p.get("H", 0) > 0:
            rc = lib.spmv_hyb_run_hot(d, p["K"], p["ld"], p["ki"], _ptr(a["ell_col"]), _ptr(a["ell_val"]),
                                      p["tail_nnz"], _ptr(a["tail_row"]), _ptr(a["tail_col"]), _ptr(a["tail_val"]),
                                      _ptr(x), _ptr(y), p["H"], _ptr(a["hot"]), _ptr(a["ws"]), a["ws"].numel())
        elif self.fmt == "hyb" and "win" in a:  # single-pass tail, or no tail (K = the longest row)
            rc = lib.spmv_hyb_run_tail_xwin(d, p["K"], p["ld"], p["ki"], _ptr(a["ell_col"]), _ptr(a["ell_val"]),
                                            p["tail_nnz"], _ptr(a["tail_row"]), _ptr(a["tail_col"]),
                                            _ptr(a["tail_val"]), _ptr(x), _ptr(y), _ptr(a.get("tails")),
                                            _ptr(a["win"]), p["xcap"])
        elif self.fmt == "hyb" and "tails" in a:
            rc = lib.spmv_hyb_run_tail(d, p["K"], p["ld"], p["ki"], _ptr(a["ell_col"]), _ptr(a["ell_val"]),
                                       p["tail_nnz"], _ptr(a["tail_row"]), _ptr(a["tail_col"]), _ptr(a["tail_val"]),
                                       _ptr(x), _ptr(y), _ptr(a["tails"]))
        elif self.fmt == "hyb":
            rc = lib.spmv_hyb_run(d, p["K"], p["ld"], p["ki"], _ptr(a["ell_col"]), _ptr(a["ell_val"]), p["tail_nnz"],
                                  _ptr(a["tail_row"]), _ptr(a["tail_col"]), _ptr(a["tail_val"]), _ptr(x), _ptr(y),
                                  _ptr(a["ws"]), a["ws"].numel())
        elif self.fmt == "csrg":
            rc = lib.spmv_csrg_run(d, p["groups"], p["n_pairs"], _ptr(a["pair_ptr"]), _ptr(a["col_g"]),
                                   _ptr(a["val_g"]), _ptr(a.get("own_lo")), _ptr(a["blk_off"]), _ptr(a["pair_row"]),
                                   _ptr(x), _ptr(y), _ptr(a["ws"]), a["ws"].numel())
        else:
            raise SpmvError(OTHER_ERROR, "run", f"format {self.fmt} has no plan and no entry point")
        _check(rc, f"spmv_{self.fmt}_run")

    def _plan_info(self, what: str, struct, mode_names: dict) -> dict:
        """The struct that spmv_plan_get_<what> fills, as a dict: mode by its
        name, kernel as a str, arrays as lists, every other field an int
        (reserved ones left out)."""
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, what, f"format {self.fmt} has no plan")
        info = struct()
        _check(getattr(hip_lib(), f"spmv_plan_get_{what}")(self.plan, ctypes.byref(info)), f"spmv_plan_get_{what}")
        out = {}
        for name, _ in struct._fields_:
            v = getattr(info, name)
            if name == "mode":
                out[name] = mode_names[v]
            elif name != "reserved":
                out[name] = v.decode() if isinstance(v, bytes) else int(v) if isinstance(v, int) else [int(e) for e in v]
        return out

    @property
    def multi_supported(self) -> bool:
        """run_multi can run this matrix (spmv_plan_multi_supported)."""
        return self.plan is not None and bool(hip_lib().spmv_plan_multi_supported(self.plan))

    def run_multi(self, X, Y, stream=None) -> None:
        """Y = A X on `stream` for k vectors stored row-major (spmv_plan_run_multi):
        X is (>= n_cols, k), Y is (>= n_rows, k), float64 on the matrix's
        device with inner stride 1; their row strides (>= k) are ldx and ldy,
        so column slices of wider tensors work.  Only Y[:n_rows, :k] is written."""
        k, ldx, ldy = _check_blocks("run_multi", X, self.n_cols, Y, self.n_rows, self.device)
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "run_multi", f"format {self.fmt} has no plan: no multi-vector run")
        st = _stream_handle(stream, self.device)
        _check(hip_lib().spmv_plan_run_multi(self.plan, k, _ptr(X), ldx, _ptr(Y), ldy, st),
               f"spmv_plan_run_multi ({self.fmt})")

    def prepare_multi(self, mode="balanced", long_len=None, seg_len=None) -> None:
        """The balanced mode of run_multi (and of run_t_multi in copy mode) for
        CSR matrices with long rows (spmv_plan_prepare_multi, build time):
        rows of more than long_len entries are cut into segments of seg_len
        entries with 16 entry lanes each; None = the library's rule.
        mode None frees everything: the unprepared run again."""
        if not isinstance(mode, (str, type(None))) or mode not in MULTI_MODES:
            raise SpmvError(OTHER_ERROR, "prepare_multi", 'mode must be "balanced" or None')
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "prepare_multi", f"format {self.fmt} has no plan: no multi-vector run")
        o = MultiOpts(-1 if long_len is None else int(long_len), -1 if seg_len is None else int(seg_len))
        _check(hip_lib().spmv_plan_prepare_multi(self.plan, MULTI_MODES[mode], ctypes.byref(o)),
               f"spmv_plan_prepare_multi ({self.fmt})")

    @property
    def multi_info(self) -> dict:
        """spmv_multi_info as a dict; mode is None or "balanced"."""
        return self._plan_info("multi_info", MultiInfo, _MULTI_MODE_NAMES)

    @property
    def transpose_supported(self) -> bool:
        """prepare_transpose / run_t can run this matrix (spmv_plan_transpose_supported)."""
        return self.plan is not None and bool(hip_lib().spmv_plan_transpose_supported(self.plan))

    def prepare_transpose(self, mode="scatter") -> None:
        """Build what run_t needs (spmv_plan_prepare_transpose, build time):
        "scatter" (no second copy of the matrix, fp64 atomics, not bitwise
        reproducible), "copy" (A^T built on the device and run by the forward
        kernels, reproducible) or None (free everything)."""
        if mode not in TRANSPOSE_MODES:
            raise SpmvError(OTHER_ERROR, "prepare_transpose", 'mode must be "scatter", "copy" or None')
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "prepare_transpose", f"format {self.fmt} has no plan: no transposed run")
        _check(hip_lib().spmv_plan_prepare_transpose(self.plan, TRANSPOSE_MODES[mode]),
               f"spmv_plan_prepare_transpose ({self.fmt})")

    @property
    def transpose_info(self) -> dict:
        """spmv_transpose_info as a dict; mode is None, "scatter" or "copy"."""
        return self._plan_info("transpose_info", TransposeInfo, _TRANSPOSE_MODE_NAMES)

    def run_t(self, x, y, stream=None) -> None:
        """y = A^T x on `stream` (spmv_plan_run_t): x has >= n_rows entries,
        y[:n_cols] is overwritten.  Needs prepare_transpose first."""
        _check_vectors("run_t", x, self.n_rows, y, self.n_cols, self.device)
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "run_t", f"format {self.fmt} has no plan: no transposed run")
        _check(hip_lib().spmv_plan_run_t(self.plan, _ptr(x), _ptr(y), _stream_handle(stream, self.device)),
               f"spmv_plan_run_t ({self.fmt})")

    @property
    def symmetric_supported(self) -> bool:
        """prepare_symmetric / run_sym can run this matrix (spmv_plan_symmetric_supported):
        a CSR plan over a square matrix."""
        return self.plan is not None and bool(hip_lib().spmv_plan_symmetric_supported(self.plan))

    def prepare_symmetric(self, mode="fused") -> None:
        """Build what run_sym needs (spmv_plan_prepare_symmetric, build time):
        "fused" (one pass over the stored half, no second copy, fp64 atomics,
        not bitwise reproducible), "expand" (A = S + S^T - diag S built on the
        device and run by the forward kernels, reproducible) or None (free
        everything)."""
        if mode not in SYMMETRIC_MODES:
            raise SpmvError(OTHER_ERROR, "prepare_symmetric", 'mode must be "fused", "expand" or None')
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "prepare_symmetric", f"format {self.fmt} has no plan: no symmetric run")
        _check(hip_lib().spmv_plan_prepare_symmetric(self.plan, SYMMETRIC_MODES[mode]),
               f"spmv_plan_prepare_symmetric ({self.fmt})")

    @property
    def symmetric_info(self) -> dict:
        """spmv_symmetric_info as a dict; mode is None, "fused" or "expand"."""
        return self._plan_info("symmetric_info", SymmetricInfo, _SYMMETRIC_MODE_NAMES)

    def symmetric_arrays(self):
        """Expand mode: host copies (row_ptr[n+1], col, val) of the CSR of A
        the plan built on the device (spmv_plan_get_symmetric_arrays)."""
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "symmetric_arrays", f"format {self.fmt} has no plan")
        lib = hip_lib()
        p_ptr, p_col, p_val, z = _vp(), _vp(), _vp(), _c_i64()
        _check(lib.spmv_plan_get_symmetric_arrays(self.plan, ctypes.byref(p_ptr), ctypes.byref(p_col),
                                                  ctypes.byref(p_val), ctypes.byref(z)),
               "spmv_plan_get_symmetric_arrays")
        out = (np.empty(self.n_rows + 1, np.int64), np.empty(z.value, np.int32), np.empty(z.value, np.float64))
        for host, dptr in zip(out, (p_ptr, p_col, p_val)):
            if host.nbytes:
                _check(lib.spmv_download(_ptr(host), dptr, host.nbytes, None), "spmv_download")
        return out

    def _not_square(self):
        """The symmetric runs' own refusal (for _check_*'s refuse), or None."""
        return None if self.n_rows == self.n_cols else "the matrix is not square"

    def run_sym(self, x, y, stream=None) -> None:
        """y = (S + S^T - diag S) x on `stream` (spmv_plan_run_sym), S the
        stored half this matrix holds: x has >= n entries, y[:n] is
        overwritten.  Needs prepare_symmetric first."""
        _check_vectors("run_sym", x, self.n_cols, y, self.n_rows, self.device, refuse=self._not_square())
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "run_sym", f"format {self.fmt} has no plan: no symmetric run")
        _check(hip_lib().spmv_plan_run_sym(self.plan, _ptr(x), _ptr(y), _stream_handle(stream, self.device)),
               f"spmv_plan_run_sym ({self.fmt})")

    @property
    def symmetric_multi_info(self) -> dict:
        """spmv_symmetric_multi_info as a dict (cap_cols, window_blocks and
        flush_entries are lists over the kernel widths 1, 2, 4, 8); mode as in
        symmetric_info."""
        return self._plan_info("symmetric_multi_info", SymmetricMultiInfo, _SYMMETRIC_MODE_NAMES)

    def run_sym_multi(self, X, Y, stream=None) -> None:
        """Y = (S + S^T - diag S) X on `stream` for k vectors stored row-major
        (spmv_plan_run_sym_multi), S the stored half this matrix holds: X and
        Y are (>= n, k), float64 on the matrix's device with inner stride 1;
        their row strides (>= k) are ldx and ldy.  Only Y[:n, :k] is written.
        Needs prepare_symmetric first."""
        k, ldx, ldy = _check_blocks("run_sym_multi", X, self.n_cols, Y, self.n_rows, self.device,
                                    refuse=self._not_square())
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "run_sym_multi", f"format {self.fmt} has no plan: no symmetric run")
        st = _stream_handle(stream, self.device)
        _check(hip_lib().spmv_plan_run_sym_multi(self.plan, k, _ptr(X), ldx, _ptr(Y), ldy, st),
               f"spmv_plan_run_sym_multi ({self.fmt})")

    @property
    def transpose_multi_info(self) -> dict:
        """spmv_transpose_multi_info as a dict (cap_cols and lds_blocks are
        lists over the kernel widths 1, 2, 4, 8); mode as in transpose_info."""
        return self._plan_info("transpose_multi_info", TransposeMultiInfo, _TRANSPOSE_MODE_NAMES)

    def run_t_multi(self, X, Y, stream=None) -> None:
        """Y = A^T X on `stream` for k vectors stored row-major
        (spmv_plan_run_t_multi): X is (>= n_rows, k), Y is (>= n_cols, k),
        float64 on the matrix's device with inner stride 1; their row strides
        (>= k) are ldx and ldy.  Only Y[:n_cols, :k] is written.  Needs
        prepare_transpose first."""
        k, ldx, ldy = _check_blocks("run_t_multi", X, self.n_rows, Y, self.n_cols, self.device)
        if self.plan is None:
            raise SpmvError(OTHER_ERROR, "run_t_multi", f"format {self.fmt} has no plan: no transposed run")
        st = _stream_handle(stream, self.device)
        _check(hip_lib().spmv_plan_run_t_multi(self.plan, k, _ptr(X), ldx, _ptr(Y), ldy, st),
               f"spmv_plan_run_t_multi ({self.fmt})")


# the library's A/B switches (include/spmv_ext.h; placement and load policy only)
OPTIONS = {"xwin_remap": 1, "xcd_remap": 2, "stream_nt": 3, "csr_col16": 5}


class BlockJacobi:
    """A block-Jacobi preconditioner resident in HBM (spmv_bjacobi_*,
    include/spmv_ext.h): the inverses of the bs x bs diagonal blocks, built on
    the device.  apply / apply_dot take row-major (>= n, k) float64 blocks
    with unit inner stride (a 1-D tensor is one column)."""

    def __init__(self, handle, device):
        self.handle = handle
        self.device = device
        self.n = self.info()["n"]

    @classmethod
    def from_coo(cls, m: Coo, bs: int, device="cuda:0", col_base: int = 0, symmetric_half: bool = False):
        """CSR on the host (file order inside a row), upload, create; the
        uploads are dropped: the object keeps only the inverse."""
        if not isinstance(bs, (int, np.integer)) or isinstance(bs, bool) or not 1 <= bs <= 16:
            raise SpmvError(OTHER_ERROR, "BlockJacobi.from_coo", f"bs must be an integer in 1..16, not {bs!r}")
        if col_base < 0:
            raise SpmvError(OTHER_ERROR, "BlockJacobi.from_coo", "col_base must be >= 0")
        lib = hip_lib()
        torch = _torch()
        dev = torch.device(device)
        ptr, col, val = csr_from_coo(m)
        d_ptr, d_col, d_val = (_dev_tensor(a, dev) for a in (ptr, col, val))
        d = Dims(m.n_rows, m.n_cols, m.nnz, dev.index or 0, torch.cuda.current_stream(dev).cuda_stream)
        handle = _vp()
        _check(lib.spmv_bjacobi_create(d, _ptr(d_ptr), _ptr(d_col), _ptr(d_val), int(bs), int(col_base),
                                       int(bool(symmetric_half)), ctypes.byref(handle)), "spmv_bjacobi_create")
        return cls(handle, dev)

    def __del__(self):
        handle, self.handle = getattr(self, "handle", None), None
        if handle is not None and _hip is not None and not sys.is_finalizing():
            _hip.spmv_bjacobi_destroy(handle)

    def info(self) -> dict:
        info = BjacobiInfo()
        _check(hip_lib().spmv_bjacobi_get_info(self.handle, ctypes.byref(info)), "spmv_bjacobi_get_info")
        out = {k: int(getattr(info, k)) for k in ("bs", "n", "n_blocks", "singular_blocks", "col_base", "owned_bytes")}
        out["symmetric_half"] = bool(info.symmetric_half)
        out["kernel"] = info.kernel.decode()
        return out

    def inverse(self):
        """A tensor copy of the inverse, (n_blocks * bs, bs)."""
        torch = _torch()
        i = self.info()
        host = np.empty((i["n_blocks"] * i["bs"], i["bs"]), np.float64)
        p = _vp()
        _check(hip_lib().spmv_bjacobi_inverse(self.handle, ctypes.byref(p)), "spmv_bjacobi_inverse")
        if host.size:  # the build synchronised: the inverse is complete
            with torch.cuda.device(self.device):
                _check(hip_lib().spmv_download(_ptr(host), p, host.nbytes, None), "download of the inverse")
        return torch.from_numpy(host).to(self.device)

    def _blocks(self, what, R, Z):
        torch = _torch()
        n = self.n
        for t in (R, Z):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or t.dim() not in (1, 2):
                raise SpmvError(OTHER_ERROR, what, "R and Z must be 1-D or 2-D float64 tensors")
            if t.dim() == 2 and t.shape[1] > 1 and t.stride(1) != 1:
                raise SpmvError(OTHER_ERROR, what, "R and Z need unit inner stride")
            if t.dim() == 1 and t.numel() > 1 and t.stride(0) != 1:
                raise SpmvError(OTHER_ERROR, what, "a 1-D R or Z must be contiguous")
            if t.shape[0] < n:
                raise SpmvError(OTHER_ERROR, what, "R or Z has too few rows")
            if not _on_device(t, self.device):
                raise SpmvError(OTHER_ERROR, what, f"R and Z must be on {self.device}")
        k = R.shape[1] if R.dim() == 2 else 1
        if (Z.shape[1] if Z.dim() == 2 else 1) != k or k < 1:
            raise SpmvError(OTHER_ERROR, what, "R and Z must have the same number k >= 1 of columns")
        return k, _ld(R, k), _ld(Z, k)  # a 1-D tensor of several entries is contiguous: its stride is k = 1

    def _stream(self, stream):
        return _stream_handle(stream, self.device)

    def apply(self, R, Z, stream=None) -> None:
        """Z = M^-1 R on `stream` (default: torch's current stream)."""
        k, ldr, ldz = self._blocks("BlockJacobi.apply", R, Z)
        _check(hip_lib().spmv_bjacobi_apply_multi(self.handle, k, _ptr(R), ldr, _ptr(Z), ldz, self._stream(stream)),
               "spmv_bjacobi_apply_multi")

    def apply_dot(self, R, Z, out, ws, stream=None) -> None:
        """Z = M^-1 R, out[:k] = column sums of R Z, out[k:2k] of R R; ws
        from ws(n, k)."""
        torch = _torch()
        k, ldr, ldz = self._blocks("BlockJacobi.apply_dot", R, Z)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_contiguous() or \
                out.numel() < 2 * k or out.device != R.device or ws.device != R.device:
            raise SpmvError(OTHER_ERROR, "BlockJacobi.apply_dot", "out must hold 2k float64 scalars on the device")
        _check(hip_lib().spmv_bjacobi_apply_dot_multi(self.handle, k, _ptr(R), ldr, _ptr(Z), ldz, _ptr(out), _ptr(ws),
                                                      ws.numel() * ws.element_size(), self._stream(stream)),
               "spmv_bjacobi_apply_dot_multi")

    def ws(self, n: int, k: int):
        torch = _torch()
        return torch.empty(hip_lib().spmv_bjacobi_ws_bytes(n, k), dtype=torch.uint8, device=self.device)

    def _cheb_args(self, what, a, b, R, AZ, D, Zin, Zout):
        """The checks of _blocks on every block of a Chebyshev step (AZ =
        None: step 0, Zin is then ignored); returns the C arguments from k to
        ldzout."""
        if AZ is None:
            Zin = None
        elif Zin is None:
            raise SpmvError(OTHER_ERROR, what, "a general step (AZ given) needs Zin")
        k, ldr, ldd = self._blocks(what, R, D)
        lds = {}
        for name, t in (("AZ", AZ), ("Zin", Zin), ("Zout", Zout)):
            lds[name] = 0 if t is None else self._blocks(what, R, t)[2]
        return (k, float(a), float(b), _ptr(R), ldr, _ptr(AZ), lds["AZ"], _ptr(D), ldd, _ptr(Zin), lds["Zin"],
                _ptr(Zout), lds["Zout"])

    def cheb_step(self, a, b, R, AZ, D, Zin, Zout, stream=None) -> None:
        """One step of the Chebyshev recurrence over M^-1
        (spmv_bjacobi_cheb_step_multi) on `stream`: AZ = None is step 0,
        D = Zout = b M^-1 R; otherwise D = a D + b M^-1 (R - AZ) and
        Zout = Zin + D.  Zout may be Zin itself."""
        args = self._cheb_args("BlockJacobi.cheb_step", a, b, R, AZ, D, Zin, Zout)
        _check(hip_lib().spmv_bjacobi_cheb_step_multi(self.handle, *args, self._stream(stream)),
               "spmv_bjacobi_cheb_step_multi")

    def cheb_step_dot(self, a, b, R, AZ, D, Zin, Zout, out, ws, stream=None) -> None:
        """cheb_step, and out[:k] = column sums of R Zout, out[k:2k] of R R; ws
        from ws(n, k)."""
        torch = _torch()
        args = self._cheb_args("BlockJacobi.cheb_step_dot", a, b, R, AZ, D, Zin, Zout)
        k = args[0]
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_contiguous() or \
                out.numel() < 2 * k or out.device != R.device or ws.device != R.device:
            raise SpmvError(OTHER_ERROR, "BlockJacobi.cheb_step_dot", "out must hold 2k float64 scalars on the device")
        _check(hip_lib().spmv_bjacobi_cheb_step_dot_multi(self.handle, *args, _ptr(out), _ptr(ws),
                                                          ws.numel() * ws.element_size(), self._stream(stream)),
               "spmv_bjacobi_cheb_step_dot_multi")


def set_option(name: str, value: int | None) -> None:
    """spmv_set_option: None / -1 = each kernel's default, 0 off, 1 on."""
    _check(hip_lib().spmv_set_option(OPTIONS[name], -1 if value is None else int(value)), f"set_option {name}")


def get_option(name: str) -> int:
    return int(hip_lib().spmv_get_option(OPTIONS[name]))


def _tri(v) -> int:
    """None -> -1 (the library's rule), else 0 / 1."""
    return -1 if v is None else int(bool(v))


def plan_opts(**kw) -> PlanOpts:
    """spmv_plan_opts with the library defaults, then the given fields."""
    o = PlanOpts()
    hip_lib().spmv_plan_opts_init(ctypes.byref(o))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


_PLAN_INFO_KEYS = ("lanes", "variant", "ki", "xcap", "xwin", "head", "single_pass", "index16", "split_T", "n_chunks",
                   "big_tiles", "head_bytes", "ws_bytes", "owned_bytes", "H")


def _attach_plan(dm: DeviceMatrix, what: str, create, *args, opts: PlanOpts) -> None:
    """Create the C plan of dm (spmv_plan_<fmt>) and copy its choices
    (spmv_plan_info) into dm.params."""
    plan = _vp()
    _check(create(dm.dims(), *args, ctypes.byref(opts), ctypes.byref(plan)), what)
    dm.plan = plan
    info = PlanInfo()
    _check(hip_lib().spmv_plan_get_info(plan, ctypes.byref(info)), "spmv_plan_get_info")
    for k in _PLAN_INFO_KEYS:
        dm.params[k] = int(getattr(info, k))
    dm.params["kernel"] = info.kernel.decode()
    dm.params["plan"] = info.desc.decode()


def plan_info(dm: DeviceMatrix) -> dict:
    """The plan's choices as a dict (the fields of spmv_plan_info)."""
    return {k: dm.params[k] for k in _PLAN_INFO_KEYS + ("kernel", "plan") if k in dm.params}


def _csr_xwin(dm: DeviceMatrix) -> None:
    """Per-row-group column windows for the x-window CSR kernel (the
    CSR16 / CSR-f32 formats of spmv_ext.h; CSR itself plans its own)."""
    torch = _torch()
    p, a = dm.params, dm.arrays
    rows = p.setdefault("xwin_rows", 0)
    nbytes = hip_lib().spmv_csr_xwin_bytes(dm.n_rows, dm.nnz, p["lanes"], rows)
    a["win"] = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dm.device)
    cap = _c_i32(0)
    _check(hip_lib().spmv_csr_xwin_build(dm.dims(), _ptr(a["row_ptr"]), _ptr(a["col"]), p["lanes"], rows,
                                         _ptr(a["win"]), a["win"].numel(), ctypes.byref(cap)), "spmv_csr_xwin_build")
    p["xcap"] = cap.value
    p["variant"] = 3


def _plan_coo(dm, row, col, val, *, xwin=None, coo_tail=None, hot=None):
    dm.arrays = dict(row=_dev_tensor(row, dm.device), col=_dev_tensor(col, dm.device), val=_dev_tensor(val, dm.device))
    o = plan_opts(xwin=_tri(xwin), coo_pass=_tri(coo_tail), H=-1 if hot is None else int(hot))
    a = dm.arrays
    _attach_plan(dm, "spmv_plan_coo", hip_lib().spmv_plan_coo, _ptr(a["row"]), _ptr(a["col"]), _ptr(a["val"]),
                 opts=o)
    dm.stored_bytes = 16 * dm.nnz


def _plan_csr(dm, *, lanes=0, variant=0, xwin=None, xwin_rows=0, hot=None, bigplan=True):
    a = dm.arrays
    o = plan_opts(lanes=int(lanes), variant=int(variant) if variant else -1, xwin=_tri(xwin), xwin_rows=int(xwin_rows),
                  bigplan=-1 if bigplan else 0, H=-1 if hot is None else int(hot))
    _attach_plan(dm, "spmv_plan_csr", hip_lib().spmv_plan_csr, _ptr(a["row_ptr"]), _ptr(a["col"]), _ptr(a["val"]),
                 opts=o)
    dm.params["xwin_rows"] = int(xwin_rows)
    dm.stored_bytes = 12 * dm.nnz + 8 * (dm.n_rows + 1)


def _plan_ell(dm, *, xwin=None):
    a, p = dm.arrays, dm.params
    _attach_plan(dm, "spmv_plan_ell", hip_lib().spmv_plan_ell, p["K"], p["ld"], p["ki"], _ptr(a["col"]), _ptr(a["val"]),
                 opts=plan_opts(xwin=_tri(xwin)))
    dm.stored_bytes = 12 * p["stored"]


def _plan_sell(dm, *, xwin=None, split=None, hot=None, head=None, index16=False):
    a, p = dm.arrays, dm.params
    o = plan_opts(xwin=_tri(xwin), split=-1 if split is None else int(split), H=-1 if hot is None else int(hot),
                  head=_tri(head), index16=int(bool(index16)))
    _attach_plan(dm, "spmv_plan_sell", hip_lib().spmv_plan_sell, p["C"], p["sigma"], p["ki"], p["n_slices"],
                 _ptr(a["slice_ptr"]), _ptr(a["perm"]), _ptr(a["col"]), _ptr(a["val"]), opts=o)
    per_slot = 10 if index16 else 12
    dm.stored_bytes = per_slot * p["stored"] + 8 * (p["n_slices"] + 1) + 4 * p["n_slices"] * p["C"]


def _plan_cmrs(dm, *, variant=None, xwin=None, hot=None):
    a, p = dm.arrays, dm.params
    v = -1 if variant is None else (1 if int(variant) == 0 else 2)  # python 0 strip runs / 1 tiles
    o = plan_opts(variant=v, xwin=_tri(xwin), H=-1 if hot is None else int(hot))
    _attach_plan(dm, "spmv_plan_cmrs", hip_lib().spmv_plan_cmrs, p["h"], p["n_strips"], _ptr(a["strip_ptr"]),
                 _ptr(a["row_in_strip"]), _ptr(a["col"]), _ptr(a["val"]), opts=o)
    dm.stored_bytes = 13 * dm.nnz + 8 * (p["n_strips"] + 1)


def _plan_bsr(dm, b, n_blocks, fill, *, lanes=0):
    """The C plan of a BSR matrix (spmv_plan_bsr): d.nnz is the stored values
    n_blocks * b * b, while dm.nnz stays the matrix's entries (bytes_alg)."""
    a = dm.arrays
    d = dm.dims()
    d.nnz = n_blocks * b * b
    n_brows = (dm.n_rows + b - 1) // b
    plan = _vp()
    _check(hip_lib().spmv_plan_bsr(d, b, n_brows, _ptr(a["brow_ptr"]), _ptr(a["bcol"]), _ptr(a["bval"]),
                                   ctypes.byref(plan_opts(lanes=int(lanes))), ctypes.byref(plan)), "spmv_plan_bsr")
    dm.plan = plan
    info = PlanInfo()
    _check(hip_lib().spmv_plan_get_info(plan, ctypes.byref(info)), "spmv_plan_get_info")
    for k in _PLAN_INFO_KEYS:
        dm.params[k] = int(getattr(info, k))
    dm.params.update(kernel=info.kernel.decode(), plan=info.desc.decode(), format=int(info.format), b=b,
                     n_brows=n_brows, n_blocks=n_blocks, fill=fill)
    dm.stored_bytes = 8 * n_blocks * b * b + 4 * n_blocks + 8 * (n_brows + 1)


def to_device(m: Coo, fmt: str, device="cuda:0", *, lanes: int = 0, variant: int = 0, ki: int = 0, C: int = 64,
              sigma: int = 1024, h: int = 8, ell_max_padding: float | None = 64.0,
              xwin: bool | None = None, xwin_rows: int = 0, split: int | None = None,
              cmrs_variant: int | None = None, hot: int | None = None,
              csr16_max_escape: float | None = 0.5, groups: int = 0, head: bool = True,
              sell_head: bool | None = None, coo_tail: bool | None = None, bigplan: bool = True,
              hyb_k: int = 0, block: int = 3, bsr_max_fill: float | None = None) -> DeviceMatrix:
    """Build `fmt` on the host (libspmv_host.so), upload it and, for the
    reference's five formats and SELL16, create its C plan (spmv.h): the
    library picks the kernel path — x windows in LDS (CSR, ELL, SELL, CMRS
    by default; COO opt-in), the entry-balanced tiles for skewed rows, the
    SELL head copy / split, the single-pass COO — exactly as ./bin/<fmt>.
    The keywords override its rules: xwin (None = the library's default),
    variant (CSR: 0 = the skew rule, 1-4 forced), cmrs_variant (None rule,
    0 strip runs, 1 tiles), split (SELL: None rule, 0 off, T), hot (None =
    the hot-column rule, 0 none, H forced), sell_head (None/True = the head
    copy where the small-matrix kernel runs), coo_tail (None = the single
    pass where the tail plan accepts the matrix, True = it or raise, False =
    the carry pass), bigplan (tiled CSR's big-tile plan), hyb_k (HYB's ELL
    width: 0 = spmv_hyb_plan's rule, K > 0 forced).
    fmt "bsr" (BLOCK_FORMATS): block CSR with block x block blocks (2, 3 or
    4) through spmv_plan_bsr; lanes = the lanes per block row (0 = the rule).
    bsr_max_fill: None = raise SpmvError, as ELL and CSR16 do, when the BSR
    arrays are not smaller than CSR's 12 nnz + 8 (n_rows + 1) bytes (a derived
    break-even, not a measured one); a float = refuse a fill (stored values /
    entries) above it; float("inf") = no check."""
    torch = _torch()
    device = torch.device(device)
    dm = DeviceMatrix(fmt, m.n_rows, m.n_cols, m.nnz, device)
    if fmt == "coo":
        row, col, val = coo_sort_by_row(m)
        _plan_coo(dm, row, col, val, xwin=xwin, coo_tail=coo_tail, hot=hot)
        return dm
    ptr, col, val = csr_from_coo(m)
    if fmt == "csr":
        dm.arrays = dict(row_ptr=_dev_tensor(ptr, device), col=_dev_tensor(col, device), val=_dev_tensor(val, device))
        _plan_csr(dm, lanes=lanes, variant=variant, xwin=xwin, xwin_rows=xwin_rows, hot=hot, bigplan=bigplan)
    elif fmt == "csrf32":
        # fp32 values, fp64 products and sums (§8f row 4): the row-group x-window
        # kernel, or for skewed rows the entry-balanced one with the hot table
        v = variant or host_lib().spmv_csr_pick_variant(m.n_rows, _ptr(ptr))
        dm.params = dict(lanes=lanes or hip_lib().spmv_csr_auto_lanes(m.n_rows, m.nnz), xwin_rows=xwin_rows,
                         variant=4 if v == 4 else 3, H=0)
        dm.arrays = dict(row_ptr=_dev_tensor(ptr, device), col=_dev_tensor(col, device),
                         val=_dev_tensor(val.astype(np.float32), device))
        dm.stored_bytes = 8 * m.nnz + 8 * (m.n_rows + 1)
        if v == 4:
            H, hot_cols, col_hot = hot_columns(m.n_cols, col, 0 if hot is None else hot) if hot != 0 else (0, None, col)
            dm.params["H"] = H
            if H > 0:
                dm.arrays["col"] = _dev_tensor(col_hot, device)
                dm.arrays["hot"] = _dev_tensor(hot_cols, device)
            dm.arrays["ws"] = torch.empty(hip_lib().spmv_csr_hot_ws_bytes(m.n_rows, m.nnz, H), dtype=torch.uint8,
                                          device=device)
            n_plan = hip_lib().spmv_csr_tiled_plan_len(m.nnz)
            if n_plan > 0:
                dm.arrays["own_lo"] = torch.empty(n_plan, dtype=torch.int32, device=device)
                _check(hip_lib().spmv_csr_tiled_plan(dm.dims(), _ptr(dm.arrays["row_ptr"]), _ptr(dm.arrays["own_lo"])),
                       "spmv_csr_tiled_plan")
        else:
            _csr_xwin(dm)
    elif fmt == "csr16":
        c = csr16_build(col)
        if csr16_max_escape is not None and c["n_esc"] > csr16_max_escape * max(c["n_blocks"], 1):
            # columns spread wider than 16 bits in most blocks (R-MAT): the
            # escapes store more than plain CSR; reported N/A like ELL padding
            raise SpmvError(OTHER_ERROR, "csr16_build", f"{c['n_esc']} of {c['n_blocks']} 64-entry blocks "
                            f"need 32-bit escapes (> {csr16_max_escape:.0%})")
        dm.params = dict(lanes=lanes or hip_lib().spmv_csr_auto_lanes(m.n_rows, m.nnz), n_blocks=c["n_blocks"],
                         n_esc=c["n_esc"])
        dm.arrays = dict(row_ptr=_dev_tensor(ptr, device), blk_base=_dev_tensor(c["blk_base"], device),
                         col_off=_dev_tensor(c["col_off"], device), col_esc=_dev_tensor(c["col_esc"], device),
                         val=_dev_tensor(val, device))
        dm.stored_bytes = 10 * m.nnz + 4 * c["n_blocks"] + 256 * c["n_esc"] + 8 * (m.n_rows + 1)
        if xwin is None or xwin:
            # windows of the x-window pipeline from the int32 columns (the
            # same values), uploaded only for the build
            dm.arrays["col"] = _dev_tensor(col, device)
            dm.params["xwin_rows"] = xwin_rows
            _csr_xwin(dm)
            dm.params.pop("variant", None)
            del dm.arrays["col"]
    elif fmt == "ell":
        ki = ki or 2  # measured best for ELL (profiles/round1_sweep.md)
        e = ell_build(m.n_rows, ptr, col, val, ki=ki, max_padding=ell_max_padding)
        dm.params = dict(K=e["K"], ld=e["ld"], ki=ki, stored=e["stored"])
        dm.arrays = dict(col=_dev_tensor(e["col"], device), val=_dev_tensor(e["val"], device))
        _plan_ell(dm, xwin=xwin)
    elif fmt in ("sell", "sell16"):
        # sell16: SELL-C-σ with 16-bit column offsets from each workgroup's
        # window base (§8f row 4), built by the plan on the device; refused
        # when a window spans > 65,536 columns (R-MAT), like csr16's escapes
        ki = ki or hip_lib().spmv_sell_auto_ki(m.n_rows, C)  # 1 (σ-window kernel) or 2 (small matrices)
        s = sell_build(m.n_rows, ptr, col, val, C=C, sigma=sigma, ki=ki)
        dm.params = dict(C=C, sigma=sigma, ki=ki, n_slices=s["n_slices"], stored=s["stored"])
        dm.arrays = dict(slice_ptr=_dev_tensor(s["slice_ptr"], device), perm=_dev_tensor(s["perm"], device),
                         col=_dev_tensor(s["col"], device), val=_dev_tensor(s["val"], device))
        if fmt == "sell":
            _plan_sell(dm, xwin=xwin, split=split, hot=hot, head=sell_head)
        else:
            _plan_sell(dm, xwin=True, split=0, hot=0, head=head, index16=True)
            del dm.arrays["col"]  # read at plan creation only: the runs read the plan's 16-bit offsets
    elif fmt == "csrg":
        # column-grouped CSR for gather-bound power-law matrices (R-MAT)
        # G = 4 measured best on the R-MAT (0.757-0.785 ms vs 0.768-0.83 at G = 8,
        # profiles/round3/rmat_tiled_r.log): more groups add pairs
        g = csrg_build(m.n_rows, ptr, col, val, groups=groups or 4)
        dm.params = dict(groups=g["groups"], n_pairs=g["n_pairs"])
        dm.arrays = {k: _dev_tensor(g[k], device) for k in ("pair_ptr", "col_g", "val_g", "blk_off")}
        dm.arrays["pair_row"] = _dev_tensor(g["pair_row"].view(np.int16), device)
        ws = hip_lib().spmv_csrg_ws_bytes(g["n_pairs"], m.nnz)
        dm.arrays["ws"] = torch.empty(max(ws, 16), dtype=torch.uint8, device=device)
        n_plan = hip_lib().spmv_csr_tiled_plan_len(m.nnz)
        if n_plan > 0:  # tile -> first pair table over the pair CSR, built once
            dm.arrays["own_lo"] = torch.empty(n_plan, dtype=torch.int32, device=device)
            pd = Dims(g["n_pairs"], m.n_cols, m.nnz, device.index or 0, torch.cuda.current_stream(device).cuda_stream)
            _check(hip_lib().spmv_csr_tiled_plan(pd, _ptr(dm.arrays["pair_ptr"]), _ptr(dm.arrays["own_lo"])),
                   "spmv_csr_tiled_plan")
        dm.stored_bytes = 12 * m.nnz + 10 * g["n_pairs"] + 4 * g["blk_off"].size
    elif fmt == "hyb":
        hb = hyb_build(m.n_rows, ptr, col, val, ki=ki or 2, K=hyb_k)
        dm.params = dict(K=hb["K"], ld=hb["ld"], ki=hb["ki"], tail_nnz=hb["tail_nnz"], stored=hb["stored"], H=0)
        if hot != 0:  # one table over the ELL and tail columns together
            ne, nt_ = hb["stored"], hb["tail_nnz"]
            both = np.concatenate([hb["ell_col"][:ne], hb["tail_col"][:nt_]])
            H, hot_cols, both_hot = hot_columns(m.n_cols, both, hot or 0)
            if H > 0:
                dm.params["H"] = H
                hb["ell_col"] = both_hot[:ne]
                hb["tail_col"] = np.concatenate([both_hot[ne:], np.zeros(max(1 - nt_, 0), np.int32)])
        ws = hip_lib().spmv_hyb_hot_ws_bytes(hb["tail_nnz"], dm.params["H"])
        dm.arrays = {k: _dev_tensor(hb[k], device) for k in ("ell_col", "ell_val", "tail_row", "tail_col", "tail_val")}
        dm.arrays["ws"] = torch.empty(max(ws, 16), dtype=torch.uint8, device=device)
        if dm.params["H"] > 0:
            dm.arrays["hot"] = _dev_tensor(hot_cols, device)
        elif hb["tail_nnz"] > 0 and coo_tail is not False:
            # single-pass tail (no carry pass) where every tail row ends
            # within 80 entries of its tile, as the COO format
            td = dm.dims()
            td.nnz = hb["tail_nnz"]
            tb = hip_lib().spmv_coo_tail_bytes(hb["tail_nnz"])
            tails = torch.empty(max(tb, 4), dtype=torch.uint8, device=device)
            rc = hip_lib().spmv_coo_tail_build(td, _ptr(dm.arrays["tail_row"]), _ptr(tails), tails.numel())
            if rc == SUCCESS:
                dm.arrays["tails"] = tails
                dm.params["single_pass"] = 1
            elif coo_tail:
                raise SpmvError(rc, "spmv_coo_tail_build (hyb tail)", hip_lib().spmv_last_error().decode())
        if (xwin is None or xwin) and ("tails" in dm.arrays or hb["tail_nnz"] == 0) and hb["stored"] > 0:
            # the ELL part through the x-window ELL kernel (same bits): one
            # cant-like matrix cold, a full ELL 12.26 vs 13.36 us (profiles/HISTORY.md §H9)
            a, p = dm.arrays, dm.params
            nbytes = hip_lib().spmv_ell_xwin_bytes(dm.n_rows)
            a["win"] = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
            cap = _c_i32(0)
            _check(hip_lib().spmv_ell_xwin_build(dm.dims(), p["K"], p["ld"], p["ki"], _ptr(a["ell_col"]),
                                                 _ptr(a["win"]), a["win"].numel(), ctypes.byref(cap)),
                   "spmv_ell_xwin_build (hyb)")
            p["xcap"] = cap.value
        dm.stored_bytes = 12 * hb["stored"] + 16 * hb["tail_nnz"]
        # the first (ELL) kernel; K = 0 runs the tail alone as COO
        dm.params["kernel"] = ("coo_staged_kernel" if hb["K"] == 0 else
                               "ell_xwin_kernel" if "win" in dm.arrays else "ell_kernel")
    elif fmt == "cmrs":
        c = cmrs_build(m.n_rows, ptr, h=h)
        dm.params = dict(h=h, n_strips=c["n_strips"])
        dm.arrays = dict(strip_ptr=_dev_tensor(c["strip_ptr"], device),
                         row_in_strip=_dev_tensor(c["row_in_strip"], device),
                         col=_dev_tensor(col, device), val=_dev_tensor(val, device))
        _plan_cmrs(dm, variant=cmrs_variant, xwin=xwin, hot=hot)
    elif fmt == "bsr":
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or block not in (2, 3, 4):
            raise SpmvError(OTHER_ERROR, "to_device", f"bsr: block must be 2, 3 or 4, not {block!r}")
        b = int(block)
        s = bsr_build(m.n_rows, m.n_cols, ptr, col, val, b)
        bsr_check_fill(m.n_rows, m.nnz, s, bsr_max_fill)
        dm.arrays = dict(brow_ptr=_dev_tensor(s["brow_ptr"], device), bcol=_dev_tensor(s["bcol"], device),
                         bval=_dev_tensor(s["bval"], device))
        _plan_bsr(dm, b, s["n_blocks"], s["fill"], lanes=lanes)
    else:
        raise SpmvError(OTHER_ERROR, "to_device", f"unknown format {fmt}")
    return dm


def device_build(m: Coo, fmt: str, device="cuda:0", *, lanes: int = 0, ki: int = 0, C: int = 64,
                 sigma: int = 1024, h: int = 8, xwin: bool | None = None, split: int | None = None,
                 cmrs_variant: int | None = None) -> DeviceMatrix:
    """Like to_device, but only the raw COO (file order) crosses PCIe: CSR,
    ELL, SELL and CMRS are built on the device by the spmv_dev_* builders
    (SURVEY.md §8f row 2); the arrays equal the host builders'.  The same C
    plans run them."""
    torch = _torch()
    device = torch.device(device)
    if fmt not in ("csr", "ell", "sell", "cmrs"):
        raise SpmvError(OTHER_ERROR, "device_build", "format must be csr, ell, sell or cmrs")
    lib = hip_lib()
    N, Z = m.n_rows, m.nnz
    d_row, d_col, d_val = (_dev_tensor(a, device) for a in (m.row, m.col, m.val))
    ptr = torch.empty(N + 1, dtype=torch.int64, device=device)
    col = torch.empty(max(Z, 1), dtype=torch.int32, device=device)
    val = torch.empty(max(Z, 1), dtype=torch.float64, device=device)
    dm = DeviceMatrix(fmt, N, m.n_cols, Z, device)
    d = dm.dims()
    _check(lib.spmv_dev_csr_from_coo(d, _ptr(d_row), _ptr(d_col), _ptr(d_val), _ptr(ptr), _ptr(col), _ptr(val)),
           "spmv_dev_csr_from_coo")
    del d_row, d_col, d_val
    if fmt == "csr":
        dm.arrays = dict(row_ptr=ptr, col=col, val=val)
        _plan_csr(dm, lanes=lanes, variant=3, xwin=xwin)
    elif fmt == "ell":
        ki = ki or 2
        K, ld = _c_i32(0), _c_i64(0)
        _check(lib.spmv_dev_ell_plan(d, _ptr(ptr), ki, ctypes.byref(K), ctypes.byref(ld)), "spmv_dev_ell_plan")
        stored = K.value * ld.value
        ec = torch.empty(max(stored, 1), dtype=torch.int32, device=device)
        ev = torch.empty(max(stored, 1), dtype=torch.float64, device=device)
        _check(lib.spmv_dev_ell_fill(d, _ptr(ptr), _ptr(col), _ptr(val), K.value, ld.value, ki, _ptr(ec), _ptr(ev)),
               "spmv_dev_ell_fill")
        dm.params = dict(K=K.value, ld=ld.value, ki=ki, stored=stored)
        dm.arrays = dict(col=ec, val=ev)
        _plan_ell(dm, xwin=xwin)
    elif fmt == "sell":
        ki = ki or hip_lib().spmv_sell_auto_ki(m.n_rows, C)  # as to_device
        ns = (N + C - 1) // C
        perm = torch.empty(max(ns * C, 1), dtype=torch.int32, device=device)
        sp = torch.empty(ns + 1, dtype=torch.int64, device=device)
        scol = torch.empty(max(ns, 1), dtype=torch.int32, device=device)
        stored = _c_i64(0)
        _check(lib.spmv_dev_sell_plan(d, _ptr(ptr), _ptr(col), C, sigma, ki, ns, _ptr(perm), _ptr(sp), _ptr(scol),
                                      ctypes.byref(stored)), "spmv_dev_sell_plan")
        sc = torch.empty(max(stored.value, 1), dtype=torch.int32, device=device)
        sv = torch.empty(max(stored.value, 1), dtype=torch.float64, device=device)
        _check(lib.spmv_dev_sell_fill(d, _ptr(ptr), _ptr(col), _ptr(val), C, ki, ns, _ptr(sp), _ptr(perm), _ptr(scol),
                                      _ptr(sc), _ptr(sv)), "spmv_dev_sell_fill")
        dm.params = dict(C=C, sigma=sigma, ki=ki, n_slices=ns, stored=stored.value)
        dm.arrays = dict(slice_ptr=sp, perm=perm, col=sc, val=sv)
        _plan_sell(dm, xwin=xwin, split=split)
    else:
        ns = (N + h - 1) // h
        stp = torch.empty(ns + 1, dtype=torch.int64, device=device)
        rin = torch.empty(max(Z, 1), dtype=torch.uint8, device=device)
        _check(lib.spmv_dev_cmrs_build(d, _ptr(ptr), h, _ptr(stp), _ptr(rin)), "spmv_dev_cmrs_build")
        dm.params = dict(h=h, n_strips=ns)
        dm.arrays = dict(strip_ptr=stp, row_in_strip=rin, col=col, val=val)
        _plan_cmrs(dm, variant=cmrs_variant, xwin=xwin)
    dm.arrays["row_ptr_csr"] = ptr
    return dm


def dev_csr_transpose(dm: DeviceMatrix):
    """A^T of a CSR DeviceMatrix as CSR, built on the device
    (spmv_dev_csr_transpose) -> (t_ptr[n_cols+1], t_col[nnz], t_val[nnz])
    device tensors, element for element csr_transpose's arrays."""
    torch = _torch()
    a = dm.arrays
    if dm.fmt != "csr" or not all(k in a for k in ("row_ptr", "col", "val")):
        raise SpmvError(OTHER_ERROR, "dev_csr_transpose", "needs a CSR DeviceMatrix")
    t_ptr = torch.empty(dm.n_cols + 1, dtype=torch.int64, device=dm.device)
    t_col = torch.empty(max(dm.nnz, 1), dtype=torch.int32, device=dm.device)
    t_val = torch.empty(max(dm.nnz, 1), dtype=torch.float64, device=dm.device)
    _check(hip_lib().spmv_dev_csr_transpose(dm.dims(), _ptr(a["row_ptr"]), _ptr(a["col"]), _ptr(a["val"]),
                                            _ptr(t_ptr), _ptr(t_col), _ptr(t_val)), "spmv_dev_csr_transpose")
    return t_ptr, t_col[: dm.nnz], t_val[: dm.nnz]


def banded_to_device(n: int, fmt: str, device="cuda:0", row_begin: int = 0, row_end: int | None = None,
                     seed: int = 2, C: int = 64, sigma: int = 1024, ki: int = 2, lanes: int = 0,
                     variant: int = 0, xwin: bool = True, xwin_rows: int = 0) -> DeviceMatrix:
    """Rows [row_begin, row_end) of the banded matrix (BASELINE.json
    configs[4]) generated directly in HBM by spmv_gen_banded_device, as CSR
    or SELL, run by its C plan (no hot-column table: the banded columns
    are uniform).  Row ids are local to the shard; columns are global (x is
    the full, replicated vector)."""
    torch = _torch()
    device = torch.device(device)
    row_end = n if row_end is None else row_end
    m = row_end - row_begin
    dm = DeviceMatrix(fmt, m, n, 16 * m, device)
    stream = torch.cuda.current_stream(device)
    if fmt == "csr":
        ptr = torch.empty(m + 1, dtype=torch.int64, device=device)
        col = torch.empty(16 * m, dtype=torch.int32, device=device)
        val = torch.empty(16 * m, dtype=torch.float64, device=device)
        rc = hip_lib().spmv_gen_banded_device(n, seed, row_begin, row_end, 0, 0, 0, _ptr(ptr), None, _ptr(col),
                                              _ptr(val), device.index or 0, stream.cuda_stream)
        _check(rc, "spmv_gen_banded_device")
        dm.arrays = dict(row_ptr=ptr, col=col, val=val)
        _plan_csr(dm, lanes=lanes, variant=variant, xwin=xwin, xwin_rows=xwin_rows, hot=0)
    elif fmt == "sell":
        ns = (m + C - 1) // C
        sp = torch.empty(ns + 1, dtype=torch.int64, device=device)
        perm = torch.empty(ns * C, dtype=torch.int32, device=device)
        col = torch.empty(ns * C * 16, dtype=torch.int32, device=device)
        val = torch.empty(ns * C * 16, dtype=torch.float64, device=device)
        rc = hip_lib().spmv_gen_banded_device(n, seed, row_begin, row_end, 1, C, ki, _ptr(sp), _ptr(perm),
                                              _ptr(col), _ptr(val), device.index or 0, stream.cuda_stream)
        _check(rc, "spmv_gen_banded_device")
        dm.params = dict(C=C, sigma=sigma, ki=ki, n_slices=ns, stored=ns * C * 16)
        dm.arrays = dict(slice_ptr=sp, perm=perm, col=col, val=val)
        _plan_sell(dm, xwin=xwin, split=0, hot=0)
    else:
        raise SpmvError(OTHER_ERROR, "banded_to_device", "format must be csr or sell")
    return dm


def read_bin(path) -> Coo:
    """Binary cache written by write_bin / the drivers' --cache."""
    lib = host_lib()
    info = MtxInfo()
    p = str(path).encode()
    _check_host(lib.spmv_bin_read_info(p, ctypes.byref(info)), f"read {path}")
    row = np.empty(info.nnz, np.int32)
    col = np.empty(info.nnz, np.int32)
    val = np.empty(info.nnz, np.float64)
    _check_host(lib.spmv_bin_read(p, ctypes.byref(info), _ptr(row), _ptr(col), _ptr(val)), f"read {path}")
    return Coo(info.n_rows, info.n_cols, row, col, val, bool(info.symmetric), str(path))


def write_bin(path, m: Coo) -> None:
    info = MtxInfo(m.n_rows, m.n_cols, m.nnz, int(m.symmetric), 0, 0)
    _check_host(host_lib().spmv_bin_write(str(path).encode(), ctypes.byref(info), _ptr(m.row), _ptr(m.col),
                                          _ptr(m.val)), f"write {path}")


def flush_cache(stream=None, nbytes: int = 0) -> None:
    """Evict the 256 MiB Infinity Cache + L2s (512 MiB scratch write)."""
    torch = _torch()
    s = stream if stream is not None else torch.cuda.current_stream()
    _check(hip_lib().spmv_flush_cache(s.cuda_stream, nbytes), "spmv_flush_cache")


def device_name(device: int = 0) -> str:
    buf = ctypes.create_string_buffer(256)
    _check(hip_lib().spmv_device_name(device, buf, 256), "spmv_device_name")
    return buf.value.decode()
