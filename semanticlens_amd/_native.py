"""ctypes binding of ``libsemanticlens_hip.so`` (C ABI: ``include/semanticlens_amd.h``).

This is the only module that talks to the native library.  There is NO CPU
fallback: if the library is missing, or a tensor cannot be placed on a HIP
device, the call raises.  PyTorch is used for device memory and streams only
(``tensor.data_ptr()`` / ``torch.cuda.current_stream()``).
"""
from __future__ import annotations

import ctypes
import math
import operator
import os
from collections import namedtuple
from pathlib import Path

import torch

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / "lib" / "libsemanticlens_hip.so"

# enums of include/semanticlens_amd.h
SL_F32, SL_F16, SL_BF16 = 0, 1, 2
SL_CONV_MAX, SL_CONV_MEAN, SL_CONV_SUM = 0, 1, 2
SL_TOK_MEAN, SL_TOK_ABSMEAN, SL_TOK_MAX, SL_TOK_ABSMAX, SL_TOK_TOKEN = 0, 1, 2, 3, 4
SL_TIES_TOTAL, SL_TIES_ATEN = 0, 1
SL_MAX_SLOTS = 16
SL_PROF_REDUCE, SL_PROF_MERGE, SL_PROF_GEMM, SL_PROF_GATHER, SL_PROF_SCORES, SL_PROF_BATCHNORM, SL_PROF_TOPK = 0, 1, 2, 3, 4, 5, 6
SL_PROF_SOFTMAX = 7
SL_ACT_NONE, SL_ACT_GELU, SL_ACT_QUICKGELU, SL_ACT_GELU_TANH = 0, 1, 2, 3
TIE_MODES = {"total": SL_TIES_TOTAL, "aten": SL_TIES_ATEN}
SL_PP_PLAN_STRIDE = 16
PP_RESIZE_MODES = {"shortest": 0, "squash": 1}
PP_INTERP = {"bicubic": 0, "bilinear": 1}
SL_RENDER_CROP, SL_RENDER_OPAQUE, SL_RENDER_LIGHTEN = 0, 1, 2
RENDER_STYLES = {"crop": SL_RENDER_CROP, "opaque": SL_RENDER_OPAQUE, "lighten": SL_RENDER_LIGHTEN}

_DTYPES = {torch.float32: SL_F32, torch.float16: SL_F16, torch.bfloat16: SL_BF16}

_i64 = ctypes.c_int64
_vp = ctypes.c_void_p
_int = ctypes.c_int
_sz = ctypes.c_size_t

# name -> (restype, argtypes); must list every symbol include/semanticlens_amd.h declares
SIGNATURES = {
    "sl_last_error": (ctypes.c_char_p, []),
    "sl_abi_version": (_int, []),
    "sl_device_count": (_int, []),
    "sl_reduce_conv": (_int, [_vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "sl_reduce_tokens": (_int, [_vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _i64, _vp, _vp, _vp]),
    "sl_reduce_conv_p": (_int, [_vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp, _i64, _i64]),
    "sl_reduce_tokens_p": (_int, [_vp, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _i64, _vp, _vp, _vp, _i64, _i64]),
    "sl_actmax_init": (_int, [_vp, _vp, _i64, _i64, _vp]),
    "sl_actmax_merge": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _int, _vp]),
    "sl_actmax_update": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _int, _vp, _sz, _vp]),
    "sl_actmax_aten_ws_bytes": (_sz, [_i64, _i64, _i64]),
    "sl_actmax_update_multi": (_int, [_vp, _vp, _vp, _vp, _vp, _int, _i64, _i64, _vp]),
    "sl_actmax_update_multi_supported": (_int, [_i64, _i64, _i64]),
    "sl_aten_topk_order_host": (_int, [_vp, _i64, _i64, _vp]),
    "sl_set_option": (_int, [ctypes.c_char_p, _i64]),
    "sl_get_option": (_i64, [ctypes.c_char_p]),
    "sl_reduce_conv_multi": (_int, [_vp, _int, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _vp, _vp]),
    "sl_reduce_tokens_multi": (_int, [_vp, _int, _int, _i64, _i64, _i64, _i64, _i64, _i64, _int, _i64, _vp, _vp]),
    "sl_actmax_merge_states": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "sl_comm_unique_id": (_int, [_vp]),
    "sl_comm_init_from_unique_id": (_int, [_vp, _int, _int, ctypes.POINTER(_vp)]),
    "sl_comm_destroy": (_int, [_vp]),
    "sl_comm_info": (_int, [_vp, ctypes.POINTER(_int), ctypes.POINTER(_int), ctypes.POINTER(_int)]),
    "sl_comm_allgather": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "sl_comm_allreduce": (_int, [_vp, _vp, _i64, _int, _int, _vp]),
    "sl_actmax_packed_bytes": (_sz, [_int, _vp, _i64]),
    "sl_actmax_pack": (_int, [_int, _vp, _vp, _vp, _i64, _vp, _vp]),
    "sl_actmax_merge_packed": (_int, [_int, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp]),
    "sl_actmax_allgather_merge_ws_bytes": (_sz, [_int, _vp, _i64, _int]),
    "sl_actmax_allgather_merge": (_int, [_vp, _int, _vp, _vp, _vp, _i64, _vp, _sz, _vp]),
    "sl_gather_rows": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp]),
    "sl_gather_rows_shard": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "sl_similarity": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp, _sz, _vp]),
    "sl_similarity_ws_bytes": (_sz, [_i64, _i64, _i64, _i64]),
    "sl_set_gemm_mode": (_int, [_int]),
    "sl_set_reduce_policy": (_int, [_i64, _i64]),
    "sl_abs_norm_rows": (_int, [_vp, _i64, _i64, ctypes.c_float, _vp]),
    "sl_similarity_multi": (_int, [_vp, _i64, _i64, _vp, _vp, _int, _vp, _vp, _sz, _vp]),
    "sl_similarity_multi_ws_bytes": (_sz, [_i64, _i64, _vp, _int]),
    "sl_clarity": (_int, [_vp, _i64, _i64, _i64, _vp, _vp]),
    "sl_clarity_multi": (_int, [_vp, _vp, _int, _i64, _i64, _vp, _vp]),
    "sl_redundancy": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _sz, _vp]),
    "sl_redundancy_ws_bytes": (_sz, [_i64, _i64, _i64]),
    "sl_template_mean": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "sl_poly2means": (_int, [_vp, _i64, _i64, _i64, _vp, _int, _vp, _int, _vp, _vp, _vp, _sz, _vp]),
    "sl_poly2means_ws_bytes": (_sz, [_i64, _i64, _i64]),
    "sl_kmeans_trials": (_int, [_int]),
    "sl_polykmeans": (_int, [_vp, _i64, _i64, _i64, _int, _vp, _int, _vp, _int, _vp, _vp, _vp, _sz, _vp]),
    "sl_polykmeans_ws_bytes": (_sz, [_i64, _i64, _i64, _int, _int]),
    "sl_poly2means_labels": (_int, [_vp, _i64, _i64, _i64, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sl_polykmeans_labels": (_int, [_vp, _i64, _i64, _i64, _int, _vp, _int, _vp, _int, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sl_facet_stats": (_int, [_vp, _i64, _i64, _i64, _vp, _int, _vp, _vp, _vp, _vp]),
    "sl_silhouette_ws_bytes": (_sz, [_i64, _i64, _i64]),
    "sl_silhouette": (_int, [_vp, _i64, _i64, _i64, _vp, _int, _int, _int, _vp, _vp, _vp, _sz, _vp]),
    "sl_linear": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _int, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "sl_layernorm": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, ctypes.c_float, _vp, _vp, _i64, _vp]),
    "sl_attention": (_int, [_vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "sl_attention_bf16x3": (_int, [_vp, _i64, _i64, _i64, _i64, _int, _vp, _vp, _vp]),
    "sl_patchify": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _vp]),
    "sl_attention_pool": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "sl_attention_pool_q": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp]),
    "sl_tokens_from_map": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "sl_split_elems": (_sz, [_i64, _i64]),
    "sl_split_bf16": (_int, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "sl_linear_bf16x3": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _int, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "sl_broadcast_row": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "sl_embed_tokens": (_int, [_vp, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "sl_preprocess_plan": (_int, [_vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    "sl_preprocess": (_int, [_vp, _vp, _i64, _int, _int, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sl_render_ws_bytes": (_sz, [_i64, _i64, _i64]),
    "sl_render_heatmaps": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _int, ctypes.c_float, ctypes.c_float, ctypes.c_double, _int, _int,
                                  _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "sl_condition_init": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _int, _vp, _i64, _i64, _i64, _vp]),
    "sl_preprocess_plan_rois": (_int, [_vp, _vp, _i64, _vp, _vp, _i64, _int, _int, _int, _vp, _vp]),
    "sl_activation_heat_boxes": (_int, [_vp, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _int,
                                        ctypes.c_float, _vp, _vp, _vp, _sz, _vp]),
    "sl_heat_boxes": (_int, [_vp, _i64, _i64, _i64, _int, ctypes.c_float, _vp, _vp, _sz, _vp]),
    "sl_batchnorm_infer": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_double, _int, _vp, _vp]),
    "sl_batchnorm_infer_add_relu": (_int, [_vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_double, _vp, _vp]),
    "sl_batchnorm_infer_add_bn_relu": (_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _i64, _i64,
                                              _i64, _vp, _vp]),
    "sl_batchnorm_infer_relu_maxpool": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _vp, _vp, _vp, ctypes.c_double, _int, _int, _int,
                                               _int, _int, _int, _vp, _vp]),
    "sl_conv1x1_64_256": (_int, [_vp, _vp, _i64, _i64, _int, _vp, _vp, _vp]),
    "sl_conv1x1_bn_add_relu": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _vp, _i64, _i64, _vp, _vp]),
    "sl_conv1x1_bn_add_conv1x1_bn_relu": (_int, [_vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp,
                                                 ctypes.c_double, _i64, _i64, _vp, _vp]),
    "sl_topk_init": (_int, [_vp, _vp, _i64, _i64, _vp]),
    "sl_topk_merge": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _sz, _vp]),
    "sl_topk_merge_biased": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _sz, _vp]),
    "sl_topk_merge_ws_bytes": (_sz, [_i64, _i64, _i64]),
    "sl_topk_merge_states": (_int, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp]),
    "sl_softmax_init": (_int, [_vp, _i64, _vp]),
    "sl_softmax_merge": (_int, [_vp, _i64, _vp, _i64, _i64, ctypes.c_double, _vp, _sz, _vp]),
    "sl_softmax_merge_ws_bytes": (_sz, [_i64, _i64]),
    "sl_softmax_finish": (_int, [_vp, _i64, ctypes.c_double, _vp, _i64, _vp, _vp, _vp, _vp]),
    "sl_rank_merge": (_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "sl_rank_merge_splits": (_i64, [_i64, _i64]),
    "sl_omp_init": (_int, [_vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "sl_omp_step": (_int, [_vp, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _i64, _i64, ctypes.c_double, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                           _vp, _vp, _vp, _vp]),
    "sl_mutualmax_merge": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _i64, _vp]),
    "sl_mutualmax_finish": (_int, [_vp, _i64, _vp, _vp, _vp]),
    "sl_segmax_merge": (_int, [_vp, _i64, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp]),
    "sl_unionfind_init": (_int, [_vp, _vp, _vp, _i64, _vp]),
    "sl_threshold_union_merge": (_int, [_vp, _vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, ctypes.c_float, _vp]),
    "sl_unionfind_flatten": (_int, [_vp, _i64, _vp, _vp]),
    "sl_group_min_merge": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _vp]),
    "sl_group_min_finish": (_int, [_vp, _vp, _i64, _vp, _vp]),
    "sl_cosine_nt": (_int, [_vp, _i64, _vp, _i64, _i64, _vp, _vp, _sz, _vp]),
    "sl_cosine_nt_ws_bytes": (_sz, [_i64, _i64, _i64]),
    "sl_prof_enable": (_int, [_int]),
    "sl_prof_reset": (_int, []),
    "sl_prof_read": (_int, [_int, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_i64), ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


class NativeLibraryError(RuntimeError):
    """The HIP library is missing or a native call failed."""


def lib():
    """Load (once) and return the native library; raise loudly if it is not built."""
    global _lib
    if _lib is None:
        path = Path(os.environ.get("SEMANTICLENS_AMD_LIB", LIB_PATH))
        if not path.exists():
            raise NativeLibraryError(
                f"{path} not found. semanticlens_amd has no CPU fallback: build the HIP library first "
                "(python -c 'import __graft_entry__ as g; g.build()' or make -C semanticlens_amd/csrc)."
            )
        handle = ctypes.CDLL(str(path))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if the library lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def _check(rc: int, what: str) -> int:
    if rc < 0:
        msg = lib().sl_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(msg or f"{what}: invalid argument")
        raise NativeLibraryError(f"{what} failed ({rc}): {msg}")
    return rc


def default_device() -> torch.device:
    """The HIP device native state lives on.  Raises when there is none (no CPU fallback)."""
    if not torch.cuda.is_available():
        raise NativeLibraryError(
            "semanticlens_amd needs a HIP device (MI355X): torch.cuda.is_available() is False and there is "
            "no CPU fallback for the concept-DB hot path."
        )
    return torch.device("cuda", torch.cuda.current_device())


def resolve_device(device=None) -> torch.device:
    """``device`` with its index filled in: ``"cuda"`` means the CURRENT device (the usual pattern after
    ``torch.cuda.set_device(rank)``), so that ``tensor.device == resolve_device(...)`` holds for tensors living there."""
    if device is None:
        return default_device()
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        return default_device()
    return dev


def to_device(t: torch.Tensor, device: torch.device | None = None) -> torch.Tensor:
    """Place ``t`` on a HIP device (host->device copies are plumbing, not compute)."""
    if t.is_cuda:
        return t
    return t.to(device or default_device())


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream(t: torch.Tensor):
    """torch's current stream on the tensor's device as a raw ``hipStream_t`` (every kernel is enqueued on it)."""
    if _raw_stream is not None:  # 0.2 us; the Stream object route costs 1.8 of a call's ~9 us on the host
        return _vp(_raw_stream(t.device.index))
    return _vp(torch.cuda.current_stream(t.device).cuda_stream)


class _NoGuard:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_GUARD = _NoGuard()


def _on(device: torch.device):
    """Device guard for a native call: nothing to do when ``device`` is already current (the usual case; saves 1.2 us)."""
    if device.index is None or torch.cuda.current_device() == device.index:
        return _NO_GUARD
    return torch.cuda.device(device)


def _ptr(t: torch.Tensor | None):
    return _vp(t.data_ptr()) if t is not None and t.numel() > 0 else _vp(None)


def _need_f32(what: str, *tensors):
    """The encoder entry points take raw fp32 device pointers: refuse anything else instead of reinterpreting its bytes."""
    for t in tensors:
        if t is not None and (t.dtype != torch.float32 or not t.is_cuda):
            raise TypeError(f"{what}: expected float32 tensors on a HIP device, got {t.dtype} on {t.device}")


def _dtype_code(t: torch.Tensor) -> int:
    try:
        return _DTYPES[t.dtype]
    except KeyError:
        raise TypeError(f"activation dtype {t.dtype} is not supported (float32, float16, bfloat16)") from None


# ------------------------------------------------------------------------------------------------
# K1 / K2
# ------------------------------------------------------------------------------------------------
def _flatten_spatial(x: torch.Tensor):
    """(B,C,H,W) -> strides (sb, sc, ss) of the (B,C,H*W) view, making a copy only if H,W cannot merge.  The stride of a
    size-1 dimension carries no information (torch keeps whatever the view had), so it is never used."""
    B, C, H, W = x.shape
    sb, sc, sh, sw = x.stride()
    if H == 1:
        return x, sb, sc, sw
    if W == 1:
        return x, sb, sc, sh
    if sh != W * sw:
        x = x.contiguous()
        return x, C * H * W, H * W, 1
    return x, sb, sc, sw


def _policy_args(policy):
    """``(nt_min_bytes, tail_bytes)`` -> the two trailing arguments of ``sl_reduce_*_p``; ``None`` (the pair or an entry) = -1, the
    process default."""
    nt_min, tail = policy if policy is not None else (None, None)
    return -1 if nt_min is None else int(nt_min), -1 if tail is None else int(tail)


def reduce_conv(x: torch.Tensor, agg: int, cand: torch.Tensor | None, out_f32: torch.Tensor | None, policy=None):
    """Launch K1 on a 4-D device tensor.  ``cand`` (B,C) bf16 and/or ``out_f32`` (B,C) f32 are filled.  ``policy``: the cache
    policy of this call, ``(nt_min_bytes, tail_bytes)``; ``None`` entries take the process default (:func:`set_reduce_policy`)."""
    assert x.is_cuda and x.ndim == 4
    B, C, H, W = x.shape
    x, sb, sc, ss = _flatten_spatial(x)
    with _on(x.device):
        rc = lib().sl_reduce_conv_p(_ptr(x), _dtype_code(x), B, C, H * W, sb, sc, ss, agg, _ptr(cand), _ptr(out_f32), _stream(x),
                                    *_policy_args(policy))
    _check(rc, "sl_reduce_conv_p")


def abs_norm_rows(x: torch.Tensor, eps: float = 1e-10) -> torch.Tensor:
    """In place on a contiguous (B, C) fp32 device tensor: ``x[b] /= x[b].abs().sum() + eps`` (the relevance visualizer's
    ``abs_norm``)."""
    assert x.is_cuda and x.ndim == 2 and x.dtype == torch.float32 and x.is_contiguous()
    with _on(x.device):
        _check(lib().sl_abs_norm_rows(_ptr(x), x.shape[0], x.shape[1], float(eps), _stream(x)), "sl_abs_norm_rows")
    return x


def reduce_tokens(x: torch.Tensor, agg: int, pos: int, cand: torch.Tensor | None, out_f32: torch.Tensor | None, policy=None):
    """Launch K2 on a 3-D device tensor (B,T,F).  ``policy``: as for :func:`reduce_conv`."""
    assert x.is_cuda and x.ndim == 3
    B, T, F = x.shape
    sb, st, sf = x.stride()
    with _on(x.device):
        rc = lib().sl_reduce_tokens_p(
            _ptr(x), _dtype_code(x), B, T, F, sb, st, sf, agg, pos, _ptr(cand), _ptr(out_f32), _stream(x), *_policy_args(policy)
        )
    _check(rc, "sl_reduce_tokens_p")


def reduce_multi(kind: str, xs: list[torch.Tensor], agg: int, pos: int, cand: torch.Tensor):
    """K1 / K2 over ``L`` device tensors of ONE shape, strides and dtype into ``cand`` ``(L, B, C)`` bf16: one launch when the
    component axis is contiguous (``sl_reduce_*_multi``)."""
    x0 = xs[0]
    L = len(xs)
    assert all(x.is_cuda and x.shape == x0.shape and x.stride() == x0.stride() and x.dtype == x0.dtype for x in xs)
    assert cand.is_contiguous() and cand.dtype == torch.bfloat16 and cand.shape[0] == L
    if kind == "conv":
        flat = [_flatten_spatial(x) for x in xs]  # identical strides: the same answer (view or copy) for every tensor
        xs = [f[0] for f in flat]
        sb, sc, ss = flat[0][1:]
    ptrs = (_vp * L)(*[x.data_ptr() for x in xs])
    with _on(x0.device):
        if kind == "conv":
            B, C = x0.shape[:2]
            S = x0.shape[2] * x0.shape[3]
            rc = lib().sl_reduce_conv_multi(ptrs, L, _dtype_code(x0), B, C, S, sb, sc, ss, agg, _ptr(cand), _stream(x0))
            _check(rc, "sl_reduce_conv_multi")
        else:
            B, T, F = x0.shape
            sb, st, sf = x0.stride()
            rc = lib().sl_reduce_tokens_multi(ptrs, L, _dtype_code(x0), B, T, F, sb, st, sf, agg, pos, _ptr(cand), _stream(x0))
            _check(rc, "sl_reduce_tokens_multi")


_policy_explicit = False  # the caller chose a cache policy (set_reduce_policy or the environment): the tuner keeps out


def set_reduce_policy(nt_min_bytes: int | None = None, tail_bytes: int | None = None):
    """Process default of the K1 / K2 cache policy (include/semanticlens_amd.h ``sl_set_reduce_policy``), for reduce calls that
    pass no ``policy``: ``(0, 0)`` reads everything with the read-once policy (cold inputs), ``None`` restores the built-in
    default (inputs just written by the previous kernel).  An explicit choice also switches the per-layer
    :class:`ReducePolicyTuner` of the collect hooks off."""
    global _policy_explicit
    _policy_explicit = nt_min_bytes is not None or tail_bytes is not None
    _check(lib().sl_set_reduce_policy(*_policy_args((nt_min_bytes, tail_bytes))), "sl_set_reduce_policy")


def reduce_policy_is_explicit() -> bool:
    return _policy_explicit or "SL_NT_MIN_BYTES" in os.environ or "SL_REDUCE_TAIL_MB" in os.environ


class ReducePolicyTuner:
    """Which cache policy a hooked layer's reduce should read its input with — measured, per layer, on the first batches.

    The reduce kernels cannot know their producer.  The library default (inputs below 256 MiB and the last 240 MiB of larger
    ones with the default policy, the head read-once) is what a layer ending in an IN-PLACE activation wants (torchvision's
    Bottleneck: the whole output was just re-written, so the Infinity Cache holds its tail).  A layer whose output comes out of
    a residual ADD of two other tensors (transformer blocks, ConvNeXt) streamed three times its size through that cache: only
    ~80 MB of the output's tail are still there, and reading 240 MiB with the default policy thrashes (ConvNeXt-L's stage
    outputs: 0.625 of spec with the default, 0.693 with an 80 MiB tail; ViT-B/16's 155 MB block outputs 0.718 -> 0.742 with
    nt from 96 MiB: ``profiles/r04_reduce_policy_sweep.txt``).  So each layer tries the candidates on its first launches (one untimed +
    ``TRIALS`` timed each, HIP events read back only once they have completed: no synchronisation) and keeps the faster;
    results do not depend on the policy.  The policy is an argument of each launch: the tuner writes no process state, so
    collectors on several threads or streams do not see each other's candidates.  Off when the caller chose a policy
    (``set_reduce_policy`` / ``SL_NT_MIN_BYTES`` / ``SL_REDUCE_TAIL_MB``) or with ``SL_REDUCE_AUTOTUNE=0``; inputs below 96 MiB are
    never tuned."""

    # (nt_min_bytes, tail_bytes); None = the library default.  Round 5: behind a three-stream residual add the 617 MB ConvNeXt-L
    # stage reads 0.690 with an 80 MiB tail and 0.715 with 128 MiB (profiles/r05_k2_producer_lab.txt): a third candidate
    CANDIDATES = ((None, None), (96 << 20, 80 << 20), (96 << 20, 128 << 20))
    MIN_BYTES = 96 << 20
    TRIALS = 3

    def __init__(self):
        self.choice = None
        self._key = None
        self._calls = 0
        self._samples = [[] for _ in self.CANDIDATES]
        self._pending = []

    @staticmethod
    def enabled() -> bool:
        return os.environ.get("SL_REDUCE_AUTOTUNE", "1") != "0" and not reduce_policy_is_explicit()

    def run(self, launch, nbytes: int, batch: int):
        """``launch(policy)`` enqueues the reduce on the current stream with that cache policy (``reduce_conv`` /
        ``reduce_tokens``'s ``policy``): the candidate or the chosen one, ``None`` where the tuner keeps out."""
        if nbytes < self.MIN_BYTES or batch <= 0 or not self.enabled():
            return launch(None)
        key = nbytes // batch
        if key != self._key:  # another layer shape behind the same hook: start over
            self.__init__()
            self._key = key
        if self.choice is not None:
            return launch(self.CANDIDATES[self.choice] if self.choice else None)
        idx = self._calls % len(self.CANDIDATES)
        timed = self._calls >= len(self.CANDIDATES)  # the first launch of each candidate also pays first-use costs
        self._calls += 1
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = launch(self.CANDIDATES[idx])
        e1.record()
        if timed:
            self._pending.append((idx, e0, e1, nbytes))
        self._harvest()
        return out

    _registry: dict = {}

    @classmethod
    def for_site(cls, key) -> "ReducePolicyTuner":
        """The tuner of one call site (a hooked module): kept for the life of the process, so a second visualizer over the same
        model does not measure again."""
        t = cls._registry.get(key)
        if t is None:
            t = cls._registry[key] = cls()
        return t

    def _harvest(self):
        keep = []
        for idx, e0, e1, nbytes in self._pending:
            if e1.query():
                self._samples[idx].append(e0.elapsed_time(e1) / nbytes)
            else:
                keep.append((idx, e0, e1, nbytes))
        self._pending = keep
        if all(len(s_) >= self.TRIALS for s_ in self._samples):
            med = [sorted(s_)[len(s_) // 2] for s_ in self._samples]
            best = min(range(len(med)), key=med.__getitem__)
            self.choice = best if med[best] < 0.98 * med[0] else 0  # the default unless another is clearly faster
            self.medians_ns_per_mb = [m * 1e12 for m in med]  # ms per byte -> ns per MB
            self._pending = []


# ------------------------------------------------------------------------------------------------
# K3 / K4
# ------------------------------------------------------------------------------------------------
def actmax_update_multi_supported(C: int, k: int, B: int) -> bool:
    return bool(lib().sl_actmax_update_multi_supported(C, k, B))


def actmax_update_multi(states: list[tuple[torch.Tensor, torch.Tensor]], cands: list[torch.Tensor], id_bases: list[int], B: int):
    """``SL_TIES_ATEN`` update of ``L`` states ``(C_l, k)`` from ``L`` candidate matrices ``(B, C_l)`` bf16 in one launch."""
    L = len(states)
    k = states[0][0].shape[1]
    assert len(cands) == L and all(c.is_contiguous() and tuple(c.shape) == (B, v.shape[0]) and v.shape[1] == k for c, (v, _) in zip(cands, states))
    vp = (_vp * L)(*[v.data_ptr() for v, _ in states])
    ip = (_vp * L)(*[i.data_ptr() for _, i in states])
    cp = (_vp * L)(*[c.data_ptr() for c in cands])
    hb = (_i64 * L)(*id_bases)
    hc = (_i64 * L)(*[v.shape[0] for v, _ in states])
    with _on(cands[0].device):
        rc = lib().sl_actmax_update_multi(vp, ip, hb, hc, cp, L, k, B, _stream(cands[0]))
    _check(rc, "sl_actmax_update_multi")


def actmax_init(vals: torch.Tensor, ids: torch.Tensor):
    C, k = vals.shape
    with _on(vals.device):
        _check(lib().sl_actmax_init(_ptr(vals), _ptr(ids), C, k, _stream(vals)), "sl_actmax_init")


def actmax_merge(vals, ids, cand: torch.Tensor, slot_stride: int, id_bases: list[int], rows: list[int]):
    C, k = vals.shape
    n = len(rows)
    hb = (_i64 * max(n, 1))(*id_bases)
    hr = (_i64 * max(n, 1))(*rows)
    with _on(vals.device):
        rc = lib().sl_actmax_merge(_ptr(vals), _ptr(ids), C, k, _ptr(cand), slot_stride, hb, hr, n, _stream(vals))
    _check(rc, "sl_actmax_merge")


def set_option(name: str, value: int) -> None:
    """Force one of several bit-identical kernel variants (``g3_tile``, ``f32_tile``, ``g3_strip_off``, ``colreduce_nw``, ``bn_policy``, ``g3_shared``; 0 = the
    dispatcher's own rule).  For the parity tests; ``SL_OPTIONS="name=value,..."`` presets them for a process."""
    _check(lib().sl_set_option(name.encode(), int(value)), "sl_set_option")


def get_option(name: str) -> int:
    return int(lib().sl_get_option(name.encode()))


def aten_topk_order_host(row_bf16: torch.Tensor, k: int) -> torch.Tensor:
    """Positions ``torch.topk(row, k)`` selects on the CPU according to the library's restatement (host code, no device)."""
    row = row_bf16.detach().to("cpu", torch.bfloat16).contiguous()
    out = torch.empty(k, dtype=torch.int32)
    _check(lib().sl_aten_topk_order_host(row.data_ptr(), row.numel(), k, out.data_ptr()), "sl_aten_topk_order_host")
    return out


_ATEN_SELFTEST: dict | None = None


def aten_order_selftest(rows: int = 200, force: bool = False) -> dict:
    """Once per process (first ``tie_mode="aten"`` use): the restatement the K3 kernels evaluate against the INSTALLED
    ``torch.topk`` on ``rows`` tie-heavy bf16 rows covering both of ATen's branches (``k * 64 <= n``: partial_sort; else
    nth_element + sort) — ~1 ms of host work.  The restatement is pinned to libstdc++ 11's introselect / introsort and
    torch 2.10's TopKImpl.h (the reference locks torch 2.7.1, same code); a host whose pair orders ties differently gets a
    warning naming the versions, because ``aten`` ids would then differ from what ``torch.topk`` gives THERE."""
    global _ATEN_SELFTEST
    if _ATEN_SELFTEST is not None and not force:
        return _ATEN_SELFTEST
    g = torch.Generator().manual_seed(1234)
    bad, cases = 0, 0
    shapes = [(20, 64), (20, 256), (100, 32), (5, 7), (1, 1), (3, 250), (2, 128), (20, 2000), (100, 6500)]  # (k, B): n = k + B
    for i in range(rows):
        k, B = shapes[i % len(shapes)]
        n = k + B
        row = (torch.randint(0, 12, (n,), generator=g).float() / 4).to(torch.bfloat16)  # ties are the point
        if i % 7 == 0:
            row[int(torch.randint(0, n, (1,), generator=g))] = float("nan")
        if i % 5 == 0:
            row[:k] = -0.0  # a fresh state: the sentinel (activation_caching.py:108)
        want = torch.topk(row, k).indices.to(torch.int32)
        got = aten_topk_order_host(row, k)
        cases += 1
        bad += int(not torch.equal(want, got))
    _ATEN_SELFTEST = {"rows": cases, "mismatches": bad, "torch": torch.__version__}
    if bad:
        import warnings

        warnings.warn(
            f"semanticlens_amd: tie_mode='aten' reproduces torch.topk's CPU tie order as restated for libstdc++ 11 / torch 2.7-2.10 "
            f"(ATen TopKImpl.h); the installed torch {torch.__version__} selects different positions on {bad} of {cases} tie-heavy rows. "
            "Top-k VALUES are unaffected; sample ids among tied values may differ from torch.topk on this host.  tie_mode='total' is "
            "independent of the host library.", RuntimeWarning, stacklevel=3)
    return _ATEN_SELFTEST


def actmax_aten_ws_bytes(C: int, k: int, B: int) -> int:
    return int(lib().sl_actmax_aten_ws_bytes(C, k, B))


def actmax_update(vals, ids, cand: torch.Tensor, sample_ids: torch.Tensor | None, id_base: int, B: int, ties: int,
                  ws: torch.Tensor | None):
    C, k = vals.shape
    with _on(vals.device):
        rc = lib().sl_actmax_update(
            _ptr(vals), _ptr(ids), C, k, _ptr(cand), _ptr(sample_ids), id_base, B, ties, _ptr(ws),
            ws.numel() * ws.element_size() if ws is not None else 0, _stream(vals),
        )
    _check(rc, "sl_actmax_update")


def actmax_merge_states(vals, ids, other_vals: torch.Tensor, other_ids: torch.Tensor):
    C, k = vals.shape
    R = other_vals.shape[0]
    with _on(vals.device):
        rc = lib().sl_actmax_merge_states(_ptr(vals), _ptr(ids), C, k, _ptr(other_vals), _ptr(other_ids), R, _stream(vals))
    _check(rc, "sl_actmax_merge_states")


# ------------------------------------------------------------------------------------------------
# K4 with its exchange step: RCCL behind the C ABI (csrc/comm.hip)
# ------------------------------------------------------------------------------------------------
SL_COMM_ID_BYTES = 128
_COMM_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int64: 2}
_COMM_OPS = {"sum": 0, "max": 1, "min": 2}


def _state_tables(states):
    """ctypes tables (C[], vals*[], ids*[]) + k of live device states [(vals (C,k) bf16, ids (C,k) int64)]."""
    k = int(states[0][0].shape[1])
    dev = states[0][0].device
    for vals, ids in states:
        if not (vals.is_cuda and ids.is_cuda and vals.device == dev and ids.device == dev and vals.is_contiguous() and ids.is_contiguous()):
            raise ValueError("states are contiguous tensors on one HIP device")
        if vals.dtype != torch.bfloat16 or ids.dtype != torch.int64 or vals.shape != ids.shape or vals.ndim != 2 or vals.shape[1] != k:
            raise ValueError("states are (C, k) bf16 values + (C, k) int64 ids with one k")
    n = len(states)
    C = (_i64 * n)(*[int(v.shape[0]) for v, _ in states])
    pv = (_vp * n)(*[v.data_ptr() for v, _ in states])
    pi = (_vp * n)(*[i.data_ptr() for _, i in states])
    return n, C, pv, pi, k


def actmax_pack(states) -> torch.Tensor:
    """One rank's packed block of all layers' states (uint8, ``sl_actmax_packed_bytes`` long; layout of ``sl_actmax_pack``)."""
    n, C, pv, pi, k = _state_tables(states)
    dev = states[0][0].device
    out = torch.empty(int(lib().sl_actmax_packed_bytes(n, C, k)), dtype=torch.uint8, device=dev)
    with _on(dev):
        rc = lib().sl_actmax_pack(n, pv, pi, C, k, _ptr(out), _stream(out))
    _check(rc, "sl_actmax_pack")
    return out


def actmax_merge_packed(states, gathered: torch.Tensor, skip_rank: int = -1):
    """K4 of every layer against ``gathered`` = ``(R, packed_bytes)`` uint8 blocks (e.g. all-gathered), in place."""
    n, C, pv, pi, k = _state_tables(states)
    dev = states[0][0].device
    P = int(lib().sl_actmax_packed_bytes(n, C, k))
    if not (gathered.is_cuda and gathered.device == dev and gathered.dtype == torch.uint8 and gathered.is_contiguous()
            and gathered.ndim == 2 and gathered.shape[1] == P):
        raise ValueError(f"gathered states are a contiguous (R, {P}) uint8 tensor on {dev}")
    with _on(dev):
        rc = lib().sl_actmax_merge_packed(n, pv, pi, C, k, _ptr(gathered), gathered.shape[0], int(skip_rank), _stream(gathered))
    _check(rc, "sl_actmax_merge_packed")


class Comm:
    """One RCCL communicator of the native library (``sl_comm_*``): one process per GPU, created collectively.

    ``Comm.unique_id()`` on rank 0 -> hand the 128 bytes to every process -> ``Comm(id, world, rank, device)`` on all of
    them.  Collectives are enqueued on torch's current stream of ``device``."""

    def __init__(self, unique_id: bytes, world: int, rank: int, device=None):
        if len(unique_id) != SL_COMM_ID_BYTES:
            raise ValueError(f"an RCCL unique id is {SL_COMM_ID_BYTES} bytes, got {len(unique_id)}")
        self.device = resolve_device(device)
        self.world, self.rank = int(world), int(rank)
        handle = _vp()
        buf = ctypes.create_string_buffer(bytes(unique_id), SL_COMM_ID_BYTES)
        with _on(self.device):
            rc = lib().sl_comm_init_from_unique_id(ctypes.cast(buf, _vp), self.world, self.rank, ctypes.byref(handle))
        _check(rc, "sl_comm_init_from_unique_id")
        self._h = handle

    @staticmethod
    def unique_id() -> bytes:
        buf = ctypes.create_string_buffer(SL_COMM_ID_BYTES)
        _check(lib().sl_comm_unique_id(ctypes.cast(buf, _vp)), "sl_comm_unique_id")
        return buf.raw

    def info(self):
        w, r, d = _int(), _int(), _int()
        _check(lib().sl_comm_info(self._h, ctypes.byref(w), ctypes.byref(r), ctypes.byref(d)), "sl_comm_info")
        return w.value, r.value, d.value

    def destroy(self):
        if self._h is not None:
            h, self._h = self._h, None
            _check(lib().sl_comm_destroy(h), "sl_comm_destroy")

    def _dev(self, t: torch.Tensor):
        if not (t.is_cuda and t.device == self.device and t.is_contiguous()):
            raise ValueError(f"collectives take contiguous tensors on {self.device}")
        return t

    def allgather(self, send: torch.Tensor) -> torch.Tensor:
        """``(world,) + send.shape``: block r is rank r's ``send`` (equal sizes on every rank)."""
        send = self._dev(send)
        recv = torch.empty((self.world,) + tuple(send.shape), dtype=send.dtype, device=self.device)
        with _on(self.device):
            rc = lib().sl_comm_allgather(self._h, _ptr(send), _ptr(recv), send.numel() * send.element_size(), _stream(send))
        _check(rc, "sl_comm_allgather")
        return recv

    def allreduce(self, t: torch.Tensor, op: str = "sum") -> torch.Tensor:
        """In place; fp32 / fp64 / int64, ``op`` "sum", "max" or "min"."""
        t = self._dev(t)
        with _on(self.device):
            rc = lib().sl_comm_allreduce(self._h, _ptr(t), t.numel(), _COMM_DTYPES[t.dtype], _COMM_OPS[op], _stream(t))
        _check(rc, "sl_comm_allreduce")
        return t

    def actmax_allgather_merge(self, states):
        """``states``: [(vals (C_l,k) bf16, ids (C_l,k) int64)] live device tensors, updated in place to the global top-k:
        pack -> ONE all-gather -> K4 per layer against the other ranks' blocks (``sl_actmax_allgather_merge``)."""
        if not states:
            return
        n, C, pv, pi, k = _state_tables(states)
        self._dev(states[0][0])
        need = lib().sl_actmax_allgather_merge_ws_bytes(n, C, k, self.world)
        ws = torch.empty(max(int(need), 16), dtype=torch.uint8, device=self.device)
        with _on(self.device):
            rc = lib().sl_actmax_allgather_merge(self._h, n, pv, pi, C, k, _ptr(ws), ws.numel(), _stream(ws))
        _check(rc, "sl_actmax_allgather_merge")
        ws.record_stream(torch.cuda.current_stream(self.device))


# ------------------------------------------------------------------------------------------------
# K5
# ------------------------------------------------------------------------------------------------
def gather_rows(emb: torch.Tensor, ids: torch.Tensor, check: bool = True) -> torch.Tensor:
    """``emb[ids]`` for emb (N,D) f32 on the device; negative ids wrap; out-of-range raises IndexError
    (``check=False`` skips that readback — and its host synchronisation — for indices known to be in range;
    out-of-range rows are then left unwritten)."""
    assert emb.is_cuda and emb.dtype == torch.float32 and emb.ndim == 2
    emb = emb.contiguous()
    ids_d = to_device(ids, emb.device).to(torch.int64).contiguous()
    N, D = emb.shape
    out = torch.empty(tuple(ids_d.shape) + (D,), dtype=torch.float32, device=emb.device)
    flag = torch.zeros(1, dtype=torch.int32, device=emb.device)
    with _on(emb.device):
        rc = lib().sl_gather_rows(_ptr(emb), N, D, _ptr(ids_d), ids_d.numel(), _ptr(out), _ptr(flag), _stream(emb))
    _check(rc, "sl_gather_rows")
    if check and int(flag.item()) != 0:
        raise IndexError(f"index out of range in embeds[sample_ids] (dataset size {N})")
    return out


def gather_rows_shard(emb_local: torch.Tensor, ids: torch.Tensor, row_offset: int, n_total: int) -> torch.Tensor:
    """Sharded ``emb[ids]``: rows this shard does not hold come back as zeros (sum over shards = full gather)."""
    assert emb_local.is_cuda and emb_local.dtype == torch.float32 and emb_local.ndim == 2
    emb_local = emb_local.contiguous()
    ids_d = to_device(ids, emb_local.device).to(torch.int64).contiguous()
    n_local, D = emb_local.shape
    out = torch.empty(tuple(ids_d.shape) + (D,), dtype=torch.float32, device=emb_local.device)
    flag = torch.zeros(1, dtype=torch.int32, device=emb_local.device)
    with _on(emb_local.device):
        rc = lib().sl_gather_rows_shard(
            _ptr(emb_local), n_local, D, _ptr(ids_d), ids_d.numel(), row_offset, n_total, _ptr(out), _ptr(flag),
            _stream(emb_local),
        )
    _check(rc, "sl_gather_rows_shard")
    if int(flag.item()) != 0:
        raise IndexError(f"index out of range in embeds[sample_ids] (dataset size {n_total})")
    return out


# ------------------------------------------------------------------------------------------------
# K6 / K7 / K8 / K10
# ------------------------------------------------------------------------------------------------
def _f32c(t: torch.Tensor, device=None) -> torch.Tensor:
    return to_device(t, device).to(torch.float32).contiguous()


def similarity(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    xd = _f32c(x)
    yd = _f32c(y, xd.device)
    if xd.ndim != 2 or yd.ndim != 2:
        raise ValueError("similarity_score expects 2-D tensors")
    xr, xc = xd.shape
    yr, yc = yd.shape
    if xd.shape == yd.shape:
        out = torch.empty((xr,), dtype=torch.float32, device=xd.device)
    elif xc == yr:
        out = torch.empty((xr, yc), dtype=torch.float32, device=xd.device)
    elif xc == yc:
        out = torch.empty((xr, yr), dtype=torch.float32, device=xd.device)
    else:
        raise ValueError("x and y must have the same shape")
    nbytes = int(lib().sl_similarity_ws_bytes(xr, xc, yr, yc))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
    with _on(xd.device):
        rc = lib().sl_similarity(_ptr(xd), xr, xc, _ptr(yd), yr, yc, _ptr(out), _ptr(ws), nbytes, _stream(xd))
    _check(rc, "sl_similarity")
    return out


def set_gemm_mode(mode: str | None):
    """Arithmetic of the cosine GEMMs: "bf16x3" (default), "f32" (fp32-input MFMA) or None (environment)."""
    _check(lib().sl_set_gemm_mode({None: -1, "f32": 0, "bf16x3": 1}[mode]), "sl_set_gemm_mode")


def similarity_multi(x: torch.Tensor, ys: list[torch.Tensor]) -> list[torch.Tensor] | None:
    """``[similarity(x, y) for y in ys]`` with the query normalised/split once.  Returns None when a layer would
    take one of ``similarity_score``'s shape-quirk branches (the caller then goes layer by layer)."""
    if x.ndim != 2 or any(y.ndim != 2 or y.shape[1] != x.shape[1] for y in ys):
        return None
    Q, K = x.shape
    if any(y.shape[0] == Q or y.shape[0] == K for y in ys) or not ys:
        return None
    xd = _f32c(x)
    yds = [_f32c(y, xd.device) for y in ys]
    outs = [torch.empty((Q, y.shape[0]), dtype=torch.float32, device=xd.device) for y in yds]
    L = len(yds)
    cs = (_i64 * L)(*[y.shape[0] for y in yds])
    yp = (_vp * L)(*[y.data_ptr() if y.numel() else None for y in yds])
    op = (_vp * L)(*[o.data_ptr() if o.numel() else None for o in outs])
    nbytes = int(lib().sl_similarity_multi_ws_bytes(Q, K, cs, L))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=xd.device)
    with _on(xd.device):
        rc = lib().sl_similarity_multi(_ptr(xd), Q, K, yp, cs, L, op, _ptr(ws), nbytes, _stream(xd))
    _check(rc, "sl_similarity_multi")
    return outs


def clarity(V: torch.Tensor) -> torch.Tensor:
    Vd = _f32c(V)
    lead = Vd.shape[:-2]
    n, D = Vd.shape[-2:]
    C = int(torch.tensor(lead).prod().item()) if len(lead) else 1
    out = torch.empty((C,), dtype=torch.float32, device=Vd.device)
    with _on(Vd.device):
        _check(lib().sl_clarity(_ptr(Vd), C, n, D, _ptr(out), _stream(Vd)), "sl_clarity")
    return out.reshape(lead)


def clarity_multi(Vs: list[torch.Tensor]) -> list[torch.Tensor] | None:
    """``[clarity(V) for V in Vs]`` as ONE launch when every ``V`` is ``(C_l, n, D)`` with the same ``(n, D)``; None otherwise
    (the caller then goes layer by layer)."""
    if not Vs or any(V.ndim != 3 for V in Vs) or len({tuple(V.shape[1:]) for V in Vs}) != 1:
        return None
    vds = [_f32c(Vs[0])]
    vds += [_f32c(V, vds[0].device) for V in Vs[1:]]
    n, D = vds[0].shape[1:]
    outs = [torch.empty((V.shape[0],), dtype=torch.float32, device=vds[0].device) for V in vds]
    L = len(vds)
    cs = (_i64 * L)(*[V.shape[0] for V in vds])
    vp = (_vp * L)(*[V.data_ptr() if V.numel() else None for V in vds])
    op = (_vp * L)(*[o.data_ptr() if o.numel() else None for o in outs])
    with _on(vds[0].device):
        _check(lib().sl_clarity_multi(vp, cs, L, n, D, op, _stream(vds[0])), "sl_clarity_multi")
    return outs


def redundancy(V: torch.Tensor) -> torch.Tensor:
    Vd = _f32c(V)
    lead = Vd.shape[:-2]
    C, D = Vd.shape[-2:]
    Bt = int(torch.tensor(lead).prod().item()) if len(lead) else 1
    out = torch.empty((Bt,), dtype=torch.float32, device=Vd.device)
    nbytes = int(lib().sl_redundancy_ws_bytes(Bt, C, D))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=Vd.device)
    with _on(Vd.device):
        _check(lib().sl_redundancy(_ptr(Vd), Bt, C, D, _ptr(out), _ptr(ws), nbytes, _stream(Vd)), "sl_redundancy")
    return out.reshape(lead)


def template_mean(E: torch.Tensor, E0: torch.Tensor, Q: int) -> torch.Tensor:
    Ed = _f32c(E)
    E0d = _f32c(E0, Ed.device)
    T, D = E0d.shape
    if Ed.shape != (Q * T, D):
        raise ValueError(f"templated embeddings have shape {tuple(Ed.shape)}, expected {(Q * T, D)}")
    out = torch.empty((Q, D), dtype=torch.float32, device=Ed.device)
    with _on(Ed.device):
        _check(lib().sl_template_mean(_ptr(Ed), _ptr(E0d), Q, T, D, _ptr(out), _stream(Ed)), "sl_template_mean")
    return out


# ------------------------------------------------------------------------------------------------
# K17: streaming fp32 top-k over cosine tiles
# ------------------------------------------------------------------------------------------------
TOPK_MAX_K = 1024
TOPK_TILE_BYTES = 128 << 20  # the similarity tile one GEMM writes and one merge reads


def check_topk_k(k) -> int:
    try:
        k = operator.index(k)  # any integral type (numpy.int64 included); floats and strings are refused
    except TypeError:
        raise ValueError(f"k must be an integer, got {k!r}") from None
    if k < 1 or k > TOPK_MAX_K:
        raise ValueError(f"k = {k} not in [1, {TOPK_MAX_K}]")
    return k


def topk_init(vals: torch.Tensor, ids: torch.Tensor):
    """Empty ``(R, k)`` state: values -inf, ids -1."""
    R, k = vals.shape
    with _on(vals.device):
        _check(lib().sl_topk_init(_ptr(vals), _ptr(ids), R, k, _stream(vals)), "sl_topk_init")


def topk_new(R: int, k: int, device) -> tuple[torch.Tensor, torch.Tensor]:
    vals = torch.empty((R, k), dtype=torch.float32, device=device)
    ids = torch.empty((R, k), dtype=torch.int64, device=device)
    topk_init(vals, ids)
    return vals, ids


def _tile_view(cand: torch.Tensor) -> tuple[torch.Tensor, int]:
    """``(cand, ld)`` as the merge kernels read an ``(R, B)`` tile: unit column stride, a row stride of at least ``B``, else a copy."""
    R, B = cand.shape
    if B > 1 and cand.stride(1) != 1:
        cand = cand.contiguous()
    ld = cand.stride(0) if R > 1 else B
    if ld < B:
        cand, ld = cand.contiguous(), B
    return cand, ld


def _check_cand_tile(what: str, cand: torch.Tensor, device=None, rows: int | None = None):
    """What every merge refuses first: a candidate tile that is not 2-D float32 on ``device`` (any HIP device when ``None``), or
    not of ``rows`` rows."""
    if cand.ndim != 2 or cand.dtype != torch.float32 or (not cand.is_cuda if device is None else cand.device != device):
        where = "device tensor" if device is None else f"tensor on {device}"
        raise ValueError(f"{what}: the candidate tile must be a 2-D float32 {where}, got {tuple(cand.shape)} {cand.dtype} on "
                         f"{cand.device}")
    if rows is not None and cand.shape[0] != rows:
        raise ValueError(f"{what}: candidate tile {tuple(cand.shape)} {cand.dtype} does not fit a state of {rows} rows")


def _ws_for(nbytes: int, ws: torch.Tensor | None, device) -> torch.Tensor | None:
    """``ws`` where it holds ``nbytes``, else a new uint8 buffer of that size on ``device``; ``nbytes == 0`` allocates nothing."""
    if nbytes and (ws is None or ws.numel() < nbytes):
        ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def topk_merge(vals: torch.Tensor, ids: torch.Tensor, cand: torch.Tensor, id_base: int = 0, ws: torch.Tensor | None = None):
    """Fold the ``(R, B)`` fp32 tile ``cand`` (unit column stride, any row stride) into the state; column ``j`` has the id
    ``id_base + j``.  ``ws``: a uint8 device buffer to use as the workspace of a split row when it is large enough."""
    R, k = vals.shape
    _check_cand_tile("topk_merge", cand, rows=R)
    B = cand.shape[1]
    cand, ld = _tile_view(cand)
    nbytes = int(lib().sl_topk_merge_ws_bytes(R, k, B))
    ws = _ws_for(nbytes, ws, vals.device)
    with _on(vals.device):
        rc = lib().sl_topk_merge(_ptr(vals), _ptr(ids), R, k, _ptr(cand), ld, B, id_base, _ptr(ws), nbytes, _stream(vals))
    _check(rc, "sl_topk_merge")


def topk_merge_biased(vals: torch.Tensor, ids: torch.Tensor, cand: torch.Tensor, row_bias: torch.Tensor, col_bias: torch.Tensor,
                      id_base: int = 0, ws: torch.Tensor | None = None):
    """``topk_merge`` under another score (K29): column ``j`` of row ``r`` ranks by ``(2 * cand[r, j] - row_bias[r]) - col_bias[j]``
    in fp32 (csrc/biased_score.hpp) and the state holds the scores.  ``row_bias (R,)`` and ``col_bias (B,)``: contiguous float32 on
    the tile's device; ``col_bias[0]`` belongs to the tile's first column, whatever ``id_base``."""
    R, k = vals.shape
    _check_cand_tile("topk_merge_biased", cand, rows=R)
    B = cand.shape[1]
    for name, bias, n in (("row_bias", row_bias, R), ("col_bias", col_bias, B)):
        if bias.ndim != 1 or bias.dtype != torch.float32 or bias.shape[0] != n or bias.device != cand.device or not bias.is_contiguous():
            raise ValueError(f"topk_merge_biased: {name} must be a contiguous 1-D float32 tensor of {n} entries on {cand.device}, got "
                             f"{tuple(bias.shape)} {bias.dtype} on {bias.device}")
    cand, ld = _tile_view(cand)
    nbytes = int(lib().sl_topk_merge_ws_bytes(R, k, B))
    ws = _ws_for(nbytes, ws, vals.device)
    with _on(vals.device):
        rc = lib().sl_topk_merge_biased(_ptr(vals), _ptr(ids), R, k, _ptr(cand), ld, B, id_base, _ptr(row_bias), _ptr(col_bias), _ptr(ws),
                                        nbytes, _stream(vals))
    _check(rc, "sl_topk_merge_biased")


def topk_merge_states(vals: torch.Tensor, ids: torch.Tensor, other_vals: torch.Tensor, other_ids: torch.Tensor):
    """Fold ``(R, M)`` explicit (value, id) entries into the state (negative ids are empty slots)."""
    R, k = vals.shape
    if other_vals.shape != other_ids.shape or other_vals.ndim != 2 or other_vals.shape[0] != R:
        raise ValueError(f"topk_merge_states: entries {tuple(other_vals.shape)} / {tuple(other_ids.shape)} do not fit {R} rows")
    ov = other_vals.to(torch.float32).contiguous()
    oi = other_ids.to(torch.int64).contiguous()
    with _on(vals.device):
        rc = lib().sl_topk_merge_states(_ptr(vals), _ptr(ids), R, k, _ptr(ov), _ptr(oi), ov.shape[1], _stream(vals))
    _check(rc, "sl_topk_merge_states")


def cosine_nt(x: torch.Tensor, y: torch.Tensor, out: torch.Tensor, ws: torch.Tensor | None = None) -> torch.Tensor:
    """``out[:] = normalize(x) @ normalize(y).T`` for contiguous fp32 device tensors of any shapes (K6's kernels, without
    ``similarity_score``'s shape branches)."""
    M, K = x.shape
    Nn = y.shape[0]
    nbytes = int(lib().sl_cosine_nt_ws_bytes(M, Nn, K))
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    with _on(x.device):
        rc = lib().sl_cosine_nt(_ptr(x), M, _ptr(y), Nn, K, _ptr(out), _ptr(ws), ws.numel(), _stream(x))
    _check(rc, "sl_cosine_nt")
    return out


def topk_chunk_rows(R: int, n_cols: int, tile_bytes: int = TOPK_TILE_BYTES) -> int:
    """Columns per tile so that an ``(R, chunk)`` fp32 tile stays at or under ``tile_bytes``."""
    return max(1, min(n_cols, tile_bytes // (4 * max(R, 1))))


def _check_probe_args(fn: str, x: torch.Tensor, y: torch.Tensor, **chunks):
    """What every probe checks first, before a device is touched: 2-D operands of one width, ``chunk_*`` of at least 1."""
    if x.ndim != 2 or y.ndim != 2:
        raise ValueError(f"{fn} expects 2-D tensors")
    if y.shape[1] != x.shape[1]:
        raise ValueError(f"embedding widths differ: {x.shape[1]} vs {y.shape[1]}")
    for name, chunk in chunks.items():
        if chunk is not None and chunk < 1:
            raise ValueError(f"{name} = {chunk} must be at least 1")


def tile_plan(m: int, n: int, chunk_rows: int | None = None, chunk_cols: int | None = None) -> tuple[int, int]:
    """``(rows, cols)`` of ``mutual_probe``'s / ``setmax_probe``'s tile of an ``(m, n)`` cosine matrix: by default all ``n`` columns and
    as many rows as keep it at or under ``TOPK_TILE_BYTES``; the columns are cut too only where a single row would pass that size."""
    cols = min(chunk_cols or min(n, TOPK_TILE_BYTES // 4), n)
    return min(chunk_rows or topk_chunk_rows(cols, m), m), cols


def tile_walk(m: int, n: int, rows: int, cols: int):
    """The ``(r0, nr, c0, nc)`` rectangles of ``(rows, cols)`` tiles over an ``(m, n)`` matrix, row blocks outermost."""
    for r0 in range(0, m, rows):
        for c0 in range(0, n, cols):
            yield r0, min(rows, m - r0), c0, min(cols, n - c0)


def _cosine_tiles(xd: torch.Tensor, yd: torch.Tensor, rows: int, cols: int, walk=None):
    """``normalize(xd) @ normalize(yd).T`` one ``tile_walk`` rectangle at a time, as ``(r0, nr, c0, nc, out)``: the cosine GEMM (K6)
    writes ``out (nr, nc)`` into ONE reused buffer, with one reused workspace (both allocated by the call, before anything is
    iterated), on the operands' stream; the consumer folds it on that stream before asking for the next.  ``walk``: another
    walk of rectangles of at most ``(rows, cols)`` (``upper_tile_walk``)."""
    walk = walk if walk is not None else tile_walk(xd.shape[0], yd.shape[0], rows, cols)
    tile = torch.empty(rows * cols, dtype=torch.float32, device=xd.device)
    ws = torch.empty(int(lib().sl_cosine_nt_ws_bytes(rows, cols, xd.shape[1])), dtype=torch.uint8, device=xd.device)

    def tiles():
        for r0, nr, c0, nc in walk:
            out = tile[: nr * nc].view(nr, nc)
            cosine_nt(xd[r0 : r0 + nr], yd[c0 : c0 + nc], out, ws)
            yield r0, nr, c0, nc, out

    return tiles()


def _row_tiles(xd: torch.Tensor, yd: torch.Tensor, chunk_rows: int | None):
    """``(step, tiles)`` of the row probes' walk: ``_cosine_tiles`` over tiles of all ``R`` rows of ``xd`` (the walk's single-row-block
    case) by ``step`` rows of ``yd`` — ``chunk_rows``, by default ``topk_chunk_rows``' — the last tile narrower."""
    R, n = xd.shape[0], yd.shape[0]
    step = min(chunk_rows or topk_chunk_rows(R, n), n)
    return step, _cosine_tiles(xd, yd, R, step)


# A consumer of the row probes' tiles: ``ws_bytes(R, step)`` is the split-row workspace its merge of an ``(R, step)`` tile needs,
# ``merge(out, c0, ws)`` folds the tile ``out`` whose first column is row ``c0`` of ``y``.
_Fold = namedtuple("_Fold", "ws_bytes merge")


def _row_probe(fn: str, x: torch.Tensor, y: torch.Tensor, chunk_rows: int | None, setup):
    """The walk of ``topk_probe``, ``softmax_probe`` and ``rank_probe``.  Checks the arguments, brings both operands to the device
    and calls ``setup(R, device)``, which makes (or checks) the caller's state and gives ``(result, [fold, ...])``; returns
    ``result``.  Unless an operand is empty, each tile the cosine GEMM (K6) writes is folded by every ``_Fold`` in list order on the
    same stream.  The tile buffer and ONE merge workspace are allocated before the first tile: all kernels split a row by one
    rule (csrc/rowseg_tile.hpp) and the workspace grows with the tile's width, so the largest fold's serves every merge."""
    _check_probe_args(fn, x, y, chunk_rows=chunk_rows)
    xd = _f32c(x)
    yd = _f32c(y, xd.device)
    R, n = xd.shape[0], yd.shape[0]
    result, folds = setup(R, xd.device)
    if R == 0 or n == 0:
        return result
    step, tiles = _row_tiles(xd, yd, chunk_rows)
    merge_ws = _ws_for(max(int(fold.ws_bytes(R, step)) for fold in folds), None, xd.device)
    for _, _, c0, _, out in tiles:
        for fold in folds:
            fold.merge(out, c0, merge_ws)
    return result


def _topk_fold(vals: torch.Tensor, ids: torch.Tensor, id_base: int):
    return _Fold(lambda R, step: lib().sl_topk_merge_ws_bytes(R, vals.shape[1], step),
                 lambda out, c0, ws: topk_merge(vals, ids, out, id_base + c0, ws))


def topk_probe(x: torch.Tensor, y: torch.Tensor, k: int, chunk_rows: int | None = None, id_base: int = 0, state=None):
    """Per row of ``x (R, D)``: the ``k`` largest cosines against the rows of ``y (N, D)`` (row ``j`` has the id
    ``id_base + j``), as ``(values (R, k) float32, ids (R, k) int64)``.

    Always ``normalize(x) @ normalize(y).T`` — none of ``similarity_score``'s shape branches apply.  The cosine GEMM (K6, in
    the arithmetic ``set_gemm_mode`` selects) writes one reused ``(R, chunk_rows)`` tile at a time and K17 folds it into the
    state on the same stream, so the ``(R, N)`` matrix never exists.  ``state``: continue an existing ``(values, ids)`` pair."""
    k = check_topk_k(k)

    def setup(R, device):
        vals, ids = state if state is not None else topk_new(R, k, device)
        return (vals, ids), [_topk_fold(vals, ids, id_base)]

    return _row_probe("topk_probe", x, y, chunk_rows, setup)


# ------------------------------------------------------------------------------------------------
# K29: hubness-corrected (CSLS) top-k over the same cosine tiles
# ------------------------------------------------------------------------------------------------
def check_neighbours(m) -> int:
    """The neighbourhood size of a CSLS density: an integer in ``[1, TOPK_MAX_K]`` (a density is the mean of a K17 state's row)."""
    try:
        m = operator.index(m)
    except TypeError:
        raise ValueError(f"neighbours must be an integer, got {m!r}") from None
    if m < 1 or m > TOPK_MAX_K:
        raise ValueError(f"neighbours = {m} not in [1, {TOPK_MAX_K}]")
    return m


def topk_density(vals: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    """``(R,)`` float32: per row of a K17 state the mean, taken in float64, of the entries present (``ids >= 0``); NaN for a row
    without any.  Plain torch on the state's device: the state is ``(R, m)``, not a hot path."""
    present = ids >= 0
    total = torch.where(present, vals.to(torch.float64), 0.0).sum(1)
    return (total / present.sum(1)).to(torch.float32)


def csls_probe(x: torch.Tensor, y: torch.Tensor, k: int, neighbours: int = 10, chunk_rows: int | None = None):
    """Per row of ``x (R, D)``: the ``k`` rows of ``y (N, D)`` of largest CSLS score (Conneau et al. 2018),
    ``csls(i, j) = 2 cos(x_i, y_j) - r_i - q_j``, as ``(scores (R, k) float32, ids (R, k) int64, r (R,) float32, q (N,) float32)``.
    ``r_i`` is the mean of row ``i``'s ``neighbours`` largest cosines over ``y`` (how crowded its neighbourhood is), ``q_j`` the mean
    of ``y_j``'s ``neighbours`` largest cosines over ``x`` (how much of a hub ``y_j`` is); with fewer candidates than ``neighbours``
    on a side, the mean over those present.

    Three passes over the ``_row_probe`` walk, none of which forms the ``(R, N)`` matrix: ``topk_probe(x, y)`` gives ``r``,
    ``topk_probe(y, x)`` gives ``q``, and in the third K29 folds each cosine tile ranking it by the score, computed in registers
    (csrc/biased_score.hpp) from the tile, ``r`` and the tile's slice of ``q``.  Order: K17's on the score, NaN first; a NaN
    cosine or density makes the score NaN.  An empty ``x`` or ``y`` gives K17's empty result and empty or NaN densities."""
    k = check_topk_k(k)
    m = check_neighbours(neighbours)
    _check_probe_args("csls_probe", x, y, chunk_rows=chunk_rows)
    xd = _f32c(x)
    yd = _f32c(y, xd.device)
    r = topk_density(*topk_probe(xd, yd, m, chunk_rows))
    q = topk_density(*topk_probe(yd, xd, m, chunk_rows))

    def setup(R, device):
        vals, ids = topk_new(R, k, device)
        fold = _Fold(lambda R, step: lib().sl_topk_merge_ws_bytes(R, k, step),
                     lambda out, c0, ws: topk_merge_biased(vals, ids, out, r, q[c0 : c0 + out.shape[1]], c0, ws))
        return (vals, ids, r, q), [fold]

    return _row_probe("csls_probe", xd, yd, chunk_rows, setup)


# ------------------------------------------------------------------------------------------------
# K25: streaming softmax statistics over the same cosine tiles
# ------------------------------------------------------------------------------------------------
SOFTMAX_STATE_WIDTH = 4  # doubles per row: (m, a, b, n) (include/semanticlens_amd.h, csrc/softmax_state.hpp)
_LOG2E = 1.4426950408889634
_F32_MIN_NORMAL, _F32_MAX = 1.1754943508222875e-38, 3.4028234663852886e38


def check_logit_scale(scale) -> float:
    """``scale`` as a float: a finite number above 0 (``scale * log2 e`` a normal fp32 number), else ``ValueError``."""
    try:
        if isinstance(scale, (str, bytes)):
            raise TypeError
        value = float(scale)
    except (TypeError, ValueError):
        raise ValueError(f"logit_scale must be a number, got {scale!r}") from None
    if not math.isfinite(value) or value <= 0:
        raise ValueError(f"logit_scale = {value} must be finite and > 0")
    if not _F32_MIN_NORMAL <= value * _LOG2E <= _F32_MAX:
        raise ValueError(f"logit_scale = {value} leaves the range the kernel's fp32 exponent covers")
    return value


def _check_softmax_state(what: str, state: torch.Tensor, R: int | None = None):
    if (state.ndim != 2 or state.shape[1] != SOFTMAX_STATE_WIDTH or state.dtype != torch.float64 or not state.is_cuda
            or not state.is_contiguous()):
        raise ValueError(f"{what}: a state is a contiguous (R, {SOFTMAX_STATE_WIDTH}) float64 device tensor, got {tuple(state.shape)} "
                         f"{state.dtype} on {state.device}")
    if R is not None and state.shape[0] != R:
        raise ValueError(f"{what}: a state of {state.shape[0]} rows does not fit {R}")


def softmax_new(R: int, device) -> torch.Tensor:
    """Empty ``(R, 4)`` float64 state: ``(m, a, b, n) = (-inf, 0, 0, 0)`` per row."""
    state = torch.empty((R, SOFTMAX_STATE_WIDTH), dtype=torch.float64, device=device)
    with _on(state.device):
        _check(lib().sl_softmax_init(_ptr(state), R, _stream(state)), "sl_softmax_init")
    return state


def softmax_merge(state: torch.Tensor, cand: torch.Tensor, scale: float, ws: torch.Tensor | None = None):
    """Fold the ``(R, B)`` fp32 tile ``cand`` (unit column stride, any row stride), as logits ``scale * cand``, into the state.
    ``ws``: a uint8 device buffer to use as the workspace of a split row when it is large enough."""
    scale = check_logit_scale(scale)
    _check_cand_tile("softmax_merge", cand)
    R, B = cand.shape
    _check_softmax_state("softmax_merge", state, R)
    cand, ld = _tile_view(cand)
    nbytes = int(lib().sl_softmax_merge_ws_bytes(R, B))
    ws = _ws_for(nbytes, ws, state.device)
    with _on(state.device):
        rc = lib().sl_softmax_merge(_ptr(state), R, _ptr(cand), ld, B, scale, _ptr(ws), nbytes, _stream(state))
    _check(rc, "sl_softmax_merge")


def softmax_finish(state: torch.Tensor, scale: float, vals: torch.Tensor | None = None):
    """``(probs, log_z, entropy)`` of a state: ``log_z`` and ``entropy`` ``(R,)`` float64; ``probs (R, k)`` float32 =
    ``exp(scale * vals - log_z)`` for K17's sorted ``vals (R, k)`` of the same candidates (0 for an empty slot), ``None`` without
    ``vals``."""
    scale = check_logit_scale(scale)
    _check_softmax_state("softmax_finish", state)
    R = state.shape[0]
    probs, k = None, 0
    if vals is not None:
        if vals.ndim != 2 or vals.shape[0] != R or vals.dtype != torch.float32 or vals.device != state.device:
            raise ValueError(f"softmax_finish: values {tuple(vals.shape)} {vals.dtype} do not fit a state of {R} rows")
        vals = vals.contiguous()
        k = check_topk_k(vals.shape[1])
        probs = torch.empty((R, k), dtype=torch.float32, device=state.device)
    log_z = torch.empty(R, dtype=torch.float64, device=state.device)
    entropy = torch.empty(R, dtype=torch.float64, device=state.device)
    with _on(state.device):
        rc = lib().sl_softmax_finish(_ptr(state), R, scale, _ptr(vals), k, _ptr(probs), _ptr(log_z), _ptr(entropy), _stream(state))
    _check(rc, "sl_softmax_finish")
    return probs, log_z, entropy


def _softmax_fold(sm: torch.Tensor, scale: float):
    return _Fold(lambda R, step: lib().sl_softmax_merge_ws_bytes(R, step), lambda out, c0, ws: softmax_merge(sm, out, scale, ws))


def softmax_probe(x: torch.Tensor, y: torch.Tensor, k: int, scale: float, chunk_rows: int | None = None, id_base: int = 0,
                  state=None):
    """``topk_probe`` with the softmax statistics of the same cosines: every tile the cosine GEMM writes is folded by K17 and then
    by K25 on the same stream — one GEMM per tile, one reused tile buffer, one reused workspace.  Returns (and continues, as
    ``state``) the triple ``(values (R, k), ids (R, k), softmax state (R, 4))``; ``values`` and ``ids`` are ``topk_probe``'s."""
    k = check_topk_k(k)
    scale = check_logit_scale(scale)

    def setup(R, device):
        vals, ids, sm = state if state is not None else (*topk_new(R, k, device), softmax_new(R, device))
        return (vals, ids, sm), [_topk_fold(vals, ids, id_base), _softmax_fold(sm, scale)]

    return _row_probe("softmax_probe", x, y, chunk_rows, setup)


# ------------------------------------------------------------------------------------------------
# K26: ranks of given keys among the candidates of the same cosine tiles
# ------------------------------------------------------------------------------------------------
RANK_MAX_TARGETS = 16  # key slots per row (include/semanticlens_amd.h: SL_RANK_MAX_TARGETS)


def check_rank_targets(targets, R: int, n: int) -> torch.Tensor:
    """``targets`` as an ``(R, T)`` int64 CPU tensor, ``T`` the longest row (at least 1), rows padded with -1 = unused slot.  Per
    row: an int, ``None`` / -1 (no target), or a list of up to ``RANK_MAX_TARGETS`` ints, each in ``[0, n)`` or -1; a tensor or
    array of one or two dimensions is read as its ``tolist()``.  Anything else is a ``ValueError``."""
    if hasattr(targets, "tolist"):
        t = torch.as_tensor(targets)
        if t.ndim in (1, 2) and t.numel() and not t.dtype.is_floating_point and not t.dtype.is_complex and t.dtype != torch.bool:
            t = t.to("cpu", torch.int64).reshape(t.shape[0], -1)  # the whole array at once: no Python loop over the rows
            if t.shape[0] != R:
                raise ValueError(f"targets has {t.shape[0]} entries for {R} rows")
            if t.shape[1] > RANK_MAX_TARGETS:
                raise ValueError(f"targets holds {t.shape[1]} targets per row, more than {RANK_MAX_TARGETS}")
            if int(t.min()) < -1 or int(t.max()) >= n:
                raise ValueError(f"targets: an index lies outside [0, {n}) (-1 = no target)")
            return t.clone().contiguous()
        targets = targets.tolist()
    if isinstance(targets, (str, bytes)) or not isinstance(targets, (list, tuple)):
        raise ValueError(f"targets must be a sequence with one entry per row, got {type(targets).__name__}")
    if len(targets) != R:
        raise ValueError(f"targets has {len(targets)} entries for {R} rows")
    rows = []
    for r, entry in enumerate(targets):
        if hasattr(entry, "tolist"):
            entry = entry.tolist()
        items = list(entry) if isinstance(entry, (list, tuple)) else [entry]
        if len(items) > RANK_MAX_TARGETS:
            raise ValueError(f"targets[{r}] holds {len(items)} targets, more than {RANK_MAX_TARGETS}")
        row = []
        for item in items:
            if item is None:
                item = -1
            try:
                if isinstance(item, bool):
                    raise TypeError
                item = operator.index(item)
            except TypeError:
                raise ValueError(f"targets[{r}]: {item!r} is not an index") from None
            if not -1 <= item < n:
                raise ValueError(f"targets[{r}]: index {item} outside [0, {n}) (-1 = no target)")
            row.append(item)
        rows.append(row)
    T = max([1] + [len(row) for row in rows])
    out = torch.full((R, T), -1, dtype=torch.int64)
    for r, row in enumerate(rows):
        if row:
            out[r, : len(row)] = torch.tensor(row, dtype=torch.int64)
    return out


def _check_rank_state(what: str, counts: torch.Tensor, key_vals: torch.Tensor, key_ids: torch.Tensor, R: int | None = None):
    if (counts.ndim != 2 or counts.dtype != torch.int64 or not counts.is_cuda or not counts.is_contiguous()
            or not 1 <= counts.shape[1] <= RANK_MAX_TARGETS):
        raise ValueError(f"{what}: counts are a contiguous (R, T) int64 device tensor with T in [1, {RANK_MAX_TARGETS}], got "
                         f"{tuple(counts.shape)} {counts.dtype} on {counts.device}")
    for name, t, dtype in (("key values", key_vals, torch.float32), ("key ids", key_ids, torch.int64)):
        if t.shape != counts.shape or t.dtype != dtype or t.device != counts.device or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {tuple(counts.shape)} {dtype} tensor on {counts.device}, got "
                             f"{tuple(t.shape)} {t.dtype} on {t.device}")
    if R is not None and counts.shape[0] != R:
        raise ValueError(f"{what}: counts of {counts.shape[0]} rows do not fit {R}")


def rank_merge(counts: torch.Tensor, cand: torch.Tensor, key_vals: torch.Tensor, key_ids: torch.Tensor, id_base: int = 0):
    """Per row and slot with ``key_ids >= 0``: ``counts (R, T) int64 +=`` the number of columns of the ``(R, B)`` fp32 tile ``cand`` (unit
    column stride, any row stride; column ``j`` has the id ``id_base + j``) that order before the key ``(key_vals, key_ids)`` in K17's
    order; the key's own column is never counted (K26, csrc/rank_order.hpp)."""
    _check_cand_tile("rank_merge", cand)
    R, B = cand.shape
    _check_rank_state("rank_merge", counts, key_vals, key_ids, R)
    cand, ld = _tile_view(cand)
    with _on(counts.device):
        rc = lib().sl_rank_merge(_ptr(counts), R, counts.shape[1], _ptr(cand), ld, B, id_base, _ptr(key_vals), _ptr(key_ids),
                                 _stream(counts))
    _check(rc, "sl_rank_merge")


def rank_keys(x: torch.Tensor, y: torch.Tensor, targets: torch.Tensor, chunk_rows: int | None = None) -> torch.Tensor:
    """``(R, T)`` float32: the cosine of row ``r`` of ``x (R, D)`` to row ``targets[r, t]`` of ``y (n, D)``, NaN where ``targets`` is
    negative.  The values come out of the cosine GEMM (K6) — the unique target rows of ``y`` as the columns of the tiles
    ``topk_probe`` walks — so they are computed in the arithmetic mode and from the operand preparation of the tiles they will be
    compared with; two K6 calls differ by the accumulation order at most."""
    _check_probe_args("rank_keys", x, y, chunk_rows=chunk_rows)
    if targets.ndim != 2 or targets.shape[0] != x.shape[0] or targets.dtype != torch.int64:
        raise ValueError(f"rank_keys: targets {tuple(targets.shape)} {targets.dtype} are not (R, T) int64 for {x.shape[0]} rows")
    if targets.numel() and not (-1 <= int(targets.min()) and int(targets.max()) < y.shape[0]):
        raise ValueError(f"rank_keys: a target lies outside [0, {y.shape[0]}) (-1 = no target)")
    used = targets >= 0
    nothing = not bool(used.any())
    xd = _f32c(x)
    R = xd.shape[0]
    vals = torch.full(targets.shape, float("nan"), dtype=torch.float32, device=xd.device)
    if R == 0 or nothing:
        return vals
    uniq = torch.unique(targets[used])  # sorted
    pos = torch.searchsorted(uniq, targets.clamp(min=0)).to(xd.device)  # the column of yu that holds targets[r, t]
    used = used.to(xd.device)
    yu = _f32c(y[uniq.to(y.device)], xd.device)
    for _, _, c0, nc, out in _row_tiles(xd, yu, chunk_rows)[1]:
        here = used & (pos >= c0) & (pos < c0 + nc)
        vals = torch.where(here, out.gather(1, (pos - c0).clamp(0, nc - 1)), vals)
    return vals


def rank_probe(x: torch.Tensor, y: torch.Tensor, key_vals: torch.Tensor, key_ids: torch.Tensor, chunk_rows: int | None = None,
               id_base: int = 0, state: torch.Tensor | None = None, softmax=None) -> torch.Tensor:
    """``topk_probe``'s walk with K26 as the fold: per row of ``x (R, D)`` and key slot, the number of rows of ``y (N, D)`` (row ``j``
    has the id ``id_base + j``) whose cosine orders before the key ``(key_vals, key_ids) (R, T)``.  Returns (and continues, as
    ``state``) the ``(R, T)`` int64 counts; slots with a negative key id stay as they are.  ``softmax=(state, scale)``: K25 folds the
    same tiles into that ``(R, 4)`` softmax state, as ``softmax_probe`` does."""
    def setup(R, device):
        counts = state if state is not None else torch.zeros(key_ids.shape, dtype=torch.int64, device=device)
        _check_rank_state("rank_probe", counts, key_vals, key_ids, R)
        folds = [_Fold(lambda R, step: 0, lambda out, c0, ws: rank_merge(counts, out, key_vals, key_ids, id_base + c0))]  # no workspace
        if softmax is not None and softmax[0] is not None:
            sm, scale = softmax[0], check_logit_scale(softmax[1])
            _check_softmax_state("rank_probe", sm, R)
            folds.append(_softmax_fold(sm, scale))
        return counts, folds

    return _row_probe("rank_probe", x, y, chunk_rows, setup)


# ------------------------------------------------------------------------------------------------
# K28: orthogonal matching pursuit over a vocabulary — K6 + K17 find the candidates of a pass, one kernel does the step between two
# ------------------------------------------------------------------------------------------------
OMP_MAX_TERMS = 16  # include/semanticlens_amd.h: SL_OMP_MAX_TERMS
OMP_MIN_PIVOT = 1e-10  # SL_OMP_MIN_PIVOT and SL_OMP_RESIDUAL_DONE: design constants (csrc/omp_state.hpp says what they mean)
OMP_RESIDUAL_DONE = 1e-8

# What a pursuit carries per component (the header describes every array); ``residual`` is the working row the next pass reads —
# zeros once the component is finished — and ``last`` the residual to report, complete after step ``s - 1``.
OmpState = namedtuple("OmpState", "ids chol rhs coefs corr explained n_terms finished residual last")


def check_omp_terms(n_terms) -> int:
    try:
        if isinstance(n_terms, bool):
            raise TypeError
        n_terms = operator.index(n_terms)
    except TypeError:
        raise ValueError(f"n_terms must be an integer, got {n_terms!r}") from None
    if not 1 <= n_terms <= OMP_MAX_TERMS:
        raise ValueError(f"n_terms = {n_terms} not in [1, {OMP_MAX_TERMS}]")
    return n_terms


def check_min_correlation(min_correlation) -> float:
    try:
        if isinstance(min_correlation, (str, bytes, bool)):
            raise TypeError
        value = float(min_correlation)
    except (TypeError, ValueError):
        raise ValueError(f"min_correlation must be a number, got {min_correlation!r}") from None
    if not (math.isfinite(value) and 0.0 <= value < 1.0):
        raise ValueError(f"min_correlation = {value} must be finite and in [0, 1)")
    return value


def _check_omp_rows(what: str, name: str, t: torch.Tensor, cols: int | None = None):
    if t.ndim != 2 or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or (cols is not None and t.shape[1] != cols):
        width = "D" if cols is None else str(cols)
        raise ValueError(f"{what}: {name} must be a contiguous (n, {width}) float32 device tensor, got {tuple(t.shape)} {t.dtype} on "
                         f"{t.device}")


def omp_new(x: torch.Tensor, s: int) -> OmpState:
    """The empty state of a pursuit of ``s`` terms for the components ``x (C, D)`` (contiguous fp32 on the device): ``x / |x|`` as the
    working residual, no term chosen; a zero row or one with a non-finite coordinate is finished at once (``explained`` and
    ``last`` NaN)."""
    s = check_omp_terms(s)
    _check_omp_rows("omp_new", "the components", x)
    C, D = x.shape
    dev = x.device
    st = OmpState(ids=torch.empty((C, s), dtype=torch.int64, device=dev),
                  chol=torch.empty((C, s * (s + 1) // 2), dtype=torch.float64, device=dev),
                  rhs=torch.empty((C, s), dtype=torch.float64, device=dev),
                  coefs=torch.empty((C, s), dtype=torch.float64, device=dev),
                  corr=torch.empty((C, s), dtype=torch.float32, device=dev),
                  explained=torch.empty((C, s), dtype=torch.float64, device=dev),
                  n_terms=torch.empty((C,), dtype=torch.int32, device=dev),
                  finished=torch.empty((C,), dtype=torch.int32, device=dev),
                  residual=torch.empty((C, D), dtype=torch.float32, device=dev),
                  last=torch.empty((C, D), dtype=torch.float32, device=dev))
    with _on(dev):
        rc = lib().sl_omp_init(_ptr(x), C, D, s, _ptr(st.ids), _ptr(st.coefs), _ptr(st.corr), _ptr(st.explained), _ptr(st.n_terms),
                               _ptr(st.finished), _ptr(st.residual), _ptr(st.last), _stream(x))
    _check(rc, "sl_omp_init")
    return st


def omp_step(state: OmpState, x: torch.Tensor, w: torch.Tensor, cand_vals: torch.Tensor, cand_ids: torch.Tensor, t: int,
             min_correlation: float = 0.0):
    """Step ``t`` of the pursuit (K28, one launch): per unfinished component take the first of the candidates
    ``(cand_vals, cand_ids) (C, k >= t + 1)`` — best first, ids indexing the rows of ``w (V, D)`` — that is not chosen yet, append it,
    solve the least squares and write the new residual, or stop the component (``csrc/omp_state.hpp`` holds the rules).  ``x`` and
    ``w`` are contiguous fp32 device tensors and are used where they lie: any 4-byte aligned start works."""
    s = state.ids.shape[1]
    _check_omp_rows("omp_step", "the components", x)
    C, D = x.shape
    _check_omp_rows("omp_step", "the vocabulary", w, D)
    if (cand_vals.shape != cand_ids.shape or cand_vals.ndim != 2 or cand_vals.shape[0] != C or cand_vals.dtype != torch.float32
            or cand_ids.dtype != torch.int64 or cand_vals.device != x.device or cand_ids.device != x.device):
        raise ValueError(f"omp_step: candidates must be (C = {C}, k) float32 values and int64 ids on {x.device}, got "
                         f"{tuple(cand_vals.shape)} {cand_vals.dtype} / {tuple(cand_ids.shape)} {cand_ids.dtype}")
    shapes = dict(ids=(C, s), chol=(C, s * (s + 1) // 2), rhs=(C, s), coefs=(C, s), corr=(C, s), explained=(C, s), n_terms=(C,),
                  finished=(C,), residual=(C, D), last=(C, D))
    for name, shape in shapes.items():
        part = getattr(state, name)
        if tuple(part.shape) != shape or part.device != x.device or not part.is_contiguous():
            raise ValueError(f"omp_step: state.{name} {tuple(part.shape)} on {part.device} is not a contiguous {shape} tensor on {x.device}")
    cand_vals, cand_ids = cand_vals.contiguous(), cand_ids.contiguous()
    with _on(x.device):
        rc = lib().sl_omp_step(_ptr(x), C, D, _ptr(w), w.shape[0], _ptr(cand_vals), _ptr(cand_ids), cand_vals.shape[1], t, s,
                               min_correlation, _ptr(state.ids), _ptr(state.chol), _ptr(state.rhs), _ptr(state.coefs),
                               _ptr(state.corr), _ptr(state.explained), _ptr(state.n_terms), _ptr(state.finished),
                               _ptr(state.residual), _ptr(state.last), _stream(x))
    _check(rc, "sl_omp_step")


def decompose_probe(x: torch.Tensor, w: torch.Tensor, s: int, min_correlation: float = 0.0, chunk_rows: int | None = None) -> OmpState:
    """Greedy orthogonal matching pursuit of every row of ``x (C, D)`` over the rows of ``w (V, D)``, ``s`` terms at most: the final
    ``OmpState``.  Step ``t`` is one ``topk_probe`` of the working residuals with ``k = t + 1`` — among ``t + 1`` candidates one is not
    chosen yet — then one ``omp_step``, all on one stream; the ``(C, V)`` matrix is never formed and nothing is read back."""
    s = check_omp_terms(s)
    min_correlation = check_min_correlation(min_correlation)
    _check_probe_args("decompose_probe", x, w, chunk_rows=chunk_rows)
    if w.shape[0] == 0:
        raise ValueError("decompose_probe: the vocabulary is empty")
    xd = _f32c(x)
    wd = _f32c(w, xd.device)
    state = omp_new(xd, s)
    if xd.shape[0] == 0:
        return state
    for t in range(s):
        vals, ids = topk_probe(state.residual, wd, t + 1, chunk_rows)
        omp_step(state, xd, wd, vals, ids, t, min_correlation)
    return state

# ------------------------------------------------------------------------------------------------
# K20: mutual best matches (row and column maxima of every cosine tile in one read)
# ------------------------------------------------------------------------------------------------
MUTUALMAX_MAX_ID = (1 << 32) - 2  # a packed state entry holds a 32-bit id; 2^32 - 1 is left out (csrc/packed_best.hpp: kMaxPackedId)


def _check_mutualmax_state(what: str, state: torch.Tensor, n: int | None = None):
    if state.ndim != 1 or state.dtype != torch.int64 or not state.is_cuda or (state.numel() > 1 and state.stride(0) != 1):
        raise ValueError(f"{what}: a state is a 1-D int64 device tensor with unit stride, got {tuple(state.shape)} {state.dtype} on "
                         f"{state.device}")
    if n is not None and state.shape[0] != n:
        raise ValueError(f"{what}: a state of {state.shape[0]} entries does not fit {n}")


def mutualmax_merge(row_state: torch.Tensor, col_state: torch.Tensor, cand: torch.Tensor, row_id_base: int = 0, col_id_base: int = 0):
    """Fold the ``(R, B)`` fp32 tile ``cand`` (unit column stride, any row stride) into ``row_state (R,)`` — the best column of
    every row — and ``col_state (B,)`` — the best row of every column — in one read of the tile.  States are int64 tensors of
    packed entries (``torch.zeros`` is the empty state; decode with ``mutualmax_finish``); row ``r`` has the id
    ``row_id_base + r``, column ``j`` the id ``col_id_base + j``, all within ``[0, MUTUALMAX_MAX_ID]``."""
    _check_cand_tile("mutualmax_merge", cand)
    R, B = cand.shape
    _check_mutualmax_state("mutualmax_merge", row_state, R)
    _check_mutualmax_state("mutualmax_merge", col_state, B)
    cand, ld = _tile_view(cand)
    with _on(cand.device):
        rc = lib().sl_mutualmax_merge(_ptr(row_state), _ptr(col_state), R, B, _ptr(cand), ld, row_id_base, col_id_base, _stream(cand))
    _check(rc, "sl_mutualmax_merge")


def mutualmax_finish(state: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Decode a packed state into K17's ``k = 1`` form: ``(values (n,) float32, ids (n,) int64)``, ``(-inf, -1)`` where nothing
    was seen.  A zero comes back as ``+0.0`` and a NaN as the canonical quiet NaN, whatever went in."""
    _check_mutualmax_state("mutualmax_finish", state)
    n = state.shape[0]
    vals = torch.empty(n, dtype=torch.float32, device=state.device)
    ids = torch.empty(n, dtype=torch.int64, device=state.device)
    with _on(state.device):
        _check(lib().sl_mutualmax_finish(_ptr(state), n, _ptr(vals), _ptr(ids), _stream(state)), "sl_mutualmax_finish")
    return vals, ids


def mutual_probe(x: torch.Tensor, y: torch.Tensor, chunk_rows: int | None = None, chunk_cols: int | None = None):
    """Best cosine match in both directions from ONE pass over ``normalize(x) @ normalize(y).T``:
    ``((x_vals (len(x),), x_ids), (y_vals (len(y),), y_ids))`` — for every row of ``x`` its best row of ``y`` (``x_ids`` index
    ``y``) and for every row of ``y`` its best row of ``x`` (``y_ids`` index ``x``).  Order as in ``topk_probe``: NaN first,
    then the larger cosine, equal cosines by the smaller id; ``(-inf, -1)`` when the other operand is empty.

    The cosine GEMM (K6, in the arithmetic ``set_gemm_mode`` selects) writes one reused tile of ``chunk_rows`` rows of ``x``
    against ``chunk_cols`` rows of ``y`` and K20 folds its row and column maxima into two states on the same stream; the
    ``(len(x), len(y))`` matrix never exists.  ``tile_plan`` has the default tile."""
    _check_probe_args("mutual_probe", x, y, chunk_rows=chunk_rows, chunk_cols=chunk_cols)
    if max(x.shape[0], y.shape[0]) > MUTUALMAX_MAX_ID + 1:
        raise ValueError(f"mutual_probe: more than {MUTUALMAX_MAX_ID + 1} rows do not fit a packed state's 32-bit ids")
    xd = _f32c(x)
    yd = _f32c(y, xd.device)
    m, n = xd.shape[0], yd.shape[0]
    row_state = torch.zeros(m, dtype=torch.int64, device=xd.device)
    col_state = torch.zeros(n, dtype=torch.int64, device=xd.device)
    if m and n:
        for r0, nr, c0, nc, out in _cosine_tiles(xd, yd, *tile_plan(m, n, chunk_rows, chunk_cols)):
            mutualmax_merge(row_state[r0 : r0 + nr], col_state[c0 : c0 + nc], out, r0, c0)
    return mutualmax_finish(row_state), mutualmax_finish(col_state)


# ------------------------------------------------------------------------------------------------
# K22: per-set best cosine (the column maxima of every cosine tile, one per segment of its rows)
# ------------------------------------------------------------------------------------------------
def segmax_merge(state: torch.Tensor, cand: torch.Tensor, row_seg: torch.Tensor, row_id_base: int = 0):
    """Fold the ``(R, B)`` fp32 tile ``cand`` (unit column stride, any row stride) into ``state (G, B)``: entry ``(g, j)`` is the
    best row of column ``j`` among the rows ``r`` with ``row_seg[r] == g`` (rows whose segment is outside ``[0, G)`` are
    ignored).  ``state`` is an int64 device tensor of K20's packed entries with unit column stride and any row stride — a column
    slice of a ``(G, C)`` state — and ``torch.zeros`` is the empty state; ``row_seg`` is ``(R,)`` int32 on the device; row ``r``
    has the id ``row_id_base + r`` within ``[0, MUTUALMAX_MAX_ID]``."""
    _check_cand_tile("segmax_merge", cand)
    R, B = cand.shape
    if state.ndim != 2 or state.dtype != torch.int64 or state.device != cand.device or state.shape[1] != B:
        raise ValueError(f"segmax_merge: the state must be a (G, {B}) int64 tensor on {cand.device}, got {tuple(state.shape)} "
                         f"{state.dtype} on {state.device}")
    G = state.shape[0]
    state_ld = state.stride(0) if G > 1 else B
    if (B > 1 and state.stride(1) != 1) or state_ld < B:
        raise ValueError(f"segmax_merge: the state needs unit column stride and a row stride of at least {B}, got {state.stride()}")
    if row_seg.ndim != 1 or row_seg.dtype != torch.int32 or row_seg.device != cand.device or row_seg.shape[0] != R:
        raise ValueError(f"segmax_merge: the segment table must be a ({R},) int32 tensor on {cand.device}, got {tuple(row_seg.shape)} "
                         f"{row_seg.dtype} on {row_seg.device}")
    if R > 1 and row_seg.stride(0) != 1:
        row_seg = row_seg.contiguous()
    cand, ld = _tile_view(cand)
    with _on(cand.device):
        rc = lib().sl_segmax_merge(_ptr(state), state_ld, G, R, B, _ptr(cand), ld, _ptr(row_seg), row_id_base, _stream(cand))
    _check(rc, "sl_segmax_merge")


def check_set_offsets(set_offsets, P: int) -> list[int]:
    """``G + 1`` host ints, non-decreasing, from 0 to ``P`` (a set may be empty); returns them as a list."""
    try:
        offsets = [operator.index(o) for o in set_offsets]
    except TypeError:
        raise ValueError(f"set_offsets must be a sequence of integers, got {set_offsets!r}") from None
    if not offsets or offsets[0] != 0 or offsets[-1] != P:
        raise ValueError(f"set_offsets must start at 0 and end at the number of prompt rows ({P}), got {offsets[:1]} ... {offsets[-1:]}")
    if any(b < a for a, b in zip(offsets, offsets[1:])):
        raise ValueError("set_offsets must be non-decreasing")
    return offsets


def setmax_probe(x: torch.Tensor, set_offsets, y: torch.Tensor, chunk_rows: int | None = None, chunk_cols: int | None = None,
                 id_base: int = 0, state: torch.Tensor | None = None) -> torch.Tensor:
    """Per set of prompt vectors and per row of ``y (C, D)``: the best cosine over the set and the prompt that has it, as the raw
    ``(G, C)`` int64 state (decode with ``setmax_finish``; pass it back as ``state=`` with the next chunk of prompts, whose first
    row has the id ``id_base``).  ``x (P, D)`` holds the prompt vectors set-major, set ``g`` being rows
    ``set_offsets[g]:set_offsets[g + 1]``.  Order as in ``mutual_probe``: NaN first, then the larger cosine, equal cosines by
    the smaller id.

    Tiling is ``mutual_probe``'s: the cosine GEMM (K6, in the arithmetic ``set_gemm_mode`` selects) writes one reused tile of
    ``chunk_rows`` prompts against ``chunk_cols`` rows of ``y`` and K22 folds its per-set column maxima into the state on the
    same stream, so the ``(P, C)`` matrix never exists."""
    _check_probe_args("setmax_probe", x, y, chunk_rows=chunk_rows, chunk_cols=chunk_cols)
    m, n = x.shape[0], y.shape[0]
    offsets = check_set_offsets(set_offsets, m)
    G = len(offsets) - 1
    if id_base < 0 or id_base + m > MUTUALMAX_MAX_ID + 1:
        raise ValueError(f"setmax_probe: prompt ids from {id_base} leave [0, {MUTUALMAX_MAX_ID}], the range a packed state entry holds")
    if state is not None and (state.ndim != 2 or tuple(state.shape) != (G, n) or state.dtype != torch.int64 or not state.is_cuda):
        raise ValueError(f"setmax_probe: state must be a ({G}, {n}) int64 device tensor, got {tuple(state.shape)} {state.dtype}")
    xd = _f32c(x)
    yd = _f32c(y, xd.device)
    if state is None:
        state = torch.zeros((G, n), dtype=torch.int64, device=xd.device)
    if m and n and G:
        counts = torch.tensor([b - a for a, b in zip(offsets, offsets[1:])], dtype=torch.int64)
        seg = torch.repeat_interleave(torch.arange(G, dtype=torch.int32), counts).to(xd.device)
        for r0, nr, c0, nc, out in _cosine_tiles(xd, yd, *tile_plan(m, n, chunk_rows, chunk_cols)):
            segmax_merge(state[:, c0 : c0 + nc], out, seg[r0 : r0 + nr], id_base + r0)
    return state


def setmax_finish(state: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """Decode a ``(G, C)`` state: ``(values (G, C) float32, ids (G, C) int64)``, ``(-inf, -1)`` for a set that held no prompt."""
    if state.ndim != 2:
        raise ValueError(f"setmax_finish: a state is a (G, C) int64 device tensor, got {tuple(state.shape)}")
    vals, ids = mutualmax_finish(state.contiguous().view(-1))
    return vals.view(state.shape), ids.view(state.shape)


# ------------------------------------------------------------------------------------------------
# K24: redundancy groups (the connected components of "cosine >= threshold" and every component's degree)
# ------------------------------------------------------------------------------------------------
REDGROUPS_MAX_N = (1 << 31) - 1  # the forest's entries are int32 ids


def upper_tile_walk(n: int, rows: int, cols: int):
    """The ``(r0, nr, c0, nc)`` rectangles that cover the upper triangle of an ``(n, n)`` matrix: for the row block at ``r0``
    they start at column ``r0 - r0 % 4`` and run to ``n`` in steps of ``cols``, rounded up to a multiple of 4 so that every
    rectangle starts on one.  Every pair ``i < j`` lies in exactly one rectangle; a rectangle that would hold none is left out;
    nothing left of the diagonal block is multiplied."""
    cols = -(-cols // 4) * 4
    for r0 in range(0, n, rows):
        for c0 in range(r0 - r0 % 4, n, cols):
            nc = min(cols, n - c0)
            if c0 + nc - 1 > r0:
                yield r0, min(rows, n - r0), c0, nc


def check_threshold(threshold) -> float:
    """A finite float, before a device is touched."""
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError(f"threshold must be a finite float, got {threshold!r}") from None
    if not math.isfinite(threshold):
        raise ValueError(f"threshold must be a finite float, got {threshold!r}")
    return threshold


def _check_states(what: str, *states) -> int:
    """K24's states: 1-D int32 device tensors with unit stride, all on one device and of one length, which is returned."""
    first = states[0]
    for s in states:
        if (s.ndim != 1 or s.dtype != torch.int32 or not s.is_cuda or s.device != first.device or s.shape != first.shape
                or (s.numel() > 1 and s.stride(0) != 1)):
            raise ValueError(f"{what}: a state is a 1-D int32 device tensor with unit stride, all on one device and of one length, "
                             f"got {tuple(s.shape)} {s.dtype} on {s.device}")
    return first.shape[0]


def _check_status(what: str, status: torch.Tensor, device):
    if tuple(status.shape) != (1,) or status.dtype != torch.int32 or status.device != device:
        raise ValueError(f"{what}: the status word is one int32 on {device}, got {tuple(status.shape)} {status.dtype} on {status.device}")


def unionfind_new(n: int, device) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The empty state ``(parent (n,), degree (n,), status (1,))``, all int32: ``parent[i] = i``, zeros."""
    parent = torch.empty(n, dtype=torch.int32, device=device)
    degree = torch.empty(n, dtype=torch.int32, device=device)
    status = torch.empty(1, dtype=torch.int32, device=device)
    with _on(parent.device):
        _check(lib().sl_unionfind_init(_ptr(parent), _ptr(degree), _ptr(status), n, _stream(parent)), "sl_unionfind_init")
    return parent, degree, status


def threshold_union_merge(parent: torch.Tensor, degree: torch.Tensor, status: torch.Tensor, cand: torch.Tensor, threshold: float,
                          row_id_base: int = 0, col_id_base: int = 0):
    """Fold the ``(R, B)`` fp32 tile ``cand`` (unit column stride, any row stride) into the forest and the degrees of ``n``
    components: every element with ``row_id_base + r < col_id_base + c`` and a value ``>= threshold`` is an edge."""
    n = _check_states("threshold_union_merge", parent, degree)
    _check_status("threshold_union_merge", status, parent.device)
    _check_cand_tile("threshold_union_merge", cand, parent.device)
    R, B = cand.shape
    cand, ld = _tile_view(cand)
    with _on(cand.device):
        rc = lib().sl_threshold_union_merge(_ptr(parent), _ptr(degree), _ptr(status), n, _ptr(cand), ld, R, B, row_id_base, col_id_base,
                                            check_threshold(threshold), _stream(cand))
    _check(rc, "sl_threshold_union_merge")


def unionfind_flatten(parent: torch.Tensor, status: torch.Tensor):
    """``parent[i] = `` its root.  After the last tile ``parent`` holds the labels: the smallest id of every component's group."""
    _check_states("unionfind_flatten", parent)
    _check_status("unionfind_flatten", status, parent.device)
    with _on(parent.device):
        _check(lib().sl_unionfind_flatten(_ptr(parent), parent.shape[0], _ptr(status), _stream(parent)), "sl_unionfind_flatten")


def group_min_merge(state: torch.Tensor, labels: torch.Tensor, cand: torch.Tensor, row_id_base: int = 0, col_id_base: int = 0):
    """Fold the tile into ``state (n,)`` int32 (``torch.full(-1)`` is the empty state): entry ``label`` takes the smallest order
    key among the upper-triangle elements whose row and column both carry ``label`` in ``labels (n,)`` int32."""
    n = _check_states("group_min_merge", state, labels)
    _check_cand_tile("group_min_merge", cand, state.device)
    R, B = cand.shape
    cand, ld = _tile_view(cand)
    with _on(cand.device):
        rc = lib().sl_group_min_merge(_ptr(state), _ptr(labels), n, _ptr(cand), ld, R, B, row_id_base, col_id_base, _stream(cand))
    _check(rc, "sl_group_min_merge")


def group_min_finish(state: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """``(n,)`` float32: the value at ``state[labels[i]]``, NaN for the empty entry."""
    n = _check_states("group_min_finish", state, labels)
    out = torch.empty(n, dtype=torch.float32, device=labels.device)
    with _on(labels.device):
        _check(lib().sl_group_min_finish(_ptr(state), _ptr(labels), n, _ptr(out), _stream(labels)), "sl_group_min_finish")
    return out


def redundancy_probe(x: torch.Tensor, threshold: float, chunk_rows: int | None = None, chunk_cols: int | None = None,
                     cohesion: bool = False):
    """The connected components of the graph "cosine >= threshold" over the rows of ``x (C, D)``, as ``(labels (C,) int64,
    degree (C,) int32, cohesion (C,) float32 | None)``: a row's label is the smallest row id of its group, its degree the number
    of OTHER rows at or above the threshold, its cohesion the smallest pairwise cosine inside its group (NaN for a singleton).
    A NaN cosine is never an edge, a tie at the threshold is, the diagonal is not.

    The cosine GEMM (K6, in the arithmetic ``set_gemm_mode`` selects) writes one reused tile of the ``upper_tile_walk`` — the
    upper triangle only, about half the products of ``mutual_probe(x, x)`` — and K24 folds it into a union-find forest and the
    degrees on the same stream, then flattens the forest, so that the chains are short for the next tile and the flatten after
    the last tile leaves the labels.  The status word is read once, at the end.  ``cohesion=True`` walks the tiles a second
    time with the final labels.  ``tile_plan`` has the default tile."""
    threshold = check_threshold(threshold)
    _check_probe_args("redundancy_probe", x, x, chunk_rows=chunk_rows, chunk_cols=chunk_cols)
    n = x.shape[0]
    if n > REDGROUPS_MAX_N:
        raise ValueError(f"redundancy_probe: more than {REDGROUPS_MAX_N} rows do not fit the forest's int32 ids")
    xd = _f32c(x)
    if n < 2:  # nothing to pair: no launch
        labels = torch.zeros(n, dtype=torch.int64, device=xd.device)
        nan = torch.full((n,), float("nan"), dtype=torch.float32, device=xd.device) if cohesion else None
        return labels, torch.zeros(n, dtype=torch.int32, device=xd.device), nan
    rows, cols = tile_plan(n, n, chunk_rows, chunk_cols)
    cols = -(-cols // 4) * 4  # the walk's step
    parent, degree, status = unionfind_new(n, xd.device)
    for r0, _, c0, _, out in _cosine_tiles(xd, xd, rows, cols, upper_tile_walk(n, rows, cols)):
        threshold_union_merge(parent, degree, status, out, threshold, r0, c0)
        unionfind_flatten(parent, status)
    if int(status.item()):
        raise RuntimeError("redundancy_probe: a union-find loop passed its cap of n + 1 steps; the forest's invariant was broken")
    coh = None
    if cohesion:
        state = torch.full((n,), -1, dtype=torch.int32, device=xd.device)
        for r0, _, c0, _, out in _cosine_tiles(xd, xd, rows, cols, upper_tile_walk(n, rows, cols)):
            group_min_merge(state, parent, out, r0, c0)
        coh = group_min_finish(state, parent)
    return parent.to(torch.int64), degree, coh


# ------------------------------------------------------------------------------------------------
# K16
# ------------------------------------------------------------------------------------------------
BN_MAX_CHANNELS = 4096
BN_MAX_ELEMENTS = (1 << 31) - 1


def batchnorm_infer(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float,
                    relu: bool = False, residual: torch.Tensor | None = None) -> torch.Tensor:
    """Inference BatchNorm2d of a contiguous NCHW fp32 device tensor into a fresh tensor, bit for bit what
    ``F.batch_norm(..., training=False)`` gives, with ``relu_`` (``relu=True``) or ``relu_(y + residual)`` (``residual`` given) fused
    in.  The caller has checked dtype, layout and alignment (``component_visualization/_bn_fuse.py``); the library re-checks what
    it can see."""
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    with _on(x.device):
        if residual is None:
            rc = lib().sl_batchnorm_infer(_ptr(x), B, C, H * W, _ptr(mean), _ptr(var), _ptr(weight), _ptr(bias), float(eps),
                                          1 if relu else 0, _ptr(out), _stream(x))
        else:
            rc = lib().sl_batchnorm_infer_add_relu(_ptr(x), _ptr(residual), B, C, H * W, _ptr(mean), _ptr(var), _ptr(weight),
                                                   _ptr(bias), float(eps), _ptr(out), _stream(x))
    _check(rc, "sl_batchnorm_infer")
    return out


BN_DUAL_MAX_CHANNELS = 2048  # two constant tables per block: half of BN_MAX_CHANNELS


def batchnorm_infer_add_bn_relu(xa: torch.Tensor, bn_a, xb: torch.Tensor, bn_b) -> torch.Tensor:
    """``relu_(F.batch_norm(xa, *bn_a) + F.batch_norm(xb, *bn_b))`` of two contiguous NCHW fp32 device tensors of one shape in one
    pass, bit for bit (K19).  ``bn_a`` and ``bn_b`` are ``(mean, var, weight, bias, eps)``; ``xa`` is the left operand of the add.
    Raises ``ValueError`` for what the entry point does not take (more than ``BN_DUAL_MAX_CHANNELS`` channels among it)."""
    if xa.shape != xb.shape or xa.dim() != 4 or xa.device != xb.device:
        raise ValueError(f"batchnorm_infer_add_bn_relu: two 4-D tensors of one shape and device expected, got {tuple(xa.shape)} and "
                         f"{tuple(xb.shape)}")
    B, C, H, W = xa.shape
    for t in (xa, xb):
        if t.dtype is not torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError("batchnorm_infer_add_bn_relu: inputs must be contiguous NCHW fp32, 16-byte aligned")
    for p in (*bn_a[:4], *bn_b[:4]):
        if p.dtype is not torch.float32 or p.device != xa.device or not p.is_contiguous() or p.numel() != C:
            raise ValueError(f"batchnorm_infer_add_bn_relu: per-channel tensors must be contiguous fp32 of {C} elements on {xa.device}")
    out = torch.empty_like(xa)
    with _on(xa.device):
        rc = lib().sl_batchnorm_infer_add_bn_relu(_ptr(xa), *(_ptr(p) for p in bn_a[:4]), float(bn_a[4]), _ptr(xb),
                                                  *(_ptr(p) for p in bn_b[:4]), float(bn_b[4]), B, C, H * W, _ptr(out), _stream(xa))
    _check(rc, "sl_batchnorm_infer_add_bn_relu")
    return out


BN_POOL_MAX_WIDTH = 4096
BN_POOL_STAGE_BYTES = 64 * 1024  # a plane with more bytes of rows than this is pooled in bands of rows


def bn_pool_supported(kernel_size, stride, padding) -> bool:
    """Whether ``sl_batchnorm_infer_relu_maxpool`` takes these per-axis (h, w) pool parameters."""
    return all(k in (2, 3) and s in (1, 2) and 0 <= p <= k // 2 for k, s, p in zip(kernel_size, stride, padding))


def batchnorm_infer_relu_maxpool(x: torch.Tensor, mean: torch.Tensor, var: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor,
                                 eps: float, kernel_size, stride, padding) -> torch.Tensor:
    """``F.max_pool2d(relu_(F.batch_norm(x, ..., training=False)), kernel_size, stride, padding)`` of a contiguous NCHW fp32 device
    tensor in one pass, bit for bit (K18).  ``kernel_size``, ``stride`` and ``padding`` are (h, w) pairs; the library refuses
    what ``bn_pool_supported`` does not list."""
    B, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw) = kernel_size, stride, padding
    oh, ow = ((n + 2 * p - k) // s + 1 if s > 0 else 0 for n, k, s, p in ((H, kh, sh, ph), (W, kw, sw, pw)))
    out = torch.empty((B, C, max(oh, 0), max(ow, 0)), dtype=x.dtype, device=x.device)
    with _on(x.device):
        rc = lib().sl_batchnorm_infer_relu_maxpool(_ptr(x), B, C, H, W, _ptr(mean), _ptr(var), _ptr(weight), _ptr(bias),
                                                   float(eps), kh, kw, sh, sw, ph, pw, _ptr(out), _stream(x))
    _check(rc, "sl_batchnorm_infer_relu_maxpool")
    return out


# ------------------------------------------------------------------------------------------------
# K27
# ------------------------------------------------------------------------------------------------
CONV_TAIL_IN, CONV_TAIL_OUT = 64, 256  # the one pointwise shape the kernels take
CONV_TAIL_SPLITS = 7  # candidates for how the GEMM behind a 1x1 convolution cuts K = 64 into partial sums (semanticlens_amd.h)
CONV_TAIL_MAX_ELEMENTS = (1 << 31) - 1  # of the output


def _conv_tail_operands(what: str, x: torch.Tensor, w: torch.Tensor):
    if x.dim() != 4 or x.shape[1] != CONV_TAIL_IN or w.numel() != CONV_TAIL_IN * CONV_TAIL_OUT or w.shape[:2] != (CONV_TAIL_OUT,
                                                                                                                 CONV_TAIL_IN):
        raise ValueError(f"{what}: a (N, {CONV_TAIL_IN}, H, W) input and a ({CONV_TAIL_OUT}, {CONV_TAIL_IN}[, 1, 1]) weight expected, "
                         f"got {tuple(x.shape)} and {tuple(w.shape)}")
    for t in (x, w):
        if t.dtype is not torch.float32 or not t.is_cuda or t.device != x.device or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{what}: operands must be contiguous fp32 on one HIP device, 16-byte aligned")
    B, _, H, W = x.shape
    return B, H, W


def _conv_tail_out(x: torch.Tensor) -> torch.Tensor:
    return torch.empty((x.shape[0], CONV_TAIL_OUT, x.shape[2], x.shape[3]), dtype=x.dtype, device=x.device)


def _conv_tail_bn(what: str, x: torch.Tensor, bn):
    for p in bn[:4]:
        if p.dtype is not torch.float32 or p.device != x.device or not p.is_contiguous() or p.numel() != CONV_TAIL_OUT:
            raise ValueError(f"{what}: per-channel tensors must be contiguous fp32 of {CONV_TAIL_OUT} elements on {x.device}")


def conv1x1_64_256(x: torch.Tensor, w: torch.Tensor, split: int, k_order: torch.Tensor | None = None) -> torch.Tensor:
    """The raw product of a 64 -> 256 channel pointwise convolution (no bias) under partial-sum candidate ``split``; ``k_order``
    (64 int32 on the device) is the order in which the MFMA steps take the input channels, ascending when None."""
    B, H, W = _conv_tail_operands("conv1x1_64_256", x, w)
    out = _conv_tail_out(x)
    if k_order is not None and (k_order.dtype is not torch.int32 or k_order.device != x.device or k_order.numel() != CONV_TAIL_IN
                                or not k_order.is_contiguous()
                                or sorted(k_order.tolist()) != list(range(CONV_TAIL_IN))):
        raise ValueError("conv1x1_64_256: k_order must be a permutation of 0..63 as contiguous int32 on the input's device")
    with _on(x.device):
        rc = lib().sl_conv1x1_64_256(_ptr(x), _ptr(w), B, H * W, int(split), _ptr(k_order), _ptr(out), _stream(x))
    _check(rc, "sl_conv1x1_64_256")
    return out


def conv1x1_bn_add_relu(x: torch.Tensor, w: torch.Tensor, bn, identity: torch.Tensor) -> torch.Tensor:
    """``relu_(F.batch_norm(F.conv2d(x, w), *bn) + identity)`` in one pass; ``bn`` is ``(mean, var, weight, bias, eps)``."""
    B, H, W = _conv_tail_operands("conv1x1_bn_add_relu", x, w)
    out = _conv_tail_out(x)
    _conv_tail_bn("conv1x1_bn_add_relu", x, bn)
    if (identity.shape != out.shape or identity.dtype is not torch.float32 or identity.device != x.device
            or not identity.is_contiguous() or identity.data_ptr() % 16):
        raise ValueError(f"conv1x1_bn_add_relu: the identity must be contiguous fp32 of shape {tuple(out.shape)} on {x.device}")
    with _on(x.device):
        rc = lib().sl_conv1x1_bn_add_relu(_ptr(x), _ptr(w), *(_ptr(p) for p in bn[:4]), float(bn[4]), _ptr(identity), B, H * W,
                                          _ptr(out), _stream(x))
    _check(rc, "sl_conv1x1_bn_add_relu")
    return out


def conv1x1_bn_add_conv1x1_bn_relu(xa: torch.Tensor, wa: torch.Tensor, bn_a, xb: torch.Tensor, wb: torch.Tensor,
                                   bn_b) -> torch.Tensor:
    """``relu_(F.batch_norm(F.conv2d(xa, wa), *bn_a) + F.batch_norm(F.conv2d(xb, wb), *bn_b))`` in one pass; ``xa``'s side is the
    left operand of the add, as in ``batchnorm_infer_add_bn_relu``."""
    what = "conv1x1_bn_add_conv1x1_bn_relu"
    B, H, W = _conv_tail_operands(what, xa, wa)
    _conv_tail_operands(what, xb, wb)
    if xb.shape != xa.shape or xb.device != xa.device:
        raise ValueError(f"{what}: two inputs of one shape and device expected, got {tuple(xa.shape)} and {tuple(xb.shape)}")
    _conv_tail_bn(what, xa, bn_a)
    _conv_tail_bn(what, xa, bn_b)
    out = _conv_tail_out(xa)
    with _on(xa.device):
        rc = lib().sl_conv1x1_bn_add_conv1x1_bn_relu(_ptr(xa), _ptr(wa), *(_ptr(p) for p in bn_a[:4]), float(bn_a[4]), _ptr(xb),
                                                     _ptr(wb), *(_ptr(p) for p in bn_b[:4]), float(bn_b[4]), B, H * W,
                                                     _ptr(out), _stream(xa))
    _check(rc, what)
    return out


# ------------------------------------------------------------------------------------------------
# measurement
# ------------------------------------------------------------------------------------------------
def prof_enable(on: bool = True):
    _check(lib().sl_prof_enable(1 if on else 0), "sl_prof_enable")


def prof_reset():
    _check(lib().sl_prof_reset(), "sl_prof_reset")


def prof_read(family: int):
    """(total_ms, launches, work) for one kernel family; synchronises the recorded events."""
    ms, n, w = ctypes.c_double(), _i64(), ctypes.c_double()
    _check(lib().sl_prof_read(family, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(w)), "sl_prof_read")
    return ms.value, n.value, w.value


# ------------------------------------------------------------------------------------------------
# K9
# ------------------------------------------------------------------------------------------------
POLY2_MAX_N = 128  # sl_poly2means keeps a component's state in LDS; larger n / other k: sl_polykmeans


POLYK_MAX_N = 1024        # sl_polykmeans: samples per component (kMaxNGeneral in csrc/kmeans.hip)
POLYK_MAX_CLUSTERS = 16   # sl_polykmeans: n_clusters (kMaxClusters)
POLYK_MAX_COMPONENTS = 65535  # components per launch (grid.y of the Gram kernel)


def _poly_ws_budget() -> int:
    """Workspace bytes one K9 launch may take (default 8 GiB; ``SL_POLY_WS_GB``).  More components than fit run as
    consecutive launches over component chunks — every component is independent, so the scores do not change."""
    import os

    return int(float(os.environ.get("SL_POLY_WS_GB", "8")) * (1 << 30))


FACET_MAX_CLUSTERS = 16  # sl_facet_stats: n_clusters (kMaxFacets in csrc/facets.hip)
FACET_MAX_N = 1024       # sl_facet_stats: samples per component


def _facet_stats_into(Vd: torch.Tensor, labels: torch.Tensor, n_clusters: int, centres, counts, clarity):
    """One ``sl_facet_stats`` call on contiguous device tensors; the caller holds the device guard."""
    C, n, D = Vd.shape
    rc = lib().sl_facet_stats(_ptr(Vd), C, n, D, _ptr(labels), int(n_clusters), _ptr(centres), _ptr(counts), _ptr(clarity), _stream(Vd))
    _check(rc, "sl_facet_stats")


def facet_stats(V: torch.Tensor, labels: torch.Tensor, n_clusters: int, clarity: bool = True):
    """K21: per component of ``V (C, n, D)`` and cluster ``j`` of ``labels (C, n)``: ``(centres (C, kc, D) float32 — the mean of
    the raw rows with label ``j`` —, counts (C, kc) int32, clarity (C, kc) float32 or None)``, on the device.  A label outside
    ``[0, n_clusters)`` belongs to no facet; an empty facet has a zero centre, a facet of fewer than two rows a NaN clarity."""
    if V.ndim != 3 or labels.ndim != 2 or tuple(labels.shape) != tuple(V.shape[:2]):
        raise ValueError(f"facet_stats expects V (C, n, D) and labels (C, n), got {tuple(V.shape)} and {tuple(labels.shape)}")
    if not 1 <= n_clusters <= FACET_MAX_CLUSTERS:
        raise ValueError(f"n_clusters={n_clusters} not in [1, {FACET_MAX_CLUSTERS}]")
    if V.shape[1] > FACET_MAX_N:
        raise ValueError(f"n_samples={V.shape[1]} exceeds the device kernel's maximum of {FACET_MAX_N} samples per component")
    Vd = _f32c(V)
    ld = to_device(labels, Vd.device).to(torch.int32).contiguous()
    C, n, D = Vd.shape
    centres = torch.empty((C, n_clusters, D), dtype=torch.float32, device=Vd.device)
    counts = torch.empty((C, n_clusters), dtype=torch.int32, device=Vd.device)
    clar = torch.empty((C, n_clusters), dtype=torch.float32, device=Vd.device) if clarity else None
    if C and n and D:
        with _on(Vd.device):
            _facet_stats_into(Vd, ld, n_clusters, centres, counts, clar)
    else:  # nothing to read: every facet is empty
        centres.zero_()
        counts.zero_()
        if clar is not None:
            clar.fill_(float("nan"))
    return centres, counts, clar


SIL_MAX_N = 1024        # sl_silhouette: samples per component (kSilMaxN in csrc/silhouette.hip)
SIL_MAX_CLUSTERS = 16   # sl_silhouette: n_clusters (kSilMaxClusters)
SIL_MAX_SETS = 15       # sl_silhouette: label sets per call (kSilMaxSets)
SIL_METRICS = {"euclidean": 0, "cosine": 1}


def check_silhouette_metric(metric) -> int:
    """``metric`` as ``sl_silhouette``'s code; ``ValueError`` for anything but ``"euclidean"`` and ``"cosine"``."""
    if not isinstance(metric, str) or metric not in SIL_METRICS:
        raise ValueError(f"metric={metric!r} is not one of {sorted(SIL_METRICS)}")
    return SIL_METRICS[metric]


def silhouette(V: torch.Tensor, labels: torch.Tensor, n_clusters: int, metric: str = "euclidean", samples: bool = True):
    """K23: scikit-learn's ``silhouette_samples`` / ``silhouette_score`` of every component of ``V (C, n, D)`` under ``labels
    (C, n)`` or ``(m, C, n)`` int32 (``m`` label sets, one read of ``V``): ``(samples float64 shaped like labels, or None; mean
    float64 (C,) or (m, C))``, on the device.  A label outside ``[0, n_clusters)`` takes the sample out (NaN, not part of the
    mean); fewer than two non-empty clusters give NaN.

    Any number of components: calls are chunked by the Gram kernel's grid limit (65 535 components) and by the workspace
    budget K9 uses — every component is independent, so the results do not change."""
    if V.ndim != 3 or labels.ndim not in (2, 3) or tuple(labels.shape[-2:]) != tuple(V.shape[:2]):
        raise ValueError(f"silhouette expects V (C, n, D) and labels (C, n) or (m, C, n), got {tuple(V.shape)} and {tuple(labels.shape)}")
    if labels.dtype != torch.int32:
        raise ValueError(f"labels must be int32, got {labels.dtype}")
    C, n, D = V.shape
    m = labels.shape[0] if labels.ndim == 3 else 1
    if not 1 <= m <= SIL_MAX_SETS:
        raise ValueError(f"m={m} label sets not in [1, {SIL_MAX_SETS}]")
    if isinstance(n_clusters, bool) or not isinstance(n_clusters, int) or not 2 <= n_clusters <= SIL_MAX_CLUSTERS:
        raise ValueError(f"n_clusters={n_clusters!r} not in [2, {SIL_MAX_CLUSTERS}]")
    if not 2 <= n <= SIL_MAX_N:
        raise ValueError(f"n_samples={n} not in [2, {SIL_MAX_N}]: the device kernel's range of samples per component")
    if D < 1:
        raise ValueError(f"D={D}: at least one feature")
    code = check_silhouette_metric(metric)
    Vd = _f32c(V)
    ld = to_device(labels, Vd.device).contiguous().view(m, C, n)
    dev = Vd.device
    out_s = torch.empty((m, C, n), dtype=torch.float64, device=dev) if samples else None
    out_m = torch.empty((m, C), dtype=torch.float64, device=dev)
    if C:
        per_comp = n * n * 8
        chunk = max(1, min(C, POLYK_MAX_COMPONENTS, _poly_ws_budget() // per_comp))
        ws = None
        with _on(dev):
            for c0 in range(0, C, chunk):
                cc = min(chunk, C - c0)
                whole = cc == C
                # a chunk of the (m, C, ...) tensors is not contiguous: it goes through contiguous copies
                lc = ld if whole else ld[:, c0:c0 + cc].contiguous()
                sc = out_s if whole or out_s is None else torch.empty((m, cc, n), dtype=torch.float64, device=dev)
                mc = out_m if whole else torch.empty((m, cc), dtype=torch.float64, device=dev)
                nbytes = int(lib().sl_silhouette_ws_bytes(cc, n, D))
                if ws is None:
                    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                rc = lib().sl_silhouette(_ptr(Vd[c0:c0 + cc]), cc, n, D, _ptr(lc), m, n_clusters, code, _ptr(sc), _ptr(mc), _ptr(ws),
                                         nbytes, _stream(Vd))
                _check(rc, "sl_silhouette")
                if not whole:
                    out_m[:, c0:c0 + cc] = mc
                    if out_s is not None:
                        out_s[:, c0:c0 + cc] = sc
    if labels.ndim == 2:
        return (out_s[0] if out_s is not None else None), out_m[0]
    return out_s, out_m


def poly2means(V: torch.Tensor, first_center, rand, replace_empty_clusters: bool = True, n_clusters: int = 2, labels=None,
               stats=None) -> torch.Tensor:
    """polysemanticity of V (C,n,D): k-means per component on the device; float64 (C,) result.

    ``labels``: a ``(C, n)`` int32 device tensor that receives scikit-learn's ``labels_`` of the clustering each score comes
    from (K21; ``sl_*_labels``).  ``stats``: with ``labels``, ``(centres (C, kc, D) f32, counts (C, kc) i32, clarity (C, kc) f32)``
    device tensors filled by ``sl_facet_stats`` chunk by chunk, right behind the chunk's clustering.

    Any number of components: calls are chunked by the Gram kernel's grid limit (65 535 components) and by the workspace
    budget.  ``n_samples > 1024`` with ``n_clusters != 2`` (or > 128 samples), and ``n_clusters > 16``, raise
    ``ValueError`` — limits the reference (scikit-learn on the host, scores.py:131-185) does not have."""
    import numpy as np

    Vd = _f32c(V)
    if Vd.ndim != 3:
        raise ValueError("polysemanticity_score expects a (n_components, n_samples, n_features) tensor")
    C, n, D = Vd.shape
    first_center = np.ascontiguousarray(first_center, dtype=np.int32)
    rand = np.ascontiguousarray(rand, dtype=np.float64)
    n_init = int(first_center.shape[0])
    out = torch.empty((C,), dtype=torch.float64, device=Vd.device)
    mincnt = torch.empty((C,), dtype=torch.int32, device=Vd.device)
    if labels is not None and not (labels.is_cuda and labels.dtype == torch.int32 and labels.is_contiguous() and tuple(labels.shape) == (C, n)):
        raise ValueError(f"labels must be a contiguous ({C}, {n}) int32 device tensor")
    if stats is not None and labels is None:
        raise ValueError("stats are computed from the labels: pass labels too")
    general = n_clusters != 2 or n > POLY2_MAX_N
    if general:
        if n_clusters > POLYK_MAX_CLUSTERS:
            raise ValueError(f"n_clusters={n_clusters} exceeds the device kernel's maximum of {POLYK_MAX_CLUSTERS}")
        if n > POLYK_MAX_N:
            raise ValueError(f"n_samples={n} exceeds the device kernel's maximum of {POLYK_MAX_N} samples per component")
    if C == 0:
        return out
    # the storage variant (csrc/kmeans.hip): entry point family, the arguments only it takes (ws_bytes: after C, n, D; the call:
    # after D), and whether the call still reads the host arrays of the draws after it returns
    name, ws_extra, call_extra, reads_host_async = \
        ("sl_polykmeans", (int(n_clusters), n_init), (int(n_clusters),), True) if general else ("sl_poly2means", (), (), False)
    ws_bytes, entry = getattr(lib(), name + "_ws_bytes"), getattr(lib(), name if labels is None else name + "_labels")
    chunk = max(1, min(C, POLYK_MAX_COMPONENTS, _poly_ws_budget() // max(int(ws_bytes(1, n, D, *ws_extra)), 1)))
    ws = None
    with _on(Vd.device):
        for c0 in range(0, C, chunk):
            cc = min(chunk, C - c0)
            Vc, oc, mc = Vd[c0:c0 + cc], out[c0:c0 + cc], mincnt[c0:c0 + cc]
            lc = labels[c0:c0 + cc] if labels is not None else None
            nbytes = int(ws_bytes(cc, n, D, *ws_extra))
            if ws is None or ws.numel() < nbytes:
                ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=Vd.device)
            rc = entry(_ptr(Vc), cc, n, D, *call_extra, first_center.ctypes.data_as(_vp), n_init, rand.ctypes.data_as(_vp),
                       1 if replace_empty_clusters else 0, _ptr(oc), _ptr(mc), *(() if lc is None else (_ptr(lc),)), _ptr(ws), nbytes,
                       _stream(Vd))
            if reads_host_async:
                torch.cuda.current_stream(Vd.device).synchronize()  # the draws were copied from host arrays owned by this call
            _check(rc, name)
            if stats is not None:
                _facet_stats_into(Vc, lc, n_clusters, *(t[c0:c0 + cc] for t in stats))
    return out


# ------------------------------------------------------------------------------------------------
# K11: native transformer-tower primitives (all on torch's current stream, fp32, contiguous)
# ------------------------------------------------------------------------------------------------
def linear(x, w, bias=None, act=SL_ACT_NONE, residual=None, out=None, scatter=None, rowadd=None):
    """out = act(x @ w.T + bias) (+ residual).  x (M,K), w (N,K).  ``scatter=(rows_per_group, group_stride,
    row_offset)`` writes row r to (r // rpg) * group_stride + row_offset + r % rpg of ``out`` (+ ``rowadd`` rows)."""
    M, K = x.shape
    Nn = w.shape[0]
    _need_f32("linear", x, w, bias, residual, out, rowadd)
    if out is None:
        out = torch.empty((M, Nn), dtype=torch.float32, device=x.device)
    rpg, gs, ro = scatter if scatter is not None else (0, 0, 0)
    with _on(x.device):
        rc = lib().sl_linear(_ptr(x), M, K, _ptr(w), Nn, _ptr(bias), act, _ptr(residual), _ptr(out), out.stride(0) if out.ndim == 2 else Nn,
                             rpg, gs, ro, _ptr(rowadd), _stream(x))
    _check(rc, "sl_linear")
    return out


class Split:
    """An fp32 matrix carried as a split matrix (hi = bf16(v), lo = bf16(v - hi)): operand of the bf16x3 GEMM.

    One buffer of ``rows x 2 Kp`` bf16 values, ``Kp`` = ``cols`` rounded up to 32 and zero padded; each 32-wide k-tile of a
    row is one 128-byte line ``[hi(32) | lo(32)]`` (``include/semanticlens_amd.h``).  ``hi`` / ``lo`` materialise the two
    halves as ``(rows, cols)`` bf16 tensors (tests, debugging)."""

    def __init__(self, rows: int, cols: int, device):
        self.shape = (rows, cols)
        self.kp = (cols + 31) // 32 * 32
        # producers write columns < cols only; the padding (if any) must read as zero in the GEMM
        alloc = torch.empty if self.kp == cols else torch.zeros
        self.buf = alloc((rows, 2 * self.kp), dtype=torch.bfloat16, device=device)
        assert self.buf.numel() == int(lib().sl_split_elems(rows, cols))

    def _half(self, which: int) -> torch.Tensor:
        rows, cols = self.shape
        return self.buf.view(rows, self.kp // 32, 2, 32)[:, :, which, :].reshape(rows, self.kp)[:, :cols]

    @property
    def hi(self) -> torch.Tensor:
        return self._half(0)

    @property
    def lo(self) -> torch.Tensor:
        return self._half(1)

    @classmethod
    def of(cls, x: torch.Tensor, row_scale: torch.Tensor | None = None) -> "Split":
        _need_f32("Split.of", x, row_scale)
        x = x.contiguous()
        out = cls(x.shape[0], x.shape[1], x.device)
        with _on(x.device):
            rc = lib().sl_split_bf16(_ptr(x), _ptr(row_scale), x.shape[0], x.shape[1], _ptr(out.buf), _stream(x))
        _check(rc, "sl_split_bf16")
        return out


def _split_ptr(sp):
    return _ptr(sp.buf) if sp is not None else _vp(None)


def linear3(x: Split, w: Split, bias=None, act=SL_ACT_NONE, residual=None, out=None, out_split: Split | None = None,
            scatter=None, rowadd=None):
    """bf16x3 version of :func:`linear`: x, w are :class:`Split` operands; the result is fp32 ``out`` (optionally
    + residual, or scattered rows) or, with ``out_split``, split bf16 ready to feed the next GEMM."""
    M, K = x.shape
    Nn = w.shape[0]
    dev = x.buf.device
    _need_f32("linear3", bias, residual, out, rowadd)
    if w.shape[1] != K:
        raise ValueError(f"linear3: x has {K} columns, w has {w.shape[1]}")
    if out is None and out_split is None:
        out = torch.empty((M, Nn), dtype=torch.float32, device=dev)
    ldo = out.stride(0) if out is not None else Nn
    rpg, gs, ro = scatter if scatter is not None else (0, 0, 0)
    with _on(dev):
        rc = lib().sl_linear_bf16x3(_ptr(x.buf), M, K, _ptr(w.buf), Nn, _ptr(bias), act, _ptr(residual), _ptr(out),
                                    _split_ptr(out_split), ldo, rpg, gs, ro, _ptr(rowadd), _stream(x.buf))
    _check(rc, "sl_linear_bf16x3")
    return out if out is not None else out_split


def layernorm(x, gamma, beta, eps, out=None, rows=None, x_row_stride=None, out_split: Split | None = None):
    _need_f32("layernorm", x, gamma, beta, out)
    cols = x.shape[-1]
    rows = rows if rows is not None else x.numel() // cols
    xs = x_row_stride if x_row_stride is not None else cols
    if out is None and out_split is None:
        out = torch.empty((rows, cols), dtype=torch.float32, device=x.device)
    with _on(x.device):
        rc = lib().sl_layernorm(_ptr(x), rows, cols, xs, _ptr(gamma), _ptr(beta), float(eps), _ptr(out), _split_ptr(out_split),
                                cols, _stream(x))
    _check(rc, "sl_layernorm")
    return out if out is not None else out_split


def attention(qkv, B, T, H, head_dim, causal, out=None, out_split: Split | None = None, bf16x3: bool = False):
    """softmax(q k^T / sqrt(d)) v per (batch, head).  ``bf16x3``: both products in the split-bf16 x3 arithmetic of
    :func:`linear3` (``sl_attention_bf16x3``) instead of fp32-input MFMAs."""
    _need_f32("attention", qkv, out)
    if out is None and out_split is None:
        out = torch.empty((B * T, H * head_dim), dtype=torch.float32, device=qkv.device)
    fn = lib().sl_attention_bf16x3 if bf16x3 else lib().sl_attention
    with _on(qkv.device):
        rc = fn(_ptr(qkv), B, T, H, head_dim, 1 if causal else 0, _ptr(out), _split_ptr(out_split), _stream(qkv))
    _check(rc, "sl_attention_bf16x3" if bf16x3 else "sl_attention")
    return out if out is not None else out_split


def _attention_pool(name, q, q_stride, kv, B, T, H, head_dim, out):
    W = H * head_dim
    _need_f32(name, q, kv, out)
    if out is None:
        out = torch.empty((B, W), dtype=torch.float32, device=kv.device)
    q_args = (_ptr(q),) if q_stride is None else (_ptr(q), q_stride)  # the C entry points differ in this argument only
    with _on(kv.device):
        rc = getattr(lib(), "sl_" + name)(*q_args, _ptr(kv), kv.stride(0), W, B, T, H, head_dim, _ptr(out), _stream(kv))
    _check(rc, "sl_" + name)
    return out


def attention_pool(q, kv, B, T, H, head_dim, out=None):
    """One query per head against the keys / values of each image: ``q`` (H*head_dim) projected probe, ``kv`` (B*T, 2*W)
    rows ``[k | v]`` -> ``(B, W)``."""
    return _attention_pool("attention_pool", q, None, kv, B, T, H, head_dim, out)


def attention_pool_q(q, kv, B, T, H, head_dim, out=None):
    """``attention_pool`` with one query per image: ``q`` (B, H*head_dim) -> ``(B, W)`` (CLIP-ResNet attention pool)."""
    return _attention_pool("attention_pool_q", q, q.stride(0), kv, B, T, H, head_dim, out)


def tokens_from_map(fmap, pos, out=None):
    """(B, C, H, W) trunk output + (HW + 1, C) positions -> (B, HW + 1, C) token rows, row 0 = mean token (``sl_tokens_from_map``)."""
    B, C = fmap.shape[:2]
    S = fmap[0, 0].numel()
    fmap = fmap.contiguous()
    _need_f32("tokens_from_map", fmap, pos, out)
    if out is None:
        out = torch.empty((B, S + 1, C), dtype=torch.float32, device=fmap.device)
    with _on(fmap.device):
        rc = lib().sl_tokens_from_map(_ptr(fmap), B, C, S, _ptr(pos), _ptr(out), _stream(fmap))
    _check(rc, "sl_tokens_from_map")
    return out


def patchify(img, P, out=None, out_split: Split | None = None):
    B, C, Hi, Wi = img.shape
    _need_f32("patchify", img, out)
    if out is None and out_split is None:
        out = torch.empty((B * (Hi // P) * (Wi // P), C * P * P), dtype=torch.float32, device=img.device)
    with _on(img.device):
        rc = lib().sl_patchify(_ptr(img), B, C, Hi, Wi, P, _ptr(out), _split_ptr(out_split), _stream(img))
    _check(rc, "sl_patchify")
    return out if out is not None else out_split


def broadcast_row(v, add, G, group_stride_elems, out):
    with _on(out.device):
        rc = lib().sl_broadcast_row(_ptr(v), _ptr(add), G, group_stride_elems, v.numel(), _ptr(out), _stream(out))
    _check(rc, "sl_broadcast_row")


def embed_tokens(table, ids, pos, out=None):
    B, T = ids.shape
    vocab, W = table.shape
    if out is None:
        out = torch.empty((B * T, W), dtype=torch.float32, device=table.device)
    with _on(table.device):
        rc = lib().sl_embed_tokens(_ptr(table), vocab, _ptr(ids), B, T, W, _ptr(pos), _ptr(out), _stream(table))
    _check(rc, "sl_embed_tokens")
    return out


# ------------------------------------------------------------------------------------------------
# K12: image preprocessing (foundation_models/clip.py:157-163 of the reference runs it per sample on the host)
# ------------------------------------------------------------------------------------------------
def preprocess_plan(hw, size: int, resize_mode: str = "shortest", interp: str = "bicubic", pixel_offsets=None):
    """Host-side plan for a ragged batch: ``hw`` (B, 2) heights/widths -> (plan (B, 16) int64 CPU tensor, info dict).
    Pure host arithmetic inside the library (no device needed)."""
    hw_t = torch.as_tensor(hw, dtype=torch.int32).reshape(-1, 2).contiguous()
    B = hw_t.shape[0]
    plan = torch.zeros((B, SL_PP_PLAN_STRIDE), dtype=torch.int64)
    info = (ctypes.c_int64 * 4)()
    off = None if pixel_offsets is None else torch.as_tensor(pixel_offsets, dtype=torch.int64).contiguous()
    if resize_mode not in PP_RESIZE_MODES or interp not in PP_INTERP:
        raise ValueError(f"unknown resize_mode/interpolation {resize_mode!r}/{interp!r}")
    _check(lib().sl_preprocess_plan(_vp(hw_t.data_ptr()) if B else _vp(None), _vp(off.data_ptr()) if off is not None and B else _vp(None),
                                    B, int(size), PP_RESIZE_MODES[resize_mode], PP_INTERP[interp],
                                    _vp(plan.data_ptr()) if B else _vp(None), ctypes.cast(info, _vp)), "sl_preprocess_plan")
    return plan, {"ws_bytes": int(info[0]), "coef_bytes": int(info[1]), "max_h": int(info[2]), "pixel_bytes": int(info[3])}


def preprocess_plan_rois(hw, boxes, index, size: int, resize_mode: str = "shortest", interp: str = "bicubic",
                         pixel_offsets=None):
    """Plan entries for sub-rectangles: ``hw`` (N, 2) the packed images' heights/widths, ``boxes`` (P, 4) (row1, row2, col1,
    col2) clamped to the image (must stay non-empty), ``index`` (P,) the image of each box -> (plan (P, 16) int64 CPU
    tensor, info dict) for :func:`preprocess`; each result equals the transform of the cropped image."""
    hw_t = torch.as_tensor(hw, dtype=torch.int32).reshape(-1, 2).contiguous()
    box = torch.as_tensor(boxes, dtype=torch.int32).reshape(-1, 4).contiguous()
    idx = torch.as_tensor(index, dtype=torch.int64).reshape(-1).contiguous()
    if idx.shape[0] != box.shape[0]:
        raise ValueError(f"preprocess_plan_rois: {box.shape[0]} boxes for {idx.shape[0]} indices")
    if resize_mode not in PP_RESIZE_MODES or interp not in PP_INTERP:
        raise ValueError(f"unknown resize_mode/interpolation {resize_mode!r}/{interp!r}")
    N_, P = hw_t.shape[0], box.shape[0]
    plan = torch.zeros((P, SL_PP_PLAN_STRIDE), dtype=torch.int64)
    info = (ctypes.c_int64 * 4)()
    off = None if pixel_offsets is None else torch.as_tensor(pixel_offsets, dtype=torch.int64).contiguous()
    _check(lib().sl_preprocess_plan_rois(_vp(hw_t.data_ptr()) if N_ else _vp(None), _vp(off.data_ptr()) if off is not None and N_ else _vp(None),
                                         N_, _vp(idx.data_ptr()) if P else _vp(None), _vp(box.data_ptr()) if P else _vp(None), P,
                                         int(size), PP_RESIZE_MODES[resize_mode], PP_INTERP[interp],
                                         _vp(plan.data_ptr()) if P else _vp(None), ctypes.cast(info, _vp)), "sl_preprocess_plan_rois")
    return plan, {"ws_bytes": int(info[0]), "coef_bytes": int(info[1]), "max_h": int(info[2]), "pixel_bytes": int(info[3])}


def preprocess(pixels: torch.Tensor, plan: torch.Tensor, info: dict, size: int, mean, std, interp: str = "bicubic",
               want_u8: bool = False, want_f32: bool = True):
    """Packed raw RGB bytes on the device + uploaded plan -> (B, 3, size, size) fp32 (and/or (B, size, size, 3) uint8)."""
    if not pixels.is_cuda or pixels.dtype != torch.uint8:
        raise TypeError("pixels must be a uint8 tensor on a HIP device")
    dev = pixels.device
    B = plan.shape[0]
    plan_d = plan.to(dev, non_blocking=True) if not plan.is_cuda else plan
    out = torch.empty((B, 3, size, size), dtype=torch.float32, device=dev) if want_f32 else None
    out_u8 = torch.empty((B, size, size, 3), dtype=torch.uint8, device=dev) if want_u8 else None
    ws = torch.empty((max(info["ws_bytes"], 16),), dtype=torch.uint8, device=dev)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    sd = (ctypes.c_float * 3)(*[float(v) for v in std])
    with _on(dev):
        _check(lib().sl_preprocess(_ptr(pixels), _ptr(plan_d), B, int(size), PP_INTERP[interp], info["max_h"], info["coef_bytes"],
                                   ctypes.cast(m, _vp), ctypes.cast(sd, _vp), _ptr(out), _ptr(out_u8), _ptr(ws),
                                   info["ws_bytes"], _stream(pixels)), "sl_preprocess")
    return out, out_u8


# ------------------------------------------------------------------------------------------------
# K13: heatmap rendering (utils/render.py of the reference loops over the images on the host) and the start relevance
# of a conditional backward
# ------------------------------------------------------------------------------------------------
def render_heatmaps(rel: torch.Tensor, img: torch.Tensor, style: str, kernel_size: int = 51, vis_th: float = 0.02,
                    crop_th: float = 0.01, alpha: float = 0.4, rf: bool = False, want_heat: bool = False):
    """K13 on ``rel`` (B, Cin, H, W) and ``img`` (B, 3, H, W) fp32 device tensors (same device) ->
    ``(heat (B, H, W) fp32 or None, box (B, 4) int32, flags (B,) int32, rgb (B, H, W, 3) uint8)``, all on the device.
    ``box`` is the square crop box (row1, row2, col1, col2), ``flags`` bit 0 = crop applied, bit 1 = mask non-empty; the
    rendered image is ``rgb[b, :h, :w]`` with ``(h, w)`` the box clamped to the image when bit 0 is set, else (H, W).
    The limits on ``kernel_size`` and the plane are checked by the native call only: ``kernel_size`` even, below 1 or with
    ``kernel_size // 2 >= min(H, W)`` raises ``ValueError``; ``kernel_size > 255`` or ``W + kernel_size - 1 > 16384`` raises
    ``NativeLibraryError`` ("exceeds the supported maximum")."""
    if rel.ndim != 4 or img.ndim != 4 or img.shape[1] != 3 or rel.shape[0] != img.shape[0] or rel.shape[2:] != img.shape[2:]:
        raise ValueError(f"render_heatmaps: expected rel (B, Cin, H, W) and img (B, 3, H, W), got {tuple(rel.shape)} and {tuple(img.shape)}")
    if style not in RENDER_STYLES:
        raise ValueError(f"render_heatmaps: style must be one of {sorted(RENDER_STYLES)}, got {style!r}")
    _need_f32("render_heatmaps", rel, img)
    if rel.device != img.device:
        raise ValueError(f"render_heatmaps: rel on {rel.device}, img on {img.device}")
    rel, img = rel.contiguous(), img.contiguous()
    B, Cin, H, W = rel.shape
    dev = rel.device
    heat = torch.empty((B, H, W), dtype=torch.float32, device=dev) if want_heat else None
    box = torch.empty((B, 4), dtype=torch.int32, device=dev)
    flags = torch.empty((B,), dtype=torch.int32, device=dev)
    rgb = torch.zeros((B, H, W, 3), dtype=torch.uint8, device=dev)
    if B == 0:
        return heat, box, flags, rgb
    ws_bytes = lib().sl_render_ws_bytes(B, H, W)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    with _on(dev):
        _check(lib().sl_render_heatmaps(_ptr(rel), B, Cin, H, W, _ptr(img), int(kernel_size), float(vis_th), float(crop_th), float(alpha),
                                        RENDER_STYLES[style], int(bool(rf)), _ptr(heat), _ptr(box), _ptr(flags), _ptr(rgb),
                                        _ptr(ws), ws_bytes, _stream(rel)), "sl_render_heatmaps")
    return heat, box, flags, rgb


def condition_init(act: torch.Tensor, channels, rf: bool) -> torch.Tensor:
    """``grad_outputs`` of a conditional backward from the hooked layer output ``act`` ((B, C, H, W), (B, T, F) with the
    channels on F, or (B, C)): ``rf`` keeps ``act`` at the first argmax position of channel ``channels[i]`` of row ``i``
    only, else the whole channel; zero elsewhere.  Same shape and dtype as ``act``."""
    if not act.is_cuda:
        raise TypeError(f"condition_init: expected a tensor on a HIP device, got {act.device}")
    x = act.detach()
    if x.dtype != torch.float32:
        x = x.float()
    ch = torch.as_tensor(channels, dtype=torch.int64).reshape(-1)
    if ch.numel() != x.shape[0]:
        raise ValueError(f"condition_init: {ch.numel()} channels for {x.shape[0]} rows")
    out = torch.zeros(x.shape, dtype=torch.float32, device=x.device)
    if x.shape[0] == 0 or out.numel() == 0:
        return out.to(act.dtype)
    if x.ndim == 4:
        B, C, H, W = x.shape
        x, sb, sc, ss = _flatten_spatial(x)
        S, ob, oc, os_ = H * W, C * H * W, H * W, 1
    elif x.ndim == 3:  # tokens (B, T, F): the (B, F, T) view
        B, T, C = x.shape
        sb, ss, sc = x.stride()
        S, ob, oc, os_ = T, T * C, 1, C
    elif x.ndim == 2:
        B, C = x.shape
        sb, sc = x.stride()
        S, ss, ob, oc, os_ = 1, 1, C, 1, 1
    else:
        raise ValueError(f"condition_init: layer outputs must be 2-, 3- or 4-D, got {x.ndim}-D")
    if ch.numel() and (int(ch.min()) < 0 or int(ch.max()) >= C):
        raise ValueError(f"condition_init: channel ids must lie in [0, {C}), got {ch.tolist()}")
    ch_d = ch.to(x.device)
    with _on(x.device):
        _check(lib().sl_condition_init(_ptr(x), B, C, S, sb, sc, ss, _ptr(ch_d), int(bool(rf)), _ptr(out), ob, oc, os_, _stream(x)),
               "sl_condition_init")
    return out if act.dtype == torch.float32 else out.to(act.dtype)


# ------------------------------------------------------------------------------------------------
# K14: crop boxes of heatmaps without a canvas
# ------------------------------------------------------------------------------------------------
def check_crop_args(crop_th: float, kernel_size: int, H: int | None = None, W: int | None = None):
    """The limits K14 (and K13) put on the crop arguments, checked on the host before anything runs."""
    if not (isinstance(kernel_size, int) and not isinstance(kernel_size, bool)) or kernel_size < 1 or kernel_size % 2 == 0:
        raise ValueError(f"kernel_size must be an odd positive integer, got {kernel_size!r}")
    if kernel_size > 255:
        raise ValueError(f"kernel_size must be at most 255, got {kernel_size}")
    if not (0.0 <= float(crop_th) < 1.0):
        raise ValueError("'crop_th' must be between [0, 1)")
    if H is not None and W is not None and not (kernel_size // 2 < H and kernel_size // 2 < W):
        raise ValueError(f"kernel_size // 2 = {kernel_size // 2} must be smaller than H and W ({H} x {W}) for reflect padding")


def _layer_view(x: torch.Tensor):
    """A layer output as the (B, C, S) strided view of sl_condition_init: (x, B, C, S, sb, sc, ss, conv grid or None)."""
    if x.ndim == 4:
        B, C, H, W = x.shape
        x, sb, sc, ss = _flatten_spatial(x)
        return x, B, C, H * W, sb, sc, ss, (H, W)
    if x.ndim == 3:  # tokens (B, T, F): the (B, F, T) view
        B, T, C = x.shape
        sb, ss, sc = x.stride()
        return x, B, C, T, sb, sc, ss, None
    if x.ndim == 2:
        B, C = x.shape
        sb, sc = x.stride()
        return x, B, C, 1, sb, sc, 1, (1, 1)
    raise ValueError(f"layer outputs must be 2-, 3- or 4-D, got {x.ndim}-D")


def activation_heat_boxes(act: torch.Tensor, rows, channels, size, kernel_size: int = 51, crop_th: float = 0.01,
                          token_grid=None, prefix_tokens: int = 0, want_heat: bool = False):
    """K14 on a layer output ``act`` ((B, C, H', W'), (B, T, F) tokens with ``token_grid`` (gh, gw) starting at token
    ``prefix_tokens``, or (B, C)) for the pairs (``rows[j]``, ``channels[j]``) at model input ``size`` (H, W) ->
    ``(heat (P, H, W) fp32 or None, box (P, 4) int32)`` on the device.  heat = max(bilinear upsample, 0); box = the
    CROP-style square box of ``render_heatmaps`` on that heat.  fp32 only (other dtypes are cast, as ``condition_init``)."""
    if not act.is_cuda:
        raise TypeError(f"activation_heat_boxes: expected a tensor on a HIP device, got {act.device}")
    H, W = (int(v) for v in size)
    check_crop_args(crop_th, kernel_size, H, W)
    x = act.detach()
    if x.dtype != torch.float32:
        x = x.float()
    x, B, C, S, sb, sc, ss, grid = _layer_view(x)
    prefix = 0
    if grid is None:
        if token_grid is None:
            raise ValueError("activation_heat_boxes: token layers need token_grid")
        grid, prefix = (int(token_grid[0]), int(token_grid[1])), int(prefix_tokens or 0)
        if grid[0] < 1 or grid[1] < 1 or prefix < 0 or prefix + grid[0] * grid[1] > S:
            raise ValueError(f"activation_heat_boxes: prefix_tokens {prefix} + token_grid {grid} does not fit {S} tokens")
    r = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
    ch = torch.as_tensor(channels, dtype=torch.int64).reshape(-1)
    if r.numel() != ch.numel():
        raise ValueError(f"activation_heat_boxes: {r.numel()} rows for {ch.numel()} channels")
    if r.numel() and not r.is_cuda and (int(r.min()) < 0 or int(r.max()) >= B):
        raise ValueError(f"activation_heat_boxes: rows must lie in [0, {B})")
    if ch.numel() and not ch.is_cuda and (int(ch.min()) < 0 or int(ch.max()) >= C):
        raise ValueError(f"activation_heat_boxes: channel ids must lie in [0, {C})")
    dev = x.device
    P = r.numel()
    heat = torch.empty((P, H, W), dtype=torch.float32, device=dev) if want_heat else None
    box = torch.empty((P, 4), dtype=torch.int32, device=dev)
    if P == 0:
        return heat, box
    ws_bytes = lib().sl_render_ws_bytes(P, H, W)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=dev)
    r_d, ch_d = r.to(dev, non_blocking=True), ch.to(dev, non_blocking=True)
    with _on(dev):
        _check(lib().sl_activation_heat_boxes(_ptr(x), B, C, S, sb, sc, ss, prefix, grid[0], grid[1], _ptr(r_d), _ptr(ch_d), P, H, W,
                                              int(kernel_size), float(crop_th), _ptr(heat), _ptr(box), _ptr(ws), ws_bytes, _stream(x)),
               "sl_activation_heat_boxes")
    return heat, box


def heat_boxes(heat: torch.Tensor, kernel_size: int = 51, crop_th: float = 0.01) -> torch.Tensor:
    """K14 on full-resolution heat (P, H, W) on the device -> box (P, 4) int32 (the CROP-style box of ``render_heatmaps``)."""
    if not heat.is_cuda or heat.ndim != 3:
        raise ValueError(f"heat_boxes: expected (P, H, W) on a HIP device, got {tuple(heat.shape)} on {heat.device}")
    P, H, W = heat.shape
    check_crop_args(crop_th, kernel_size, H, W)
    h = heat.detach().to(torch.float32).contiguous()
    box = torch.empty((P, 4), dtype=torch.int32, device=h.device)
    if P == 0:
        return box
    ws_bytes = lib().sl_render_ws_bytes(P, H, W)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=h.device)
    with _on(h.device):
        _check(lib().sl_heat_boxes(_ptr(h), P, H, W, int(kernel_size), float(crop_th), _ptr(box), _ptr(ws), ws_bytes, _stream(h)),
               "sl_heat_boxes")
    return box
