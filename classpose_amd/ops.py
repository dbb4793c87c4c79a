"""Thin torch-tensor wrappers over the C ABI, one per reference call it replaces.

Names follow the reference / cellpose functions (``follow_flows``,
``get_masks``, ``remove_bad_flow_masks``, ``fill_holes_and_remove_small_masks``,
``compute_class_masks``, ``remove_border_instances``, ``normalize_img`` ...) so
the parity tests read like the reference's own tests.  All tensors live on the
GPU; every function raises if the HIP library is missing (no CPU fallback).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import CpxTiling, check, ptr
from .engine import make_tiling, percentile_params, taper_1d

_ws_cache: dict = {}


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _pp_ws(nT: int, H: int, W: int, dev) -> torch.Tensor:
    key = ("pp", nT, H, W, str(dev))
    if key not in _ws_cache:
        n = _lib.lib().cpx_postproc_workspace_bytes(nT, H, W)
        _ws_cache[key] = torch.empty(n, dtype=torch.uint8, device=dev)
    return _ws_cache[key]


def _batched(x: torch.Tensor, nd: int):
    """Accept the un-batched reference shape; return (batched view, was_batched)."""
    if x.dim() == nd:
        return x.unsqueeze(0), False
    return x, True


# ---- a6 -------------------------------------------------------------------
def normalize_stats(tiles_u8: torch.Tensor) -> torch.Tensor:
    tiles_u8, _ = _batched(tiles_u8, 3)
    nT, H, W, _c = tiles_u8.shape
    dev = tiles_u8.device
    stats = torch.empty((nT, 3, 4), dtype=torch.float32, device=dev)
    hist = torch.empty(nT * 768, dtype=torch.int32, device=dev)
    lo, hi = percentile_params(H * W, 1), percentile_params(H * W, 99)
    check(_lib.lib().cpx_normalize_stats_u8(ptr(tiles_u8), nT, H, W, lo[0], lo[1], hi[0], hi[1],
                                            ptr(stats), ptr(hist), _stream(dev)), "normalize_stats")
    return stats


def normalize_img(tiles_u8: torch.Tensor) -> torch.Tensor:
    """cellpose transforms.normalize_img on uint8 (n,H,W,3) tiles -> float32 (n,H,W,3)."""
    t, was = _batched(tiles_u8.contiguous(), 3)
    stats = normalize_stats(t)
    out = torch.empty(t.shape, dtype=torch.float32, device=t.device)
    check(_lib.lib().cpx_normalize_apply_u8(ptr(t), ptr(stats), t.shape[0], t.shape[1], t.shape[2],
                                            ptr(out), _stream(t.device)), "normalize_apply")
    return out if was else out[0]


# ---- a3 -------------------------------------------------------------------
def resized_shape(h: int, w: int, resize_factor: float) -> tuple[int, int]:
    """Output (h, w) of resize_tile_to_target_mpp (predict_wsi.py:117-118)."""
    return max(1, int(round(h * resize_factor))), max(1, int(round(w * resize_factor)))


def resize_tile_to_target_mpp(tiles_u8: torch.Tensor, resize_factor: float,
                              out: torch.Tensor | None = None) -> torch.Tensor:
    """predict_wsi.resize_tile_to_target_mpp on uint8 (n,h,w,3) / (h,w,3) device tiles:
    cv2.resize(..., INTER_LINEAR) to round(h*f) x round(w*f); factor 1.0 returns the input."""
    if resize_factor == 1.0:
        return tiles_u8
    t, was = _batched(tiles_u8.contiguous(), 3)
    dh, dw = resized_shape(t.shape[1], t.shape[2], resize_factor)
    if out is None:
        out = torch.empty((t.shape[0], dh, dw, 3), dtype=torch.uint8, device=t.device)
    check(_lib.lib().cpx_resize_linear_u8(ptr(t), t.shape[0], t.shape[1], t.shape[2], ptr(out), dh, dw,
                                          _stream(t.device)), "resize_linear_u8")
    return out if was else out[0]


def resize_u8(tiles_u8: torch.Tensor, dh: int, dw: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """cv2.resize(..., INTER_LINEAR) of uint8 (n,h,w,3) / (h,w,3) device tiles to exactly dh x dw: the image side of
    ``eval(diameter=)`` (models.py:633-639), where the sizes are ``int(h * 30 / diameter)`` and not rounded."""
    t, was = _batched(tiles_u8.contiguous(), 3)
    if out is None:
        out = torch.empty((t.shape[0], dh, dw, 3), dtype=torch.uint8, device=t.device)
    check(_lib.lib().cpx_resize_linear_u8(ptr(t), t.shape[0], t.shape[1], t.shape[2], ptr(out), dh, dw,
                                          _stream(t.device)), "resize_linear_u8")
    return out if was else out[0]


# ---- a10b -------------------------------------------------------------------
def resize_fields(t: torch.Tensor, dh: int, dw: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """transforms.resize_image on network fields (models.py:733-748, 782-792): float32 [..., h, w] device tensor ->
    [..., dh, dw], cv2.INTER_LINEAR plane by plane (``cpx_resize_linear_f32``)."""
    if t.dtype != torch.float32 or t.dim() < 2 or not t.is_cuda:
        raise ValueError("resize_fields: expected a float32 [..., h, w] device tensor")
    t = t.contiguous()
    sh, sw = t.shape[-2:]
    n = t.numel() // (sh * sw)
    if out is None:
        out = torch.empty((*t.shape[:-2], dh, dw), dtype=torch.float32, device=t.device)
    if n:
        check(_lib.lib().cpx_resize_linear_f32(ptr(t), n, sh, sw, ptr(out), dh, dw, _stream(t.device)), "resize_linear_f32")
    return out


def resize_nearest(t: torch.Tensor, dh: int, dw: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """transforms.resize_image(..., interpolation=cv2.INTER_NEAREST) on id / class maps (models.py:804-820): uint8, or the
    uint16 ids kept in an int16 tensor, [..., h, w] on the device -> [..., dh, dw] (``cpx_resize_nearest``)."""
    if t.dtype not in (torch.uint8, torch.int16) or t.dim() < 2 or not t.is_cuda:
        raise ValueError("resize_nearest: expected a uint8 or int16 [..., h, w] device tensor")
    t = t.contiguous()
    sh, sw = t.shape[-2:]
    n = t.numel() // (sh * sw)
    if out is None:
        out = torch.empty((*t.shape[:-2], dh, dw), dtype=t.dtype, device=t.device)
    if n:
        check(_lib.lib().cpx_resize_nearest(ptr(t), t.element_size(), n, sh, sw, ptr(out), dh, dw, _stream(t.device)),
              "resize_nearest")
    return out


# ---- a7 -------------------------------------------------------------------
def make_subtiles(tiles_u8: torch.Tensor, bsize: int = 256, augment: bool = False,
                  tile_overlap: float = 0.1):
    """pad + make_tiles of core.run_net on normalised pixels -> float32 (n*ny*nx, 3, b, b)."""
    t, _ = _batched(tiles_u8.contiguous(), 3)
    nT, H, W, _c = t.shape
    til = make_tiling(H, W, bsize, augment, tile_overlap)
    stats = normalize_stats(t)
    out = torch.empty((nT * til.ny * til.nx, 3, bsize, bsize), dtype=torch.float32, device=t.device)
    check(_lib.lib().cpx_make_subtiles_f32(ptr(t), ptr(stats), nT, C.byref(til), ptr(out),
                                           _stream(t.device)), "make_subtiles_f32")
    return out, til


def make_patches(tiles_u8: torch.Tensor, bsize: int = 256, augment: bool = False,
                 tile_overlap: float = 0.1, dtype: torch.dtype = torch.bfloat16):
    t, _ = _batched(tiles_u8.contiguous(), 3)
    nT, H, W, _c = t.shape
    til = make_tiling(H, W, bsize, augment, tile_overlap)
    stats = normalize_stats(t)
    nS = nT * til.ny * til.nx
    out = torch.empty((nS * (bsize // 8) ** 2, 192), dtype=dtype, device=t.device)
    check(_lib.lib().cpx_make_patches(ptr(t), ptr(stats), nT, C.byref(til), _DT[dtype], ptr(out),
                                      _stream(t.device)), "make_patches")
    return out, til


def blend_subtiles(y: torch.Tensor, y_class: torch.Tensor, til: CpxTiling, nT: int):
    """unaugment + average_tiles + crop of core.run_net: y (nS,3,b,b), y_class (nS,ncls,b,b)."""
    dev = y.device
    ncls = y_class.shape[1]
    H, W = til.H, til.W
    dP = torch.empty((nT, 2, H, W), dtype=torch.float32, device=dev)
    cp = torch.empty((nT, H, W), dtype=torch.float32, device=dev)
    lg = torch.empty((nT, ncls, H, W), dtype=torch.float32, device=dev)
    taper = torch.from_numpy(taper_1d(til.bsize)).to(dev)
    check(_lib.lib().cpx_blend_subtiles_nchw(ptr(y.contiguous()), ptr(y_class.contiguous()), ncls, nT,
                                             C.byref(til), ptr(taper), ptr(dP), ptr(cp), ptr(lg),
                                             _stream(dev)), "blend_nchw")
    return dP, cp, lg


def blend_head(head: torch.Tensor, ld_head: int, ncls: int, til: CpxTiling, nT: int):
    dev = head.device
    H, W = til.H, til.W
    dP = torch.empty((nT, 2, H, W), dtype=torch.float32, device=dev)
    cp = torch.empty((nT, H, W), dtype=torch.float32, device=dev)
    lg = torch.empty((nT, max(ncls, 1), H, W), dtype=torch.float32, device=dev)
    taper = torch.from_numpy(taper_1d(til.bsize)).to(dev)
    check(_lib.lib().cpx_blend_subtiles(ptr(head), ld_head, ncls, nT, C.byref(til), ptr(taper),
                                        ptr(dP), ptr(cp), ptr(lg), _stream(dev)), "blend")
    return dP, cp, lg


# ---- a11-a16 ----------------------------------------------------------------
def follow_flows(dP: torch.Tensor, cellprob: torch.Tensor, niter: int = 200,
                 cellprob_threshold: float = 0.0, return_float: bool = False):
    """dP (n,2,H,W) RAW network flows, cellprob (n,H,W).  Returns packed int32 end
    points (n,H*W) [(y<<16)|x, -1 = inactive] and optionally float (n,2,H*W)."""
    dP, _ = _batched(dP.contiguous(), 3)
    cellprob, _ = _batched(cellprob.contiguous(), 2)
    nT, _two, H, W = dP.shape
    dev = dP.device
    pf = torch.empty((nT, H * W), dtype=torch.int32, device=dev)
    fl = torch.empty((nT, 2, H * W), dtype=torch.float32, device=dev) if return_float else None
    check(_lib.lib().cpx_follow_flows(ptr(dP), ptr(cellprob), nT, H, W, cellprob_threshold, niter,
                                      ptr(pf), ptr(fl), ptr(_pp_ws(nT, H, W, dev)), _stream(dev)),
          "follow_flows")
    return (pf, fl) if return_float else pf


def get_masks(p_final: torch.Tensor, H: int, W: int, max_size_fraction: float = 0.4):
    nT = p_final.shape[0]
    dev = p_final.device
    masks = torch.empty((nT, H, W), dtype=torch.int32, device=dev)
    nlab = torch.empty(nT, dtype=torch.int32, device=dev)
    check(_lib.lib().cpx_get_masks(ptr(p_final.contiguous()), nT, H, W, max_size_fraction, ptr(masks),
                                   ptr(nlab), ptr(_pp_ws(nT, H, W, dev)), _stream(dev)), "get_masks")
    return masks, nlab


def remove_bad_flow_masks(masks: torch.Tensor, dP: torch.Tensor, threshold: float = 0.4,
                          return_errors: bool = False):
    """In place on int32 masks (n,H,W); dP (n,2,H,W) raw network flows."""
    nT, H, W = masks.shape
    dev = masks.device
    L = _lib.lib().cpx_postproc_max_labels(H, W)
    errs = torch.zeros((nT, L), dtype=torch.float64, device=dev) if return_errors else None
    check(_lib.lib().cpx_remove_bad_flow_masks(ptr(masks), ptr(dP.contiguous()), nT, H, W, threshold,
                                               ptr(errs), ptr(_pp_ws(nT, H, W, dev)), _stream(dev)),
          "remove_bad_flow_masks")
    return (masks, errs) if return_errors else masks


def fill_holes_and_remove_small_masks(masks: torch.Tensor, min_size: int = 15):
    nT, H, W = masks.shape
    dev = masks.device
    nlab = torch.empty(nT, dtype=torch.int32, device=dev)
    check(_lib.lib().cpx_fill_holes_and_remove_small_masks(ptr(masks), nT, H, W, min_size, ptr(nlab),
                                                           ptr(_pp_ws(nT, H, W, dev)), _stream(dev)),
          "fill_holes_and_remove_small_masks")
    return masks, nlab


def compute_class_masks(masks: torch.Tensor, y_class: torch.Tensor) -> torch.Tensor:
    """masks int32 (n,H,W), y_class float32 (n,ncls,H,W) -> uint8 (n,H,W)."""
    nT, H, W = masks.shape
    dev = masks.device
    cm = torch.empty((nT, H, W), dtype=torch.uint8, device=dev)
    check(_lib.lib().cpx_compute_class_masks(ptr(masks), ptr(y_class.contiguous()), nT, y_class.shape[1],
                                             H, W, ptr(cm), ptr(_pp_ws(nT, H, W, dev)), _stream(dev)),
          "compute_class_masks")
    return cm


def remove_border_instances(masks: torch.Tensor, class_masks: torch.Tensor | None = None):
    nT, H, W = masks.shape
    dev = masks.device
    check(_lib.lib().cpx_remove_border_instances(ptr(masks), ptr(class_masks), nT, H, W,
                                                 ptr(_pp_ws(nT, H, W, dev)), _stream(dev)),
          "remove_border_instances")
    return masks if class_masks is None else (masks, class_masks)


def compute_masks(dP: torch.Tensor, cellprob: torch.Tensor, logits: torch.Tensor | None = None,
                  niter: int = 200, cellprob_threshold: float = 0.0, flow_threshold: float = 0.4,
                  min_size: int = 15, max_size_fraction: float = 0.4):
    """dynamics.resize_and_compute_masks (+ compute_class_masks) on a batch of tiles."""
    nT, _two, H, W = dP.shape
    dev = dP.device
    ncls = 0 if logits is None else logits.shape[1]
    masks = torch.empty((nT, H, W), dtype=torch.int16, device=dev)
    cm = torch.empty((nT, H, W), dtype=torch.uint8, device=dev)
    nlab = torch.empty(nT, dtype=torch.int32, device=dev)
    check(_lib.lib().cpx_compute_masks(ptr(dP.contiguous()), ptr(cellprob.contiguous()),
                                       ptr(logits.contiguous()) if logits is not None else None, nT,
                                       ncls, H, W, cellprob_threshold, flow_threshold, niter, min_size,
                                       max_size_fraction, ptr(masks), ptr(cm), ptr(nlab),
                                       ptr(_pp_ws(nT, H, W, dev)), _stream(dev)), "compute_masks")
    return masks, cm, nlab


def instance_confidence(masks_u16: torch.Tensor, logits: torch.Tensor | None, cellprob: torch.Tensor | None,
                        rec_counts: torch.Tensor, max_rec: int, out=None):
    """Per-cell class confidence of a batch (``cpx_instance_confidence``; include/classpose_hip.h has the definitions):
    masks_u16 (n,H,W) uint16 ids in an int16 tensor, logits (n,ncls,H,W) float32 or None, cellprob (n,H,W) float32 or None,
    rec_counts (n,) int32 on the device -> (votes int32 (n,max_rec,ncls), prob_q (n,max_rec,ncls), cellprob_q (n,max_rec)),
    the two sums as uint64 bits in int64 tensors.  Rows below min(rec_counts, max_rec) are defined, the others are whatever
    the buffers held (``out`` = the three tensors to write into; fresh ones are uninitialised).  Without a class part
    (logits None or ncls <= 1) votes and prob_q come back as None, without cellprob cellprob_q does."""
    nT, H, W = masks_u16.shape
    dev = masks_u16.device
    ncls = 0 if logits is None else int(logits.shape[1])
    cls_part = logits is not None and ncls > 1
    if masks_u16.dtype not in (torch.int16, torch.uint16) or not masks_u16.is_contiguous():
        raise ValueError("instance_confidence: masks_u16 must be a contiguous 16-bit (n, H, W) tensor")
    if rec_counts.dtype != torch.int32 or rec_counts.numel() < nT or rec_counts.device != dev:
        raise ValueError("instance_confidence: rec_counts must be int32 [n] on the masks' device")
    for name, t, shape in (("logits", logits, (nT, ncls, H, W)), ("cellprob", cellprob, (nT, H, W))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
            raise ValueError(f"instance_confidence: {name} must be a contiguous float32 {shape} tensor on {dev}")
    max_rec = int(max_rec)
    if out is None:
        votes = torch.empty((nT, max_rec, ncls), dtype=torch.int32, device=dev) if cls_part else None
        prob_q = torch.empty((nT, max_rec, ncls), dtype=torch.int64, device=dev) if cls_part else None
        cellprob_q = torch.empty((nT, max_rec), dtype=torch.int64, device=dev) if cellprob is not None else None
    else:
        votes, prob_q, cellprob_q = out
    L = _lib.lib()
    need = L.cpx_instance_confidence_workspace_bytes(nT, ncls, H, W, max_rec)
    ws = torch.empty(need, dtype=torch.uint8, device=dev) if need else None
    check(L.cpx_instance_confidence(ptr(masks_u16), ptr(logits), ptr(cellprob), ptr(rec_counts), nT, ncls, H, W, max_rec,
                                    ptr(votes), ptr(prob_q), ptr(cellprob_q), ptr(ws), need, _stream(dev)), "instance_confidence")
    return votes, prob_q, cellprob_q


def masks_to_numpy(masks_i16: torch.Tensor) -> np.ndarray:
    """uint16 instance ids (stored in an int16 tensor) -> numpy uint16."""
    return masks_i16.cpu().numpy().view(np.uint16)


# ---- network building blocks --------------------------------------------------
EPI = dict(bf16=0, gelu=1, resid=2, f32=3, pos=4, relu=5, qkv=6)


def gemm(A: torch.Tensor, Wt: torch.Tensor, epilogue: str = "bf16", bias=None, aux=None):
    M, K = A.shape
    N = Wt.shape[0]
    dev = A.device
    out = torch.empty((M, N), dtype=torch.float32 if epilogue == "f32" else A.dtype, device=dev)
    check(_lib.lib().cpx_gemm(_DT[A.dtype], ptr(A), ptr(Wt), M, N, K, EPI[epilogue], ptr(bias), ptr(aux),
                              ptr(out), N, _stream(dev)), "gemm")
    return out


_DT = {torch.bfloat16: _lib.DT_BF16, torch.float16: _lib.DT_F16, torch.float32: _lib.DT_F32}


def conv3x3(x: torch.Tensor, Wt: torch.Tensor, epilogue: str = "bf16", bias=None):
    """3x3 / padding-1 convolution over 32 x 32-token images as an implicit GEMM: x (S*1024, C) token-major,
    Wt (N, 9*C) with k = (3 ky + kx) * C + c (``weight.permute(0, 2, 3, 1).reshape(N, 9 * C)`` of a Conv2d)."""
    M, Cc = x.shape
    N = Wt.shape[0]
    out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    check(_lib.lib().cpx_conv3x3(_DT[x.dtype], ptr(x), ptr(Wt), M, N, Cc, EPI[epilogue], ptr(bias), ptr(out), N,
                                 _stream(x.device)), "conv3x3")
    return out


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-6):
    out = torch.empty_like(x)
    check(_lib.lib().cpx_layernorm(_DT[x.dtype], ptr(x), ptr(w), ptr(b), x.shape[0], x.shape[1], eps, ptr(out),
                                   _stream(x.device)), "layernorm")
    return out


def attention(qkv: torch.Tensor, rel_h: torch.Tensor, rel_w: torch.Tensor):
    """qkv (nS*1024, 3072) bf16 / fp16 / fp32; rel_* (64,64) tables of the same type (x8, zero last row)."""
    M = qkv.shape[0]
    nS = M // 1024
    vt = torch.empty((M, 1024), dtype=qkv.dtype, device=qkv.device)
    out = torch.empty((M, 1024), dtype=qkv.dtype, device=qkv.device)
    check(_lib.lib().cpx_attention(_DT[qkv.dtype], ptr(qkv), ptr(rel_h), ptr(rel_w), nS, ptr(vt), ptr(out),
                                   _stream(qkv.device)), "attention")
    return out


def row_stats(x: torch.Tensor) -> torch.Tensor:
    """(sum, sum of squares) of each 1024-wide row into slot 0 of [rows][4][2].  bf16 through the product library; fp16 under
    ``_lib.use_debug_library()`` (cpx_row_stats_dt)."""
    if x.dim() != 2 or x.shape[1] != 1024 or not x.is_contiguous():
        raise ValueError(f"row_stats takes contiguous [rows][1024] rows, not {tuple(x.shape)}")
    st = torch.empty((x.shape[0], 4, 2), dtype=torch.float32, device=x.device)
    L = _lib.lib()
    if x.dtype != torch.bfloat16:             # debug library only: the product has no such symbol (AttributeError)
        check(L.cpx_row_stats_dt(_DT[x.dtype], ptr(x), x.shape[0], ptr(st), _stream(x.device)), "row_stats")
    else:
        check(L.cpx_row_stats(ptr(x), x.shape[0], ptr(st), _stream(x.device)), "row_stats")
    return st


def gemm_ln(A, Wt, epilogue="bf16", bias=None, aux=None, ln_stats=None, ln_colsum=None, want_stats=False):
    """GEMM with a LayerNorm over the input row folded in / output row statistics emitted.  bf16 through the product
    library; under ``_lib.use_debug_library()`` the half type follows ``A.dtype`` (bf16 or fp16, cpx_gemm_ln_dt)."""
    M, K = A.shape
    N = Wt.shape[0]
    dev = A.device
    out = torch.empty((M, N), dtype=torch.float32 if epilogue == "f32" else A.dtype, device=dev)
    st = torch.zeros((M, 4, 2), dtype=torch.float32, device=dev) if want_stats else None
    L = _lib.lib()
    args = (ptr(A), ptr(Wt), M, N, K, EPI[epilogue], ptr(bias), ptr(aux), ptr(out), N, ptr(ln_stats), ptr(ln_colsum), ptr(st), _stream(dev))
    if A.dtype != torch.bfloat16:             # debug library only: the product has no such symbol (AttributeError)
        check(L.cpx_gemm_ln_dt(_DT[A.dtype], *args), "gemm_ln")
    else:
        check(L.cpx_gemm_ln(*args), "gemm_ln")
    return (out, st) if want_stats else out


# ---- f2 ---------------------------------------------------------------------
def dedup_grid(centers: np.ndarray, max_dist: float) -> tuple[float, float, float, int, int]:
    """(x0, y0, cell, grid_w, grid_h) of the bucket grid ``cpx_dedup_pairs`` wants for these centres.  The cell edge is a
    power of two (8 up to max_dist 7.99999, then 16, 32, ...) with cell * (1 - 2^-20) >= max_dist: the kernel's
    ``(x - x0) * (1 / cell)`` is then exact but for the rounding of the difference, and that margin absorbs it, so two
    points within max_dist of each other are never more than one cell apart (a cell edge of max_dist itself, with an
    inexact reciprocal, put some two cells apart and the 3 x 3 scan lost the pair)."""
    if not (np.isfinite(max_dist) and max_dist > 0):
        raise ValueError(f"max_dist must be positive and finite, got {max_dist}")
    cell = 8.0
    while cell * (1.0 - 2.0 ** -20) < max_dist:
        cell *= 2.0
    lo, hi = centers.min(0), centers.max(0)
    x0, y0 = float(np.floor(lo[0])) - cell, float(np.floor(lo[1])) - cell
    gw, gh = int((hi[0] - x0) // cell) + 2, int((hi[1] - y0) // cell) + 2
    return x0, y0, cell, gw, gh


def dedup_pairs(centers: np.ndarray, max_dist: float = 15 / 2, device=None) -> np.ndarray:
    """``KDTree(centers).query_pairs(max_dist)`` (predict_wsi.py:923-927) as an int32 (P, 2) array of (i, j),
    i < j, sorted by i: the uniform-grid radius search of ``cpx_dedup_pairs`` on the device.
    centers: (n, 2) float64 host array (the rounded centroids)."""
    centers = np.ascontiguousarray(centers, dtype=np.float64).reshape(-1, 2)
    n = len(centers)
    if n < 2:
        return np.zeros((0, 2), np.int32)
    dev = torch.device(device if device is not None else "cuda")
    x0, y0, cell, gw, gh = dedup_grid(centers, max_dist)
    L = _lib.lib()
    c = torch.from_numpy(centers).to(dev)
    nbytes = L.cpx_dedup_pairs_workspace_bytes(n, gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    st = _stream(dev)
    check(L.cpx_dedup_pairs(ptr(c), n, x0, y0, cell, gw, gh, float(max_dist), None, 0, ptr(tot), ptr(ws), nbytes, st),
          "dedup_pairs(count)")
    P = int(tot.item())
    if P == 0:
        return np.zeros((0, 2), np.int32)
    pairs = torch.empty((P, 2), dtype=torch.int32, device=dev)
    check(L.cpx_dedup_pairs(ptr(c), n, x0, y0, cell, gw, gh, float(max_dist), ptr(pairs), P, ptr(tot), ptr(ws), nbytes, st),
          "dedup_pairs(write)")
    return pairs.cpu().numpy()


# ---- a16b -------------------------------------------------------------------
PQ_WS_LIMIT = 1 << 30          # bytes of table workspace per call: larger batches run in chunks of images


def _pq_ids(x: torch.Tensor):
    """(contiguous tensor, bytes per id): int32, or the uint16 ids ``compute_masks`` / ``Engine`` keep in an int16 tensor."""
    if x.dtype == torch.int32:
        return x.contiguous(), 4
    if x.dtype == torch.int16 or x.dtype == getattr(torch, "uint16", None):
        return x.contiguous(), 2
    raise ValueError(f"instance ids must be int32 or uint16-in-int16, not {x.dtype}")


def pq_full_table_cap(H: int, W: int) -> int:
    """Slots per table with which ``cpx_pq_stats`` cannot overflow: a power of two >= 2 * H * W."""
    return max(16, 1 << (2 * H * W - 1).bit_length())


def pq_stats(true_ids: torch.Tensor, pred_ids: torch.Tensor, true_cls: torch.Tensor | None = None,
             pred_cls: torch.Tensor | None = None, nr_classes: int = 1, match_iou: float = 0.5,
             filter_unlabelled: bool | None = None, no_border_instances: bool = False, return_lists: bool = False,
             table_cap: int | None = None) -> dict:
    """Per-(image, class) panoptic-quality statistics of device-resident maps (``cpx_pq_stats``): what
    ``get_multi_pq_info`` (stats_utils.py:8-61) returns per image after ``filter_out_unlabelled_cells`` and
    ``remove_border_instances``, or ``get_pq``'s counts per image in binary mode (``true_cls is None``).

    true_ids / pred_ids (n, H, W) int32 or the engine's uint16-in-int16 ids; true_cls / pred_cls (n, H, W) uint8.  The inputs are
    not modified.  Returns host arrays ``tp, fp, fn`` int32 (n, nr_classes) and ``iou_sum`` float64; with ``return_lists`` also
    ``pairs`` / ``insts`` (structured, see cpx_pq_pair / cpx_pq_inst) and ``nobg`` (n, 2).  Tables start at H * W / 16 slots per
    image; an image that fills them is repeated with tables that cannot fill (2 * H * W slots)."""
    binary = true_cls is None
    if (pred_cls is None) != binary:
        raise ValueError("give both class maps or neither")
    if filter_unlabelled is None:
        filter_unlabelled = not binary
    if binary and (nr_classes != 1 or filter_unlabelled):
        raise ValueError("binary mode has one pseudo-class and no unlabelled-cell filter")
    if not 1 <= nr_classes <= 255:
        raise ValueError(f"nr_classes must be in 1..255, not {nr_classes}")
    true_ids, _ = _batched(true_ids, 2)
    pred_ids, _ = _batched(pred_ids, 2)
    t_ids, idb = _pq_ids(true_ids)
    p_ids, idb2 = _pq_ids(pred_ids)
    if idb != idb2 or t_ids.shape != p_ids.shape:
        raise ValueError("true and predicted ids differ in type or shape")
    nI, H, W = t_ids.shape
    dev = t_ids.device
    if not binary:
        true_cls, _ = _batched(true_cls, 2)
        pred_cls, _ = _batched(pred_cls, 2)
        if true_cls.dtype != torch.uint8 or pred_cls.dtype != torch.uint8 or true_cls.shape != t_ids.shape or pred_cls.shape != t_ids.shape:
            raise ValueError("class maps must be uint8 of the ids' shape")
        true_cls, pred_cls = true_cls.contiguous(), pred_cls.contiguous()
    L = _lib.lib()
    full_cap = pq_full_table_cap(H, W)
    cap0 = min(full_cap, max(1024, 1 << max(H * W // 16 - 1, 1).bit_length())) if table_cap is None else int(table_cap)
    out = dict(tp=np.zeros((nI, nr_classes), np.int32), fp=np.zeros((nI, nr_classes), np.int32),
               fn=np.zeros((nI, nr_classes), np.int32), iou_sum=np.zeros((nI, nr_classes), np.float64))
    pairs_all, insts_all, nobg_all = [], [], np.zeros((nI, 2), np.int32)

    def run(idx: torch.Tensor | None, lo: int, hi: int, cap: int):
        """images lo:hi (idx None) or the listed ones, with tables of `cap` slots -> (status, stats, lists)"""
        sel = (lambda x: x[lo:hi]) if idx is None else (lambda x: x.index_select(0, idx))
        ti, pi = sel(t_ids), sel(p_ids)
        tc, pc = (None, None) if binary else (sel(true_cls), sel(pred_cls))
        n = ti.shape[0]
        nbytes = L.cpx_pq_workspace_bytes(n, H, W, nr_classes, cap)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        cnt = torch.empty((3, n, nr_classes), dtype=torch.int32, device=dev)
        ious = torch.empty((n, nr_classes), dtype=torch.float64, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        nobg = torch.empty((n, 2), dtype=torch.int32, device=dev)
        pairs = insts = lc = None
        mx = 0
        if return_lists:
            mx = min(n * cap, 1 << 26)
            pairs = torch.empty((mx, 8), dtype=torch.int32, device=dev)
            insts = torch.empty((mx, 6), dtype=torch.int32, device=dev)
            lc = torch.empty(2, dtype=torch.int32, device=dev)
        check(L.cpx_pq_stats(ptr(ti), ptr(pi), idb, ptr(tc), ptr(pc), n, H, W, nr_classes, float(match_iou),
                             int(bool(filter_unlabelled)), int(bool(no_border_instances)), cap, ptr(cnt[0]), ptr(cnt[1]),
                             ptr(cnt[2]), ptr(ious), ptr(status), ptr(nobg), ptr(pairs), mx, ptr(insts), mx, ptr(lc),
                             ptr(ws), nbytes, _stream(dev)), "pq_stats")
        lists = None
        if return_lists:
            npair, ninst = (int(v) for v in lc.cpu())
            if npair > mx or ninst > mx:
                raise _lib.CpxError(f"pq_stats: {npair} pairs / {ninst} instances exceed the list limit of {mx} entries per call")
            lists = (pairs[:npair].cpu().numpy(), insts[:ninst].cpu().numpy(), nobg.cpu().numpy())
        return status.cpu().numpy(), cnt.cpu().numpy(), ious.cpu().numpy(), lists

    def store(where, res, which=None):
        _st, cnt, ious, lists = res
        rows = slice(None) if which is None else which
        out["tp"][where], out["fp"][where], out["fn"][where] = cnt[0][rows], cnt[1][rows], cnt[2][rows]
        out["iou_sum"][where] = ious[rows]
        if lists is not None:
            pr, ins, nb = lists
            local = np.arange(len(nb)) if which is None else which
            glob = np.arange(where.start, where.stop) if isinstance(where, slice) else np.asarray(where)
            lut = np.full(len(nb), -1, np.int64)
            lut[local] = glob
            pr, ins = pr[lut[pr[:, 0]] >= 0].copy(), ins[lut[ins[:, 0]] >= 0].copy()
            pr[:, 0], ins[:, 0] = lut[pr[:, 0]], lut[ins[:, 0]]
            pairs_all.append(pr); insts_all.append(ins)
            nobg_all[glob] = nb[local]

    def chunk_of(cap: int) -> int:
        per = L.cpx_pq_workspace_bytes(1, H, W, nr_classes, cap)
        return max(1, min(65535, PQ_WS_LIMIT // per))

    step = chunk_of(cap0)
    redo: list[int] = []
    for lo in range(0, nI, step):
        hi = min(nI, lo + step)
        res = run(None, lo, hi, cap0)
        ok = np.flatnonzero(res[0] == 0)
        store(lo + ok, res, ok)
        redo += [lo + int(i) for i in np.flatnonzero(res[0] != 0)]
    if redo:
        if cap0 >= full_cap and table_cap is None:
            raise _lib.CpxError(f"pq_stats: tables of {cap0} slots (2 * H * W) filled up")
        if table_cap is not None:
            raise _lib.CpxError(f"pq_stats: table_cap = {cap0} slots is too small for image(s) {redo[:8]} (limit without overflow: {full_cap})")
        step = chunk_of(full_cap)
        for k in range(0, len(redo), step):
            part = redo[k:k + step]
            res = run(torch.tensor(part, dtype=torch.long, device=dev), 0, 0, full_cap)
            if res[0].any():
                raise _lib.CpxError(f"pq_stats: tables of {full_cap} slots (2 * H * W) filled up")
            store(np.asarray(part), res, None)
    if return_lists:
        out["pairs"] = np.concatenate(pairs_all) if pairs_all else np.zeros((0, 8), np.int32)
        out["insts"] = np.concatenate(insts_all) if insts_all else np.zeros((0, 6), np.int32)
        out["nobg"] = nobg_all
    return out


# ---- t1: training the 1x1 class head (csrc/cpx_train.hip) -------------------------------------------------------
def neck_features(net_ws: torch.Tensor, n_subtiles: int, dtype: torch.dtype) -> torch.Tensor:
    """View of the neck output [n_subtiles * 1024, 256] that ``cpx_net_forward`` left in its workspace ``net_ws`` (uint8):
    valid until the next forward on that workspace -- clone it to keep it."""
    off = _lib.lib().cpx_net_neck_offset(n_subtiles, _DT[dtype])
    if off == 0:
        raise ValueError("neck_features: invalid n_subtiles / dtype")
    n = n_subtiles * 1024 * 256 * torch.empty(0, dtype=dtype).element_size()
    return net_ws[off:off + n].view(dtype).view(n_subtiles * 1024, 256)


def patchify_f32(x: torch.Tensor, dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """float32 NCHW crops (n, 3, H, W), already normalised -> patch rows (n * H/8 * W/8, 192) rounded as ``x.to(dtype)``."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or x.shape[2] % 8 or x.shape[3] % 8:
        raise ValueError("patchify_f32: expected float32 (n, 3, H, W) with H, W multiples of 8")
    x = x.contiguous()
    n, _c, H, W = x.shape
    out = torch.empty((n * (H // 8) * (W // 8), 192), dtype=dtype, device=x.device)
    check(_lib.lib().cpx_patchify_f32(ptr(x), n, H, W, _DT[dtype], ptr(out), _stream(x.device)), "patchify_f32")
    return out


class ClassLossOut:
    """Device results of ``class_loss`` (nothing is copied to the host until ``check_status`` / ``.item()``)."""
    __slots__ = ("ce", "tversky", "tp", "fp", "fn", "n_annot", "dlogits", "status")

    def check_status(self):
        flags, first = (int(v) for v in self.status.tolist())
        if flags & 2:
            raise ValueError(f"class_loss: image {first} has a label outside [0, nclasses) other than -100")
        if flags & 1:
            raise ValueError(f"class_loss: image {first} has no annotated pixel (every label is -100); the reference's "
                             "Tversky loss is NaN for such a batch -- drop the image")


def class_loss(head: torch.Tensor, labels: torch.Tensor, ncls: int, col0: int = 192, class_weights: torch.Tensor | None = None,
               alpha: float = 0.3, gamma: float = 1.33, eps: float = 1e-6, w_ce: float = 1.0, w_tv: float = 1.0,
               dlogits: torch.Tensor | None = None, check_status: bool = True) -> ClassLossOut:
    """Cross-entropy (ignore_index = -100) + focal Tversky loss of the reference's head training and their gradient.
    head (n * H/8 * W/8, ld_head) float32 token-major (class columns from ``col0``), labels (n, H, W) int16."""
    if head.dtype != torch.float32 or head.dim() != 2 or not head.is_contiguous():
        raise ValueError("class_loss: head must be a contiguous float32 (rows, ld_head) tensor")
    if labels.dtype != torch.int16 or labels.dim() != 3:
        raise ValueError("class_loss: labels must be int16 (n, H, W)")
    labels = labels.contiguous()
    nI, H, W = labels.shape
    rows, ld = head.shape
    if H % 8 or W % 8 or rows != nI * (H // 8) * (W // 8) or not 2 <= ncls <= 64 or ld < col0 + ncls * 64:
        raise ValueError(f"class_loss: head {tuple(head.shape)} does not fit labels {tuple(labels.shape)} with {ncls} classes")
    dev = head.device
    L = _lib.lib()
    o = ClassLossOut()
    o.ce = torch.empty(1, dtype=torch.float32, device=dev)
    o.tversky = torch.empty(1, dtype=torch.float32, device=dev)
    o.tp, o.fp, o.fn = (torch.empty((nI, ncls), dtype=torch.float32, device=dev) for _ in range(3))
    o.n_annot = torch.empty(nI, dtype=torch.int32, device=dev)
    o.status = torch.empty(2, dtype=torch.int32, device=dev)
    o.dlogits = dlogits if dlogits is not None else torch.empty((rows, ncls * 64), dtype=torch.float32, device=dev)
    if o.dlogits.shape != (rows, ncls * 64) or o.dlogits.dtype != torch.float32 or not o.dlogits.is_contiguous():
        raise ValueError("class_loss: dlogits must be contiguous float32 (rows, ncls * 64)")
    if class_weights is not None:
        class_weights = class_weights.to(device=dev, dtype=torch.float32).contiguous()
        if class_weights.numel() != ncls:
            raise ValueError("class_loss: one class weight per class")
    key = ("closs", nI, H, W, ncls, str(dev))
    if key not in _ws_cache:
        _ws_cache[key] = torch.empty(L.cpx_class_loss_workspace_bytes(nI, H, W, ncls), dtype=torch.uint8, device=dev)
    ws = _ws_cache[key]
    check(L.cpx_class_loss(ptr(head), ld, col0, ptr(labels), nI, H, W, ncls, ptr(class_weights), alpha, gamma, eps, w_ce, w_tv,
                           ptr(o.ce), ptr(o.tversky), ptr(o.tp), ptr(o.fp), ptr(o.fn), ptr(o.n_annot), ptr(o.dlogits),
                           ptr(o.status), ptr(ws), ws.numel(), _stream(dev)), "class_loss")
    if check_status:
        o.check_status()
    return o


class SegLossOut:
    """Device results of ``seg_loss``: ``flow`` and ``cp`` (1,) float32 (the loss is their sum), ``dlogits`` (rows, 192)."""
    __slots__ = ("flow", "cp", "dlogits")


def seg_loss(head: torch.Tensor, targets: torch.Tensor, w_seg: float = 1.0, dlogits: torch.Tensor | None = None) -> SegLossOut:
    """cellpose ``train._loss_fn_seg`` (restated from cellpose 4.0.x) on the flow columns 0..191 of the token-major ``head``
    (n * H/8 * W/8, ld_head) float32 and its gradient: ``targets`` (n, 3, H, W) float32 = (mask, flow Y, flow X);
    flow = mean((z - 5 t)^2) / 2 over both flow channels, cp = BCE-with-logits of the cellprob channel against mask > 0.5."""
    if head.dtype != torch.float32 or head.dim() != 2 or not head.is_contiguous() or head.shape[1] < 192:
        raise ValueError("seg_loss: head must be a contiguous float32 (rows, ld_head >= 192) tensor")
    if targets.dtype != torch.float32 or targets.dim() != 4 or targets.shape[1] != 3 or targets.device != head.device:
        raise ValueError("seg_loss: targets must be float32 (n, 3, H, W) on the head's device")
    targets = targets.contiguous()
    nI, _c, H, W = targets.shape
    rows, ld = head.shape
    if H % 8 or W % 8 or nI == 0 or rows != nI * (H // 8) * (W // 8):
        raise ValueError(f"seg_loss: head {tuple(head.shape)} does not fit targets {tuple(targets.shape)}")
    dev = head.device
    L = _lib.lib()
    o = SegLossOut()
    o.flow = torch.empty(1, dtype=torch.float32, device=dev)
    o.cp = torch.empty(1, dtype=torch.float32, device=dev)
    o.dlogits = dlogits if dlogits is not None else torch.empty((rows, 192), dtype=torch.float32, device=dev)
    if o.dlogits.shape != (rows, 192) or o.dlogits.dtype != torch.float32 or not o.dlogits.is_contiguous() or o.dlogits.device != dev:
        raise ValueError("seg_loss: dlogits must be contiguous float32 (rows, 192)")
    key = ("sloss", nI, H, W, str(dev))
    if key not in _ws_cache:
        _ws_cache[key] = torch.empty(L.cpx_seg_loss_workspace_bytes(nI, H, W), dtype=torch.uint8, device=dev)
    ws = _ws_cache[key]
    check(L.cpx_seg_loss(ptr(head), ld, ptr(targets), nI, H, W, float(w_seg), ptr(o.flow), ptr(o.cp), ptr(o.dlogits), ptr(ws),
                         ws.numel(), _stream(dev)), "seg_loss")
    return o


def masks_to_flows(masks: torch.Tensor, check_status: bool = True):
    """cellpose ``dynamics.masks_to_flows_gpu`` per image (restated; checked against ``oracle.dynamics.masks_to_flows``): int32
    device ``masks`` (n, H, W) or (H, W), ids compact in 1..n and 0 = background -> float32 (n, 2, H, W) or (2, H, W) unit flows
    (dY, dX), 0 on the background.  Raises ``ValueError`` on a negative id or on more labels than ``cpx_postproc_max_labels``
    (with ``check_status=False`` returns ``(flows, status)`` instead)."""
    if masks.dtype != torch.int32 or masks.dim() not in (2, 3) or not masks.is_cuda:
        raise ValueError("masks_to_flows: expected int32 device masks (n, H, W) or (H, W)")
    m, was = _batched(masks.contiguous(), 2)
    nT, H, W = m.shape
    dev = m.device
    flows = torch.empty((nT, 2, H, W), dtype=torch.float32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    check(_lib.lib().cpx_masks_to_flows(ptr(m), nT, H, W, ptr(flows), ptr(status), ptr(_pp_ws(nT, H, W, dev)), _stream(dev)),
          "masks_to_flows")
    flows = flows if was else flows[0]
    if not check_status:
        return flows, status
    bits = int(status.item())
    if bits & 2:
        raise ValueError("masks_to_flows: an instance id is negative")
    if bits & 1:
        raise ValueError(f"masks_to_flows: an instance id is above the {_lib.lib().cpx_postproc_max_labels(H, W) - 1} labels a "
                         f"{H} x {W} map may hold (ids must be compact in 1..n: renumber them)")
    return flows


def warp_flow_targets(pool_tgt: torch.Tensor, px_off: torch.Tensor, hw: torch.Tensor, image_of, inv, vec, out_hw,
                      check_status: bool = True):
    """``cpx_warp_affine_pool_flow_f32``: ``pool_tgt`` float32 (3 * pool_px,), per image of the table (px_off, hw) the planes
    (mask, flow Y, flow X) as [3][h][w] from float 3 * px_off[i]; crop t samples image ``image_of[t]`` by ``inv[t]`` like
    ``warp_affine`` and maps the flow pair through ``vec[t]`` (``augment.flow_vec``).  Returns (float32 (n, 3, dh, dw), status)."""
    dev, nI, pool_px = _pool_table(pool_tgt, px_off, hw, "warp_flow_targets", torch.float32)
    image_of, inv, vec, n = _crop_maps(image_of, inv, dev, "warp_flow_targets", vec)
    dh, dw, out, _lab_out, status = _pool_outputs(None, pool_px, n, out_hw, dev, "warp_flow_targets")
    check(_lib.lib().cpx_warp_affine_pool_flow_f32(ptr(pool_tgt), ptr(px_off), ptr(hw), nI, pool_px, ptr(image_of), ptr(inv),
                                                   ptr(vec), n, dh, dw, ptr(out), ptr(status), _stream(dev)),
          "warp_affine_pool_flow_f32")
    if check_status:
        _raise_status(status, "warp_flow_targets", _POOL_BITS)
    return out, status


def head_wgrad(dlogits: torch.Tensor, feat: torch.Tensor):
    """(dW (n_cols, 256), db (n_cols,)) float32 of the 1x1 head: dW = dlogits^T feat, db = column sums; dlogits (rows, n_cols)
    float32, feat (rows, 256) in the network dtype."""
    if dlogits.dtype != torch.float32 or dlogits.dim() != 2 or feat.dim() != 2 or feat.shape != (dlogits.shape[0], 256) \
            or feat.dtype not in _DT or dlogits.shape[1] % 32 or not dlogits.is_contiguous() or not feat.is_contiguous():
        raise ValueError("head_wgrad: expected contiguous dlogits (rows, n_cols % 32 == 0) float32 and feat (rows, 256)")
    rows, N = dlogits.shape
    dev = dlogits.device
    L = _lib.lib()
    dW = torch.empty((N, 256), dtype=torch.float32, device=dev)
    db = torch.empty(N, dtype=torch.float32, device=dev)
    key = ("wgrad", rows, N, str(dev))
    if key not in _ws_cache:
        _ws_cache[key] = torch.empty(L.cpx_head_wgrad_workspace_bytes(rows, N), dtype=torch.uint8, device=dev)
    ws = _ws_cache[key]
    check(L.cpx_head_wgrad(ptr(dlogits), ptr(feat), _DT[feat.dtype], rows, N, ptr(dW), ptr(db), ptr(ws), ws.numel(),
                           _stream(dev)), "head_wgrad")
    return dW, db


def adamw_step(param: torch.Tensor, grad: torch.Tensor, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, step: int, lr: float,
               betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.1) -> None:
    """One torch.optim.AdamW step in place on float32 device tensors; ``step`` counts from 1 (bias corrections in double here)."""
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != param.numel() or t.device != param.device:
            raise ValueError("adamw_step: four contiguous float32 tensors of one size on one device")
    if step < 1:
        raise ValueError("adamw_step: step counts from 1")
    check(_lib.lib().cpx_adamw_step(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr), betas[0], betas[1],
                                    eps, weight_decay, 1.0 - betas[0] ** step, 1.0 - betas[1] ** step, _stream(param.device)),
          "adamw_step")


def round_weights(src: torch.Tensor, dst_ptr: int, dtype_code: int, keep_f32: bool) -> None:
    """``cpx_round_weights`` from a float32 device tensor into device memory at ``dst_ptr`` (16-byte aligned)."""
    check(_lib.lib().cpx_round_weights(ptr(src), dst_ptr, src.numel(), dtype_code, int(keep_f32), _stream(src.device)), "round_weights")


def unet_head_backward(weights, feat: torch.Tensor, fwd_ws: torch.Tensor, dlogits: torch.Tensor, grads: torch.Tensor,
                       workspace: torch.Tensor) -> torch.Tensor:
    """``cpx_unet_head_backward``: the gradient of every packed operand and bias of the UNet head of ``weights``
    (an ``engine.NetWeights``) into the flat float32 ``grads``.  ``feat`` (n * 1024, 256) in the network dtype, ``fwd_ws`` the
    workspace ``cpx_unet_head_forward`` ran this batch in, ``dlogits`` (n * 1024, ncls * 64) float32, ``workspace`` uint8 of at
    least ``cpx_unet_backward_workspace_bytes``."""
    c = weights.c
    L = _lib.lib()
    if not c.n_unet_ops:
        raise ValueError("unet_head_backward: the weights have no UNet head")
    if feat.dim() != 2 or feat.shape[1] != 256 or feat.shape[0] % 1024 or feat.dtype not in _DT or _DT[feat.dtype] != c.dtype \
            or not feat.is_contiguous():
        raise ValueError("unet_head_backward: feat must be contiguous (n * 1024, 256) in the network dtype")
    nS = feat.shape[0] // 1024
    if dlogits.dtype != torch.float32 or tuple(dlogits.shape) != (feat.shape[0], c.ncls * 64) or not dlogits.is_contiguous():
        raise ValueError("unet_head_backward: dlogits must be contiguous float32 (n * 1024, ncls * 64)")
    if grads.dtype != torch.float32 or not grads.is_contiguous() or \
            grads.numel() != L.cpx_unet_param_layout(c.unet_ops, c.n_unet_ops, None, None, None, None):
        raise ValueError("unet_head_backward: grads must be the flat float32 buffer of cpx_unet_param_layout")
    if workspace.dtype != torch.uint8 or fwd_ws.dtype != torch.uint8:
        raise ValueError("unet_head_backward: workspaces are uint8 tensors")
    check(L.cpx_unet_head_backward(c.unet_ops, c.n_unet_ops, ptr(feat), nS, c.dtype, ptr(fwd_ws), fwd_ws.numel(), ptr(dlogits),
                                   ptr(grads), ptr(workspace), workspace.numel(), _stream(feat.device)), "unet_head_backward")
    return grads


# ---- training the neck (csrc/cpx_train_neck.hip) ------------------------------------------------------------------
def backbone_rows(net_ws: torch.Tensor, n_subtiles: int, dtype: torch.dtype) -> torch.Tensor:
    """View of the last block's output x [n_subtiles * 1024, 1024] that ``cpx_net_forward`` left in its workspace ``net_ws`` (uint8),
    the input of the neck (``cpx_net_backbone_offset``): valid until the next forward on that workspace -- clone it to keep it."""
    off = _lib.lib().cpx_net_backbone_offset(n_subtiles, _DT[dtype])
    if off == 2 ** 64 - 1:
        raise ValueError("backbone_rows: invalid n_subtiles / dtype")
    n = n_subtiles * 1024 * 1024 * torch.empty(0, dtype=dtype).element_size()
    return net_ws[off:off + n].view(dtype).view(n_subtiles * 1024, 1024)


class NeckForwardOut:
    """Results of ``neck_forward_train``: ``head`` float32 (rows, ld_head) and views into ``workspace`` of the saved activations
    ``y0`` (before LayerNorm 1), ``a1`` (after it), ``y2`` (before LayerNorm 2) and ``feat`` (the neck output), (rows, 256) each."""
    __slots__ = ("head", "y0", "a1", "y2", "feat", "workspace")


def neck_train_workspace(n_subtiles: int, dtype_code: int, device) -> torch.Tensor:
    return torch.empty(_lib.lib().cpx_neck_train_workspace_bytes(n_subtiles, dtype_code), dtype=torch.uint8, device=device)


def neck_forward_train(weights, x: torch.Tensor, head: torch.Tensor | None = None,
                       workspace: torch.Tensor | None = None) -> NeckForwardOut:
    """``cpx_neck_forward_train``: the tail of ``cpx_net_forward`` (neck and head GEMM of ``weights``, an ``engine.NetWeights``) on
    the backbone rows ``x`` (n * 1024, 1024) in the network dtype, keeping every intermediate."""
    c, L = weights.c, _lib.lib()
    if x.dim() != 2 or x.shape[1] != 1024 or x.shape[0] == 0 or x.shape[0] % 1024 or x.dtype not in _DT or _DT[x.dtype] != c.dtype \
            or not x.is_contiguous() or not x.is_cuda:
        raise ValueError("neck_forward_train: x must be contiguous device rows (n * 1024, 1024) in the network dtype")
    if c.n_unet_ops:
        raise NotImplementedError("neck_forward_train: the neck does not train under a UNet semantic head")
    rows, nS, dev = x.shape[0], x.shape[0] // 1024, x.device
    if workspace is None:
        workspace = neck_train_workspace(nS, c.dtype, dev)
    if head is None:
        head = torch.empty((rows, c.ld_head), dtype=torch.float32, device=dev)
    if head.dtype != torch.float32 or tuple(head.shape) != (rows, c.ld_head) or not head.is_contiguous() or workspace.dtype != torch.uint8:
        raise ValueError("neck_forward_train: head must be contiguous float32 (rows, ld_head) and workspace uint8")
    check(L.cpx_neck_forward_train(C.byref(c), ptr(x), nS, ptr(head), ptr(workspace), workspace.numel(), _stream(dev)), "neck_forward_train")
    off = (C.c_size_t * 4)()
    check(L.cpx_neck_train_layout(nS, c.dtype, off), "neck_train_layout")
    o = NeckForwardOut()
    o.head, o.workspace = head, workspace
    n = rows * 256 * x.element_size()
    o.y0, o.a1, o.y2, o.feat = (workspace[off[i]:off[i] + n].view(x.dtype).view(rows, 256) for i in range(4))
    return o


def layernorm_backward(y: torch.Tensor, gamma: torch.Tensor, dout: torch.Tensor, eps: float = 1e-6):
    """``cpx_layernorm_backward``: (dy (rows, C) float32, dgamma (C,), dbeta (C,)) of LayerNorm over the C = 256 (the neck) or 1024 (a
    transformer block) channels of the stored pre-norm tensor ``y`` (rows, C) in the network dtype, from ``dout`` (rows, C) float32;
    float64 inside, rounded once."""
    if y.dim() != 2 or y.shape[1] not in (256, 1024) or y.dtype not in _DT or not y.is_contiguous() or not y.is_cuda:
        raise ValueError("layernorm_backward: y must be contiguous device rows (rows, 256) or (rows, 1024) of bf16 / fp16 / fp32")
    Cn = y.shape[1]
    if dout.dtype != torch.float32 or dout.shape != y.shape or not dout.is_contiguous() or dout.device != y.device:
        raise ValueError("layernorm_backward: dout must be contiguous float32 of y's shape on y's device")
    if gamma.dtype != torch.float32 or gamma.numel() != Cn or not gamma.is_contiguous() or gamma.device != y.device:
        raise ValueError("layernorm_backward: gamma must be float32 (C,) on y's device")
    rows, dev, L = y.shape[0], y.device, _lib.lib()
    dy = torch.empty((rows, Cn), dtype=torch.float32, device=dev)
    dgamma, dbeta = torch.empty(Cn, dtype=torch.float32, device=dev), torch.empty(Cn, dtype=torch.float32, device=dev)
    key = ("lnbwd", rows, Cn, str(dev))
    if key not in _ws_cache:
        _ws_cache[key] = torch.empty(L.cpx_layernorm_backward_bytes(rows, Cn), dtype=torch.uint8, device=dev)
    ws = _ws_cache[key]
    check(L.cpx_layernorm_backward(_DT[y.dtype], ptr(y), ptr(gamma), ptr(dout), rows, Cn, eps, ptr(dy), ptr(dgamma), ptr(dbeta),
                                   ptr(ws), ws.numel(), _stream(dev)), "layernorm_backward")
    return dy, dgamma, dbeta


NECK_GRAD_NAMES = ("W0", "gamma1", "beta1", "W2", "gamma2", "beta2")
NECK_GRAD_SHAPES = ((256, 1024), (256,), (256,), (256, 2304), (256,), (256,))


def neck_grad_layout() -> tuple[int, list[int]]:
    """(element count, element offsets of W0, gamma1, beta1, W2, gamma2, beta2) of the flat gradient buffer of ``neck_backward``."""
    off = (C.c_longlong * 6)()
    n = _lib.lib().cpx_neck_grad_layout(off)
    return int(n), [int(v) for v in off]


def neck_backward_workspace(n_subtiles: int, dtype_code: int, ld_head: int, device):
    """(uint8 workspace of ``neck_backward``, byte offsets of dfeat, dy2, da1, dy0 -- float32 (rows, 256) each -- inside it)."""
    off = (C.c_size_t * 4)()
    n = _lib.lib().cpx_neck_backward_workspace_bytes(n_subtiles, dtype_code, ld_head, off)
    if n == 0:
        raise ValueError("neck_backward_workspace: invalid n_subtiles / dtype / ld_head")
    return torch.empty(n, dtype=torch.uint8, device=device), [int(v) for v in off]


def neck_backward_workspace_offsets(n_subtiles: int, dtype_code: int, ld_head: int) -> list[int]:
    """Byte offsets of dfeat, dy2, da1, dy0 inside the workspace of ``neck_backward`` (no allocation)."""
    off = (C.c_size_t * 4)()
    if _lib.lib().cpx_neck_backward_workspace_bytes(n_subtiles, dtype_code, ld_head, off) == 0:
        raise ValueError("neck_backward_workspace_offsets: invalid n_subtiles / dtype / ld_head")
    return [int(v) for v in off]


def neck_backward(weights, x: torch.Tensor, fwd: NeckForwardOut, dhead: torch.Tensor, grads: torch.Tensor | None = None,
                  workspace: torch.Tensor | None = None) -> torch.Tensor:
    """``cpx_neck_backward``: the gradients of the six neck tensors of ``weights`` into the flat float32 ``grads``
    (``neck_grad_layout``), from ``x`` and ``fwd`` (what ``neck_forward_train`` ran this batch on and returned) and ``dhead``
    (rows, ld_head) float32, the gradient with respect to the head buffer (padding columns 0)."""
    c, L = weights.c, _lib.lib()
    rows, dev = x.shape[0], x.device
    if x.dim() != 2 or x.shape[1] != 1024 or rows == 0 or rows % 1024 or x.dtype not in _DT or _DT[x.dtype] != c.dtype or not x.is_contiguous():
        raise ValueError("neck_backward: x must be contiguous (n * 1024, 1024) in the network dtype")
    if dhead.dtype != torch.float32 or tuple(dhead.shape) != (rows, c.ld_head) or not dhead.is_contiguous() or dhead.device != dev:
        raise ValueError("neck_backward: dhead must be contiguous float32 (rows, ld_head) on x's device")
    n_g, _off = neck_grad_layout()
    if grads is None:
        grads = torch.empty(n_g, dtype=torch.float32, device=dev)
    if grads.dtype != torch.float32 or grads.numel() != n_g or not grads.is_contiguous() or grads.device != dev:
        raise ValueError("neck_backward: grads must be the flat float32 buffer of neck_grad_layout")
    if workspace is None:
        workspace, _o = neck_backward_workspace(rows // 1024, c.dtype, c.ld_head, dev)
    if workspace.dtype != torch.uint8 or fwd.workspace.dtype != torch.uint8:
        raise ValueError("neck_backward: workspaces are uint8 tensors")
    check(L.cpx_neck_backward(C.byref(c), ptr(x), rows // 1024, ptr(fwd.workspace), fwd.workspace.numel(), ptr(dhead), ptr(grads),
                              ptr(workspace), workspace.numel(), _stream(dev)), "neck_backward")
    return grads


# ---- training the transformer blocks (csrc/cpx_train_blocks.hip) ---------------------------------------------------
def attention_backward_workspace(n_subtiles: int, device) -> torch.Tensor:
    n = _lib.lib().cpx_attention_backward_workspace_bytes(n_subtiles)
    if n == 0:
        raise ValueError("attention_backward_workspace: invalid n_subtiles")
    return torch.empty(n, dtype=torch.uint8, device=device)


def attention_backward(qkv: torch.Tensor, rel_h: torch.Tensor, rel_w: torch.Tensor, out: torch.Tensor, dout: torch.Tensor,
                       workspace: torch.Tensor | None = None, grad_dtype=torch.float32):
    """``cpx_attention_backward``: (dqkv (rows, 3072), drel_h (64, 64), drel_w (64, 64)), all float32, of the function
    ``attention(qkv.float(), rel_h.float(), rel_w.float())`` computes, from the stored ``qkv`` (n * 1024, 3072) and attention output
    ``out`` (n * 1024, 1024) in the network dtype, the operand tables (64, 64) of that dtype (rel_pos / scale, zero last row) and
    ``dout`` (n * 1024, 1024) float32.  The table gradients are with respect to the operand tables, summed over heads and crops.
    ``grad_dtype`` torch.bfloat16 (bf16 tensors only): ``cpx_attention_backward_bf16``, every product on bf16 operands -- ``dout``, P and
    dS' rounded once -- with float32 accumulation; ``out`` is not read in either mode."""
    if grad_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"attention_backward: grad_dtype is torch.float32 or torch.bfloat16, not {grad_dtype}")
    if grad_dtype == torch.bfloat16 and qkv.dtype != torch.bfloat16:
        raise ValueError("attention_backward: grad_dtype torch.bfloat16 needs bf16 qkv (the operands are the stored values)")
    rows, dev = qkv.shape[0], qkv.device
    if qkv.dim() != 2 or qkv.shape[1] != 3072 or rows == 0 or rows % 1024 or qkv.dtype not in _DT or not qkv.is_contiguous() or not qkv.is_cuda:
        raise ValueError("attention_backward: qkv must be contiguous device rows (n * 1024, 3072) of bf16 / fp16 / fp32")
    for t, shape, what in ((rel_h, (64, 64), "rel_h"), (rel_w, (64, 64), "rel_w"), (out, (rows, 1024), "out")):
        if t.dtype != qkv.dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"attention_backward: {what} must be contiguous {shape} of qkv's dtype on its device")
    if dout.dtype != torch.float32 or tuple(dout.shape) != (rows, 1024) or not dout.is_contiguous() or dout.device != dev:
        raise ValueError("attention_backward: dout must be contiguous float32 (rows, 1024) on qkv's device")
    if workspace is None:
        workspace = attention_backward_workspace(rows // 1024, dev)
    if workspace.dtype != torch.uint8:
        raise ValueError("attention_backward: the workspace is a uint8 tensor")
    dqkv = torch.empty((rows, 3072), dtype=torch.float32, device=dev)
    drh, drw = torch.empty((64, 64), dtype=torch.float32, device=dev), torch.empty((64, 64), dtype=torch.float32, device=dev)
    if grad_dtype == torch.bfloat16:
        check(_lib.lib().cpx_attention_backward_bf16(ptr(qkv), ptr(rel_h), ptr(rel_w), ptr(dout), rows // 1024, ptr(dqkv), ptr(drh), ptr(drw),
                                                     ptr(workspace), workspace.numel(), _stream(dev)), "attention_backward")
        return dqkv, drh, drw
    check(_lib.lib().cpx_attention_backward(_DT[qkv.dtype], ptr(qkv), ptr(rel_h), ptr(rel_w), ptr(out), ptr(dout), rows // 1024, ptr(dqkv),
                                            ptr(drh), ptr(drw), ptr(workspace), workspace.numel(), _stream(dev)), "attention_backward")
    return dqkv, drh, drw


def gelu_backward(pre: torch.Tensor, dh: torch.Tensor) -> torch.Tensor:
    """``cpx_gelu_backward``: dh * gelu'(pre) for the erf GELU, float32 tensors of one shape (a multiple of 4 elements)."""
    if pre.dtype != torch.float32 or dh.dtype != torch.float32 or pre.shape != dh.shape or not pre.is_contiguous() or not dh.is_contiguous() \
            or not pre.is_cuda or dh.device != pre.device or pre.numel() == 0 or pre.numel() % 4:
        raise ValueError("gelu_backward: pre and dh must be contiguous float32 device tensors of one shape, a multiple of 4 elements")
    out = torch.empty_like(pre)
    check(_lib.lib().cpx_gelu_backward(ptr(pre), ptr(dh), pre.numel(), ptr(out), _stream(pre.device)), "gelu_backward")
    return out


BLOCK_GRAD_NAMES = ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "rel_h", "rel_w", "proj_w", "proj_b", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
BLOCK_GRAD_SHAPES = ((1024,), (1024,), (3072, 1024), (3072,), (64, 64), (64, 64), (1024, 1024), (1024,), (1024,), (1024,), (4096, 1024),
                     (4096,), (1024, 4096), (1024,))


def block_grad_layout() -> tuple[int, list[int]]:
    """(element count, element offsets of the 14 tensors of ``BLOCK_GRAD_NAMES``) of one block's record in the flat float32 gradient
    and parameter buffers of ``blocks_backward`` (``cpx_block_grad_layout``)."""
    off = (C.c_longlong * 14)()
    n = _lib.lib().cpx_block_grad_layout(off)
    return int(n), [int(v) for v in off]


class BlocksForwardOut:
    """Results of ``blocks_forward_train``: ``head`` float32 (rows, ld_head); per trained block views ``x[j]``, ``qkv[j]``, ``ao[j]``,
    ``x_mid[j]`` into ``workspace`` (the block's input, qkv rows, attention output, rows after the attention residual); ``x_out``, the
    last block's output (the neck's input); and ``neck``, the ``NeckForwardOut`` of the tail.  ``keep``: None, or the layer-drop mask
    (K, n) uint8 numpy the forward ran with, and ``n_keep`` the K counts of kept crops (n everywhere without a mask): the views of block
    j stay full-size and hold the block's kept crops, compacted in crop order, in their first ``n_keep[j] * 1024`` rows."""
    __slots__ = ("head", "x", "qkv", "ao", "x_mid", "x_out", "neck", "workspace", "first_block", "keep", "n_keep")


def blocks_train_workspace(n_subtiles: int, dtype_code: int, n_blocks: int, device, drop: bool = False) -> torch.Tensor:
    """The workspace of ``blocks_forward_train``; ``drop``: with the staging rows a ``keep`` mask needs behind it."""
    L = _lib.lib()
    n = (L.cpx_blocks_train_workspace_bytes_drop if drop else L.cpx_blocks_train_workspace_bytes)(n_subtiles, dtype_code, n_blocks)
    if n == 0:
        raise ValueError("blocks_train_workspace: invalid n_subtiles / dtype / n_blocks")
    return torch.empty(n, dtype=torch.uint8, device=device)


def _crop_list(crops):
    """a crop list -> (int32 numpy, its ctypes pointer); the array must outlive the call"""
    a = np.ascontiguousarray(np.asarray(crops, dtype=np.int64).reshape(-1).astype(np.int32))
    return a, a.ctypes.data_as(C.POINTER(C.c_int))


def _crop_rows(t: torch.Tensor, what: str) -> int:
    if t.dim() != 2 or t.shape[1] != 1024 or t.shape[0] % 1024 or t.dtype not in _DT or not t.is_contiguous() or not t.is_cuda:
        raise ValueError(f"{what}: contiguous device rows (n * 1024, 1024) in bf16, fp16 or float32")
    return t.shape[0] // 1024


def gather_crops(src: torch.Tensor, crops, dst: torch.Tensor | None = None, stats: torch.Tensor | None = None) -> torch.Tensor:
    """``cpx_gather_crops``: the rows of the crops ``crops`` (strictly increasing indices) of the full ``src`` (n * 1024, 1024) into the
    compact ``dst`` (len(crops) * 1024, 1024), in list order.  ``stats`` (len(crops) * 1024, 4, 2) float32, for a half type: the row
    statistics of the gathered rows in the same pass, bitwise ``cpx_row_stats`` of them."""
    nS = _crop_rows(src, "gather_crops: src")
    a, pa = _crop_list(crops)
    if dst is None:
        dst = torch.empty((a.size * 1024, 1024), dtype=src.dtype, device=src.device)
    if dst.dtype != src.dtype or dst.device != src.device or _crop_rows(dst, "gather_crops: dst") < a.size:
        raise ValueError("gather_crops: dst holds len(crops) * 1024 rows of src's dtype on its device")
    if stats is not None and (stats.dtype != torch.float32 or stats.numel() < a.size * 1024 * 8 or not stats.is_contiguous()
                              or stats.device != src.device):
        raise ValueError("gather_crops: stats is contiguous float32 (len(crops) * 1024, 4, 2)")
    check(_lib.lib().cpx_gather_crops(_DT[src.dtype], ptr(src), nS, pa, a.size, ptr(dst), ptr(stats), _stream(src.device)), "gather_crops")
    return dst


def scatter_crops(src: torch.Tensor, crops, dst: torch.Tensor) -> torch.Tensor:
    """``cpx_scatter_crops``: the compact rows ``src`` (len(crops) * 1024, 1024) back to the crops ``crops`` of the full ``dst``
    (n * 1024, 1024); the other crops of ``dst`` are untouched."""
    nS = _crop_rows(dst, "scatter_crops: dst")
    a, pa = _crop_list(crops)
    if src.dtype != dst.dtype or src.device != dst.device or _crop_rows(src, "scatter_crops: src") < a.size:
        raise ValueError("scatter_crops: src holds len(crops) * 1024 rows of dst's dtype on its device")
    check(_lib.lib().cpx_scatter_crops(_DT[dst.dtype], ptr(src), nS, pa, a.size, ptr(dst), _stream(dst.device)), "scatter_crops")
    return dst


def _keep_mask(keep, K: int, n: int, what: str):
    """a layer-drop mask -> contiguous uint8 numpy (K, n) of 0 / 1 (None stays None)"""
    if keep is None:
        return None
    if isinstance(keep, torch.Tensor):
        keep = keep.cpu().numpy()
    keep = np.asarray(keep)
    if keep.shape != (K, n) or keep.dtype.kind not in "ub":
        raise ValueError(f"{what}: keep is a uint8 array ({K}, {n}) = (trained blocks, crops), not {keep.dtype} {keep.shape}")
    return np.ascontiguousarray(keep != 0, dtype=np.uint8)


def blocks_forward_train(weights, x: torch.Tensor, first_block: int, head: torch.Tensor | None = None,
                         workspace: torch.Tensor | None = None, keep=None) -> BlocksForwardOut:
    """``cpx_blocks_forward_train_drop``: blocks ``first_block`` .. depth - 1 of ``weights`` (an ``engine.NetWeights``) and the tail on the
    rows ``x`` (n * 1024, 1024) in the network dtype -- the input of block ``first_block`` --, keeping what the backward needs.  Without
    ``keep`` the mask pointer is null: ``cpx_blocks_forward_train``.  ``keep`` (K, n) uint8, host: layer drop, block j runs on crop i where
    ``keep[j, i]`` is non-zero and passes the other crops through; the workspace is then ``blocks_train_workspace(..., drop=True)``."""
    c, L = weights.c, _lib.lib()
    if x.dim() != 2 or x.shape[1] != 1024 or x.shape[0] == 0 or x.shape[0] % 1024 or x.dtype not in _DT or _DT[x.dtype] != c.dtype \
            or not x.is_contiguous() or not x.is_cuda:
        raise ValueError("blocks_forward_train: x must be contiguous device rows (n * 1024, 1024) in the network dtype")
    if c.n_unet_ops:
        raise NotImplementedError("blocks_forward_train: the blocks do not train under a UNet semantic head (the neck does not)")
    if not 0 <= first_block < c.depth:
        raise ValueError(f"blocks_forward_train: first_block {first_block} outside 0 .. {c.depth - 1}")
    rows, nS, dev, K = x.shape[0], x.shape[0] // 1024, x.device, c.depth - first_block
    keep = _keep_mask(keep, K, nS, "blocks_forward_train")
    if workspace is None:
        workspace = blocks_train_workspace(nS, c.dtype, K, dev, drop=keep is not None)
    if head is None:
        head = torch.empty((rows, c.ld_head), dtype=torch.float32, device=dev)
    if head.dtype != torch.float32 or tuple(head.shape) != (rows, c.ld_head) or not head.is_contiguous() or workspace.dtype != torch.uint8:
        raise ValueError("blocks_forward_train: head must be contiguous float32 (rows, ld_head) and workspace uint8")
    check(L.cpx_blocks_forward_train_drop(C.byref(c), ptr(x), nS, first_block, None if keep is None else keep.ctypes.data, ptr(head),
                                          ptr(workspace), workspace.numel(), _stream(dev)),
          "blocks_forward_train" if keep is None else "blocks_forward_train (keep)")
    off = (C.c_size_t * (4 * K + 2))()
    check(L.cpx_blocks_train_layout(nS, c.dtype, K, off), "blocks_train_layout")
    es = x.element_size()

    def view(o, width):
        return workspace[o:o + rows * width * es].view(x.dtype).view(rows, width)
    o = BlocksForwardOut()
    o.head, o.workspace, o.first_block = head, workspace, first_block
    o.keep, o.n_keep = keep, [nS] * K if keep is None else [int(v) for v in keep.sum(axis=1)]
    o.x, o.qkv, o.ao, o.x_mid = ([view(off[4 * j + i], wd) for j in range(K)] for i, wd in enumerate((1024, 3072, 1024, 1024)))
    o.x_out = view(off[4 * K], 1024)
    nb = L.cpx_neck_train_workspace_bytes(nS, c.dtype)
    nws = workspace[off[4 * K + 1]:off[4 * K + 1] + nb]
    noff = (C.c_size_t * 4)()
    check(L.cpx_neck_train_layout(nS, c.dtype, noff), "neck_train_layout")
    nk = NeckForwardOut()
    nk.head, nk.workspace = head, nws
    nk.y0, nk.a1, nk.y2, nk.feat = (nws[noff[i]:noff[i] + rows * 256 * es].view(x.dtype).view(rows, 256) for i in range(4))
    o.neck = nk
    return o


def _grad_dtype_code(grad_dtype, net_dtype_code: int, what: str) -> int:
    """the ``grad_dtype`` argument of the blocks' backward -> its dtype code; bf16 gradients go with a bf16 network only"""
    if grad_dtype == torch.float32:
        return _DT[torch.float32]
    if grad_dtype != torch.bfloat16:
        raise ValueError(f"{what}: grad_dtype is torch.float32 or torch.bfloat16, not {grad_dtype}")
    if net_dtype_code != _DT[torch.bfloat16]:
        raise ValueError(f"{what}: grad_dtype torch.bfloat16 needs a bf16 network (fp16 gradients would need loss scaling; a float32 "
                         "network has no half-precision operands)")
    return _DT[torch.bfloat16]


def _attn_grad_dtype_code(attn_grad_dtype, grad_dtype_code: int, what: str) -> int:
    """the ``attn_grad_dtype`` argument of the blocks' backward -> its dtype code; a bf16 attention backward goes with bf16 gradient GEMMs only"""
    if attn_grad_dtype == torch.float32:
        return _DT[torch.float32]
    if attn_grad_dtype != torch.bfloat16:
        raise ValueError(f"{what}: attn_grad_dtype is torch.float32 or torch.bfloat16, not {attn_grad_dtype}")
    if grad_dtype_code != _DT[torch.bfloat16]:
        raise ValueError(f"{what}: attn_grad_dtype torch.bfloat16 needs grad_dtype torch.bfloat16")
    return _DT[torch.bfloat16]


def blocks_backward_workspace(n_subtiles: int, dtype_code: int, device, grad_dtype=torch.float32, attn_grad_dtype=torch.float32) -> torch.Tensor:
    gd = _grad_dtype_code(grad_dtype, dtype_code, "blocks_backward_workspace")
    n = _lib.lib().cpx_blocks_backward_workspace_bytes_mp(n_subtiles, dtype_code, gd, _attn_grad_dtype_code(attn_grad_dtype, gd, "blocks_backward_workspace"))
    if n == 0:
        raise ValueError("blocks_backward_workspace: invalid n_subtiles / dtype")
    return torch.empty(n, dtype=torch.uint8, device=device)


def blocks_backward(weights, params: torch.Tensor, fwd: BlocksForwardOut, dy0: torch.Tensor, grads: torch.Tensor | None = None,
                    workspace: torch.Tensor | None = None, dx_all: torch.Tensor | None = None, grad_dtype=torch.float32,
                    attn_grad_dtype=torch.float32, dx_in: torch.Tensor | None = None) -> torch.Tensor:
    """``cpx_blocks_backward_drop``: the gradients of the K trained blocks of ``fwd`` into the flat float32 ``grads`` (K records of
    ``block_grad_layout``), from ``params`` (the K blocks' unfolded parameters as the forward reads them, same layout) and ``dy0``
    (rows, 256) float32, which ``neck_backward`` leaves in its workspace.  ``dx_all`` (K + 1, rows, 1024) float32, when given, receives
    the gradient of every trained block's input and (last) of the last block's output.  ``grad_dtype`` torch.float32: the exact-float32
    products of ``cpx_blocks_backward``; torch.bfloat16 (a bf16 network only): every product on bf16 operands with float32 accumulation.
    ``attn_grad_dtype`` torch.bfloat16 (with ``grad_dtype`` torch.bfloat16 only): the attention backward on bf16 operands too
    (``cpx_attention_backward_bf16``); torch.float32 leaves it in float32.  ``dx_in`` (rows, 1024) float32, when given, receives the
    gradient of the first trained block's input alone (record 0 of ``dx_all`` without the rest): what ``embed_backward`` takes.
    The mask of a forward under layer drop (``fwd.keep``) goes along; without one the mask pointer is null (``cpx_blocks_backward_in``)."""
    c, L = weights.c, _lib.lib()
    gd = _grad_dtype_code(grad_dtype, c.dtype, "blocks_backward")
    ad = _attn_grad_dtype_code(attn_grad_dtype, gd, "blocks_backward")
    K, rows, dev = len(fwd.x), fwd.x_out.shape[0], fwd.x_out.device
    n_g, _off = block_grad_layout()
    if params.dtype != torch.float32 or params.numel() != n_g * K or not params.is_contiguous() or params.device != dev:
        raise ValueError("blocks_backward: params must be the flat float32 buffer of K records of block_grad_layout")
    if dy0.dtype != torch.float32 or tuple(dy0.shape) != (rows, 256) or not dy0.is_contiguous() or dy0.device != dev:
        raise ValueError("blocks_backward: dy0 must be contiguous float32 (rows, 256) on the forward's device")
    if grads is None:
        grads = torch.empty(n_g * K, dtype=torch.float32, device=dev)
    if grads.dtype != torch.float32 or grads.numel() != n_g * K or not grads.is_contiguous() or grads.device != dev:
        raise ValueError("blocks_backward: grads must be the flat float32 buffer of K records of block_grad_layout")
    if dx_all is not None and (dx_all.dtype != torch.float32 or tuple(dx_all.shape) != (K + 1, rows, 1024) or not dx_all.is_contiguous()
                               or dx_all.device != dev):
        raise ValueError("blocks_backward: dx_all must be contiguous float32 (K + 1, rows, 1024)")
    if dx_in is not None and (dx_in.dtype != torch.float32 or tuple(dx_in.shape) != (rows, 1024) or not dx_in.is_contiguous()
                              or dx_in.device != dev):
        raise ValueError("blocks_backward: dx_in must be contiguous float32 (rows, 1024)")
    if workspace is None:
        workspace = blocks_backward_workspace(rows // 1024, c.dtype, dev, grad_dtype, attn_grad_dtype)
    if workspace.dtype != torch.uint8 or fwd.workspace.dtype != torch.uint8:
        raise ValueError("blocks_backward: workspaces are uint8 tensors")
    keep = getattr(fwd, "keep", None)                      # (a BlocksForwardOut put together by hand has no mask)
    check(L.cpx_blocks_backward_drop(C.byref(c), ptr(params), rows // 1024, fwd.first_block, None if keep is None else keep.ctypes.data,
                                     ptr(fwd.workspace), fwd.workspace.numel(), ptr(dy0), gd, ad, ptr(grads), ptr(dx_all), ptr(dx_in), ptr(workspace),
                                     workspace.numel(), _stream(dev)), "blocks_backward" if keep is None else "blocks_backward (keep)")
    return grads


def gemm_tn_bf16(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None, add: bool = False) -> torch.Tensor:
    """``cpx_gemm_tn_bf16``: a^T b for bf16 device matrices a (M, N) and b (M, K), float32 accumulation, into (or, with ``add``, on top
    of) the float32 ``out`` (N, K) -- which may be a column slice of a wider contiguous matrix."""
    if a.dtype != torch.bfloat16 or b.dtype != torch.bfloat16 or a.dim() != 2 or b.dim() != 2 or a.shape[0] != b.shape[0] \
            or not a.is_contiguous() or not b.is_contiguous() or not a.is_cuda or b.device != a.device:
        raise ValueError("gemm_tn_bf16: a (M, N) and b (M, K) must be contiguous bf16 matrices on one device")
    (M, N), K = a.shape, b.shape[1]
    if out is None:
        if add:
            raise ValueError("gemm_tn_bf16: add needs an out to add to")
        out = torch.empty((N, K), dtype=torch.float32, device=a.device)
    if out.dtype != torch.float32 or tuple(out.shape) != (N, K) or out.stride(1) != 1 or out.device != a.device:
        raise ValueError("gemm_tn_bf16: out must be float32 (N, K) with unit column stride on the operands' device")
    check(_lib.lib().cpx_gemm_tn_bf16(ptr(a), ptr(b), M, N, K, int(bool(add)), ptr(out), out.stride(0), _stream(a.device)), "gemm_tn_bf16")
    return out


def colsum_add(dy: torch.Tensor, db: torch.Tensor, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """``cpx_colsum_add``: db += the column sums of the float32 (rows, N) ``dy``, float64 partial sums in a fixed tree, in place."""
    if dy.dtype != torch.float32 or dy.dim() != 2 or not dy.is_contiguous() or not dy.is_cuda or db.dtype != torch.float32 \
            or tuple(db.shape) != (dy.shape[1],) or not db.is_contiguous() or db.device != dy.device:
        raise ValueError("colsum_add: dy (rows, N) and db (N,) must be contiguous float32 tensors on one device")
    rows, N = dy.shape
    n = _lib.lib().cpx_colsum_workspace_bytes(rows, N)
    if n == 0:
        raise ValueError("colsum_add: rows and N must be positive multiples of 64")
    if workspace is None:
        workspace = torch.empty(n, dtype=torch.uint8, device=dy.device)
    if workspace.dtype != torch.uint8:
        raise ValueError("colsum_add: the workspace is a uint8 tensor")
    check(_lib.lib().cpx_colsum_add(ptr(dy), rows, N, ptr(db), ptr(workspace), workspace.numel(), _stream(dy.device)), "colsum_add")
    return db


EMBED_GRAD_NAMES = ("pe_w", "pe_b", "pos")
EMBED_GRAD_SHAPES = ((1024, 192), (1024,), (1024, 1024))


def embed_grad_layout() -> tuple[int, list[int]]:
    """(element count, element offsets of the three tensors of ``EMBED_GRAD_NAMES``) of the flat float32 record of ``embed_backward``
    (``cpx_embed_grad_layout``): W (1024, 192) with k in the order of ``patchify_f32``, b (1024,), pos (1024, 1024)."""
    off = (C.c_longlong * 3)()
    n = _lib.lib().cpx_embed_grad_layout(off)
    return int(n), [int(v) for v in off]


def embed_backward_workspace(n_subtiles: int, dtype_code: int, device, grad_dtype=torch.float32) -> torch.Tensor:
    gd = _grad_dtype_code(grad_dtype, dtype_code, "embed_backward_workspace")
    n = _lib.lib().cpx_embed_backward_workspace_bytes(n_subtiles, dtype_code, gd)
    if n == 0:
        raise ValueError("embed_backward_workspace: invalid n_subtiles / dtype")
    return torch.empty(n, dtype=torch.uint8, device=device)


def embed_backward(patches: torch.Tensor, dx_in: torch.Tensor, grads: torch.Tensor | None = None, workspace: torch.Tensor | None = None,
                   grad_dtype=torch.float32) -> torch.Tensor:
    """``cpx_embed_backward``: the gradients of the patch embedding ``x = round(p W^T + b + pos)`` into the flat float32 ``grads`` (one
    record of ``embed_grad_layout``, overwritten), from the patch rows ``patches`` (n * 1024, 192) in the network dtype as the forward
    read them and ``dx_in`` (n * 1024, 1024) float32, the gradient of block 0's input (``blocks_backward(..., dx_in=)``).  ``grad_dtype``
    torch.float32: dW on the exact-float32 MFMA; torch.bfloat16 (bf16 patches only): dW = r(dx)^T p on the bf16 MFMA with float32
    accumulation.  db and dpos are float64 sums of the unrounded ``dx_in`` in both modes."""
    if patches.dim() != 2 or patches.shape[1] != 192 or patches.shape[0] == 0 or patches.shape[0] % 1024 or patches.dtype not in _DT \
            or not patches.is_contiguous() or not patches.is_cuda:
        raise ValueError("embed_backward: patches must be contiguous device rows (n * 1024, 192) in a network dtype")
    rows, dev, dt = patches.shape[0], patches.device, _DT[patches.dtype]
    gd = _grad_dtype_code(grad_dtype, dt, "embed_backward")
    if dx_in.dtype != torch.float32 or tuple(dx_in.shape) != (rows, 1024) or not dx_in.is_contiguous() or dx_in.device != dev:
        raise ValueError("embed_backward: dx_in must be contiguous float32 (rows, 1024) on the patches' device")
    n_g, _off = embed_grad_layout()
    if grads is None:
        grads = torch.empty(n_g, dtype=torch.float32, device=dev)
    if grads.dtype != torch.float32 or grads.numel() != n_g or not grads.is_contiguous() or grads.device != dev:
        raise ValueError("embed_backward: grads must be the flat float32 record of embed_grad_layout")
    if workspace is None:
        workspace = embed_backward_workspace(rows // 1024, dt, dev, grad_dtype)
    if workspace.dtype != torch.uint8:
        raise ValueError("embed_backward: the workspace is a uint8 tensor")
    check(_lib.lib().cpx_embed_backward(dt, ptr(patches), ptr(dx_in), rows // 1024, gd, ptr(grads), ptr(workspace), workspace.numel(),
                                        _stream(dev)), "embed_backward")
    return grads


# ---- t2: training-time augmentation (csrc/cpx_augment.hip) --------------------------------------------------------
def hed_jitter(img_u8: torch.Tensor, sigma: torch.Tensor, bias: torch.Tensor, cutoff_range=(0.15, 0.85),
               simple_mode: bool = False):
    """``HEDTransform.transform`` on uint8 (n, H, W, 3) device patches with the per-image draws ``sigma`` / ``bias`` (n, 3) float32.
    Returns (uint8 patches, int32 (n,) ``applied``: 0 where the patch mean lies outside ``cutoff_range`` and the patch is a copy)."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise ValueError("hed_jitter: expected uint8 (n, H, W, 3)")
    img_u8 = img_u8.contiguous()
    n, H, W, _c = img_u8.shape
    dev = img_u8.device
    sigma = torch.as_tensor(sigma, dtype=torch.float32).to(dev).contiguous()
    bias = torch.as_tensor(bias, dtype=torch.float32).to(dev).contiguous()
    if sigma.shape != (n, 3) or bias.shape != (n, 3):
        raise ValueError("hed_jitter: sigma and bias are (n, 3)")
    out = torch.empty_like(img_u8)
    applied = torch.empty(n, dtype=torch.int32, device=dev)
    check(_lib.lib().cpx_hed_jitter_u8(ptr(img_u8), n, H, W, ptr(sigma), ptr(bias), float(cutoff_range[0]), float(cutoff_range[1]),
                                       int(bool(simple_mode)), ptr(out), ptr(applied), _stream(dev)), "hed_jitter_u8")
    return out, applied


def warp_affine(src: torch.Tensor, inv, out_hw, labels: torch.Tensor | None = None, label_fill: int = 0):
    """Affine warp of uint8 (n, sh, sw, 3) or float32 (n, 3, sh, sw) device images by the per-image INVERSE maps ``inv`` (n, 6)
    float64 (source = inv . (x, y, 1)) into float32 (n, 3, dh, dw): bilinear with a constant border of 0; int16 ``labels``
    (n, sh, sw) are sampled at the nearest pixel, ``label_fill`` outside the source.  Returns (image, labels or None)."""
    dh, dw = (int(v) for v in out_hw)
    u8 = src.dtype == torch.uint8
    if src.dim() != 4 or not ((u8 and src.shape[3] == 3) or (src.dtype == torch.float32 and src.shape[1] == 3)):
        raise ValueError("warp_affine: expected uint8 (n, sh, sw, 3) or float32 (n, 3, sh, sw)")
    src = src.contiguous()
    n = src.shape[0]
    sh, sw = (src.shape[1], src.shape[2]) if u8 else (src.shape[2], src.shape[3])
    dev = src.device
    inv = _f64(inv, dev)
    if inv.shape != (n, 6):
        raise ValueError("warp_affine: inv is (n, 6) float64")
    lab_out = None
    if labels is not None:
        if labels.dtype != torch.int16 or labels.shape != (n, sh, sw) or labels.device != dev:
            raise ValueError("warp_affine: labels must be int16 (n, sh, sw) on the images' device")
        labels = labels.contiguous()
        lab_out = torch.empty((n, dh, dw), dtype=torch.int16, device=dev)
    out = torch.empty((n, 3, dh, dw), dtype=torch.float32, device=dev)
    fn = _lib.lib().cpx_warp_affine_u8 if u8 else _lib.lib().cpx_warp_affine_f32
    check(fn(ptr(src), ptr(labels), n, sh, sw, ptr(inv), dh, dw, int(label_fill), ptr(out), ptr(lab_out), _stream(dev)), "warp_affine")
    return out, lab_out


def _f64(a, dev) -> torch.Tensor:
    a = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64) if not isinstance(a, torch.Tensor) else a)
    return a.to(device=dev, dtype=torch.float64).contiguous()


def _pool_table(pool, px_off, hw, what: str, dtype=torch.uint8):
    """(device, nI, pool_px) of a ragged pool of 3 ``dtype`` values per pixel with its table (px_off, hw)."""
    if pool.dtype != dtype or pool.dim() != 1 or pool.numel() % 3 or not pool.is_contiguous() or not pool.is_cuda:
        name, unit = ("pool_u8", "uint8 device vector of 3 bytes") if dtype == torch.uint8 else ("pool_tgt", "float32 device vector of 3 values")
        raise ValueError(f"{what}: {name} is a contiguous {unit} per pixel")
    dev = pool.device
    nI = px_off.numel()
    if px_off.dtype != torch.int64 or px_off.dim() != 1 or nI == 0 or px_off.device != dev or not px_off.is_contiguous():
        raise ValueError(f"{what}: px_off is int64 (nI,) on the pool's device")
    if hw.dtype != torch.int32 or hw.shape != (nI, 2) or hw.device != dev or not hw.is_contiguous():
        raise ValueError(f"{what}: hw is int32 (nI, 2) on the pool's device")
    return dev, nI, pool.numel() // 3


def _crop_maps(image_of, inv, dev, what: str, vec=None):
    """(image_of (n,) int32, inv (n, 6) float64, vec (n, 4) float64 or None, n) of a pool warp's crops on ``dev``."""
    image_of = torch.as_tensor(image_of).to(device=dev, dtype=torch.int32).contiguous()
    n = image_of.numel()
    inv, vec = _f64(inv, dev), None if vec is None else _f64(vec, dev)
    if image_of.dim() != 1 or n == 0 or inv.shape != (n, 6) or (vec is not None and vec.shape != (n, 4)):
        raise ValueError(f"{what}: image_of is (n,), inv (n, 6)" + ("" if vec is None else " and vec (n, 4)") + " float64")
    return image_of, inv, vec, n


def _pool_outputs(pool_lab, pool_px: int, n: int, out_hw, dev, what: str):
    """(dh, dw, float32 (n, 3, dh, dw), int16 (n, dh, dw) or None without ``pool_lab``, int32 (1,) status) of a pool warp."""
    dh, dw = (int(v) for v in out_hw)
    lab_out = None
    if pool_lab is not None:
        if pool_lab.dtype != torch.int16 or pool_lab.shape != (pool_px,) or pool_lab.device != dev or not pool_lab.is_contiguous():
            raise ValueError(f"{what}: pool_lab is a contiguous int16 vector of one label per pool pixel on the pool's device")
        lab_out = torch.empty((n, dh, dw), dtype=torch.int16, device=dev)
    out = torch.empty((n, 3, dh, dw), dtype=torch.float32, device=dev)
    return dh, dw, out, lab_out, torch.empty(1, dtype=torch.int32, device=dev)


_POOL_BITS = ((1, "an image index outside the pool"), (2, "a table entry outside the pool"))


def _raise_status(status: torch.Tensor, what: str, texts) -> None:
    """``ValueError`` with the text of the first set bit of ``texts`` ((bit, text), ...) when the status word is not zero."""
    bits = int(status.item())
    if bits:
        raise ValueError(f"{what}: " + next((text for bit, text in texts if bits & bit), f"status {bits}"))


def pool_byte_sums(pool_u8: torch.Tensor, px_off: torch.Tensor, hw: torch.Tensor) -> torch.Tensor:
    """Exact integer byte sum of every image of a ragged pool (``cpx_pool_byte_sums``): pool_u8 the images packed back to back as
    (h_i, w_i, 3) uint8, px_off (nI,) int64 pixel offsets, hw (nI, 2) int32.  Returns int64 (nI,) on the device; raises ``ValueError``
    when a table entry does not lie inside the pool (nothing is read through it)."""
    dev, nI, pool_px = _pool_table(pool_u8, px_off, hw, "pool_byte_sums")
    sums = torch.empty(nI, dtype=torch.int64, device=dev)                     # a sum is below 2^63: the uint64 of the kernel, as int64
    status = torch.empty(1, dtype=torch.int32, device=dev)
    check(_lib.lib().cpx_pool_byte_sums(ptr(pool_u8), ptr(px_off), ptr(hw), nI, pool_px, ptr(sums), ptr(status), _stream(dev)),
          "pool_byte_sums")
    if int(status.item()):
        raise ValueError("pool_byte_sums: an image of the table lies outside the pool")
    return sums


def warp_affine_pool(pool_u8: torch.Tensor, pool_lab: torch.Tensor | None, px_off: torch.Tensor, hw: torch.Tensor, image_of, inv,
                     out_hw, sigma=None, bias=None, applied=None, simple_mode: bool = False, label_fill: int = 0,
                     check_status: bool = True):
    """``cpx_warp_affine_pool_u8``: crop t is ``warp_affine`` of image ``image_of[t]`` of the pool by ``inv[t]``; with ``sigma`` / ``bias``
    (n, 3) float32 and ``applied`` (n,) int32, all per crop, the stain jitter of ``hed_jitter`` is applied to the in-source taps of the
    crops with ``applied != 0`` -- bitwise ``hed_jitter`` of the whole image, then ``warp_affine``.  pool_lab: int16 class maps at the
    pool's pixel offsets, or None.  Returns (float32 (n, 3, dh, dw), int16 (n, dh, dw) or None, int32 (1,) status: bit 0 an
    ``image_of`` outside the pool's images, bit 1 a table entry outside the pool; such crops are zeros / ``label_fill``).
    ``check_status`` raises ``ValueError`` on a non-zero status."""
    dev, nI, pool_px = _pool_table(pool_u8, px_off, hw, "warp_affine_pool")
    image_of, inv, _vec, n = _crop_maps(image_of, inv, dev, "warp_affine_pool")
    if (sigma is None) != (bias is None) or (sigma is None) != (applied is None):
        raise ValueError("warp_affine_pool: sigma, bias and applied go together")
    if sigma is not None:
        sigma = torch.as_tensor(sigma, dtype=torch.float32).to(dev).contiguous()
        bias = torch.as_tensor(bias, dtype=torch.float32).to(dev).contiguous()
        applied = torch.as_tensor(applied).to(device=dev, dtype=torch.int32).contiguous()
        if sigma.shape != (n, 3) or bias.shape != (n, 3) or applied.shape != (n,):
            raise ValueError("warp_affine_pool: sigma and bias are (n, 3), applied (n,)")
    dh, dw, out, lab_out, status = _pool_outputs(pool_lab, pool_px, n, out_hw, dev, "warp_affine_pool")
    check(_lib.lib().cpx_warp_affine_pool_u8(ptr(pool_u8), ptr(pool_lab), ptr(px_off), ptr(hw), nI, pool_px, ptr(image_of), ptr(inv), n,
                                             ptr(sigma), ptr(bias), ptr(applied), int(bool(simple_mode)), dh, dw, int(label_fill),
                                             ptr(out), ptr(lab_out), ptr(status), _stream(dev)), "warp_affine_pool_u8")
    if check_status:
        _raise_status(status, "warp_affine_pool", _POOL_BITS)
    return out, lab_out, status


# ---- t5: H&E stain-matrix perturbation (csrc/cpx_augment.hip, host side in stain.py) --------------------------------
_stain_tables: dict = {}


def _stain_table(dev, which: str) -> torch.Tensor:
    """The 256-entry float64 table ``which`` ("density" / "linear") of ``stain`` on ``dev``, uploaded once per device."""
    from . import stain
    key = (which, str(dev))
    if key not in _stain_tables:
        host = stain.density_table() if which == "density" else stain.linear_table()
        _stain_tables[key] = torch.from_numpy(np.ascontiguousarray(host, np.float64)).to(dev)
    return _stain_tables[key]


def stain_samples(pool_u8: torch.Tensor, px_off: torch.Tensor, hw: torch.Tensor, out_off=None, out_triples: int | None = None,
                  check_status: bool = True):
    """``cpx_stain_samples`` on a ragged pool (layout as ``pool_byte_sums``): per image the tissue-pixel count and the bytes of the
    pixels ``extract_stains`` fits its NMF on (``stain.select_samples`` is the host statement).  Returns ``(k (nI,) int64 on the
    host, samples: a list of (m_i, 3) uint8 host arrays, status (1,) int32 device, raw (out_triples, 3) uint8 device buffer)``.
    ``out_off`` (nI,) int64, the triple offset of every image in the buffer, and ``out_triples`` default to the capacities
    ``stain.sample_capacity`` packed back to back; the buffer starts zeroed.  Status bit 1: a table entry outside the pool, bit 2: an
    output range outside the buffer -- ``check_status`` raises ``ValueError`` on either."""
    from . import stain
    dev, nI, pool_px = _pool_table(pool_u8, px_off, hw, "stain_samples")
    hw_host = hw.cpu().numpy().astype(np.int64)
    px = hw_host[:, 0] * hw_host[:, 1]
    cap = stain.sample_capacity(np.maximum(px, 0))
    if out_off is None:
        out_off = np.concatenate([[0], np.cumsum(cap)[:-1]]).astype(np.int64)
    out_off = np.ascontiguousarray(out_off, np.int64)
    if out_off.shape != (nI,):
        raise ValueError("stain_samples: out_off is (nI,) int64")
    if out_triples is None:
        out_triples = int(max(1, (out_off + cap).max()))
    L = _lib.lib()
    ws = torch.empty(max(8, L.cpx_stain_samples_workspace_bytes(nI, pool_px)), dtype=torch.uint8, device=dev)
    raw = torch.zeros((int(out_triples), 3), dtype=torch.uint8, device=dev)
    k = torch.zeros(nI, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    off_dev = torch.from_numpy(out_off).to(dev)
    check(L.cpx_stain_samples(ptr(pool_u8), ptr(px_off), ptr(hw), nI, pool_px, ptr(_stain_table(dev, "linear")), float(stain.Y_THRESHOLD),
                              ptr(off_dev), int(out_triples), ptr(k), ptr(raw), ptr(status), ptr(ws),
                              ws.numel(), _stream(dev)), "stain_samples")
    bits = int(status.item())
    if check_status and bits:
        raise ValueError("stain_samples: " + ("an image of the table lies outside the pool" if bits & 2
                                              else "a sample range lies outside the output buffer"))
    k_host, raw_host = k.cpu().numpy(), raw.cpu().numpy()
    samples = []
    for i in range(nI):
        m = int(stain.n_selected(k_host[i], px[i])) if px[i] > 0 else 0
        ok = 0 <= out_off[i] and out_off[i] + cap[i] <= out_triples
        samples.append(raw_host[out_off[i]:out_off[i] + m].copy() if ok else np.zeros((0, 3), np.uint8))
    return k_host, samples, status, raw


def _stain_args(params, mode, n: int, dev, what: str):
    params = _f64(params, dev)
    mode = torch.as_tensor(mode).to(device=dev, dtype=torch.int32).contiguous()
    if params.shape != (n, 14) or mode.shape != (n,):
        raise ValueError(f"{what}: params are (n, 14) float64 and mode (n,) int32")
    return params, mode


def he_stain(img_u8: torch.Tensor, params, mode) -> torch.Tensor:
    """``augment_stains`` on uint8 (n, H, W, 3) device images with the per-image ``params`` (n, 14) float64 of
    ``stain.stain_params`` (Hinv, M, the two stain factors); image t is transformed where ``mode[t] == 2`` and copied elsewhere."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise ValueError("he_stain: expected uint8 (n, H, W, 3)")
    img_u8 = img_u8.contiguous()
    n, H, W, _c = img_u8.shape
    dev = img_u8.device
    params, mode = _stain_args(params, mode, n, dev, "he_stain")
    out = torch.empty_like(img_u8)
    check(_lib.lib().cpx_he_stain_u8(ptr(img_u8), n, H, W, ptr(params), ptr(mode), ptr(_stain_table(dev, "density")), ptr(out),
                                     _stream(dev)), "he_stain_u8")
    return out


def warp_affine_pool_stain(pool_u8: torch.Tensor, pool_lab: torch.Tensor | None, px_off: torch.Tensor, hw: torch.Tensor, image_of,
                           inv, out_hw, mode, sigma=None, bias=None, simple_mode: bool = False, params=None, label_fill: int = 0,
                           check_status: bool = True):
    """``cpx_warp_affine_pool_stain_u8``: ``warp_affine_pool`` with a colour transform per crop, ``mode`` (n,) int32 -- 0 none, 1 the
    stain jitter with ``sigma`` / ``bias`` (n, 3) (the cut-off already applied by the caller), 2 the stain perturbation of ``he_stain``
    with ``params`` (n, 14).  ``sigma`` / ``bias`` / ``params`` left out are zeros (their modes must then not occur).  Returns what
    ``warp_affine_pool`` returns."""
    dev, nI, pool_px = _pool_table(pool_u8, px_off, hw, "warp_affine_pool_stain")
    image_of, inv, _vec, n = _crop_maps(image_of, inv, dev, "warp_affine_pool_stain")
    mode, sigma, bias, params = _colour_args(mode, sigma, bias, params, n, dev, "warp_affine_pool_stain")
    dh, dw, out, lab_out, status = _pool_outputs(pool_lab, pool_px, n, out_hw, dev, "warp_affine_pool_stain")
    check(_lib.lib().cpx_warp_affine_pool_stain_u8(ptr(pool_u8), ptr(pool_lab), ptr(px_off), ptr(hw), nI, pool_px, ptr(image_of), ptr(inv),
                                                   n, ptr(sigma), ptr(bias), int(bool(simple_mode)), ptr(params),
                                                   ptr(_stain_table(dev, "density")), ptr(mode), dh, dw, int(label_fill), ptr(out),
                                                   ptr(lab_out), ptr(status), _stream(dev)), "warp_affine_pool_stain_u8")
    if check_status:
        _raise_status(status, "warp_affine_pool_stain", _POOL_BITS)
    return out, lab_out, status


# ---- t6: image quality -- Gaussian blur and hue / brightness / saturation (csrc/cpx_augment.hip) ------------------------------
BLUR_MAX_RADIUS = 8
_unit_tables: dict = {}


def unit_table_host() -> np.ndarray:
    """``arange(256, float32) / float32(255)``: the float32 value of every byte as ``_hbs_adjust`` forms it, numpy's own division."""
    return np.arange(256, dtype=np.float32) / np.float32(255)


def _unit_table(dev) -> torch.Tensor:
    key = str(dev)
    if key not in _unit_tables:
        _unit_tables[key] = torch.from_numpy(unit_table_host()).to(dev)
    return _unit_tables[key]


def _hbs_args(hbs, apply, n: int, dev, what: str):
    hbs = torch.zeros((n, 4), dtype=torch.float32) if hbs is None else torch.as_tensor(hbs, dtype=torch.float32)
    apply = torch.zeros(n, dtype=torch.int32) if apply is None else torch.as_tensor(apply)
    hbs, apply = hbs.to(dev).contiguous(), apply.to(device=dev, dtype=torch.int32).contiguous()
    if hbs.shape != (n, 4) or apply.shape != (n,):
        raise ValueError(f"{what}: hbs is (n, 4) float32 {{hue, brightness, saturation, 1 - saturation}} and apply (n,)")
    return hbs, apply


def hbs(img_u8: torch.Tensor, hbs, apply) -> torch.Tensor:
    """``_hbs_adjust`` (hue shift, brightness, saturation in float32) on uint8 (n, H, W, 3) device images with the per-image values
    ``hbs`` (n, 4) float32 {hue, brightness, saturation, 1 - saturation}; image t is transformed where ``apply[t] != 0`` and copied
    elsewhere."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3:
        raise ValueError("hbs: expected uint8 (n, H, W, 3)")
    img_u8 = img_u8.contiguous()
    n, H, W, _c = img_u8.shape
    dev = img_u8.device
    par, apply = _hbs_args(hbs, apply, n, dev, "hbs")
    out = torch.empty_like(img_u8)
    check(_lib.lib().cpx_hbs_u8(ptr(img_u8), n, H, W, ptr(par), ptr(apply), ptr(_unit_table(dev)), ptr(out), _stream(dev)), "hbs_u8")
    return out


def _colour_args(mode, sigma, bias, params, n: int, dev, what: str):
    """mode (n,) in {0, 1, 2} (None = all 0), sigma / bias (n, 3) float32 and params (n, 14) float64 of the pool kernels' colour
    stage on ``dev``; what is left out is zeros, and its mode must then not occur."""
    mode_host = np.zeros(n, np.int64) if mode is None else np.asarray(mode.cpu() if isinstance(mode, torch.Tensor) else mode).astype(np.int64)
    if mode_host.shape != (n,) or mode_host.min() < 0 or mode_host.max() > 2:
        raise ValueError(f"{what}: mode is (n,) with values 0, 1, 2")
    if (sigma is None) != (bias is None) or (sigma is None and (mode_host == 1).any()) or (params is None and (mode_host == 2).any()):
        raise ValueError(f"{what}: mode 1 needs sigma and bias, mode 2 needs params")
    sigma = torch.zeros((n, 3), dtype=torch.float32) if sigma is None else torch.as_tensor(sigma, dtype=torch.float32)
    bias = torch.zeros((n, 3), dtype=torch.float32) if bias is None else torch.as_tensor(bias, dtype=torch.float32)
    sigma, bias = sigma.to(dev).contiguous(), bias.to(dev).contiguous()
    if sigma.shape != (n, 3) or bias.shape != (n, 3):
        raise ValueError(f"{what}: sigma and bias are (n, 3)")
    params, mode = _stain_args(np.zeros((n, 14)) if params is None else params, mode_host, n, dev, what)
    return mode, sigma, bias, params


def blur_pool_rects(pool_u8: torch.Tensor, px_off: torch.Tensor, hw: torch.Tensor, image_of, rects, radius, weights,
                    scratch: torch.Tensor | None = None, scratch_off=None, mode=None, sigma=None, bias=None, simple_mode: bool = False,
                    params=None, check_status: bool = True):
    """``cpx_blur_pool_rects_u8``: request j is the rectangle ``rects[j]`` = (y0, x0, h, w) of ``scipy.ndimage.gaussian_filter`` (per
    channel, reflect about the image's borders, uint8 in and out) of image ``image_of[j]`` of the pool AFTER the colour stage of
    ``warp_affine_pool_stain`` (``mode`` / ``sigma`` / ``bias`` / ``params`` per request; default none), with ``radius[j]`` in 0 .. 8 and
    ``weights[j]`` (17,) float64 from ``augment.gauss_weights``.  The h * w * 3 bytes go to ``scratch`` (a uint8 device vector) from byte
    ``scratch_off[j]`` on; both default to a fresh buffer with the rectangles packed back to back.  Returns (scratch, scratch_off (k,)
    int64 on the host, status (1,) int32: bit 0 / 1 as ``warp_affine_pool``, bit 2 a bad rectangle, bit 3 a range outside the scratch;
    such a request touches nothing).  ``check_status`` raises ``ValueError`` on a non-zero status."""
    dev, nI, pool_px = _pool_table(pool_u8, px_off, hw, "blur_pool_rects")
    image_of = torch.as_tensor(image_of).to(device=dev, dtype=torch.int32).contiguous()
    k = image_of.numel()
    rects_host = np.ascontiguousarray(rects.cpu() if isinstance(rects, torch.Tensor) else rects, dtype=np.int64).reshape(-1, 4)
    radius_host = np.ascontiguousarray(radius.cpu() if isinstance(radius, torch.Tensor) else radius, dtype=np.int64).reshape(-1)
    weights_host = np.ascontiguousarray(weights.cpu() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64)
    if image_of.dim() != 1 or k == 0 or rects_host.shape != (k, 4) or radius_host.shape != (k,) or weights_host.shape != (k, 17):
        raise ValueError("blur_pool_rects: image_of (k,), rects (k, 4), radius (k,) and weights (k, 17) float64 expected")
    if radius_host.min() < 0 or radius_host.max() > BLUR_MAX_RADIUS:
        raise ValueError(f"blur_pool_rects: a radius outside 0 .. {BLUR_MAX_RADIUS} (sigma above 2)")
    if np.abs(rects_host).max() > np.iinfo(np.int32).max:
        raise ValueError("blur_pool_rects: rectangles are int32")
    nbytes = 3 * np.maximum(rects_host[:, 2], 0) * np.maximum(rects_host[:, 3], 0)
    if scratch_off is None:
        scratch_off = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
    scratch_off = np.ascontiguousarray(scratch_off, dtype=np.int64)
    if scratch_off.shape != (k,):
        raise ValueError("blur_pool_rects: scratch_off is (k,) int64")
    if scratch is None:
        scratch = torch.empty(int(max(1, (scratch_off + nbytes).max())), dtype=torch.uint8, device=dev)
    if scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.numel() == 0 or scratch.device != dev or not scratch.is_contiguous():
        raise ValueError("blur_pool_rects: scratch is a contiguous uint8 vector on the pool's device")
    max_h, max_w = int(max(1, rects_host[:, 2].max())), int(max(1, rects_host[:, 3].max()))
    mode, sigma, bias, params = _colour_args(mode, sigma, bias, params, k, dev, "blur_pool_rects")
    status = torch.empty(1, dtype=torch.int32, device=dev)
    rects_dev = torch.from_numpy(rects_host.astype(np.int32)).to(dev)
    radius_dev = torch.from_numpy(radius_host.astype(np.int32)).to(dev)
    weights_dev, off_dev = torch.from_numpy(weights_host).to(dev), torch.from_numpy(scratch_off).to(dev)
    check(_lib.lib().cpx_blur_pool_rects_u8(ptr(pool_u8), ptr(px_off), ptr(hw), nI, pool_px, ptr(image_of), ptr(rects_dev),
                                            ptr(radius_dev), ptr(weights_dev), ptr(off_dev), k, max_h, max_w, ptr(sigma), ptr(bias),
                                            int(bool(simple_mode)), ptr(params), ptr(_stain_table(dev, "density")), ptr(mode),
                                            ptr(scratch), scratch.numel(), ptr(status), _stream(dev)), "blur_pool_rects_u8")
    if check_status:
        _raise_status(status, "blur_pool_rects", _POOL_BITS + ((4, "a rectangle outside its image"), (8, "a range outside the scratch")))
    return scratch, scratch_off, status


def blur(img_u8: torch.Tensor, radius, weights) -> torch.Tensor:
    """``scipy.ndimage.gaussian_filter(plane, sigma)`` per channel on uint8 (n, H, W, 3) device images, image t with ``radius[t]`` and
    ``weights[t]`` (17,) float64 of ``augment.gauss_weights(sigma_t)`` (radius 0: a copy).  The images are viewed as a pool of
    equal-sized images and blurred whole by ``blur_pool_rects``."""
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[3] != 3 or not img_u8.is_cuda:
        raise ValueError("blur: expected uint8 (n, H, W, 3) on the device")
    img_u8 = img_u8.contiguous()
    n, H, W, _c = img_u8.shape
    dev = img_u8.device
    px_off = torch.arange(n, dtype=torch.int64, device=dev) * (H * W)
    hw = torch.tensor([[H, W]] * n, dtype=torch.int32, device=dev)
    out = torch.empty_like(img_u8)
    blur_pool_rects(img_u8.view(-1), px_off, hw, np.arange(n), np.tile([0, 0, H, W], (n, 1)), radius, weights, out.view(-1))
    return out


def warp_affine_pool_quality(pool_u8: torch.Tensor, pool_lab: torch.Tensor | None, px_off: torch.Tensor, hw: torch.Tensor, image_of,
                             inv, out_hw, mode=None, sigma=None, bias=None, simple_mode: bool = False, params=None, hbs=None,
                             hbs_apply=None, scratch: torch.Tensor | None = None, override_off=None, override_rect=None,
                             label_fill: int = 0, check_status: bool = True):
    """``cpx_warp_affine_pool_quality_u8``: ``warp_affine_pool_stain`` plus, per crop, the HBS jitter of ``ops.hbs`` on the in-image taps
    (``hbs`` (n, 4), ``hbs_apply`` (n,)) and an override source: where ``override_off[t] >= 0`` the in-image taps are read from
    ``scratch`` at that byte offset as the rectangle ``override_rect[t]`` = (y0, x0, h, w) of the crop's image (what ``blur_pool_rects``
    wrote) and the colour stage is skipped.  Status bit 4: a tap inside the image but outside the rectangle (it is 0 and nothing is
    read), bit 3: a range outside the scratch; bits 0 / 1 and the returns as ``warp_affine_pool``."""
    dev, nI, pool_px = _pool_table(pool_u8, px_off, hw, "warp_affine_pool_quality")
    image_of, inv, _vec, n = _crop_maps(image_of, inv, dev, "warp_affine_pool_quality")
    mode, sigma, bias, params = _colour_args(mode, sigma, bias, params, n, dev, "warp_affine_pool_quality")
    par, hbs_apply = _hbs_args(hbs, hbs_apply, n, dev, "warp_affine_pool_quality")
    if (override_off is None) != (override_rect is None):
        raise ValueError("warp_affine_pool_quality: override_off and override_rect go together")
    ov_off = np.full(n, -1, np.int64) if override_off is None else np.ascontiguousarray(override_off, dtype=np.int64)
    ov_rect = np.zeros((n, 4), np.int32) if override_rect is None else np.ascontiguousarray(override_rect, dtype=np.int32)
    if ov_off.shape != (n,) or ov_rect.shape != (n, 4):
        raise ValueError("warp_affine_pool_quality: override_off is (n,) int64 and override_rect (n, 4) int32")
    if scratch is None and (ov_off >= 0).any():
        raise ValueError("warp_affine_pool_quality: an override needs the scratch")
    if scratch is not None and (scratch.dtype != torch.uint8 or scratch.dim() != 1 or scratch.device != dev or not scratch.is_contiguous()):
        raise ValueError("warp_affine_pool_quality: scratch is a contiguous uint8 vector on the pool's device")
    dh, dw, out, lab_out, status = _pool_outputs(pool_lab, pool_px, n, out_hw, dev, "warp_affine_pool_quality")
    ov_off_dev, ov_rect_dev = torch.from_numpy(ov_off).to(dev), torch.from_numpy(ov_rect).to(dev)
    check(_lib.lib().cpx_warp_affine_pool_quality_u8(
        ptr(pool_u8), ptr(pool_lab), ptr(px_off), ptr(hw), nI, pool_px, ptr(image_of), ptr(inv), n, ptr(sigma), ptr(bias),
        int(bool(simple_mode)), ptr(params), ptr(_stain_table(dev, "density")), ptr(mode), ptr(par), ptr(hbs_apply), ptr(_unit_table(dev)),
        ptr(scratch), 0 if scratch is None else scratch.numel(), ptr(ov_off_dev), ptr(ov_rect_dev), dh, dw, int(label_fill), ptr(out), ptr(lab_out), ptr(status), _stream(dev)),
        "warp_affine_pool_quality_u8")
    if check_status:
        _raise_status(status, "warp_affine_pool_quality", _POOL_BITS + ((8, "a range outside the scratch"),
                                                                        (16, "a tap outside the crop's blurred rectangle")))
    return out, lab_out, status


def normalize_stats_f32(x: torch.Tensor) -> torch.Tensor:
    """(n, 3, 4) float32 {x01, x99 - x01, mode, x99} of float32 (n, 3, H, W) planes: np.percentile(plane, [1, 99]) exactly."""
    if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3 or not x.is_contiguous():
        raise ValueError("normalize_stats_f32: expected contiguous float32 (n, 3, H, W)")
    n, _c, H, W = x.shape
    stats = torch.empty((n, 3, 4), dtype=torch.float32, device=x.device)
    lo, hi = percentile_params(H * W, 1), percentile_params(H * W, 99)
    check(_lib.lib().cpx_normalize_stats_f32(ptr(x), n, H, W, lo[0], lo[1], hi[0], hi[1], ptr(stats), _stream(x.device)),
          "normalize_stats_f32")
    return stats


def normalize_img_f32(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """cellpose transforms.normalize_img on float32 NCHW (n, 3, H, W) crops, per crop and channel -> float32 (n, 3, H, W)."""
    x = x.contiguous()
    stats = normalize_stats_f32(x)
    out = torch.empty_like(x) if out is None else out
    check(_lib.lib().cpx_normalize_apply_f32(ptr(x), ptr(stats), x.shape[0], x.shape[2], x.shape[3], ptr(out), _stream(x.device)),
          "normalize_apply_f32")
    return out


# ---- t3: dataset statistics of (instance, class) maps (csrc/cpx_labelstats.hip) -----------------------------------
def label_stats(inst: torch.Tensor, cls: torch.Tensor, ncls: int, workspace: torch.Tensor | None = None, check_status: bool = True):
    """``cpx_label_stats`` on device maps: inst (n, H, W) int32 instance ids (any non-negative values), cls (n, H, W) int16 class
    maps.  Returns five device tensors ``(class_px (n, ncls) int64, inst_per_class (n, ncls) int32, n_masks (n,) int32,
    mid_area (n, 2) int32, status (n,) int32)``: pixels per class, ``np.unique(inst[cls == j]).size``, the number of ids that
    cellpose's ``diameters`` keeps (all but the smallest) and the two middle order statistics of their areas.  Raises
    ``ValueError`` naming the first image with a negative id or a class >= ``ncls``.  ``workspace``: a uint8 device tensor of at
    least ``cpx_label_stats_workspace_bytes`` to reuse between calls (allocated here when absent or too small)."""
    if inst.dtype != torch.int32 or cls.dtype != torch.int16 or inst.dim() != 3 or inst.shape != cls.shape:
        raise ValueError("label_stats: inst must be int32 (n, H, W) and cls int16 of the same shape")
    if not inst.is_cuda or inst.device != cls.device:
        raise ValueError("label_stats: both maps must be on one cuda device")
    inst, cls = inst.contiguous(), cls.contiguous()
    n, H, W = inst.shape
    dev = inst.device
    L = _lib.lib()
    nbytes = L.cpx_label_stats_workspace_bytes(n, H, W, int(ncls))
    if nbytes == 0:
        raise ValueError(f"label_stats: unsupported arguments n={n}, H={H}, W={W}, ncls={ncls} (1 <= ncls <= 64, n <= 65535)")
    if workspace is None or workspace.numel() < nbytes or workspace.device != dev or workspace.dtype != torch.uint8:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    class_px = torch.empty((n, ncls), dtype=torch.int64, device=dev)
    inst_per_class = torch.empty((n, ncls), dtype=torch.int32, device=dev)
    n_masks = torch.empty(n, dtype=torch.int32, device=dev)
    mid_area = torch.empty((n, 2), dtype=torch.int32, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    check(L.cpx_label_stats(ptr(inst), ptr(cls), n, H, W, int(ncls), ptr(class_px), ptr(inst_per_class), ptr(n_masks), ptr(mid_area),
                            ptr(status), ptr(workspace), workspace.numel(), _stream(dev)), "label_stats")
    if check_status:
        bad = torch.nonzero(status).flatten()
        if bad.numel():
            i = int(bad[0])
            bits = int(status[i])
            what = "a negative instance id" if bits & 1 else f"a class >= {ncls}"
            raise ValueError(f"label_stats: image {i} has {what}")
    return class_px, inst_per_class, n_masks, mid_area, status


# ---- r1: polygon rings -> instance-id maps (csrc/cpx_rasterize.hip) ------------------------------------------------
# the constants of csrc/cpx_rasterize.hip the tests probe both sides of (tests/test_rasterize_host.py pins them on the source)
RASTER_SMALL_MAX_VERTICES = 256      # RS_SMALL_VERTS: a ring of more vertices takes the large-ring path
RASTER_SMALL_MAX_AREA = 4096         # RS_SMALL_AREA: so does a ring whose clipped bounding box holds more pixels
RASTER_EDGE_CHUNK = 512              # RL_CHUNK: edges the large-ring path compacts per pass
RASTER_MAX_DIM = 32768               # RS_MAX_DIM: H, W limit


def _rs_array(x, np_dtype, torch_dtype, what: str):
    """a numpy array or a torch tensor of the one dtype the kernel reads; anything else raises (no silent casts of ids)"""
    if isinstance(x, torch.Tensor):
        if x.dtype != torch_dtype:
            raise ValueError(f"rasterize_polygons: {what} must be {torch_dtype}, not {x.dtype}")
        return x
    x = np.asarray(x)
    if x.dtype != np_dtype:
        raise ValueError(f"rasterize_polygons: {what} must be {np.dtype(np_dtype).name}, not {x.dtype}")
    return x


def rasterize_polygons(xy, ring_off, ring_value, shape, ring_image=None, n_images: int = 1, out: torch.Tensor | None = None,
                       device=None) -> torch.Tensor:
    """``cpx_rasterize_polygons``: rings -> int32 instance maps ``(n_images, H, W)`` on the device, by the rule of
    include/classpose_hip.h (pixel centre on the ring or odd crossing number; ``max`` with what the map holds).

    xy (n_vertices, 2) float64 in image-local pixels, ring_off (n_rings + 1,) int64 offsets into xy, ring_value (n_rings,) int32
    > 0, ring_image (n_rings,) int32 in ``0..n_images-1`` or None = image 0: numpy arrays (uploaded here) or tensors on the
    device.  ``out``: an int32 device map to paint onto (composes with its contents); else a zeroed one on ``device``.  Every
    argument is validated before the launch -- dtypes, offsets, values, image indices, finite coordinates -- and ``ValueError``
    is raised; the kernel never sees a bad offset or a NaN."""
    try:
        H, W = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError(f"rasterize_polygons: shape must be (H, W), not {shape!r}") from None
    n_images = int(n_images)
    if not (1 <= H <= RASTER_MAX_DIM and 1 <= W <= RASTER_MAX_DIM) or n_images < 1:
        raise ValueError(f"rasterize_polygons: need 1 <= H, W <= {RASTER_MAX_DIM} and n_images >= 1, not {(n_images, H, W)}")
    xy = _rs_array(xy, np.float64, torch.float64, "xy")
    ring_off = _rs_array(ring_off, np.int64, torch.int64, "ring_off")
    ring_value = _rs_array(ring_value, np.int32, torch.int32, "ring_value")
    if ring_image is not None:
        ring_image = _rs_array(ring_image, np.int32, torch.int32, "ring_image")
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError(f"rasterize_polygons: xy must be (n_vertices, 2), not {tuple(xy.shape)}")
    if ring_off.ndim != 1 or ring_off.shape[0] < 1 or ring_value.ndim != 1 or ring_value.shape[0] != ring_off.shape[0] - 1:
        raise ValueError("rasterize_polygons: ring_off must hold n_rings + 1 offsets for the n_rings entries of ring_value")
    n_rings, n_vertices = int(ring_value.shape[0]), int(xy.shape[0])
    if ring_image is not None and tuple(ring_image.shape) != (n_rings,):
        raise ValueError("rasterize_polygons: ring_image must hold one image index per ring")
    if int(ring_off[0]) < 0 or int(ring_off[-1]) > n_vertices or not bool((ring_off[1:] >= ring_off[:-1]).all()):
        raise ValueError(f"rasterize_polygons: ring_off must be non-decreasing within 0..{n_vertices}")
    if n_rings and not bool((ring_value > 0).all()):
        raise ValueError("rasterize_polygons: every ring_value must be > 0")
    if ring_image is not None and n_rings and not bool(((ring_image >= 0) & (ring_image < n_images)).all()):
        raise ValueError(f"rasterize_polygons: ring_image must lie in 0..{n_images - 1}")
    finite = torch.isfinite(xy).all() if isinstance(xy, torch.Tensor) else np.isfinite(xy).all()
    if not bool(finite):
        raise ValueError("rasterize_polygons: xy holds a NaN or an infinity")
    given = [t for t in (xy, ring_off, ring_value, ring_image, out) if isinstance(t, torch.Tensor)]
    if out is not None:
        if out.dtype != torch.int32 or tuple(out.shape) != (n_images, H, W) or not out.is_contiguous():
            raise ValueError(f"rasterize_polygons: out must be a contiguous int32 tensor of shape {(n_images, H, W)}")
    dev = given[0].device if given else torch.device("cuda" if device is None else device)
    if dev.type != "cuda" or any(t.device != dev for t in given):
        raise ValueError("rasterize_polygons: tensors must be on one cuda device")
    if out is None:
        out = torch.zeros((n_images, H, W), dtype=torch.int32, device=dev)
    if n_rings == 0:
        return out
    up = lambda t: None if t is None else (t.contiguous() if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)).to(dev))
    xy, ring_off, ring_value, ring_image = up(xy), up(ring_off), up(ring_value), up(ring_image)
    L = _lib.lib()
    nbytes = L.cpx_rasterize_workspace_bytes(n_rings, n_vertices, n_images, H, W)
    if nbytes == 0:
        raise ValueError(f"rasterize_polygons: unsupported arguments n_rings={n_rings}, n_images={n_images}, H={H}, W={W}")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.cpx_rasterize_polygons(ptr(xy), ptr(ring_off), ptr(ring_value), ptr(ring_image), n_rings, n_images, H, W, ptr(out),
                                   ptr(ws), nbytes, _stream(dev)), "rasterize_polygons")
    return out


def ids_to_classes(inst: torch.Tensor, class_of) -> torch.Tensor:
    """``cpx_ids_to_classes``: uint8 ``class_of[inst]`` of an int32 device map; class_of (n_ids + 1,) uint8, numpy or on the
    device, entry 0 = the background's class.  An id outside ``0..n_ids`` raises ``ValueError``."""
    if not isinstance(inst, torch.Tensor) or inst.dtype != torch.int32:
        raise ValueError("ids_to_classes: inst must be an int32 tensor")
    if not isinstance(class_of, torch.Tensor):
        class_of = np.asarray(class_of)
        if class_of.dtype != np.uint8:
            raise ValueError(f"ids_to_classes: class_of must be uint8, not {class_of.dtype}")
        class_of = torch.from_numpy(np.ascontiguousarray(class_of))
    if class_of.dtype != torch.uint8 or class_of.dim() != 1 or class_of.numel() < 1:
        raise ValueError("ids_to_classes: class_of must be a uint8 vector with an entry for id 0")
    if not inst.is_cuda:
        raise ValueError("ids_to_classes: inst must be on a cuda device")
    inst = inst.contiguous()
    dev = inst.device
    class_of = class_of.to(dev).contiguous()
    n_ids = class_of.numel() - 1
    cls = torch.empty(inst.shape, dtype=torch.uint8, device=dev)
    if inst.numel() == 0:
        return cls
    lo, hi = int(inst.min()), int(inst.max())
    if lo < 0 or hi > n_ids:
        raise ValueError(f"ids_to_classes: ids span {lo}..{hi} but class_of covers 0..{n_ids}")
    check(_lib.lib().cpx_ids_to_classes(ptr(inst), inst.numel(), ptr(class_of), n_ids, ptr(cls), _stream(dev)), "ids_to_classes")
    return cls


# ---- r2: value maps -> instance maps by connected components (csrc/cpx_components.hip) ------------------------------
COMPONENTS_TILE = 64                 # CC_TILE: the tile side the device tests probe both sides of (pinned on the source)
COMPONENTS_MAX_PIXELS = 1 << 28      # CC_MAX_PX: H * W limit


def label_components(maps: torch.Tensor, connectivity: int = 8, workspace: torch.Tensor | None = None):
    """``cpx_label_components`` on device maps: maps (n, H, W) int32, 0 = background, every other value (negatives included) is
    foreground; neighbouring pixels of equal value are connected, by edges (``connectivity=4``) or edges and corners (8).
    Returns two device tensors ``(labels (n, H, W) int32, n_components (n,) int32)``: per image, 0 on background and the
    component's 1-based rank by the raster index of its first pixel -- the numbering of ``skimage.measure.label`` and
    ``scipy.ndimage.label``.  ``workspace``: a uint8 device tensor of at least ``cpx_label_components_workspace_bytes`` to reuse
    between calls (allocated here when absent or too small)."""
    if not isinstance(maps, torch.Tensor) or maps.dtype != torch.int32 or maps.dim() != 3:
        raise ValueError("label_components: maps must be an int32 (n, H, W) tensor")
    if connectivity not in (4, 8):
        raise ValueError(f"label_components: connectivity must be 4 or 8, not {connectivity!r}")
    if not maps.is_cuda:
        raise ValueError("label_components: maps must be on a cuda device")
    maps = maps.contiguous()
    n, H, W = maps.shape
    dev = maps.device
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    n_components = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return labels, n_components
    L = _lib.lib()
    nbytes = L.cpx_label_components_workspace_bytes(n, H, W)
    if nbytes == 0:
        raise ValueError(f"label_components: unsupported arguments n={n}, H={H}, W={W} (n <= 65535, H, W >= 1, H * W <= 2^28)")
    if workspace is None or workspace.numel() < nbytes or workspace.device != dev or workspace.dtype != torch.uint8:
        workspace = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    check(L.cpx_label_components(ptr(maps), n, H, W, int(connectivity), ptr(labels), ptr(n_components), ptr(workspace),
                                 workspace.numel(), _stream(dev)), "label_components")
    return labels, n_components


# ---- r3: touching cells of one class -> separate instances by distance peaks (csrc/cpx_split.hip) --------------------
SPLIT_MAX_DIAG2 = 1 << 30            # SP_MAX_DIAG2: H * H + W * W limit, so that squared distances and their sums are int32
SPLIT_MAX_MIN_DISTANCE = 64          # SP_MAX_WINDOW
SPLIT_MAX_MIN_RADIUS = 32768         # SP_MAX_RADIUS


def _split_maps(inst, what: str) -> torch.Tensor:
    if not isinstance(inst, torch.Tensor) or inst.dtype != torch.int32 or inst.dim() != 3:
        raise ValueError(f"{what}: inst must be an int32 (n, H, W) tensor")
    if not inst.is_cuda:
        raise ValueError(f"{what}: inst must be on a cuda device")
    n, H, W = inst.shape
    if n and not (n <= 65535 and H >= 1 and W >= 1 and H * W <= COMPONENTS_MAX_PIXELS and H * H + W * W <= SPLIT_MAX_DIAG2):
        raise ValueError(f"{what}: unsupported arguments n={n}, H={H}, W={W} (n <= 65535, H, W >= 1, H * W <= 2^28, "
                         "H * H + W * W <= 2^30)")
    return inst.contiguous()


def distance_sq(inst: torch.Tensor) -> torch.Tensor:
    """``cpx_distance_sq`` on device maps: inst (n, H, W) int32 -> (n, H, W) int32, per pixel of value v != 0 the exact squared
    Euclidean distance to the nearest pixel of its image with another value (0 included), ``H * H + W * W`` where the image holds
    no other value, 0 on pixels of value 0.  The image border is not a site."""
    inst = _split_maps(inst, "distance_sq")
    n, H, W = inst.shape
    d2 = torch.empty((n, H, W), dtype=torch.int32, device=inst.device)
    if n == 0:
        return d2
    ws = torch.empty((n, H, W), dtype=torch.int32, device=inst.device)
    check(_lib.lib().cpx_distance_sq(ptr(inst), n, H, W, ptr(d2), ptr(ws), ws.numel() * 4, _stream(inst.device)), "distance_sq")
    return d2


def split_touching(inst: torch.Tensor, min_distance: int = 5, min_radius: int = 2, connectivity: int = 8,
                   seed_cap: int | None = None, return_seeds: bool = False):
    """``cpx_split_touching`` on device instance maps: inst (n, H, W) int32, 0 = background, ids 1 .. H * W as
    ``label_components`` writes them.  The peaks of the squared distance map (``distance_sq``) that are at least ``min_radius``
    from the instance's edge and that no pixel of the same instance within ``min_distance`` (Chebyshev) beats are seeds; an
    instance with two or more seeds is cut into its seeds' Euclidean Voronoi cells; ``label_components`` with ``connectivity``
    numbers the result.  Returns two device tensors ``(labels (n, H, W) int32, counts (n,) int32)``; with ``return_seeds`` also a
    list of n int32 device tensors, the raster indices of each image's seeds by (instance id, raster index).  The seed lists
    start at ``seed_cap`` entries per image (default: max(1024, H * W / 16)); when an image has more, the call is repeated once
    with the largest count it reported.  The input is not modified."""
    inst = _split_maps(inst, "split_touching")
    if connectivity not in (4, 8):
        raise ValueError(f"split_touching: connectivity must be 4 or 8, not {connectivity!r}")
    if not 1 <= int(min_distance) <= SPLIT_MAX_MIN_DISTANCE:
        raise ValueError(f"split_touching: min_distance must be in 1..{SPLIT_MAX_MIN_DISTANCE}, not {min_distance!r}")
    if not 1 <= int(min_radius) <= SPLIT_MAX_MIN_RADIUS:
        raise ValueError(f"split_touching: min_radius must be in 1..{SPLIT_MAX_MIN_RADIUS}, not {min_radius!r}")
    n, H, W = inst.shape
    dev = inst.device
    labels = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    counts = torch.empty(n, dtype=torch.int32, device=dev)
    if n == 0:
        return (labels, counts, []) if return_seeds else (labels, counts)
    L = _lib.lib()
    cap = min(H * W, max(1024, H * W // 16) if seed_cap is None else max(1, int(seed_cap)))
    while True:
        ws = torch.empty(L.cpx_split_workspace_bytes(n, H, W, cap), dtype=torch.uint8, device=dev)
        seeds = torch.empty((n, cap), dtype=torch.int32, device=dev)
        n_seeds = torch.empty(n, dtype=torch.int32, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)
        check(L.cpx_split_touching(ptr(inst), n, H, W, int(min_distance), int(min_radius), int(connectivity), cap, ptr(labels),
                                   ptr(counts), ptr(seeds), ptr(n_seeds), ptr(status), ptr(ws), ws.numel(), _stream(dev)),
              "split_touching")
        st, ns = status.cpu().numpy(), n_seeds.cpu().numpy()
        if (st & 2).any():
            raise ValueError(f"split_touching: image {int(np.flatnonzero(st & 2)[0])} has an instance id outside 0..{H * W}")
        if not st.any():
            break
        if int(ns.max()) <= cap:
            raise RuntimeError(f"split_touching: status {st.tolist()} with {int(ns.max())} seeds in lists of {cap}")
        cap = int(ns.max())                                             # <= H * W: one seed per pixel at the most
    if return_seeds:
        return labels, counts, [seeds[k, :int(ns[k])] for k in range(n)]
    return labels, counts
