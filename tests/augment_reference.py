"""numpy restatements of the three augmentation stages of csrc/cpx_augment.hip, written from their contract
(include/classpose_hip.h, section t2), in float64 and in float32.  The float64 versions are the yardstick; the float32 versions
bound what float32 arithmetic can deliver (the relative-L2 rule of the project: err(device) <= 4 * err(float32 restatement)).
Test helpers only: nothing here is on a product path."""
from __future__ import annotations

import numpy as np

RGB_FROM_HED = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]]).astype(np.float32)


# ---- stain jitter ---------------------------------------------------------------------------------------------
def hed_applied(img_u8: np.ndarray, cutoff) -> bool:
    mean = (float(img_u8.astype(np.int64).sum()) / img_u8.size) / 255.0
    return bool(cutoff[0] <= mean <= cutoff[1])


def hed_jitter_float(img_u8: np.ndarray, sigma, bias, hed_from_rgb, simple_mode: bool, dtype=np.float64) -> np.ndarray:
    """x in [0, 1] BEFORE the ``* 255`` and the truncation, of one (H, W, 3) uint8 patch that is inside the cut-off; every step in
    ``dtype``.  The matrices are the float32 ones, widened."""
    f = dtype
    M1, M2 = hed_from_rgb.astype(f), RGB_FROM_HED.astype(f)
    rgb = (img_u8 / 255.0).astype(np.float32).astype(f)
    if simple_mode:
        rgb = np.clip(rgb, f(np.float32(1e-6)), f(1))
    else:
        rgb = rgb + f(1)
    l = -np.log(rgb)
    h = l[..., 0:1] * M1[0] + l[..., 1:2] * M1[1] + l[..., 2:3] * M1[2]
    h = h * (f(1) + np.asarray(sigma, np.float32).astype(f)) + np.asarray(bias, np.float32).astype(f)
    h = -h
    x = np.exp(h[..., 0:1] * M2[0] + h[..., 1:2] * M2[1] + h[..., 2:3] * M2[2])
    if not simple_mode:
        x = np.clip(x - f(1), f(-1), f(1))
        x = (x - f(-1)) / f(2) * f(2) + f(-1)
    return np.clip(x, f(0), f(1))


def hed_jitter(img_u8, sigma, bias, hed_from_rgb, cutoff, simple_mode, dtype=np.float64):
    """(uint8 result, applied, 255 * x of the float restatement or None)"""
    if not hed_applied(img_u8, cutoff):
        return img_u8.copy(), False, None
    x = hed_jitter_float(img_u8, sigma, bias, hed_from_rgb, simple_mode, dtype)
    v = x * dtype(255)
    return v.astype(np.uint8), True, v


def check_hed_against(dev_u8: np.ndarray, ref_u8: np.ndarray, v64: np.ndarray, window: float = 1e-3) -> dict:
    """The acceptance rule of the stain jitter: ``dev`` may differ from ``ref`` by one level only where the float64 restatement's
    255 * x lies within ``window`` of an integer; no difference above 1.  Returns the counts; raises AssertionError."""
    d = dev_u8.astype(np.int32) - ref_u8.astype(np.int32)
    near = np.abs(v64 - np.rint(v64)) <= window
    assert np.abs(d).max() <= 1, f"largest difference {np.abs(d).max()} levels"
    bad = (d != 0) & ~near
    assert not bad.any(), f"{int(bad.sum())} pixels differ outside the {window} window"
    return dict(differ=int((d != 0).sum()), near=int(near.sum()))


# ---- warp -----------------------------------------------------------------------------------------------------
def source_coords(inv6: np.ndarray, dh: int, dw: int):
    """float64 (sx, sy), each (dh, dw): m0 * x + m1 * y + m2 evaluated left to right."""
    ys, xs = np.meshgrid(np.arange(dh, dtype=np.float64), np.arange(dw, dtype=np.float64), indexing="ij")
    m = np.asarray(inv6, np.float64)
    return m[0] * xs + m[1] * ys + m[2], m[3] * xs + m[4] * ys + m[5]


def warp_image(src_chw: np.ndarray, inv6, dh: int, dw: int, dtype=np.float64) -> np.ndarray:
    """Bilinear, constant border 0: src (3, sh, sw) of any real dtype -> (3, dh, dw) in ``dtype``.  In float32 the weight is
    float32(sx - floor(sx)) and each lerp is a + (b - a) * w."""
    f = dtype
    _c, sh, sw = src_chw.shape
    sx, sy = source_coords(inv6, dh, dw)
    fx, fy = np.floor(sx), np.floor(sy)
    wx, wy = (sx - fx).astype(f), (sy - fy).astype(f)
    ok = (sx >= -1) & (sx < sw) & (sy >= -1) & (sy < sh)
    x0 = np.where(ok, fx, -5).astype(np.int64)
    y0 = np.where(ok, fy, -5).astype(np.int64)
    pad = np.zeros((3, sh + 2, sw + 2), f)
    pad[:, 1:-1, 1:-1] = src_chw.astype(f)

    def tap(y, x):
        inside = (y >= -1) & (y <= sh) & (x >= -1) & (x <= sw)
        v = pad[:, np.clip(y + 1, 0, sh + 1), np.clip(x + 1, 0, sw + 1)]
        return np.where(inside, v, f(0))
    a, b, d, e = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = a + (b - a) * wx
    bot = d + (e - d) * wx
    return (top + (bot - top) * wy).astype(f)


def warp_labels(lab: np.ndarray, inv6, dh: int, dw: int, fill: int) -> np.ndarray:
    sh, sw = lab.shape
    sx, sy = source_coords(inv6, dh, dw)
    nx, ny = np.floor(sx + 0.5), np.floor(sy + 0.5)
    ok = (nx >= 0) & (nx < sw) & (ny >= 0) & (ny < sh)
    out = np.full((dh, dw), fill, np.int16)
    out[ok] = lab[ny[ok].astype(np.int64), nx[ok].astype(np.int64)]
    return out


def half_integer_distance(inv6, dh: int, dw: int) -> float:
    """Smallest distance of a sampled source coordinate to a half-integer (where nearest-neighbour sampling would flip)."""
    sx, sy = source_coords(inv6, dh, dw)
    return float(min(np.abs((sx + 0.5) - np.rint(sx + 0.5)).min(), np.abs((sy + 0.5) - np.rint(sy + 0.5)).min()))


# ---- float32 percentile normalisation -------------------------------------------------------------------------
def normalize_plane_f32(plane: np.ndarray):
    """(stats [x01, x99 - x01, mode, x99] float32, normalised plane float32) of one float32 plane: cellpose normalize_img ->
    normalize99 per plane, numpy float32 arithmetic.  The two percentiles are taken as cellpose's normalize99 (and oracle/tiling.py)
    takes them, one scalar call each: numpy then keeps the quantile arithmetic in float32, where a list ``[1, 99]`` would promote it
    to float64 and change x99 in the last bits."""
    p = np.ascontiguousarray(plane, np.float32)
    x01, x99 = np.percentile(p, 1), np.percentile(p, 99)
    assert x01.dtype == np.float32 and x99.dtype == np.float32
    den = np.float32(x99 - x01)
    if np.ptp(p) == 0:
        mode, out = 0, p.copy()
    elif den > np.float32(1e-3):
        mode, out = 1, (p - x01) / den
    else:
        mode, out = 2, np.zeros_like(p)
    return np.array([x01, den, mode, x99], np.float32), out.astype(np.float32)


def normalize_f32(x_nchw: np.ndarray):
    n, c = x_nchw.shape[:2]
    stats = np.zeros((n, c, 4), np.float32)
    out = np.empty_like(x_nchw, dtype=np.float32)
    for i in range(n):
        for k in range(c):
            stats[i, k], out[i, k] = normalize_plane_f32(x_nchw[i, k])
    return stats, out
