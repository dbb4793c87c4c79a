"""CPU restatement (test infrastructure) of the two resizes ``ClassposeModel.eval(diameter=)`` applies to its outputs:

* ``resize_linear_f32``  ``cv2.resize(..., interpolation=cv2.INTER_LINEAR)`` on float32 planes, what cellpose's
  ``transforms.resize_image`` runs image by image on dP / cellprob / y_class
  (/root/reference/src/classpose/models.py:733-748, 782-792);
* ``resize_nearest``     ``cv2.INTER_NEAREST`` on the id and class maps (models.py:804-820);
* ``resize_image`` / ``resize_gradients`` / ``resize_cellprob``  the cellpose helpers themselves
  (``transforms.resize_image``, ``CellposeModel._resize_gradients`` / ``_resize_cellprob``), restated from cellpose 4.0.x:
  channels last, ``resize_image``, channels first again.

Neither OpenCV nor cellpose is present here, so all of it is PARITY UNPINNED: the coordinate rule is the one
``oracle.tiling.resize_linear_u8`` restates from OpenCV's resize.cpp, with float32 weights in place of the 11-bit fixed
point; every product and every sum is rounded to float32 and nothing is fused (whether a given OpenCV build contracts
``S0 * a0 + S1 * a1`` into an FMA cannot be known here).  The uint8 image resize stays ``oracle.tiling.resize_linear_u8``.

Not imported by anything under ``classpose_amd/``.
"""
from __future__ import annotations

import numpy as np

INTER_NEAREST, INTER_LINEAR = 0, 1          # cv2's constants


def linear_taps(dlen: int, slen: int, clamp_weight: bool):
    """(s0, s1, f): the two clipped source indices and the float32 weight of the second, per destination index"""
    scale = 1.0 / (np.float64(dlen) / np.float64(slen))
    f = ((np.arange(dlen, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = f - s.astype(np.float32)
    if clamp_weight:
        lo = s < 0
        f[lo], s[lo] = 0, 0
        hi = s >= slen - 1
        f[hi], s[hi] = 0, slen - 1
    return np.clip(s, 0, slen - 1), np.clip(s + 1, 0, slen - 1), f.astype(np.float32)


def resize_linear_f32(src: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """float32 [..., sh, sw] -> [..., dh, dw], every plane on its own"""
    src = np.asarray(src)
    assert src.dtype == np.float32
    sh, sw = src.shape[-2:]
    if (sh, sw) == (dh, dw):
        return src.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        if sh == 2 * dh and sw == 2 * dw:
            a, b = src[..., 0::2, 0::2], src[..., 0::2, 1::2]
            c, d = src[..., 1::2, 0::2], src[..., 1::2, 1::2]
            return (((a + b) + (c + d)) * np.float32(0.25)).astype(np.float32)
        x0, x1, fx = linear_taps(dw, sw, True)
        y0, y1, fy = linear_taps(dh, sh, False)
        gx, gy = np.float32(1) - fx, np.float32(1) - fy
        h = src[..., :, x0] * gx + src[..., :, x1] * fx                       # [..., sh, dw]
        out = h[..., y0, :] * gy[:, None] + h[..., y1, :] * fy[:, None]
    assert out.dtype == np.float32
    return out


def resize_nearest(src: np.ndarray, dh: int, dw: int) -> np.ndarray:
    """any dtype [..., sh, sw] -> [..., dh, dw]"""
    src = np.asarray(src)
    sh, sw = src.shape[-2:]
    if (sh, sw) == (dh, dw):
        return src.copy()
    sx = np.minimum(np.floor(np.arange(dw) * (1.0 / (np.float64(dw) / sw))).astype(np.int64), sw - 1)
    sy = np.minimum(np.floor(np.arange(dh) * (1.0 / (np.float64(dh) / sh))).astype(np.int64), sh - 1)
    return src[..., sy[:, None], sx[None, :]]


def _resize_2d(img: np.ndarray, Ly: int, Lx: int, interpolation: int) -> np.ndarray:
    """cv2.resize(img, (Lx, Ly), interpolation=...) of one [h, w] or [h, w, c] image"""
    if interpolation == INTER_NEAREST:
        planes = img if img.ndim == 2 else np.moveaxis(img, -1, 0)
        out = resize_nearest(planes, Ly, Lx)
    elif img.dtype == np.uint8:
        from oracle.tiling import resize_linear_u8
        assert img.ndim == 3 and img.shape[-1] == 3
        return resize_linear_u8(img, Lx, Ly)
    else:
        planes = np.ascontiguousarray(img if img.ndim == 2 else np.moveaxis(img, -1, 0), dtype=np.float32)
        out = resize_linear_f32(planes, Ly, Lx)
    return out if img.ndim == 2 else np.ascontiguousarray(np.moveaxis(out, 0, -1))


def resize_image(img0: np.ndarray, Ly: int | None = None, Lx: int | None = None, rsz=None, interpolation=INTER_LINEAR,
                 no_channels: bool = False) -> np.ndarray:
    """cellpose.transforms.resize_image: [Ly0, Lx0], [Ly0, Lx0, c], [n, Ly0, Lx0] (no_channels) or [n, Ly0, Lx0, c];
    stacks go image by image through cv2.resize (so a uint8 image takes OpenCV's 8-bit path) into a float32 array; a
    single image keeps the type cv2.resize returns."""
    if Ly is None and rsz is None:
        raise ValueError("must give size to resize to or factor to use for resizing")
    if Ly is None:
        rsz = [rsz, rsz] if not isinstance(rsz, (list, np.ndarray)) else rsz
        k = 0 if (img0.ndim == 2 or (img0.ndim == 3 and not no_channels)) else 1
        Ly, Lx = int(img0.shape[k] * rsz[-2]), int(img0.shape[k + 1] * rsz[-1])
    if (img0.ndim > 2 and no_channels) or (img0.ndim == 4 and not no_channels):
        shape = (img0.shape[0], Ly, Lx) if no_channels else (img0.shape[0], Ly, Lx, img0.shape[-1])
        imgs = np.zeros(shape, np.float32)
        for i, img in enumerate(img0):
            imgs[i] = _resize_2d(img, Ly, Lx, interpolation)
        return imgs
    return _resize_2d(img0, Ly, Lx, interpolation)


def resize_cellprob(prob: np.ndarray, to_y_size: int, to_x_size: int, to_z_size=None) -> np.ndarray:
    """CellposeModel._resize_cellprob, 2-D case: [Ly, Lx] float32"""
    assert prob.ndim == 2
    return resize_image(prob, Ly=to_y_size, Lx=to_x_size, no_channels=True)


def resize_gradients(grads: np.ndarray, to_y_size: int, to_x_size: int, to_z_size=None) -> np.ndarray:
    """CellposeModel._resize_gradients, 2-D case: [c, Ly, Lx] -> channels last, resize_image, channels first"""
    assert grads.ndim == 3
    return resize_image(grads.transpose(1, 2, 0), Ly=to_y_size, Lx=to_x_size, no_channels=False).transpose(2, 0, 1)
