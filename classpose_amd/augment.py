"""Training-time augmentation of class-head crops on the device.

The reference's loader (dataset.py:23-56) applies a stain jitter in the HED colour space, then cellpose's
``random_rotate_and_resize`` (flip, rotation, scale, crop), and normalises AFTER both.  Here the host only draws the random
parameters; the pixels stay on the device: ``ops.hed_jitter`` -> ``ops.warp_affine`` -> ``ops.normalize_img_f32`` ->
``ops.patchify_f32`` (csrc/cpx_augment.hip, csrc/cpx_train.hip).

Random draws come from the numpy ``Generator`` passed in, in the order documented on each sampler.  The reference draws from the
global ``np.random`` state, so its sample stream is not reproduced; its distributions are.

Still different from the reference: the warp samples at exact double-precision source coordinates (OpenCV quantises them to
1 / 32 pixel) and the ``enhanced`` pipeline is not built.  The rescale by cell diameter (dataset.py:35-45) is the ``rescale``
argument of the samplers: per crop ``diameter / diam_mean``, the diameters from ``dataset_stats.label_stats``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops

# float32 stain matrices of transforms/hed.py:11-14: RGB_FROM_HED as written there, HED_FROM_RGB = float32(scipy.linalg.inv(RGB_FROM_HED))
# (the nine values of tests/golden/reference_augment.npz; the kernel carries the same literals)
RGB_FROM_HED = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11], [0.27, 0.57, 0.78]], dtype=np.float32)
HED_FROM_RGB = np.array([[1.87798285, -1.00767875, -0.556115806],
                         [-0.0659080595, 1.13473034, -0.135521799],
                         [-0.601907432, -0.480414152, 1.57358813]], dtype=np.float32)

_HED_VALUE = 0.25
# augmentation_configs.py:10-25.  These values are part of the user-facing contract.
AUGMENT_CONFIGS = {
    "hed_only": {
        "sigma_ranges": [(-_HED_VALUE, _HED_VALUE)] * 3,
        "bias_ranges": [(-_HED_VALUE, _HED_VALUE)] * 3,
        "cutoff_range": (0.15, 0.85),
        "simple_mode": False,
    },
}
MAX_RESAMPLE = 8


def get_config(name: str | None) -> dict | None:
    """The stain-jitter settings of a named configuration; ``None`` and ``"geometry"`` mean no colour augmentation."""
    if name is None or name == "geometry":
        return None
    if name == "enhanced":
        raise NotImplementedError("the 'enhanced' augmentation is not built: it needs the H&E stain-matrix perturbation, Gaussian "
                                  "blur, additive noise and the hue / brightness / saturation jitter")
    if name not in AUGMENT_CONFIGS:
        raise ValueError(f"unknown augmentation {name!r}: one of {sorted(AUGMENT_CONFIGS) + ['geometry']}")
    return AUGMENT_CONFIGS[name]


def affine_inverse(flip, theta, scale, dxy, sh: int, sw: int, out: int = 256) -> np.ndarray:
    """(n, 6) float64 inverse maps, source (sx, sy) = inv . (x, y, 1), of cellpose's forward map
    ``dst = scale * R(theta) * (src - cc) + cc1`` with ``R = [[cos, -sin], [sin, cos]]``, ``cc = (sw / 2, sh / 2)`` and
    ``cc1 = cc - ([sw, sh] - out) / 2 + dxy``.  Where ``flip`` is set the horizontal flip of the source, ``sx -> sw - 1 - sx``,
    is folded into the map."""
    flip, theta, scale = np.asarray(flip, bool), np.asarray(theta, np.float64), np.asarray(scale, np.float64)
    dxy = np.asarray(dxy, np.float64).reshape(-1, 2)
    cc = np.array([sw / 2, sh / 2], np.float64)
    cc1 = cc - (np.array([sw, sh], np.float64) - out) / 2 + dxy                     # (n, 2)
    c, s = np.cos(theta) / scale, np.sin(theta) / scale
    inv = np.empty((len(theta), 6), np.float64)
    inv[:, 0], inv[:, 1] = c, s                                                     # (1 / scale) R^T
    inv[:, 3], inv[:, 4] = -s, c
    inv[:, 2] = cc[0] - (c * cc1[:, 0] + s * cc1[:, 1])
    inv[:, 5] = cc[1] - (-s * cc1[:, 0] + c * cc1[:, 1])
    inv[flip, 0:2] = -inv[flip, 0:2]
    inv[flip, 2] = (sw - 1) - inv[flip, 2]
    return inv


def affine_forward(theta, scale, dxy, sh: int, sw: int, out: int = 256) -> np.ndarray:
    """(n, 6) float64 forward maps ``dst = fwd . (sx, sy, 1)`` of the same parametrisation, without the flip."""
    theta, scale = np.asarray(theta, np.float64), np.asarray(scale, np.float64)
    dxy = np.asarray(dxy, np.float64).reshape(-1, 2)
    cc = np.array([sw / 2, sh / 2], np.float64)
    cc1 = cc - (np.array([sw, sh], np.float64) - out) / 2 + dxy
    c, s = np.cos(theta) * scale, np.sin(theta) * scale
    fwd = np.empty((len(theta), 6), np.float64)
    fwd[:, 0], fwd[:, 1] = c, -s
    fwd[:, 3], fwd[:, 4] = s, c
    fwd[:, 2] = cc1[:, 0] - (c * cc[0] - s * cc[1])
    fwd[:, 5] = cc1[:, 1] - (s * cc[0] + c * cc[1])
    return fwd


def _check_rescale(rescale, n: int) -> np.ndarray | None:
    if rescale is None:
        return None
    rescale = np.asarray(rescale, np.float64)
    if rescale.shape != (n,) or not np.all(rescale > 0):
        raise ValueError(f"rescale: {n} positive factors (diameter / diam_mean per crop) expected")
    return rescale


def sample_affine_params(rng: np.random.Generator, n: int, sh: int, sw: int, out: int = 256, scale_range: float = 0.5,
                         do_flip: bool = True, rotate: bool = True, rescale=None) -> dict:
    """The random parameters behind ``sample_affine``: ``flip`` (n,) bool, ``theta``, ``scale`` (n,), ``dxy`` (n, 2).
    Draw order, always all four so that the stream does not depend on the switches: ``rng.random(n)`` for the flips, ``rng.random(n)``
    for theta, ``rng.random(n)`` for the scale, ``rng.random((n, 2))`` for the shift (x, y).  ``rescale`` (n,) float64, the per-crop
    ``diameter / diam_mean`` (dataset.py:35-38), divides the scale; the crop room behind ``dxy`` follows from the divided scale.
    It changes neither the number nor the order of the draws, and ``rescale=None`` is bitwise the sampler without it."""
    r = float(np.clip(scale_range, 0.0, 2.0))
    rescale = _check_rescale(rescale, n)
    u_flip, u_theta, u_scale, u_dxy = rng.random(n), rng.random(n), rng.random(n), rng.random((n, 2))
    flip = (u_flip > 0.5) & bool(do_flip)
    theta = 2 * np.pi * u_theta if rotate else np.zeros(n)
    scale = (1 - r / 2) + r * u_scale
    if rescale is not None:
        scale = scale / rescale
    room = np.maximum(0.0, np.stack([sw * scale - out, sh * scale - out], 1))
    return dict(flip=flip, theta=theta, scale=scale, dxy=(u_dxy - 0.5) * room)


def sample_affine(rng: np.random.Generator, n: int, sh: int, sw: int, out: int = 256, scale_range: float = 0.5,
                  do_flip: bool = True, rotate: bool = True, rescale=None):
    """(flips (n,) bool, inverse maps (n, 6) float64) of ``n`` random flip / rotation / scale / crop transforms from a
    ``sh`` x ``sw`` source into ``out`` x ``out``, in the parametrisation of cellpose's ``random_rotate_and_resize``.

    Restated from cellpose 4.0.x, whose wheel is not available to pin against (unpinned): ``flip = u > 0.5``, ``theta = 2 pi u``,
    ``scale = (1 - r / 2) + r u`` with ``r = clamp(scale_range, 0, 2)``, ``dxy = (u2 - 0.5) * max(0, [sw * scale - out,
    sh * scale - out])``; with ``rescale`` the scale is ``((1 - r / 2) + r u) / rescale`` before ``dxy`` is formed from it, also
    restated from cellpose and unpinned for the same reason.  See ``affine_inverse`` for the map and ``sample_affine_params`` for
    the order of the draws."""
    p = sample_affine_params(rng, n, sh, sw, out, scale_range, do_flip, rotate, rescale)
    return p["flip"], affine_inverse(p["flip"], p["theta"], p["scale"], p["dxy"], sh, sw, out)


def identity_maps(n: int) -> np.ndarray:
    return np.tile(np.array([1.0, 0.0, 0.0, 0.0, 1.0, 0.0]), (n, 1))


def sample_hed(rng: np.random.Generator, n: int, sigma_ranges, bias_ranges):
    """(sigma, bias) float32 (n, 3): per image three sigmas, then three biases, uniform in their ranges -- the order of
    ``HEDTransform.sample_sigma`` / ``sample_bias``.  One ``rng.uniform`` call of shape (n, 2, 3); images outside the cut-off consume
    their draws too (the reference does not draw for them)."""
    lo = np.array([[r[0] for r in sigma_ranges], [r[0] for r in bias_ranges]], np.float64)
    hi = np.array([[r[1] for r in sigma_ranges], [r[1] for r in bias_ranges]], np.float64)
    u = rng.uniform(lo, hi, size=(n, 2, 3))
    return u[:, 0].astype(np.float32), u[:, 1].astype(np.float32)


@dataclass
class BatchParams:
    """What ``augment_batch`` drew for one batch: everything ``apply_params`` needs."""
    sigma: np.ndarray | None        # (n, 3) float32, None without colour augmentation
    bias: np.ndarray | None
    inv: np.ndarray                 # (n, 6) float64 inverse maps (identity without geometry)
    flip: np.ndarray                # (n,) bool


def sample_batch_params(rng: np.random.Generator, n: int, sh: int, sw: int, config: dict | None, scale_range: float = 0.5,
                        geometry: bool = True, out: int = 256, rescale=None) -> BatchParams:
    """Draw order per batch: ``sample_hed`` (when ``config`` is given), then ``sample_affine`` (when ``geometry``), which takes
    ``rescale`` (n,) -- without geometry there is no scale to divide and ``rescale`` is refused."""
    if rescale is not None and not geometry:
        raise ValueError("rescale needs the geometric augmentation")
    sigma = bias = None
    if config is not None:
        sigma, bias = sample_hed(rng, n, config["sigma_ranges"], config["bias_ranges"])
    if geometry:
        flip, inv = sample_affine(rng, n, sh, sw, out, scale_range, rescale=rescale)
    else:
        flip, inv = np.zeros(n, bool), identity_maps(n)
    return BatchParams(sigma, bias, inv, flip)


def apply_params(X: torch.Tensor, labels: torch.Tensor, p: BatchParams, config: dict | None, label_fill: int = 0,
                 out_hw=(256, 256)):
    """The device chain up to the normalised float32 crops: (float32 (n, 3, dh, dw), int16 (n, dh, dw)).  uint8 crops get the stain
    jitter (when ``config`` and the draws are given), the warp and the float32 normalisation; float32 crops are by contract already
    normalised and get the warp only."""
    if X.dtype == torch.uint8:
        if config is not None and p.sigma is not None:
            X, _applied = ops.hed_jitter(X, p.sigma, p.bias, config["cutoff_range"], config.get("simple_mode", False))
        x, lab = ops.warp_affine(X, p.inv, out_hw, labels, label_fill)
        return ops.normalize_img_f32(x, out=x), lab
    return ops.warp_affine(X, p.inv, out_hw, labels, label_fill)


def _to_device(X, labels, device):
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X))
    if not isinstance(labels, torch.Tensor):
        labels = torch.from_numpy(np.ascontiguousarray(labels))
    dev = torch.device(device) if device is not None else (X.device if X.is_cuda else torch.device("cuda"))
    u8 = X.dtype == torch.uint8 and X.dim() == 4 and X.shape[3] == 3
    f32 = X.dtype == torch.float32 and X.dim() == 4 and X.shape[1] == 3
    if not (u8 or f32):
        raise ValueError("augment_batch: crops must be uint8 (n, H, W, 3) or float32 (n, 3, H, W)")
    sh, sw = (X.shape[1], X.shape[2]) if u8 else (X.shape[2], X.shape[3])
    if labels.dtype.is_floating_point or tuple(labels.shape) != (X.shape[0], sh, sw):
        raise ValueError(f"augment_batch: labels must be integer class maps {(X.shape[0], sh, sw)}")
    return X.to(dev).contiguous(), labels.to(device=dev, dtype=torch.int16).contiguous(), sh, sw


def augment_batch(X, labels, rng: np.random.Generator, config: str | None = "hed_only", scale_range: float = 0.5,
                  label_fill: int = 0, geometry: bool = True, dtype: torch.dtype = torch.bfloat16, device=None, out: int = 256,
                  rescale=None):
    """One augmented training batch on the device: (patch rows (n * (out / 8)^2, 192) in ``dtype``, int16 labels (n, out, out)), what
    ``HeadTrainer.step`` takes.  Stain jitter (``config``: a name of ``AUGMENT_CONFIGS``, or None / "geometry" for none), warp
    (``geometry``), float32 normalisation, ``ops.patchify_f32``.  ``label_fill`` is the class of out-of-frame pixels: 0 as in the
    reference, where out-of-frame is background, or -100 to leave them out of the loss.  A crop whose warped labels are all -100
    gets a new transform, at most ``MAX_RESAMPLE`` times.  Draw order of a resampling round: one ``sample_batch_params`` call for the
    k crops that are still empty, in ascending crop order -- so fresh stain values (k, 2, 3) first when ``config`` is set, then the
    four affine draws of size k -- after everything the batch drew before.  ``rescale`` (n,) float64, the per-crop
    ``diameter / diam_mean``, divides the random scale (``sample_affine_params``); a resampling round passes the factors of the
    crops that are still empty."""
    cfg = get_config(config)
    X, labels, sh, sw = _to_device(X, labels, device)
    n = X.shape[0]
    rescale = _check_rescale(rescale, n)
    p = sample_batch_params(rng, n, sh, sw, cfg, scale_range, geometry, out, rescale)
    x, lab = apply_params(X, labels, p, cfg, label_fill, (out, out))
    for _ in range(MAX_RESAMPLE):
        empty = torch.nonzero((lab == -100).flatten(1).all(1)).flatten()
        if empty.numel() == 0:
            break
        if not geometry:
            raise ValueError(f"augment_batch: crop {int(empty[0])} has no annotated pixel")
        q = sample_batch_params(rng, int(empty.numel()), sh, sw, cfg, scale_range, geometry, out,
                                None if rescale is None else rescale[empty.cpu().numpy()])
        x2, lab2 = apply_params(X[empty], labels[empty], q, cfg, label_fill, (out, out))
        x[empty], lab[empty] = x2, lab2
    else:
        if bool((lab == -100).flatten(1).all(1).any()):
            raise ValueError(f"augment_batch: a crop had no annotated pixel after {MAX_RESAMPLE} resampled transforms")
    return ops.patchify_f32(x, dtype), lab
