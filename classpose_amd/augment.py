"""Training-time augmentation of class-head crops on the device.

The reference's loader (dataset.py:23-56) applies a stain jitter in the HED colour space, then cellpose's
``random_rotate_and_resize`` (flip, rotation, scale, crop), and normalises AFTER both.  Here the host only draws the random
parameters; the pixels stay on the device: ``ops.hed_jitter`` -> ``ops.warp_affine`` -> ``ops.normalize_img_f32`` ->
``ops.patchify_f32`` (csrc/cpx_augment.hip, csrc/cpx_train.hip).

Random draws come from the numpy ``Generator`` passed in, in the order documented on each sampler.  The reference draws from the
global ``np.random`` state, so its sample stream is not reproduced; its distributions are.

Whole annotated images of any size live in an ``ImagePool``: uploaded once, packed back to back, and
``augment_batch_pool`` cuts every crop of a batch out of its own image with one fused launch (``ops.warp_affine_pool``: the stain
jitter on the taps, the warp) -- the fresh random window per epoch of dataset.py:23-56.  ``grid_crops`` are the deterministic
windows used where nothing is augmented.

The H&E stain-matrix perturbation (configurations ``he_staining`` and ``hed_he``) re-renders every crop from its image's
own two-stain basis: the basis is fitted once per image on the host (``stain.stain_basis`` on the samples of ``ops.stain_samples``,
cached on the ``ImagePool``), the draws perturb it, and the pixels go through ``ops.he_stain`` or, on a pool, through the taps of
``ops.warp_affine_pool_stain``.

The image-quality stage (configurations ``quality`` and ``hed_he_quality``, the latter the reference's whole ``enhanced``
pipeline under a name of its own) follows the colour stage: a Gaussian blur (``ops.blur``; on a pool ``ops.blur_pool_rects`` on the
footprint of each gated crop, read back by the taps of ``ops.warp_affine_pool_quality``) and the hue / brightness / saturation
jitter (``ops.hbs``, or on the same taps).  The reference's additive noise is an identity on uint8 and is not built.

Still different from the reference: the warp samples at exact double-precision source coordinates (OpenCV quantises them to
1 / 32 pixel).  The rescale by cell diameter (dataset.py:35-45) is the ``rescale``
argument of the samplers: per crop ``diameter / diam_mean``, the diameters from ``dataset_stats.label_stats``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import ops, stain
from .stain import stain_basis  # noqa: F401  (augment.stain_basis: the two-stain basis of an image from its samples)

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
    # augmentation_configs.py:36-46 (he_staining_config, hed_probability of ENHANCED_CONFIG), under names of their own:
    # the stain-matrix perturbation alone, and the colour stage of `enhanced` (per image the HED jitter or the perturbation)
    "he_staining": {
        "he_staining": {"amount_matrix": 0.15, "amount_stains": 0.4, "probability": 0.9},
    },
    "hed_he": {
        "sigma_ranges": [(-_HED_VALUE, _HED_VALUE)] * 3,
        "bias_ranges": [(-_HED_VALUE, _HED_VALUE)] * 3,
        "cutoff_range": (0.15, 0.85),
        "simple_mode": False,
        "hed_probability": 0.5,
        "he_staining": {"amount_matrix": 0.15, "amount_stains": 0.4, "probability": 0.9},
    },
}
# augmentation_configs.py:47-60 (gaussian_blur_config, hbs_config of ENHANCED_CONFIG): the image-quality stage alone, and after the
# colour stage of "hed_he" -- the latter is everything the reference's `enhanced` strategy does to a pixel
_QUALITY = {
    "gaussian_blur": {"sigma_range": (0, 2), "probability": 0.1},
    "hbs": {"hue": 0.1, "brightness": 0.1, "saturation": (0.9, 1.1), "probability": 0.9},
}
AUGMENT_CONFIGS["quality"] = dict(_QUALITY)
AUGMENT_CONFIGS["hed_he_quality"] = {**AUGMENT_CONFIGS["hed_he"], **_QUALITY}
MAX_RESAMPLE = 8


def get_config(name: str | None) -> dict | None:
    """The stain-jitter settings of a named configuration; ``None`` and ``"geometry"`` mean no colour augmentation."""
    if name is None or name == "geometry":
        return None
    if name == "enhanced":
        raise NotImplementedError("the name 'enhanced' is not enabled: 'hed_he_quality' runs the reference's pipeline (the colour stage "
                                  "'hed_he', then the Gaussian blur and the hue / brightness / saturation jitter)")
    if name not in AUGMENT_CONFIGS:
        raise ValueError(f"unknown augmentation {name!r}: one of {sorted(AUGMENT_CONFIGS) + ['geometry']}")
    return AUGMENT_CONFIGS[name]


def _source_shapes(sh, sw, n: int):
    """(sh, sw) as float64 (n,) arrays: a scalar source shape for every crop, or one per crop.  Sizes are integers, so the
    conversion is exact and what follows is bitwise the arithmetic on the integers themselves."""
    sh, sw = np.asarray(sh, np.float64), np.asarray(sw, np.float64)
    if sh.shape not in ((), (n,)) or sw.shape not in ((), (n,)):
        raise ValueError(f"source shapes: a scalar or one value per crop ({n}) expected")
    if not (np.all(sh > 0) and np.all(sw > 0)):
        raise ValueError("source shapes must be positive")
    return np.broadcast_to(sh, (n,)), np.broadcast_to(sw, (n,))


def affine_inverse(flip, theta, scale, dxy, sh, sw, out: int = 256) -> np.ndarray:
    """(n, 6) float64 inverse maps, source (sx, sy) = inv . (x, y, 1), of cellpose's forward map
    ``dst = scale * R(theta) * (src - cc) + cc1`` with ``R = [[cos, -sin], [sin, cos]]``, ``cc = (sw / 2, sh / 2)`` and
    ``cc1 = cc - ([sw, sh] - out) / 2 + dxy``.  Where ``flip`` is set the horizontal flip of the source, ``sx -> sw - 1 - sx``,
    is folded into the map.  ``sh`` / ``sw``: the source shape, a scalar or one per crop."""
    flip, theta, scale = np.asarray(flip, bool), np.asarray(theta, np.float64), np.asarray(scale, np.float64)
    dxy = np.asarray(dxy, np.float64).reshape(-1, 2)
    sh, sw = _source_shapes(sh, sw, len(theta))
    cc = np.stack([sw / 2, sh / 2], 1)                                              # (n, 2)
    cc1 = cc - (np.stack([sw, sh], 1) - out) / 2 + dxy
    c, s = np.cos(theta) / scale, np.sin(theta) / scale
    inv = np.empty((len(theta), 6), np.float64)
    inv[:, 0], inv[:, 1] = c, s                                                     # (1 / scale) R^T
    inv[:, 3], inv[:, 4] = -s, c
    inv[:, 2] = cc[:, 0] - (c * cc1[:, 0] + s * cc1[:, 1])
    inv[:, 5] = cc[:, 1] - (-s * cc1[:, 0] + c * cc1[:, 1])
    inv[flip, 0:2] = -inv[flip, 0:2]
    inv[flip, 2] = (sw[flip] - 1) - inv[flip, 2]
    return inv


def affine_forward(theta, scale, dxy, sh, sw, out: int = 256) -> np.ndarray:
    """(n, 6) float64 forward maps ``dst = fwd . (sx, sy, 1)`` of the same parametrisation, without the flip."""
    theta, scale = np.asarray(theta, np.float64), np.asarray(scale, np.float64)
    dxy = np.asarray(dxy, np.float64).reshape(-1, 2)
    sh, sw = _source_shapes(sh, sw, len(theta))
    cc = np.stack([sw / 2, sh / 2], 1)
    cc1 = cc - (np.stack([sw, sh], 1) - out) / 2 + dxy
    c, s = np.cos(theta) * scale, np.sin(theta) * scale
    fwd = np.empty((len(theta), 6), np.float64)
    fwd[:, 0], fwd[:, 1] = c, -s
    fwd[:, 3], fwd[:, 4] = s, c
    fwd[:, 2] = cc1[:, 0] - (c * cc[:, 0] - s * cc[:, 1])
    fwd[:, 5] = cc1[:, 1] - (s * cc[:, 0] + c * cc[:, 1])
    return fwd


def _check_rescale(rescale, n: int) -> np.ndarray | None:
    if rescale is None:
        return None
    rescale = np.asarray(rescale, np.float64)
    if rescale.shape != (n,) or not np.all(rescale > 0):
        raise ValueError(f"rescale: {n} positive factors (diameter / diam_mean per crop) expected")
    return rescale


def sample_affine_params(rng: np.random.Generator, n: int, sh, sw, out: int = 256, scale_range: float = 0.5,
                         do_flip: bool = True, rotate: bool = True, rescale=None) -> dict:
    """The random parameters behind ``sample_affine``: ``flip`` (n,) bool, ``theta``, ``scale`` (n,), ``dxy`` (n, 2).
    Draw order, always all four so that the stream does not depend on the switches: ``rng.random(n)`` for the flips, ``rng.random(n)``
    for theta, ``rng.random(n)`` for the scale, ``rng.random((n, 2))`` for the shift (x, y).  ``rescale`` (n,) float64, the per-crop
    ``diameter / diam_mean`` (dataset.py:35-38), divides the scale; the crop room behind ``dxy`` follows from the divided scale.
    It changes neither the number nor the order of the draws, and ``rescale=None`` is bitwise the sampler without it.
    ``sh`` / ``sw`` are a scalar or one value per crop (crops of an ``ImagePool``): every crop's room follows from its own source,
    and neither the number nor the order of the draws depends on the shapes."""
    r = float(np.clip(scale_range, 0.0, 2.0))
    rescale = _check_rescale(rescale, n)
    sh, sw = _source_shapes(sh, sw, n)
    u_flip, u_theta, u_scale, u_dxy = rng.random(n), rng.random(n), rng.random(n), rng.random((n, 2))
    flip = (u_flip > 0.5) & bool(do_flip)
    theta = 2 * np.pi * u_theta if rotate else np.zeros(n)
    scale = (1 - r / 2) + r * u_scale
    if rescale is not None:
        scale = scale / rescale
    room = np.maximum(0.0, np.stack([sw * scale - out, sh * scale - out], 1))
    return dict(flip=flip, theta=theta, scale=scale, dxy=(u_dxy - 0.5) * room)


def sample_affine(rng: np.random.Generator, n: int, sh, sw, out: int = 256, scale_range: float = 0.5,
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


def flow_vec(flip, theta) -> np.ndarray:
    """(n, 4) float64 vector matrices of ``ops.warp_flow_targets`` for the draws ``flip`` / ``theta`` of ``sample_affine_params``:
    ``[cos t, f sin t, -sin t, f cos t]`` with ``f = -1`` where flipped, ``+1`` otherwise, so that ``Y' = vec[0] Y + vec[1] X`` and
    ``X' = vec[2] Y + vec[3] X``.  Restated from the flow branch of cellpose 4.0.x ``transforms.random_rotate_and_resize`` (unpinned,
    like ``sample_affine``): the X flow of a flipped source is negated, then ``Y' = X sin t + Y cos t``, ``X' = X cos t - Y sin t``.
    The scale does not rescale the vectors."""
    flip, theta = np.asarray(flip, bool).reshape(-1), np.asarray(theta, np.float64).reshape(-1)
    if flip.shape != theta.shape:
        raise ValueError("flow_vec: one flip and one theta per crop")
    f = np.where(flip, -1.0, 1.0)
    c, s = np.cos(theta), np.sin(theta)
    return np.stack([c, f * s, -s, f * c], 1)


def identity_vecs(n: int) -> np.ndarray:
    return np.tile(np.array([1.0, 0.0, 0.0, 1.0]), (n, 1))


def sample_hed(rng: np.random.Generator, n: int, sigma_ranges, bias_ranges):
    """(sigma, bias) float32 (n, 3): per image three sigmas, then three biases, uniform in their ranges -- the order of
    ``HEDTransform.sample_sigma`` / ``sample_bias``.  One ``rng.uniform`` call of shape (n, 2, 3); images outside the cut-off consume
    their draws too (the reference does not draw for them)."""
    lo = np.array([[r[0] for r in sigma_ranges], [r[0] for r in bias_ranges]], np.float64)
    hi = np.array([[r[1] for r in sigma_ranges], [r[1] for r in bias_ranges]], np.float64)
    u = rng.uniform(lo, hi, size=(n, 2, 3))
    return u[:, 0].astype(np.float32), u[:, 1].astype(np.float32)


def _has_hed(config: dict | None) -> bool:
    return config is not None and "sigma_ranges" in config


def _has_he(config: dict | None) -> bool:
    return config is not None and "he_staining" in config


def sample_he(rng: np.random.Generator, n: int):
    """(u_gate (n,), U (n, 2, 3), u (n, 2)) float64 of the stain perturbation: ``rng.random(n)`` for the probability gate, then
    ``rng.uniform(-1, 1, (n, 2, 3))`` for the stain matrix, then ``rng.uniform(-1, 1, (n, 2))`` for the two concentrations -- the
    order of ``HEStainingTransform.transform`` / ``augment_stains``.  All three are drawn for every crop, whatever the gate decides
    (the reference draws nothing for a skipped image, and draws from a legacy ``RandomState`` seeded per image)."""
    return rng.random(n), rng.uniform(-1.0, 1.0, size=(n, 2, 3)), rng.uniform(-1.0, 1.0, size=(n, 2))


def _has_quality(config: dict | None) -> bool:
    return config is not None and "gaussian_blur" in config


def sample_quality(rng: np.random.Generator, n: int, config: dict):
    """(u_blur, sigma, u_hbs, hue, brightness, saturation), each (n,) float64, of the image-quality stage: ``rng.random(n)`` for the
    blur's gate, ``rng.uniform(lo, hi, n)`` for sigma, ``rng.random(n)`` for the HBS gate, then ``rng.uniform`` for the hue shift in
    +-hue, the brightness offset in +-brightness (the factor is 1 + offset) and the saturation factor in its range -- the order of
    ``GaussianBlurTransform.transform`` and ``_hbs_adjust``.  All six are drawn for every crop, whatever the gates decide; a stage
    applies where ``u <= probability`` (the reference skips where ``random() > probability``)."""
    b, h = config["gaussian_blur"], config["hbs"]
    u_blur = rng.random(n)
    sigma = rng.uniform(b["sigma_range"][0], b["sigma_range"][1], n)
    u_hbs = rng.random(n)
    hue = rng.uniform(-h["hue"], h["hue"], n)
    brightness = rng.uniform(-h["brightness"], h["brightness"], n)
    saturation = rng.uniform(h["saturation"][0], h["saturation"][1], n)
    return u_blur, sigma, u_hbs, hue, brightness, saturation


def gauss_weights(sigma: float) -> tuple[int, np.ndarray]:
    """(radius, weights (17,) float64) of ``scipy.ndimage.gaussian_filter(x, sigma)`` with its defaults (truncate 4, order 0):
    ``radius = int(4 * sigma + 0.5)``, ``phi = exp(-0.5 / sigma**2 * x**2)`` for ``x = -radius .. radius``, ``phi / phi.sum()`` in
    entries ``0 .. 2 * radius``, zeros beyond.  Radius 0 (sigma < 0.125) is the identity, weight 1."""
    sigma = float(sigma)
    if not 0.0 <= sigma <= 2.0:
        raise ValueError(f"gauss_weights: sigma in [0, 2] expected (radius at most 8), got {sigma}")
    radius = int(4.0 * sigma + 0.5)
    w = np.zeros(17, np.float64)
    if radius == 0:
        w[0] = 1.0
        return 0, w
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * x ** 2)
    w[:2 * radius + 1] = phi / phi.sum()
    return radius, w


def footprint_rects(inv, sh, sw, out_hw=(256, 256)):
    """(rects (n, 4) int64 rows (y0, x0, h, w), ok (n,) bool): per crop the part of its ``sh`` x ``sw`` image that the bilinear taps of
    the ``out_hw`` window under the inverse map ``inv`` can touch.  The source coordinates are affine in the output pixel and are
    formed as the kernel forms them (``(a * x + b * y) + c`` in double, each rounding monotone), so their extremes lie at the four
    corners of the window; the taps of a coordinate s are floor(s) and floor(s) + 1.  Clipped to the image; ``ok`` is False where
    nothing of the image is left (or the map is not finite) and the rectangle is zeros."""
    inv = np.asarray(inv, np.float64).reshape(-1, 6)
    n = len(inv)
    sh, sw = _source_shapes(sh, sw, n)
    dh, dw = (int(v) for v in out_hw)
    xs, ys = np.array([0.0, dw - 1.0, 0.0, dw - 1.0]), np.array([0.0, 0.0, dh - 1.0, dh - 1.0])
    sx = (inv[:, 0:1] * xs + inv[:, 1:2] * ys) + inv[:, 2:3]
    sy = (inv[:, 3:4] * xs + inv[:, 4:5] * ys) + inv[:, 5:6]
    rects, ok = np.zeros((n, 4), np.int64), np.zeros(n, bool)
    for t in range(n):
        if not (np.all(np.isfinite(sx[t])) and np.all(np.isfinite(sy[t]))):
            continue
        x_lo, x_hi = max(np.floor(sx[t].min()), 0.0), min(np.floor(sx[t].max()) + 1.0, sw[t] - 1.0)
        y_lo, y_hi = max(np.floor(sy[t].min()), 0.0), min(np.floor(sy[t].max()) + 1.0, sh[t] - 1.0)
        if x_lo > x_hi or y_lo > y_hi:
            continue
        rects[t] = (int(y_lo), int(x_lo), int(y_hi - y_lo) + 1, int(x_hi - x_lo) + 1)
        ok[t] = True
    return rects, ok


@dataclass
class StainBases:
    """The two-stain bases of a set of images: H (n, 2, 3), Hinv (n, 3, 2) float64, ok (n,) bool -- False where the fit gave no
    finite basis and the image stays unaugmented (its rows are zeros)."""
    H: np.ndarray
    Hinv: np.ndarray
    ok: np.ndarray

    def __len__(self) -> int:
        return len(self.ok)

    def take(self, idx) -> "StainBases":
        idx = np.asarray(idx, np.int64)
        return StainBases(self.H[idx], self.Hinv[idx], self.ok[idx])

    @classmethod
    def from_samples(cls, samples) -> "StainBases":
        """One ``stain.stain_basis`` per entry of ``samples`` (each (m, 3) uint8)."""
        n = len(samples)
        H, Hinv, ok = np.zeros((n, 2, 3)), np.zeros((n, 3, 2)), np.zeros(n, bool)
        for i, smp in enumerate(samples):
            h, hinv = stain.stain_basis(smp)
            if h is not None:
                H[i], Hinv[i], ok[i] = h, hinv, True
        return cls(H, Hinv, ok)


def stain_bases_of(X, device=None, chunk: int = 64) -> StainBases:
    """The stain bases of uint8 crops (n, H, W, 3), numpy or torch: the samples come from ``ops.stain_samples`` (the crops as a
    pool of equal-sized images, ``chunk`` at a time), the fit runs on the host.  Once per training set."""
    if isinstance(X, np.ndarray):
        X = torch.from_numpy(np.ascontiguousarray(X))
    if X.dtype != torch.uint8 or X.dim() != 4 or X.shape[3] != 3:
        raise ValueError("stain_bases_of: crops must be uint8 (n, H, W, 3)")
    dev = torch.device(device) if device is not None else (X.device if X.is_cuda else torch.device("cuda"))
    samples = []
    for s in range(0, X.shape[0], chunk):
        x = X[s:s + chunk].to(dev).contiguous()
        px_off, hw, _px = pool_table([(x.shape[1], x.shape[2])] * x.shape[0])
        _k, smp, _st, _raw = ops.stain_samples(x.view(-1), torch.from_numpy(px_off).to(dev), torch.from_numpy(hw).to(dev))
        samples += smp
    return StainBases.from_samples(samples)


@dataclass
class BatchParams:
    """What ``augment_batch`` drew for one batch: everything ``apply_params`` needs."""
    sigma: np.ndarray | None        # (n, 3) float32, None without the HED jitter
    bias: np.ndarray | None
    inv: np.ndarray                 # (n, 6) float64 inverse maps (identity without geometry)
    flip: np.ndarray                # (n,) bool
    use_hed: np.ndarray | None = None   # (n,) bool, "hed_he" only: True = the HED jitter for this crop, False = the stain perturbation
    he_gate: np.ndarray | None = None   # (n,) float64 in [0, 1): the perturbation applies where he_gate <= probability
    he_matrix: np.ndarray | None = None     # (n, 2, 3) float64 in [-1, 1): U of M = max(H + amount_matrix * U, 0)
    he_stains: np.ndarray | None = None     # (n, 2) float64 in [-1, 1): u of the factors 1 + amount_stains * u
    blur_gate: np.ndarray | None = None     # (n,) float64 in [0, 1): the blur applies where blur_gate <= probability
    blur_sigma: np.ndarray | None = None    # (n,) float64 in the sigma range
    hbs_gate: np.ndarray | None = None      # (n,) float64 in [0, 1): the HBS jitter applies where hbs_gate <= probability
    hbs_hue: np.ndarray | None = None       # (n,) float64 in +-hue
    hbs_brightness: np.ndarray | None = None    # (n,) float64 in +-brightness: the factor is 1 + this
    hbs_saturation: np.ndarray | None = None    # (n,) float64 in the saturation range
    theta: np.ndarray | None = None         # (n,) float64, the rotation of the affine draw (zeros without geometry): ``flow_vec`` needs it


def quality_params(p: BatchParams, config: dict):
    """(blurred (n,) bool, radius (n,) int32, weights (n, 17) float64, hbs (n, 4) float32, hbs_apply (n,) int32) of a batch for
    ``ops.blur`` / ``ops.blur_pool_rects`` and ``ops.hbs`` / ``ops.warp_affine_pool_quality``.  A crop is blurred where its gate passed
    and its radius is not 0 (radius 0 is the identity).  hbs rows: float32 of {hue, 1 + brightness, saturation, 1 - saturation}, the
    last formed in double first."""
    n = len(p.blur_gate)
    gated = p.blur_gate <= config["gaussian_blur"]["probability"]
    radius, weights = np.zeros(n, np.int32), np.zeros((n, 17), np.float64)
    weights[:, 0] = 1.0
    for t in np.flatnonzero(gated):
        radius[t], weights[t] = gauss_weights(p.blur_sigma[t])
    hbs = np.stack([p.hbs_hue, 1.0 + p.hbs_brightness, p.hbs_saturation, 1.0 - p.hbs_saturation], 1).astype(np.float32)
    apply = (p.hbs_gate <= config["hbs"]["probability"]).astype(np.int32)
    return gated & (radius > 0), radius, weights, hbs, apply


def stain_mode_params(p: BatchParams, config: dict, bases: StainBases, hed_applied=None):
    """(mode (n,) int32, params (n, 14) float64) of a batch for ``ops.he_stain`` / ``ops.warp_affine_pool_stain``.  Mode per crop:
    where ``p.use_hed`` (all False without the HED jitter in ``config``) 1 if ``hed_applied`` (the jitter's cut-off decision of the
    crop's image; None = all inside) else 0; elsewhere 2 if ``he_gate <= probability`` and the image has a finite basis, else 0."""
    he = config["he_staining"]
    n = len(p.he_gate)
    if len(bases) != n:
        raise ValueError(f"stain bases: one per crop ({n}) expected, got {len(bases)}")
    use_hed = np.zeros(n, bool) if p.use_hed is None else p.use_hed
    applied = np.ones(n, bool) if hed_applied is None else np.asarray(hed_applied).astype(bool)
    mode = np.where(use_hed, np.where(applied, 1, 0), np.where((p.he_gate <= he["probability"]) & bases.ok, 2, 0)).astype(np.int32)
    params = np.zeros((n, 14), np.float64)
    for t in np.flatnonzero(mode == 2):
        params[t] = stain.stain_params(bases.H[t], bases.Hinv[t], p.he_matrix[t], p.he_stains[t], he["amount_matrix"],
                                       he["amount_stains"])
    return mode, params


def sample_batch_params(rng: np.random.Generator, n: int, sh, sw, config: dict | None, scale_range: float = 0.5,
                        geometry: bool = True, out: int = 256, rescale=None) -> BatchParams:
    """Draw order per batch: ``rng.random(n)`` for the choice between the HED jitter (``u < hed_probability``) and the stain
    perturbation (when ``config`` has both: "hed_he"), then ``sample_hed`` (when ``config`` has the jitter), then ``sample_he`` (when
    it has the perturbation), then ``sample_quality`` (when it has the image-quality stage: "quality", "hed_he_quality"), then
    ``sample_affine`` (when ``geometry``), which takes ``rescale`` (n,) -- without geometry there is
    no scale to divide and ``rescale`` is refused.  Every draw is made for every crop, whatever the choice and the gates decide.
    "hed_only" and "geometry" draw what they always drew."""
    if rescale is not None and not geometry:
        raise ValueError("rescale needs the geometric augmentation")
    sigma = bias = use_hed = gate = U = u = None
    if _has_hed(config) and _has_he(config):
        use_hed = rng.random(n) < config["hed_probability"]
    if _has_hed(config):
        sigma, bias = sample_hed(rng, n, config["sigma_ranges"], config["bias_ranges"])
    if _has_he(config):
        gate, U, u = sample_he(rng, n)
    quality = sample_quality(rng, n, config) if _has_quality(config) else (None,) * 6
    if geometry:                                              # sample_affine, keeping the rotation it drew
        a = sample_affine_params(rng, n, sh, sw, out, scale_range, rescale=rescale)
        flip, theta = a["flip"], a["theta"]
        inv = affine_inverse(flip, theta, a["scale"], a["dxy"], sh, sw, out)
    else:
        flip, inv, theta = np.zeros(n, bool), identity_maps(n), np.zeros(n)
    return BatchParams(sigma, bias, inv, flip, use_hed, gate, U, u, *quality, theta)


def _colour_stage(X: torch.Tensor, p: BatchParams, config: dict, bases: StainBases | None) -> torch.Tensor:
    """The colour stage of a configuration with the stain perturbation on uint8 crops: ``ops.he_stain`` on the crops it falls to,
    ``ops.hed_jitter`` on those the choice gave to the jitter."""
    if bases is None:
        bases = stain_bases_of(X)
    mode, params = stain_mode_params(p, config, bases)
    out = ops.he_stain(X, params, np.where(mode == 2, 2, 0))
    if p.use_hed is not None and p.use_hed.any():
        ci = torch.from_numpy(np.flatnonzero(p.use_hed)).to(X.device)
        jit, _applied = ops.hed_jitter(X[ci], p.sigma[p.use_hed], p.bias[p.use_hed], config["cutoff_range"],
                                       config.get("simple_mode", False))
        out[ci] = jit
    return out


def apply_params(X: torch.Tensor, labels: torch.Tensor, p: BatchParams, config: dict | None, label_fill: int = 0,
                 out_hw=(256, 256), stain_bases: StainBases | None = None):
    """The device chain up to the normalised float32 crops: (float32 (n, 3, dh, dw), int16 (n, dh, dw)).  uint8 crops get the colour
    stage (when ``config`` and the draws are given: the stain jitter, the stain perturbation, or per crop one of the two), the warp
    and the float32 normalisation; float32 crops are by contract already normalised and get the warp only.  ``stain_bases``: one
    basis per crop for the stain perturbation; computed here from the crops when absent.  With the image-quality stage in
    ``config`` the gated crops go through ``ops.blur`` and ``ops.hbs`` between the colour stage and the warp."""
    if X.dtype == torch.uint8:
        if _has_he(config) and p.he_gate is not None:
            X = _colour_stage(X, p, config, stain_bases)
        elif config is not None and p.sigma is not None:
            X, _applied = ops.hed_jitter(X, p.sigma, p.bias, config["cutoff_range"], config.get("simple_mode", False))
        if _has_quality(config) and p.blur_gate is not None:
            blurred, radius, weights, hbs, hbs_apply = quality_params(p, config)
            if blurred.any():
                ci = torch.from_numpy(np.flatnonzero(blurred)).to(X.device)
                Xb = X.clone()
                Xb[ci] = ops.blur(X[ci], radius[blurred], weights[blurred])
                X = Xb
            X = ops.hbs(X, hbs, hbs_apply)
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
                  rescale=None, stain_bases: StainBases | None = None, flow_targets: torch.Tensor | None = None):
    """One augmented training batch on the device: (patch rows (n * (out / 8)^2, 192) in ``dtype``, int16 labels (n, out, out)), what
    ``HeadTrainer.step`` takes.  Stain jitter (``config``: a name of ``AUGMENT_CONFIGS``, or None / "geometry" for none), warp
    (``geometry``), float32 normalisation, ``ops.patchify_f32``.  ``label_fill`` is the class of out-of-frame pixels: 0 as in the
    reference, where out-of-frame is background, or -100 to leave them out of the loss.  A crop whose warped labels are all -100
    gets a new transform, at most ``MAX_RESAMPLE`` times.  Draw order of a resampling round: one ``sample_batch_params`` call for the
    k crops that are still empty, in ascending crop order -- so fresh stain values (k, 2, 3) first when ``config`` is set, then the
    four affine draws of size k -- after everything the batch drew before.  ``rescale`` (n,) float64, the per-crop
    ``diameter / diam_mean``, divides the random scale (``sample_affine_params``); a resampling round passes the factors of the
    crops that are still empty.  ``stain_bases`` (``stain_bases_of`` of these crops, in their order) spares the configurations with
    the stain perturbation ("he_staining", "hed_he") the fit per call; a resampling round reuses the bases of its crops.
    ``flow_targets`` (n, 3, sh, sw) float32 on the device, the (mask, flow Y, flow X) planes of the crops (``flow_targets_of``):
    the result then has a third value, the planes under each crop's final transform (``ops.warp_flow_targets``), float32
    (n, 3, out, out).  It changes no draw."""
    cfg = get_config(config)
    X, labels, sh, sw = _to_device(X, labels, device)
    n = X.shape[0]
    if flow_targets is not None and (not isinstance(flow_targets, torch.Tensor) or flow_targets.dtype != torch.float32
                                     or tuple(flow_targets.shape) != (n, 3, sh, sw) or flow_targets.device != X.device):
        raise ValueError(f"augment_batch: flow_targets must be float32 {(n, 3, sh, sw)} on the crops' device")
    rescale = _check_rescale(rescale, n)
    if _has_he(cfg) and X.dtype == torch.uint8 and stain_bases is None:
        stain_bases = stain_bases_of(X)
    p = sample_batch_params(rng, n, sh, sw, cfg, scale_range, geometry, out, rescale)
    x, lab = apply_params(X, labels, p, cfg, label_fill, (out, out), stain_bases)
    for _ in range(MAX_RESAMPLE):
        empty = torch.nonzero((lab == -100).flatten(1).all(1)).flatten()
        if empty.numel() == 0:
            break
        if not geometry:
            raise ValueError(f"augment_batch: crop {int(empty[0])} has no annotated pixel")
        q = sample_batch_params(rng, int(empty.numel()), sh, sw, cfg, scale_range, geometry, out,
                                None if rescale is None else rescale[empty.cpu().numpy()])
        x2, lab2 = apply_params(X[empty], labels[empty], q, cfg, label_fill, (out, out),
                                None if stain_bases is None else stain_bases.take(empty.cpu().numpy()))
        x[empty], lab[empty] = x2, lab2
        e = empty.cpu().numpy()
        p.inv[e], p.flip[e], p.theta[e] = q.inv, q.flip, q.theta
    else:
        if bool((lab == -100).flatten(1).all(1).any()):
            raise ValueError(f"augment_batch: a crop had no annotated pixel after {MAX_RESAMPLE} resampled transforms")
    if flow_targets is None:
        return ops.patchify_f32(x, dtype), lab
    px_off, hw, _px = pool_table([(sh, sw)] * n)                  # pre-cut crops of equal shape: a pool with a regular table
    tgt, _status = ops.warp_flow_targets(flow_targets.contiguous().view(-1), torch.from_numpy(px_off).to(X.device),
                                         torch.from_numpy(hw).to(X.device), np.arange(n), p.inv, flow_vec(p.flip, p.theta), (out, out))
    return ops.patchify_f32(x, dtype), lab, tgt


# ---------------------------------------------------------------------------------------------------------------------
# whole annotated images of any size: the device-resident pool
# ---------------------------------------------------------------------------------------------------------------------
def pool_table(shapes) -> tuple[np.ndarray, np.ndarray, int]:
    """(px_off (nI,) int64, hw (nI, 2) int32, pool_px) of images of ``shapes`` [(h, w), ...] packed back to back."""
    hw = np.asarray(shapes, np.int64).reshape(-1, 2)
    if len(hw) == 0 or np.any(hw <= 0) or np.any(hw > np.iinfo(np.int32).max):
        raise ValueError("pool_table: at least one image, and positive sizes")
    px = hw[:, 0] * hw[:, 1]
    px_off = np.concatenate([[0], np.cumsum(px)[:-1]]).astype(np.int64)
    return px_off, hw.astype(np.int32), int(px.sum())


def check_pool_table(px_off, hw, pool_px: int) -> None:
    """What the kernels rely on: positive sizes, image i + 1 starts where image i ends (so the offsets are monotone and nothing
    overlaps), and the pool is exactly the sum of h * w pixels long."""
    px_off, hw = np.asarray(px_off), np.asarray(hw)
    if px_off.ndim != 1 or len(px_off) == 0 or hw.shape != (len(px_off), 2):
        raise ValueError("pool table: px_off (nI,) and hw (nI, 2) expected")
    if np.any(hw <= 0):
        raise ValueError("pool table: image sizes must be positive")
    px = hw[:, 0].astype(np.int64) * hw[:, 1].astype(np.int64)
    if px_off[0] != 0 or np.any(np.diff(px_off) != px[:-1]):
        raise ValueError("pool table: offsets must start at 0 and grow by h * w from image to image")
    if int(px_off[-1] + px[-1]) != int(pool_px):
        raise ValueError(f"pool table: the pool holds {pool_px} pixels, the images {int(px_off[-1] + px[-1])}")


class ImagePool:
    """Whole annotated images of any size on the device, uploaded once: ``pool_u8`` the (h_i, w_i, 3) uint8 images packed back to
    back, ``pool_lab`` the int16 class maps at the same pixel offsets, ``px_off`` / ``hw`` the table (host copies ``px_off_host`` /
    ``hw_host``), ``pool_tgt`` (with ``instances``: the flow-head targets, see ``flow_targets_of``; else None), ``byte_sums`` (nI,) int64 on the host -- the exact byte sum of every image, from which ``applied`` forms the stain
    jitter's cut-off decision per image.  ``diameters`` (nI,) float64 or None travel with the images for ``rescale``.

    images: a sequence of (H, W, 3) uint8 arrays; labels: (H, W) integer class maps (-100 = not annotated) in int16 range."""

    def __init__(self, images, labels, diameters=None, device="cuda:0", instances=None):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("an ImagePool lives on the device: pass a cuda device (there is no CPU path)")
        images, labels = list(images), list(labels)
        if len(images) == 0 or len(images) != len(labels):
            raise ValueError("ImagePool: one class map per image, and at least one image")
        for i, (im, lab) in enumerate(zip(images, labels)):
            im, lab = np.asarray(im), np.asarray(lab)
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f"ImagePool: image {i} must be (H, W, 3) uint8, got {im.shape} {im.dtype}")
            if lab.shape != im.shape[:2] or not np.issubdtype(lab.dtype, np.integer):
                raise ValueError(f"ImagePool: class map {i} must be an integer map {im.shape[:2]}, got {lab.shape} {lab.dtype}")
            if lab.size and (lab.min() < -32768 or lab.max() > 32767):
                raise ValueError(f"ImagePool: class map {i} has values outside int16")
        self.px_off_host, self.hw_host, self.pool_px = pool_table([np.asarray(im).shape[:2] for im in images])
        check_pool_table(self.px_off_host, self.hw_host, self.pool_px)
        host_u8 = np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])
        host_lab = np.concatenate([np.asarray(lab).astype(np.int16).reshape(-1) for lab in labels])
        if host_u8.size != 3 * self.pool_px or host_lab.size != self.pool_px:
            raise ValueError("ImagePool: the packed pool does not have the length of its table")
        dev = self.device
        self.pool_u8, self.pool_lab = torch.from_numpy(host_u8).to(dev), torch.from_numpy(host_lab).to(dev)
        self.px_off, self.hw = torch.from_numpy(self.px_off_host).to(dev), torch.from_numpy(self.hw_host).to(dev)
        self.byte_sums = ops.pool_byte_sums(self.pool_u8, self.px_off, self.hw).cpu().numpy()
        self.annotated = np.array([bool((np.asarray(lab) != -100).any()) for lab in labels])
        if diameters is not None:
            diameters = np.asarray(diameters, np.float64)
            if diameters.shape != (len(images),) or not np.all(diameters > 0):
                raise ValueError("ImagePool: one positive diameter per image")
        self.diameters = diameters
        self._grid = None
        self._stain = None
        # with instance maps the pool also holds the flow-head targets: per image three float32 planes (mask, flow Y, flow X)
        # as [3][h][w] from float 3 * px_off[i] of ``pool_tgt`` (12 more bytes per pixel)
        self.pool_tgt = None
        self._grid_tgt = None
        if instances is not None:
            instances = list(instances)
            if len(instances) != len(images):
                raise ValueError("ImagePool: one instance map per image")
            for i, (im, inst) in enumerate(zip(images, instances)):
                if np.asarray(inst).shape != np.asarray(im).shape[:2]:
                    raise ValueError(f"ImagePool: instance map {i} must be {np.asarray(im).shape[:2]}, got {np.asarray(inst).shape}")
            self.pool_tgt = torch.cat([t.reshape(-1) for t in flow_targets_of(instances, dev)])

    def __len__(self) -> int:
        return len(self.px_off_host)

    @property
    def nbytes(self) -> int:
        """Device bytes of the pool: 3 per pixel of image, 2 per pixel of class map, 16 per table row; with instance maps 12 more
        per pixel for the three float32 target planes."""
        return (5 if self.pool_tgt is None else 17) * self.pool_px + 16 * len(self)

    def applied(self, cutoff_range) -> np.ndarray:
        """(nI,) int32: 1 where ``lo <= (byte sum / byte count) / 255.0 <= hi`` in double, the test of ``cpx_hed_jitter_u8`` on the
        WHOLE image (dataset.py:41 hands the whole image to the transform)."""
        count = 3.0 * self.hw_host[:, 0].astype(np.float64) * self.hw_host[:, 1].astype(np.float64)
        mean = (self.byte_sums.astype(np.float64) / count) / 255.0
        return ((float(cutoff_range[0]) <= mean) & (mean <= float(cutoff_range[1]))).astype(np.int32)

    def stain_basis(self) -> StainBases:
        """The two-stain basis of every image, fitted the first time a configuration with the stain perturbation asks
        for it and kept: the samples from ``ops.stain_samples`` (one pass over the pool), ``stain.stain_basis`` per image on the
        host."""
        if self._stain is None:
            _k, samples, _status, _raw = ops.stain_samples(self.pool_u8, self.px_off, self.hw)
            self._stain = StainBases.from_samples(samples)
        return self._stain


def sample_batch_params_pool(pool: ImagePool, idx, rng: np.random.Generator, config: dict | None, scale_range: float = 0.5,
                             geometry: bool = True, out: int = 256, rescale=None) -> BatchParams:
    """``sample_batch_params`` for crops out of images ``idx`` of a pool: the same draws in the same order, every crop's room from
    its own image.  Without geometry the map is the identity: the window at the image's origin."""
    idx = np.asarray(idx, np.int64)
    return sample_batch_params(rng, len(idx), pool.hw_host[idx, 0], pool.hw_host[idx, 1], config, scale_range, geometry, out, rescale)


def pool_colour_args(pool: ImagePool, idx, p: BatchParams, config: dict):
    """(mode (n,) int32, sigma, bias (n, 3) float32 or None, simple_mode, params (n, 14) float64 or None): the colour stage of the
    crops out of images ``idx`` as ``ops.warp_affine_pool_stain`` / ``ops.blur_pool_rects`` / ``ops.warp_affine_pool_quality`` take it.
    With the stain perturbation in ``config`` the modes are those of ``stain_mode_params`` (the jitter's cut-off from the pool's byte
    sums, the bases from the pool's cached ``stain_basis()``); without it every crop is in mode 0."""
    idx = np.asarray(idx, np.int64)
    sigma = bias = applied = params = None
    simple = False
    mode = np.zeros(len(idx), np.int32)
    if _has_he(config) and p.he_gate is not None:
        if p.sigma is not None:
            sigma, bias, applied = p.sigma, p.bias, pool.applied(config["cutoff_range"])[idx]
            simple = config.get("simple_mode", False)
        mode, params = stain_mode_params(p, config, pool.stain_basis().take(idx), applied)
    return mode, sigma, bias, simple, params


def apply_params_pool(pool: ImagePool, idx, p: BatchParams, config: dict | None, label_fill: int = 0, out_hw=(256, 256)):
    """The device chain of ``apply_params`` for crops out of images ``idx`` of a pool: one fused launch (stain jitter on the taps
    of the images inside the cut-off, warp), then the float32 normalisation.  With the stain perturbation in ``config`` the launch
    is ``ops.warp_affine_pool_stain``: per crop the jitter, the perturbation from the pool's cached ``stain_basis()``, or neither.
    With the image-quality stage in ``config``: one ``ops.blur_pool_rects`` launch writes, for every blurred crop, the blur of its
    colour-transformed image on the crop's ``footprint_rects`` rectangle into a scratch allocated here, and one
    ``ops.warp_affine_pool_quality`` launch warps all crops, the blurred ones out of the scratch, with the HBS jitter on the taps."""
    idx = np.asarray(idx, np.int64)
    sigma = bias = applied = None
    simple = False
    if _has_quality(config) and p.blur_gate is not None:
        n = len(idx)
        mode, sigma, bias, simple, params = pool_colour_args(pool, idx, p, config)
        blurred, radius, weights, hbs, hbs_apply = quality_params(p, config)
        rects, ok = footprint_rects(p.inv, pool.hw_host[idx, 0], pool.hw_host[idx, 1], out_hw)
        blurred &= ok
        scratch, ov_off = None, np.full(n, -1, np.int64)
        if blurred.any():
            b = np.flatnonzero(blurred)
            scratch, off, _status = ops.blur_pool_rects(
                pool.pool_u8, pool.px_off, pool.hw, idx[b], rects[b], radius[b], weights[b], mode=mode[b],
                sigma=None if sigma is None else sigma[b], bias=None if bias is None else bias[b], simple_mode=simple,
                params=None if params is None else params[b])
            ov_off[b] = off
        x, lab, _status = ops.warp_affine_pool_quality(pool.pool_u8, pool.pool_lab, pool.px_off, pool.hw, idx, p.inv, out_hw, mode, sigma,
                                                       bias, simple, params, hbs, hbs_apply, scratch, ov_off, rects, label_fill)
        return ops.normalize_img_f32(x, out=x), lab
    if _has_he(config) and p.he_gate is not None:
        mode, sigma, bias, simple, params = pool_colour_args(pool, idx, p, config)
        x, lab, _status = ops.warp_affine_pool_stain(pool.pool_u8, pool.pool_lab, pool.px_off, pool.hw, idx, p.inv, out_hw, mode, sigma,
                                                     bias, simple, params, label_fill)
        return ops.normalize_img_f32(x, out=x), lab
    if config is not None and p.sigma is not None:
        sigma, bias, applied = p.sigma, p.bias, pool.applied(config["cutoff_range"])[idx]
        simple = config.get("simple_mode", False)
    x, lab, _status = ops.warp_affine_pool(pool.pool_u8, pool.pool_lab, pool.px_off, pool.hw, idx, p.inv, out_hw, sigma, bias, applied,
                                           simple, label_fill)
    return ops.normalize_img_f32(x, out=x), lab


def augment_batch_pool(pool: ImagePool, idx, rng: np.random.Generator, config: str | None = "hed_only", scale_range: float = 0.5,
                       label_fill: int = 0, geometry: bool = True, dtype: torch.dtype = torch.bfloat16, out: int = 256,
                       rescale=None, flow_targets: bool = False):
    """``augment_batch`` for one window out of each of the images ``idx`` (repeats allowed) of an ``ImagePool``: (patch rows, int16
    labels (n, out, out)).  The draws, their order, the resampling of crops whose labels are all -100 and the tail
    (``normalize_img_f32`` -> ``patchify_f32``) are those of ``augment_batch``; on a pool of equal-sized images the result is bitwise
    ``augment_batch`` of the same images.  The stain jitter's cut-off test sees the whole image, as in the reference.
    ``flow_targets=True`` (a pool built with ``instances``) adds a third value: the pool's target planes under each crop's final
    transform, float32 (n, 3, out, out).  It changes no draw."""
    cfg = get_config(config)
    if flow_targets and pool.pool_tgt is None:
        raise ValueError("augment_batch_pool: flow_targets needs a pool built with instances")
    idx = np.asarray(idx, np.int64)
    n = len(idx)
    if idx.ndim != 1 or n == 0 or idx.min() < 0 or idx.max() >= len(pool):
        raise ValueError(f"augment_batch_pool: image indices in [0, {len(pool)}) expected")
    rescale = _check_rescale(rescale, n)
    p = sample_batch_params_pool(pool, idx, rng, cfg, scale_range, geometry, out, rescale)
    x, lab = apply_params_pool(pool, idx, p, cfg, label_fill, (out, out))
    for _ in range(MAX_RESAMPLE):
        empty = torch.nonzero((lab == -100).flatten(1).all(1)).flatten()
        if empty.numel() == 0:
            break
        if not geometry:
            raise ValueError(f"augment_batch_pool: crop {int(empty[0])} has no annotated pixel")
        e = empty.cpu().numpy()
        q = sample_batch_params_pool(pool, idx[e], rng, cfg, scale_range, geometry, out, None if rescale is None else rescale[e])
        x2, lab2 = apply_params_pool(pool, idx[e], q, cfg, label_fill, (out, out))
        x[empty], lab[empty] = x2, lab2
        p.inv[e], p.flip[e], p.theta[e] = q.inv, q.flip, q.theta
    else:
        if bool((lab == -100).flatten(1).all(1).any()):
            raise ValueError(f"augment_batch_pool: a crop had no annotated pixel after {MAX_RESAMPLE} resampled transforms")
    if not flow_targets:
        return ops.patchify_f32(x, dtype), lab
    tgt, _status = ops.warp_flow_targets(pool.pool_tgt, pool.px_off, pool.hw, idx, p.inv, flow_vec(p.flip, p.theta), (out, out))
    return ops.patchify_f32(x, dtype), lab, tgt


def grid_origins(h: int, crop: int = 256) -> list[int]:
    """Window origins along an axis of length ``h``: ``n = max(1, ceil(h / crop))`` windows, the first at 0 and the last at
    ``h - crop``, origin k at ``(k * (h - crop)) // (n - 1)``; one window at 0 where the axis is no longer than the crop."""
    h, crop = int(h), int(crop)
    n = max(1, -(-h // crop))
    if n == 1:
        return [0]
    return [(k * (h - crop)) // (n - 1) for k in range(n)]


def grid_windows(hw, crop: int = 256) -> np.ndarray:
    """(M, 3) int64 rows (image, y0, x0): the windows of ``grid_origins`` of every image, images in order, rows before columns."""
    rows = [(i, y0, x0) for i, (h, w) in enumerate(np.asarray(hw).reshape(-1, 2))
            for y0 in grid_origins(h, crop) for x0 in grid_origins(w, crop)]
    return np.asarray(rows, np.int64).reshape(-1, 3)


def grid_crops(pool: ImagePool, crop: int = 256, chunk: int = 64):
    """The deterministic windows used where nothing is augmented (validation, and training without ``augment``): (uint8
    (M, crop, crop, 3), int16 (M, crop, crop), windows (M, 3) int64 rows (image, y0, x0)), the first two on the device.  Cut by the
    pool kernel with integer-translation maps, so every pixel is exact; beyond the image the pixels are 0 and the labels -100,
    always.  A window without an annotated pixel is dropped.  Cached on the pool for the default arguments."""
    if crop == 256 and pool._grid is not None:
        return pool._grid
    win = grid_windows(pool.hw_host, crop)
    xs, labs, keep = [], [], []
    for s in range(0, len(win), chunk):
        w = win[s:s + chunk]
        inv = np.zeros((len(w), 6), np.float64)
        inv[:, 0] = inv[:, 4] = 1.0
        inv[:, 2], inv[:, 5] = w[:, 2], w[:, 1]
        x, lab, _status = ops.warp_affine_pool(pool.pool_u8, pool.pool_lab, pool.px_off, pool.hw, w[:, 0], inv, (crop, crop),
                                               label_fill=-100)
        k = (lab != -100).flatten(1).any(1)
        xs.append(x[k].to(torch.uint8).permute(0, 2, 3, 1).contiguous())
        labs.append(lab[k])
        keep.append(k.cpu().numpy())
    res = (torch.cat(xs), torch.cat(labs), win[np.concatenate(keep)])
    if crop == 256:
        pool._grid = res
    return res


def grid_flow_targets(pool: ImagePool, crop: int = 256, chunk: int = 64) -> torch.Tensor:
    """The flow-head targets of the windows ``grid_crops`` keeps, float32 (M, 3, crop, crop) on the device: plain windows of the
    pool's stored planes, cut by ``ops.warp_flow_targets`` with integer-translation maps and the identity vector matrix, so every
    value is exact; beyond the image mask and flows are 0.  Cached on the pool for the default crop."""
    if pool.pool_tgt is None:
        raise ValueError("grid_flow_targets: the pool was built without instances")
    if crop == 256 and pool._grid_tgt is not None:
        return pool._grid_tgt
    win = grid_crops(pool, crop, chunk)[2]
    outs = []
    for s in range(0, len(win), chunk):
        w = win[s:s + chunk]
        inv = identity_maps(len(w))
        inv[:, 2], inv[:, 5] = w[:, 2], w[:, 1]
        outs.append(ops.warp_flow_targets(pool.pool_tgt, pool.px_off, pool.hw, w[:, 0], inv, identity_vecs(len(w)), (crop, crop))[0])
    res = torch.cat(outs)
    if crop == 256:
        pool._grid_tgt = res
    return res


FLOW_WS_LIMIT = 1 << 30         # bytes of post-processing workspace per ``ops.masks_to_flows`` call: larger groups run in chunks


def renumber_instances(inst) -> np.ndarray:
    """An integer instance map with arbitrary non-negative ids -> int32 with the ids compact in 1..n in ascending order of the old
    ids, 0 stays the background (what ``fastremap.renumber`` gives the reference, up to the order).  Host, once per image."""
    inst = np.asarray(inst)
    if inst.ndim != 2 or not np.issubdtype(inst.dtype, np.integer):
        raise ValueError(f"instance maps must be 2-D integer arrays, got {inst.shape} {inst.dtype}")
    if inst.size and inst.min() < 0:
        raise ValueError("instance ids must be non-negative (0 = background)")
    u, inverse = np.unique(inst, return_inverse=True)
    inverse = inverse.reshape(inst.shape)
    return (inverse if len(u) and u[0] == 0 else inverse + 1).astype(np.int32)


def flow_targets_of(instances, device="cuda:0", ws_limit: int = FLOW_WS_LIMIT) -> list:
    """The flow-head targets of whole instance maps, once per data set: per map a float32 device tensor (3, h, w) = (mask, flow Y,
    flow X) -- cellpose ``dynamics.labels_to_flows`` restated: the mask plane is ``instances > 0``, the flows those of
    ``ops.masks_to_flows`` on the WHOLE image (its iteration count depends on the whole image, as in the reference).  Ids are
    renumbered on the host, maps of one shape go to the device together, in chunks whose workspace stays below ``ws_limit``."""
    from . import _lib
    dev = torch.device(device)
    maps = [renumber_instances(m) for m in instances]
    out = [None] * len(maps)
    by_shape: dict = {}
    for i, m in enumerate(maps):
        by_shape.setdefault(m.shape, []).append(i)
    L = _lib.lib()
    for (h, w), ids in by_shape.items():
        if h < 2 or w < 2:
            raise ValueError(f"flow targets: an instance map of {h} x {w} is too small")
        per = max(1, L.cpx_postproc_workspace_bytes(1, h, w))
        chunk = int(max(1, min(len(ids), ws_limit // per)))
        for s in range(0, len(ids), chunk):
            part = ids[s:s + chunk]
            m = torch.from_numpy(np.stack([maps[i] for i in part])).to(dev)
            flows = ops.masks_to_flows(m)
            tgt = torch.cat([(m > 0).to(torch.float32)[:, None], flows], 1)
            for k, i in enumerate(part):
                out[i] = tgt[k].contiguous()
        for k in {chunk, len(ids) % chunk}:                              # one-off: do not keep the workspaces of whole images
            ops._ws_cache.pop(("pp", k, h, w, str(dev)), None)
    return out
