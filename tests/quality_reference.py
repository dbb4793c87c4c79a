"""Restatements of the reference's image-quality augmentation (transforms/image_quality.py), the yardsticks of the quality tests:

* ``gaussian_blur``: ``scipy.ndimage.gaussian_filter(plane, sigma)`` per channel on uint8, in numpy float64 in scipy's own order;
* ``hbs_numpy``: ``_hbs_adjust`` (torchvision's adjust_hue / adjust_brightness / adjust_saturation) in numpy float32, one rounding
  per operation -- where torchvision calls ``add_(other, alpha=)`` (the grey value and the saturation blend) that operation is
  ATen's ``fmadd``, ONE rounding of ``a + alpha * other`` (``fma32``);
* ``hbs_torch``: the same with the tensor operations torchvision's ``transforms/v2/functional/_color.py`` uses.

torchvision is not installed where these were written: the two HBS formulations are stated from its source as known and are
unpinned against the wheel.  The layout is always (H, W, 3).
"""
from __future__ import annotations

import numpy as np

F = np.float32


def gauss_kernel(sigma: float):
    """(radius, weights (2 radius + 1,) float64) with scipy's defaults (truncate 4)."""
    radius = int(4.0 * float(sigma) + 0.5)
    x = np.arange(-radius, radius + 1)
    phi = np.exp(-0.5 / (float(sigma) * float(sigma)) * x ** 2) if radius else np.ones(1)
    return radius, phi / phi.sum()


def reflect(p, n: int):
    """scipy's `reflect` (d c b a | a b c d | d c b a), for any distance beyond the border."""
    m = np.mod(p, 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _pass(x_u8: np.ndarray, w: np.ndarray, r: int, axis: int) -> np.ndarray:
    """One correlate1d pass along ``axis`` of a (H, W) uint8 plane: double accumulation from the outermost pair inwards (scipy's
    symmetric branch), the result cast to uint8 by truncation."""
    x = np.moveaxis(x_u8, axis, 0).astype(np.float64)
    n = x.shape[0]
    c = np.arange(n)
    acc = x[c] * w[r]
    for k in range(r, 0, -1):
        acc = acc + (x[reflect(c - k, n)] + x[reflect(c + k, n)]) * w[r - k]
    return np.moveaxis(acc.astype(np.uint8), 0, axis)


def gaussian_blur(img_u8: np.ndarray, sigma: float) -> np.ndarray:
    """``gaussian_filter(img[..., c], sigma)`` for each channel of a (H, W, 3) uint8 image: axis 0 first, then axis 1."""
    r, w = gauss_kernel(sigma)
    out = np.empty_like(img_u8)
    for c in range(img_u8.shape[2]):
        out[..., c] = _pass(_pass(img_u8[..., c], w, r, 0), w, r, 1)
    return out


def fma32(a, b, c):
    """float32 ``a * b + c`` with one rounding.  The product of two float32 is exact in double; the sum in double is rounded once
    more on the way to float32, which differs from the single rounding only where the double sum lands exactly half way between
    two float32 values while the exact sum does not -- the error term of the double sum (TwoSum) then says which way."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    r = s.astype(F)
    tie = (err != 0) & (np.abs(s - r.astype(np.float64)) * 2 == np.abs(np.spacing(r).astype(np.float64)))
    if np.any(tie):
        s = np.where(tie, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        r = s.astype(F)
    return r


def hbs_values(hue: float, brightness: float, saturation: float) -> np.ndarray:
    """float32 {hue, brightness, saturation, 1 - saturation}: the last is formed in double before it is rounded."""
    return np.array([hue, brightness, saturation, 1.0 - float(saturation)], np.float64).astype(F)


def hbs_numpy(img_u8: np.ndarray, hue: float, brightness: float, saturation: float) -> np.ndarray:
    """``_hbs_adjust`` on (..., 3) uint8 in numpy float32.  ``brightness`` is the factor (1 + the draw)."""
    hue_f, br_f, sat_f, oms_f = hbs_values(hue, brightness, saturation)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (np.arange(256, dtype=F) / F(255))[img_u8]
        r, g, b = x[..., 0], x[..., 1], x[..., 2]
        if hue_f != 0:
            maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
            eq = maxc == minc
            cr = maxc - minc
            s = cr / np.where(eq, F(1), maxc)
            d = np.where(eq, F(1), cr)
            rc, gc, bc = (maxc - r) / d, (maxc - g) / d, (maxc - b) / d
            hr = np.where(maxc == r, bc - gc, F(0))
            hg = np.where((maxc == g) & (maxc != r), (rc + F(2)) - bc, F(0))
            hb = np.where((maxc != g) & (maxc != r), (gc + F(4)) - rc, F(0))
            h = np.fmod(((hr + hg) + hb) * F(1.0 / 6.0) + F(1), F(1))
            h = np.fmod(h + hue_f, F(1))
            h = np.where(h < 0, h + F(1), h)                                # remainder with the divisor's sign
            h6 = h * F(6)
            fl = np.floor(h6)
            f = h6 - fl
            i = fl.astype(np.int32) % 6
            v, sxf, oms = maxc, s * f, F(1) - s
            q = np.clip((F(1) - sxf) * v, F(0), F(1))
            t = np.clip((sxf + oms) * v, F(0), F(1))
            p = np.clip(oms * v, F(0), F(1))
            r = np.choose(i, [v, q, p, p, t, v])
            g = np.choose(i, [t, v, v, q, p, p])
            b = np.choose(i, [p, p, t, v, v, q])
        r, g, b = (np.clip(c * br_f, F(0), F(1)) for c in (r, g, b))
        if sat_f != 1:
            gray = fma32(b, F(0.114), fma32(g, F(0.587), r * F(0.2989)))
            r, g, b = (np.clip(fma32(gray, oms_f, c * sat_f), F(0), F(1)) for c in (r, g, b))
        out = np.stack([r, g, b], -1)
        assert out.dtype == F
        return np.clip(out * F(255), 0, 255).astype(np.uint8)


def hbs_torch(img_u8: np.ndarray, hue: float, brightness: float, saturation: float) -> np.ndarray:
    """The same on the CPU with the tensor operations of torchvision's v2 functional colour code, channel first as ``_hbs_adjust``
    hands the image over.  Its agreement with ``hbs_numpy`` rests on ATen's ``add_(other, alpha=)`` being a fused multiply-add on
    the CPU that runs it (torch 2.10.0 on x86-64 with FMA: observed, also for a single element).  On a torch build or a CPU
    without FMA that operation rounds twice (``a + alpha * b``), and the two formulations would then differ in a few bytes per ten
    million (3 of 11.3 million on ``hbs_inputs`` with ``HBS_SETS``, all where a hue shift precedes the saturation blend)."""
    import torch
    hue_f, br_f, sat_f, oms_f = (float(v) for v in hbs_values(hue, brightness, saturation))
    flat = np.ascontiguousarray(img_u8).reshape(-1, 1, 3)
    image = torch.as_tensor(np.transpose(flat, (2, 0, 1)).copy(), dtype=torch.float32) / 255.0
    if hue_f != 0:
        r, g, _ = image.unbind(dim=-3)
        minc, maxc = torch.aminmax(image, dim=-3)
        eqc = maxc == minc
        channels_range = maxc - minc
        ones = torch.ones_like(maxc)
        s = channels_range / torch.where(eqc, ones, maxc)
        divisor = torch.where(eqc, ones, channels_range).unsqueeze_(dim=-3)
        rc, gc, bc = ((maxc.unsqueeze(dim=-3) - image) / divisor).unbind(dim=-3)
        mask_maxc_neq_r = maxc != r
        mask_maxc_eq_g = maxc == g
        hg = rc.add(2.0).sub_(bc).mul_(mask_maxc_eq_g & mask_maxc_neq_r)
        hr = bc.sub_(gc).mul_(~mask_maxc_neq_r)
        hb = gc.add_(4.0).sub_(rc).mul_(mask_maxc_neq_r.logical_and_(mask_maxc_eq_g.logical_not_()))
        h = hr.add_(hg).add_(hb)
        h = h.mul_(1.0 / 6.0).add_(1.0).fmod_(1.0)
        h = h.add_(hue_f).remainder_(1.0)
        h6 = h.mul(6.0)
        i = torch.floor(h6)
        f = h6.sub_(i)
        i = i.to(dtype=torch.int32)
        v = maxc
        sxf = s * f
        one_minus_s = 1.0 - s
        q = (1.0 - sxf).mul_(v).clamp_(0.0, 1.0)
        t = sxf.add_(one_minus_s).mul_(v).clamp_(0.0, 1.0)
        p = one_minus_s.mul_(v).clamp_(0.0, 1.0)
        i.remainder_(6)
        vpqt = torch.stack((v, p, q, t), dim=-3)
        select = torch.tensor([[0, 2, 1, 1, 3, 0], [3, 0, 0, 2, 1, 1], [1, 1, 3, 0, 0, 2]], dtype=torch.long)
        select = select[:, i.to(torch.long)]
        image = vpqt.gather(-3, select)
    image = image.mul(br_f).clamp_(0, 1.0)
    if sat_f != 1:
        r, g, b = image.unbind(dim=-3)
        gray = r.mul(0.2989).add_(g, alpha=0.587).add_(b, alpha=0.114).unsqueeze(dim=-3)
        # float32(1 - saturation) formed in double on the host: alpha is that float32 value
        image = image.mul(sat_f).add_(gray.expand_as(image), alpha=oms_f).clamp_(0, 1.0)
    result = np.transpose(image.numpy(), (1, 2, 0))
    out = np.clip(result * 255, 0, 255).astype(np.uint8)
    return out.reshape(img_u8.shape)


# eight parameter sets {hue, brightness factor, saturation}: the neutral ones, the ends of the hue range, and mixtures
HBS_SETS = [(0.0, 1.0, 1.0), (0.1, 1.0, 1.0), (-0.1, 1.0, 1.0), (0.0, 1.1, 1.0), (0.0, 1.0, 0.9), (0.0371, 0.93, 1.07),
            (-0.0912, 1.0999, 0.9001), (0.1, 0.9, 1.1)]


def hbs_inputs(seed: int = 5) -> np.ndarray:
    """(m, 3) uint8: a lattice of the colour cube with stride 5 at three offsets, all greys, primaries and ties, random colours."""
    rng = np.random.default_rng(seed)
    parts = []
    for o in (0, 2, 4):
        v = np.arange(o, 256, 5, dtype=np.uint8)
        parts.append(np.stack(np.meshgrid(v, v, v, indexing="ij"), -1).reshape(-1, 3))
    grey = np.arange(256, dtype=np.uint8)
    parts.append(np.stack([grey, grey, grey], -1))
    ties = [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255),
            (200, 200, 10), (10, 200, 200), (200, 10, 200), (1, 1, 0), (0, 1, 1), (1, 0, 1), (254, 255, 255), (255, 254, 254)]
    parts.append(np.array(ties, np.uint8))
    a = np.arange(256, dtype=np.uint8)
    parts.append(np.stack([a, a, a[::-1]], -1))                             # r == g rows
    parts.append(np.stack([a, a[::-1], a[::-1]], -1))                       # g == b rows
    parts.append(rng.integers(0, 256, (256 * 256, 3), dtype=np.uint8))
    return np.concatenate(parts)
