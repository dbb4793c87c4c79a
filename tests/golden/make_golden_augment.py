"""Mint the augmentation fixture from the REFERENCE's own stain transform (run in the build container only).

    python tests/golden/make_golden_augment.py      # rewrites tests/golden/reference_augment.npz / .json

``classpose.transforms.hed`` is imported under the stub finder of make_golden.py.  Frozen: its float32 ``RGB_FROM_HED`` /
``HED_FROM_RGB`` and the outputs of ``HEDTransform.transform`` on small uint8 patches, with the sigma / bias values the transform
drew (it is given a generator that logs its draws).  ``simple_mode=True`` is pure reference arithmetic.  The complex mode calls
``skimage.exposure.rescale_intensity``, which is not installed: the stub module is given the documented formula of that one call
(clip to ``in_range``, then ``(x - imin) / (imax - imin) * (omax - omin) + omin`` with (-1, 1) on both sides, the 'dtype' output
range of a float image), and the .json says so.  The fixture holds data only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)


def rescale_intensity(image, in_range="image", out_range="dtype"):
    """The documented arithmetic of skimage.exposure.rescale_intensity for a float image, in_range a pair, out_range 'dtype'."""
    assert out_range == "dtype" and image.dtype.kind == "f" and tuple(in_range) == (-1, 1)
    imin, imax = in_range
    omin, omax = -1, 1
    image = np.clip(image, imin, imax)
    image = (image - imin) / (imax - imin)
    return (image * (omax - omin) + omin).astype(image.dtype)


class LoggingRng:
    """Stands in for the numpy Generator of HEDTransform: the same draws, remembered."""

    def __init__(self, seed):
        self.rng, self.draws = np.random.default_rng(seed), []

    def uniform(self, low, high):
        v = self.rng.uniform(low=low, high=high)
        self.draws.append(float(v))
        return v


def main():
    import make_golden
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REF)
    import skimage.exposure
    skimage.exposure.rescale_intensity = rescale_intensity
    from classpose.transforms import hed as rhed
    from classpose.transforms.augmentation_configs import HED_ONLY_CONFIG

    cfg = HED_ONLY_CONFIG["hed_config"]
    rng = np.random.default_rng(20261018)
    arrays = {"RGB_FROM_HED": rhed.RGB_FROM_HED, "HED_FROM_RGB": rhed.HED_FROM_RGB}
    assert rhed.RGB_FROM_HED.dtype == np.float32 and rhed.HED_FROM_RGB.dtype == np.float32

    def smooth(h, w, lo, hi):
        """a tissue-like patch: low-frequency colour field plus pixel noise, spanning [lo, hi]"""
        coarse = rng.random((h // 8 + 2, w // 8 + 2, 3))
        field = np.kron(coarse, np.ones((8, 8, 1)))[:h, :w]
        v = 0.7 * field + 0.3 * rng.random((h, w, 3))
        return np.clip(lo + (hi - lo) * v, 0, 255).astype(np.uint8)

    specs = [
        dict(name="mid_complex", h=64, w=80, lo=0, hi=255, simple=False),
        dict(name="mid_simple", h=72, w=64, lo=0, hi=255, simple=True),
        dict(name="pink_complex", h=96, w=64, lo=90, hi=250, simple=False),
        dict(name="pink_simple", h=64, w=96, lo=90, hi=250, simple=True),
        dict(name="dark_below_cutoff", h=64, w=64, lo=0, hi=60, simple=False),
        dict(name="bright_above_cutoff", h=80, w=72, lo=225, hi=255, simple=False),
        dict(name="extremes_complex", h=64, w=64, lo=-40, hi=300, simple=False),
        dict(name="extremes_simple", h=64, w=64, lo=-40, hi=300, simple=True),
    ]
    meta = {"rescale_intensity": "RESTATED: skimage is not installed; the one call rescale_intensity(x, in_range=(-1, 1)) of "
                                 "combine_stains ran the documented formula clip(x, -1, 1), (x + 1) / 2 * 2 - 1 in the image's "
                                 "float32, not the wheel.  simple_mode=True cases do not reach it.",
            "config": {"sigma_ranges": [list(r) for r in cfg["sigma_ranges"]], "bias_ranges": [list(r) for r in cfg["bias_ranges"]],
                       "cutoff_range": list(cfg["cutoff_range"])},
            "numpy": np.__version__, "cases": []}
    for i, s in enumerate(specs):
        patch = smooth(s["h"], s["w"], s["lo"], s["hi"])
        log = LoggingRng(1000 + i)
        t = rhed.HEDTransform(sigma_ranges=cfg["sigma_ranges"], bias_ranges=cfg["bias_ranges"], cutoff_range=cfg["cutoff_range"],
                              seed=log, channel_dimension=2, simple_mode=s["simple"])
        out = t.transform(patch.copy())
        applied = len(log.draws) == 6
        if applied:
            assert out.dtype == np.uint8
            sigma, bias = log.draws[:3], log.draws[3:]
        else:
            assert not log.draws and out is not None
            out = patch.copy()                     # the reference returns patch / 255.0 untouched: the pixels are the input's
            sigma, bias = [0.0] * 3, [0.0] * 3
        arrays[s["name"] + "_in"], arrays[s["name"] + "_out"] = patch, out
        meta["cases"].append(dict(name=s["name"], simple_mode=s["simple"], applied=applied, sigma=sigma, bias=bias,
                                  mean=float(np.mean(patch) / 255.0), changed=int((out != patch).sum())))
        print(s["name"], "applied", applied, "mean %.3f" % meta["cases"][-1]["mean"], "changed", meta["cases"][-1]["changed"])
    assert sum(not c["applied"] for c in meta["cases"]) == 2
    np.savez_compressed(os.path.join(HERE, "reference_augment.npz"), **arrays)
    with open(os.path.join(HERE, "reference_augment.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote reference_augment.npz", os.path.getsize(os.path.join(HERE, "reference_augment.npz")), "bytes")


if __name__ == "__main__":
    main()
