"""Mint the Gaussian-blur fixture from the REFERENCE's own GaussianBlurTransform (run in the build container only).

    python tests/golden/make_golden_quality.py      # rewrites tests/golden/reference_quality.npz / .json

``classpose.transforms.image_quality`` is imported under the stub finder of make_golden.py: scipy is the real package, torchvision
and skimage are stubs.  Every case constructs a ``GaussianBlurTransform`` whose sigma range pins the sigma wanted (a degenerate
range ``(s, s)``) and whose probability is 1, seeds it, and calls ``transform`` on an (H, W, 3) uint8 image with H > 4 (below that
the reference guesses a channel-first layout).  Frozen: the input, the seed, the sigma the transform drew (replayed from the seed)
and the output.  The script asserts that the float64 restatement of tests/quality_reference.py gives the same bytes.
The hue / brightness / saturation transform calls torchvision, which is not installed: it cannot be minted, and the .json says so.
The fixture holds data only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

SIZES = [(5, 7), (8, 8), (17, 16), (37, 53), (64, 96)]
SIGMAS = [0.05, 0.124, 0.126, 0.3, 0.7, 1.3, 1.77, 2.0]         # radius 0, 0, 1, 1, 3, 5, 7, 8


def main():
    import make_golden
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REF)
    import scipy
    import quality_reference as qr
    from classpose.transforms import image_quality as riq
    from classpose.transforms.augmentation_configs import ENHANCED_CONFIG

    rng = np.random.default_rng(20261018)

    def tissue(h, w):
        """low-frequency stain fields rendered through an H&E basis, plus pixel noise"""
        basis = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])
        conc = np.kron(rng.random((h // 8 + 2, w // 8 + 2, 2)), np.ones((8, 8, 1)))[:h, :w] * 2.0
        return np.clip(255 * np.exp(-(conc @ basis)) + rng.normal(0, 4.0, (h, w, 3)), 0, 255).astype(np.uint8)

    images = {}
    for h, w in SIZES:
        images[f"noise_{h}x{w}"] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for h, w in SIZES[2:]:
        images[f"tissue_{h}x{w}"] = tissue(h, w)
    for v in (255, 254, 1):
        images[f"const{v}_17x16"] = np.full((17, 16, 3), v, np.uint8)

    meta = {"hbs": "NOT MINTED: HueBrightnessSaturationTransform._hbs_adjust calls torchvision (adjust_hue, adjust_brightness, "
                   "adjust_saturation), which is not installed; tests/quality_reference.py restates it twice instead (numpy float32 "
                   "and torch tensor operations), unpinned against the wheel.",
            "config": {k: ENHANCED_CONFIG[k] for k in ("gaussian_blur_config", "hbs_config") if k in ENHANCED_CONFIG},
            "numpy": np.__version__, "scipy": scipy.__version__, "cases": []}
    arrays = dict(images)
    seed = 7000
    # every sigma on the small images; the larger ones, whose bytes make up the file, take a spread of radii each
    some = {"noise_37x53": [0.126, 0.7, 1.77, 2.0], "noise_64x96": [1.3, 2.0], "tissue_37x53": [0.7, 1.3], "tissue_64x96": [2.0]}
    for name, img in images.items():
        for sigma in some.get(name, SIGMAS):
            seed += 1
            tr = riq.GaussianBlurTransform(sigma_range=(sigma, sigma), probability=1.0, seed=seed)
            out = tr.transform(img.copy())
            replay = np.random.default_rng(seed)
            replay.random()
            drew = float(replay.uniform(sigma, sigma))
            assert drew == sigma and out.dtype == np.uint8 and out.shape == img.shape
            mine = qr.gaussian_blur(img, drew)
            assert np.array_equal(mine, out), (name, sigma)
            key = f"{name}_s{len(meta['cases'])}"
            arrays[key] = out
            meta["cases"].append(dict(image=name, out=key, seed=seed, sigma=drew, radius=int(4 * drew + 0.5),
                                      changed=int((out != img).sum())))
    const = {(c["image"], c["sigma"]): arrays[c["out"]] for c in meta["cases"]}
    assert np.all(const[("const255_17x16", 1.3)] == 254)           # the weights sum to just under 1 and the casts truncate
    assert {c["radius"] for c in meta["cases"]} >= {0, 1, 3, 5, 7, 8}
    np.savez_compressed(os.path.join(HERE, "reference_quality.npz"), **arrays)
    with open(os.path.join(HERE, "reference_quality.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote reference_quality.npz", os.path.getsize(os.path.join(HERE, "reference_quality.npz")), "bytes,", len(meta["cases"]), "cases")


if __name__ == "__main__":
    main()
