"""Mint the stain-perturbation fixture from the REFERENCE's own H&E stain augmentation (run in the build container only).

    python tests/golden/make_golden_stain.py      # rewrites tests/golden/reference_stain.npz / .json

``classpose.transforms.he_staining`` is imported under the stub finder of make_golden.py, with scikit-learn's NMF as installed.
Frozen: ``rgb_to_density`` of an image that holds every byte, and on 8 uint8 patches the tissue mask, the rows ``extract_stains`` handed to ``NMF.fit`` (the class is
wrapped to remember them), ``H`` and the stains it returned, and the output of ``augment_stains`` under a legacy ``RandomState``
that logs its draws.  OpenCV is not installed: the stub ``cv2.cvtColor`` is given the restated lightness (the documented float
formula, D65 luminance, L * 2.55 rounded to 8 bits; ``classpose_amd.stain.lightness_u8``), and the .json says so.  The script
asserts that no output value has ``255 * exp(-x)`` within 1e-9 of an integer in the float64 restatement of
tests/stain_reference.py, so the fixture can be demanded exactly of any float64 implementation -- but for the values that are 255
because both stains were clamped to zero from well below it (x is then exactly 0 in every evaluation; counted per case as
``exactly_255``).  The fixture holds data only.
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


class LoggingRandomState:
    """Stands in for the legacy RandomState that HEStainingTransform hands to augment_stains: the same draws, remembered."""

    def __init__(self, seed):
        self.rng, self.draws = np.random.RandomState(seed), []

    def uniform(self, low, high, size):
        v = self.rng.uniform(low, high, size)
        self.draws.append(np.array(v))
        return v


def main():
    import make_golden
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REF)
    import cv2
    import sklearn
    import stain_reference as sr
    from classpose_amd import stain
    from classpose.transforms import he_staining as rhe
    from classpose.transforms.augmentation_configs import ENHANCED_CONFIG

    def cvt_color(x, code):
        assert code is cv2.COLOR_RGB2LAB and x.dtype == np.uint8
        return np.stack([stain.lightness_u8(x), np.zeros(x.shape[:2], np.uint8), np.zeros(x.shape[:2], np.uint8)], -1)
    cv2.cvtColor = cvt_color

    fitted = []

    class LoggingNMF(rhe.NMF):
        def fit(self, X, y=None, **kw):
            fitted.append(np.array(X))
            return super().fit(X, y, **kw)
    rhe.NMF = LoggingNMF

    cfg = ENHANCED_CONFIG["he_staining_config"]
    rng = np.random.default_rng(20261018)
    true_basis = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])

    def tissue(h, w, strength, noise=4.0):
        """an H&E-like patch: two low-frequency concentration fields rendered through a stain basis, plus pixel noise"""
        coarse = rng.random((h // 8 + 2, w // 8 + 2, 2))
        conc = np.kron(coarse, np.ones((8, 8, 1)))[:h, :w] * strength
        return np.clip(255 * np.exp(-(conc @ true_basis)) + rng.normal(0, noise, (h, w, 3)), 0, 255).astype(np.uint8)

    def background(h, w):
        return np.clip(243 + rng.normal(0, 4, (h, w, 3)), 0, 255).astype(np.uint8)

    def few(h, w):
        x = background(h, w)
        x[20:30, 31:41] = tissue(10, 10, 2.0)          # 100 pixels of tissue at the most
        return x

    def extremes(h, w):
        x = tissue(h, w, 1.8)
        x[rng.random((h, w)) < 0.03] = 0
        x[rng.random((h, w)) < 0.03] = 255
        x[5, 7] = (0, 255, 0)
        return x

    specs = [
        dict(name="tissue_a", make=lambda: tissue(64, 80, 1.5)),
        dict(name="tissue_b", make=lambda: tissue(72, 64, 2.5)),
        dict(name="tissue_pale", make=lambda: tissue(96, 64, 0.9)),
        dict(name="tissue_dark", make=lambda: tissue(64, 96, 3.5, 2.0)),
        dict(name="tissue_odd", make=lambda: tissue(71, 83, 2.0)),
        dict(name="all_background", make=lambda: background(64, 64)),
        dict(name="few_tissue_pixels", make=lambda: few(80, 72)),
        dict(name="zeros_and_255s", make=lambda: extremes(64, 64)),
    ]
    meta = {"cvtColor": "RESTATED: OpenCV is not installed; the one call cv2.cvtColor(x, COLOR_RGB2LAB) of rgb_to_lab ran the "
                        "documented float formula (sRGB linearisation, Y = 0.212671 R + 0.715160 G + 0.072169 B, L = 116 cbrt(Y) - 16 "
                        "or 903.3 Y, L * 2.55 rounded to 8 bits), not the wheel, whose 8-bit path is table-driven and may differ "
                        "where L rounds to 199 or 200.  Only channel 0 is used.",
            "config": dict(cfg), "window": sr.WINDOW, "numpy": np.__version__, "sklearn": sklearn.__version__, "cases": []}
    # rgb_to_density is a function of the byte: frozen once on an image that holds every byte, not per patch
    every_byte = np.repeat(np.arange(256, dtype=np.uint8).reshape(16, 16, 1), 3, axis=2)
    arrays = {"every_byte_in": every_byte, "every_byte_density": rhe.rgb_to_density(every_byte)}
    for i, s in enumerate(specs):
        patch = s["make"]()
        name = s["name"]
        mask = rhe.rgb_to_lab(patch)[..., 0] < 200
        del fitted[:]
        H, stains = rhe.extract_stains(patch)
        assert len(fitted) == 1
        fit_rows = fitted[0]
        log = LoggingRandomState(3000 + i)
        out = rhe.augment_stains(patch.copy(), amount_matrix=cfg["amount_matrix"], amount_stains=cfg["amount_stains"], rng=log)
        assert out.dtype == np.uint8 and len(log.draws) == 2 and np.all(np.isfinite(H))
        U, u = log.draws[0].reshape(2, 3), log.draws[1].reshape(2)
        # the float64 restatement gives these bytes, and none of its values sits in the window: the fixture can be demanded exactly
        params = stain.stain_params(H, np.linalg.pinv(H), U, u, cfg["amount_matrix"], cfg["amount_stains"])
        mine, v64, exact = sr.he_stain(patch, params)
        assert np.array_equal(mine, out), name
        gap = float(np.abs(v64 - np.rint(v64))[~exact].min())
        assert gap > sr.WINDOW and not sr.near_integer(v64, exact).any(), (name, gap)
        for key, val in (("in", patch), ("mask", mask), ("fit_rows", fit_rows), ("H", H),
                         ("stains", stains), ("out", out)):
            arrays[f"{name}_{key}"] = val
        meta["cases"].append(dict(name=name, shape=list(patch.shape[:2]), tissue_pixels=int(mask.sum()), fit_rows=int(len(fit_rows)),
                                  U=U.tolist(), u=u.tolist(), seed=3000 + i, changed=int((out != patch).sum()),
                                  nearest_integer_gap=gap, exactly_255=int(exact.sum())))
        print(name, patch.shape, "tissue", int(mask.sum()), "fit rows", len(fit_rows), "changed", meta["cases"][-1]["changed"],
              "gap %.2e" % gap)
    c = {m["name"]: m for m in meta["cases"]}
    assert c["all_background"]["tissue_pixels"] == 0 and c["all_background"]["fit_rows"] == 32        # all 4096 pixels, [::128]
    assert 0 < c["few_tissue_pixels"]["tissue_pixels"] <= 128 == stain.SUBSAMPLE
    assert c["few_tissue_pixels"]["fit_rows"] == c["few_tissue_pixels"]["tissue_pixels"]
    zin = arrays["zeros_and_255s_in"]
    assert (zin == 0).any() and (zin == 255).any()
    np.savez_compressed(os.path.join(HERE, "reference_stain.npz"), **arrays)
    with open(os.path.join(HERE, "reference_stain.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote reference_stain.npz", os.path.getsize(os.path.join(HERE, "reference_stain.npz")), "bytes")


if __name__ == "__main__":
    main()
