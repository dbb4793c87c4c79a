"""Host side of the image-quality augmentation (classpose_amd.augment "quality" / "hed_he_quality"): the float64
restatement of the blur against the reference-minted fixture tests/golden/reference_quality.npz and against scipy, the two
restatements of the hue / brightness / saturation jitter against each other, the samplers and their draw order, the footprint
rectangle, the declarations and the CLI flags.  No GPU."""
from __future__ import annotations

import json
import os
import re
import subprocess

import numpy as np
import pytest

import quality_reference as qr
from classpose_amd import _lib, augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fixture():
    with open(os.path.join(GOLD, "reference_quality.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_quality.npz")), meta


def _unhex(values, dtype=np.float64):
    return np.array([float.fromhex(v) for v in values], dtype)


def test_the_fixture_covers_what_it_should():
    npz, meta = _fixture()
    assert os.path.getsize(os.path.join(GOLD, "reference_quality.npz")) <= 200 * 1024
    assert "NOT MINTED" in meta["hbs"] and "torchvision" in meta["hbs"]
    shapes = {tuple(npz[c["image"]].shape[:2]) for c in meta["cases"]}
    assert shapes == {(5, 7), (8, 8), (17, 16), (37, 53), (64, 96)} and all(h > 4 for h, _w in shapes)
    assert {c["radius"] for c in meta["cases"]} >= {0, 1, 3, 5, 7, 8}
    assert {c["image"].split("_")[0] for c in meta["cases"]} == {"noise", "tissue", "const255", "const254", "const1"}
    cfg = augment.AUGMENT_CONFIGS["hed_he_quality"]
    assert list(cfg["gaussian_blur"]["sigma_range"]) == meta["config"]["gaussian_blur_config"]["sigma_range"]
    assert cfg["gaussian_blur"]["probability"] == meta["config"]["gaussian_blur_config"]["probability"] == 0.1
    assert {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg["hbs"].items()} == meta["config"]["hbs_config"]
    assert augment.AUGMENT_CONFIGS["quality"]["hbs"] == cfg["hbs"] and augment.AUGMENT_CONFIGS["quality"]["gaussian_blur"] == cfg["gaussian_blur"]
    hed_he = augment.AUGMENT_CONFIGS["hed_he"]
    assert all(cfg[k] == hed_he[k] for k in hed_he) and "sigma_ranges" not in augment.AUGMENT_CONFIGS["quality"]
    assert "he_staining" not in augment.AUGMENT_CONFIGS["quality"]


def test_blur_restatement_equals_the_fixture_exactly():
    npz, meta = _fixture()
    for c in meta["cases"]:
        img, want = npz[c["image"]], npz[c["out"]]
        # the sigma is the one the seeded transform drew
        r = np.random.default_rng(c["seed"])
        r.random()
        assert float(r.uniform(c["sigma"], c["sigma"])) == c["sigma"]
        got = qr.gaussian_blur(img, c["sigma"])
        assert np.array_equal(got, want), (c["image"], c["sigma"])
        radius, w = augment.gauss_weights(c["sigma"])
        kr, kw = qr.gauss_kernel(c["sigma"])
        assert radius == kr == c["radius"] and np.array_equal(w[:2 * radius + 1], kw) and not w[2 * radius + 1:].any()
        if radius == 0:
            assert np.array_equal(want, img) and c["changed"] == 0
    by = {(c["image"], c["sigma"]): npz[c["out"]] for c in meta["cases"]}
    assert np.all(by[("const255_17x16", 1.3)] == 254)


def test_blur_restatement_equals_scipy_live():
    ndi = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(3)
    differ = 0
    for shape in [(1, 1), (3, 5), (8, 8), (17, 16), (37, 53), (65, 65)]:
        img = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
        for sigma in (0.05, 0.124, 0.126, 0.7, 1.3, 1.77, 2.0):
            want = np.stack([ndi.gaussian_filter(img[..., c], sigma) for c in range(3)], -1)
            differ += int((qr.gaussian_blur(img, sigma) != want).sum())
            from scipy.ndimage._filters import _gaussian_kernel1d
            radius, w = augment.gauss_weights(sigma)
            assert np.array_equal(w[:2 * radius + 1], _gaussian_kernel1d(sigma, 0, radius))
    c255 = np.full((9, 11, 3), 255, np.uint8)
    assert np.all(ndi.gaussian_filter(c255[..., 0], 1.3) == 254) and np.all(qr.gaussian_blur(c255, 1.3) == 254)
    print(f"bytes that differ from scipy.ndimage.gaussian_filter: {differ}")
    assert differ == 0
    with pytest.raises(ValueError):
        augment.gauss_weights(2.2)


def test_the_two_hbs_formulations_agree_byte_for_byte():
    x = qr.hbs_inputs()
    assert len(qr.HBS_SETS) == 8 and len(x) > 256 * 256
    for ps in qr.HBS_SETS:
        a, b = qr.hbs_numpy(x, *ps), qr.hbs_torch(x, *ps)
        differ = int((a != b).sum())
        print(f"hue {ps[0]:+.4f} brightness {ps[1]:.4f} saturation {ps[2]:.4f}: {differ} bytes differ, {int((a != x).sum())} changed")
        assert differ == 0, ps
        if ps == (0.0, 1.0, 1.0):
            assert np.array_equal(a, x)                                   # neutral parameters return the input
        else:
            assert (a != x).any()
    # the 256 x 256 x 3 layout gives what the flat one gives
    img = x[-256 * 256:].reshape(256, 256, 3)
    assert np.array_equal(qr.hbs_numpy(img, 0.05, 1.05, 0.95).reshape(-1, 3), qr.hbs_numpy(x[-256 * 256:], 0.05, 1.05, 0.95))


def test_fma32_is_one_rounding():
    from fractions import Fraction
    rng = np.random.default_rng(9)
    a, b, c = (rng.random(2000).astype(np.float32) for _ in range(3))
    c[:500] *= np.float32(1e-4)
    got = qr.fma32(a, b, c)
    for i in range(0, 2000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))                                       # Python rounds a Fraction to double correctly ...
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: abs(Fraction(float(v)) - exact))   # ... so the nearest float32 is one of these three
        assert got[i] == best


def test_additive_noise_is_an_identity_on_uint8():
    noise = np.random.default_rng(0).normal(0, 0.01, (64, 64, 3)).astype(np.uint8)
    assert not noise.any()


def test_draw_order_of_the_new_configurations_is_frozen():
    n = 300
    for name in ("quality", "hed_he_quality"):
        cfg = augment.get_config(name)
        p = augment.sample_batch_params(np.random.default_rng(11), n, 300, 280, cfg, 0.5)
        r = np.random.default_rng(11)
        if name == "hed_he_quality":
            assert np.array_equal(p.use_hed, r.random(n) < 0.5)
            s, b = augment.sample_hed(r, n, cfg["sigma_ranges"], cfg["bias_ranges"])
            assert np.array_equal(p.sigma, s) and np.array_equal(p.bias, b)
            gate, U, u = augment.sample_he(r, n)
            assert np.array_equal(p.he_gate, gate) and np.array_equal(p.he_matrix, U) and np.array_equal(p.he_stains, u)
        else:
            assert p.use_hed is None and p.sigma is None and p.he_gate is None
        assert np.array_equal(p.blur_gate, r.random(n)) and np.array_equal(p.blur_sigma, r.uniform(0, 2, n))
        assert np.array_equal(p.hbs_gate, r.random(n)) and np.array_equal(p.hbs_hue, r.uniform(-0.1, 0.1, n))
        assert np.array_equal(p.hbs_brightness, r.uniform(-0.1, 0.1, n)) and np.array_equal(p.hbs_saturation, r.uniform(0.9, 1.1, n))
        flip, inv = augment.sample_affine(r, n, 300, 280, 256, 0.5)
        assert np.array_equal(p.flip, flip) and np.array_equal(p.inv, inv)
        blurred, radius, weights, hbs, apply = augment.quality_params(p, cfg)
        gated = p.blur_gate <= 0.1
        assert np.array_equal(blurred, gated & (p.blur_sigma >= 0.125)) and 10 <= gated.sum() <= 55
        assert np.array_equal(apply, (p.hbs_gate <= 0.9).astype(np.int32)) and 0.8 < apply.mean() < 0.97
        t = int(np.flatnonzero(blurred)[0])
        assert radius[t] == int(4 * p.blur_sigma[t] + 0.5) and np.array_equal(weights[t], augment.gauss_weights(p.blur_sigma[t])[1])
        assert not radius[~gated].any() and np.all(weights[~gated, 0] == 1) and not weights[~gated, 1:].any()
        assert hbs.dtype == np.float32 and hbs.shape == (n, 4)
        assert np.array_equal(hbs[t], qr.hbs_values(p.hbs_hue[t], 1.0 + p.hbs_brightness[t], p.hbs_saturation[t]))
    # frozen values
    frozen = {
        "quality": (321, dict(
            blur_gate=['0x1.5149de48c2533p-1', '0x1.d10dcb0841c0bp-1', '0x1.ef0a750a9abd4p-2'],
            blur_sigma=['0x1.7368f618be500p+0', '0x1.1c99395eef419p+0', '0x1.cd1832bb0eaadp+0'],
            hbs_gate=['0x1.5dafa1265267bp-1', '0x1.80e7a8861d5f8p-3', '0x1.78357b9ebd964p-2'],
            hbs_hue=['0x1.7a6efe0039c3cp-4', '0x1.7773b9d2472a2p-4', '-0x1.7a05ab32175c8p-6'],
            hbs_brightness=['0x1.c2603089656c8p-5', '-0x1.303bfa3ea3dd8p-6', '0x1.412abf9d22492p-4'],
            hbs_saturation=['0x1.1489d0871b80ap+0', '0x1.dd5c46bb13fbbp-1', '0x1.15a9d52781660p+0']),
            ['-0x1.48810e7754466p-3', '-0x1.930562d42af0cp-1', '0x1.bd36f77a329b5p+7', '-0x1.930562d42af0cp-1', '0x1.48810e7754466p-3',
             '0x1.f220b9a9ef670p+7'], [True, False, False]),
        "hed_he_quality": (322, dict(
            blur_gate=['0x1.51f2cbfc8733fp-1', '0x1.ea010ffc73f4cp-1', '0x1.1c8f0e95264e9p-1'],
            blur_sigma=['0x1.98de58796093ap+0', '0x1.58f8064cb1eebp+0', '0x1.b5fe8c4dc8350p-3'],
            hbs_gate=['0x1.12fb17518aad5p-1', '0x1.9ca2ea0f63190p-1', '0x1.41e73a54064c8p-4'],
            hbs_hue=['0x1.2b62a17a845d0p-8', '0x1.5658ddcdd8f00p-11', '0x1.a6d30330b1ab0p-6'],
            hbs_brightness=['-0x1.684f4fe631ee7p-4', '-0x1.3a2198916c6bdp-5', '0x1.6579d60d432a8p-5'],
            hbs_saturation=['0x1.0c0c4d10dafe1p+0', '0x1.e4f409ac451b3p-1', '0x1.16757238bbcb7p+0']),
            ['0x1.0c7568a49c459p-5', '-0x1.15891a8759ad4p+0', '0x1.11dbb077ed8d3p+8', '0x1.15891a8759ad4p+0', '0x1.0c7568a49c459p-5',
             '0x1.a6dc08ac26200p+2'], [False, True, False]),
    }
    for name, (seed, fields, inv0, flip) in frozen.items():
        p = augment.sample_batch_params(np.random.default_rng(seed), 3, [300, 256, 301], [280, 256, 299], augment.get_config(name), 0.5,
                                        True, 256, np.array([1.0, 1.25, 0.8]))
        for f, v in fields.items():
            assert np.array_equal(getattr(p, f), _unhex(v)), (name, f)
        assert np.array_equal(p.inv[0], _unhex(inv0)) and p.flip.tolist() == flip
    p = augment.sample_batch_params(np.random.default_rng(322), 3, [300, 256, 301], [280, 256, 299], augment.get_config("hed_he_quality"),
                                    0.5, True, 256, np.array([1.0, 1.25, 0.8]))
    assert np.array_equal(p.sigma[0], _unhex(['-0x1.ea48320000000p-4', '0x1.4031820000000p-5', '-0x1.3ecff80000000p-3'], np.float32))
    assert np.array_equal(p.he_gate, _unhex(['0x1.b186a9fdb2331p-1', '0x1.c8bbbbf0430a8p-4', '0x1.2a164b7cb7556p-2']))
    # the older configurations carry no quality draws: their streams are what they were
    q = augment.sample_batch_params(np.random.default_rng(5), 4, 300, 280, augment.get_config("hed_he"), 0.5)
    assert q.blur_gate is None and q.hbs_saturation is None


def test_footprint_rectangle_contains_every_in_image_tap():
    rng = np.random.default_rng(17)
    n, out = 200, 16
    sh, sw = rng.integers(1, 60, n), rng.integers(1, 60, n)
    flip, inv = augment.sample_affine(rng, n, sh, sw, out, 0.5)
    inv[:20, 2] += rng.uniform(-40, 40, 20)                                 # mostly or wholly outside
    inv[20:40] = augment.identity_maps(20)
    inv[30:40, 2] += 0.5
    inv[40:45] = [1, 0, -3, 0, 1, 70]                                       # nothing of the image
    rects, ok = augment.footprint_rects(inv, sh, sw, (out, out))
    ys, xs = np.mgrid[0:out, 0:out].astype(np.float64)
    empty = 0
    for t in range(n):
        sx = inv[t, 0] * xs + inv[t, 1] * ys + inv[t, 2]
        sy = inv[t, 3] * xs + inv[t, 4] * ys + inv[t, 5]
        x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
        live = (sx >= -1.0) & (sx < sw[t]) & (sy >= -1.0) & (sy < sh[t])   # the kernel's test: else no tap is read
        taps = [(y0 + dy, x0 + dx) for dy in (0, 1) for dx in (0, 1)]
        ty = np.concatenate([a[live] for a, _b in taps])
        tx = np.concatenate([b[live] for _a, b in taps])
        inside = (ty >= 0) & (ty < sh[t]) & (tx >= 0) & (tx < sw[t])
        if not inside.any():
            empty += 1
            continue
        assert ok[t], t
        ry, rx, rh, rw = rects[t]
        assert ry >= 0 and rx >= 0 and rh > 0 and rw > 0 and ry + rh <= sh[t] and rx + rw <= sw[t]
        assert np.all((ty[inside] >= ry) & (ty[inside] < ry + rh) & (tx[inside] >= rx) & (tx[inside] < rx + rw)), t
    assert not ok[40:45].any() and not rects[~ok].any() and empty >= 5
    # the identity map on an image of the output's size: the whole image
    r, k = augment.footprint_rects(augment.identity_maps(1), 16, 16, (16, 16))
    assert k[0] and r[0].tolist() == [0, 0, 16, 16]
    r, k = augment.footprint_rects(np.array([[np.nan, 0, 0, 0, 1, 0]]), 16, 16, (16, 16))
    assert not k[0]


def test_quality_entry_points_are_declared_bound_and_exported():
    names = {"cpx_hbs_u8": 9, "cpx_blur_pool_rects_u8": 23, "cpx_warp_affine_pool_quality_u8": 29}
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name, nargs in names.items():
        assert name in declared and len(_lib.SIGNATURES[name][1]) == nargs
        assert re.search(rf"\bT {name}\b", exported), name
    assert _lib.ABI_VERSION == 3
    assert len(_lib.SIGNATURES["cpx_warp_affine_pool_stain_u8"][1]) == 22 and len(_lib.SIGNATURES["cpx_warp_affine_pool_u8"][1]) == 20
    section = hdr[hdr.index("t6  image quality"):hdr.index("a17  polygonisation")]
    for cite in ("image_quality.py:41-75", "image_quality.py:173-217", "augmentation_configs.py:28-61"):
        assert cite in section
    from classpose_amd import ops
    for fn in ("hbs", "blur", "blur_pool_rects", "warp_affine_pool_quality"):
        assert callable(getattr(ops, fn))
    assert np.array_equal(ops.unit_table_host(), np.arange(256, dtype=np.float32) / np.float32(255))


def test_cli_accepts_both_names_and_enhanced_points_to_them(tmp_path):
    from classpose_amd.entrypoints import train_head
    base = ["--images", "X", "--labels", "Y", "--pretrained_model", "P", "--save_path", "S", "--model_name", "M"]
    for name in ("quality", "hed_he_quality"):
        assert train_head.build_parser().parse_args(base + ["--augment", name]).augment == name
        assert train_head.build_parser().parse_args(["--data_path", "D"] + base[4:] + ["--augment", name]).augment == name
        assert augment.get_config(name) is augment.AUGMENT_CONFIGS[name]
    with pytest.raises(NotImplementedError, match="hed_he_quality") as e:
        augment.get_config("enhanced")
    msg = str(e.value)
    assert "blur" in msg and "hue" in msg and "hed_he" in msg and "additive noise" not in msg
    with pytest.raises(ValueError, match="hed_he_quality"):
        augment.get_config("nonsense")
