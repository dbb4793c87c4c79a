"""Host side of the device augmentation (classpose_amd.augment): the restatements of tests/augment_reference.py against
the reference-minted fixture, the transform sampler, and the CLI flags.  No GPU."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

import augment_reference as ar
from classpose_amd import augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fixture():
    with open(os.path.join(GOLD, "reference_augment.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_augment.npz")), meta


def test_stain_matrices_are_the_references():
    from scipy import linalg
    npz, _ = _fixture()
    assert augment.HED_FROM_RGB.dtype == np.float32 and augment.RGB_FROM_HED.dtype == np.float32
    assert np.array_equal(augment.RGB_FROM_HED.view(np.uint32), npz["RGB_FROM_HED"].view(np.uint32))
    assert np.array_equal(augment.HED_FROM_RGB.view(np.uint32), npz["HED_FROM_RGB"].view(np.uint32))
    inv = np.float32(linalg.inv(augment.RGB_FROM_HED))
    assert np.array_equal(augment.HED_FROM_RGB.view(np.uint32), inv.view(np.uint32))
    assert np.array_equal(ar.RGB_FROM_HED.view(np.uint32), npz["RGB_FROM_HED"].view(np.uint32))


def test_the_fixture_covers_what_it_should():
    npz, meta = _fixture()
    cases = meta["cases"]
    assert len(cases) >= 6 and "RESTATED" in meta["rescale_intensity"]
    assert sum(not c["applied"] for c in cases) == 2
    lo, hi = meta["config"]["cutoff_range"]
    assert any(c["mean"] < lo for c in cases) and any(c["mean"] > hi for c in cases)
    assert {c["simple_mode"] for c in cases if c["applied"]} == {True, False}
    for c in cases:
        assert 64 <= min(npz[c["name"] + "_in"].shape[:2]) and max(npz[c["name"] + "_in"].shape[:2]) <= 96
    cfg = augment.AUGMENT_CONFIGS["hed_only"]
    assert [list(r) for r in cfg["sigma_ranges"]] == meta["config"]["sigma_ranges"] == [[-0.25, 0.25]] * 3
    assert [list(r) for r in cfg["bias_ranges"]] == meta["config"]["bias_ranges"] == [[-0.25, 0.25]] * 3
    assert list(cfg["cutoff_range"]) == meta["config"]["cutoff_range"] == [0.15, 0.85]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_equals_the_reference_fixture(dtype):
    """Both restatements against HEDTransform.transform under the rule of the GPU test: the decision equal, untouched patches
    byte-equal, a transformed pixel off by one level only where the float64 restatement's 255 x is within 1e-3 of an integer."""
    npz, meta = _fixture()
    cut = meta["config"]["cutoff_range"]
    for c in meta["cases"]:
        src, ref = npz[c["name"] + "_in"], npz[c["name"] + "_out"]
        out, applied, _v = ar.hed_jitter(src, c["sigma"], c["bias"], npz["HED_FROM_RGB"], cut, c["simple_mode"], dtype)
        assert applied == c["applied"], c["name"]
        if not applied:
            assert np.array_equal(out, ref) and np.array_equal(out, src)
            continue
        v64 = ar.hed_jitter(src, c["sigma"], c["bias"], npz["HED_FROM_RGB"], cut, c["simple_mode"], np.float64)[2]
        r = ar.check_hed_against(out, ref, v64)
        print(f"{c['name']} ({dtype.__name__}): {r['differ']} of {ref.size} values differ from the reference, all inside the window")
        assert (ref != src).any()


def test_sample_affine_is_cellposes_parametrisation():
    sh, sw, out, n = 320, 288, 256, 64
    rng = np.random.default_rng(5)
    p = augment.sample_affine_params(rng, n, sh, sw, out, scale_range=0.5)
    r = 0.5
    assert np.all(p["scale"] >= 1 - r / 2) and np.all(p["scale"] <= 1 + r / 2) and p["scale"].std() > 0.05
    assert np.all(p["theta"] >= 0) and np.all(p["theta"] < 2 * np.pi) and 5 < p["flip"].sum() < n - 5
    room = np.maximum(0, np.stack([sw * p["scale"] - out, sh * p["scale"] - out], 1))
    assert np.all(np.abs(p["dxy"]) <= room / 2 + 1e-12)
    noflip = np.zeros(n, bool)
    inv = augment.affine_inverse(noflip, p["theta"], p["scale"], p["dxy"], sh, sw, out)
    fwd = augment.affine_forward(p["theta"], p["scale"], p["dxy"], sh, sw, out)

    def mat(m6):
        M = np.zeros((len(m6), 3, 3))
        M[:, :2] = m6.reshape(-1, 2, 3)
        M[:, 2, 2] = 1
        return M
    assert np.abs(mat(fwd) @ mat(inv) - np.eye(3)).max() <= 1e-12
    assert np.abs((mat(fwd) @ mat(inv))[:, :2, :2] - np.eye(2)).max() <= 1e-12
    # the centre of the source lands on cc1
    cc = np.array([sw / 2, sh / 2, 1.0])
    cc1 = cc[:2] - (np.array([sw, sh]) - out) / 2 + p["dxy"]
    assert np.abs((mat(fwd) @ cc)[:, :2] - cc1).max() <= 1e-12
    assert np.abs((mat(inv) @ np.concatenate([cc1, np.ones((n, 1))], 1)[..., None])[:, :2, 0] - cc[:2]).max() <= 1e-12
    # forward = scale * R(theta)
    assert np.allclose(fwd[:, 0], p["scale"] * np.cos(p["theta"])) and np.allclose(fwd[:, 1], -p["scale"] * np.sin(p["theta"]))
    assert np.allclose(fwd[:, 3], p["scale"] * np.sin(p["theta"]))
    # the flip is folded into the map: sx -> sw - 1 - sx, sy unchanged
    flipped = augment.affine_inverse(~noflip, p["theta"], p["scale"], p["dxy"], sh, sw, out)
    pts = np.array([[0.0, 0.0, 1.0], [255.0, 0.0, 1.0], [17.0, 201.0, 1.0]]).T
    a, b = mat(inv) @ pts, mat(flipped) @ pts
    assert np.abs(b[:, 0] - ((sw - 1) - a[:, 0])).max() <= 1e-12 and np.array_equal(a[:, 1], b[:, 1])


def test_sample_affine_streams():
    a = augment.sample_affine(np.random.default_rng(9), 16, 256, 256)
    b = augment.sample_affine(np.random.default_rng(9), 16, 256, 256)
    c = augment.sample_affine(np.random.default_rng(10), 16, 256, 256)
    assert a[1].dtype == np.float64 and a[1].shape == (16, 6) and a[0].dtype == bool
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.array_equal(a[1], c[1])
    # the switches do not shift the stream: the same maps up to the flip / the rotation
    f0, i0 = augment.sample_affine(np.random.default_rng(9), 16, 256, 256, do_flip=False)
    assert not f0.any() and np.array_equal(i0[~a[0]], a[1][~a[0]]) and np.array_equal(i0[:, 3:], a[1][:, 3:])
    assert np.allclose(i0[a[0], 2], 255 - a[1][a[0], 2], atol=1e-12, rtol=0) and a[0].any()
    _f, i1 = augment.sample_affine(np.random.default_rng(9), 16, 256, 256, do_flip=False, rotate=False)
    assert np.all(i1[:, 1] == 0) and np.all(i1[:, 3] == 0) and np.all(i1[:, 0] > 0)
    # scale_range is clamped to [0, 2]; 0 means no scaling, and a 256 source then maps onto itself up to the rotation
    _f, i2 = augment.sample_affine(np.random.default_rng(9), 4, 256, 256, scale_range=0.0, do_flip=False, rotate=False)
    assert np.array_equal(i2, augment.identity_maps(4))
    p = augment.sample_affine_params(np.random.default_rng(1), 200, 256, 256, scale_range=7.0)
    assert p["scale"].min() >= 0 and p["scale"].max() <= 2


def test_sample_hed_and_configs():
    cfg = augment.get_config("hed_only")
    s, b = augment.sample_hed(np.random.default_rng(3), 50, cfg["sigma_ranges"], cfg["bias_ranges"])
    assert s.shape == b.shape == (50, 3) and s.dtype == b.dtype == np.float32
    assert np.abs(s).max() <= 0.25 and np.abs(b).max() <= 0.25 and s.std() > 0.1 and not np.array_equal(s, b)
    s2, _ = augment.sample_hed(np.random.default_rng(3), 50, cfg["sigma_ranges"], cfg["bias_ranges"])
    assert np.array_equal(s, s2)
    assert augment.get_config(None) is None and augment.get_config("geometry") is None
    with pytest.raises(NotImplementedError, match="blur"):
        augment.get_config("enhanced")
    with pytest.raises(ValueError):
        augment.get_config("nonsense")


def test_cli_flags():
    from classpose_amd.entrypoints import train_head
    base = ["--images", "X", "--labels", "Y", "--pretrained_model", "P", "--save_path", "S", "--model_name", "M"]
    a = train_head.build_parser().parse_args(base)
    assert a.augment is None and a.scale_range == 0.5 and a.augment_label_fill == 0
    a = train_head.build_parser().parse_args(base + ["--augment", "hed_only", "--scale_range", "0.25", "--augment_label_fill", "-100"])
    assert a.augment == "hed_only" and a.scale_range == 0.25 and a.augment_label_fill == -100
    assert train_head.build_parser().parse_args(base + ["--augment", "geometry"]).augment == "geometry"
    with pytest.raises(SystemExit):
        train_head.build_parser().parse_args(base + ["--augment", "nonsense"])


def test_enhanced_raises_before_anything_runs(tmp_path):
    """train_class_head(augment="enhanced") names the missing pieces; no device is touched (the trainer is never used)."""
    from classpose_amd.train import train_class_head
    X = np.zeros((1, 256, 256, 3), np.uint8)
    Y = np.zeros((1, 256, 256), np.int16)
    with pytest.raises(NotImplementedError, match="hue"):
        train_class_head(None, X, Y, n_epochs=1, save_path=tmp_path, augment="enhanced")


def test_restatement_warp_basics():
    """The warp restatement on cases with a known answer: identity, an integer shift with a zero border, label fill."""
    rng = np.random.default_rng(0)
    src = rng.integers(0, 256, (3, 20, 24)).astype(np.float64)
    ident = np.array([1.0, 0, 0, 0, 1.0, 0])
    assert np.array_equal(ar.warp_image(src, ident, 20, 24), src)
    shift = np.array([1.0, 0, -3, 0, 1.0, 2])           # source = (x - 3, y + 2)
    w = ar.warp_image(src, shift, 20, 24, np.float32)
    assert np.array_equal(w[:, :18, 3:], src[:, 2:, :21].astype(np.float32)) and not w[:, :, :3].any() and not w[:, 18:].any()
    lab = rng.integers(0, 5, (20, 24)).astype(np.int16)
    l = ar.warp_labels(lab, shift, 20, 24, -100)
    assert np.array_equal(l[:18, 3:], lab[2:, :21]) and np.all(l[:, :3] == -100) and np.all(l[18:] == -100)
    half = np.array([1.0, 0, 0.5, 0, 1.0, 0])            # half-pixel shift: the mean of two neighbours, the last column half-faded
    h = ar.warp_image(src, half, 20, 24)
    assert np.array_equal(h[:, :, :-1], (src[:, :, :-1] + src[:, :, 1:]) / 2) and np.array_equal(h[:, :, -1], src[:, :, -1] / 2)


def test_restatement_normalisation_modes():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((1, 3, 40, 50)).astype(np.float32)
    x[0, 1] = 3.25
    x[0, 2] = 1.0 + 1e-4 * rng.random((40, 50)).astype(np.float32)
    st, out = ar.normalize_f32(x)
    assert list(st[0, :, 2]) == [1, 0, 2]
    assert np.array_equal(out[0, 1], x[0, 1]) and not out[0, 2].any()
    lo, hi = np.percentile(out[0, 0], [1, 99])
    assert abs(lo) < 1e-6 and abs(hi - 1) < 1e-6
