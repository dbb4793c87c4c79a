"""Host side of the dataset statistics: the restated reference functions against the reference-minted fixture
tests/golden/reference_label_stats.npz, argument checking of the new training options, the command line, and the C ABI's books."""
from __future__ import annotations

import json
import os
import re
import subprocess

import numpy as np
import pytest

import label_stats_reference as lsr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fixture():
    with open(os.path.join(GOLD, "reference_label_stats.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_label_stats.npz")), meta


def test_fixture_covers_the_cases_and_the_restatement_reproduces_it():
    arr, meta = _fixture()
    assert "RESTATED" in meta["diameters"] and len(meta["cases"]) >= 8
    ncls = meta["n_classes"]
    ms = arr["n_masks"]
    assert 0 in ms and 1 in ms and any(m > 1 and m % 2 for m in ms) and any(m > 1 and m % 2 == 0 for m in ms)
    assert arr["class_counts"][meta["absent_class"]] == 0 and arr["class_weights"][meta["absent_class"]] == 0
    tied = [k for k in range(len(ms)) if ms[k] > 1 and ms[k] % 2 == 0 and arr["mid_area"][k, 0] == arr["mid_area"][k, 1]]
    split = [k for k in range(len(ms)) if arr["mid_area"][k, 0] != arr["mid_area"][k, 1]]
    assert tied and split
    seen = dict(neg100=False, nobg=False, big=False, two=False, bg_class=False)
    for k, c in enumerate(meta["cases"]):
        inst, cls = arr[f"inst_{k}"], arr[f"cls_{k}"]
        assert inst.dtype == np.int32 and cls.dtype == np.int16 and inst.shape == (c["H"], c["W"]) and 32 <= c["H"] <= 64
        r = lsr.numpy_label_stats(inst[None], cls[None], ncls)
        # the per-image restatement is the reference's get_instance_counts / get_class_counts (minted by its own functions)
        assert np.array_equal(r["inst_per_class"][0], arr["instance_counts"][k]) and np.array_equal(r["class_px"][0], arr["class_px"][k])
        assert r["n_masks"][0] == ms[k] and np.array_equal(r["mid_area"][0], arr["mid_area"][k]) and r["diameters"][0] == arr["diameters"][k]
        seen["neg100"] |= bool((cls == -100).any())
        seen["nobg"] |= bool(inst.min() > 0)
        seen["big"] |= bool(inst.max() == 2_000_000_000)
        seen["bg_class"] |= bool(((inst == 0) & (cls > 0)).any())
        seen["two"] |= any(np.unique(cls[(inst == i) & (cls >= 0)]).size > 1 for i in np.unique(inst[inst > 0]))
    assert all(seen.values()), seen
    assert np.array_equal(arr["class_px"].sum(0), arr["class_counts"])


def test_get_class_weights_equals_the_reference_exactly():
    from classpose_amd import dataset_stats as ds
    arr, meta = _fixture()
    w = ds.get_class_weights(arr["class_counts"])
    assert w.dtype == np.float64 and np.array_equal(w, arr["class_weights"])
    assert w[meta["absent_class"]] == 0.0
    with pytest.raises(ValueError, match="no positive class counts"):
        ds.get_class_weights(np.zeros(5, np.int64))


def test_oversampling_probabilities_equal_the_reference():
    from classpose_amd import dataset_stats as ds
    arr, _meta = _fixture()
    for power, key in ((1, "probs_power_1"), (0.5, "probs_power_0p5")):
        p = ds.compute_oversampling_probabilities(arr["class_counts"], arr["instance_counts"], power)
        ref = arr[key]
        dev = np.abs(p - ref) / np.maximum(np.spacing(np.abs(ref)), np.finfo(np.float64).tiny)
        print(f"power {power}: largest deviation {dev.max():.1f} ulp")
        assert dev.max() <= 4                                 # the same numpy float64 operations
        assert abs(p.sum() - 1) < 1e-12 and (p >= 0).all()
    # the class-0 weight is forced to 0: an image that holds background only is never drawn
    cc = np.array([1000, 10, 40], np.int64)
    ic = np.array([[1, 0, 0], [1, 2, 0], [1, 0, 4]], np.float64)
    w = np.array([0.0, 2 * (1.0 / 10), 4 * (1.0 / 40)])
    assert np.array_equal(ds.compute_oversampling_probabilities(cc, ic), w / w.sum())


def test_diameters_from_mid_areas_and_clamp():
    from classpose_amd import dataset_stats as ds
    arr, _meta = _fixture()
    d = ds.diameters_from_mid_areas(arr["mid_area"])
    ref = arr["diameters"]
    assert d.dtype == np.float64 and np.all(np.abs(d - ref) <= 4 * 2.0 ** -52 * ref)
    assert d[arr["n_masks"] == 0].tolist() == [0.0]
    c = ds.clamp_diameters(d)
    assert np.array_equal(c, np.where(d < 5, 5.0, d)) and (d < 5).any() and c is not d


def test_rescale_keeps_the_order_and_number_of_draws():
    from classpose_amd import augment
    n = 6
    rs = np.array([0.5, 1.0, 2.0, 0.25, 3.0, 1.5])
    a_rng, b_rng = np.random.default_rng(9), np.random.default_rng(9)
    a = augment.sample_affine_params(a_rng, n, 640, 512, 256, 0.5)
    b = augment.sample_affine_params(b_rng, n, 640, 512, 256, 0.5, rescale=rs)
    assert a_rng.random() == b_rng.random()                                 # both consumed the same stream
    assert np.array_equal(a["flip"], b["flip"]) and np.array_equal(a["theta"], b["theta"])
    assert np.array_equal(b["scale"], a["scale"] / rs)
    u = np.random.default_rng(9)
    _uf, _ut, _us, u_dxy = u.random(n), u.random(n), u.random(n), u.random((n, 2))
    room = np.maximum(0.0, np.stack([512 * b["scale"] - 256, 640 * b["scale"] - 256], 1))      # from the DIVIDED scale
    assert np.array_equal(b["dxy"], (u_dxy - 0.5) * room) and (room > 0).any() and (room == 0).any()
    ones = augment.sample_affine_params(np.random.default_rng(9), n, 640, 512, 256, 0.5, rescale=np.ones(n))
    assert all(np.array_equal(a[k], ones[k]) for k in a)
    # sample_affine / sample_batch_params hand the factors through
    _f, inv = augment.sample_affine(np.random.default_rng(9), n, 640, 512, 256, 0.5, rescale=rs)
    assert np.array_equal(inv, augment.affine_inverse(b["flip"], b["theta"], b["scale"], b["dxy"], 640, 512, 256))
    bp = augment.sample_batch_params(np.random.default_rng(9), n, 640, 512, None, 0.5, True, 256, rescale=rs)
    assert np.array_equal(bp.inv, inv)
    for bad in (np.ones(n - 1), np.zeros(n), -np.ones(n)):
        with pytest.raises(ValueError, match="rescale"):
            augment.sample_affine_params(np.random.default_rng(9), n, 640, 512, 256, 0.5, rescale=bad)
    with pytest.raises(ValueError, match="geometric"):
        augment.sample_batch_params(np.random.default_rng(9), n, 640, 512, None, 0.5, False, 256, rescale=rs)


def test_train_class_head_checks_train_probs_and_rescale(tmp_path):
    from classpose_amd.train import train_class_head
    X, Y = np.zeros((3, 256, 256, 3), np.uint8), np.zeros((3, 256, 256), np.int16)
    kw = dict(save_path=tmp_path, model_name="m", n_epochs=1)
    for probs, msg in (([0.5, 0.5], "same length"), ([0.5, -0.1, 0.6], "non-negative"), ([0.0, 0.0, 0.0], "positive value"),
                       ([np.nan, 1.0, 1.0], "positive value")):
        with pytest.raises(ValueError, match=msg):
            train_class_head(None, X, Y, train_probs=probs, **kw)
    with pytest.raises(ValueError, match="needs augment"):
        train_class_head(None, X, Y, rescale=True, diameters=np.full(3, 20.0), **kw)
    with pytest.raises(ValueError, match="needs the diameters"):
        train_class_head(None, X, Y, rescale=True, augment="geometry", **kw)
    with pytest.raises(ValueError, match="one positive diameter"):
        train_class_head(None, X, Y, rescale=True, augment="geometry", diameters=np.array([20.0, 0.0, 5.0]), **kw)
    with pytest.raises(ValueError, match="one positive diameter"):
        train_class_head(None, X, Y, rescale=True, augment="geometry", diameters=np.full(2, 20.0), **kw)


REQ = ["--images", "X.npy", "--labels", "Y.npy", "--pretrained_model", "ck.pt", "--save_path", "out", "--model_name", "m"]


def test_parser_has_the_new_flags_and_their_defaults():
    from classpose_amd.entrypoints import train_head
    p = train_head.build_parser()
    a = p.parse_args(REQ)
    assert a.instances is None and a.test_instances is None and a.auto_class_weights is False and a.class_weights is None
    assert a.oversampling_method == "none" and a.oversampling_power == 1.0 and a.rescale is False and a.diam_mean == 30.0
    assert a.min_train_masks == 0
    train_head.check_args(a)                                               # the old command line needs nothing new
    a = p.parse_args(REQ + ["--instances", "I.npy", "--test_instances", "TI.npy", "--test_images", "TX.npy", "--test_labels", "TY.npy",
                            "--auto_class_weights", "--oversampling_method", "custom", "--oversampling_power", "0.5", "--rescale",
                            "--diam_mean", "24", "--min_train_masks", "5", "--augment", "geometry"])
    assert (a.instances, a.test_instances, a.auto_class_weights, a.oversampling_method, a.oversampling_power, a.rescale, a.diam_mean,
            a.min_train_masks) == ("I.npy", "TI.npy", True, "custom", 0.5, True, 24.0, 5)
    train_head.check_args(a)
    a = p.parse_args(REQ + ["--class_weights", "1", "2.5"])
    assert a.class_weights == [1.0, 2.5]                                   # keeps its type
    with pytest.raises(SystemExit):                                        # mutually exclusive
        p.parse_args(REQ + ["--class_weights", "1", "2", "--auto_class_weights"])
    with pytest.raises(SystemExit):
        p.parse_args(REQ + ["--oversampling_method", "undersample"])
    for flags in (["--auto_class_weights"], ["--oversampling_method", "custom"], ["--rescale", "--augment", "geometry"],
                  ["--min_train_masks", "1"], ["--test_instances", "TI.npy", "--test_images", "TX.npy", "--test_labels", "TY.npy"]):
        with pytest.raises(SystemExit, match="needs --instances"):
            train_head.check_args(p.parse_args(REQ + flags))
    with pytest.raises(SystemExit, match="needs --augment"):
        train_head.check_args(p.parse_args(REQ + ["--instances", "I.npy", "--rescale"]))
    helptext = p.format_help()
    assert "opt-in" in helptext and "reference" in helptext


def test_label_stats_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    for name in ("cpx_label_stats", "cpx_label_stats_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert len(_lib.SIGNATURES["cpx_label_stats"][1]) == 14
    L = _lib.lib()
    assert L.cpx_label_stats_workspace_bytes(32, 256, 256, 7) > 0
    assert L.cpx_label_stats_workspace_bytes(32, 256, 256, 0) == 0 and L.cpx_label_stats_workspace_bytes(32, 256, 256, 65) == 0
    assert L.cpx_label_stats_workspace_bytes(1, 256, 256, 64) > 0 and L.cpx_label_stats_workspace_bytes(0, 256, 256, 7) == 0
    # two tables of a power of two >= 2 * H * W slots of 8 bytes per image at the least
    assert L.cpx_label_stats_workspace_bytes(32, 256, 256, 7) >= 32 * 2 * (2 * 256 * 256) * 8


def test_label_stats_refuses_host_tensors_and_bad_shapes():
    import torch
    from classpose_amd import dataset_stats as ds, ops
    i, c = torch.zeros((1, 8, 8), dtype=torch.int32), torch.zeros((1, 8, 8), dtype=torch.int16)
    with pytest.raises(ValueError, match="cuda"):
        ops.label_stats(i, c, 3)
    with pytest.raises(ValueError, match="int32"):
        ops.label_stats(i.long(), c, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ds.label_stats(i.numpy(), c.numpy(), 3, device="cpu")
    with pytest.raises(ValueError, match="one shape"):
        ds.label_stats(np.zeros((2, 8, 8), np.int32), np.zeros((2, 8, 9), np.int16), 3)
