"""Host side of training from whole annotated images of any size (classpose_amd.train_data, the samplers and the window grid of
classpose_amd.augment, the train_head flags): no GPU.

Yardstick of the loader: tests/golden/reference_train_data.npz, minted by the reference's own ``load_data_arrays``,
``_split_labels``, ``_filter_labels_and_images``, ``subsample_dataset`` and ``split_dataset`` (tests/golden/make_golden_train_data.py)."""
from __future__ import annotations

import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from classpose_amd import _lib, augment, train_data
from classpose_amd.entrypoints import train_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "reference_train_data.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_train_data.npz")), meta


def _write_case(gold, case, folder):
    from make_golden_train_data import save_case
    npz, _meta = gold
    n, name = case["n"], case["name"]
    save_case(str(folder), [npz[f"{name}_image_{i}"] for i in range(n)], [npz[f"{name}_labels_{i}"] for i in range(n)], case["saved_as"])


# ---- 1. the loader against the reference's own results ---------------------------------------------------------------
def test_loader_equals_the_reference_integer_for_integer(gold, tmp_path):
    npz, meta = gold
    assert [c["name"] for c in meta["cases"]] == ["ragged", "objdtype", "floatlabels"]
    for case in meta["cases"]:
        name, n = case["name"], case["n"]
        _write_case(gold, case, tmp_path / name)
        images, labels = train_data.load_data_arrays(tmp_path / name)
        assert str(images[0].dtype) == case["loaded_image_dtype"] and str(labels[0].dtype) == case["loaded_label_dtype"], name
        for i in range(n):
            assert np.array_equal(images[i], npz[f"{name}_loaded_image_{i}"]) and images[i].dtype == npz[f"{name}_loaded_image_{i}"].dtype
        inst, cls = train_data.split_labels(labels)
        for i in range(n):
            assert cls[i].dtype == np.int16 and np.array_equal(cls[i], npz[f"{name}_cls_{i}"]), (name, i)
            assert np.array_equal(inst[i], npz[f"{name}_inst_{i}"]), (name, i)
        kept = [i for i in range(n) if case["kept"][i]]
        u8 = [train_data.image_to_uint8(im) for im in images]
        a, b, c, keep = train_data.filter_single_pixel(u8, inst, cls)
        assert list(keep) == kept and len(a) == len(b) == len(c) == len(kept)
        data = train_data.load_dataset(tmp_path / name)
        assert len(data) == len(kept) and data.n_classes == case["max_class"] + 1
        for k, i in enumerate(kept):                                         # all three lists dropped together: still aligned
            assert data.images[k].dtype == np.uint8 and np.array_equal(data.images[k], npz[f"{name}_image_{i}"]), (name, i)
            assert np.array_equal(data.instances[k], npz[f"{name}_inst_{i}"]) and np.array_equal(data.classes[k], npz[f"{name}_cls_{i}"])
    ragged = meta["cases"][0]
    assert ragged["kept"].count(False) == 1 and len({npz[f"ragged_image_{i}"].shape for i in range(ragged["n"])}) == ragged["n"]
    # both masking rules occur in the fixture
    lab0, cls0 = npz["ragged_labels_0"], npz["ragged_cls_0"]
    assert ((lab0[..., 0] == 0) & (lab0[..., 1] > 0)).any() and (cls0[(lab0[..., 0] == 0) & (lab0[..., 1] > 0)] == -100).all()
    lab1, cls1 = npz["ragged_labels_1"], npz["ragged_cls_1"]
    assert ((lab1[..., 0] > 0) & (lab1[..., 1] == 0)).any() and (cls1[(lab1[..., 0] > 0) & (lab1[..., 1] == 0)] == -100).all()


def test_loader_refuses_what_it_cannot_hold(tmp_path):
    with pytest.raises(FileNotFoundError):
        train_data.load_data_arrays(tmp_path)
    with pytest.raises(ValueError, match="integer values"):
        train_data.image_to_uint8(np.full((4, 4, 3), 0.5, np.float32))
    with pytest.raises(ValueError, match="integer values"):
        train_data.image_to_uint8(np.full((4, 4, 3), 256.0, np.float32))
    with pytest.raises(ValueError):
        train_data.image_to_uint8(np.zeros((4, 4, 3), np.int32))
    with pytest.raises(ValueError):
        train_data.image_to_uint8(np.zeros((4, 4), np.uint8))
    assert train_data.image_to_uint8(np.full((2, 2, 3), 255.0, np.float32)).dtype == np.uint8
    # floating labels that are not integers lose distinct values in the conversion
    np.save(tmp_path / "images.npy", np.zeros((2, 4, 4, 3), np.uint8))
    lab = np.zeros((2, 4, 4, 2), np.float64)
    lab[0, 0, 0], lab[0, 1, 1] = (1.0, 1.0), (1.5, 1.0)
    np.save(tmp_path / "labels.npy", lab)
    with pytest.raises(ValueError, match="unique labels"):
        train_data.load_data_arrays(tmp_path)


def test_subsample_and_split_indices_equal_the_reference(gold):
    npz, meta = gold
    assert {(s["n"], s["seed"], s["fraction"]) for s in meta["splits"]} == {(n, sd, f) for n in (10, 37) for sd in (0, 42) for f in (0.5, 0.8)}
    for s in meta["splits"]:
        n, seed, f, key = s["n"], s["seed"], s["fraction"], s["key"]
        sub = train_data.subsample_indices(n, f, seed)
        tr, te = train_data.split_indices(n, f, seed)
        assert np.array_equal(sub, npz[f"{key}_sub"]) and np.array_equal(tr, npz[f"{key}_train"]) and np.array_equal(te, npz[f"{key}_test"])
        str_, ste = train_data.split_indices(len(sub), f, seed)             # subsample, then split what is left
        assert np.array_equal(sub[str_], npz[f"{key}_sub_train"]) and np.array_equal(sub[ste], npz[f"{key}_sub_test"])
        assert sorted(np.concatenate([tr, te])) == list(range(n))
    assert np.array_equal(train_data.subsample_indices(7, None, 0), np.arange(7))
    tr, te = train_data.split_indices(7, 1.0, 0)
    assert np.array_equal(tr, np.arange(7)) and te is None


def test_stats_chunk_keeps_the_workspace_under_the_budget():
    L = _lib.lib()
    one = L.cpx_label_stats_workspace_bytes(1, 1024, 1024, 7)
    tables = (2 * 8 + 4) * (1 << 21) + 4 * (1 << 20)                        # one 1024 x 1024 image: 44 MB (2^21 slots)
    assert tables <= one <= tables + 4096
    for H, W, budget in ((1024, 1024, 1 << 30), (256, 256, 1 << 30), (300, 520, 64 << 20), (1024, 1024, 1 << 20)):
        c = train_data.stats_chunk(H, W, 7, budget)
        assert c >= 1
        if c > 1:
            assert L.cpx_label_stats_workspace_bytes(c, H, W, 7) <= budget
        if c < 65535:
            assert L.cpx_label_stats_workspace_bytes(c + 1, H, W, 7) > budget
    assert train_data.stats_chunk(1024, 1024, 7, 1 << 20) == 1


# ---- 2. the window grid ----------------------------------------------------------------------------------------------
def test_grid_origins():
    hand = {100: [0], 256: [0], 257: [0, 1], 512: [0, 256], 1000: [0, 248, 496, 744]}
    for h, origins in hand.items():
        assert augment.grid_origins(h) == origins, h
        if h > 256:
            assert origins[-1] == h - 256
            covered = np.zeros(h, bool)
            for o in origins:
                covered[o:o + 256] = True
            assert covered.all(), h
    for h in range(1, 1400, 7):                                             # every pixel is covered, the last window ends the image
        o = augment.grid_origins(h)
        assert o[0] == 0 and o == sorted(o) and (h <= 256 or o[-1] == h - 256)
        assert all(b - a <= 256 for a, b in zip(o, o[1:]))
    win = augment.grid_windows([(100, 300), (520, 256)])
    assert win.tolist() == [[0, 0, 0], [0, 0, 44], [1, 0, 0], [1, 132, 0], [1, 264, 0]]


def test_pool_table_is_validated():
    px_off, hw, total = augment.pool_table([(1, 1), (5, 7), (37, 53), (301, 299)])
    assert px_off.tolist() == [0, 1, 36, 1997] and total == 1997 + 301 * 299 and hw.dtype == np.int32 and px_off.dtype == np.int64
    assert (3 * px_off[3]) % 2 == 1                                         # the 37 x 53 image makes the next byte offset odd
    augment.check_pool_table(px_off, hw, total)
    with pytest.raises(ValueError, match="pool holds"):
        augment.check_pool_table(px_off, hw, total + 1)
    bad = px_off.copy()
    bad[2] = 35
    with pytest.raises(ValueError, match="offsets"):
        augment.check_pool_table(bad, hw, total)
    with pytest.raises(ValueError, match="offsets"):
        augment.check_pool_table(px_off[::-1].copy(), hw, total)
    z = hw.copy()
    z[1, 0] = 0
    with pytest.raises(ValueError, match="positive"):
        augment.check_pool_table(px_off, z, total)
    with pytest.raises(ValueError):
        augment.pool_table([])
    with pytest.raises(ValueError):
        augment.pool_table([(4, 0)])


# ---- 3. the samplers with per-crop shapes ----------------------------------------------------------------------------
def _affine_inverse_before(flip, theta, scale, dxy, sh, sw, out=256):
    """augment.affine_inverse as it stood before it took per-crop shapes, kept here word for word as the yardstick."""
    flip, theta, scale = np.asarray(flip, bool), np.asarray(theta, np.float64), np.asarray(scale, np.float64)
    dxy = np.asarray(dxy, np.float64).reshape(-1, 2)
    cc = np.array([sw / 2, sh / 2], np.float64)
    cc1 = cc - (np.array([sw, sh], np.float64) - out) / 2 + dxy
    c, s = np.cos(theta) / scale, np.sin(theta) / scale
    inv = np.empty((len(theta), 6), np.float64)
    inv[:, 0], inv[:, 1] = c, s
    inv[:, 3], inv[:, 4] = -s, c
    inv[:, 2] = cc[0] - (c * cc1[:, 0] + s * cc1[:, 1])
    inv[:, 5] = cc[1] - (-s * cc1[:, 0] + c * cc1[:, 1])
    inv[flip, 0:2] = -inv[flip, 0:2]
    inv[flip, 2] = (sw - 1) - inv[flip, 2]
    return inv


def _sample_affine_before(rng, n, sh, sw, out=256, scale_range=0.5, rescale=None):
    """augment.sample_affine_params + affine_inverse as they stood before, word for word."""
    r = float(np.clip(scale_range, 0.0, 2.0))
    u_flip, u_theta, u_scale, u_dxy = rng.random(n), rng.random(n), rng.random(n), rng.random((n, 2))
    flip = (u_flip > 0.5) & True
    theta = 2 * np.pi * u_theta
    scale = (1 - r / 2) + r * u_scale
    if rescale is not None:
        scale = scale / rescale
    room = np.maximum(0.0, np.stack([sw * scale - out, sh * scale - out], 1))
    dxy = (u_dxy - 0.5) * room
    return flip, theta, scale, dxy, _affine_inverse_before(flip, theta, scale, dxy, sh, sw, out)


@pytest.mark.parametrize("sh,sw", [(256, 256), (200, 333), (1024, 1000)])
def test_sampler_with_shape_arrays_is_bitwise_the_sampler_before(sh, sw):
    n = 9
    rsc = np.linspace(0.4, 2.5, n)
    for rescale in (None, rsc):
        flip0, theta0, scale0, dxy0, inv0 = _sample_affine_before(np.random.default_rng(5), n, sh, sw, 256, 0.5, rescale)
        for shapes in ((sh, sw), (np.full(n, sh), np.full(n, sw)), (np.full(n, sh, np.int32), sw)):
            g = np.random.default_rng(5)
            p = augment.sample_affine_params(g, n, shapes[0], shapes[1], 256, 0.5, rescale=rescale)
            assert np.array_equal(p["flip"], flip0)
            for a, b in ((p["theta"], theta0), (p["scale"], scale0), (p["dxy"], dxy0)):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
            inv = augment.affine_inverse(p["flip"], p["theta"], p["scale"], p["dxy"], shapes[0], shapes[1], 256)
            assert np.array_equal(inv.view(np.uint64), inv0.view(np.uint64))
            assert g.random() == np.random.default_rng(5).random(5 * n + 1)[-1]            # five draws per crop, no more
        f2, inv2 = augment.sample_affine(np.random.default_rng(5), n, np.full(n, sh), np.full(n, sw), 256, 0.5, rescale=rescale)
        assert np.array_equal(f2, flip0) and np.array_equal(inv2.view(np.uint64), inv0.view(np.uint64))
    assert flip0.any() and not flip0.all()


def test_sampler_uses_each_crops_own_room():
    n = 6
    sh = np.array([256, 100, 1024, 300, 256, 2000])
    sw = np.array([256, 900, 1024, 257, 512, 31])
    p = augment.sample_affine_params(np.random.default_rng(8), n, sh, sw, 256, 0.5)
    u = np.random.default_rng(8).random(5 * n)
    u_dxy = u[3 * n:].reshape(n, 2)
    room = np.maximum(0.0, np.stack([sw * p["scale"] - 256, sh * p["scale"] - 256], 1))
    assert np.array_equal(p["dxy"], (u_dxy - 0.5) * room)
    assert p["dxy"][1, 1] == 0 and p["dxy"][5, 0] == 0 and abs(p["dxy"][5, 1]) > 0      # no room along an axis shorter than the crop
    inv = augment.affine_inverse(p["flip"], p["theta"], p["scale"], p["dxy"], sh, sw, 256)
    for i in range(n):                                                      # row i is the scalar-shape map of its own shape
        one = augment.affine_inverse(p["flip"][i:i + 1], p["theta"][i:i + 1], p["scale"][i:i + 1], p["dxy"][i:i + 1], int(sh[i]), int(sw[i]), 256)
        assert np.array_equal(inv[i], one[0])
        fwd = augment.affine_forward(p["theta"][i:i + 1], p["scale"][i:i + 1], p["dxy"][i:i + 1], int(sh[i]), int(sw[i]), 256)[0]
        assert np.array_equal(augment.affine_forward(p["theta"], p["scale"], p["dxy"], sh, sw, 256)[i], fwd)
    with pytest.raises(ValueError):
        augment.sample_affine_params(np.random.default_rng(0), 3, np.array([256, 256]), 256)
    with pytest.raises(ValueError):
        augment.sample_affine_params(np.random.default_rng(0), 2, np.array([256, 0]), 256)


# ---- 4. command line -------------------------------------------------------------------------------------------------
REQ = ["--pretrained_model", "C", "--save_path", "D", "--model_name", "N"]


def test_cli_data_path_flags():
    p = train_head.build_parser()
    a = p.parse_args(REQ + ["--data_path", "DIR"])
    assert (a.data_path, a.test_data_path, a.train_fraction, a.subsample_fraction, a.images, a.labels) == ("DIR", None, 0.8, None, None, None)
    train_head.check_args(a)                                                # --data_path alone is enough
    a = p.parse_args(REQ + ["--data_path", "DIR", "--test_data_path", "T", "--train_fraction", "0.5", "--subsample_fraction", "0.25",
                            "--auto_class_weights", "--oversampling_method", "custom", "--rescale", "--augment", "hed_only",
                            "--min_train_masks", "2"])
    assert (a.test_data_path, a.train_fraction, a.subsample_fraction) == ("T", 0.5, 0.25)
    train_head.check_args(a)                                                # the instance options work from channel 0: no --instances
    for extra in (["--images", "X.npy"], ["--labels", "Y.npy"], ["--images", "X.npy", "--labels", "Y.npy"], ["--instances", "I.npy"],
                  ["--test_images", "X.npy", "--test_labels", "Y.npy"]):
        with pytest.raises(SystemExit):
            train_head.check_args(p.parse_args(REQ + ["--data_path", "DIR"] + extra))
    with pytest.raises(SystemExit):
        train_head.check_args(p.parse_args(REQ))                            # neither
    with pytest.raises(SystemExit):
        train_head.check_args(p.parse_args(REQ + ["--images", "X.npy"]))    # half of the arrays
    with pytest.raises(SystemExit):
        train_head.check_args(p.parse_args(REQ + ["--images", "X", "--labels", "Y", "--test_data_path", "T"]))
    with pytest.raises(SystemExit):
        train_head.check_args(p.parse_args(REQ + ["--data_path", "DIR", "--train_fraction", "0"]))
    with pytest.raises(SystemExit):
        train_head.check_args(p.parse_args(REQ + ["--data_path", "DIR", "--rescale"]))          # needs --augment
    # an old command line parses to the same values of the old flags, and the new ones stay at their defaults
    old = p.parse_args(REQ + ["--images", "X.npy", "--labels", "Y.npy", "--instances", "I.npy", "--rescale", "--augment", "geometry"])
    train_head.check_args(old)
    assert (old.images, old.labels, old.instances, old.rescale, old.augment, old.nclasses) == ("X.npy", "Y.npy", "I.npy", True, "geometry", None)
    assert (old.data_path, old.test_data_path, old.subsample_fraction) == (None, None, None)


def test_pool_entry_points_are_declared_bound_and_exported():
    names = {"cpx_pool_byte_sums", "cpx_warp_affine_pool_u8"}
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    assert names <= set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    for n in names:
        assert hasattr(L, n)
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    assert names <= exported
    assert len(_lib.SIGNATURES["cpx_warp_affine_pool_u8"][1]) == 20 and len(_lib.SIGNATURES["cpx_pool_byte_sums"][1]) == 8
