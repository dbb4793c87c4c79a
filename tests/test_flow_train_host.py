"""Host side of the flow-head training (no GPU): the vector matrices of the target warp, the ``--freeze`` / ``--train_flow_head``
command line, the symmetry of the oracle's ``masks_to_flows`` that the device tests lean on, and the bookkeeping of the C ABI."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import flow_train_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_flow_vec_against_hand_written_matrices():
    """vec = [cos t, f sin t, -sin t, f cos t], f = -1 where flipped: Y' = vec0 Y + vec1 X, X' = vec2 Y + vec3 X."""
    from classpose_amd import augment
    want = {  # (flip, quarter turns) -> the matrix with exact entries
        (False, 0): [1, 0, 0, 1], (False, 1): [0, 1, -1, 0], (False, 2): [-1, 0, 0, -1], (False, 3): [0, -1, 1, 0],
        (True, 0): [1, 0, 0, -1], (True, 1): [0, -1, -1, 0], (True, 2): [-1, 0, 0, 1], (True, 3): [0, 1, 1, 0],
    }
    keys = sorted(want)
    flip = np.array([k[0] for k in keys])
    theta = np.array([k[1] * np.pi / 2 for k in keys])
    got = augment.flow_vec(flip, theta)
    assert got.shape == (8, 4) and got.dtype == np.float64
    assert np.abs(got - np.array([want[k] for k in keys], np.float64)).max() <= 4e-16       # cos / sin of k pi / 2 in double
    # a unit flow along +X of an unflipped source turned by a quarter: Y' = X sin t = 1, X' = X cos t = 0
    v = augment.flow_vec([False], [np.pi / 2])[0]
    assert abs(v[0] * 0 + v[1] * 1 - 1) < 1e-15 and abs(v[2] * 0 + v[3] * 1) < 1e-15
    with pytest.raises(ValueError):
        augment.flow_vec([True, False], [0.0])
    assert np.array_equal(augment.identity_vecs(2), [[1, 0, 0, 1], [1, 0, 0, 1]])


def test_batch_params_keep_the_rotation_without_changing_a_draw():
    """``sample_batch_params`` now keeps theta; flips and maps are bitwise those of ``sample_affine`` on the same stream."""
    from classpose_amd import augment
    p = augment.sample_batch_params(np.random.default_rng(5), 6, 300, 280, None, 0.5)
    flip, inv = augment.sample_affine(np.random.default_rng(5), 6, 300, 280, 256, 0.5)
    assert np.array_equal(p.flip, flip) and np.array_equal(p.inv, inv)
    q = augment.sample_affine_params(np.random.default_rng(5), 6, 300, 280, 256, 0.5)
    assert np.array_equal(p.theta, q["theta"])
    g = augment.sample_batch_params(np.random.default_rng(5), 3, 256, 256, None, geometry=False)
    assert np.array_equal(g.theta, np.zeros(3)) and np.array_equal(augment.flow_vec(g.flip, g.theta), augment.identity_vecs(3))


def _parse(*argv):
    from classpose_amd.entrypoints import train_head
    base = ["--pretrained_model", "m.pt", "--save_path", "out", "--model_name", "m"]
    args = train_head.build_parser().parse_args(base + list(argv))
    train_head.check_args(args)
    return args


def test_freeze_and_train_flow_head_parsing():
    arrays = ["--images", "X.npy", "--labels", "Y.npy"]
    assert _parse(*arrays).train_flow_head is False
    assert _parse(*arrays, "--freeze", "backbone", "segmentation_head", "neck").train_flow_head is False
    assert _parse(*arrays, "--freeze", "neck", "segmentation_head", "backbone").train_flow_head is False
    assert _parse(*arrays, "--instances", "I.npy", "--train_flow_head").train_flow_head is True
    assert _parse(*arrays, "--instances", "I.npy", "--freeze", "backbone", "neck").train_flow_head is True
    assert _parse(*arrays, "--instances", "I.npy", "--freeze", "neck", "backbone", "--train_flow_head").train_flow_head is True
    assert _parse("--data_path", "D", "--freeze", "backbone", "neck").train_flow_head is True
    assert _parse("--data_path", "D", "--train_flow_head").train_flow_head is True
    assert _parse("--data_path", "D").train_flow_head is False


def test_freeze_and_train_flow_head_error_exits():
    arrays = ["--images", "X.npy", "--labels", "Y.npy"]
    with pytest.raises(SystemExit, match="needs --instances or --data_path"):
        _parse(*arrays, "--train_flow_head")
    with pytest.raises(SystemExit, match="needs --instances or --data_path"):
        _parse(*arrays, "--freeze", "backbone", "neck")
    with pytest.raises(SystemExit, match="needs --test_instances"):
        _parse(*arrays, "--instances", "I.npy", "--test_images", "X.npy", "--test_labels", "Y.npy", "--train_flow_head")
    with pytest.raises(SystemExit, match="training the neck is not built"):
        _parse(*arrays, "--freeze", "backbone")
    with pytest.raises(SystemExit, match="training the neck is not built"):
        _parse(*arrays, "--freeze", "backbone", "segmentation_head")
    with pytest.raises(SystemExit, match="training the backbone is not built"):
        _parse(*arrays, "--freeze", "neck")
    with pytest.raises(SystemExit, match="training the backbone and training the neck is not built"):
        _parse(*arrays, "--freeze", "none")
    with pytest.raises(SystemExit, match="training the backbone and training the neck is not built"):
        _parse(*arrays, "--freeze", "segmentation_head")
    with pytest.raises(SystemExit, match="stands alone"):
        _parse(*arrays, "--freeze", "none", "backbone")
    with pytest.raises(SystemExit, match="contradicts"):
        _parse(*arrays, "--instances", "I.npy", "--train_flow_head", "--freeze", "backbone", "segmentation_head", "neck")
    with pytest.raises(SystemExit):                                     # argparse: not one of the reference's choices
        _parse(*arrays, "--freeze", "class_head")


def test_oracle_masks_to_flows_symmetry():
    """With rot90 the quarter turn that takes +X to +Y (``flow_train_reference.rot90`` = np.rot90(., -1); the opposite turn is checked
    with the conjugate identity): masks_to_flows(rot90(m)) == (rot90(F_x), -rot90(F_y)) and masks_to_flows(m[:, ::-1]) == (F_y[:, ::-1], -F_x[:, ::-1]) to 1e-9
    everywhere except each label's own centre pixel, the normalised difference of equal numbers (at most one pixel per label, the
    centre the oracle reports, is left out).  The device warp test pins the sign conventions of the target warp on this."""
    from oracle import dynamics
    m = fr.symmetric_map()
    assert m.max() == 5 and all((m == k).any() for k in range(1, 6))
    F, dbg = dynamics.masks_to_flows(m, return_debug=True)
    assert F.shape == (2, 96, 96) and np.all(F[:, m == 0] == 0)
    nrm = np.sqrt((F ** 2).sum(0))
    skip = fr.centre_mask(m, dbg["centers"])
    assert skip.sum() == 5 and np.all(m[skip] > 0)
    assert np.abs(nrm[(m > 0) & ~skip] - 1).max() < 1e-9
    for name, mt, want, sk in (("rot90", fr.rot90(m).copy(), fr.rot90_flows(F), fr.rot90(skip)),
                               ("rot90 the other way", np.rot90(m).copy(), fr.rot90_ccw_flows(F), np.rot90(skip)),
                               ("fliplr", m[:, ::-1].copy(), fr.fliplr_flows(F), skip[:, ::-1])):
        Ft, dbgt = dynamics.masks_to_flows(mt, return_debug=True)
        assert np.array_equal(fr.centre_mask(mt, dbgt["centers"]), sk), name       # the centres move with the map
        d = np.abs(Ft - want).max(0)
        print(f"{name}: max |difference| off the centres = {d[~sk].max():.3e}, differing pixels overall = {int((d > 1e-9).sum())}")
        assert d[~sk].max() <= 1e-9, name


def test_renumber_instances():
    from classpose_amd import augment
    m = np.array([[0, 7, 7], [1000000, 0, 3]], np.int64)
    assert np.array_equal(augment.renumber_instances(m), [[0, 2, 2], [3, 0, 1]])
    assert augment.renumber_instances(m).dtype == np.int32
    assert np.array_equal(augment.renumber_instances(np.array([[5, 9]])), [[1, 2]])          # no background at all
    assert np.array_equal(augment.renumber_instances(np.zeros((2, 2), np.uint16)), np.zeros((2, 2)))
    with pytest.raises(ValueError, match="non-negative"):
        augment.renumber_instances(np.array([[0, -1]]))
    with pytest.raises(ValueError):
        augment.renumber_instances(np.zeros((2, 2), np.float32))


def test_new_entry_points_are_declared_bound_and_exported():
    from classpose_amd import _lib
    names = {"cpx_masks_to_flows": 8, "cpx_warp_affine_pool_flow_f32": 14, "cpx_seg_loss_workspace_bytes": 3, "cpx_seg_loss": 13}
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    for name, nargs in names.items():
        assert name in declared and len(_lib.SIGNATURES[name][1]) == nargs, name
    assert _lib.ABI_VERSION == 3
    assert "unpinned" in hdr or "not pinned" in hdr                      # the cellpose restatements say so
    if os.path.exists(_lib.LIB_PATH):
        import ctypes
        L = ctypes.CDLL(_lib.LIB_PATH)
        for name in names:
            assert hasattr(L, name), name
