"""No GPU: the connected-component rule stated twice on the CPU (tests/components_reference.py: scipy per value with an explicit
renumbering, against a breadth-first fill), the C ABI entries of csrc/cpx_components.hip (declared, bound, exported; the workspace
query and the refusals that need no device), the argument checks of the wrappers that run before any device is touched, and the
validation of ``train_head --instances_from_labels``."""
import os
import re
import subprocess

import numpy as np
import pytest

import components_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule, twice -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(cr.CASES))
def test_scipy_and_fill_versions_agree(name, connectivity):
    labels, counts = cr.expected(name, connectivity)
    for k, m in enumerate(cr.CASES[name]):
        lab, cnt = cr.label_fill(m, connectivity)
        assert cnt == counts[k] and np.array_equal(lab, labels[k]), (name, k)
        assert np.array_equal(lab > 0, m != 0) and (cnt == 0 or lab.max() == cnt)
    if name in cr.KNOWN_COUNTS:
        assert counts.tolist() == cr.KNOWN_COUNTS[name][connectivity]


def test_literal_labels_of_the_rule():
    m = np.array([[0, 5, 0, 5],
                  [5, 0, 0, 5],
                  [0, -1, -1, 0],
                  [7, 0, 0, -1]], np.int32)
    lab4, n4 = cr.label_scipy(m, 4)
    lab8, n8 = cr.label_scipy(m, 8)
    assert n4 == 6 and lab4.tolist() == [[0, 1, 0, 2], [3, 0, 0, 2], [0, 4, 4, 0], [5, 0, 0, 6]]
    assert n8 == 4 and lab8.tolist() == [[0, 1, 0, 2], [1, 0, 0, 2], [0, 3, 3, 0], [4, 0, 0, 3]]
    # a U open to the top whose right prong starts higher: ONE component, numbered from the right prong's first pixel
    u = np.array([[0, 0, 2, 0, 1],
                  [1, 0, 2, 0, 1],
                  [1, 1, 1, 1, 1]], np.int32)
    assert cr.label_scipy(u, 4)[0].tolist() == cr.label_fill(u, 4)[0].tolist() == [[0, 0, 1, 0, 2], [2, 0, 1, 0, 2], [2, 2, 2, 2, 2]]


def test_the_shapes_sit_on_both_sides_of_the_tile():
    from classpose_amd import _lib, ops
    src = open(os.path.join(_lib.CSRC, "cpx_components.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (CC_[A-Z_]+) (\d+)\b", src, re.M)}
    assert consts["CC_TILE"] == ops.COMPONENTS_TILE == cr.TILE == 64 and consts["CC_MAX_PX"] == ops.COMPONENTS_MAX_PIXELS == 1 << 28
    assert consts["CC_TILE"] ** 2 == consts["CC_TILE_PX"] == consts["CC_THR"] * consts["CC_STRIP"]
    T = cr.TILE
    shapes = {m.shape[1:] for m in cr.CASES.values()}
    assert {(1, 1), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, T + 3), (300, 520)} <= shapes
    assert any(h == 1 and w > T for h, w in shapes) and any(w == 1 and h > T for h, w in shapes) and any(w % 64 for _h, w in shapes)
    assert cr.CASES["serpentine_257"].shape == (1, 257, 257) and int(cr.CASES["serpentine_257"].sum()) > 257 * 257 // 2
    assert int(cr.CASES["spiral_257"].sum()) > 257 * 257 // 2 - 257
    # the U: prongs in tile columns 0 and 2 from tile row 0, base in tile row 2, first pixel in the RIGHT prong
    u = cr.CASES["u_and_combs"][0]
    first = np.argwhere(u == 4)[0]
    assert first.tolist() == [5, 2 * T + 30] and u[20, 10] == 4 and u[19, 10] == 0 and u[2 * T + 30, 10:2 * T + 31].all()


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_components_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    for name in ("cpx_label_components_workspace_bytes", "cpx_label_components"):
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert len(_lib.SIGNATURES["cpx_label_components"][1]) == 10 and len(_lib.SIGNATURES["cpx_label_components_workspace_bytes"][1]) == 3
    assert _lib.ABI_VERSION == 3 and "run_cellpose_semantic.py:89-100" in hdr and "train_utils.py:407-436" in hdr
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert re.search(r"^NAMES = .*\bcpx_components\b", mk, re.M) and "cpx_components.o: cpx_components.hip" in mk


def test_workspace_query_and_refusals_without_a_device():
    from classpose_amd import _lib
    L = _lib.lib()
    q = L.cpx_label_components_workspace_bytes
    assert q(1, 1, 1) > 0 and q(65535, 1, 1) > 0 and q(1, 1 << 14, 1 << 14) >= 4 << 28 and q(1, 1, 1 << 28) > 0
    assert q(8, 200, 333) >= 8 * 200 * 333 * 4 and q(8, 200, 333) > q(7, 200, 333)
    for bad in ((0, 8, 8), (65536, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, 0), (1, -8, 8), (1, (1 << 14) + 1, 1 << 14), (1, 1 << 28, 2),
                (1, 1 << 20, 1 << 20)):
        assert q(*bad) == 0, bad
    f = L.cpx_label_components
    big = 1 << 40
    # refused before any launch, with null pointers: the connectivity, the geometry, the workspace size, then the pointers
    assert f(None, 1, 8, 8, 3, None, None, None, big, None) != 0 and b"connectivity" in L.cpx_last_error()
    assert f(None, 1, 8, 8, 6, None, None, None, big, None) != 0 and b"connectivity" in L.cpx_last_error()
    assert f(None, 1, 0, 8, 8, None, None, None, big, None) != 0 and b"invalid argument" in L.cpx_last_error()
    assert f(None, 65536, 8, 8, 8, None, None, None, big, None) != 0
    assert f(None, 1, 8, 8, 8, None, None, None, q(1, 8, 8) - 1, None) != 0 and b"workspace_bytes" in L.cpx_last_error()
    assert f(None, 1, 8, 8, 4, None, None, None, q(1, 8, 8), None) != 0 and b"map &&" in L.cpx_last_error()
    assert f(4096, 1, 8, 8, 4, 4096, 8192, 8192, q(1, 8, 8), None) != 0 and b"labels" in L.cpx_last_error()      # labels aliases map
    assert f(None, 0, 8, 8, 8, None, None, None, 0, None) == 0                                                    # n == 0: a no-op


# ---- the wrappers' checks before any device --------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_before_any_launch():
    import torch
    from classpose_amd import dataset_stats as ds, ops, train_data
    ok = torch.zeros((1, 8, 8), dtype=torch.int32)
    with pytest.raises(ValueError, match="int32"):
        ops.label_components(ok.to(torch.int64))
    with pytest.raises(ValueError, match="int32"):
        ops.label_components(ok[0])
    with pytest.raises(ValueError, match="int32"):
        ops.label_components(np.zeros((1, 8, 8), np.int32))
    with pytest.raises(ValueError, match="connectivity"):
        ops.label_components(ok, connectivity=3)
    with pytest.raises(ValueError, match="cuda"):
        ops.label_components(ok)
    maps = np.zeros((2, 8, 8), np.int32)
    with pytest.raises(RuntimeError, match="cuda device"):
        ds.instances_from_classes(maps, device="cpu")
    with pytest.raises(RuntimeError, match="cuda device"):
        ds.label_stats(maps, maps, 3, device="cpu", label_instances=True)
    with pytest.raises(RuntimeError, match="cuda device"):
        train_data.ragged_label_stats([maps[0]], [maps[0]], 3, device="cpu", label_instances=True, connectivity=4)
    assert "Not built" not in ds.__doc__ and "label_instances=True" in ds.__doc__


# ---- train_head --instances_from_labels ------------------------------------------------------------------------------------------
REQ = ["--images", "X.npy", "--labels", "Y.npy", "--pretrained_model", "ck.pt", "--save_path", "out", "--model_name", "m"]
TEST = ["--test_images", "TX.npy", "--test_labels", "TY.npy"]


def test_instances_from_labels_validation():
    from classpose_amd.entrypoints import train_head
    p = train_head.build_parser()
    a = p.parse_args(REQ)
    assert a.instances_from_labels is False and a.instance_connectivity is None
    train_head.check_args(a)
    # what used to need --instances passes with the new flag, alone and all together, with and without a validation set
    for flags in (["--auto_class_weights"], ["--oversampling_method", "custom"], ["--rescale", "--augment", "geometry"],
                  ["--min_train_masks", "1"], ["--train_flow_head"], ["--freeze", "backbone", "neck"], ["--train_flow_head"] + TEST,
                  ["--auto_class_weights", "--oversampling_method", "custom", "--rescale", "--augment", "geometry", "--min_train_masks", "2",
                   "--train_flow_head", "--instance_connectivity", "8"] + TEST):
        a = p.parse_args(REQ + flags + ["--instances_from_labels"])
        train_head.check_args(a)
        assert a.instances_from_labels is True
    assert p.parse_args(REQ + ["--instances_from_labels", "--instance_connectivity", "8"]).instance_connectivity == 8
    # every refused combination
    for flags, msg in ((["--instances", "I.npy"], "not with --instances"),
                       (["--test_instances", "TI.npy"] + TEST, "not with --test_instances"),
                       (["--instances", "I.npy", "--test_instances", "TI.npy"] + TEST, "not with --instances, --test_instances")):
        with pytest.raises(SystemExit, match=msg):
            train_head.check_args(p.parse_args(REQ + flags + ["--instances_from_labels"]))
    with pytest.raises(SystemExit, match="not with --data_path"):
        train_head.check_args(p.parse_args(REQ[4:] + ["--data_path", "DIR", "--instances_from_labels"]))
    for extra in ([], ["--instances", "I.npy"], ["--auto_class_weights", "--instances", "I.npy"]):
        with pytest.raises(SystemExit, match="--instance_connectivity goes with --instances_from_labels"):
            train_head.check_args(p.parse_args(REQ + extra + ["--instance_connectivity", "4"]))
    with pytest.raises(SystemExit, match="--instance_connectivity goes with"):
        train_head.check_args(p.parse_args(REQ[4:] + ["--data_path", "DIR", "--instance_connectivity", "8"]))
    with pytest.raises(SystemExit):
        p.parse_args(REQ + ["--instances_from_labels", "--instance_connectivity", "6"])
    # without the flag the old refusals stand, and now name it
    for flags in (["--auto_class_weights"], ["--min_train_masks", "1"]):
        with pytest.raises(SystemExit, match="needs --instances or --instances_from_labels"):
            train_head.check_args(p.parse_args(REQ + flags))
    with pytest.raises(SystemExit, match="needs --instances or --data_path, or --instances_from_labels"):
        train_head.check_args(p.parse_args(REQ + ["--train_flow_head"]))
    with pytest.raises(SystemExit, match="needs --test_instances or --instances_from_labels"):
        train_head.check_args(p.parse_args(REQ + ["--train_flow_head", "--instances", "I.npy"] + TEST))
    with pytest.raises(SystemExit, match="needs --augment"):
        train_head.check_args(p.parse_args(REQ + ["--rescale", "--instances_from_labels"]))
    helptext = " ".join(p.format_help().split())
    assert "--instances_from_labels" in helptext and "become one instance" in helptext
