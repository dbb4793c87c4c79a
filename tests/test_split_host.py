"""No GPU: the splitting rule of csrc/cpx_split.hip restated on the CPU (tests/split_reference.py) -- its distance map against
scipy's Euclidean transform and against a brute-force statement, and the outcome of the scenes the device tests stand on, proven
here at the default parameters -- then the C ABI entries, the wrappers' checks that run before any device is touched, and the
validation of ``train_head --split_touching_cells``."""
import os
import re
import subprocess

import numpy as np
import pytest

import components_reference as cr
import split_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- a. the distance map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,shape", [(1, (40, 57)), (2, (70, 66)), (3, (9, 130))])
def test_distance_map_equals_scipy_per_instance(seed, shape):
    from scipy import ndimage
    m = sr.touching_regions(shape, seed)
    ids = np.unique(m[m != 0])
    assert len(ids) >= 4 and (m == 0).any()                                 # every instance has a pixel of another value in the frame
    d2 = sr.distance_sq(m)
    assert d2.dtype == np.int32 and not d2[m == 0].any()
    for v in ids:
        want = np.rint(ndimage.distance_transform_edt(m == v) ** 2).astype(np.int64)
        assert np.array_equal(d2[m == v], want[m == v]), v
    assert np.array_equal(d2, sr.distance_sq_brute(m))


def test_distance_map_without_a_site_and_on_the_border():
    H, W = 7, 12
    assert (sr.distance_sq(np.full((H, W), 3, np.int32)) == H * H + W * W).all()
    assert not sr.distance_sq(np.zeros((H, W), np.int32)).any()
    m = np.ones((H, W), np.int32)
    m[2, 9] = 0                                                             # one site: the border is none
    ys, xs = np.mgrid[:H, :W]
    want = (ys - 2) ** 2 + (xs - 9) ** 2
    assert np.array_equal(sr.distance_sq(m), want) and np.array_equal(sr.distance_sq_brute(m), want)
    m[2, 9] = 2                                                             # another id is a site like the background
    want[2, 9] = 1
    assert np.array_equal(sr.distance_sq(m), want)
    for name in ("seams", "thin", "size_65x67"):
        for img in sr.CASES[name]:
            assert np.array_equal(sr.distance_sq(img), sr.distance_sq_brute(img)), name


# ---- the scenes at the defaults ----------------------------------------------------------------------------------------------------
def _seeds_yx(name, *params):
    W = sr.CASES[name].shape[2]
    return [divmod(int(p), W) for p in sr.expected(name, *params)[2][0]]


def test_two_discs_are_cut_on_the_bisector():
    m = sr.CASES["two_discs"][0]
    labels, counts, _seeds, d2 = sr.expected("two_discs")
    assert cr.label_scipy(m, 8)[1] == 1                                     # one component before
    assert counts.tolist() == [2] and _seeds_yx("two_discs") == [(24, 23), (24, 37)] and d2[0, 24, 23] == d2[0, 24, 37] == 101
    xs = np.mgrid[:m.shape[0], :m.shape[1]][1]
    # column 30 is as far from one centre as from the other: it goes to the raster-earlier seed, the left one
    assert np.array_equal(labels[0], np.where(m != 0, np.where(xs <= 30, 1, 2), 0))


def test_ellipse_stays_whole():
    labels, counts, seeds, _d2 = sr.expected("ellipse")
    assert counts.tolist() == [1] and len(seeds[0]) == 1 and np.array_equal(labels[0], sr.CASES["ellipse"][0])


def test_grid_of_touching_discs_gives_nine():
    m = sr.CASES["disc_grid"][0]
    assert cr.label_scipy(m, 4)[1] == 1
    labels, counts, _seeds, _d2 = sr.expected("disc_grid")
    assert counts.tolist() == [9] and _seeds_yx("disc_grid") == [(13 + 20 * i, 13 + 20 * j) for i in range(3) for j in range(3)]
    ys, xs = np.mgrid[:m.shape[0], :m.shape[1]]
    cell = 1 + 3 * np.clip((ys - 13 + 9) // 20, 0, 2) + np.clip((xs - 13 + 9) // 20, 0, 2)       # a tie goes up or left
    assert np.array_equal(labels[0], np.where(m != 0, cell, 0))


def test_thin_instance_is_left_whole_and_a_plateau_has_one_seed():
    m = sr.CASES["thin"][0]
    labels, counts, seeds, d2 = sr.expected("thin")
    assert d2[0][m == 1].max() < 4 and counts.tolist() == [2] and np.array_equal(labels[0], m)
    assert (d2[0, 34, 4:86] == 4).all() and _seeds_yx("thin") == [(34, 3)]    # 82 equal pixels in a row: the first one


@pytest.mark.parametrize("name,first", [("twin_peaks", (9, 62)), ("twin_peaks_vertical", (62, 9))])
def test_two_equal_peaks_in_one_window_give_the_raster_earlier_seed(name, first):
    m = sr.CASES[name][0]
    labels, counts, _seeds, d2 = sr.expected(name)
    top = np.argwhere(d2[0] == d2[0].max())
    assert len(top) == 2 and max(abs(top[0] - top[1])) == 4 and tuple(top[0]) == first         # argwhere is in raster order
    assert _seeds_yx(name) == [first] and counts.tolist() == [1] and np.array_equal(labels[0], m)
    assert sr.expected(name, 1, 1)[1].tolist() == [2]                       # a window that holds only one of them: two seeds


def test_the_device_cases_cover_what_they_claim():
    assert [sr.CASES[f"size_{h}x{w}"].shape for h, w in sr.SIZES] == [(3, h, w) for h, w in sr.SIZES]
    assert sr.SIZES == [(1, 1), (1, 70), (70, 1), (63, 65), (65, 67), (130, 70)] and sr.PARAMETERS == [(5, 2), (1, 1), (9, 2)]
    maps = sr.CASES["size_130x70"]
    assert (maps[1] == 1).all() and (sr.expected("size_130x70")[3][1] == 130 * 130 + 70 * 70).all()
    assert len(sr.expected("size_130x70", 1, 1)[2][2]) > 10 * 64              # one instance, hundreds of seeds, every seam
    a = maps[0]
    touching = (a[:, 1:] != a[:, :-1]) & (a[:, 1:] != 0) & (a[:, :-1] != 0)
    assert touching.sum() > 20 and touching[:, 60:66].any()                  # different ids side by side, also at the seam
    s = sr.CASES["seams"][0]
    assert s[30, 63] == s[30, 64] == 1 and s[69, 110] == 5 and s[70, 110] == 6 and s[65, 127] == 5 and s[65, 128] == 7
    yx = _seeds_yx("seams")
    assert (30, 57) in yx and (30, 71) in yx and (60, 20) in yx and (64, 20) not in yx and (100, 62) in yx and (100, 66) not in yx
    assert (0, 0) in yx                                                     # the corner disc: its window is clipped on two sides
    assert sr.expected("seams", 5, 2, 4)[1].tolist() == sr.expected("seams", 5, 2, 8)[1].tolist() == [9]


def test_connectivity_matters_for_the_last_stage():
    # two seeds whose cells meet only at a corner inside ONE instance cannot happen (a cell is convex inside its instance), but
    # an instance given as two blobs with one id that touch at a corner is one under 8 and two under 4
    m = np.zeros((12, 12), np.int32)
    m[1:6, 1:6] = 1
    m[6:11, 6:11] = 1
    assert sr.split_image(m, 5, 2, 8)[1] == 1 and sr.split_image(m, 5, 2, 4)[1] == 2
    assert sr.split_image(m, 1, 1, 8)[1] == sr.split_image(m, 1, 1, 4)[1] == 2      # two seeds: the bisector separates the blobs


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
NAMES = ("cpx_distance_sq", "cpx_split_workspace_bytes", "cpx_split_touching")


def test_split_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    for name in NAMES:
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert [len(_lib.SIGNATURES[name][1]) for name in NAMES] == [8, 4, 16]
    assert _lib.ABI_VERSION == 3                                            # additive: no bump
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert re.search(r"^NAMES = .*\bcpx_split\b", mk, re.M) and "cpx_split.o: cpx_split.hip" in mk


def test_limits_are_those_of_the_source():
    from classpose_amd import _lib, ops
    src = open(os.path.join(_lib.CSRC, "cpx_split.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (SP_[A-Z0-9_]+) (\d+)\b", src, re.M)}
    assert consts["SP_MAX_PX"] == ops.COMPONENTS_MAX_PIXELS and consts["SP_MAX_DIAG2"] == ops.SPLIT_MAX_DIAG2 == 1 << 30
    assert consts["SP_MAX_WINDOW"] == ops.SPLIT_MAX_MIN_DISTANCE and consts["SP_MAX_RADIUS"] == ops.SPLIT_MAX_MIN_RADIUS
    assert consts["SP_BLOCK"] % consts["SP_THR"] == 0


def test_workspace_query_and_refusals_without_a_device():
    from classpose_amd import _lib
    L = _lib.lib()
    q, cc = L.cpx_split_workspace_bytes, L.cpx_label_components_workspace_bytes
    assert q(1, 1, 1, 1) > 0 and q(65535, 1, 1, 1) > 0 and q(1, 1 << 14, 1 << 14, 1 << 28) > 0
    assert q(3, 200, 333, 1000) >= 3 * 200 * 333 * 4 * 4 + 3 * 1000 * 4 + cc(3, 200, 333)
    assert q(3, 200, 333, 2000) > q(3, 200, 333, 1000) > q(2, 200, 333, 1000)
    for bad in ((0, 8, 8, 8), (65536, 8, 8, 8), (1, 0, 8, 8), (1, 8, 0, 8), (1, 8, 8, 0), (1, 8, 8, 65), (1, 1, 1 << 28, 8),
                (1, 32768, 1, 8), (1, 23171, 23171, 8)):
        assert q(*bad) == 0, bad
    assert q(1, 32767, 1, 8) > 0 and q(1, 23170, 23170 // 2, 8) > 0
    f, big = L.cpx_split_touching, 1 << 40
    null = (None,) * 5
    # refused before any launch, with null pointers
    assert f(None, 1, 8, 8, 5, 2, 6, 8, *null, None, big, None) != 0 and b"connectivity" in L.cpx_last_error()
    assert f(None, 1, 8, 8, 0, 2, 8, 8, *null, None, big, None) != 0 and b"min_distance" in L.cpx_last_error()
    assert f(None, 1, 8, 8, 65, 2, 8, 8, *null, None, big, None) != 0 and b"min_distance" in L.cpx_last_error()
    assert f(None, 1, 8, 8, 5, 0, 8, 8, *null, None, big, None) != 0 and b"min_radius" in L.cpx_last_error()
    assert f(None, 1, 8, 8, 5, 2, 8, 65, *null, None, big, None) != 0 and b"seed_cap" in L.cpx_last_error()
    assert f(None, 1, 8, 0, 5, 2, 8, 8, *null, None, big, None) != 0
    assert f(None, 1, 8, 8, 5, 2, 8, 8, *null, None, q(1, 8, 8, 8) - 1, None) != 0 and b"workspace_bytes" in L.cpx_last_error()
    assert f(None, 1, 8, 8, 5, 2, 8, 8, *null, None, q(1, 8, 8, 8), None) != 0 and b"inst &&" in L.cpx_last_error()
    assert f(4096, 1, 8, 8, 5, 2, 8, 8, 4096, 8192, 8192, 8192, 8192, 8192, big, None) != 0 and b"labels" in L.cpx_last_error()
    assert f(None, 0, 8, 8, 5, 2, 8, 8, *null, None, 0, None) == 0                                  # n == 0: a no-op
    d = L.cpx_distance_sq
    assert d(None, 1, 8, 8, None, None, 8 * 8 * 4 - 1, None) != 0 and b"workspace_bytes" in L.cpx_last_error()
    assert d(None, 1, 8, 8, None, None, 8 * 8 * 4, None) != 0 and b"map &&" in L.cpx_last_error()
    assert d(4096, 1, 8, 8, 4096, 8192, 8 * 8 * 4, None) != 0 and b"d2" in L.cpx_last_error()
    assert d(None, 1, 32768, 1, None, None, big, None) != 0 and d(None, 0, 8, 8, None, None, 0, None) == 0


# ---- the wrappers' checks before any device --------------------------------------------------------------------------------------
def test_wrappers_refuse_bad_arguments_before_any_launch():
    import torch
    from classpose_amd import dataset_stats as ds, ops
    ok = torch.zeros((1, 8, 8), dtype=torch.int32)
    for fn in (ops.distance_sq, ops.split_touching):
        with pytest.raises(ValueError, match="int32"):
            fn(ok.to(torch.int64))
        with pytest.raises(ValueError, match="int32"):
            fn(ok[0])
        with pytest.raises(ValueError, match="int32"):
            fn(np.zeros((1, 8, 8), np.int32))
        with pytest.raises(ValueError, match="cuda"):
            fn(ok)
    maps = np.zeros((2, 8, 8), np.int32)
    with pytest.raises(RuntimeError, match="cuda device"):
        ds.instances_from_classes(maps, device="cpu", split_touching=True)
    with pytest.raises(RuntimeError, match="cuda device"):
        ds.label_stats(maps, maps, 3, device="cpu", label_instances=True, split_touching=True)
    assert "split_touching" in ds.__doc__ and "peak_local_max" in ds.__doc__


def test_split_touching_false_takes_the_old_path(monkeypatch):
    """``instances_from_classes`` with recording stand-ins for the two device calls (and host tensors for the device's): without
    the option only the labeller runs, with the same arguments as before; with it the labeller's maps go through the cut."""
    import torch
    from classpose_amd import dataset_stats as ds, ops
    calls = []

    def label_components(part, connectivity, workspace=None):
        calls.append(("label", tuple(part.shape), connectivity))
        return part * 10, torch.full((part.shape[0],), 3, dtype=torch.int32)

    def split_touching(inst, min_distance, min_radius, connectivity):
        calls.append(("split", tuple(inst.shape), min_distance, min_radius, connectivity))
        return inst + 1, torch.full((inst.shape[0],), 5, dtype=torch.int32)

    real_empty = torch.empty
    monkeypatch.setattr(ops, "label_components", label_components)
    monkeypatch.setattr(ops, "split_touching", split_touching)
    monkeypatch.setattr(ds, "_chunk_to_device", lambda x, lo, hi, dtype, dev: torch.from_numpy(np.asarray(x[lo:hi])).to(dtype))
    monkeypatch.setattr(torch, "empty", lambda *a, device=None, **k: real_empty(*a, **k))
    classes = np.array([[[0, 2, -100]], [[1, 1, 0]], [[3, 0, 0]]], np.int16)
    out, counts = ds.instances_from_classes(classes, device="cuda:0", chunk=2)
    assert calls == [("label", (2, 1, 3), 4), ("label", (1, 1, 3), 4)] and counts.tolist() == [3, 3, 3]
    assert out.tolist() == [[[0, 20, 0]], [[10, 10, 0]], [[30, 0, 0]]]
    again, _ = ds.instances_from_classes(classes, 4, "cuda:0", 2, False)      # the option is the fifth argument, after the old four
    assert again.tolist() == out.tolist() and len(calls) == 4 and not any(c[0] == "split" for c in calls)
    del calls[:]
    out, counts = ds.instances_from_classes(classes, connectivity=8, device="cuda:0", split_touching=True, min_distance=7, min_radius=3)
    assert calls == [("label", (3, 1, 3), 8), ("split", (3, 1, 3), 7, 3, 8)] and counts.tolist() == [5, 5, 5]
    assert out.tolist() == [[[1, 21, 1]], [[11, 11, 1]], [[31, 1, 1]]]
    with pytest.raises(ValueError, match="label_instances=True"):
        ds.label_stats(classes, classes, 4, device="cuda:0", split_touching=True)


def test_split_summary_counts_cut_components():
    import torch
    from classpose_amd import dataset_stats as ds
    before = torch.tensor([[[1, 1, 1, 0, 2, 2]], [[1, 0, 0, 0, 0, 0]]], dtype=torch.int32)
    after = torch.tensor([[[1, 2, 3, 0, 4, 4]], [[1, 0, 0, 0, 0, 0]]], dtype=torch.int32)
    assert ds.split_summary(before, after) == (3, 1, 5)
    assert ds.split_summary(before, before) == (3, 0, 3) and ds.split_summary(before * 0, before * 0) == (0, 0, 0)


# ---- train_head --split_touching_cells ---------------------------------------------------------------------------------------------
REQ = ["--images", "X.npy", "--labels", "Y.npy", "--pretrained_model", "ck.pt", "--save_path", "out", "--model_name", "m"]


def test_split_flags_parse_and_go_with_instances_from_labels():
    from classpose_amd.entrypoints import train_head
    p = train_head.build_parser()
    a = p.parse_args(REQ)
    assert a.split_touching_cells is False and a.split_min_distance is None and a.split_min_radius is None
    train_head.check_args(a)
    a = p.parse_args(REQ + ["--instances_from_labels", "--split_touching_cells"])
    train_head.check_args(a)
    assert a.split_touching_cells is True and a.split_min_distance is None and a.split_min_radius is None
    a = p.parse_args(REQ + ["--instances_from_labels", "--instance_connectivity", "8", "--split_touching_cells", "--split_min_distance", "7",
                            "--split_min_radius", "3", "--auto_class_weights", "--train_flow_head"])
    train_head.check_args(a)
    assert (a.split_min_distance, a.split_min_radius) == (7, 3)
    a = p.parse_args(REQ + ["--instances_from_labels", "--split_touching_cells", "--split_min_distance", "9"])
    train_head.check_args(a)
    assert (a.split_min_distance, a.split_min_radius) == (9, None)
    for extra in ([], ["--instances", "I.npy"], ["--auto_class_weights", "--instances", "I.npy"]):
        with pytest.raises(SystemExit, match="--split_touching_cells goes with --instances_from_labels"):
            train_head.check_args(p.parse_args(REQ + extra + ["--split_touching_cells"]))
        with pytest.raises(SystemExit, match="--split_min_distance goes with --instances_from_labels --split_touching_cells"):
            train_head.check_args(p.parse_args(REQ + extra + ["--split_min_distance", "5"]))
    with pytest.raises(SystemExit, match="--split_touching_cells goes with"):
        train_head.check_args(p.parse_args(REQ[4:] + ["--data_path", "DIR", "--split_touching_cells"]))
    with pytest.raises(SystemExit, match="--split_min_radius goes with"):
        train_head.check_args(p.parse_args(REQ + ["--instances_from_labels", "--split_min_radius", "2"]))
    for flag, value in (("--split_min_distance", "0"), ("--split_min_distance", "65"), ("--split_min_radius", "0")):
        with pytest.raises(SystemExit, match=f"{flag}: 1 to"):
            train_head.check_args(p.parse_args(REQ + ["--instances_from_labels", "--split_touching_cells", flag, value]))
    # without the flag nothing moves: the old refusal and the old help
    with pytest.raises(SystemExit, match="--instance_connectivity goes with --instances_from_labels"):
        train_head.check_args(p.parse_args(REQ + ["--instance_connectivity", "4"]))
    helptext = " ".join(p.format_help().split())
    assert "--split_touching_cells" in helptext and "become one instance" in helptext

