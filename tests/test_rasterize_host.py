"""No GPU: the rasterisation rule on the CPU (tests/rasterize_reference.py: exact integers against numpy float64 in the kernel's
operand order, both against matplotlib away from ring pixels), the GeoJSON reader and the bounding-box culling of
classpose_amd.annotations, the C ABI entries of csrc/cpx_rasterize.hip (declared, bound, exported; workspace queries), the
argument checks of ops.rasterize_polygons / ops.ids_to_classes that run before any device is touched, and the argument errors
of the two command-line tools."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import rasterize_reference as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule, twice -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rr.CASES))
def test_exact_and_float64_versions_agree(name):
    rings, shape = rr.CASES[name]
    xy, off, val, _ = rr.pack(rings)
    a = rr.rasterize(xy, off, val, shape)
    b = rr.rasterize(xy, off, val, shape, masks=rr.ring_masks_float)
    assert np.array_equal(a, b)


def test_literal_pixels_of_the_rule():
    # the unit square's corners are centres: boundary included -> 2 x 2; the half-open rule alone would give 1 x 1
    m = rr.rasterize(*rr.pack([[(1, 1), (2, 1), (2, 2), (1, 2)]])[:3], (4, 4))[0]
    assert m.tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    # edges between centres: only the inside
    m = rr.rasterize(*rr.pack([[(0.5, 0.5), (2.5, 0.5), (2.5, 2.5), (0.5, 2.5)]])[:3], (4, 4))[0]
    assert m.tolist() == [[0, 0, 0, 0], [0, 1, 1, 0], [0, 1, 1, 0], [0, 0, 0, 0]]
    # a collinear ring paints its lattice points, a two-vertex ring nothing, a bow-tie is even-odd
    assert np.argwhere(rr.rasterize(*rr.pack(rr.SINGLE["collinear"])[:3], rr.SHAPE)[0]).tolist() == [[i, i] for i in range(3, 21)]
    assert not rr.rasterize(*rr.pack(rr.SINGLE["two_vertices"])[:3], rr.SHAPE).any()
    bow = rr.rasterize(*rr.pack(rr.SINGLE["bowtie"])[:3], rr.SHAPE)[0]
    assert bow[17, 10] == 1 and bow[17, 25] == 1 and bow[10, 17] == 0 and bow[25, 17] == 0 and bow[10, 10] == 1     # left and right lobes
    # the spur: painted because its centres are ON the ring, though their crossing number is even
    spur = rr.rasterize(*rr.pack(rr.SINGLE["spur"])[:3], rr.SHAPE)[0]
    assert spur[12, 21:27].all() and not spur[11, 21:27].any() and not spur[13, 21:27].any()
    # closed == unclosed
    assert np.array_equal(rr.rasterize(*rr.pack(rr.SINGLE["triangle"])[:3], rr.SHAPE),
                          rr.rasterize(*rr.pack(rr.SINGLE["triangle_closed"])[:3], rr.SHAPE))


def test_both_versions_agree_with_matplotlib_away_from_the_ring():
    """matplotlib.path.Path.contains_points is a crossing-number test with its own boundary convention, so pixels whose centre
    is ON a ring are left out of this comparison -- and only those.  Every shared case takes part, the self-crossing ones too."""
    from matplotlib.path import Path
    ring_px = compared = excluded = 0
    for name, (rings, (H, W)) in rr.CASES.items():
        ring = np.asarray(rings[0], np.float64)
        if len(ring) < 3:
            continue
        r0, c0, par, on = rr.ring_masks_exact(ring, H, W)
        f0 = rr.ring_masks_float(ring, H, W)
        assert (r0, c0) == f0[:2] and np.array_equal(par, f0[2]) and np.array_equal(on, f0[3])
        if par.size == 0:
            continue
        rows, cols = np.mgrid[r0:r0 + par.shape[0], c0:c0 + par.shape[1]]
        inside = Path(ring, closed=False).contains_points(np.stack([cols.ravel(), rows.ravel()], 1).astype(np.float64)).reshape(par.shape)
        assert np.array_equal(inside[~on], par[~on]), name
        ring_px += int(on.sum()); excluded += int(on.sum()); compared += int((~on).sum())
    share = excluded / (excluded + compared)
    print(f"matplotlib cross-check: {compared} pixels compared, {excluded} on a ring left out ({100 * share:.2f} %), ring pixels of the exact version: {ring_px}")
    assert compared > 100000 and excluded <= ring_px and share < 0.05


# ---- the GeoJSON reader ----------------------------------------------------------------------------------------------------------
def _feat(kind, coords, name=None, fid=None):
    f = {"type": "Feature", "geometry": {"type": kind, "coordinates": coords}, "properties": {"objectType": "annotation"}}
    if name is not None:
        f["properties"]["classification"] = {"name": name, "color": [1, 2, 3]}
    if fid is not None:
        f["id"] = fid
    return f


SQ = [[2, 2], [10, 2], [10, 10], [2, 10], [2, 2]]
HOLE = [[4, 4], [8, 4], [8, 8], [4, 8], [4, 4]]
FEATURES = [
    _feat("Polygon", [SQ], "tumour", "a"),
    _feat("Point", [5.0, 6.0], "tumour"),
    _feat("Polygon", [[[20, 20], [30, 20], [30, 30], [20, 30], [20, 20]], [[22, 22], [28, 22], [28, 28], [22, 28], [22, 22]]], "stroma"),
    _feat("MultiPolygon", [[[[40, 2], [44, 2], [44, 6]]], [[[50.5, 2.25], [58, 2], [58, 9], [50, 9]], [[52, 4], [56, 4], [56, 7]]]], "tumour"),
]


def _write(tmp_path, name, obj):
    p = tmp_path / name
    p.write_text(json.dumps(obj))
    return str(p)


def test_load_features_collection_and_bare_list(tmp_path):
    from classpose_amd import annotations as an
    a = an.load_features(_write(tmp_path, "fc.geojson", {"type": "FeatureCollection", "features": FEATURES}), ["tumour", "stroma"])
    b = an.load_features(_write(tmp_path, "list.json", FEATURES), ["tumour", "stroma"])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a.n_features == 4 and a.n_points == 1
    assert a.feature_class.tolist() == [1, 0, 2, 1] and a.feature_class.dtype == np.uint8
    # rings: 1 (polygon) + 2 (polygon with a hole) + 3 (two parts, the second with a hole); the Point keeps its position
    assert a.ring_feature.tolist() == [0, 2, 2, 3, 3, 3] and a.ring_feature.dtype == np.int32
    assert a.ring_off.tolist() == [0, 5, 10, 15, 18, 22, 25] and a.ring_off.dtype == np.int64
    assert a.xy.dtype == np.float64 and a.xy.shape == (25, 2)
    assert a.xy[18].tolist() == [50.5, 2.25]
    one = an.load_features(_write(tmp_path, "one.json", FEATURES[0]), ["tumour"])
    assert one.n_features == 1 and one.ring_off.tolist() == [0, 5]


def test_load_features_unknown_class_and_bad_geometry(tmp_path):
    from classpose_amd import annotations as an
    path = _write(tmp_path, "fc.geojson", {"type": "FeatureCollection", "features": FEATURES})
    with pytest.raises(ValueError, match=r"feature 2.*'stroma'"):
        an.load_features(path, ["tumour"])
    a = an.load_features(path, ["tumour"], ignore_unknown=True)
    assert a.feature_class.tolist() == [1, 0, 0, 1] and a.ring_feature.tolist() == [0, 2, 2, 3, 3, 3]      # still an instance
    with pytest.raises(ValueError, match=r"feature 0 \(id a\)"):
        an.load_features(path, ["stroma"])
    with pytest.raises(ValueError, match="feature 0.*None"):
        an.load_features(_write(tmp_path, "noname.json", [_feat("Polygon", [SQ])]), ["tumour"])
    with pytest.raises(ValueError, match="LineString"):
        an.load_features(_write(tmp_path, "line.json", [_feat("LineString", SQ, "tumour")]), ["tumour"])
    with pytest.raises(ValueError, match="not finite"):
        an.load_features(_write(tmp_path, "nan.json", [_feat("Polygon", [[[0, 0], [1, float("nan")], [2, 2]]], "tumour")]), ["tumour"])
    with pytest.raises(ValueError, match="neither"):
        an.load_features(_write(tmp_path, "str.json", "features"), ["tumour"])
    empty = an.load_features(_write(tmp_path, "empty.json", []), ["tumour"])
    assert empty.n_features == 0 and empty.ring_off.tolist() == [0] and empty.xy.shape == (0, 2)


def test_hole_is_filled_and_later_feature_wins_on_the_cpu(tmp_path):
    """what the device tests compare against, spelled out once: local_rings + the exact rasteriser"""
    from classpose_amd import annotations as an
    a = an.load_features(_write(tmp_path, "fc.json", FEATURES + [_feat("Polygon", [[[8, 8], [24, 8], [24, 24], [8, 24]]], "stroma")]), ["tumour", "stroma"])
    xy, off, val, img = an.local_rings(a, [(0, 0, 64, 32)])
    m = rr.rasterize(xy, off, val, (32, 64), img)[0]
    assert m[25, 25] == 3 and m[21, 21] == 5 and m[9, 9] == 5 and m[5, 5] == 1 and m[2, 2] == 1 and m[6, 53] == 4
    assert val.tolist() == [1, 3, 3, 4, 4, 4, 5] and img.tolist() == [0] * 7


def test_culling_keeps_exactly_the_features_that_touch_the_region():
    from classpose_amd import annotations as an
    rng = np.random.default_rng(5)
    rings, feats = [], []
    for f in range(300):
        cx, cy = rng.integers(-40, 300, 2)
        w, h = rng.integers(1, 30, 2)
        rings.append(rr.q16([(cx, cy), (cx + w, cy + 0.5), (cx + w - 0.25, cy + h), (cx - 0.5, cy + h - 0.75)]))
        feats.append(f)
    xy, off, _, _ = rr.pack(rings)
    a = an.Annotations(xy, off, np.asarray(feats, np.int32), np.ones(300, np.uint8), 300)
    for region, ds, co in (((0, 0, 256, 256), 1.0, 0.0), ((100, 60, 64, 32), 1.0, 0.0), ((17, 33, 50, 90), 1.0, -1.0), ((0, 0, 256, 128), 2.0, 0.0)):
        x, y, w, h = region
        W, H = int(np.ceil(w / ds)), int(np.ceil(h / ds))
        kept = set(an.cull(a, region, None, ds, co).tolist())
        touching = set()
        for f in range(300):
            b = (rings[f] + co - np.array([x, y])) / ds
            if b[:, 0].min() <= W - 1 and b[:, 0].max() >= 0 and b[:, 1].min() <= H - 1 and b[:, 1].max() >= 0:
                touching.add(f)
        assert kept == touching and 0 < len(kept) < 300
        # culling drops nothing that paints: the culled call equals painting every ring (dyadic arithmetic: exact for these cases)
        lx, lo, lv, li = an.local_rings(a, [region], ds, co)
        assert sorted(set((lv - 1).tolist())) == sorted(kept)
        every = rr.rasterize(rr.q16((xy + co - np.array([x, y])) / ds), off, np.arange(1, 301, dtype=np.int32), (H, W))
        assert np.array_equal(rr.rasterize(rr.q16(lx), lo, lv, (H, W), li), every)


def test_local_rings_keeps_one_id_across_regions_and_orders_by_region():
    from classpose_amd import annotations as an
    ring = np.array([(60, 10), (70, 10), (70, 20), (60, 20)], np.float64)
    a = an.Annotations(ring, np.array([0, 4]), np.array([0], np.int32), np.array([2], np.uint8), 1)
    xy, off, val, img = an.local_rings(a, [(0, 0, 64, 64), (64, 0, 64, 64), (200, 0, 64, 64)])
    assert val.tolist() == [1, 1] and img.tolist() == [0, 1] and off.tolist() == [0, 4, 8]
    assert xy[:4, 0].tolist() == [60, 70, 70, 60] and xy[4:, 0].tolist() == [-4, 6, 6, -4]


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_rasterize_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    for name in ("cpx_rasterize_workspace_bytes", "cpx_rasterize_polygons", "cpx_ids_to_classes"):
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert len(_lib.SIGNATURES["cpx_rasterize_polygons"][1]) == 12 and len(_lib.SIGNATURES["cpx_ids_to_classes"][1]) == 6
    assert "organise-datasets.py:626-652" in hdr
    L = _lib.lib()
    q = L.cpx_rasterize_workspace_bytes
    assert q(1000, 30000, 8, 1024, 1024) >= 1000 * 24 and q(0, 0, 1, 1, 1) > 0 and q(1, 3, 1, 32768, 32768) > 0
    for bad in ((-1, 0, 1, 8, 8), (1, -1, 1, 8, 8), (1, 3, 0, 8, 8), (1, 3, 1, 0, 8), (1, 3, 1, 8, 0), (1, 3, 1, 32769, 8), (1, 3, 1, 8, 32769),
                (1 << 31, 3, 1, 8, 8)):
        assert q(*bad) == 0, bad
    # the constants the device tests probe both sides of are the kernel's
    src = open(os.path.join(_lib.CSRC, "cpx_rasterize.hip")).read()
    consts = {k: int(v) for k, v in re.findall(r"^#define (R[SL]_[A-Z_]+) (\d+)\b", src, re.M)}
    assert (consts["RS_SMALL_VERTS"], consts["RS_SMALL_AREA"], consts["RL_CHUNK"], consts["RS_MAX_DIM"]) == \
        (ops.RASTER_SMALL_MAX_VERTICES, ops.RASTER_SMALL_MAX_AREA, ops.RASTER_EDGE_CHUNK, ops.RASTER_MAX_DIM) == (256, 4096, 512, 32768)
    for n in (consts["RS_SMALL_VERTS"], consts["RL_CHUNK"], 2 * consts["RL_CHUNK"]):
        assert {n - 1, n, n + 1} <= set(rr.VERTEX_COUNTS)
    # the entry itself refuses what the query refuses, before any launch, and n_rings == 0 is a no-op without one
    assert L.cpx_rasterize_polygons(None, None, None, None, 1, 1, 0, 8, None, None, 0, None) != 0
    assert b"invalid argument" in L.cpx_last_error()
    assert L.cpx_rasterize_polygons(None, None, None, None, 0, 1, 8, 8, 4096, None, 0, None) == 0
    assert L.cpx_rasterize_polygons(None, None, None, None, 3, 1, 8, 8, 4096, None, 0, None) != 0
    assert L.cpx_ids_to_classes(None, 0, None, 0, None, None) == 0 and L.cpx_ids_to_classes(None, 5, None, 0, None, None) != 0


def test_threshold_cases_sit_on_both_sides_of_the_kernels_limits():
    from classpose_amd import ops
    """what the parametrised cases rely on: the named rings straddle the small / large limits in exactly one of the two"""
    def box_and_n(name):
        (ring,), (H, W) = rr.CASES[name]
        r0, c0, par, _ = rr.ring_masks_exact(ring, H, W)
        return par.size, len(ring)
    A, V = ops.RASTER_SMALL_MAX_AREA, ops.RASTER_SMALL_MAX_VERTICES
    assert box_and_n("area_4096") == (A, 6) and box_and_n("area_4160")[0] == A + 64 and box_and_n("area_4097_by_1") == (A + 1, 6)
    a, n = box_and_n("vertices_256")
    assert a < A and n == V
    a, n = box_and_n("vertices_257")
    assert a < A and n == V + 1
    for n in rr.VERTEX_COUNTS:
        assert box_and_n(f"star_small_box_{n}")[0] < A < box_and_n(f"star_large_box_{n}")[0]
    for w in rr.BOX_SIDES:
        for h in rr.BOX_SIDES:
            assert box_and_n(f"box_{w}x{h}")[0] == w * h


def test_rasterize_polygons_refuses_bad_arguments_before_any_launch():
    import torch
    from classpose_amd import ops
    xy, off, val, _ = rr.pack([rr.TRIANGLE, [(1, 1), (5, 1), (5, 5)]])
    ok = dict(xy=xy, ring_off=off, ring_value=val, shape=(16, 16))

    def bad(match, **kw):
        with pytest.raises(ValueError, match=match):
            ops.rasterize_polygons(**{**ok, **kw})
    bad("float64", xy=xy.astype(np.float32))
    bad("int64", ring_off=off.astype(np.int32))
    bad("int32", ring_value=val.astype(np.int64))
    bad("int32", ring_image=np.zeros(2, np.int64))
    bad(r"\(n_vertices, 2\)", xy=xy.ravel())
    bad("n_rings \\+ 1", ring_off=off[:-1])
    bad("non-decreasing", ring_off=np.array([0, 4, 3], np.int64))
    bad("non-decreasing", ring_off=np.array([0, 3, 7], np.int64))
    bad("non-decreasing", ring_off=np.array([-1, 3, 6], np.int64))
    bad("> 0", ring_value=np.array([1, 0], np.int32))
    bad("> 0", ring_value=np.array([-3, 2], np.int32))
    bad("ring_image", ring_image=np.array([0, 1], np.int32))
    bad("ring_image", ring_image=np.array([0, -1], np.int32), n_images=2)
    bad("one image index per ring", ring_image=np.array([0], np.int32))
    nan = xy.copy(); nan[2, 1] = np.nan
    bad("NaN", xy=nan)
    inf = xy.copy(); inf[0, 0] = -np.inf
    bad("NaN", xy=inf)
    bad("H, W", shape=(0, 16))
    bad("H, W", shape=(16, 32769))
    bad("H, W", n_images=0)
    bad("shape must be", shape=16)
    bad("out must be", out=torch.zeros((1, 16, 16), dtype=torch.int64))
    bad("out must be", out=torch.zeros((2, 16, 16), dtype=torch.int32))
    bad("cuda", out=torch.zeros((1, 16, 16), dtype=torch.int32))
    bad("cuda", device="cpu")
    with pytest.raises(ValueError, match="int32"):
        ops.ids_to_classes(torch.zeros((4, 4), dtype=torch.int64), np.zeros(3, np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        ops.ids_to_classes(torch.zeros((4, 4), dtype=torch.int32), np.zeros(3, np.int32))
    with pytest.raises(ValueError, match="cuda"):
        ops.ids_to_classes(torch.zeros((4, 4), dtype=torch.int32), np.zeros(3, np.uint8))


# ---- the command-line tools' argument errors ---------------------------------------------------------------------------------------
def _exits(module, argv, match):
    import importlib
    mod = importlib.import_module(f"classpose_amd.entrypoints.{module}")
    with pytest.raises(SystemExit) as e:
        mod.main(mod.build_parser().parse_args(argv))
    assert re.search(match, str(e.value)), e.value


def test_calculate_metrics_geojson_argument_errors(tmp_path, capsys):
    gt = _write(tmp_path, "gt.geojson", FEATURES)
    base = ["--gt_geojson", gt, "--pred_geojson", gt, "--class_names", "tumour", "stroma"]
    _exits("calculate_metrics_geojson", base, "--region .* or --roi_geojson")
    _exits("calculate_metrics_geojson", base + ["--region", "0", "0", "8", "8", "--roi_geojson", gt], "one of the two")
    _exits("calculate_metrics_geojson", base + ["--region", "0", "0", "0", "8"], "must be positive")
    _exits("calculate_metrics_geojson", base + ["--region", "0", "0", "8", "8", "--downsample", "0"], "--downsample")
    _exits("calculate_metrics_geojson", base + ["--region", "0", "0", "8", "8", "--match_iou", "-1"], "--match_iou")
    _exits("calculate_metrics_geojson", base + ["--region", "0", "0", "9000", "9000"], "smaller regions")
    _exits("calculate_metrics_geojson", base + ["--region", "0", "0", "64", "64", "--max_region_px", "4095"], "smaller regions")
    from classpose_amd.entrypoints import calculate_metrics_geojson as cmg
    with pytest.raises(ValueError, match="'stroma'"):
        cmg.main(cmg.build_parser().parse_args(["--gt_geojson", gt, "--pred_geojson", gt, "--class_names", "tumour", "--region", "0", "0", "8", "8"]))
    for argv in (["--pred_geojson", gt, "--class_names", "a"], ["--gt_geojson", gt, "--class_names", "a"], ["--gt_geojson", gt, "--pred_geojson", gt],
                 base + ["--region", "0", "0", "8"]):
        with pytest.raises(SystemExit):
            cmg.build_parser().parse_args(argv)
    capsys.readouterr()
    # the ROI file's polygons give whole-pixel bounding boxes
    roi = _write(tmp_path, "roi.geojson", [_feat("Polygon", [[[10.5, 20.25], [100, 20.25], [100, 90.5], [10.5, 90.5]]])])
    args = cmg.build_parser().parse_args(base + ["--roi_geojson", roi])
    assert cmg.regions_of(args) == [(10.0, 20.0, 91.0, 72.0)]
    # the existing tool keeps its required flags
    from classpose_amd.entrypoints import calculate_metrics as cm
    with pytest.raises(SystemExit):
        cm.build_parser().parse_args(["--gt_geojson", gt])
    capsys.readouterr()


def test_geojson_to_labels_argument_errors(tmp_path, capsys):
    from PIL import Image
    from classpose_amd.entrypoints import geojson_to_labels as g2l
    imgs, anns = tmp_path / "img", tmp_path / "ann"
    imgs.mkdir(); anns.mkdir()
    base = ["--images", str(imgs), "--annotations", str(anns), "--class_names", "tumour", "--out", str(tmp_path / "out")]
    _exits("geojson_to_labels", ["--images", str(tmp_path / "nowhere")] + base[2:], "not a directory")
    _exits("geojson_to_labels", base, "no image")
    Image.fromarray(np.zeros((8, 9, 3), np.uint8)).save(imgs / "a.png")
    _exits("geojson_to_labels", base, r"do not pair by file stem: \['a'\]")
    _write(anns, "a.geojson", FEATURES[:1])
    _write(anns, "b.geojson", FEATURES[:1])
    _exits("geojson_to_labels", base, r"do not pair by file stem: \['b'\]")
    _write(anns, "a.json", FEATURES[:1])
    _exits("geojson_to_labels", base, "two annotation files with the stem 'a'")
    for argv in (base[2:], base[:2] + base[4:], base[:4] + base[6:], base[:6]):
        with pytest.raises(SystemExit):
            g2l.build_parser().parse_args(argv)
    capsys.readouterr()
    assert not (tmp_path / "out").exists()
    a, b = np.zeros((4, 5, 2), np.int32), np.zeros((4, 6, 2), np.int32)
    assert g2l.stack_or_objects([a, a]).shape == (2, 4, 5, 2) and g2l.stack_or_objects([a, b]).dtype == object
