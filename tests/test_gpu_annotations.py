"""GPU: the two front ends of the device rasteriser.  ``calculate_metrics_geojson`` on a synthetic annotated / predicted pair must
write exactly the tables ``compute_multiclass_pq_metrics`` / ``compute_binary_pq_metrics`` give for the maps the exact CPU
rasteriser (tests/rasterize_reference.py) paints; ``geojson_to_labels`` must write a directory ``train_data`` loads, with the CPU
rasteriser's labels.  Coordinates are multiples of 1/16 and region origins are integers, where the kernel is exact."""
import json

import numpy as np
import pytest

import rasterize_reference as rr
from classpose_amd import annotations as an

pytestmark = pytest.mark.gpu

NAMES = ["tumour", "stroma", "immune"]


def _feature(ring, name):
    ring = np.asarray(ring, np.float64)
    closed = np.concatenate([ring, ring[:1]]).tolist()
    return {"type": "Feature", "id": "x", "geometry": {"type": "Polygon", "coordinates": [closed]},
            "properties": {"objectType": "detection", "classification": {"name": name, "color": [0, 0, 0]}}}


def _cell(rng, cx, cy):
    n = int(rng.integers(5, 12))
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    r = rng.uniform(3.0, 7.5, n)
    return rr.q16(np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1))


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    """ground truth: cells on a 16-pixel grid over 256 x 192; prediction: shifted, dropped, added and re-classed cells"""
    rng = np.random.default_rng(21)
    gt, pred = [], []
    k = 0
    for gy in range(12):
        for gx in range(16):
            cx, cy = 8 + 16 * gx + rng.uniform(-1, 1), 8 + 16 * gy + rng.uniform(-1, 1)
            ring, name = _cell(rng, cx, cy), NAMES[k % 3]
            gt.append(_feature(ring, name))
            if k % 7 != 3:                                                             # dropped
                shift = rr.q16(rng.uniform(-2.0, 2.0, 2)) if k % 2 else np.zeros(2)     # shifted
                pred.append(_feature(ring + shift, NAMES[(k + 1) % 3] if k % 5 == 0 else name))     # re-classed
            if k % 11 == 0:                                                            # added
                pred.append(_feature(_cell(rng, cx + 8, cy + 8), NAMES[k % 3]))
            k += 1
    pred.insert(5, {"type": "Feature", "geometry": {"type": "Point", "coordinates": [3.0, 4.0]}, "properties": {}})
    d = tmp_path_factory.mktemp("pair")
    (d / "gt.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": gt}))
    (d / "pred.geojson").write_text(json.dumps(pred))
    return d


REGIONS = [(0, 0, 128, 128), (100, 30, 96, 144), (120, 64, 128, 128)]                  # two sizes: two device batches


def _cpu_masks(path, regions):
    """[(H, W, 2) int32] per region: the exact CPU rasteriser on the host side of annotations.rasterize"""
    a = an.load_features(str(path), NAMES)
    class_of = np.concatenate([[0], a.feature_class]).astype(np.int32)
    out = []
    for x, y, w, h in regions:
        xy, off, val, _ = an.local_rings(a, [(x, y, w, h)])
        inst = rr.rasterize(xy, off, val, (h, w))[0]
        out.append(np.stack([inst, class_of[inst]], -1))
    return out


def test_annotations_rasterize_equals_the_cpu_version(cuda, pair):
    a = an.load_features(str(pair / "pred.geojson"), NAMES)
    assert a.n_points == 1
    same = [r for r in REGIONS if r[2:] == (128, 128)]
    inst, cls = an.rasterize(a, same, device=cuda)
    want = _cpu_masks(pair / "pred.geojson", same)
    assert inst.shape == (2, 128, 128) and str(inst.dtype) == "torch.int32" and str(cls.dtype) == "torch.uint8"
    for k, w in enumerate(want):
        assert np.array_equal(inst[k].cpu().numpy(), w[..., 0]) and np.array_equal(cls[k].cpu().numpy(), w[..., 1])
    # a cell seen from two regions keeps one id
    assert len(set(np.unique(want[0][..., 0])) & set(np.unique(want[1][..., 0])) - {0}) >= 3
    with pytest.raises(ValueError, match="one size"):
        an.rasterize(a, REGIONS, device=cuda)
    # downsample 2: local coordinates are multiples of 1/32, outside the integer version's grid: the float64 version states the
    # same arithmetic for any coordinate
    inst2, _ = an.rasterize(a, [(0, 0, 256, 192)], downsample=2.0, device=cuda)
    xy, off, val, _ = an.local_rings(a, [(0, 0, 256, 192)], 2.0)
    assert np.array_equal(inst2[0].cpu().numpy(), rr.rasterize(xy, off, val, (96, 128), masks=rr.ring_masks_float)[0])


def test_calculate_metrics_geojson_writes_the_tables_of_the_cpu_maps(cuda, pair, tmp_path, capsys):
    from classpose_amd.entrypoints import calculate_metrics_geojson as cmg
    from classpose_amd.metrics.pq import compute_binary_pq_metrics, compute_multiclass_pq_metrics
    gt_masks, pred_masks = _cpu_masks(pair / "gt.geojson", REGIONS), _cpu_masks(pair / "pred.geojson", REGIONS)
    argv = ["--gt_geojson", str(pair / "gt.geojson"), "--pred_geojson", str(pair / "pred.geojson"), "--class_names", *NAMES]
    for r in REGIONS:
        argv += ["--region", *(str(v) for v in r)]
    # multi-class
    cmg.main(cmg.build_parser().parse_args(argv + ["--output", str(tmp_path / "got.csv")]))
    want_global, want_per_image = compute_multiclass_pq_metrics(gt_masks, pred_masks, match_iou=0.5, nr_classes=len(NAMES))
    want_global.to_csv(tmp_path / "want.csv", index=False)
    want_per_image.to_csv(tmp_path / "want_per_image.csv", index=False)
    assert (tmp_path / "got.csv").read_text() == (tmp_path / "want.csv").read_text()
    assert (tmp_path / "got_per_image.csv").read_text() == (tmp_path / "want_per_image.csv").read_text()
    printed = capsys.readouterr().out
    assert want_global.to_string(index=False) in printed
    # the pair is not trivial: hits, misses and false alarms in every class
    body = want_global[want_global["class_id"] != "avg"]
    assert (body["tp"] > 0).all() and (body["fp"] > 0).all() and (body["fn"] > 0).all() and len(want_per_image) == len(REGIONS)
    # binary, without border instances
    cmg.main(cmg.build_parser().parse_args(argv + ["--binary", "--no_border_instances", "--output", str(tmp_path / "bin.csv")]))
    want_bin = compute_binary_pq_metrics([m[..., 0] for m in gt_masks], [m[..., 0] for m in pred_masks], match_iou=0.5,
                                         no_border_instances=True)
    want_bin.to_csv(tmp_path / "want_bin.csv", index=False)
    assert (tmp_path / "bin.csv").read_text() == (tmp_path / "want_bin.csv").read_text()
    assert (want_bin["tp"] > 0).all() and want_bin["fp"].sum() > 0 and want_bin["fn"].sum() > 0
    capsys.readouterr()
    # regions from an ROI file: the bounding box of its polygon
    roi = tmp_path / "roi.geojson"
    roi.write_text(json.dumps([{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [[[0, 0], [127, 0], [127, 127], [0, 127], [0, 0]]]},
                                "properties": {}}]))
    cmg.main(cmg.build_parser().parse_args(argv[:argv.index("--region")] + ["--roi_geojson", str(roi), "--output", str(tmp_path / "roi.csv")]))
    compute_multiclass_pq_metrics(gt_masks[:1], pred_masks[:1], nr_classes=len(NAMES))[0].to_csv(tmp_path / "want_roi.csv", index=False)
    assert (tmp_path / "roi.csv").read_text() == (tmp_path / "want_roi.csv").read_text()
    capsys.readouterr()


def test_geojson_to_labels_writes_what_train_data_loads(cuda, tmp_path):
    from PIL import Image
    from classpose_amd import train_data
    from classpose_amd.entrypoints import geojson_to_labels as g2l
    rng = np.random.default_rng(4)
    imgs, anns = tmp_path / "images", tmp_path / "annotations"
    imgs.mkdir(); anns.mkdir()
    sizes = {"a": (40, 48), "b": (33, 57), "c": (40, 48)}
    pixels, rings_of = {}, {}
    for stem, (H, W) in sizes.items():
        pixels[stem] = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)
        Image.fromarray(pixels[stem]).save(imgs / f"{stem}.png")
        feats, rings = [], []
        for k in range(9):
            ring = _cell(rng, rng.uniform(0, W + 2), rng.uniform(0, H + 2))        # some reach over the border
            rings.append((ring, 1 + k % 3))
            feats.append(_feature(ring, NAMES[k % 3]))
        rings_of[stem] = rings
        (anns / f"{stem}.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": feats}))
    out = tmp_path / "out"
    g2l.main(g2l.build_parser().parse_args(["--images", str(imgs), "--annotations", str(anns), "--class_names", *NAMES, "--out", str(out),
                                            "--coordinate_offset", "-1"]))
    images = np.load(out / "images.npy", allow_pickle=True)
    labels = np.load(out / "labels.npy", allow_pickle=True)
    assert images.dtype == object and labels.dtype == object and len(images) == len(labels) == 3
    data = train_data.load_dataset(str(out))
    assert len(data) == 3 and data.n_classes == 4
    for i, stem in enumerate(sorted(sizes)):
        H, W = sizes[stem]
        xy, off, val, _ = rr.pack([r - 1.0 for r, _ in rings_of[stem]])
        inst = rr.rasterize(xy, off, val, (H, W))[0]
        cls = np.concatenate([[0], [c for _, c in rings_of[stem]]])[inst]
        assert np.array_equal(images[i], pixels[stem])
        assert labels[i].shape == (H, W, 2) and np.issubdtype(labels[i].dtype, np.integer)
        assert np.array_equal(labels[i][..., 0], inst) and np.array_equal(labels[i][..., 1], cls)
        assert inst.max() > 0
        assert np.array_equal(data.images[i], pixels[stem]) and np.array_equal(data.instances[i], inst)
        assert np.array_equal(data.classes[i], cls)            # every instance has a class, so nothing is masked to -100
