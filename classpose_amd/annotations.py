"""GeoJSON annotations -> (instance, class) maps on the device: the inverse of what ``predict_wsi`` writes.

The reference has this only as one data set's recipe (paper_experiments/scripts/organise-datasets.py:626-652): features in file
order, every ring of every feature painted with ``skimage.draw.polygon``, instance id = 1-based feature index, class from
``properties.classification.name``, later features over earlier ones.  Here ``load_features`` reads the file into flat host arrays
and ``rasterize`` paints any number of equally sized regions of it in one device call (``ops.rasterize_polygons`` ->
``cpx_rasterize_polygons``; the rule is stated in include/classpose_hip.h), then looks the classes up (``ops.ids_to_classes``).

Deliberately different from the recipe: ``Point`` features (the centroid file) are skipped and counted, they still take their
position in the numbering; rings of fewer than three vertices paint nothing (``draw.polygon`` paints a two-vertex ring's pixels).
Not built: line strings, anti-aliased coverage, splitting of oversize regions.
"""
from __future__ import annotations

import json
from typing import NamedTuple

import numpy as np


class Annotations(NamedTuple):
    """Host arrays of one file.  Ring k is ``xy[ring_off[k]:ring_off[k + 1]]`` (x, y in the file's coordinates) and belongs to
    feature ``ring_feature[k]`` (0-based position in the file; its instance id is that + 1); ``feature_class[f]`` is position + 1
    in ``class_names``, 0 = none (an ignored unknown name, or a skipped feature)."""
    xy: np.ndarray              # (n_vertices, 2) float64
    ring_off: np.ndarray        # (n_rings + 1,) int64
    ring_feature: np.ndarray    # (n_rings,) int32
    feature_class: np.ndarray   # (n_features,) uint8
    n_features: int
    n_points: int = 0           # Point features skipped


def _feature_list(data, path) -> list:
    if isinstance(data, list):
        return data
    if isinstance(data, dict) and isinstance(data.get("features"), list):
        return data["features"]
    if isinstance(data, dict) and "geometry" in data:
        return [data]
    raise ValueError(f"{path}: neither a FeatureCollection nor a list of features")


def _ring(coords, where: str) -> np.ndarray:
    try:
        ring = np.asarray(coords, np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{where}: a ring is not a list of coordinate pairs") from None
    if ring.ndim != 2 or ring.shape[1] < 2:
        if ring.size == 0:
            return np.zeros((0, 2), np.float64)
        raise ValueError(f"{where}: a ring is not a list of coordinate pairs")
    if not np.isfinite(ring[:, :2]).all():
        raise ValueError(f"{where}: a coordinate is not finite")
    return ring[:, :2]


def load_features(path, class_names, ignore_unknown: bool = False) -> Annotations:
    """Read a FeatureCollection, or the bare feature list QuPath also exports.  ``Polygon`` and ``MultiPolygon`` features give
    their rings (holes included: every ring paints); ``Point`` features are skipped and counted; any other geometry raises.  The
    class is ``properties.classification.name`` looked up in ``class_names`` (position + 1); a name that is not listed -- or a
    feature without one -- raises ``ValueError`` naming the feature, unless ``ignore_unknown``: then the feature keeps its
    instance and gets class 0."""
    with open(path, "r") as f:
        features = _feature_list(json.load(f), path)
    if len(class_names) > 255:
        raise ValueError("at most 255 class names: class maps are uint8")
    index = {str(n): i + 1 for i, n in enumerate(class_names)}
    rings, ring_feature = [], []
    feature_class = np.zeros(len(features), np.uint8)
    n_points = 0
    for fi, feat in enumerate(features):
        geom = (feat or {}).get("geometry") or {}
        kind, coords = geom.get("type"), geom.get("coordinates")
        where = f"{path}: feature {fi}" + (f" (id {feat['id']})" if isinstance(feat, dict) and "id" in feat else "")
        if kind == "Point":
            n_points += 1
            continue
        if kind == "Polygon":
            parts = [coords]
        elif kind == "MultiPolygon":
            parts = coords
        else:
            raise ValueError(f"{where}: geometry {kind!r} is not supported (Polygon, MultiPolygon; Point is skipped)")
        name = ((feat.get("properties") or {}).get("classification") or {}).get("name")
        if name in index:
            feature_class[fi] = index[name]
        elif not ignore_unknown:
            raise ValueError(f"{where}: class {name!r} is not one of {list(class_names)}")
        for part in parts or []:
            for ring in part or []:
                rings.append(_ring(ring, where))
                ring_feature.append(fi)
    off = np.zeros(len(rings) + 1, np.int64)
    if rings:
        off[1:] = np.cumsum([len(r) for r in rings])
    xy = np.ascontiguousarray(np.concatenate(rings), np.float64) if rings else np.zeros((0, 2), np.float64)
    return Annotations(xy, off, np.asarray(ring_feature, np.int32), feature_class, len(features), n_points)


def feature_bounds(ann: Annotations) -> np.ndarray:
    """(n_features, 4) float64 ``x_min, y_min, x_max, y_max`` over every ring of a feature; an empty box (min > max) for a
    feature without vertices."""
    b = np.empty((ann.n_features, 4), np.float64)
    b[:, :2], b[:, 2:] = np.inf, -np.inf
    per_vertex = np.repeat(ann.ring_feature, np.diff(ann.ring_off))
    if len(per_vertex):
        np.minimum.at(b[:, 0], per_vertex, ann.xy[:, 0]); np.minimum.at(b[:, 1], per_vertex, ann.xy[:, 1])
        np.maximum.at(b[:, 2], per_vertex, ann.xy[:, 0]); np.maximum.at(b[:, 3], per_vertex, ann.xy[:, 1])
    return b


def cull(ann: Annotations, region, bounds: np.ndarray | None = None, downsample: float = 1.0, coordinate_offset: float = 0.0) -> np.ndarray:
    """Indices of the features whose bounding box touches a pixel centre of ``region`` (x, y, w, h): in local coordinates the box
    meets ``[0, W - 1] x [0, H - 1]`` (W = ceil(w / downsample)), borders included (a centre on a ring is painted).  A superset
    of the features that paint."""
    x, y, w, h = region
    w, h = np.ceil(w / downsample), np.ceil(h / downsample)
    b = feature_bounds(ann) if bounds is None else bounds
    lo_x, hi_x = (b[:, 0] + coordinate_offset - x) / downsample, (b[:, 2] + coordinate_offset - x) / downsample
    lo_y, hi_y = (b[:, 1] + coordinate_offset - y) / downsample, (b[:, 3] + coordinate_offset - y) / downsample
    return np.flatnonzero((lo_x <= w - 1) & (hi_x >= 0) & (lo_y <= h - 1) & (hi_y >= 0))


def local_rings(ann: Annotations, regions, downsample: float = 1.0, coordinate_offset: float = 0.0):
    """The host side of ``rasterize``: per region the surviving features' rings in local coordinates
    ``((v + coordinate_offset) - origin) / downsample``, concatenated -> ``(xy, ring_off, ring_value, ring_image)``."""
    regions = np.asarray(regions, np.float64).reshape(-1, 4)
    bounds = feature_bounds(ann)
    n_per_ring = np.diff(ann.ring_off)
    xs, counts, values, images = [], [], [], []
    for i, (x, y, w, h) in enumerate(regions):
        keep = np.zeros(ann.n_features, bool)
        keep[cull(ann, (x, y, w, h), bounds, downsample, coordinate_offset)] = True
        rk = np.flatnonzero(keep[ann.ring_feature])
        if not len(rk):
            continue
        vsel = np.concatenate([np.arange(ann.ring_off[k], ann.ring_off[k + 1]) for k in rk])
        xs.append(((ann.xy[vsel] + coordinate_offset) - np.array([x, y])) / downsample)
        counts.append(n_per_ring[rk])
        values.append(ann.ring_feature[rk] + 1)
        images.append(np.full(len(rk), i, np.int32))
    if not xs:
        return np.zeros((0, 2), np.float64), np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32)
    counts = np.concatenate(counts)
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return (np.ascontiguousarray(np.concatenate(xs), np.float64), off, np.concatenate(values).astype(np.int32),
            np.concatenate(images).astype(np.int32))


def rasterize(ann: Annotations, regions, downsample: float = 1.0, coordinate_offset: float = 0.0, device="cuda"):
    """Paint regions ``(x, y, w, h)`` of one common size (in the file's coordinates; the maps are ``h / downsample`` by
    ``w / downsample`` pixels) -> ``(inst (n, H, W) int32, cls (n, H, W) uint8)`` on the device.  Features are culled per region by
    bounding box on the host and only the survivors are uploaded.  Ids are the 1-based feature index of the file, so a cell seen
    from two regions keeps one id.  The reference's PUMA recipe is ``coordinate_offset=-1``."""
    from . import ops
    regions = np.asarray(regions, np.float64).reshape(-1, 4)
    if len(regions) == 0:
        raise ValueError("rasterize: no region")
    if downsample <= 0 or not np.isfinite(downsample):
        raise ValueError(f"rasterize: downsample must be positive, not {downsample}")
    sizes = {(float(w), float(h)) for _, _, w, h in regions}
    if len(sizes) != 1:
        raise ValueError(f"rasterize: regions must share one size, got {sorted(sizes)}")
    w, h = sizes.pop()
    W, H = int(np.ceil(w / downsample)), int(np.ceil(h / downsample))
    if H < 1 or W < 1:
        raise ValueError(f"rasterize: empty regions of {w} x {h}")
    xy, off, value, image = local_rings(ann, regions, downsample, coordinate_offset)
    inst = ops.rasterize_polygons(xy, off, value, (H, W), ring_image=image, n_images=len(regions), device=device)
    class_of = np.concatenate([np.zeros(1, np.uint8), ann.feature_class])
    return inst, ops.ids_to_classes(inst, class_of)
