"""numpy restatement of the reference's dataset statistics, for the label-statistics tests and the fixture's mint script.

``get_class_counts`` / ``get_instance_counts`` are restated per image from train_utils.py:387-436 (the fixture pins them on the
reference's own functions); ``diameters`` restates the three lines of cellpose.utils.diameters (4.0.8), whose wheel is absent:

    uniq, counts = fastremap.unique(masks.astype("int32"), return_counts=True)
    counts = counts[1:]
    md = np.median(counts ** 0.5);  md = 0 if isnan(md);  md /= (np.pi ** 0.5) / 2
"""
from __future__ import annotations

import numpy as np


def diameters(masks: np.ndarray):
    """(median diameter, sqrt(areas)) of cellpose.utils.diameters; ``np.unique`` sorts like ``fastremap.unique``."""
    _uniq, counts = np.unique(masks.astype("int32"), return_counts=True)
    counts = counts[1:]
    if counts.size == 0:
        return 0.0, counts ** 0.5
    md = np.median(counts ** 0.5)
    md /= (np.pi ** 0.5) / 2
    return float(md), counts ** 0.5


def numpy_label_stats(inst: np.ndarray, cls: np.ndarray, ncls: int) -> dict:
    """Per-image outputs of ``cpx_label_stats`` for maps (n, H, W), computed the reference's way, plus the float64 diameters."""
    n = len(inst)
    out = dict(class_px=np.zeros((n, ncls), np.int64), inst_per_class=np.zeros((n, ncls), np.int32), n_masks=np.zeros(n, np.int32),
               mid_area=np.zeros((n, 2), np.int32), diameters=np.zeros(n, np.float64))
    for i in range(n):
        lab = cls[i].ravel().astype(np.int64)
        out["class_px"][i] = np.bincount(lab[lab >= 0], minlength=ncls)[:ncls]
        for j in range(ncls):
            out["inst_per_class"][i, j] = np.unique(inst[i][cls[i] == j]).size
        counts = np.sort(np.unique(inst[i], return_counts=True)[1][1:])
        m = counts.size
        out["n_masks"][i] = m
        if m:
            out["mid_area"][i] = counts[(m - 1) // 2], counts[m // 2]
        out["diameters"][i] = diameters(inst[i])[0]
    return out


def random_maps(rng: np.random.Generator, n: int, H: int, W: int, ncls: int, n_cells: int, max_id: int = 2_000_000_000):
    """(inst int32, cls int16) (n, H, W): about ``n_cells`` rectangular cells with random non-contiguous ids below ``max_id`` on a
    background that carries class 0, one class per cell with a few two-class cells, and -100 / -1 regions."""
    inst = np.zeros((n, H, W), np.int32)
    cls = np.zeros((n, H, W), np.int16)
    side = max(2, int((H * W / max(n_cells, 1)) ** 0.5))
    for i in range(n):
        ids = np.unique(rng.integers(1, max_id + 1, size=2 * n_cells + 8))
        ids = rng.permutation(ids)[:n_cells]
        for k in range(n_cells):
            y0, x0 = int(rng.integers(0, H)), int(rng.integers(0, W))
            h, w = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1))
            inst[i, y0:y0 + h, x0:x0 + w] = ids[k]
            cls[i, y0:y0 + h, x0:x0 + w] = rng.integers(0, ncls)
            if k % 17 == 0:                                  # the lower half of some cells takes another class
                cls[i, y0 + h // 2:y0 + h, x0:x0 + w] = rng.integers(0, ncls)
        y0, x0 = int(rng.integers(0, H - 8)), int(rng.integers(0, W - 8))
        cls[i, y0:y0 + 7, x0:x0 + 5] = -100
        cls[i, rng.integers(0, H), :] = -1
    return inst, cls
