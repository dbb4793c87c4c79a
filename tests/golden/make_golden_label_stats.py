"""Mint the label-statistics fixture from the REFERENCE's own functions (run in the build container only).

    python tests/golden/make_golden_label_stats.py      # rewrites tests/golden/reference_label_stats.npz / .json

``classpose.train_utils`` is imported under the stub finder of make_golden.py.  Called on the CPU: ``get_class_counts``,
``get_instance_counts``, ``get_class_weights`` and ``compute_oversampling_probabilities`` (powers 1 and 0.5).
``cellpose.utils.diameters`` is not installed: its three lines are restated in tests/label_stats_reference.py, and the JSON marks
the diameters RESTATED.  The fixture holds data only.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ.setdefault("TQDM_DISABLE", "1")

NCLS = 7
ABSENT = 5            # no pixel of the whole set carries this class: its weight is 0


def paint(H, W, cells, bg_class=0):
    """cells: (y0, x0, h, w, id, class) rectangles painted in order onto a background of id 0 / ``bg_class``."""
    inst = np.zeros((H, W), np.int32)
    cls = np.full((H, W), bg_class, np.int16)
    for y0, x0, h, w, i, c in cells:
        inst[y0:y0 + h, x0:x0 + w] = i
        cls[y0:y0 + h, x0:x0 + w] = c
    return inst, cls


def grid_cells(rng, H, W, pitch, ids, sizes=None, classes=(1, 2, 3, 4, 6)):
    """One cell per grid square of ``pitch``, ids taken in order from ``ids``; sizes (h, w) random below the pitch unless given."""
    cells, k = [], 0
    for gy in range(H // pitch):
        for gx in range(W // pitch):
            if k >= len(ids):
                return cells
            h, w = sizes[k] if sizes is not None else (int(rng.integers(2, pitch)), int(rng.integers(2, pitch)))
            cells.append((gy * pitch, gx * pitch, h, w, int(ids[k]), int(classes[k % len(classes)])))
            k += 1
    return cells


def make_cases(rng):
    cases = []
    # plain: 25 cells on a background, a -100 band and box; m odd
    inst, cls = paint(64, 64, grid_cells(rng, 64, 64, 12, np.arange(1, 26)))
    cls[50:55, :] = -100
    cls[5:16, 20:29] = -100
    cases.append(("plain", inst, cls, dict(m_parity=1)))
    # empty: no instance at all
    inst, cls = paint(32, 32, [])
    cls[10:20, 4:9] = -100
    cases.append(("empty", inst, cls, dict(m=0)))
    # nobg: every pixel belongs to a cell; the SMALLEST id (7, 96 px) leaves the areas, not the background
    cells = [(0, 0, 32, 32, 40, 1), (0, 0, 12, 8, 7, 2), (0, 8, 16, 24, 9, 3), (16, 8, 16, 10, 23, 4), (12, 0, 20, 8, 11, 6)]
    inst, cls = paint(32, 32, cells)
    cases.append(("nobg", inst, cls, dict(no_background=True)))
    # bigids: non-contiguous ids up to 2 000 000 000
    ids = np.sort(rng.choice(1_999_999_000, 15, replace=False) + 1000)
    ids[-1] = 2_000_000_000
    inst, cls = paint(48, 48, grid_cells(rng, 48, 48, 12, ids))
    cls[:, 44:] = -100
    cases.append(("bigids", inst, cls, dict(max_id=2_000_000_000)))
    # twoclass: id 5 carries classes 2 and 4; background pixels (id 0) under class 3; a cell half under -100
    inst, cls = paint(32, 32, [(2, 2, 10, 10, 5, 2), (16, 4, 8, 6, 8, 1), (4, 18, 9, 9, 12, 6), (20, 20, 6, 6, 13, 1)])
    cls[7:12, 2:12] = 4
    cls[28:32, 0:16] = 3
    cls[20:23, 20:26] = -100
    cases.append(("twoclass", inst, cls, dict(two_class_id=5, bg_class=3)))
    # single: background + one cell, m == 1
    inst, cls = paint(32, 32, [(9, 11, 7, 5, 3, 6)])
    cases.append(("single", inst, cls, dict(m=1)))
    # ties: even m, and the areas around the median are tied (ten cells of 16 px between smaller and larger ones)
    sizes = [(2, 2)] * 3 + [(4, 4)] * 10 + [(6, 6)] * 3
    inst, cls = paint(64, 64, grid_cells(rng, 64, 64, 16, np.arange(101, 117) * 3, sizes))
    cases.append(("ties", inst, cls, dict(m_parity=0, tied=True)))
    # even: even m with two DIFFERENT middle areas, and pixels of another negative class (-1)
    sizes = [(2, 3), (3, 3), (3, 4), (4, 4), (4, 5), (5, 5), (5, 6), (6, 6)]
    inst, cls = paint(48, 48, grid_cells(rng, 48, 48, 12, np.array([900, 17, 350, 4, 88, 1200, 61, 5]), sizes))
    cls[40:, :] = -1
    cases.append(("even", inst, cls, dict(m_parity=0, tied=False)))
    return cases


def main():
    import make_golden
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REF)
    from classpose import train_utils as rtu
    import label_stats_reference as lsr

    rng = np.random.default_rng(20261018)
    cases = make_cases(rng)
    Y = [np.stack([inst.astype(np.int64), cls.astype(np.int64)]) for _n, inst, cls, _p in cases]
    class_counts = rtu.get_class_counts(Y, NCLS)
    instance_counts = rtu.get_instance_counts(Y, n_classes=NCLS)
    weights = rtu.get_class_weights(class_counts)
    arrays = dict(class_counts=np.asarray(class_counts, np.int64), instance_counts=np.asarray(instance_counts, np.float64),
                  class_weights=np.asarray(weights, np.float64),
                  probs_power_1=rtu.compute_oversampling_probabilities(class_counts, instance_counts, power=1),
                  probs_power_0p5=rtu.compute_oversampling_probabilities(class_counts, instance_counts, power=0.5))
    meta = {"n_classes": NCLS, "absent_class": ABSENT, "cases": [],
            "diameters": "RESTATED: cellpose is not installed; n_masks, mid_area and diameters ran the three lines of "
                         "cellpose.utils.diameters 4.0.8 (unique with counts, counts[1:], median of the square roots over "
                         "sqrt(pi) / 2) as restated in tests/label_stats_reference.py, not the wheel."}
    n_masks, mid, diam, px = [], [], [], []
    for k, (name, inst, cls, props) in enumerate(cases):
        r = lsr.numpy_label_stats(inst[None], cls[None], NCLS)
        assert np.array_equal(r["inst_per_class"][0], instance_counts[k]), name
        m = int(r["n_masks"][0])
        n_masks.append(m); mid.append(r["mid_area"][0]); diam.append(r["diameters"][0]); px.append(r["class_px"][0])
        if "m" in props:
            assert m == props["m"], (name, m)
        if "m_parity" in props:
            assert m % 2 == props["m_parity"] and m > 1, (name, m)
        if "tied" in props:
            assert (mid[-1][0] == mid[-1][1]) == props["tied"], (name, mid[-1])
        if props.get("no_background"):
            assert inst.min() > 0
        arrays[f"inst_{k}"], arrays[f"cls_{k}"] = inst, cls
        meta["cases"].append(dict(name=name, H=int(inst.shape[0]), W=int(inst.shape[1]), n_masks=m, **props))
        print(name, inst.shape, "m", m, "mid", mid[-1], "diam", diam[-1])
    assert np.array_equal(np.sum(px, 0), class_counts)
    assert class_counts[ABSENT] == 0 and weights[ABSENT] == 0 and (np.delete(class_counts, ABSENT) > 0).all()
    assert any((c[2] < 0).any() and (c[2] == -100).any() for c in cases)
    arrays["class_px"] = np.stack(px).astype(np.int64)
    arrays["n_masks"], arrays["mid_area"], arrays["diameters"] = np.array(n_masks, np.int32), np.stack(mid).astype(np.int32), np.array(diam)
    np.savez_compressed(os.path.join(HERE, "reference_label_stats.npz"), **arrays)
    with open(os.path.join(HERE, "reference_label_stats.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("class counts", class_counts.tolist(), "weights", weights.tolist())
    print("probs", arrays["probs_power_1"].tolist())
    print("wrote reference_label_stats.npz", os.path.getsize(os.path.join(HERE, "reference_label_stats.npz")), "bytes")


if __name__ == "__main__":
    main()
