"""``compute_multiclass_pq_metrics`` / ``compute_binary_pq_metrics`` with the reference's arguments, defaults and tables
(classpose/metrics/pq.py:95-290), computed from ONE device pass per batch of images (``ops.pq_stats`` -> ``cpx_pq_stats``)
instead of the reference's loops over classes, true instances and overlapping predictions.

Differences from the reference, on purpose (DESIGN, "Panoptic-quality metrics"):
  * the input arrays are NOT modified (the reference zeroes filtered / border instances in the arrays it is given);
  * ids must be non-negative and fit int32, classes must fit uint8, else ``ValueError`` (the reference renumbers any int64);
  * ``n_workers`` is accepted and ignored.
Everything from the per-(image, class) statistics to the DataFrames is host code without a GPU (``multiclass_tables``,
``binary_table``, ``assignment_stats``).
"""
from __future__ import annotations

import numpy as np
import pandas as pd

from .utils import check_and_coherce_if_necessary

GLOBAL_COLUMNS = ["class_id", "pq", "dq", "sq", "tp", "fp", "fn", "precision", "recall", "f1", "iou_sum"]
BINARY_COLUMNS = ["image_id", "pq", "dq", "sq", "tp", "fp", "fn", "precision", "recall", "f1", "iou_sum", "avg_iou"]
EPS = 1.0e-6


# ---- host: statistics -> tables ------------------------------------------------------------------------------------
def multiclass_tables(tp, fp, fn, iou_sum) -> tuple[pd.DataFrame, pd.DataFrame]:
    """(n_images, nr_classes) statistics -> (global_df, per_image_df) of pq.py:185-290: per-class sums over the images in image
    order, float64 like the reference's ``np.zeros`` accumulators (0 / 0 gives NaN there too), and the ``avg`` row."""
    tp, fp, fn = (np.asarray(a).astype(np.int64) for a in (tp, fp, fn))
    iou_sum = np.asarray(iou_sum, np.float64)
    n_img, nr = tp.shape
    per_image = []
    for i in range(n_img):
        row = {"image_id": i}
        for c in range(nr):
            t = int(tp[i, c])
            row[f"class_{c + 1}_tp"] = t
            row[f"class_{c + 1}_fp"] = int(fp[i, c])
            row[f"class_{c + 1}_fn"] = int(fn[i, c])
            row[f"class_{c + 1}_avg_iou"] = iou_sum[i, c] / t if t > 0 else 0.0
        per_image.append(row)
    rows = []
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in range(nr):
            t = f = m = s = np.float64(0.0)
            for i in range(n_img):                       # the reference adds image by image
                t, f, m, s = t + tp[i, c], f + fp[i, c], m + fn[i, c], s + iou_sum[i, c]
            dq = t / ((t + 0.5 * f + 0.5 * m) + EPS)
            sq = s / (t + EPS)
            rows.append({"class_id": c + 1, "pq": dq * sq, "dq": dq, "sq": sq, "tp": t, "fp": f, "fn": m,
                         "precision": t / (t + f), "recall": t / (t + m), "f1": (2 * t) / (2 * t + f + m), "iou_sum": s})
        avg = {"class_id": "avg"}
        for k in GLOBAL_COLUMNS[1:]:
            col = [r[k] for r in rows]
            avg[k] = np.sum(col) if k in ("tp", "fp", "fn", "iou_sum") else np.mean(col)
    rows.append(avg)
    return pd.DataFrame(rows), pd.DataFrame(per_image)


def binary_table(tp, fp, fn, iou_sum) -> pd.DataFrame:
    """(n_images,) statistics -> the DataFrame of pq.py:116-156.  Counts are Python ints there, so an image without any
    instance raises ``ZeroDivisionError`` at its precision, as the reference does."""
    rows = []
    for i in range(len(tp)):
        t, f, m = int(tp[i]), int(fp[i]), int(fn[i])
        s = np.float64(iou_sum[i])
        dq = t / ((t + 0.5 * f + 0.5 * m) + EPS)
        sq = s / (t + EPS)
        rows.append({"image_id": i, "pq": dq * sq, "dq": dq, "sq": sq, "tp": t, "fp": f, "fn": m,
                     "precision": t / (t + f), "recall": t / (t + m), "f1": (2 * t) / (2 * t + f + m),
                     "iou_sum": s, "avg_iou": s / t if t > 0 else 0.0})
    return pd.DataFrame(rows)


def assignment_stats(pairs, insts, nobg, n_images: int, nr_classes: int):
    """The ``match_iou == 0`` branch of get_pq (stats_utils.py:144-158) from the device's lists: per (image, class) the dense
    IoU matrix laid out as the reference's -- rows / columns in order of first raster appearance, plus the trailing all-zero row /
    column a background pixel adds to ``np.unique`` -- goes through the same ``scipy.optimize.linear_sum_assignment`` call
    (which of several optimal assignments it returns depends on that layout); matched pairs with iou > 0 are the true positives."""
    from scipy.optimize import linear_sum_assignment
    tp = np.zeros((n_images, nr_classes), np.int32)
    fp, fn = np.zeros_like(tp), np.zeros_like(tp)
    iou_sum = np.zeros((n_images, nr_classes), np.float64)
    pairs, insts = np.asarray(pairs).reshape(-1, 8), np.asarray(insts).reshape(-1, 6)
    ikey = insts[:, 0].astype(np.int64) * 256 + insts[:, 2]
    pkey = pairs[:, 0].astype(np.int64) * 256 + pairs[:, 1]
    for key in np.unique(ikey):
        i, c = int(key // 256), int(key % 256)
        ins = insts[ikey == key]
        firsts = [np.sort(ins[ins[:, 1] == s][:, 3]) for s in (0, 1)]
        bg = [int(nobg[i, s]) != c for s in (0, 1)]
        m = np.zeros((len(firsts[0]) + bg[0], len(firsts[1]) + bg[1]), np.float64)
        pr = pairs[pkey == key]
        if len(pr) and m.size:
            r, col = np.searchsorted(firsts[0], pr[:, 2]), np.searchsorted(firsts[1], pr[:, 3])
            inter = pr[:, 4].astype(np.int64)
            m[r, col] = inter / (pr[:, 5].astype(np.int64) + pr[:, 6].astype(np.int64) - inter)
        if m.size:
            rows, cols = linear_sum_assignment(-m)
            got = m[rows, cols]
            keep = got > 0.0
            rows, cols, got = rows[keep], cols[keep], got[keep]
        else:
            rows = cols = np.zeros(0, np.int64)
            got = np.zeros(0, np.float64)
        # the id lists minus their FIRST entry: the background, or without one the first-appearing instance
        listed = [np.arange(0 if bg[s] else 1, len(firsts[s])) for s in (0, 1)]
        tp[i, c - 1] = len(rows)
        fn[i, c - 1] = len(np.setdiff1d(listed[0], rows))
        fp[i, c - 1] = len(np.setdiff1d(listed[1], cols))
        iou_sum[i, c - 1] = got.sum()
    return tp, fp, fn, iou_sum


# ---- host -> device ------------------------------------------------------------------------------------------------
def _channel(a, what: str, hi: int, dtype) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype.kind not in "iub":
        r = np.rint(a)
        if not np.array_equal(r, a):
            raise ValueError(f"{what} must be integers")
        a = r.astype(np.int64)
    if a.size and (a.min() < 0 or a.max() > hi):
        raise ValueError(f"{what} must lie in 0..{hi} (found {a.min()}..{a.max()})")
    return np.ascontiguousarray(a, dtype=dtype)


def device_stats(gt_masks, pred_masks, nr_classes: int | None, match_iou: float, no_border_instances: bool, device=None):
    """Per-image statistics (n_images, nr_classes) of lists / arrays of masks; ``nr_classes is None`` = binary (H, W) masks.
    Images are grouped by shape and every group goes to the device as one batch."""
    import torch
    from .. import ops
    if match_iou < 0.0:
        raise AssertionError("Cant' be negative")
    if len(gt_masks) != len(pred_masks):
        raise ValueError(f"{len(gt_masks)} ground truth masks but {len(pred_masks)} predicted masks")
    binary = nr_classes is None
    nr = 1 if binary else int(nr_classes)
    n = len(gt_masks)
    out = [np.zeros((n, nr), np.int32) for _ in range(3)] + [np.zeros((n, nr), np.float64)]
    if nr == 0 or n == 0:
        return tuple(out)
    dev = torch.device(device if device is not None else "cuda")
    groups: dict = {}
    for i in range(n):
        g, p = np.asarray(gt_masks[i]), np.asarray(pred_masks[i])
        want = 2 if binary else 3
        if g.ndim != want or p.ndim != want or g.shape[:2] != p.shape[:2] or (not binary and (g.shape[2] < 2 or p.shape[2] < 2)):
            raise ValueError(f"image {i}: mask shapes {g.shape} / {p.shape} do not fit")
        groups.setdefault(g.shape[:2], []).append(i)
    for (H, W), idx in groups.items():
        if H * W == 0:
            continue
        sides = []
        for masks in (gt_masks, pred_masks):
            ids = np.stack([_channel(np.asarray(masks[i])[..., 0] if not binary else masks[i], "instance ids", 2 ** 31 - 1, np.int32) for i in idx])
            cls = None if binary else np.stack([_channel(np.asarray(masks[i])[..., 1], "classes", 255, np.uint8) for i in idx])
            sides.append((torch.from_numpy(ids).to(dev), None if cls is None else torch.from_numpy(cls).to(dev)))
        (ti, tc), (pi, pc) = sides
        res = ops.pq_stats(ti, pi, tc, pc, nr_classes=nr, match_iou=match_iou, no_border_instances=no_border_instances,
                           return_lists=match_iou == 0.0)
        if match_iou == 0.0:
            stats = assignment_stats(res["pairs"], res["insts"], res["nobg"], len(idx), nr)
        else:
            stats = (res["tp"], res["fp"], res["fn"], res["iou_sum"])
        for o, s in zip(out, stats):
            o[idx] = s
    return tuple(out)


def compute_binary_pq_metrics(gt_masks, pred_masks, match_iou: float = 0.5, no_border_instances: bool = False) -> pd.DataFrame:
    """Binary PQ of (H, W) instance masks, one row per image: ``image_id, pq, dq, sq, tp, fp, fn, precision, recall, f1,
    iou_sum, avg_iou``.  An image without instances raises ``ZeroDivisionError`` like the reference.  The inputs are not
    modified (the reference removes border instances in place)."""
    gt_masks = check_and_coherce_if_necessary(gt_masks, 2)
    pred_masks = check_and_coherce_if_necessary(pred_masks, 2)
    tp, fp, fn, iou_sum = device_stats(gt_masks, pred_masks, None, match_iou, no_border_instances)
    return binary_table(tp[:, 0], fp[:, 0], fn[:, 0], iou_sum[:, 0])


def compute_multiclass_pq_metrics(gt_masks, pred_masks, match_iou: float = 0.5, nr_classes: int = 6, n_workers: int = 0,
                                  no_border_instances: bool = False) -> tuple[pd.DataFrame, pd.DataFrame]:
    """Multi-class PQ of (H, W, 2) masks (instance ids, classes): ``(global_df, per_image_df)`` with one row per class plus
    ``avg``, and one row per image.  Unlabelled true cells and the predictions matching them are filtered first, then border
    instances if asked.  ``n_workers`` is ignored: a batch is one device pass.  The inputs are not modified (the reference
    zeroes the filtered and border instances in the arrays it is given)."""
    del n_workers
    gt_masks = check_and_coherce_if_necessary(gt_masks, 3)
    pred_masks = check_and_coherce_if_necessary(pred_masks, 3)
    if not 0 <= int(nr_classes) <= 255:
        raise ValueError(f"nr_classes must be in 0..255, not {nr_classes}")
    return multiclass_tables(*device_stats(gt_masks, pred_masks, int(nr_classes), match_iou, no_border_instances))
