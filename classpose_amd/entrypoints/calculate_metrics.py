"""``python -m classpose_amd.entrypoints.calculate_metrics``: the reference's ``classpose-calculate-metrics``
(classpose/entrypoints/calculate_metrics.py) on the device statistics of ``classpose_amd.metrics``.

Same flags, the same ``nr_classes`` rule (the largest true class BEFORE the label map), the same label-map semantics, printed
tables and ``<output>`` + ``<base>_per_image.<ext>`` files.  One difference, on purpose: ``--ignore_classes`` is applied per
image, so it also works on a directory of masks (the reference indexes the list of arrays there and fails).
"""
from __future__ import annotations

import argparse
from pathlib import Path

import numpy as np

from ..log import get_logger
from ..metrics.pq import compute_binary_pq_metrics, compute_multiclass_pq_metrics
from ..metrics.utils import load_masks

logger = get_logger(__name__)


def parse_label_map(items: list[str]) -> tuple[dict[int, int], np.ndarray]:
    """``["k=v", ...]`` -> ({0: 0, k: v, ...}, the values in order of first appearance, 0 first)."""
    mapping = {0: 0}
    values = [0]
    for item in items:
        k, v = item.split("=")
        mapping[int(k)] = int(v)
        if int(v) not in values:
            values.append(int(v))
    return mapping, np.array(values)


def apply_label_map(gt_masks, pred_masks, items: list[str]):
    """Predicted classes go through the map; true classes that are not one of the map's VALUES become 0 (they are expected to
    be in the target numbering already).  Returns new containers; the loaded arrays are edited like the reference edits them."""
    mapping, values = parse_label_map(items)
    logger.info(f"Label map: {mapping}")
    lut = np.full(max(mapping) + 1, -1, np.int64)
    for k, v in mapping.items():
        lut[k] = v
    for i in range(len(pred_masks)):
        m = np.asarray(pred_masks[i]).astype(int)
        cls = m[..., 1]
        if cls.size and (cls.min() < 0 or cls.max() >= len(lut) or (lut[cls] < 0).any()):
            raise ValueError(f"predicted mask {i} has a class without an entry in --label_map")
        m[..., 1] = lut[cls]
        pred_masks[i] = m
    for i in range(len(gt_masks)):
        cls = gt_masks[i][..., 1]
        gt_masks[i][..., 1] = np.where(np.isin(cls, values), cls, 0)
    return gt_masks, pred_masks


def main(args) -> None:
    logger.info(f"Loading ground truth masks from {args.gt_path}")
    gt_masks = load_masks(args.gt_path)
    logger.info(f"Loading predicted masks from {args.pred_path}")
    pred_masks = load_masks(args.pred_path)
    nr_classes = 0 if args.binary else int(np.max([m[..., 1].max() for m in gt_masks]))
    if args.label_map:
        logger.info(f"Applying label map: {args.label_map}")
        gt_masks, pred_masks = apply_label_map(gt_masks, pred_masks, args.label_map)
    if args.ignore_classes:
        for masks in (gt_masks, pred_masks):
            for i in range(len(masks)):
                cls = masks[i][..., 1]
                cls[np.isin(cls, args.ignore_classes)] = 0
    if isinstance(gt_masks, list) and isinstance(pred_masks, list):
        if len(gt_masks) != len(pred_masks):
            raise ValueError(f"Number of ground truth masks ({len(gt_masks)}) doesn't match predicted masks ({len(pred_masks)})")
    elif gt_masks.shape != pred_masks.shape:
        raise ValueError(f"Ground truth mask shape {gt_masks.shape} doesn't match predicted mask shape {pred_masks.shape}")

    if args.binary:
        logger.info(f"Computing binary PQ metrics with IoU threshold {args.match_iou}")
        results = compute_binary_pq_metrics(gt_masks, pred_masks, match_iou=args.match_iou,
                                            no_border_instances=args.no_border_instances)
        print("\nResults:")
        print(results.to_string(index=False))
        if args.output:
            results.to_csv(args.output, index=False)
            logger.info(f"Results saved to {args.output}")
        return
    logger.info(f"Computing multi-class PQ metrics with IoU threshold {args.match_iou} for {nr_classes} classes")
    global_results, per_image_results = compute_multiclass_pq_metrics(
        gt_masks, pred_masks, match_iou=args.match_iou, nr_classes=nr_classes, n_workers=args.n_workers,
        no_border_instances=args.no_border_instances)
    print("\nGlobal Results:")
    print(global_results.to_string(index=False))
    print("\nPer-Image Results:")
    print(per_image_results.head().to_string(index=False))
    if args.output:
        Path(args.output).parent.mkdir(parents=True, exist_ok=True)
        global_results.to_csv(args.output, index=False)
        logger.info(f"Global results saved to {args.output}")
        base, _, ext = args.output.rpartition(".")
        per_image_output = f"{base}_per_image.{ext}" if base else f"{args.output}_per_image.csv"
        per_image_results.to_csv(per_image_output, index=False)
        logger.info(f"Per-image results saved to {per_image_output}")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Compute PQ (Panoptic Quality) metrics between ground truth and predicted masks.")
    p.add_argument("--gt_path", required=True, help="Path to ground truth masks (directory or file)")
    p.add_argument("--pred_path", required=True, help="Path to predicted masks (directory or file)")
    p.add_argument("--match_iou", type=float, default=0.5, help="IoU threshold for matching instances")
    p.add_argument("--output", type=str, default=None, help="Path to save results as CSV")
    p.add_argument("--binary", action="store_true", help="Treat masks as binary instance segmentation without classes")
    p.add_argument("--ignore_classes", type=int, default=None, nargs="+", help="Classes to ignore.")
    p.add_argument("--label_map", type=str, nargs="+", default=None,
                   help="Label map for multi-class conversion: a list of k=v index pairs, e.g. --label_map 0=0 1=1 2=2.")
    p.add_argument("--no_border_instances", action="store_true", default=False,
                   help="Whether to remove border instances for metrics computations.")
    p.add_argument("--n_workers", type=int, default=1, help="Accepted for compatibility and ignored: a batch is one device pass")
    return p


def main_with_args() -> None:
    main(build_parser().parse_args())


if __name__ == "__main__":
    main_with_args()
