"""``python -m classpose_amd.entrypoints.calculate_metrics_geojson``: panoptic quality of a predicted GeoJSON (what
``predict_wsi`` writes) against an annotated one, over regions of the slide.

Both files are rasterised per region on the device (``classpose_amd.annotations.rasterize`` -> ``cpx_rasterize_polygons``) and
the device maps go straight into ``ops.pq_stats``: no map is copied to the host.  Tables and CSV files come from the same functions
of ``classpose_amd.metrics.pq`` as ``calculate_metrics`` uses; one "image" of those tables is one region, in the order given.
``nr_classes`` is the number of ``--class_names``.

    python -m classpose_amd.entrypoints.calculate_metrics_geojson --gt_geojson G --pred_geojson P --class_names N1 N2 ... \\
        (--region X Y W H [--region ...] | --roi_geojson F) [--downsample D] [--match_iou 0.5] [--binary] \\
        [--no_border_instances] [--ignore_unknown] [--coordinate_offset O] [--max_region_px N] [--output CSV]
"""
from __future__ import annotations

import argparse
import math
from pathlib import Path

import numpy as np

from ..log import get_logger

logger = get_logger(__name__)

MAX_REGION_PX = 1 << 26          # 8192 x 8192: four maps of it and pq_stats' tables of 2 * H * W slots stay within a few GiB


def regions_of(args) -> list[tuple[float, float, float, float]]:
    """``--region`` quadruples as given, or the bounding boxes of ``--roi_geojson``'s polygons grown to whole pixels."""
    if (args.region is None) == (args.roi_geojson is None):
        raise SystemExit("give --region X Y W H (repeatable) or --roi_geojson F, one of the two")
    if args.region is not None:
        regions = [tuple(float(v) for v in r) for r in args.region]
    else:
        from ..roi import load_roi_polygons
        polys = load_roi_polygons(args.roi_geojson)
        if not polys:
            raise SystemExit(f"{args.roi_geojson}: no polygon")
        regions = []
        for p in polys:
            x0, y0, x1, y1 = p.bounds
            x, y = math.floor(x0), math.floor(y0)
            regions.append((float(x), float(y), float(math.ceil(x1) - x + 1), float(math.ceil(y1) - y + 1)))
    for x, y, w, h in regions:
        if not all(math.isfinite(v) for v in (x, y, w, h)) or w <= 0 or h <= 0:
            raise SystemExit(f"region {(x, y, w, h)}: width and height must be positive")
    return regions


def region_stats(gt, pred, regions, nr_classes: int | None, downsample: float, coordinate_offset: float, match_iou: float,
                 no_border_instances: bool, max_region_px: int, device="cuda"):
    """(tp, fp, fn, iou_sum), each (n_regions, nr_classes): regions grouped by size, one device batch per group; ``nr_classes
    is None`` = binary."""
    from .. import annotations, ops
    from ..metrics.pq import assignment_stats
    binary = nr_classes is None
    nr = 1 if binary else int(nr_classes)
    out = [np.zeros((len(regions), nr), np.int32) for _ in range(3)] + [np.zeros((len(regions), nr), np.float64)]
    groups: dict = {}
    for i, (_x, _y, w, h) in enumerate(regions):
        W, H = math.ceil(w / downsample), math.ceil(h / downsample)
        if H * W > max_region_px:
            raise SystemExit(f"region {i} is {W} x {H} = {H * W} pixels at downsample {downsample}, above --max_region_px "
                             f"{max_region_px}: give smaller regions (or a larger --downsample)")
        groups.setdefault((w, h), []).append(i)
    for idx in groups.values():
        sub = [regions[i] for i in idx]
        ti, tc = annotations.rasterize(gt, sub, downsample, coordinate_offset, device)
        pi, pc = annotations.rasterize(pred, sub, downsample, coordinate_offset, device)
        res = ops.pq_stats(ti, pi, None if binary else tc, None if binary else pc, nr_classes=nr, match_iou=match_iou,
                           no_border_instances=no_border_instances, return_lists=match_iou == 0.0)
        if match_iou == 0.0:
            stats = assignment_stats(res["pairs"], res["insts"], res["nobg"], len(idx), nr)
        else:
            stats = (res["tp"], res["fp"], res["fn"], res["iou_sum"])
        for o, s in zip(out, stats):
            o[idx] = s
    return tuple(out)


def main(args) -> None:
    from .. import annotations
    from ..metrics.pq import binary_table, multiclass_tables
    regions = regions_of(args)
    if args.downsample <= 0 or not math.isfinite(args.downsample):
        raise SystemExit("--downsample must be positive")
    if args.match_iou < 0:
        raise SystemExit("--match_iou must not be negative")
    if not 1 <= len(args.class_names) <= 255:
        raise SystemExit("--class_names: between 1 and 255 names")
    gt = annotations.load_features(args.gt_geojson, args.class_names, ignore_unknown=args.ignore_unknown)
    pred = annotations.load_features(args.pred_geojson, args.class_names, ignore_unknown=args.ignore_unknown)
    for name, a in (("ground truth", gt), ("prediction", pred)):
        logger.info(f"{name}: {a.n_features} features, {len(a.ring_feature)} rings, {a.n_points} Point features skipped")
    nr = None if args.binary else len(args.class_names)
    tp, fp, fn, iou_sum = region_stats(gt, pred, regions, nr, args.downsample, args.coordinate_offset, args.match_iou,
                                       args.no_border_instances, args.max_region_px)
    if args.binary:
        results = binary_table(tp[:, 0], fp[:, 0], fn[:, 0], iou_sum[:, 0])
        print("\nResults:")
        print(results.to_string(index=False))
        if args.output:
            Path(args.output).parent.mkdir(parents=True, exist_ok=True)
            results.to_csv(args.output, index=False)
            logger.info(f"Results saved to {args.output}")
        return
    global_results, per_image_results = multiclass_tables(tp, fp, fn, iou_sum)
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
    p = argparse.ArgumentParser(description="Compute PQ (Panoptic Quality) metrics between an annotated and a predicted GeoJSON.")
    p.add_argument("--gt_geojson", required=True, help="annotated cells: FeatureCollection or feature list, Polygon / MultiPolygon")
    p.add_argument("--pred_geojson", required=True, help="predicted cells, e.g. the cell contours predict_wsi writes")
    p.add_argument("--class_names", required=True, nargs="+", help="classification names in class order: the first is class 1")
    p.add_argument("--region", type=float, nargs=4, action="append", metavar=("X", "Y", "W", "H"), default=None,
                   help="a region to score, in the files' coordinates; repeatable, one table row ('image') per region")
    p.add_argument("--roi_geojson", default=None, help="score the bounding boxes of this file's polygons instead of --region")
    p.add_argument("--downsample", type=float, default=1.0, help="file units per map pixel")
    p.add_argument("--coordinate_offset", type=float, default=0.0, help="added to every coordinate of both files")
    p.add_argument("--match_iou", type=float, default=0.5, help="IoU threshold for matching instances")
    p.add_argument("--binary", action="store_true", help="score instances only, without classes")
    p.add_argument("--no_border_instances", action="store_true", default=False, help="drop instances on a region's border")
    p.add_argument("--ignore_unknown", action="store_true", help="a feature with a name outside --class_names gets class 0 instead of an error")
    p.add_argument("--max_region_px", type=int, default=MAX_REGION_PX, help="largest region in map pixels (default 8192 x 8192)")
    p.add_argument("--output", type=str, default=None, help="Path to save results as CSV")
    return p


def main_with_args() -> None:
    main(build_parser().parse_args())


if __name__ == "__main__":
    main_with_args()
