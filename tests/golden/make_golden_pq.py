"""Mint the panoptic-quality fixture from the REFERENCE's own functions (run in the build container only).

    python tests/golden/make_golden_pq.py      # rewrites tests/golden/reference_pq.npz / .json

The reference's ``classpose.metrics`` is imported under the stub finder of make_golden.py; ``fastremap.renumber`` is
``oracle.dynamics.fr_renumber`` (pinned as a first-appearance pass by tests/test_oracle_hardening.py).  Called:
``filter_out_unlabelled_cells``, ``remove_border_instances``, ``get_multi_pq_info``, ``get_pq`` (incl. the assignment branch),
``compute_multiclass_pq_metrics``, ``compute_binary_pq_metrics`` and the CLI's ``main(args)``.  The fixture holds data only:
the input maps, per-(image, class) tp / fp / fn / iou_sum, and the DataFrames as column lists.  The reference's CPU time per
image is printed (context for profiles/pq_bench.txt).
"""
from __future__ import annotations

import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
os.environ.setdefault("TQDM_DISABLE", "1")

IOUS = (0.0, 0.3, 0.5, 0.75)


def blobs(rng, H, W, n, nr, rmin=3, rmax=7, id_mul=1, id_add=0):
    """(H, W, 2) int32 map of up to n discs (later ones overwrite), ids id_mul * k + id_add, one class in 1..nr each."""
    m = np.zeros((H, W, 2), np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    cells = []
    for k in range(1, n + 1):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(rmin, rmax + 1)
        c = int(rng.integers(1, nr + 1))
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        m[d, 0] = id_mul * k + id_add
        m[d, 1] = c
        cells.append((cy, cx, r, c))
    return m, cells


def perturb(rng, gt, nr, hi_cls):
    """A prediction from a truth: shifted, some cells missed, some spurious, some with another class (incl. > nr)."""
    H, W, _ = gt.shape
    dy, dx = (int(v) for v in rng.integers(-2, 3, 2))
    p = np.roll(gt, (dy, dx), (0, 1)).copy()
    ids = np.unique(p[..., 0]); ids = ids[ids > 0]
    for i in ids:
        u = rng.random()
        sel = p[..., 0] == i
        if u < 0.12:
            p[sel] = 0                                    # missed
        elif u < 0.30:
            p[sel, 1] = int(rng.integers(1, hi_cls + 1))  # class mismatch, possibly above nr_classes
        elif u < 0.40:
            ys = np.nonzero(sel.any(1))[0]
            p[ys[len(ys) // 2]:, :][sel[ys[len(ys) // 2]:, :]] = 0      # half the cell only
    extra, _ = blobs(rng, H, W, max(2, len(ids) // 8), nr, id_mul=1, id_add=int(gt[..., 0].max()) + 100)
    free = (p[..., 0] == 0) & (extra[..., 0] > 0)
    p[free] = extra[free]                                 # spurious
    p[..., 0] = np.where(p[..., 0] > 0, p[..., 0] * 2 + 5, 0)           # ids unrelated to the truth's, non-contiguous
    return p


def truth(rng, H, W, n, nr, **kw):
    g, _ = blobs(rng, H, W, n, nr, **kw)
    ids = np.unique(g[..., 0]); ids = ids[ids > 0]
    for i in ids:
        u = rng.random()
        sel = g[..., 0] == i
        if u < 0.12:
            g[sel, 1] = 0                                 # unlabelled cell
        elif u < 0.24:
            xs = np.nonzero(sel.any(0))[0]
            half = sel & (np.arange(W)[None, :] >= xs[len(xs) // 2])
            g[half, 1] = g[sel, 1][0] % nr + 1            # an instance with two classes
    return g


def build_cases(rng):
    cases = []
    # random scenes, non-contiguous ids, 96 x 128 and 256^2
    gts = [truth(rng, 96, 128, 40, 6, id_mul=3, id_add=7) for _ in range(3)]
    cases.append(dict(name="scenes_96x128", nr=6, gt=gts, pred=[perturb(rng, g, 6, 8) for g in gts], ious=IOUS, borders=(False, True)))
    gts = [truth(rng, 256, 256, 150, 6, id_mul=2, id_add=1) for _ in range(2)]
    cases.append(dict(name="scenes_256", nr=6, gt=gts, pred=[perturb(rng, g, 6, 7) for g in gts], ious=IOUS, borders=(False, True)))
    # unlabelled cells: one with a matching prediction (both leave), one with a poor overlap (the prediction stays, in no class)
    g = np.zeros((32, 32, 2), np.int32); p = np.zeros_like(g)
    g[4:10, 4:10] = (1, 0); p[4:10, 5:11] = (9, 2)        # IoU 30/42 > 0.5 -> removed
    g[4:10, 20:26] = (2, 0); p[8:14, 22:28] = (4, 1)      # IoU 8/64 -> stays (a class-1 false positive)
    g[20:26, 4:10] = (5, 1); p[20:26, 4:10] = (3, 1)
    g[20:26, 20:26] = (6, 2)                              # missed
    g[14:18, 12:18] = (8, 0)                              # unlabelled, no prediction at all
    cases.append(dict(name="unlabelled", nr=2, gt=[g], pred=[p], ious=IOUS, borders=(False, True)))
    # empty true / empty predicted / both empty, in one batch with a plain pair
    a, _ = blobs(rng, 40, 40, 6, 3)
    z = np.zeros_like(a)
    cases.append(dict(name="empties", nr=3, gt=[a, z, z, a], pred=[z, a, z, a.copy()], ious=IOUS, borders=(False, True), binary=False))
    # a map without background: two instances tile 8 x 8 (class 1), against themselves and against another split
    t = np.ones((8, 8, 2), np.int32); t[:, 4:, 0] = 2
    q = np.ones((8, 8, 2), np.int32); q[5:, :, 0] = 7
    h = t.copy(); h[0, 0] = 0                              # the same with one background pixel
    cases.append(dict(name="no_background", nr=2, gt=[t, t, h, t, q], pred=[t.copy(), q, t.copy(), h.copy(), h.copy()], ious=IOUS, borders=(False,)))
    # IoU of exactly 0.5 (inter 1, union 2; inter 6, union 12) must not match at 0.5
    g = np.zeros((12, 12, 2), np.int32); p = np.zeros_like(g)
    g[2, 2] = (1, 1); p[2, 2:4] = (1, 1)
    g[6:8, 2:5] = (2, 2); p[6:8, 2:8] = (2, 2)
    g[10, 2:6] = (3, 1); p[10, 2:5] = (3, 1)              # 3/4
    cases.append(dict(name="iou_half", nr=2, gt=[g], pred=[p], ious=IOUS, borders=(False, True)))
    # ragged shapes, one of them with an odd pixel count
    shapes = [(64, 64), (50, 37), (96, 128), (50, 37), (33, 70)]
    gts = [truth(rng, h_, w_, 14, 4, id_mul=5, id_add=2) for h_, w_ in shapes]
    cases.append(dict(name="ragged", nr=4, gt=gts, pred=[perturb(rng, g, 4, 5) for g in gts], ious=IOUS, borders=(False, True)))
    # one 1024^2 image with >= 1000 cells and 10 classes
    g = truth(rng, 1024, 1024, 1500, 10, rmin=6, rmax=11)
    assert len(np.unique(g[..., 0])) > 1000
    cases.append(dict(name="big_1024", nr=10, gt=[g], pred=[perturb(rng, g, 10, 11)], ious=(0.5,), borders=(False,), binary=False))
    return cases


def frame(df):
    return {c: [v.item() if hasattr(v, "item") else v for v in df[c].tolist()] for c in df.columns}


def main():
    import make_golden
    from oracle.dynamics import fr_renumber
    sys.meta_path.insert(0, make_golden._Finder())
    fr = types.ModuleType("fastremap")
    fr.renumber = lambda a, **kw: (fr_renumber(a), {})
    sys.modules["fastremap"] = fr
    sys.path.insert(0, make_golden.REF)
    from classpose.metrics import pq as rpq
    from classpose.metrics.stats_utils import get_multi_pq_info
    from classpose.metrics.utils import filter_out_unlabelled_cells
    from classpose.entrypoints import calculate_metrics as rcli

    rng = np.random.default_rng(20261016)
    arrays, meta = {}, {"cases": [], "cli": []}
    for case in build_cases(rng):
        name, nr = case["name"], case["nr"]
        for i, (g, p) in enumerate(zip(case["gt"], case["pred"])):
            arrays[f"{name}/gt_{i}"] = g.astype(np.int32)
            arrays[f"{name}/pred_{i}"] = p.astype(np.int32)
        runs = []
        for iou in case["ious"]:
            for border in case["borders"]:
                t0 = time.perf_counter()
                gts = [g.astype(np.int64).copy() for g in case["gt"]]
                prs = [p.astype(np.int64).copy() for p in case["pred"]]
                gts, prs = filter_out_unlabelled_cells(gts, prs)
                stats = []
                for g, p in zip(gts, prs):
                    if border:
                        g, p = rpq.remove_border_instances(g), rpq.remove_border_instances(p)
                    stats.append(get_multi_pq_info(g, p, nr_classes=nr, match_iou=iou))
                dt = time.perf_counter() - t0
                gdf, idf = rpq.compute_multiclass_pq_metrics([g.astype(np.int64).copy() for g in case["gt"]],
                                                             [p.astype(np.int64).copy() for p in case["pred"]],
                                                             match_iou=iou, nr_classes=nr, no_border_instances=border)
                run = dict(match_iou=iou, border=border,
                           tp=[[int(s[c][0]) for c in range(nr)] for s in stats], fp=[[int(s[c][1]) for c in range(nr)] for s in stats],
                           fn=[[int(s[c][2]) for c in range(nr)] for s in stats], iou_sum=[[float(s[c][3]) for c in range(nr)] for s in stats],
                           global_df=frame(gdf), per_image_df=frame(idf))
                if case.get("binary", True):
                    try:
                        bdf = rpq.compute_binary_pq_metrics([g[..., 0].astype(np.int64).copy() for g in case["gt"]],
                                                            [p[..., 0].astype(np.int64).copy() for p in case["pred"]],
                                                            match_iou=iou, no_border_instances=border)
                        run["binary_df"] = frame(bdf)
                    except ZeroDivisionError:
                        run["binary_df"] = "ZeroDivisionError"
                runs.append(run)
                print(f"{name}: match_iou {iou} border {border}: reference {dt / len(case['gt']):.3f} s per image "
                      f"({case['gt'][0].shape[0]} x {case['gt'][0].shape[1]}, {nr} classes)")
        meta["cases"].append(dict(name=name, nr_classes=nr, n_images=len(case["gt"]), runs=runs))
    # binary on an image without instances raises
    try:
        rpq.compute_binary_pq_metrics(np.zeros((1, 8, 8), np.int64), np.zeros((1, 8, 8), np.int64))
        meta["binary_empty_raises"] = False
    except ZeroDivisionError:
        meta["binary_empty_raises"] = True

    # the CLI's main(args) on the first two 96 x 128 scenes
    gt = np.stack([arrays["scenes_96x128/gt_0"], arrays["scenes_96x128/gt_1"]])
    pr = np.stack([arrays["scenes_96x128/pred_0"], arrays["scenes_96x128/pred_1"]])
    for extra in (dict(label_map=["1=1", "2=1", "3=2", "4=2", "5=3", "6=3", "7=3", "8=3"]), dict(ignore_classes=[2, 5]),
                  dict(binary=True, no_border_instances=True)):
        with tempfile.TemporaryDirectory() as d:
            ch = (..., 0) if extra.get("binary") else (...,)          # binary masks are (N, H, W)
            np.save(os.path.join(d, "gt.npy"), gt.astype(np.int64)[ch]); np.save(os.path.join(d, "pred.npy"), pr.astype(np.int64)[ch])
            a = dict(gt_path=os.path.join(d, "gt.npy"), pred_path=os.path.join(d, "pred.npy"), match_iou=0.5,
                     output=os.path.join(d, "out", "res.csv") if not extra.get("binary") else os.path.join(d, "res.csv"),
                     binary=False, ignore_classes=None, label_map=None, no_border_instances=False, n_workers=1)
            a.update(extra)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                rcli.main(argparse.Namespace(**a))
            files = {}
            for root, _dirs, names in os.walk(d):
                for f in names:
                    if f.endswith(".csv"):
                        files[f] = open(os.path.join(root, f)).read()
            meta["cli"].append(dict(args={k: v for k, v in extra.items()}, stdout=buf.getvalue(), csv=files))
    np.savez_compressed(os.path.join(HERE, "reference_pq.npz"), **arrays)
    with open(os.path.join(HERE, "reference_pq.json"), "w") as f:
        json.dump(meta, f)
    print("wrote", os.path.getsize(os.path.join(HERE, "reference_pq.npz")), os.path.getsize(os.path.join(HERE, "reference_pq.json")), "bytes")


if __name__ == "__main__":
    main()
