"""Device panoptic-quality statistics (cpx_pq_stats -> ops.pq_stats -> classpose_amd.metrics -> the calculate-metrics CLI) against
the reference's own results (tests/golden/reference_pq.*) and, where the reference is too slow to mint, against the numpy
restatement of tests/test_pq_host.py (itself pinned on the fixture there).

Bounds (derived, not measured): tp / fp / fn are exact.  Every IoU is ONE float64 division of exactly converted integers, bitwise
the reference's, and non-negative; two float64 summation orders of n such terms differ by at most 2 (n - 1) * 2^-53 * S, so
iou_sum is within n * 2^-52 * S of the reference's S (n = the entry's tp) and exactly equal for n <= 1.  pq / dq / sq / precision /
recall / f1 / avg_iou follow by the same host formulas: rtol n * 2^-52 plus one rounding (2^-53) per operation, of which no
formula has more than four; the avg row averages nr_classes such values.
"""
from __future__ import annotations

import io
import os
import subprocess
import sys

import numpy as np
import pytest

from test_pq_host import EPS52, all_runs, case_masks, close_sum, load_fixture, restate

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_frame(df, gold, n_of_row, extra_roundings=0):
    """columns and order exactly, integers and strings exactly, floats within (n + 2 + extra) * 2^-52 relative (exact for n <= 1
    where the value is a plain iou_sum); NaN where the reference has NaN"""
    assert list(df.columns) == list(gold.keys())
    for col in df.columns:
        got, want = df[col].tolist(), gold[col]
        assert len(got) == len(want), col
        for r, (g, w) in enumerate(zip(got, want)):
            if isinstance(w, str):
                assert g == w, (col, r, g, w)
            elif isinstance(w, int):
                assert isinstance(g, (int, np.integer)) and g == w, (col, r, g, w)
            elif np.isnan(w):
                assert np.isnan(g), (col, r, g)
            else:
                n = n_of_row(r)
                assert g == w or abs(g - w) <= (n + 2 + extra_roundings) * EPS52 * abs(w), (col, r, g, w, n)


@pytest.mark.parametrize("name,k", all_runs())
def test_every_fixture_case_through_the_metrics_module(cuda, name, k):
    from classpose_amd import metrics
    npz, meta = load_fixture()
    case = next(c for c in meta["cases"] if c["name"] == name)
    run = case["runs"][k]
    gt, pred = case_masks(npz, case)
    nr = case["nr_classes"]
    keep = [(g.copy(), p.copy()) for g, p in zip(gt, pred)]
    gdf, idf = metrics.compute_multiclass_pq_metrics(gt, pred, match_iou=run["match_iou"], nr_classes=nr,
                                                     no_border_instances=run["border"])
    assert all(np.array_equal(a, g) and np.array_equal(b, p) for (a, b), g, p in zip(keep, gt, pred)), "inputs were modified"
    tp = np.array(run["tp"]); S = np.array(run["iou_sum"])
    # per-(image, class) statistics: counts exactly, iou_sum (= avg_iou * tp there) through the per-image frame's own columns
    for i in range(case["n_images"]):
        for c in range(nr):
            assert idf[f"class_{c + 1}_tp"][i] == run["tp"][i][c], (i, c)
            assert idf[f"class_{c + 1}_fp"][i] == run["fp"][i][c], (i, c)
            assert idf[f"class_{c + 1}_fn"][i] == run["fn"][i][c], (i, c)
    from classpose_amd.metrics import pq as mpq
    st = mpq.device_stats(gt, pred, nr, run["match_iou"], run["border"])
    assert np.array_equal(st[0], tp) and np.array_equal(st[1], np.array(run["fp"])) and np.array_equal(st[2], np.array(run["fn"]))
    for i in range(case["n_images"]):
        for c in range(nr):
            print(f"{name} iou {run['match_iou']} border {run['border']} image {i} class {c + 1}: tp {tp[i, c]} iou_sum {st[3][i, c]!r} "
                  f"reference {S[i, c]!r}")
            assert close_sum(st[3][i, c], S[i, c], tp[i, c]), (i, c, st[3][i, c], S[i, c])
    tot = tp.sum(0)
    _check_frame(idf, run["per_image_df"], lambda r: int(tp[r].max(initial=0)))
    _check_frame(gdf, run["global_df"], lambda r: int(tot[r]) + case["n_images"] if r < nr else int(tot.sum()) + case["n_images"] * nr, extra_roundings=nr + 2)
    b = run.get("binary_df")
    ids = lambda ms: [m[..., 0] for m in ms]
    if isinstance(b, dict):
        bdf = metrics.compute_binary_pq_metrics(ids(gt), ids(pred), match_iou=run["match_iou"], no_border_instances=run["border"])
        _check_frame(bdf, b, lambda r: int(b["tp"][r]))
    elif b == "ZeroDivisionError":
        with pytest.raises(ZeroDivisionError):
            metrics.compute_binary_pq_metrics(ids(gt), ids(pred), match_iou=run["match_iou"], no_border_instances=run["border"])


def test_two_calls_give_the_same_bits(cuda):
    import torch
    from classpose_amd import ops
    npz, meta = load_fixture()
    case = next(c for c in meta["cases"] if c["name"] == "scenes_256")
    gt, pred = case_masks(npz, case)
    dev = lambda a, dt: torch.from_numpy(np.stack(a).astype(dt)).to(cuda)
    args = (dev([g[..., 0] for g in gt] * 8, np.int32), dev([p[..., 0] for p in pred] * 8, np.int32),
            dev([g[..., 1] for g in gt] * 8, np.uint8), dev([p[..., 1] for p in pred] * 8, np.uint8))
    for iou in (0.3, 0.5):
        a = ops.pq_stats(*args, nr_classes=6, match_iou=iou, no_border_instances=True)
        b = ops.pq_stats(*args, nr_classes=6, match_iou=iou, no_border_instances=True)
        for key in ("tp", "fp", "fn"):
            assert np.array_equal(a[key], b[key])
        assert a["iou_sum"].tobytes() == b["iou_sum"].tobytes()
        assert a["tp"].sum() > 100
        # the 16 images are 8 copies of 2: every copy has the same bits too
        assert all(a["iou_sum"][i].tobytes() == a["iou_sum"][i % 2].tobytes() for i in range(16))


def test_engine_outputs_against_themselves_without_a_host_copy(cuda):
    """masks (uint16 in int16) and classes straight from ops.compute_masks, as truth and prediction: per class tp = its
    instances, fp = fn = 0 and iou_sum == tp exactly (every IoU is 1.0)"""
    import torch
    from classpose_amd import ops, synth
    fields = [synth.analytic_fields(1234 + s, 0, 0, 256, 256, 7) for s in range(3)]
    dP, cp, lg = (torch.from_numpy(np.stack([f[j] for f in fields])).to(cuda) for j in range(3))
    masks, cm, nlab = ops.compute_masks(dP, cp, lg)
    assert masks.dtype == torch.int16 and cm.dtype == torch.uint8
    nr = int(cm.max().item())
    assert nr >= 2
    res = ops.pq_stats(masks, masks, cm, cm, nr_classes=nr, match_iou=0.5)
    m, c = ops.masks_to_numpy(masks), cm.cpu().numpy()
    for i in range(3):
        for k in range(1, nr + 1):
            want = len(np.unique(m[i][(c[i] == k) & (m[i] > 0)]))
            assert res["tp"][i, k - 1] == want and res["fp"][i, k - 1] == 0 and res["fn"][i, k - 1] == 0, (i, k, want)
            assert res["iou_sum"][i, k - 1] == float(want)
    assert res["tp"].sum() > 0
    b = ops.pq_stats(masks, masks)
    n_inst = np.array([len(np.unique(m[i][m[i] > 0])) for i in range(3)])
    assert n_inst.min() > 0 and np.array_equal(n_inst, nlab.cpu().numpy())
    assert np.array_equal(b["tp"][:, 0], n_inst) and not b["fp"].any() and not b["fn"].any()
    assert np.array_equal(b["iou_sum"][:, 0], n_inst.astype(np.float64))


def test_capacity_every_pixel_its_own_instance(cuda):
    """256^2, every pixel its own instance, against a copy shifted by one pixel: H * W instances and pairs per image.  Correct, or
    an error that names the limit -- never a wrong count."""
    import torch
    from classpose_amd import _lib, ops
    H = W = 256
    t = np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W)
    p = np.roll(t, 1, axis=1)
    want = restate(t, p, 1, 0.5, False, binary=True)[0]
    assert want[0] > 60000
    ti, pi = torch.from_numpy(t).to(cuda)[None], torch.from_numpy(p).to(cuda)[None]
    res = ops.pq_stats(ti, pi)
    assert [res["tp"][0, 0], res["fp"][0, 0], res["fn"][0, 0]] == want[:3]
    assert close_sum(res["iou_sum"][0, 0], want[3], want[0])
    # with classes: columns alternate between two classes, so the shifted copy never has the class of its pixel's truth
    ct = torch.from_numpy((1 + (np.arange(W) % 2))[None, :].repeat(H, 0).astype(np.uint8)).to(cuda)[None]
    res = ops.pq_stats(ti, pi, ct, ct, nr_classes=2)
    g, q = np.stack([t, ct[0].cpu().numpy()], -1), np.stack([p, ct[0].cpu().numpy()], -1)
    want2 = restate(g, q, 2, 0.5, False)
    for c in range(2):
        assert [res["tp"][0, c], res["fp"][0, c], res["fn"][0, c]] == want2[c][:3]
        assert close_sum(res["iou_sum"][0, c], want2[c][3], want2[c][0])
    # a table that is too small is an error naming the limit, not a truncated count
    with pytest.raises(_lib.CpxError, match="table_cap"):
        ops.pq_stats(ti, pi, table_cap=4096)


def test_capacity_batch_of_many_images(cuda):
    import torch
    from classpose_amd import ops
    npz, meta = load_fixture()
    case = next(c for c in meta["cases"] if c["name"] == "scenes_96x128")
    gt, pred = case_masks(npz, case)
    rng = np.random.default_rng(5)
    n = 96
    gts, prs = [], []
    for i in range(n):
        g, p = gt[i % 3], pred[(i + i // 3) % 3]
        s = (int(rng.integers(0, 5)), int(rng.integers(0, 5)))
        gts.append(g); prs.append(np.roll(p, s, (0, 1)))
    # one pathological image in the middle of the batch: it alone is repeated with full tables
    H, W = gts[0].shape[:2]
    dense = np.stack([np.arange(1, H * W + 1, dtype=np.int32).reshape(H, W), np.ones((H, W), np.int32)], -1)
    gts[40], prs[40] = dense, dense.copy()
    dev = lambda a, dt: torch.from_numpy(np.stack(a).astype(dt)).to(cuda)
    res = ops.pq_stats(dev([g[..., 0] for g in gts], np.int32), dev([p[..., 0] for p in prs], np.int32),
                       dev([g[..., 1] for g in gts], np.uint8), dev([p[..., 1] for p in prs], np.uint8),
                       nr_classes=6, match_iou=0.5, no_border_instances=True)
    for i in range(n):
        want = restate(gts[i], prs[i], 6, 0.5, True)
        for c in range(6):
            assert [res["tp"][i, c], res["fp"][i, c], res["fn"][i, c]] == want[c][:3], (i, c)
            assert close_sum(res["iou_sum"][i, c], want[c][3], want[c][0]), (i, c)


def _read_csv(text):
    import pandas as pd
    return pd.read_csv(io.StringIO(text))


@pytest.mark.parametrize("which", [0, 1, 2])
def test_cli_in_a_child_process(cuda, tmp_path, which):
    """``python -m classpose_amd.entrypoints.calculate_metrics`` on .npy files written from the fixture: both CSVs against the
    reference CLI's (label map, --ignore_classes, --binary --no_border_instances)"""
    npz, meta = load_fixture()
    rec = meta["cli"][which]
    gt = np.stack([npz["scenes_96x128/gt_0"], npz["scenes_96x128/gt_1"]]).astype(np.int64)
    pr = np.stack([npz["scenes_96x128/pred_0"], npz["scenes_96x128/pred_1"]]).astype(np.int64)
    binary = bool(rec["args"].get("binary"))
    if binary:
        gt, pr = gt[..., 0], pr[..., 0]
    np.save(tmp_path / "gt.npy", gt); np.save(tmp_path / "pred.npy", pr)
    out = tmp_path / ("res.csv" if binary else os.path.join("out", "res.csv"))
    cmd = [sys.executable, "-m", "classpose_amd.entrypoints.calculate_metrics", "--gt_path", str(tmp_path / "gt.npy"),
           "--pred_path", str(tmp_path / "pred.npy"), "--output", str(out)]
    for k, v in rec["args"].items():
        cmd += [f"--{k}"] + ([] if v is True else [str(x) for x in v])
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert ("\nResults:" in r.stdout) if binary else ("\nGlobal Results:" in r.stdout and "\nPer-Image Results:" in r.stdout)
    assert set(rec["csv"]) == ({"res.csv"} if binary else {"res.csv", "res_per_image.csv"})
    for fname, text in rec["csv"].items():
        want, got = _read_csv(text), _read_csv(open(out.parent / fname).read())
        assert list(got.columns) == list(want.columns), fname
        assert len(got) == len(want)
        ntot = int(want[[c for c in want.columns if c == "tp" or c.endswith("_tp")]].to_numpy().sum()) + 16
        for col in want.columns:
            for g, w in zip(got[col].tolist(), want[col].tolist()):
                if isinstance(w, str) or isinstance(w, (int, np.integer)):
                    assert g == w, (fname, col, g, w)
                elif np.isnan(w):
                    assert np.isnan(g), (fname, col)
                else:
                    assert g == w or abs(g - w) <= ntot * EPS52 * abs(w), (fname, col, g, w)


def test_cli_ignore_classes_on_a_directory_of_ragged_masks(cuda, tmp_path):
    """the one CLI behaviour changed on purpose: --ignore_classes is applied per image, so a directory of differently shaped masks
    works (the reference indexes the list there and fails).  Expected tables: the host assembly over the restatement's statistics
    of the maps with the ignored class zeroed; nr_classes stays the largest true class BEFORE that."""
    from classpose_amd.metrics import pq as mpq
    npz, meta = load_fixture()
    case = next(c for c in meta["cases"] if c["name"] == "ragged")
    gt, pred = case_masks(npz, case)
    (tmp_path / "gt").mkdir(); (tmp_path / "pred").mkdir()
    for i, (g, p) in enumerate(zip(gt, pred)):
        np.save(tmp_path / "gt" / f"m{i:02d}.npy", g); np.save(tmp_path / "pred" / f"m{i:02d}.npy", p)
    out = tmp_path / "res.csv"
    r = subprocess.run([sys.executable, "-m", "classpose_amd.entrypoints.calculate_metrics", "--gt_path", str(tmp_path / "gt"),
                        "--pred_path", str(tmp_path / "pred"), "--output", str(out), "--ignore_classes", "2", "--match_iou", "0.3"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    nr = int(max(g[..., 1].max() for g in gt))
    assert nr == case["nr_classes"]
    zero2 = lambda m: np.stack([m[..., 0], np.where(m[..., 1] == 2, 0, m[..., 1])], -1)
    st = [restate(zero2(g), zero2(p), nr, 0.3, False) for g, p in zip(gt, pred)]
    want_g, want_i = mpq.multiclass_tables(*(np.array([[s[c][j] for c in range(nr)] for s in st]) for j in range(4)))
    assert not want_g["tp"][1] and want_g["tp"][0] > 0                 # class 2 is gone, class 1 is not
    ntot = int(want_g["tp"].iloc[-1]) + 16
    for path, want in ((out, want_g), (tmp_path / "res_per_image.csv", want_i)):
        got, want = _read_csv(open(path).read()), _read_csv(want.to_csv(index=False))
        assert list(got.columns) == list(want.columns) and len(got) == len(want)
        for col in want.columns:
            for g, w in zip(got[col].tolist(), want[col].tolist()):
                if isinstance(w, (str, int, np.integer)):
                    assert g == w, (col, g, w)
                elif np.isnan(w):
                    assert np.isnan(g), col
                else:
                    assert g == w or abs(g - w) <= ntot * EPS52 * abs(w), (col, g, w)
