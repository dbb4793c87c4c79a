"""Host side of the panoptic-quality metrics (no GPU): table assembly, the assignment branch, mask loading, the CLI's flags and
label map -- against tests/golden/reference_pq.* minted from the reference (tests/golden/make_golden_pq.py).

``restate`` below is a numpy restatement of the pair-table formulation the device implements (one co-occurrence table per image
instead of the reference's loops).  It must equal the golden statistics on EVERY fixture case; the GPU tests then use it as the
expected value where the reference is too slow to mint (capacity cases, large batches).
"""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
EPS52 = 2.0 ** -52


def load_fixture():
    npz = np.load(os.path.join(HERE, "golden", "reference_pq.npz"))
    with open(os.path.join(HERE, "golden", "reference_pq.json")) as f:
        meta = json.load(f)
    return npz, meta


def case_masks(npz, case):
    gt = [npz[f"{case['name']}/gt_{i}"] for i in range(case["n_images"])]
    pred = [npz[f"{case['name']}/pred_{i}"] for i in range(case["n_images"])]
    return gt, pred


def all_runs():
    _npz, meta = load_fixture()
    return [(c["name"], k) for c in meta["cases"] for k in range(len(c["runs"]))]


# ---- the restatement -----------------------------------------------------------------------------------------------
def _first_order(a):
    """non-zero values of a in order of first raster appearance, and their pixel counts"""
    v, first, cnt = np.unique(a.ravel(), return_index=True, return_counts=True)
    keep = v != 0
    v, first, cnt = v[keep], first[keep], cnt[keep]
    o = np.argsort(first, kind="stable")
    return v[o], cnt[o]


def _pair_counts(t, p):
    """{(t, p): pixels} over pixels where both are non-zero"""
    both = (t != 0) & (p != 0)
    key = t[both].astype(np.int64) * (1 << 32) + p[both].astype(np.int64)
    k, n = np.unique(key, return_counts=True)
    return {(int(a >> 32), int(a & 0xffffffff)): int(b) for a, b in zip(k, n)}


def _remove(ids, cls, gone):
    sel = np.isin(ids, list(gone)) & (ids != 0)
    return np.where(sel, 0, ids), np.where(sel, 0, cls)


def _border_ids(ids):
    b = np.unique(np.concatenate([ids[0], ids[-1], ids[:, 0], ids[:, -1]]))
    return set(b[b != 0].tolist())


def one_class_stats(t, p, match_iou):
    """tp, fp, fn, iou_sum of two one-class (or binary) instance maps, the reference's quirks included"""
    from scipy.optimize import linear_sum_assignment
    tv, ta = _first_order(t)
    pv, pa = _first_order(p)
    bg_t, bg_p = bool((t == 0).any()), bool((p == 0).any())
    trank = {int(v): i for i, v in enumerate(tv)}
    prank = {int(v): i for i, v in enumerate(pv)}
    cells = []                                           # (row, column, iou) of the reference's pairwise_iou matrix
    for (a, b), inter in _pair_counts(t, p).items():
        r, c = trank[a], prank[b]
        if not bg_t and r == 0:
            continue                                     # the first id of a map without background is skipped as "background"
        cells.append((r, c, inter / (int(ta[r]) + int(pa[c]) - inter)))
    cells.sort()
    listed_t = list(range(0 if bg_t else 1, len(tv)))
    listed_p = list(range(0 if bg_p else 1, len(pv)))
    if match_iou > 0.0:                                  # np.nonzero order = row-major
        cells = [x for x in cells if x[2] > match_iou]
        rows, cols = np.array([x[0] for x in cells], int), np.array([x[1] for x in cells], int)
        got = np.array([x[2] for x in cells], np.float64)
    else:
        m = np.zeros((len(tv) + bg_t, len(pv) + bg_p), np.float64)
        for r, c, v in cells:
            m[r, c] = v
        rows, cols = linear_sum_assignment(-m)
        got = m[rows, cols]
        keep = got > match_iou
        rows, cols, got = rows[keep], cols[keep], got[keep]
    fn = len(set(listed_t) - set(rows.tolist()))
    fp = len(set(listed_p) - set(cols.tolist()))
    return len(rows), fp, fn, float(got.sum())


def restate(gt, pred, nr_classes, match_iou, border, binary=False):
    """per-class [tp, fp, fn, iou_sum] of one image pair; gt / pred (H, W, 2), or (H, W) when binary"""
    if binary:
        t, p = np.asarray(gt).astype(np.int64), np.asarray(pred).astype(np.int64)
        ct, cp = np.ones_like(t), np.ones_like(p)
        nr_classes = 1
    else:
        t, ct = gt[..., 0].astype(np.int64), gt[..., 1].astype(np.int64)
        p, cp = pred[..., 0].astype(np.int64), pred[..., 1].astype(np.int64)
        # unlabelled true cells leave together with every prediction of class-agnostic IoU > 0.5
        tv, ta = _first_order(t)
        pv, pa = _first_order(p)
        area_t, area_p = dict(zip(tv.tolist(), ta.tolist())), dict(zip(pv.tolist(), pa.tolist()))
        labelled = set(np.unique(t[(ct > 0) & (t != 0)]).tolist())
        gone_t, gone_p = set(), set()
        for (a, b), inter in _pair_counts(t, p).items():
            if a not in labelled and inter / (area_t[a] + area_p[b] - inter) > 0.5:
                gone_t.add(a); gone_p.add(b)
        t, ct = _remove(t, ct, gone_t)
        p, cp = _remove(p, cp, gone_p)
    if border:
        t, ct = _remove(t, ct, _border_ids(t))
        p, cp = _remove(p, cp, _border_ids(p))
    return [list(one_class_stats(t * (ct == c), p * (cp == c), match_iou)) for c in range(1, nr_classes + 1)]


def lists_from_maps(gts, preds, nr_classes, border):
    """what ``cpx_pq_stats`` hands to the assignment branch, made on the host: (pairs, insts, nobg) of a batch"""
    pairs, insts, nobg = [], [], np.zeros((len(gts), 2), np.int32)
    for i, (gt, pred) in enumerate(zip(gts, preds)):
        t, ct = gt[..., 0].astype(np.int64), gt[..., 1].astype(np.int64)
        p, cp = pred[..., 0].astype(np.int64), pred[..., 1].astype(np.int64)
        assert not border
        for c in range(1, nr_classes + 1):
            tc, pc = t * (ct == c), p * (cp == c)
            first = []
            for s, a in enumerate((tc, pc)):
                v, f, n = np.unique(a.ravel(), return_index=True, return_counts=True)
                first.append({int(x): (int(y), int(z)) for x, y, z in zip(v, f, n) if x != 0})
                insts += [[i, s, c, y, z, 0] for (y, z) in first[-1].values()]
                if not (a == 0).any():
                    nobg[i, s] = c
            drop = None if (tc == 0).any() else int(tc.ravel()[0])
            for (a, b), inter in _pair_counts(tc, pc).items():
                if a != drop:
                    pairs.append([i, c, first[0][a][0], first[1][b][0], inter, first[0][a][1], first[1][b][1], 0])
    return np.array(pairs, np.int32).reshape(-1, 8), np.array(insts, np.int32).reshape(-1, 6), nobg


def close_sum(got, want, n):
    """|got - want| <= n * 2^-52 * want, exactly equal for n <= 1: every IoU is bitwise the reference's and non-negative, and two
    float64 summation orders of n such terms differ by at most 2 (n - 1) * 2^-53 * S"""
    return got == want if n <= 1 else abs(got - want) <= n * EPS52 * abs(want)


# ---- tests ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", all_runs())
def test_restatement_equals_the_reference(name, k):
    npz, meta = load_fixture()
    case = next(c for c in meta["cases"] if c["name"] == name)
    run = case["runs"][k]
    gt, pred = case_masks(npz, case)
    for i in range(case["n_images"]):
        st = restate(gt[i], pred[i], case["nr_classes"], run["match_iou"], run["border"])
        for c in range(case["nr_classes"]):
            assert st[c][:3] == [run["tp"][i][c], run["fp"][i][c], run["fn"][i][c]], (i, c, st[c])
            assert close_sum(st[c][3], run["iou_sum"][i][c], st[c][0]), (i, c, st[c][3], run["iou_sum"][i][c])
    if isinstance(run.get("binary_df"), dict):
        b = run["binary_df"]
        for i in range(case["n_images"]):
            tp, fp, fn, s = restate(gt[i][..., 0], pred[i][..., 0], 1, run["match_iou"], run["border"], binary=True)[0]
            assert [tp, fp, fn] == [b["tp"][i], b["fp"][i], b["fn"][i]], (i, tp, fp, fn)
            assert close_sum(s, b["iou_sum"][i], tp)


def _same_frame(df, gold):
    assert list(df.columns) == list(gold.keys())
    for col in df.columns:
        got, want = df[col].tolist(), gold[col]
        assert len(got) == len(want), col
        for g, w in zip(got, want):
            if isinstance(w, str):
                assert g == w, col
            else:
                assert (g == w) or (np.isnan(g) and np.isnan(w)), (col, g, w)
                assert isinstance(w, int) == isinstance(g, (int, np.integer)), (col, type(g), type(w))


@pytest.mark.parametrize("name,k", all_runs())
def test_table_assembly_equals_the_reference_frames(name, k):
    """golden statistics -> ``multiclass_tables`` / ``binary_table`` == the reference's DataFrames, value for value (NaN included)"""
    from classpose_amd.metrics import pq
    _npz, meta = load_fixture()
    case = next(c for c in meta["cases"] if c["name"] == name)
    run = case["runs"][k]
    gdf, idf = pq.multiclass_tables(run["tp"], run["fp"], run["fn"], run["iou_sum"])
    _same_frame(gdf, run["global_df"])
    _same_frame(idf, run["per_image_df"])
    b = run.get("binary_df")
    if isinstance(b, dict):
        _same_frame(pq.binary_table(b["tp"], b["fp"], b["fn"], b["iou_sum"]), b)
    elif b == "ZeroDivisionError":
        gt, pred = case_masks(_npz, case)
        st = [restate(g[..., 0], p[..., 0], 1, run["match_iou"], run["border"], binary=True)[0] for g, p in zip(gt, pred)]
        with pytest.raises(ZeroDivisionError):
            pq.binary_table(*(np.array([s[j] for s in st]) for j in range(4)))


def test_binary_table_raises_on_an_image_without_instances():
    from classpose_amd.metrics import pq
    _npz, meta = load_fixture()
    assert meta["binary_empty_raises"] is True
    with pytest.raises(ZeroDivisionError):
        pq.binary_table([0], [0], [0], [0.0])


def test_assignment_branch_from_pair_lists():
    """match_iou == 0: ``assignment_stats`` over (pairs, insts, nobg) lists == the reference's linear_sum_assignment results"""
    from classpose_amd.metrics import pq
    npz, meta = load_fixture()
    seen = 0
    for case in meta["cases"]:
        for run in case["runs"]:
            if run["match_iou"] != 0.0 or run["border"] or case["name"] == "unlabelled":
                continue
            gt, pred = case_masks(npz, case)
            if any(((g[..., 1] == 0) & (g[..., 0] > 0)).any() for g in gt):
                continue                                 # the filter is the device's (or restate's) job, not the list builder's
            pairs, insts, nobg = lists_from_maps(gt, pred, case["nr_classes"], False)
            rs = np.random.default_rng(0)
            tp, fp, fn, s = pq.assignment_stats(pairs[rs.permutation(len(pairs))], insts[rs.permutation(len(insts))], nobg,
                                                case["n_images"], case["nr_classes"])
            assert tp.tolist() == run["tp"] and fp.tolist() == run["fp"] and fn.tolist() == run["fn"], case["name"]
            for i in range(case["n_images"]):
                for c in range(case["nr_classes"]):
                    assert close_sum(s[i, c], run["iou_sum"][i][c], tp[i, c])
            seen += 1
    assert seen >= 3


def test_load_masks_and_coercion(tmp_path):
    from classpose_amd.metrics import check_and_coherce_if_necessary, load_masks
    a = np.arange(2 * 4 * 5 * 2).reshape(2, 4, 5, 2)
    np.save(tmp_path / "a.npy", a)
    np.savez(tmp_path / "b.npz", a[0])
    assert np.array_equal(load_masks(str(tmp_path / "a.npy")), a)
    assert np.array_equal(load_masks(str(tmp_path / "b.npz")), a[0])
    d = tmp_path / "dir"; d.mkdir()
    np.save(d / "2.npy", a[1]); np.savez(d / "1.npz", a[0]); (d / "x.txt").write_text("no")
    got = load_masks(str(d))
    assert isinstance(got, list) and len(got) == 2 and np.array_equal(got[0], a[0]) and np.array_equal(got[1], a[1])
    e = tmp_path / "empty"; e.mkdir()
    with pytest.raises(ValueError):
        load_masks(str(e))
    with pytest.raises(ValueError):
        load_masks(str(tmp_path / "a.tif"))
    assert check_and_coherce_if_necessary(a, 3) is a
    assert check_and_coherce_if_necessary(a[0], 3).shape == (1, 4, 5, 2)
    assert check_and_coherce_if_necessary(a[0, ..., 0], 2).shape == (1, 4, 5)
    lst = [a[0], a[1][:2]]
    assert check_and_coherce_if_necessary(lst, 3) is lst
    obj = np.empty(2, object); obj[0], obj[1] = lst
    out = check_and_coherce_if_necessary(obj, 3)
    assert isinstance(out, list) and out[1].shape == (2, 5, 2)
    with pytest.raises(ValueError):
        check_and_coherce_if_necessary(a, 2)


def test_cli_flags_and_label_map():
    from classpose_amd.entrypoints import calculate_metrics as cm
    a = cm.build_parser().parse_args(["--gt_path", "g", "--pred_path", "p"])
    assert (a.match_iou, a.output, a.binary, a.ignore_classes, a.label_map, a.no_border_instances, a.n_workers) == \
        (0.5, None, False, None, None, False, 1)
    a = cm.build_parser().parse_args("--gt_path g --pred_path p --match_iou 0.3 --output o.csv --binary --ignore_classes 2 5 "
                                     "--label_map 1=1 2=1 --no_border_instances --n_workers 4".split())
    assert (a.match_iou, a.output, a.binary, a.ignore_classes, a.label_map, a.no_border_instances, a.n_workers) == \
        (0.3, "o.csv", True, [2, 5], ["1=1", "2=1"], True, 4)
    mapping, values = cm.parse_label_map(["1=3", "2=3", "4=1"])
    assert mapping == {0: 0, 1: 3, 2: 3, 4: 1} and values.tolist() == [0, 3, 1]
    gt = np.zeros((1, 2, 3, 2), np.int64); pr = np.zeros((1, 2, 3, 2), np.int64)
    gt[0, ..., 1] = [[0, 1, 2], [3, 4, 1]]; pr[0, ..., 1] = [[0, 1, 2], [4, 4, 1]]
    g2, p2 = cm.apply_label_map(gt, pr, ["1=3", "2=3", "4=1"])
    assert g2[0, ..., 1].tolist() == [[0, 1, 0], [3, 0, 1]]          # true classes outside the map's VALUES {0, 3, 1} -> 0
    assert p2[0, ..., 1].tolist() == [[0, 3, 3], [1, 1, 3]]
    pr[0, 0, 0, 1] = 7
    with pytest.raises(ValueError):
        cm.apply_label_map(gt, pr, ["1=3"])


def test_value_ranges_are_checked_before_the_device_is_touched():
    from classpose_amd.metrics import pq
    with pytest.raises(ValueError):
        pq._channel(np.array([[-1, 2]]), "instance ids", 2 ** 31 - 1, np.int32)
    with pytest.raises(ValueError):
        pq._channel(np.array([[2 ** 31]]), "instance ids", 2 ** 31 - 1, np.int32)
    with pytest.raises(ValueError):
        pq._channel(np.array([[256]]), "classes", 255, np.uint8)
    with pytest.raises(ValueError):
        pq._channel(np.array([[0.5]]), "classes", 255, np.uint8)
    assert pq._channel(np.array([[3.0]]), "classes", 255, np.uint8).dtype == np.uint8
