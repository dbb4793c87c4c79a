"""Per-cell class confidence: the host side of ``cpx_instance_confidence`` (include/classpose_hip.h has the definitions).

The device hands back, per cell, the vote table ``votes[c]`` (pixels whose arg-max class is c), ``prob_q[c]`` (the sum over
the cell's pixels of the softmax probability of class c, each quantised to 2^-24) and ``cellprob_q`` (the same sum for the
sigmoid of cellprob).  With n = sum_c votes[c], the cell's pixel count, and cls the cell's class-map value:

    class_vote_fraction   = votes[cls] / n
    class_probability     = prob_q[cls] / (n * 2^24)
    detection_probability = cellprob_q / (n * 2^24)
    probability: <label>  = prob_q[c] / (n * 2^24)   for every class value c (mode "full")

all in float64.  The reference has no such output (its cells carry one hard class name); HoVer-Net and CellViT write the
first of these as ``type_prob``.  Pure numpy: nothing here touches the device.
"""
from __future__ import annotations

import numpy as np

Q = float(1 << 24)
MODES = ("summary", "full")
SUMMARY_NAMES = ("class_vote_fraction", "class_probability", "detection_probability")


def row_width(ncls: int) -> int:
    """uint64 words of one cell's confidence row: votes[ncls], prob_q[ncls], cellprob_q, area (see ``pack_rows``)"""
    return 2 * max(int(ncls), 0) + 2


def _table(a, m: int) -> np.ndarray:
    """a as [m][k] (k from its last axis when it has two: ``reshape(m, -1)`` cannot tell k when m == 0)"""
    a = np.asarray(a)
    return a.reshape(m, a.shape[-1] if a.ndim >= 2 else (a.size // m if m else 0))


def pack_rows(votes, prob_q, cellprob_q, area) -> np.ndarray:
    """One uint64 row per cell, [votes | prob_q | cellprob_q | area]: what travels beside the cell table through the tile
    loop's ordering, exchange and filters.  votes / prob_q [n][ncls] (ncls may be 0: no class head)."""
    votes = _table(votes, len(cellprob_q))
    prob_q = _table(prob_q, len(cellprob_q))
    out = np.zeros((len(votes), row_width(votes.shape[1])), np.uint64)
    k = votes.shape[1]
    out[:, :k] = votes.astype(np.uint64)
    out[:, k:2 * k] = prob_q.astype(np.uint64)
    out[:, 2 * k] = np.asarray(cellprob_q).astype(np.uint64)
    out[:, 2 * k + 1] = np.asarray(area).astype(np.uint64)
    return out


def unpack_rows(rows: np.ndarray):
    """(votes int64 [n][ncls], prob_q uint64 [n][ncls], cellprob_q uint64 [n], area int64 [n]) of ``pack_rows`` rows"""
    rows = np.asarray(rows, dtype=np.uint64)
    k = (rows.shape[1] - 2) // 2
    return rows[:, :k].astype(np.int64), rows[:, k:2 * k], rows[:, 2 * k], rows[:, 2 * k + 1].astype(np.int64)


def class_label(labels, c: int) -> str:
    """the label of class-map value c: ``labels[c - 1]`` with Python's negative index for 0, like ``geojson.cell_dict``"""
    return str(labels[int(c) - 1])


def measurements(votes, prob_q, cellprob_q, cls, mode: str = "summary", labels=None, area=None):
    """Names and values of the confidence measurements of n cells -> (names, float64 [n][len(names)]).

    votes [n][ncls] integer, prob_q [n][ncls] and cellprob_q [n] uint64 as ``cpx_instance_confidence`` wrote them, cls [n]
    the cells' class-map values.  ``mode`` "summary": class_vote_fraction, class_probability, detection_probability;
    "full": those, then ``probability: <label>`` for every class value 0 .. ncls-1 (``labels[c - 1]``; without labels the
    value itself).  Without a class head (votes None or with no columns) the one measurement is detection_probability in
    either mode, and ``area`` [n] gives the pixel counts that the vote table otherwise does.  cellprob_q None: no
    detection_probability.  A cell without pixels (n == 0) gets NaN."""
    if mode not in MODES:
        raise ValueError(f"cell confidence mode {mode!r}: expected one of {MODES}")
    has_cls = votes is not None and np.asarray(votes).ndim == 2 and np.asarray(votes).shape[1] > 0
    if has_cls:
        votes = np.asarray(votes).astype(np.int64)
        m, ncls = votes.shape
        n_px = votes.sum(1).astype(np.float64)
    else:
        if area is None:
            raise ValueError("confidence.measurements: without a vote table the pixel counts come from area=")
        n_px = np.asarray(area).astype(np.float64).reshape(-1)
        m, ncls = len(n_px), 0
    names: list[str] = []
    cols: list[np.ndarray] = []
    with np.errstate(divide="ignore", invalid="ignore"):
        den = n_px * Q
        if has_cls:
            cls = np.asarray(cls).astype(np.int64).reshape(m)
            if m and (cls.min() < 0 or cls.max() >= ncls):
                raise ValueError(f"confidence.measurements: class values outside 0 .. {ncls - 1}")
            pq = np.asarray(prob_q).astype(np.uint64).reshape(m, ncls).astype(np.float64)       # < 2^44: exact
            r = np.arange(m)
            names += ["class_vote_fraction", "class_probability"]
            cols += [votes[r, cls].astype(np.float64) / n_px, pq[r, cls] / den]
        if cellprob_q is not None:
            names.append("detection_probability")
            cols.append(np.asarray(cellprob_q).astype(np.uint64).reshape(m).astype(np.float64) / den)
        if has_cls and mode == "full":
            for c in range(ncls):
                names.append("probability: " + (class_label(labels, c) if labels is not None else str(c)))
                cols.append(pq[:, c] / den)
    vals = np.stack(cols, 1) if cols else np.zeros((m, 0))
    return names, np.ascontiguousarray(vals, dtype=np.float64)


STATS_FIELDS = ("label", "cls", "area", "votes", "prob", "detection")


def stats_dtype(ncls: int) -> np.dtype:
    """one row per cell of ``ClassposeModel.eval(cell_confidence=True)``"""
    k = max(int(ncls), 0)
    return np.dtype([("label", "<i4"), ("cls", "<i4"), ("area", "<i8"), ("votes", "<i8", (k,)), ("prob", "<f8", (k,)),
                     ("detection", "<f8")])


def stats_table(label, cls, area, votes, prob_q, cellprob_q) -> np.ndarray:
    """The structured per-cell table of ``eval``: ``prob`` = prob_q / (area * 2^24), ``detection`` = cellprob_q / (area * 2^24)"""
    area = np.asarray(area).astype(np.int64).reshape(-1)
    m = len(area)
    votes = np.zeros((m, 0), np.int64) if votes is None else _table(votes, m)
    out = np.zeros(m, stats_dtype(votes.shape[1]))
    out["label"], out["cls"], out["area"] = label, cls, area
    with np.errstate(divide="ignore", invalid="ignore"):
        den = area.astype(np.float64) * Q
        if votes.shape[1]:
            out["votes"] = votes
            out["prob"] = _table(prob_q, m).astype(np.uint64).astype(np.float64) / den[:, None]
        out["detection"] = np.asarray(cellprob_q).astype(np.uint64).reshape(m).astype(np.float64) / den
    return out
