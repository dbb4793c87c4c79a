"""The connected-component rule of csrc/cpx_components.hip (include/classpose_hip.h, r2) stated twice on the CPU, and the maps
the host and the device tests share.

The rule: 0 is background; two neighbouring pixels of the same non-zero value are connected (4: edge neighbours, 8: corner
neighbours too); a component's label is its 1-based rank among the components of its image by the raster index of its first pixel.

    label_scipy   per distinct non-zero value ``scipy.ndimage.label`` with the 4- or 8-structure, then an EXPLICIT renumbering by
                  the first raster index of every component (scipy's own order is not relied on).
    label_fill    pure Python: a breadth-first fill started at every unlabelled foreground pixel in raster order.
"""
from __future__ import annotations

import functools
from collections import deque

import numpy as np

from classpose_amd import ops

TILE = ops.COMPONENTS_TILE   # CC_TILE of csrc/cpx_components.hip (tests/test_components_host.py pins both on the source): the maps follow it
T = TILE


def label_scipy(m: np.ndarray, connectivity: int):
    """m (H, W) integers -> (labels int32 (H, W), count)."""
    from scipy import ndimage
    assert connectivity in (4, 8)
    structure = np.ones((3, 3), bool) if connectivity == 8 else np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    m = np.asarray(m)
    comp = np.zeros(m.shape, np.int64)
    total = 0
    for v in np.unique(m):
        if v == 0:
            continue
        lab, k = ndimage.label(m == v, structure=structure)
        comp[lab > 0] = lab[lab > 0] + total
        total += k
    flat = comp.ravel()
    fg = np.flatnonzero(flat)
    ids, first = np.unique(flat[fg], return_index=True)          # first: position in fg of each id's first pixel, fg is ascending
    assert len(ids) == total
    rank = np.zeros(total + 1, np.int64)
    rank[ids[np.argsort(fg[first], kind="stable")]] = np.arange(1, total + 1)
    return rank[comp].astype(np.int32), total


def label_fill(m: np.ndarray, connectivity: int):
    assert connectivity in (4, 8)
    m = np.asarray(m)
    H, W = m.shape
    val = m.ravel().tolist()
    out = [0] * (H * W)
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)] + ([(-1, -1), (-1, 1), (1, -1), (1, 1)] if connectivity == 8 else [])
    count = 0
    for p0 in range(H * W):
        v = val[p0]
        if v == 0 or out[p0]:
            continue
        count += 1
        out[p0] = count
        todo = deque([p0])
        while todo:
            p = todo.popleft()
            r, c = divmod(p, W)
            for dr, dc in steps:
                rr, cc = r + dr, c + dc
                if 0 <= rr < H and 0 <= cc < W:
                    q = rr * W + cc
                    if val[q] == v and not out[q]:
                        out[q] = count
                        todo.append(q)
    return np.asarray(out, np.int32).reshape(H, W), count


@functools.lru_cache(maxsize=None)
def expected(name: str, connectivity: int):
    """label_scipy of every image of CASES[name]: (labels (n, H, W) int32, counts (n,) int32); computed once, never modified."""
    maps = CASES[name]
    res = [label_scipy(m, connectivity) for m in maps]
    labels = np.stack([r[0] for r in res])
    counts = np.asarray([r[1] for r in res], np.int32)
    labels.setflags(write=False)
    counts.setflags(write=False)
    return labels, counts


# ---- the maps ----------------------------------------------------------------------------------------------------------------
def _random(shape, density, seed, nval=3):
    rng = np.random.default_rng(seed)
    m = rng.integers(1, nval + 1, shape).astype(np.int32)
    m[rng.random(shape) >= density] = 0
    return m


def _blobs(shape, seed, n_blobs, nval=3):
    """a few dozen overlapping discs of nval values: components larger than a pixel, some across tile seams"""
    rng = np.random.default_rng(seed)
    H, W = shape
    m = np.zeros(shape, np.int32)
    rows, cols = np.mgrid[:H, :W]
    for _ in range(n_blobs):
        cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(1, max(2, min(H, W, 40) // 2 + 1))
        m[(rows - cy) ** 2 + (cols - cx) ** 2 <= r * r] = rng.integers(1, nval + 1)
    return m


def serpentine(n: int) -> np.ndarray:
    """one-pixel-wide path over n x n (n odd): every even row whole, joined alternately at its right and left end"""
    m = np.zeros((n, n), np.int32)
    m[0::2] = 1
    for k, r in enumerate(range(1, n, 2)):
        m[r, n - 1 if k % 2 == 0 else 0] = 1
    return m


def spiral(n: int) -> np.ndarray:
    """square spiral inwards from the top-left corner, one pixel wide, one pixel of background between the turns"""
    m = np.zeros((n, n), np.int32)
    r = c = 0
    dr, dc = 0, 1
    m[0, 0] = 1
    while True:
        moved = False
        for _turn in range(2):
            while True:
                r2, c2 = r + dr, c + dc
                r3, c3 = r2 + dr, c2 + dc
                if not (0 <= r2 < n and 0 <= c2 < n) or m[r2, c2] or (0 <= r3 < n and 0 <= c3 < n and m[r3, c3]):
                    break
                r, c = r2, c2
                m[r, c] = 1
                moved = True
            dr, dc = dc, -dr                                      # right -> down -> left -> up
            if moved:
                break
        if not moved:
            return m


def _u_and_combs() -> np.ndarray:
    m = np.zeros((3 * T + 10, 3 * T + 20), np.int32)
    # a U open to the top: left prong in tile column 0, right prong in tile column 2 and HIGHER (it holds the first pixel, reached
    # only through the base), base in tile row 2
    m[20:2 * T + 30, 10] = 4
    m[5:2 * T + 30, 2 * T + 30] = 4
    m[2 * T + 30, 10:2 * T + 31] = 4
    # a comb inside the U, of another value: five prongs of rising height towards the right, base in tile row 1
    for k, x in enumerate(range(20, 2 * T + 20, 30)):
        m[T + 20 - 12 * (k + 1):T + 20, x] = 7
    m[T + 20, 20:2 * T + 20] = 7
    # a comb of the U's value below it: its prongs end one pixel short of the U's base (4-separate, 8-separate too)
    m[2 * T + 32:2 * T + 40, 12:2 * T + 28:4] = 4
    m[2 * T + 40, 12:2 * T + 28] = 4
    return m


def _touching() -> np.ndarray:
    m = np.zeros((T + 40, 2 * T + 12), np.int32)
    m[2:20, 30:T] = 3; m[2:20, T:100] = 5              # different values meeting on a tile seam: separate
    m[24:40, 30:T] = 3; m[24:40, T:100] = 3            # equal values: merged (and separate from the 3 above: a gap of 4 rows)
    m[44:60, 20:50] = -1; m[44:60, 50:90] = -100       # negatives are ordinary foreground
    m[T - 2:T + 2, 100:120] = -100                     # -100 again, elsewhere: its own component, across the row seam
    m[T + 5:T + 10, 5:10] = 9; m[T + 10:T + 15, 10:15] = 9        # corner contact of equal values: merged only 8-connected
    m[T + 5:T + 10, 30:35] = 9; m[T + 10:T + 15, 35:40] = 8       # corner contact of different values: never
    m[T + 20, :] = 2; m[T + 21, :] = 6                 # two full-width lines, touching
    return m


def _batch5() -> np.ndarray:
    H, W = 2 * T + 2, 2 * T + 22
    b = np.zeros((5, H, W), np.int32)
    b[1, 40:90, 50:120] = 2
    for k in range(7):
        b[2, 10 + 15 * k:18 + 15 * k, 5 + 20 * k:15 + 20 * k] = 1 + k % 2
    dots = np.zeros((H, W), np.int32)
    dots[0::2, 0::2] = 1
    idx = np.flatnonzero(dots.ravel())
    assert len(idx) >= 4000
    dots.ravel()[idx[4000:]] = 0
    b[3] = dots * 5
    b[4] = -3
    return b


def _diagonals() -> np.ndarray:
    n = 2 * T
    d = np.zeros((2, n, n), np.int32)
    i = np.arange(n)
    d[0, i, i] = 1                    # (T - 1, T - 1) -> (T, T): through the corner where four tiles meet
    d[1, i, n - 1 - i] = 2            # (T - 1, T) -> (T, T - 1): the other way through it
    return d


def _checker(H, W, a, b):
    r, c = np.mgrid[:H, :W]
    return np.where((r + c) % 2 == 0, a, b).astype(np.int32)


SIZES = [(1, 1), (1, 2 * T + 2), (2 * T + 2, 1), (T - 1, T - 1), (T, T), (T + 1, T + 1), (2 * T + 1, T + 3), (300, 520), (37, 100)]

CASES: dict[str, np.ndarray] = {}
for _k, (_h, _w) in enumerate(SIZES):
    CASES[f"size_{_h}x{_w}"] = np.stack([_random((_h, _w), 0.6, 100 + _k), _blobs((_h, _w), 200 + _k, 30)])
CASES["size_1x1_background"] = np.zeros((1, 1, 1), np.int32)
CASES["all_background"] = np.zeros((1, T + 6, T + 6), np.int32)
CASES["all_one_value"] = np.full((1, 2 * T + 2, 2 * T + 2), 3, np.int32)
CASES["all_distinct"] = (np.arange((T + 1) * (T + 3), dtype=np.int32).reshape(1, T + 1, T + 3) + 1)
CASES["checker_one_value"] = _checker(T + 1, T + 3, 1, 0)[None]
CASES["checker_two_values"] = _checker(T + 1, T + 3, 1, 2)[None]
CASES["u_and_combs"] = _u_and_combs()[None]
CASES["serpentine_257"] = serpentine(257)[None]
CASES["spiral_257"] = spiral(257)[None]
CASES["diagonals"] = _diagonals()
CASES["touching"] = _touching()[None]
CASES["batch5"] = _batch5()
for _d in (3, 5, 7):
    CASES[f"random_density_0{_d}"] = _random((8, 200, 333), _d / 10, 40 + _d)
for _m in CASES.values():
    assert _m.dtype == np.int32 and _m.ndim == 3
    _m.setflags(write=False)

# counts that follow from the construction, whatever a labeller says: {name: {connectivity: per-image counts}}
KNOWN_COUNTS = {
    "size_1x1_background": {4: [0], 8: [0]},
    "all_background": {4: [0], 8: [0]},
    "all_one_value": {4: [1], 8: [1]},
    "all_distinct": {4: [(T + 1) * (T + 3)], 8: [(T + 1) * (T + 3)]},
    "checker_one_value": {4: [((T + 1) * (T + 3) + 1) // 2], 8: [1]},
    "checker_two_values": {4: [(T + 1) * (T + 3)], 8: [2]},
    "serpentine_257": {4: [1], 8: [1]},
    "spiral_257": {4: [1], 8: [1]},
    "diagonals": {4: [2 * T, 2 * T], 8: [1, 1]},
    "batch5": {4: [0, 1, 7, 4000, 1], 8: [0, 1, 7, 4000, 1]},
    "u_and_combs": {4: [3], 8: [3]},
}


def cell_field(seed: int, size: int, n_cells: int):
    """rings for ops.rasterize_polygons: n_cells octagons of radius 4..11 at random centres -> (xy, ring_off, ring_value)"""
    rng = np.random.default_rng(seed)
    ang = np.arange(8) * (2 * np.pi / 8)
    xy, off, val = [], [0], []
    for k in range(n_cells):
        cx, cy, r = rng.uniform(0, size), rng.uniform(0, size), rng.uniform(4, 11)
        ring = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang)], 1)
        xy.append(np.round(ring * 16) / 16)
        off.append(off[-1] + 8)
        val.append(k + 1)
    return np.concatenate(xy).astype(np.float64), np.asarray(off, np.int64), np.asarray(val, np.int32)


def instance_counts_relabelled(instances: np.ndarray, classes: np.ndarray, n_classes: int, connectivity: int = 8) -> np.ndarray:
    """get_instance_counts(label_instances=True) of the reference (train_utils.py:407-436) with label_scipy in place of
    skimage.measure.label: per image ``np.unique(label(instances)[classes == j]).size``."""
    out = np.zeros((len(instances), n_classes), np.float64)
    for i, (inst, cls) in enumerate(zip(instances, classes)):
        lab = label_scipy(inst, connectivity)[0]
        for j in range(n_classes):
            out[i, j] = np.unique(lab[cls == j]).size
    return out
