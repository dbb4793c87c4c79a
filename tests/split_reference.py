"""The rule of csrc/cpx_split.hip (include/classpose_hip.h, r3) restated on the CPU in integers, and the maps the host and the
device tests share.

    distance_sq   a. per pixel of value v != 0 the squared distance to the nearest pixel of another value (0 included), by the
                  separable form: the vertical distances g of every column, then inside every horizontal run of equal value the
                  minimum of (x - x')^2 + g(x', y)^2 over the run, capped by the first pixel past either run end.  H*H + W*W where
                  the image holds no other value, 0 on background.
    seed_list     b. p is a seed when D2[p] >= min_radius^2 and no pixel of its instance in the (2 * min_distance + 1)^2 window
                  has a larger D2, or an equal D2 and an earlier raster index.  Listed by (instance id, raster index).
    provisional   c. instances with fewer than two seeds stay whole; otherwise every pixel takes the seed of its instance with the
                  smallest squared distance, the first of equals in list order (raster order).
    split         d. ``components_reference.label_scipy`` of the provisional map.

``distance_sq_brute`` states a. once more without the separable form (every pixel against every site).
"""
from __future__ import annotations

import functools

import numpy as np

import components_reference as cr

NONE = np.iinfo(np.int64).max


def column_distance(m: np.ndarray) -> np.ndarray:
    """g (H, W) int64: the vertical distance to the nearest pixel of another value in the same column, NONE where there is none"""
    H, W = m.shape
    up = np.full((H, W), NONE, np.int64)
    down = np.full((H, W), NONE, np.int64)
    for y in range(1, H):
        same = m[y] == m[y - 1]
        up[y] = np.where(same, np.where(up[y - 1] == NONE, NONE, up[y - 1] + 1), 1)
    for y in range(H - 2, -1, -1):
        same = m[y] == m[y + 1]
        down[y] = np.where(same, np.where(down[y + 1] == NONE, NONE, down[y + 1] + 1), 1)
    return np.minimum(up, down)


def distance_sq(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m)
    H, W = m.shape
    g = column_distance(m)
    g2 = np.where(g == NONE, NONE, g * g)
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        row = m[y]
        starts = np.flatnonzero(np.r_[True, row[1:] != row[:-1]])
        ends = np.r_[starts[1:], W]
        for x0, x1 in zip(starts.tolist(), ends.tolist()):                   # the run is x0 .. x1 - 1
            if row[x0] == 0:
                continue
            xs = np.arange(x0, x1)
            dx2 = (xs[:, None] - xs[None, :]) ** 2
            cand = np.where(g2[y, x0:x1][None, :] == NONE, NONE, dx2 + np.where(g2[y, x0:x1] == NONE, 0, g2[y, x0:x1])[None, :])
            best = cand.min(1)
            if x0 > 0:
                best = np.minimum(best, (xs - (x0 - 1)) ** 2)
            if x1 < W:
                best = np.minimum(best, (x1 - xs) ** 2)
            out[y, x0:x1] = np.where(best == NONE, H * H + W * W, best)
    return out.astype(np.int32)


def distance_sq_brute(m: np.ndarray) -> np.ndarray:
    m = np.asarray(m)
    H, W = m.shape
    ys, xs = np.mgrid[:H, :W]
    out = np.zeros((H, W), np.int64)
    for v in np.unique(m):
        if v == 0:
            continue
        sy, sx = np.nonzero(m != v)
        py, px = np.nonzero(m == v)
        if len(sy) == 0:
            out[py, px] = H * H + W * W
            continue
        d = (py[:, None] - sy[None, :]) ** 2 + (px[:, None] - sx[None, :]) ** 2
        out[py, px] = d.min(1)
    return out.astype(np.int32)


def seed_list(m: np.ndarray, d2: np.ndarray, min_distance: int, min_radius: int) -> np.ndarray:
    """raster indices of the seeds, ordered by (instance id, raster index); int32"""
    m = np.asarray(m)
    H, W = m.shape
    idx = np.arange(H * W).reshape(H, W)
    found = []
    for y, x in np.argwhere((m != 0) & (d2 >= min_radius * min_radius)).tolist():
        y0, y1, x0, x1 = max(0, y - min_distance), min(H, y + min_distance + 1), max(0, x - min_distance), min(W, x + min_distance + 1)
        same = m[y0:y1, x0:x1] == m[y, x]
        dw, c, p = d2[y0:y1, x0:x1], d2[y, x], idx[y, x]
        if not (same & ((dw > c) | ((dw == c) & (idx[y0:y1, x0:x1] < p)))).any():
            found.append((int(m[y, x]), int(p)))
    return np.asarray([p for _v, p in sorted(found)], np.int32)


def provisional(m: np.ndarray, seeds: np.ndarray) -> np.ndarray:
    """int64 (H, W): 1 + the seed's place in the list on split instances, len(seeds) + id on the others, 0 on background"""
    m = np.asarray(m)
    H, W = m.shape
    out = np.where(m != 0, len(seeds) + m.astype(np.int64), 0)
    ids = m.ravel()[seeds]
    for v in np.unique(ids):
        mine = np.flatnonzero(ids == v)                                      # consecutive places, raster order
        if len(mine) < 2:
            continue
        py, px = np.nonzero(m == v)
        sy, sx = np.divmod(seeds[mine].astype(np.int64), W)
        d = (py[:, None] - sy[None, :]) ** 2 + (px[:, None] - sx[None, :]) ** 2
        out[py, px] = 1 + mine[np.argmin(d, axis=1)]                         # argmin: the first of equals
    return out


def partition_id(a: np.ndarray) -> np.ndarray:
    """the map renumbered by first raster appearance (0 stays 0): equal for two maps exactly when their partitions are equal"""
    flat = np.asarray(a).ravel()
    vals, first = np.unique(flat, return_index=True)
    order = [v for v in vals[np.argsort(first)] if v != 0]
    lut = {0: 0, **{v: k + 1 for k, v in enumerate(order)}}
    return np.asarray([lut[v] for v in flat.tolist()], np.int64).reshape(np.asarray(a).shape)


def split_image(m: np.ndarray, min_distance: int = 5, min_radius: int = 2, connectivity: int = 8):
    """one (H, W) instance map -> (labels int32 (H, W), count, seeds int32, d2 int32)"""
    d2 = distance_sq(m)
    seeds = seed_list(m, d2, min_distance, min_radius)
    labels, count = cr.label_scipy(provisional(m, seeds), connectivity)
    return labels, count, seeds, d2


@functools.lru_cache(maxsize=None)
def expected(name: str, min_distance: int = 5, min_radius: int = 2, connectivity: int = 8):
    """split_image of every image of CASES[name], computed once and never modified:
    (labels (n, H, W) int32, counts (n,) int32, [seeds of image k], d2 (n, H, W) int32)"""
    res = [split_image(m, min_distance, min_radius, connectivity) for m in CASES[name]]
    labels, d2 = np.stack([r[0] for r in res]), np.stack([r[3] for r in res])
    counts = np.asarray([r[1] for r in res], np.int32)
    for a in (labels, d2, counts):
        a.setflags(write=False)
    return labels, counts, [r[2] for r in res], d2


# ---- the maps ----------------------------------------------------------------------------------------------------------------
def disc(m: np.ndarray, cy: int, cx: int, r: int, v: int = 1, ry: int | None = None) -> None:
    """pixels with (dx / r)^2 + (dy / ry)^2 <= 1 take v (integers: dx^2 * ry^2 + dy^2 * r^2 <= r^2 * ry^2)"""
    ry = r if ry is None else ry
    ys, xs = np.mgrid[:m.shape[0], :m.shape[1]]
    m[(xs - cx) ** 2 * ry * ry + (ys - cy) ** 2 * r * r <= r * r * ry * ry] = v


def touching_regions(shape, seed: int) -> np.ndarray:
    """what cpx_label_components makes of a class map of overlapping discs: neighbouring ids without background between them"""
    return cr.label_scipy(cr._blobs(shape, seed, 12 + shape[0] * shape[1] // 600, nval=3), 4)[0]


def beads(shape) -> np.ndarray:
    """ONE instance with a peak of D2 = 2 every four pixels along bars six rows apart: far more seeds than a wave is wide at
    min_distance 1, min_radius 1, in one list that runs over every row and column seam"""
    H, W = shape
    ys, xs = np.mgrid[:H, :W]
    return (((ys % 6 == 2) | ((ys % 6 != 5) & (xs % 4 == 0)) | (xs == 0)) & (ys < H)).astype(np.int32)


def sized(shape, seed: int) -> np.ndarray:
    """three images of different content: touching regions, one instance that fills the image, the beads"""
    return np.stack([touching_regions(shape, seed), np.ones(shape, np.int32), beads(shape)])


def two_discs(H=48, W=60, cy=24, cx=23, gap=14, r=10) -> np.ndarray:
    m = np.zeros((H, W), np.int32)
    disc(m, cy, cx, r)
    disc(m, cy, cx + gap, r)
    return m


def ellipse() -> np.ndarray:
    m = np.zeros((30, 44), np.int32)
    disc(m, 14, 21, 16, ry=8)
    return m


def disc_grid(pitch=20, r=10, k=3, margin=13) -> np.ndarray:
    side = 2 * margin + pitch * (k - 1) + 1
    m = np.zeros((side, side), np.int32)
    for i in range(k):
        for j in range(k):
            disc(m, margin + pitch * i, margin + pitch * j, r)
    return m


def thin() -> np.ndarray:
    """an L of two-pixel strokes and a bar three pixels high: D2 <= 2 on the L, so it has no seed at min_radius 2; the bar's middle
    row has D2 = 4 everywhere, one plateau longer than any window"""
    m = np.zeros((40, 90), np.int32)
    m[3:5, 3:80] = 1
    m[3:30, 3:5] = 1
    m[33:36, 2:88] = 2
    return m


def twin_peaks(vertical: bool = False) -> np.ndarray:
    """two discs of radius 4 with centres 4 apart: mirror-symmetric, both centres inside one window.  The pair sits on both sides of
    pixel 64 of the axis the centres lie on."""
    m = np.zeros((20, 80), np.int32)
    disc(m, 9, 62, 4)
    disc(m, 9, 66, 4)
    return np.ascontiguousarray(m.T) if vertical else m


def seams() -> np.ndarray:
    """130 x 140, every structure on a 64-pixel seam: two discs cut at x = 64 (ids 1), the twin peaks across x = 64 and y = 64, a disc
    in the corner whose window the border clips, two regions of different ids that share an edge along a seam, and the thin L"""
    m = np.zeros((130, 140), np.int32)
    disc(m, 30, 57, 10, 1); disc(m, 30, 71, 10, 1)
    disc(m, 60, 20, 4, 2); disc(m, 64, 20, 4, 2)                     # centres on rows 60 and 64: the same column, equal D2
    disc(m, 100, 62, 4, 3); disc(m, 100, 66, 4, 3)
    disc(m, 3, 3, 6, 4)
    m[60:70, 100:128] = 5
    m[70:80, 100:128] = 6                                           # no background between 5 and 6
    m[60:80, 128:136] = 7                                           # ... nor between them and 7, which starts on column 128
    m[110:112, 30:120] = 8
    m[112:128, 30:32] = 8
    return m


SIZES = [(1, 1), (1, 70), (70, 1), (63, 65), (65, 67), (130, 70)]
CASES = {f"size_{h}x{w}": sized((h, w), 40 + k) for k, (h, w) in enumerate(SIZES)}
CASES.update({
    "two_discs": two_discs()[None], "ellipse": ellipse()[None], "disc_grid": disc_grid()[None], "thin": thin()[None],
    "twin_peaks": twin_peaks()[None], "twin_peaks_vertical": twin_peaks(True)[None], "seams": seams()[None],
    "single_130x70": touching_regions((130, 70), 45)[None],
})
for _m in CASES.values():
    _m.setflags(write=False)
PARAMETERS = [(5, 2), (1, 1), (9, 2)]                  # (min_distance, min_radius): the defaults, the smallest window, a wide one
