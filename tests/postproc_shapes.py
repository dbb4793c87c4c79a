"""Hand-built inputs for the post-processing stages behind the Euler loop (csrc/cpx_postproc.hip): convergence maps for
get_masks, instance maps for the centre pick / diffusion / flow error, logits for the class vote.  Test infrastructure:
nothing here calls the code under test, and tests/test_postproc_shapes_host.py proves every premise a case is named for on
the CPU, with the oracle alone.

A convergence case is ``(H, W, p_final, pt, inds)``: ``p_final`` the packed int32 map ``ops.get_masks`` reads
(``(y << 16) | (x & 0xFFFF)``, -1 = inactive pixel), ``(pt, inds)`` what ``oracle.dynamics.get_masks`` reads.  ``EXPECT`` holds
what each case must give, derived by hand from the rules of get_masks (a sink with more than 10 pixels that is the maximum
of its 5 x 5 window is a seed; seeds are ranked by (count, raster index); a seed grows by five 3 x 3 dilations through
cells with more than 2 pixels inside its 11 x 11 window; where two windows overlap the later rank wins)."""
from __future__ import annotations

import numpy as np
import torch

# ---- the constants of the kernels, restated (the host test asserts them against the source) -----------
LH_SLOTS, LH_PROBES = 256, 8                # the per-workgroup LDS label hash: slots, probes before an update goes to global memory
STATS_WG = 2048                             # pixels per workgroup of the label-run passes (256 threads x 8 pixels)
DIFF_SMALL_CELLS = 2048                     # padded box up to this: first diffusion launch (256 threads)
DIFF_BIG_CELLS = 8192                       # ... up to this: second launch, two planes in LDS
DIFF_HUGE_CELLS = 18 * 1024 - 96            # ... up to this: second launch, one plane in LDS; above: the global planes
DIFF_SMALL_GRID = 128                       # workgroups per tile of the first launch (at most L - 1)


def max_labels(H, W):
    return H * W // 11 + 2


def diffuse_big_grid(nT, L):
    """workgroups per tile of the second diffusion launch = the stride of the ids one workgroup runs"""
    per_tile = 32 if nT >= 8 else (128 if nT <= 2 else 256 // nT)
    return min(L - 1, per_tile)


def diffusion_path(cells):
    """0 .. 3: first launch / two planes / one plane / global planes"""
    return int(cells > DIFF_SMALL_CELLS) + int(cells > DIFF_BIG_CELLS) + int(cells > DIFF_HUGE_CELLS)


def _home(key):
    return ((int(key) * 2654435761) & 0xFFFFFFFF) >> 24


def _guaranteed_misses(keys):
    """the largest, over the windows [s, s + k) of home slots, of #keys in the window - (k + 7): a lower bound of the
    updates that find no slot"""
    per_slot = np.bincount([_home(k) for k in set(int(k) for k in keys)], minlength=LH_SLOTS)
    below = np.concatenate([[0], np.cumsum(per_slot)])
    return max(int(below[s + k] - below[s]) - (k + LH_PROBES - 1) for s in range(LH_SLOTS) for k in range(1, LH_SLOTS - s + 1))


def crowd_ids(n_ids, lo=99, k=61):
    """the ids of 1 .. n_ids - 1 whose home slots lie in [lo, lo + k): 91 of the 373 a 64 x 64 tile can hold"""
    return [l for l in range(1, n_ids) if lo <= _home(l) < lo + k]


# ---- convergence maps ------------------------------------------------------------------------------------------------
def pack_p_final(H, W, sinks):
    """sinks: [((sy, sx), pixels)], pixels = flat raster indices of the pixels that end at (sy, sx).
    -> (p_final int32 (H * W,), pt int32 tensor (2, N), inds (y, x)) with the active pixels in raster order."""
    p = np.full(H * W, -1, np.int32)
    for (sy, sx), px in sinks:
        assert 0 <= sy < H and 0 <= sx < W, "sinks stay inside the tile, as follow_flows guarantees"
        px = np.asarray(px, np.int64)
        assert px.size == 0 or (px.min() >= 0 and px.max() < H * W and np.all(p[px] == -1)), "every pixel has one sink"
        p[px] = (sy << 16) | (sx & 0xFFFF)
    act = np.flatnonzero(p != -1)
    pt = torch.from_numpy(np.stack([p[act] >> 16, p[act] & 0xFFFF]).astype(np.int32))
    return p, pt, (act // W, act % W)


def _case(H, W, counted, seed):
    """counted: [((sy, sx), n)]; the pixels are dealt from a seeded permutation of the tile, so that a label's pixels lie
    anywhere and the order of first appearance (the renumbering) is not the order of the list"""
    order = np.random.default_rng(seed).permutation(H * W)
    total = sum(n for _, n in counted)
    assert total <= H * W
    sinks, at = [], 0
    for pos, n in counted:
        sinks.append((pos, order[at:at + n]))
        at += n
    return (H, W) + pack_p_final(H, W, sinks)


def thresholds():
    c = [((10, 10), 10), ((10, 30), 11),                                       # 10: no seed; 11: a seed
         ((30, 30), 15), ((30, 31), 3), ((29, 30), 3), ((30, 29), 2), ((31, 30), 2),
         ((32, 30), 3)]                                                        # behind the 2-cell (31, 30); (31, 29) and (31, 31) are empty
    return _case(64, 64, c, 1)


def reach():
    chain = [(30, 11), (30, 12), (30, 13), (30, 14), (29, 15), (28, 14), (28, 13)]      # steps 1 .. 7 from the seed, all within 5 of it
    return _case(64, 64, [((30, 10), 15)] + [(p, 3) for p in chain], 2)


def ties():
    row = [((20, 18), 12), ((20, 10), 12), ((20, 14), 12)] + [((20, x), 3) for x in (11, 12, 13, 15, 16, 17)]
    col = [((46, 30), 12), ((43, 30), 12), ((40, 30), 12)] + [((y, 30), 3) for y in (41, 42, 44, 45)]
    return _case(64, 64, row + col, 3)


def plateau():
    return _case(64, 64, [((10, 10), 11), ((30, 31), 12), ((30, 30), 12)], 4)


def overlap():
    a = [((20, 10), 20), ((20, 14), 13)] + [((20, x), 3) for x in (11, 12, 13, 15, 16)]
    b = [((40, 40), 14), ((46, 40), 21)] + [((y, 40), 3) for y in (41, 42, 43, 44, 45)]
    return _case(64, 64, a + b, 5)


def corners():
    H, W = 40, 56
    c = []
    for (y, x), (iy, ix) in (((0, 0), (1, 1)), ((0, W - 1), (1, W - 2)), ((H - 1, 0), (H - 2, 1)), ((H - 1, W - 1), (H - 2, W - 2)),
                             ((0, 27), (1, 27)), ((H - 1, 30), (H - 2, 29)), ((17, 0), (18, 1)), ((22, W - 1), (21, W - 2))):
        c += [((y, x), 12), ((iy, ix), 3)]
    return _case(H, W, c, 6)


def fraction(n):
    """a 50 x 50 tile with one sink of n pixels (1000 = H * W * 0.4 exactly: kept; 1001: removed) and a seed of 12"""
    return _case(50, 50, [((25, 25), n), ((5, 5), 12)], 7)


def many_seeds():
    """128 x 128: a 21 x 21 grid of 11-pixel sinks, 6 apart, and five 3-pixel cells between row neighbours: 441 tied seeds
    (more than the 256 one pass of the seed grid takes, seven 64-seed ballots), each of which takes the five cells on its left
    from its left neighbour only if its rank is the later one"""
    c = []
    for i in range(21):
        for j in range(21):
            c.append(((3 + 6 * i, 3 + 6 * j), 11))
            if j:
                c += [((3 + 6 * i, 3 + 6 * j - d), 3) for d in range(1, 6)]
    return _case(128, 128, c, 8)


def crowd():
    """64 x 64: 372 tied 11-pixel sinks on every other cell, so seed k in raster order gets label k; the pixels of the labels
    whose hash slots crowd one window come first, all inside the first workgroup's 2048 pixels"""
    H = W = 64
    n = 372
    pos = [(2 * (k // 32), 2 * (k % 32)) for k in range(n)]
    first = crowd_ids(n + 1)
    rest = [l for l in range(1, n + 1) if l not in first]
    assert 11 * len(first) <= STATS_WG // 2
    sinks, at = [], 0
    for l in first + rest:                                  # 11 consecutive pixels each: one or two row runs
        sinks.append((pos[l - 1], np.arange(at, at + 11)))
        at += 11
    return (H, W) + pack_p_final(H, W, sinks)


def crowd_labels_of_first_workgroup():
    """the seed-rank labels (before the renumbering) among the first 2048 pixels of `crowd`"""
    n = 372
    first = crowd_ids(n + 1)
    rest = [l for l in range(1, n + 1) if l not in first]
    return (first + rest)[:-(-STATS_WG // 11)]


# name -> (case, number of labels, sorted pixel counts of the labels, pixels left 0)
EXPECT = {
    "thresholds": (thresholds, 2, [11, 21], 10 + 2 + 2 + 3),
    "reach": (reach, 1, [15 + 5 * 3], 6),
    "ties": (ties, 4, [12, 18, 36, 36], 0),
    "plateau": (plateau, 2, [11, 24], 0),
    "overlap": (overlap, 4, [3, 14, 36, 45], 0),
    "corners": (corners, 8, [15] * 8, 0),
    "fraction_1000": (lambda: fraction(1000), 2, [12, 1000], 0),
    "fraction_1001": (lambda: fraction(1001), 1, [12], 1001),
    "many_seeds": (many_seeds, 441, [11] * 21 + [26] * 420, 0),
    "crowd": (crowd, 372, [11] * 372, 0),
}


# ---- instance maps ---------------------------------------------------------------------------------------------------
def _disc(m, cy, cx, r, lab):
    y, x = np.ogrid[:m.shape[0], :m.shape[1]]
    m[(y - cy) ** 2 + (x - cx) ** 2 <= r * r] = lab


def touching():
    """a smooth blob cut by the level sets of a second smooth field: irregular labels that share edges"""
    from scipy import ndimage
    rng = np.random.default_rng(5)
    a = ndimage.gaussian_filter(rng.standard_normal((72, 80)), 7)
    b = ndimage.gaussian_filter(rng.standard_normal((72, 80)), 5)
    blob = a > np.quantile(a, 0.45)
    blob[[0, -1]] = False
    blob[:, [0, -1]] = False
    cut = np.digitize(b, np.quantile(b[blob], [0.2, 0.4, 0.6, 0.8]))
    lab, n = ndimage.label(blob)
    m = np.zeros(a.shape, np.int32)
    nxt = 1
    for comp in range(1, n + 1):
        for lev in range(5):
            sel = (lab == comp) & (cut == lev)
            if sel.any():
                m[sel] = nxt
                nxt += 1
    return m


def concave():
    m = np.zeros((64, 80), np.int32)
    m[4:24, 4:24] = 1                                   # a C open to the right
    m[7:21, 7:24] = 0
    _disc(m, 44, 16, 12, 2)                             # a ring
    _disc(m, 44, 16, 8, 0)
    m[4:28, 40:43] = 3                                  # an L
    m[25:28, 40:64] = 3
    return m


def even_ties():
    m = np.zeros((48, 64), np.int32)
    m[2:4, 2:4] = 1
    m[2:6, 8:12] = 2
    m[2:4, 16:22] = 3
    m[8:14, 2:4] = 4
    y, x = np.ogrid[:48, :64]
    m[(y - 25.5) ** 2 + (x - 20.5) ** 2 <= 36.0] = 5     # an even-diameter disc: the centroid lies between four pixels
    m[8:11, 30:34] = 6                                   # 3 x 4 and 5 x 2: two-way ties
    m[14:19, 40:42] = 7
    return m


def thin():
    m = np.zeros((48, 48), np.int32)
    m[2, 2] = 1
    m[5, 4:34] = 2
    m[8:38, 40] = 3
    for i in range(20):
        m[12 + i, 4 + i] = 4                             # connected by corners only
    return m


def split():
    m = np.zeros((40, 48), np.int32)
    m[4:13, 4:13] = 1
    m[30:34, 38:42] = 1                                  # the second component of id 1
    m[20:27, 20:30] = 2
    return m


def split_cold():
    """the pixels of `split` that never receive heat"""
    c = np.zeros((40, 48), bool)
    c[30:34, 38:42] = True
    return c


def serpentine():
    """a one-pixel path through a 41 x 41 box: rows two apart, joined at alternating ends"""
    m = np.zeros((45, 45), np.int32)
    for k, r in enumerate(range(2, 43, 2)):
        m[r, 2:43] = 1
        if r + 2 < 43:
            m[r + 1, 42 if k % 2 == 0 else 2] = 1
    return m


def geodesic(m, start):
    """8-connected step count from `start` inside its label (-1: unreachable)"""
    lab = m[start]
    d = np.full(m.shape, -1, np.int64)
    d[start] = 0
    front = [start]
    while front:
        nxt = []
        for y, x in front:
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < m.shape[0] and 0 <= xx < m.shape[1] and m[yy, xx] == lab and d[yy, xx] < 0:
                        d[yy, xx] = d[y, x] + 1
                        nxt.append((yy, xx))
        front = nxt
    return d


def gaps():
    H = W = 32
    top = max_labels(H, W) - 1
    m = np.zeros((H, W), np.int32)
    _disc(m, 7, 8, 5, 1)
    m[18:29, 3:9] = 7
    m[20:24, 9:14] = 7
    _disc(m, 20, 23, 6, top)
    m[20, 23:30] = 0
    return m


def _irregular(h, w, k):
    """an h x w box with its four corners cut by different arcs and wavy notches in its sides; every side keeps a pixel, so
    the box is the label's bounding box"""
    y, x = np.mgrid[:h, :w].astype(np.float64)
    s = np.ones((h, w), bool)
    r = [0.22 + 0.05 * ((k + i) % 4) for i in range(4)]
    for (cy, cx), rr in zip(((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)), r):
        ry, rx = rr * h, rr * w
        inside = (np.abs(y - cy) < ry) & (np.abs(x - cx) < rx)
        s &= ~(inside & (((np.abs(y - cy) - ry) / ry) ** 2 + ((np.abs(x - cx) - rx) / rx) ** 2 > 1.0))
    f = [0.3 + 0.05 * ((k + i) % 4) for i in range(4)]                      # the notches have depth 0 at the middle of each side
    s &= y >= 1.5 * (1 - np.cos(f[0] * (x - w // 2))) - 0.5
    s &= (h - 1 - y) >= 1.5 * (1 - np.cos(f[1] * (x - w // 2))) - 0.5
    s &= x >= 1.5 * (1 - np.cos(f[2] * (y - h // 2))) - 0.5
    s &= (w - 1 - x) >= 1.5 * (1 - np.cos(f[3] * (y - h // 2))) - 0.5
    return s


# (y0, x0, h, w) of the eight labels of `four_paths`, two per diffusion path
FOUR_PATHS_BOXES = [(0, 0, 136, 136), (0, 136, 134, 136),                  # global planes: 19 044 and 18 768 cells
                    (0, 272, 90, 88), (90, 272, 110, 88),                  # one plane: 8 280 and 10 080
                    (136, 0, 64, 120), (136, 120, 44, 44),                 # two planes: 8 052 and 2 116
                    (136, 164, 43, 43), (136, 207, 30, 40)]                # first launch: 2 025 and 1 344


def four_paths():
    """200 x 360: labels 1 .. 8 are the irregular boxes above; labels 9 .. 13 are small discs in a cut corner of each of the
    five largest, touching them (and lying inside their boxes)"""
    m = np.zeros((200, 360), np.int32)
    for k, (y0, x0, h, w) in enumerate(FOUR_PATHS_BOXES, 1):
        m[y0:y0 + h, x0:x0 + w][_irregular(h, w, k)] = k
    for j, k in enumerate((1, 2, 3, 4, 5)):
        y0, x0, h, w = FOUR_PATHS_BOXES[k - 1]
        sub = m[y0:y0 + h, x0:x0 + w]
        free = np.zeros((h, w), bool)
        free[:h // 4, :w // 4] = sub[:h // 4, :w // 4] == 0                 # the cut top-left corner
        y, x = np.mgrid[:h, :w]
        d = h // 10
        sub[free & ((y - d) ** 2 + (x - d) ** 2 <= d * d) & (y >= 2) & (x >= 2)] = 9 + j
    return m


def padded_cells(m):
    """{label: (bbox height + 2) * (bbox width + 2)}"""
    out = {}
    for l in np.unique(m[m > 0]):
        yy, xx = np.nonzero(m == l)
        out[int(l)] = int((yy.max() - yy.min() + 3) * (xx.max() - xx.min() + 3))
    return out


SAME_WG_H, SAME_WG_W = 112, 232


def same_workgroup(nT):
    """ids so that ONE workgroup of the second diffusion launch (stride = its grid) runs a one-plane label, then a two-plane
    label with a smaller box, then another two-plane label; and one of the first launch (stride 128) two small labels, the
    larger box first.  The map has a free margin of 8 pixels for the translates of the batched run."""
    L = max_labels(SAME_WG_H, SAME_WG_W)
    g = diffuse_big_grid(nT, L)
    m = np.zeros((SAME_WG_H, SAME_WG_W), np.int32)
    for lab, (y0, x0, h, w) in ((2, (8, 8, 94, 92)), (2 + g, (8, 104, 50, 48)), (2 + 2 * g, (8, 156, 60, 66)),
                                (1, (62, 104, 40, 38)), (1 + DIFF_SMALL_GRID, (72, 146, 20, 9))):
        m[y0:y0 + h, x0:x0 + w][_irregular(h, w, lab)] = lab
    return m


def translate(a, dy, dx):
    """a moved by (dy, dx) along its last two axes, zeros moving in"""
    out = np.zeros_like(a)
    H, W = a.shape[-2:]
    ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
    xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
    out[..., yd, xd] = a[..., ys, xs]
    return out


SAME_WG_SHIFTS = [(0, 0), (-7, 5), (3, -8), (8, 8), (-8, -8), (5, 0), (0, -3), (-2, 7)]


def centre_crowd():
    """64 x 64: 91 labels of 2 x 2 pixels, three apart, in the first 32 rows (one workgroup's 2048 pixels), with the ids
    whose hash slots crowd one window"""
    ids = crowd_ids(max_labels(64, 64))
    m = np.zeros((64, 64), np.int32)
    for k, l in enumerate(ids):
        y, x = 3 * (k // 21), 3 * (k % 21)
        m[y:y + 2, x:x + 2] = l
    return m


INSTANCE_MAPS = {"touching": touching, "concave": concave, "even_ties": even_ties, "thin": thin, "split": split,
                 "serpentine": serpentine, "gaps": gaps, "centre_crowd": centre_crowd}


# ---- class vote --------------------------------------------------------------------------------------------------------
VOTE_SCENARIOS = ["pixel_tie", "count_tie", "neg_zero_first", "pos_zero_first", "pos_inf", "two_pos_inf", "neg_inf", "all_neg_inf",
                  "nan_first", "nan_middle", "nan_twice", "nan_against_inf"]


def vote_logits(masks, ncls=7, seed=0):
    """float32 (ncls, H, W): label l gets scenario VOTE_SCENARIOS[l % 12] in all its pixels (ncls >= 7); the background is noise"""
    assert ncls >= 7
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((ncls,) + masks.shape).astype(np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    for l in np.unique(masks[masks > 0]):
        yy, xx = np.nonzero(masks == l)
        name = VOTE_SCENARIOS[int(l) % len(VOTE_SCENARIOS)]
        v = np.full((ncls, len(yy)), -1.0, np.float32)
        if name == "pixel_tie":
            v[2] = v[5] = 1.0
        elif name == "count_tie":                           # half the pixels say 4, half say 1 (an odd one out says 6)
            half = len(yy) // 2
            v[4, :half] = 1.0
            v[1, half:2 * half] = 1.0
            v[6, 2 * half:] = 1.0
        elif name == "neg_zero_first":
            v[1], v[3] = -0.0, 0.0
        elif name == "pos_zero_first":
            v[2], v[4] = 0.0, -0.0
        elif name == "pos_inf":
            v[0], v[3] = 3.0e38, inf
        elif name == "two_pos_inf":
            v[2] = v[5] = inf
        elif name == "neg_inf":
            v[:] = -inf
            v[4] = -3.0e38
        elif name == "all_neg_inf":
            v[:] = -inf
        elif name == "nan_first":
            v[0], v[3] = nan, 5.0
        elif name == "nan_middle":
            v[3], v[5] = nan, 5.0
        elif name == "nan_twice":
            v[2], v[5], v[6] = nan, nan, 5.0
        elif name == "nan_against_inf":
            v[1], v[4] = inf, nan
        lg[:, yy, xx] = v
    return lg


VOTE_EXPECT = {"pixel_tie": 2, "count_tie": 1, "neg_zero_first": 1, "pos_zero_first": 2, "pos_inf": 3, "two_pos_inf": 2, "neg_inf": 4,
               "all_neg_inf": 0, "nan_first": 0, "nan_middle": 3, "nan_twice": 2, "nan_against_inf": 4}


def vote_blocks(n=24, side=6, H=64, W=64):
    """labels 1 .. n as side x side blocks, one pixel apart"""
    m = np.zeros((H, W), np.int32)
    per_row = W // (side + 1)
    for k in range(n):
        y, x = (side + 1) * (k // per_row), (side + 1) * (k % per_row)
        m[y:y + side, x:x + side] = k + 1
    return m


# ---- border removal ----------------------------------------------------------------------------------------------------
def border_cases():
    """name -> int32 map"""
    out = {}
    m = np.zeros((24, 40), np.int32)
    m[5:12, 5:12] = 1                                       # interior
    m[0, 39] = 2                                            # touches with one corner pixel only ...
    m[1:4, 36:39] = 2
    m[1, 39] = 0
    m[20:23, 0:1] = 3
    m[20:23, 1:6] = 3
    m[14:18, 20:30] = 4                                     # interior
    out["corner_pixel"] = m
    m = np.zeros((24, 40), np.int32)
    m[0:3, 10:14] = 1
    m[21:24, 20:24] = 2
    m[8:12, 0:3] = 3
    m[10:14, 37:40] = 4
    m[8:14, 15:25] = 5                                      # interior, kept
    m[1:5, 30:34] = 6                                       # one pixel off the top: kept
    out["each_side"] = m
    m = np.zeros((24, 40), np.int32)
    m[0:3, 0:3] = 3
    m[10:13, 10:13] = 9
    m[21:24, 30:33] = 200
    m[5:8, 20:25] = 41
    out["id_gaps"] = m
    m = np.zeros((16, 16), np.int32)
    m[0:2, 4:6] = 65535
    m[6:9, 6:9] = 65534
    m[12:14, 12:14] = 7
    out["id_65535"] = m
    return out
