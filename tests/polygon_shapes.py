"""Shape generators for the polygoniser tests (plain numpy; no GPU, no reference tree): uint16 id maps that put ring
sizes, local tops, offending edge pairs and record counts on the boundaries of the device polygoniser
(csrc/cpx_polygons.hip: 64-lane chunks of the local-top search, the lane-strided partners and the 16-edge early exit of
the validity vote, the 1024-record chunks of the scan, the vertex pool), the numpy restatement of cpx_instance_records,
and the comparison with oracle/polygons.py that the host and the device tests share.  The expected vertex counts and
validities (SMALL_RINGS, VIS_EXPECT, ...) are the oracle's, run on the CPU: tests/test_polygon_shapes_host.py asserts them
on the oracle and on the host polygoniser, tests/test_gpu_polygons_edges.py on the device."""
import functools

import numpy as np

from classpose_amd.engine import RECORD_DTYPE
from oracle import polygons as opoly

# the second placement of the scaled cases: a non-dyadic prediction-to-slide scale and a large level-0 origin
SCALES = ((1.0, (0.0, 0.0)), (2.2727, (98321.0, 65541.0)))


def records(m, cm=None):
    """what cpx_instance_records emits; the class is the class map at the instance's first raster pixel when cm is given"""
    labs = [l for l in np.unique(m) if l]
    recs = np.zeros(len(labs), RECORD_DTYPE)
    for i, l in enumerate(labs):
        ys, xs = np.nonzero(m == l)
        cls = 1 + int(l) % 6 if cm is None else int(cm[ys[0], xs[0]])
        recs[i] = (0, l, cls, len(ys), ys.min(), xs.min(), ys.max() + 1, xs.max() + 1, ys.sum(), xs.sum())
    return recs


def class_map(m, recs):
    """the class map whose instances carry their record's class"""
    cm = np.zeros(m.shape, np.uint8)
    for r in recs:
        cm[m == r["label"]] = r["cls"]
    return cm


# ---- comb: one component, a local top per tooth, ring size 6 * nt + 3 -------------------------------------------------------
COMB_H = 14
COMB_NT = (3, 10, 11, 15, 16, 17, 21, 22, 40)                 # rings of 21 ... 243 vertices: both sides of 64, 128 and of multiples of 16
COMB_DEFECTS = tuple((40, d, k) for k in ("spike", "pinch") for d in (0, 10, 21, 39))
# the offending edge pairs (i, j) of a defect ring of n vertices, whichever tooth carries the defect
COMB_PAIRS = {"spike": lambda n: [(0, n - 2), (0, n - 1)], "pinch": lambda n: [(0, n - 2), (0, n - 1), (1, n - 2), (1, n - 1)]}
COMB_N_PTS = {None: lambda nt: 6 * nt + 3, "spike": lambda nt: 6 * nt + 4, "pinch": lambda nt: 6 * nt + 5}


def comb_pixels(nt, defect=None, kind=None):
    """bool [COMB_H, 4 nt + 4]: a bar with nt teeth; ``kind`` on tooth ``defect``: "spike" = a 1-px whisker rising from the
    tooth's left column, "pinch" = one pixel touching the tooth's top-right corner diagonally.  Either one rises above the
    teeth, so it is the raster-first pixel and the ring starts on it whichever tooth carries it: the ring folds back over
    its first edge at the wrap, and the offending pairs are COMB_PAIRS -- edge 0 or 1 against the last two edges, more than
    three 64-lane strides apart (comb_down puts the offending pairs elsewhere on the ring)."""
    W = 4 * nt + 4
    b = np.zeros((COMB_H, W), bool)
    b[8:12, 1:W - 1] = True
    for k in range(nt):
        b[4:8, 2 + 4 * k: 4 + 4 * k] = True
    if kind is not None:
        x = 2 + 4 * defect
        if kind == "spike":
            b[1:4, x] = True
        elif kind == "pinch":
            b[3, x + 2] = True
        else:
            raise ValueError(kind)
    return b


def comb(nt, defect=None, kind=None):
    return comb_pixels(nt, defect, kind).astype(np.uint16)


def comb_expect(nt, kind=None):
    """(n_pts, valid) of a comb's ring"""
    return COMB_N_PTS[kind](nt), int(kind is None)


# ---- comb with its teeth pointing down: the ring starts on the bar, so a defect on tooth k sits near ring index 6 k + 4 ---------
DOWN_DEFECTS = ((40, 0), (40, 39), (41, 40))
# (nt, tooth) -> the offending edge pairs (i, j), all between non-neighbouring edges (no lane-0 partner j = i + 1 among them):
# (40, 39): 249 vertices, the pairs end in the edge that votes (i = 239); (41, 40): 255 vertices, every pair lies behind the last vote (i = 239)
DOWN_PAIRS = {(40, 0): 3, (40, 39): 237, (41, 40): 243}       # the first offending edge; the seven pairs are
DOWN_PAIR_SHAPE = ((0, 6), (0, 7), (1, 5), (1, 6), (1, 7), (2, 5), (2, 6))    # (first + di, first + dj)


def comb_down_pixels(nt, defect=None):
    """bool [14, 6 nt + 2]: a bar with nt teeth hanging from it (period 6); ``defect``: a 2x2 block touching that tooth's
    bottom-right corner diagonally, so the ring passes two of its vertices twice (invalid, without any fold-back)"""
    W = 6 * nt + 2
    b = np.zeros((COMB_H, W), bool)
    b[2:6, 1:W - 1] = True
    for k in range(nt):
        b[6:10, 2 + 6 * k: 4 + 6 * k] = True
    if defect is not None:
        b[10:12, 4 + 6 * defect: 6 + 6 * defect] = True
    return b


def comb_down(nt, defect=None):
    return comb_down_pixels(nt, defect).astype(np.uint16)


def comb_down_expect(nt, defect=None):
    return (6 * nt + 3, 1) if defect is None else (6 * nt + 9, 0)


def offending_pairs(xy):
    """every edge pair (i, j), i < j, of the open ring xy (pixel coordinates: integers, so int64 is exact) that breaks its
    validity, by the rules of oracle.polygons.ring_is_valid"""
    p = np.asarray(xy).astype(np.int64)
    assert np.array_equal(p, np.asarray(xy))
    n = len(p)
    i, j = np.triu_indices(n, 1)
    a0, a1, b0, b1 = p[i], p[(i + 1) % n], p[j], p[(j + 1) % n]

    def orient(a, b, c):
        return np.sign((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))

    def on(a, b, c):
        return (np.minimum(a, b) <= c).all(1) & (c <= np.maximum(a, b)).all(1)

    o1, o2, o3, o4 = orient(a0, a1, b0), orient(a0, a1, b1), orient(b0, b1, a0), orient(b0, b1, a1)
    cross = ((o1 * o2 < 0) & (o3 * o4 < 0)) | ((o1 == 0) & on(a0, a1, b0)) | ((o2 == 0) & on(a0, a1, b1)) | \
        ((o3 == 0) & on(b0, b1, a0)) | ((o4 == 0) & on(b0, b1, a1))
    nxt, wrap = j == i + 1, (i == 0) & (j == n - 1) & (j != i + 1)
    sh, pa, pb = np.where(nxt[:, None], a1, a0), np.where(nxt[:, None], a0, a1), np.where(nxt[:, None], b1, b0)
    fold = (orient(sh, pa, pb) == 0) & (((pa - sh) * (pb - sh)).sum(1) > 0)
    bad = np.where(nxt | wrap, fold, cross)
    return list(zip(i[bad].tolist(), j[bad].tolist()))


# ---- small rings ---------------------------------------------------------------------------------------------------------
# label -> (n_pts, valid)
SMALL_RINGS = {1: (10, 1),      # two 3x3 squares sharing a corner PIXEL: the 8-connected trace cuts the corner
               2: (10, 0),      # two 3x3 squares touching only diagonally: the ring passes its pinch vertex twice
               3: (10, 0),      # ... joined by a 1-px diagonal neck: two edges run over each other
               4: (6, 0),       # a block with a whisker rising from its raster-first pixel: the fold-back is the wrap pair (0, n - 1)
               5: (9, 0)}       # a block with a side whisker: a fold-back in the middle of the ring
SMALL_H, SMALL_W = 24, 41          # an odd width


def small_rings(labels=(1, 2, 3, 4, 5)):
    a, b, c, d, e = labels
    m = np.zeros((SMALL_H, SMALL_W), np.uint16)
    m[2:5, 2:5] = a; m[4:7, 4:7] = a
    m[2:5, 12:15] = b; m[5:8, 15:18] = b
    m[2:5, 24:27] = c; m[5, 27] = c; m[6:9, 28:31] = c
    m[13:16, 4:7] = d; m[10:13, 4] = d
    m[11:16, 14:20] = e; m[13, 20:24] = e
    return m


HIGH_LABELS = (1, 32767, 32768, 40000, 65535)


# ---- several components under one label: which start wins -------------------------------------------------------------------
VIS_H, VIS_W = 40, 200
# label -> (first vertex (x, y), n_pts, valid)
VIS_EXPECT = {1: ((9, 5), 4, 1),          # the block between the U's arms
              2: ((22, 2), 10, 1),        # the U itself
              3: ((66, 20), 4, 1),        # second component's top in lane 63 of the first chunk
              4: ((67, 24), 4, 1),        # ... in lane 0 of the second chunk
              5: ((139, 28), 4, 1),       # ... in the partial third chunk
              6: ((190, 34), 4, 1)}       # both components start in the same row, 187 px apart


def vis_map():
    m = np.zeros((VIS_H, VIS_W), np.uint16)
    # 1: a U with a short right arm and a block between the arms.  Tops in raster order: left arm (row 2), block (row 5),
    #    right arm (row 8, on the U's border, already visited): the last NEW component is the block
    m[2:16, 2:4] = 1; m[8:16, 16:18] = 1; m[14:16, 2:18] = 1; m[5:9, 9:11] = 1
    # 2: the mirror: the block (rows 0..3, between the arms) starts before both arms: the outline is the U's, from its left arm
    m[2:16, 22:24] = 2; m[8:16, 36:38] = 2; m[14:16, 22:38] = 2; m[0:4, 29:31] = 2
    # 3 - 5: first component at the box's left edge, the second one lower down and 63 / 64 / 136 columns to the right
    m[18:20, 3:5] = 3; m[20:22, 66:68] = 3
    m[22:24, 3:5] = 4; m[24:26, 67:69] = 4
    m[26:28, 3:5] = 5; m[28:30, 139:141] = 5
    # 6: both components start in row 34, in the first and in the third chunk
    m[34:36, 3:5] = 6; m[34:37, 190:193] = 6
    return m


# ---- wide shapes and tile edges --------------------------------------------------------------------------------------------
EDGE_H, EDGE_W = 61, 200


def _crop(b):
    ys, xs = np.nonzero(b)
    return b[ys.min(): ys.max() + 1, xs.min(): xs.max() + 1]


def edge_tiles():
    """[4, 61, 200] and, per tile, label -> (n_pts, valid)"""
    t = np.zeros((4, EDGE_H, EDGE_W), np.uint16)
    exp = []
    # 0: a 40-tooth comb whose whisker tip is the tile's pixel (0, 1)... its box starts at x = 0 and y = 0; a second one
    #    flush with the bottom-right corner; a plain one in between
    c = _crop(comb_pixels(40, 0, "spike"))
    t[0, :c.shape[0], :c.shape[1]][c] = 1
    c = _crop(comb_pixels(22))
    t[0, 20:20 + c.shape[0], 19:19 + c.shape[1]][c] = 2
    c = _crop(comb_pixels(40, 39, "pinch"))
    t[0, EDGE_H - c.shape[0]:, EDGE_W - c.shape[1]:][c] = 3
    exp.append({1: comb_expect(40, "spike"), 2: comb_expect(22), 3: comb_expect(40, "pinch")})
    # 1: one instance over the whole tile
    t[1] = 1
    exp.append({1: (4, 1)})
    # 2: 1-px lines along the four edges, single pixels in the four corners
    t[2, 0, 2:EDGE_W - 2] = 1; t[2, EDGE_H - 1, 2:EDGE_W - 2] = 2; t[2, 2:EDGE_H - 2, 0] = 3; t[2, 2:EDGE_H - 2, EDGE_W - 1] = 4
    t[2, 0, 0] = 5; t[2, 0, EDGE_W - 1] = 6; t[2, EDGE_H - 1, 0] = 7; t[2, EDGE_H - 1, EDGE_W - 1] = 8
    exp.append({1: (2, 0), 2: (2, 0), 3: (2, 0), 4: (2, 0), 5: (1, 0), 6: (1, 0), 7: (1, 0), 8: (1, 0)})
    # 3: valid instances on the four edges, the horizontal ones wider than two 64-lane chunks
    t[3, 0:3, 10:190] = 1; t[3, EDGE_H - 3:, 10:190] = 2; t[3, 5:56, 0:3] = 3; t[3, 5:56, EDGE_W - 3:] = 4
    exp.append({1: (4, 1), 2: (4, 1), 3: (4, 1), 4: (4, 1)})
    return t, exp


NARROW_EXPECT = {1: (4, 1), 2: (2, 0), 3: (1, 0)}


def narrow_tile():
    """a 2-column tile"""
    m = np.zeros((11, 2), np.uint16)
    m[0:4, :] = 1; m[5:9, 1] = 2; m[10, 0] = 3
    return m


# ---- dense tile: more records than one 1024-thread chunk of the scan ---------------------------------------------------------
DENSE = 128
DENSE_N = (1023, 1024, 1025, 1500)                             # one short of, exactly, one more than a 1024-record chunk of the scan; more than max_labels


def dense_tile(n):
    """128 x 128, the first n sites of a stride-3 lattice, alternately a single pixel (1 vertex) and a 2x2 square (4 vertices, valid)"""
    per = DENSE // 3
    assert 0 <= n <= per * per
    m = np.zeros((DENSE, DENSE), np.uint16)
    for k in range(n):
        y, x = 3 * (k // per), 3 * (k % per)
        if k & 1:
            m[y: y + 2, x: x + 2] = k + 1
        else:
            m[y, x] = k + 1
    return m


def dense_records(n):
    """records() of dense_tile(n) without n passes over the tile"""
    per = DENSE // 3
    recs = np.zeros(n, RECORD_DTYPE)
    k = np.arange(n)
    y, x, s = 3 * (k // per), 3 * (k % per), 1 + (k & 1)
    recs["label"] = k + 1; recs["cls"] = 1 + (k + 1) % 6; recs["area"] = s * s
    recs["y0"] = y; recs["x0"] = x; recs["y1"] = y + s; recs["x1"] = x + s
    recs["sum_y"] = np.where(s == 2, 4 * y + 2, y); recs["sum_x"] = np.where(s == 2, 4 * x + 2, x)
    return recs


def dense_expect(n):
    """(n_pts, valid) per record"""
    odd = (np.arange(n) & 1).astype(np.int32)
    return 1 + 3 * odd, odd


# ---- random blobs (the recipe of test_host_polygonizer_equals_oracle_random_blobs) ---------------------------------------------
BLOBS = ((0, 0.02), (1, 0.0), (2, 0.05), (3, 0.0), (4, 0.03))
BLOB_H, BLOB_W = 96, 128


def blob_tile(seed, thr):
    from scipy.ndimage import binary_fill_holes, gaussian_filter, label
    rng = np.random.default_rng(seed)
    img = gaussian_filter(rng.standard_normal((BLOB_H, BLOB_W)), 2.5) > thr
    lab, n = label(binary_fill_holes(img))
    lab[lab == n] = 1                                         # merged labels: multi-component instances occur
    return lab.astype(np.uint16)


# ---- the comparison with the oracle ---------------------------------------------------------------------------------------
def _edge(i):
    return lambda: edge_tiles()[0][i]


MAPS = {"small": small_rings, "high": lambda: small_rings(HIGH_LABELS), "vis": vis_map, "narrow": narrow_tile,
        **{f"edge{i}": _edge(i) for i in range(4)},
        **{f"dense{n}": functools.partial(dense_tile, n) for n in (1,) + DENSE_N},
        **{f"blob{s}": functools.partial(blob_tile, s, t) for s, t in BLOBS},
        **{f"comb{nt}": functools.partial(comb, nt) for nt in COMB_NT},
        **{f"comb{nt}_{k}{d}": functools.partial(comb, nt, d, k) for nt, d, k in COMB_DEFECTS},
        **{f"down{nt}_{d}": functools.partial(comb_down, nt, d) for nt, d in DOWN_DEFECTS}}


def _oracle_tile(m, cm, scale, origin):
    """((label, contours[0] in level-0 coordinates) of every label, the oracle's PostProcessor loop: its valid cells)"""
    contours = []
    for lab in [l for l in np.unique(m) if l]:
        ys, xs = np.nonzero(m == lab)
        cont = opoly.find_contours_external_simple((m == lab)[ys.min(): ys.max() + 1, xs.min(): xs.max() + 1])[0]
        contours.append((int(lab), (cont + [xs.min(), ys.min()]) * scale + np.asarray(origin)))
    return contours, opoly.post_process_tile(m, cm, origin, scale)


@functools.lru_cache(maxsize=None)
def _oracle_map(key, scale, origin):
    m = MAPS[key]()
    return _oracle_tile(m, class_map(m, records(m)), scale, origin)


def compare_with_oracle(m, cm, scale, origin, cells, xy, perimeter_rel=1e-14):
    """cells / xy (one row per label of m, label order) against the oracle: the contour and the validity of every cell; area
    exact, perimeter to perimeter_rel (relative), centroid to 1e-9 and the class for the valid ones.  Returns the number of
    valid cells.  ``m`` may be a key of MAPS (cm = None: the classes are those of records()); the oracle's answer for such
    a map is computed once per process and shared by the host and the device tests."""
    if isinstance(m, str):
        contours, ref = _oracle_map(m, float(scale), (float(origin[0]), float(origin[1])))
    else:
        contours, ref = _oracle_tile(m, cm, scale, origin)
    assert len(cells) == len(contours)
    for c, (lab, exp) in zip(cells, contours):
        # every contour (valid or not) equals OpenCV-order contours[0]
        assert np.array_equal(xy[c["offset"]: c["offset"] + c["n_pts"]], exp), lab
    assert [lab for c, (lab, _) in zip(cells, contours) if c["valid"] == 1] == [r["label"] for r in ref]
    for c, r in zip(cells[cells["valid"] == 1], ref):
        assert c["area"] == r["area"] and abs(c["perimeter"] - r["perimeter"]) <= perimeter_rel * r["perimeter"], r["label"]
        assert abs(c["cx"] - r["centroid_raw"][0]) < 1e-9 and abs(c["cy"] - r["centroid_raw"][1]) < 1e-9, r["label"]
        assert c["cls"] - 1 == r["class_int"]
    return len(ref)
