"""The CPU statement of the rasterisation rule (include/classpose_hip.h, cpx_rasterize_polygons), twice, and the
ring cases the host and the device tests share.  Plain numpy: no GPU, no reference tree.

THE RULE.  Pixel (r, c) has its centre at x = c, y = r.  A ring paints the pixel when the centre lies on the ring (an edge or a
vertex) or has an odd crossing number (even-odd, half-open edge test min(y0, y1) <= y < max(y0, y1)).  With
    d = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
on the edge:  d == 0 and the centre inside the edge's closed box;   crossing:  (y0 <= py < y1 and d > 0) or (y1 <= py < y0 and d < 0).
A closing vertex equal to the first is dropped; fewer than three vertices after that paint nothing; rings are clipped to the image.

  * ``ring_masks_exact``  integer arithmetic on coordinates scaled by 16 (they must be multiples of 1/16): int64 cannot round,
                          |coordinate| <= 32768 keeps every product below 2^41;
  * ``ring_masks_float``  numpy float64 in the kernel's operand order (numpy rounds every ufunc on its own: no contraction).
Both return ``(r0, c0, parity, on)``: the clipped bounding box's corner and two bool arrays over the box.
"""
import math

import numpy as np
from scipy import ndimage

SCALE = 16


def _drop_closing(x, y):
    if len(x) >= 2 and x[0] == x[-1] and y[0] == y[-1]:
        x, y = x[:-1], y[:-1]
    return x, y


def _masks(x, y, H, W, scale, lo_hi):
    """x, y: vertex coordinates times ``scale`` (int64 with scale 16, float64 with scale 1); lo_hi(min, max) -> the integer
    range of pixel coordinates inside [min, max]"""
    x, y = _drop_closing(x, y)
    empty = (0, 0, np.zeros((0, 0), bool), np.zeros((0, 0), bool))
    n = len(x)
    if n < 3:
        return empty
    c0, c1 = lo_hi(x.min(), x.max())
    r0, r1 = lo_hi(y.min(), y.max())
    c0, r0, c1, r1 = max(c0, 0), max(r0, 0), min(c1, W - 1), min(r1, H - 1)
    if c0 > c1 or r0 > r1:
        return empty
    par = np.zeros((r1 - r0 + 1, c1 - c0 + 1), bool)
    on = np.zeros_like(par)
    px = (np.arange(c0, c1 + 1) * scale).astype(x.dtype)[None, :]
    for e in range(n):
        x0, y0, x1, y1 = x[e], y[e], x[(e + 1) % n], y[(e + 1) % n]
        a, b = lo_hi(min(y0, y1), max(y0, y1))                 # the rows whose centre is inside the edge's closed y range
        a, b = max(a, r0), min(b, r1)
        if a > b:
            continue
        py = (np.arange(a, b + 1) * scale).astype(x.dtype)[:, None]
        d = (x1 - x0) * (py - y0) - (y1 - y0) * (px - x0)
        cross = ((y0 <= py) & (py < y1) & (d > 0)) | ((y1 <= py) & (py < y0) & (d < 0))
        par[a - r0:b - r0 + 1] ^= cross
        on[a - r0:b - r0 + 1] |= (d == 0) & (min(x0, x1) <= px) & (px <= max(x0, x1))
    return r0, c0, par, on


def to_sixteenths(ring) -> np.ndarray:
    ring = np.asarray(ring, np.float64).reshape(-1, 2)
    q = ring * SCALE
    assert np.array_equal(q, np.rint(q)) and (np.abs(ring) <= 32768).all(), "the exact version takes multiples of 1/16 up to 32768"
    return q.astype(np.int64)


def ring_masks_exact(ring, H, W):
    q = to_sixteenths(ring)
    return _masks(q[:, 0], q[:, 1], H, W, SCALE, lambda lo, hi: (-((-int(lo)) // SCALE), int(hi) // SCALE))


def ring_masks_float(ring, H, W):
    ring = np.asarray(ring, np.float64).reshape(-1, 2)
    return _masks(ring[:, 0].copy(), ring[:, 1].copy(), H, W, 1, lambda lo, hi: (math.ceil(lo), math.floor(hi)))


def rasterize(xy, ring_off, ring_value, shape, ring_image=None, n_images=1, out=None, masks=ring_masks_exact):
    """int32 maps (n_images, H, W): every ring painted as ``max`` onto ``out`` (a copy) or onto zeros"""
    H, W = shape
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    res = np.zeros((n_images, H, W), np.int32) if out is None else np.array(out, np.int32)
    for k in range(len(ring_value)):
        r0, c0, par, on = masks(xy[ring_off[k]:ring_off[k + 1]], H, W)
        img = 0 if ring_image is None else int(ring_image[k])
        view = res[img, r0:r0 + par.shape[0], c0:c0 + par.shape[1]]
        np.maximum(view, np.where(par | on, np.int32(ring_value[k]), np.int32(0)), out=view)
    return res


def pack(rings, values=None, images=None):
    """list of (n, 2) rings -> (xy float64, ring_off int64, ring_value int32, ring_image int32 | None)"""
    rings = [np.asarray(r, np.float64).reshape(-1, 2) for r in rings]
    off = np.zeros(len(rings) + 1, np.int64)
    off[1:] = np.cumsum([len(r) for r in rings])
    xy = np.concatenate(rings) if rings else np.zeros((0, 2))
    values = np.arange(1, len(rings) + 1) if values is None else values
    return (np.ascontiguousarray(xy, np.float64), off, np.asarray(values, np.int32),
            None if images is None else np.asarray(images, np.int32))


# ---- the shared cases: name -> (rings, (H, W)); every coordinate is a multiple of 1/16 ----------------------------------------
def q16(a):
    return np.rint(np.asarray(a, np.float64) * SCALE) / SCALE


def star(n, cx, cy, r_out, r_in):
    """n vertices alternating between two radii, quantised to 1/16"""
    t = 2 * np.pi * np.arange(n) / n
    r = np.where(np.arange(n) % 2 == 0, r_out, r_in)
    return q16(np.stack([cx + r * np.cos(t), cy + r * np.sin(t)], 1))


def cut_box(c0, r0, w, h):
    """a hexagon (two corners of a rectangle cut) whose clipped bounding box holds exactly w x h pixel centres from (r0, c0)"""
    x0, x1, y0, y1 = c0 - 0.25, c0 + w - 1 + 0.25, r0 - 0.25, r0 + h - 1 + 0.25
    return q16([(x0, y0 + (y1 - y0) / 3), (x0 + (x1 - x0) / 3, y0), (x1, y0), (x1, y1 - (y1 - y0) / 3), (x1 - (x1 - x0) / 3, y1), (x0, y1)])


TRIANGLE = [(3.25, 2.5), (30.0625, 10.0), (12.0, 33.75)]
SHAPE = (40, 48)
SINGLE = {
    "triangle": [TRIANGLE],
    "concave_u": [[(4, 4), (12, 4), (12, 24.5), (28, 24.5), (28, 4), (36.5, 4), (36.5, 34), (4, 34)]],
    "bowtie": [[(5, 5), (30, 30), (30, 5), (5, 30)]],
    "spur": [[(5, 5), (20, 5), (20, 12), (26, 12), (20, 12), (20, 20), (5, 20)]],
    "vertices_on_centres": [[(6, 3), (25, 8), (33, 21), (17, 35), (4, 19)]],
    "diagonal_through_centres": [[(2, 2), (22, 22), (2, 22)]],
    "axis_edges_on_integers": [[(4, 6), (30, 6), (30, 25), (4, 25)]],
    "half_integers": [[(4.5, 6.5), (30.5, 6.5), (30.5, 25.5), (17.5, 30.5), (4.5, 25.5)]],
    "sixteenths": [[(4.0625, 6.9375), (31.3125, 3.4375), (35.5625, 27.1875), (15.8125, 36.0625), (7.4375, 20.5625)]],
    "collinear": [[(3, 3), (10, 10), (20, 20)]],
    "collinear_flat": [[(3, 7), (30, 7), (12, 7)]],
    "two_vertices": [[(3, 3), (20, 9)]],
    "two_vertices_closed": [[(3, 3), (20, 9), (3, 3)]],
    "triangle_closed": [TRIANGLE + TRIANGLE[:1]],
    "clip_left": [[(-9.5, 5), (12, 9.25), (-3, 30)]],
    "clip_right": [[(40, 5), (60.5, 9.25), (44, 30)]],
    "clip_top": [[(10, -8), (30, -2.5), (22, 14)]],
    "clip_bottom": [[(10, 30), (30, 33.5), (22, 55)]],
    "clip_all_sides": [[(-5, -7), (60, -3), (55, 50), (-8, 44)]],
    "outside_left": [[(-30, 5), (-2, 9), (-12, 30)]],
    "outside_right": [[(48.5, 5), (70, 9), (55, 30)]],
    "outside_above": [[(5, -20), (30, -0.0625), (12, -9)]],
    "outside_below": [[(5, 39.0625), (30, 45), (12, 60)]],
}
CASES = {k: (v, SHAPE) for k, v in SINGLE.items()}

BOX_SIDES = (1, 63, 64, 65, 129)
for _w in BOX_SIDES:
    for _h in BOX_SIDES:
        CASES[f"box_{_w}x{_h}"] = ([cut_box(7, 5, _w, _h)], (140, 144))

# the kernel names a small-ring limit of 256 vertices / 4096 box pixels and a chunk of 512 edges (classpose_amd.ops.RASTER_*;
# tests/test_rasterize_host.py pins these numbers on the kernel source); 64 is the wave
VERTEX_COUNTS = (3, 4, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
STAR_SHAPE = (384, 512)
for _n in VERTEX_COUNTS:
    CASES[f"star_small_box_{_n}"] = ([star(_n, 250.5, 190.25, 28.0, 13.5)], STAR_SHAPE)      # box 57 x 57: the vertex limit decides
    CASES[f"star_large_box_{_n}"] = ([star(_n, 250.5, 190.25, 185.0, 70.0)], STAR_SHAPE)
# both sides of each limit, the other one held low
CASES["area_4096"] = ([cut_box(9, 11, 64, 64)], (100, 100))
CASES["area_4160"] = ([cut_box(9, 11, 65, 64)], (100, 100))
CASES["area_4097_by_1"] = ([cut_box(1, 1, 4097, 1)], (3, 4100))
CASES["vertices_256"] = CASES["star_small_box_256"]
CASES["vertices_257"] = CASES["star_small_box_257"]
# every edge straddles most rows: the compacted list of the large path is full in every chunk
CASES["zigzag_1400"] = ([q16(np.stack([40.0 + 0.25 * np.arange(1400), np.where(np.arange(1400) % 2 == 0, 3.5, 90.25)], 1))], (96, 420))


def ragged_cells(seed, H=256, W=256, pitch=25, r_lo=2.0, r_hi=11.0):
    """uint16 id map of disjoint, star-convex (hence hole-free), ragged cells on a jittered grid"""
    rng = np.random.default_rng(seed)
    m = np.zeros((H, W), np.uint16)
    yy, xx = np.mgrid[0:H, 0:W]
    label = 0
    for gy in range(H // pitch):
        for gx in range(W // pitch):
            cy, cx = gy * pitch + pitch // 2 + rng.integers(-1, 2), gx * pitch + pitch // 2 + rng.integers(-1, 2)
            a, b = rng.uniform(r_lo, r_hi, 2)
            k = 16
            rag = rng.uniform(0.6, 1.0, k)
            th = np.arctan2(yy - cy, xx - cx) + rng.uniform(0, 2 * np.pi)
            rr = rag[(np.floor(th / (2 * np.pi) * k).astype(int)) % k]
            inside = ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2 <= rr ** 2
            comp, _ = ndimage.label(inside, structure=np.ones((3, 3), int))        # one 8-connected component: the centre's
            label += 1
            m[comp == comp[cy, cx]] = label
    return m
