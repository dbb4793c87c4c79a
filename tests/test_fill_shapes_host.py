"""CPU only: the premises of tests/test_gpu_fill_handbuilt.py.  The kernel constants that tests/fill_shapes.py restates are
compared with the source text, and every property a case is named for is proved with the oracle and scipy alone -- so a
builder that stops producing its property, or a kernel constant that moves, fails here and not silently on the device."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest
from scipy import ndimage

import fill_shapes as S
from oracle import dynamics

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "classpose_amd", "csrc", "cpx_postproc.hip")


def _oracle(c):
    return dynamics.fill_holes_and_remove_small_masks(c.m.astype(np.uint16), c.min_size).astype(np.int32)


def _naive(m, min_size):
    """the filter as one would write it: labels below min_size out before and after the fill, ids by first appearance"""
    m = m.copy()
    a = np.bincount(m.ravel())
    m[np.isin(m, np.flatnonzero(a < min_size))] = 0
    m = dynamics.fr_renumber(m)
    out = dynamics.fill_holes_and_remove_small_masks(m, 0)
    a = np.bincount(out.ravel())
    out[np.isin(out, np.flatnonzero(a < min_size))] = 0
    return dynamics.fr_renumber(out)


def test_the_restated_constants_are_the_kernels():
    src = open(SRC).read()
    for pat in (rf"#define NTHR {S.NTHR}\b", rf"#define RUN_PX {S.RUN_PX}\b", rf"#define TAIL_LDS {S.TAIL_LDS}\b",
                rf"__launch_bounds__\({S.SIZE_FILTER_THREADS}\) k_size_filter", rf"dim3\({S.SIZE_FILTER_THREADS}\), 0, s, min_size",
                rf"const int per = \(vmax \+ {S.SIZE_FILTER_THREADS}\) / {S.SIZE_FILTER_THREADS};", r"const int per = \(vm \+ NTHR\) / NTHR;",
                rf"if \(bh > {S.MID} \|\| bw > {S.MID}\)", rf"if \(bh > {S.WORD} \|\| bw > {S.WORD}\)", rf"if \(bh <= {S.WORD} && bw <= {S.WORD}\) continue;",
                r"if \(vmax <= TAIL_LDS\)", r"\(k\+\+ & \(NTHR / 64 - 1\)\) != wave", r"return H \* W / 11 \+ 2;",
                r"const int r = lane \+ 64 \* j;", r"x0 \+ 64 \* w"):
        assert re.search(pat, src), pat
    assert S.WG_PX == 2048 and S.SEAMS == tuple(v for k in (1, 2, 3) for v in (S.WORD * k - 1, S.WORD * k))
    assert S.max_labels(S.SLICE_TILE, S.SLICE_TILE) == 2329


@pytest.mark.parametrize("name", list(S.STAGE_CASES))
def test_every_stage_case_is_what_it_declares(name):
    c = S.STAGE_CASES[name]()
    ref = _oracle(c)
    assert c.m.dtype == np.int32 and c.m.min() >= 0 and c.m.max() < S.max_labels(*c.m.shape), "ids within the tables"
    if c.path is not None:
        assert S.path_of(c.m) == c.path
    if c.filled is not None:
        assert int(((c.m == 0) & (ref > 0)).sum()) == c.filled
    if c.nlab is not None:
        present = len(np.unique(c.m[c.m > 0]))
        assert c.nlab == (int(ref.max()) if c.min_size > 0 else present)
    if c.min_size > 0:
        assert np.array_equal(np.unique(ref[ref > 0]), np.arange(1, ref.max() + 1))


# ---- A.1 -----------------------------------------------------------------------------------------------------------------
def test_small_boxes_touch_every_corner_and_edge_and_have_the_named_sizes():
    m = S.small_boxes_at_edges().m
    b = S.boxes(m)
    H, W = m.shape
    assert {(0, 0), (0, W - 3), (H - 3, 0), (H - 3, W - 3)} <= {(y, x) for y, x, _, _ in b.values()}
    assert any(y == 0 and 0 < x < W - 3 for y, x, _, _ in b.values()) and any(y == H - 3 and 0 < x < W - 3 for y, x, _, _ in b.values())
    assert any(x == 0 and 0 < y < H - 3 for y, x, _, _ in b.values()) and any(x == W - 3 and 0 < y < H - 3 for y, x, _, _ in b.values())
    assert {b[9][2:], b[10][2:], b[11][2:]} == {(1, 1), (1, 9), (9, 1)}
    assert all(int(S.holes_of(m, l).sum()) == 1 for l in range(1, 9))


@pytest.mark.parametrize("h,w", [(63, 63), (64, 64), (63, 64), (64, 63)])
def test_small_ring_holes_reach_the_last_inner_column_and_row(h, w):
    m = S.small_ring(h, w).m
    y0, x0, bh, bw = S.boxes(m)[1]
    assert (bh, bw) == (h, w) and (y0 + bh, x0 + bw) == m.shape, "pressed into the bottom right corner"
    holes = S.holes_of(m, 1)
    assert holes[y0 + bh - 2, x0 + bw - 2] and holes[y0 + 1, x0 + 1] and holes[y0 + bh - 2, x0 + 1]


def test_the_background_is_four_connected():
    m = S.corner_and_edge().m
    assert int(S.holes_of(m, 1).sum()) == 9 and int(S.holes_of(m, 2).sum()) == 0
    eight = ndimage.binary_fill_holes(m == 1, structure=np.ones((3, 3), bool)) & (m != 1)
    assert not eight.any(), "with an 8-connected background the corner would open the hole"
    assert m[2, 2] == 0 and m[3, 3] == 0 and m[2, 3] == 1 and m[3, 2] == 1, "two free pixels that meet in a corner only"
    assert m[2, 10] == 0 and m[3, 10] == 0, "the edge opening is 4-connected to the hole"


def test_the_spiral_needs_more_rounds_than_a_word_has_bits():
    o, c = S.spiral(False), S.spiral(True)
    y0, x0, bh, bw = S.boxes(o.m)[1]
    assert bh <= S.WORD and bw <= S.WORD
    assert S.flood_rounds(o.m[y0:y0 + bh, x0:x0 + bw] == 1) > 64
    lab, n = ndimage.label(o.m[y0:y0 + bh, x0:x0 + bw] == 0)
    assert n == 1 and int(S.holes_of(o.m, 1).sum()) == 0, "one channel, open"
    assert int(S.holes_of(c.m, 1).sum()) == c.filled > 1900 and (o.m != c.m).sum() == 1, "closed by one pixel, all of it a hole"


# ---- A.2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(65, 65), (64, 65), (65, 64), (128, 128), (129, 129), (192, 193), (256, 256), (256, 10), (10, 256)])
def test_mid_boxes_have_their_holes_on_and_across_the_seams(h, w):
    m = S.mid_box(h, w).m
    y0, x0, bh, bw = S.boxes(m)[1]
    assert (bh, bw) == (h, w) and (bh > S.WORD or bw > S.WORD) and max(bh, bw) <= S.MID
    holes = S.holes_of(m, 1)[y0:y0 + bh, x0:x0 + bw]
    assert sorted(map(tuple, np.argwhere(holes))) == S.seam_holes(h, w)
    lab, n = ndimage.label(holes)
    comp = [np.argwhere(lab == k + 1) for k in range(n)]
    for s in S.SEAMS:
        if s <= h - 2:
            assert any(len(c) == 1 and c[0][0] == s for c in comp), f"a one-pixel hole in row {s}"
        if s <= w - 2:
            assert any(len(c) == 1 and c[0][1] == s for c in comp), f"a one-pixel hole in column {s}"
    for s in (64, 128, 192):
        if s <= w - 2:
            assert any({s - 1, s} <= set(c[:, 1]) and len(set(c[:, 0])) == 1 for c in comp), f"a hole across column seam {s}"
        if s <= h - 2:
            assert any({s - 1, s} <= set(c[:, 0]) and len(set(c[:, 1])) == 1 for c in comp), f"a hole across row seam {s}"


def test_every_channel_is_open_at_one_end_only():
    o, c = S.channels(False).m, S.channels(True).m
    ends = {}
    for l, (y0, x0, bh, bw) in S.boxes(o).items():
        assert {bh, bw} == {9, 256}
        box = o[y0:y0 + bh, x0:x0 + bw] == l
        free = np.argwhere(~box)
        assert len(free) == 255 and ndimage.label(~box)[1] == 1, "one channel through all four words / row blocks"
        border = [(y, x) for y, x in free if y in (0, bh - 1) or x in (0, bw - 1)]
        assert len(border) == 1
        y, x = border[0]
        ends[l] = "right" if x == bw - 1 else "left" if x == 0 else "bottom" if y == bh - 1 else "top"
        assert int(S.holes_of(c, l).sum()) == 254 and int(S.holes_of(o, l).sum()) == 0
    assert sorted(ends.values()) == ["bottom", "left", "right", "top"]


def test_six_mid_labels_with_holes_in_the_fifth_and_sixth():
    m = S.mid_six().m
    b = S.boxes(m)
    assert len(b) == 6 > S.NTHR // 64 and all(bh > S.WORD for _, _, bh, _ in b.values())
    assert all(int(S.holes_of(m, l).sum()) == 7 for l in (1, 2, 3, 4, 5, 6))
    assert all(S.holes_of(m, l)[3 + 64].any() for l in (5, 6)), "also in the second row block"


# ---- A.3 -----------------------------------------------------------------------------------------------------------------
def test_serial_cases():
    b = S.boxes(S.serial_257().m)
    assert b[1][2:] == (257, 12) and b[2][2:] == (256, 12)
    for side in (100, 30):
        for outer_first in (True, False):
            c = S.conflict(side, outer_first)
            outer = 1 if outer_first else 2
            assert (c.m[S.holes_of(c.m, outer)] == 3 - outer).sum() == 20 and S.boxes(c.m)[outer][2:] == (side, side)
            ref = _oracle(c)
            assert ref.max() == 1 and (ref > 0).sum() == side * side, "the inner label vanishes"


def test_nesting_orders():
    a, b = S.nest3(True), S.nest3(False)
    assert np.array_equal(a.m > 0, b.m > 0) and [np.unique(c.m).tolist() for c in (a, b)] == [[0, 1, 2, 3]] * 2
    assert a.m[2, 3] == 1 and b.m[2, 3] == 3 and a.m[25, 30] == 3 and b.m[25, 30] == 1
    for c in (a, b):
        assert (c.m[S.holes_of(c.m, c.m[2, 3])] == 2).any() and (c.m[S.holes_of(c.m, 2)] == c.m[25, 30]).any(), "three deep"
    # at min_size > 0 the first filter renumbers by first raster appearance BEFORE the fill, so the ids as given do not matter: the outer
    # label comes first in both, ends up with everything and is 1 ...
    assert np.array_equal(_oracle(a), _oracle(b)) and _oracle(a).max() == 1
    # ... at min_size <= 0 the fill runs in the order of the ids as given, and the survivor keeps the rank of its id: 1 or 3
    a0, b0 = _oracle(S.nest3(True, 0)), _oracle(S.nest3(False, 0))
    assert np.unique(a0).tolist() == [0, 1] and np.unique(b0).tolist() == [0, 3]
    # rings that cross, both closed: the order decides which of the two is filled, and the maps differ by more than their ids
    cl, cr = S.interlocked("left"), S.interlocked("right")
    assert all(int(S.holes_of(c.m, k).sum()) == 522 for c in (cl, cr) for k in (1, 2)) and cl.min_size == cr.min_size == 0
    l, r = _oracle(cl), _oracle(cr)
    assert not np.array_equal(l > 0, r > 0) and l.max() == r.max() == 2
    assert (l == 1).sum() == 196 + 522 == (r == 1).sum() and (l == 2).sum() == 196 - 50 == (r == 2).sum()
    assert l[6, 6] == 1 and r[6, 6] == 2, "the filled ring is the left one, then the right one"
    u, f = _oracle(S.interlocked("right", 1)), _oracle(S.interlocked("right", 1, True))
    assert np.array_equal(u > 0, l > 0) and np.array_equal(f[::-1] > 0, r > 0), "min_size = 1: the raster order decides"


# ---- A.4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_size", [1, 2, 15, 16])
def test_size_cases_sit_on_the_threshold(min_size):
    c = S.sizes(min_size)
    areas = np.bincount(c.m.ravel())[1:]
    assert min_size in areas and (min_size == 1 or min_size - 1 in areas)
    assert sorted(np.bincount(_oracle(c).ravel())[1:]) == sorted(a for a in areas if a >= min_size)


def test_the_positional_quirk_shows_with_and_without_background():
    for bg in (True, False):
        c = S.quirk(bg)
        ids = np.unique(c.m)
        assert (ids[0] == 0) == bg and (np.diff(ids[ids > 0]) > 1).any(), "gaps"
        assert not np.array_equal(_oracle(c), _naive(c.m, c.min_size)), "the reference does not remove the labels below min_size"


def test_small_label_in_a_hole_leaves_a_plain_hole():
    c = S.small_in_hole()
    assert (c.m == 2).sum() == 14 < c.min_size and (c.m[S.holes_of(c.m, 1)] == 2).sum() == 14
    after = np.where(c.m == 2, 0, c.m)
    assert S.path_of(after) == "small" and (_oracle(c) > 0).sum() == 20 * 20


def test_reverse_appearance():
    c = S.reverse_appearance()
    ids, first = np.unique(c.m.ravel(), return_index=True)
    assert np.all(np.diff(first[1:]) < 0), "the larger the id, the earlier its first pixel"
    ref = _oracle(c)
    assert [int(ref[c.m == l][0]) for l in range(1, 7)] == [6, 5, 4, 3, 2, 1]


@pytest.mark.parametrize("vmax", [1023, 1024, 1025, 2047, 2048, 2049])
def test_slice_cases(vmax):
    c = S.slices(vmax)
    assert c.m.shape == (S.SLICE_TILE, S.SLICE_TILE) and c.m.max() == vmax and c.min_size == 2
    areas = np.bincount(c.m.ravel())[1:]
    assert set(areas) == {0, 1, 2} and (c.m == 0).any()
    per = (vmax + S.SIZE_FILTER_THREADS) // S.SIZE_FILTER_THREADS
    assert per == {1023: 1, 1024: 2, 1025: 2, 2047: 2, 2048: 3, 2049: 3}[vmax]
    last = (vmax - 1) // per
    assert areas[last * per:vmax].any() and (last == S.SIZE_FILTER_THREADS - 1 or last < S.SIZE_FILTER_THREADS - 1), "the last slice has a label"
    assert not np.array_equal(_oracle(c), _naive(c.m, 2)), "positions, not values: the ranks matter"


def test_min_size_zero_and_below_ranks_the_ids():
    for s in (0, -1):
        a, b = _oracle(S.nonpositive(s, False)), _oracle(S.nonpositive(s, True))
        assert np.array_equal(a, b) and np.unique(b).tolist() == [0, 1, 2, 3], "ids {2, 5, 9} come back as {1, 2, 3}"
    two = np.zeros((4, 8), np.uint16)
    two[1, 1:3], two[2, 4:7] = 2, 5
    assert np.unique(dynamics.fill_holes_and_remove_small_masks(two, 0)).tolist() == [0, 1, 2]
    c = S.nonpositive(0, True, True)
    assert np.unique(c.m).tolist() == [0, 2, 5, 9, 13] and (c.m[S.holes_of(c.m, 5)] == 13).sum() == 6
    assert np.unique(_oracle(c)).tolist() == [0, 1, 2, 3] and c.nlab == 4, "the overwritten label still counts"


# ---- A.5, A.6 ------------------------------------------------------------------------------------------------------------
def test_odd_tile_geometry():
    m = S.odd_tile().m
    H, W = m.shape
    assert (H, W) == (67, 93) and W % S.RUN_PX and (H * W) % S.WG_PX
    assert m[10, W - 1] == 3 == m[11, 0] and m[10, W - 2] != 3 and m[11, 1] != 3
    assert m[H - 1, W - 1] == 12 and (H * W) % S.RUN_PX, "the last thread's run is cut by the end of the tile"
    flat = m.ravel()
    assert flat[S.WG_PX - 1] == 7 == flat[S.WG_PX + W - 1] and S.boxes(m)[7][0] * W < S.WG_PX
    assert np.unique(m).tolist() == [0, 1, 3, 6, 7, 12, 13]


def test_batch_tiles():
    m, paths = S.batch_tiles()
    assert m.shape == (8,) + S.BATCH_HW and m.max() < S.max_labels(*S.BATCH_HW) and m.min() == 0
    assert [S.path_of(t) for t in m] == paths == ["none", "small", "small", "mid", "serial", "serial", "small", "small"]
    assert not m[0].any() and not (m[1] == 0).any() and len(np.unique(m[6])) == 2001 and len(np.unique(m[7])) == 2
    assert (m[4][S.holes_of(m[4], 2)] == 1).any() and max(S.boxes(m[5])[1][2:]) > S.MID
    assert all(1 in np.bincount(t.ravel()) for t in (m[1], m[2], m[4], m[6])), "one-pixel labels for min_size = 2 to remove"


# ---- B -------------------------------------------------------------------------------------------------------------------
def test_the_wide_label_sums_past_two_to_the_32():
    m = S.wide_label()
    assert m.shape == (48, 16384) and (m == 1).sum() == 40 * 16384
    want = 40 * (16383 * 16384 // 2)
    assert want > 2 ** 32 and abs(want - 5.4e9) < 1e8
    xs = np.nonzero(m)[1].astype(np.int64)
    assert int(xs.sum()) == want
    cm = S.class_map_of(S.odd_tile().m)
    assert all(len(np.unique(cm[S.odd_tile().m == l])) == 1 for l in (1, 3, 6, 7, 12, 13)) and cm.max() <= 6


# ---- C -------------------------------------------------------------------------------------------------------------------
def _stages(dP, cp):
    out, st = dynamics.compute_masks(dP, cp, flow_threshold=None, return_stages=True)
    return out, st["masks_flowfiltered"]


@pytest.mark.parametrize("side", list(S.RING_SIDES))
@pytest.mark.parametrize("inner", [False, True])
def test_ring_fields_reach_the_fill_as_a_ring(side, inner):
    m, (dP, cp) = S.ring_field(side, inner)
    T, hole = int(1.7 * side) + 8, S.RING_SIDES[side]
    out, sm = _stages(dP, cp)
    assert m.shape == (T, T) and side * side - hole * hole <= 0.4 * T * T
    b = S.boxes(sm)
    assert sm.max() == (2 if inner else 1) and b[1][2:] == (side, side) and (sm == 1).sum() == side * side - hole * hole
    holes = S.holes_of(sm, 1)
    y, x = np.argwhere(holes).min(0)
    assert holes.sum() == hole * hole and holes[y:y + hole, x:x + hole].all(), "a square hole"
    assert (sm[holes] != 0).sum() == (16 if inner else 0) and (not inner or ((sm == 2).sum() == 16 and b[2][2:] == (4, 4)))
    assert (sm == 0).any() and out.max() == 1 and (out == 1).sum() == side * side and S.boxes(out)[1][2:] == (side, side)


def test_bar_fields():
    m, (dP, cp) = S.bars_field()
    out, sm = _stages(dP, cp)
    assert m.shape == (64, 64) and np.bincount(sm.ravel())[1:].tolist() == list(S.BAR_AREAS) == [11, 12, 13, 14, 15, 16, 14, 15]
    assert np.bincount(out.ravel())[1:].tolist() == [15, 16, 15]


@pytest.mark.parametrize("name", list(S.GRIDS))
def test_grid_fields(name):
    build, n_stage, n_small, bg, n_out = S.GRIDS[name]
    out, sm = _stages(*build())
    areas = np.bincount(sm.ravel())[1:]
    assert sm.max() == len(areas) == n_stage and (areas < 15).sum() == n_small and set(areas) <= {12, 14, 36}
    assert bool((sm == 0).any()) == bg and out.max() == n_out
    assert (n_stage > S.TAIL_LDS) == name.startswith(("192x198", "192x194")) or n_stage == S.TAIL_LDS
    if not bg and n_small:
        assert n_out == n_stage - 2 * n_small and (np.bincount(out.ravel())[1:] == 36).all(), "off by one: a whole cell goes for every small one"
