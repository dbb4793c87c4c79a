"""Hand-built id maps and network fields for the hole fill, the two size filters, the renumbering and the per-cell records
(csrc/cpx_postproc.hip: k_size_filter, k_fill_parallel, fill_label_big, fill_serial_body, k_first, k_renumber_rank, tail_rank,
k_rec_stats, k_rec_write, the tails of k_count_labels_f and k_finish_f).  Builders only: nothing here calls the code under test.
Every property a case is named for is proved on the CPU by tests/test_fill_shapes_host.py, with the oracle and scipy alone, and
the kernel constants restated below are compared there with the source text.

A stage case is ``Case(m, min_size, path, filled, nlab)``: the map(s), the min_size it is run with, the fill path the tile
takes on the device (decided by `path_of` from boxes and holes alone), the number of background pixels the oracle turns into
labels, and the label count the entry reports.  Every id satisfies 0 <= id < max_labels(H, W)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np
from scipy import ndimage

WORD = 64               # k_fill_parallel: one 64-bit word per row, one lane per row; boxes up to WORD x WORD
MID = 256               # fill_label_big: four words per row, four rows per lane; boxes up to MID x MID
TAIL_LDS = 1024         # tail_rank: up to this many labels by comparison through LDS, above by bitmap
NTHR = 256              # the workgroup of the pixel passes and of the fused tails (per-thread label slices)
SIZE_FILTER_THREADS = 1024      # k_size_filter's workgroup (per-thread label slices)
RUN_PX = 8              # pixels per thread of the run passes
WG_PX = NTHR * RUN_PX   # = 2 048 pixels per workgroup
SEAMS = (63, 64, 127, 128, 191, 192)        # the last / first column of a row word, the last / first row of a row block

Case = namedtuple("Case", "m min_size path filled nlab")


def max_labels(H, W):
    return H * W // 11 + 2


def blank(H, W):
    return np.zeros((H, W), np.int32)


def solid(m, y0, x0, h, w, lab):
    m[y0:y0 + h, x0:x0 + w] = lab


def ring(m, y0, x0, h, w, lab, t=1):
    m[y0:y0 + h, x0:x0 + w] = lab
    m[y0 + t:y0 + h - t, x0 + t:x0 + w - t] = 0


# ---- what the host test measures ---------------------------------------------------------------------------------------
def boxes(m):
    """{id: (y0, x0, bh, bw)}"""
    return {i + 1: (s[0].start, s[1].start, s[0].stop - s[0].start, s[1].stop - s[1].start)
            for i, s in enumerate(ndimage.find_objects(m)) if s is not None}


def holes_of(m, lab):
    """the pixels of `lab`'s holes (4-connected background, scipy's default), as a full-size mask"""
    own = m == lab
    return ndimage.binary_fill_holes(own) & ~own


def path_of(m):
    """the device's route for a tile from its boxes and holes: 'serial' (a box above MID, or a hole that holds another id),
    'mid' (a box above WORD), 'small', or 'none' (no label)"""
    b = boxes(m)
    if not b:
        return "none"
    if any(bh > MID or bw > MID for _, _, bh, bw in b.values()) or any((m[holes_of(m, l)] != 0).any() for l in b):
        return "serial"
    return "mid" if any(bh > WORD or bw > WORD for _, _, bh, bw in b.values()) else "small"


def flood_rounds(own):
    """rounds of the device's flood on one box: seeds on the box border, then per round one row up / down and a whole-row fill"""
    free = ~own
    runs, n = ndimage.label(free, structure=[[0, 0, 0], [1, 1, 1], [0, 0, 0]])

    def hfill(o):
        hit = np.zeros(n + 1, bool)
        hit[runs[o]] = True
        hit[0] = False
        return hit[runs]
    o = np.zeros_like(free)
    o[0], o[-1], o[:, 0], o[:, -1] = free[0], free[-1], free[:, 0], free[:, -1]
    o, k = hfill(o), 0
    while True:
        nn = o.copy()
        nn[1:] |= o[:-1] & free[1:]
        nn[:-1] |= o[1:] & free[:-1]
        nn = hfill(nn)
        k += 1
        if np.array_equal(nn, o):
            return k
        o = nn


# ---- A.1 the small path ------------------------------------------------------------------------------------------------
def small_boxes_at_edges():
    """3 x 3 rings pressed against every corner and edge of the tile, a 1 x 1, a 1 x 9 and a 9 x 1 label"""
    m = blank(40, 50)
    for k, (y, x) in enumerate([(0, 0), (0, 47), (37, 0), (37, 47), (0, 20), (37, 20), (18, 0), (18, 47)]):
        ring(m, y, x, 3, 3, k + 1)
    m[10, 10] = 9
    m[12, 10:19] = 10
    m[14:23, 30] = 11
    return Case(m, 1, "small", 8, 11)


def small_ring(h, w):
    """an h x w ring of thickness 1 (the hole reaches column bw - 2 and row bh - 2) around an island of itself, pressed
    into the tile's bottom right corner"""
    m = blank(h + 2, w + 3)
    ring(m, 2, 3, h, w, 1)
    solid(m, 2 + h // 2 - 3, 3 + w // 2 - 4, 5, 7, 1)
    return Case(m, 1, "small", (h - 2) * (w - 2) - 35, 1)


def corner_and_edge():
    """id 1: a 5 x 5 ring without its corner pixel -- the hole meets the outside through a diagonal only and is filled (the
    background is 4-connected).  id 2: the same ring without an edge pixel -- the hole is open and stays background."""
    m = blank(9, 16)
    ring(m, 2, 2, 5, 5, 1)
    m[2, 2] = 0
    ring(m, 2, 9, 5, 5, 2)
    m[2, 10] = 0
    return Case(m, 1, "small", 9, 2)


def spiral(closed, h=63, w=64):
    """an h x w block with a one-pixel channel that spirals inwards from an entrance at column 0; closed: the entrance is label"""
    m = blank(h + 2, w + 2)
    b = np.ones((h, w), np.int32)
    top, bot, left, right = 1, h - 2, 1, w - 2
    b[top, 0:right + 1] = 0
    while bot - top >= 2 and right - left >= 2:
        b[top:bot + 1, right] = 0
        b[bot, left:right + 1] = 0
        top += 2
        if bot - top < 2:
            break
        b[top:bot + 1, left] = 0
        right -= 2
        if right - left < 2:
            break
        b[top, left:right + 1] = 0
        bot -= 2
        left += 2
    if closed:
        b[1, 0] = 1
    m[1:1 + h, 1:1 + w] = b
    return Case(m, 1, "small", int((b == 0).sum()) if closed else 0, 1)


# ---- A.2 the mid path --------------------------------------------------------------------------------------------------
def seam_holes(h, w):
    """hole pixels (box coordinates) of an h x w box: one-pixel holes in the seam rows and the seam columns, and two-pixel
    holes across every seam, wherever the box has them in its interior"""
    px = set()
    for i, s in enumerate(SEAMS):
        c = 3 + 2 * (i % 3)
        if s <= h - 2 and c <= w - 2:
            px.add((s, c))
        if s <= w - 2 and c <= h - 2:
            px.add((c, s))
    for s in (64, 128, 192):                    # (row / column 1: next to the box's wall, clear of the one-pixel holes)
        if s <= w - 2:
            px |= {(1, s - 1), (1, s)}
        if s <= h - 2:
            px |= {(s - 1, 1), (s, 1)}
    return sorted(px)


def mid_box(h, w):
    m = blank(h + 5, w + 7)
    solid(m, 2, 3, h, w, 1)
    px = seam_holes(h, w)
    for y, x in px:
        m[2 + y, 3 + x] = 0
    return Case(m, 1, "mid", len(px), 1)


def channels(closed):
    """four 256-pixel bars with a one-pixel channel along them.  Open, each channel meets the outside at ONE end only: the right
    (what reaches the words to the left is the right-to-left carry of row_fill), the left, the bottom (dn_blk) and the top
    (up_blk); all of it stays background.  Closed, all of it is filled."""
    m = blank(300, 300)
    for k, (y, x) in enumerate([(2, 3), (14, 3)]):
        solid(m, y, x, 9, 256, k + 1)
        m[y + 4, x + 1:x + 255] = 0
    for k, (y, x) in enumerate([(30, 5), (30, 20)]):
        solid(m, y, x, 256, 9, k + 3)
        m[y + 1:y + 255, x + 4] = 0
    if not closed:
        m[6, 3 + 255] = 0
        m[18, 3] = 0
        m[30 + 255, 9] = 0
        m[30, 24] = 0
    return Case(m, 1, "mid", 4 * 254 if closed else 0, 4)


def mid_six():
    """six 66 x 10 labels with holes in one tile: the mid path hands them to four waves in turn, so the fifth and sixth are
    second labels of waves 0 and 1"""
    m = blank(72, 90)
    for k in range(6):
        solid(m, 3, 2 + 14 * k, 66, 10, k + 1)
        m[10 + 9 * k:12 + 9 * k, 5 + 14 * k:8 + 14 * k] = 0
        m[3 + 64, 6 + 14 * k] = 0
    return Case(m, 1, "mid", 6 * 7, 6)


# ---- A.3 the serial path -----------------------------------------------------------------------------------------------
def serial_257():
    m = blank(262, 32)
    solid(m, 2, 2, 257, 12, 1)
    solid(m, 2, 17, 256, 12, 2)
    for y in (5, 63, 64, 130, 254):
        m[2 + y, 6:9] = 0
        m[2 + y, 20:24] = 0
    return Case(m, 1, "serial", 5 * 7, 2)


def conflict(side, outer_first):
    """a ring of `side` pixels whose hole holds another label; the reference fills label by label, so the inner one vanishes"""
    m = blank(side + 6, side + 4)
    a, b = (1, 2) if outer_first else (2, 1)
    ring(m, 3, 2, side, side, a, 3)
    solid(m, 3 + side // 2 - 2, 2 + side // 2 - 2, 4, 5, b)
    return Case(m, 1, "serial", (side - 6) ** 2 - 20, 1)


def nest3(outer_first, min_size=1):
    """ring in ring around a block, with background between them; ids 1, 2, 3 from the outside in, or from the inside out"""
    m = blank(80, 84)
    a, b, c = (1, 2, 3) if outer_first else (3, 2, 1)
    ring(m, 2, 3, 70, 75, a, 2)
    ring(m, 12, 14, 40, 45, b, 2)
    solid(m, 25, 30, 8, 9, c)
    bg_inside = 66 * 71 - (40 * 45 - 36 * 41) - 72
    return Case(m, min_size, "serial", bg_inside, 1 if min_size > 0 else 3)


def interlocked(first, min_size=0, flip=False):
    """two rings that cross, each closed on its own (a diagonal joint closes a ring against the 4-connected background): whichever
    id is lower is filled first and cuts the other ring open, which then has no hole.  That is the order of the ids as given only at
    min_size <= 0: above, the first filter renumbers by first raster appearance before the fill, so there the raster order decides
    (flip: upside down, the right ring comes first)"""
    m = blank(40, 60)
    a, b = (1, 2) if first == "left" else (2, 1)
    ring(m, 5, 5, 24, 30, a, 2)                 # the left ring: rows 5 .. 28, columns 5 .. 34
    rb = blank(40, 60)
    ring(rb, 12, 22, 24, 30, 1, 2)              # the right ring: rows 12 .. 35, columns 22 .. 51
    m[rb > 0] = b
    m[12, 33] = m[13, 34] = m[27, 22] = m[28, 23] = a       # the two 2 x 2 crossings, shared diagonally: both rings stay closed
    return Case(m[::-1].copy() if flip else m, min_size, "serial", 522 - 50, 2)


# ---- A.4 size filter and renumbering -----------------------------------------------------------------------------------
def sizes(min_size):
    """bars of min_size - 1, min_size and min_size + 1 pixels, contiguous ids, with background"""
    m = blank(8, 40)
    areas = [a for a in (min_size - 1, min_size, min_size + 1, min_size - 1, min_size) if a > 0]
    for k, a in enumerate(areas):
        m[1 + k, 2:2 + a] = k + 1
    return Case(m, min_size, None, 0, sum(a >= min_size for a in areas))


def quirk(background):
    """id gaps: the reference removes the label whose VALUE is the position of a small count, with the background's count
    dropped from the front -- or, in a tile without background, the first label's"""
    m = blank(12, 40)
    if background:
        m[1:6, 1:6] = 1
        m[1:6, 10:15] = 2
        m[1:6, 20:25] = 4
        m[1:3, 30:33] = 5
        m[7:11, 1:7] = 7
        m[7:9, 10:13] = 9
    else:                                       # four stripes and two short pieces on the tile's edge (no piece lies in a hole)
        for k, l in enumerate((2, 3, 8, 9)):
            m[:, 10 * k:10 * k + 10] = l
        m[0, 10:15] = 5
        m[11, 33:37] = 12
    return Case(m, 15, None, None, None)


def small_in_hole():
    """a 14-pixel label in the hole of a ring: the first filter removes it, the hole is then plain and the small path fills it"""
    m = blank(30, 30)
    ring(m, 4, 4, 20, 20, 1, 3)
    m[12:14, 10:17] = 2
    return Case(m, 15, "serial", 14 * 14 - 14, 1)


def reverse_appearance():
    m = blank(20, 30)
    for k in range(6):
        m[1 + 3 * k:4 + 3 * k, 2:22] = 6 - k
    m[2, 5:9] = 0
    return Case(m, 15, "small", 4, 6)


SLICE_TILE = 160


def slices(vmax):
    """one- and two-pixel labels, ids up to vmax with every seventh id absent, min_size = 2: the ranks that decide which label
    VALUE goes are sums over the per-thread label slices"""
    m = blank(SLICE_TILE, SLICE_TILE)
    for k in range(1, vmax + 1):
        if k % 7 == 3 and k != vmax:
            continue
        y, x = 2 * ((k - 1) // 50), 3 * ((k - 1) % 50)
        m[y, x] = k
        if k % 3:
            m[y, x + 1] = k
    return Case(m, 2, None, 0, None)


def nonpositive(min_size, gapped, nested=False):
    """min_size <= 0: no filter; ids with gaps come back as 1..n in the order of their values"""
    m = blank(30, 40)
    ids = (2, 5, 9) if gapped else (1, 2, 3)
    ring(m, 2, 2, 10, 12, ids[1], 2)
    ring(m, 15, 4, 9, 9, ids[0])
    solid(m, 3, 20, 4, 4, ids[2])
    m[25, 1] = ids[2]
    filled = 6 * 8 + 49
    if nested:
        solid(m, 5, 5, 2, 3, ids[2] + 4)
        filled -= 6
    return Case(m, min_size, "serial" if nested else "small", filled, 4 if nested else 3)


# ---- A.5 geometry of the run passes ------------------------------------------------------------------------------------
def odd_tile():
    """67 x 93: W is no multiple of RUN_PX and H * W none of WG_PX; id 3 on the last pixel of a row and the first of the next;
    (its box is therefore the whole width, which selects the mid path); id 7 crosses the first workgroup's last pixel; id 12 ends at
    the tile's last pixel; ids with gaps"""
    m = blank(67, 93)
    ring(m, 1, 1, 12, 20, 1, 2)
    m[10, 92] = 3
    m[11, 0] = 3
    m[8:10, 90:92] = 3
    ring(m, 20, 70, 30, 23, 6, 4)
    solid(m, 22, 0, 2048 // 93 + 3, 9, 7)           # crosses the first workgroup's last pixel
    m[30, 3] = 0
    m[66, 80:93] = 12
    m[64:66, 88:93] = 12
    solid(m, 60, 2, 5, 5, 13)
    m[62, 4] = 0
    return Case(m, 1, "mid", 8 * 16 + 22 * 15 + 2, 6)


# ---- A.6 a batch with another path in every tile -----------------------------------------------------------------------
BATCH_HW = (264, 100)
BATCH_MIN_SIZE = 2


def batch_tiles():
    """[8, 264, 100] and the path of every tile: empty, no background at all, small only, mid only, conflict, a box above
    256, 2 000 labels, one label"""
    H, W = BATCH_HW
    t = [blank(H, W) for _ in range(8)]
    k = 0
    for y in range(0, H, 24):                       # 1: 55 cells of 24 x 20, no background; two of them cut into pieces of 1 and 2 pixels
        for x in range(0, W, 20):
            k += 1
            t[1][y:y + 24, x:x + 20] = k
    t[1][0, 0] = 56
    t[1][24, 45:47] = 57
    t[1][100, 99] = 58
    for i in range(5):                              # 2: small rings, one single pixel
        ring(t[2], 5 + 50 * i, 10 + 5 * i, 30 + 8 * i, 40 + 5 * i, 5 - i, 2)
    t[2][3, 3] = 6
    ring(t[3], 10, 5, 200, 90, 1, 5)                # 3: mid, with islands and seam holes
    solid(t[3], 60, 30, 20, 30, 1)
    t[3][73:75, 40:50] = 0
    t[3][250:252, 5:80] = 2
    ring(t[4], 20, 20, 40, 40, 2, 3)                # 4: a hole that holds another label
    solid(t[4], 35, 35, 5, 5, 1)
    solid(t[4], 100, 10, 1, 1, 3)
    solid(t[5], 2, 40, 260, 12, 1)                  # 5: a box above 256
    t[5][100:103, 44:48] = 0
    ring(t[5], 10, 60, 30, 30, 2)
    for k in range(1, 2001):                        # 6: 2 000 labels of one, two or three pixels
        y, x = 2 * ((k - 1) // 33), 3 * ((k - 1) % 33)
        t[6][y, x:x + 1 + k % 3] = k
    ring(t[7], 100, 30, 30, 30, 1, 4)               # 7: one label
    paths = ["none", "small", "small", "mid", "serial", "serial", "small", "small"]
    return np.stack(t), paths


STAGE_CASES = {
    "small_boxes_at_edges": small_boxes_at_edges,
    **{f"small_ring_{h}x{w}": (lambda h=h, w=w: small_ring(h, w)) for h, w in ((63, 63), (64, 64), (63, 64), (64, 63))},
    "corner_and_edge": corner_and_edge,
    "spiral_open": lambda: spiral(False),
    "spiral_closed": lambda: spiral(True),
    **{f"mid_box_{h}x{w}": (lambda h=h, w=w: mid_box(h, w))
       for h, w in ((65, 65), (64, 65), (65, 64), (128, 128), (129, 129), (192, 193), (256, 256), (256, 10), (10, 256))},
    "channels_open": lambda: channels(False),
    "channels_closed": lambda: channels(True),
    "mid_six": mid_six,
    "serial_257": serial_257,
    "mid_conflict_outer_first": lambda: conflict(100, True),
    "mid_conflict_inner_first": lambda: conflict(100, False),
    "small_conflict_outer_first": lambda: conflict(30, True),
    "small_conflict_inner_first": lambda: conflict(30, False),
    "nest3_outer_first": lambda: nest3(True),
    "nest3_inner_first": lambda: nest3(False),
    "nest3_outer_first_min0": lambda: nest3(True, 0),
    "nest3_inner_first_min0": lambda: nest3(False, 0),
    "interlocked_left_first": lambda: interlocked("left"),
    "interlocked_right_first": lambda: interlocked("right"),
    "interlocked_min1": lambda: interlocked("right", 1),
    "interlocked_min1_flipped": lambda: interlocked("right", 1, True),
    **{f"sizes_{s}": (lambda s=s: sizes(s)) for s in (1, 2, 15, 16)},
    "quirk_with_background": lambda: quirk(True),
    "quirk_without_background": lambda: quirk(False),
    "small_in_hole": small_in_hole,
    "reverse_appearance": reverse_appearance,
    **{f"slices_{v}": (lambda v=v: slices(v)) for v in (1023, 1024, 1025, 2047, 2048, 2049)},
    **{f"min{s}_{'gapped' if g else 'contiguous'}": (lambda s=s, g=g: nonpositive(s, g)) for s in (0, -1) for g in (False, True)},
    "min0_gapped_nested": lambda: nonpositive(0, True, True),
    "odd_tile": odd_tile,
}


# ---- B records -----------------------------------------------------------------------------------------------------------
WIDE_HW = (48, 16384)


def wide_label():
    """one label over 40 full rows of a 48 x 16 384 tile: sum_x = 40 * 16 383 * 16 384 / 2 > 2^32"""
    m = np.zeros(WIDE_HW, np.uint16)
    m[3:43] = 1
    return m


def class_map_of(m):
    """a class map that is constant on every label and differs between neighbours in id"""
    return ((m.astype(np.int64) * 5 + 1) % 7 * (m > 0)).astype(np.uint8)


# ---- C fields for both chains ----------------------------------------------------------------------------------------------
def sink_field(m, sinks):
    """dP = 5 * (sink + 0.5 - pixel) and cellprob = 1 on the pixels of every label of the hand map `m`, cellprob = -1 elsewhere;
    sinks: {id: (sy, sx)}, the 2 x 2 block at the sink inside the label"""
    H, W = m.shape
    yy, xx = np.mgrid[:H, :W].astype(np.float32)
    dP = np.zeros((2, H, W), np.float32)
    for l, (sy, sx) in sinks.items():
        assert (m[sy:sy + 2, sx:sx + 2] == l).all()
        on = m == l
        dP[0][on] = (5.0 * (sy + 0.5 - yy))[on]
        dP[1][on] = (5.0 * (sx + 0.5 - xx))[on]
    cp = np.where(m > 0, 1.0, -1.0).astype(np.float32)
    return dP, cp


RING_SIDES = {64: 20, 65: 20, 129: 40, 193: 60, 256: 80, 257: 80}      # ring side: hole side


def ring_field(side, inner):
    """a square ring with a square hole, and with `inner` a 4 x 4 label in the hole"""
    T = int(1.7 * side) + 8
    m = blank(T, T)
    o, hole = (T - side) // 2, RING_SIDES[side]
    solid(m, o, o, side, side, 1)
    ho = o + (side - hole) // 2
    solid(m, ho, ho, hole, hole, 0)
    sinks = {1: (o + 4, o + side // 2)}
    if inner:
        solid(m, ho + hole // 2 - 2, ho + hole // 2 - 2, 4, 4, 2)
        sinks[2] = (ho + hole // 2 - 1, ho + hole // 2 - 1)
    return m, sink_field(m, sinks)


BAR_AREAS = (11, 12, 13, 14, 15, 16, 14, 15)


def bars_field():
    """eight bars of two rows on a 64 x 64 tile, of 11 .. 16 pixels: min_size = 15 keeps three"""
    m = blank(64, 64)
    sinks = {}
    for k, a in enumerate(BAR_AREAS):
        y, x = 4 + 7 * k, 5 + 3 * k
        m[y, x:x + (a + 1) // 2] = k + 1
        m[y + 1, x:x + a // 2] = k + 1
        sinks[k + 1] = (y, x + 1)
    return m, sink_field(m, sinks)


def grid_field(H, W, trim=(), tiny=(), off=()):
    """sinks on a 6-pixel grid (the (centre - pixel) * 2.5 field), everything foreground but: cells in `trim` keep 14 of their
    36 pixels, cells in `tiny` 9 (too few for a seed, so they never become a label), cells in `off` none.  Cells are (row,
    column) of the grid."""
    g = 6
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    cy, cx = (np.floor(yy / g) * g + (g - 1) / 2), (np.floor(xx / g) * g + (g - 1) / 2)
    dP = np.stack([(cy - yy) * 2.5, (cx - xx) * 2.5]).astype(np.float32)
    cp = np.ones((H, W), np.float32)
    for r, c in off:
        cp[g * r:g * r + g, g * c:g * c + g] = -1.0
    for r, c in tiny:
        cp[g * r:g * r + g, g * c:g * c + g] = -1.0
        cp[g * r + 1:g * r + 4, g * c + 1:g * c + 4] = 1.0
    for r, c in trim:
        cp[g * r:g * r + g, g * c:g * c + g] = -1.0
        cp[g * r + 1:g * r + 5, g * c + 1:g * c + 5] = 1.0          # 16 pixels around the sink ...
        cp[g * r + 1, g * c + 1] = cp[g * r + 4, g * c + 4] = -1.0       # ... less two corners
    return dP, cp


# name: (builder of (dP, cellprob), labels of the stage map, of which below min_size = 15, background present, labels of the result)
# (a tile whose width is no multiple of 6 ends in a column of 6 x 2 cells: labels of 12 pixels WITHOUT any background, so the filter's
# positions are off by one and it removes as many whole cells besides)
GRIDS = {
    "192x192": (lambda: grid_field(192, 192), 1024, 0, False, 1024),
    "192x198": (lambda: grid_field(192, 198), 1056, 0, False, 1056),
    "192x198_trim3": (lambda: grid_field(192, 198, trim=((7, 7),), tiny=((0, 5), (31, 32))), 1054, 1, True, 1053),
    "96x96_trim1": (lambda: grid_field(96, 96, trim=((3, 4),)), 256, 1, True, 255),
    "96x102": (lambda: grid_field(96, 102), 272, 0, False, 272),
    "96x98": (lambda: grid_field(96, 98), 272, 16, False, 240),
    "192x194": (lambda: grid_field(192, 194), 1056, 32, False, 992),
    "96x96_off1": (lambda: grid_field(96, 96, off=((2, 9),)), 255, 0, True, 255),
    "96x102_off15": (lambda: grid_field(96, 102, off=tuple((5, c) for c in range(15))), 257, 0, True, 257),
    "192x198_off31": (lambda: grid_field(192, 198, off=tuple((9, c) for c in range(31))), 1025, 0, True, 1025),
}
