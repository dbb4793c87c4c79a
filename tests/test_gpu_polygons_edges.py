"""GPU: the device polygoniser (csrc/cpx_polygons.hip: k_poly_count, k_poly_scan, k_poly_write, pg_ring_is_valid) at the
boundaries its one-wave-per-instance form has -- 64-lane chunks of the local-top search, the visited-border skip between a
label's components, the lane-strided partners / 16-edge votes / wrap pair of the validity test, more than 1024 records
per tile in the scan, a vertex pool that is too small, hostile records, labels >= 32768, tile edges, odd widths, a
non-dyadic scale with large origins, workspace reuse.

Every result is compared bit for bit with the host polygoniser (cpx_polygonize_host), with oracle/polygons.py (contour and
validity of every cell; area exact, perimeter to 1e-12 relative, centroid to 1e-9 for valid cells: the tolerances of
tests/test_gpu_polygons.py) and with the literal vertex counts and validities the maps of tests/polygon_shapes.py were
built for (tests/test_polygon_shapes_host.py pins those on the CPU).  Records are built in numpy, so that hostile ones and
more labels than cpx_postproc_max_labels can be fed; cpx_instance_records is cross-checked against the same numpy rows.
All output buffers carry a sentinel-filled guard behind them, and every call checks it."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import polygon_shapes as ps
from classpose_amd import _lib, engine, postprocess
from classpose_amd._lib import ptr

pytestmark = pytest.mark.gpu

CELL, REC = engine.CELL_DTYPE, engine.RECORD_DTYPE
FIELDS = ("area", "perimeter", "cx", "cy", "n_pts", "valid", "cls", "offset")
SENTINEL = 0xA5
GUARD_CELLS, GUARD_PTS, GUARD_WS = 64, 256, 256


def _alloc(cuda, nT, H, W, max_rec, max_pts):
    L = _lib.lib()
    ws_bytes = L.cpx_polygonize_workspace_bytes(nT, H, W, max_rec)
    return types.SimpleNamespace(
        key=(nT, H, W, max_rec, max_pts), ws_bytes=ws_bytes,
        cells=torch.full(((nT * max_rec + GUARD_CELLS) * CELL.itemsize,), SENTINEL, dtype=torch.uint8, device=cuda),
        pool=torch.full(((max_pts + GUARD_PTS) * 16,), SENTINEL, dtype=torch.uint8, device=cuda),
        tot=torch.full((1 + 16,), -1, dtype=torch.int32, device=cuda),
        ws=torch.full((ws_bytes + GUARD_WS,), 0xFF, dtype=torch.uint8, device=cuda))         # a dirty workspace: the call clears what it needs


def _poly(cuda, maps, recs, counts=None, max_rec=None, max_pts=None, scale=1.0, origins=None, bufs=None):
    """cpx_polygonize_device on maps [nT, H, W] uint16 with recs = one numpy RECORD_DTYPE array per tile (the records buffer
    holds exactly nT * max_rec rows; counts default to the arrays' lengths).  Returns cells [nT, max_rec] (raw, unwritten
    slots included), xy [max_pts, 2], total and per tile the written rows.  The guards behind every buffer are asserted here,
    on every call; that the cell slots past a tile's records and the pool rows no cell owns are untouched is asserted only
    when the buffers are fresh (bufs = None): reused ones hold an earlier call's rows there."""
    maps = np.ascontiguousarray(maps, dtype=np.uint16)
    nT, H, W = maps.shape
    counts = [len(r) for r in recs] if counts is None else list(counts)
    max_rec = max(1, max(len(r) for r in recs)) if max_rec is None else max_rec
    if max_pts is None:
        max_pts = max(1, sum(int(c["n_pts"].sum()) for c in (postprocess.polygonize_tile(maps[t], recs[t], 1.0, (0, 0))[0] for t in range(nT))))
    origins = np.zeros((nT, 2)) if origins is None else np.asarray(origins, np.float64).reshape(nT, 2)
    table = np.zeros((nT, max_rec), REC)
    for t, r in enumerate(recs):
        assert len(r) <= max_rec
        table[t, :len(r)] = r
        table["tile"][t, :len(r)] = t
    fresh = bufs is None
    if fresh:
        bufs = _alloc(cuda, nT, H, W, max_rec, max_pts)
    assert bufs.key == (nT, H, W, max_rec, max_pts)
    d_maps = torch.from_numpy(maps.view(np.int16)).to(cuda)
    d_recs = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(cuda)
    d_cnt = torch.tensor(counts, dtype=torch.int32, device=cuda)
    d_org = torch.from_numpy(origins).to(cuda)
    assert d_recs.numel() == nT * max_rec * C.sizeof(_lib.CpxRecord)
    _lib.check(_lib.lib().cpx_polygonize_device(ptr(d_maps), ptr(d_recs), ptr(d_cnt), nT, H, W, max_rec, float(scale), ptr(d_org),
                                                ptr(bufs.pool), max_pts, ptr(bufs.cells), ptr(bufs.tot), ptr(bufs.ws),
                                                torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    raw_cells = bufs.cells.cpu().numpy()
    raw_pool = bufs.pool.cpu().numpy()
    tot = bufs.tot.cpu().numpy()
    # the guards
    assert (raw_cells[nT * max_rec * CELL.itemsize:] == SENTINEL).all(), "cells written behind nT * max_rec"
    assert (raw_pool[max_pts * 16:] == SENTINEL).all(), "vertex pool written behind max_pts"
    assert (tot[1:] == -1).all()
    assert (bufs.ws[bufs.ws_bytes:] == 0xFF).all().item(), "workspace written behind cpx_polygonize_workspace_bytes"
    cells = raw_cells[:nT * max_rec * CELL.itemsize].view(CELL).reshape(nT, max_rec)
    xy = raw_pool[:max_pts * 16].view(np.float64).reshape(max_pts, 2)
    used = [min(c, max_rec) for c in counts]
    if fresh:
        # slots past a tile's records are nobody's; pool rows no cell owns are untouched
        rows = raw_cells[:nT * max_rec * CELL.itemsize].reshape(nT, max_rec, CELL.itemsize)
        for t in range(nT):
            assert (rows[t, used[t]:] == SENTINEL).all(), f"tile {t}: cell slots past its records written"
        owned = np.zeros(max_pts, bool)
        for t in range(nT):
            for c in cells[t, :used[t]]:
                owned[c["offset"]: c["offset"] + c["n_pts"]] = True
        assert (raw_pool[:max_pts * 16].reshape(max_pts, 16)[~owned] == SENTINEL).all(), "pool rows outside every cell written"
    return types.SimpleNamespace(cells=cells, xy=xy, total=int(tot[0]), tiles=[cells[t, :used[t]] for t in range(nT)], bufs=bufs)


def _host_tiles(maps, recs, scale, origins):
    """the host polygoniser per tile, offsets moved to the batch's pool: [(cells, xy)]"""
    out, base = [], 0
    for t in range(len(maps)):
        hc, hxy = postprocess.polygonize_tile(np.ascontiguousarray(maps[t]), recs[t], scale, origins[t])
        hc = hc.copy()
        hc["offset"] += base
        base += len(hxy)
        out.append((hc, hxy))
    return out, base


def _assert_equals_host(res, maps, recs, scale=1.0, origins=None):
    origins = [(0.0, 0.0)] * len(maps) if origins is None else origins
    host, total = _host_tiles(maps, recs, scale, origins)
    assert res.total == total
    for t, (hc, hxy) in enumerate(host):
        dc = res.tiles[t]
        assert len(dc) == len(hc)
        for name in FIELDS:
            assert np.array_equal(dc[name], hc[name]), (t, name)
        if len(hc):
            base = int(hc["offset"][0])
            assert np.array_equal(res.xy[base: base + len(hxy)], hxy), t
    return host


def _expect(cells, exp):
    assert [(int(c["n_pts"]), int(c["valid"])) for c in cells] == list(exp)


def _one(cuda, key, scale=1.0, origin=(0.0, 0.0)):
    """one map in one call: device == host bit for bit, device == oracle"""
    m = ps.MAPS[key]()
    recs = ps.records(m)
    res = _poly(cuda, m[None], [recs], scale=scale, origins=[origin])
    _assert_equals_host(res, m[None], [recs], scale, [origin])
    ps.compare_with_oracle(key, None, scale, origin, res.tiles[0], res.xy, perimeter_rel=1e-12)
    return m, recs, res


# ---- ring validity across lanes, votes and the wrap ------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,origin", ps.SCALES)
@pytest.mark.parametrize("nt", ps.COMB_NT)
def test_comb_rings(cuda, nt, scale, origin):
    """valid rings of 21 ... 243 vertices: every lane stride and every 16-edge vote runs to the end without a false alarm;
    every tooth is a local top of the one component, in every 64-lane chunk of the box"""
    m, recs, res = _one(cuda, f"comb{nt}", scale, origin)
    _expect(res.tiles[0], [({3: 21, 10: 63, 11: 69, 15: 93, 16: 99, 17: 105, 21: 129, 22: 135, 40: 243}[nt], 1)])


@pytest.mark.parametrize("scale,origin", ps.SCALES)
@pytest.mark.parametrize("nt,defect,kind", ps.COMB_DEFECTS)
def test_comb_defects(cuda, nt, defect, kind, scale, origin):
    """the ring starts on the defect: the only offending pairs are edge 0 (and 1) against the last two edges, j - i > 192,
    the wrap pair (0, n - 1) among them (polygon_shapes.COMB_PAIRS, asserted in test_polygon_shapes_host.py)"""
    m, recs, res = _one(cuda, f"comb{nt}_{kind}{defect}", scale, origin)
    _expect(res.tiles[0], [({"spike": 244, "pinch": 245}[kind], 0)])


@pytest.mark.parametrize("nt,defect", ps.DOWN_DEFECTS)
def test_comb_down(cuda, nt, defect):
    """offending pairs between non-neighbouring edges only (no lane-0 partner): at the ring's start, ending in the edge that
    votes (i = 239), and behind the last vote (i >= 243 of 255: only the final vote can see them)"""
    m, recs, res = _one(cuda, f"down{nt}_{defect}")
    _expect(res.tiles[0], [{(40, 0): (249, 0), (40, 39): (249, 0), (41, 40): (255, 0)}[nt, defect]])


@pytest.mark.parametrize("scale,origin", ps.SCALES)
@pytest.mark.parametrize("key", ["small", "high"])
def test_small_rings(cuda, key, scale, origin):
    """rings shorter than one vote interval, on a tile of odd width; "high": the same map with labels up to 65535 in the uint16 map"""
    m, recs, res = _one(cuda, key, scale, origin)
    assert recs["label"].tolist() == ([1, 2, 3, 4, 5] if key == "small" else [1, 32767, 32768, 40000, 65535])
    _expect(res.tiles[0], [(10, 1), (10, 0), (10, 0), (6, 0), (9, 0)])


# ---- which component's start wins -------------------------------------------------------------------------------------------
def test_component_choice(cuda):
    """a U's later top lies on a border that is already visited; second components in lane 63, lane 64 and a partial third chunk"""
    m, recs, res = _one(cuda, "vis")
    c, xy = res.tiles[0], res.xy
    got = {int(r["label"]): (tuple(xy[k["offset"]].astype(int).tolist()), int(k["n_pts"]), int(k["valid"])) for r, k in zip(recs, c)}
    assert got == {1: ((9, 5), 4, 1), 2: ((22, 2), 10, 1), 3: ((66, 20), 4, 1), 4: ((67, 24), 4, 1), 5: ((139, 28), 4, 1),
                   6: ((190, 34), 4, 1)}
    assert xy[c[0]["offset"]: c[0]["offset"] + 4].tolist() == [[9, 5], [9, 8], [10, 8], [10, 5]]            # the block, not the U


# ---- tile edges, wide boxes, odd widths ----------------------------------------------------------------------------------------
def test_edge_tiles(cuda):
    """61 x 200 (three 64-lane chunks and a partial one): combs flush with the corners, one instance over the whole tile,
    lines and pixels on the edges, valid instances on the edges; per-tile origins"""
    maps, exp = ps.edge_tiles()
    recs = [ps.records(m) for m in maps]
    origins = [(0.0, 0.0), (1000.0, 17.0), (5.0, 333.0), (98321.0, 65541.0)]
    res = _poly(cuda, maps, recs, origins=origins)
    _assert_equals_host(res, maps, recs, 1.0, origins)
    want = [[(244, 0), (135, 1), (245, 0)], [(4, 1)], [(2, 0)] * 4 + [(1, 0)] * 4, [(4, 1)] * 4]
    for t in range(4):
        ps.compare_with_oracle(f"edge{t}", None, 1.0, origins[t], res.tiles[t], res.xy, perimeter_rel=1e-12)
        _expect(res.tiles[t], want[t])
    c = res.tiles[1][0]
    assert res.xy[c["offset"]: c["offset"] + 4].tolist() == [[1000, 17], [1000, 77], [1199, 77], [1199, 17]]


def test_narrow_tile(cuda):
    m, recs, res = _one(cuda, "narrow", 2.2727, (98321.0, 65541.0))
    assert m.shape[1] == 2
    _expect(res.tiles[0], [(4, 1), (2, 0), (1, 0)])


# ---- the scan: more than 1024 records in a tile, empty tiles, the clamp ---------------------------------------------------------
def _dense_batch(ns):
    return np.stack([ps.dense_tile(n) for n in ns]), [ps.dense_records(n) for n in ns]


def _dense_equals_oracle(res, ns):
    """every tile of a dense batch against the oracle: contours, validity, metrics of all its records"""
    for t, n in enumerate(ns):
        if n:
            assert ps.compare_with_oracle(f"dense{n}", None, 1.0, (0, 0), res.tiles[t], res.xy, perimeter_rel=1e-12) == n // 2


def test_scan_across_chunks_and_tiles(cuda):
    ns = [1025, 0, 1, 1500, 1024]
    maps, recs = _dense_batch(ns)
    res = _poly(cuda, maps, recs, max_rec=2048)
    _assert_equals_host(res, maps, recs)
    _dense_equals_oracle(res, ns)
    flat = np.concatenate(res.tiles)
    assert len(flat) == sum(ns)
    # the exclusive scan in (tile, record) order, the true total, a densely used pool
    assert np.array_equal(flat["offset"], np.concatenate([[0], np.cumsum(flat["n_pts"])[:-1]]))
    assert res.total == int(flat["n_pts"].sum()) == sum(int(ps.dense_expect(n)[0].sum()) for n in ns)
    for n, c in zip(ns, res.tiles):
        n_pts, valid = ps.dense_expect(n)
        assert np.array_equal(c["n_pts"], n_pts) and np.array_equal(c["valid"], valid)
    sq = res.tiles[3][1499]                                    # the last record of the fullest tile: a 2x2 square
    y, x = 3 * (1499 // 42), 3 * (1499 % 42)
    assert res.xy[sq["offset"]: sq["offset"] + 4].tolist() == [[x, y], [x, y + 1], [x + 1, y + 1], [x + 1, y]]


def test_scan_chunk_boundary(cuda):
    """1023, 1024 and 1025 records: one short of, exactly and one more than a 1024-thread chunk; max_rec no multiple of anything"""
    ns = [1023, 1024, 1025]
    maps, recs = _dense_batch(ns)
    res = _poly(cuda, maps, recs, max_rec=1025)
    _assert_equals_host(res, maps, recs)
    _dense_equals_oracle(res, ns)
    flat = np.concatenate(res.tiles)
    assert np.array_equal(flat["offset"], np.concatenate([[0], np.cumsum(flat["n_pts"])[:-1]]))
    assert res.total == sum(int(ps.dense_expect(n)[0].sum()) for n in ns) == 2556 + 2560 + 2561


def test_counts_above_max_rec_are_clamped(cuda):
    """counts[t] = max_rec + 7 with a records buffer of exactly max_rec rows per tile: the same as the true count, and no
    cell slot behind the table (the clamped tile is the last one: its excess would land in the guard)"""
    ns = [1024, 1500]
    maps, recs = _dense_batch(ns)
    plain = _poly(cuda, maps, recs, max_rec=1500)
    _assert_equals_host(plain, maps, recs)
    _dense_equals_oracle(plain, ns)
    res = _poly(cuda, maps, recs, counts=[1024, 1507], max_rec=1500, max_pts=plain.total)
    assert res.total == plain.total and len(res.tiles[1]) == 1500
    assert np.array_equal(res.cells.view(np.uint8), plain.cells.view(np.uint8)) and np.array_equal(res.xy, plain.xy)


# ---- a pool that is too small ---------------------------------------------------------------------------------------------------
def _overflow_map():
    """label 1 a single pixel, 2 a 2x2 square, 3 the 40-tooth comb (243 vertices), 4.. the small rings"""
    m = np.zeros((14 + ps.SMALL_H, 4 * 40 + 4 + 8), np.uint16)
    m[0, 0] = 1; m[3:5, 0:2] = 2
    m[:14, 8:] = ps.comb(40) * 3
    s = ps.small_rings()
    m[14:, :ps.SMALL_W][s > 0] = s[s > 0] + 3
    return m


def test_pool_overflow(cuda):
    m = _overflow_map()
    recs = ps.records(m)
    hc, hxy = postprocess.polygonize_tile(m, recs, 1.0, (0, 0))
    assert hc["n_pts"].tolist() == [1, 4, 243, 10, 10, 10, 6, 9] and hc["valid"].tolist() == [0, 1, 1, 1, 0, 0, 0, 0]
    P = int(hc["n_pts"].sum())
    assert P == 293 and int(hc["offset"][2]) == 5
    for max_pts in (P, P - 1, 5 + 243 - 1, 1):
        res = _poly(cuda, m[None], [recs], max_pts=max_pts)           # asserts: nothing behind max_pts rows, no row outside a cell
        dc = res.tiles[0]
        assert res.total == P                                         # still the true total: the caller learns what it needs
        fits = hc["offset"] + hc["n_pts"] <= max_pts
        assert fits.tolist() == {P: [1] * 8, P - 1: [1] * 7 + [0], 247: [1, 1] + [0] * 6, 1: [1] + [0] * 7}[max_pts]
        for name in FIELDS:
            assert np.array_equal(dc[name][fits], hc[name][fits]), (max_pts, name)
        for a in hc[fits]:
            assert np.array_equal(res.xy[a["offset"]: a["offset"] + a["n_pts"]], hxy[a["offset"]: a["offset"] + a["n_pts"]])
        assert (dc["n_pts"][~fits] == 0).all() and (dc["valid"][~fits] == 0).all()


# ---- hostile records --------------------------------------------------------------------------------------------------------------
def test_hostile_records(cuda):
    m = ps.small_rings()
    H, W = m.shape
    good = ps.records(m)
    bad = np.zeros(7, REC)
    bad[:] = good[0]                                           # label 1: box y 2..7, x 2..7
    bad["cls"] = 4
    bad["x1"][0] = bad["x0"][0]                                # empty box
    bad["x1"][1] = bad["x0"][1] - 3                            # x1 < x0
    bad["y1"][2] = H + 1                                       # below the tile
    bad["x0"][3] = -1                                          # left of the tile
    bad["label"][4] = 77                                       # a label the map does not hold
    bad["y0"][5], bad["y1"][5], bad["x0"][5], bad["x1"][5] = 18, 23, 30, 39      # a box that misses the label's pixels
    bad["x1"][6] = W + 64                                      # right of the tile
    recs = np.concatenate([good[:2], bad[:3], good[2:], bad[3:]])
    is_bad = np.array([0, 0, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1], bool)
    res = _poly(cuda, m[None], [recs], scale=2.2727, origins=[(98321.0, 65541.0)])
    _assert_equals_host(res, m[None], [recs], 2.2727, [(98321.0, 65541.0)])
    dc = res.tiles[0]
    assert (dc["n_pts"][is_bad] == 0).all() and (dc["valid"][is_bad] == 0).all() and (dc["cls"][is_bad] == 4).all()
    # the good cells are what they are without the hostile rows (offsets apart: empty cells take no pool rows)
    alone = _poly(cuda, m[None], [good], scale=2.2727, origins=[(98321.0, 65541.0)])
    for name in FIELDS:
        assert np.array_equal(dc[name][~is_bad], alone.tiles[0][name]), name
    assert np.array_equal(res.xy[:res.total], alone.xy[:alone.total]) and res.total == alone.total
    _expect(dc[~is_bad], [(10, 1), (10, 0), (10, 0), (6, 0), (9, 0)])


# ---- workspace reuse -----------------------------------------------------------------------------------------------------------------
def test_workspace_and_output_reuse(cuda):
    """A, B, A through the same workspace and output buffers; B has A's geometry under other labels, so every border pixel
    the second call marks is a start pixel of the third"""
    a = ps.vis_map()
    b = np.where(a > 0, 7 - a, 0).astype(np.uint16)
    ra, rb = ps.records(a), ps.records(b)
    fresh_a = _poly(cuda, a[None], [ra], max_pts=64)
    fresh_b = _poly(cuda, b[None], [rb], max_pts=64)
    _assert_equals_host(fresh_a, a[None], [ra])
    _assert_equals_host(fresh_b, b[None], [rb])
    bufs = fresh_a.bufs
    for m, r, want in ((b, rb, fresh_b), (a, ra, fresh_a), (a, ra, fresh_a)):
        res = _poly(cuda, m[None], [r], max_pts=64, bufs=bufs)
        assert res.total == want.total
        assert np.array_equal(res.tiles[0].view(np.uint8), want.tiles[0].copy().view(np.uint8))
        assert np.array_equal(res.xy[:res.total], want.xy[:want.total])


# ---- random blobs: one batch, twice ----------------------------------------------------------------------------------------------------
BLOB_ORIGINS = [(7.0, 9.0)] * len(ps.BLOBS)


@pytest.fixture(scope="module")
def blob_batch(cuda):
    maps = np.stack([ps.blob_tile(s, t) for s, t in ps.BLOBS])
    recs = [ps.records(m) for m in maps]
    return maps, recs, _poly(cuda, maps, recs, origins=BLOB_ORIGINS), _poly(cuda, maps, recs, origins=BLOB_ORIGINS)


def test_blobs_equal_host_and_repeat(cuda, blob_batch):
    maps, recs, first, second = blob_batch
    assert maps.shape == (5, 96, 128)
    _assert_equals_host(first, maps, recs, 1.0, BLOB_ORIGINS)
    assert first.total == second.total
    assert np.array_equal(first.cells.view(np.uint8), second.cells.view(np.uint8))
    assert np.array_equal(first.xy.view(np.uint8), second.xy.view(np.uint8))


@pytest.mark.parametrize("k", range(len(ps.BLOBS)))
def test_blobs_equal_oracle(cuda, blob_batch, k):
    maps, recs, first, _ = blob_batch
    assert len(first.tiles[k]) > 5
    ps.compare_with_oracle(f"blob{ps.BLOBS[k][0]}", None, 1.0, BLOB_ORIGINS[k], first.tiles[k], first.xy, perimeter_rel=1e-12)


# ---- cpx_instance_records emits what polygon_shapes.records restates -----------------------------------------------------------------------
def _device_records(cuda, maps, cms, max_rec):
    L = _lib.lib()
    nT, H, W = maps.shape
    d_maps = torch.from_numpy(np.ascontiguousarray(maps).view(np.int16)).to(cuda)
    d_cm = torch.from_numpy(np.ascontiguousarray(cms)).to(cuda)
    d_recs = torch.zeros(nT * max_rec * C.sizeof(_lib.CpxRecord), dtype=torch.uint8, device=cuda)
    d_cnt = torch.zeros(nT, dtype=torch.int32, device=cuda)
    ws = torch.empty(L.cpx_postproc_workspace_bytes(nT, H, W), dtype=torch.uint8, device=cuda)
    _lib.check(L.cpx_instance_records(ptr(d_maps), ptr(d_cm), nT, H, W, max_rec, ptr(d_recs), ptr(d_cnt), ptr(ws),
                                      torch.cuda.current_stream().cuda_stream))
    return d_recs.cpu().numpy().view(REC).reshape(nT, max_rec), d_cnt.cpu().numpy()


@pytest.mark.parametrize("keys", [("comb3",), ("comb17",), ("comb40",), ("comb40_spike0",), ("comb40_pinch39",), ("down41_40",),
                                  ("small",), ("dense1023",), ("dense1025",), tuple(f"blob{s}" for s, _ in ps.BLOBS)])
def test_instance_records_equal_numpy_records(cuda, keys):
    """the maps whose labels are contiguous from 1 (dense: 1025 labels; 1500 are more than cpx_postproc_max_labels(128, 128) = 1491)"""
    maps = np.stack([ps.MAPS[k]() for k in keys])
    want = [ps.records(m) for m in maps]
    cms = np.stack([ps.class_map(m, r) for m, r in zip(maps, want)])
    assert _lib.lib().cpx_postproc_max_labels(128, 128) == 1491
    got, counts = _device_records(cuda, maps, cms, 2048)
    for t, w in enumerate(want):
        assert counts[t] == len(w) == int(maps[t].max())
        w = w.copy()
        w["tile"] = t
        for name in REC.names:
            assert np.array_equal(got[t, :len(w)][name], w[name]), (keys[t], name)
