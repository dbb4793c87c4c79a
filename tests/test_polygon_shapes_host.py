"""CPU: the id maps of tests/polygon_shapes.py through the product's host polygoniser (cpx_polygonize_host) against
oracle/polygons.py, with the vertex counts and validities those maps were built for asserted as literals -- what
tests/test_gpu_polygons_edges.py then asserts on the device polygoniser -- and the oracle's own account of WHICH edge
pairs break each defect ring, so that the inputs are known to sit where the device's lanes and votes change."""
import numpy as np
import pytest

import polygon_shapes as ps
from classpose_amd import postprocess


def _host(key, scale=1.0, origin=(0.0, 0.0)):
    m = ps.MAPS[key]()
    recs = ps.records(m)
    cells, xy = postprocess.polygonize_tile(m, recs, scale, origin)
    assert np.array_equal(cells["cls"], recs["cls"])
    assert np.array_equal(cells["offset"], np.concatenate([[0], np.cumsum(cells["n_pts"])[:-1]])) and len(xy) == cells["n_pts"].sum()
    return m, recs, cells, xy


def _expect(cells, exp):
    assert [(int(c["n_pts"]), int(c["valid"])) for c in cells] == list(exp)


@pytest.mark.parametrize("scale,origin", ps.SCALES)
@pytest.mark.parametrize("nt", ps.COMB_NT)
def test_comb_rings(nt, scale, origin):
    m, recs, cells, xy = _host(f"comb{nt}", scale, origin)
    ps.compare_with_oracle(f"comb{nt}", None, scale, origin, cells, xy)
    _expect(cells, [({3: 21, 10: 63, 11: 69, 15: 93, 16: 99, 17: 105, 21: 129, 22: 135, 40: 243}[nt], 1)])
    _expect(cells, [ps.comb_expect(nt)])
    # every tooth is a local top of the one component, and the teeth reach into every 64-lane chunk of the box
    assert m.shape[1] == 4 * nt + 4 and recs["x1"][0] - recs["x0"][0] == 4 * nt + 2


@pytest.mark.parametrize("scale,origin", ps.SCALES)
@pytest.mark.parametrize("nt,defect,kind", ps.COMB_DEFECTS)
def test_comb_defects(nt, defect, kind, scale, origin):
    key = f"comb{nt}_{kind}{defect}"
    m, recs, cells, xy = _host(key, scale, origin)
    ps.compare_with_oracle(key, None, scale, origin, cells, xy)
    _expect(cells, [({"spike": 244, "pinch": 245}[kind], 0)])
    _expect(cells, [ps.comb_expect(nt, kind)])
    if scale == 1.0:    # the ring starts on the defect (it is the raster-first pixel) and folds back over its first edge at the wrap
        ys, xs = np.nonzero(m)
        assert xy[0].tolist() == [xs[0], ys[0]] and ys[0] < 4
        assert ps.offending_pairs(xy) == ps.COMB_PAIRS[kind](len(xy))


@pytest.mark.parametrize("nt,defect", ps.DOWN_DEFECTS)
def test_comb_down(nt, defect):
    """teeth pointing down: the defect is not the ring's start, its offending pairs lie where the tooth is"""
    key = f"down{nt}_{defect}"
    m, recs, cells, xy = _host(key)
    ps.compare_with_oracle(key, None, 1.0, (0, 0), cells, xy)
    _expect(cells, [{(40, 0): (249, 0), (40, 39): (249, 0), (41, 40): (255, 0)}[nt, defect]])
    _expect(cells, [ps.comb_down_expect(nt, defect)])
    first = ps.DOWN_PAIRS[nt, defect]
    assert first == {(40, 0): 3, (40, 39): 237, (41, 40): 243}[nt, defect]
    assert ps.offending_pairs(xy) == [(first + di, first + dj) for di, dj in ps.DOWN_PAIR_SHAPE]


@pytest.mark.parametrize("scale,origin", ps.SCALES)
@pytest.mark.parametrize("key", ["small", "high"])
def test_small_rings(key, scale, origin):
    m, recs, cells, xy = _host(key, scale, origin)
    assert recs["label"].tolist() == ([1, 2, 3, 4, 5] if key == "small" else [1, 32767, 32768, 40000, 65535])
    assert ps.compare_with_oracle(key, None, scale, origin, cells, xy) == 1
    _expect(cells, [(10, 1), (10, 0), (10, 0), (6, 0), (9, 0)])
    _expect(cells, ps.SMALL_RINGS.values())
    assert m.shape[1] % 2 == 1
    if scale != 1.0:
        return
    pairs = [ps.offending_pairs(xy[c["offset"]: c["offset"] + c["n_pts"]]) for c in cells]
    assert pairs[0] == [] and pairs[3] == [(0, 4), (0, 5)] and pairs[4] == [(3, 5), (3, 6), (4, 5), (4, 6)]
    # the two pinched rings: no fold-back between neighbours (no pair with j == i + 1), so lane 0 of the device's vote sees nothing
    assert pairs[1] == pairs[2] == [(1, 7), (1, 8), (2, 6), (2, 7), (2, 8), (3, 6), (3, 7)]


def test_component_choice():
    m, recs, cells, xy = _host("vis")
    assert ps.compare_with_oracle("vis", None, 1.0, (0, 0), cells, xy) == 6
    got = {int(r["label"]): (tuple(xy[c["offset"]].astype(int).tolist()), int(c["n_pts"]), int(c["valid"])) for r, c in zip(recs, cells)}
    assert got == {1: ((9, 5), 4, 1), 2: ((22, 2), 10, 1), 3: ((66, 20), 4, 1), 4: ((67, 24), 4, 1), 5: ((139, 28), 4, 1),
                   6: ((190, 34), 4, 1)} == ps.VIS_EXPECT
    # the boxes put the second component's top in lane 63 of the first chunk, lane 0 of the second and into a partial third one
    assert [int(c["x1"] - c["x0"]) for c in recs[2:5]] == [65, 66, 138] and int(recs["x0"][2]) == 3


@pytest.mark.parametrize("i", range(4))
def test_edge_tiles(i):
    m, recs, cells, xy = _host(f"edge{i}")
    assert m.shape == (61, 200)
    ps.compare_with_oracle(f"edge{i}", None, 1.0, (0, 0), cells, xy)
    want = [[(244, 0), (135, 1), (245, 0)], [(4, 1)], [(2, 0)] * 4 + [(1, 0)] * 4, [(4, 1)] * 4][i]
    _expect(cells, want)
    _expect(cells, ps.edge_tiles()[1][i].values())
    if i == 0:      # the combs touch x = 0 / y = 0 and the bottom-right corner
        assert (recs["x0"][0], recs["y0"][0], recs["x1"][2], recs["y1"][2]) == (0, 0, 200, 61)
    if i == 1:
        assert xy.tolist() == [[0, 0], [0, 60], [199, 60], [199, 0]]


def test_narrow_tile():
    m, recs, cells, xy = _host("narrow")
    assert m.shape[1] == 2
    assert ps.compare_with_oracle("narrow", None, 1.0, (0, 0), cells, xy) == 1
    _expect(cells, [(4, 1), (2, 0), (1, 0)])
    _expect(cells, ps.NARROW_EXPECT.values())


@pytest.mark.parametrize("n", ps.DENSE_N)
def test_dense_tile(n):
    m = ps.dense_tile(n)
    recs = ps.dense_records(n)
    assert len(np.unique(m)) == n + 1
    if n == 1025:
        assert np.array_equal(recs, ps.records(m))          # the closed form is the generic restatement
    cells, xy = postprocess.polygonize_tile(m, recs, 1.0, (0, 0))
    n_pts, valid = ps.dense_expect(n)
    assert np.array_equal(cells["n_pts"], n_pts) and np.array_equal(cells["valid"], valid)
    assert n_pts[:4].tolist() == [1, 4, 1, 4] and valid[:4].tolist() == [0, 1, 0, 1]
    sq = cells[1]
    assert xy[sq["offset"]: sq["offset"] + 4].tolist() == [[3, 0], [3, 1], [4, 1], [4, 0]] and sq["area"] == 1.0 and sq["perimeter"] == 4.0
    assert ps.DENSE_N == (1023, 1024, 1025, 1500)
    assert ps.compare_with_oracle(f"dense{n}", None, 1.0, (0, 0), cells, xy) == n // 2 == {1023: 511, 1024: 512, 1025: 512, 1500: 750}[n]


@pytest.mark.parametrize("seed,thr", ps.BLOBS[3:])
def test_random_blobs(seed, thr):
    """the first three (seed, thr) are test_oracle_polygons.py::test_host_polygonizer_equals_oracle_random_blobs, on the same maps"""
    assert ps.BLOBS[:3] == ((0, 0.02), (1, 0.0), (2, 0.05))
    m, recs, cells, xy = _host(f"blob{seed}", 1.0, (7, 9))
    assert m.shape == (96, 128) and len(cells) > 5
    ps.compare_with_oracle(f"blob{seed}", None, 1.0, (7, 9), cells, xy)
