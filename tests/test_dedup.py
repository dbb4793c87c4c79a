"""a18 / f2: de-duplication (predict_wsi.py:896-965).  Default = ``geojson.dedup_exact``: scipy's own pair set walked in
ITS order, result-identical to the reference (equality tests below).  Opt-in fast path = the device radius search
(cpx_dedup_pairs, exact pair set) + ``geojson.dedup_from_pairs`` (models the set order; documented tolerance inside
clusters of >= 3 cells only)."""
import numpy as np
import pytest
from scipy.spatial import KDTree

from classpose_amd import geojson


def _clustered(rng, n_cells, extent, tie_frac=0.3):
    """centroids as the tile loop produces them: most cells once, some 2x (edge overlaps), some 4x (corner
    overlaps), a few chains; a share of the copies with EQUAL areas (flow-injection slides), 2-decimal rounding"""
    base = rng.uniform(0, extent, (n_cells, 2))
    area = rng.integers(30, 400, n_cells).astype(np.float64)
    mult = rng.choice([1, 2, 3, 4], n_cells, p=[0.6, 0.25, 0.05, 0.10])
    pts, sz = [], []
    for b, a, m in zip(base, area, mult):
        for k in range(m):
            pts.append(b + rng.uniform(-2.5, 2.5, 2) * (k > 0))
            sz.append(a if rng.random() < tie_frac else a + rng.integers(-5, 6))
    chain = np.array([[extent + 50 + 5.0 * k, 50.0] for k in range(7)])            # A-B-C-... chain, 5 px apart
    pts += chain.tolist(); sz += [50, 60, 55, 60, 10, 70, 70]
    order = rng.permutation(len(pts))
    return np.round(np.asarray(pts)[order], 2), np.asarray(sz, np.float64)[order]


def _scipy_pairs(c, r=7.5):
    p = KDTree(c).query_pairs(r, output_type="ndarray").astype(np.int32)
    return p[np.lexsort((p[:, 1], p[:, 0]))] if len(p) else p.reshape(0, 2)


def test_dedup_from_pairs_equals_reference_loop_golden(golden):
    """kept ids of the reference's own deduplicate (golden fixture incl. the A-B-C chain)"""
    _, js = golden
    pts = np.array(js["geojson"]["points"])
    pairs = _scipy_pairs(pts[:, :2])
    assert geojson.dedup_from_pairs(len(pts), pts[:, 2], pairs).tolist() == js["geojson"]["kept_ids"]


def test_dedup_exact_equals_reference_golden(golden):
    """the default path against the kept ids of the reference's own deduplicate (incl. the A-B-C chain)"""
    _, js = golden
    pts = np.array(js["geojson"]["points"])
    st = {}
    assert geojson.dedup_exact(pts[:, :2], pts[:, 2], stats=st).tolist() == js["geojson"]["kept_ids"]
    assert st["n_pairs"] == len(_scipy_pairs(pts[:, :2])) and st["n_order_dependent"] >= 3


@pytest.mark.parametrize("seed,n_cells", [(0, 3000), (1, 3000), (2, 3000), (3, 60000)])
def test_dedup_exact_equals_verbatim_loop(seed, n_cells):
    """EQUALITY (no tolerance) of the default path with the reference's loop run verbatim over scipy's own set
    (geojson.dedup_indices, golden-pinned), on cell tables full of >= 3-cell clusters, equal areas and chains"""
    c, a = _clustered(np.random.default_rng(seed), n_cells, 4000.0 * (n_cells / 3000) ** 0.5)
    st = {}
    got = geojson.dedup_exact(c, a, stats=st).tolist()
    ref = geojson.dedup_indices(c.tolist(), a.tolist())
    assert got == ref
    assert st["n_order_dependent"] > 0.1 * n_cells                       # the order-dependent case is what is being tested
    assert st["n_order_dependent"] == geojson.count_order_dependent(len(c), _scipy_pairs(c))


def test_dedup_exact_trivial_inputs():
    assert geojson.dedup_exact(np.zeros((0, 2)), np.zeros(0)).tolist() == []
    assert geojson.dedup_exact(np.array([[0.0, 0.0], [100.0, 0.0]]), np.ones(2)).tolist() == [0, 1]
    assert geojson.dedup_exact(np.array([[0.0, 0.0], [3.0, 0.0]]), np.array([5.0, 5.0])).tolist() == [0]      # tie keeps i
    assert geojson.dedup_exact(np.array([[0.0, 0.0], [3.0, 0.0]]), np.array([5.0, 6.0])).tolist() == [1]


def _reference_loop(n, sizes, neighbours):
    """predict_wsi.py:929-960 verbatim over a given pair set"""
    groups, member_to_group = {}, {}
    for pair in neighbours:
        if (pair[0] not in member_to_group) and (pair[1] not in member_to_group):
            group_idx = len(groups)
            groups[group_idx] = []
            member_to_group[pair[0]] = group_idx
            member_to_group[pair[1]] = group_idx
        else:
            group_idx = member_to_group[pair[0]] if pair[0] in member_to_group else member_to_group[pair[1]]
        if pair[0] not in groups[group_idx]:
            groups[group_idx].append(pair[0])
        if pair[1] not in groups[group_idx]:
            groups[group_idx].append(pair[1])
    to_remove = {}
    for k in groups:
        group = groups[k]
        if len(group) > 1:
            largest = group[np.argmax([sizes[i] for i in group])]
            for i in group:
                if i != largest and i not in to_remove:
                    to_remove[i] = True
    return [i for i in range(n) if i not in to_remove]


def _assert_same_up_to_ambiguous_clusters(n, pairs, got, ref, max_frac):
    """kept ids may differ only inside connected components of >= 3 cells (where the reference's own outcome
    depends on hash-collision displacement inside its Python set), and only in a small fraction of them"""
    diff = set(ref) ^ set(got)
    assert len(diff) <= max_frac * n, (len(diff), n)
    deg = np.bincount(pairs.ravel(), minlength=n)
    nb = {i: set() for i in diff}
    for i, j in pairs[np.isin(pairs[:, 0], list(diff)) | np.isin(pairs[:, 1], list(diff))].tolist():
        if i in nb: nb[i].add(j)
        if j in nb: nb[j].add(i)
    assert all(deg[i] >= 2 or any(deg[j] >= 2 for j in nb[i]) for i in diff)    # never in a 2-cell component


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_dedup_from_pairs_equals_reference_loop_random(seed):
    """the OPT-IN fast path (vectorised 2-cell components + the reference's loop over the remaining pairs in hash-slot
    order; CLASSPOSE_DEDUP_BACKEND=device) against (1) the reference's loop run verbatim over a Python set of the same pairs and (2) the loop
    over scipy's own set (geojson.dedup_indices, golden-pinned): identical outside >= 3-cell clusters, and
    inside them up to the collision-displacement ambiguity of the reference's set order, ties and chains included"""
    c, a = _clustered(np.random.default_rng(seed), 3000, 4000.0)
    pairs = _scipy_pairs(c)
    got = geojson.dedup_from_pairs(len(c), a, pairs).tolist()
    same_set = set(zip(pairs[:, 0].tolist(), pairs[:, 1].tolist()))
    _assert_same_up_to_ambiguous_clusters(len(c), pairs, got, _reference_loop(len(c), a.tolist(), same_set), 0.002)
    ref = geojson.dedup_indices(c.tolist(), a.tolist())
    assert 0.55 * len(c) < len(ref) < 0.8 * len(c)
    _assert_same_up_to_ambiguous_clusters(len(c), pairs, got, ref, 0.002)


def test_set_order_model_matches_cpython():
    """hash((i, j)) and the table mask are CPython's; slot order == real set iteration order up to collisions"""
    rng = np.random.default_rng(0)
    a = rng.integers(0, 3_000_000, 500)
    b = a + rng.integers(1, 5000, 500)
    h = geojson._tuple2_hash(a, b)
    assert all(int(x) == (hash((int(i), int(j))) & 0xFFFFFFFFFFFFFFFF) for x, i, j in zip(h, a, b))
    for n in (1, 5, 6, 19, 20, 77, 307, 1229, 3120, 50001, 120000):
        assert geojson._fast_set_table_mask(n) == geojson._set_table_mask(n), n
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    real = list(set(zip(pairs[:, 0].tolist(), pairs[:, 1].tolist())))
    slot = geojson._tuple2_hash(pairs[:, 0], pairs[:, 1]) & np.uint64(geojson._fast_set_table_mask(len(pairs)))
    pred = [tuple(x) for x in pairs[np.argsort(slot, kind="stable")].tolist()]
    pos = {t: i for i, t in enumerate(real)}
    assert sum(pos[x] > pos[y] for x, y in zip(pred, pred[1:])) <= 0.08 * len(pred)


def test_dedup_from_pairs_no_pairs_and_empty():
    assert geojson.dedup_from_pairs(5, np.ones(5), np.zeros((0, 2), np.int32)).tolist() == [0, 1, 2, 3, 4]
    assert geojson.dedup_from_pairs(0, np.ones(0), np.zeros((0, 2), np.int32)).tolist() == []


@pytest.mark.gpu
def test_device_pairs_equal_kdtree_query_pairs_golden(cuda, golden):
    from classpose_amd import ops
    _, js = golden
    pts = np.array(js["geojson"]["points"])
    pairs = ops.dedup_pairs(pts[:, :2], 7.5, cuda)
    assert np.array_equal(pairs, _scipy_pairs(pts[:, :2]))                    # incl. the 7.4 / 7.6 px boundary cases
    assert geojson.dedup_from_pairs(len(pts), pts[:, 2], pairs).tolist() == js["geojson"]["kept_ids"]


@pytest.mark.gpu
@pytest.mark.parametrize("n_cells,extent", [(500, 700.0), (650_000, 40_000.0)])
def test_device_pairs_equal_kdtree_query_pairs_synthetic(cuda, n_cells, extent):
    """~10^6 centroids spread like a 40k^2 slide's cell table: identical pair SET, then identical kept ids"""
    import time
    from classpose_amd import ops
    c, a = _clustered(np.random.default_rng(7), n_cells, extent)
    # exact-radius cases: partners at distance exactly 7.5 (3-4-5 triangle scaled) must be included (<=)
    c[:2] = [[100.0, 100.0], [104.5, 106.0]]
    ops.dedup_pairs(c[:1000], 7.5, cuda)                                      # warm-up
    t0 = time.perf_counter()
    pairs = ops.dedup_pairs(c, 7.5, cuda)
    t1 = time.perf_counter()
    keep = geojson.dedup_from_pairs(len(c), a, pairs)
    t2 = time.perf_counter()
    ref = _scipy_pairs(c)
    assert np.array_equal(pairs, ref)
    assert (0, 1) in set(map(tuple, pairs[:50].tolist()))
    print(f"{len(c)} centroids, {len(pairs)} pairs: device search {1e3 * (t1 - t0):.1f} ms incl. H2D/D2H, "
          f"host grouping {1e3 * (t2 - t1):.1f} ms")
    t3 = time.perf_counter()
    full = _reference_loop(len(c), a.tolist(), set(zip(pairs[:, 0].tolist(), pairs[:, 1].tolist())))
    print(f"   (the reference's loop over the whole pair set: {time.perf_counter() - t3:.2f} s)")
    _assert_same_up_to_ambiguous_clusters(len(c), pairs, keep.tolist(), full, 0.002)


# ---- the device radius search at other radii and at its edges ---------------------------------------------------------------
# Reference: scipy KDTree.query_pairs, which on every input below equals the brute-force float64 test
# dx * dx + dy * dy <= r * r over all pairs (asserted where the reference is built).
RADII = [0.7, 2.5, 5, 7.5, 8, 8.01, 9.3, 10, 13]
# Three points on a line whose pair (1, 2) a cell edge of max_dist itself loses: floor((x - x0) * (1 / cell)) with the rounded
# reciprocal puts points 1 and 2 two cells apart.  The third set is the edge of a power-of-two cell equal to max_dist:
# fl(15 - (7 - 2^-50)) is exactly 8, the pair counts, and the points sit in cells [-1, 7) and [15, 23) of a grid from -17.
THREE_POINTS = [(9.3, [-500.0, -81.5, -72.2]), (8.01, [-499.98, 1718.77, 1726.78]), (8.0, [-8.5, 7.0 - 2.0 ** -50, 15.0])]


def _dd_thr():
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "classpose_amd", "csrc", "cpx_dedup.hip")
    with open(src) as f:
        return int(re.search(r"^#define\s+DD_THR\s+(\d+)", f.read(), re.M).group(1))


def _brute_pairs(c, r):
    """{(i, j), i < j : dx * dx + dy * dy <= r * r} in float64, sorted by (i, j)"""
    dx = c[:, None, 0] - c[None, :, 0]
    dy = c[:, None, 1] - c[None, :, 1]
    i, j = np.nonzero(np.triu(dx * dx + dy * dy <= np.float64(r) * np.float64(r), 1))
    return np.stack([i, j], 1).astype(np.int32)


def _edge_points(r):
    """~1000 shuffled points: a 26 x 26 half-integer lattice from a negative origin scaled by r / 2.5 (step r / 5: the (3, 4) and
    (5, 0) steps are partners at exactly r wherever the step is exact, across cell borders), 40 exact duplicates, and a clump
    of 300 points of 2 decimals inside a 5 x 5 box (one or two cells: hundreds of partners per point at the larger radii)"""
    rng = np.random.default_rng(int(r * 100))
    k = np.arange(26) * 0.5
    gx, gy = np.meshgrid(k, k)
    lat = np.stack([gx.ravel(), gy.ravel()], 1) * (r / 2.5) + np.array([-10.5, -3.0])
    dup = lat[rng.choice(len(lat), 40, replace=False)]
    clump = np.round(rng.uniform(0, 5, (300, 2)) + np.array([5 * r + 20.25, -1.5]), 2)
    pts = np.concatenate([lat, dup, clump])
    return np.ascontiguousarray(pts[rng.permutation(len(pts))])


_EDGE_REF = {}


def _edge_case(r, n=None, collinear=False):
    """(points, reference pairs) built once per case and left unchanged"""
    key = (r, n, collinear)
    if key not in _EDGE_REF:
        c = _edge_points(r)
        if collinear:
            c[:, 1] = -3.0
        if n is not None:
            c = np.ascontiguousarray(c[:n])
        ref = _scipy_pairs(c, r)
        assert np.array_equal(ref, _brute_pairs(c, r))
        c.setflags(write=False)
        ref.setflags(write=False)
        _EDGE_REF[key] = (c, ref)
    return _EDGE_REF[key]


def _assert_pairs_equal(got, ref, what):
    """exact equality of two (P, 2) pair lists sorted by (i, j); a failure counts what is missing / extra and shows the first"""
    if got.shape == ref.shape and np.array_equal(got, ref):
        return
    g, f = set(map(tuple, got.tolist())), set(map(tuple, ref.tolist()))
    missing, extra = sorted(f - g), sorted(g - f)
    if not missing and not extra:
        bad = np.argwhere(got != ref) if got.shape == ref.shape else []
        raise AssertionError(f"{what}: same pair set in another order or with repeats ({len(got)} vs {len(ref)} rows), "
                             f"first differing element {bad[0].tolist() if len(bad) else None}")
    raise AssertionError(f"{what}: {len(got)} pairs, reference {len(ref)}; {len(missing)} missing (first {missing[:1]}), "
                         f"{len(extra)} extra (first {extra[:1]})")


def test_edge_point_sets_hold_what_they_are_for():
    """host check of the inputs: partners at exactly r, zero-distance pairs, negative coordinates, crowded points"""
    for r in (2.5, 5, 7.5, 10):                                    # r / 5 and every lattice coordinate exact
        c, ref = _edge_case(r)
        d = c[ref[:, 0]] - c[ref[:, 1]]
        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        assert (d2 == r * r).sum() >= 600 and (d2 == 0).sum() >= 40
        assert (c < 0).any() and np.bincount(ref[:, 0]).max() >= (200 if r >= 7.5 else 5)
    for r in RADII:
        c, ref = _edge_case(r)
        assert len(c) == 26 * 26 + 340 and len(ref) > 2000


@pytest.mark.gpu
@pytest.mark.parametrize("r", RADII)
def test_device_pairs_equal_query_pairs_at_every_radius(cuda, r):
    from classpose_amd import ops
    c, ref = _edge_case(r)
    _assert_pairs_equal(ops.dedup_pairs(c.copy(), r, cuda), ref, f"r = {r}, {len(c)} points")


@pytest.mark.gpu
@pytest.mark.parametrize("r", [2.5, 7.5, 9.3])
def test_device_pairs_equal_query_pairs_collinear(cuda, r):
    """all y equal: a grid two cells high, every lattice column collapsed into 26 exact duplicates"""
    from classpose_amd import ops
    c, ref = _edge_case(r, collinear=True)
    _assert_pairs_equal(ops.dedup_pairs(c.copy(), r, cuda), ref, f"collinear, r = {r}")


@pytest.mark.gpu
@pytest.mark.parametrize("r", [7.5, 13])
@pytest.mark.parametrize("dn", [None, -1, 0, 1])
def test_device_pairs_equal_query_pairs_around_a_block_of_points(cuda, dn, r):
    """n = 2 and n = DD_THR - 1, DD_THR, DD_THR + 1: the last block of one thread per point empty but for one, full, absent"""
    from classpose_amd import ops
    n = 2 if dn is None else _dd_thr() + dn
    c, ref = _edge_case(r, n=n)
    _assert_pairs_equal(ops.dedup_pairs(c.copy(), r, cuda), ref, f"n = {n}, r = {r}")


@pytest.mark.gpu
@pytest.mark.parametrize("r,xs", THREE_POINTS)
def test_device_pairs_do_not_lose_a_pair_two_cells_apart(cuda, r, xs):
    from classpose_amd import ops
    c = np.stack([np.array(xs), np.zeros(3)], 1)
    ref = _scipy_pairs(c, r)
    assert ref.tolist() == [[1, 2]] and np.array_equal(ref, _brute_pairs(c, r))
    _assert_pairs_equal(ops.dedup_pairs(c.copy(), r, cuda), ref, f"r = {r}, x = {xs}")


def test_dedup_grid_cell_edge():
    """host: the cell edge is a power of two with room above max_dist; 8 for the production radius, as before"""
    from classpose_amd import ops
    c = np.array([[-3.5, 2.0], [40.0, 9.0]])
    assert ops.dedup_grid(c, 7.5) == (-12.0, -6.0, 8.0, 8, 3)
    for r, cell in [(0.7, 8.0), (7.5, 8.0), (7.99999, 8.0), (8.0, 16.0), (8.01, 16.0), (9.3, 16.0), (13, 16.0), (16, 32.0), (100, 128.0)]:
        assert ops.dedup_grid(c, r)[2] == cell
    for r in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.dedup_grid(c, r)


def _dedup_two_pass(c, r, max_pairs_of, dev, guard=512):
    """cpx_dedup_pairs called directly: pass 1, then pass 2 with max_pairs = max_pairs_of(n_pairs) into a buffer of
    max_pairs + guard rows pre-filled with a sentinel.  Returns (n_pairs, max_pairs, the whole buffer as numpy)."""
    import torch
    from classpose_amd import _lib, ops
    from classpose_amd._lib import ptr
    x0, y0, cell, gw, gh = ops.dedup_grid(c, r)
    L = _lib.lib()
    cd = torch.from_numpy(c.copy()).to(dev)
    nbytes = L.cpx_dedup_pairs_workspace_bytes(len(c), gw, gh)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    tot = torch.zeros(1, dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.cpx_dedup_pairs(ptr(cd), len(c), x0, y0, cell, gw, gh, float(r), None, 0, ptr(tot), ptr(ws), nbytes, st), "count")
    P = int(tot.item())
    mp = max_pairs_of(P)
    buf = torch.full((mp + guard, 2), -777, dtype=torch.int32, device=dev)
    _lib.check(L.cpx_dedup_pairs(ptr(cd), len(c), x0, y0, cell, gw, gh, float(r), ptr(buf), mp, ptr(tot), ptr(ws), nbytes, st), "write")
    return P, mp, buf.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("r", [7.5, 13])
def test_device_pairs_pass_two_stops_at_max_pairs(cuda, r):
    """pass 2 with room for about half of the pairs: nothing behind max_pairs is written, every written pair is one of the
    reference's, and every point whose whole slice lies before the limit has exactly the reference's partners"""
    c, ref = _edge_case(r)
    P, mp, buf = _dedup_two_pass(c, r, lambda P: P // 2 + 3, cuda)
    assert P == len(ref) and 0 < mp < P
    bad = np.argwhere(buf[mp:] != -777)
    assert len(bad) == 0, f"{len(bad)} elements written behind max_pairs = {mp}, first at row {mp + bad[0][0]}"
    cnt = np.bincount(ref[:, 0], minlength=len(c))
    off = np.cumsum(cnt) - cnt                                      # the reference list is sorted by i: slices are the kernel's
    whole = off + cnt <= mp
    last = int(np.nonzero(whole & (cnt > 0))[0].max())
    n_whole = int(off[last] + cnt[last])
    assert n_whole > mp - 400
    _assert_pairs_equal(buf[:n_whole], ref[:n_whole], f"r = {r}: slices that end before max_pairs = {mp}")
    ref_set = set(map(tuple, ref.tolist()))
    rest = buf[n_whole:mp]
    assert len(rest) and (rest[:, 0] == rest[0, 0]).all()          # one point straddles the limit
    stray = [p for p in map(tuple, rest.tolist()) if p not in ref_set]
    assert not stray, f"{len(stray)} written pairs are not in the reference, first {stray[0]}"
    assert len(set(map(tuple, rest.tolist()))) == len(rest)


@pytest.mark.gpu
def test_device_pairs_cut_slice_holds_the_smallest_partners_of_a_one_cell_clump(cuda):
    """301 points: an anchor at (0.5, 0.5), which puts the cell borders on multiples of 8, and 300 inside the cell
    [96, 104)^2, most of them partners of each other at r = 7.5.  A cell's slice is sorted by point index (k_dd_cell_sort),
    so where max_pairs cuts a point's partners the ones written are its SMALLEST partners; without the sort they would be
    whichever the bucketing's atomics placed first."""
    rng = np.random.default_rng(5)
    c = np.concatenate([[[0.5, 0.5]], np.round(rng.uniform(96.5, 103.5, (300, 2)), 2)])
    c = np.ascontiguousarray(c[rng.permutation(len(c))])
    from classpose_amd import ops
    assert ops.dedup_grid(c, 7.5)[:3] == (-8.0, -8.0, 8.0)
    ref = _scipy_pairs(c, 7.5)
    assert np.array_equal(ref, _brute_pairs(c, 7.5))
    cnt = np.bincount(ref[:, 0], minlength=len(c))
    off = np.cumsum(cnt) - cnt
    i = int(np.nonzero(cnt >= 100)[0][40])                          # a point with many partners, some way into the list
    mp = int(off[i] + cnt[i] // 2)
    P, _, buf = _dedup_two_pass(c, 7.5, lambda P: mp, cuda)
    assert P == len(ref)
    assert (buf[mp:] == -777).all()
    _assert_pairs_equal(buf[:mp], ref[:mp], f"first {mp} pairs: point {i} keeps {cnt[i] // 2} of its {cnt[i]} partners")
