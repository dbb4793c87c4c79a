"""CPU: every premise the hand-built post-processing cases of tests/postproc_shapes.py are named for, proved with the oracle
alone (no GPU, no library): the seed counts and ranks of the convergence maps and the label sizes they must give, where the
centres of the instance maps lie, which pixels never receive heat, which diffusion path a label's box takes, which ids one
workgroup runs one after the other, that the crowded maps overflow the label hash, and numpy's arg-max rule for the vote."""
import os
import re

import numpy as np
import pytest

import postproc_shapes as S
from oracle import classmask, dynamics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RPAD = 20


def test_the_restated_constants_are_the_kernels():
    assert (S.DIFF_SMALL_CELLS, S.DIFF_BIG_CELLS, S.DIFF_HUGE_CELLS) == (2048, 8192, 18336)
    assert [S.diffusion_path(c) for c in (1, 2048, 2049, 8192, 8193, 18336, 18337)] == [0, 0, 1, 1, 2, 2, 3]
    src = open(os.path.join(ROOT, "classpose_amd", "csrc", "cpx_postproc.hip")).read()
    defs = dict(re.findall(r"^#define (\w+) +(\d+)\b", src, re.M))
    assert int(defs["DIFF_SMALL_CELLS"]) == S.DIFF_SMALL_CELLS and int(defs["DIFF_BIG_CELLS"]) == S.DIFF_BIG_CELLS
    assert int(defs["DIFF_HUGE_PER_THREAD"]) * int(defs["DIFF_BIG_THREADS"]) - 96 == S.DIFF_HUGE_CELLS
    assert int(defs["RPAD"]) == RPAD and int(defs["NTHR"]) == S.LH_SLOTS == 256 and int(defs["RUN_PX"]) * 256 == S.STATS_WG
    assert "const int per_tile = nT >= 8 ? 32 : (nT <= 2 ? 128 : 256 / nT);" in src
    assert [S.diffuse_big_grid(n, 1000) for n in (1, 2, 3, 5, 7, 8, 9)] == [128, 128, 85, 51, 36, 32, 32]
    assert S.diffuse_big_grid(1, 95) == 94
    assert 50 * 50 * 0.4 == 1000.0


def test_pack_p_final_is_both_readers_input():
    H, W = 5, 300
    p, pt, inds = S.pack_p_final(H, W, [((4, 299), [0, 7, 1499]), ((0, 0), [300])])
    assert p.dtype == np.int32 and p.shape == (H * W,) and (p == -1).sum() == H * W - 4
    assert p[7] == (4 << 16) | 299 and p[300] == 0
    assert pt.numpy().tolist() == [[4, 4, 0, 4], [299, 299, 0, 299]]
    assert inds[0].tolist() == [0, 0, 1, 4] and inds[1].tolist() == [0, 7, 0, 299]
    with pytest.raises(AssertionError):
        S.pack_p_final(H, W, [((5, 0), [0])])
    with pytest.raises(AssertionError):
        S.pack_p_final(H, W, [((0, 0), [3]), ((1, 1), [3])])


def _oracle(name, fraction=0.4):
    H, W, p, pt, inds = S.EXPECT[name][0]()
    m, dbg = dynamics.get_masks(pt, inds, (H, W), max_size_fraction=fraction, return_debug=True)
    act = p != -1
    assert np.array_equal(np.flatnonzero(act) // W, inds[0]) and np.array_equal((p[act] >> 16), pt[0].numpy())
    return H, W, p, m.astype(np.int64), dbg


@pytest.mark.parametrize("name", list(S.EXPECT))
def test_the_oracle_gives_the_hand_derived_labels(name):
    _, nlab, sizes, zeros = S.EXPECT[name]
    H, W, p, m, dbg = _oracle(name)
    got = sorted(np.bincount(m.ravel())[1:].tolist())
    print(f"  {name}: {m.max()} labels, sizes {got[:6]}{' ...' if len(got) > 6 else ''}, {int(((m == 0).ravel() & (p != -1)).sum())} active pixels left 0")
    assert m.max() == nlab and got == sizes
    assert int(((m == 0).ravel() & (p != -1)).sum()) == zeros


def _h(dbg, y, x):
    return int(dbg["h1"][y + RPAD, x + RPAD])


def test_thresholds_and_reach_premises():
    _, _, _, m, dbg = _oracle("thresholds")
    assert (_h(dbg, 10, 10), _h(dbg, 10, 30), _h(dbg, 30, 30)) == (10, 11, 15)
    assert [_h(dbg, *c) for c in ((30, 31), (29, 30), (30, 29), (31, 30), (32, 30))] == [3, 3, 2, 2, 3]
    assert (dbg["seeds"] - RPAD).tolist() == [[10, 30], [30, 30]]
    M1 = dbg["M1"][RPAD:-RPAD, RPAD:-RPAD]
    assert M1[30, 31] == M1[29, 30] == 2 and M1[30, 29] == M1[31, 30] == M1[32, 30] == 0 and M1[10, 10] == 0
    _, _, _, m, dbg = _oracle("reach")
    M1 = dbg["M1"][RPAD:-RPAD, RPAD:-RPAD]
    chain = [(30, 11), (30, 12), (30, 13), (30, 14), (29, 15), (28, 14), (28, 13)]
    assert all(max(abs(y - 30), abs(x - 10)) <= 5 for y, x in chain)
    assert [int(M1[c]) for c in chain] == [1] * 5 + [0] * 2


def test_ties_plateau_overlap_premises():
    _, _, _, m, dbg = _oracle("ties")
    seeds = (dbg["seeds"] - RPAD).tolist()
    assert seeds == sorted(seeds) and len(seeds) == 6 and all(_h(dbg, *s) == 12 for s in seeds)       # rank = raster order
    M1 = dbg["M1"][RPAD:-RPAD, RPAD:-RPAD]
    assert [int(M1[20, x]) for x in range(10, 19)] == [2, 2, 2, 3, 3, 3, 3, 3, 3] and not (M1 == 1).any()
    assert [int(M1[y, 30]) for y in range(40, 47)] == [5, 6, 6, 6, 6, 6, 6] and not (M1 == 4).any()
    _, _, _, m, dbg = _oracle("plateau")
    assert (dbg["seeds"] - RPAD).tolist() == [[10, 10], [30, 30], [30, 31]]
    assert not (dbg["M1"] == 2).any() and (dbg["M1"] == 3).sum() == 2           # the earlier label of the plateau has no cell at all
    _, _, _, m, dbg = _oracle("overlap")
    assert (dbg["seeds"] - RPAD).tolist() == [[20, 14], [40, 40], [20, 10], [46, 40]]
    M1 = dbg["M1"][RPAD:-RPAD, RPAD:-RPAD]
    assert [int(M1[20, x]) for x in range(10, 17)] == [3] * 6 + [1] and [int(M1[y, 40]) for y in range(40, 47)] == [2] + [4] * 6


def test_corners_fraction_many_seeds_premises():
    H, W, _, m, dbg = _oracle("corners")
    seeds = (dbg["seeds"] - RPAD).tolist()
    assert len(seeds) == 8 and {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)} <= {tuple(s) for s in seeds}
    assert all(y in (0, H - 1) or x in (0, W - 1) for y, x in seeds)
    for name, n, kept in (("fraction_1000", 1000, True), ("fraction_1001", 1001, False)):
        H, W, p, m, dbg = _oracle(name)
        assert (H, W) == (50, 50) and _h(dbg, 25, 25) == n and H * W * 0.4 == 1000.0
        assert ((np.bincount(m.ravel())[1:] == n).any()) == kept
    _, _, _, m, dbg = _oracle("many_seeds")
    assert len(dbg["seeds"]) == 441 > 256 and all(int(dbg["h1"][tuple(s)]) == 11 for s in dbg["seeds"])
    assert dbg["seeds"].tolist() == sorted(dbg["seeds"].tolist())


def test_crowd_overflows_the_label_hash_of_one_workgroup():
    H, W, p, m, dbg = _oracle("crowd")
    assert len(dbg["seeds"]) == 372 and S.max_labels(H, W) == 374
    q = np.where(p != -1, p, 0)
    rank_label = np.where(p != -1, dbg["M1"][(q >> 16) + RPAD, (q & 0xFFFF) + RPAD], 0)              # the labels k_gather and k_big_first see
    first_wg = np.unique(rank_label[:S.STATS_WG])
    first_wg = first_wg[first_wg > 0]
    assert sorted(first_wg.tolist()) == sorted(S.crowd_labels_of_first_workgroup())
    misses = S._guaranteed_misses(first_wg)
    print(f"  crowd: {len(first_wg)} labels in the first workgroup's pixels, at least {misses} updates miss the LDS hash")
    assert misses > 0


# ---- instance maps ---------------------------------------------------------------------------------------------------
def _flows(m):
    F, dbg = dynamics.masks_to_flows(m, return_debug=True)
    assert np.isfinite(F).all() and np.all(F[:, m == 0] == 0)
    ids = np.unique(m[m > 0])
    centres = {int(l): tuple(int(v) for v in c) for l, c in zip(ids, dbg["centers"])}
    for l, c in centres.items():
        assert m[c] == l
    return F, dbg, centres


def _centroid_pixel(m, l):
    yy, xx = np.nonzero(m == l)
    return int(round(yy.mean())), int(round(xx.mean()))


def test_touching_and_gaps():
    m = S.touching()
    ids = np.unique(m[m > 0])
    assert len(ids) >= 6 and ids.max() < S.max_labels(*m.shape) and m.dtype == np.int32
    for l in ids:                                                                   # every label shares an edge with another one
        sel = m == l
        nb = np.zeros_like(sel)
        nb[1:] |= sel[:-1]; nb[:-1] |= sel[1:]; nb[:, 1:] |= sel[:, :-1]; nb[:, :-1] |= sel[:, 1:]
        assert ((m != l) & (m > 0) & nb).any(), l
    _flows(m)
    g = S.gaps()
    assert np.unique(g).tolist() == [0, 1, 7, S.max_labels(32, 32) - 1] and S.max_labels(32, 32) == 95
    _, _, centres = _flows(g)
    assert set(centres) == {1, 7, 94}


def test_concave_centroids_lie_outside_their_labels():
    m = S.concave()
    _, _, centres = _flows(m)
    for l in (1, 2, 3):
        assert m[_centroid_pixel(m, l)] != l, l
        assert m[centres[l]] == l


def test_even_extents_tie_and_the_first_pixel_in_raster_order_is_the_centre():
    m = S.even_ties()
    _, _, centres = _flows(m)
    assert centres == {1: (2, 2), 2: (3, 9), 3: (2, 18), 4: (10, 2), 5: (25, 20), 6: (9, 31), 7: (16, 40)}
    for l, n_tied in ((1, 4), (2, 4), (3, 4), (4, 4), (5, 4), (6, 2), (7, 2)):
        yy, xx = np.nonzero(m == l)
        d2 = (xx - xx.mean()) ** 2 + (yy - yy.mean()) ** 2
        assert (d2 == d2.min()).sum() == n_tied, l


def test_thin_split_and_serpentine():
    m = S.thin()
    F, _, centres = _flows(m)
    assert centres[1] == (2, 2) and np.all(F[:, 2, 2] == 0) and centres[2] == (5, 18) and centres[3] == (22, 40)
    assert np.abs(F[1, m == 2]).max() > 0.5 and np.abs(F[0, m == 3]).max() > 0.5
    assert (m == 4).sum() == 20 and np.all(F[:, m == 4] == 0)          # a staircase's central differences only see cells off the label
    m = S.split()
    F, _, centres = _flows(m)
    cold = S.split_cold()
    assert 4 <= centres[1][0] < 13 and 4 <= centres[1][1] < 13 and np.all(m[cold] == 1)
    assert np.all(F[:, cold] == 0) and np.abs(F[:, (m == 1) & ~cold]).max() > 0.5
    m = S.serpentine()
    F, dbg, centres = _flows(m)
    yy, xx = np.nonzero(m)
    assert (yy.max() - yy.min() + 1, xx.max() - xx.min() + 1) == (41, 41) and dbg["n_iter"] == 168 < (m > 0).sum()
    d = S.geodesic(m, centres[1])
    assert (d[m > 0] >= 0).all()
    cold = d > dbg["n_iter"] + 1
    assert cold.sum() > 100 and np.all(F[:, cold] == 0) and np.abs(F[:, (d > 0) & (d < 100)]).max() > 0.5


@pytest.fixture(scope="module")
def four():
    return S.four_paths()


def test_four_paths_has_two_labels_on_each_side_of_every_limit(four):
    m = four
    cells = S.padded_cells(m)
    for k, (y0, x0, h, w) in enumerate(S.FOUR_PATHS_BOXES, 1):
        yy, xx = np.nonzero(m == k)
        assert (yy.min(), xx.min(), yy.max() + 1, xx.max() + 1) == (y0, x0, y0 + h, x0 + w), k
        assert cells[k] == (h + 2) * (w + 2) and (m[y0:y0 + h, x0:x0 + w] == k).sum() < 0.95 * h * w      # no rectangle
    assert [S.diffusion_path(cells[k]) for k in range(1, 9)] == [3, 3, 2, 2, 1, 1, 0, 0]
    assert [cells[k] for k in range(1, 9)] == [19044, 18768, 8280, 10080, 8052, 2116, 2025, 1344]
    for j, k in enumerate((1, 2, 3, 4, 5)):                                        # every large label touches a small neighbour inside its box
        small = m == 9 + j
        assert small.sum() > 20 and S.diffusion_path(cells[9 + j]) == 0
        assert ((m[1:] == k) & small[:-1]).any() or ((m[:, 1:] == k) & small[:, :-1]).any()
    assert m.max() == 13 < S.max_labels(*m.shape)


def test_four_paths_oracle(four):
    F, dbg, centres = _flows(four)
    assert dbg["n_iter"] == 2 * (136 + 136 + 2) and len(centres) == 13


@pytest.mark.parametrize("nT", [1, 8])
def test_same_workgroup_runs_the_labels_in_the_named_order(nT):
    m = S.same_workgroup(nT)
    L = S.max_labels(*m.shape)
    g = S.diffuse_big_grid(nT, L)
    assert g == (128 if nT == 1 else 32) and min(L - 1, S.DIFF_SMALL_GRID) == 128
    cells = S.padded_cells(m)
    ids = sorted(cells)
    assert ids == sorted([1, 1 + 128, 2, 2 + g, 2 + 2 * g]) and max(ids) < L
    second = [l for l in ids if (l - 2) % g == 0 and S.diffusion_path(cells[l]) > 0]        # what workgroup 1 of the second launch runs, in order
    assert second == [2, 2 + g, 2 + 2 * g]
    assert [S.diffusion_path(cells[l]) for l in second] == [2, 1, 1] and cells[2 + g] < cells[2]
    assert not [l for l in ids if (l - 2) % g == 0 and l not in second]
    first = [l for l in ids if (l - 1) % 128 == 0 and S.diffusion_path(cells[l]) == 0]      # workgroup 0 of the first launch
    assert first == [1, 129] and cells[1] > cells[129]
    yy, xx = np.nonzero(m)
    assert yy.min() >= 8 and xx.min() >= 8 and yy.max() < m.shape[0] - 8 and xx.max() < m.shape[1] - 8
    assert len(set(S.SAME_WG_SHIFTS)) == 8 and all(abs(a) <= 8 and abs(b) <= 8 for a, b in S.SAME_WG_SHIFTS)
    F, dbg, _ = _flows(m)
    moved = S.translate(m, -7, 5)                                   # the oracle commutes with a translation, bit for bit
    assert np.array_equal(dynamics.masks_to_flows(moved), S.translate(F, -7, 5))


def test_centre_crowd_overflows_the_label_hash_with_four_way_ties():
    m = S.centre_crowd()
    ids = np.unique(m[m > 0])
    assert len(ids) >= 91 and np.all(np.bincount(m.ravel())[ids] == 4) and not m.reshape(-1)[S.STATS_WG:].any()
    assert S._guaranteed_misses(ids) > 0 and ids.max() < S.max_labels(64, 64)
    _, _, centres = _flows(m)
    for l, (cy, cx) in centres.items():
        assert m[cy, cx] == m[cy + 1, cx + 1] == l and (cy == 0 or m[cy - 1, cx] != l) and (cx == 0 or m[cy, cx - 1] != l)


# ---- class vote and border removal -------------------------------------------------------------------------------------
def test_the_vote_scenarios_under_numpys_rule():
    m = S.vote_blocks()
    for ncls in (7, 32):
        lg = S.vote_logits(m, ncls)
        cm, _ = classmask.compute_class_masks(m, lg)
        for l in range(1, int(m.max()) + 1):
            name = S.VOTE_SCENARIOS[l % len(S.VOTE_SCENARIOS)]
            assert np.all(cm[m == l] == S.VOTE_EXPECT[name]), (l, name)
        assert np.all(cm[m == 0] == 0)
    assert np.isnan(lg).any() and np.isinf(lg).any() and np.signbit(lg[lg == 0]).any()
    assert np.argmax(np.array([1.0, np.nan, np.inf, np.nan], np.float32)) == 1


def test_the_border_cases_under_the_reference_rule():
    want = {"corner_pixel": [1, 4], "each_side": [5, 6], "id_gaps": [9, 41], "id_65535": [7, 65534]}
    for name, m in S.border_cases().items():
        out = classmask.remove_border_instances(m.copy())
        assert np.unique(out[out > 0]).tolist() == want[name], name
    m = S.border_cases()["corner_pixel"]
    edge = np.zeros(m.shape, bool)
    edge[[0, -1]] = True
    edge[:, [0, -1]] = True
    assert ((m == 2) & edge).sum() == 1 and m[0, -1] == 2
