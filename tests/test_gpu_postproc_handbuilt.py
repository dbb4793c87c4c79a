"""GPU: the post-processing stages behind the Euler loop on inputs built by hand (tests/postproc_shapes.py; every premise is
proved on the CPU by tests/test_postproc_shapes_host.py).  The synthetic network fields of tests/test_gpu_postproc.py never
state these boundary conditions: the two thresholds, the rank of tied seeds, overlapping windows, the five-dilation reach and
the size fraction at equality in get_masks; centroids outside their label, 2- and 4-way centre ties, touching labels,
disconnected ids, one-pixel lines, id gaps, every diffusion path and two paths in one workgroup's LDS in the centre pick and
the diffusion; ties and non-finite logits in the class vote; the border removal's corner cases.

Yardsticks, none of them the code under test:
  * ids: ``oracle.dynamics.get_masks``, integer for integer;
  * flows: ``oracle.dynamics.masks_to_flows`` (float64) under the rule of tests/test_gpu_flow_train.py, unchanged:
    |got - ref| <= 2^-25 + 1e-12, at most the one oracle-reported centre pixel per label left out, the background exactly 0;
  * flow errors: ``oracle.dynamics.remove_bad_flow_masks``, rtol 1e-12 / atol 1e-14 on the ids that are present, equal survivors;
  * class maps: ``oracle.classmask.compute_class_masks`` (numpy's arg-max: the first maximum, a NaN beats every number and
    the first NaN wins) and ``oracle.classmask.remove_border_instances``, exactly.
Every test prints what it measured before it asserts (run with -s)."""
from __future__ import annotations

import time

import numpy as np
import pytest
import torch

import postproc_shapes as S
from classpose_amd import _lib, ops, synth
from oracle import classmask, dynamics
from test_gpu_flow_train import MTF_TOL, _compare_flows
from test_gpu_postproc import _chain

pytestmark = pytest.mark.gpu


# ---- get_masks -------------------------------------------------------------------------------------------------------
def _get_masks(cuda, p, H, W):
    pd = torch.from_numpy(np.ascontiguousarray(p.reshape(-1, H * W))).to(cuda)
    t0 = time.perf_counter()
    got, nlab = ops.get_masks(pd, H, W, 0.4)
    g, n = got.cpu().numpy(), nlab.cpu().numpy()
    dt = time.perf_counter() - t0
    again, nagain = ops.get_masks(pd, H, W, 0.4)
    assert torch.equal(got, again) and torch.equal(nlab, nagain), "two runs are bitwise equal"
    return g, n, dt


@pytest.mark.parametrize("name", list(S.EXPECT))
def test_get_masks_equals_the_oracle_on_hand_built_convergence_maps(cuda, name):
    H, W, p, pt, inds = S.EXPECT[name][0]()
    ref = dynamics.get_masks(pt, inds, (H, W)).astype(np.int32)
    got, nlab, dt = _get_masks(cuda, p, H, W)
    print(f"  {name}: {int((got[0] != ref).sum())} of {H * W} ids differ (tolerance 0); nlabels {int(nlab[0])} (oracle {int(ref.max())}); {dt * 1e3:.1f} ms")
    assert np.array_equal(got[0], ref) and int(nlab[0]) == int(ref.max()) == S.EXPECT[name][1]


def test_get_masks_size_fraction_at_equality_batched(cuda):
    a, b = S.fraction(1000), S.fraction(1001)
    refs = [dynamics.get_masks(c[3], c[4], (50, 50)).astype(np.int32) for c in (a, b)]
    got, nlab, dt = _get_masks(cuda, np.stack([a[2], b[2]]), 50, 50)
    sizes = [sorted(np.bincount(g.ravel())[1:].tolist()) for g in got]
    print(f"  label sizes: tile 0 {sizes[0]} (1000 = H * W * 0.4 is kept), tile 1 {sizes[1]} (1001 is removed); nlabels {nlab.tolist()}; {dt * 1e3:.1f} ms")
    assert np.array_equal(got[0], refs[0]) and np.array_equal(got[1], refs[1])
    assert nlab.tolist() == [2, 1] and sizes == [[12, 1000], [12]]


def test_get_masks_batch_with_an_inactive_tile_and_a_tile_without_seeds(cuda):
    H, W, p, pt, inds = S.overlap()
    low = S._case(H, W, [((12, 12), 10), ((12, 13), 10), ((40, 40), 9), ((41, 41), 3)], 9)         # no count above 10
    ref = dynamics.get_masks(pt, inds, (H, W)).astype(np.int32)
    assert not dynamics.get_masks(low[3], low[4], (H, W)).any()
    got, nlab, dt = _get_masks(cuda, np.stack([p, np.full(H * W, -1, np.int32), low[2]]), H, W)
    print(f"  nT = 3: {int((got[0] != ref).sum())} ids differ in the case, {int(got[1].any())} / {int(got[2].any())} labels in the other two; "
          f"nlabels {nlab.tolist()}; {dt * 1e3:.1f} ms")
    assert np.array_equal(got[0], ref) and not got[1].any() and not got[2].any() and nlab.tolist() == [int(ref.max()), 0, 0]


# ---- centre pick, diffusion, flow error ----------------------------------------------------------------------------------
MAPS = dict(S.INSTANCE_MAPS, four_paths=S.four_paths, same_workgroup_1=lambda: S.same_workgroup(1), same_workgroup_8=lambda: S.same_workgroup(8))
_cache = {}


def _oracle(name):
    """(map, oracle flows float64, centre mask, seeded dP float32, oracle filtered map, oracle errors): once per name, never modified"""
    if name not in _cache:
        import flow_train_reference as fr
        m = MAPS[name]()
        F, dbg = dynamics.masks_to_flows(m, return_debug=True)
        rng = np.random.default_rng(17)
        noise = rng.standard_normal((2,) + m.shape)
        dP = np.where((m % 2 == 0)[None], 5.0 * F + 1.2 * noise, 2.0 * noise).astype(np.float32)   # even ids follow their flows, odd ids do not
        own = dynamics.masks_to_flows
        dynamics.masks_to_flows = lambda maski: F           # the oracle's flow_error computes exactly this again (3 s on four_paths)
        try:
            want, errs = dynamics.remove_bad_flow_masks(m, dP, 0.4, return_errors=True)
        finally:
            dynamics.masks_to_flows = own
        for a in (m, F, dP, want, errs):
            a.setflags(write=False)
        _cache[name] = (m, F, fr.centre_mask(m, dbg["centers"]), dP, want, errs, dbg)
    return _cache[name]


def _cold(name, m, dbg):
    """the pixels that never receive heat (None: the map has none by construction)"""
    if name == "split":
        return S.split_cold()
    if name == "serpentine":
        c = tuple(int(v) for v in dbg["centers"][0])
        return S.geodesic(m, c) > dbg["n_iter"] + 1
    return None


def _check_errors(name, e, errs, m, got_masks, want):
    present = np.unique(m[m > 0]) - 1
    e, r = e[present], errs[present]
    rel = np.abs(e - r) / np.maximum(np.abs(r), 1e-300)
    print(f"  {name}: flow errors of {len(present)} labels, max relative deviation {rel.max():.3e} (tolerance rtol 1e-12, atol 1e-14); "
          f"{len(np.unique(want)) - 1} ids survive; nearest error to the threshold {np.abs(r - 0.4).min():.3e}")
    assert not (np.abs(r - 0.4) < 1e-9).any()
    assert np.allclose(e, r, rtol=1e-12, atol=1e-14), name
    assert np.array_equal(got_masks, want.astype(np.int32)), name


@pytest.mark.parametrize("name", list(S.INSTANCE_MAPS) + ["four_paths", "same_workgroup_1"])
def test_masks_to_flows_equals_the_oracle_on_hand_built_maps(cuda, name):
    m, F, skip, _, _, _, dbg = _oracle(name)
    md = torch.from_numpy(m.copy()).to(cuda)
    t0 = time.perf_counter()
    got = ops.masks_to_flows(md)
    g = got.cpu().numpy()
    dt = time.perf_counter() - t0
    again = ops.masks_to_flows(md)
    print(f"  {name}: {m.shape[0]} x {m.shape[1]}, {len(np.unique(m)) - 1} labels, n_iter {dbg['n_iter']}, {dt * 1e3:.1f} ms")
    _compare_flows(name, g, m, F, skip)
    assert torch.equal(got, again), "two runs are bitwise equal"
    cold = _cold(name, m, dbg)
    if cold is not None:
        assert cold.any() and np.all(F[:, cold] == 0)
        print(f"  {name}: {int(cold.sum())} never-heated pixels, largest |flow| there {np.abs(g[:, cold]).max():.1e} (must be exactly 0)")
        assert np.all(g[:, cold] == 0)


@pytest.mark.parametrize("name", list(S.INSTANCE_MAPS) + ["four_paths", "same_workgroup_1"])
def test_remove_bad_flow_masks_equals_the_oracle_on_hand_built_maps(cuda, name):
    m, _, _, dP, want, errs, _ = _oracle(name)
    assert m.max() < S.max_labels(*m.shape)
    t0 = time.perf_counter()
    got, e = ops.remove_bad_flow_masks(torch.from_numpy(m.copy()).to(cuda)[None], torch.from_numpy(dP).to(cuda)[None], 0.4, return_errors=True)
    g, e = got.cpu().numpy()[0], e.cpu().numpy()[0]
    print(f"  {name}: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    _check_errors(name, e, errs, m, g, want)
    if name in ("touching", "four_paths"):
        assert 0 < len(np.unique(want)) - 1 < len(np.unique(m)) - 1, "some ids go and some stay"


def test_one_workgroup_runs_labels_of_different_paths_in_a_batch_of_eight_translates(cuda):
    """nT = 8: the second diffusion launch has 32 workgroups per tile, and workgroup 1 runs ids 2 (one plane), 34 (two planes, smaller
    box), 66 (two planes) in the same LDS; the first launch's workgroup 0 runs ids 1 and 129.  The oracle commutes with a translation bit
    for bit (tests/test_postproc_shapes_host.py), so its one result is moved with the map."""
    m, F, skip, dP, want, errs, _ = _oracle("same_workgroup_8")
    maps = np.stack([S.translate(m, *s) for s in S.SAME_WG_SHIFTS])
    assert all((t > 0).sum() == (m > 0).sum() for t in maps) and len({t.tobytes() for t in maps}) == 8
    md = torch.from_numpy(maps).to(cuda)
    t0 = time.perf_counter()
    got = ops.masks_to_flows(md)
    g = got.cpu().numpy()
    print(f"  masks_to_flows, nT = 8: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    again = ops.masks_to_flows(md)
    for t, s in enumerate(S.SAME_WG_SHIFTS):
        _compare_flows(f"tile {t}, moved by {s}", g[t], maps[t], S.translate(F, *s), S.translate(skip, *s))
    assert torch.equal(got, again), "two runs are bitwise equal"
    dPs = np.stack([S.translate(dP, *s) for s in S.SAME_WG_SHIFTS])
    t0 = time.perf_counter()
    out, e = ops.remove_bad_flow_masks(md.clone(), torch.from_numpy(dPs).to(cuda), 0.4, return_errors=True)
    out, e = out.cpu().numpy(), e.cpu().numpy()
    print(f"  remove_bad_flow_masks, nT = 8: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    for t, s in enumerate(S.SAME_WG_SHIFTS):
        _check_errors(f"tile {t}", e[t], errs, maps[t], out[t], S.translate(want, *s))


# ---- class vote ----------------------------------------------------------------------------------------------------------
def _report_vote(name, got, ref, m):
    bad = np.unique(m[(got.astype(np.int64) != ref) & (m > 0)])
    print(f"  {name}: {int((got.astype(np.int64) != ref).sum())} pixels differ (tolerance 0)"
          + (f"; wrong labels and their scenarios: {[(int(l), S.VOTE_SCENARIOS[int(l) % len(S.VOTE_SCENARIOS)]) for l in bad]}" if len(bad) else ""))
    assert np.array_equal(got.astype(np.int64), ref), name


@pytest.mark.parametrize("ncls", [7, 32])
def test_class_vote_ties_and_non_finite_logits_follow_numpy(cuda, ncls):
    m = S.vote_blocks()
    lg = S.vote_logits(m, ncls)
    if ncls == 32:
        lg[31][m == 12] = 9.0                              # the last class the table has room for wins a label
    ref, _ = classmask.compute_class_masks(m, lg)
    assert ncls != 32 or np.all(ref[m == 12] == 31)
    maps = np.stack([m, np.zeros_like(m), m[::-1].copy()])
    lgs = np.stack([lg, lg, lg[:, ::-1].copy()])
    got = ops.compute_class_masks(torch.from_numpy(maps).to(cuda), torch.from_numpy(lgs).to(cuda)).cpu().numpy()
    _report_vote(f"ncls = {ncls}, tile 0", got[0], ref, m)
    assert not got[1].any()
    _report_vote(f"ncls = {ncls}, tile 2 (upside down)", got[2], ref[::-1], maps[2])


def test_class_vote_with_one_class_and_with_more_classes_than_the_table(cuda):
    m = S.vote_blocks()
    md = torch.from_numpy(m).to(cuda)[None]
    lg = np.random.default_rng(1).standard_normal((1, 1) + m.shape).astype(np.float32)
    lg[0, 0, ::3, ::5] = np.nan
    lg[0, 0, 1::3, ::4] = -np.inf
    got = ops.compute_class_masks(md, torch.from_numpy(lg).to(cuda)).cpu().numpy()
    print(f"  ncls = 1: {int(got.any())} non-zero classes")
    assert not got.any()
    with pytest.raises(_lib.CpxError):
        ops.compute_class_masks(md, torch.zeros((1, 33) + m.shape, device=cuda))
    ok = ops.compute_class_masks(md, torch.zeros((1, 32) + m.shape, device=cuda)).cpu().numpy()
    assert not ok.any()


def test_class_vote_of_the_fused_chain_follows_numpy(cuda):
    H = W = 256
    dP, cp, _, _ = synth.analytic_fields(1234, 0, 0, W, H, 7)
    ref = dynamics.compute_masks(dP, cp).astype(np.int32)
    assert ref.max() >= 2 * len(S.VOTE_SCENARIOS), "every scenario has a label"
    lg = S.vote_logits(ref, 7)
    want, _ = classmask.compute_class_masks(ref, lg)
    for l in range(1, int(ref.max()) + 1):
        assert np.all(want[ref == l] == S.VOTE_EXPECT[S.VOTE_SCENARIOS[l % len(S.VOTE_SCENARIOS)]])
    t0 = time.perf_counter()
    out = _chain(_lib.lib(), *(torch.from_numpy(a[None]).to(cuda) for a in (dP, cp, lg)))
    print(f"  fused chain, {int(ref.max())} labels: {(time.perf_counter() - t0) * 1e3:.1f} ms")
    assert np.array_equal(out[0][0], ref.astype(np.uint16)), "ids"
    _report_vote("fused chain", out[1][0], want, ref)
    assert np.array_equal(out[3][0]["cls"], classmask.instance_records(ref, want)["cls"]), "the records carry the same classes"


# ---- border removal --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_classes", [False, True])
def test_border_removal_corner_cases(cuda, with_classes):
    for name, m in S.border_cases().items():
        want = classmask.remove_border_instances(m.copy())
        md = torch.from_numpy(m.copy()).to(cuda)[None]
        if with_classes:
            cls = (m % 5 + 1).astype(np.uint8) * (m > 0)
            got, gc = ops.remove_border_instances(md, torch.from_numpy(cls).to(cuda)[None])
            assert np.array_equal(gc.cpu().numpy()[0], cls * (want > 0)), name
        else:
            got = ops.remove_border_instances(md)
        got = got.cpu().numpy()[0]
        print(f"  {name}{' + class map' if with_classes else ''}: ids kept {np.unique(got[got > 0]).tolist()} (reference {np.unique(want[want > 0]).tolist()})")
        assert np.array_equal(got, want), name


def test_border_removal_batch_with_an_empty_tile(cuda):
    c = S.border_cases()
    maps = np.stack([c["corner_pixel"], np.zeros_like(c["corner_pixel"]), c["id_gaps"]])
    cls = ((maps % 3) + 1).astype(np.uint8) * (maps > 0)
    want = np.stack([classmask.remove_border_instances(m.copy()) for m in maps])
    got, gc = ops.remove_border_instances(torch.from_numpy(maps.copy()).to(cuda), torch.from_numpy(cls).to(cuda))
    got, gc = got.cpu().numpy(), gc.cpu().numpy()
    print(f"  nT = 3: ids kept per tile {[np.unique(g[g > 0]).tolist() for g in got]}")
    assert np.array_equal(got, want) and np.array_equal(gc, cls * (want > 0)) and not got[1].any()
