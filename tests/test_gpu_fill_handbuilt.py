"""GPU: the hole fill, the two size filters, the renumbering and the per-cell records on inputs built by hand
(tests/fill_shapes.py; every premise is proved on the CPU by tests/test_fill_shapes_host.py).  The maps sit on the kernels'
constants: boxes of 64 / 65 and 256 / 257 pixels, holes on and across bit 63 / 64 of a row word and lane 63 / 0 of a row block,
channels that only the right-to-left carry or the neighbouring row block can reach, more mid-size labels than waves, label
counts at the slices of the size filters and at both sides of the tail's LDS table, records with fewer slots than labels and
coordinate sums past 2^32, min_size <= 0.

Yardsticks, none of them the code under test, all compared exactly (every pixel, every count, every field of every record):
  * A, the stage entry: ``oracle.dynamics.fill_holes_and_remove_small_masks``;
  * B, cpx_instance_records through the raw ABI: ``oracle.classmask.instance_records``;
  * C, cpx_compute_masks_records of the product library (fused chain), of the debug library with the stage-wise chain, and
    ``oracle.dynamics.compute_masks`` + ``instance_records``.
Every test prints what it measured before it asserts (run with -s)."""
from __future__ import annotations

import ctypes as C
import time

import numpy as np
import pytest
import torch

import fill_shapes as S
from classpose_amd import _lib, engine, ops
from classpose_amd._lib import ptr
from oracle import classmask, dynamics
from test_gpu_postproc import _chain

pytestmark = pytest.mark.gpu

_cache = {}


def _once(key, f):
    """a reference is computed once, shared and never modified"""
    if key not in _cache:
        _cache[key] = f()
        for a in (_cache[key] if isinstance(_cache[key], tuple) else (_cache[key],)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


def _fill_ref(m, min_size):
    return dynamics.fill_holes_and_remove_small_masks(m.astype(np.uint16), min_size).astype(np.int32)


def _count(m, ref, min_size):
    """what the entry reports: the labels of the result, or at min_size <= 0 the ids present before the fill"""
    return int(ref.max()) if min_size > 0 else len(np.unique(m[m > 0]))


def _fill(cuda, maps, min_size):
    assert maps.min() >= 0 and maps.max() < S.max_labels(*maps.shape[1:]), "ids within the tables"
    d = torch.from_numpy(maps.copy()).to(cuda)
    t0 = time.perf_counter()
    out, nlab = ops.fill_holes_and_remove_small_masks(d, min_size)
    out, nlab = out.cpu().numpy(), nlab.cpu().numpy()
    return out, nlab, time.perf_counter() - t0


# ---- A: the stage entry ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.STAGE_CASES))
def test_stage_entry_equals_the_oracle_on_hand_built_maps(cuda, name):
    c = S.STAGE_CASES[name]()
    ref = _once(("stage", name), lambda: _fill_ref(c.m, c.min_size))
    got, nlab, dt = _fill(cuda, c.m[None], c.min_size)
    want_n = _count(c.m, ref, c.min_size)
    print(f"  {name}: {c.m.shape[0]} x {c.m.shape[1]}, min_size {c.min_size}, path {c.path}: {int((got[0] != ref).sum())} ids differ (tolerance 0), "
          f"ids {np.unique(got[0])[:6].tolist()} (oracle {np.unique(ref)[:6].tolist()}), nlabels {int(nlab[0])} (want {want_n}); {dt * 1e3:.1f} ms")
    assert np.array_equal(got[0], ref), name
    assert int(nlab[0]) == want_n and (c.nlab is None or want_n == c.nlab), name
    if c.filled is not None:
        assert int(((c.m == 0) & (got[0] > 0)).sum()) == c.filled


def _batch_ref():
    maps, _ = S.batch_tiles()
    return maps, np.stack([_fill_ref(m, S.BATCH_MIN_SIZE) for m in maps])


def test_batch_with_another_path_in_every_tile_and_its_reverse_through_one_workspace(cuda):
    """nT = 8: empty, no background, small, mid, conflict, a box above 256, 2 000 labels, one label -- then the same tiles in reverse
    order through the same cached workspace, and the first order again: a flag or a table that one tile or one call leaves behind
    would reach another tile"""
    maps, refs = _once("batch", _batch_ref)
    for order in (list(range(8)), list(range(7, -1, -1)), list(range(8))):
        got, nlab, dt = _fill(cuda, maps[order], S.BATCH_MIN_SIZE)
        print(f"  order {order}: ids that differ per tile {[int((got[i] != refs[t]).sum()) for i, t in enumerate(order)]}, nlabels {nlab.tolist()}; {dt * 1e3:.1f} ms")
        for i, t in enumerate(order):
            assert np.array_equal(got[i], refs[t]), (order, t)
            assert int(nlab[i]) == int(refs[t].max()), (order, t)


def test_min_size_zero_in_a_batch_after_a_filtering_call(cuda):
    """the workspace of a min_size > 0 call (flags, ranks) is reused by a min_size <= 0 call on tiles of the same shape"""
    a, b, n = S.nonpositive(0, True).m, S.nonpositive(0, True, True).m, S.nonpositive(0, False).m
    maps = np.stack([a, b, np.zeros_like(a), n])
    _fill(cuda, maps, 15)
    for ms in (0, -1):
        got, nlab, dt = _fill(cuda, maps, ms)
        refs = [_fill_ref(m, ms) for m in maps]
        print(f"  min_size {ms}: ids per tile {[np.unique(g).tolist() for g in got]}, nlabels {nlab.tolist()} (want [3, 4, 0, 3]); {dt * 1e3:.1f} ms")
        assert all(np.array_equal(g, r) for g, r in zip(got, refs)) and nlab.tolist() == [3, 4, 0, 3]


# ---- B: the records ----------------------------------------------------------------------------------------------------------
REC = engine.RECORD_DTYPE
CANARY = 0xA5


def _records(cuda, maps, cms, max_rec, spare=2):
    """cpx_instance_records through the raw ABI into a buffer of canary bytes with `spare` slots behind the last tile's"""
    L = _lib.lib()
    nT, H, W = maps.shape
    assert REC.itemsize == C.sizeof(_lib.CpxRecord) and maps.dtype == np.uint16 and int(maps.max()) < S.max_labels(H, W)
    d_maps = torch.from_numpy(maps.view(np.int16)).to(cuda)
    d_cm = torch.from_numpy(cms).to(cuda)
    d_recs = torch.full(((nT * max_rec + spare) * REC.itemsize,), CANARY, dtype=torch.uint8, device=cuda)
    d_cnt = torch.full((nT,), -1, dtype=torch.int32, device=cuda)
    nbytes = L.cpx_postproc_workspace_bytes(nT, H, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=cuda)
    t0 = time.perf_counter()
    _lib.check(L.cpx_instance_records(ptr(d_maps), ptr(d_cm), nT, H, W, max_rec, ptr(d_recs), ptr(d_cnt), ptr(ws),
                                      torch.cuda.current_stream().cuda_stream))
    got, counts = d_recs.cpu().numpy().view(REC), d_cnt.cpu().numpy()
    return got, counts, nbytes, time.perf_counter() - t0


def _expected_records(maps, cms, max_rec, spare=2):
    exp = np.frombuffer(bytes([CANARY]) * ((len(maps) * max_rec + spare) * REC.itemsize), REC).copy()
    for t, (m, cm) in enumerate(zip(maps, cms)):
        if not m.any():
            continue
        r = classmask.instance_records(m, cm)
        for l in np.unique(m[m > 0]):
            if l - 1 < max_rec:
                e = exp[t * max_rec + l - 1:t * max_rec + l]
                e["tile"], e["label"], e["cls"], e["area"] = t, l, r["cls"][l - 1], r["area"][l - 1]
                e["y0"], e["x0"], e["y1"], e["x1"] = r["bbox"][l - 1]
                e["sum_y"], e["sum_x"] = r["sum_y"][l - 1], r["sum_x"][l - 1]
    return exp


def _check_records(name, got, counts, maps, exp):
    bad = [f for f in REC.names if not np.array_equal(got[f], exp[f])]
    print(f"  {name}: counts {counts.tolist()} (largest ids {[int(m.max()) for m in maps]}), fields that differ {bad} (tolerance 0), "
          f"{int((got.view(np.uint8).reshape(-1, REC.itemsize) == CANARY).all(1).sum())} of {len(got)} slots untouched")
    assert counts.tolist() == [int(m.max()) for m in maps], name
    for f in REC.names:
        assert np.array_equal(got[f], exp[f]), (name, f)
    assert got.tobytes() == exp.tobytes(), name


def _odd_maps():
    m = S.odd_tile().m.astype(np.uint16)
    return m, np.where(m == 1, 0, m).astype(np.uint16), np.ascontiguousarray(m[:, ::-1])


def test_records_of_the_odd_tile_with_id_gaps(cuda):
    m = _odd_maps()[0][None]
    cms = S.class_map_of(m)
    max_rec = S.max_labels(*m.shape[1:])
    got, counts, _, dt = _records(cuda, m, cms, max_rec)
    _check_records(f"67 x 93, ids {np.unique(m)[1:].tolist()}, {dt * 1e3:.1f} ms", got, counts, m, _expected_records(m, cms, max_rec))
    assert (got[[1, 3, 4, 7]].view(np.uint8) == CANARY).all(), "the slots of the absent ids 2, 4, 5, 8 keep the canary"


def test_records_with_fewer_slots_than_labels(cuda):
    """max_rec = 5 < the largest id 13: counts still say 13, ids 6 .. 13 are not written anywhere -- id 6 = max_rec + 1 is present, its
    record would land in the next tile's first slot; tile 1 has no id 1, so that slot keeps the canary, as do the spare slots
    behind the last tile"""
    a, b, _ = _odd_maps()
    maps = np.stack([a, b])
    cms = S.class_map_of(maps)
    assert 6 in maps[0] and 6 in maps[1] and 1 not in maps[1]
    got, counts, _, dt = _records(cuda, maps, cms, 5)
    _check_records(f"max_rec 5, nT 2, {dt * 1e3:.1f} ms", got, counts, maps, _expected_records(maps, cms, 5))
    assert (got[[1, 3, 4, 5, 6, 8, 9, 10, 11]].view(np.uint8) == CANARY).all() and got["label"][[0, 2, 7]].tolist() == [1, 3, 3]


def test_records_of_a_batch_with_an_empty_middle_tile(cuda):
    a, _, f = _odd_maps()
    maps = np.stack([a, np.zeros_like(a), f])
    cms = S.class_map_of(maps)
    got, counts, _, dt = _records(cuda, maps, cms, 20)
    _check_records(f"nT 3, empty middle tile, {dt * 1e3:.1f} ms", got, counts, maps, _expected_records(maps, cms, 20))
    assert counts[1] == 0 and (got[20:40].view(np.uint8) == CANARY).all()


def test_records_with_a_coordinate_sum_past_two_to_the_32(cuda):
    m = S.wide_label()[None]
    cms = S.class_map_of(m)
    got, counts, nbytes, dt = _records(cuda, m, cms, 3)
    want = 40 * (16383 * 16384 // 2)
    print(f"  48 x 16 384: workspace {nbytes} bytes ({nbytes / 2 ** 20:.1f} MiB); sum_x {int(got['sum_x'][0])} (want {want} = {want / 2 ** 32:.3f} x 2^32), "
          f"sum_y {int(got['sum_y'][0])}; {dt * 1e3:.1f} ms")
    assert nbytes < 2 ** 28
    exp = np.frombuffer(bytes([CANARY]) * (5 * REC.itemsize), REC).copy()
    exp[0] = (0, 1, int(cms[0, 3, 0]), 40 * 16384, 3, 0, 43, 16384, 16384 * sum(range(3, 43)), want)
    _check_records("48 x 16 384", got, counts, m, exp)


# ---- C: both chains, from fields built out of hand maps --------------------------------------------------------------------------
def _chain_ref(dP, cp):
    """oracle: (ids uint16, records with every field but the tile) of one tile; min_size 15, no flow-error filter"""
    ids = dynamics.compute_masks(dP, cp, flow_threshold=None).astype(np.uint16)
    n = int(ids.max())
    exp = np.zeros(n, REC)
    if n:
        r = classmask.instance_records(ids, np.zeros(ids.shape, np.uint8))
        exp["label"], exp["cls"], exp["area"] = np.arange(1, n + 1), r["cls"], r["area"]
        exp["y0"], exp["x0"], exp["y1"], exp["x1"] = r["bbox"].T
        exp["sum_y"], exp["sum_x"] = r["sum_y"], r["sum_x"]
    return ids, exp


def _sparse_grid(H, W):
    on = {(1, 2), (9, 4), (15, 15), (0, W // 6 - 1), (H // 6 - 1, 0)}
    return S.grid_field(H, W, off=tuple((r, c) for r in range(H // 6) for c in range(W // 6) if (r, c) not in on))


def _ring(side, inner):
    return S.ring_field(side, inner)[1]


def _bars_flipped():
    dP, cp = S.bars_field()[1]
    return np.ascontiguousarray(np.stack([dP[0, :, ::-1], -dP[1, :, ::-1]])), np.ascontiguousarray(cp[:, ::-1])


FIELDS = {
    **{f"ring_{s}{'_inner' if i else ''}": (lambda s=s, i=i: _ring(s, i)) for s in S.RING_SIDES for i in (False, True)},
    "bars": lambda: S.bars_field()[1],
    "bars_flipped": _bars_flipped,
    "empty_64": lambda: (np.zeros((2, 64, 64), np.float32), np.full((64, 64), -1.0, np.float32)),
    **{f"grid_{k}": v[0] for k, v in S.GRIDS.items()},
    "sparse_192x198": lambda: _sparse_grid(192, 198),
    "sparse_96x102": lambda: _sparse_grid(96, 102),
    "sparse_96x96": lambda: _sparse_grid(96, 96),
    "sparse_96x98": lambda: _sparse_grid(96, 98),
}
SINGLE = [k for k in FIELDS if not k.startswith(("sparse", "empty", "bars_flipped"))]
BATCHES = {
    **{f"rings_{s}": [f"ring_{s}", f"ring_{s}_inner"] for s in S.RING_SIDES},
    "bars": ["bars", "empty_64", "bars_flipped", "bars"],
    "grids_192x198": ["sparse_192x198", "grid_192x198", "grid_192x198_trim3", "grid_192x198_off31", "sparse_192x198"],
    "grids_96x96": ["grid_96x96_trim1", "sparse_96x96", "grid_96x96_off1"],
    "grids_96x102": ["grid_96x102", "grid_96x102_off15", "sparse_96x102"],
    "grids_96x98": ["sparse_96x98", "grid_96x98"],
}


def _three_ways(cuda, names):
    fields = [_once(("field", n), FIELDS[n]) for n in names]
    refs = [_once(("chain", n), lambda f=f: _chain_ref(*f)) for n, f in zip(names, fields)]
    dP = torch.from_numpy(np.stack([f[0] for f in fields])).to(cuda)
    cp = torch.from_numpy(np.stack([f[1] for f in fields])).to(cuda)
    t0 = time.perf_counter()
    product = _chain(_lib.lib(), dP, cp, None, flow_threshold=0.0)
    dt = time.perf_counter() - t0
    with _lib.use_debug_library() as L:
        L.cpx_postproc_set_fused(0)
        try:
            staged = _chain(L, dP, cp, None, flow_threshold=0.0)
        finally:
            L.cpx_postproc_set_fused(1)
    assert product[5] < staged[5], "the product library ran the fused chain, the debug library the stage-wise one"
    for way, got in (("fused", product), ("stage-wise", staged)):
        for t, (n, (ids, exp)) in enumerate(zip(names, refs)):
            r = got[3][t]
            bad = [f for f in REC.names if f != "tile" and (len(r) != len(exp) or not np.array_equal(r[f], exp[f]))]
            print(f"  {way}, tile {t} ({n}): {int((got[0][t] != ids).sum())} ids differ (tolerance 0), nlabels {int(got[2][t])}, records {int(got[4][t])} "
                  f"(oracle {int(ids.max())}), record fields that differ {bad}" + (f"; {dt * 1e3:.1f} ms for the batch" if way == "fused" and t == 0 else ""))
    for way, got in (("fused", product), ("stage-wise", staged)):
        for t, (n, (ids, exp)) in enumerate(zip(names, refs)):
            assert np.array_equal(got[0][t], ids), (way, n)
            assert int(got[2][t]) == int(got[4][t]) == int(ids.max()) == len(got[3][t]), (way, n)
            for f in REC.names:
                assert np.array_equal(got[3][t][f], np.full(len(exp), t) if f == "tile" else exp[f]), (way, n, f)
            assert not got[1][t].any(), "no vote: class 0"
    return refs


@pytest.mark.parametrize("name", SINGLE)
def test_both_chains_equal_the_oracle_on_single_tiles(cuda, name):
    (ids, exp), = _three_ways(cuda, [name])
    if name.startswith("ring"):
        side = int(name.split("_")[1])
        assert ids.max() == 1 and exp["area"][0] == side * side and exp["y1"][0] - exp["y0"][0] == side, "one filled square"
    elif name == "bars":
        assert exp["area"].tolist() == [15, 16, 15]
    else:
        assert ids.max() == S.GRIDS[name[5:]][4]


@pytest.mark.parametrize("name", list(BATCHES))
def test_both_chains_equal_the_oracle_on_batches_of_sparse_and_dense_tiles(cuda, name):
    refs = _three_ways(cuda, BATCHES[name])
    counts = [int(r[0].max()) for r in refs]
    print(f"  labels per tile {counts}")
    if name.startswith("grids"):
        assert min(counts) == 5 and max(counts) >= 240, "a sparse tile next to a dense one"
