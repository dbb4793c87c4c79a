"""GPU: the stage-wise post-processing entry points on id maps that overflow the per-workgroup LDS label hash
(csrc/cpx_postproc.hip: lh_slot gives up after 8 probes of its 256 slots, and the update then goes to the per-label tables
in global memory).  The fields of the other tests never get there: a workgroup of theirs sees a few dozen labels.

Labels whose home slots lie in a window of k slots can only ever occupy those and the 7 behind them, so MORE than k + 7 such
labels in one workgroup's pixels miss whatever order they arrive in; `_guaranteed_misses` restates the hash and every test
asserts that condition on its own input, so that a change of the hash or of its size cannot quietly end the coverage.
Expected values are numpy's / the oracle's, compared exactly."""
import ctypes as C

import numpy as np
import pytest
import torch

import polygon_shapes as ps
from postproc_shapes import _guaranteed_misses, _home
from classpose_amd import _lib, engine, ops
from classpose_amd._lib import ptr
from oracle import classmask, dynamics

pytestmark = pytest.mark.gpu

H = W = 64
NCLS = 7
LH_SLOTS, LH_PROBES, PP_MAXCLS = 256, 8, 32
STATS_WG, VOTE_WG = 2048, 256                   # pixels per workgroup: the label-run passes (8 per thread), the class vote (1 per thread)
WIN_LO, WIN_K = 99, 61                          # the window of home slots the map's labels come from


@pytest.fixture(scope="module")
def maps():
    """[3, H, W]: tile 0 the overflowing labels in the first workgroup's pixels, tile 1 empty, tile 2 the same ids in the
    second workgroup's"""
    n_lab = H * W // 11 + 2
    assert n_lab == 374 == _lib.lib().cpx_postproc_max_labels(H, W)
    crowd = [l for l in range(1, n_lab) if WIN_LO <= _home(l) < WIN_LO + WIN_K]
    assert len(crowd) == 91
    tile = np.zeros(H * W, np.int32)
    tile[1:2 * len(crowd):2] = crowd                                    # isolated single pixels (rows 0 .. 2), ascending; tile 2 takes them descending
    rest = [l for l in range(1, n_lab) if l not in crowd]
    a, b, c, d = rest[-1], rest[5], rest[-7], rest[40]
    tile = tile.reshape(H, W)
    tile[5, 10:13] = a                                                  # runs of 2 - 3 pixels; b ends at x = W - 1 and c starts at x = 0 of the next row
    tile[6, W - 2:] = b
    tile[7, :3] = c
    tile[7, 5:7] = d
    tile[9, 30:32] = d                                                  # (a second run of the same label, two rows down)
    flat = tile.reshape(-1)
    used = np.flatnonzero(flat)
    assert used.max() < STATS_WG // 2
    other = np.zeros(H * W, np.int32)
    other[STATS_WG + used] = flat[used]
    other[STATS_WG + 1:STATS_WG + 2 * len(crowd):2] = crowd[::-1]
    maps = np.stack([tile, np.zeros((H, W), np.int32), other.reshape(H, W)])
    for t, lo in ((0, 0), (2, STATS_WG)):
        labels = np.unique(maps[t].reshape(-1)[lo:lo + STATS_WG])
        assert labels[0] == 0 and np.array_equal(labels, np.unique(maps[t]))            # the whole tile is one workgroup's
        assert _guaranteed_misses(labels[1:]) >= 91 - (WIN_K + LH_PROBES - 1) == 23
    return maps


def test_instance_records_with_the_label_hash_overflowing(cuda, maps):
    want = [ps.records(m) for m in maps]
    cms = np.stack([ps.class_map(m, r) for m, r in zip(maps, want)])
    L = _lib.lib()
    nT, max_rec, REC = len(maps), 374, engine.RECORD_DTYPE
    d_maps = torch.from_numpy(maps.astype(np.uint16).view(np.int16)).to(cuda)
    d_cm = torch.from_numpy(cms).to(cuda)
    d_recs = torch.zeros(nT * max_rec * C.sizeof(_lib.CpxRecord), dtype=torch.uint8, device=cuda)
    d_cnt = torch.full((nT,), -1, dtype=torch.int32, device=cuda)
    ws = torch.empty(L.cpx_postproc_workspace_bytes(nT, H, W), dtype=torch.uint8, device=cuda)
    _lib.check(L.cpx_instance_records(ptr(d_maps), ptr(d_cm), nT, H, W, max_rec, ptr(d_recs), ptr(d_cnt), ptr(ws),
                                      torch.cuda.current_stream().cuda_stream))
    got, counts = d_recs.cpu().numpy().view(REC).reshape(nT, max_rec), d_cnt.cpu().numpy()
    for t, w in enumerate(want):
        assert counts[t] == int(maps[t].max())
        exp = np.zeros(max_rec, REC)                    # a record sits at slot label - 1; the slots of absent labels stay as they were
        w = w.copy()
        w["tile"] = t
        exp[w["label"] - 1] = w
        for name in REC.names:
            assert np.array_equal(got[t][name], exp[name]), (t, name)


def test_fill_holes_and_size_filter_with_the_label_hash_overflowing(cuda, maps):
    out, nlab = ops.fill_holes_and_remove_small_masks(torch.from_numpy(maps.copy()).to(cuda), 1)
    out, nlab = out.cpu().numpy(), nlab.cpu().numpy()
    for t, m in enumerate(maps):
        ref = dynamics.fill_holes_and_remove_small_masks(m.astype(np.uint16), 1)
        assert np.array_equal(out[t], ref.astype(np.int32)), t
        assert nlab[t] == ref.max() == len(np.unique(m)) - 1


def _vote_logits(maps):
    """the vote's keys are label * 32 + class + 1: every labelled pixel whose label has a class that puts its key into one
    32-slot window of home slots (the window that most labels can reach) gets that class, the others what the noise gives"""
    def classes_into(l, lo):
        return [c for c in range(NCLS) if lo <= _home(l * PP_MAXCLS + c + 1) < lo + 32]
    labels = [int(l) for l in np.unique(maps[0])[1:]]
    lo = max(range(LH_SLOTS - 32), key=lambda s: sum(bool(classes_into(l, s)) for l in labels))
    logits = np.random.default_rng(11).standard_normal((len(maps), NCLS, H * W)).astype(np.float32)
    for t, m in enumerate(maps):
        for p in np.flatnonzero(m):
            hit = classes_into(int(m.reshape(-1)[p]), lo)
            if hit:
                logits[t, hit[0], p] = 10.0
    for t, first in ((0, 0), (2, STATS_WG)):
        px = slice(first, first + VOTE_WG)                                              # one workgroup of the vote has all of the crowd
        lab, cls = maps[t].reshape(-1)[px], logits[t, :, px].argmax(0)
        assert np.count_nonzero(lab) >= 91
        assert _guaranteed_misses(lab[lab > 0] * PP_MAXCLS + cls[lab > 0] + 1) > 0
    return logits.reshape(len(maps), NCLS, H, W)


def test_class_vote_with_the_label_hash_overflowing(cuda, maps):
    logits = _vote_logits(maps)
    cm = ops.compute_class_masks(torch.from_numpy(maps).to(cuda), torch.from_numpy(logits).to(cuda)).cpu().numpy()
    for t, m in enumerate(maps):
        ref, _ = classmask.compute_class_masks(m, logits[t])
        assert np.array_equal(cm[t].astype(np.int64), ref), t
        assert t == 1 or len(np.unique(ref)) > 2
