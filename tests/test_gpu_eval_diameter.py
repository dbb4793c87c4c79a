"""``ClassposeModel.eval(diameter=)`` and ``Engine(net_hw=, resample=)`` on the device: against the reference's own run
(tests/golden/reference_eval_diameter.npz) with the network fields injected, and against the hand composition of the existing
ops with the synthetic network.  Everything is compared bit for bit."""
from __future__ import annotations

import os
import sys

import numpy as np
import pytest
import torch

import resize_reference as rr
from classpose_amd import engine, ops, synth
from classpose_amd.models import ClassposeModel

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))

pytestmark = pytest.mark.gpu

NCLS = 4
_cache: dict = {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _fixture():
    import make_golden_eval_diameter as mgd
    if "g" not in _cache:
        _cache["g"], _cache["tile"] = np.load(mgd.FIXTURE), mgd.diameter_tile()
        assert int(_cache["tile"].astype(np.int64).sum()) == int(_cache["g"]["tilesum"])
    return mgd, _cache["g"], _cache["tile"]


def _net_fields(tile, Hs, Ws):
    """what the reference's network stage hands on at network size, on the CPU (oracle.tiling + the stand-in decode_net)"""
    import make_golden_eval as mge
    from oracle import tiling
    key = ("fields", Hs, Ws)
    if key not in _cache:
        x = tiling.normalize_img(tiling.resize_linear_u8(tile, Ws, Hs)[None])

        def fw(im):
            o = mge.decode_net(torch.from_numpy(np.ascontiguousarray(im)), mge.NCLS).numpy()
            return o[:, mge.NCLS:], o[:, :mge.NCLS]
        _cache[key] = tiling.run_net(fw, x, batch_size=8, augment=False, tile_overlap=0.1, bsize=256)
    return _cache[key]


def _weights(cuda, depth):
    key = ("w", depth)
    if key not in _cache:
        _cache[key] = engine.NetWeights.from_state_dict(synth.make_state_dict(NCLS, None, depth=depth, seed=7), "bf16", cuda)
    return _cache[key]


def _model(cuda):
    if "model" not in _cache:
        _cache["model"] = ClassposeModel(pretrained_model=synth.make_state_dict(NCLS, None, depth=2, seed=7), device=cuda,
                                         precision="bf16", max_batch_tiles=2)
    return _cache["model"]


def _net_hw(H, W, d):
    return int(H * (30.0 / d)), int(W * (30.0 / d))


@pytest.mark.parametrize("row", range(5))
def test_engine_with_injected_fields_equals_reference_eval(cuda, row):
    """fixture row `row`: the reference's network-size fields go in, ids, classes and the fields at tile size come out as the
    reference returned them"""
    mgd, g, tile = _fixture()
    diam, resample = mgd.ROWS[row]
    H, W = tile.shape[:2]
    Hs, Ws = _net_hw(H, W, diam)
    dP, cp, yc = _net_fields(tile, Hs, Ws)
    eng = engine.Engine(_weights(cuda, 1), H, W, batch_tiles=1, net_hw=(Hs, Ws), resample=resample)
    assert eng.rescaled == ((Hs, Ws) != (H, W))
    inj = tuple(torch.from_numpy(np.ascontiguousarray(a)[None]).to(cuda) for a in (dP, cp, yc))
    o = eng.run(torch.from_numpy(tile[None]).to(cuda), inject=inj, records=resample)
    assert o.masks.shape == (1, H, W) and o.class_masks.shape == (1, H, W) and o.dP.shape == (1, 2, H, W)
    assert o.cellprob.shape == (1, H, W) and o.logits.shape == (1, NCLS, H, W)
    masks = ops.masks_to_numpy(o.masks)[0]
    assert np.array_equal(masks, g[f"{row}_masks"]) and int(masks.max()) == mgd.CELLS[row] == int(o.nlabels[0])
    assert np.array_equal(o.class_masks[0].cpu().numpy(), g[f"{row}_class_masks"])
    # an engine that does not rescale hands back the injected fields' slot buffers, like before: compare what the dynamics consumed
    got = (inj[0][0], inj[1][0], inj[2][0]) if not eng.rescaled else (o.dP[0], o.cellprob[0], o.logits[0])
    for name, a in zip(("dP", "cellprob", "yclass"), got):
        assert np.array_equal(_bits(a.cpu().numpy()[..., ::4, ::4]), _bits(g[f"{row}_{name}"])), name
    if resample and eng.rescaled:           # records are in tile coordinates: one per cell, areas those of the id map
        rec = eng.fetch_records(1, o)
        assert len(rec) == mgd.CELLS[row] and np.array_equal(np.sort(rec["area"]), np.sort(np.bincount(masks.ravel())[1:]))


def _hand_composition(cuda, model, tile, d):
    """u8 resize to the truncated sizes -> a plain Engine at network size -> ops.resize_fields -> ops.compute_masks"""
    H, W = tile.shape[:2]
    Hs, Ws = _net_hw(H, W, d)
    t = torch.from_numpy(tile[None]).to(cuda)
    small = ops.resize_u8(t, Hs, Ws)
    eng = engine.Engine(model.weights, Hs, Ws, batch_tiles=model.max_batch_tiles)
    o = eng.run(small, records=False)
    return (Hs, Ws), o, small


@pytest.mark.parametrize("d", [20, 45])
def test_eval_diameter_equals_hand_composition(cuda, d):
    _mgd, _g, tile = _fixture()
    model = _model(cuda)
    H, W = tile.shape[:2]
    (Hs, Ws), o, small = _hand_composition(cuda, model, tile, d)
    from oracle import tiling
    assert np.array_equal(small[0].cpu().numpy(), tiling.resize_linear_u8(tile, Ws, Hs))
    dP, cp, lg = (ops.resize_fields(a, H, W) for a in (o.dP, o.cellprob, o.logits))
    m, cm, nl = ops.compute_masks(dP, cp, lg)
    masks, flows, class_masks, styles = model.eval(tile, diameter=d)
    assert masks.dtype == np.uint16 and masks.shape == (H, W) and np.array_equal(masks, ops.masks_to_numpy(m)[0])
    assert class_masks.dtype == np.int64 and np.array_equal(class_masks, cm[0].cpu().numpy())
    assert np.array_equal(_bits(flows[1]), _bits(dP[0].cpu().numpy())) and flows[1].shape == (2, H, W)
    assert np.array_equal(_bits(flows[2]), _bits(cp[0].cpu().numpy()))
    assert np.array_equal(_bits(flows[3]), _bits(lg[0].cpu().numpy())) and flows[3].shape == (NCLS, H, W)
    assert flows[0].shape == (H, W, 3) and flows[4] == (1, Hs, Ws, 3) and styles.shape == (256,)
    # and the fields are the CPU restatement's resize of the network-size fields
    assert np.array_equal(_bits(flows[1]), _bits(rr.resize_linear_f32(o.dP[0].cpu().numpy(), H, W)))


def test_diameter_30_is_diameter_none(cuda):
    _mgd, _g, tile = _fixture()
    model = _model(cuda)
    a, b = model.eval(tile, diameter=30.0), model.eval(tile)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2]) and a[1][4] == b[1][4] == (1, *tile.shape)
    for k in (0, 1, 2, 3):
        assert np.array_equal(a[1][k], b[1][k], equal_nan=True) and a[1][k].dtype == b[1][k].dtype
    c = model.eval(tile, diameter=30.0, resample=False)              # nothing to resample without a rescale
    assert np.array_equal(c[0], b[0]) and np.array_equal(_bits(c[1][1]), _bits(b[1][1]))


def test_list_of_diameters_equals_single_calls(cuda):
    _mgd, _g, tile = _fixture()
    model = _model(cuda)
    other = np.ascontiguousarray(tile[::-1])
    masks, flows, class_masks, _ = model.eval([tile, other], diameter=[20, 45])
    for i, (im, d) in enumerate(((tile, 20), (other, 45))):
        m1, f1, c1, _ = model.eval(im, diameter=d)
        assert np.array_equal(masks[i], m1) and np.array_equal(class_masks[i], c1) and flows[i][4] == f1[4]
        assert all(np.array_equal(_bits(flows[i][k]), _bits(f1[k])) for k in (1, 2, 3))
    same, _f, _c, _ = model.eval([tile, other], diameter=np.array([45.0, 45.0]))      # one group, one batch of two
    assert np.array_equal(same[1], masks[1])
    with pytest.raises(ValueError, match="entries"):
        model.eval([tile, other], diameter=[20.0])


def test_resample_false_returns_the_network_size_ids_at_tile_size(cuda):
    _mgd, _g, tile = _fixture()
    model = _model(cuda)
    H, W = tile.shape[:2]
    (Hs, Ws), o, _small = _hand_composition(cuda, model, tile, 45)
    ids_net, cls_net = ops.masks_to_numpy(o.masks)[0], o.class_masks[0].cpu().numpy()
    assert ids_net.shape == (Hs, Ws)
    masks, flows, class_masks, _ = model.eval(tile, diameter=45, resample=False)
    assert masks.shape == (H, W) and np.array_equal(masks, rr.resize_nearest(ids_net, H, W))
    assert np.array_equal(class_masks, rr.resize_nearest(cls_net, H, W))
    assert np.array_equal(np.unique(masks), np.unique(ids_net))                # upscaling by nearest loses no id
    for k, a in ((1, o.dP), (2, o.cellprob), (3, o.logits)):
        assert np.array_equal(_bits(flows[k]), _bits(rr.resize_linear_f32(a[0].cpu().numpy(), H, W)))
    assert flows[4] == (1, Hs, Ws, 3)


def test_errors(cuda):
    _mgd, _g, tile = _fixture()
    model = _model(cuda)
    for bad in (0, -3.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="diameter"):
            model.eval(tile, diameter=bad)
    with pytest.raises(ValueError, match="diameter=1.0.*16x16"):              # 200 x 232 -> 6000 x 6960: a 29 x 33 sub-tile grid
        model.eval(tile, diameter=1.0)
    with pytest.raises(ValueError, match="diameter"):                         # 200 x 232 -> 0 x 0
        model.eval(tile, diameter=1e4)
    eng = engine.Engine(_weights(cuda, 1), 200, 232, batch_tiles=1, net_hw=(133, 154), resample=False)
    t = torch.from_numpy(tile[None]).to(cuda)
    with pytest.raises(ValueError, match="resample=False"):
        eng.run(t, records=True)
    with pytest.raises(ValueError, match="resample=False"):
        eng.run(t, records=False, polygons=(1.0, [[0, 0]]))
    with pytest.raises(ValueError, match="network size"):                     # inject fields are at network size
        z = torch.zeros((1, 2, 200, 232), device=cuda)
        engine.Engine(_weights(cuda, 1), 200, 232, batch_tiles=1, net_hw=(133, 154)).run(t, inject=(z, z[:, 0], z), records=False)
    with pytest.raises(ValueError):
        engine.Engine(_weights(cuda, 1), 200, 232, batch_tiles=1, net_hw=(0, 154))


def test_default_engine_has_no_resize_buffers_and_launches_nothing_new(cuda):
    """net_hw absent or equal to the tile size: the same buffers, the same post-processing launch count and the same bits"""
    from classpose_amd import _lib
    _mgd, _g, tile = _fixture()
    w = _weights(cuda, 1)
    t = torch.from_numpy(tile[None]).to(cuda)
    L = _lib.lib()
    outs, launches = [], []
    for kw in ({}, dict(net_hw=(200, 232), resample=False)):
        eng = engine.Engine(w, 200, 232, batch_tiles=1, **kw)
        assert not eng.rescaled and not any(hasattr(sl, "tiles_net") or hasattr(sl, "out_dP") for sl in eng.slots)
        n0 = L.cpx_postproc_launch_count()
        o = eng.run(t)
        launches.append(L.cpx_postproc_launch_count() - n0)
        torch.cuda.synchronize()
        assert o.dP.data_ptr() == eng.slots[0].dP.data_ptr() and o.masks.data_ptr() == eng.slots[0].masks.data_ptr()
        outs.append([x.clone() for x in (o.masks, o.class_masks, o.dP, o.cellprob, o.logits)])
    assert launches[0] == launches[1] and all(torch.equal(a, b) for a, b in zip(*outs))
