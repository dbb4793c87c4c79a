"""CPU: the host side of training the UNet semantic head -- the float64 restatement against the reference's own numbers, the
flat parameter layout and its pack / unpack helpers, the fresh head, the command line's structure check, the bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import unet_train_reference as ur
from classpose_amd import _lib, engine, synth, train, train_unet
from classpose_amd.entrypoints import train_head

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "reference_unet_train.npz"))
FTS, NCLS = [int(c) for c in GOLD["fts"]], int(GOLD["ncls"])
NEW = ("cpx_unet_wgrad_slab_rows", "cpx_unet_param_layout", "cpx_unet_refresh_operands", "cpx_unet_backward_workspace_bytes",
       "cpx_unet_grad_layout", "cpx_unet_head_backward")


def _close(got, ref, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = float(np.abs(ref).max()) or 1.0
    err = float(np.abs(got - ref).max()) / scale
    assert err <= 1e-12, f"{what}: {err:.3e}"
    return err


@pytest.mark.parametrize("name", ["b1", "b2w"])
def test_restatement_equals_reference(name):
    """unet_forward + pixel_logits + class_loss under float64 autograd == the reference's UNet, pixel shuffle, _loss_fn_class,
    _loss_fn_tversky and LossAggregator, to 1e-12 (largest difference relative to the largest magnitude of each array)"""
    nI = GOLD[name + "_labels"].shape[0]
    feat = ur.make_feat(nI, nI)
    _close([float(feat.sum()), float(feat.abs().sum())], GOLD[name + "_feat_sums"], "features")
    sd = ur.make_params(FTS, NCLS, 1)
    cw = GOLD[name + "_weights"] if name + "_weights" in GOLD.files else None
    r = ur.loss_and_grads(sd, feat, torch.from_numpy(GOLD[name + "_labels"].astype(np.int64)), FTS, NCLS, class_weights=cw)
    worst = _close([float(r["ce"]), float(r["tversky"]), float(r["loss"])], GOLD[name + "_losses"], "losses")
    # the reference's logits are [B, ncls, 256, 256]; its gradient with respect to them, by autograd of the restated pixel shuffle
    z = r["logits"].numpy().reshape(-1)
    st = int(GOLD["stride"])
    worst = max(worst, _close(z[::st], GOLD[name + "_logits_sample"], "logits sample"))
    worst = max(worst, _close([z.sum(), np.abs(z).sum()], GOLD[name + "_logits_sums"], "logits sums"))
    gst = int(GOLD["gstride"])
    for k in ur.unet_keys(FTS):
        g = r["grads"][k].numpy().reshape(-1)
        ref = GOLD[f"{name}_g:{k.removeprefix('out_class.')}"]
        worst = max(worst, _close(g if g.size <= 2048 else g[::gst], ref, k))
        worst = max(worst, _close([g.sum(), np.abs(g).sum()], GOLD[f"{name}_gs:{k.removeprefix('out_class.')}"], k + " sums"))
    print(f"{name}: restatement vs reference, worst scaled error {worst:.3e}")


def test_dlogits_of_restatement_equal_reference():
    """d loss / d logits of the restatement (autograd on the logits alone) == the reference's y.grad sample"""
    from train_reference import loss_and_grad
    for name in ("b1", "b2w"):
        nI = GOLD[name + "_labels"].shape[0]
        sd = {k: v.double() for k, v in ur.make_params(FTS, NCLS, 1).items()}
        z = ur.pixel_logits(ur.unet_forward(sd, ur.make_feat(nI, nI), len(FTS)), NCLS)
        cw = GOLD[name + "_weights"] if name + "_weights" in GOLD.files else None
        r = loss_and_grad(z, torch.from_numpy(GOLD[name + "_labels"].astype(np.int64)), cw)
        dz = r["dlogits"].numpy().reshape(-1)
        _close(dz[::int(GOLD["stride"])], GOLD[name + "_dlogits_sample"], "dlogits sample")
        _close([dz.sum(), np.abs(dz).sum()], GOLD[name + "_dlogits_sums"], "dlogits sums")


def test_key_order_and_shapes_match_reference():
    keys = [str(k) for k in GOLD["keys"]]
    shapes = [tuple(int(x) for x in str(s).split()) for s in GOLD["shapes"]]
    assert [k.removeprefix("out_class.") for k in ur.unet_keys(FTS)] == keys
    sd = ur.make_params(FTS, NCLS, 1)
    assert [tuple(sd["out_class." + k].shape) for k in keys] == shapes
    fresh = train_unet.fresh_unet_head(FTS, NCLS, head_seed=3)
    assert sorted(k for k in fresh if k != "W3") == sorted("out_class." + k for k in keys)
    assert all(tuple(fresh["out_class." + k].shape) == s for k, s in zip(keys, shapes))
    assert tuple(fresh["W3"].shape) == (NCLS * 64, NCLS, 8, 8)


def test_fresh_head_is_seeded_and_scaled():
    a, b, c = (train_unet.fresh_unet_head([16, 24], 3, head_seed=s) for s in (5, 5, 6))
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(a[k], c[k]) for k in a)
    for k, v in a.items():
        if k.endswith(".weight"):
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]          # ConvTranspose2d [cin][cout][2][2]: torch takes size(1) too
            bound = 1.0 / np.sqrt(fan_in)
            assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.9 * bound, k
            assert float(a[k[:-6] + "bias"].abs().max()) <= bound
    with pytest.raises(ValueError):
        train_unet.fresh_unet_head([8, 8, 8, 8, 8], 3)
    with pytest.raises(ValueError):
        train_unet.fresh_unet_head([8, 8], 1)


@pytest.mark.parametrize("fts", [[64, 128], [20, 36], [12, 20, 36, 68]], ids=lambda f: "-".join(map(str, f)))
def test_pack_unpack_and_operands(fts):
    """pack -> unpack is the identity; packing equals, bit for bit, the operands NetWeights.from_state_dict(sd, "fp32", "cpu")
    builds (fp32: the rounded master is the master); the host's layout is the library's"""
    ncls = 3
    sd = synth.make_state_dict(ncls, fts, depth=1, seed=4)
    flat = train_unet.pack_params(sd, fts, ncls * 64)
    back = train_unet.unpack_params(flat, fts, ncls * 64)
    plan = train_unet.unet_plan(fts, ncls * 64)
    assert sorted(back) == sorted(k + s for k, *_ in plan for s in (".weight", ".bias"))
    assert sorted(back) == sorted(k for k in sd if k.startswith("out_class."))
    for k, v in back.items():
        assert torch.equal(v, sd[k].float()), k
    assert torch.equal(train_unet.pack_params(back, fts, ncls * 64), flat)
    w = engine.NetWeights.from_state_dict(sd, "fp32", "cpu")
    n = w.c.n_unet_ops
    assert n == len(plan)
    total, lay = train_unet.param_layout(fts, ncls * 64)
    w_off, b_off, n_pad, k_pad = (C.c_longlong * n)(), (C.c_longlong * n)(), (C.c_int * n)(), (C.c_int * n)()
    assert _lib.lib().cpx_unet_param_layout(w.c.unet_ops, n, w_off, b_off, n_pad, k_pad) == total == flat.numel()
    assert [tuple(t) for t in zip(w_off, b_off, n_pad, k_pad)] == lay
    for i, (wo, bo, npad, kpad) in enumerate(lay):
        op = w.c.unet_ops[i]
        wt = np.ctypeslib.as_array(C.cast(op.weight, C.POINTER(C.c_float)), (npad * kpad,))
        bs = np.ctypeslib.as_array(C.cast(op.bias, C.POINTER(C.c_float)), (npad,))
        assert np.array_equal(wt, flat[wo:wo + npad * kpad].numpy()), plan[i][0]
        assert np.array_equal(bs, flat[bo:bo + npad].numpy()), plan[i][0]


def test_cli_structure_is_checked():
    p = train_head.build_parser()
    base = ["--images", "x.npy", "--labels", "y.npy", "--pretrained_model", "m", "--save_path", "d", "--model_name", "n"]
    args = p.parse_args(base + ["--feature_transformation_structure", "16", "24", "--nclasses", "3"])
    assert args.feature_transformation_structure == [16, 24]
    train_head.check_args(args)
    with pytest.raises(SystemExit):
        train_head.check_args(p.parse_args(base + ["--feature_transformation_structure", "8", "8", "8", "8", "8"]))
    with pytest.raises(ValueError):
        train_unet.prepare_unet_state_dict(synth.make_state_dict(1, None, depth=1, seed=1), 3, 0, [8, 8, 8, 8, 8])


def test_prepare_state_dicts():
    unet = synth.make_state_dict(3, [16, 24], depth=1, seed=2)
    with pytest.raises(NotImplementedError):
        train.prepare_state_dict(unet)                         # the 1x1 trainer still refuses a UNet checkpoint
    sd, ncls, fts = train_unet.prepare_unet_state_dict(unet)
    assert (ncls, fts) == (3, [16, 24]) and all(torch.equal(sd[k], unet[k]) for k in unet)
    with pytest.raises(ValueError):
        train_unet.prepare_unet_state_dict(unet, feature_transformation_structure=[16, 32])
    with pytest.raises(ValueError):
        train_unet.prepare_unet_state_dict(unet, nclasses=4)
    plain = synth.make_state_dict(1, None, depth=1, seed=2)    # no semantic head at all
    with pytest.raises(ValueError):
        train_unet.prepare_unet_state_dict(plain)
    with pytest.raises(ValueError):
        train_unet.prepare_unet_state_dict(plain, feature_transformation_structure=[16, 24])
    sd, ncls, fts = train_unet.prepare_unet_state_dict(plain, 5, 7, [16, 24])
    assert ncls == 5 and engine.NetWeights.infer_structure(sd)[:2] == ([16, 24], 5)
    conv = synth.make_state_dict(4, None, depth=1, seed=2)     # a 1x1 head: replaced, its class count kept
    sd, ncls, fts = train_unet.prepare_unet_state_dict(conv, None, 7, [16, 24])
    assert ncls == 4 and "out_class.weight" not in sd and engine.NetWeights.infer_structure(sd)[:2] == ([16, 24], 4)


def test_entry_points_declared_exported_bound():
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert _lib.lib().cpx_unet_wgrad_slab_rows() == 512
    assert "cpx_unet_head_layout" in _lib._PRIVATE and "cpx_unet_head_layout" not in _lib.SIGNATURES
