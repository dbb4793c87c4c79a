"""Host side of training the neck: the ``--train_neck`` flag of the train_head command line, and the float64 restatement
tests/neck_train_reference.py pinned on torch's own autograd (``F.layer_norm``, ``F.conv2d``)."""
from __future__ import annotations

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import neck_train_reference as nr
from classpose_amd.entrypoints import train_head

BASE = ["--pretrained_model", "ck.pt", "--save_path", "out", "--model_name", "m"]
ARRAYS = ["--images", "X.npy", "--labels", "Y.npy"]


def _args(*extra):
    a = train_head.build_parser().parse_args(BASE + list(extra))
    train_head.check_args(a)
    return a


def test_train_neck_defaults_off_and_parses():
    assert _args(*ARRAYS).train_neck is False
    a = _args(*ARRAYS, "--train_neck")
    assert a.train_neck is True and a.train_flow_head is False


def test_train_neck_combines_with_the_flow_head():
    a = _args(*ARRAYS, "--instances", "I.npy", "--train_neck", "--train_flow_head")
    assert a.train_neck is True and a.train_flow_head is True
    a = _args("--data_path", "d", "--train_neck", "--train_flow_head")
    assert a.train_neck is True and a.train_flow_head is True
    with pytest.raises(SystemExit, match="needs --instances or --data_path"):
        _args(*ARRAYS, "--train_neck", "--train_flow_head")


@pytest.mark.parametrize("freeze", [["backbone", "neck"], ["backbone", "segmentation_head", "neck"], ["neck"]])
def test_train_neck_contradicts_a_frozen_neck(freeze):
    with pytest.raises(SystemExit, match="contradicts"):
        _args(*ARRAYS, "--instances", "I.npy", "--train_neck", "--freeze", *freeze)


@pytest.mark.parametrize("freeze", [["backbone"], ["backbone", "segmentation_head"]])
def test_the_reference_spellings_point_to_train_neck(freeze):
    for extra in ([], ["--train_neck"]):
        with pytest.raises(SystemExit, match="training the neck is not built.*--train_neck"):
            _args(*ARRAYS, "--instances", "I.npy", "--freeze", *freeze, *extra)


def test_train_neck_refuses_a_unet_head():
    with pytest.raises(SystemExit, match="UNet"):
        _args(*ARRAYS, "--train_neck", "--feature_transformation_structure", "16", "24")


# ---- the restatement ------------------------------------------------------------------------------------------------
def test_ln_backward_is_autograd_of_layer_norm():
    g = torch.Generator().manual_seed(1)
    rows, C = 37, 256
    y = (torch.randn(rows, C, generator=g) * torch.logspace(-2, 1, rows)[:, None] + torch.randn(rows, 1, generator=g)).double()
    gamma, beta = torch.randn(C, generator=g).double(), torch.randn(C, generator=g).double()
    dout = torch.randn(rows, C, generator=g).double() * torch.logspace(-3, 0, C).double()[None]
    dout[::7] = 0
    yv, gv, bv = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    out = F.layer_norm(yv, (C,), gv, bv, nr.EPS)
    assert torch.allclose(out.detach(), nr.layernorm(y, gamma, beta), rtol=1e-12, atol=1e-12)
    out.backward(dout)
    r = nr.ln_backward(y, gamma, dout)
    for name, got, ref in (("dy", r["dy"], yv.grad), ("dgamma", r["dgamma"], gv.grad), ("dbeta", r["dbeta"], bv.grad)):
        err = float((got - ref).abs().max() / ref.abs().max())
        print(f"{name}: max error / max magnitude = {err:.3e}")
        assert err <= 1e-12
    assert not bool(r["dy"][::7].any()), "zero rows of dout give zero rows of dy"
    assert bool((r["S_dy"] >= r["dy"].abs() * (1 - 1e-12)).all()) and bool((r["S_dgamma"] >= r["dgamma"].abs() * (1 - 1e-12)).all())


def test_conv_layout_and_straight_through():
    g = torch.Generator().manual_seed(2)
    nS = 2
    a = torch.randn(nS * 1024, 256, generator=g).double()
    w = torch.randn(256, 256, 3, 3, generator=g).double() * 0.02
    W2 = w.permute(0, 2, 3, 1).reshape(256, 2304)
    ref = F.conv2d(a.reshape(nS, 32, 32, 256).permute(0, 3, 1, 2), w, padding=1).permute(0, 2, 3, 1).reshape(-1, 256)
    assert torch.equal(nr.conv3x3_tokens(a, W2, nS), ref)
    # the operand layout is im2col's: column tap * 256 + c of the unfolded input
    col = F.unfold(a.reshape(nS, 32, 32, 256).permute(0, 3, 1, 2), 3, padding=1)            # [nS, c * 9 + tap, 1024]
    col = col.reshape(nS, 256, 9, 1024).permute(0, 3, 2, 1).reshape(nS * 1024, 2304)
    assert torch.allclose(col @ W2.T, ref, rtol=1e-12, atol=1e-12)
    x = torch.randn(5, 7, generator=g).double().requires_grad_(True)
    y = nr.ste(x, torch.bfloat16)
    assert torch.equal(y.detach(), x.detach().float().to(torch.bfloat16).double())
    y.sum().backward()
    assert torch.equal(x.grad, torch.ones_like(x))
    assert nr.ste(x, None) is x and nr.ste(x, torch.float32) is x


def test_params_round_trip_the_state_dict_layout():
    from classpose_amd import synth
    sd = synth.make_state_dict(3, None, depth=1, seed=5)
    P = nr.params_from_state_dict(sd)
    assert {k: tuple(v.shape) for k, v in P.items()} == {
        "W0": (256, 1024), "gamma1": (256,), "beta1": (256,), "W2": (256, 2304), "gamma2": (256,), "beta2": (256,),
        "Wc": (192, 256), "bc": (192,), "Wf": (192, 256), "bf": (192,)}
    assert torch.equal(P["W2"].view(256, 3, 3, 256).permute(0, 3, 1, 2), sd["encoder.neck.2.weight"].float())
    x = torch.randn(1024, 1024, generator=torch.Generator().manual_seed(3)).double()
    lab = torch.from_numpy(np.random.default_rng(0).integers(0, 3, (1, 256, 256)))
    r = nr.loss_and_grads(P, x, lab, None, 3)
    assert all(bool(torch.isfinite(v).all()) for v in r["grads"].values()) and float(r["grads"]["W0"].abs().max()) > 0
    assert not bool(r["grads"]["Wf"].any()), "without targets the flow head gets no gradient"
