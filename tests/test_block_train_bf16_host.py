"""The CPU restatement of the bf16-gradient block backward (tests/block_train_bf16_reference.py) against autograd, the declarations of
the new entry points, and the train_head refusals of --grad_precision, none of which needs a device.

With the rounding switched off the hand-written backward is block_train_reference.block_grads in float64; with it on it is what
float64 autograd finds when every Linear reads its input through a straight-through ``round_bf16`` and hands its output gradient to
the two products through a ``round_bf16`` of the gradient -- the positions DESIGN 6r states, and no other."""
from __future__ import annotations

import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

import block_train_bf16_reference as b16
import block_train_reference as br
from neck_train_reference import layernorm, ste
from classpose_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SD = {}


def _case(seed):
    if "sd" not in _SD:
        _SD["sd"] = synth.make_state_dict(3, None, depth=1, seed=51)
    P = br.params_from_state_dict(_SD["sd"], 0)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(1024, 1024, generator=g) * torch.logspace(-0.5, 0.5, 1024)[:, None]
    dout = torch.randn(1024, 1024, generator=g) * torch.logspace(-2, 0, 1024)[None]
    return P, x, dout


def _rel(a, b):
    return float((a - b).norm() / b.norm())


class _RoundGrad(torch.autograd.Function):
    """the identity whose gradient is rounded to bf16: behind a matrix product, both of the product's gradients take round(dy)"""

    @staticmethod
    def forward(ctx, y):
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        return b16.round_bf16(g)


def _linear(a, W, b):
    ar = a + (b16.round_bf16(a) - a).detach()                          # straight-through rounding of the input operand
    return _RoundGrad.apply(ar @ W.T) + b                              # the bias gradient sees the unrounded dy


def _autograd(P, x, dout, net_dtype, fold):
    """block_train_reference.block_forward with every Linear replaced by ``_linear``, differentiated by float64 autograd"""
    dt = torch.float64
    R = {k: v.clone().requires_grad_(True) for k, v in br.rounded(P, dt, net_dtype).items()}
    xx = x.to(dt).clone().requires_grad_(True)
    half = net_dtype not in (None, torch.float32)

    def ln_linear(rows, g, beta, W, bias):
        if fold and half:
            return _linear(br._xhat(rows), ste(W * g[None, :], net_dtype), bias + W @ beta)
        return _linear(ste(layernorm(rows, g, beta), net_dtype), W, bias)
    Rh, Rw = br.rel_operand(R["rel_h"], net_dtype), br.rel_operand(R["rel_w"], net_dtype)
    qkv = ste(ln_linear(xx, R["ln1_g"], R["ln1_b"], R["qkv_w"], R["qkv_b"]), net_dtype)
    ao = ste(br.attention(qkv, Rh, Rw, 1), net_dtype)
    x_mid = ste(xx + _linear(ao, R["proj_w"], R["proj_b"]), net_dtype)
    h = ste(F.gelu(ln_linear(x_mid, R["ln2_g"], R["ln2_b"], R["fc1_w"], R["fc1_b"])), net_dtype)
    out = ste(x_mid + _linear(h, R["fc2_w"], R["fc2_b"]), net_dtype)
    (out * dout.to(dt)).sum().backward()
    return {"grads": {k: R[k].grad for k in R}, "dx": xx.grad}


@pytest.mark.parametrize("net,fold", [(None, True), (torch.bfloat16, True), (torch.bfloat16, False)])
def test_without_rounding_the_restatement_is_block_grads(net, fold):
    P, x, dout = _case(11)
    want = br.block_grads(P, x, dout, 1, torch.float64, net, fold)
    got = b16.block_backward(P, x, dout, 1, torch.float64, net, fold, rnd=b16.identity)
    errs = {k: _rel(got["grads"][k], want["grads"][k]) for k in br.NAMES}
    errs["dx"] = _rel(got["dx"], want["dx"])
    print(f"net {net} fold {fold}: worst relative error {max(errs.values()):.3e} ({max(errs, key=errs.get)})")
    assert max(errs.values()) < 1e-10


@pytest.mark.parametrize("fold", [True, False])
def test_with_rounding_it_is_autograd_through_straight_through_roundings(fold):
    """and the roundings are there: the rounded gradients differ from the unrounded ones by about a bf16 ulp, 2^-9 relative"""
    P, x, dout = _case(12)
    net = torch.bfloat16
    want = _autograd(P, x, dout, net, fold)
    got = b16.block_backward(P, x, dout, 1, torch.float64, net, fold, rnd=b16.round_bf16)
    plain = br.block_grads(P, x, dout, 1, torch.float64, net, fold)
    errs = {k: _rel(got["grads"][k], want["grads"][k]) for k in br.NAMES}
    errs["dx"] = _rel(got["dx"], want["dx"])
    away = {k: _rel(got["grads"][k], plain["grads"][k]) for k in br.OPERANDS}
    print(f"fold {fold}: against autograd with the roundings, worst {max(errs.values()):.3e} ({max(errs, key=errs.get)}); "
          f"against the unrounded gradients " + ", ".join(f"{k} {v:.3e}" for k, v in away.items()))
    assert max(errs.values()) < 1e-10
    assert all(2.0 ** -13 < v < 2.0 ** -5 for v in away.values())


def test_round_bf16_is_round_to_nearest_even():
    t = torch.tensor([1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -0.0, 3.3895313892515355e38])
    want = torch.tensor([1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -0.0, 3.3895313892515355e38])
    got = b16.round_bf16(t)
    assert torch.equal(got, want) and torch.signbit(got[4])
    assert torch.equal(b16.round_bf16(t.double()), want.double())
    assert b16.top_backward(torch.tensor([[1.0 + 2.0 ** -8]]), torch.tensor([[3.0]]), b16.round_bf16).item() == 3.0


def test_bf16_gradient_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    for name in ("cpx_gemm_tn_bf16", "cpx_blocks_backward_ex", "cpx_blocks_backward_workspace_bytes_ex", "cpx_colsum_add",
                 "cpx_colsum_workspace_bytes", "cpx_blocks_backward", "cpx_blocks_backward_workspace_bytes"):
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
    assert len(_lib.SIGNATURES["cpx_gemm_tn_bf16"][1]) == 9 and len(_lib.SIGNATURES["cpx_blocks_backward_ex"][1]) == 13
    assert len(_lib.SIGNATURES["cpx_blocks_backward"][1]) == 12, "the existing entry keeps its signature"
    L = _lib.lib()
    f32, b16_, f16 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16
    q = L.cpx_blocks_backward_workspace_bytes_ex
    for dt in (f32, b16_, f16):
        assert q(3, dt, f32) == L.cpx_blocks_backward_workspace_bytes(3, dt) > 0
    assert 0 < q(3, b16_, b16_) < q(3, b16_, f32), "the bf16 mode holds no transposed float32 operands"
    assert q(32, b16_, b16_) == q(3, b16_, b16_), "slabs: the workspace does not grow with the batch"
    assert q(3, f16, b16_) == 0 and q(3, f32, b16_) == 0 and q(3, b16_, f16) == 0 and q(0, b16_, b16_) == 0
    c = L.cpx_colsum_workspace_bytes
    assert c(1024, 1024) >= 16 * 1024 * 8 and c(1000, 1024) == 0 and c(1024, 1000) == 0 and c(0, 64) == 0


def _args(**kw):
    from classpose_amd.entrypoints import train_head
    a = train_head.build_parser().parse_args(["--images", "i.npy", "--labels", "l.npy", "--pretrained_model", "m.pt", "--save_path", "s",
                                              "--model_name", "n"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_cli_refuses_bf16_gradients_without_trained_bf16_blocks():
    """check_args runs before anything touches the device"""
    from classpose_amd.entrypoints import train_head
    assert _args().grad_precision == "fp32"
    with pytest.raises(SystemExit, match=r"--grad_precision bf16 goes with --train_blocks"):
        train_head.check_args(_args(grad_precision="bf16"))
    with pytest.raises(SystemExit, match=r"--precision bf16: fp16 gradients would need loss scaling"):
        train_head.check_args(_args(grad_precision="bf16", train_blocks=1, precision="fp16"))
    with pytest.raises(SystemExit, match=r"--precision bf16: a fp32 network has no half-precision operands"):
        train_head.check_args(_args(grad_precision="bf16", train_blocks=1, precision="fp32"))
    ok = _args(grad_precision="bf16", train_blocks=1, precision="bf16")
    train_head.check_args(ok)
    assert ok.grad_precision == "bf16" and ok.train_neck
    plain = _args(train_blocks=1)
    train_head.check_args(plain)
    assert plain.grad_precision == "fp32"
    with pytest.raises(SystemExit):
        train_head.build_parser().parse_args(["--grad_precision", "fp16"])


def test_trainer_argument_check_names_the_reason():
    from classpose_amd.train import check_grad_precision
    check_grad_precision("fp32", 0, "fp16")
    check_grad_precision("bf16", 2, "bf16")
    for args, what in ((("bf16", 0, "bf16"), "train_blocks > 0"), (("bf16", 1, "fp16"), "loss scaling"), (("bf16", 1, "fp32"), "no half-precision"),
                       (("fp16", 1, "bf16"), "'fp32' or 'bf16'")):
        with pytest.raises(ValueError, match=what):
            check_grad_precision(*args)
