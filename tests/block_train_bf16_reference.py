"""CPU restatement of the block backward with bf16 gradient GEMMs (cpx_blocks_backward_ex with CPX_DT_BF16): the backward of
one transformer block written out by hand on top of tests/block_train_reference.py, with ``round_bf16`` at exactly the operand positions
of the mode's contract and nowhere else, passed straight through.  Per Linear y = a W^T + b with gradient dy:

    forward   y  = round(a) W^T + b          (the recomputed lin1 pre-activation; qkv, proj and lin2 outputs come from what was stored)
    backward  dW = round(dy)^T round(a)      da = round(dy) W      db = column sums of the UNROUNDED dy

W is the operand the forward multiplied by (the folded one, round_net(W diag(gamma)), where LayerNorm is folded) and is exact in bf16.
Nothing else is rounded: LayerNorm, GELU and attention backward and the residual adds are plain arithmetic in ``dtype``.  ``rnd`` selects
the rounding (``round_bf16``) or switches it off (``identity``), ``dtype`` the arithmetic; with the rounding off the result is
block_train_reference.block_grads (tests/test_block_train_bf16_host.py pins that, and pins the rounded form on autograd through
straight-through roundings at the same tensors)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import block_train_reference as br
from neck_train_reference import EPS, layernorm, ste


def round_bf16(t: torch.Tensor) -> torch.Tensor:
    """round to nearest even to bf16, kept in t's dtype"""
    return t.float().to(torch.bfloat16).to(t.dtype)


def identity(t: torch.Tensor) -> torch.Tensor:
    return t


def linear_forward(a, W, b, rnd):
    return rnd(a) @ W.T + b


def linear_backward(dy, a, W, rnd):
    """(dW, db, da) of y = a W^T + b"""
    r = rnd(dy)
    return r.T @ rnd(a), dy.sum(0), r @ W


def ln_backward(x, gamma, dout):
    """(dx, dgamma, dbeta) of neck_train_reference.layernorm in x's dtype"""
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + EPS)
    xh = (x - mean) * rstd
    g = dout * gamma
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, (dout * xh).sum(0), dout.sum(0)


def top_backward(dy0, W0, rnd):
    """the gradient of the last block's output rows: round(dy0) W0"""
    return rnd(dy0) @ W0


def block_backward(P: dict, x: torch.Tensor, dout: torch.Tensor, nS: int, dtype=torch.float64, net_dtype=None, fold: bool = True,
                   stored: dict | None = None, rnd=round_bf16) -> dict:
    """d <dout, block(x)> / d every parameter and d / dx by hand: {"grads": {name: tensor}, "dx": tensor}; the arguments of
    block_train_reference.block_grads plus ``rnd``."""
    half = net_dtype not in (None, torch.float32)
    with torch.no_grad():
        R = br.rounded(P, dtype, net_dtype)
        x, dout = x.to(dtype), dout.to(dtype)
        Rh, Rw = br.rel_operand(R["rel_h"], net_dtype), br.rel_operand(R["rel_w"], net_dtype)
        st = lambda t: ste(t, net_dtype)
        held = lambda t, key: stored[key].to(dtype) if stored is not None and key in stored else t
        ones = torch.ones(1024, dtype=dtype)

        def ln_operands(rows, g, beta, W, bias):
            """(a, operand, bias) of the Linear behind a LayerNorm, as the device forms them"""
            if fold and half:
                return br._xhat(rows), st(W * g[None, :]), bias + W @ beta
            return st(layernorm(rows, g, beta)), W, bias

        def ln_linear_backward(rows, g, beta, W, dWf, dbf, da):
            """the gradient of the rows, of gamma and beta, and of the unfolded W and b"""
            if fold and half:
                dxl = ln_backward(rows, ones, da)[0]
                return dxl, (dWf * W).sum(0), dbf @ W, dWf * g[None, :] + dbf[:, None] * beta[None, :], dbf
            dxl, dg, db = ln_backward(rows, g, da)
            return dxl, dg, db, dWf, dbf

        # the forward, as the device recomputes it
        a1, Wq, bq = ln_operands(x, R["ln1_g"], R["ln1_b"], R["qkv_w"], R["qkv_b"])
        qkv = held(st(linear_forward(a1, Wq, bq, rnd)), "qkv")
        ao = held(st(br.attention(qkv, Rh, Rw, nS)), "ao")
        x_mid = held(st(x + linear_forward(ao, R["proj_w"], R["proj_b"], rnd)), "x_mid")
        a2, W1, b1 = ln_operands(x_mid, R["ln2_g"], R["ln2_b"], R["fc1_w"], R["fc1_b"])
        pre = linear_forward(a2, W1, b1, rnd)
        h = st(F.gelu(pre))
        # the backward
        G = {}
        G["fc2_w"], G["fc2_b"], dh = linear_backward(dout, h, R["fc2_w"], rnd)
        dWf, dbf, da2 = linear_backward(dh * br.gelu_grad(pre), a2, W1, rnd)
        dxl, G["ln2_g"], G["ln2_b"], G["fc1_w"], G["fc1_b"] = ln_linear_backward(x_mid, R["ln2_g"], R["ln2_b"], R["fc1_w"], dWf, dbf, da2)
        dxm = dout + dxl
        G["proj_w"], G["proj_b"], dO = linear_backward(dxm, ao, R["proj_w"], rnd)
        ab = br.attention_backward(qkv, Rh, Rw, dO, nS)
        for name, key in (("rel_h", "dRh"), ("rel_w", "dRw")):
            G[name] = 8.0 * br.interp_matrix(R[name].shape[0]).to(dtype).T @ ab[key][:63]
        dWf, dbf, da1 = linear_backward(ab["dqkv"], a1, Wq, rnd)
        dxl, G["ln1_g"], G["ln1_b"], G["qkv_w"], G["qkv_b"] = ln_linear_backward(x, R["ln1_g"], R["ln1_b"], R["qkv_w"], dWf, dbf, da1)
        return {"grads": {k: G[k] for k in br.NAMES}, "dx": dxm + dxl}
