"""Float64 torch restatement (CPU) of training the neck: the tail of the network (vit_sam.py:216-249: 1x1 conv, LayerNorm2d, 3x3
conv, LayerNorm2d, then the two 1x1 heads on the token grid) with straight-through rounding for bf16 / fp16, and LayerNorm over
channels with its backward spelled out.  The yardstick of tests/test_neck_train_host.py (which pins ``ln_backward`` on float64
autograd of ``F.layer_norm``) and tests/test_gpu_neck_train.py.

Parameters travel as a dict in the device's operand layout:
    W0 [256, 1024], gamma1, beta1 [256], W2 [256, 2304] (k = tap * 256 + c, ``neck.2.weight.permute(0, 2, 3, 1)``), gamma2, beta2 [256],
    Wc [ncls * 64, 256], bc, Wf [192, 256], bf.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

import flow_train_reference as fr
import train_reference as tr

EPS = float(np.float32(1e-6))          # the device passes 1e-6 as a float
NECK = ("W0", "gamma1", "beta1", "W2", "gamma2", "beta2")
HEADS = ("Wc", "bc", "Wf", "bf")
OPERANDS = ("W0", "W2", "Wc", "Wf")    # stay in the network dtype; the vectors are rounded through it and kept float32


def ste(x: torch.Tensor, net_dtype) -> torch.Tensor:
    """Round to ``net_dtype`` in the forward, identity in the backward; None / float32: nothing."""
    if net_dtype is None or net_dtype == torch.float32:
        return x
    return x + (x.detach().float().to(net_dtype).to(x.dtype) - x.detach())


def params_from_state_dict(sd: dict) -> dict:
    return {"W0": sd["encoder.neck.0.weight"].float().reshape(256, 1024).clone(),
            "gamma1": sd["encoder.neck.1.weight"].float().clone(), "beta1": sd["encoder.neck.1.bias"].float().clone(),
            "W2": sd["encoder.neck.2.weight"].float().permute(0, 2, 3, 1).reshape(256, 2304).clone(),
            "gamma2": sd["encoder.neck.3.weight"].float().clone(), "beta2": sd["encoder.neck.3.bias"].float().clone(),
            "Wc": sd["out_class.weight"].float().reshape(-1, 256).clone(), "bc": sd["out_class.bias"].float().clone(),
            "Wf": sd["out.weight"].float().reshape(192, 256).clone(), "bf": sd["out.bias"].float().clone()}


def layernorm(y: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = EPS) -> torch.Tensor:
    """LayerNorm over the last dimension (LayerNorm2d on token-major rows): biased variance."""
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * gamma + beta


def ln_backward(y: torch.Tensor, gamma: torch.Tensor, dout: torch.Tensor, eps: float = EPS) -> dict:
    """The backward of ``layernorm`` in float64, as cpx_layernorm_backward states it, and per output element the sum S of the
    magnitudes of its terms: dy, dgamma, dbeta, S_dy, S_dgamma, S_dbeta."""
    y, gamma, dout = y.double(), gamma.double(), dout.double()
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xh = (y - mean) * rstd
    g = dout * gamma
    mg, mgx = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    dy = rstd * (g - mg - xh * mgx)
    s_dy = rstd * (g.abs() + g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    return {"dy": dy, "dgamma": (dout * xh).sum(0), "dbeta": dout.sum(0),
            "S_dy": s_dy, "S_dgamma": (dout * xh).abs().sum(0), "S_dbeta": dout.abs().sum(0)}


def conv3x3_tokens(a: torch.Tensor, W2: torch.Tensor, nS: int) -> torch.Tensor:
    """3x3 / padding 1 convolution of token-major rows [nS * 1024, 256] per 32 x 32 crop with the operand-layout weight."""
    x = a.reshape(nS, 32, 32, 256).permute(0, 3, 1, 2)
    w = W2.reshape(256, 3, 3, 256).permute(0, 3, 1, 2)
    return F.conv2d(x, w, padding=1).permute(0, 2, 3, 1).reshape(nS * 1024, 256)


def rounded(P: dict, dtype, net_dtype) -> dict:
    """The parameters as the forward reads them: every tensor rounded through the network dtype, as at load."""
    return {k: (v.float().to(net_dtype).to(dtype) if net_dtype not in (None, torch.float32) else v.to(dtype)) for k, v in P.items()}


def tail(R: dict, x: torch.Tensor, net_dtype=None) -> dict:
    """y0, a1, y2, feat and the two heads' token-major logits, from the (already rounded) parameters ``R`` and backbone rows ``x``."""
    nS = x.shape[0] // 1024
    y0 = ste(x @ R["W0"].T, net_dtype)
    a1 = ste(layernorm(y0, R["gamma1"], R["beta1"]), net_dtype)
    y2 = ste(conv3x3_tokens(a1, R["W2"], nS), net_dtype)
    feat = ste(layernorm(y2, R["gamma2"], R["beta2"]), net_dtype)
    return {"y0": y0, "a1": a1, "y2": y2, "feat": feat, "flow": feat @ R["Wf"].T + R["bf"], "cls": feat @ R["Wc"].T + R["bc"]}


def loss_and_grads(P: dict, x: torch.Tensor, labels: torch.Tensor, targets, ncls: int, dtype=torch.float64, net_dtype=None) -> dict:
    """seg (when ``targets`` is given) + ce + tversky of one batch in ``dtype`` and d loss / d every parameter (straight-through
    the rounding of parameters and activations): {"loss", "seg", "ce", "tversky", "grads": {name: tensor}}."""
    R = {k: v.clone().requires_grad_(True) for k, v in rounded(P, dtype, net_dtype).items()}
    t = tail(R, x.to(dtype), net_dtype)
    n = x.shape[0] // 1024
    ce, tv, *_ = tr.class_loss(tr.tokens_to_nchw(t["cls"], 0, ncls, n, 256, 256), labels)
    loss, seg = ce + tv, None
    if targets is not None:
        flow, cp = fr.seg_loss(tr.tokens_to_nchw(t["flow"], 0, 3, n, 256, 256), targets.to(dtype))
        seg = flow + cp
        loss = seg + loss
    loss.backward()
    zero = lambda k: torch.zeros_like(R[k])
    return {"loss": loss.detach(), "seg": None if seg is None else seg.detach(), "ce": ce.detach(), "tversky": tv.detach(),
            "grads": {k: (R[k].grad if R[k].grad is not None else zero(k)) for k in R}}


def replay(P0: dict, x, labels, targets, ncls: int, lrs, dtype, net_dtype, weight_decay: float):
    """CPU replay of ``HeadTrainer.step`` with ``train_neck``: AdamW on every tensor with one step counter, the masters re-rounded
    every step.  Returns (losses (steps,), final masters)."""
    P = {k: v.to(dtype).clone() for k, v in P0.items()}
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    losses = []
    for step, lr in enumerate(lrs, 1):
        r = loss_and_grads(P, x, labels, targets, ncls, dtype, net_dtype)
        losses.append(float(r["loss"]))
        for k in P:
            if targets is None and k in ("Wf", "bf"):
                continue
            tr.adamw_step(P[k], r["grads"][k].to(dtype), M[k], V[k], step, lr, weight_decay=weight_decay)
    return np.array(losses), P
