"""Torch restatement (CPU, float64 or float32) of training transformer blocks: one block's forward (vit_sam.py:148-197 with
flash_forward :15-65) -- LayerNorm, qkv, attention with the decomposed rel-pos bias, proj, residual, LayerNorm, lin1, erf GELU, lin2,
residual -- on token-major rows, differentiated by autograd, and the hand-written backward formulas the kernels of
csrc/cpx_train_blocks.hip cite (``attention_backward``, ``gelu_grad``; LayerNorm: ``neck_train_reference.ln_backward``).  The
yardstick of tests/test_block_train_host.py (which pins the forward on oracle.net and the formulas on float64 autograd) and
tests/test_gpu_block_train.py.

For bf16 / fp16 it is the straight-through replay neck_train_reference uses: every tensor the device stores in the network dtype
(qkv, the attention output, the rows after either residual, the hidden activations) is rounded in the forward and the gradient passes
through the rounding; ``fold=True`` forms qkv and lin1 as the device does with LayerNorm folded into them (cpx_fold_layernorm: the
operand is round(W diag(gamma)), the bias b + W beta), which has the same derivative with respect to W, b, gamma and beta;
``fold=False`` is the network built with fuse_ln=False, which stores the LayerNorm output in the network dtype: rounded here as well.

A block's parameters travel as a dict in the order of cpx_block_grad_layout:
    ln1_g, ln1_b [1024] | qkv_w [3072, 1024], qkv_b | rel_h, rel_w (the checkpoint's shape, e.g. [27, 64]) | proj_w [1024, 1024], proj_b |
    ln2_g, ln2_b | fc1_w [4096, 1024], fc1_b | fc2_w [1024, 4096], fc2_b
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import flow_train_reference as fr
import neck_train_reference as nr
import train_reference as tr
from neck_train_reference import EPS, layernorm, ste

NAMES = ("ln1_g", "ln1_b", "qkv_w", "qkv_b", "rel_h", "rel_w", "proj_w", "proj_b", "ln2_g", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.rel_pos_h", "attn.rel_pos_w", "attn.proj.weight",
        "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.lin1.weight", "mlp.lin1.bias", "mlp.lin2.weight", "mlp.lin2.bias")
OPERANDS = ("qkv_w", "proj_w", "fc1_w", "fc2_w")
SCALE = 0.125                            # 64^-1/2
HEADS, HD, GRID = 16, 64, 32


def params_from_state_dict(sd: dict, i: int) -> dict:
    return {n: sd[f"encoder.blocks.{i}.{k}"].float().clone() for n, k in zip(NAMES, KEYS)}


def interp_matrix(n: int, size: int = 63) -> torch.Tensor:
    """A [size, n] float64 with get_rel_pos's resize (F.interpolate, linear) = A @ rel_pos; the identity when n == size."""
    if n == size:
        return torch.eye(n, dtype=torch.float64)
    eye = torch.eye(n, dtype=torch.float64)
    return F.interpolate(eye.reshape(1, n, n).permute(0, 2, 1), size=size, mode="linear").reshape(n, size).permute(1, 0).contiguous()


def rel_operand(rel: torch.Tensor, net_dtype) -> torch.Tensor:
    """The table as the kernels read it (engine.NetWeights): interpolated to 63 rows in the network dtype, times 1 / scale = 8, a zero
    row appended -> [64, 64] in rel's dtype; the gradient passes straight through the roundings to ``rel``."""
    A = interp_matrix(rel.shape[0]).to(rel.dtype)
    lin = A @ rel
    if net_dtype not in (None, torch.float32):
        r = rel.detach().float().to(net_dtype)
        val = r if r.shape[0] == 63 else F.interpolate(r.reshape(1, r.shape[0], -1).permute(0, 2, 1), size=63, mode="linear").reshape(-1, 63).permute(1, 0)
        lin = lin + (val.to(rel.dtype) - lin.detach())
    return torch.cat([lin * 8.0, torch.zeros(1, 64, dtype=rel.dtype)], 0)


def _rel_index() -> torch.Tensor:
    a = torch.arange(GRID)
    return a[:, None] - a[None, :] + GRID - 1          # [q][k] -> table row


def _split(qkv: torch.Tensor, nS: int):
    t = qkv.reshape(nS, 1024, 3, HEADS, HD).permute(2, 0, 3, 1, 4)
    return t[0], t[1], t[2]                              # [nS, 16, 1024, 64] each


def _logits(q, k, Rh, Rw, nS):
    """S' = q . (k + Rh[qy - ky + 31] + Rw[qx - kx + 31]) [nS, 16, 1024, 1024]"""
    idx = _rel_index()
    qg = q.reshape(nS, HEADS, GRID, GRID, HD)
    bh = torch.einsum("bnhwc,hkc->bnhwk", qg, Rh[idx])   # [.., qy, qx, ky]
    bw = torch.einsum("bnhwc,wkc->bnhwk", qg, Rw[idx])   # [.., qy, qx, kx]
    bias = (bh[..., :, None] + bw[..., None, :]).reshape(nS, HEADS, 1024, 1024)
    return q @ k.transpose(-1, -2) + bias


def attention(qkv: torch.Tensor, Rh: torch.Tensor, Rw: torch.Tensor, nS: int) -> torch.Tensor:
    """What cpx_attention computes: qkv [nS * 1024, 3072], operand tables [64, 64] -> [nS * 1024, 1024]."""
    q, k, v = _split(qkv, nS)
    P = torch.softmax(_logits(q, k, Rh, Rw, nS) * SCALE, -1)
    return (P @ v).permute(0, 2, 1, 3).reshape(nS * 1024, HEADS * HD)


def attention_backward(qkv: torch.Tensor, Rh: torch.Tensor, Rw: torch.Tensor, dO: torch.Tensor, nS: int) -> dict:
    """The derivative of ``attention`` by hand, as the header of csrc/cpx_train_blocks.hip states it: dqkv, dRh, dRw (operand tables)."""
    q, k, v = _split(qkv, nS)
    P = torch.softmax(_logits(q, k, Rh, Rw, nS) * SCALE, -1)
    O = P @ v
    dOh = dO.reshape(nS, 1024, HEADS, HD).permute(0, 2, 1, 3)
    delta = (dOh * O).sum(-1, keepdim=True)
    dS = SCALE * P * (dOh @ v.transpose(-1, -2) - delta)                 # d loss / d S'
    dv = P.transpose(-1, -2) @ dOh
    dk = dS.transpose(-1, -2) @ q
    d5 = dS.reshape(nS, HEADS, GRID, GRID, GRID, GRID)                   # [.., qy, qx, ky, kx]
    Gh, Gw = d5.sum(-1), d5.sum(-2)                                      # [.., qy, qx, ky], [.., qy, qx, kx]
    idx = _rel_index()
    dq = dS @ k + (torch.einsum("bnhwk,hkc->bnhwc", Gh, Rh[idx]) + torch.einsum("bnhwk,wkc->bnhwc", Gw, Rw[idx])).reshape(nS, HEADS, 1024, HD)
    qg = q.reshape(nS, HEADS, GRID, GRID, HD)
    dRh, dRw = torch.zeros_like(Rh), torch.zeros_like(Rw)
    dRh.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->hkc", Gh, qg).reshape(-1, HD))
    dRw.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->wkc", Gw, qg).reshape(-1, HD))
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(nS * 1024, 3 * HEADS * HD)
    return {"dqkv": dqkv, "dRh": dRh, "dRw": dRw}


def gelu_grad(x: torch.Tensor) -> torch.Tensor:
    """d gelu / dx of the erf GELU: Phi(x) + x phi(x)"""
    return 0.5 * torch.erfc(-x / math.sqrt(2.0)) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def rounded(P: dict, dtype, net_dtype) -> dict:
    """The parameters as the load rounds them: every tensor through the network dtype (the rel tables are rounded by rel_operand)."""
    half = net_dtype not in (None, torch.float32)
    return {k: (v.float().to(net_dtype).to(dtype) if half and not k.startswith("rel_") else v.to(dtype)) for k, v in P.items()}


def _xhat(x):
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + EPS)


def _ln_linear(x, g, b, W, bias, net_dtype, fold):
    if fold and net_dtype not in (None, torch.float32):
        return _xhat(x) @ ste(W * g[None, :], net_dtype).T + (bias + W @ b)
    # unfolded: the half-precision network stores the LayerNorm output in the network dtype before the GEMM reads it (cpx_layernorm),
    # and the backward's recompute rounds it the same way (k_ln_fwd1024<DT, true>); ste is the identity for None / float32
    return ste(layernorm(x, g, b), net_dtype) @ W.T + bias


def _held(computed: torch.Tensor, stored, key: str) -> torch.Tensor:
    """``computed`` with the value the device stored for it (when given) and the gradient of ``computed``: the straight-through replay
    on the device's own stored tensors"""
    if stored is None or key not in stored:
        return computed
    return computed + (stored[key].to(computed.dtype) - computed).detach()


def block_forward(R: dict, x: torch.Tensor, nS: int, net_dtype=None, fold: bool = True, stored: dict | None = None) -> dict:
    """One block from the (already rounded) parameters ``R`` on rows ``x``: the stored tensors and the output rows.  ``stored``: the
    device's own qkv / ao / x_mid, taken as the values of those tensors (the half-precision attention kernel rounds P to the network
    dtype, so its stored output is not the rounded float32 attention; the backward differentiates at what was stored)."""
    Rh, Rw = rel_operand(R["rel_h"], net_dtype), rel_operand(R["rel_w"], net_dtype)
    qkv = _held(ste(_ln_linear(x, R["ln1_g"], R["ln1_b"], R["qkv_w"], R["qkv_b"], net_dtype, fold), net_dtype), stored, "qkv")
    ao = _held(ste(attention(qkv, Rh, Rw, nS), net_dtype), stored, "ao")
    x_mid = _held(ste(x + ao @ R["proj_w"].T + R["proj_b"], net_dtype), stored, "x_mid")
    pre = _ln_linear(x_mid, R["ln2_g"], R["ln2_b"], R["fc1_w"], R["fc1_b"], net_dtype, fold)
    h = ste(F.gelu(pre), net_dtype)
    out = ste(x_mid + h @ R["fc2_w"].T + R["fc2_b"], net_dtype)
    return {"x": x, "qkv": qkv, "ao": ao, "x_mid": x_mid, "pre": pre, "h": h, "out": out}


def block_grads(P: dict, x: torch.Tensor, dout: torch.Tensor, nS: int, dtype=torch.float64, net_dtype=None, fold: bool = True,
                stored: dict | None = None) -> dict:
    """d <dout, block(x)> / d every parameter and d / dx, by autograd in ``dtype``: {"grads": {name: tensor}, "dx": tensor}"""
    R = {k: v.clone().requires_grad_(True) for k, v in rounded(P, dtype, net_dtype).items()}
    xx = x.to(dtype).clone().requires_grad_(True)
    o = block_forward(R, xx, nS, net_dtype, fold, stored)
    (o["out"] * dout.to(dtype)).sum().backward()
    return {"grads": {k: R[k].grad for k in R}, "dx": xx.grad, "fwd": {k: v.detach() for k, v in o.items()}}


def loss_and_grads(PB: list, PN: dict, x: torch.Tensor, labels: torch.Tensor, targets, ncls: int, dtype=torch.float64, net_dtype=None,
                   fold: bool = True) -> dict:
    """The blocks ``PB`` (a list of parameter dicts, first trained block first), the neck and both heads ``PN``
    (neck_train_reference's dict) on rows ``x``: the losses and d loss / d every parameter."""
    RB = [{k: v.clone().requires_grad_(True) for k, v in rounded(P, dtype, net_dtype).items()} for P in PB]
    RN = {k: v.clone().requires_grad_(True) for k, v in nr.rounded(PN, dtype, net_dtype).items()}
    n = x.shape[0] // 1024
    h = x.to(dtype)
    for R in RB:
        h = block_forward(R, h, n, net_dtype, fold)["out"]
    t = nr.tail(RN, h, net_dtype)
    ce, tv, *_ = tr.class_loss(tr.tokens_to_nchw(t["cls"], 0, ncls, n, 256, 256), labels)
    loss, seg = ce + tv, None
    if targets is not None:
        flow, cp = fr.seg_loss(tr.tokens_to_nchw(t["flow"], 0, 3, n, 256, 256), targets.to(dtype))
        seg = flow + cp
        loss = seg + loss
    loss.backward()
    g = lambda R: {k: (R[k].grad if R[k].grad is not None else torch.zeros_like(R[k])) for k in R}
    return {"loss": loss.detach(), "seg": None if seg is None else seg.detach(), "ce": ce.detach(), "tversky": tv.detach(),
            "blocks": [g(R) for R in RB], "neck": g(RN)}


def replay(PB0: list, PN0: dict, x, labels, targets, ncls: int, lrs, dtype, net_dtype, weight_decay: float, fold: bool = True):
    """CPU replay of ``HeadTrainer.step`` with ``train_blocks``: AdamW on every tensor with one step counter, the masters re-rounded
    every step.  Returns (losses (steps,), final block masters, final neck and head masters)."""
    import numpy as np
    PB = [{k: v.to(dtype).clone() for k, v in P.items()} for P in PB0]
    PN = {k: v.to(dtype).clone() for k, v in PN0.items()}
    groups = PB + [PN]
    M = [{k: torch.zeros_like(v) for k, v in P.items()} for P in groups]
    V = [{k: torch.zeros_like(v) for k, v in P.items()} for P in groups]
    losses = []
    for step, lr in enumerate(lrs, 1):
        r = loss_and_grads(PB, PN, x, labels, targets, ncls, dtype, net_dtype, fold)
        losses.append(float(r["loss"]))
        for P, G, m, v in zip(groups, r["blocks"] + [r["neck"]], M, V):
            for k in P:
                if targets is None and k in ("Wf", "bf"):
                    continue
                tr.adamw_step(P[k], G[k].to(dtype), m[k], v[k], step, lr, weight_decay=weight_decay)
    return np.array(losses), PB, PN
