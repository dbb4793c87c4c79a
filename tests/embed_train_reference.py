"""CPU statement of training the patch embedding and the position table (csrc/cpx_train_embed.hip) on top of
tests/block_train_reference.py.  The forward is

    x = ste(p W^T + b + pos[row % 1024])         p [rows, 192] patch rows, W [1024, 192], b [1024], pos [1024, 1024]

from leaf tensors, handed to block_train_reference.loss_and_grads unchanged (its ``x.to(dtype)`` is the identity for an equal dtype, so
autograd reaches the leaves); ``replay`` is block_train_reference.replay with the three tensors as one more group.

``loss_and_grads_bf16`` is the comparator of the bf16 gradient modes: the same network with the backward written out as the device
runs it -- the tail by autograd down to dy0, then block_train_bf16_reference.block_backward (attn_bwd_bf16_reference's with the bf16
attention backward) block by block, then ``embed_backward`` with dx rounded to bf16 in dW alone."""
from __future__ import annotations

import numpy as np
import torch

import attn_bwd_bf16_reference as ab
import block_train_bf16_reference as b16
import block_train_reference as br
import flow_train_reference as fr
import neck_train_reference as nr
import train_reference as tr
from neck_train_reference import ste

KEYS = ("encoder.patch_embed.proj.weight", "encoder.patch_embed.proj.bias", "encoder.pos_embed")
NAMES = ("pe_w", "pe_b", "pos")


def params_from_state_dict(sd: dict) -> dict:
    return {"pe_w": sd[KEYS[0]].float().reshape(1024, 192).clone(), "pe_b": sd[KEYS[1]].float().clone(),
            "pos": sd[KEYS[2]].float().reshape(1024, 1024).clone()}


def rounded(P: dict, dtype, net_dtype) -> dict:
    """The three tensors as the load rounds them: each through the network dtype."""
    return nr.rounded(P, dtype, net_dtype)


def embed(R: dict, p: torch.Tensor, net_dtype=None) -> torch.Tensor:
    """Block 0's input rows from the (already rounded) parameters ``R`` and patch rows ``p``."""
    n = p.shape[0] // 1024
    return ste(p @ R["pe_w"].T + R["pe_b"] + R["pos"].repeat(n, 1), net_dtype)


def embed_backward(p: torch.Tensor, dx: torch.Tensor, rnd=b16.identity) -> dict:
    """The three gradients by hand in dx's dtype; ``rnd`` rounds dx in dW alone (db and dpos take the unrounded dx)."""
    n = p.shape[0] // 1024
    return {"pe_w": rnd(dx).T @ p.to(dx.dtype), "pe_b": dx.sum(0), "pos": dx.view(n, 1024, 1024).sum(0)}


def loss_and_grads(PE: dict, PB: list, PN: dict, p: torch.Tensor, labels, targets, ncls: int, dtype=torch.float64, net_dtype=None,
                   fold: bool = True) -> dict:
    """block_train_reference.loss_and_grads from patch rows: its result plus "embed", the gradients of the three tensors."""
    RE = {k: v.clone().requires_grad_(True) for k, v in rounded(PE, dtype, net_dtype).items()}
    x = embed(RE, p.to(dtype), net_dtype)
    r = br.loss_and_grads(PB, PN, x, labels, targets, ncls, dtype, net_dtype, fold)
    r["embed"] = {k: RE[k].grad for k in NAMES}
    return r


def loss_and_grads_bf16(PE: dict, PB: list, PN: dict, p: torch.Tensor, labels, targets, ncls: int, dtype=torch.float32, net_dtype=torch.bfloat16,
                        fold: bool = True, attn_bf16: bool = False) -> dict:
    """The same result with the backward of the bf16 gradient modes (``attn_bf16``: the bf16 attention backward too)."""
    n = p.shape[0] // 1024
    with torch.no_grad():
        xs = [embed(rounded(PE, dtype, net_dtype), p.to(dtype), net_dtype)]
        for P in PB:
            xs.append(br.block_forward(br.rounded(P, dtype, net_dtype), xs[-1], n, net_dtype, fold)["out"])
    RN = {k: v.clone().requires_grad_(True) for k, v in nr.rounded(PN, dtype, net_dtype).items()}
    # the tail from y0 = x_out W0^T as a leaf (nr.tail with the identity in W0's place: y0 I is y0 exactly), so that dy0 can be rounded
    y0 = (xs[-1] @ RN["W0"].detach().T).requires_grad_(True)
    RI = dict(RN, W0=torch.eye(256, dtype=dtype))
    t = nr.tail(RI, y0, net_dtype)
    ce, tv, *_ = tr.class_loss(tr.tokens_to_nchw(t["cls"], 0, ncls, n, 256, 256), labels)
    loss = ce + tv
    if targets is not None:
        flow, cp = fr.seg_loss(tr.tokens_to_nchw(t["flow"], 0, 3, n, 256, 256), targets.to(dtype))
        loss = flow + cp + loss
    loss.backward()
    with torch.no_grad():
        dy0 = y0.grad
        neck = {k: (RN[k].grad if RN[k].grad is not None else torch.zeros_like(RN[k])) for k in RN}
        neck["W0"] = dy0.T @ xs[-1]                                    # the neck's own gradients stay float32 in every mode
        dx = b16.top_backward(dy0, RN["W0"].detach(), b16.round_bf16)
        blocks = [None] * len(PB)
        backward = ab.block_backward if attn_bf16 else b16.block_backward
        for j in reversed(range(len(PB))):
            r = backward(PB[j], xs[j], dx, n, dtype, net_dtype, fold, rnd=b16.round_bf16)
            blocks[j], dx = r["grads"], r["dx"]
        return {"loss": loss.detach(), "blocks": blocks, "neck": neck, "embed": embed_backward(p.to(dtype), dx, b16.round_bf16), "dx_in": dx}


def replay(PE0: dict, PB0: list, PN0: dict, p, labels, targets, ncls: int, lrs, dtype, net_dtype, weight_decay: float, fold: bool = True):
    """CPU replay of ``HeadTrainer.step`` with ``train_embed``: AdamW on every tensor with one step counter, the masters re-rounded
    every step.  Returns (losses (steps,), final embedding masters, final block masters, final neck and head masters)."""
    PE = {k: v.to(dtype).clone() for k, v in PE0.items()}
    PB = [{k: v.to(dtype).clone() for k, v in P.items()} for P in PB0]
    PN = {k: v.to(dtype).clone() for k, v in PN0.items()}
    groups = [PE] + PB + [PN]
    M = [{k: torch.zeros_like(v) for k, v in P.items()} for P in groups]
    V = [{k: torch.zeros_like(v) for k, v in P.items()} for P in groups]
    losses = []
    for step, lr in enumerate(lrs, 1):
        r = loss_and_grads(PE, PB, PN, p, labels, targets, ncls, dtype, net_dtype, fold)
        losses.append(float(r["loss"]))
        for P, G, m, v in zip(groups, [r["embed"]] + r["blocks"] + [r["neck"]], M, V):
            for k in P:
                if targets is None and k in ("Wf", "bf"):
                    continue
                tr.adamw_step(P[k], G[k].to(dtype), m[k], v[k], step, lr, weight_decay=weight_decay)
    return np.array(losses), PE, PB, PN
