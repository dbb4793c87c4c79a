"""CPU statement of layer drop (stochastic depth) for the trained blocks, on tests/block_train_reference.py.

``keep[j][n]`` is 1 where trained block j runs on crop n:
    x_{j+1}[n] = block_j(x_j[n]) if keep[j][n] else x_j[n]
``blocks_forward`` computes exactly that: ``br.block_forward`` on the kept crops alone, the other crops left as they are.
``reference_expression`` is the reference's own line (vit_sam.py:165-173) with mask = 1 - keep,
    x = x * mask + blk(x) * (1 - mask)
with ``blk`` on ALL crops; tests/test_layer_drop_host.py holds the two equal in float64, values and gradients.  ``loss_and_grads`` and
``replay`` are ``br.loss_and_grads`` / ``br.replay`` (with ``PE``: ``embed_train_reference``'s, from patch rows) under a mask per step."""
from __future__ import annotations

import numpy as np
import torch

import block_train_reference as br
import embed_train_reference as er
import flow_train_reference as fr
import neck_train_reference as nr
import train_reference as tr


def kept(keep, j: int) -> list[int]:
    return [n for n, k in enumerate(keep[j]) if k]


def blocks_forward(RB: list, x: torch.Tensor, keep, net_dtype=None, fold: bool = True) -> torch.Tensor:
    """The blocks ``RB`` (rounded parameters, first trained block first) on rows ``x`` (n * 1024, 1024) under ``keep`` (K, n): every
    block on its kept crops only."""
    n = x.shape[0] // 1024
    h = x.view(n, 1024, 1024)
    for j, R in enumerate(RB):
        idx = kept(keep, j)
        if not idx:
            continue
        ii = torch.tensor(idx)
        out = br.block_forward(R, h[ii].reshape(-1, 1024), len(idx), net_dtype, fold)["out"]
        h = h.index_copy(0, ii, out.view(len(idx), 1024, 1024))
    return h.reshape(-1, 1024)


def reference_expression(RB: list, x: torch.Tensor, keep, net_dtype=None, fold: bool = True) -> torch.Tensor:
    """vit_sam.py:165-173 with mask = 1 - keep: every block on every crop, then the blend."""
    n = x.shape[0] // 1024
    h = x
    for j, R in enumerate(RB):
        mask = (1 - torch.as_tensor(np.asarray(keep[j], dtype=np.float64))).to(x.dtype)[:, None, None]
        blk = br.block_forward(R, h, n, net_dtype, fold)["out"]
        h = (h.view(n, 1024, 1024) * mask + blk.view(n, 1024, 1024) * (1 - mask)).reshape(-1, 1024)
    return h


def loss_and_grads(PB: list, PN: dict, x: torch.Tensor, labels: torch.Tensor, targets, ncls: int, keep, dtype=torch.float64, net_dtype=None,
                   fold: bool = True, PE: dict | None = None) -> dict:
    """``br.loss_and_grads`` under the mask ``keep`` (K, n).  With ``PE`` (embed_train_reference's dict) ``x`` are patch rows and the
    result has "embed" too.  A block that keeps nothing has zero gradients."""
    RB = [{k: v.clone().requires_grad_(True) for k, v in br.rounded(P, dtype, net_dtype).items()} for P in PB]
    RN = {k: v.clone().requires_grad_(True) for k, v in nr.rounded(PN, dtype, net_dtype).items()}
    RE = None if PE is None else {k: v.clone().requires_grad_(True) for k, v in er.rounded(PE, dtype, net_dtype).items()}
    n = x.shape[0] // 1024
    h = x.to(dtype) if RE is None else er.embed(RE, x.to(dtype), net_dtype)
    h = blocks_forward(RB, h, keep, net_dtype, fold)
    t = nr.tail(RN, h, net_dtype)
    ce, tv, *_ = tr.class_loss(tr.tokens_to_nchw(t["cls"], 0, ncls, n, 256, 256), labels)
    loss, seg = ce + tv, None
    if targets is not None:
        flow, cp = fr.seg_loss(tr.tokens_to_nchw(t["flow"], 0, 3, n, 256, 256), targets.to(dtype))
        seg = flow + cp
        loss = seg + loss
    loss.backward()
    g = lambda R: {k: (R[k].grad if R[k].grad is not None else torch.zeros_like(R[k])) for k in R}
    r = {"loss": loss.detach(), "seg": None if seg is None else seg.detach(), "ce": ce.detach(), "tversky": tv.detach(),
         "blocks": [g(R) for R in RB], "neck": g(RN)}
    if RE is not None:
        r["embed"] = g(RE)
    return r


def replay(PB0: list, PN0: dict, x, labels, targets, ncls: int, lrs, keeps, dtype, net_dtype, weight_decay: float, fold: bool = True,
           PE0: dict | None = None):
    """``br.replay`` with the mask ``keeps[step]`` per step: AdamW on every tensor with one step counter -- a block with zero gradients
    still decays, as torch's AdamW treats a zero gradient.  Returns (losses, final block masters, final neck and head masters[, final
    embedding masters])."""
    PB = [{k: v.to(dtype).clone() for k, v in P.items()} for P in PB0]
    PN = {k: v.to(dtype).clone() for k, v in PN0.items()}
    PE = None if PE0 is None else {k: v.to(dtype).clone() for k, v in PE0.items()}
    groups = PB + [PN] + ([] if PE is None else [PE])
    M = [{k: torch.zeros_like(v) for k, v in P.items()} for P in groups]
    V = [{k: torch.zeros_like(v) for k, v in P.items()} for P in groups]
    losses = []
    for step, (lr, keep) in enumerate(zip(lrs, keeps), 1):
        r = loss_and_grads(PB, PN, x, labels, targets, ncls, keep, dtype, net_dtype, fold, PE)
        losses.append(float(r["loss"]))
        for P, G, m, v in zip(groups, r["blocks"] + [r["neck"]] + ([] if PE is None else [r["embed"]]), M, V):
            for k in P:
                if targets is None and k in ("Wf", "bf"):
                    continue
                tr.adamw_step(P[k], G[k].to(dtype), m[k], v[k], step, lr, weight_decay=weight_decay)
    return (np.array(losses), PB, PN) if PE is None else (np.array(losses), PB, PN, PE)
