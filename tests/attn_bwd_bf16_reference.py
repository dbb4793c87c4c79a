"""CPU restatement of the attention backward on bf16 operands (cpx_attention_backward_bf16) on top of
tests/block_train_reference.py, with ``round_bf16`` at exactly the operand positions of the contract and nowhere else:

    S'    = q . (k + Rh[qy - ky + 31] + Rw[qx - kx + 31])       nothing rounded (q, k, v and the tables are bf16 values already)
    P     = softmax_j(scale S')                                 exponent (S' - m) * scale, normalised before any rounding
    dP    = r(dO) v^T                                           r(dO) is the only form in which dO enters anything
    delta = sum_j P dP                                          from the unrounded P and dP
    dS'   = scale P (dP - delta)
    dv    = r(P)^T r(dO)        dk = r(dS')^T q
    dq    = r(dS') k + sum_ky r(G_h) Rh[..] + sum_kx r(G_w) Rw[..]
    G_h, G_w = the row-group sums of the unrounded dS';  dRh, dRw from the unrounded G_h, G_w and q

``rnd`` selects the rounding (``round_bf16``) or switches it off (``identity``); the arithmetic runs in qkv's dtype, one crop at a time
(the crops are independent; the table gradients are added in crop order).  With the rounding off the result is
block_train_reference.attention_backward (tests/test_attn_bwd_bf16_host.py pins that).

``block_backward`` is block_train_bf16_reference.block_backward with this attention backward in the place of the unrounded one."""
from __future__ import annotations

import torch

import block_train_bf16_reference as bb
import block_train_reference as br
from block_train_bf16_reference import identity, round_bf16  # noqa: F401  (re-exported)


def _one_crop(qkv, Rh, Rw, dO, rnd):
    q, k, v = br._split(qkv, 1)
    S = br._logits(q, k, Rh, Rw, 1)
    e = torch.exp((S - S.max(-1, keepdim=True).values) * br.SCALE)
    del S
    P = e * (1.0 / e.sum(-1, keepdim=True))
    del e
    dOr = rnd(dO).reshape(1, 1024, br.HEADS, br.HD).permute(0, 2, 1, 3)
    dP = dOr @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = br.SCALE * P * (dP - delta)
    del dP
    dv = rnd(P).transpose(-1, -2) @ dOr
    del P
    dSr = rnd(dS)
    dk = dSr.transpose(-1, -2) @ q
    d5 = dS.reshape(1, br.HEADS, br.GRID, br.GRID, br.GRID, br.GRID)      # [.., qy, qx, ky, kx]
    Gh, Gw = d5.sum(-1), d5.sum(-2)
    idx = br._rel_index()
    bias = torch.einsum("bnhwk,hkc->bnhwc", rnd(Gh), Rh[idx]) + torch.einsum("bnhwk,wkc->bnhwc", rnd(Gw), Rw[idx])
    dq = dSr @ k + bias.reshape(1, br.HEADS, 1024, br.HD)
    qg = q.reshape(1, br.HEADS, br.GRID, br.GRID, br.HD)
    dRh, dRw = torch.zeros_like(Rh), torch.zeros_like(Rw)
    dRh.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->hkc", Gh, qg).reshape(-1, br.HD))
    dRw.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->wkc", Gw, qg).reshape(-1, br.HD))
    dqkv = torch.stack([dq, dk, dv], 0).permute(1, 3, 0, 2, 4).reshape(1024, 3 * br.HEADS * br.HD)
    return dqkv, dRh, dRw


def attention_backward_bf16(qkv: torch.Tensor, Rh: torch.Tensor, Rw: torch.Tensor, dO: torch.Tensor, nS: int, rnd=round_bf16) -> dict:
    """{"dqkv", "dRh", "dRw"} as block_train_reference.attention_backward returns them, under the contract above"""
    dO = dO.to(qkv.dtype)
    parts = [_one_crop(qkv[c * 1024:(c + 1) * 1024], Rh, Rw, dO[c * 1024:(c + 1) * 1024], rnd) for c in range(nS)]
    dRh, dRw = parts[0][1], parts[0][2]
    for p in parts[1:]:
        dRh, dRw = dRh + p[1], dRw + p[2]
    return {"dqkv": torch.cat([p[0] for p in parts], 0), "dRh": dRh, "dRw": dRw}


def block_backward(*args, attn_rnd=round_bf16, **kw) -> dict:
    """block_train_bf16_reference.block_backward (same arguments) with ``attention_backward_bf16`` as its attention backward: the
    function is substituted in block_train_reference for the duration of the call"""
    plain = br.attention_backward
    br.attention_backward = lambda qkv, Rh, Rw, dO, nS: attention_backward_bf16(qkv, Rh, Rw, dO, nS, attn_rnd)
    try:
        return bb.block_backward(*args, **kw)
    finally:
        br.attention_backward = plain
