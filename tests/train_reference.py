"""Float64 torch restatement of the frozen-backbone training step (the yardstick of tests/test_train_host.py and
tests/test_gpu_train.py; pinned on the reference's own functions through tests/golden/reference_train.npz).

``class_loss``   pixel cross-entropy (ignore_index = -100) and focal Tversky loss as the reference's ``_loss_fn_class`` /
                 ``_loss_fn_tversky`` compute them, in whatever dtype the logits have; ``loss_and_grad`` adds autograd.
``adamw_replay`` torch.optim.AdamW semantics step by step in float64.
``lr_schedule``  is NOT restated here: the product's array is compared with the fixture directly.
"""
from __future__ import annotations

import numpy as np
import torch


def class_loss(logits: torch.Tensor, labels: torch.Tensor, class_weights=None, alpha=0.3, gamma=1.33, eps=1e-6):
    """logits [B, C, H, W] (any float dtype), labels [B, H, W] integer with -100 = not annotated.
    Returns (ce, tversky, tp, fp, fn) with tp / fp / fn of shape [B, C]."""
    B, C = logits.shape[:2]
    lbl = labels.long()
    w = None if class_weights is None else torch.as_tensor(class_weights, dtype=logits.dtype)
    ce = torch.nn.functional.cross_entropy(logits, lbl, weight=w, ignore_index=-100, reduction="mean")
    valid = (lbl != -100).to(logits.dtype)[:, None]
    one_hot = torch.nn.functional.one_hot(torch.where(lbl == -100, torch.zeros_like(lbl), lbl), num_classes=C)
    one_hot = one_hot.permute(0, 3, 1, 2).to(logits.dtype)
    p = torch.softmax(logits, dim=1)
    tp = torch.sum(p * one_hot * valid, dim=(2, 3))
    fp = torch.sum(p * (1 - one_hot) * valid, dim=(2, 3))
    fn = torch.sum((1 - p) * one_hot * valid, dim=(2, 3))
    raw = 1.0 - tp / (tp + alpha * fp + (1 - alpha) * fn)
    loss = torch.clip(raw, eps, 1 - eps).pow(1 / gamma)
    if w is not None:
        loss = loss * w
    return ce, loss.mean(), tp, fp, fn


def raw_tversky(tp, fp, fn, alpha=0.3):
    return 1.0 - tp / (tp + alpha * fp + (1 - alpha) * fn)


def loss_and_grad(logits, labels, class_weights=None, alpha=0.3, gamma=1.33, eps=1e-6, w_ce=1.0, w_tv=1.0):
    """dict of float64 results for logits given in any dtype: ce, tversky, loss, tp, fp, fn and dlogits = d loss / d logits."""
    z = logits.detach().double().clone().requires_grad_(True)
    cw = None if class_weights is None else torch.as_tensor(class_weights).double()
    ce, tv, tp, fp, fn = class_loss(z, labels, cw, alpha, gamma, eps)
    loss = w_ce * ce + w_tv * tv
    loss.backward()
    return dict(ce=ce.detach(), tversky=tv.detach(), loss=loss.detach(), tp=tp.detach(), fp=fp.detach(), fn=fn.detach(),
                dlogits=z.grad.detach())


def loss_and_grad_f32(logits, labels, class_weights=None, alpha=0.3, gamma=1.33, eps=1e-6, w_ce=1.0, w_tv=1.0):
    """The same in float32 on the CPU: its error against ``loss_and_grad`` sets the tolerance of the device tests."""
    z = logits.detach().float().clone().requires_grad_(True)
    cw = None if class_weights is None else torch.as_tensor(class_weights).float()
    ce, tv, tp, fp, fn = class_loss(z, labels, cw, alpha, gamma, eps)
    loss = w_ce * ce + w_tv * tv
    loss.backward()
    return dict(ce=ce.detach(), tversky=tv.detach(), loss=loss.detach(), tp=tp.detach(), fp=fp.detach(), fn=fn.detach(),
                dlogits=z.grad.detach())


def tokens_to_nchw(head: torch.Tensor, col0: int, ncls: int, nI: int, H: int, W: int) -> torch.Tensor:
    """Token-major head buffer [nI * (H/8) * (W/8)][ld] -> logits [nI, ncls, H, W]: column col0 + c*64 + i*8 + j of token
    (ph, pw) is pixel (8 ph + i, 8 pw + j) of class c (the pixel shuffle of the 1x1 out_class head)."""
    th, tw = H // 8, W // 8
    x = head[:, col0:col0 + ncls * 64].reshape(nI, th, tw, ncls, 8, 8)
    return x.permute(0, 3, 1, 4, 2, 5).reshape(nI, ncls, H, W)


def nchw_to_tokens(x: torch.Tensor) -> torch.Tensor:
    """Inverse of ``tokens_to_nchw`` for a tensor [nI, ncls, H, W] -> [nI * (H/8) * (W/8)][ncls * 64]."""
    nI, ncls, H, W = x.shape
    th, tw = H // 8, W // 8
    return x.reshape(nI, ncls, th, 8, tw, 8).permute(0, 2, 4, 1, 3, 5).reshape(nI * th * tw, ncls * 64)


def adamw_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1):
    """One torch.optim.AdamW step (decoupled weight decay, amsgrad off) on float64 tensors, in place."""
    p.mul_(1 - lr * weight_decay)
    m.mul_(beta1).add_(g, alpha=1 - beta1)
    v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = (v.sqrt() / np.sqrt(bc2)).add_(eps)
    p.addcdiv_(m, denom, value=-lr / bc1)


def adamw_replay(p0, grads, lrs, **kw):
    """Parameters after every step of an AdamW run in float64: list of tensors."""
    p = torch.as_tensor(p0).double().clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    out = []
    for t, (g, lr) in enumerate(zip(grads, lrs), 1):
        adamw_step(p, torch.as_tensor(g).double(), m, v, t, float(lr), **kw)
        out.append(p.clone())
    return out


def rel_l2(x, ref) -> float:
    x = torch.as_tensor(x).double().reshape(-1)
    ref = torch.as_tensor(ref).double().reshape(-1)
    d = float(torch.linalg.vector_norm(ref))
    return float(torch.linalg.vector_norm(x - ref)) / d if d > 0 else float(torch.linalg.vector_norm(x - ref))
