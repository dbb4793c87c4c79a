"""Torch restatement of training the UNet semantic head (the yardstick of tests/test_unet_train_host.py and
tests/test_gpu_unet_train.py; pinned on the reference's own ``classpose.unet.UNet``, ``_loss_fn_class`` and ``_loss_fn_tversky``
through tests/golden/reference_unet_train.npz).

``unet_forward``   classpose.unet.UNet.forward (unet.py:175-196) as a function of a state dict, in the dtype of ``x``.  With
                   ``ste=<torch dtype>`` every weight, bias and op output is rounded to that dtype in the forward and the rounding is
                   the identity in the backward (straight-through) -- the numerics contract of the device trainer.
``loss_and_grads`` the two losses of train_reference.class_loss on the UNet's logits and autograd down to every parameter.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from train_reference import class_loss


def make_feat(nI: int, seed: int) -> torch.Tensor:
    """Deterministic pseudo-random neck features [nI, 256, 32, 32] float64, multiples of 1/16 in [-2, 2] (exact in bf16 and fp16):
    an integer hash of the element index, so the fixture need not store them."""
    idx = np.arange(nI * 256 * 1024, dtype=np.uint64)
    h = (idx * np.uint64(2654435761) + np.uint64(seed * 40503 + 1)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    v = ((h % np.uint64(65)).astype(np.float64) - 32.0) / 16.0
    return torch.from_numpy(v.reshape(nI, 256, 32, 32))


def _hash01(n: int, seed: int) -> np.ndarray:
    idx = np.arange(n, dtype=np.uint64)
    h = (idx * np.uint64(2654435761) + np.uint64(seed * 40503 + 1)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return h


def make_params(fts, ncls: int, seed: int) -> dict:
    """Deterministic UNet(256, ncls * 64, fts) parameters {key: float32 tensor}: multiples of bound / 4096 in [-bound, bound],
    bound = 1 / sqrt(fan_in) (the scale of torch's default initialisation), from an integer hash -- not stored in the fixture."""
    chans = {}
    cin = 256
    for n, c in enumerate(fts):
        chans[f"out_class.encoder_blocks.{n}."] = (cin, c)
        cin = c
    seq = [*fts[::-1], ncls * 64]
    for i in range(len(fts)):
        chans[f"out_class.decoder_blocks.{i}."] = (2 * seq[i], seq[i + 1])
    chans["out_class.bottleneck_down."] = chans["out_class.bottleneck_up."] = (fts[-1], fts[-1])
    sd = {}
    for j, key in enumerate(unet_keys(fts)):
        pfx = key[:key.index("block.")] if "block." in key else key[:key.rindex(".", 0, key.rindex("."))] + "."
        ci, co = chans[pfx]
        if "conv1" in key:
            shape = (co, ci, 3, 3)
        elif "conv2" in key:
            shape = (co, co, 3, 3)
        else:
            shape = (co, co, 2, 2)                  # downconv [cout][cin][2][2], upconv [cin][cout][2][2]: square either way
        bound = 1.0 / np.sqrt(shape[1] * shape[2] * shape[3])
        if key.endswith(".bias"):
            shape = (co,)
        n = int(np.prod(shape))
        v = ((_hash01(n, seed * 1000 + j) % np.uint64(8193)).astype(np.float64) - 4096.0) / 4096.0 * bound
        sd[key] = torch.from_numpy(v.astype(np.float32).reshape(shape))
    return sd


def _ste(t: torch.Tensor, dt) -> torch.Tensor:
    if dt is None or dt == t.dtype:
        return t
    return t + (t.detach().to(dt).to(t.dtype) - t.detach())


def unet_keys(fts, prefix: str = "out_class.") -> list[str]:
    """Parameter keys of UNet(., ., fts) in the order of torch's state_dict()."""
    keys = []

    def blk(p, tail):
        for conv in ("block.conv1", "block.conv2", tail):
            keys.extend([f"{p}{conv}.weight", f"{p}{conv}.bias"])

    for n in range(len(fts)):
        blk(f"{prefix}encoder_blocks.{n}.", "downconv")
    for n in range(len(fts)):
        blk(f"{prefix}decoder_blocks.{n}.", "upconv")
    blk(f"{prefix}bottleneck_down.", "downconv")
    blk(f"{prefix}bottleneck_up.", "upconv")
    return keys


def unet_forward(p: dict, x: torch.Tensor, n_levels: int, prefix: str = "out_class.", ste=None, taps: dict | None = None):
    """p: {key: tensor of x.dtype}; x [B, 256, h, w] -> [B, out_ch, h, w].  ``taps`` (a dict) receives every conv's output after
    its activation and rounding, keyed by the conv's state-dict prefix."""
    def conv(key, t, act, kind):
        w, b = _ste(p[prefix + key + ".weight"], ste), _ste(p[prefix + key + ".bias"], ste)
        if kind == 0:
            y = F.conv2d(t, w, b, padding=1)
        elif kind == 1:
            y = F.conv2d(t, w, b, stride=2)
        else:
            y = F.conv_transpose2d(t, w, b, stride=2)
        if act:
            y = torch.relu(y)
        y = _ste(y, ste)
        if taps is not None:
            taps[prefix + key] = y
        return y

    def block(pfx, t, skip_last=False):
        t = conv(pfx + "block.conv1", t, True, 0)
        return conv(pfx + "block.conv2", t, not skip_last, 0)

    feats = []
    for n in range(n_levels):
        x = conv(f"encoder_blocks.{n}.downconv", block(f"encoder_blocks.{n}.", x), False, 1)
        feats.append(x)
    feats = feats[::-1]
    x = conv("bottleneck_down.downconv", block("bottleneck_down.", x), False, 1)
    x = conv("bottleneck_up.upconv", block("bottleneck_up.", x), False, 2)
    for i in range(n_levels):
        x = block(f"decoder_blocks.{i}.", torch.cat((x, feats[i]), dim=1), skip_last=i == n_levels - 1)
        x = conv(f"decoder_blocks.{i}.upconv", x, False, 2)
    return x


def pixel_logits(y: torch.Tensor, ncls: int) -> torch.Tensor:
    """UNet output [B, ncls * 64, 32, 32] -> logits [B, ncls, 256, 256]: channel c * 64 + i * 8 + j of token (ph, pw) is pixel
    (8 ph + i, 8 pw + j) of class c (conv_transpose2d with W3 = the identity, vit_sam.py:236-249)."""
    B, _, th, tw = y.shape
    return y.reshape(B, ncls, 8, 8, th, tw).permute(0, 1, 4, 2, 5, 3).reshape(B, ncls, th * 8, tw * 8)


def loss_and_grads(sd: dict, feat: torch.Tensor, labels: torch.Tensor, fts, ncls: int, dtype=torch.float64, ste=None,
                   class_weights=None, alpha=0.3, gamma=1.33, eps=1e-6, w_ce=1.0, w_tv=1.0, taps: dict | None = None) -> dict:
    """feat [B, 256, 32, 32], labels [B, 256, 256] (-100: not annotated).  Returns ce, tversky, loss, logits [B, ncls, 256, 256] and
    grads {key: d loss / d parameter}, all computed in ``dtype`` and returned as float64."""
    keys = unet_keys(fts)
    p = {k: sd[k].detach().to(dtype).clone().requires_grad_(True) for k in keys}
    y = unet_forward(p, feat.detach().to(dtype), len(fts), ste=ste, taps=taps)
    z = pixel_logits(y, ncls)
    cw = None if class_weights is None else torch.as_tensor(class_weights).to(dtype)
    ce, tv, *_ = class_loss(z, labels, cw, alpha, gamma, eps)
    loss = w_ce * ce + w_tv * tv
    loss.backward()
    return dict(ce=ce.detach().double(), tversky=tv.detach().double(), loss=loss.detach().double(), logits=z.detach().double(),
                grads={k: p[k].grad.detach().double() for k in keys})
