"""Fine-tuning the UNet semantic head (``--feature_transformation_structure``, classpose/unet.py:121-196) on the device with
the backbone, the neck and the flow head frozen.

The companion of ``train.HeadTrainer`` for checkpoints whose ``out_class`` is ``classpose.unet.UNet``: the forward is the
inference head (``cpx_unet_head_forward``, which leaves every op's output in its workspace -- the saved activations), the loss and
its gradient are ``cpx_class_loss``, the backward through the op list is ``cpx_unet_head_backward`` (csrc/cpx_train_unet.hip) and
the update is ONE ``cpx_adamw_step`` over a flat float32 buffer that holds every packed operand ``[Npad][Kpad]`` followed by its
bias ``[Npad]``, in op order -- the layout of ``engine.NetWeights._build_unet_ops``.  The reference's key layout
(``out_class.encoder_blocks.N.block.conv1.weight`` ...) exists only in ``state_dict()``.

Numerics contract: the forward multiplies operands rounded to the network dtype and stores every op's output in it; the backward
is float32 throughout and treats both roundings as the identity (straight-through), with the ReLU mask "stored output > 0" and
the data gradient taken through the ROUNDED operand.  Padded channels and the operand padding receive exact zero gradients, so
they stay exact zeros under AdamW.  No atomics: a step is bitwise reproducible.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import torch

from . import _lib, engine, ops
from ._lib import check, ptr
from .train import TOKENS, HeadTrainer, _of_class_group

MAX_LEVELS = 4          # 32 x 32 tokens halve once per level and once more in the bottleneck (engine.NetWeights.from_state_dict)


def _up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


def check_structure(fts) -> list[int]:
    fts = [int(c) for c in fts]
    if not fts or any(c < 1 for c in fts):
        raise ValueError("feature_transformation_structure: one positive channel count per level")
    if len(fts) > MAX_LEVELS:
        raise ValueError(f"UNet semantic head: at most {MAX_LEVELS} encoder levels fit the 32 x 32 token grid")
    return fts


def unet_plan(fts, out_ch: int) -> list[tuple[str, int, int, int, int]]:
    """The convolutions of classpose.unet.UNet(256, out_ch, fts) in the op order of ``_build_unet_ops``:
    (state-dict prefix, kind, cin_a, cin_b, cout) with the REAL channel counts; kind 0: 3x3, 1: 2x2 stride 2, 2: transposed 2x2."""
    plan = []

    def block(pfx, cin_a, cin_b, cout):
        plan.append((pfx + "block.conv1", 0, cin_a, cin_b, cout))
        plan.append((pfx + "block.conv2", 0, cout, 0, cout))

    cin = 256
    for n, c in enumerate(fts):
        p = f"out_class.encoder_blocks.{n}."
        block(p, cin, 0, c)
        plan.append((p + "downconv", 1, c, 0, c))
        cin = c
    c = fts[-1]
    block("out_class.bottleneck_down.", c, 0, c)
    plan.append(("out_class.bottleneck_down.downconv", 1, c, 0, c))
    block("out_class.bottleneck_up.", c, 0, c)
    plan.append(("out_class.bottleneck_up.upconv", 2, c, 0, c))
    seq = [*fts[::-1], out_ch]
    for i in range(len(fts)):
        p = f"out_class.decoder_blocks.{i}."
        block(p, seq[i], seq[i], seq[i + 1])
        plan.append((p + "upconv", 2, seq[i + 1], 0, seq[i + 1]))
    return plan


def param_layout(fts, out_ch: int):
    """(total elements, [(w_off, b_off, Npad, Kpad)] per op) of the flat parameter buffer -- what ``cpx_unet_param_layout`` returns
    for the op list ``_build_unet_ops`` makes of this structure."""
    p8 = lambda c: _up(c, 8)
    off, lay = 0, []
    for _key, kind, ca, cb, co in unet_plan(fts, out_ch):
        taps = (9, 4, 1)[kind]
        n_pad = _up(4 * p8(co) if kind == 2 else p8(co), 128)
        k_pad = _up(taps * (p8(ca) + p8(cb)), 64)
        lay.append((off, off + n_pad * k_pad, n_pad, k_pad))
        off += n_pad * k_pad + n_pad
    return off, lay


def pack_params(sd: dict, fts, out_ch: int) -> torch.Tensor:
    """State dict (reference keys) -> the flat float32 buffer; values are taken as they are (no rounding)."""
    p8 = lambda c: _up(c, 8)
    total, lay = param_layout(fts, out_ch)
    flat = torch.zeros(total, dtype=torch.float32)
    for (key, kind, cin_a, cin_b, cout), (w_off, b_off, n_pad, k_pad) in zip(unet_plan(fts, out_ch), lay):
        w, b = sd[key + ".weight"].detach().float(), sd[key + ".bias"].detach().float()
        ca, cb, co = p8(cin_a), p8(cin_b), p8(cout)
        if kind == 2:           # ConvTranspose2d [cin][cout][2][2] -> rows (dy, dx, co), cols ci
            if tuple(w.shape) != (cin_a, cout, 2, 2):
                raise ValueError(f"{key}.weight: expected {(cin_a, cout, 2, 2)}, got {tuple(w.shape)}")
            wt = torch.zeros(2, 2, co, ca)
            wt[:, :, :cout, :cin_a] = w.permute(2, 3, 1, 0)
            wm = wt.reshape(4 * co, ca)
            bt = torch.zeros(4, co)
            bt[:, :cout] = b[None, :]
            bm = bt.reshape(-1)
        else:                   # Conv2d [cout][cin_a + cin_b][k][k] -> cols (ky, kx, ci of a | ci of b)
            k = 3 if kind == 0 else 2
            if tuple(w.shape) != (cout, cin_a + cin_b, k, k):
                raise ValueError(f"{key}.weight: expected {(cout, cin_a + cin_b, k, k)}, got {tuple(w.shape)}")
            wt = torch.zeros(co, k, k, ca + cb)
            wk = w.permute(0, 2, 3, 1)
            wt[:cout, :, :, :cin_a] = wk[..., :cin_a]
            wt[:cout, :, :, ca:ca + cin_b] = wk[..., cin_a:]
            wm = wt.reshape(co, -1)
            bm = torch.zeros(co)
            bm[:cout] = b
        W = flat[w_off:w_off + n_pad * k_pad].view(n_pad, k_pad)
        W[:wm.shape[0], :wm.shape[1]] = wm
        flat[b_off:b_off + bm.shape[0]] = bm
    return flat


def unpack_params(flat: torch.Tensor, fts, out_ch: int) -> dict:
    """The inverse of ``pack_params``: {reference key: float32 tensor}."""
    p8 = lambda c: _up(c, 8)
    flat = flat.detach().float().cpu()
    total, lay = param_layout(fts, out_ch)
    if flat.numel() != total:
        raise ValueError(f"unpack_params: {flat.numel()} elements, the structure has {total}")
    sd = {}
    for (key, kind, cin_a, cin_b, cout), (w_off, b_off, n_pad, k_pad) in zip(unet_plan(fts, out_ch), lay):
        ca, cb, co = p8(cin_a), p8(cin_b), p8(cout)
        W = flat[w_off:w_off + n_pad * k_pad].view(n_pad, k_pad)
        if kind == 2:
            wt = W[:4 * co, :ca].reshape(2, 2, co, ca)
            sd[key + ".weight"] = wt[:, :, :cout, :cin_a].permute(3, 2, 0, 1).contiguous()
            sd[key + ".bias"] = flat[b_off:b_off + cout].clone()
        else:
            k = 3 if kind == 0 else 2
            wt = W[:co, :k * k * (ca + cb)].reshape(co, k, k, ca + cb)
            wk = torch.cat([wt[:cout, :, :, :cin_a], wt[:cout, :, :, ca:ca + cin_b]], -1)
            sd[key + ".weight"] = wk.permute(0, 3, 1, 2).contiguous()
            sd[key + ".bias"] = flat[b_off:b_off + cout].clone()
    return sd


def fresh_unet_head(fts, nclasses: int, head_seed: int = 0) -> dict:
    """A freshly initialised ``UNet(256, nclasses * 64, fts)`` as state-dict entries plus ``W3``: torch's default
    ``Conv2d`` / ``ConvTranspose2d`` initialisation (kaiming_uniform_(a = sqrt(5)) and the matching bias bound, both
    1 / sqrt(fan_in); a transposed conv's fan_in is cout * 4), drawn from a generator seeded with ``head_seed``."""
    fts = check_structure(fts)
    if nclasses is None or nclasses < 2:
        raise ValueError("a fresh UNet head needs nclasses >= 2")
    g = torch.Generator().manual_seed(head_seed)
    oc = nclasses * 64
    sd = {}
    for key, kind, cin_a, cin_b, cout in unet_plan(fts, oc):
        k = 3 if kind == 0 else 2
        shape = (cin_a, cout, 2, 2) if kind == 2 else (cout, cin_a + cin_b, k, k)
        bound = 1.0 / np.sqrt(float(shape[1] * k * k))
        sd[key + ".weight"] = (torch.rand(shape, generator=g) * 2 - 1) * bound
        sd[key + ".bias"] = (torch.rand(cout, generator=g) * 2 - 1) * bound
    sd["W3"] = torch.eye(oc).reshape(oc, nclasses, 8, 8)
    return sd


def has_unet_head(sd: dict) -> bool:
    return any(k.removeprefix("module.").startswith("out_class.encoder_blocks.") for k in sd)


def prepare_unet_state_dict(pretrained_model, nclasses: int | None = None, head_seed: int = 0,
                            feature_transformation_structure=None) -> tuple[dict, int, list[int]]:
    """(state dict with a UNet ``out_class`` in the reference's key layout, class count, channel list).  With
    ``feature_transformation_structure`` a checkpoint without a UNet head gets a fresh one on its backbone (its 1x1 head, if any, is
    dropped; the class count is the checkpoint's, or ``nclasses`` when it has none); a checkpoint that has one must match.  Host only."""
    sd = pretrained_model if isinstance(pretrained_model, dict) else \
        torch.load(os.fspath(pretrained_model), map_location="cpu", weights_only=True)
    sd = {k.removeprefix("module."): v for k, v in sd.items()}
    want = None if feature_transformation_structure is None else check_structure(feature_transformation_structure)
    if has_unet_head(sd):
        fts, ncls, _depth = engine.NetWeights.infer_structure(sd)
        fts = check_structure(fts)
        if want is not None and want != fts:
            raise ValueError(f"the checkpoint's UNet head has channels {fts}, not {want}")
        if ncls < 2:
            raise ValueError("the checkpoint's UNet head has no W3: cannot tell its class count")
    else:
        if want is None:
            raise ValueError("the checkpoint has no UNet semantic head: pass feature_transformation_structure to initialise one")
        ncls = sd["W3"].shape[1] if "W3" in sd and sd["W3"].shape[1] >= 2 else nclasses
        if ncls is None or ncls < 2:
            raise ValueError("the checkpoint has no semantic head: pass nclasses >= 2 to initialise one")
        sd = {k: v for k, v in sd.items() if not k.startswith("out_class.")}
        sd.update(fresh_unet_head(want, ncls, head_seed))
        fts = want
    if nclasses is not None and nclasses != ncls:
        raise ValueError(f"nclasses={nclasses} but the checkpoint's head has {ncls} classes")
    plan = unet_plan(fts, ncls * 64)
    missing = [k + s for k, *_ in plan for s in (".weight", ".bias") if k + s not in sd]
    if missing:
        raise ValueError(f"UNet head: the checkpoint lacks {missing[0]} (and {len(missing) - 1} more)")
    return sd, ncls, fts


class UNetParams:
    """The UNet head as a parameter group (see ``train.LinearHead``): the flat float32 master ``params`` of ``param_layout`` --
    checked against the library's -- with ``grads`` and the AdamW moments ``m``, ``v`` beside it, the head's forward (whose
    workspace holds the saved activations) and backward, and the reference's key layout in ``keys`` / ``state()``."""

    def __init__(self, sd: dict, weights, fts, out_ch: int):
        self.weights, self.fts, self.out_ch = weights, fts, out_ch
        self.keys = tuple(k + s for k, *_ in unet_plan(fts, out_ch) for s in (".weight", ".bias"))
        c, self._L = weights.c, _lib.lib()
        n = c.n_unet_ops
        total, self.layout = param_layout(fts, out_ch)
        w_off, b_off, n_pad, k_pad = (C.c_longlong * n)(), (C.c_longlong * n)(), (C.c_int * n)(), (C.c_int * n)()
        if self._L.cpx_unet_param_layout(c.unet_ops, n, w_off, b_off, n_pad, k_pad) != total or \
                [tuple(t) for t in zip(w_off, b_off, n_pad, k_pad)] != self.layout:
            raise _lib.CpxError("UNetHeadTrainer: the host's parameter layout differs from the library's")
        self.params = pack_params(sd, fts, out_ch).to(weights.device)         # float32 master copy
        self.grads, self.m, self.v = (torch.zeros_like(self.params) for _ in range(3))
        self._ws: dict = {}

    def _workspace(self, size_fn: str, nS: int) -> torch.Tensor:
        """The workspace of ``nS`` crops that the library's ``size_fn`` sizes, allocated once."""
        if (size_fn, nS) not in self._ws:
            c = self.weights.c
            nbytes = getattr(self._L, size_fn)(c.unet_ops, c.n_unet_ops, nS, c.dtype)
            self._ws[size_fn, nS] = torch.empty(nbytes, dtype=torch.uint8, device=self.params.device)
        return self._ws[size_fn, nS]

    def forward(self, feat: torch.Tensor, out: torch.Tensor) -> None:
        """``cpx_unet_head_forward``: the class columns (from 192) of the head buffer ``out``."""
        c, nS = self.weights.c, feat.shape[0] // TOKENS
        ws = self._workspace("cpx_unet_workspace_bytes", nS)
        check(self._L.cpx_unet_head_forward(c.unet_ops, c.n_unet_ops, ptr(feat), nS, ptr(out), c.ld_head, 192, c.dtype, ptr(ws),
                                            ws.numel(), torch.cuda.current_stream(feat.device).cuda_stream), "unet_head_forward")

    def backward(self, feat: torch.Tensor, dlogits: torch.Tensor) -> torch.Tensor:
        """``grads`` of the batch whose ``forward(feat, ...)`` ran last; ``dlogits`` from ``cpx_class_loss``."""
        nS = feat.shape[0] // TOKENS
        return ops.unet_head_backward(self.weights, feat, self._workspace("cpx_unet_workspace_bytes", nS), dlogits, self.grads,
                                      self._workspace("cpx_unet_backward_workspace_bytes", nS))

    def update(self, step: int, lr: float, **adam) -> None:
        ops.adamw_step(self.params, self.grads, self.m, self.v, step, lr, **adam)      # net.parameters(): decay on the biases too
        self.refresh()

    def refresh(self) -> None:
        """Master parameters -> the operands the op list points at, rounded as at load."""
        c = self.weights.c
        check(self._L.cpx_unet_refresh_operands(c.unet_ops, c.n_unet_ops, ptr(self.params), c.dtype,
                                                torch.cuda.current_stream(self.params.device).cuda_stream), "unet_refresh_operands")

    def state(self) -> dict:
        return unpack_params(self.params, self.fts, self.out_ch)


class UNetHeadTrainer(HeadTrainer):
    """Trains ``out_class`` = ``classpose.unet.UNet(256, nclasses * 64, fts)`` of a checkpoint; everything else stays as loaded.
    The public surface is ``HeadTrainer``'s, and ``train.train_class_head`` runs with either; the class group is ``UNetParams``
    (``params``, ``grads``, ``m``, ``v`` and ``layout`` are reachable from the trainer)."""

    def __init__(self, pretrained_model, nclasses: int | None = None, device="cuda:0", precision: str = "bf16", class_weights=None,
                 weight_decay: float = 0.1, alpha: float = 0.3, gamma: float = 1.33, eps: float = 1e-6, feature_batch: int = 8,
                 head_seed: int = 0, betas=(0.9, 0.999), adam_eps: float = 1e-8, feature_transformation_structure=None,
                 train_flow_head: bool = False, train_neck: bool = False, train_blocks: int = 0, train_embed: bool = False,
                 layer_drop: float = 0.0, layer_drop_seed: int = 0):
        if train_embed:
            raise NotImplementedError("train_embed: the UNet head's backward gives the neck output no gradient, so none reaches the "
                                      "blocks or the patch embedding; they train under the 1x1 class head only")
        if train_blocks:
            raise NotImplementedError("train_blocks: the UNet head's backward gives the neck output no gradient, so none reaches the "
                                      "blocks; they train under the 1x1 class head only")
        if train_neck:
            raise NotImplementedError("train_neck: the UNet head's backward gives the neck output no gradient; the neck trains "
                                      "under the 1x1 class head only")
        self._structure = feature_transformation_structure
        super().__init__(pretrained_model, nclasses, device, precision, class_weights, weight_decay, alpha, gamma, eps, feature_batch,
                         head_seed, betas, adam_eps, train_flow_head=train_flow_head, layer_drop=layer_drop, layer_drop_seed=layer_drop_seed)

    def _prepare(self, pretrained_model, nclasses, head_seed) -> tuple[dict, int]:
        sd, ncls, self.fts = prepare_unet_state_dict(pretrained_model, nclasses, head_seed, self._structure)
        return sd, ncls

    def _class_group(self) -> UNetParams:
        return UNetParams(self.sd, self.weights, self.fts, self.nclasses * 64)

    def _net_workspace_bytes(self, nS: int) -> int:
        c = self.weights.c
        return super()._net_workspace_bytes(nS) + self._L.cpx_unet_workspace_bytes(c.unet_ops, c.n_unet_ops, nS, c.dtype)

    params, grads, m, v, layout = (_of_class_group(n) for n in ("params", "grads", "m", "v", "layout"))

    def head(self, feat: torch.Tensor) -> torch.Tensor:
        """The head launches of ``cpx_net_forward`` on ``feat``: float32 (rows, ld_head), flow columns 0..191 from the head GEMM,
        class columns from 192 written by the UNet, whose workspace then holds the saved activations of this batch."""
        out = super().head(feat)
        self.groups[0].forward(feat, out)
        return out

    def backward(self, feat: torch.Tensor, dlogits: torch.Tensor) -> torch.Tensor:
        """``self.grads`` (flat, float32) of the batch whose forward ``head(feat)`` ran last; ``dlogits`` from ``cpx_class_loss``."""
        return self.groups[0].backward(feat, dlogits)


def make_trainer(pretrained_model, nclasses: int | None = None, feature_transformation_structure=None, **kw):
    """``UNetHeadTrainer`` for a checkpoint with ``out_class.encoder_blocks.*`` keys (or when a structure is asked for),
    ``HeadTrainer`` otherwise; ``kw`` are the trainers' common arguments."""
    sd = pretrained_model if isinstance(pretrained_model, dict) else \
        torch.load(os.fspath(pretrained_model), map_location="cpu", weights_only=True)
    if feature_transformation_structure is not None or has_unet_head(sd):
        return UNetHeadTrainer(sd, nclasses, feature_transformation_structure=feature_transformation_structure, **kw)
    return HeadTrainer(sd, nclasses, **kw)
