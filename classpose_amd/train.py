"""Fine-tuning the 1x1 semantic class head (and, on request, the flow head) on the device with the backbone and the neck frozen.

The reference's cheapest adaptation mode, ``--freeze backbone segmentation_head neck`` (paper_experiments/run_training.py:92-98,
354-358; vit_sam.py:199-249): ``train_class_seg`` (train.py:356-655) then has two active losses with weight 1 each, the pixel
cross-entropy with ``ignore_index=-100`` and the focal Tversky loss, optimised by AdamW under the schedule of train.py:460-469.
Here the forward is the inference network (``cpx_net_forward``), and the loss, its gradient, the weight gradient and the AdamW
update are the HIP kernels of csrc/cpx_train.hip.  Because the frozen backbone is deterministic, the neck features of a fixed
training set are computed once and kept on the device (512 KB per 256 x 256 crop in bf16); an epoch then costs only the head.

Deliberately different from the reference:
  * the backbone runs as in inference.  The reference calls ``net.train()`` every epoch (train.py:609), which re-enables the
    stochastic layer drop of ``ClassTransformer.forward`` (vit_sam.py:165-173) even in a frozen backbone;
  * an image without a single annotated pixel raises ``ValueError`` (the reference's Tversky loss is NaN for such a batch);
  * augmentation is the device chain of ``classpose_amd.augment`` (stain jitter, flip / rotation / scale / crop, normalisation
    after both), which samples at exact source coordinates where OpenCV quantises them; the ``enhanced`` pipeline is not built;
  * oversampling (``train_probs``) and the rescale by cell diameter (``rescale``, ``diameters``) are opt-in arguments of
    ``train_class_head``, fed by ``classpose_amd.dataset_stats``; the reference's command line has both on by default;
  * no HDF5 datasets, learned loss weighting, multi-GPU exchange or optimiser-state resume.

``train_neck=True`` also trains the neck (``NeckParams``; the reference's ``--freeze backbone segmentation_head``, with
``train_flow_head`` its ``--freeze backbone``): the cache then holds the backbone's output rows and every step runs the neck's
training forward and ``cpx_neck_backward``.

``train_blocks=K`` also trains the last K transformer blocks (``BlockParams``) and, with K = depth, ``train_embed=True`` the
patch embedding and the position table (``EmbedParams``): the cache then holds patch rows and every step runs the whole
network, which with ``train_flow_head`` is the reference's run without ``--freeze``.  ``layer_drop=rate`` then drops trained blocks
per crop as the reference's ``net.train()`` does (``layer_drop_probs``, ``draw_keep_mask``, ``step(keep=)``).

``train_flow_head=True`` also trains the flow head ``out`` (``FlowHead``): the reference's ``--freeze backbone neck``, seg + CE +
Tversky with multiplier 1 each (train.py:482-493), the seg loss being cellpose's ``_loss_fn_seg`` restated (``ops.seg_loss``).

The reference's other class head, the UNet of ``--feature_transformation_structure``, is trained by
``train_unet.UNetHeadTrainer`` (same public surface; ``make_trainer`` picks the trainer from the checkpoint, and
``train_class_head`` runs with either).

A trainer owns its ``engine.NetWeights`` and updates the head operands in place: sharing them with an ``Engine`` that is running on
another stream is the caller's risk.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np
import torch

from . import _lib, augment as _augment, engine, ops
from ._lib import check, ptr
from .log import get_logger

train_logger = get_logger(__name__)

CROP = 256          # the network's sub-tile size: training crops are exactly one sub-tile
TOKENS = 1024


def lr_schedule(learning_rate: float, n_epochs: int) -> np.ndarray:
    """Per-epoch learning rates of train.py:460-469: ten warm-up epochs from 0 (entry 0 is 0.0; fewer than 10 epochs still yield
    10 entries), then constant; above 99 epochs the last 50 are replaced by ten halvings of 5 epochs each, above 300 the last 100
    by ten halvings of 10."""
    LR = np.linspace(0, learning_rate, 10)
    LR = np.append(LR, learning_rate * np.ones(max(0, n_epochs - 10)))
    if n_epochs > 300:
        LR = LR[:-100]
        for _ in range(10):
            LR = np.append(LR, LR[-1] / 2 * np.ones(10))
    elif n_epochs > 99:
        LR = LR[:-50]
        for _ in range(10):
            LR = np.append(LR, LR[-1] / 2 * np.ones(5))
    return LR


def prepare_state_dict(pretrained_model, nclasses: int | None = None, head_seed: int = 0) -> tuple[dict, int]:
    """(state dict with a 1x1 ``out_class`` head in the reference's key layout, class count).  A checkpoint without a semantic head
    (a plain Cellpose-SAM backbone) gets a freshly initialised one -- nn.Conv2d's default initialisation, seeded -- when ``nclasses``
    is given, the reference's starting point (README.md:197).  Host only."""
    sd = pretrained_model if isinstance(pretrained_model, dict) else \
        torch.load(os.fspath(pretrained_model), map_location="cpu", weights_only=True)
    sd = {k.removeprefix("module."): v for k, v in sd.items()}
    if any(k.startswith("out_class.encoder_blocks.") for k in sd):
        raise NotImplementedError("the checkpoint has a UNet semantic head: only the 1x1 out_class head is trainable here")
    if "out_class.weight" not in sd:
        if nclasses is None or nclasses < 2:
            raise ValueError("the checkpoint has no semantic head: pass nclasses >= 2 to initialise one")
        g = torch.Generator().manual_seed(head_seed)
        bound = 1.0 / np.sqrt(256.0)            # kaiming_uniform_(a = sqrt(5)) of a 1x1 conv with fan_in 256, and its bias bound
        oc = nclasses * 64
        sd["out_class.weight"] = (torch.rand(oc, 256, 1, 1, generator=g) * 2 - 1) * bound
        sd["out_class.bias"] = (torch.rand(oc, generator=g) * 2 - 1) * bound
        sd["W3"] = torch.eye(oc).reshape(oc, nclasses, 8, 8)
    ncls = sd["out_class.weight"].shape[0] // 64
    if "W3" not in sd:
        sd["W3"] = torch.eye(ncls * 64).reshape(ncls * 64, ncls, 8, 8)
    if sd["W3"].shape[1] != ncls or tuple(sd["out_class.weight"].shape[1:]) != (256, 1, 1):
        raise ValueError("out_class / W3 of the checkpoint do not describe a 1x1 head over 256 channels")
    if nclasses is not None and nclasses != ncls:
        raise ValueError(f"nclasses={nclasses} but the checkpoint's head has {ncls} classes")
    return sd, ncls


def _labels_i16(labels, dev) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(labels) if not isinstance(labels, torch.Tensor) else labels)
    if t.dim() != 3 or t.shape[1:] != (CROP, CROP) or t.dtype.is_floating_point:
        raise ValueError(f"labels: expected integer class maps (n, {CROP}, {CROP}), got {tuple(t.shape)} {t.dtype}")
    return t.to(device=dev, dtype=torch.int16).contiguous()


def _targets_f32(flow_targets, n: int, dev) -> torch.Tensor:
    t = torch.as_tensor(flow_targets)
    if t.dim() != 4 or tuple(t.shape) != (n, 3, CROP, CROP) or t.dtype != torch.float32:
        raise ValueError(f"flow_targets: expected float32 (mask, flow Y, flow X) planes {(n, 3, CROP, CROP)}, got {tuple(t.shape)} {t.dtype}")
    return t.to(dev).contiguous()


class LinearHead:
    """A parameter group -- a set of tensors that trains.  The trainer iterates over its groups; every group has ``keys`` (the
    state-dict keys it owns, in the reference's layout), ``update(step, lr, **adam)`` (one AdamW step from the gradients the group
    holds, then ``refresh``), ``refresh()`` (masters -> the operands of the trainer's ``engine.NetWeights``, rounded exactly as at
    load) and ``state()`` ({key: cpu tensor} in the reference's layout).

    This group is a 1x1 head ``prefix`` = nn.Conv2d(256, n_cols, 1) at rows ``row0 .. row0 + n_cols`` of ``head_w`` / ``head_b``: the
    float32 masters ``w`` [n_cols, 256] and ``b`` [n_cols] and their AdamW moments.  The class head ``out_class`` sits at row 192, the
    flow head ``out`` (vit_sam.py:181-182) at row 0; the pixel shuffles ``W3`` / ``W2`` are fixed and stay as loaded."""

    def __init__(self, sd: dict, weights, prefix: str, row0: int, n_cols: int):
        self.keys = (prefix + ".weight", prefix + ".bias")
        w, b = (sd[k] for k in self.keys)
        if tuple(w.shape) != (n_cols, 256, 1, 1) or tuple(b.shape) != (n_cols,):
            raise ValueError(f"{prefix}.weight / {prefix}.bias of the checkpoint do not describe a 1x1 head of {n_cols} columns over 256 channels")
        dev = weights.device
        self.weights, self.row0 = weights, row0
        self.w = w.detach().float().reshape(n_cols, 256).contiguous().to(dev)
        self.b = b.detach().float().contiguous().to(dev)
        self.m_w, self.v_w, self.m_b, self.v_b = (torch.zeros_like(t) for t in (self.w, self.w, self.b, self.b))
        self.dW = self.db = None

    def backward(self, feat: torch.Tensor, dlogits: torch.Tensor) -> None:
        """Holds the gradients of the batch: ``dlogits`` (rows, n_cols) of the head's loss and the features the head GEMM read."""
        self.dW, self.db = ops.head_wgrad(dlogits, feat)

    def update(self, step: int, lr: float, **adam) -> None:
        ops.adamw_step(self.w, self.dW, self.m_w, self.v_w, step, lr, **adam)
        ops.adamw_step(self.b, self.db, self.m_b, self.v_b, step, lr, **adam)      # net.parameters(): decay on the bias too
        self.refresh()

    def refresh(self) -> None:
        c = self.weights.c
        half = c.dtype != _lib.DT_F32
        ops.round_weights(self.w, c.head_w + self.row0 * 256 * (2 if half else 4), c.dtype, keep_f32=not half)
        ops.round_weights(self.b, c.head_b + self.row0 * 4, c.dtype, keep_f32=True)

    def state(self) -> dict:
        return {self.keys[0]: self.w.detach().cpu().reshape(-1, 256, 1, 1).clone(), self.keys[1]: self.b.detach().cpu().clone()}


class FlowHead(LinearHead):
    """The flow head ``out`` = nn.Conv2d(256, 192, 1) as a group (trained by the reference's ``--freeze backbone neck``,
    run_training.py:92-98), shared by ``HeadTrainer`` and ``train_unet.UNetHeadTrainer``."""

    def __init__(self, sd: dict, weights, element_size: int | None = None):
        super().__init__(sd, weights, "out", 0, 192)


NECK_KEYS = ("encoder.neck.0.weight", "encoder.neck.1.weight", "encoder.neck.1.bias", "encoder.neck.2.weight", "encoder.neck.3.weight",
             "encoder.neck.3.bias")


class NeckParams:
    """The neck as a group (vit_sam.py:216-249; trained by the reference's ``--freeze backbone`` and ``--freeze backbone
    segmentation_head``): float32 masters of its six tensors in operand layout, as views of ONE flat buffer in the order of
    ``ops.neck_grad_layout`` -- ``W0`` [256, 1024], ``gamma1``, ``beta1``, ``W2`` [256, 2304] (``neck.2.weight`` permuted (0, 2, 3, 1) as
    ``NetWeights`` does), ``gamma2``, ``beta2`` -- their AdamW moments and the gradient buffer ``cpx_neck_backward`` fills.  Weight
    decay applies to every tensor, the LayerNorm vectors included: the reference hands ``net.parameters()`` to AdamW."""
    keys = NECK_KEYS

    def __init__(self, sd: dict, weights):
        shapes = {"encoder.neck.0.weight": (256, 1024, 1, 1), "encoder.neck.2.weight": (256, 256, 3, 3)}
        for k in NECK_KEYS:
            if k not in sd or tuple(sd[k].shape) != shapes.get(k, (256,)):
                raise ValueError(f"{k} of the checkpoint does not describe the Cellpose-SAM neck")
        dev = weights.device
        self.weights = weights
        n, self.off = ops.neck_grad_layout()
        src = (sd[NECK_KEYS[0]].reshape(256, 1024), sd[NECK_KEYS[1]], sd[NECK_KEYS[2]],
               sd[NECK_KEYS[3]].permute(0, 2, 3, 1).reshape(256, 2304), sd[NECK_KEYS[4]], sd[NECK_KEYS[5]])
        flat = torch.cat([t.detach().float().reshape(-1) for t in src])
        if flat.numel() != n:
            raise _lib.CpxError("NeckParams: the host's parameter layout differs from the library's")
        self.params = flat.contiguous().to(dev)
        self.grads, self.m, self.v = (torch.zeros_like(self.params) for _ in range(3))

    def view(self, i: int) -> torch.Tensor:
        """Master tensor ``i`` of ``ops.NECK_GRAD_NAMES`` (a view of ``params``)."""
        shape = ops.NECK_GRAD_SHAPES[i]
        return self.params[self.off[i]:self.off[i] + int(np.prod(shape))].view(shape)

    def update(self, step: int, lr: float, **adam) -> None:
        """One AdamW step of all six tensors from the flat ``grads``, then ``refresh``."""
        ops.adamw_step(self.params, self.grads, self.m, self.v, step, lr, **adam)
        self.refresh()

    def refresh(self) -> None:
        """Masters -> ``neck0_w`` / ``neck2_w`` and the LayerNorm vectors of ``self.weights`` in place, rounded exactly as at load: the
        GEMM operands to the network dtype, the vectors through it and back to float32."""
        c = self.weights.c
        half = c.dtype != _lib.DT_F32
        dst = (c.neck0_w, c.neck_ln1_w, c.neck_ln1_b, c.neck2_w, c.neck_ln2_w, c.neck_ln2_b)
        for i, d in enumerate(dst):
            ops.round_weights(self.view(i), d, c.dtype, keep_f32=(not half) or i not in (0, 3))

    def state(self) -> dict:
        v = [self.view(i).detach().cpu().clone() for i in range(6)]
        return {NECK_KEYS[0]: v[0].reshape(256, 1024, 1, 1), NECK_KEYS[1]: v[1], NECK_KEYS[2]: v[2],
                NECK_KEYS[3]: v[3].view(256, 3, 3, 256).permute(0, 3, 1, 2).contiguous(), NECK_KEYS[4]: v[4], NECK_KEYS[5]: v[5]}


BLOCK_KEYS = ("norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.rel_pos_h", "attn.rel_pos_w", "attn.proj.weight",
              "attn.proj.bias", "norm2.weight", "norm2.bias", "mlp.lin1.weight", "mlp.lin1.bias", "mlp.lin2.weight", "mlp.lin2.bias")
_REL = (4, 5)                     # rel_pos_h, rel_pos_w in BLOCK_KEYS / ops.BLOCK_GRAD_NAMES


def rel_interp_matrix(n: int, size: int = 63) -> torch.Tensor:
    """A [size, n] float32 with ``engine.interp_rel_pos(t) == A @ t`` (get_rel_pos's linear resize is a linear map): the identity when
    the checkpoint's table already has ``size`` rows."""
    return engine.interp_rel_pos(torch.eye(n, dtype=torch.float32), size).contiguous()


class BlockParams:
    """The last ``K`` transformer blocks as a group (the reference trains them whenever ``--freeze`` does not name the backbone):
    float32 masters of every tensor of blocks ``first .. depth - 1`` as views of ONE flat buffer, ``K`` records in the order of
    ``ops.block_grad_layout`` -- norm1 gamma, beta | qkv W, b | (rel_h, rel_w slots, unused) | proj W, b | norm2 gamma, beta | lin1 W, b |
    lin2 W, b --, their AdamW moments, the gradient buffer ``cpx_blocks_backward`` fills and ``rounded``, the same record with every
    tensor rounded through the network dtype: the UNFOLDED parameters as the forward reads them, which that backward takes.

    The rel-pos tables keep the checkpoint's shape (``rel[j][t]`` [n, 64], e.g. n = 27): the kernels read the table interpolated to 63
    rows and divided by the scale, and their gradient of that operand goes back to the master through the transpose of the
    interpolation, a [63, n] matrix formed once on the host and kept on the device, times the 1 / scale = 8 of the operand convention.
    Each table takes an AdamW launch of its own, and ``refresh`` brings it to the host, interpolates it there in the network dtype with
    the load's own call and uploads it: 2 K small device-to-host synchronisations per step, the price of an operand that is bitwise the
    load's (torch's CPU and device interpolation need not round alike).

    ``refresh`` re-rounds every operand exactly as ``NetWeights.from_state_dict`` does, ``cpx_fold_layernorm`` included where LayerNorm
    is folded into qkv / lin1, so the next forward -- and inference from the saved checkpoint -- computes what was trained.  Weight
    decay applies to every tensor, as in the neck's group: the reference hands ``net.parameters()`` to AdamW."""

    def __init__(self, sd: dict, weights, K: int):
        depth = weights.depth
        if not 1 <= K <= depth:
            raise ValueError(f"train_blocks = {K}: the checkpoint has {depth} blocks")
        self.weights, self.K, self.first = weights, K, depth - K
        dev = weights.device
        self.n, self.off = ops.block_grad_layout()
        self.keys = tuple(f"encoder.blocks.{i}.{k}" for i in range(self.first, depth) for k in BLOCK_KEYS)
        flat, self.rel, self._At = [], [], []
        for i in range(self.first, depth):
            for t, (k, shape) in enumerate(zip(BLOCK_KEYS, ops.BLOCK_GRAD_SHAPES)):
                v = sd[f"encoder.blocks.{i}.{k}"].detach().float()
                if t in _REL:
                    if v.dim() != 2 or v.shape[1] != 64:
                        raise ValueError(f"encoder.blocks.{i}.{k}: expected a [n, 64] rel-pos table")
                    flat.append(torch.zeros(64 * 64))
                else:
                    if tuple(v.shape) != shape:
                        raise ValueError(f"encoder.blocks.{i}.{k} of the checkpoint does not describe a ViT-L block")
                    flat.append(v.reshape(-1))
            self.rel.append([sd[f"encoder.blocks.{i}.{BLOCK_KEYS[t]}"].detach().float().contiguous().to(dev) for t in _REL])
            self._At.append([(8.0 * rel_interp_matrix(r.shape[0]).T).contiguous().to(dev) for r in self.rel[-1]])
        self.params = torch.cat(flat).contiguous().to(dev)
        if self.params.numel() != self.n * K:
            raise _lib.CpxError("BlockParams: the host's parameter layout differs from the library's")
        self.grads, self.m, self.v, self.rounded = (torch.zeros_like(self.params) for _ in range(4))
        self.rel_grads = [[torch.zeros_like(r) for r in pair] for pair in self.rel]
        self.rel_m = [[torch.zeros_like(r) for r in pair] for pair in self.rel]
        self.rel_v = [[torch.zeros_like(r) for r in pair] for pair in self.rel]
        self._round_masters()

    def view(self, j: int, t: int, buf: torch.Tensor | None = None) -> torch.Tensor:
        """Tensor ``t`` of ``ops.BLOCK_GRAD_NAMES`` of trained block ``j`` (a view of ``params``, or of ``buf``: ``grads``, ``rounded``)."""
        shape = ops.BLOCK_GRAD_SHAPES[t]
        o = self.n * j + self.off[t]
        return (self.params if buf is None else buf)[o:o + int(np.prod(shape))].view(shape)

    def finish_backward(self) -> None:
        """After ``cpx_blocks_backward``: the operand tables' gradients -> the masters' shape, and their slots of ``grads`` cleared so
        that the one AdamW step over the flat buffer leaves the unused slots of ``params`` at zero."""
        for j in range(self.K):
            for a, t in enumerate(_REL):
                g = self.view(j, t, self.grads)
                torch.matmul(self._At[j][a], g[:63], out=self.rel_grads[j][a])
                g.zero_()

    def update(self, step: int, lr: float, **adam) -> None:
        ops.adamw_step(self.params, self.grads, self.m, self.v, step, lr, **adam)
        for j in range(self.K):
            for a in range(2):
                ops.adamw_step(self.rel[j][a], self.rel_grads[j][a], self.rel_m[j][a], self.rel_v[j][a], step, lr, **adam)
        self.refresh()

    def _round_masters(self) -> None:
        ops.round_weights(self.params, self.rounded.data_ptr(), self.weights.c.dtype, keep_f32=True)

    def refresh(self) -> None:
        """Masters -> the operands of ``self.weights`` in place, as ``NetWeights.from_state_dict`` forms them, and -> ``rounded``."""
        w = self.weights
        c, L = w.c, _lib.lib()
        half = c.dtype != _lib.DT_F32
        hd = engine.NET_DTYPES[w.precision]
        st = torch.cuda.current_stream(w.device).cuda_stream
        self._round_masters()
        for j in range(self.K):
            b = w.blocks[self.first + j]
            V = lambda t: self.view(j, t)
            vec = lambda t, dst: ops.round_weights(V(t), dst, c.dtype, keep_f32=True)
            mat = lambda t, dst: ops.round_weights(V(t), dst, c.dtype, keep_f32=not half)
            vec(0, b.ln1_w); vec(1, b.ln1_b); vec(8, b.ln2_w); vec(9, b.ln2_b)
            for tw, tb, tg, tbeta, dw, db, dcs, N in ((2, 3, 0, 1, b.qkv_w, b.qkv_b, b.qkv_colsum, 3072), (10, 11, 8, 9, b.fc1_w, b.fc1_b, b.fc1_colsum, 4096)):
                if c.fuse_ln:
                    check(L.cpx_fold_layernorm(ptr(V(tw)), ptr(V(tb)), ptr(V(tg)), ptr(V(tbeta)), N, 1024, c.dtype, dw, db, dcs, st), "fold_layernorm")
                else:
                    mat(tw, dw); vec(tb, db)
            mat(6, b.proj_w); vec(7, b.proj_b); mat(12, b.fc2_w); vec(13, b.fc2_b)
            for a, dst in enumerate((b.rel_h, b.rel_w)):
                # the load's own steps (a [n, 64] table: the host is the place): interpolate in the network dtype, x 8, a zero row
                t = engine.interp_rel_pos(self.rel[j][a].detach().cpu().to(hd)).float() * 8.0
                t = torch.cat([t, torch.zeros(1, 64)], 0).contiguous().to(w.device)
                ops.round_weights(t, dst, c.dtype, keep_f32=not half)

    def state(self) -> dict:
        out = {}
        for j in range(self.K):
            for t, k in enumerate(BLOCK_KEYS):
                v = self.rel[j][_REL.index(t)] if t in _REL else self.view(j, t)
                out[f"encoder.blocks.{self.first + j}.{k}"] = v.detach().cpu().clone()
        return out


EMBED_KEYS = ("encoder.patch_embed.proj.weight", "encoder.patch_embed.proj.bias", "encoder.pos_embed")


class EmbedParams:
    """The patch embedding and the position table as a group (what the reference trains on top of every block when ``--freeze`` is not
    given): float32 masters of ``patch_embed.proj.weight`` as ``W`` [1024, 192] (k in the order of ``ops.patchify_f32``),
    ``patch_embed.proj.bias`` [1024] and ``pos_embed`` [1024 tokens, 1024] as views of ONE flat buffer in the order of
    ``ops.embed_grad_layout``, their AdamW moments and the gradient buffer ``cpx_embed_backward`` fills.  Weight decay applies to all
    three: the reference hands ``net.parameters()`` to AdamW.  The position table is the architecture's own 32 x 32 grid."""
    keys = EMBED_KEYS

    def __init__(self, sd: dict, weights):
        shapes = ((1024, 3, 8, 8), (1024,), (1, 32, 32, 1024))
        for k, shape in zip(EMBED_KEYS, shapes):
            if k not in sd or tuple(sd[k].shape) != shape:
                what = "a position table of another grid size is not built" if k == EMBED_KEYS[2] and k in sd else "missing or of another shape"
                raise ValueError(f"{k} of the checkpoint is not {shape}: {what}")
        self.weights = weights
        n, self.off = ops.embed_grad_layout()
        flat = torch.cat([sd[k].detach().float().reshape(-1) for k in EMBED_KEYS])
        if flat.numel() != n:
            raise _lib.CpxError("EmbedParams: the host's parameter layout differs from the library's")
        self.params = flat.contiguous().to(weights.device)
        self.grads, self.m, self.v = (torch.zeros_like(self.params) for _ in range(3))

    def view(self, i: int, buf: torch.Tensor | None = None) -> torch.Tensor:
        """Master tensor ``i`` of ``ops.EMBED_GRAD_NAMES`` (a view of ``params``, or of ``buf``: ``grads``)."""
        shape = ops.EMBED_GRAD_SHAPES[i]
        return (self.params if buf is None else buf)[self.off[i]:self.off[i] + int(np.prod(shape))].view(shape)

    def update(self, step: int, lr: float, **adam) -> None:
        """One AdamW step of all three tensors from the flat ``grads``, then ``refresh``."""
        ops.adamw_step(self.params, self.grads, self.m, self.v, step, lr, **adam)
        self.refresh()

    def refresh(self) -> None:
        """Masters -> ``pe_w`` / ``pe_b`` / ``pos`` of ``self.weights`` in place, rounded exactly as at load: the GEMM operand to the
        network dtype, the two epilogue operands through it and back to float32."""
        c = self.weights.c
        half = c.dtype != _lib.DT_F32
        ops.round_weights(self.view(0), c.pe_w, c.dtype, keep_f32=not half)
        ops.round_weights(self.view(1), c.pe_b, c.dtype, keep_f32=True)
        ops.round_weights(self.view(2), c.pos, c.dtype, keep_f32=True)

    def state(self) -> dict:
        v = [self.view(i).detach().cpu().clone() for i in range(3)]
        return {EMBED_KEYS[0]: v[0].reshape(1024, 3, 8, 8), EMBED_KEYS[1]: v[1], EMBED_KEYS[2]: v[2].reshape(1, 32, 32, 1024)}


def layer_drop_probs(depth: int, rate: float) -> np.ndarray:
    """The probability with which each of ``depth`` blocks is dropped per crop (vit_sam.py:165, ``torch.linspace(0, rdrop, nlay)``):
    float64 (depth,), 0 for block 0 up to ``rate`` for the last."""
    if int(depth) < 1:
        raise ValueError(f"layer_drop_probs: depth {depth} is not a count of blocks")
    if not 0.0 <= float(rate) < 1.0:
        raise ValueError(f"layer_drop: a rate in [0, 1), not {rate!r}")
    return np.linspace(0.0, float(rate), int(depth), dtype=np.float64)


def draw_keep_mask(rng, n: int, depth: int, K: int, rate: float):
    """One layer-drop mask for ``n`` crops and the last ``K`` of ``depth`` blocks: uint8 (K, n), 1 where the block runs on the crop.
    Block i is dropped where a uniform draw is strictly below ``layer_drop_probs(depth, rate)[i]``, its ABSOLUTE index -- the
    reference's ``torch.rand((n, nlay)) < torch.linspace(0, rdrop, nlay)`` restricted to the trained blocks (its own random stream is
    not reproduced).  One ``rng.random((n, K))`` per mask; rate 0 returns None without drawing."""
    if not 1 <= int(K) <= int(depth):
        raise ValueError(f"draw_keep_mask: K = {K} trained blocks of depth {depth}")
    p = layer_drop_probs(depth, rate)[int(depth) - int(K):]
    if float(rate) == 0.0:
        return None
    u = np.asarray(rng.random((int(n), int(K))), dtype=np.float64)
    return np.ascontiguousarray(~(u < p[None, :]).T, dtype=np.uint8)


def check_layer_drop(layer_drop: float, train_blocks: int) -> None:
    """``layer_drop`` is a rate in [0, 1) and, above 0, needs trained blocks; raises ``ValueError`` with the reason otherwise."""
    if not 0.0 <= float(layer_drop) < 1.0:
        raise ValueError(f"layer_drop: a rate in [0, 1), not {layer_drop!r} (the reference's rdrop is 0.4)")
    if float(layer_drop) > 0.0 and int(train_blocks) <= 0:
        raise ValueError("layer_drop drops trained transformer blocks per crop: it needs train_blocks > 0 (the frozen blocks run once, "
                         "into the cache, and stay deterministic)")


def _of_class_group(name: str) -> property:
    return property(lambda self: getattr(self.groups[0], name))


class HeadTrainer:
    """Trains ``out_class`` (nn.Conv2d(256, nclasses * 64, 1)) of a checkpoint; everything else stays as loaded.

    The forward numerics are the inference engine's: GEMM operands rounded to the network dtype, a float32 master copy of the head kept
    here and re-rounded into the operands after every update, so a saved head run by ``predict_wsi`` computes the logits it was
    trained on.  ``feature_batch`` is the fixed number of crops per backbone launch (short batches are padded): kernel selection
    depends on the row count, so a fixed one keeps a crop's features bitwise independent of how the crops are batched.

    What trains is ``groups``, in order: the class head (``LinearHead``; ``w``, ``b`` and its moments are reachable from the trainer),
    then ``flow`` (``train_flow_head``) and ``neck`` (``train_neck``), each None when it does not train."""

    def __init__(self, pretrained_model, nclasses: int | None = None, device="cuda:0", precision: str = "bf16", class_weights=None,
                 weight_decay: float = 0.1, alpha: float = 0.3, gamma: float = 1.33, eps: float = 1e-6, feature_batch: int = 8,
                 head_seed: int = 0, betas=(0.9, 0.999), adam_eps: float = 1e-8, train_flow_head: bool = False,
                 train_neck: bool = False, train_blocks: int = 0, grad_precision: str = "fp32", attn_grad_precision: str = "fp32",
                 train_embed: bool = False, layer_drop: float = 0.0, layer_drop_seed: int = 0):
        self.device = torch.device(device)
        self.train_embed = bool(train_embed)
        self.train_blocks = int(train_blocks)
        if self.train_blocks < 0:
            raise ValueError("train_blocks: a count of blocks, 0 for none")
        # ``grad_precision`` = "bf16": the matrix products of the blocks' backward take bf16 operands; masters, AdamW,
        # ``refresh`` and the checkpoint are what they are in "fp32"
        check_grad_precision(grad_precision, self.train_blocks, precision)
        self.grad_precision = grad_precision
        # ``attn_grad_precision`` = "bf16" (with ``grad_precision`` "bf16"): the attention backward on bf16 operands too
        check_attn_grad_precision(attn_grad_precision, grad_precision)
        self.attn_grad_precision = attn_grad_precision
        # ``layer_drop`` = rate > 0: every ``step`` drops trained blocks per crop (stochastic depth) under a mask drawn from a
        # generator of the trainer's own; at 0 nothing is ever drawn.  ``evaluate`` never drops
        self.set_layer_drop(layer_drop, layer_drop_seed)
        train_neck = bool(train_neck) or self.train_blocks > 0           # the blocks' gradient comes through the neck
        if self.device.type != "cuda":
            raise RuntimeError("the head is trained by HIP kernels: pass a cuda device (there is no CPU path)")
        self.sd, self.nclasses = self._prepare(pretrained_model, nclasses, head_seed)
        self.precision = precision
        self.weights = engine.NetWeights.from_state_dict(self.sd, precision, self.device)
        self.dtype = engine.NET_DTYPES[precision]
        self.weight_decay, self.alpha, self.gamma, self.eps = weight_decay, alpha, gamma, eps
        self.betas, self.adam_eps = betas, adam_eps
        self.w_ce, self.w_tv, self.w_seg = 1.0, 1.0, 1.0  # LossAggregator(optimise=False): every multiplier exp(-0) = 1
        dev = self.device
        self.set_class_weights(class_weights)
        self.n_steps = 0
        self.feature_batch = int(feature_batch)
        self._L = _lib.lib()
        nS, c = self.feature_batch, self.weights.c
        self._net_ws = torch.empty(self._net_workspace_bytes(nS), dtype=torch.uint8, device=dev)
        self._head_fb = torch.empty((nS * TOKENS, c.ld_head), dtype=torch.float32, device=dev)
        self._buf: dict = {}
        # ``train_flow_head``: the flow head ``out`` trains too (the reference's ``--freeze backbone neck``); ``step`` / ``evaluate``
        # then take ``flow_targets`` and add the seg loss.  ``train_neck``: so does the neck -- the reference's ``--freeze
        # backbone segmentation_head``, with ``train_flow_head`` its ``--freeze backbone``; ``step`` / ``evaluate`` then start from
        # backbone rows (``backbone_features``)
        self.flow = FlowHead(self.sd, self.weights) if train_flow_head else None
        self.neck = NeckParams(self.sd, self.weights) if train_neck else None
        # ``train_blocks`` = K: the last K transformer blocks train too -- with ``train_flow_head`` and K = depth the
        # reference's run without ``--freeze``, except for the patch embedding and the position table (``train_embed``); ``step`` / ``evaluate`` then
        # start from the input rows of block depth - K (``backbone_features``)
        self.blocks = BlockParams(self.sd, self.weights, self.train_blocks) if self.train_blocks else None
        # ``train_embed``: the patch embedding and the position table train too -- with ``train_blocks`` = depth and
        # ``train_flow_head`` the reference's run without ``--freeze``, every parameter; ``step`` / ``evaluate`` then start from patch
        # rows (``patch_rows``)
        self.embed = None
        if self.train_embed:
            if self.train_blocks != self.weights.depth:
                raise ValueError(f"train_embed needs train_blocks = {self.weights.depth}, the checkpoint's depth (train_blocks is "
                                 f"{self.train_blocks}): the gradient reaches the patch embedding only through every block")
            self.embed = EmbedParams(self.sd, self.weights)
        self.diam_labels = None
        self.groups = [g for g in (self._class_group(), self.flow, self.neck, self.blocks, self.embed) if g is not None]

    # what ``train_unet.UNetHeadTrainer`` replaces: the checkpoint's preparation, the class group and the forward workspace
    def _prepare(self, pretrained_model, nclasses, head_seed) -> tuple[dict, int]:
        return prepare_state_dict(pretrained_model, nclasses, head_seed)

    def _class_group(self):
        return LinearHead(self.sd, self.weights, "out_class", 192, self.nclasses * 64)

    def _net_workspace_bytes(self, nS: int) -> int:
        return self._L.cpx_net_workspace_bytes(nS, self.weights.c.dtype)

    w, b, m_w, v_w, m_b, v_b = (_of_class_group(n) for n in ("w", "b", "m_w", "v_w", "m_b", "v_b"))

    def set_layer_drop(self, layer_drop: float, layer_drop_seed: int = 0) -> None:
        """The layer-drop rate of the following steps and a fresh ``np.random.default_rng(layer_drop_seed)`` for their masks."""
        check_layer_drop(layer_drop, self.train_blocks)
        self.layer_drop = float(layer_drop)
        self.layer_drop_seed = layer_drop_seed
        self._drop_rng = np.random.default_rng(layer_drop_seed)

    def set_diam_labels(self, diameters) -> None:
        """With the flow head training, ``diam_labels`` of the saved checkpoint becomes the mean diameter of the training set
        (train.py:440-442); no-op otherwise."""
        if self.flow is not None and diameters is not None and len(diameters):
            self.diam_labels = float(np.mean(np.asarray(diameters, np.float64)))

    def set_class_weights(self, class_weights) -> None:
        """Replace the per-class loss weights (None: unweighted) -- for weights that are computed from the training set after the
        trainer exists (``dataset_stats.get_class_weights``).  Takes effect from the next ``step`` / ``evaluate``."""
        if class_weights is not None:
            class_weights = torch.as_tensor(np.float32(class_weights)).to(self.device)  # train.py:444-448
            if class_weights.numel() != self.nclasses:
                raise ValueError("class_weights: one weight per class")
        self.class_weights = class_weights

    # -- forward pieces ----------------------------------------------------------------------------------------
    def _patches(self, X) -> torch.Tensor:
        dev = self.device
        if isinstance(X, np.ndarray):
            X = torch.from_numpy(np.ascontiguousarray(X))
        if X.dim() == 2 and X.shape[1] == 192 and X.dtype == self.dtype and X.is_cuda:      # patch rows (augment.augment_batch)
            if X.shape[0] % TOKENS:
                raise ValueError("patch rows: 1024 per crop")
            return X.contiguous()
        if X.dtype == torch.uint8:
            if X.dim() != 4 or X.shape[1:] != (CROP, CROP, 3):
                raise ValueError(f"uint8 crops must be (n, {CROP}, {CROP}, 3), got {tuple(X.shape)}")
            x = ops.normalize_img(X.to(dev)).permute(0, 3, 1, 2).contiguous()          # cellpose normalize_img, then NCHW
        elif X.dtype == torch.float32:
            if X.dim() != 4 or X.shape[1:] != (3, CROP, CROP):
                raise ValueError(f"float32 crops must be (n, 3, {CROP}, {CROP}) (already normalised), got {tuple(X.shape)}")
            x = X.to(dev)
        else:
            raise ValueError("crops must be uint8 (n, 256, 256, 3) or float32 (n, 3, 256, 256)")
        return ops.patchify_f32(x, self.dtype)

    def _forward_rows(self, X, rows_of, width: int, c=None) -> torch.Tensor:
        """``cpx_net_forward`` on n crops, ``feature_batch`` at a time; keeps ``rows_of(workspace, feature_batch, dtype)`` (n * 1024, width).
        ``c``: the weight struct to run (default: the trainer's own)."""
        patches = self._patches(X)
        n = patches.shape[0] // TOKENS
        FB, dev = self.feature_batch, self.device
        c = self.weights.c if c is None else c
        out = torch.empty((n * TOKENS, width), dtype=self.dtype, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        for s in range(0, n, FB):
            k = min(FB, n - s)
            chunk = patches[s * TOKENS:(s + k) * TOKENS]
            if k < FB:
                chunk = torch.cat([chunk, torch.zeros(((FB - k) * TOKENS, 192), dtype=self.dtype, device=dev)])
            check(self._L.cpx_net_forward(C.byref(c), ptr(chunk), FB, ptr(self._head_fb), ptr(self._net_ws), self._net_ws.numel(), st),
                  "net_forward")
            out[s * TOKENS:(s + k) * TOKENS] = rows_of(self._net_ws, FB, self.dtype)[:k * TOKENS]
        return out

    def features(self, X) -> torch.Tensor:
        """Neck features (n * 1024, 256) in the network dtype of n crops: the input of the class head."""
        return self._forward_rows(X, ops.neck_features, 256)

    def backbone_features(self, X) -> torch.Tensor:
        """The last FROZEN block's output (n * 1024, 1024) in the network dtype of n crops: the input of the neck, or with
        ``train_blocks`` = K that of block depth - K; what a trainer built with ``train_neck`` caches (2 MB per crop in bf16, against
        512 KB of neck features).  The frozen prefix is ``cpx_net_forward`` on a copy of the weight struct whose depth is depth - K (the
        copy points at the same operands; its tail runs on and is ignored); with K = depth the rows are the patch embedding's launch
        itself."""
        K, c = self.train_blocks, self.weights.c
        if K == 0:
            return self._forward_rows(X, ops.backbone_rows, 1024)
        if K == c.depth:
            return self._embed(self._patches(X))
        prefix = type(c).from_buffer_copy(c)              # the trainer's own struct is never changed: other users see its full depth
        prefix.depth = c.depth - K
        return self._forward_rows(X, ops.backbone_rows, 1024, prefix)

    def _embed(self, patches: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """The patch embedding's launch of ``cpx_net_forward`` on patch rows: block 0's input rows (n * 1024, 1024) in the network dtype."""
        c = self.weights.c
        if out is None:
            out = torch.empty((patches.shape[0], 1024), dtype=self.dtype, device=self.device)
        check(self._L.cpx_gemm(c.dtype, ptr(patches), c.pe_w, patches.shape[0], 1024, 192, ops.EPI["pos"], c.pe_b, c.pos, ptr(out), 1024,
                               torch.cuda.current_stream(self.device).cuda_stream), "patch embedding")
        return out

    def patch_rows(self, X) -> torch.Tensor:
        """Patch rows (n * 1024, 192) in the network dtype of n crops: the input of the patch embedding, what a trainer built with
        ``train_embed`` caches (384 KB per crop in bf16, against 2 MB of backbone rows)."""
        return self._patches(X)

    def _blocks_forward(self, X, keep=None):
        """The training forward of the last K blocks and the tail on the rows of ``X``: (x_out, the tail's ``ops.NeckForwardOut``).
        With ``train_embed`` it starts from patch rows, which are kept for the embedding's backward.  ``keep``: a layer-drop mask."""
        if self.embed is not None:
            self._rows = self._as_rows(X, 192, "patch rows")
            key = ("emb_x", self._rows.shape[0])
            if key not in self._buf:
                self._buf[key] = torch.empty((self._rows.shape[0], 1024), dtype=self.dtype, device=self.device)
            x = self._embed(self._rows, self._buf[key])
        else:
            x = self._as_rows(X, 1024, "backbone rows")
        rows, c = x.shape[0], self.weights.c
        key = ("blk_fwd", rows)
        if key in self._buf and keep is not None and not self._buf[key][2]:
            del self._buf[key]                            # (a mask on a trainer that has run without one: the workspace gains its staging rows)
        if key not in self._buf:
            drop = keep is not None or self.layer_drop > 0
            self._buf[key] = (torch.empty((rows, c.ld_head), dtype=torch.float32, device=self.device),
                              ops.blocks_train_workspace(rows // TOKENS, c.dtype, self.train_blocks, self.device, drop=drop), drop)
        head, ws, _drop = self._buf[key]
        self._bfwd = ops.blocks_forward_train(self.weights, x, c.depth - self.train_blocks, head=head, workspace=ws, keep=keep)
        return self._bfwd.x_out, self._bfwd.neck

    def _blocks_backward(self) -> None:
        """``cpx_blocks_backward`` from the dy0 the neck's backward has just left in its workspace."""
        fwd = self._bfwd
        rows, c = fwd.x_out.shape[0], self.weights.c
        key = ("blk_bwd", rows)
        grad_dtype = torch.bfloat16 if self.grad_precision == "bf16" else torch.float32
        attn_grad_dtype = torch.bfloat16 if self.attn_grad_precision == "bf16" else torch.float32
        if key not in self._buf:
            self._buf[key] = ops.blocks_backward_workspace(rows // TOKENS, c.dtype, self.device, grad_dtype, attn_grad_dtype)
        nws = self._buf[("neck_bwd", rows)][1]
        off = ops.neck_backward_workspace_offsets(rows // TOKENS, c.dtype, c.ld_head)[3]
        dy0 = nws[off:off + rows * 256 * 4].view(torch.float32).view(rows, 256)
        dx_in = None
        if self.embed is not None:                        # the gradient of block 0's input, then the embedding's own backward
            ekey = ("emb_bwd", rows)
            if ekey not in self._buf:
                self._buf[ekey] = (torch.empty((rows, 1024), dtype=torch.float32, device=self.device),
                                   ops.embed_backward_workspace(rows // TOKENS, c.dtype, self.device, grad_dtype))
            dx_in, ews = self._buf[ekey]
        ops.blocks_backward(self.weights, self.blocks.rounded, fwd, dy0, self.blocks.grads, self._buf[key], grad_dtype=grad_dtype,
                            attn_grad_dtype=attn_grad_dtype, dx_in=dx_in)
        self.blocks.finish_backward()
        if self.embed is not None:
            ops.embed_backward(self._rows, dx_in, self.embed.grads, ews, grad_dtype=grad_dtype)

    def _as_rows(self, X, width: int, what: str) -> torch.Tensor:
        """``X`` itself when it is cached rows of that width, else its crops through the backbone (width 192: through ``_patches``)."""
        if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[1] == width and X.dtype == self.dtype and X.is_cuda:
            if X.shape[0] % TOKENS:
                raise ValueError(f"{what}: 1024 rows per crop")
            return X.contiguous()
        if width == 192:
            return self._patches(X)
        return self.features(X) if width == 256 else self.backbone_features(X)

    def _neck_forward(self, X):
        """The training tail on the backbone rows of ``X`` (or on ``X`` itself when it is such rows): (x, ``ops.NeckForwardOut``)."""
        x = self._as_rows(X, 1024, "backbone rows")
        rows, c = x.shape[0], self.weights.c
        key = ("neck_fwd", rows)
        if key not in self._buf:
            self._buf[key] = (torch.empty((rows, c.ld_head), dtype=torch.float32, device=self.device),
                              ops.neck_train_workspace(rows // TOKENS, c.dtype, self.device))
        head, ws = self._buf[key]
        return x, ops.neck_forward_train(self.weights, x, head=head, workspace=ws)

    def _neck_backward(self, x, fwd, o, seg) -> torch.Tensor:
        """``cpx_neck_backward`` from the packed gradient of the head buffer: flow columns from the seg loss (zeros without it), class
        columns from the class loss, padding columns 0."""
        rows, c, ncols = x.shape[0], self.weights.c, self.nclasses * 64
        key = ("neck_bwd", rows)
        if key not in self._buf:
            self._buf[key] = (torch.zeros((rows, c.ld_head), dtype=torch.float32, device=self.device),
                              ops.neck_backward_workspace(rows // TOKENS, c.dtype, c.ld_head, self.device)[0])
        dhead, ws = self._buf[key]
        if seg is None:
            dhead[:, :192].zero_()
        else:
            dhead[:, :192].copy_(seg.dlogits)
        dhead[:, 192:192 + ncols].copy_(o.dlogits)
        return ops.neck_backward(self.weights, x, fwd, dhead, self.neck.grads, ws)

    def head(self, feat: torch.Tensor) -> torch.Tensor:
        """The head launch of ``cpx_net_forward`` on ``feat``: float32 (rows, ld_head), flow columns 0..191, class columns from 192."""
        c = self.weights.c
        rows = feat.shape[0]
        key = ("head", rows)
        if key not in self._buf:
            self._buf[key] = torch.empty((rows, c.ld_head), dtype=torch.float32, device=self.device)
        out = self._buf[key]
        check(self._L.cpx_gemm(c.dtype, ptr(feat), c.head_w, rows, c.ld_head, 256, ops.EPI["f32"], c.head_b, None, ptr(out), c.ld_head,
                               torch.cuda.current_stream(self.device).cuda_stream), "head gemm")
        return out

    def _loss(self, X, labels, keep=None):
        self._fwd = None
        if self.neck is not None:
            x, fwd = self._blocks_forward(X, keep) if self.blocks is not None else self._neck_forward(X)
            self._fwd = (x, fwd)
            feat = fwd.feat
        else:
            feat = self._as_rows(X, 256, "features")
        lab = _labels_i16(labels, self.device)
        if lab.shape[0] * TOKENS != feat.shape[0]:
            raise ValueError(f"{feat.shape[0] // TOKENS} crops but {lab.shape[0]} label maps")
        head = self.head(feat) if self.neck is None else fwd.head
        key = ("dl", feat.shape[0])
        if key not in self._buf:
            self._buf[key] = torch.empty((feat.shape[0], self.nclasses * 64), dtype=torch.float32, device=self.device)
        o = ops.class_loss(head, lab, self.nclasses, 192, self.class_weights, self.alpha, self.gamma, self.eps, self.w_ce, self.w_tv,
                           dlogits=self._buf[key], check_status=True)
        return feat, head, o

    def _seg_loss(self, head: torch.Tensor, flow_targets):
        """The seg loss of the batch whose head buffer is ``head`` and its gradient on the flow columns; None without targets."""
        if flow_targets is None:
            return None
        if self.flow is None:
            raise ValueError("flow_targets: the trainer was built without train_flow_head")
        rows = head.shape[0]
        key = ("dlf", rows)
        if key not in self._buf:
            self._buf[key] = torch.empty((rows, 192), dtype=torch.float32, device=self.device)
        return ops.seg_loss(head, _targets_f32(flow_targets, rows // TOKENS, self.device), self.w_seg, dlogits=self._buf[key])

    def _result(self, o, n, seg=None) -> dict:
        ce, tv = float(o.ce.item()), float(o.tversky.item())
        if seg is None:
            return {"ce": ce, "tversky": tv, "loss": self.w_ce * ce + self.w_tv * tv, "n": n}
        fl, cp = float(seg.flow.item()), float(seg.cp.item())
        return {"ce": ce, "tversky": tv, "seg": fl + cp, "seg_flow": fl, "seg_cp": cp,
                "loss": self.w_seg * (fl + cp) + self.w_ce * ce + self.w_tv * tv, "n": n}

    # -- public ------------------------------------------------------------------------------------------------
    def evaluate(self, X, labels, flow_targets=None, return_head: bool = False) -> dict:
        """Losses of a batch without an update.  ``return_head`` adds the float32 head buffer (a view that the next call overwrites).
        ``flow_targets`` (n, 3, 256, 256) float32 (mask, flow Y, flow X), for a trainer built with ``train_flow_head``: the result
        gains "seg" and "loss" is seg + ce + tversky."""
        feat, head, o = self._loss(X, labels)
        seg = self._seg_loss(head, flow_targets)
        r = self._result(o, feat.shape[0] // TOKENS, seg)
        if return_head:
            r["head"] = head
        return r

    def _step_mask(self, labels, keep):
        """The layer-drop mask of one step: the explicit ``keep`` (K, n), else one draw at the trainer's rate (None at rate 0)."""
        if keep is None and self.layer_drop == 0.0:
            return None
        if self.blocks is None:
            raise ValueError("keep: the trainer was built without train_blocks, there is no block to drop")
        n = len(labels)
        if keep is None:
            return draw_keep_mask(self._drop_rng, n, self.weights.depth, self.train_blocks, self.layer_drop)
        shape = tuple(getattr(keep, "shape", ()))
        if shape != (self.train_blocks, n):
            raise ValueError(f"keep: a uint8 mask ({self.train_blocks}, {n}) = (trained blocks, crops), not {shape}")
        return keep

    def step(self, X, labels, lr: float, flow_targets=None, keep=None) -> dict:
        """One optimisation step on a batch of crops (or of cached ``features``) at learning rate ``lr``; returns the losses of the
        batch BEFORE the update, like the reference's loop.  With ``flow_targets`` (see ``evaluate``) the flow head takes the same
        step from the seg loss: same step counter, betas and weight decay; without them it does not move.  ``keep`` (train_blocks, n)
        uint8: the layer-drop mask of this step (block j runs on crop i where ``keep[j, i]``); without it one is drawn when the
        trainer's ``layer_drop`` is above 0.  The losses are those of the dropped forward."""
        feat, head, o = self._loss(X, labels, self._step_mask(labels, keep))             # raises before anything is updated
        seg = self._seg_loss(head, flow_targets)          # (so does this)
        # every gradient from the operands of THIS forward (the neck's backward reads ``head_w``): before any refresh
        if self.neck is not None:
            self._neck_backward(*self._fwd, o, seg)
        if self.blocks is not None:
            self._blocks_backward()                       # (reads the dy0 of that neck backward and the operands of this forward)
        self.groups[0].backward(feat, o.dlogits)
        if seg is not None:
            self.flow.backward(feat, seg.dlogits)
        self.n_steps += 1
        kw = dict(betas=self.betas, eps=self.adam_eps, weight_decay=self.weight_decay)     # net.parameters(): decay on every tensor
        for g in self.groups:
            if g is not self.flow or seg is not None:
                g.update(self.n_steps, lr, **kw)
        return self._result(o, feat.shape[0] // TOKENS, seg)

    def state_dict(self) -> dict:
        """The checkpoint in the reference's key layout (vit_sam.py:269-285): every group's ``keys`` from its master copies
        (``out_class.weight`` [ncls * 64, 256, 1, 1], ``out_class.bias``; ``out.*`` and ``encoder.neck.*`` when they train), every
        other entry -- ``W3``, ``W2`` -- as loaded."""
        sd = dict(self.sd)
        for g in self.groups:
            sd.update(g.state())
        return self._flow_state(sd)

    def _flow_state(self, sd: dict) -> dict:
        """With the flow head training, ``diam_labels`` when ``set_diam_labels`` was given the training diameters."""
        if self.flow is not None and self.diam_labels is not None and "diam_labels" in sd:
            sd["diam_labels"] = torch.full_like(sd["diam_labels"], self.diam_labels)
        return sd

    def save(self, path, save_only_trainable_params: bool = False) -> None:
        sd = self.state_dict()
        if save_only_trainable_params:                    # the reference pops every parameter with requires_grad False
            sd = {k: sd[k] for g in self.groups for k in g.keys}
        torch.save(sd, os.fspath(path))

def check_grad_precision(grad_precision: str, train_blocks: int, precision: str) -> None:
    """``grad_precision`` "bf16" goes with trained blocks of a bf16 network only; raises ``ValueError`` with the reason otherwise."""
    if grad_precision not in ("fp32", "bf16"):
        raise ValueError(f"grad_precision: 'fp32' or 'bf16', not {grad_precision!r}")
    if grad_precision == "bf16":
        if int(train_blocks) <= 0:
            raise ValueError("grad_precision bf16 is the backward of the trained transformer blocks: it needs train_blocks > 0 "
                             "(the neck's and the heads' gradients stay float32)")
        if precision == "fp16":
            raise ValueError("grad_precision bf16 needs precision bf16: fp16 gradients would need loss scaling, which is not built")
        if precision != "bf16":
            raise ValueError(f"grad_precision bf16 needs precision bf16: a {precision} network has no half-precision operands")


def check_attn_grad_precision(attn_grad_precision: str, grad_precision: str) -> None:
    """``attn_grad_precision`` "bf16" (the attention backward on bf16 operands) goes with ``grad_precision`` "bf16" only -- which
    ``check_grad_precision`` ties to trained blocks of a bf16 network; raises ``ValueError`` with the reason otherwise."""
    if attn_grad_precision not in ("fp32", "bf16"):
        raise ValueError(f"attn_grad_precision: 'fp32' or 'bf16', not {attn_grad_precision!r}")
    if attn_grad_precision == "bf16" and grad_precision != "bf16":
        raise ValueError("attn_grad_precision bf16 needs grad_precision bf16: it is the last float32 product of the bf16 backward of the "
                         "trained blocks, not a mode of the float32 backward")


def make_trainer(pretrained_model, nclasses: int | None = None, feature_transformation_structure=None, **kw):
    """The trainer of a checkpoint's class head: ``train_unet.UNetHeadTrainer`` when the state dict has
    ``out_class.encoder_blocks.*`` keys (or a fresh UNet head of ``feature_transformation_structure`` is asked for),
    ``HeadTrainer`` otherwise.  ``kw``: the arguments both trainers share."""
    from . import train_unet
    return train_unet.make_trainer(pretrained_model, nclasses, feature_transformation_structure, **kw)


def _check_dataset(images, labels, what: str):
    images, labels = np.asarray(images), np.asarray(labels)
    ok_u8 = images.dtype == np.uint8 and images.ndim == 4 and images.shape[1:] == (CROP, CROP, 3)
    ok_f32 = images.dtype == np.float32 and images.ndim == 4 and images.shape[1:] == (3, CROP, CROP)
    if not (ok_u8 or ok_f32):
        raise ValueError(f"{what} images: expected (N, 256, 256, 3) uint8 or (N, 3, 256, 256) float32, got {images.shape} {images.dtype}")
    if labels.shape != (len(images), CROP, CROP) or not np.issubdtype(labels.dtype, np.integer):
        raise ValueError(f"{what} labels: expected integer class maps {(len(images), CROP, CROP)}, got {labels.shape} {labels.dtype}")
    empty = np.nonzero((labels == -100).reshape(len(labels), -1).all(1))[0]
    if len(empty):
        raise ValueError(f"{what} image {int(empty[0])} has no annotated pixel (every label is -100): drop it")
    return images, labels


def _crop_targets(instances, n: int, dev, what: str) -> torch.Tensor:
    """Flow-head targets (n, 3, 256, 256) float32 on the device of pre-cut crops from their instance maps, built once."""
    if instances is None:
        raise ValueError(f"train_flow_head needs {what}: integer instance maps aligned with the crops")
    instances = np.asarray(instances)
    if instances.shape != (n, CROP, CROP) or not np.issubdtype(instances.dtype, np.integer):
        raise ValueError(f"{what}: expected integer instance maps {(n, CROP, CROP)}, got {instances.shape} {instances.dtype}")
    return torch.stack(_augment.flow_targets_of(list(instances), dev))


def _is_u8_crops(images) -> bool:
    dt = getattr(images, "dtype", None)
    return (dt == np.uint8 or dt == torch.uint8) and images.ndim == 4 and images.shape[3] == 3


# what differs between the two sets ``train_class_head`` resolves: (name in messages, name of the instances argument, the two refusals of a pool)
_TRAINING = ("training", "instances", "an ImagePool carries its own class maps: pass labels=None",
             "train_flow_head: an ImagePool carries its own instances (build it with instances=..., pass instances=None)")
_VALIDATION = ("validation", "test_instances", "a validation ImagePool carries its own class maps: pass test_labels=None",
               "train_flow_head: a validation ImagePool carries its own instances (build it with instances=...)")


def _check_pool(pool, labels, instances, flow: bool, names) -> None:
    what, _inst, own_labels, own_instances = names
    if flow and (pool.pool_tgt is None or instances is not None):
        raise ValueError(own_instances)
    if labels is not None:
        raise ValueError(own_labels)
    empty = np.flatnonzero(~pool.annotated)
    if len(empty):
        raise ValueError(f"{what} image {int(empty[0])} has no annotated pixel (every label is -100): drop it")


def _resolve_dataset(images, labels, instances, trainer, flow: bool, names):
    """A set of fixed 256 x 256 crops from arrays or from an ``ImagePool`` (its cached ``augment.grid_crops``): ``(crops, class maps,
    flow-head targets float32 (N, 3, 256, 256) on the device or None, the pool's window table or None)``.  The targets (``flow``) come
    from ``instances`` or from the pool itself."""
    if isinstance(images, _augment.ImagePool):
        _check_pool(images, labels, instances, flow, names)
        x, y, win = _augment.grid_crops(images)
        return x, y, _augment.grid_flow_targets(images) if flow else None, win
    images, labels = _check_dataset(images, labels, names[0])
    return images, labels, _crop_targets(instances, len(images), trainer.device, names[1]) if flow else None, None


def _probs(train_probs, n: int) -> np.ndarray:
    train_probs = np.asarray(train_probs, dtype=np.float64)
    if train_probs.ndim != 1 or train_probs.shape[0] != n:
        raise ValueError("train_probs must have the same length as the dataset")
    return train_probs


def _normalised_probs(train_probs, n: int) -> np.ndarray:
    train_probs = _probs(train_probs, n)
    if np.any(train_probs < 0):
        raise ValueError("train_probs must be non-negative")
    if not float(train_probs.sum()) > 0.0:
        raise ValueError("train_probs must sum to a positive value")
    return train_probs / train_probs.sum()


def _rescale_factors(augment, diameters, n: int, diam_mean: float) -> np.ndarray:
    if augment is None:
        raise ValueError("rescale=True divides the random scale of the augmentation: it needs augment")
    if diameters is None:
        raise ValueError("rescale=True needs the diameters of the training images")
    diameters = np.asarray(diameters, dtype=np.float64)
    if diameters.shape != (n,) or not np.all(diameters > 0) or not diam_mean > 0:
        raise ValueError("diameters: one positive diameter per training image, and a positive diam_mean")
    return diameters / float(diam_mean)


def _epoch_order(rng, nimg: int, nimg_per_epoch: int, train_probs) -> np.ndarray:
    if train_probs is not None:
        return rng.choice(nimg, nimg_per_epoch, p=train_probs)
    return rng.permutation(nimg)[:nimg_per_epoch] if nimg_per_epoch <= nimg else rng.choice(nimg, nimg_per_epoch)


def _validate(trainer, X, labels, tgts, batch_size: int, cached: bool) -> tuple[float, float]:
    """Sample-weighted mean (loss, seg loss) of the validation set, in order; ``X`` cached rows (N, 1024, width) or crops."""
    tsum, tseg, tcount = 0.0, 0.0, 0
    for s in range(0, len(X), batch_size):
        x, y = X[s:s + batch_size], labels[s:s + batch_size]
        if cached:
            x = x.reshape(-1, X.shape[2])
        r = trainer.evaluate(x, y) if tgts is None else trainer.evaluate(x, y, flow_targets=tgts[s:s + batch_size])
        tsum += r["loss"] * r["n"]
        tseg += r.get("seg", 0.0) * r["n"]
        tcount += r["n"]
    return tsum / tcount, tseg / tcount


def train_class_head(trainer: HeadTrainer, images, labels, test_images=None, test_labels=None, batch_size: int = 8,
                     n_epochs: int = 100, learning_rate: float = 5e-5, nimg_per_epoch: int | None = None, cache_features: bool = True,
                     save_path=None, model_name: str | None = None, random_seed: int = 42, transform=None,
                     augment: str | None = None, scale_range: float = 0.5, label_fill: int = 0, train_probs=None, diameters=None,
                     diam_mean: float = 30.0, rescale: bool = False, train_flow_head: bool = False, instances=None,
                     test_instances=None, layer_drop: float | None = None, layer_drop_seed: int | None = None):
    """The epoch loop of train.py:606-655 for the frozen-backbone mode: per-epoch learning rate from ``lr_schedule``, seeded sampling
    without replacement (with, when ``nimg_per_epoch`` exceeds the set), sample-weighted running means of CE / Tversky / total,
    validation once per epoch, ``checkpoint_last.pt`` and ``checkpoint_best.pt`` (lowest validation loss; training loss without a
    validation set) next to the final model.  ``cache_features`` runs the backbone once per image; ``transform(X, labels, rng) ->
    (X, labels)``, a host callback per batch for callers who augment, forces the uncached path.
    ``augment`` ("hed_only": stain jitter + geometry, "he_staining": H&E stain-matrix perturbation + geometry, "hed_he": per image
    one of the two colour transforms + geometry, "quality": Gaussian blur and hue / brightness / saturation jitter + geometry,
    "hed_he_quality": "hed_he" followed by "quality", the reference's whole `enhanced` pipeline, "geometry": flip / rotation /
    scale / crop alone) augments every training
    batch on the device with ``augment.augment_batch`` (``scale_range``, ``label_fill`` as there), drawing from the epoch's
    generator after the sampling order and after ``transform``, which still runs first.  The training path is then uncached;
    validation is never augmented and its features are still cached when ``cache_features`` is set.
    ``train_probs`` (one non-negative weight per image, positive sum; normalised here, checked as the reference's
    ``DistributedEpochSampler`` checks them, dataset.py:560-570) turns the epoch's order into ``rng.choice(nimg, nimg_per_epoch,
    p=train_probs)``, the oversampling draw of dataset.py:597-601.  ``rescale=True`` divides the random scale of every augmented
    crop by ``diameters[i] / diam_mean`` (dataset.py:35-45): it needs ``augment`` and ``diameters`` (one per image, e.g.
    ``dataset_stats.clamp_diameters(label_stats(...).diameters)``).  With the defaults neither changes anything.
    ``images`` may be an ``augment.ImagePool`` of whole annotated images of any size (then ``labels`` is None; likewise the
    validation set).  The epoch's order is then drawn over the IMAGES and every draw is one fresh 256 x 256 window of its image
    (dataset.py:23-56): with ``augment`` the batches come from ``augment.augment_batch_pool``, ``train_probs`` / ``diameters`` are
    per image (``diameters`` defaults to the pool's), and ``transform`` is refused (there is no host crop to hand it).  Without
    ``augment`` the training set is the pool's cached ``augment.grid_crops``, one entry per window (``train_probs`` of an image go
    to each of its windows); validation always runs on the cached grid crops of its pool.  Array inputs behave as before.
    ``train_flow_head=True`` (a trainer built with ``train_flow_head``) trains the flow head too, the reference's ``--freeze backbone
    neck``: every step and every validation batch also gets the flow targets of its crops, and the seg loss is logged and counted
    next to CE / Tversky.  The targets come from ``instances`` / ``test_instances`` ((N, 256, 256) integer instance maps aligned
    with the crops; ``augment.flow_targets_of``, once) or, for an ``ImagePool``, from the pool itself (built with ``instances``);
    an augmented batch warps them with the crop, everything else uses plain windows of the stored planes.  ``transform`` is refused
    (a host callback cannot move the targets).  ``diameters``, when given, also set the checkpoint's ``diam_labels``.
    ``layer_drop`` / ``layer_drop_seed``, when given, go to ``trainer.set_layer_drop`` (the seed defaults to ``random_seed``) before the
    first step; left at None the trainer keeps the rate and the generator it was built with.  Validation never drops.
    Returns ``(path of the final model, train_losses, test_losses)``."""
    if layer_drop is not None:
        trainer.set_layer_drop(layer_drop, random_seed if layer_drop_seed is None else layer_drop_seed)
    if train_flow_head:
        if trainer.flow is None:
            raise ValueError("train_flow_head=True needs a trainer built with train_flow_head=True")
        if transform is not None:
            raise ValueError("train_flow_head: transform is a host callback on crops and cannot move the flow targets")
    elif instances is not None or test_instances is not None:
        raise ValueError("instances / test_instances are the flow head's targets: they need train_flow_head=True")
    pool = tgts = test_tgts = None                        # flow-head targets of pre-cut / grid crops, float32 (N, 3, 256, 256) on the device
    if isinstance(images, _augment.ImagePool) and transform is not None:
        raise ValueError("transform is a host callback on crops: an ImagePool has none to hand it")
    if isinstance(images, _augment.ImagePool) and augment is not None:       # the pool itself is the training set: every draw a fresh window
        pool, images = images, None
        _check_pool(pool, labels, instances, train_flow_head, _TRAINING)
        diameters = pool.diameters if diameters is None else diameters
    else:
        src = images
        images, labels, tgts, win = _resolve_dataset(images, labels, instances, trainer, train_flow_head, _TRAINING)
        if win is not None:                               # a pool's grid crops: an image's ``train_probs`` go to each of its windows
            diameters = None
            if train_probs is not None:
                train_probs = _probs(train_probs, len(src))[win[:, 0]]
    has_test = test_images is not None
    if has_test:
        test_images, test_labels, test_tgts, _win = _resolve_dataset(test_images, test_labels, test_instances, trainer, train_flow_head, _VALIDATION)
    if train_flow_head:
        trainer.set_diam_labels(diameters)
    nimg = len(pool) if pool is not None else len(images)
    nimg_per_epoch = nimg if nimg_per_epoch is None else int(nimg_per_epoch)
    if train_probs is not None:
        train_probs = _normalised_probs(train_probs, nimg)
    rsc = _rescale_factors(augment, diameters, nimg, diam_mean) if rescale else None
    LR = lr_schedule(learning_rate, n_epochs)
    model_name = "classpose_head" if model_name is None else model_name
    model_dir = (Path.cwd() if save_path is None else Path(save_path)) / model_name
    model_dir.mkdir(parents=True, exist_ok=True)
    filename = model_dir / model_name
    if augment is not None and augment != "geometry":
        _augment.get_config(augment)                       # unknown names and "enhanced" raise before anything is computed
    cached = cache_features and transform is None and augment is None        # a pool without augment trains on its grid crops
    # the stain perturbation re-renders from the image's own stain basis, a per-image constant: fitted once here for pre-cut
    # crops (a pool caches its own).  A transform callback changes the crops per batch, so their bases are then fitted per batch.
    bases = None
    if pool is None and transform is None and _augment._has_he(_augment.get_config(augment)) and _is_u8_crops(images):
        bases = _augment.stain_bases_of(images, trainer.device)
    test_cached = cache_features and has_test and (cached or augment is not None)
    dev = trainer.device
    lab_dev = feats = None
    # a trainer that trains the neck starts from the backbone's output instead of the neck's
    neck = getattr(trainer, "neck", None) is not None
    cache, width = (trainer.backbone_features, 1024) if neck else (trainer.features, 256)
    # one that trains the patch embedding starts from the patch rows themselves
    embed = getattr(trainer, "embed", None) is not None
    if embed:
        cache, width = trainer.patch_rows, 192
        train_logger.info(">>> train_embed: the cache holds patch rows (%d KB per crop), every step runs the patch embedding and all "
                          "%d blocks", TOKENS * 192 * (4 if trainer.precision == "fp32" else 2) // 1024, trainer.train_blocks)
    if cached:
        train_logger.info(">>> caching %s of %d training crops", "patch rows" if embed else "backbone rows" if neck else "neck features", nimg)
        feats = cache(images).view(nimg, TOKENS, width)
        lab_dev = _labels_i16(labels, dev)
    if test_cached:
        test_images, test_labels = cache(test_images).view(len(test_images), TOKENS, width), _labels_i16(test_labels, dev)
    train_logger.info(">>> n_epochs=%d, n_train=%d, n_test=%s, AdamW, learning_rate=%0.5f, weight_decay=%0.5f, cached features: %s",
                      n_epochs, nimg, len(test_images) if has_test else None, learning_rate, trainer.weight_decay, cached)
    aug_kw = dict(config=augment, scale_range=scale_range, label_fill=label_fill, dtype=trainer.dtype, out=CROP)

    def batch(idx, rng):
        """(crops or cached rows, class maps, flow targets or None) of the images ``idx``; draws from ``rng``: transform, then augment."""
        rs = None if rsc is None else rsc[idx]
        if cached:
            ti = torch.from_numpy(idx).to(dev)
            return feats[ti].reshape(-1, width), lab_dev[ti], None if tgts is None else tgts[ti.to(tgts.device)]
        if pool is not None:
            res = _augment.augment_batch_pool(pool, idx, rng, rescale=rs, flow_targets=train_flow_head, **aug_kw)
            return res if train_flow_head else (*res, None)
        x, y, t = images[idx], labels[idx], None if tgts is None else tgts[torch.from_numpy(idx).to(tgts.device)]
        if transform is not None:
            x, y = transform(x, y, rng)
        if augment is not None:
            res = _augment.augment_batch(x, y, rng, device=dev, rescale=rs, stain_bases=None if bases is None else bases.take(idx),
                                         flow_targets=t, **aug_kw)
            x, y, t = res if t is not None else (*res, None)
        return x, y, t

    train_losses, test_losses = np.zeros(n_epochs), np.zeros(n_epochs)
    best = np.inf
    for iepoch in range(n_epochs):
        rng = np.random.default_rng([random_seed, iepoch])
        order = _epoch_order(rng, nimg, nimg_per_epoch, train_probs)
        lr = float(LR[iepoch])
        sums, count = np.zeros(4), 0
        for s in range(0, len(order), batch_size):
            idx = order[s:s + batch_size]
            x, y, t = batch(idx, rng)
            r = trainer.step(x, y, lr) if t is None else trainer.step(x, y, lr, flow_targets=t)
            sums += np.array([r["ce"], r["tversky"], r["loss"], r.get("seg", 0.0)]) * len(idx)
            count += len(idx)
        train_losses[iepoch] = sums[2] / count
        seg_msg = f"seg={sums[3] / count:.4f}, " if train_flow_head else ""
        msg = f"{iepoch}, train_loss={sums[2] / count:.4f} ({seg_msg}ce={sums[0] / count:.4f}, tversky={sums[1] / count:.4f}), LR={LR[iepoch]:.6f}"
        if has_test:
            test_losses[iepoch], tseg = _validate(trainer, test_images, test_labels, test_tgts, batch_size, test_cached)
            msg += f", test_loss={test_losses[iepoch]:.4f}" + (f" (seg={tseg:.4f})" if train_flow_head else "")
        train_logger.info(msg)
        trainer.save(model_dir / "checkpoint_last.pt")
        score = test_losses[iepoch] if has_test else train_losses[iepoch]
        if score < best:
            best = score
            trainer.save(model_dir / "checkpoint_best.pt")
    trainer.save(filename)
    train_logger.info(">>> saved model to %s", filename)
    return filename, train_losses, test_losses
