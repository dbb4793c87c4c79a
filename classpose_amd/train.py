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


class FlowHead:
    """The trainable state of the flow head ``out`` = nn.Conv2d(256, 192, 1) (vit_sam.py:181-182; trained by the reference's
    ``--freeze backbone neck``, run_training.py:92-98), shared by ``HeadTrainer`` and ``train_unet.UNetHeadTrainer``: the float32
    master ``w`` [192, 256] and ``b`` [192], their AdamW moments, and the refresh of rows 0..191 of the head operands (``head_w`` /
    ``head_b`` of the trainer's ``engine.NetWeights``), rounded as at load.  The pixel shuffle ``W2`` is fixed and stays as loaded."""

    def __init__(self, sd: dict, weights, element_size: int):
        if tuple(sd["out.weight"].shape) != (192, 256, 1, 1) or tuple(sd["out.bias"].shape) != (192,):
            raise ValueError("out.weight / out.bias of the checkpoint do not describe a 1x1 flow head over 256 channels")
        dev = weights.device
        self.weights, self._es = weights, element_size
        self.w = sd["out.weight"].detach().float().reshape(192, 256).contiguous().to(dev)
        self.b = sd["out.bias"].detach().float().contiguous().to(dev)
        self.m_w, self.v_w, self.m_b, self.v_b = (torch.zeros_like(t) for t in (self.w, self.w, self.b, self.b))

    def update(self, dlogits: torch.Tensor, feat: torch.Tensor, step: int, lr: float, **kw) -> None:
        """One AdamW step from the seg-loss gradient ``dlogits`` (rows, 192) and the features the head GEMM read."""
        dW, db = ops.head_wgrad(dlogits, feat)
        ops.adamw_step(self.w, dW, self.m_w, self.v_w, step, lr, **kw)
        ops.adamw_step(self.b, db, self.m_b, self.v_b, step, lr, **kw)
        self.refresh()

    def refresh(self) -> None:
        c = self.weights.c
        half = c.dtype != _lib.DT_F32
        ops.round_weights(self.w, c.head_w, c.dtype, keep_f32=not half)
        ops.round_weights(self.b, c.head_b, c.dtype, keep_f32=True)

    def state(self) -> dict:
        return {"out.weight": self.w.detach().cpu().reshape(192, 256, 1, 1).clone(), "out.bias": self.b.detach().cpu().clone()}


NECK_KEYS = ("encoder.neck.0.weight", "encoder.neck.1.weight", "encoder.neck.1.bias", "encoder.neck.2.weight", "encoder.neck.3.weight",
             "encoder.neck.3.bias")


class NeckParams:
    """The trainable state of the neck (vit_sam.py:216-249; trained by the reference's ``--freeze backbone`` and ``--freeze backbone
    segmentation_head``): float32 masters of its six tensors in operand layout, as views of ONE flat buffer in the order of
    ``ops.neck_grad_layout`` -- ``W0`` [256, 1024], ``gamma1``, ``beta1``, ``W2`` [256, 2304] (``neck.2.weight`` permuted (0, 2, 3, 1) as
    ``NetWeights`` does), ``gamma2``, ``beta2`` -- their AdamW moments and the gradient buffer ``cpx_neck_backward`` fills.  Weight
    decay applies to every tensor, the LayerNorm vectors included: the reference hands ``net.parameters()`` to AdamW."""

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

    def update(self, grads: torch.Tensor, step: int, lr: float, **kw) -> None:
        """One AdamW step of all six tensors from the flat ``grads``, then ``refresh``."""
        ops.adamw_step(self.params, grads, self.m, self.v, step, lr, **kw)
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


class HeadTrainer:
    """Trains ``out_class`` (nn.Conv2d(256, nclasses * 64, 1)) of a checkpoint; everything else stays as loaded.

    The forward numerics are the inference engine's: GEMM operands rounded to the network dtype, a float32 master copy of the head kept
    here and re-rounded into the operands after every update, so a saved head run by ``predict_wsi`` computes the logits it was
    trained on.  ``feature_batch`` is the fixed number of crops per backbone launch (short batches are padded): kernel selection
    depends on the row count, so a fixed one keeps a crop's features bitwise independent of how the crops are batched."""

    def __init__(self, pretrained_model, nclasses: int | None = None, device="cuda:0", precision: str = "bf16", class_weights=None,
                 weight_decay: float = 0.1, alpha: float = 0.3, gamma: float = 1.33, eps: float = 1e-6, feature_batch: int = 8,
                 head_seed: int = 0, betas=(0.9, 0.999), adam_eps: float = 1e-8, train_flow_head: bool = False,
                 train_neck: bool = False):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("the head is trained by HIP kernels: pass a cuda device (there is no CPU path)")
        self.sd, self.nclasses = prepare_state_dict(pretrained_model, nclasses, head_seed)
        self.precision = precision
        self.weights = engine.NetWeights.from_state_dict(self.sd, precision, self.device)
        self.dtype = engine.NET_DTYPES[precision]
        self.weight_decay, self.alpha, self.gamma, self.eps = weight_decay, alpha, gamma, eps
        self.betas, self.adam_eps = betas, adam_eps
        self.w_ce, self.w_tv = 1.0, 1.0                  # LossAggregator(optimise=False): both multipliers exp(-0) = 1
        ncols = self.nclasses * 64
        dev = self.device
        self.set_class_weights(class_weights)
        self.w = self.sd["out_class.weight"].detach().float().reshape(ncols, 256).contiguous().to(dev)      # master copies
        self.b = self.sd["out_class.bias"].detach().float().contiguous().to(dev)
        self.m_w, self.v_w, self.m_b, self.v_b = (torch.zeros_like(t) for t in (self.w, self.w, self.b, self.b))
        self.n_steps = 0
        self.feature_batch = int(feature_batch)
        c = self.weights.c
        self._L = _lib.lib()
        nS = self.feature_batch
        self._net_ws = torch.empty(self._L.cpx_net_workspace_bytes(nS, c.dtype), dtype=torch.uint8, device=dev)
        self._head_fb = torch.empty((nS * TOKENS, c.ld_head), dtype=torch.float32, device=dev)
        self._es = torch.empty(0, dtype=self.dtype).element_size()
        self._buf: dict = {}
        self._init_flow_head(train_flow_head)
        # ``train_neck``: the neck trains too (``NeckParams``) -- the reference's ``--freeze backbone segmentation_head``, with
        # ``train_flow_head`` its ``--freeze backbone``.  ``step`` / ``evaluate`` then start from backbone rows (``backbone_features``)
        self.neck = NeckParams(self.sd, self.weights) if train_neck else None

    def _init_flow_head(self, train_flow_head: bool) -> None:
        """``train_flow_head``: the flow head ``out`` trains too (the reference's ``--freeze backbone neck``); ``step`` / ``evaluate``
        then take ``flow_targets`` and add the seg loss, multiplier 1 like the other two (LossAggregator(optimise=False))."""
        self.w_seg = 1.0
        self.flow = FlowHead(self.sd, self.weights, self._es) if train_flow_head else None
        self.diam_labels = None

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

    def features(self, X) -> torch.Tensor:
        """Neck features (n * 1024, 256) in the network dtype of n crops: the input of the class head."""
        patches = self._patches(X)
        n = patches.shape[0] // TOKENS
        FB, c, dev = self.feature_batch, self.weights.c, self.device
        out = torch.empty((n * TOKENS, 256), dtype=self.dtype, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        for s in range(0, n, FB):
            k = min(FB, n - s)
            chunk = patches[s * TOKENS:(s + k) * TOKENS]
            if k < FB:
                chunk = torch.cat([chunk, torch.zeros(((FB - k) * TOKENS, 192), dtype=self.dtype, device=dev)])
            check(self._L.cpx_net_forward(C.byref(c), ptr(chunk), FB, ptr(self._head_fb), ptr(self._net_ws), self._net_ws.numel(), st),
                  "net_forward")
            out[s * TOKENS:(s + k) * TOKENS] = ops.neck_features(self._net_ws, FB, self.dtype)[:k * TOKENS]
        return out

    def backbone_features(self, X) -> torch.Tensor:
        """The last block's output (n * 1024, 1024) in the network dtype of n crops: the input of the neck, what a trainer built with
        ``train_neck`` caches (2 MB per crop in bf16, against 512 KB of neck features)."""
        patches = self._patches(X)
        n = patches.shape[0] // TOKENS
        FB, c, dev = self.feature_batch, self.weights.c, self.device
        out = torch.empty((n * TOKENS, 1024), dtype=self.dtype, device=dev)
        st = torch.cuda.current_stream(dev).cuda_stream
        for s in range(0, n, FB):
            k = min(FB, n - s)
            chunk = patches[s * TOKENS:(s + k) * TOKENS]
            if k < FB:
                chunk = torch.cat([chunk, torch.zeros(((FB - k) * TOKENS, 192), dtype=self.dtype, device=dev)])
            check(self._L.cpx_net_forward(C.byref(c), ptr(chunk), FB, ptr(self._head_fb), ptr(self._net_ws), self._net_ws.numel(), st),
                  "net_forward")
            out[s * TOKENS:(s + k) * TOKENS] = ops.backbone_rows(self._net_ws, FB, self.dtype)[:k * TOKENS]
        return out

    def _as_backbone(self, X) -> torch.Tensor:
        if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[1] == 1024 and X.dtype == self.dtype and X.is_cuda:
            if X.shape[0] % TOKENS:
                raise ValueError("backbone rows: 1024 rows per crop")
            return X.contiguous()
        return self.backbone_features(X)

    def _neck_forward(self, X):
        """The training tail on the backbone rows of ``X`` (or on ``X`` itself when it is such rows): (x, ``ops.NeckForwardOut``)."""
        x = self._as_backbone(X)
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

    def _as_features(self, X) -> torch.Tensor:
        if isinstance(X, torch.Tensor) and X.dim() == 2 and X.shape[1] == 256 and X.dtype == self.dtype and X.is_cuda:
            if X.shape[0] % TOKENS:
                raise ValueError("features: 1024 rows per crop")
            return X.contiguous()
        return self.features(X)

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

    def _loss(self, X, labels):
        self._fwd = None
        if self.neck is not None:
            x, fwd = self._neck_forward(X)
            self._fwd = (x, fwd)
            feat = fwd.feat
        else:
            feat = self._as_features(X)
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

    def _flow_kw(self) -> dict:
        return dict(betas=self.betas, eps=self.adam_eps, weight_decay=self.weight_decay)

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

    def step(self, X, labels, lr: float, flow_targets=None) -> dict:
        """One optimisation step on a batch of crops (or of cached ``features``) at learning rate ``lr``; returns the losses of the
        batch BEFORE the update, like the reference's loop.  With ``flow_targets`` (see ``evaluate``) the flow head takes the same
        step from the seg loss: same step counter, betas and weight decay."""
        feat, head, o = self._loss(X, labels)             # raises before anything is updated
        seg = self._seg_loss(head, flow_targets)          # (so does this)
        if self.neck is not None:                         # reads the head operand of THIS forward: before any refresh
            self._neck_backward(*self._fwd, o, seg)
        dW, db = ops.head_wgrad(o.dlogits, feat)
        self.n_steps += 1
        kw = dict(betas=self.betas, eps=self.adam_eps, weight_decay=self.weight_decay)     # net.parameters(): decay on the bias too
        ops.adamw_step(self.w, dW, self.m_w, self.v_w, self.n_steps, lr, **kw)
        ops.adamw_step(self.b, db, self.m_b, self.v_b, self.n_steps, lr, **kw)
        self._refresh_operands()
        if seg is not None:
            self.flow.update(seg.dlogits, feat, self.n_steps, lr, **kw)
        if self.neck is not None:
            self.neck.update(self.neck.grads, self.n_steps, lr, **kw)
        return self._result(o, feat.shape[0] // TOKENS, seg)

    def _refresh_operands(self) -> None:
        """Master weights -> the head operands of ``self.weights`` in place (rows 192... of head_w and head_b), rounded as at load."""
        c = self.weights.c
        half = c.dtype != _lib.DT_F32
        ops.round_weights(self.w, c.head_w + 192 * 256 * self._es, c.dtype, keep_f32=not half)
        ops.round_weights(self.b, c.head_b + 192 * 4, c.dtype, keep_f32=True)

    def state_dict(self) -> dict:
        """The checkpoint in the reference's key layout (vit_sam.py:269-285): ``out_class.weight`` [ncls * 64, 256, 1, 1],
        ``out_class.bias``, ``W3``; every other entry as loaded."""
        sd = dict(self.sd)
        sd["out_class.weight"] = self.w.detach().cpu().reshape(self.nclasses * 64, 256, 1, 1).clone()
        sd["out_class.bias"] = self.b.detach().cpu().clone()
        return self._flow_state(sd)

    def _flow_state(self, sd: dict) -> dict:
        """With the flow head training: ``out.weight`` [192, 256, 1, 1] and ``out.bias`` from the master copies (``W2`` as loaded),
        and ``diam_labels`` when ``set_diam_labels`` was given the training diameters."""
        if self.flow is not None:
            sd.update(self.flow.state())
            if self.diam_labels is not None and "diam_labels" in sd:
                sd["diam_labels"] = torch.full_like(sd["diam_labels"], self.diam_labels)
        if self.neck is not None:                         # ``encoder.neck.*`` from the master copies
            sd.update(self.neck.state())
        return sd

    def save(self, path, save_only_trainable_params: bool = False) -> None:
        sd = self.state_dict()
        if save_only_trainable_params:                    # the reference pops every parameter with requires_grad False
            sd = {k: sd[k] for k in ("out_class.weight", "out_class.bias") + (("out.weight", "out.bias") if self.flow is not None else ())
                  + (NECK_KEYS if self.neck is not None else ())}
        torch.save(sd, os.fspath(path))


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


def _pool_annotated(pool, what: str) -> None:
    empty = np.flatnonzero(~pool.annotated)
    if len(empty):
        raise ValueError(f"{what} image {int(empty[0])} has no annotated pixel (every label is -100): drop it")


def _pool_training_set(pool, labels, transform, augment, train_probs, diameters):
    """What ``train_class_head`` trains on when it is handed an ``ImagePool``: with ``augment`` the pool itself, else its cached grid
    crops as device arrays.  Returns ``(images, labels, pool or None, train_probs, diameters)``."""
    if labels is not None:
        raise ValueError("an ImagePool carries its own class maps: pass labels=None")
    if transform is not None:
        raise ValueError("transform is a host callback on crops: an ImagePool has none to hand it")
    _pool_annotated(pool, "training")
    if augment is not None:
        return None, None, pool, train_probs, pool.diameters if diameters is None else diameters
    x, y, win = _augment.grid_crops(pool)
    if train_probs is not None:
        train_probs = np.asarray(train_probs, dtype=np.float64)
        if train_probs.shape != (len(pool),):
            raise ValueError("train_probs must have the same length as the dataset")
        train_probs = train_probs[win[:, 0]]
    return x, y, None, train_probs, None


def train_class_head(trainer: HeadTrainer, images, labels, test_images=None, test_labels=None, batch_size: int = 8,
                     n_epochs: int = 100, learning_rate: float = 5e-5, nimg_per_epoch: int | None = None, cache_features: bool = True,
                     save_path=None, model_name: str | None = None, random_seed: int = 42, transform=None,
                     augment: str | None = None, scale_range: float = 0.5, label_fill: int = 0, train_probs=None, diameters=None,
                     diam_mean: float = 30.0, rescale: bool = False, train_flow_head: bool = False, instances=None,
                     test_instances=None):
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
    Returns ``(path of the final model, train_losses, test_losses)``."""
    pool = None
    tgts = test_tgts = None                               # flow-head targets of pre-cut / grid crops, float32 (N, 3, 256, 256) on the device
    if train_flow_head:
        if trainer.flow is None:
            raise ValueError("train_flow_head=True needs a trainer built with train_flow_head=True")
        if transform is not None:
            raise ValueError("train_flow_head: transform is a host callback on crops and cannot move the flow targets")
    elif instances is not None or test_instances is not None:
        raise ValueError("instances / test_instances are the flow head's targets: they need train_flow_head=True")
    if isinstance(images, _augment.ImagePool):
        src_pool = images
        if train_flow_head and (src_pool.pool_tgt is None or instances is not None):
            raise ValueError("train_flow_head: an ImagePool carries its own instances (build it with instances=..., pass instances=None)")
        images, labels, pool, train_probs, diameters = _pool_training_set(images, labels, transform, augment, train_probs, diameters)
        if train_flow_head and pool is None:
            tgts = _augment.grid_flow_targets(src_pool)
    else:
        images, labels = _check_dataset(images, labels, "training")
        if train_flow_head:
            tgts = _crop_targets(instances, len(images), trainer.device, "instances")
    has_test = test_images is not None
    if has_test and isinstance(test_images, _augment.ImagePool):
        if test_labels is not None:
            raise ValueError("a validation ImagePool carries its own class maps: pass test_labels=None")
        _pool_annotated(test_images, "validation")
        if train_flow_head:
            if test_images.pool_tgt is None or test_instances is not None:
                raise ValueError("train_flow_head: a validation ImagePool carries its own instances (build it with instances=...)")
            test_tgts = _augment.grid_flow_targets(test_images)
        test_images, test_labels, _win = _augment.grid_crops(test_images)
    elif has_test:
        test_images, test_labels = _check_dataset(test_images, test_labels, "validation")
        if train_flow_head:
            test_tgts = _crop_targets(test_instances, len(test_images), trainer.device, "test_instances")
    if train_flow_head:
        trainer.set_diam_labels(diameters)
    nimg = len(pool) if pool is not None else len(images)
    nimg_per_epoch = nimg if nimg_per_epoch is None else int(nimg_per_epoch)
    if train_probs is not None:
        train_probs = np.asarray(train_probs, dtype=np.float64)
        if train_probs.ndim != 1 or train_probs.shape[0] != nimg:
            raise ValueError("train_probs must have the same length as the dataset")
        if np.any(train_probs < 0):
            raise ValueError("train_probs must be non-negative")
        if not float(train_probs.sum()) > 0.0:
            raise ValueError("train_probs must sum to a positive value")
        train_probs = train_probs / train_probs.sum()
    rsc = None
    if rescale:
        if augment is None:
            raise ValueError("rescale=True divides the random scale of the augmentation: it needs augment")
        if diameters is None:
            raise ValueError("rescale=True needs the diameters of the training images")
        diameters = np.asarray(diameters, dtype=np.float64)
        if diameters.shape != (nimg,) or not np.all(diameters > 0) or not diam_mean > 0:
            raise ValueError("diameters: one positive diameter per training image, and a positive diam_mean")
        rsc = diameters / float(diam_mean)
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
    test_cached = cached or (cache_features and augment is not None)
    dev = trainer.device
    lab_dev = test_lab_dev = feats = test_feats = None
    # a trainer that trains the neck starts from the backbone's output instead of the neck's
    neck = getattr(trainer, "neck", None) is not None
    cache, width = (trainer.backbone_features, 1024) if neck else (trainer.features, 256)
    if cached:
        train_logger.info(">>> caching %s of %d training crops", "backbone rows" if neck else "neck features", nimg)
        feats = cache(images).view(nimg, TOKENS, width)
        lab_dev = _labels_i16(labels, dev)
    if test_cached:
        if has_test:
            test_feats = cache(test_images).view(len(test_images), TOKENS, width)
            test_lab_dev = _labels_i16(test_labels, dev)
    train_logger.info(">>> n_epochs=%d, n_train=%d, n_test=%s, AdamW, learning_rate=%0.5f, weight_decay=%0.5f, cached features: %s",
                      n_epochs, nimg, len(test_images) if has_test else None, learning_rate, trainer.weight_decay, cached)
    train_losses, test_losses = np.zeros(n_epochs), np.zeros(n_epochs)
    best = np.inf
    for iepoch in range(n_epochs):
        rng = np.random.default_rng([random_seed, iepoch])
        if train_probs is not None:
            order = rng.choice(nimg, nimg_per_epoch, p=train_probs)
        else:
            order = rng.permutation(nimg)[:nimg_per_epoch] if nimg_per_epoch <= nimg else rng.choice(nimg, nimg_per_epoch)
        sums, count = np.zeros(4), 0
        for s in range(0, len(order), batch_size):
            idx = order[s:s + batch_size]
            t = None
            if tgts is not None:
                t = tgts[torch.from_numpy(idx).to(tgts.device)]
            if cached:
                ti = torch.from_numpy(idx).to(dev)
                x, y = feats[ti].reshape(-1, width), lab_dev[ti]
            elif pool is not None:
                res = _augment.augment_batch_pool(pool, idx, rng, config=augment, scale_range=scale_range, label_fill=label_fill,
                                                  dtype=trainer.dtype, out=CROP, rescale=None if rsc is None else rsc[idx],
                                                  flow_targets=train_flow_head)
                x, y, t = res if train_flow_head else (*res, None)
            else:
                x, y = images[idx], labels[idx]
                if transform is not None:
                    x, y = transform(x, y, rng)
                if augment is not None:
                    res = _augment.augment_batch(x, y, rng, config=augment, scale_range=scale_range, label_fill=label_fill,
                                                 dtype=trainer.dtype, device=dev, out=CROP,
                                                 rescale=None if rsc is None else rsc[idx],
                                                 stain_bases=None if bases is None else bases.take(idx), flow_targets=t)
                    x, y, t = res if t is not None else (*res, None)
            r = trainer.step(x, y, float(LR[iepoch])) if t is None else trainer.step(x, y, float(LR[iepoch]), flow_targets=t)
            sums += np.array([r["ce"], r["tversky"], r["loss"], r.get("seg", 0.0)]) * len(idx)
            count += len(idx)
        train_losses[iepoch] = sums[2] / count
        seg_msg = f"seg={sums[3] / count:.4f}, " if train_flow_head else ""
        msg = f"{iepoch}, train_loss={sums[2] / count:.4f} ({seg_msg}ce={sums[0] / count:.4f}, tversky={sums[1] / count:.4f}), LR={LR[iepoch]:.6f}"
        if has_test:
            tsum, tseg, tcount = 0.0, 0.0, 0
            for s in range(0, len(test_images), batch_size):
                if test_cached:
                    x, y = test_feats[s:s + batch_size].reshape(-1, width), test_lab_dev[s:s + batch_size]
                else:
                    x, y = test_images[s:s + batch_size], test_labels[s:s + batch_size]
                r = trainer.evaluate(x, y) if test_tgts is None else trainer.evaluate(x, y, flow_targets=test_tgts[s:s + batch_size])
                tsum += r["loss"] * r["n"]
                tseg += r.get("seg", 0.0) * r["n"]
                tcount += r["n"]
            test_losses[iepoch] = tsum / tcount
            msg += f", test_loss={test_losses[iepoch]:.4f}" + (f" (seg={tseg / tcount:.4f})" if train_flow_head else "")
        train_logger.info(msg)
        trainer.save(model_dir / "checkpoint_last.pt")
        score = test_losses[iepoch] if has_test else train_losses[iepoch]
        if score < best:
            best = score
            trainer.save(model_dir / "checkpoint_best.pt")
    trainer.save(filename)
    train_logger.info(">>> saved model to %s", filename)
    return filename, train_losses, test_losses
