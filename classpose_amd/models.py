"""``ClassposeModel`` -- the reference's in-process model API on the MI355X engine.

Mirrors /root/reference/src/classpose/models.py:233-827 for the 2-D path used by the WSI
worker (predict_wsi.py:716-756) and by paper_experiments/run_inference.py:196-208: same
constructor arguments, same ``eval`` signature and return tuple
``(masks uint16, (rgb_flow, dP, cellprob, y_class, x.shape), class_masks int64, styles)``.
Everything between the uint8 image and the id maps runs on the GPU through the C ABI.  ``diameter=`` is the
reference's rescale to 30 px cells (models.py:633-639, 733-748, 782-820): the uint8 image is resized by 30 / diameter
on the device, the network runs at that size, and the fields (``resample=True``) or the maps (``resample=False``) are
resized back, see ``engine.Engine(net_hw=, resample=)``.  The 3-D / stitching / anisotropy branches of the reference
raise NotImplementedError instead of silently doing something else.
"""
from __future__ import annotations

import threading

import numpy as np
import torch

from . import engine, ops
from .log import get_logger

models_logger = get_logger(__name__)
PRECISIONS = ("fp32", "fp16", "bf16")


def resolve_precision(precision: str, device: torch.device | None = None) -> str:
    """models.py:37-69.  gfx950 has bf16 MFMA, so bf16 never falls back to fp16; fp32 runs on the
    exact-f32 matrix instruction (v_mfma_f32_32x32x2_f32, 1/16 of the bf16 rate) with float32
    weights and activations end to end."""
    if precision not in PRECISIONS:
        raise ValueError(f"Unknown precision '{precision}'. Expected one of {sorted(PRECISIONS)}.")
    models_logger.info("Using inference precision: %s", precision)
    return precision


def dx_to_circ(dP: np.ndarray) -> np.ndarray:
    """cellpose.plot.dx_to_circ (flow visualisation returned as flows[0])."""
    mag = np.sqrt(np.sum(dP ** 2, axis=0)).astype(np.float32)
    x01, x99 = np.percentile(mag, 1), np.percentile(mag, 99)
    mag = (mag - x01) / (x99 - x01) if x99 - x01 > 1e-3 else np.zeros_like(mag)
    mag = 255 * np.clip(mag, 0, 1.0) / 2
    ang = np.arctan2(dP[1], dP[0]) + np.pi
    rgb = np.zeros((*dP.shape[1:], 3), "uint8")
    for k in range(3):
        rgb[..., k] = np.clip(mag * (np.cos(ang + 2 * np.pi * k / 3) + 1), 0, 255).astype("uint8")
    return rgb


class ClassposeModel:
    def __init__(self, gpu: bool = True, pretrained_model: str | dict = "cpsam", model_type=None,
                 diam_mean=None, device: torch.device | None = None, nchan=None, nclasses: int = 3,
                 feature_transformation_structure: list[int] | None = None, precision: str = "bf16",
                 max_batch_tiles: int = 8, max_engines: int = 4):
        if device is None:
            device = torch.device("cuda:0")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("the MI355X engine has no CPU path: pass a cuda device")
        self.device = device
        self.precision = resolve_precision(precision, device)
        sd = pretrained_model if isinstance(pretrained_model, dict) else \
            torch.load(pretrained_model, map_location="cpu", weights_only=True)
        self.weights = engine.NetWeights.from_state_dict(sd, self.precision, device)
        if nclasses not in (None, self.weights.ncls):
            models_logger.warning("nclasses=%s but the checkpoint has %s classes; using the checkpoint",
                                  nclasses, self.weights.ncls)
        self.nclasses = self.weights.ncls
        self.max_batch_tiles = max_batch_tiles
        # several Python threads may share one model and call eval concurrently (the reference's --inference_threads,
        # predict_wsi.py:728-798): the weights are shared and read-only; an ENGINE (network + post-processing work spaces, output
        # slots, two HIP streams: ~0.9 GB for 8 tiles of 256 px at ViT-L, growing with the tile area) is checked out of a bounded pool
        # per (tile shape, options) for the duration of one batch and returned afterwards.  At most `max_engines` exist per key, so N
        # concurrent callers overlap on the GPU up to that number and queue beyond it, and a caller that starts a fresh thread per
        # request re-uses the pool's engines instead of leaking one per thread (round 4 keyed the table by thread id and never pruned).
        self.max_engines = max(1, int(max_engines))
        self._pool: dict = {}                    # key -> {"idle": [Engine], "n": engines created}
        self._cv = threading.Condition()
        self.timing = []

    class _Lease:
        def __init__(self, model, key, make):
            self.model, self.key, self.make, self.eng = model, key, make, None

        def __enter__(self):
            m = self.model
            with m._cv:
                slot = m._pool.setdefault(self.key, {"idle": [], "n": 0})
                while True:
                    if slot["idle"]:
                        self.eng = slot["idle"].pop()
                        return self.eng
                    if slot["n"] < m.max_engines:
                        slot["n"] += 1                       # reserve; built outside the lock (allocations take tens of ms)
                        break
                    m._cv.wait()
            try:
                self.eng = self.make()
            except BaseException:
                with m._cv:
                    slot["n"] -= 1
                    m._cv.notify()
                raise
            return self.eng

        def __exit__(self, *exc):
            m = self.model
            with m._cv:
                m._pool[self.key]["idle"].append(self.eng)
                m._cv.notify()

    def _engine(self, H, W, augment, tile_overlap, kw, net_hw=None, resample=True):
        """``with self._engine(...) as eng:`` -- an engine of the bounded pool for this tile shape, network shape and these options"""
        resample = bool(resample) or net_hw is None          # without a rescale there is nothing to resample: one pool entry
        key = (H, W, bool(augment), float(tile_overlap), tuple(sorted(kw.items())), net_hw, resample)
        return self._Lease(self, key, lambda: engine.Engine(self.weights, H, W, batch_tiles=self.max_batch_tiles,
                                                            augment=augment, tile_overlap=tile_overlap, net_hw=net_hw,
                                                            resample=resample, **kw))

    @staticmethod
    def _net_shapes(imgs, diameter, augment, tile_overlap):
        """Per image the network size ``(int(H * 30 / d), int(W * 30 / d))`` of models.py:633-639 (truncated, in Python float
        arithmetic), or None where that is the image's own size (``diameter=None``, or a diameter that changes nothing)."""
        if diameter is None:
            return [None] * len(imgs)
        if isinstance(diameter, (list, tuple, np.ndarray)) and np.ndim(diameter) > 0:
            ds = [d for d in diameter]
            if len(ds) != len(imgs):
                raise ValueError(f"diameter has {len(ds)} entries for {len(imgs)} images")
        else:
            ds = [diameter] * len(imgs)
        out = []
        for im, d in zip(imgs, ds):
            d = float(d)
            if not (np.isfinite(d) and d > 0):
                raise ValueError(f"diameter must be positive and finite, got {d}")
            scaling = 30.0 / d
            H, W = im.shape[:2]
            Hs, Ws = int(H * scaling), int(W * scaling)
            if Hs < 1 or Ws < 1:
                raise ValueError(f"diameter={d} would resize a {H}x{W} image to {Hs}x{Ws}")
            try:
                engine.make_tiling(Hs, Ws, engine.BSIZE, augment, tile_overlap)
            except ValueError as e:
                raise ValueError(f"diameter={d} resizes the {H}x{W} image to {Hs}x{Ws}: {e}") from None
            out.append((Hs, Ws) if (Hs, Ws) != (H, W) else None)
        return out

    def engines_alive(self) -> int:
        with self._cv:
            return sum(slot["n"] for slot in self._pool.values())

    def eval(self, x, batch_size: int = 8, resample: bool = True, channels=None, channel_axis=None,
             z_axis=None, normalize=True, invert: bool = False, rescale=None, diameter=None,
             flow_threshold: float = 0.4, cellprob_threshold: float = 0.0, do_3D: bool = False,
             anisotropy=None, flow3D_smooth=0, stitch_threshold: float = 0.0, min_size: int = 15,
             max_size_fraction: float = 0.4, niter=None, augment: bool = False,
             tile_overlap: float = 0.1, bsize: int = 256, compute_masks: bool = True, progress=None,
             cell_confidence: bool = False):
        """``cell_confidence=True`` (not in the reference): the return gains a fifth element, per image one structured array
        with a row per id of ``masks`` -- ``label``, ``cls`` (its class-map value), ``area`` (pixels), ``votes[ncls]`` (pixels
        whose arg-max class is c), ``prob[ncls]`` (the mean softmax probability of class c over the cell's pixels) and
        ``detection`` (the mean sigmoid of cellprob); classpose_amd/confidence.py has the definitions.  The statistics are
        computed from the id map and the fields that the class vote read, at the size the vote ran at: with ``diameter=`` and
        ``resample=False`` that is the NETWORK's size, so ``area`` and ``votes`` count pixels of the resized image there, not
        of the returned ``masks``.  With the default the four-tuple is what it was."""
        if do_3D or stitch_threshold > 0 or invert or normalize is not True:
            raise NotImplementedError("only the 2-D path of ClassposeModel.eval is built "
                                      "(no do_3D / stitch / invert / custom normalize)")
        if bsize != 256:
            raise NotImplementedError("bsize is fixed to 256 like the WSI worker (predict_wsi.py:1563)")
        is_list = isinstance(x, (list, tuple))
        imgs = list(x) if is_list else [x]
        outs = [None] * len(imgs)
        # images of equal shape are batched across the list (the reference loops one by one)
        groups: dict = {}
        for i, im in enumerate(imgs):
            im = np.asarray(im)
            if im.ndim != 3 or im.shape[-1] != 3 or im.dtype != np.uint8:
                raise ValueError("expected uint8 (H, W, 3) RGB tiles")
            imgs[i] = im
        # (rescale= is ignored like in the reference, which only warns that it is deprecated)
        net_shapes = self._net_shapes(imgs, diameter, augment, tile_overlap)
        for i, im in enumerate(imgs):
            groups.setdefault((im.shape, net_shapes[i]), []).append(i)
        kw = dict(niter=200 if not niter else int(niter), cellprob_threshold=cellprob_threshold,
                  flow_threshold=flow_threshold, min_size=min_size, max_size_fraction=max_size_fraction)
        nT = self.max_batch_tiles
        for (shape, net_hw), idxs in groups.items():
            for s in range(0, len(idxs), nT):
                chunk = idxs[s:s + nT]
                tiles = torch.from_numpy(np.stack([np.ascontiguousarray(imgs[i]) for i in chunk])).to(self.device)
                with self._engine(shape[0], shape[1], augment, tile_overlap, kw, net_hw, resample) as eng:     # held for this batch only
                    o = eng.run(tiles, records=False, confidence=bool(cell_confidence))
                    conf = self._confidence_tables(eng, o, len(chunk)) if cell_confidence else None
                    masks = ops.masks_to_numpy(o.masks) if compute_masks else None
                    cm = o.class_masks.cpu().numpy().astype(np.int64) if compute_masks else None
                    dP, cp = o.dP.cpu().numpy(), o.cellprob.cpu().numpy()
                    yc = o.logits.cpu().numpy() if o.logits is not None else None
                for k, i in enumerate(chunk):
                    outs[i] = (masks[k].copy() if compute_masks else np.zeros(0),
                               (dx_to_circ(dP[k]), dP[k].copy(), cp[k].copy(),
                                yc[k].copy() if yc is not None else None,
                                (1, *shape) if net_hw is None else (1, *net_hw, shape[2])),      # x.shape: of the resized image
                               cm[k].copy() if compute_masks else np.zeros(0),
                               np.zeros(256, np.float32))          # styles: noise in the reference (vit_sam.py:197)
                    if cell_confidence:
                        outs[i] = outs[i] + (conf[k],)
        if is_list:
            return tuple([o[j] for o in outs] for j in range(5 if cell_confidence else 4))
        return outs[0]

    @staticmethod
    def _confidence_tables(eng, o, n: int) -> list:
        """per image of a collected batch the ``confidence.stats_table`` of its cells (rows 0 .. nlabels-1 of the device tables)"""
        from . import confidence
        nlab = o.nlabels[:n].cpu().numpy()
        mx = int(nlab.max()) if n else 0
        cq = o.cellprob_q[:n, :mx].cpu().numpy().view(np.uint64)
        if o.votes is not None:
            votes, pq = o.votes[:n, :mx].cpu().numpy(), o.prob_q[:n, :mx].cpu().numpy().view(np.uint64)
        else:
            # no class head: the pixel counts come from the id map the statistics were taken on
            ids = eng._last.masks[:n].to(torch.int32) & 0xFFFF
            area = torch.stack([torch.bincount(ids[t].reshape(-1), minlength=mx + 1)[1:mx + 1] for t in range(n)]).cpu().numpy() if n else None
        tables = []
        for t in range(n):
            k = int(nlab[t])
            label = np.arange(1, k + 1)
            if o.votes is not None:
                v = votes[t, :k].astype(np.int64)
                tables.append(confidence.stats_table(label, v.argmax(1) if k else np.zeros(0, np.int64), v.sum(1), v, pq[t, :k], cq[t, :k]))
            else:
                tables.append(confidence.stats_table(label, np.zeros(k, np.int64), area[t, :k], None, None, cq[t, :k]))
        return tables
