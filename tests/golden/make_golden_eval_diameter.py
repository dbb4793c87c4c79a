"""Mint the ``diameter`` golden vector from the reference's OWN ``ClassposeModel.eval`` (build container only):

* ``ClassposeModel.eval``  /root/reference/src/classpose/models.py:478-827, the branches at 633-639 (image resize by
  30 / diameter), 733-748 (fields back to the image size before the dynamics, ``resample=True``) and 782-820 (fields, ids and
  classes back afterwards)

run under the stub finder of ``make_golden.py`` exactly like ``make_golden_eval.py`` runs the plain path, on the stand-in
network ``make_golden_eval.decode_net``.  What lives in the ABSENT wheels is supplied at the call boundary and stays
"unpinned": ``transforms.resize_image`` and ``CellposeModel._resize_gradients`` / ``_resize_cellprob`` come from
``tests/resize_reference.py`` (OpenCV's linear / nearest resize and cellpose's wrappers, restated), ``normalize_img`` and the
tiling helpers from ``oracle.tiling``, the dynamics from ``oracle.dynamics``.  What the vector PINS is what the reference owns:
``image_scaling = 30.0 / diameter``, the truncated sizes, that the image is resized BEFORE it is normalised, which arrays are
resized when and to what with which interpolation, where the dynamics and the class vote run, and the return structure.

Every ``resize_image`` / ``normalize_img`` / dynamics call is logged in order.  Fixtures hold data only.
    python tests/golden/make_golden_eval_diameter.py
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402
import make_golden_eval as mge  # noqa: E402

SEED, CROP = 31, (200, 232)
ROWS = ((20, True), (45, True), (15, True), (30, True), (45, False))          # (diameter, resample)
CELLS = (60, 60, 60, 60, 56)
FIXTURE = os.path.join(HERE, "reference_eval_diameter.npz")


def diameter_tile() -> np.ndarray:
    return np.ascontiguousarray(mge.eval_tile(SEED)[:CROP[0], :CROP[1]])


def main():
    sys.meta_path.insert(0, mg._Finder())
    sys.path.insert(0, mg.REF)
    import resize_reference as rr
    from oracle import dynamics as odyn
    from oracle import tiling
    from classpose_amd import models as our_models
    import cellpose.transforms as ctf
    ctf.get_pad_yx, ctf.make_tiles = tiling.get_pad_yx, tiling.make_tiles
    ctf.average_tiles, ctf.unaugment_tiles = tiling.average_tiles, tiling.unaugment_tiles
    import cellpose.core as ccore
    ccore.tqdm_out = None
    sys.modules.setdefault("tqdm", types.ModuleType("tqdm")).trange = range
    import classpose.models as rm

    rm.cv2.INTER_NEAREST, rm.cv2.INTER_LINEAR = rr.INTER_NEAREST, rr.INTER_LINEAR
    log = []

    def convert_image(x, channel_axis=None, z_axis=None, do_3D=False):
        return x

    def normalize_img(x, **params):
        log.append(dict(call="normalize_img", shape=list(x.shape), dtype=str(x.dtype)))
        return tiling.normalize_img(x)

    def resize_image(x, Ly=None, Lx=None, rsz=None, interpolation=rr.INTER_LINEAR, no_channels=False):
        log.append(dict(call="resize_image", shape=list(x.shape), dtype=str(x.dtype), Ly=int(Ly), Lx=int(Lx),
                        interpolation={rr.INTER_NEAREST: "nearest", rr.INTER_LINEAR: "linear"}[interpolation],
                        no_channels=bool(no_channels)))
        return rr.resize_image(x, Ly=Ly, Lx=Lx, rsz=rsz, interpolation=interpolation, no_channels=no_channels)

    def resize_and_compute_masks(dP, cellprob, **kw):
        # resize= is [Ly, Lx] when the fields are not at the image size (resample=False, models.py:139); cellpose >= 4.0.1 only
        # warns that resizing there is deprecated and returns the masks at the fields' size -- restated, and recorded here
        log.append(dict(call="resize_and_compute_masks", dP_shape=list(dP.shape), niter=int(kw["niter"]),
                        resize=None if kw.get("resize") is None else [int(v) for v in kw["resize"]]))
        return odyn.compute_masks(np.ascontiguousarray(dP), np.ascontiguousarray(cellprob), niter=kw["niter"],
                                  cellprob_threshold=kw["cellprob_threshold"], flow_threshold=kw["flow_threshold"],
                                  min_size=kw["min_size"], max_size_fraction=kw["max_size_fraction"])

    rm.transforms.convert_image = convert_image
    rm.transforms.normalize_img = normalize_img
    rm.transforms.resize_image = resize_image
    rm.dynamics.resize_and_compute_masks = resize_and_compute_masks
    rm.plot.dx_to_circ = our_models.dx_to_circ
    rm.utils.TqdmToLogger = lambda *a, **k: None
    rm.normalize_default = {"lowhigh": None, "percentile": None, "normalize": True, "norm3D": True, "sharpen_radius": 0,
                            "smooth_radius": 0, "tile_norm_blocksize": 0, "tile_norm_smooth3D": 1, "invert": False}

    class FakeNet(nn.Module):
        def __init__(self, ncls):
            super().__init__()
            self.n_cell_classes, self.device = ncls, torch.device("cpu")
            self.dummy = nn.Parameter(torch.zeros(1))

        def forward(self, X):
            return mge.decode_net(X, self.n_cell_classes), torch.zeros(X.shape[0], 256)

    me = types.SimpleNamespace(net=FakeNet(mge.NCLS), nclasses=mge.NCLS, device=torch.device("cpu"), timing=[])
    for name in ("eval", "_run_net", "_compute_masks"):
        setattr(me, name, types.MethodType(getattr(rm.ClassposeModel, name), me))
    # the two helpers the reference inherits from cellpose.models.CellposeModel (absent): restated in resize_reference
    me._resize_gradients = lambda g, to_y_size=None, to_x_size=None, to_z_size=None: \
        (log.append(dict(call="_resize_gradients", shape=list(g.shape))), resize_via(g, to_y_size, to_x_size, True))[1]
    me._resize_cellprob = lambda p, to_y_size=None, to_x_size=None, to_z_size=None: \
        (log.append(dict(call="_resize_cellprob", shape=list(p.shape))), resize_via(p, to_y_size, to_x_size, False))[1]

    def resize_via(a, Ly, Lx, grads):
        # through the patched transforms.resize_image, so that these calls are logged like the reference's own
        if grads:
            return resize_image(a.transpose(1, 2, 0), Ly=Ly, Lx=Lx, no_channels=False).transpose(2, 0, 1)
        return resize_image(a, Ly=Ly, Lx=Lx, no_channels=True)

    tile = diameter_tile()
    out = {"n": np.array(len(ROWS)), "tilesum": np.array(int(tile.astype(np.int64).sum()))}
    for k, (diam, resample) in enumerate(ROWS):
        log.clear()
        with torch.no_grad():
            masks, flows, class_masks, styles = me.eval([tile], batch_size=8, diameter=diam, resample=resample, bsize=256,
                                                        compute_masks=True)
        m, cm = np.asarray(masks[0]), np.asarray(class_masks[0])
        assert m.shape == CROP and cm.shape == CROP and int(m.max()) == CELLS[k], (diam, resample, m.shape, int(m.max()))
        out[f"{k}_cfg"] = np.array([diam, int(resample)])
        out[f"{k}_masks"] = m.astype(np.uint16)
        out[f"{k}_class_masks"] = cm.astype(np.uint8)
        out[f"{k}_dP"] = np.asarray(flows[0][1])[:, ::4, ::4].astype(np.float32)
        out[f"{k}_cellprob"] = np.asarray(flows[0][2])[::4, ::4].astype(np.float32)
        out[f"{k}_yclass"] = np.asarray(flows[0][3])[:, ::4, ::4].astype(np.float32)
        out[f"{k}_shape_x"] = np.array(flows[0][4])
        out[f"{k}_log"] = np.array(json.dumps(log))
        print(k, diam, resample, "cells:", int(m.max()), "x.shape:", tuple(flows[0][4]))
        for e in log:
            print("   ", json.dumps(e))
    np.savez_compressed(FIXTURE, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(FIXTURE) // 1024, "KiB")


if __name__ == "__main__":
    main()
