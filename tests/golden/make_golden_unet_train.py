"""Mint the UNet-head training fixture from the REFERENCE's own modules (run in the build container only).

    python tests/golden/make_golden_unet_train.py      # rewrites tests/golden/reference_unet_train.npz

``classpose.unet`` imports only torch; ``classpose.train`` is imported under the stub finder of make_golden.py.  Called, all in
float64 on the CPU: ``UNet(256, ncls * 64, fts)`` (its ``state_dict`` gives the key order and the shapes), the pixel shuffle ``conv_transpose2d(., W3 = identity, stride 8)`` of the class head, ``_loss_fn_class``,
``_loss_fn_tversky`` and ``LossAggregator(n_losses=2, optimise=False)``, with autograd down to every UNet parameter.
fts = [12, 20], 2 classes, one case of 1 crop and one of 2 crops (with class weights), labels with -100 regions.  The logits
gradient is 2 x 2 x 256 x 256 float64, so it is stored as a fixed strided sample plus its sum and absolute sum; a parameter
gradient of more than 2048 elements likewise (stride 23); the neck features and the parameters are formulas of the element index
(tests/unet_train_reference.py) and not stored.  The fixture holds data only.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("TQDM_DISABLE", "1")

FTS, NCLS, STRIDE, GSTRIDE = [12, 20], 2, 97, 23


def main():
    import torch
    import make_golden
    from make_golden_train import make_labels
    from unet_train_reference import make_feat, make_params
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REF)
    from classpose import train as rtrain
    from classpose.unet import UNet

    rng = np.random.default_rng(20261018)
    arrays = {}
    net = UNet(256, NCLS * 64, FTS).double()
    sd = net.state_dict()
    arrays["keys"] = np.array(list(sd.keys()))
    arrays["shapes"] = np.array([" ".join(map(str, v.shape)) for v in sd.values()])
    arrays["fts"], arrays["ncls"], arrays["stride"], arrays["gstride"] = np.array(FTS), np.array(NCLS), np.array(STRIDE), np.array(GSTRIDE)
    # the parameters are a formula too (tests/unet_train_reference.make_params, float32 values at the default initialisation's scale)
    net.load_state_dict({k.removeprefix("out_class."): v.double() for k, v in make_params(FTS, NCLS, 1).items()}, strict=True)
    W3 = torch.eye(NCLS * 64, dtype=torch.float64).reshape(NCLS * 64, NCLS, 8, 8)
    agg = rtrain.LossAggregator(n_losses=2, optimise=False).double()
    for name, nI, weights in (("b1", 1, False), ("b2w", 2, True)):
        feat = make_feat(nI, nI).numpy()             # a formula of the element index (tests/unet_train_reference.py): not stored
        lab = make_labels(rng, nI, 256, 256, NCLS)
        cw = rng.uniform(0.5, 2.0, NCLS) if weights else None
        net.zero_grad(set_to_none=True)
        y_cls = torch.nn.functional.conv_transpose2d(net(torch.from_numpy(feat)), W3, stride=8)
        y_cls.retain_grad()
        y = torch.cat([y_cls, torch.zeros(nI, 3, 256, 256, dtype=torch.float64)], 1)
        lbl = torch.from_numpy(lab.astype(np.float64))[:, None]
        cwt = None if cw is None else torch.from_numpy(cw).double()
        ce = rtrain._loss_fn_class(lbl.clone(), y, class_weights=cwt)
        tv = rtrain._loss_fn_tversky(lbl.clone(), y, n_classes=NCLS, class_weights=cwt)
        loss = agg(ce, tv)
        loss.backward()
        arrays[name + "_feat_sums"], arrays[name + "_labels"] = np.array([feat.sum(), np.abs(feat).sum()]), lab
        if cw is not None:
            arrays[name + "_weights"] = cw
        arrays[name + "_losses"] = np.array([float(ce), float(tv), float(loss)])
        z, dz = y_cls.detach().numpy().reshape(-1), y_cls.grad.numpy().reshape(-1)
        arrays[name + "_logits_sample"], arrays[name + "_logits_sums"] = z[::STRIDE], np.array([z.sum(), np.abs(z).sum()])
        arrays[name + "_dlogits_sample"], arrays[name + "_dlogits_sums"] = dz[::STRIDE], np.array([dz.sum(), np.abs(dz).sum()])
        for k, prm in net.named_parameters():
            g = prm.grad.numpy().reshape(-1)
            arrays[f"{name}_g:{k}"] = g.copy() if g.size <= 2048 else g[::GSTRIDE].copy()
            arrays[f"{name}_gs:{k}"] = np.array([g.sum(), np.abs(g).sum()])
        print(name, float(ce), float(tv), float(loss))
    out = os.path.join(HERE, "reference_unet_train.npz")
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
