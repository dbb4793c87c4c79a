"""Mint the head-training fixture from the REFERENCE's own functions (run in the build container only).

    python tests/golden/make_golden_train.py      # rewrites tests/golden/reference_train.npz / .json

``classpose.train`` is imported under the stub finder of make_golden.py.  Called, all in float64 on the CPU:
``_loss_fn_class``, ``_loss_fn_tversky`` and ``LossAggregator(n_losses=2, optimise=False)`` with autograd for d loss / d logits;
``torch.optim.AdamW`` for a 10-step trajectory; the learning-rate array is produced by executing the schedule statements of
``train_class_seg`` (located with ``inspect`` at mint time: the reference computes it inline).  The fixture holds data only.
"""
from __future__ import annotations

import inspect
import json
import os
import sys
import textwrap

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
os.environ.setdefault("TQDM_DISABLE", "1")


def make_labels(rng, nI, H, W, ncls, absent=None, all_zero=None):
    """Blocky class maps with -100 regions: image ``absent[0]`` never shows class ``absent[1]``; image ``all_zero`` is class 0 everywhere."""
    lab = np.zeros((nI, H, W), np.int16)
    for b in range(nI):
        coarse = rng.integers(0, ncls, (H // 8, W // 8))
        if absent is not None and b == absent[0]:
            coarse[coarse == absent[1]] = (absent[1] + 1) % ncls
        else:                                         # every class present otherwise (no accidental absences)
            coarse.reshape(-1)[rng.permutation(coarse.size)[:ncls]] = np.arange(ncls)
        lab[b] = np.kron(coarse, np.ones((8, 8), np.int64))
        # sparse not-annotated regions: a band, a box and scattered pixels
        lab[b, rng.integers(0, H - 6):, :][:5] = -100
        y0, x0 = rng.integers(0, H - 12), rng.integers(0, W - 12)
        lab[b, y0:y0 + 11, x0:x0 + 9] = -100
        lab[b][rng.random((H, W)) < 0.03] = -100
    if all_zero is not None:
        lab[all_zero] = 0
    return lab


def main():
    import torch
    import make_golden
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REF)
    from classpose import train as rtrain

    rng = np.random.default_rng(20261017)
    arrays, meta = {}, {"cases": [], "lr": [], "adamw": {}}
    specs = [
        dict(name="c7", nI=2, ncls=7, weights=False, absent=None, all_zero=None),
        dict(name="c7w", nI=3, ncls=7, weights=True, absent=(1, 4), all_zero=None),
        dict(name="c10", nI=3, ncls=10, weights=False, absent=(0, 7), all_zero=2),
        dict(name="c10w", nI=3, ncls=10, weights=True, absent=(2, 1), all_zero=0),
    ]
    H = W = 32           # (the whole fixture stays under the 1 MiB limit for a committed file; float64 gradients do not compress)
    agg = rtrain.LossAggregator(n_losses=2, optimise=False).double()
    for s in specs:
        lab = make_labels(rng, s["nI"], H, W, s["ncls"], s["absent"], s["all_zero"])
        onehot = np.eye(s["ncls"])[np.where(lab < 0, 0, lab)].transpose(0, 3, 1, 2)
        logits = rng.standard_normal((s["nI"], s["ncls"], H, W)) * 1.5 + 2.0 * onehot * (rng.random((s["nI"], 1, H, W)) < 0.7)
        logits = np.round(logits * 256) / 256           # exactly representable in float32 (and stored as such)
        cw = rng.uniform(0.5, 2.0, s["ncls"]) if s["weights"] else None
        # what the reference's network returns: class logits first, then the 3 flow / cell-probability channels
        y = torch.from_numpy(np.concatenate([logits, np.zeros((s["nI"], 3, H, W))], 1)).double().requires_grad_(True)
        lbl = torch.from_numpy(lab.astype(np.float64))[:, None]
        cwt = None if cw is None else torch.from_numpy(cw).double()
        ce = rtrain._loss_fn_class(lbl.clone(), y, class_weights=cwt)
        tv = rtrain._loss_fn_tversky(lbl.clone(), y, n_classes=s["ncls"], class_weights=cwt)
        loss = agg(ce, tv)
        loss.backward()
        g = y.grad[:, :-3].numpy()
        assert np.all(y.grad[:, -3:].numpy() == 0)
        # raw Tversky losses, for the note on clip-edge distance (recomputed from the reference's formula on its softmax)
        p = torch.softmax(y[:, :-3].detach(), 1).numpy()
        valid = (lab != -100)[:, None]
        oh = onehot
        tp = (p * oh * valid).sum((2, 3)); fp = (p * (1 - oh) * valid).sum((2, 3)); fn = ((1 - p) * oh * valid).sum((2, 3))
        raw = 1 - tp / (tp + 0.3 * fp + 0.7 * fn)
        present = (oh * valid).sum((2, 3)) > 0
        edge = float(np.minimum(raw[present], 1 - raw[present]).min())
        assert edge >= 0.1, (s["name"], edge)
        assert np.all(raw[~present] == 1.0)
        n = s["name"]
        arrays[n + "_logits"], arrays[n + "_labels"], arrays[n + "_dlogits"] = logits.astype(np.float32), lab, g
        if cw is not None:
            arrays[n + "_weights"] = cw
        meta["cases"].append(dict(name=n, nI=s["nI"], ncls=s["ncls"], H=H, W=W, weights=s["weights"], absent=s["absent"],
                                  all_zero=s["all_zero"], ce=float(ce), tversky=float(tv), loss=float(loss),
                                  min_clip_edge_distance=edge, n_absent=int((~present).sum())))
        print(n, float(ce), float(tv), "edge", edge, "absent", int((~present).sum()))

    # an image without any annotated pixel: the reference returns NaN (documented difference: the engine raises ValueError)
    y = torch.randn(2, 7 + 3, 16, 16, dtype=torch.float64)
    lbl = torch.zeros(2, 1, 16, 16, dtype=torch.float64); lbl[1] = -100
    meta["all_ignored_image_tversky_is_nan"] = bool(torch.isnan(rtrain._loss_fn_tversky(lbl.clone(), y, n_classes=7)))
    lbl[:] = -100
    meta["all_ignored_batch_ce_is_nan"] = bool(torch.isnan(rtrain._loss_fn_class(lbl.clone(), y)))

    # learning-rate schedule: the statements of train_class_seg between "LR = np.linspace" and the next logger call
    src = inspect.getsource(rtrain.train_class_seg).splitlines()
    i0 = next(i for i, l in enumerate(src) if l.strip().startswith("LR = np.linspace"))
    i1 = next(i for i in range(i0, len(src)) if src[i].strip().startswith("train_logger.info"))
    block = textwrap.dedent("\n".join(src[i0:i1]))
    for n_epochs in (5, 20, 100, 400):
        env = {"np": np, "learning_rate": 5e-5, "n_epochs": n_epochs}
        exec(block, env)
        arrays[f"lr_{n_epochs}"] = np.asarray(env["LR"], np.float64)
        meta["lr"].append(dict(n_epochs=n_epochs, learning_rate=5e-5, n=int(len(env["LR"]))))

    # AdamW trajectory
    p0 = rng.standard_normal(48)
    grads = rng.standard_normal((10, 48)) * np.logspace(-3, 0, 48)[None]
    lrs = np.array([0.0, 1e-3, 2e-3, 3e-3, 3e-3, 3e-3, 1.5e-3, 1.5e-3, 1e-4, 1e-4])
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).double())
    opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=0.1)
    traj = []
    for g, lr in zip(grads, lrs):
        for grp in opt.param_groups:
            grp["lr"] = float(lr)
        opt.zero_grad(set_to_none=True)
        p.grad = torch.from_numpy(g.copy()).double()
        opt.step()
        traj.append(p.detach().numpy().copy())
    arrays["adamw_p0"], arrays["adamw_grads"], arrays["adamw_lrs"], arrays["adamw_traj"] = p0, grads, lrs, np.stack(traj)
    meta["adamw"] = dict(weight_decay=0.1, betas=[0.9, 0.999], eps=1e-8, steps=10)

    np.savez_compressed(os.path.join(HERE, "reference_train.npz"), **arrays)
    with open(os.path.join(HERE, "reference_train.json"), "w") as f:
        json.dump(meta, f)
    print("wrote reference_train.npz", os.path.getsize(os.path.join(HERE, "reference_train.npz")), "bytes")


if __name__ == "__main__":
    main()
