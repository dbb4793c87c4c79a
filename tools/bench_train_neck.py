"""The price of training the neck next to the two heads.  One process, interleaved rounds, medians (the set-up of
tools/bench_train_flow.py).

    python tools/bench_train_neck.py [--rounds 9] [--crops 32] [--out profiles/train_neck_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_neck.py --profile-steps 5      (kernels of the cached step only)

Workload: `--crops` uint8 crops of 256^2 of the synthetic slide with blocky class maps and a jittered grid of disc instances, a seeded
ViT-L checkpoint with a fresh 7-class 1x1 head, bf16.
  (h)  HeadTrainer.step from cached neck features, both heads, no train_neck: the cached step as it was before this feature
  (n)  HeadTrainer(train_neck=True).step from cached backbone rows: the neck's training forward, three losses, cpx_neck_backward, both
       heads' updates, the neck's AdamW step and refresh
  (ph) HeadTrainer.step from pixels, both heads, no train_neck: the step of the parent commit (a trainer built without the flag
       runs its code) -- the baseline of (pn)
  (pn) the same from pixels with train_neck: cpx_net_forward, then the training tail once more on its x, then (n)
  (e)  the step of (n) in eager PyTorch with autograd on the same GPU, from the same cached rows: bf16 linear / LayerNorm / 3x3 conv /
       linear on bf16 casts of float32 masters, float32 losses, torch.optim.AdamW on the masters
Every round times all five, the order reversed in odd rounds.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from classpose_amd import augment, synth
from classpose_amd.train import HeadTrainer


def make_labels(n, size, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.kron(rng.integers(0, ncls, (n, size // 8, size // 8)), np.ones((1, 8, 8), np.int64)).astype(np.int16)
    for b in range(n):
        y0 = int(rng.integers(0, size - 56))
        lab[b, y0:y0 + 20] = -100
    return lab


def make_instances(size, seed, pitch=40):
    """(size, size) int32: one disc of radius 8..14 per cell of a `pitch` grid, its centre jittered inside the cell."""
    rng = np.random.default_rng(seed)
    m = np.zeros((size, size), np.int32)
    yy, xx = np.mgrid[:pitch, :pitch]
    k = 0
    for gy in range(size // pitch):
        for gx in range(size // pitch):
            r = int(rng.integers(8, 15))
            cy, cx = (int(v) for v in rng.integers(r + 1, pitch - r - 1, 2)) if pitch - r - 1 > r + 1 else (pitch // 2, pitch // 2)
            k += 1
            cell = m[gy * pitch:(gy + 1) * pitch, gx * pitch:(gx + 1) * pitch]
            cell[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
    return m


def tokens_to_nchw(x, ch, n):
    return x.view(n, 32, 32, ch, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(n, ch, 256, 256)


class EagerStep:
    """The neck and both 1x1 heads in eager PyTorch: autograd + torch.optim.AdamW, the losses of the reference restated on device
    tensors."""

    def __init__(self, tr, ncls):
        self.ncls = ncls
        sd, dev = tr.sd, tr.device
        par = lambda t: torch.nn.Parameter(t.detach().float().clone().to(dev))
        self.W0 = par(sd["encoder.neck.0.weight"].reshape(256, 1024))
        self.g1, self.b1 = par(sd["encoder.neck.1.weight"]), par(sd["encoder.neck.1.bias"])
        self.W2 = par(sd["encoder.neck.2.weight"])
        self.g2, self.b2 = par(sd["encoder.neck.3.weight"]), par(sd["encoder.neck.3.bias"])
        self.W = par(torch.cat([sd["out.weight"].reshape(192, 256), tr.w.cpu()]))
        self.b = par(torch.cat([sd["out.bias"].float(), tr.b.cpu()]))
        self.params = [self.W0, self.g1, self.b1, self.W2, self.g2, self.b2, self.W, self.b]
        self.opt = torch.optim.AdamW(self.params, lr=1e-4, weight_decay=tr.weight_decay)

    def __call__(self, x, labels, tg, lr):
        n, bf = labels.shape[0], torch.bfloat16
        for g in self.opt.param_groups:
            g["lr"] = lr
        self.opt.zero_grad(set_to_none=True)
        y0 = x @ self.W0.to(bf).T
        a1 = F.layer_norm(y0, (256,), self.g1.to(bf), self.b1.to(bf), 1e-6)
        y2 = F.conv2d(a1.view(n, 32, 32, 256).permute(0, 3, 1, 2), self.W2.to(bf), padding=1).permute(0, 2, 3, 1).reshape(-1, 256)
        feat = F.layer_norm(y2, (256,), self.g2.to(bf), self.b2.to(bf), 1e-6)
        y = (feat @ self.W.to(bf).T).float() + self.b.to(bf).float()
        z = tokens_to_nchw(y[:, :192], 3, n)
        logits = tokens_to_nchw(y[:, 192:192 + self.ncls * 64], self.ncls, n)
        seg = F.mse_loss(z[:, :2], 5.0 * tg[:, 1:]) / 2 + F.binary_cross_entropy_with_logits(z[:, 2], (tg[:, 0] > 0.5).float())
        lab = labels.long()
        ce = F.cross_entropy(logits, lab, ignore_index=-100)
        valid = (lab != -100)
        p = torch.softmax(logits, 1) * valid[:, None]
        onehot = F.one_hot(lab.clamp_min(0), self.ncls).permute(0, 3, 1, 2) * valid[:, None]
        tp, fp, fn = (p * onehot).sum((2, 3)), (p * (1 - onehot) * valid[:, None]).sum((2, 3)), ((1 - p) * onehot).sum((2, 3))
        tv = ((1 - tp / (tp + 0.3 * fp + 0.7 * fn)).clamp(1e-6, 1 - 1e-6) ** (1 / 1.33)).mean()
        loss = seg + ce + tv
        loss.backward()
        self.opt.step()
        return float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many cached train_neck steps and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, ncls = args.crops, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    ims = np.stack([synth.render_region(300, 256 * (k % 8), 256 * (k // 8), 256, 256) for k in range(n)])
    labs = make_labels(n, 256, ncls, 7 + ncls)
    tg = torch.stack(augment.flow_targets_of([make_instances(256, 90 + k) for k in range(n)], dev)).contiguous()
    lr = 1e-4
    trn = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n, train_flow_head=True, train_neck=True)
    rows = trn.backbone_features(ims)
    if args.profile_steps:
        for _ in range(args.profile_steps):
            trn.step(rows, labs, lr, flow_targets=tg)
        torch.cuda.synchronize()
        return
    trh = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n, train_flow_head=True)
    feat = trh.features(ims)
    eager = EagerStep(trn, ncls)
    ev = trn.evaluate(rows, labs, flow_targets=tg)
    fns = {"h": lambda: trh.step(feat, labs, lr, flow_targets=tg)["loss"], "n": lambda: trn.step(rows, labs, lr, flow_targets=tg)["loss"],
           "ph": lambda: trh.step(ims, labs, lr, flow_targets=tg)["loss"], "pn": lambda: trn.step(ims, labs, lr, flow_targets=tg)["loss"],
           "e": lambda: eager(rows, torch.from_numpy(labs).to(dev), tg, lr)}
    first = {k: f() for k, f in fns.items()}
    # (the eager forward rounds where torch's bf16 kernels round, not where the device does: loose agreement only)
    assert abs(first["e"] - ev["loss"]) <= 2e-2 * abs(ev["loss"]), (first, ev)
    for f in fns.values():
        for _ in range(2):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for rnd in range(args.rounds):
        for k in (list(fns) if rnd % 2 == 0 else list(fns)[::-1]):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fns[k]()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"bench_train_neck: {torch.cuda.get_device_name(0)}, {n} crops of 256^2 per step, bf16, {ncls} classes, ViT depth {args.depth}, "
             f"{args.rounds} interleaved rounds (order reversed in odd rounds), warmed up, host wall clock around a synchronised step, "
             f"medians (ms); first losses {({k: round(v, 4) for k, v in first.items()})}"]
    for k, what in (("h", "step from cached neck features, both heads (the cached step before this feature)"),
                    ("n", "step from cached backbone rows, neck + both heads                              "),
                    ("ph", "step from pixels, both heads (the step of the parent commit)                   "),
                    ("pn", "step from pixels, neck + both heads                                            "),
                    ("e", "eager PyTorch + autograd, neck + both heads, cached backbone rows              ")):
        lines.append(f"  ({k:2s}) {what} median {med[k]:9.3f}   min {min(times[k]):9.3f} max {max(times[k]):9.3f}   {[round(v, 3) for v in times[k]]}")
    lines.append(f"  (n) - (h) = {med['n'] - med['h']:.3f} ms; (pn) - (ph) = {med['pn'] - med['ph']:.3f} ms ({100 * (med['pn'] - med['ph']) / med['ph']:.1f} % of (ph))")
    verdict = "the device step is FASTER than eager PyTorch" if max(times["n"]) < min(times["e"]) else \
        ("the device step LOSES to eager PyTorch" if min(times["n"]) > max(times["e"]) else "the device step and eager PyTorch overlap: no call")
    lines.append(f"  (e) / (n) = {med['e'] / med['n']:.2f}: {verdict} (every round of one below every round of the other, or no call)")
    lines.append(f"  cache per crop: {rows.numel() * rows.element_size() // n // 1024} KiB of backbone rows against "
                 f"{feat.numel() * feat.element_size() // n // 1024} KiB of neck features")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
