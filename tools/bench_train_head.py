"""Training the 1x1 class head: what a step costs next to the frozen forward, and next to the same head step in eager PyTorch.
One process, interleaved rounds, medians (the style of tools/bench_pq.py).

    python tools/bench_train_head.py [--rounds 9] [--crops 32] [--out profiles/train_head_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_head.py --depth 1 --profile-steps 5      (kernels only)

Workload: `--crops` random float32 crops of 256^2 (the backbone's time does not depend on the pixels), blocky random class maps with a
band and 2 % scattered pixels without annotation, a seeded ViT-L checkpoint with a fresh 7- / 10-class head, bf16.
  (f) cpx_net_forward alone on the crops' patch rows: the baseline -- inference already pays it
  (a) HeadTrainer.step from pixels: patchify, forward, head GEMM, loss + gradient, weight gradient, AdamW, operand refresh, and the
      two loss scalars on the host
  (b) HeadTrainer.step from cached neck features: everything of (a) behind the backbone
  (c) the head step of (b) in eager PyTorch-ROCm from the same cached features: float32 linear on the widened features, pixel
      shuffle by permute, nn.functional.cross_entropy(ignore_index=-100), the focal Tversky loss, autograd, torch.optim.AdamW
Every round times all four, the order reversed in odd rounds.  The eager losses are compared with the device's before anything is timed.
"""
import argparse
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from classpose_amd import _lib, synth
from classpose_amd.train import HeadTrainer


def make_labels(n, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.kron(rng.integers(0, ncls, (n, 32, 32)), np.ones((1, 8, 8), np.int64)).astype(np.int16)
    for b in range(n):
        y0 = int(rng.integers(0, 200))
        lab[b, y0:y0 + 20] = -100
        lab[b][rng.random((256, 256)) < 0.02] = -100
    return lab


class EagerHead:
    """The head step as one would write it without kernels: float32 master weights, autograd, torch.optim.AdamW."""

    def __init__(self, trainer):
        self.ncls = trainer.nclasses
        self.W = torch.nn.Parameter(trainer.w.clone())
        self.b = torch.nn.Parameter(trainer.b.clone())
        self.opt = torch.optim.AdamW([self.W, self.b], lr=1e-3, weight_decay=trainer.weight_decay)
        self.alpha, self.gamma, self.eps = trainer.alpha, trainer.gamma, trainer.eps

    def losses(self, feat, labels):
        n = labels.shape[0]
        Wr, br = self.W.to(feat.dtype).float(), self.b.to(feat.dtype).float()          # operands rounded like the engine's (differentiable)
        z = torch.nn.functional.linear(feat.float(), Wr, br)
        z = z.view(n, 32, 32, self.ncls, 8, 8).permute(0, 3, 1, 4, 2, 5).reshape(n, self.ncls, 256, 256)
        lbl = labels.long()
        ce = torch.nn.functional.cross_entropy(z, lbl, ignore_index=-100)
        valid = (lbl != -100).float()[:, None]
        oh = torch.nn.functional.one_hot(lbl.clamp_min(0), self.ncls).permute(0, 3, 1, 2)
        p = torch.softmax(z, 1)
        tp = (p * oh * valid).sum((2, 3)); fp = (p * (1 - oh) * valid).sum((2, 3)); fn = ((1 - p) * oh * valid).sum((2, 3))
        tv = torch.clip(1 - tp / (tp + self.alpha * fp + (1 - self.alpha) * fn), self.eps, 1 - self.eps).pow(1 / self.gamma).mean()
        return ce, tv

    def step(self, feat, labels, lr):
        for g in self.opt.param_groups:
            g["lr"] = lr
        ce, tv = self.losses(feat, labels)
        self.opt.zero_grad(set_to_none=True)
        (ce + tv).backward()
        self.opt.step()
        return float(ce.item()), float(tv.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, nargs="+", default=[7, 10])
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many cached steps per class count and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.crops
    lines = [f"bench_train_head: {torch.cuda.get_device_name(0)}, {n} crops of 256^2, bf16, ViT depth {args.depth}, "
             f"{args.rounds} interleaved rounds, warmed up, medians (ms)"]
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    X = torch.randn(n, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(dev)
    lr = 1e-4
    for ncls in args.classes:
        tr = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n)
        lab = torch.from_numpy(make_labels(n, ncls, 7 + ncls)).to(dev)
        feat = tr.features(X)
        if args.profile_steps:
            for _ in range(args.profile_steps):
                tr.step(feat, lab, lr)
            torch.cuda.synchronize()
            continue
        eager = EagerHead(tr)
        ev = tr.evaluate(feat, lab)
        with torch.no_grad():
            ce, tv = eager.losses(feat, lab)
        assert abs(ev["ce"] - float(ce)) <= 1e-4 * abs(ev["ce"]) and abs(ev["tversky"] - float(tv)) <= 1e-4 * abs(ev["tversky"]), \
            (ev, float(ce), float(tv))
        patches = tr._patches(X)
        L, c = _lib.lib(), tr.weights.c
        st = torch.cuda.current_stream(dev).cuda_stream

        def forward():
            _lib.check(L.cpx_net_forward(C.byref(c), _lib.ptr(patches), n, _lib.ptr(tr._head_fb), _lib.ptr(tr._net_ws),
                                         tr._net_ws.numel(), st), "net_forward")
        fns = {"f": forward, "a": lambda: tr.step(X, lab, lr), "b": lambda: tr.step(feat, lab, lr), "c": lambda: eager.step(feat, lab, lr)}
        for f in fns.values():              # warm-up: allocations, code objects, autograd's workspace
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
        lines.append(f"{ncls} classes ({ncls * 64} head columns), {n * 1024} token rows:")
        for k, what in (("f", "cpx_net_forward alone          "), ("a", "full step from pixels          "),
                        ("b", "step from cached features      "), ("c", "eager PyTorch head step (cached)")):
            lines.append(f"  ({k}) {what} median {med[k]:8.3f}   {[round(x, 3) for x in times[k]]}")
        lines.append(f"  price of training over the forward (a) - (f) = {med['a'] - med['f']:.3f} ms = {100 * (med['a'] - med['f']) / med['f']:.1f} % of the forward; "
                     f"cached step / eager head step (b)/(c) = {med['b'] / med['c']:.3f}; an epoch over cached features costs "
                     f"{100 * med['b'] / med['a']:.1f} % of one from pixels")
        del tr, eager, feat, patches
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
