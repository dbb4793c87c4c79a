"""Training the UNet class head: what a step costs next to the frozen forward, and next to the same head step in eager PyTorch.
One process, interleaved rounds, medians (the style of tools/bench_train_head.py).

    python tools/bench_train_unet.py [--rounds 9] [--crops 32] [--out profiles/train_unet_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_unet.py --depth 1 --profile-steps 5      (kernels only)

Workload: `--crops` random float32 crops of 256^2, blocky random class maps with a band and 2 % scattered pixels without annotation,
a seeded ViT-L checkpoint with a fresh 7-class UNet head of channels [64, 128] and [64, 128, 256, 512], bf16.
  (f) cpx_net_forward alone on the crops' patch rows (it includes the UNet head's forward): the baseline -- inference already pays it
  (a) UNetHeadTrainer.step from pixels: patchify, forward, head GEMM + UNet forward, loss + gradient, backward, AdamW, operand
      refresh, and the two loss scalars on the host
  (b) UNetHeadTrainer.step from cached neck features: everything of (a) behind the backbone
  (c) the head step of (b) in eager PyTorch-ROCm from the same cached features: unet.UNet restated with torch.nn.functional convolutions
      in the network dtype (bf16 parameters cast from float32 masters, so autograd returns float32 gradients), pixel shuffle by
      permute, float32 losses, autograd, torch.optim.AdamW on the float32 masters
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
import torch.nn.functional as F

from classpose_amd import _lib, synth, train_unet


def make_labels(n, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.kron(rng.integers(0, ncls, (n, 32, 32)), np.ones((1, 8, 8), np.int64)).astype(np.int16)
    for b in range(n):
        y0 = int(rng.integers(0, 200))
        lab[b, y0:y0 + 20] = -100
        lab[b][rng.random((256, 256)) < 0.02] = -100
    return lab


class EagerUNetHead:
    """The head step as one would write it without kernels: float32 master parameters, forward in the network dtype, autograd,
    torch.optim.AdamW."""

    def __init__(self, trainer):
        self.ncls, self.fts, self.dtype = trainer.nclasses, trainer.fts, trainer.dtype
        sd = train_unet.unpack_params(trainer.params, self.fts, self.ncls * 64)
        self.p = {k: torch.nn.Parameter(v.to(trainer.device)) for k, v in sd.items()}
        self.opt = torch.optim.AdamW(list(self.p.values()), lr=1e-3, weight_decay=trainer.weight_decay)
        self.alpha, self.gamma, self.eps = trainer.alpha, trainer.gamma, trainer.eps

    def forward(self, x):
        dt = self.dtype

        def conv(key, t, act, kind):
            w, b = self.p["out_class." + key + ".weight"].to(dt), self.p["out_class." + key + ".bias"].to(dt)
            y = F.conv2d(t, w, b, padding=1) if kind == 0 else F.conv2d(t, w, b, stride=2) if kind == 1 else F.conv_transpose2d(t, w, b, stride=2)
            return torch.relu(y) if act else y

        def block(pfx, t, skip_last=False):
            return conv(pfx + "block.conv2", conv(pfx + "block.conv1", t, True, 0), not skip_last, 0)

        n_lv, feats = len(self.fts), []
        for n in range(n_lv):
            x = conv(f"encoder_blocks.{n}.downconv", block(f"encoder_blocks.{n}.", x), False, 1)
            feats.append(x)
        feats = feats[::-1]
        x = conv("bottleneck_down.downconv", block("bottleneck_down.", x), False, 1)
        x = conv("bottleneck_up.upconv", block("bottleneck_up.", x), False, 2)
        for i in range(n_lv):
            x = block(f"decoder_blocks.{i}.", torch.cat((x, feats[i]), 1), skip_last=i == n_lv - 1)
            x = conv(f"decoder_blocks.{i}.upconv", x, False, 2)
        return x

    def losses(self, feat, labels):
        n = labels.shape[0]
        x = feat.view(n, 32, 32, 256).permute(0, 3, 1, 2)
        y = self.forward(x).float()
        z = y.view(n, self.ncls, 8, 8, 32, 32).permute(0, 1, 4, 2, 5, 3).reshape(n, self.ncls, 256, 256)
        lbl = labels.long()
        ce = F.cross_entropy(z, lbl, ignore_index=-100)
        valid = (lbl != -100).float()[:, None]
        oh = F.one_hot(lbl.clamp_min(0), self.ncls).permute(0, 3, 1, 2)
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
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--structures", default="64,128;64,128,256,512", help="channel lists separated by ';'")
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many cached steps per structure and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, ncls = args.crops, args.classes
    lines = [f"bench_train_unet: {torch.cuda.get_device_name(0)}, {n} crops of 256^2, {ncls} classes, bf16, ViT depth {args.depth}, "
             f"{args.rounds} interleaved rounds, warmed up, medians (ms)"]
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    X = torch.randn(n, 3, 256, 256, generator=torch.Generator().manual_seed(1)).to(dev)
    lr = 1e-4
    for fts in ([int(c) for c in s.split(",")] for s in args.structures.split(";")):
        tr = train_unet.UNetHeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n,
                                        feature_transformation_structure=fts)
        lab = torch.from_numpy(make_labels(n, ncls, 7 + ncls)).to(dev)
        feat = tr.features(X)
        print(f"UNet {fts}: features cached", flush=True)
        if args.profile_steps:
            for _ in range(args.profile_steps):
                tr.step(feat, lab, lr)
            torch.cuda.synchronize()
            continue
        eager = EagerUNetHead(tr)
        ev = tr.evaluate(feat, lab)
        with torch.no_grad():
            ce, tv = eager.losses(feat, lab)
        # (the eager forward rounds where torch's bf16 convolutions round, not where the device does: loose agreement only)
        assert abs(ev["ce"] - float(ce)) <= 2e-2 * abs(ev["ce"]) and abs(ev["tversky"] - float(tv)) <= 2e-2 * abs(ev["tversky"]), \
            (ev, float(ce), float(tv))
        patches = tr._patches(X)
        L, c = _lib.lib(), tr.weights.c
        st = torch.cuda.current_stream(dev).cuda_stream

        def forward():
            _lib.check(L.cpx_net_forward(C.byref(c), _lib.ptr(patches), n, _lib.ptr(tr._head_fb), _lib.ptr(tr._net_ws),
                                         tr._net_ws.numel(), st), "net_forward")
        fns = {"f": forward, "a": lambda: tr.step(X, lab, lr), "b": lambda: tr.step(feat, lab, lr), "c": lambda: eager.step(feat, lab, lr)}
        for f in fns.values():              # warm-up: allocations, code objects, autograd's workspace, MIOpen's kernel search
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        print(f"UNet {fts}: warmed up", flush=True)
        times = {k: [] for k in fns}
        for rnd in range(args.rounds):
            for k in (list(fns) if rnd % 2 == 0 else list(fns)[::-1]):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                fns[k]()
                torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: float(np.median(v)) for k, v in times.items()}
        below = sum(b < c_ for b, c_ in zip(times["b"], times["c"]))
        lines.append(f"UNet {fts}, {tr.params.numel()} packed parameters, {n * 1024} token rows, device losses ce {ev['ce']:.4f} tversky {ev['tversky']:.4f} "
                     f"(eager {float(ce):.4f} {float(tv):.4f}):")
        for k, what in (("f", "cpx_net_forward alone          "), ("a", "full step from pixels          "),
                        ("b", "step from cached features      "), ("c", "eager PyTorch head step (cached)")):
            lines.append(f"  ({k}) {what} median {med[k]:8.3f}   {[round(x, 3) for x in times[k]]}")
        lines.append(f"  price of training over the forward (a) - (f) = {med['a'] - med['f']:.3f} ms = {100 * (med['a'] - med['f']) / med['f']:.1f} % of the forward; "
                     f"cached step / eager head step (b)/(c) = {med['b'] / med['c']:.3f}, device below eager in {below} of {args.rounds} rounds")
        del tr, eager, feat, patches
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
