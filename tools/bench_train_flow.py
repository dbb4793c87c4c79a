"""The price of training the flow head next to the class head.  One process, interleaved rounds, medians (the set-up of
tools/bench_train_quality.py).

    python tools/bench_train_flow.py [--rounds 9] [--crops 32] [--out profiles/train_flow_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_flow.py --depth 1 --profile-steps 5      (kernels only)

Workload: `--images` uint8 images of 1024^2 of the synthetic slide with blocky class maps and a jittered grid of disc instances,
`--crops` windows of 256^2 per step, a seeded ViT-L checkpoint with a fresh 7-class 1x1 head, bf16.
  (c)  HeadTrainer.step from cached neck features, class head only: the step as it was before this feature (a trainer built
       without train_flow_head runs the code of the parent commit) -- the baseline of (f)
  (f)  the same step with flow_targets: + cpx_seg_loss, cpx_head_wgrad over 192 columns, two cpx_adamw_step, two cpx_round_weights
  (pc) augment.augment_batch_pool(config="geometry") from an ImagePool + the class-only step: the baseline of (pf)
  (pf) the same with flow_targets=True (+ cpx_warp_affine_pool_flow_f32) and both heads
  (e)  the same three-loss step on both 1x1 heads in eager PyTorch with autograd on the same GPU, from the same cached features:
       bf16 GEMM with float32 output, MSE / 2 + BCE-with-logits + cross-entropy + focal Tversky, torch.optim.AdamW on float32
       master weights that are re-rounded to bf16 every step
Every round times all five, the order reversed in odd rounds.  The one-off target build (augment.flow_targets_of on all `--images`
whole images) is timed on its own, `--build_rounds` times.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

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
    """Both 1x1 heads in eager PyTorch: autograd + torch.optim.AdamW, the losses of the reference restated on device tensors."""

    def __init__(self, tr, ncls):
        self.ncls = ncls
        W = torch.cat([tr.sd["out.weight"].reshape(192, 256), tr.w.cpu()]).float().to(tr.device)
        b = torch.cat([tr.sd["out.bias"].float(), tr.b.cpu()]).to(tr.device)
        self.W, self.b = torch.nn.Parameter(W), torch.nn.Parameter(b)
        self.opt = torch.optim.AdamW([self.W, self.b], lr=1e-4, weight_decay=tr.weight_decay)

    def __call__(self, feat, labels, tg, lr):
        n = labels.shape[0]
        for g in self.opt.param_groups:
            g["lr"] = lr
        self.opt.zero_grad(set_to_none=True)
        y = (feat @ self.W.to(torch.bfloat16).T).float() + self.b.to(torch.bfloat16).float()
        z = tokens_to_nchw(y[:, :192], 3, n)
        logits = tokens_to_nchw(y[:, 192:192 + self.ncls * 64], self.ncls, n)
        seg = torch.nn.functional.mse_loss(z[:, :2], 5.0 * tg[:, 1:]) / 2 + \
            torch.nn.functional.binary_cross_entropy_with_logits(z[:, 2], (tg[:, 0] > 0.5).float())
        lab = labels.long()
        ce = torch.nn.functional.cross_entropy(logits, lab, ignore_index=-100)
        valid = (lab != -100)
        p = torch.softmax(logits, 1) * valid[:, None]
        onehot = torch.nn.functional.one_hot(lab.clamp_min(0), self.ncls).permute(0, 3, 1, 2) * valid[:, None]
        tp, fp, fn = (p * onehot).sum((2, 3)), (p * (1 - onehot) * valid[:, None]).sum((2, 3)), ((1 - p) * onehot).sum((2, 3))
        tv = ((1 - tp / (tp + 0.3 * fp + 0.7 * fn)).clamp(1e-6, 1 - 1e-6) ** (1 / 1.33)).mean()
        loss = seg + ce + tv
        loss.backward()
        self.opt.step()
        return float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--build_rounds", type=int, default=3)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many (pf) pool steps with both heads and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, nI, S, ncls = args.crops, args.images, args.size, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    big = np.stack([synth.render_region(300, S * (k % 4), S * (k // 4), S, S) for k in range(nI)])
    big_lab = make_labels(nI, S, ncls, 7 + ncls)
    big_inst = [make_instances(S, 90 + k) for k in range(nI)]
    # the one-off target build, on its own
    build_ms = []
    for _ in range(args.build_rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        tg_all = augment.flow_targets_of(big_inst, dev)
        torch.cuda.synchronize(); build_ms.append((time.perf_counter() - t0) * 1e3)
    del tg_all
    trc = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n)
    trf = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n, train_flow_head=True)
    pool_c = augment.ImagePool(list(big), list(big_lab), device=dev)
    pool_f = augment.ImagePool(list(big), list(big_lab), device=dev, instances=big_inst)
    eager = EagerStep(trc, ncls)
    lr = 1e-4
    # cached features of one fixed set of windows: the grid crops of the first images
    x, y, _win = augment.grid_crops(pool_f)
    tg = augment.grid_flow_targets(pool_f)
    x, y, tg = x[:n], y[:n].contiguous(), tg[:n].contiguous()
    feat = trc.features(x)
    order = np.random.default_rng(0)
    rng = {k: np.random.default_rng(1) for k in ("pc", "pf")}

    def step_pc(idx):
        xb, yb = augment.augment_batch_pool(pool_c, idx, rng["pc"], "geometry", dtype=trc.dtype)
        return trc.step(xb, yb, lr)

    def step_pf(idx):
        xb, yb, tb = augment.augment_batch_pool(pool_f, idx, rng["pf"], "geometry", dtype=trf.dtype, flow_targets=True)
        return trf.step(xb, yb, lr, flow_targets=tb)
    if args.profile_steps:
        for _ in range(args.profile_steps):
            step_pf(order.integers(0, nI, n))
        torch.cuda.synchronize()
        return
    fns = {"c": lambda i: trc.step(feat, y, lr), "f": lambda i: trf.step(feat, y, lr, flow_targets=tg), "pc": step_pc, "pf": step_pf,
           "e": lambda i: eager(feat, y, tg, lr)}
    for f in fns.values():
        for _ in range(3):
            f(order.integers(0, nI, n))
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for rnd in range(args.rounds):
        idx = order.integers(0, nI, n)
        for k in (list(fns) if rnd % 2 == 0 else list(fns)[::-1]):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fns[k](idx)
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"bench_train_flow: {torch.cuda.get_device_name(0)}, {n} windows of 256^2 per step out of {nI} uint8 images of {S}^2, bf16, "
             f"{ncls} classes, ViT depth {args.depth}, {args.rounds} interleaved rounds (order reversed in odd rounds), warmed up, "
             f"host wall clock around a synchronised step, medians (ms)"]
    for k, what in (("c", "step from cached features, class head only (the step before this feature)"),
                    ("f", "step from cached features, class head + flow head                        "),
                    ("pc", "augmented pool step (geometry), class head only                         "),
                    ("pf", "augmented pool step (geometry), both heads, targets warped with the crop"),
                    ("e", "eager PyTorch + autograd, both heads, three losses, cached features      ")):
        lines.append(f"  ({k:2s}) {what} median {med[k]:9.3f}   min {min(times[k]):9.3f} max {max(times[k]):9.3f}   {[round(v, 3) for v in times[k]]}")
    lines.append(f"  (f) - (c) = {med['f'] - med['c']:.3f} ms ({100 * (med['f'] - med['c']) / med['c']:.1f} % of (c)); "
                 f"(pf) - (pc) = {med['pf'] - med['pc']:.3f} ms ({100 * (med['pf'] - med['pc']) / med['pc']:.1f} % of (pc))")
    verdict = "the device step is FASTER than eager PyTorch" if max(times["f"]) < min(times["e"]) else \
        ("the device step LOSES to eager PyTorch" if min(times["f"]) > max(times["e"]) else "the device step and eager PyTorch overlap: no call")
    lines.append(f"  (e) / (f) = {med['e'] / med['f']:.2f}: {verdict} (every round of one below every round of the other, or no call)")
    lines.append(f"  one-off target build, augment.flow_targets_of on {nI} whole images of {S}^2 ({int(np.mean([m.max() for m in big_inst]))} "
                 f"instances each), host renumbering and upload included: {[round(v, 1) for v in build_ms]} ms (the first call also allocates)")
    lines.append(f"  pool bytes: {pool_c.nbytes / 2 ** 20:.1f} MiB without instances, {pool_f.nbytes / 2 ** 20:.1f} MiB with the three float32 target planes")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
