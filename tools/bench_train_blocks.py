"""The price of training the last K transformer blocks next to the neck and the two heads.  One process, interleaved
rounds, medians (the set-up of tools/bench_train_neck.py, whose workload and eager tail this reuses).

    python tools/bench_train_blocks.py [--rounds 7] [--crops 32] [--out profiles/train_blocks_bench.txt]
    python tools/bench_train_blocks.py --grad_precision both --skip_eager --out profiles/train_blocks_bf16_bench.txt     
    python tools/bench_train_blocks.py --grad_precision all --skip_eager --out profiles/train_blocks_attn_bf16_bench.txt  
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_blocks.py --profile-steps 3 [--grad_precision bf16 [--attn_grad_precision bf16] | --grad_precision all]
                                                                                              (kernels of the cached K = 1 step only)

Workload: `--crops` uint8 crops of 256^2 of the synthetic slide, a seeded ViT-L checkpoint with a fresh 7-class 1x1 head, bf16.
  (n)   HeadTrainer(train_neck=True).step from cached backbone rows: the neck-only step of the parent commit
  (b1) (b2) (b4)  HeadTrainer(train_blocks=K).step from the cached input rows of block depth - K: the training forward of K blocks and
        the tail, three losses, cpx_neck_backward, cpx_blocks_backward, every AdamW step and refresh
  (e1) (e2) (e4)  the same blocks, neck and heads in eager PyTorch with autograd on the same GPU, from the same cached rows: bf16 kernels
        on bf16 casts of float32 masters (scaled_dot_product_attention with the decomposed rel-pos bias as its mask), float32 losses,
        torch.optim.AdamW on the masters
  (p1)  (b1) from pixels: the frozen 23 blocks first
  (g1) (g2) (g4)  with --grad_precision both: (bK) with grad_precision="bf16", the blocks' backward on bf16 operands, in the same
        process and the same rounds; --grad_precision bf16 runs (bK) itself in that mode
  (a1) (a2) (a4)  with --grad_precision all: (gK) and, third, the same step with attn_grad_precision="bf16" as well -- the attention
        backward on bf16 operands; --profile-steps with "all" runs its steps in each of the three modes, one after another
Every round times all of them, the order reversed in odd rounds.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import torch.nn.functional as F

from bench_train_neck import EagerStep, make_instances, make_labels
from classpose_amd import augment, engine, synth
from classpose_amd.train import BLOCK_KEYS, HeadTrainer


class EagerBlocks(EagerStep):
    """K blocks in front of bench_train_neck's eager neck and heads."""

    def __init__(self, tr, ncls, K):
        super().__init__(tr, ncls)
        sd, dev, depth = tr.sd, tr.device, tr.weights.depth
        self.blocks = [[torch.nn.Parameter(sd[f"encoder.blocks.{i}.{k}"].detach().float().clone().to(dev)) for k in BLOCK_KEYS]
                       for i in range(depth - K, depth)]
        self.params = self.params + [p for b in self.blocks for p in b]
        self.opt = torch.optim.AdamW(self.params, lr=1e-4, weight_decay=tr.weight_decay)
        a = torch.arange(32, device=dev)
        self.idx = a[:, None] - a[None, :] + 31

    def block(self, x, p, n):
        bf = torch.bfloat16
        g1, b1, Wq, bq, rh, rw, Wp, bp, g2, b2, W1, c1, W2, c2 = (t.to(bf) for t in p)
        h = F.layer_norm(x, (1024,), g1, b1, 1e-6)
        q, k, v = F.linear(h, Wq, bq).view(n, 1024, 3, 16, 64).permute(2, 0, 3, 1, 4).unbind(0)
        qg = q.reshape(n, 16, 32, 32, 64)
        Rh, Rw = engine.interp_rel_pos(rh)[self.idx], engine.interp_rel_pos(rw)[self.idx]
        bias = (torch.einsum("bnhwc,hkc->bnhwk", qg, Rh)[..., :, None] + torch.einsum("bnhwc,wkc->bnhwk", qg, Rw)[..., None, :]).reshape(n, 16, 1024, 1024)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=bias, scale=0.125)
        x = x + F.linear(o.transpose(1, 2).reshape(n * 1024, 1024), Wp, bp)
        h = F.layer_norm(x, (1024,), g2, b2, 1e-6)
        return x + F.linear(F.gelu(F.linear(h, W1, c1)), W2, c2)

    def __call__(self, x, labels, tg, lr):
        n = labels.shape[0]
        for p in self.blocks:
            x = self.block(x, p, n)
        return super().__call__(x, labels, tg, lr)      # (its zero_grad comes after this forward: no gradient exists yet)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--blocks", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many cached K = 1 steps and exit (for rocprofv3)")
    ap.add_argument("--grad_precision", default="fp32", choices=["fp32", "bf16", "both", "all"],
                    help="the blocks' backward of (bK): float32 products, bf16 operands, both modes side by side ((bK) float32, (gK) bf16), or "
                         "all three ((aK): bf16 operands in the attention backward as well)")
    ap.add_argument("--attn_grad_precision", default="fp32", choices=["fp32", "bf16"],
                    help="with --grad_precision bf16: the attention backward of (bK) and of the --profile-steps run on bf16 operands too")
    ap.add_argument("--skip_eager", action="store_true", help="leave out the eager PyTorch steps (eK) and the step from pixels (p1)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    base_mode = "bf16" if args.grad_precision == "bf16" else "fp32"
    if args.attn_grad_precision == "bf16" and args.grad_precision != "bf16":
        ap.error("--attn_grad_precision bf16 goes with --grad_precision bf16 (--grad_precision all times it as (aK))")
    base_kw = dict(grad_precision=base_mode, attn_grad_precision=args.attn_grad_precision)
    dev = torch.device("cuda:0")
    n, ncls = args.crops, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    ims = np.stack([synth.render_region(300, 256 * (k % 8), 256 * (k // 8), 256, 256) for k in range(n)])
    labs = make_labels(n, 256, ncls, 7 + ncls)
    labd = torch.from_numpy(labs).to(dev)
    tg = torch.stack(augment.flow_targets_of([make_instances(256, 90 + k) for k in range(n)], dev)).contiguous()
    lr = 1e-4
    mk = lambda **kw: HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n, train_flow_head=True, **kw)
    if args.profile_steps:
        modes = [base_kw] if args.grad_precision != "all" else \
            [dict(grad_precision="fp32"), dict(grad_precision="bf16"), dict(grad_precision="bf16", attn_grad_precision="bf16")]
        for mode in modes:
            t = mk(train_blocks=1, **mode)
            rows = t.backbone_features(ims)
            for _ in range(args.profile_steps):
                t.step(rows, labs, lr, flow_targets=tg)
            torch.cuda.synchronize()
        return
    fns, what, first_ev = {}, {}, {}
    trn = mk(train_neck=True)
    rows_n = trn.backbone_features(ims)
    fns["n"], what["n"] = (lambda: trn.step(rows_n, labs, lr, flow_targets=tg)["loss"]), "step from cached backbone rows, neck + both heads (the parent commit's step)"
    for K in args.blocks:
        t = mk(train_blocks=K, **base_kw)
        rows = t.backbone_features(ims)
        first_ev[K] = t.evaluate(rows, labs, flow_targets=tg)["loss"]
        fns[f"b{K}"] = (lambda t=t, rows=rows: t.step(rows, labs, lr, flow_targets=tg)["loss"])
        what[f"b{K}"] = f"step from cached rows, last {K} block(s) + neck + both heads, {base_mode} gradient products" + \
            (", bf16 attention backward" if args.attn_grad_precision == "bf16" else "")
        if args.grad_precision in ("both", "all"):
            t16 = mk(train_blocks=K, grad_precision="bf16")
            fns[f"g{K}"] = (lambda t=t16, rows=rows: t.step(rows, labs, lr, flow_targets=tg)["loss"])
            what[f"g{K}"] = "the same step with grad_precision bf16: the blocks' backward on bf16 operands"
        if args.grad_precision == "all":
            ta = mk(train_blocks=K, grad_precision="bf16", attn_grad_precision="bf16")
            fns[f"a{K}"] = (lambda t=ta, rows=rows: t.step(rows, labs, lr, flow_targets=tg)["loss"])
            what[f"a{K}"] = "the same step with attn_grad_precision bf16 as well: the attention backward on bf16 operands"
        if args.skip_eager:
            continue
        e = EagerBlocks(t, ncls, K)
        fns[f"e{K}"] = (lambda e=e, rows=rows: e(rows, labd, tg, lr))
        what[f"e{K}"] = f"eager PyTorch + autograd, last {K} block(s) + neck + both heads, the same cached rows"
        if K == args.blocks[0]:
            fns[f"p{K}"] = (lambda t=t: t.step(ims, labs, lr, flow_targets=tg)["loss"])
            what[f"p{K}"] = f"step from pixels, last {K} block(s) + neck + both heads (the frozen {args.depth - K} blocks first)"
    first = {k: f() for k, f in fns.items()}
    for K in () if args.skip_eager else args.blocks:      # (the eager forward rounds where torch's bf16 kernels round: loose agreement only)
        assert abs(first[f"e{K}"] - first_ev[K]) <= 5e-2 * abs(first_ev[K]), (K, first, first_ev)
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for rnd in range(args.rounds):
        for k in (list(fns) if rnd % 2 == 0 else list(fns)[::-1]):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fns[k]()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"bench_train_blocks: {torch.cuda.get_device_name(0)}, {n} crops of 256^2 per step, bf16, {ncls} classes, ViT depth {args.depth}, "
             f"{args.rounds} interleaved rounds (order reversed in odd rounds), warmed up, host wall clock around a synchronised step, "
             f"medians (ms); first losses {({k: round(v, 4) for k, v in first.items()})}"]
    for k in fns:
        lines.append(f"  ({k:2s}) {what[k]:96s} median {med[k]:10.3f}   min {min(times[k]):10.3f} max {max(times[k]):10.3f}   {[round(v, 1) for v in times[k]]}")
    for K in args.blocks if args.grad_precision == "all" else ():
        g, a = f"g{K}", f"a{K}"
        order = "EVERY round of the bf16 attention backward lies below every round of grad_precision bf16 alone" if max(times[a]) < min(times[g]) else \
            "the rounds of the two modes OVERLAP"
        lines.append(f"  K = {K}: ({g}) / ({a}) = {med[g] / med[a]:.2f}; ({g}) - ({a}) = {(med[g] - med[a]) / K:.1f} ms per trained block; ({a}) - (n) = "
                     f"{(med[a] - med['n']) / K:.1f} ms per trained block; {order}")
    for K in args.blocks if args.grad_precision in ("both", "all") else ():
        b, g = f"b{K}", f"g{K}"
        order = "EVERY round of the bf16 mode lies below every round of the float32 mode" if max(times[g]) < min(times[b]) else \
            "the rounds of the two modes OVERLAP"
        lines.append(f"  K = {K}: ({b}) / ({g}) = {med[b] / med[g]:.2f}; ({g}) - (n) = {med[g] - med['n']:.1f} ms, {(med[g] - med['n']) / K:.1f} ms per "
                     f"trained block (float32 mode {(med[b] - med['n']) / K:.1f}); {order}")
    for K in () if args.skip_eager else args.blocks:
        b, e = f"b{K}", f"e{K}"
        verdict = "the device step is FASTER than eager PyTorch" if max(times[b]) < min(times[e]) else \
            ("the device step LOSES to eager PyTorch" if min(times[b]) > max(times[e]) else "the device step and eager PyTorch overlap: no call")
        lines.append(f"  K = {K}: ({b}) - (n) = {med[b] - med['n']:.1f} ms, {(med[b] - med['n']) / K:.1f} ms per trained block; ({e}) / ({b}) = "
                     f"{med[e] / med[b]:.2f}: {verdict}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
