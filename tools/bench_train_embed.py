"""The price of training the patch embedding and the position table on top of all 24 blocks.  One process, interleaved rounds,
medians with ranges (the set-up of tools/bench_train_blocks.py, whose workload this reuses).

    python tools/bench_train_embed.py [--rounds 7] [--crops 32] [--out profiles/train_embed_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_embed.py --profile-steps 2     (kernels of the train_embed steps only)

Workload: `--crops` uint8 crops of 256^2 of the synthetic slide, a seeded ViT-L checkpoint with a fresh 7-class 1x1 head, bf16, K = depth.
  (f0) (f1)  HeadTrainer(train_blocks=depth).step with float32 gradient products: (f0) without train_embed, from the cached input rows of
        block 0 -- the parent commit's path, launch for launch --, (f1) with train_embed, from cached patch rows: the embedding's launch, the
        same blocks, dx_in, cpx_embed_backward, one more AdamW step and refresh
  (h0) (h1)  the same pair with grad_precision = attn_grad_precision = "bf16"
  (k32) (k16)  ops.embed_backward alone on the rows and the dx_in of that step, grad_dtype float32 and bfloat16
Every round times all of them, the order reversed in odd rounds."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from bench_train_neck import make_instances, make_labels
from classpose_amd import augment, ops, synth
from classpose_amd.train import HeadTrainer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many train_embed steps in each gradient mode and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, ncls, K = args.crops, args.classes, args.depth
    backbone = synth.make_state_dict(1, None, depth=K, seed=0)
    ims = np.stack([synth.render_region(300, 256 * (k % 8), 256 * (k // 8), 256, 256) for k in range(n)])
    labs = make_labels(n, 256, ncls, 7 + ncls)
    tg = torch.stack(augment.flow_targets_of([make_instances(256, 90 + k) for k in range(n)], dev)).contiguous()
    lr = 1e-4
    modes = {"f": dict(grad_precision="fp32"), "h": dict(grad_precision="bf16", attn_grad_precision="bf16")}
    mk = lambda **kw: HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n, train_flow_head=True, train_blocks=K, **kw)
    if args.profile_steps:
        for kw in modes.values():
            t = mk(train_embed=True, **kw)
            rows = t.patch_rows(ims)
            for _ in range(args.profile_steps):
                t.step(rows, labs, lr, flow_targets=tg)
            torch.cuda.synchronize()
            del t
        return
    fns, what = {}, {}
    for m, kw in modes.items():
        name = "float32 gradient products" if m == "f" else "bf16 gradient products and bf16 attention backward"
        t0, t1 = mk(**kw), mk(train_embed=True, **kw)
        x0, p1 = t0.backbone_features(ims), t1.patch_rows(ims)
        assert t0.embed is None and t1.embed is not None and torch.equal(t0.evaluate(x0, labs, flow_targets=tg, return_head=True)["head"],
                                                                         t1.evaluate(p1, labs, flow_targets=tg, return_head=True)["head"])
        fns[f"{m}0"] = (lambda t=t0, x=x0: t.step(x, labs, lr, flow_targets=tg)["loss"])
        what[f"{m}0"] = f"step from cached block-0 rows, {K} blocks + neck + both heads, {name} (the parent commit's step)"
        fns[f"{m}1"] = (lambda t=t1, x=p1: t.step(x, labs, lr, flow_targets=tg)["loss"])
        what[f"{m}1"] = "the same step with train_embed, from cached patch rows"
    first = {k: f() for k, f in fns.items()}
    dx_in = t1._buf[("emb_bwd", n * 1024)][0].clone()                   # a real gradient of block 0's input
    for code, gd in (("k32", torch.float32), ("k16", torch.bfloat16)):
        ws, g = ops.embed_backward_workspace(n, ops._DT[p1.dtype], dev, gd), torch.empty(ops.embed_grad_layout()[0], device=dev)
        fns[code] = (lambda ws=ws, g=g, gd=gd: ops.embed_backward(p1, dx_in, g, ws, grad_dtype=gd))
        what[code] = f"cpx_embed_backward alone, dW in {'float32 (exact-float32 MFMA behind transposing copies)' if gd == torch.float32 else 'bf16 (k_embed_dw16 + k_embed_dw_finish)'}"
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
    lines = [f"bench_train_embed: {torch.cuda.get_device_name(0)}, {n} crops of 256^2 per step, bf16, {ncls} classes, ViT depth {K}, all {K} blocks trained, "
             f"{args.rounds} interleaved rounds (order reversed in odd rounds), warmed up, host wall clock around a synchronised step, "
             f"medians (ms); first losses {({k: round(v, 4) for k, v in first.items()})}"]
    for k in fns:
        lines.append(f"  ({k:3s}) {what[k]:118s} median {med[k]:10.3f}   min {min(times[k]):10.3f} max {max(times[k]):10.3f}   {[round(v, 2) for v in times[k]]}")
    for m in modes:
        a, b = f"{m}0", f"{m}1"
        order = "the rounds of the two OVERLAP: the difference is within the run-to-run spread" if min(times[b]) <= max(times[a]) else \
            "every round with train_embed lies above every round without"
        lines.append(f"  ({b}) - ({a}) = {med[b] - med[a]:.2f} ms = {100 * (med[b] - med[a]) / med[a]:.2f} % of the step without train_embed; {order}")
    verdict = "the bf16 dW kernel is FASTER than the float32 route" if max(times["k16"]) < min(times["k32"]) else \
        ("the bf16 dW kernel LOSES to the float32 route" if min(times["k16"]) > max(times["k32"]) else "the two routes overlap: no call")
    lines.append(f"  (k32) / (k16) = {med['k32'] / med['k16']:.2f}: {verdict} (both include dpos and db, the same two launches)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
