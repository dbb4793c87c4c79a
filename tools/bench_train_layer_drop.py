"""What layer drop (train_head --layer_drop) takes off the step: a dropped (block, crop) pair is computed neither forward nor
backward.  One process, interleaved rounds, medians with ranges (the set-up of tools/bench_train_blocks.py, whose workload this reuses).

    python tools/bench_train_layer_drop.py [--rounds 9] [--crops 32] [--blocks 4 24] [--rate 0.4] [--out profiles/train_layer_drop_bench.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_layer_drop.py --profile-steps 3 --profile-mask all|pairs|halves
    python tools/bench_train_layer_drop.py --summarise DIR_all DIR_pairs DIR_halves --out profiles/train_layer_drop_kernel_stats.txt

Workload: `--crops` uint8 crops of 256^2 of the synthetic slide, a seeded ViT-L checkpoint with a fresh 7-class 1x1 head, bf16, bf16
gradient products and bf16 attention backward, cached rows.
  (n)    HeadTrainer(train_neck=True).step: the neck and both heads alone -- what a step costs outside the blocks
  (kK)   HeadTrainer(train_blocks=K).step(keep=None): rate 0, bitwise the step without the feature (cpx_blocks_forward_train,
         cpx_blocks_backward_in) and therefore its stand-in
  (dK)   the same trainer's step(keep=mask), the mask drawn once by draw_keep_mask(default_rng(--seed), crops, depth, K, rate) and the
         same in every round; f = its dropped share of the K * crops (block, crop) pairs
Every round times all of them, the order reversed in odd rounds.  GATE (exit status 1): every round of (dK) lies below every round of
(kK), at every K.  Reported, not gated: (dK) / (kK) against 1 - f * (blocks' share of the step), the share taken as ((kK) - (n)) / (kK).

--profile-steps: that many K = `--profile-blocks` steps under one hand-made mask, for rocprofv3 (a run of its own per mask).  Each mask
keeps 16 of 32 crops in every block, so the forwards are the same work; the backwards differ in how the kept crops sit in the slabs of
two: "pairs" keeps crops 4i, 4i + 1 (half the slabs whole, half empty), "halves" keeps the even crops (every slab one crop, 1024 rows per
launch where "pairs" has 2048); "all" drops nothing.  --summarise adds the three runs' kernel times up.
"""
import argparse
import csv
import glob
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def kernel_stats(d):
    """{kernel name: (calls, total ns)} of the *kernel_stats.csv under directory ``d``"""
    files = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
    if len(files) != 1:
        raise SystemExit(f"{d}: expected one *kernel_stats.csv, found {files}")
    with open(files[0], newline="") as f:
        return {r["Name"]: (int(r["Calls"]), int(r["TotalDurationNs"])) for r in csv.DictReader(f)}


def summarise(dirs, steps, K, out):
    names = ("all", "pairs", "halves")
    st = {n: kernel_stats(d) for n, d in zip(names, dirs)}
    tot = {n: sum(v[1] for v in st[n].values()) for n in names}
    short = lambda k: k if len(k) <= 100 else k[:97] + "..."
    lines = [f"rocprofv3 --kernel-trace --stats -- python tools/bench_train_layer_drop.py --profile-steps {steps} --profile-mask all | pairs | halves",
             f"(three runs of their own; 32 crops, bf16, both bf16 gradient switches, K = {K}, the cached rows made in the same process: the frozen "
             "blocks' kernels are in every run alike).  Every mask but \"all\" keeps 16 crops in every block: \"pairs\" as 8 whole slabs of two, "
             "\"halves\" as 16 slabs with one kept crop each.",
             "", "sum of all kernel time (ms): " + ", ".join(f"{n} {tot[n] / 1e6:.3f}" for n in names)]
    per = steps * K
    d_hp, d_ap = tot["halves"] - tot["pairs"], tot["all"] - tot["pairs"]
    lines += [f"halves - pairs = {d_hp / 1e6:.3f} ms over {steps} steps and {K} blocks: {d_hp / per / 16 / 1e3:.1f} us per one-crop slab body on top of half a "
              f"two-crop body; all - pairs = {d_ap / 1e6:.3f} ms = what the 16 dropped crops per block cost, {d_ap / per / 1e6:.3f} ms per block and step",
              f"a block's kept crops regrouped into whole slabs would take {100.0 * d_hp / tot['halves']:.2f} % off the kernel time of the \"halves\" run "
              f"({100.0 * d_hp / max(d_ap, 1):.1f} % of what dropping half the pairs saves)", "",
              "kernels whose total differs most between halves and pairs (Name, calls halves / pairs, total ms halves / pairs):"]
    keys = sorted(set(st["halves"]) | set(st["pairs"]), key=lambda k: -abs(st["halves"].get(k, (0, 0))[1] - st["pairs"].get(k, (0, 0))[1]))
    for k in keys[:16]:
        h, p = st["halves"].get(k, (0, 0)), st["pairs"].get(k, (0, 0))
        lines.append(f"  {short(k)}, {h[0]} / {p[0]}, {h[1] / 1e6:.3f} / {p[1] / 1e6:.3f}")
    lines += ["", "the compaction kernel (k_move_crop_rows) in the halves run: " +
              ", ".join(f"{short(k)}: {v[0]} calls, {v[1] / 1e6:.3f} ms" for k, v in st["halves"].items() if "k_move_crop_rows" in k)]
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "w") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--blocks", type=int, nargs="+", default=[4, 24])
    ap.add_argument("--rate", type=float, default=0.4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many steps under --profile-mask and exit (for rocprofv3)")
    ap.add_argument("--profile-mask", default="all", choices=["all", "pairs", "halves"])
    ap.add_argument("--profile-blocks", type=int, default=4)
    ap.add_argument("--summarise", nargs=3, default=None, metavar="DIR", help="the rocprofv3 output directories of the all, pairs and halves runs")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.summarise:
        return summarise(args.summarise, args.profile_steps or 3, args.profile_blocks, args.out)
    import numpy as np
    import torch

    from bench_train_neck import make_instances, make_labels
    from classpose_amd import augment, synth
    from classpose_amd.train import HeadTrainer, draw_keep_mask
    dev = torch.device("cuda:0")
    n, ncls = args.crops, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    ims = np.stack([synth.render_region(300, 256 * (k % 8), 256 * (k // 8), 256, 256) for k in range(n)])
    labs = make_labels(n, 256, ncls, 7 + ncls)
    tg = torch.stack(augment.flow_targets_of([make_instances(256, 90 + k) for k in range(n)], dev)).contiguous()
    lr = 1e-4
    mk = lambda **kw: HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n, train_flow_head=True, **kw)
    mkb = lambda K: mk(train_blocks=K, grad_precision="bf16", attn_grad_precision="bf16")
    if args.profile_steps:
        K = args.profile_blocks
        crop = np.arange(n)
        row = {"all": np.ones(n, bool), "pairs": crop % 4 < 2, "halves": crop % 2 == 0}[args.profile_mask]
        keep = np.ascontiguousarray(np.broadcast_to(row.astype(np.uint8), (K, n)))
        t = mkb(K)
        rows = t.backbone_features(ims)
        for _ in range(args.profile_steps):
            t.step(rows, labs, lr, flow_targets=tg, keep=keep)
        torch.cuda.synchronize()
        return None
    fns, what, share = {}, {}, {}
    trn = mk(train_neck=True)
    rows_n = trn.backbone_features(ims)
    fns["n"], what["n"] = (lambda: trn.step(rows_n, labs, lr, flow_targets=tg)["loss"]), "step from cached backbone rows, neck + both heads: the step outside the blocks"
    for K in args.blocks:
        t = mkb(K)
        rows = t.backbone_features(ims)
        keep = draw_keep_mask(np.random.default_rng(args.seed), n, args.depth, K, args.rate)
        share[K] = 1.0 - float(keep.mean())
        fns[f"k{K}"] = (lambda t=t, rows=rows: t.step(rows, labs, lr, flow_targets=tg)["loss"])
        what[f"k{K}"] = f"step from cached rows, last {K} blocks + neck + both heads, rate 0 (the step without the feature)"
        fns[f"d{K}"] = (lambda t=t, rows=rows, keep=keep: t.step(rows, labs, lr, flow_targets=tg, keep=keep)["loss"])
        what[f"d{K}"] = f"the same trainer's step under one mask of rate {args.rate:g}: f = {share[K]:.4f} of the {K * n} (block, crop) pairs dropped"
    first = {k: f() for k, f in fns.items()}
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
    lines = [f"bench_train_layer_drop: {torch.cuda.get_device_name(0)}, {n} crops of 256^2 per step, bf16, {ncls} classes, ViT depth {args.depth}, bf16 "
             f"gradient products and bf16 attention backward, {args.rounds} interleaved rounds (order reversed in odd rounds), warmed up, host wall "
             f"clock around a synchronised step, medians (ms); masks from seed {args.seed}; first losses {({k: round(v, 4) for k, v in first.items()})}"]
    for k in fns:
        lines.append(f"  ({k:3s}) {what[k]:112s} median {med[k]:10.3f}   min {min(times[k]):10.3f} max {max(times[k]):10.3f}   {[round(v, 1) for v in times[k]]}")
    gate = True
    for K in args.blocks:
        k, d = f"k{K}", f"d{K}"
        below = max(times[d]) < min(times[k])
        gate = gate and below
        blocks_share = (med[k] - med["n"]) / med[k]
        expect = 1.0 - share[K] * blocks_share
        lines.append(f"  K = {K}: ({d}) / ({k}) = {med[d] / med[k]:.4f}; 1 - f * (blocks' share of the step) = 1 - {share[K]:.4f} * {blocks_share:.4f} = {expect:.4f}, "
                     f"the measured ratio lies {med[d] / med[k] - expect:+.4f} from it; ({k}) - ({d}) = {med[k] - med[d]:.1f} ms; "
                     + ("EVERY round with drop lies below every round without" if below else "GATE FAILED: the rounds with and without drop OVERLAP"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    return None if gate else 1


if __name__ == "__main__":
    sys.exit(main())
