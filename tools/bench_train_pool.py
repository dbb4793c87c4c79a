"""Augmented class-head training from whole 1024^2 images: the device-resident pool with its fused gather kernel against the same
step built from the pieces that existed before it.  One process, interleaved rounds, medians (the style of
tools/bench_train_augment.py).

    python tools/bench_train_pool.py [--rounds 9] [--crops 32] [--out profiles/train_pool_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_pool.py --depth 1 --profile-steps 5      (kernels only)

Workload: `--images` uint8 images of 1024^2 of the synthetic slide with blocky class maps, `--crops` windows of 256^2 per step, a
seeded ViT-L checkpoint with a fresh 7-class head, bf16.
  (a) augment.augment_batch_pool from an ImagePool (uploaded once) + HeadTrainer.step
  (b) the same step from the pieces before the pool: the step's source images taken from HOST memory (images[idx], as
      train_class_head does), ops.hed_jitter on the whole sources, ops.warp_affine for the one shape group, normalisation, patchify
      -- augment.augment_batch on 1024^2 sources -- + the step
  (c) augment.augment_batch from 256^2 host crops + the step (leg (a) of tools/bench_train_augment.py), for scale
(a) and (b) draw the same transforms from equal seeds and are compared bitwise before anything is timed.  Every round times all
three, the order reversed in odd rounds.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many pool steps and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, nI, S, ncls = args.crops, args.images, args.size, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    big = np.stack([synth.render_region(300, S * (k % 4), S * (k // 4), S, S) for k in range(nI)])
    big_lab = make_labels(nI, S, ncls, 7 + ncls)
    small = np.stack([synth.render_region(300, 256 * (k % 8), 256 * (k // 8), 256, 256) for k in range(n)])
    small_lab = make_labels(n, 256, ncls, 8 + ncls)
    tr = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n)
    pool = augment.ImagePool(list(big), list(big_lab), device=dev)
    lr = 1e-4
    order = np.random.default_rng(0)
    rng = {k: np.random.default_rng(1) for k in "abc"}

    def batch_a(idx, g):
        return augment.augment_batch_pool(pool, idx, g, "hed_only", dtype=tr.dtype)

    def batch_b(idx, g):
        return augment.augment_batch(big[idx], big_lab[idx], g, "hed_only", dtype=tr.dtype, device=dev)
    if args.profile_steps:
        for _ in range(args.profile_steps):
            tr.step(*batch_a(order.integers(0, nI, n), rng["a"]), lr)
        torch.cuda.synchronize()
        return
    idx0 = order.integers(0, nI, n)
    (pa, la), (pb, lb) = batch_a(idx0, np.random.default_rng(3)), batch_b(idx0, np.random.default_rng(3))
    assert torch.equal(pa, pb) and torch.equal(la, lb), "the pool step and the step from the earlier pieces differ"
    del pa, la, pb, lb
    fns = {"a": lambda i: tr.step(*batch_a(i, rng["a"]), lr), "b": lambda i: tr.step(*batch_b(i, rng["b"]), lr),
           "c": lambda i: tr.step(*augment.augment_batch(small, small_lab, rng["c"], "hed_only", dtype=tr.dtype, device=dev), lr)}
    for f in fns.values():                  # warm-up: allocations, code objects
        for _ in range(3):
            f(order.integers(0, nI, n))
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for rnd in range(args.rounds):
        idx = order.integers(0, nI, n)      # one draw of source images per round, shared by (a) and (b)
        for k in (list(fns) if rnd % 2 == 0 else list(fns)[::-1]):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fns[k](idx)
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"bench_train_pool: {torch.cuda.get_device_name(0)}, {n} windows of 256^2 per step out of {nI} uint8 images of {S}^2, bf16, "
             f"{ncls} classes, ViT depth {args.depth}, {args.rounds} interleaved rounds, warmed up, medians (ms)"]
    for k, what in (("a", "pool step (ImagePool + augment_batch_pool)       "), ("b", f"earlier pieces, {S}^2 sources from the host     "),
                    ("c", "augment_batch from 256^2 host crops (for scale)  ")):
        lines.append(f"  ({k}) {what} median {med[k]:9.3f}   {[round(x, 3) for x in times[k]]}")
    ok = max(times["a"]) < min(times["b"])
    lines.append(f"  (b)/(a) = {med['b'] / med['a']:.2f}, (a) - (c) = {med['a'] - med['c']:.3f} ms; every round of (a) below every round of (b): {ok}")
    puma = 200 * (5 * 1024 * 1024 + 16)
    lines.append(f"  pool bytes: this pool {pool.nbytes} ({pool.nbytes / 2 ** 20:.1f} MiB); 200 images of 1024^2 (a PUMA-sized set): {puma} "
                 f"({puma / 2 ** 30:.2f} GiB); host upload per step of (b): {n * S * S * 5} bytes")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
