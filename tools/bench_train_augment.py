"""Augmented class-head training: what the device augmentation adds to a training step, and what the same augmentation costs on
the host.  One process, interleaved rounds, medians (the style of tools/bench_train_head.py).

    python tools/bench_train_augment.py [--rounds 9] [--crops 32] [--out profiles/train_augment_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_augment.py --depth 1 --profile-steps 5      (kernels only)

Workload: `--crops` uint8 crops of 256^2 of the synthetic slide on the HOST (where the training loop keeps its set), blocky random
class maps, a seeded ViT-L checkpoint with a fresh 7-class head, bf16.
  (f) cpx_net_forward alone on the crops' patch rows: the baseline
  (u) HeadTrainer.step from the host uint8 crops, no augmentation: the uncached step of train_class_head
  (a) augment.augment_batch (draws on the host; stain jitter, warp, float32 normalisation, patchify on the device) + the step
  (h) the same augmentation on the host, as a `transform=` callback would have to do it without OpenCV / skimage: the float32 numpy
      restatement of tests/augment_reference.py, then the step from float32 crops
Every round times all four, the order reversed in odd rounds.  Leg (h) IS the test suite's restatement, so this tool imports
tests/augment_reference.py (it puts tests/ on sys.path): the one tool here that depends on a test helper.
"""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import augment_reference as ar
from classpose_amd import _lib, augment, synth
from classpose_amd.train import HeadTrainer


def make_labels(n, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.kron(rng.integers(0, ncls, (n, 32, 32)), np.ones((1, 8, 8), np.int64)).astype(np.int16)
    for b in range(n):
        y0 = int(rng.integers(0, 200))
        lab[b, y0:y0 + 20] = -100
    return lab


def host_augment(X, labels, rng, cfg, scale_range=0.5):
    """augment_batch's stages in float32 numpy: (float32 (n, 3, 256, 256) normalised crops, int16 labels)."""
    n = len(X)
    p = augment.sample_batch_params(rng, n, 256, 256, cfg, scale_range, True, 256)
    out = np.empty((n, 3, 256, 256), np.float32)
    lab = np.empty((n, 256, 256), np.int16)
    for i in range(n):
        j = ar.hed_jitter(X[i], p.sigma[i], p.bias[i], augment.HED_FROM_RGB, cfg["cutoff_range"], False, np.float32)[0]
        out[i] = ar.warp_image(j.transpose(2, 0, 1), p.inv[i], 256, 256, np.float32)
        lab[i] = ar.warp_labels(labels[i], p.inv[i], 256, 256, 0)
    return ar.normalize_f32(out)[1], lab


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many augmented steps and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, ncls = args.crops, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    X = np.stack([synth.render_region(300, 256 * (k % 8), 256 * (k // 8), 256, 256) for k in range(n)])
    lab = make_labels(n, ncls, 7 + ncls)
    tr = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n)
    cfg = augment.get_config("hed_only")
    lr = 1e-4
    rng_a, rng_h = np.random.default_rng(1), np.random.default_rng(1)

    def step_a():
        return tr.step(*augment.augment_batch(X, lab, rng_a, "hed_only", dtype=tr.dtype, device=dev), lr)
    if args.profile_steps:
        for _ in range(args.profile_steps):
            step_a()
        torch.cuda.synchronize()
        return
    # the two augmentations draw the same transforms and agree before anything is timed
    xa, la = augment.apply_params(torch.from_numpy(X[:2]).to(dev), torch.from_numpy(lab[:2]).to(dev),
                                  augment.sample_batch_params(np.random.default_rng(3), 2, 256, 256, cfg), cfg)
    xh, lh = host_augment(X[:2], lab[:2], np.random.default_rng(3), cfg)
    assert np.array_equal(la.cpu().numpy(), lh) and np.abs(xa.cpu().numpy() - xh).max() < 0.05, np.abs(xa.cpu().numpy() - xh).max()
    patches = tr._patches(X)
    L, c = _lib.lib(), tr.weights.c
    st = torch.cuda.current_stream(dev).cuda_stream

    def forward():
        _lib.check(L.cpx_net_forward(C.byref(c), _lib.ptr(patches), n, _lib.ptr(tr._head_fb), _lib.ptr(tr._net_ws),
                                     tr._net_ws.numel(), st), "net_forward")
    fns = {"f": forward, "u": lambda: tr.step(X, lab, lr), "a": step_a, "h": lambda: tr.step(*host_augment(X, lab, rng_h, cfg), lr)}
    for k, f in fns.items():                # warm-up: allocations, code objects
        for _ in range(1 if k == "h" else 3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for rnd in range(args.rounds):
        for k in (list(fns) if rnd % 2 == 0 else list(fns)[::-1]):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fns[k]()
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"bench_train_augment: {torch.cuda.get_device_name(0)}, {n} uint8 crops of 256^2 from the host, bf16, {ncls} classes, "
             f"ViT depth {args.depth}, {args.rounds} interleaved rounds, warmed up, medians (ms)"]
    for k, what in (("f", "cpx_net_forward alone                 "), ("u", "uncached step from uint8, unaugmented "),
                    ("a", "device-augmented step (hed_only)      "), ("h", "host-augmented step (numpy float32)    ")):
        lines.append(f"  ({k}) {what} median {med[k]:9.3f}   {[round(x, 3) for x in times[k]]}")
    ok = max(times["a"]) < min(times["h"])
    lines.append(f"  device price of augmentation (a) - (u) = {med['a'] - med['u']:.3f} ms = {100 * (med['a'] - med['u']) / med['u']:.1f} % of (u); "
                 f"host route / device route (h)/(a) = {med['h'] / med['a']:.1f}; every round of (a) below every round of (h): {ok}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        raise SystemExit("a round of the device-augmented step was not below every round of the host-augmented step")


if __name__ == "__main__":
    main()
