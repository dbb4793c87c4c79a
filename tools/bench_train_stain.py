"""The price of the H&E stain-matrix perturbation in augmented class-head training from whole 1024^2 images.  One
process, interleaved rounds, medians (the set-up of tools/bench_train_pool.py).

    python tools/bench_train_stain.py [--rounds 9] [--crops 32] [--out profiles/train_stain_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_stain.py --depth 1 --profile-steps 5      (kernels only)

Workload: `--images` uint8 images of 1024^2 of the synthetic slide with blocky class maps, `--crops` windows of 256^2 per step, a
seeded ViT-L checkpoint with a fresh 7-class head, bf16.
  (a) augment.augment_batch_pool(config="hed_he") from an ImagePool + HeadTrainer.step: per crop the HED jitter or the stain
      perturbation on the taps of the fused pool kernel, the bases cached on the pool
  (p) the same step with "hed_only": what the pool step cost before; (a) - (p) is the price of the feature
  (h) the reference's formulation on the host: per drawn image the colour transform of "hed_he" on the WHOLE image in numpy
      float64 -- for the stain perturbation the NMF refitted at every draw, as extract_stains does -- then the device geometry
      from the transformed host images (augment.augment_batch(config="geometry")) + the step
Every round times all three, the order reversed in odd rounds.  Accepted when every round of (a) is below every round of (h).
The one-off set-up per image (samples kernel, host fit) is timed apart.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from classpose_amd import augment, ops, stain, synth
from classpose_amd.train import HeadTrainer


def make_labels(n, size, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.kron(rng.integers(0, ncls, (n, size // 8, size // 8)), np.ones((1, 8, 8), np.int64)).astype(np.int16)
    for b in range(n):
        y0 = int(rng.integers(0, size - 56))
        lab[b, y0:y0 + 20] = -100
    return lab


def host_colour(images, g, cfg):
    """"hed_he" on whole host images as the reference computes it: numpy float64, the stain basis refitted per draw."""
    import augment_reference as ar
    import stain_reference as sr
    n = len(images)
    use_hed = g.random(n) < cfg["hed_probability"]
    sigma, bias = augment.sample_hed(g, n, cfg["sigma_ranges"], cfg["bias_ranges"])
    gate, U, u = augment.sample_he(g, n)
    he = cfg["he_staining"]
    out = np.empty_like(images)
    for t in range(n):
        if use_hed[t]:
            out[t] = ar.hed_jitter(images[t], sigma[t], bias[t], augment.HED_FROM_RGB, cfg["cutoff_range"], False, np.float64)[0]
        elif gate[t] <= he["probability"]:
            H, Hinv = stain.image_basis(images[t])
            out[t] = images[t] if H is None else sr.he_stain(images[t], stain.stain_params(H, Hinv, U[t], u[t], he["amount_matrix"],
                                                                                           he["amount_stains"]))[0]
        else:
            out[t] = images[t]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0, help="fit the bases, run this many hed_he pool steps and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, nI, S, ncls = args.crops, args.images, args.size, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    big = np.stack([synth.render_region(300, S * (k % 4), S * (k // 4), S, S) for k in range(nI)])
    big_lab = make_labels(nI, S, ncls, 7 + ncls)
    tr = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n)
    pool = augment.ImagePool(list(big), list(big_lab), device=dev)
    cfg = augment.get_config("hed_he")
    lr = 1e-4
    order = np.random.default_rng(0)
    rng = {k: np.random.default_rng(1) for k in "aph"}

    # the one-off set-up: samples (device, warmed up once) and the fit (host), per image
    ops.stain_samples(pool.pool_u8, pool.px_off, pool.hw)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    _k, samples, _st, _raw = ops.stain_samples(pool.pool_u8, pool.px_off, pool.hw)
    torch.cuda.synchronize(); t_samples = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    pool._stain = augment.StainBases.from_samples(samples)
    t_fit = (time.perf_counter() - t0) * 1e3

    def batch_a(idx, g):
        return augment.augment_batch_pool(pool, idx, g, "hed_he", dtype=tr.dtype)

    def batch_p(idx, g):
        return augment.augment_batch_pool(pool, idx, g, "hed_only", dtype=tr.dtype)

    def batch_h(idx, g):
        return augment.augment_batch(host_colour(big[idx], g, cfg), big_lab[idx], g, "geometry", dtype=tr.dtype, device=dev)
    if args.profile_steps:
        for _ in range(args.profile_steps):
            tr.step(*batch_a(order.integers(0, nI, n), rng["a"]), lr)
        torch.cuda.synchronize()
        return
    fns = {"a": lambda i: tr.step(*batch_a(i, rng["a"]), lr), "p": lambda i: tr.step(*batch_p(i, rng["p"]), lr),
           "h": lambda i: tr.step(*batch_h(i, rng["h"]), lr)}
    for k, f in fns.items():                # warm-up: allocations, code objects (the host leg once: it takes seconds)
        for _ in range(1 if k == "h" else 3):
            f(order.integers(0, nI, n))
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for rnd in range(args.rounds):
        idx = order.integers(0, nI, n)      # one draw of source images per round, shared by the legs
        for k in (list(fns) if rnd % 2 == 0 else list(fns)[::-1]):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fns[k](idx)
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    lines = [f"bench_train_stain: {torch.cuda.get_device_name(0)}, {n} windows of 256^2 per step out of {nI} uint8 images of {S}^2, bf16, "
             f"{ncls} classes, ViT depth {args.depth}, {args.rounds} interleaved rounds, warmed up, medians (ms)"]
    for k, what in (("a", "pool step, hed_he (HED jitter or stain perturbation per crop)  "),
                    ("p", "pool step, hed_only (the step before this feature)             "),
                    ("h", "hed_he on whole host images in numpy float64, NMF per draw     ")):
        lines.append(f"  ({k}) {what} median {med[k]:9.3f}   {[round(x, 3) for x in times[k]]}")
    ok = max(times["a"]) < min(times["h"])
    lines.append(f"  (a) - (p) = {med['a'] - med['p']:.3f} ms ({100 * (med['a'] - med['p']) / med['p']:.1f} % of (p)), (h)/(a) = {med['h'] / med['a']:.1f}; "
                 f"every round of (a) below every round of (h): {ok}")
    lines.append(f"  one-off set-up of the {nI} images: ops.stain_samples {t_samples:.3f} ms in all (three launches, one download), the host "
                 f"fit {t_fit / nI:.1f} ms per image ({[len(s) for s in samples]} sample rows)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
