"""The price of the image-quality stage (Gaussian blur, hue / brightness / saturation jitter) in augmented class-head training
from whole 1024^2 images.  One process, interleaved rounds, medians (the set-up of tools/bench_train_stain.py).

    python tools/bench_train_quality.py [--rounds 9] [--crops 32] [--out profiles/train_quality_bench.txt]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_train_quality.py --depth 1 --profile-steps 5      (kernels only)

Workload: `--images` uint8 images of 1024^2 of the synthetic slide with blocky class maps, `--crops` windows of 256^2 per step, a
seeded ViT-L checkpoint with a fresh 7-class head, bf16.
  (a) augment.augment_batch_pool(config="hed_he_quality") from an ImagePool + HeadTrainer.step: the colour stage, the blur of the
      gated crops' footprints (ops.blur_pool_rects), the fused pool kernel with HBS on the taps
  (p) the same step with "hed_he": what the pool step cost before; (a) - (p) is the price of the feature
  (h) the reference's formulation of the quality stage on the host: per drawn image scipy.ndimage.gaussian_filter per channel
      and the float32 HBS in numpy on the WHOLE image, then the device geometry from the transformed host images
      (augment.augment_batch(config="geometry")) + the step.  The colour stage is left out of (h), which only flatters it.
Every round times all three, the order reversed in odd rounds.  Accepted when every round of (a) is below every round of (h).
cpx_blur_pool_rects_u8 is also timed alone on the blurred crops of the rounds' draws with their own colour modes and parameters,
and once with every one of the `--crops` windows blurred at radius 8: every argument is uploaded beforehand, two device events
bracket 20 back-to-back calls of the C entry (its 4-byte status memset and the kernel, nothing else), the median of 7 such
brackets divided by 20.  The same through the debug library at a 64 x 64 tile (cpx_blur_set_tile) beside the product's 32 x 32.
"""
import argparse
import dataclasses
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from classpose_amd import _lib, augment, ops, synth
from classpose_amd.train import HeadTrainer


def make_labels(n, size, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.kron(rng.integers(0, ncls, (n, size // 8, size // 8)), np.ones((1, 8, 8), np.int64)).astype(np.int16)
    for b in range(n):
        y0 = int(rng.integers(0, size - 56))
        lab[b, y0:y0 + 20] = -100
    return lab


def host_quality(images, g, cfg):
    """blur + HBS on whole host images as the reference computes them: scipy per channel, float32 HBS in numpy."""
    import quality_reference as qr
    from scipy.ndimage import gaussian_filter
    n = len(images)
    u_blur, sigma, u_hbs, hue, brightness, saturation = augment.sample_quality(g, n, cfg)
    out = np.empty_like(images)
    for t in range(n):
        x = images[t]
        if u_blur[t] <= cfg["gaussian_blur"]["probability"]:
            x = np.stack([gaussian_filter(x[..., c], sigma[t]) for c in range(3)], -1)
        if u_hbs[t] <= cfg["hbs"]["probability"]:
            x = qr.hbs_numpy(x, hue[t], 1.0 + brightness[t], saturation[t])
        out[t] = x
    return out


class BlurLaunch:
    """The arguments of one cpx_blur_pool_rects_u8 call, on the device before anything is timed."""

    def __init__(self, pool, idx, rects, radius, weights, colour):
        mode, sigma, bias, simple, params = colour
        dev, k = pool.device, len(idx)
        self.pool, self.k, self.simple = pool, k, int(bool(simple))
        self.max_h, self.max_w = int(rects[:, 2].max()), int(rects[:, 3].max())
        nbytes = 3 * rects[:, 2] * rects[:, 3]
        self.pixels = int(nbytes.sum()) // 3
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)      # noqa: E731
        self.image_of, self.rects, self.radius = up(idx, np.int32), up(rects, np.int32), up(radius, np.int32)
        self.weights, self.off = up(weights, np.float64), up(np.concatenate([[0], np.cumsum(nbytes)[:-1]]), np.int64)
        self.mode = up(mode, np.int32)
        self.sigma = up(np.zeros((k, 3)) if sigma is None else sigma, np.float32)
        self.bias = up(np.zeros((k, 3)) if bias is None else bias, np.float32)
        self.params = up(np.zeros((k, 14)) if params is None else params, np.float64)
        self.density = ops._stain_table(dev, "density")
        self.scratch = torch.empty(int(nbytes.sum()), dtype=torch.uint8, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.modes = np.bincount(np.asarray(mode), minlength=3).tolist()

    def __call__(self, L):
        pool, p = self.pool, _lib.ptr
        return L.cpx_blur_pool_rects_u8(p(pool.pool_u8), p(pool.px_off), p(pool.hw), len(pool), pool.pool_px, p(self.image_of),
                                        p(self.rects), p(self.radius), p(self.weights), p(self.off), self.k, self.max_h, self.max_w,
                                        p(self.sigma), p(self.bias), self.simple, p(self.params), p(self.density), p(self.mode),
                                        p(self.scratch), self.scratch.numel(), p(self.status), _lib.current_stream())

    def time(self, L, inner=20, reps=7):
        """median over ``reps`` of (device time of ``inner`` back-to-back calls) / inner, in ms"""
        for _ in range(3):
            _lib.check(self(L), "blur_pool_rects_u8")
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                self(L)
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b) / inner)
        return float(np.median(ts))


def take(p, m):
    """the BatchParams rows ``m`` (a boolean mask)"""
    return augment.BatchParams(*[None if v is None else v[m] for v in
                                 (getattr(p, f.name) for f in dataclasses.fields(augment.BatchParams))])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--crops", type=int, default=32)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--classes", type=int, default=7)
    ap.add_argument("--profile-steps", type=int, default=0, help="run this many hed_he_quality pool steps and exit (for rocprofv3)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n, nI, S, ncls = args.crops, args.images, args.size, args.classes
    backbone = synth.make_state_dict(1, None, depth=args.depth, seed=0)
    big = np.stack([synth.render_region(300, S * (k % 4), S * (k // 4), S, S) for k in range(nI)])
    big_lab = make_labels(nI, S, ncls, 7 + ncls)
    tr = HeadTrainer(dict(backbone), nclasses=ncls, device=dev, precision="bf16", feature_batch=n)
    pool = augment.ImagePool(list(big), list(big_lab), device=dev)
    pool.stain_basis()
    cfg = augment.get_config("hed_he_quality")
    lr = 1e-4
    order = np.random.default_rng(0)
    rng = {k: np.random.default_rng(1) for k in "aph"}
    blurred_per_step = []

    def batch_a(idx, g):
        return augment.augment_batch_pool(pool, idx, g, "hed_he_quality", dtype=tr.dtype)

    def batch_p(idx, g):
        return augment.augment_batch_pool(pool, idx, g, "hed_he", dtype=tr.dtype)

    def batch_h(idx, g):
        return augment.augment_batch(host_quality(big[idx], g, cfg), big_lab[idx], g, "geometry", dtype=tr.dtype, device=dev)
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
            if k == "a":                    # the count is taken outside the timed region
                c = np.random.default_rng()
                c.bit_generator.state = rng["a"].bit_generator.state
                p = augment.sample_batch_params_pool(pool, idx, c, cfg)
                b = augment.quality_params(p, cfg)
                rects, ok = augment.footprint_rects(p.inv, pool.hw_host[idx, 0], pool.hw_host[idx, 1])
                m = b[0] & ok
                colour = augment.pool_colour_args(pool, idx[m], take(p, m), cfg) if m.any() else None
                blurred_per_step.append((int(m.sum()), idx[m], rects[m], b[1][m], b[2][m], colour))
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fns[k](idx)
            torch.cuda.synchronize(); times[k].append((time.perf_counter() - t0) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    counts = [c[0] for c in blurred_per_step]
    launches = [BlurLaunch(pool, *c[1:]) for c in blurred_per_step if c[0]]
    # the worst case: every window of one more draw blurred at radius 8, with the colour stage the draw gave it
    idx_w = order.integers(0, nI, n)
    pw = augment.sample_batch_params_pool(pool, idx_w, np.random.default_rng(2), cfg)
    rects_w, ok_w = augment.footprint_rects(pw.inv, pool.hw_host[idx_w, 0], pool.hw_host[idx_w, 1])
    r8, w8 = augment.gauss_weights(2.0)
    nw = int(ok_w.sum())
    worst = BlurLaunch(pool, idx_w[ok_w], rects_w[ok_w], np.full(nw, r8), np.tile(w8, (nw, 1)),
                       augment.pool_colour_args(pool, idx_w[ok_w], take(pw, ok_w), cfg))
    kernel_ms = {}
    L = _lib.lib()
    kernel_ms[32] = [x.time(L) for x in launches + [worst]]
    with _lib.use_debug_library() as D:
        for tile in (32, 64):
            D.cpx_blur_set_tile(tile)
            kernel_ms[("debug", tile)] = [x.time(D) for x in launches + [worst]]
        D.cpx_blur_set_tile(32)
    lines = [f"bench_train_quality: {torch.cuda.get_device_name(0)}, {n} windows of 256^2 per step out of {nI} uint8 images of {S}^2, bf16, "
             f"{ncls} classes, ViT depth {args.depth}, {args.rounds} interleaved rounds, warmed up, medians (ms)"]
    for k, what in (("a", "pool step, hed_he_quality (colour stage, blur, HBS)            "),
                    ("p", "pool step, hed_he (the step before this feature)               "),
                    ("h", "blur (scipy) + HBS (numpy float32) on whole host images        ")):
        lines.append(f"  ({k}) {what} median {med[k]:9.3f}   {[round(x, 3) for x in times[k]]}")
    ok = max(times["a"]) < min(times["h"])
    lines.append(f"  (a) - (p) = {med['a'] - med['p']:.3f} ms ({100 * (med['a'] - med['p']) / med['p']:.1f} % of (p)), (h)/(a) = {med['h'] / med['a']:.1f}; "
                 f"every round of (a) below every round of (h): {ok}")
    lines.append(f"  blurred crops per step of (a): {counts} (mean {np.mean(counts):.2f}; expected 0.1 * 15/16 * {n} = {0.09375 * n:.1f})")
    lines.append("  cpx_blur_pool_rects_u8 alone, arguments resident, events around 20 back-to-back calls of the entry, median of 7 (ms per call):")
    lines.append(f"    requests per launch {[x.k for x in launches]} + worst case {worst.k}; footprint pixels {[x.pixels for x in launches]} + "
                 f"{worst.pixels}; colour modes [none, HED, H&E] {[x.modes for x in launches]} + {worst.modes}")
    for key, what in ((32, "product library, 32 x 32 tile"), (("debug", 32), "debug library,   32 x 32 tile"),
                      (("debug", 64), "debug library,   64 x 64 tile")):
        v = kernel_ms[key]
        lines.append(f"    {what}: steps {[round(x, 4) for x in v[:-1]]}, all {worst.k} windows at radius 8: {v[-1]:.4f}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
