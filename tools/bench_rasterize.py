"""Polygon rings -> instance maps: the device rasteriser (ops.rasterize_polygons -> cpx_rasterize_polygons) against host
formulations on the same machine; one process, interleaved rounds (order reversed in odd rounds), medians with ranges.

    python tools/bench_rasterize.py [--rounds 7] [--out profiles/rasterize_bench.txt]
    python tools/bench_rasterize.py --profile      # the device path alone, three calls per workload (for rocprofv3 --kernel-trace --stats)

Workloads (seeded, coordinates in sixteenths):
  (a) eight 1024^2 images with about 1 300 cells each (the density of the README's post-processing line), 20 to 60 vertices per cell;
  (b) one 8192^2 image with a few hundred thousand such cells plus four outline rings of about 5 000 vertices that span most of it.
Paths, each ending with the int32 maps on the DEVICE (host paths: in host memory; no copy back is counted for anyone):
  (1) device, resident   vertices, offsets and values already on the device -> zeroed maps + ops.rasterize_polygons (its argument
                         checks, which synchronise once, are part of the call)
  (2) device, upload     the same from host arrays: (1) plus the upload
  (3) PIL                PIL.ImageDraw.polygon per ring into a mode "I" image: a C scan-line rasteriser with a DIFFERENT edge rule,
                         here for speed only, its pixels are not compared
  (4) numpy              the exact restatement of the rule (tests/rasterize_reference.py, float64 version) on a subset of the rings,
                         scaled to all of them; three rounds
Before anything is timed the device maps are compared with (4) on that subset for equality.
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

import rasterize_reference as rr
from classpose_amd import ops


def make_cells(rng, centres, r_lo=6.0, r_hi=11.0):
    """wobbly closed curves around ``centres`` (n, 2): (xy, ring_off) with 20..60 vertices each, quantised to 1/16"""
    n = len(centres)
    nv = rng.integers(20, 61, n)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(nv)
    ring = np.repeat(np.arange(n), nv)
    k = np.arange(off[-1]) - off[ring]
    th = 2 * np.pi * k / nv[ring]
    r = rng.uniform(r_lo, r_hi, n)[ring] * (1 + 0.2 * np.sin(3 * th + rng.uniform(0, 6.28, n)[ring]))
    xy = centres[ring] + np.stack([r * np.cos(th), 0.8 * r * np.sin(th)], 1)
    return rr.q16(xy), off


def outline(rng, cx, cy, radius, n=5000):
    th = 2 * np.pi * np.arange(n) / n
    r = radius * (1 + 0.08 * np.sin(7 * th + rng.uniform(0, 6.28)) + 0.01 * rng.uniform(-1, 1, n))
    return rr.q16(np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1))


def workload_a(seed=1):
    rng = np.random.default_rng(seed)
    xs, counts, images = [], [], []
    for i in range(8):
        xy, off = make_cells(rng, rng.uniform(0, 1024, (1300, 2)))
        xs.append(xy); counts.append(np.diff(off)); images.append(np.full(1300, i, np.int32))
    counts = np.concatenate(counts)
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return dict(name="(a) 8 x 1024^2, 1300 cells each", xy=np.concatenate(xs), off=off, value=np.arange(1, len(counts) + 1, dtype=np.int32),
                image=np.concatenate(images), n_images=8, shape=(1024, 1024), first_cell=0)


def workload_b(seed=2, size=8192, pitch=15):
    rng = np.random.default_rng(seed)
    g = np.arange(pitch // 2, size, pitch, dtype=np.float64)
    centres = np.stack(np.meshgrid(g, g), -1).reshape(-1, 2) + rng.uniform(-3, 3, (len(g) ** 2, 2))
    outlines = [outline(rng, cx, cy, rad) for cx, cy, rad in ((2100, 2100, 1900), (6000, 2200, 1900), (2200, 6000, 1950), (5900, 5900, 2000))]
    cxy, coff = make_cells(rng, centres)
    xy = np.concatenate(outlines + [cxy])
    counts = np.concatenate([[len(o) for o in outlines], np.diff(coff)])
    off = np.zeros(len(counts) + 1, np.int64)
    off[1:] = np.cumsum(counts)
    return dict(name=f"(b) 1 x {size}^2, {len(centres)} cells + 4 outlines of 5000 vertices", xy=xy, off=off,
                value=np.arange(1, len(counts) + 1, dtype=np.int32), image=None, n_images=1, shape=(size, size), first_cell=4)


def pil_maps(w):
    from PIL import Image, ImageDraw
    H, W = w["shape"]
    ims = [Image.new("I", (W, H), 0) for _ in range(w["n_images"])]
    draws = [ImageDraw.Draw(im) for im in ims]
    xy, off, val, img = w["xy"], w["off"], w["value"], w["image"]
    flat = xy.ravel()
    for k in range(len(val)):
        draws[0 if img is None else img[k]].polygon(flat[2 * off[k]:2 * off[k + 1]].tolist(), fill=int(val[k]))
    return ims


def subset(w, n=200):
    """the first n cells of image 0 (and for (b) the rows they touch): (xy, off, value) for the numpy restatement"""
    k0 = w["first_cell"]
    off = w["off"][k0:k0 + n + 1]
    return w["xy"][off[0]:off[-1]], off - off[0], w["value"][k0:k0 + n]


def timed(fn, sync, min_window=0.25):
    """ms per call over a window of at least min_window seconds"""
    sync(); t0 = time.perf_counter(); fn(); sync()
    once = time.perf_counter() - t0
    if once >= min_window:
        return once * 1e3
    reps = max(1, int(min_window / max(once, 1e-6)))
    sync(); t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="(b) at 2048^2 (a quick look)")
    ap.add_argument("--profile", action="store_true", help="run the device path three times per workload and nothing else")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = [f"bench_rasterize: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds, order reversed in odd rounds; ms per call, "
             "median [min .. max]"]
    for w in (workload_a(), workload_b(size=2048) if args.small else workload_b()):
        H, W = w["shape"]
        d = {k: None if w[k] is None else torch.from_numpy(w[k]).to(dev) for k in ("xy", "off", "value", "image")}
        resident = lambda: ops.rasterize_polygons(d["xy"], d["off"], d["value"], (H, W), ring_image=d["image"], n_images=w["n_images"])
        upload = lambda: ops.rasterize_polygons(w["xy"], w["off"], w["value"], (H, W), ring_image=w["image"], n_images=w["n_images"], device=dev)
        if args.profile:
            for _ in range(3):
                resident()
            sync()
            continue
        # equality with the numpy restatement on the subset, painted alone
        sxy, soff, sval = subset(w)
        want = rr.rasterize(sxy, soff, sval, (H, W), masks=rr.ring_masks_float)[0]
        got = ops.rasterize_polygons(sxy, soff, sval, (H, W), device=dev)[0].cpu().numpy()
        assert np.array_equal(got, want), "the device differs from the numpy restatement"
        full = resident()
        assert np.array_equal(upload().cpu().numpy(), full.cpu().numpy())
        painted = int((full > 0).sum())
        paths = {"1": resident, "2": upload, "3": lambda: pil_maps(w)}
        times = {k: [] for k in ("1", "2", "3", "4")}
        for rnd in range(args.rounds):
            for k in (("1", "2", "3") if rnd % 2 == 0 else ("3", "2", "1")):
                times[k].append(timed(paths[k], sync))
        scale = (len(w["value"]) - w["first_cell"]) / len(sval)
        for _ in range(3):
            t0 = time.perf_counter()
            rr.rasterize(sxy, soff, sval, (H, W), masks=rr.ring_masks_float)
            times["4"].append((time.perf_counter() - t0) * 1e3 * scale)
        fmt = lambda v: f"{np.median(v):10.3f} [{min(v):.3f} .. {max(v):.3f}]"
        n_rings, n_vert = len(w["value"]), len(w["xy"])
        lines += [f"{w['name']}: {n_rings} rings, {n_vert} vertices, {painted} of {w['n_images'] * H * W} pixels painted",
                  f"  (1) device, vertices resident   {fmt(times['1'])}",
                  f"  (2) device, with the upload     {fmt(times['2'])}",
                  f"  (3) PIL.ImageDraw per ring      {fmt(times['3'])}   (another edge rule: speed only)",
                  f"  (4) numpy restatement           {fmt(times['4'])}   ({len(sval)} cells timed, scaled by {scale:.1f}; cells only)",
                  f"  ratio of medians (1)/(3) = {np.median(times['1']) / np.median(times['3']):.5f}, (2)/(3) = "
                  f"{np.median(times['2']) / np.median(times['3']):.5f}; slowest (2) {max(times['2']):.3f} ms, fastest (3) {min(times['3']):.3f} ms"]
    if args.profile:
        return
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
