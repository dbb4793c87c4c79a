"""Value maps -> instance maps: the device labeller (ops.label_components -> cpx_label_components) against scipy on the host and an
eager PyTorch formulation on the same GPU; one process, interleaved rounds (order reversed in odd rounds), medians with ranges.

    python tools/bench_label_components.py [--rounds 7] [--out profiles/label_components_bench.txt]
    python tools/bench_label_components.py --profile    # the device path alone, three calls per workload (for rocprofv3 --kernel-trace --stats)

Workloads (seeded), 8-connected, every path from maps that are where the path works to labels and counts in the same place:
  (a) 4096 class maps of 256^2 with about 100 cells of 7 classes each (64 distinct maps, each in 64 flips / shifts);
  (b) 64 class maps of 1024^2 with about 1 600 cells each;
  (c) one class map of 8192^2 made by ops.rasterize_polygons: a few hundred thousand cells, painted with their class.
Paths:
  (1) device   ops.label_components with a reused workspace, maps resident on the device
  (2) scipy    scipy.ndimage.label per distinct non-zero value with the full structure and an offset per value (NO renumbering into
               raster order, which (1) and (3) deliver: in scipy's favour), maps in host memory.  (a): the first 256 maps, scaled by
               16; (b): the first 16 maps, scaled by 4; (c): the top 2048 rows, scaled by 4
  (3) eager    PyTorch on the same GPU: labels = linear index, then repeatedly the minimum over the 3 x 3 neighbours of equal value
               (masks computed once) until nothing changes (checked every 4th sweep), then torch.unique(return_inverse=True) for the
               per-image ranks
Before anything is timed (1) is compared with (3) on every pixel and with tests/components_reference.label_scipy on a part.
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

import components_reference as cr
from classpose_amd import _lib, ops

STEPS8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def cell_rings(rng, centres, classes, r_lo=5.0, r_hi=10.0, nv=12):
    """12-gons around ``centres`` (n, 2), quantised to 1/16 -> (xy, ring_off, ring_value = class)"""
    n = len(centres)
    th = 2 * np.pi * np.arange(nv) / nv
    r = rng.uniform(r_lo, r_hi, n)[:, None] * (1 + 0.15 * np.sin(3 * th[None] + rng.uniform(0, 6.28, n)[:, None]))
    xy = centres[:, None, :] + np.stack([r * np.cos(th), 0.85 * r * np.sin(th)], -1)
    return np.round(xy.reshape(-1, 2) * 16) / 16, np.arange(n + 1, dtype=np.int64) * nv, classes.astype(np.int32)


def class_maps(seed, n_images, size, cells_per_image, dev):
    rng = np.random.default_rng(seed)
    n = n_images * cells_per_image
    xy, off, val = cell_rings(rng, rng.uniform(0, size, (n, 2)), rng.integers(1, 8, n))
    image = np.repeat(np.arange(n_images, dtype=np.int32), cells_per_image)
    return ops.rasterize_polygons(xy, off, val, (size, size), ring_image=image, n_images=n_images, device=dev)


def workloads(dev, small):
    base = class_maps(1, 64, 256, 100, dev)
    parts = []
    for k in range(16 if small else 64):
        m = base.roll((37 * k) % 256, 2).roll((91 * k) % 256, 1)
        parts.append(m.flip(2) if k & 1 else m)
    yield "(a) %d x 256^2, about 100 cells of 7 classes each" % (64 * len(parts)), torch.cat(parts).contiguous(), 16, None
    yield "(b) 64 x 1024^2, about 1600 cells each", class_maps(2, 64, 1024, 1600, dev), 4, None
    size = 2048 if small else 8192
    yield f"(c) 1 x {size}^2 from ops.rasterize_polygons, {(size // 15) ** 2} cells", class_maps(3, 1, size, (size // 15) ** 2, dev), 1, size // 4


def scipy_label(maps: np.ndarray):
    from scipy import ndimage
    structure = np.ones((3, 3), bool)
    out = np.zeros(maps.shape, np.int32)
    counts = np.zeros(len(maps), np.int32)
    for i, m in enumerate(maps):
        total = 0
        for v in np.unique(m):
            if v == 0:
                continue
            lab, k = ndimage.label(m == v, structure=structure)
            out[i][lab > 0] = lab[lab > 0] + total
            total += k
        counts[i] = total
    return out, counts


class Eager:
    def __init__(self, m: torch.Tensor):
        self.m = m
        n, H, W = m.shape
        self.pairs = []
        for dy, dx in STEPS8:
            ya, yb = (slice(max(0, -dy), H - max(0, dy)), slice(max(0, dy), H - max(0, -dy)))
            xa, xb = (slice(max(0, -dx), W - max(0, dx)), slice(max(0, dx), W - max(0, -dx)))
            a, b = (slice(None), ya, xa), (slice(None), yb, xb)
            if m[a].numel():
                self.pairs.append((a, b, (m[a] == m[b]) & (m[a] != 0)))
        self.sweeps = 0

    def __call__(self):
        m = self.m
        n, H, W = m.shape
        HW = H * W
        big = torch.tensor(HW, dtype=torch.int32, device=m.device)
        lab = torch.where(m != 0, torch.arange(HW, dtype=torch.int32, device=m.device).view(1, H, W), big)
        sweeps = 0
        while True:
            for _ in range(4):
                new = lab.clone()
                for a, b, eq in self.pairs:
                    new[a] = torch.minimum(new[a], torch.where(eq, lab[b], big))
                prev, lab = lab, new
                sweeps += 1
            if torch.equal(prev, lab):
                break
        self.sweeps = sweeps
        stride = HW + 1
        keys = lab.to(torch.int64) + torch.arange(n, device=m.device).view(n, 1, 1) * stride
        uniq, inv = torch.unique(keys, return_inverse=True)
        img = uniq // stride
        is_bg = uniq % stride == HW
        first = torch.searchsorted(uniq, torch.arange(n, device=m.device) * stride)
        rank = torch.arange(len(uniq), device=m.device) - first[img] + 1
        rank[is_bg] = 0
        counts = torch.bincount(img[~is_bg], minlength=n)
        return rank[inv].to(torch.int32), counts.to(torch.int32)


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
    ap.add_argument("--small", action="store_true", help="(a) with 1024 maps, (c) at 2048^2 (a quick look)")
    ap.add_argument("--profile", action="store_true", help="run the device path three times per workload and nothing else")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = [f"bench_label_components: {torch.cuda.get_device_name(0)}, connectivity 8, {args.rounds} interleaved rounds, order reversed in odd "
             "rounds, one warm-up call of every path first; ms per call, median [min .. max]"]
    for name, maps, scipy_scale, scipy_rows in workloads(dev, args.small):
        n, H, W = maps.shape
        ws = torch.empty(_lib.lib().cpx_label_components_workspace_bytes(n, H, W), dtype=torch.uint8, device=dev)
        device = lambda: ops.label_components(maps, 8, workspace=ws)
        if args.profile:
            for _ in range(3):
                device()
            sync()
            continue
        host_maps = (maps[:max(1, n // scipy_scale)] if scipy_rows is None else maps[:, :scipy_rows]).cpu().numpy()
        scale = scipy_scale if scipy_rows is None else H / scipy_rows
        eager = Eager(maps)
        labels, counts = device()                                    # these three calls are the warm-up, and the comparison
        elab, ecnt = eager()
        assert torch.equal(labels, elab) and torch.equal(counts, ecnt), "the device differs from the eager formulation"
        part = host_maps[0]
        want, wn = cr.label_scipy(part, 8)
        got = ops.label_components(torch.from_numpy(part).to(dev)[None], 8)
        assert np.array_equal(got[0][0].cpu().numpy(), want) and int(got[1][0]) == wn, "the device differs from the scipy statement of the rule"
        scipy_label(host_maps[:1])
        del elab, got
        paths = {"1": device, "2": lambda: scipy_label(host_maps), "3": eager}
        times = {k: [] for k in paths}
        for rnd in range(args.rounds):
            for k in (("1", "2", "3") if rnd % 2 == 0 else ("3", "2", "1")):
                t = timed(paths[k], sync, min_window=0.25 if k == "1" else 0.0)
                times[k].append(t * (scale if k == "2" else 1.0))
        fmt = lambda v: f"{np.median(v):11.3f} [{min(v):.3f} .. {max(v):.3f}]"
        fg = int((maps != 0).sum())
        lines += [f"{name}: {int(counts.sum())} components, {fg} of {n * H * W} pixels foreground, workspace {ws.numel() / 2 ** 20:.1f} MiB",
                  f"  (1) device, ops.label_components   {fmt(times['1'])}   ({n * H * W / np.median(times['1']) / 1e6:.2f} Gpixel/s)",
                  f"  (2) scipy.ndimage.label per value  {fmt(times['2'])}" + (f"   (timed on 1/{scale:g} of the pixels, scaled by {scale:g})" if scale != 1 else ""),
                  f"  (3) eager PyTorch, same GPU        {fmt(times['3'])}   ({eager.sweeps} sweeps)",
                  f"  every round of (1) below every round of (2): {max(times['1']) < min(times['2'])}; of (3): {max(times['1']) < min(times['3'])}; "
                  f"ratio of medians (2)/(1) = {np.median(times['2']) / np.median(times['1']):.1f}, (3)/(1) = {np.median(times['3']) / np.median(times['1']):.1f}"]
        del eager, labels, maps, ws
        torch.cuda.empty_cache()
    if args.profile:
        return
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
