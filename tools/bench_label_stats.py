"""Dataset statistics of training crops: the hand-written device pass against the same formulation in eager PyTorch on the same
GPU and against the reference's formulation in numpy on the host; one process, interleaved rounds, medians (the style of
tools/bench_pq.py and tools/bench_train_augment.py).

    python tools/bench_label_stats.py [--rounds 9] [--out profiles/label_stats_bench.txt]
    python tools/bench_label_stats.py --profile        # the device path alone, three times (to run under rocprofv3 --kernel-trace --stats)

Workload: 4096 crops of 256^2, 7 classes, about 100 rectangular cells per crop with random non-contiguous ids below 2 * 10^9, a
-100 box per crop; 256 distinct crops repeated 16 times (building them is host work; the work per crop does not depend on that).
Every path starts from DEVICE-resident maps (int32 ids, int16 classes) and ends with class counts, per-image instance counts,
mask counts and float64 diameters on the HOST.
  (a) device   dataset_stats.label_stats (cpx_label_stats, chunks of 1024 crops)
  (b) eager    torch.unique on packed 64-bit keys (image, id) and (image, class, id), bincount / scatter_add, a sort for the medians,
               in chunks of 1024 crops too: what one would write without a kernel
  (c) numpy    the reference's formulation on the host, per image: n_classes np.unique(inst[cls == j]) calls, one np.bincount and
               one np.unique(return_counts=True).  Timed on the 256 distinct crops (from host arrays, no copy counted) and scaled by
               16, three rounds: it is two orders of magnitude away and does not need nine.
(a) and (b) are compared with (c) for equality before anything is timed.  Every round times (a) and (b), the order alternating.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from classpose_amd import dataset_stats

NCLS = 7


def make_maps(seed, n, size=256, n_cells=100):
    rng = np.random.default_rng(seed)
    inst = np.zeros((n, size, size), np.int32)
    cls = np.zeros((n, size, size), np.int16)
    for i in range(n):
        ids = rng.permutation(np.unique(rng.integers(1, 2_000_000_000, size=2 * n_cells)))[:n_cells]
        for k in range(n_cells):
            y0, x0 = int(rng.integers(0, size - 8)), int(rng.integers(0, size - 8))
            h, w = int(rng.integers(6, 30)), int(rng.integers(6, 30))
            inst[i, y0:y0 + h, x0:x0 + w] = ids[k]
            cls[i, y0:y0 + h, x0:x0 + w] = 1 + ids[k] % (NCLS - 1)
        y0, x0 = int(rng.integers(0, size - 40)), int(rng.integers(0, size - 40))
        cls[i, y0:y0 + 40, x0:x0 + 30] = -100
    return inst, cls


def eager_stats(inst, cls, ncls, chunk=1024):
    """The statistics of dataset_stats.label_stats from device maps, in eager PyTorch."""
    dev = inst.device
    N = inst.shape[0]
    px_all, ipc_all, m_all, mid_all = [], [], [], []
    for lo in range(0, N, chunk):
        i = inst[lo:lo + chunk].long().flatten(1)
        c = cls[lo:lo + chunk].long().flatten(1)
        n = i.shape[0]
        img = torch.arange(n, device=dev)[:, None]
        valid = c >= 0
        ic = (img * ncls + c)[valid]
        px_all.append(torch.bincount(ic, minlength=n * ncls).view(n, ncls))
        u2 = torch.unique((ic << 32) | i[valid])
        ipc_all.append(torch.bincount(u2 >> 32, minlength=n * ncls).view(n, ncls))
        uk, counts = torch.unique(((img << 32) | i).flatten(), return_counts=True)      # sorted: per image, ids ascending
        uimg = uk >> 32
        nids = torch.bincount(uimg, minlength=n)
        first = torch.cumsum(nids, 0) - nids
        keep = torch.ones_like(uk, dtype=torch.bool)
        keep[first[nids > 0]] = False                                                     # counts[1:]: the smallest id of each image
        m = torch.clamp(nids - 1, min=0)
        srt = torch.sort((uimg[keep] << 32) | counts[keep]).values & 0xffffffff           # areas ascending inside each image
        start = torch.cumsum(m, 0) - m
        has = m > 0
        pad = torch.cat([srt, torch.zeros(1, dtype=srt.dtype, device=dev)])
        a0 = torch.where(has, pad[torch.where(has, start + (m - 1) // 2, 0)], 0)
        a1 = torch.where(has, pad[torch.where(has, start + m // 2, 0)], 0)
        m_all.append(m); mid_all.append(torch.stack([a0, a1], 1))
    px, ipc, m, mid = (torch.cat(x).cpu().numpy() for x in (px_all, ipc_all, m_all, mid_all))
    return dataset_stats.LabelStats(px.sum(0), ipc.astype(np.float64), m, dataset_stats.diameters_from_mid_areas(mid))


def numpy_stats(inst, cls, ncls):
    """train_utils.get_class_counts / get_instance_counts and cellpose.utils.diameters, as the reference runs them on the host."""
    labels = np.concatenate([c.ravel() for c in cls]).astype(np.int64, copy=False)
    class_counts = np.bincount(labels[labels >= 0], minlength=ncls)
    counts = np.zeros((len(inst), ncls))
    n_masks, diam = np.zeros(len(inst), np.int64), np.zeros(len(inst))
    for i in range(len(inst)):
        for j in range(ncls):
            counts[i, j] = np.unique(inst[i][cls[i] == j]).size
        a = np.unique(inst[i], return_counts=True)[1][1:]
        n_masks[i] = a.size
        diam[i] = np.median(a ** 0.5) / (np.pi ** 0.5 / 2) if a.size else 0.0
    return dataset_stats.LabelStats(class_counts, counts, n_masks, diam)


def same(x, y, repeat=1):
    return (np.array_equal(x.class_counts, y.class_counts * repeat) and np.array_equal(x.instance_counts, np.tile(y.instance_counts, (repeat, 1)))
            and np.array_equal(x.n_masks, np.tile(y.n_masks, repeat)) and np.allclose(x.diameters, np.tile(y.diameters, repeat), rtol=1e-15, atol=0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/16 of the crops (a quick look)")
    ap.add_argument("--profile", action="store_true", help="run the device path three times and nothing else")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    distinct, repeat = (16, 16) if args.small else (256, 16)
    inst_h, cls_h = make_maps(1234, distinct)
    inst = torch.from_numpy(inst_h).to(dev).repeat(repeat, 1, 1)
    cls = torch.from_numpy(cls_h).to(dev).repeat(repeat, 1, 1)
    fa = lambda: dataset_stats.label_stats(inst, cls, NCLS, device=dev, chunk=1024)
    fb = lambda: eager_stats(inst, cls, NCLS)
    if args.profile:
        for _ in range(3):
            fa()
        torch.cuda.synchronize()
        return
    ref = numpy_stats(inst_h, cls_h, NCLS)
    ra, rb = fa(), fb()                                     # warm-up, and the comparison
    assert same(ra, ref, repeat), "the device path differs from the numpy formulation"
    assert same(rb, ref, repeat), "the eager formulation differs from the numpy formulation"
    fa(); fb()
    times = {"a": [], "b": [], "c": []}
    for rnd in range(args.rounds):
        for which in (("a", "b") if rnd % 2 == 0 else ("b", "a")):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            (fa if which == "a" else fb)()
            torch.cuda.synchronize(); times[which].append((time.perf_counter() - t0) * 1e3)
    for _ in range(3):
        t0 = time.perf_counter()
        numpy_stats(inst_h, cls_h, NCLS)
        times["c"].append((time.perf_counter() - t0) * 1e3 * repeat)
    med = lambda v: float(np.median(v))
    ma, mb, mc = med(times["a"]), med(times["b"]), med(times["c"])
    n = inst.shape[0]
    lines = [f"bench_label_stats: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds, {n} crops of 256^2, {NCLS} classes, "
             f"{int(ra.n_masks.min())}..{int(ra.n_masks.max())} cells per crop (median {int(np.median(ra.n_masks))}), device maps -> LabelStats on the host",
             f"  (a) device dataset_stats.label_stats   median {ma:9.2f} ms   {[round(x, 2) for x in times['a']]}",
             f"  (b) eager torch.unique / bincount      median {mb:9.2f} ms   {[round(x, 2) for x in times['b']]}",
             f"  (c) numpy per image on the host        median {mc:9.2f} ms   {[round(x, 1) for x in times['c']]}   ({distinct} crops timed, x {repeat})",
             f"  ratio of medians (a)/(b) = {ma / mb:.4f}; rounds with (a) first {med(times['a'][0::2]) / med(times['b'][0::2]):.4f}, "
             f"rounds with (b) first {med(times['a'][1::2]) / med(times['b'][1::2]):.4f}; (a)/(c) = {ma / mc:.5f}; per crop (a) {ma / n * 1e3:.2f} us",
             f"  every round of (a) below every round of (b): {max(times['a']) < min(times['b'])} (max (a) {max(times['a']):.2f} ms, min (b) {min(times['b']):.2f} ms)"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
