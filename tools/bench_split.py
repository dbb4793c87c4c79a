"""Instance maps with merged touching cells -> split instance maps: the device chain (ops.split_touching -> cpx_split_touching)
against the same rule on the host, scipy's Euclidean transform per instance plus numpy; one process, interleaved rounds (order
reversed in odd rounds), medians with ranges.

    python tools/bench_split.py [--rounds 7] [--out profiles/split_bench.txt]
    python tools/bench_split.py --profile    # the device path alone, three calls per workload (for rocprofv3 --kernel-trace --stats)

Workloads: the class maps of tools/bench_label_components.py (seeded), labelled 8-connected by ops.label_components, so touching
cells of one class share an id: (a) 4096 x 256^2, (b) 64 x 1024^2, (c) 1 x 8192^2.  min_distance 5, min_radius 2, connectivity 8.
Paths, each from maps that are where the path works to labels and counts in the same place:
  (1) device   ops.split_touching, maps resident on the device (the call allocates its workspace and reads the status words back)
  (2) host     per instance (scipy.ndimage.find_objects, one pixel of margin) ``distance_transform_edt`` squared and rounded; the
               seeds by a maximum filter over a key that orders (D2, earlier raster index); every pixel of an instance with two or
               more seeds to its nearest seed; the pieces labelled per value and numbered by their first raster pixel.  Maps in
               host memory.  (a): the first 64 maps, scaled by 64; (b): the first 2 maps, scaled by 32; (c): the top 512 rows,
               scaled by 16
Before anything is timed (1) is compared with (2) on every pixel of the host's part, and with tests/split_reference on one map.
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

import split_reference as sr
from bench_label_components import timed, workloads
from classpose_amd import ops

MIN_DISTANCE, MIN_RADIUS, CONNECTIVITY = 5, 2, 8
HOST_PART = {"(a)": (64, None), "(b)": (2, None), "(c)": (1, 512)}              # images, rows


def _grown(sl, shape, by):
    return tuple(slice(max(0, s.start - by), min(n, s.stop + by)) for s, n in zip(sl, shape))


def _number_by_first_pixel(comp, total):
    flat = comp.ravel()
    fg = np.flatnonzero(flat)
    ids, first = np.unique(flat[fg], return_index=True)
    rank = np.zeros(total + 1, np.int64)
    rank[ids[np.argsort(fg[first], kind="stable")]] = np.arange(1, total + 1)
    return rank[comp].astype(np.int32)


def host_split_image(m: np.ndarray):
    from scipy import ndimage
    H, W = m.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    prov = np.zeros((H, W), np.int64)
    n_prov = 0
    for v, sl in enumerate(ndimage.find_objects(m), 1):
        if sl is None:
            continue
        box = _grown(sl, (H, W), 1)                                             # the margin holds other values: sites
        mask = m[box] == v
        d2 = np.rint(ndimage.distance_transform_edt(mask) ** 2).astype(np.int64) if not mask.all() else np.full(mask.shape, H * H + W * W)
        key = np.where(mask, d2 * (H * W) + (H * W - 1 - idx[box]), -1)         # larger D2 first, then the earlier pixel
        top = ndimage.maximum_filter(key, size=2 * MIN_DISTANCE + 1, mode="constant", cval=-1)
        sy, sx = np.nonzero((top == key) & mask & (d2 >= MIN_RADIUS * MIN_RADIUS))
        if len(sy) < 2:
            prov[box][mask] = n_prov + 1
            n_prov += 1
            continue
        py, px = np.nonzero(mask)
        near = np.argmin((py[:, None] - sy[None, :]) ** 2 + (px[:, None] - sx[None, :]) ** 2, axis=1)
        prov[box][mask] = n_prov + 1 + near
        n_prov += len(sy)
    structure = np.ones((3, 3), bool) if CONNECTIVITY == 8 else None
    comp = np.zeros((H, W), np.int64)
    total = 0
    for v, sl in enumerate(ndimage.find_objects(prov.astype(np.int32)), 1):
        if sl is None:
            continue
        lab, k = ndimage.label(prov[sl] == v, structure=structure)
        comp[sl][lab > 0] = lab[lab > 0] + total
        total += k
    return _number_by_first_pixel(comp, total), total


def host_split(maps: np.ndarray):
    res = [host_split_image(m) for m in maps]
    return np.stack([r[0] for r in res]), np.asarray([r[1] for r in res], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="(a) with 1024 maps, (c) at 2048^2 (a quick look)")
    ap.add_argument("--profile", action="store_true", help="run the device path three times per workload and nothing else")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    lines = [f"bench_split: {torch.cuda.get_device_name(0)}, min_distance {MIN_DISTANCE}, min_radius {MIN_RADIUS}, connectivity {CONNECTIVITY}, "
             f"{args.rounds} interleaved rounds, order reversed in odd rounds, one warm-up call of every path first; ms per call, median [min .. max]"]
    for name, classes, _scale, _rows in workloads(dev, args.small):
        inst, before = ops.label_components(classes, CONNECTIVITY)
        del classes
        n, H, W = inst.shape
        device = lambda: ops.split_touching(inst, MIN_DISTANCE, MIN_RADIUS, CONNECTIVITY)
        if args.profile:
            for _ in range(3):
                device()
            sync()
            continue
        images, rows = HOST_PART[name[:3]]
        images = min(images, n)
        part = inst[:images] if rows is None else inst[:, :min(rows, H)]
        scale = n * H * W / part.numel()
        if rows is not None:                                                    # a part of an image: its own components, cut at the edge
            part, _ = ops.label_components(part.contiguous(), CONNECTIVITY)
        host_maps = part.cpu().numpy()
        labels, counts = device()                                               # these calls are the warm-up, and the comparison
        want, want_counts = host_split(host_maps)
        got, got_counts = ops.split_touching(part.contiguous(), MIN_DISTANCE, MIN_RADIUS, CONNECTIVITY)
        assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_counts.cpu().numpy(), want_counts), "the device differs from the host formulation"
        crop = host_maps[0][:256, :256]
        ref = sr.split_image(crop, MIN_DISTANCE, MIN_RADIUS, CONNECTIVITY)
        one = ops.split_touching(torch.from_numpy(np.ascontiguousarray(crop)).to(dev)[None], MIN_DISTANCE, MIN_RADIUS, CONNECTIVITY)
        assert np.array_equal(one[0][0].cpu().numpy(), ref[0]) and int(one[1][0]) == ref[1], "the device differs from the restatement"
        del got, one
        paths = {"1": device, "2": lambda: host_split(host_maps)}
        times = {k: [] for k in paths}
        for rnd in range(args.rounds):
            for k in (("1", "2") if rnd % 2 == 0 else ("2", "1")):
                t = timed(paths[k], sync, min_window=0.25 if k == "1" else 0.0)
                times[k].append(t * (scale if k == "2" else 1.0))
        fmt = lambda v: f"{np.median(v):11.3f} [{min(v):.3f} .. {max(v):.3f}]"
        lines += [f"{name}: {int(before.sum())} components -> {int(counts.sum())} instances, {int((inst != 0).sum())} of {n * H * W} pixels foreground",
                  f"  (1) device, ops.split_touching         {fmt(times['1'])}   ({n * H * W / np.median(times['1']) / 1e6:.2f} Gpixel/s)",
                  f"  (2) host, scipy EDT per instance + numpy {fmt(times['2'])}   (timed on 1/{scale:g} of the pixels, scaled by {scale:g})",
                  f"  every round of (1) below every round of (2): {max(times['1']) < min(times['2'])}; ratio of medians (2)/(1) = "
                  f"{np.median(times['2']) / np.median(times['1']):.1f}"]
        del labels, inst
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
