"""Panoptic-quality statistics: the hand-written device path against the same formulation in eager PyTorch, one process,
interleaved rounds, medians (the style of tools/ab_*.py).

    python tools/bench_pq.py [--rounds 9] [--out profiles/pq_bench.txt]

Workloads (classpose_amd.synth: truth = the analytic nuclei of a region, class = nucleus identity mod classes; prediction = the
truth shifted by (1, 2) pixels with every 9th nucleus missed and every 7th given the next class):
    A  4096 images of 256^2, 7 classes      B  64 images of 1024^2, 10 classes
Rendering is host work, so A is 256 distinct regions repeated 16 times and B 8 regions repeated 8 times; the work per image
does not depend on that.
  (a) device   ops.pq_stats: device-resident int32 ids + uint8 classes -> tp / fp / fn / iou_sum on the host
  (b) eager    the same pair-table formulation with torch.unique(return_counts=True) on 64-bit keys and scatter_add on the
               same GPU, also ending with the statistics on the host: what one would write without a kernel
Both run the unlabelled-cell filter and no border removal, match_iou 0.5.  Their counts are compared before anything is timed.
Every round times both, the order alternating between rounds; the ratio of medians is reported for each order separately too.
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from classpose_amd import ops, synth


def render(seed, size, n_distinct, repeat, nr):
    gts, prs = [], []
    for k in range(n_distinct):
        owner, _cx, _cy, _r, ident = synth._owner_map(seed, k * size, (k % 7) * size, size, size)[:5]
        ids = (owner + 1).astype(np.int32)
        cls_of = np.concatenate([[0], (ident % nr + 1)]).astype(np.uint8)
        g_cls = cls_of[ids]
        p_ids, p_cls = np.roll(ids, (1, 2), (0, 1)), np.roll(g_cls, (1, 2), (0, 1))
        p_cls = np.where((p_ids % 7 == 3) & (p_ids > 0), p_cls % nr + 1, p_cls).astype(np.uint8)
        miss = (p_ids % 9 == 4)
        p_ids, p_cls = np.where(miss, 0, p_ids).astype(np.int32), np.where(miss, 0, p_cls).astype(np.uint8)
        gts.append((ids, g_cls)); prs.append((p_ids, p_cls))
    st = lambda xs, j: np.concatenate([np.stack([x[j] for x in xs])] * repeat)
    return st(gts, 0), st(gts, 1), st(prs, 0), st(prs, 1)


def eager_pq(t, p, ct, cp, nr, match_iou):
    """(n, H, W) device maps -> tp, fp, fn (n, nr) int64 and iou_sum float64 on the host; pair tables by torch.unique on 64-bit keys"""
    n = t.shape[0]
    M = int(torch.maximum(t.max(), p.max()).item()) + 1
    t, p, ct, cp = t.long().flatten(), p.long().flatten(), ct.long().flatten(), cp.long().flatten()
    img = torch.arange(n, device=t.device).repeat_interleave(t.numel() // n)
    one = torch.ones_like(t)
    # unlabelled true cells and the predictions matching them (class-agnostic IoU > 0.5)
    it, ip = img * M + t, img * M + p
    area_t = torch.zeros(n * M, dtype=torch.long, device=t.device).scatter_add_(0, it, one)
    area_p = torch.zeros(n * M, dtype=torch.long, device=t.device).scatter_add_(0, ip, one)
    lab = torch.zeros(n * M, dtype=torch.long, device=t.device).scatter_add_(0, it, (ct > 0).long()) > 0
    both = (t > 0) & (p > 0)
    uk, inter = torch.unique(it[both] * M + p[both], return_counts=True)
    kt = uk // M
    kp = (kt // M) * M + uk % M
    rem = (~lab[kt]) & (inter.double() / (area_t[kt] + area_p[kp] - inter).double() > 0.5)
    gone_t = torch.zeros(n * M, dtype=torch.bool, device=t.device); gone_t[kt[rem]] = True
    gone_p = torch.zeros(n * M, dtype=torch.bool, device=t.device); gone_p[kp[rem]] = True
    t = torch.where(gone_t[it], 0, t); p = torch.where(gone_p[ip], 0, p)
    # per-class tables
    vt, vp = (t > 0) & (ct >= 1) & (ct <= nr), (p > 0) & (cp >= 1) & (cp <= nr)
    C = nr + 1
    kt_all, kp_all = (img * C + ct) * M + t, (img * C + cp) * M + p
    a_t = torch.zeros(n * C * M, dtype=torch.long, device=t.device).scatter_add_(0, kt_all[vt], one[vt])
    a_p = torch.zeros(n * C * M, dtype=torch.long, device=t.device).scatter_add_(0, kp_all[vp], one[vp])
    both = vt & vp & (ct == cp)
    uk, inter = torch.unique(kt_all[both] * M + p[both], return_counts=True)
    a = uk // M
    b = (a // M) * M + uk % M
    iou = inter.double() / (a_t[a] + a_p[b] - inter).double()
    m = iou > match_iou
    ic = a[m] // M
    tp = torch.zeros(n * C, dtype=torch.long, device=t.device).scatter_add_(0, ic, torch.ones_like(ic))
    s = torch.zeros(n * C, dtype=torch.float64, device=t.device).scatter_add_(0, ic, iou[m])
    mt = torch.zeros(n * C * M, dtype=torch.bool, device=t.device); mt[a[m]] = True
    mp = torch.zeros(n * C * M, dtype=torch.bool, device=t.device); mp[b[m]] = True
    fn = ((a_t > 0) & ~mt).view(n * C, M).sum(1)
    fp = ((a_p > 0) & ~mp).view(n * C, M).sum(1)
    out = [x.view(n, C)[:, 1:].cpu().numpy() for x in (tp, fp, fn, s)]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1/16 of the images (a quick look)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"bench_pq: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds, match_iou 0.5, unlabelled-cell filter on"]
    div = 16 if args.small else 1
    for name, size, distinct, repeat, nr in (("A 4096 x 256^2, 7 classes", 256, 256 // div, 16, 7), ("B 64 x 1024^2, 10 classes", 1024, max(8 // div, 1), 8 if not args.small else 4, 10)):
        maps = [torch.from_numpy(x).to(dev) for x in render(1234, size, distinct, repeat, nr)]
        t, ct, p, cp = maps
        fa = lambda: ops.pq_stats(t, p, ct, cp, nr_classes=nr, match_iou=0.5)
        fb = lambda: eager_pq(t, p, ct, cp, nr, 0.5)
        ra, rb = fa(), fb()
        for k, j in (("tp", 0), ("fp", 1), ("fn", 2)):
            assert np.array_equal(ra[k], rb[j]), f"{name}: {k} differs between the device path and the eager formulation"
        assert np.allclose(ra["iou_sum"], rb[3], rtol=1e-12, atol=0)
        times = {"a": [], "b": []}
        for rnd in range(args.rounds):
            for which in (("a", "b") if rnd % 2 == 0 else ("b", "a")):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                (fa if which == "a" else fb)()
                torch.cuda.synchronize(); times[which].append((time.perf_counter() - t0) * 1e3)
        med = lambda v: float(np.median(v))
        ma, mb = med(times["a"]), med(times["b"])
        lines.append(f"{name}: {t.shape[0]} images, {int(ra['tp'].sum())} true positives, {int(ra['fp'].sum())} fp, {int(ra['fn'].sum())} fn")
        lines.append(f"  (a) device ops.pq_stats   median {ma:9.2f} ms   {[round(x, 2) for x in times['a']]}")
        lines.append(f"  (b) eager torch.unique    median {mb:9.2f} ms   {[round(x, 2) for x in times['b']]}")
        lines.append(f"  ratio of medians (a)/(b) = {ma / mb:.4f}; rounds with (a) first {med(times['a'][0::2]) / med(times['b'][0::2]):.4f}, "
                     f"rounds with (b) first {med(times['a'][1::2]) / med(times['b'][1::2]):.4f}; per image (a) {ma / t.shape[0] * 1e3:.1f} us")
        del maps, t, ct, p, cp
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
