"""Per-cell class confidence (--cell_confidence, cpx_instance_confidence): what it costs.  One process, interleaved rounds,
medians with ranges (the style of tools/bench_label_stats.py and tools/bench_pq.py).

    python tools/bench_cell_confidence.py [--rounds 9] [--out profiles/cell_confidence_bench.txt]
    python tools/bench_cell_confidence.py --profile      # the entry alone, a few times (to run under rocprofv3 --kernel-trace --stats)

1. The entry alone, from device-resident inputs: the final id maps and record counts of the fused chain on synthetic fields
   (logits = the analytic one-hot x 4 plus N(0, 2) noise, so the softmax is not saturated), 8 tiles of 256^2 with 7 classes
   and 8 tiles of 1024^2 with 10 classes.  Both workgroup footprints of the debug library (cpx_confidence_set_footprint):
   256 consecutive pixels against a 16 x 16 block, in alternating order; microseconds per call (HIP events around 20 calls)
   and GB/s against the bytes the pass must read, nT * H * W * (4 * ncls + 6).
2. The engine step at the headline geometry (8 tiles of 256^2, 7 classes, 24 blocks, injected fields, polygons, the batch's
   counts read back before the next batch is taken, as the tile loop does): confidence=True against False, wall time per step.
3. The contours file of a 10 000^2 slide's worth of cells (synthetic table: 81 cells per 256 px tile at stride 224, 16 vertices
   each): size and the native writer's time without extras, with the 3 of `summary` and the 10 of `full` (7 classes).
"""
import argparse
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from classpose_amd import _lib, engine, geojson, ops, synth
from classpose_amd._lib import ptr


def chain_inputs(L, dev, nT, T, ncls, seed):
    rng = np.random.default_rng(seed)
    f = [synth.analytic_fields(seed, 1000 * k, 500, T, T, ncls)[:3] for k in range(nT)]
    dP, cp = (torch.from_numpy(np.stack([a[i] for a in f])).to(dev) for i in range(2))
    lg = torch.from_numpy(np.stack([a[2] for a in f]) + rng.normal(0, 2, (nT, ncls, T, T)).astype(np.float32)).to(dev)
    max_rec = min(L.cpx_postproc_max_labels(T, T), 65535)
    masks = torch.empty((nT, T, T), dtype=torch.int16, device=dev)
    cm = torch.empty((nT, T, T), dtype=torch.uint8, device=dev)
    nlab = torch.empty(nT, dtype=torch.int32, device=dev)
    recs = torch.empty(nT * max_rec * engine.RECORD_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    cnt = torch.empty(nT, dtype=torch.int32, device=dev)
    ws = torch.empty(L.cpx_postproc_workspace_bytes(nT, T, T), dtype=torch.uint8, device=dev)
    _lib.check(L.cpx_compute_masks_records(ptr(dP), ptr(cp), ptr(lg), nT, ncls, T, T, 0.0, 0.4, 200, 15, 0.4, ptr(masks), ptr(cm),
                                           ptr(nlab), max_rec, ptr(recs), ptr(cnt), ptr(ws), torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return masks, lg, cp, cnt, max_rec


def entry_alone(L, dev, rounds, lines, profile=False):
    for nT, T, ncls in ((8, 256, 7), (8, 1024, 10)):
        masks, lg, cp, cnt, max_rec = chain_inputs(L, dev, nT, T, ncls, 11)
        out = ops.instance_confidence(masks, lg, cp, cnt, max_rec)
        call = lambda: ops.instance_confidence(masks, lg, cp, cnt, max_rec, out=out)
        if profile:
            for _ in range(5):
                call()
            torch.cuda.synchronize()
            continue
        res = {}
        for foot in (0, 1):
            L.cpx_confidence_set_footprint(foot)
            call()
            torch.cuda.synchronize()
            res[foot] = tuple(t.clone() for t in out)
        assert all(torch.equal(a, b) for a, b in zip(res[0], res[1])), "the two footprints disagree"
        reps, times = 20, {0: [], 1: []}
        for rnd in range(rounds):
            for foot in ((0, 1) if rnd % 2 == 0 else (1, 0)):
                L.cpx_confidence_set_footprint(foot)
                call()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    call()
                e1.record()
                torch.cuda.synchronize()
                times[foot].append(e0.elapsed_time(e1) / reps * 1e3)
        L.cpx_confidence_set_footprint(0)
        nbytes = nT * T * T * (4 * ncls + 6)
        cells = int(cnt.sum())
        fg = float((masks != 0).float().mean())
        lines.append(f"  entry alone, {nT} tiles of {T}^2, {ncls} classes, {cells} cells, {fg:.0%} of the pixels in a cell, "
                     f"{nbytes / 1e6:.1f} MB to read, clear + pass, {reps} calls per timing:")
        for foot, name in ((0, "256 consecutive pixels"), (1, "16 x 16 block         ")):
            m = float(np.median(times[foot]))
            lines.append(f"    {name}  median {m:8.1f} us  [{min(times[foot]):.1f} .. {max(times[foot]):.1f}]  {nbytes / m / 1e3:7.1f} GB/s   "
                         f"{[round(x, 1) for x in times[foot]]}")
        lines.append(f"    ratio of medians 16 x 16 / row = {np.median(times[1]) / np.median(times[0]):.3f}")


def engine_step(dev, rounds, lines, depth):
    NCLS, T, bt, steps = 7, 256, 8, 12
    sd = synth.make_state_dict(NCLS, None, depth=depth, seed=0)
    w = engine.NetWeights.from_state_dict(sd, "bf16", dev)
    eng = engine.Engine(w, T, batch_tiles=bt)
    rng = np.random.default_rng(5)
    batches = []
    for b in range(3):
        tiles = torch.from_numpy(np.stack([synth.render_region(7, 224 * (bt * b + k), 0, T, T) for k in range(bt)])).to(dev)
        f = [synth.analytic_fields(7, 224 * (bt * b + k), 0, T, T, NCLS)[:3] for k in range(bt)]
        inj = tuple(torch.from_numpy(np.stack([a[i] for a in f])).to(dev) for i in range(3))
        batches.append((tiles, inj, [(224.0 * (bt * b + k), 0.0) for k in range(bt)]))

    def run(conf):
        prev = None
        for i in range(steps):
            tiles, inj, org = batches[i % len(batches)]
            sid = eng.submit(tiles, inject=inj, polygons=(1.0, org), confidence=conf)
            if prev is not None:
                out = eng.result(prev)
                out.rec_counts.cpu()                    # the host waits for the previous batch, one step behind the device
            prev = sid
        eng.result(prev).rec_counts.cpu()
        torch.cuda.synchronize()

    for conf in (False, True):
        run(conf)
    times = {False: [], True: []}
    for rnd in range(rounds):
        for conf in ((False, True) if rnd % 2 == 0 else (True, False)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(conf)
            times[conf].append((time.perf_counter() - t0) / steps * 1e3)
    a, b = float(np.median(times[False])), float(np.median(times[True]))
    lines.append(f"  engine step, {bt} tiles of {T}^2, {NCLS} classes, {depth} blocks, bf16, injected fields, device polygons, {steps} steps per timing:")
    lines.append(f"    confidence=False  median {a:7.3f} ms/step  [{min(times[False]):.3f} .. {max(times[False]):.3f}]  {[round(x, 3) for x in times[False]]}")
    lines.append(f"    confidence=True   median {b:7.3f} ms/step  [{min(times[True]):.3f} .. {max(times[True]):.3f}]  {[round(x, 3) for x in times[True]]}")
    lines.append(f"    difference of medians {1e3 * (b - a):+.1f} us/step ({(b / a - 1) * 100:+.2f} %); spread of the rounds "
                 f"{1e3 * (max(times[False]) - min(times[False])):.1f} us (False), {1e3 * (max(times[True]) - min(times[True])):.1f} us (True)")


def contours_file(rounds, lines):
    from classpose_amd.entrypoints.predict_wsi import CELL_ROW
    rng = np.random.default_rng(3)
    n = 44 * 44 * 81                                    # tiles of a 10 000^2 slide at stride 224, ~81 cells each
    cells = np.zeros(n, CELL_ROW)
    cells["n_pts"], cells["cls"] = 16, rng.integers(1, 7, n)
    cells["area"], cells["perimeter"] = rng.uniform(100, 400, n), rng.uniform(30, 80, n)
    cells["cx"], cells["cy"] = rng.uniform(0, 1e4, n), rng.uniform(0, 1e4, n)
    xy = rng.integers(0, 20000, (16 * n, 2)).astype(np.float64) * 0.5
    labels = ["Neutrophil", "Epithelial", "Lymphocyte", "Plasma cell", "Eosinophil", "Connective"]
    full_names = ["class_vote_fraction", "class_probability", "detection_probability"] + ["probability: " + labels[c - 1] for c in range(7)]
    extra = rng.integers(0, 1 << 24, (n, 10)).astype(np.float64) / rng.integers(1, 300, (n, 1)) / (1 << 24)
    variants = (("no extras", None, None), ("summary", full_names[:3], np.ascontiguousarray(extra[:, :3])), ("full", full_names, extra))
    keep = np.arange(n)
    with tempfile.TemporaryDirectory() as d:
        a, b = os.path.join(d, "c.geojson"), os.path.join(d, "p.geojson")
        times, size = {v[0]: [] for v in variants}, {}
        for rnd in range(max(3, rounds // 3)):
            for name, names, ex in (variants if rnd % 2 == 0 else variants[::-1]):
                t0 = time.perf_counter()
                geojson.write_feature_collections(a, b, cells, xy, keep, labels, extra_names=names, extra=ex)
                times[name].append(time.perf_counter() - t0)
                size[name] = os.path.getsize(a)
    lines.append(f"  contours file, {n} cells of 16 vertices (a 10 000^2 slide's worth), native writer, both files written:")
    for name, _, _ in variants:
        lines.append(f"    {name:10s} {size[name] / 1e6:8.1f} MB ({size[name] / size['no extras']:.3f} x)   median {np.median(times[name]):.3f} s  "
                     f"[{min(times[name]):.3f} .. {max(times[name]):.3f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--depth", type=int, default=24)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="run the entry alone a few times and nothing else")
    ap.add_argument("--only", choices=["entry", "engine", "file"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = [f"bench_cell_confidence: {torch.cuda.get_device_name(0)}, {args.rounds} interleaved rounds"]
    if args.profile:
        entry_alone(_lib.lib(), dev, 0, lines, profile=True)
        return
    if args.only in (None, "entry"):
        with _lib.use_debug_library() as D:
            entry_alone(D, dev, args.rounds, lines)
    if args.only in (None, "engine"):
        engine_step(dev, args.rounds, lines, args.depth)
    if args.only in (None, "file"):
        contours_file(args.rounds, lines)
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
