"""Network-size fields -> tile-size fields, the hot step of ``eval(diameter=)``: ops.resize_fields (cpx_resize_linear_f32) against eager
PyTorch on the same GPU; one process, interleaved rounds (order reversed in odd rounds), medians with ranges.

    python tools/bench_resize_fields.py [--rounds 7] [--out profiles/resize_fields_bench.txt]
    python tools/bench_resize_fields.py --profile    # one eval(diameter=45) batch of 8 tiles of 1024^2 (for rocprofv3 --kernel-trace --stats)

Workload: 8 tiles x 13 planes (dP 2, cellprob 1, 10 class logits) of float32, resident on the device before and after, in the three
buffers the engine keeps them in (so three launches per call on either side), destination buffers allocated once:
  683^2 -> 1024^2 (diameter 45), 1536^2 -> 1024^2 (diameter 20), 2048^2 -> 1024^2 (diameter 15: the exact 2 x 2 area path).
Paths:
  (1) device   ops.resize_fields(src, 1024, 1024, out=dst) per buffer
  (2) torch    torch.nn.functional.interpolate(src, size=(1024, 1024), mode="bilinear", align_corners=False) per buffer, or
               avg_pool2d(src, 2) for the 2 x case; same sample positions, another rounding: compared for speed only (the largest
               difference is printed)
Before anything is timed (1) is compared bit for bit with tests/resize_reference on one plane of each shape.
Bytes are algorithmic: every source element read once, every destination element written once.
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
import torch.nn.functional as F

import resize_reference as rr
from bench_label_components import timed
from classpose_amd import ops

N_TILES, PLANES, DST = 8, (2, 1, 10), 1024
SHAPES = ((683, "diameter 45"), (1536, "diameter 20"), (2048, "diameter 15, area path"))
HBM_BYTES_PER_S = 8e12


def profile(dev):
    from classpose_amd import synth
    from classpose_amd.models import ClassposeModel
    model = ClassposeModel(pretrained_model=synth.make_state_dict(10, None, depth=2, seed=3), device=dev, precision="bf16", max_batch_tiles=N_TILES)
    tiles = [synth.render_region(91 + k, 0, 0, DST, DST) for k in range(N_TILES)]
    for _ in range(2):                      # the first call builds the engine
        masks, _flows, _cm, _styles = model.eval(tiles, diameter=45)
    torch.cuda.synchronize()
    print("eval(diameter=45):", [int(m.max()) for m in masks], "cells")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--profile", action="store_true", help="one eval(diameter=45) batch and nothing else")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    sync = torch.cuda.synchronize
    if args.profile:
        return profile(dev)
    lines = [f"bench_resize_fields: {torch.cuda.get_device_name(0)}, {N_TILES} tiles x {sum(PLANES)} float32 planes in three buffers, device-resident in and out, "
             f"{args.rounds} interleaved rounds, order reversed in odd rounds, one warm-up call of every path first; ms per call, median [min .. max]"]
    g = torch.Generator(device=dev).manual_seed(1)
    dsts = [torch.empty((N_TILES, p, DST, DST), dtype=torch.float32, device=dev) for p in PLANES]
    ok = True
    for s, what in SHAPES:
        srcs = [torch.randn((N_TILES, p, s, s), generator=g, dtype=torch.float32, device=dev) for p in PLANES]
        area = s == 2 * DST

        def device():
            for a, b in zip(srcs, dsts):
                ops.resize_fields(a, DST, DST, out=b)

        def eager():
            return [F.avg_pool2d(a, 2) if area else F.interpolate(a, size=(DST, DST), mode="bilinear", align_corners=False) for a in srcs]
        device()
        want = rr.resize_linear_f32(srcs[2][3, 7].cpu().numpy(), DST, DST)
        assert np.array_equal(dsts[2][3, 7].cpu().numpy().view(np.uint32), want.view(np.uint32)), "the device differs from the restatement"
        diff = max(float((a - b).abs().max()) for a, b in zip(eager(), dsts))
        paths = {"1": device, "2": eager}
        times = {k: [] for k in paths}
        for rnd in range(args.rounds):
            for k in (("1", "2") if rnd % 2 == 0 else ("2", "1")):
                times[k].append(timed(paths[k], sync))
        nbytes = N_TILES * sum(PLANES) * (s * s + DST * DST) * 4
        fmt = lambda v: f"{np.median(v):9.4f} [{min(v):.4f} .. {max(v):.4f}]"
        rate = lambda v: f"{nbytes / (np.median(v) * 1e-3) / 1e12:.2f} TB/s = {nbytes / (np.median(v) * 1e-3) / HBM_BYTES_PER_S * 100:.0f} % of 8 TB/s"
        below = max(times["1"]) < min(times["2"])
        ok &= below
        lines += [f"{s}^2 -> {DST}^2 ({what}): {nbytes / 1e6:.0f} MB read + written; largest |torch - device| = {diff:.2e} on standard-normal input",
                  f"  (1) device, ops.resize_fields x 3                 {fmt(times['1'])}   ({rate(times['1'])})",
                  f"  (2) torch, {'avg_pool2d' if area else 'interpolate(bilinear)'} x 3, eager".ljust(52) + f"{fmt(times['2'])}   ({rate(times['2'])})",
                  f"  every round of (1) below every round of (2): {below}; ratio of medians (2)/(1) = {np.median(times['2']) / np.median(times['1']):.2f}"]
        del srcs
        torch.cuda.empty_cache()
    lines.append(f"acceptance (every device round below every torch round at every shape): {ok}")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
