"""tests/resize_reference.py (the CPU restatement of the float32 linear and the nearest resize behind ``eval(diameter=)``) checked
on its own, and the hand composition of oracle + restatement against the reference's own ``ClassposeModel.eval(diameter=)`` run
(tests/golden/reference_eval_diameter.npz, minted by tests/golden/make_golden_eval_diameter.py).  No GPU."""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resize_reference as rr

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

LINEAR_SHAPES = [((37, 53), (64, 80)), ((64, 80), (37, 53)), ((64, 80), (32, 53)), ((133, 154), (200, 232)),
                 ((300, 348), (200, 232)), ((1, 9), (4, 9)), ((9, 1), (9, 4))]
AREA_SHAPES = [((64, 96), (32, 48)), ((400, 464), (200, 232)), ((10, 6), (5, 3))]
# Largest |restatement - torch| over the shapes above on standard-normal input (max |src| = 1.9 .. 5.0), measured on the CPU:
#   bilinear 9.775e-05 (133 x 154 -> 200 x 232; torch forms the source coordinate in float32 from a float32 scale, the restatement
#   in float64 as OpenCV does, so the WEIGHTS differ by a few ulp of the coordinate ~ 1e-5, times |S1 - S0| up to ~ 8),
#   area 2.384e-07 (summation order).  The bounds are ten times that, and both stay under 1e-3 * max |src| >= 1.9e-3; a wrong tap
#   costs O(1).
LINEAR_BOUND, AREA_BOUND = 9.775e-4, 2.384e-6


def _randn(shape, seed):
    return np.random.default_rng(seed).standard_normal(shape).astype(np.float32)


def test_identity_sizes_copy():
    s = _randn((3, 17, 23), 1)
    for fn in (rr.resize_linear_f32, rr.resize_nearest):
        o = fn(s, 17, 23)
        assert np.array_equal(o, s) and o is not s and not np.shares_memory(o, s)


@pytest.mark.parametrize("src_hw,dst_hw", LINEAR_SHAPES + AREA_SHAPES)
def test_constant_plane_stays_constant(src_hw, dst_hw):
    # 0.75 * (1 - f) + 0.75 * f is not exactly 0.75 for every float32 f: constant to within an ulp, and exactly for a power of two
    c = rr.resize_linear_f32(np.full((2, *src_hw), 0.75, np.float32), *dst_hw)
    assert c.shape == (2, *dst_hw) and np.abs(c - np.float32(0.75)).max() <= 2 ** -23
    assert np.all(rr.resize_nearest(np.full((2, *src_hw), 7, np.uint16), *dst_hw) == 7)


@pytest.mark.parametrize("src_hw,dst_hw", LINEAR_SHAPES)
def test_linear_agrees_with_torch_bilinear(src_hw, dst_hw):
    """same sample positions as F.interpolate(bilinear, align_corners=False), different rounding: largest difference measured 9.775e-05, bound ten times that"""
    s = _randn((3, *src_hw), 11)
    got = rr.resize_linear_f32(s, *dst_hw)
    ref = F.interpolate(torch.from_numpy(s)[None], size=dst_hw, mode="bilinear", align_corners=False)[0].numpy()
    dev = float(np.abs(got - ref).max())
    print(f"{src_hw} -> {dst_hw}: max |restatement - torch| = {dev:.3e}, max |src| = {np.abs(s).max():.3f}")
    assert LINEAR_BOUND < 1e-3 * np.abs(s).max()
    assert dev <= LINEAR_BOUND


@pytest.mark.parametrize("src_hw,dst_hw", AREA_SHAPES)
def test_exact_half_agrees_with_avg_pool(src_hw, dst_hw):
    """exact 2 x decimation is the 2 x 2 mean (cv2 re-dispatches it to INTER_AREA): largest difference measured 2.384e-07, bound ten times that"""
    s = _randn((3, *src_hw), 12)
    got = rr.resize_linear_f32(s, *dst_hw)
    ref = F.avg_pool2d(torch.from_numpy(s)[None], 2)[0].numpy()
    dev = float(np.abs(got - ref).max())
    print(f"{src_hw} -> {dst_hw}: max |restatement - avg_pool2d| = {dev:.3e}")
    assert AREA_BOUND < 1e-3 * np.abs(s).max()
    assert dev <= AREA_BOUND
    a, b, c, d = s[:, 0::2, 0::2], s[:, 0::2, 1::2], s[:, 1::2, 0::2], s[:, 1::2, 1::2]
    assert np.array_equal(got, ((a + b) + (c + d)) * np.float32(0.25))          # the stated summation order, bitwise


def test_half_in_one_axis_only_is_not_the_area_path():
    s = _randn((1, 64, 80), 13)
    got = rr.resize_linear_f32(s, 32, 53)
    y_only = (s[:, 0::2] + s[:, 1::2]) * np.float32(0.5)                        # in y the taps are rows 2i, 2i + 1 at weight 0.5 each
    x0, x1, fx = rr.linear_taps(53, 80, True)
    h = s[:, :, x0] * (np.float32(1) - fx) + s[:, :, x1] * fx
    assert np.array_equal(got, h[:, 0::2] * np.float32(0.5) + h[:, 1::2] * np.float32(0.5)) and got.shape == y_only[:, :, :53].shape


@pytest.mark.parametrize("src_hw,dst_hw", LINEAR_SHAPES + AREA_SHAPES)
def test_nearest_is_plain_index_arithmetic(src_hw, dst_hw):
    (sh, sw), (dh, dw) = src_hw, dst_hw
    s = np.random.default_rng(3).integers(0, 65536, (2, sh, sw)).astype(np.uint16)
    got = rr.resize_nearest(s, dh, dw)
    assert got.dtype == np.uint16
    for y in range(dh):
        sy = min(int(np.floor(y * (1.0 / (dh / sh)))), sh - 1)
        for x in (0, 1, dw // 2, dw - 1):
            sx = min(int(np.floor(x * (1.0 / (dw / sw)))), sw - 1)
            assert np.array_equal(got[:, y, x], s[:, sy, sx]), (y, x)


def test_clamps_left_right_but_not_top_bottom():
    """upscaling: the first and last columns copy the source's (weight zeroed), the first and last rows do too but through
    clipped indices with the weight kept (both taps on the same row)"""
    s = _randn((1, 37, 53), 14)
    o = rr.resize_linear_f32(s, 64, 80)
    x0, x1, fx = rr.linear_taps(80, 53, True)
    y0, y1, fy = rr.linear_taps(64, 37, False)
    assert fx[0] == 0 and x0[0] == 0 and fx[-1] == 0 and x0[-1] == 52
    assert fy[0] != 0 and y0[0] == y1[0] == 0 and y0[-1] == 36 and y1[-1] == 36
    assert np.array_equal(o[0, 5, 0], (s[0, y0[5], 0] * (1 - fy[5]) + s[0, y1[5], 0] * fy[5]).astype(np.float32))


def compose(tile, diameter, resample):
    """eval(diameter=) by hand: oracle.tiling (u8 resize, normalize_img, run_net on decode_net) + resize_reference +
    oracle.dynamics / classmask.  Returns what the reference returns plus the call log in the fixture's format."""
    import make_golden_eval as mge
    from oracle import classmask, dynamics, tiling
    H, W = tile.shape[:2]
    scaling = 30.0 / diameter
    Hs, Ws = int(H * scaling), int(W * scaling)
    log = [dict(call="resize_image", shape=[1, H, W, 3], dtype="uint8", Ly=Hs, Lx=Ws, interpolation="linear", no_channels=False)]
    img = tiling.resize_linear_u8(tile, Ws, Hs)
    log.append(dict(call="normalize_img", shape=[1, Hs, Ws, 3], dtype="float32"))
    x = tiling.normalize_img(img[None])

    def fw(im):
        o = mge.decode_net(torch.from_numpy(np.ascontiguousarray(im)), mge.NCLS).numpy()
        return o[:, mge.NCLS:], o[:, :mge.NCLS]
    dP, cp, yc = tiling.run_net(fw, x, batch_size=8, augment=False, tile_overlap=0.1, bsize=256)

    def lin(shape, no_channels):
        return dict(call="resize_image", shape=shape, dtype="float32", Ly=H, Lx=W, interpolation="linear", no_channels=no_channels)

    def fields_to_tile(pre):
        nonlocal dP, cp, yc
        h, w = dP.shape[-2:]
        if pre:
            log.extend([lin([1, h, w, 2], False), lin([1, h, w], True), lin([1, h, w, mge.NCLS], False)])
        else:
            log.extend([dict(call="_resize_gradients", shape=[2, h, w]), lin([h, w, 2], False),
                        dict(call="_resize_cellprob", shape=[h, w]), lin([h, w], True),
                        dict(call="_resize_gradients", shape=[mge.NCLS, h, w]), lin([h, w, mge.NCLS], False)])
        dP, cp, yc = (rr.resize_linear_f32(a, H, W) for a in (dP, cp, yc))
    if resample:
        fields_to_tile(True)
    h, w = cp.shape
    log.append(dict(call="resize_and_compute_masks", dP_shape=[2, h, w], niter=200, resize=None if (h, w) == (H, W) else [H, W]))
    masks = dynamics.compute_masks(dP, cp).astype(np.uint16)
    cm, _ = classmask.compute_class_masks(masks, yc)
    fields_to_tile(False)
    for dt in ("uint16", "int64"):
        log.append(dict(call="resize_image", shape=[h, w], dtype=dt, Ly=H, Lx=W, interpolation="nearest", no_channels=True))
    masks, cm = rr.resize_nearest(masks, H, W), rr.resize_nearest(cm, H, W)
    return dict(masks=masks, class_masks=cm.astype(np.uint8), dP=dP, cellprob=cp, yclass=yc, shape_x=(1, Hs, Ws, 3), log=log)


def test_composition_equals_reference_eval_diameter():
    """Every array and the whole call log of the reference's five runs (diameter 20 / 45 / 15 / 30 with resample, 45 without), bit
    for bit: this composition is what the GPU tests use as their oracle."""
    import make_golden_eval_diameter as mgd
    g = np.load(mgd.FIXTURE)
    tile = mgd.diameter_tile()
    assert int(tile.astype(np.int64).sum()) == int(g["tilesum"]) and int(g["n"]) == len(mgd.ROWS)
    for k, (diam, resample) in enumerate(mgd.ROWS):
        assert [int(v) for v in g[f"{k}_cfg"]] == [diam, int(resample)]
        c = compose(tile, diam, resample)
        assert np.array_equal(c["masks"], g[f"{k}_masks"]) and int(c["masks"].max()) == mgd.CELLS[k], k
        assert np.array_equal(c["class_masks"], g[f"{k}_class_masks"]), k
        for name in ("dP", "cellprob", "yclass"):
            a = c[name][..., ::4, ::4]
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), g[f"{k}_{name}"].view(np.uint32)), (k, name)
        assert tuple(int(v) for v in g[f"{k}_shape_x"]) == c["shape_x"], k
        assert json.loads(str(g[f"{k}_log"])) == c["log"], k
    sizes = [json.loads(str(g[f"{k}_log"]))[0] for k in range(5)]
    assert [(s["Ly"], s["Lx"]) for s in sizes] == [(300, 348), (133, 154), (400, 464), (200, 232), (133, 154)]
