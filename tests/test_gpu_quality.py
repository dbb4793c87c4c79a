"""Image-quality augmentation on the device (csrc/cpx_augment.hip t6 -> ops.blur / blur_pool_rects / hbs / warp_affine_pool_quality
-> augment "quality" / "hed_he_quality" -> train_class_head -> train_head --augment).

Yardsticks: the reference-minted fixture tests/golden/reference_quality.npz and the float64 restatement of the blur, the float32
restatement of the hue / brightness / saturation jitter (tests/quality_reference.py), and the kernels the fused pool kernel
composes.  The arithmetic is IEEE and ordered: ZERO bytes may differ anywhere, with no exemptions.  Every test prints the figures
it observed before it asserts (-s)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import quality_reference as qr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SENTINEL = 173
SIZES = [(1, 1), (5, 7), (37, 53), (301, 299), (256, 256)]
SIGMAS = [0.05, 0.124, 0.126, 0.7, 1.3, 1.77, 2.0]
TILE = 32                                                   # BLUR_TILE of csrc/cpx_augment.hip
TRUE_BASIS = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])


def _weights(sigmas):
    from classpose_amd import augment
    rw = [augment.gauss_weights(s) for s in sigmas]
    return np.array([r for r, _w in rw], np.int32), np.stack([w for _r, w in rw])


def _guarded_pool(ims, dev, labs=None, pad=77):
    from classpose_amd import augment
    px_off, hw, total = augment.pool_table([im.shape[:2] for im in ims])
    buf = torch.full((pad + 3 * total + pad,), SENTINEL, dtype=torch.uint8, device=dev)
    buf[pad:pad + 3 * total] = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(dev)
    pool_lab = None
    if labs is not None:
        pool_lab = torch.from_numpy(np.concatenate([lab.reshape(-1) for lab in labs])).to(dev)
    return buf, buf[pad:pad + 3 * total], pool_lab, torch.from_numpy(px_off).to(dev), torch.from_numpy(hw).to(dev)


def _random_params(rng, n):
    from classpose_amd import stain
    out = np.empty((n, 14))
    for t in range(n):
        H = TRUE_BASIS + rng.uniform(-0.05, 0.05, (2, 3))
        H = H / np.linalg.norm(H, axis=1, keepdims=True)
        out[t] = stain.stain_params(H, np.linalg.pinv(H), rng.uniform(-1, 1, (2, 3)), rng.uniform(-1, 1, 2), 0.15, 0.4)
    return out


@pytest.fixture(scope="module")
def ragged():
    rng = np.random.default_rng(8)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    labs = [rng.integers(0, 7, (h, w)).astype(np.int16) for h, w in SIZES]
    return ims, labs


# ---- 1. whole images ------------------------------------------------------------------------------------------------
def test_blur_equals_the_fixture(cuda):
    from classpose_amd import ops
    with open(os.path.join(GOLD, "reference_quality.json")) as f:
        meta = json.load(f)
    npz = np.load(os.path.join(GOLD, "reference_quality.npz"))
    differ = 0
    by_image = {}
    for c in meta["cases"]:
        by_image.setdefault(c["image"], []).append(c)
    for name, cases in by_image.items():                                 # one launch per image: its sigmas as a batch of mixed radii
        img = npz[name]
        radius, weights = _weights([c["sigma"] for c in cases])
        X = torch.from_numpy(np.repeat(img[None], len(cases), 0)).to(cuda)
        out = ops.blur(X, radius, weights).cpu().numpy()
        for k, c in enumerate(cases):
            d = int((out[k] != npz[c["out"]]).sum())
            differ += d
            assert d == 0, (name, c["sigma"])
    print(f"{len(meta['cases'])} fixture cases, {differ} bytes differ")
    assert differ == 0


@pytest.mark.parametrize("shape", [(1, 1), (3, 5), (8, 8), (17, 16), (37, 53), (TILE + 1, 2 * TILE + 1)])
def test_blur_equals_the_restatement(cuda, shape):
    from classpose_amd import ops
    rng = np.random.default_rng(shape[0] * 1000 + shape[1])
    h, w = shape
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in SIGMAS]
    ims += [np.full((h, w, 3), v, np.uint8) for v in (255, 254, 1)]
    sigmas = SIGMAS + [1.3, 1.3, 2.0]
    radius, weights = _weights(sigmas)
    n = len(ims)
    per, pad = h * w * 3, 50
    src = torch.from_numpy(np.stack(ims)).to(cuda)
    # the output sits between sentinel bytes, at an odd address
    buf = torch.full((pad + 1 + n * per + pad,), SENTINEL, dtype=torch.uint8, device=cuda)
    scratch = buf[pad + 1:pad + 1 + n * per]
    px_off = torch.arange(n, dtype=torch.int64, device=cuda) * (h * w)
    hw = torch.tensor([[h, w]] * n, dtype=torch.int32, device=cuda)
    _s, off, status = ops.blur_pool_rects(src.view(-1), px_off, hw, np.arange(n), np.tile([0, 0, h, w], (n, 1)), radius, weights, scratch)
    assert int(status.item()) == 0 and np.array_equal(off, np.arange(n) * per)
    got = scratch.view(n, h, w, 3).cpu().numpy()
    differ = 0
    for t in range(n):
        want = qr.gaussian_blur(ims[t], sigmas[t])
        differ += int((got[t] != want).sum())
        if radius[t] == 0:
            assert np.array_equal(got[t], ims[t])
    print(f"{shape}: radii {radius.tolist()}, {differ} bytes differ from the float64 restatement")
    assert differ == 0
    if h >= 3 and w >= 3:
        assert np.all(got[len(SIGMAS)] == 254)                            # constant 255 at sigma 1.3 comes out as 254
    assert bool((buf[:pad + 1] == SENTINEL).all()) and bool((buf[pad + 1 + n * per:] == SENTINEL).all())
    assert torch.equal(ops.blur(src, radius, weights), scratch.view(n, h, w, 3))
    with pytest.raises(ValueError, match="radius"):
        ops.blur(src, radius + 8, weights)


# ---- 2. rectangles --------------------------------------------------------------------------------------------------
def _rects_of(h, w, rng):
    """whole image, the four corners, the four borders, single pixels, interiors -- clipped to what the image has"""
    out = [(0, 0, h, w), (0, 0, 1, 1), (h - 1, w - 1, 1, 1), (0, w - 1, 1, 1), (h - 1, 0, 1, 1)]
    a, b = max(1, h // 3), max(1, w // 3)
    out += [(0, 0, a, b), (0, w - b, a, b), (h - a, 0, a, b), (h - a, w - b, a, b)]                 # corners
    out += [(0, b // 2, a, max(1, w - b)), (h - a, 0, a, w), (a // 2, 0, max(1, h - a), b), (0, w - b, h, b)]   # borders
    for _ in range(3):
        y0, x0 = int(rng.integers(0, h)), int(rng.integers(0, w))
        out.append((y0, x0, int(rng.integers(1, h - y0 + 1)), int(rng.integers(1, w - x0 + 1))))
    if h > 140 and w > 140:
        out += [(TILE - 3, TILE + 5, TILE + 7, 2 * TILE + 1), (100, 90, 1, 130), (17, 201, 150, 1)]
    return sorted(set(out))


def test_blur_rectangles_equal_the_whole_image_result(cuda, ragged):
    from classpose_amd import ops
    ims, _labs = ragged
    rng = np.random.default_rng(4)
    buf, pool_u8, _lab, px_off, hw = _guarded_pool(ims, cuda)
    assert pool_u8.data_ptr() % 2 == 1
    nI = len(ims)
    sig, bias = (rng.uniform(-0.25, 0.25, (nI, 3)).astype(np.float32) for _ in range(2))
    params = _random_params(rng, nI)
    sigmas = [2.0, 1.3, 2.0, 1.77, 0.7]
    radius, weights = _weights(sigmas)
    total = differ = 0
    for m in (0, 1, 2):
        # the colour stage and the blur of every whole image, by the whole-image ops
        whole = []
        for i, im in enumerate(ims):
            x = torch.from_numpy(im[None]).to(cuda)
            if m == 1:
                x, _a = ops.hed_jitter(x, sig[i:i + 1], bias[i:i + 1], (0.0, 1.0), False)
            elif m == 2:
                x = ops.he_stain(x, params[i:i + 1], [2])
            if m:
                assert np.array_equal(qr.gaussian_blur(x[0].cpu().numpy(), sigmas[i]),
                                      ops.blur(x, radius[i:i + 1], weights[i:i + 1])[0].cpu().numpy())
            whole.append(ops.blur(x, radius[i:i + 1], weights[i:i + 1])[0].cpu().numpy())
        image_of, rects = [], []
        for i, (h, w) in enumerate(SIZES):
            for r in _rects_of(h, w, rng):
                image_of.append(i)
                rects.append(r)
        image_of, rects = np.array(image_of), np.array(rects)
        k = len(rects)
        scratch, off, status = ops.blur_pool_rects(pool_u8, px_off, hw, image_of, rects, radius[image_of], weights[image_of],
                                                   mode=np.full(k, m), sigma=sig[image_of], bias=bias[image_of], params=params[image_of])
        assert int(status.item()) == 0
        got = scratch.cpu().numpy()
        for j in range(k):
            y0, x0, h, w = rects[j]
            g = got[off[j]:off[j] + 3 * h * w].reshape(h, w, 3)
            d = int((g != whole[image_of[j]][y0:y0 + h, x0:x0 + w]).sum())
            differ += d
            assert d == 0, (m, int(image_of[j]), rects[j].tolist())
        total += k
    print(f"{total} rectangles in colour modes 0, 1, 2: {differ} bytes differ from the whole-image result")
    assert differ == 0 and bool((buf[:77] == SENTINEL).all()) and bool((buf[-77:] == SENTINEL).all())


def test_a_bad_request_touches_nothing_and_sets_its_bit(cuda, ragged):
    from classpose_amd import ops
    ims, _labs = ragged
    _buf, pool_u8, _lab, px_off, hw = _guarded_pool(ims, cuda)
    image_of = np.array([2, 3, 4, 2])
    rects = np.array([(0, 0, 37, 53), (10, 20, 100, 90), (200, 100, 56, 156), (5, 5, 20, 30)])
    radius, weights = _weights([2.0, 1.3, 0.7, 1.77])
    nbytes = 3 * rects[:, 2] * rects[:, 3]
    off = np.concatenate([[0], np.cumsum(nbytes)[:-1]])
    size = int(nbytes.sum())
    good = torch.full((size,), SENTINEL, dtype=torch.uint8, device=cuda)
    _s, _o, status = ops.blur_pool_rects(pool_u8, px_off, hw, image_of, rects, radius, weights, good, off)
    assert int(status.item()) == 0
    good = good.cpu().numpy()

    def run(**kw):
        a = dict(image_of=image_of.copy(), rects=rects.copy(), off=off.copy(), hw=hw, px_off=px_off)
        a.update(kw)
        scratch = torch.full((size,), SENTINEL, dtype=torch.uint8, device=cuda)
        _s, _o, st = ops.blur_pool_rects(pool_u8, a["px_off"], a["hw"], a["image_of"], a["rects"], radius, weights, scratch, a["off"],
                                         check_status=False)
        return scratch.cpu().numpy(), int(st.item())

    def expect(got, bad_j):
        for j in range(4):
            seg = slice(off[j], off[j] + nbytes[j])
            if j == bad_j:
                assert np.all(got[seg] == SENTINEL), j
            else:
                assert np.array_equal(got[seg], good[seg]), j
    r = rects.copy()
    r[1] = (250, 20, 100, 90)                                            # sticks out of its 301 x 299 image
    got, st = run(rects=r)
    assert st == 4
    expect(got, 1)
    r = rects.copy()
    r[3] = (5, 5, 0, 30)
    got, st = run(rects=r)
    assert st == 4
    expect(got, 3)
    io = image_of.copy()
    io[0] = 5
    got, st = run(image_of=io)
    assert st == 1
    expect(got, 0)
    bad_hw = hw.clone()
    bad_hw[4, 0] = 1 << 20                                               # a table entry beyond the pool
    got, st = run(hw=bad_hw)
    assert st == 2
    expect(got, 2)
    o = off.copy()
    o[2] = size - 10                                                     # the range runs past the scratch
    got, st = run(off=o)
    assert st == 8
    expect(got, 2)
    assert np.all(got[size - 10:] == good[size - 10:])
    o[2] = -4
    got, st = run(off=o)
    assert st == 8
    expect(got, 2)
    with pytest.raises(ValueError, match="rectangle"):
        ops.blur_pool_rects(pool_u8, px_off, hw, image_of, r, radius, weights)
    with pytest.raises(ValueError, match="radius"):
        ops.blur_pool_rects(pool_u8, px_off, hw, image_of, rects, [9, 1, 1, 1], weights)
    print("status bits 1, 2, 4, 8 seen; every other request's bytes unchanged")


# ---- 3. hue / brightness / saturation -------------------------------------------------------------------------------
def test_hbs_equals_the_restatement(cuda):
    from classpose_amd import ops
    x = qr.hbs_inputs()
    m = len(x)
    w = 509
    h = -(-m // w)
    img = np.zeros((h * w, 3), np.uint8)
    img[:m] = x
    img = img.reshape(h, w, 3)
    sets = qr.HBS_SETS
    n = len(sets) + 1
    par = np.stack([qr.hbs_values(*ps) for ps in sets] + [qr.hbs_values(0.07, 1.05, 0.93)])
    apply = np.ones(n, np.int32)
    apply[-1] = 0                                                        # apply = 0 copies, whatever the values
    out = ops.hbs(torch.from_numpy(np.repeat(img[None], n, 0)).to(cuda), par, apply).cpu().numpy()
    differ = 0
    for t, ps in enumerate(sets):
        want = qr.hbs_numpy(img, *ps)
        d = int((out[t] != want).sum())
        print(f"hue {ps[0]:+.4f} brightness {ps[1]:.4f} saturation {ps[2]:.4f}: {d} of {want.size} bytes differ")
        differ += d
    assert differ == 0
    assert np.array_equal(out[0], img) and np.array_equal(out[-1], img) and (out[1] != img).any()


# ---- 4. the fused pool kernel ---------------------------------------------------------------------------------------
def _pool_maps(shapes, dh, dw, rng):
    """identity, half-pixel, mostly outside, the whole source, then turns about the centre"""
    inv = np.empty((len(shapes), 6))
    for t, (h, w) in enumerate(shapes):
        kind = t % 5
        if kind == 0:
            inv[t] = [1, 0, 0, 0, 1, 0]
        elif kind == 1:
            inv[t] = [1, 0, 0.5, 0, 1, 0.5]
        elif kind == 2:
            inv[t] = [1, 0, w - 3.25, 0, 1, h - 2.5]
        elif kind == 3:
            inv[t] = [w / dw, 0, -0.5, 0, h / dh, -0.5]
        else:
            th, s = rng.uniform(0, 2 * np.pi), rng.uniform(0.6, 1.8)
            c, sn = np.cos(th) / s, np.sin(th) / s
            cx, cy, ox, oy = (w - 1) / 2, (h - 1) / 2, (dw - 1) / 2, (dh - 1) / 2
            inv[t] = [c, sn, cx - (c * ox + sn * oy), -sn, c, cy - (-sn * ox + c * oy)]
    return inv


def test_quality_pool_kernel_equals_its_parts_bitwise(cuda, ragged):
    from classpose_amd import augment, ops
    ims, labs = ragged
    rng = np.random.default_rng(12)
    _buf, pool_u8, pool_lab, px_off, hw = _guarded_pool(ims, cuda, labs)
    image_of = np.array([3, 0, 4, 2, 1, 3, 3, 4, 2, 0, 1, 4, 4, 3, 2, 3], np.int32)
    n, (dh, dw) = len(image_of), (64, 48)
    shapes = [SIZES[i] for i in image_of]
    inv = _pool_maps(shapes, dh, dw, rng)
    mode = np.array([2, 2, 1, 0, 2, 1, 0, 2, 2, 1, 0, 0, 2, 2, 1, 0], np.int32)
    blurred = np.array([1, 1, 0, 1, 0, 1, 1, 0, 1, 0, 1, 1, 1, 0, 0, 1], bool)
    hbs_on = np.array([1, 0, 1, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1, 1, 0, 1], np.int32)
    sig_blur = rng.uniform(0.13, 2.0, n)
    sig_blur[0], sig_blur[3] = 2.0, 1.9
    radius, weights = _weights(sig_blur)
    params = _random_params(rng, n)
    sigma, bias = (rng.uniform(-0.25, 0.25, (n, 3)).astype(np.float32) for _ in range(2))
    par = np.stack([qr.hbs_values(rng.uniform(-0.1, 0.1), 1 + rng.uniform(-0.1, 0.1), rng.uniform(0.9, 1.1)) for _ in range(n)])
    rects, ok = augment.footprint_rects(inv, [s[0] for s in shapes], [s[1] for s in shapes], (dh, dw))
    assert ok.all()
    b = np.flatnonzero(blurred)
    scratch, off, st = ops.blur_pool_rects(pool_u8, px_off, hw, image_of[b], rects[b], radius[b], weights[b], mode=mode[b], sigma=sigma[b],
                                           bias=bias[b], params=params[b])
    ov_off = np.full(n, -1, np.int64)
    ov_off[b] = off
    got, got_lab, status = ops.warp_affine_pool_quality(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias, False,
                                                        params, par, hbs_on, scratch, ov_off, rects, label_fill=-100)
    assert int(status.item()) == 0 and got.dtype == torch.float32 and tuple(got.shape) == (n, 3, dh, dw)
    differ = 0
    for t, i in enumerate(image_of):
        whole = torch.from_numpy(ims[i][None]).to(cuda)
        lab = torch.from_numpy(labs[i][None]).to(cuda)
        if mode[t] == 2:
            whole = ops.he_stain(whole, params[t:t + 1], [2])
        elif mode[t] == 1:
            whole, _a = ops.hed_jitter(whole, sigma[t:t + 1], bias[t:t + 1], (0.0, 1.0), False)
        if blurred[t]:
            whole = ops.blur(whole, radius[t:t + 1], weights[t:t + 1])
        whole = ops.hbs(whole, par[t:t + 1], hbs_on[t:t + 1])
        want, want_lab = ops.warp_affine(whole, inv[t:t + 1], (dh, dw), lab, -100)
        d = int((got[t] != want[0]).sum())
        differ += d
        assert d == 0 and torch.equal(got_lab[t], want_lab[0]), (t, int(i), int(mode[t]), bool(blurred[t]), int(hbs_on[t]))
    print(f"{n} crops, {int(blurred.sum())} blurred, {int(hbs_on.sum())} with HBS: {differ} values differ from the per-crop composition")
    assert differ == 0
    # nothing gated: bitwise the stain entry
    plain, plain_lab, _s = ops.warp_affine_pool_stain(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias, False, params,
                                                      label_fill=-100)
    q0, l0, _s = ops.warp_affine_pool_quality(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias, False, params,
                                              label_fill=-100)
    assert torch.equal(q0, plain) and torch.equal(l0, plain_lab) and not torch.equal(got, plain)
    # a rectangle made too small: the bit is set, the labels are untouched, nothing faults because nothing is read through it
    small = rects.copy()
    t0 = int(b[0])
    small[t0, 2:] = np.maximum(1, small[t0, 2:] // 2)
    q1, l1, s1 = ops.warp_affine_pool_quality(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias, False, params, par,
                                              hbs_on, scratch, ov_off, small, label_fill=-100, check_status=False)
    assert int(s1.item()) == 16 and torch.equal(l1, got_lab)
    keep = [t for t in range(n) if t != t0]
    assert torch.equal(q1[keep], got[keep])
    with pytest.raises(ValueError, match="outside the crop's blurred rectangle"):
        ops.warp_affine_pool_quality(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias, False, params, par, hbs_on,
                                     scratch, ov_off, small, label_fill=-100)
    far = ov_off.copy()
    far[t0] = scratch.numel() - 5
    _q, l2, s2 = ops.warp_affine_pool_quality(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias, False, params, par,
                                              hbs_on, scratch, far, rects, label_fill=-100, check_status=False)
    assert int(s2.item()) == 8 and torch.equal(l2, got_lab)


# ---- 5. the loop ----------------------------------------------------------------------------------------------------
def _synthetic_ragged(ncls, sizes, seed0=300):
    from classpose_amd import synth
    ims, labs = [], []
    for k, (h, w) in enumerate(sizes):
        x0, y0 = 600 * (k % 3), 600 * (k // 3)
        ims.append(synth.render_region(seed0, x0, y0, w, h))
        lab = synth.analytic_fields(seed0, x0, y0, w, h, ncls)[2].argmax(0).astype(np.int16)
        lab[(40 + 11 * k) % 150:][:24] = -100
        labs.append(lab)
    return ims, labs


TRAIN_SIZES = [(300, 280), (256, 256), (200, 333), (384, 260), (270, 400), (512, 300)]


def _seed_with_blur(pool, idx, name, start):
    """the first seed from ``start`` whose draws blur at least two of the crops and leave at least one unblurred"""
    from classpose_amd import augment
    cfg = augment.get_config(name)
    for seed in range(start, start + 400):
        p = augment.sample_batch_params_pool(pool, idx, np.random.default_rng(seed), cfg)
        blurred = augment.quality_params(p, cfg)[0]
        if 2 <= blurred.sum() < len(idx):
            return seed
    raise AssertionError("no seed blurs two crops")


@pytest.mark.parametrize("name", ["hed_he_quality", "quality"])
def test_augment_batch_pool_quality_equals_the_ops_by_hand(cuda, name):
    from classpose_amd import augment, ops
    ims, labs = _synthetic_ragged(7, TRAIN_SIZES)
    pool = augment.ImagePool(ims, labs, device=cuda)
    cfg = augment.get_config(name)
    idx = np.array([5, 0, 3, 3, 1, 2, 4, 0, 5, 2, 1, 4])
    seed = _seed_with_blur(pool, idx, name, 70)
    got, got_lab = augment.augment_batch_pool(pool, idx, np.random.default_rng(seed), name, dtype=torch.float32)
    p = augment.sample_batch_params_pool(pool, idx, np.random.default_rng(seed), cfg)
    blurred, radius, weights, hbs, hbs_apply = augment.quality_params(p, cfg)
    mode = np.zeros(len(idx), np.int32)
    if name == "hed_he_quality":
        mode, params = augment.stain_mode_params(p, cfg, pool.stain_basis().take(idx), pool.applied(cfg["cutoff_range"])[idx])
    print(f"{name} seed {seed}: modes {mode.tolist()}, blurred {blurred.astype(int).tolist()}, HBS {hbs_apply.tolist()}")
    xs, ls = [], []
    for t, i in enumerate(idx):
        whole = torch.from_numpy(ims[i][None]).to(cuda)
        if mode[t] == 2:
            whole = ops.he_stain(whole, params[t:t + 1], [2])
        elif mode[t] == 1:
            whole, _a = ops.hed_jitter(whole, p.sigma[t:t + 1], p.bias[t:t + 1], cfg["cutoff_range"], False)
        if blurred[t]:
            whole = ops.blur(whole, radius[t:t + 1], weights[t:t + 1])
        whole = ops.hbs(whole, hbs[t:t + 1], hbs_apply[t:t + 1])
        x, lab = ops.warp_affine(whole, p.inv[t:t + 1], (256, 256), torch.from_numpy(labs[i][None]).to(cuda), 0)
        xs.append(x)
        ls.append(lab)
    x = torch.cat(xs)
    want = ops.patchify_f32(ops.normalize_img_f32(x, out=x), torch.float32)
    assert torch.equal(got, want) and torch.equal(got_lab, torch.cat(ls))
    # pre-cut crops of one size against a pool of the same crops
    eq_ims, eq_labs = _synthetic_ragged(7, [(256, 256)] * 4)
    eq = augment.ImagePool(eq_ims, eq_labs, device=cuda)
    sel = np.array([2, 0, 3, 3, 1, 0])
    X, Y = np.stack(eq_ims)[sel], np.stack(eq_labs)[sel]
    s2 = _seed_with_blur(eq, sel, name, 9)
    pa, la = augment.augment_batch_pool(eq, sel, np.random.default_rng(s2), name, dtype=torch.float32, label_fill=-100)
    pb, lb = augment.augment_batch(X, Y, np.random.default_rng(s2), name, dtype=torch.float32, device=cuda, label_fill=-100)
    assert torch.equal(pa, pb) and torch.equal(la, lb)
    base = "hed_he" if name == "hed_he_quality" else "geometry"
    plain, _l = augment.augment_batch_pool(eq, sel, np.random.default_rng(s2), base, dtype=torch.float32, label_fill=-100)
    assert not torch.equal(plain, pa)


def test_train_class_head_hed_he_quality_equals_the_replay_by_hand(cuda, tmp_path):
    from classpose_amd import augment, synth
    from classpose_amd.train import HeadTrainer, lr_schedule, train_class_head
    ncls, bs, n_epochs, lr, seed = 7, 4, 2, 2e-3, 42
    sd = synth.make_state_dict(ncls, None, depth=1)
    ims, labs = _synthetic_ragged(ncls, TRAIN_SIZES)
    pool = augment.ImagePool(ims, labs, device=cuda)
    runs = []
    for k in range(2):
        t = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
        path, tl, _vl = train_class_head(t, pool, None, batch_size=bs, n_epochs=n_epochs, learning_rate=lr, save_path=tmp_path / f"run{k}",
                                         model_name="head", random_seed=seed, augment="hed_he_quality", scale_range=0.5, label_fill=-100)
        runs.append((t, path, tl))
    t, path, tl = runs[0]
    h = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    w0 = h.w.clone()
    LR = lr_schedule(lr, n_epochs)
    for ep in range(n_epochs):
        rng = np.random.default_rng([seed, ep])
        order = rng.permutation(6)
        sums, count = 0.0, 0
        for s in range(0, 6, bs):
            idx = order[s:s + bs]
            x, y = augment.augment_batch_pool(pool, idx, rng, "hed_he_quality", scale_range=0.5, label_fill=-100, dtype=h.dtype)
            r = h.step(x, y, float(LR[ep]))
            sums += r["loss"] * len(idx)
            count += len(idx)
        print(f"epoch {ep}: train loss {tl[ep]:.6f} (replay {sums / count:.6f})")
        assert tl[ep] == sums / count
    assert torch.equal(t.w, h.w) and torch.equal(t.b, h.b) and not torch.equal(t.w, w0)
    _t1, path1, tl1 = runs[1]
    assert np.array_equal(tl, tl1)
    for name in ("head", "checkpoint_last.pt", "checkpoint_best.pt"):
        assert (path.parent / name).read_bytes() == (path1.parent / name).read_bytes(), name
    # pre-cut crops are accepted too (two epochs: the schedule's first learning rate is 0)
    keep = [i for i, im in enumerate(ims) if im.shape[0] >= 256 and im.shape[1] >= 256]
    X, Y = np.stack([ims[i][:256, :256] for i in keep]), np.stack([labs[i][:256, :256] for i in keep])
    ta = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    _p, tla, _v = train_class_head(ta, X, Y, batch_size=bs, n_epochs=n_epochs, learning_rate=lr, save_path=tmp_path / "crops", model_name="head",
                                   random_seed=seed, augment="quality")
    assert np.isfinite(tla).all() and not torch.equal(ta.w, w0)


def test_cli_trains_with_hed_he_quality_in_a_child_process(cuda, tmp_path):
    from classpose_amd import synth
    ncls = 5
    sd = synth.make_state_dict(1, None, depth=1, seed=12)               # a plain backbone: the CLI initialises the head
    torch.save(sd, tmp_path / "backbone.pt")
    sizes = [(300, 280), (256, 256), (200, 333), (384, 260)]
    ims, _l = _synthetic_ragged(ncls, sizes)
    rng = np.random.default_rng(3)
    images, labels = np.empty(len(sizes), object), np.empty(len(sizes), object)
    for k, (h, w) in enumerate(sizes):
        lab = np.zeros((h, w, 2), np.int32)
        for c in range(6 + 3 * k):
            y0, x0, ch, cw = int(rng.integers(0, h - 30)), int(rng.integers(0, w - 30)), int(rng.integers(6, 26)), int(rng.integers(6, 26))
            lab[y0:y0 + ch, x0:x0 + cw, 0] = 1000 * k + c + 1
            lab[y0:y0 + ch, x0:x0 + cw, 1] = 1 + (3 * c) % 4
        images[k], labels[k] = ims[k], lab
    (tmp_path / "data").mkdir()
    np.save(tmp_path / "data" / "images.npy", images, allow_pickle=True)
    np.save(tmp_path / "data" / "labels.npy", labels, allow_pickle=True)
    cmd = [sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--data_path", str(tmp_path / "data"), "--train_fraction", "0.75",
           "--pretrained_model", str(tmp_path / "backbone.pt"), "--n_epochs", "2", "--batch_size", "4", "--learning_rate", "1e-3",
           "--augment", "hed_he_quality", "--save_path", str(tmp_path), "--model_name", "m", "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    assert "train_loss=" in r.stderr and "image pool:" in r.stderr
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["out_class.weight"].shape == (ncls * 64, 256, 1, 1)
