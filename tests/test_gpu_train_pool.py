"""Training windows from a device-resident pool of whole annotated images of any size (csrc/cpx_augment.hip t4 -> ops ->
classpose_amd.augment.ImagePool / augment_batch_pool / grid_crops -> train_class_head -> train_head --data_path).

Yardsticks: the kernels this one fuses (``ops.hed_jitter``, ``ops.warp_affine``: bitwise), numpy (byte sums, window slicing:
exact) and, for the ragged pool, the float64 restatement of tests/augment_reference.py under the bounds derived in
tests/test_gpu_augment.py: per element |device - float64| <= 8 * 2^-24 * 255, relative L2 err(device) <=
max(4 * err(float32 restatement), 2^-20), labels exact.  Every test prints the figures it observed before it asserts (-s)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_reference as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -20
WARP_ABS = 8 * 2.0 ** -24 * 255
SIZES = [(1, 1), (5, 7), (37, 53), (301, 299)]          # the 37 x 53 image makes every later byte offset odd


def _rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


def _ragged_images(sizes, seed):
    """uint8 images of values <= 250 (255 is the sentinel of the guarded pool) and class maps 0..6 with a -100 band."""
    rng = np.random.default_rng(seed)
    ims = [rng.integers(0, 251, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    labs = [rng.integers(0, 7, (h, w)).astype(np.int16) for h, w in sizes]
    for lab in labs:
        if lab.shape[0] > 8:
            lab[3:5] = -100
    return ims, labs


def _guarded_pool(ims, labs, dev, pad_u8=77, pad_lab=33):
    """The pool inside larger buffers of 255 / 32767 on both sides, at an odd byte offset: (pool_u8, pool_lab, px_off, hw)."""
    from classpose_amd import augment
    px_off, hw, total = augment.pool_table([im.shape[:2] for im in ims])
    buf = torch.full((pad_u8 + 3 * total + pad_u8,), 255, dtype=torch.uint8, device=dev)
    lbuf = torch.full((pad_lab + total + pad_lab,), 32767, dtype=torch.int16, device=dev)
    buf[pad_u8:pad_u8 + 3 * total] = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(dev)
    lbuf[pad_lab:pad_lab + total] = torch.from_numpy(np.concatenate([lab.reshape(-1) for lab in labs])).to(dev)
    return buf[pad_u8:pad_u8 + 3 * total], lbuf[pad_lab:pad_lab + total], torch.from_numpy(px_off).to(dev), torch.from_numpy(hw).to(dev)


def _centred_maps(rng, shapes, dh, dw, scales=(0.5, 2.0)):
    """Inverse maps that turn by a random angle and scale about the source's centre, which lands on the output's centre."""
    inv = np.empty((len(shapes), 6))
    for t, (h, w) in enumerate(shapes):
        th, s = rng.uniform(0, 2 * np.pi), rng.uniform(*scales)
        c, sn = np.cos(th) / s, np.sin(th) / s
        cx, cy, ox, oy = (w - 1) / 2 + rng.uniform(-0.3, 0.3), (h - 1) / 2 + rng.uniform(-0.3, 0.3), (dw - 1) / 2, (dh - 1) / 2
        inv[t] = [c, sn, cx - (c * ox + sn * oy), -sn, c, cy - (-sn * ox + c * oy)]
    return inv


# ---- 1. byte sums ---------------------------------------------------------------------------------------------------
def test_byte_sums_are_numpys_and_applied_is_hed_jitters(cuda):
    from classpose_amd import augment, ops
    rng = np.random.default_rng(1)
    ims, labs = _ragged_images(SIZES, 1)
    ims[1] = rng.integers(0, 31, (5, 7, 3), dtype=np.uint8)                # mean / 255 below 0.15
    ims[2] = rng.integers(230, 251, (37, 53, 3), dtype=np.uint8)           # above 0.85
    pool_u8, _pl, px_off, hw = _guarded_pool(ims, labs, cuda)
    assert pool_u8.data_ptr() % 2 == 1 and (3 * int(px_off[3])) % 2 == 1
    sums = ops.pool_byte_sums(pool_u8, px_off, hw).cpu().numpy()
    want = np.array([int(im.astype(np.int64).sum()) for im in ims])
    print("byte sums", sums.tolist(), "numpy", want.tolist())
    assert sums.dtype == np.int64 and np.array_equal(sums, want)
    pool = augment.ImagePool(ims, labs, device=cuda)
    assert np.array_equal(pool.byte_sums, want) and pool.nbytes == 5 * pool.pool_px + 16 * 4
    cut = augment.get_config("hed_only")["cutoff_range"]
    applied = pool.applied(cut)
    for i, im in enumerate(ims):
        _o, ap = ops.hed_jitter(torch.from_numpy(im[None]).to(cuda), np.zeros((1, 3), np.float32), np.zeros((1, 3), np.float32), cut)
        assert int(ap.item()) == int(applied[i]) == int(ar.hed_applied(im, cut)), i
    print("applied", applied.tolist())
    assert applied.tolist() == [int(ar.hed_applied(ims[0], cut)), 0, 0, 1]
    # a table entry that leaves the pool is refused without being read
    bad = px_off.clone()
    bad[3] += 1
    with pytest.raises(ValueError, match="outside the pool"):
        ops.pool_byte_sums(pool_u8, bad, hw)


# ---- 2. warp without jitter -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sh,sw", [(256, 256), (200, 333)])
def test_pool_warp_equals_warp_affine_bitwise(cuda, sh, sw):
    from classpose_amd import augment, ops
    rng = np.random.default_rng(sh)
    n = 8
    for dh, dw in ((16, 24), (256, 256)):
        ims, labs = _ragged_images([(sh, sw)] * n, sh + dh)
        _f, inv = augment.sample_affine(rng, n, sh, sw, dw, scale_range=0.5)
        inv[0] = [1, 0, 0, 0, 1, 0]                                         # identity
        inv[1] = [1, 0, 0.5, 0, 1, 0.5]                                     # half a pixel: every weight 0.5, labels on the rounding edge
        inv[2] = [1, 0, sw - dw / 2, 0, 1, sh - dh / 2]                     # mostly beyond the right and lower edges
        inv[3] = _centred_maps(rng, [(sh, sw)], dh, dw, (0.05, 0.06))[0]    # the whole source and a wide border around it
        pool_u8, pool_lab, px_off, hw = _guarded_pool(ims, labs, cuda)
        order = rng.permutation(n)                                          # crop t comes from image order[t]
        X, L = torch.from_numpy(np.stack(ims)[order]).to(cuda), torch.from_numpy(np.stack(labs)[order]).to(cuda)
        for fill in (0, -100):
            want, want_lab = ops.warp_affine(X, inv, (dh, dw), L, fill)
            got, got_lab, status = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, order, inv, (dh, dw), label_fill=fill)
            assert int(status.item()) == 0
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_lab, want_lab), (dh, dw, fill)
        assert (got_lab[2] == -100).float().mean() > 0.5 and got[3].any() and (got[3] == 0).float().mean() > 0.3
        if (dh, dw) == (16, 24):
            assert np.array_equal(got[0].cpu().numpy(), ims[order[0]][:16, :24].transpose(2, 0, 1).astype(np.float32))
        only, none, _s = ops.warp_affine_pool(pool_u8, None, px_off, hw, order, inv, (dh, dw))
        assert none is None and torch.equal(only, want)
        print(f"{sh}x{sw} -> {dh}x{dw}: pool kernel bitwise equal to warp_affine on {n} crops, both label fills")


# ---- 3. fused jitter ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("simple_mode", [False, True])
def test_fused_jitter_equals_hed_jitter_then_warp_bitwise(cuda, simple_mode):
    from classpose_amd import augment, ops
    rng = np.random.default_rng(31 + simple_mode)
    nI, sh, sw, dh, dw = 6, 64, 80, 16, 24
    ims, labs = _ragged_images([(sh, sw)] * nI, 32)
    ims[1] = rng.integers(0, 31, (sh, sw, 3), dtype=np.uint8)              # below the cut-off: copied unchanged
    ims[4] = rng.integers(230, 251, (sh, sw, 3), dtype=np.uint8)           # above it
    ims[2][:8] = 0
    ims[2][8:16] = 250
    cfg = augment.get_config("hed_only")
    image_of = np.array([0, 1, 2, 3, 4, 5, 2, 2, 0, 5, 1, 3])
    n = len(image_of)
    sigma, bias = augment.sample_hed(rng, n, cfg["sigma_ranges"], cfg["bias_ranges"])
    inv = _centred_maps(rng, [(sh, sw)] * n, dh, dw, (0.2, 1.5))
    inv[6] = [1, 0, 0, 0, 1, 0]
    inv[7] = [1, 0, sw - 3.25, 0, 1, sh - 2.5]                              # mostly outside: only a corner of the source is seen
    inv[8] = [1, 0, -20.5, 0, 1, -13.75]                                    # mostly outside on the other side
    inv[9] = [1, 0, 500.0, 0, 1, 0]                                         # entirely outside
    X, L = torch.from_numpy(np.stack(ims)).to(cuda), torch.from_numpy(np.stack(labs)).to(cuda)
    ti = torch.from_numpy(image_of).to(cuda)
    jit, applied = ops.hed_jitter(X[ti], sigma, bias, cfg["cutoff_range"], simple_mode)          # the whole images, then the warp
    want, want_lab = ops.warp_affine(jit, inv, (dh, dw), L[ti], 0)
    pool = augment.ImagePool(ims, labs, device=cuda)
    ap = pool.applied(cfg["cutoff_range"])[image_of]
    assert np.array_equal(ap, applied.cpu().numpy()) and ap.tolist() == [1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0, 1]
    got, got_lab, status = ops.warp_affine_pool(pool.pool_u8, pool.pool_lab, pool.px_off, pool.hw, image_of, inv, (dh, dw), sigma, bias, ap,
                                                simple_mode, 0)
    plain, _l, _s = ops.warp_affine_pool(pool.pool_u8, pool.pool_lab, pool.px_off, pool.hw, image_of, inv, (dh, dw))
    differ = int((got != want).sum())
    print(f"simple_mode={simple_mode}: {differ} of {want.numel()} values differ from hed_jitter -> warp_affine; "
          f"{int((got != plain).sum())} differ from the unjittered warp")
    assert int(status.item()) == 0 and torch.equal(got.view(torch.int32), want.view(torch.int32)) and torch.equal(got_lab, want_lab)
    assert not torch.equal(got[0], plain[0]) and torch.equal(got[1], plain[1]) and torch.equal(got[4], plain[4]) and torch.equal(got[10], plain[10])
    assert not got[9].any() and (got[7] == 0).float().mean() > 0.8 and got[7].any() and got[8].any()


# ---- 4. ragged pool -------------------------------------------------------------------------------------------------
def test_ragged_pool_against_the_float64_restatement(cuda):
    from classpose_amd import augment, ops
    sizes = SIZES + [(256, 256)]
    ims, labs = _ragged_images(sizes, 4)
    pool_u8, pool_lab, px_off, hw = _guarded_pool(ims, labs, cuda)
    rng = np.random.default_rng(44)
    image_of = np.array([3, 0, 4, 1, 2, 2, 4, 0, 3, 1, 4, 3])              # every image, scrambled, with repeats
    assert set(image_of) == set(range(5))
    n, dh, dw = len(image_of), 16, 24
    shapes = [sizes[i] for i in image_of]
    inv = _centred_maps(rng, shapes, dh, dw)
    inv[6] = [1, 0, 240.0, 0, 1, 248.0]                                     # the lower right corner of the 256 x 256 image and beyond
    inv[8] = [1, 0, 0.5, 0, 1, 290.25]                                      # the last rows of the 301 x 299 image: the pool's last bytes
    for t in range(n):                                                      # nearest-neighbour sampling away from half-integer coordinates
        if t != 8:
            assert ar.half_integer_distance(inv[t], dh, dw) > 1e-9, t
    got, got_lab, status = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), label_fill=-100)
    got, got_lab = got.cpu().numpy(), got_lab.cpu().numpy()
    assert int(status.item()) == 0 and got.shape == (n, 3, dh, dw) and got_lab.shape == (n, dh, dw)
    assert got.max() <= 250 and got.min() >= 0 and (got_lab != 32767).all() and (np.abs(got_lab) <= 100).all()      # no sentinel shows
    seen = 0
    for t, i in enumerate(image_of):
        chw = ims[i].transpose(2, 0, 1)
        r64, r32 = ar.warp_image(chw, inv[t], dh, dw, np.float64), ar.warp_image(chw, inv[t], dh, dw, np.float32)
        worst, e_dev, e_32 = float(np.abs(got[t] - r64).max()), _rel_l2(got[t], r64), _rel_l2(r32, r64)
        tol = max(4 * e_32, FLOOR)
        print(f"crop {t} of image {i} {sizes[i]}: max |device - float64| = {worst:.3e} (bound {WARP_ABS:.3e}), err(device) = {e_dev:.3e}, "
              f"err(float32 restatement) = {e_32:.3e}, tolerance = {tol:.3e}")
        assert worst <= WARP_ABS, (t, worst)
        assert e_dev <= tol, (t, e_dev, tol)
        seen += bool(r64.any())
        assert np.array_equal(got_lab[t], ar.warp_labels(labs[i], inv[t], dh, dw, -100)), t      # crop 8: an exact translation
    assert seen >= n - 1
    # with the stain jitter: every crop is hed_jitter of its own whole image, then warp_affine of it, bitwise
    cfg = augment.get_config("hed_only")
    sigma, bias = augment.sample_hed(rng, n, cfg["sigma_ranges"], cfg["bias_ranges"])
    ap = np.array([int(ar.hed_applied(ims[i], cfg["cutoff_range"])) for i in image_of], np.int32)
    fused, fl, _s = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), sigma, bias, ap, False, -100)
    for t, i in enumerate(image_of):
        j, a = ops.hed_jitter(torch.from_numpy(ims[i][None]).to(cuda), sigma[t:t + 1], bias[t:t + 1], cfg["cutoff_range"], False)
        w, lw = ops.warp_affine(j, inv[t:t + 1], (dh, dw), torch.from_numpy(labs[i][None]).to(cuda), -100)
        assert int(a.item()) == ap[t] and torch.equal(fused[t].view(torch.int32), w[0].view(torch.int32)) and torch.equal(fl[t], lw[0]), t
    assert (fl != 32767).all()


# ---- 5. image index out of range ------------------------------------------------------------------------------------
def test_image_index_out_of_range_is_never_dereferenced(cuda):
    from classpose_amd import ops
    ims, labs = _ragged_images(SIZES, 5)
    pool_u8, pool_lab, px_off, hw = _guarded_pool(ims, labs, cuda)
    nI, dh, dw = len(ims), 16, 24
    inv = np.tile(np.array([1.0, 0, 0.25, 0, 1.0, 0.25]), (5, 1))
    good = np.array([3, 2, 3, 1, 2])
    want, want_lab, st0 = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, good, inv, (dh, dw), label_fill=-7)
    bad = good.copy()
    bad[1], bad[3] = nI, -1
    with pytest.raises(ValueError, match="image index outside the pool"):
        ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, bad, inv, (dh, dw), label_fill=-7)
    got, got_lab, st = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, bad, inv, (dh, dw), label_fill=-7, check_status=False)
    print("status", int(st0.item()), "->", int(st.item()))
    assert int(st0.item()) == 0 and int(st.item()) == 1
    for t in (1, 3):
        assert not got[t].any() and bool((got_lab[t] == -7).all())
    for t in (0, 2, 4):
        assert torch.equal(got[t], want[t]) and torch.equal(got_lab[t], want_lab[t]) and got[t].any()
    # the status word is cleared by the next call
    _g, _l, st2 = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, good, inv, (dh, dw), label_fill=-7)
    assert int(st2.item()) == 0


# ---- 6. grid crops --------------------------------------------------------------------------------------------------
def test_grid_crops_equal_numpy_slicing(cuda):
    from classpose_amd import augment
    sizes = [(300, 520), (100, 300), (256, 600)]
    ims, labs = _ragged_images(sizes, 6)
    labs[2][:, 344:] = -100                                                 # the last window of image 2 has no annotated pixel
    pool = augment.ImagePool(ims, labs, device=cuda)
    x, y, win = augment.grid_crops(pool)
    want_win = [[0, 0, 0], [0, 0, 132], [0, 0, 264], [0, 44, 0], [0, 44, 132], [0, 44, 264], [1, 0, 0], [1, 0, 44], [2, 0, 0], [2, 0, 172]]
    assert win.tolist() == want_win and [2, 0, 344] in augment.grid_windows(pool.hw_host).tolist()
    assert x.dtype == torch.uint8 and tuple(x.shape) == (10, 256, 256, 3) and y.dtype == torch.int16 and tuple(y.shape) == (10, 256, 256)
    x, y = x.cpu().numpy(), y.cpu().numpy()
    for k, (i, y0, x0) in enumerate(want_win):
        im = np.zeros((256, 256, 3), np.uint8)
        lab = np.full((256, 256), -100, np.int16)
        part, lpart = ims[i][y0:y0 + 256, x0:x0 + 256], labs[i][y0:y0 + 256, x0:x0 + 256]
        im[:part.shape[0], :part.shape[1]], lab[:part.shape[0], :part.shape[1]] = part, lpart
        assert np.array_equal(x[k], im) and np.array_equal(y[k], lab), (k, i, y0, x0)
    assert not x[6][100:].any() and (y[6][100:] == -100).all() and x[6][:100].any()          # below the 100 rows: padding
    assert augment.grid_crops(pool)[0] is pool._grid[0]                                      # cached on the pool
    print("10 of 11 windows kept, every pixel and label equal to numpy slicing")


# ---- 7. training replay ---------------------------------------------------------------------------------------------
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


def test_train_class_head_from_a_pool_equals_the_replay_by_hand(cuda, tmp_path):
    from classpose_amd import augment, synth
    from classpose_amd.train import HeadTrainer, lr_schedule, train_class_head
    ncls, bs, n_epochs, lr, seed = 7, 4, 2, 2e-3, 42
    sd = synth.make_state_dict(ncls, None, depth=1, seed=11)
    sizes = [(300, 280), (256, 256), (200, 333), (384, 260), (270, 400), (512, 300)]
    ims, labs = _synthetic_ragged(ncls, sizes)
    probs = np.array([4.0, 0.0, 1.0, 1.0, 2.0, 0.5])                        # not normalised; image 1 is never drawn
    diam = np.array([12.0, 30.0, 45.0, 20.0, 36.0, 60.0])
    pool = augment.ImagePool(ims, labs, diam, device=cuda)
    test_pool = augment.ImagePool(ims[4:], labs[4:], device=cuda)
    runs = []
    for k in range(2):
        t = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
        path, tl, vl = train_class_head(t, pool, None, test_pool, None, batch_size=bs, n_epochs=n_epochs, learning_rate=lr,
                                        save_path=tmp_path / f"run{k}", model_name="head", random_seed=seed, augment="hed_only",
                                        scale_range=0.5, train_probs=probs, rescale=True, diam_mean=30.0)
        runs.append((t, path, tl, vl))
    t, path, tl, vl = runs[0]
    h = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    w0 = h.w.clone()
    LR = lr_schedule(lr, n_epochs)
    vx, vy, vwin = augment.grid_crops(test_pool)
    assert len(vwin) == len(augment.grid_windows(test_pool.hw_host)) == 2 * 2 + 2 * 2
    drawn = []
    for ep in range(n_epochs):
        rng = np.random.default_rng([seed, ep])
        order = rng.choice(6, 6, p=probs / probs.sum())                     # over the IMAGES: one window per draw
        drawn += order.tolist()
        sums, count = 0.0, 0
        for s in range(0, 6, bs):
            idx = order[s:s + bs]
            x, y = augment.augment_batch_pool(pool, idx, rng, "hed_only", scale_range=0.5, label_fill=0, dtype=h.dtype,
                                              rescale=diam[idx] / 30.0)
            r = h.step(x, y, float(LR[ep]))
            sums += r["loss"] * len(idx)
            count += len(idx)
        tsum, tcount = 0.0, 0
        for s in range(0, len(vx), bs):                                     # validation: the cached grid crops, never augmented
            r = h.evaluate(vx[s:s + bs], vy[s:s + bs])
            tsum += r["loss"] * r["n"]
            tcount += r["n"]
        print(f"epoch {ep}: train loss {tl[ep]:.6f} (replay {sums / count:.6f}), validation loss {vl[ep]:.6f} (replay {tsum / tcount:.6f})")
        assert tl[ep] == sums / count and vl[ep] == tsum / tcount
    assert 1 not in drawn and len(set(drawn)) < len(drawn)
    assert torch.equal(t.w, h.w) and torch.equal(t.b, h.b) and not torch.equal(t.w, w0)
    _t1, path1, tl1, vl1 = runs[1]
    assert np.array_equal(tl, tl1) and np.array_equal(vl, vl1)
    for name in ("head", "checkpoint_last.pt", "checkpoint_best.pt"):
        assert (path.parent / name).read_bytes() == (path1.parent / name).read_bytes(), name
    # a pool of equal-sized crops is bitwise augment_batch of the same crops
    eq_ims, eq_labs = _synthetic_ragged(ncls, [(256, 256)] * 4)
    eq = augment.ImagePool(eq_ims, eq_labs, device=cuda)
    idx = np.array([2, 0, 3, 3])
    pa, la = augment.augment_batch_pool(eq, idx, np.random.default_rng(9), "hed_only", dtype=torch.float32)
    pb, lb = augment.augment_batch(np.stack(eq_ims)[idx], np.stack(eq_labs)[idx], np.random.default_rng(9), "hed_only", dtype=torch.float32,
                                   device=cuda)
    assert torch.equal(pa, pb) and torch.equal(la, lb)
    # without augment the pool trains on its grid crops like the arrays they are
    ta, tb = (HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4) for _ in range(2))
    gx, gy, _w = augment.grid_crops(pool)
    _p, tla, _v = train_class_head(ta, pool, None, batch_size=bs, n_epochs=2, learning_rate=lr, save_path=tmp_path / "ga", model_name="head")
    _p, tlb, _v = train_class_head(tb, gx.cpu().numpy(), gy.cpu().numpy(), batch_size=bs, n_epochs=2, learning_rate=lr,
                                   save_path=tmp_path / "gb", model_name="head")
    assert np.array_equal(tla, tlb) and torch.equal(ta.w, tb.w)
    with pytest.raises(ValueError, match="labels=None"):
        train_class_head(ta, pool, np.zeros((6, 256, 256), np.int16), save_path=tmp_path / "x", model_name="head")
    with pytest.raises(ValueError, match="transform"):
        train_class_head(ta, pool, None, save_path=tmp_path / "x", model_name="head", transform=lambda x, y, r: (x, y))


# ---- 8. command line ------------------------------------------------------------------------------------------------
def test_cli_trains_from_a_data_directory_in_a_child_process(cuda, tmp_path):
    from classpose_amd import dataset_stats as ds, models, synth, train_data
    ncls = 5
    sd = synth.make_state_dict(1, None, depth=1, seed=12)               # a plain backbone: the CLI initialises the head
    torch.save(sd, tmp_path / "backbone.pt")
    sizes = [(300, 280), (256, 256), (200, 333), (384, 260), (270, 400), (260, 300)]
    ims, _l = _synthetic_ragged(ncls, sizes)
    rng = np.random.default_rng(3)
    images, labels = np.empty(6, object), np.empty(6, object)
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
    cmd = [sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--data_path", str(tmp_path / "data"), "--train_fraction", "0.7",
           "--pretrained_model", str(tmp_path / "backbone.pt"), "--n_epochs", "2", "--batch_size", "4", "--learning_rate", "1e-3",
           "--auto_class_weights", "--oversampling_method", "custom", "--rescale", "--augment", "hed_only", "--save_path",
           str(tmp_path), "--model_name", "m", "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    log = r.stderr
    data = train_data.load_dataset(tmp_path / "data")
    tr, te = train_data.split_indices(6, 0.7, 42)
    assert len(tr) == 4 and len(te) == 2 and data.n_classes == ncls
    counts = np.bincount(np.concatenate([data.classes[i][data.classes[i] >= 0].astype(np.int64) for i in tr]), minlength=ncls)
    weights = ds.get_class_weights(counts)
    assert "inferred number of classes: 5" in log and f"class weights = {weights.tolist()}" in log, log[-3000:]
    assert "4 training images, 2 validation images" in log and "n_train=4" in log and "test_loss=" in log
    assert "Custom oversampling - probability range:" in log and "diameters:" in log and "image pool:" in log
    m = models.ClassposeModel(pretrained_model=str(out), device=cuda, precision="bf16", max_batch_tiles=2)
    assert m.nclasses == ncls
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["out_class.weight"].shape == (ncls * 64, 256, 1, 1)
