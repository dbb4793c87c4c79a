"""H&E stain-matrix perturbation on the device (csrc/cpx_augment.hip t5 -> ops.stain_samples / he_stain / warp_affine_pool_stain ->
augment "he_staining" / "hed_he" -> train_class_head -> train_head --augment).

Yardsticks: numpy for the tissue samples (exact), the reference-minted fixture tests/golden/reference_stain.npz and the float64
restatement tests/stain_reference.py for the transform (a value may be off by one level only where the restatement's
255 exp(-x) lies within 1e-9 of an integer, and at most 1e-6 of the values may use that), and the kernels the fused pool kernel
composes (bitwise).  Every test prints the figures it observed before it asserts (-s)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stain_reference as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SENTINEL = 254                                           # fills the guards around the pool; no image holds it
SIZES = [(1, 1), (5, 7), (37, 53), (301, 299), (256, 256)]          # the 37 x 53 image makes every later byte offset odd
TRUE_BASIS = np.array([[0.65, 0.70, 0.29], [0.07, 0.99, 0.11]])


def _guarded_pool(ims, dev, labs=None, pad=77):
    """The pool inside a larger buffer of sentinel bytes on both sides, at an odd byte offset."""
    from classpose_amd import augment
    px_off, hw, total = augment.pool_table([im.shape[:2] for im in ims])
    buf = torch.full((pad + 3 * total + pad,), SENTINEL, dtype=torch.uint8, device=dev)
    buf[pad:pad + 3 * total] = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(dev)
    pool_lab = None
    if labs is not None:
        pool_lab = torch.from_numpy(np.concatenate([lab.reshape(-1) for lab in labs])).to(dev)
    return buf, buf[pad:pad + 3 * total], pool_lab, torch.from_numpy(px_off).to(dev), torch.from_numpy(hw).to(dev)


def _numpy_samples(img):
    """extract_stains' selection, on the bytes: density[mask] (all pixels when the mask is empty), [::128] beyond 128."""
    from classpose_amd import stain
    values = img[stain.tissue_mask(img)]
    k = len(values)
    if k == 0:
        values = img.reshape(-1, 3)
    return (values[::128] if len(values) > 128 else values), k


def _sample_images():
    rng = np.random.default_rng(21)
    ims = [rng.integers(0, 254, (h, w, 3), dtype=np.uint8) for h, w in SIZES]

    def bright(h, w):
        return rng.integers(240, 254, (h, w, 3), dtype=np.uint8)

    def with_tissue(h, w, positions):
        im = bright(h, w)
        im.reshape(-1, 3)[np.asarray(positions)] = rng.integers(0, 90, (len(positions), 3), dtype=np.uint8)
        return im
    edges = [0, 63, 64, 255, 256, 1023, 1024, 1025, 2047, 2048, 3071, 3072, 4095, 4096, 64 * 67 - 1]
    ims.append(bright(20, 30))                                                          # no tissue pixel: every pixel is a value
    ims.append(with_tissue(40, 50, rng.choice(2000, 128, replace=False)))               # exactly 128: all of them
    ims.append(with_tissue(40, 50, rng.choice(2000, 129, replace=False)))               # 129: ranks 0 and 128
    ims.append(with_tissue(64, 67, edges))                                              # around the chunk and wave boundaries
    ims.append(with_tissue(64, 67, sorted(set(edges) | set(range(5, 64 * 67, 7)))))     # the same, with a stride pick across them
    names = [f"{h}x{w}" for h, w in SIZES] + ["none", "exactly128", "129", "edges", "edges_stride"]
    return ims, names


# ---- 1. tissue samples ----------------------------------------------------------------------------------------------
def test_stain_samples_equal_numpy_on_a_ragged_pool(cuda):
    from classpose_amd import ops, stain
    ims, names = _sample_images()
    buf, pool_u8, _lab, px_off, hw = _guarded_pool(ims, cuda)
    assert pool_u8.data_ptr() % 2 == 1
    k, samples, status, raw = ops.stain_samples(pool_u8, px_off, hw)
    want = [_numpy_samples(im) for im in ims]
    for name, im, (w, wk), got, gk in zip(names, ims, want, samples, k):
        print(f"{name}: {gk} tissue pixels of {im.shape[0] * im.shape[1]}, {len(got)} samples")
        assert gk == wk and got.shape == w.shape and np.array_equal(got, w), name
    by = dict(zip(names, k))
    assert by["none"] == 0 and len(samples[names.index("none")]) == 5 and by["exactly128"] == 128 and by["129"] == 129
    assert len(samples[names.index("exactly128")]) == 128 and len(samples[names.index("129")]) == 2
    assert by["edges"] == 15 and by["edges_stride"] > 128 and by["301x299"] > 128 * 128
    assert int(status.item()) == 0
    # nothing but the selected samples was written, and no guard byte came through
    raw = raw.cpu().numpy()
    cap = stain.sample_capacity([im.shape[0] * im.shape[1] for im in ims])
    off = np.concatenate([[0], np.cumsum(cap)[:-1]])
    for o, c, s in zip(off, cap, samples):
        assert not raw[o + len(s):o + c].any()
    assert not (raw == SENTINEL).any() and len(raw) == cap.sum()
    assert bool((buf[:77] == SENTINEL).all()) and bool((buf[-77:] == SENTINEL).all())
    # the result does not depend on where the samples go: offsets in reverse order, with gaps
    off2 = np.concatenate([[0], np.cumsum(cap[::-1] + 3)[:-1]])[::-1].astype(np.int64)
    k2, samples2, _st, _raw = ops.stain_samples(pool_u8, px_off, hw, out_off=off2, out_triples=int((cap + 3).sum()))
    assert np.array_equal(k2, k) and all(np.array_equal(a, b) for a, b in zip(samples, samples2))


def test_stain_samples_refuse_bad_tables_and_leave_neighbours_alone(cuda):
    from classpose_amd import ops, stain
    ims, _names = _sample_images()
    _buf, pool_u8, _lab, px_off, hw = _guarded_pool(ims, cuda)
    k, samples, _st, raw = ops.stain_samples(pool_u8, px_off, hw)
    bad = px_off.clone()
    bad[3] = pool_u8.numel() // 3 - 5                                    # the 301 x 299 image would run off the pool's end
    with pytest.raises(ValueError, match="outside the pool"):
        ops.stain_samples(pool_u8, bad, hw)
    kb, sb, st, rawb = ops.stain_samples(pool_u8, bad, hw, check_status=False)
    assert int(st.item()) == 2 and kb[3] == 0
    cap = stain.sample_capacity([im.shape[0] * im.shape[1] for im in ims])
    off = np.concatenate([[0], np.cumsum(cap)[:-1]])
    rawb, raw = rawb.cpu().numpy(), raw.cpu().numpy()
    assert not rawb[off[3]:off[3] + cap[3]].any()                       # nothing written for the bad image
    for i in range(len(ims)):
        if i != 3:
            assert kb[i] == k[i] and np.array_equal(sb[i], samples[i]) and np.array_equal(rawb[off[i]:off[i] + cap[i]], raw[off[i]:off[i] + cap[i]])
    # an output range outside the buffer: bit 2, that image alone is skipped
    short = off.copy()
    short[-1] = cap.sum()                                                # starts where the buffer ends
    with pytest.raises(ValueError, match="output buffer"):
        ops.stain_samples(pool_u8, px_off, hw, out_off=short, out_triples=int(cap.sum()))
    ko, so, st, _r = ops.stain_samples(pool_u8, px_off, hw, out_off=short, out_triples=int(cap.sum()), check_status=False)
    assert int(st.item()) == 4 and ko[-1] == 0 and np.array_equal(ko[:-1], k[:-1]) and np.array_equal(so[0], samples[0])
    st2 = ops.stain_samples(pool_u8, px_off, hw)[2]
    assert int(st2.item()) == 0                                          # the status word is cleared by the next call


# ---- 2. the transform -----------------------------------------------------------------------------------------------
def test_he_stain_equals_the_reference_fixture_exactly(cuda):
    from classpose_amd import ops, stain
    with open(os.path.join(GOLD, "reference_stain.json")) as f:
        meta = json.load(f)
    npz = np.load(os.path.join(GOLD, "reference_stain.npz"))
    cfg = meta["config"]
    for c in meta["cases"]:
        img, H = npz[c["name"] + "_in"], npz[c["name"] + "_H"]
        params = stain.stain_params(H, np.linalg.pinv(H), c["U"], c["u"], cfg["amount_matrix"], cfg["amount_stains"])
        out = ops.he_stain(torch.from_numpy(img[None]).to(cuda), params[None], [2]).cpu().numpy()[0]
        ref = npz[c["name"] + "_out"]
        print(f"{c['name']}: {int((out != ref).sum())} of {ref.size} values differ from augment_stains")
        assert np.array_equal(out, ref), c["name"]
        same = ops.he_stain(torch.from_numpy(img[None]).to(cuda), params[None], [0]).cpu().numpy()[0]
        assert np.array_equal(same, img)


def _random_params(rng, n):
    from classpose_amd import stain
    out = np.empty((n, 14))
    for t in range(n):
        H = TRUE_BASIS + rng.uniform(-0.05, 0.05, (2, 3))
        H = H / np.linalg.norm(H, axis=1, keepdims=True)
        out[t] = stain.stain_params(H, np.linalg.pinv(H), rng.uniform(-1, 1, (2, 3)), rng.uniform(-1, 1, 2), 0.15, 0.4)
    return out


def test_he_stain_batch_of_32_against_float64(cuda):
    from classpose_amd import ops
    rng = np.random.default_rng(5)
    n = 32
    X = rng.integers(0, 256, (n, 256, 256, 3), dtype=np.uint8)
    conc = rng.random((8, 256, 256, 2)) * 2.0                            # a quarter of the crops are rendered tissue
    X[:8] = np.clip(255 * np.exp(-(conc @ TRUE_BASIS)) + rng.normal(0, 3, (8, 256, 256, 3)), 0, 255).astype(np.uint8)
    params = _random_params(rng, n)
    mode = np.where(np.arange(n) % 5 == 3, 0, 2).astype(np.int32)
    mode[7] = 1                                                         # any mode but 2 is a copy here
    out = ops.he_stain(torch.from_numpy(X).to(cuda), params, mode).cpu().numpy()
    differ = window = size = 0
    for t in range(n):
        if mode[t] != 2:
            assert np.array_equal(out[t], X[t]), t
            continue
        ref, v64, exact = sr.he_stain(X[t], params[t])
        r = sr.check_against(out[t], ref, v64, exact)
        differ, window, size = differ + r["differ"], window + r["in_window"], size + r["size"]
        assert (out[t] != X[t]).any()
    print(f"{differ} of {size} values differ from the float64 restatement, all among the {window} inside the 1e-9 window")
    assert differ <= 1e-6 * size


# ---- 3. the fused pool kernel ---------------------------------------------------------------------------------------
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


def test_fused_pool_kernel_equals_its_parts_bitwise(cuda):
    from classpose_amd import ops
    rng = np.random.default_rng(8)
    ims = [rng.integers(0, 254, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    labs = [rng.integers(0, 7, (h, w)).astype(np.int16) for h, w in SIZES]
    _buf, pool_u8, pool_lab, px_off, hw = _guarded_pool(ims, cuda, labs)
    image_of = np.array([3, 0, 4, 2, 1, 3, 3, 4, 2, 0, 1, 4, 4, 3, 2], np.int32)       # scrambled, with repeats
    n, (dh, dw) = len(image_of), (64, 48)
    inv = _pool_maps([SIZES[i] for i in image_of], dh, dw, rng)
    mode = np.array([2, 2, 1, 0, 2, 1, 0, 2, 2, 1, 0, 0, 2, 2, 1], np.int32)
    params = _random_params(rng, n)
    sigma, bias = (rng.uniform(-0.25, 0.25, (n, 3)).astype(np.float32) for _ in range(2))
    got, got_lab, status = ops.warp_affine_pool_stain(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias, False,
                                                      params, label_fill=-100)
    assert int(status.item()) == 0 and got.dtype == torch.float32 and tuple(got.shape) == (n, 3, dh, dw)
    differ = 0
    for t, i in enumerate(image_of):
        whole = torch.from_numpy(ims[i][None]).to(cuda)
        lab = torch.from_numpy(labs[i][None]).to(cuda)
        one = np.array([i], np.int32)
        if mode[t] == 2:                                                 # he_stain of the whole image, then warp_affine of it
            want, want_lab = ops.warp_affine(ops.he_stain(whole, params[t:t + 1], [2]), inv[t:t + 1], (dh, dw), lab, -100)
        elif mode[t] == 1:                                               # the existing pool kernel with the same jitter
            want, want_lab, _s = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, one, inv[t:t + 1], (dh, dw), sigma[t:t + 1],
                                                      bias[t:t + 1], [1], False, -100)
        else:                                                            # the existing pool kernel without jitter
            want, want_lab, _s = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, one, inv[t:t + 1], (dh, dw), label_fill=-100)
        d = int((got[t] != want[0]).sum())
        differ += d
        assert d == 0 and torch.equal(got_lab[t], want_lab[0]), (t, int(i), int(mode[t]))
    plain, _l, _s = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), label_fill=-100)
    changed = [bool((got[t] != plain[t]).any()) for t in range(n)]
    print(f"{differ} values differ from the parts; crops changed by their colour transform: {changed}")
    assert all(changed[t] == (mode[t] != 0) for t in range(n) if image_of[t] != 0 and (plain[t] != 0).any())
    # all crops in mode 0 / mode 1 are the existing entry, whole batch at once
    m0, l0, _s = ops.warp_affine_pool_stain(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), np.zeros(n, np.int32), label_fill=-100)
    assert torch.equal(m0, plain) and torch.equal(l0, _l)
    m1, _l1, _s = ops.warp_affine_pool_stain(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), np.ones(n, np.int32), sigma, bias,
                                             label_fill=-100)
    j1, _l2, _s = ops.warp_affine_pool(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), sigma, bias, np.ones(n, np.int32), False, -100)
    assert torch.equal(m1, j1)
    with pytest.raises(ValueError, match="mode 2 needs params"):
        ops.warp_affine_pool_stain(pool_u8, pool_lab, px_off, hw, image_of, inv, (dh, dw), mode, sigma, bias)
    bad = image_of.copy()
    bad[4] = 99
    with pytest.raises(ValueError, match="image index"):
        ops.warp_affine_pool_stain(pool_u8, pool_lab, px_off, hw, bad, inv, (dh, dw), mode, sigma, bias, False, params)


# ---- 4. the loop ----------------------------------------------------------------------------------------------------
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


def test_augment_batch_pool_hed_he_equals_the_ops_by_hand(cuda):
    from classpose_amd import augment, ops, stain
    ims, labs = _synthetic_ragged(7, TRAIN_SIZES)
    pool = augment.ImagePool(ims, labs, device=cuda)
    bases = pool.stain_basis()
    assert pool.stain_basis() is bases and len(bases) == 6 and bases.ok.all()
    for i, im in enumerate(ims):                                          # the device's samples are the host's, so is the basis
        H, Hinv = stain.image_basis(im)
        assert np.array_equal(bases.H[i], H) and np.array_equal(bases.Hinv[i], Hinv)
    cfg = augment.get_config("hed_he")
    idx = np.array([5, 0, 3, 3, 1, 2, 4, 0, 5, 2, 1, 4])
    got, got_lab = augment.augment_batch_pool(pool, idx, np.random.default_rng(77), "hed_he", dtype=torch.float32)
    p = augment.sample_batch_params_pool(pool, idx, np.random.default_rng(77), cfg)
    mode, params = augment.stain_mode_params(p, cfg, bases.take(idx), pool.applied(cfg["cutoff_range"])[idx])
    print(f"modes of the 12 crops: {mode.tolist()}")
    assert {1, 2} <= set(mode.tolist())
    xs, ls = [], []
    for t, i in enumerate(idx):
        whole = torch.from_numpy(ims[i][None]).to(cuda)
        if mode[t] == 2:
            whole = ops.he_stain(whole, params[t:t + 1], [2])
        elif p.use_hed[t]:
            whole, _a = ops.hed_jitter(whole, p.sigma[t:t + 1], p.bias[t:t + 1], cfg["cutoff_range"], False)
        x, lab = ops.warp_affine(whole, p.inv[t:t + 1], (256, 256), torch.from_numpy(labs[i][None]).to(cuda), 0)
        xs.append(x)
        ls.append(lab)
    x = torch.cat(xs)
    want = ops.patchify_f32(ops.normalize_img_f32(x, out=x), torch.float32)
    assert torch.equal(got, want) and torch.equal(got_lab, torch.cat(ls))
    # he_staining alone, and the crop path with and without bases handed in, against a pool of the same crops
    eq_ims, eq_labs = _synthetic_ragged(7, [(256, 256)] * 4)
    eq = augment.ImagePool(eq_ims, eq_labs, device=cuda)
    sel = np.array([2, 0, 3, 3])
    X, Y = np.stack(eq_ims)[sel], np.stack(eq_labs)[sel]
    for name in ("he_staining", "hed_he"):
        pa, la = augment.augment_batch_pool(eq, sel, np.random.default_rng(9), name, dtype=torch.float32, label_fill=-100)
        pb, lb = augment.augment_batch(X, Y, np.random.default_rng(9), name, dtype=torch.float32, device=cuda, label_fill=-100)
        pc, lc = augment.augment_batch(X, Y, np.random.default_rng(9), name, dtype=torch.float32, device=cuda, label_fill=-100,
                                       stain_bases=augment.stain_bases_of(np.stack(eq_ims), cuda).take(sel))
        assert torch.equal(pa, pb) and torch.equal(la, lb) and torch.equal(pb, pc) and torch.equal(lb, lc), name
    plain, _l = augment.augment_batch_pool(eq, sel, np.random.default_rng(9), "geometry", dtype=torch.float32)
    assert not torch.equal(plain, pa)


def test_train_class_head_hed_he_equals_the_replay_by_hand(cuda, tmp_path):
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
                                         model_name="head", random_seed=seed, augment="hed_he", scale_range=0.5, label_fill=-100)
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
            x, y = augment.augment_batch_pool(pool, idx, rng, "hed_he", scale_range=0.5, label_fill=-100, dtype=h.dtype)
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
    # pre-cut crops: the bases are fitted once for the set, and the run is the replay with them handed in
    keep = [i for i, im in enumerate(ims) if im.shape[0] >= 256 and im.shape[1] >= 256]
    X, Y = np.stack([ims[i][:256, :256] for i in keep]), np.stack([labs[i][:256, :256] for i in keep])
    ta, tb = (HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4) for _ in range(2))
    _p, tla, _v = train_class_head(ta, X, Y, batch_size=bs, n_epochs=n_epochs, learning_rate=lr, save_path=tmp_path / "crops",
                                   model_name="head", random_seed=seed, augment="he_staining")
    bases = augment.stain_bases_of(X, cuda)
    assert len(bases) == len(X) == 5
    for ep in range(n_epochs):
        rng = np.random.default_rng([seed, ep])
        order = rng.permutation(len(X))
        for s in range(0, len(X), bs):
            idx = order[s:s + bs]
            x, y = augment.augment_batch(X[idx], Y[idx], rng, "he_staining", dtype=tb.dtype, device=cuda, stain_bases=bases.take(idx))
            tb.step(x, y, float(LR[ep]))
    assert torch.equal(ta.w, tb.w) and torch.equal(ta.b, tb.b) and not torch.equal(ta.w, w0)


def test_cli_trains_with_he_staining_in_a_child_process(cuda, tmp_path):
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
           "--augment", "he_staining", "--save_path", str(tmp_path), "--model_name", "m", "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    assert "train_loss=" in r.stderr and "image pool:" in r.stderr
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["out_class.weight"].shape == (ncls * 64, 256, 1, 1)
