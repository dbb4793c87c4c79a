"""Device augmentation of class-head training (csrc/cpx_augment.hip -> ops -> classpose_amd.augment -> train_class_head -> CLI).

Yardsticks: the reference-minted fixture tests/golden/reference_augment.npz for the stain jitter, and the float64 restatements of
tests/augment_reference.py (pinned on that fixture by tests/test_augment_host.py), evaluated on the same inputs the device read.

Bounds, none of them taken from what the device returns:
  * stain jitter: equal to the reference, except that a pixel may be off by one level where the float64 restatement's 255 x lies
    within 1e-3 of an integer (float32 against float64 differs by at most 6e-7 before the truncation, 1.5e-4 levels);
  * warp, image: per element |device - float64| <= 8 * 2^-24 * 255 (three lerps of at most two roundings each, plus the weight
    cast, on values <= 255), and relative L2 err(device) <= max(4 * err(float32 restatement), 2^-20);
  * warp, labels: exact;
  * float32 normalisation: bit-equal to np.percentile(plane, 1) / np.percentile(plane, 99) (scalar calls, as cellpose's normalize99
    makes them: float32 quantile arithmetic) followed by the normalize99 rule in numpy float32.
Every test prints the figures it observed before it asserts (run with -s)."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import augment_reference as ar

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FLOOR = 2.0 ** -20
WARP_ABS = 8 * 2.0 ** -24 * 255


def _fixture():
    with open(os.path.join(GOLD, "reference_augment.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_augment.npz")), meta


def _rel_l2(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(x - ref) / max(np.linalg.norm(ref), 1e-300))


# ---- 1. stain jitter ------------------------------------------------------------------------------------------------
def test_hed_jitter_against_the_reference_fixture(cuda):
    from classpose_amd import augment, ops
    npz, meta = _fixture()
    cut = meta["config"]["cutoff_range"]
    assert np.array_equal(augment.HED_FROM_RGB, npz["HED_FROM_RGB"])
    for c in meta["cases"]:
        src, ref = npz[c["name"] + "_in"], npz[c["name"] + "_out"]
        out, applied = ops.hed_jitter(torch.from_numpy(src[None]).to(cuda), np.float32([c["sigma"]]), np.float32([c["bias"]]), cut,
                                      c["simple_mode"])
        out = out.cpu().numpy()[0]
        assert bool(applied.item()) == c["applied"], c["name"]
        if not c["applied"]:
            assert np.array_equal(out, src) and np.array_equal(out, ref)
            print(f"{c['name']}: outside the cut-off, copied")
            continue
        v64 = ar.hed_jitter(src, c["sigma"], c["bias"], npz["HED_FROM_RGB"], cut, c["simple_mode"], np.float64)[2]
        r = ar.check_hed_against(out, ref, v64)
        print(f"{c['name']}: {r['differ']} of {ref.size} values differ from the reference by one level, all inside the window "
              f"({r['near']} values lie in it)")


@pytest.mark.parametrize("simple_mode", [False, True])
def test_hed_jitter_batch_of_32_against_float64(cuda, simple_mode):
    from classpose_amd import augment, ops
    rng = np.random.default_rng(77 + simple_mode)
    n = 32
    X = rng.integers(0, 256, (n, 256, 256, 3), dtype=np.uint8)
    X[3] = rng.integers(0, 50, (256, 256, 3), dtype=np.uint8)              # below the cut-off
    X[17] = rng.integers(225, 256, (256, 256, 3), dtype=np.uint8)          # above it
    X[5, :64] = 0
    X[5, 64:128] = 255
    cfg = augment.get_config("hed_only")
    sigma, bias = augment.sample_hed(rng, n, cfg["sigma_ranges"], cfg["bias_ranges"])
    out, applied = ops.hed_jitter(torch.from_numpy(X).to(cuda), sigma, bias, cfg["cutoff_range"], simple_mode)
    out, applied = out.cpu().numpy(), applied.cpu().numpy()
    differ = 0
    for i in range(n):
        ref, ap, v64 = ar.hed_jitter(X[i], sigma[i], bias[i], augment.HED_FROM_RGB, cfg["cutoff_range"], simple_mode, np.float64)
        assert bool(applied[i]) == ap, i
        if not ap:
            assert np.array_equal(out[i], X[i])
            continue
        differ += ar.check_hed_against(out[i], ref, v64)["differ"]
    assert list(np.flatnonzero(applied == 0)) == [3, 17]
    print(f"simple_mode={simple_mode}: {differ} of {30 * 196608} values differ from the float64 restatement by one level, all inside the window")


# ---- 2. / 3. warp ---------------------------------------------------------------------------------------------------
def _rot90_about(cx, cy):
    """inverse map of a quarter turn about (cx, cy), built like augment.affine_inverse does (cos(pi / 2) is not 0 in double)"""
    c, s = np.cos(np.pi / 2), np.sin(np.pi / 2)
    return np.array([c, s, cx - (c * cx + s * cy), -s, c, cy - (-s * cx + c * cy)])


def _maps(sh, sw, seed, n_random=5):
    from classpose_amd import augment
    flip = augment.affine_inverse([True], [0.0], [1.0], [[0.0, 0.0]], sh, sw, 256)[0]
    # leaves the frame on every side: the source shrunk to 60 % about its centre
    outside = np.array([1 / 0.6, 0, sw / 2 - 128 / 0.6, 0, 1 / 0.6, sh / 2 - 128 / 0.6])
    named = [("identity", np.array([1.0, 0, 0, 0, 1.0, 0])), ("flip", flip), ("quarter turn", _rot90_about(128.0, 128.0)),
             ("beyond every side", outside)]
    _f, rnd = augment.sample_affine(np.random.default_rng(seed), n_random, sh, sw, 256, scale_range=0.5)
    return named + [(f"random {k}", m) for k, m in enumerate(rnd)]


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("sh,sw", [(256, 256), (320, 288)])
def test_warp_image_and_labels(cuda, dtype, sh, sw):
    from classpose_amd import ops
    rng = np.random.default_rng(sh + (dtype == "u8"))
    maps = _maps(sh, sw, seed=11 + sh)
    n = len(maps)
    inv = np.stack([m for _n, m in maps])
    if dtype == "u8":
        src = rng.integers(0, 256, (n, sh, sw, 3), dtype=np.uint8)
        chw = src.transpose(0, 3, 1, 2)
    else:
        src = (rng.standard_normal((n, 3, sh, sw)) * 40 + 100).clip(-255, 255).astype(np.float32)
        chw = src
    lab = rng.integers(0, 7, (n, sh, sw)).astype(np.int16)
    lab[:, 5:9] = -100
    # nearest-neighbour sampling is only well defined away from half-integer source coordinates: checked on the CPU first
    for name, m in maps:
        d = ar.half_integer_distance(m, 256, 256)
        assert d > 1e-9, (name, d)
    for fill in (0, -100):
        out, lo = ops.warp_affine(torch.from_numpy(src).to(cuda), inv, (256, 256), torch.from_numpy(lab).to(cuda), fill)
        out, lo = out.cpu().numpy(), lo.cpu().numpy()
        assert out.shape == (n, 3, 256, 256) and out.dtype == np.float32 and lo.shape == (n, 256, 256) and lo.dtype == np.int16
        for i, (name, m) in enumerate(maps):
            assert np.array_equal(lo[i], ar.warp_labels(lab[i], m, 256, 256, fill)), (name, fill)
    assert (lo[3] == -100).sum() > 256 * 256 * 0.3 and not out[3][:, 0].any() and not out[3][:, :, -1].any()    # the frame is left on every side
    for i, (name, m) in enumerate(maps):
        r64 = ar.warp_image(chw[i], m, 256, 256, np.float64)
        r32 = ar.warp_image(chw[i], m, 256, 256, np.float32)
        worst = float(np.abs(out[i] - r64).max())
        e_dev, e_32 = _rel_l2(out[i], r64), _rel_l2(r32, r64)
        tol = max(4 * e_32, FLOOR)
        print(f"{dtype} {sh}x{sw} {name}: max |device - float64| = {worst:.3e} (bound {WARP_ABS:.3e}), err(device) = {e_dev:.3e}, "
              f"err(float32 restatement) = {e_32:.3e}, tolerance = {tol:.3e}")
        assert worst <= WARP_ABS, (name, worst)
        assert e_dev <= tol, (name, e_dev, tol)
        assert r64.any()
    if (sh, sw) == (256, 256):
        assert np.array_equal(out[0], chw[0].astype(np.float32)) and np.array_equal(lo[0], lab[0])        # identity: the source exactly
        assert np.array_equal(out[1], chw[1].astype(np.float32)[:, :, ::-1])                             # the flip alone
    # without labels
    only, none = ops.warp_affine(torch.from_numpy(src).to(cuda), inv, (256, 256))
    assert none is None and np.array_equal(only.cpu().numpy(), out)


# ---- 4. float32 normalisation ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(256, 256), (250, 190)])
def test_normalize_f32_is_numpys_percentile_exactly(cuda, H, W):
    from classpose_amd import ops
    rng = np.random.default_rng(H)
    x = np.zeros((5, 3, H, W), np.float32)
    x[0] = rng.standard_normal((3, H, W)) * 3 - 0.5                           # negatives and positives
    x[1] = rng.integers(-3, 12, (3, H, W))                                    # integer-valued with heavy ties
    x[1, 2] = rng.integers(0, 2, (H, W)) * 255.0
    x[2, 0] = 7.5                                                             # constant: mode 0
    x[2, 1] = 0.0
    x[2, 2] = -2.0 + 5e-4 * rng.random((H, W))                                # range below 1e-3: mode 2
    src = rng.integers(0, 256, (1, H, W, 3), dtype=np.uint8)                  # a warped image with a zero-filled border
    m = np.array([[0.9, 0.5, -40.0, -0.5, 0.9, 60.0]])
    x[3] = ops.warp_affine(torch.from_numpy(src).to(cuda), m, (H, W))[0].cpu().numpy()[0]
    x[4] = np.float32(rng.standard_normal((3, H, W))) * np.float32(1e-30)     # tiny magnitudes, both signs, and signed zeros
    x[4, 0, :4] = 0.0
    x[4, 0, 4:8] = -0.0
    assert (x[3] == 0).mean() > 0.05 and (x[3] > 0).mean() > 0.3
    xd = torch.from_numpy(x).to(cuda)
    stats = ops.normalize_stats_f32(xd).cpu().numpy()
    out = ops.normalize_img_f32(xd).cpu().numpy()
    st_ref, out_ref = ar.normalize_f32(x)
    for i in range(5):
        for c in range(3):
            print(f"{H}x{W} image {i} channel {c}: device stats {stats[i, c]}, numpy {st_ref[i, c]}")
    assert list(st_ref[2, :, 2]) == [0, 0, 2] and np.all(st_ref[[0, 1, 3], :, 2] == 1)
    assert np.array_equal(stats.view(np.uint32), st_ref.view(np.uint32))
    assert np.array_equal(out.view(np.uint32), out_ref.view(np.uint32))
    assert np.array_equal(xd.cpu().numpy().view(np.uint32), x.view(np.uint32))           # the input is left alone


# ---- 5. augment_batch -----------------------------------------------------------------------------------------------
def _synthetic_set(n, ncls, seed0=300):
    """The synthetic set of tests/test_gpu_train.py, rebuilt here: uint8 crops of the synthetic slide, labels from its analytic class
    map with a -100 band."""
    from classpose_amd import synth
    ims, labs = [], []
    for k in range(n):
        x0, y0 = 256 * (k % 4), 256 * (k // 4)
        ims.append(synth.render_region(seed0, x0, y0, 256, 256))
        lg = synth.analytic_fields(seed0, x0, y0, 256, 256, ncls)[2]
        lab = lg.argmax(0).astype(np.int16)
        lab[(40 + 11 * k) % 200:][:24] = -100
        labs.append(lab)
    return np.stack(ims), np.stack(labs)


def test_augment_batch_is_the_composition_of_its_stages(cuda):
    from classpose_amd import augment, ops
    ims, labs = _synthetic_set(8, 7)
    cfg = augment.get_config("hed_only")
    for dtype in (torch.bfloat16, torch.float32):
        p, l = augment.augment_batch(ims, labs, np.random.default_rng(4), "hed_only", scale_range=0.5, dtype=dtype, device=cuda)
        rng = np.random.default_rng(4)                                        # the documented order: stain draws, then the transforms
        sigma, bias = augment.sample_hed(rng, 8, cfg["sigma_ranges"], cfg["bias_ranges"])
        _flip, inv = augment.sample_affine(rng, 8, 256, 256, 256, 0.5)
        X, L = torch.from_numpy(ims).to(cuda), torch.from_numpy(labs).to(cuda)
        j, applied = ops.hed_jitter(X, sigma, bias, cfg["cutoff_range"], False)
        w, lw = ops.warp_affine(j, inv, (256, 256), L, 0)
        x = ops.normalize_img_f32(w)
        assert applied.all() and not torch.equal(j, X)
        assert p.dtype == dtype and p.shape == (8 * 1024, 192) and l.dtype == torch.int16
        assert torch.equal(p, ops.patchify_f32(x, dtype)) and torch.equal(l, lw)
    p2, l2 = augment.augment_batch(ims, labs, np.random.default_rng(4), "hed_only", dtype=torch.float32, device=cuda)
    p3, l3 = augment.augment_batch(ims, labs, np.random.default_rng(5), "hed_only", dtype=torch.float32, device=cuda)
    assert torch.equal(p, p2) and torch.equal(l, l2) and not torch.equal(p, p3) and not torch.equal(l, l3)
    # geometry alone draws no stain values; without geometry the labels pass through and the pixels are normalised as inference does
    pg, lg = augment.augment_batch(ims, labs, np.random.default_rng(4), "geometry", dtype=torch.float32, device=cuda)
    _f, inv_g = augment.sample_affine(np.random.default_rng(4), 8, 256, 256, 256, 0.5)
    wg, lwg = ops.warp_affine(X, inv_g, (256, 256), L, 0)
    assert torch.equal(pg, ops.patchify_f32(ops.normalize_img_f32(wg), torch.float32)) and torch.equal(lg, lwg)
    pn, ln = augment.augment_batch(ims, labs, np.random.default_rng(4), None, geometry=False, dtype=torch.float32, device=cuda)
    plain = ops.patchify_f32(ops.normalize_img(X).permute(0, 3, 1, 2).contiguous(), torch.float32)
    assert torch.equal(ln, L) and torch.equal(pn, plain)
    # float32 crops are already normalised: geometry only
    xf = ops.normalize_img(X).permute(0, 3, 1, 2).contiguous()
    pf, lf = augment.augment_batch(xf, labs, np.random.default_rng(4), "hed_only", dtype=torch.float32, device=cuda)
    rng = np.random.default_rng(4)
    augment.sample_hed(rng, 8, cfg["sigma_ranges"], cfg["bias_ranges"])        # drawn and unused: the stream is the uint8 path's
    _f, inv_f = augment.sample_affine(rng, 8, 256, 256, 256, 0.5)
    wf, lwf = ops.warp_affine(xf, inv_f, (256, 256), L, 0)
    assert torch.equal(pf, ops.patchify_f32(wf, torch.float32)) and torch.equal(lf, lwf)


def test_augment_batch_resamples_a_crop_without_annotation(cuda):
    from classpose_amd import augment
    ims, labs = _synthetic_set(4, 7)
    labs = labs.copy()
    labs[:] = -100
    labs[:, 0:40, 0:40] = 1                             # a small annotated island in a corner: many transforms lose it
    first = augment.sample_batch_params(np.random.default_rng(4), 4, 256, 256, augment.get_config("hed_only"), 0.5, True, 256)
    lost = [i for i in range(4) if (ar.warp_labels(labs[i], first.inv[i], 256, 256, -100) == -100).all()]
    assert lost, "the seed is chosen so that the first transforms lose the island of at least one crop"
    p, l = augment.augment_batch(ims, labs, np.random.default_rng(4), "hed_only", label_fill=-100, dtype=torch.bfloat16, device=cuda)
    assert bool(((l != -100).flatten(1).any(1)).all())
    keep = [i for i in range(4) if i not in lost]       # the crops that kept their island keep their first transform
    for i in keep:
        assert np.array_equal(l[i].cpu().numpy(), ar.warp_labels(labs[i], first.inv[i], 256, 256, -100))
    print(f"crops {lost} drew a new transform")
    labs[:] = -100                                      # nothing annotated at all: eight new transforms cannot help
    with pytest.raises(ValueError, match="no annotated pixel"):
        augment.augment_batch(ims, labs, np.random.default_rng(0), "hed_only", label_fill=-100, dtype=torch.bfloat16, device=cuda)


# ---- 6. loop wiring -------------------------------------------------------------------------------------------------
def test_train_class_head_augmented_equals_the_replay_by_hand(cuda, tmp_path):
    from classpose_amd import augment, synth
    from classpose_amd.train import HeadTrainer, lr_schedule, train_class_head
    ncls, bs, n_epochs, lr, seed = 7, 4, 2, 2e-3, 42
    sd = synth.make_state_dict(ncls, None, depth=2, seed=11)
    ims, labs = _synthetic_set(8, ncls)
    tr_x, tr_y, te_x, te_y = ims[:6], labs[:6], ims[6:], labs[6:]
    runs = []
    for k in range(2):
        t = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
        seen = []

        def spy(x, y, rng, t=t, seen=seen):             # runs before the augmentation and draws nothing: the weights before each step
            seen.append((t.w.clone(), t.b.clone()))
            return x, y
        path, tl, vl = train_class_head(t, tr_x, tr_y, te_x, te_y, batch_size=bs, n_epochs=n_epochs, learning_rate=lr,
                                        save_path=tmp_path / f"run{k}", model_name="head", random_seed=seed, transform=spy,
                                        augment="hed_only", scale_range=0.5, label_fill=0)
        runs.append((t, path, tl, vl, seen))
    t, path, tl, vl, seen = runs[0]
    # the replay: the epoch generator gives the order, then augment_batch draws from it batch by batch
    h = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    LR = lr_schedule(lr, n_epochs)
    step = 0
    for ep in range(n_epochs):
        rng = np.random.default_rng([seed, ep])
        order = rng.permutation(6)
        sums, count = 0.0, 0
        for s in range(0, 6, bs):
            idx = order[s:s + bs]
            assert torch.equal(seen[step][0], h.w) and torch.equal(seen[step][1], h.b), f"weights before step {step}"
            x, y = augment.augment_batch(tr_x[idx], tr_y[idx], rng, "hed_only", scale_range=0.5, label_fill=0, dtype=h.dtype, device=cuda)
            r = h.step(x, y, float(LR[ep]))
            sums += r["loss"] * len(idx)
            count += len(idx)
            step += 1
        assert tl[ep] == sums / count
        ev = h.evaluate(te_x, te_y)                      # two validation crops: one unaugmented batch
        print(f"epoch {ep}: train loss {tl[ep]:.6f}, validation loss {vl[ep]:.6f} (unaugmented evaluate {ev['loss']:.6f})")
        assert vl[ep] == ev["loss"]
    assert step == len(seen) == 4
    assert torch.equal(t.w, h.w) and torch.equal(t.b, h.b) and not torch.equal(t.w, seen[0][0])
    # the augmented crops differ from the plain ones, so does the loss of the first step
    plain = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    order0 = np.random.default_rng([seed, 0]).permutation(6)[:bs]
    assert plain.evaluate(tr_x[order0], tr_y[order0])["loss"] != h.evaluate(
        *augment.augment_batch(tr_x[order0], tr_y[order0], np.random.default_rng(1), "hed_only", dtype=h.dtype, device=cuda))["loss"]
    # two runs with one seed: byte-equal checkpoints
    t1, path1, tl1, vl1, _ = runs[1]
    assert np.array_equal(tl, tl1) and np.array_equal(vl, vl1)
    for name in ("head", "checkpoint_last.pt", "checkpoint_best.pt"):
        a, b = (path.parent / name).read_bytes(), (path1.parent / name).read_bytes()
        assert a == b, name
    # a different seed trains on different pixels
    t3 = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    train_class_head(t3, tr_x, tr_y, te_x, te_y, batch_size=bs, n_epochs=n_epochs, learning_rate=lr, save_path=tmp_path / "run3",
                     model_name="head", random_seed=seed + 1, augment="hed_only")
    assert not torch.equal(t3.w, t.w)


# ---- 7. CLI ---------------------------------------------------------------------------------------------------------
def test_cli_trains_with_augmentation_in_a_child_process(cuda, tmp_path):
    from classpose_amd import engine, synth
    ncls = 5
    sd = synth.make_state_dict(1, None, depth=2, seed=12)              # a plain backbone: the CLI initialises the head
    torch.save(sd, tmp_path / "backbone.pt")
    ims, labs = _synthetic_set(8, ncls)
    np.save(tmp_path / "X.npy", ims)
    np.save(tmp_path / "Y.npy", labs)
    cmd = [sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--images", str(tmp_path / "X.npy"), "--labels",
           str(tmp_path / "Y.npy"), "--test_images", str(tmp_path / "X.npy"), "--test_labels", str(tmp_path / "Y.npy"),
           "--pretrained_model", str(tmp_path / "backbone.pt"), "--nclasses", str(ncls), "--n_epochs", "2", "--batch_size", "4",
           "--learning_rate", "1e-3", "--augment", "hed_only", "--scale_range", "0.5", "--save_path", str(tmp_path),
           "--model_name", "m", "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    ck = torch.load(out, map_location="cpu", weights_only=True)          # what predict_wsi's loader does with --model_path
    assert ck["out_class.weight"].shape == (ncls * 64, 256, 1, 1) and ck["W3"].shape == (ncls * 64, ncls, 8, 8)
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    assert w.ncls == ncls and w.c.n_unet_ops == 0
    assert (tmp_path / "m" / "checkpoint_best.pt").exists() and (tmp_path / "m" / "checkpoint_last.pt").exists()
