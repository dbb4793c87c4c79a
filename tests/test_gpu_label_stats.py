"""Dataset statistics on the device: ``cpx_label_stats`` / ``ops.label_stats`` / ``dataset_stats.label_stats`` against
the reference-minted fixture tests/golden/reference_label_stats.npz and the numpy restatement of tests/label_stats_reference.py
(pinned on that fixture by tests/test_label_stats_host.py), and the training options that consume them: ``rescale`` of the
augmentation, ``train_probs`` / ``rescale`` of ``train_class_head``, and the command line.

Every device output is an integer and is compared for equality.  The float64 diameters are formed on the host as
(sqrt(a0) + sqrt(a1)) / 2 / (sqrt(pi) / 2) where the restatement computes np.median(counts ** 0.5) / (pi ** 0.5 / 2): two
pow-versus-sqrt roundings of at most 1 ulp each, one addition and one division bound the difference by 4 * 2^-52 relative."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import label_stats_reference as lsr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
DIAM_RTOL = 4 * 2.0 ** -52
NAMES = ("class_px", "inst_per_class", "n_masks", "mid_area")


def _fixture():
    with open(os.path.join(GOLD, "reference_label_stats.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_label_stats.npz")), meta


def _device_stats(inst, cls, ncls, dev):
    from classpose_amd import ops
    out = ops.label_stats(torch.from_numpy(inst).to(dev), torch.from_numpy(cls).to(dev), ncls)
    assert [t.dtype for t in out] == [torch.int64, torch.int32, torch.int32, torch.int32, torch.int32]
    assert all(t.device.type == "cuda" for t in out) and not bool(out[4].any())
    return dict(zip(NAMES, (t.cpu().numpy() for t in out[:4])))


def _compare(got: dict, ref: dict, tag: str):
    for k in NAMES:
        assert got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k]), f"{tag}: {k}"


def _diam_dev(d, ref):
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(ref > 0, np.abs(d - ref) / ref, np.abs(d - ref))
    return float(rel.max())


def test_fixture_cases_integer_for_integer(cuda):
    from classpose_amd import dataset_stats as ds
    arr, meta = _fixture()
    ncls = meta["n_classes"]
    total = np.zeros(ncls, np.int64)
    worst = 0.0
    for k, c in enumerate(meta["cases"]):
        inst, cls = arr[f"inst_{k}"][None], arr[f"cls_{k}"][None]
        got = _device_stats(inst, cls, ncls, cuda)
        ref = dict(class_px=arr["class_px"][k:k + 1], inst_per_class=arr["instance_counts"][k:k + 1].astype(np.int32),
                   n_masks=arr["n_masks"][k:k + 1], mid_area=arr["mid_area"][k:k + 1])
        _compare(got, ref, c["name"])
        s = ds.label_stats(inst, cls, ncls, device=cuda)
        assert s.class_counts.dtype == np.int64 and s.instance_counts.dtype == np.float64 and s.diameters.dtype == np.float64
        assert np.array_equal(s.instance_counts, arr["instance_counts"][k:k + 1]) and s.n_masks[0] == arr["n_masks"][k]
        dev_k = _diam_dev(s.diameters, arr["diameters"][k:k + 1])
        worst = max(worst, dev_k)
        print(f"{c['name']}: m = {int(s.n_masks[0])}, diameter {s.diameters[0]!r} (restated {arr['diameters'][k]!r}, deviation {dev_k:.3e})")
        assert dev_k <= DIAM_RTOL, c["name"]
        total += s.class_counts
    print(f"largest relative deviation of a diameter: {worst:.3e} (bound {DIAM_RTOL:.3e})")
    assert np.array_equal(total, arr["class_counts"])                       # the reference's get_class_counts of the whole set
    assert np.array_equal(ds.get_class_weights(total), arr["class_weights"])
    # the two cases of one shape in ONE call: images do not leak into each other
    same = [k for k, c in enumerate(meta["cases"]) if (c["H"], c["W"]) == (32, 32)]
    assert len(same) >= 3
    got = _device_stats(np.stack([arr[f"inst_{k}"] for k in same]), np.stack([arr[f"cls_{k}"] for k in same]), ncls, cuda)
    _compare(got, dict(class_px=arr["class_px"][same], inst_per_class=arr["instance_counts"][same].astype(np.int32),
                       n_masks=arr["n_masks"][same], mid_area=arr["mid_area"][same]), "batched 32 x 32")


@pytest.fixture(scope="module")
def sixteen():
    """16 images of 256 x 256 with about 150 cells, 7 classes, and their numpy statistics (computed once, never modified)."""
    inst, cls = lsr.random_maps(np.random.default_rng(61), 16, 256, 256, 7, 150)
    ref = lsr.numpy_label_stats(inst, cls, 7)
    for a in (inst, cls, *ref.values()):
        a.setflags(write=False)
    return inst, cls, ref


def test_sixteen_random_images(cuda, sixteen):
    from classpose_amd import dataset_stats as ds
    inst, cls, ref = sixteen
    assert ref["n_masks"].min() > 60 and int(inst.max()) > 1_000_000_000
    got = _device_stats(inst, cls, 7, cuda)
    _compare(got, ref, "16 x 256 x 256")
    d = ds.diameters_from_mid_areas(got["mid_area"])
    dev = _diam_dev(d, ref["diameters"])
    print(f"m = {ref['n_masks'].min()} .. {ref['n_masks'].max()}, largest relative deviation of a diameter {dev:.3e}")
    assert dev <= DIAM_RTOL
    # two runs give the same bits
    again = _device_stats(inst, cls, 7, cuda)
    _compare(again, got, "second run")
    # five images alone equal the same images inside the run of sixteen
    five = _device_stats(inst[3:8], cls[3:8], 7, cuda)
    _compare(five, {k: got[k][3:8] for k in NAMES}, "5 of 16")


@pytest.mark.parametrize("ncls", [1, 7, 64])
def test_odd_size_and_class_counts(cuda, ncls):
    """250 x 190 = 47 500 pixels: no multiple of the 4096-pixel workgroup tile nor of a thread's 16-pixel strip."""
    inst, cls = lsr.random_maps(np.random.default_rng(70 + ncls), 3, 250, 190, ncls, 90)
    if ncls == 64:
        cls[0, :8, :8] = 63
    ref = lsr.numpy_label_stats(inst, cls, ncls)
    got = _device_stats(inst, cls, ncls, cuda)
    _compare(got, ref, f"250 x 190, {ncls} classes")
    from classpose_amd import dataset_stats as ds
    assert _diam_dev(ds.diameters_from_mid_areas(got["mid_area"]), ref["diameters"]) <= DIAM_RTOL


def test_every_pixel_its_own_id_and_a_single_id(cuda):
    """65 536 distinct ids in one image: both tables at their designed load (half full); and one id that covers an image."""
    rng = np.random.default_rng(5)
    ids = np.unique(rng.integers(1, 2_000_000_001, size=80_000))
    assert ids.size >= 65536
    inst = np.zeros((2, 256, 256), np.int32)
    inst[0] = rng.permutation(ids)[:65536].reshape(256, 256)
    inst[1] = 1_234_567_890
    cls = np.zeros((2, 256, 256), np.int16)
    cls[0] = rng.integers(-1, 7, (256, 256))
    cls[1] = 4
    cls[1, :3] = -100
    ref = lsr.numpy_label_stats(inst, cls, 7)
    assert ref["n_masks"].tolist() == [65535, 0] and ref["mid_area"].tolist() == [[1, 1], [0, 0]]
    assert ref["inst_per_class"][1].tolist() == [0, 0, 0, 0, 1, 0, 0] and ref["inst_per_class"][0].sum() == (cls[0] >= 0).sum()
    got = _device_stats(inst, cls, 7, cuda)
    _compare(got, ref, "65 536 ids / one id")


def test_bad_maps_raise_and_name_the_image(cuda):
    from classpose_amd import dataset_stats as ds, ops
    inst, cls = lsr.random_maps(np.random.default_rng(8), 4, 32, 32, 5, 6)
    bad = inst.copy()
    bad[2, 5, 7] = -3
    with pytest.raises(ValueError, match="image 2 has a negative instance id"):
        ops.label_stats(torch.from_numpy(bad).to(cuda), torch.from_numpy(cls).to(cuda), 5)
    with pytest.raises(ValueError, match="image 2 has a negative instance id"):
        ds.label_stats(bad, cls, 5, device=cuda)
    badc = cls.copy()
    badc[1, 31, 31] = 5
    with pytest.raises(ValueError, match="image 1 has a class >= 5"):
        ops.label_stats(torch.from_numpy(inst).to(cuda), torch.from_numpy(badc).to(cuda), 5)
    with pytest.raises(ValueError, match="image 3 has a class >= 5"):                     # the global index across chunks
        ds.label_stats(inst, np.roll(badc, 2, axis=0), 5, device=cuda, chunk=2)
    st = ops.label_stats(torch.from_numpy(bad).to(cuda), torch.from_numpy(badc).to(cuda), 5, check_status=False)[4]
    assert st.tolist() == [0, 2, 1, 0]
    ops.label_stats(torch.from_numpy(inst).to(cuda), torch.from_numpy(cls).to(cuda), 5)  # the clean maps pass


def test_chunking_does_not_change_the_result(cuda):
    from classpose_amd import dataset_stats as ds
    inst, cls = lsr.random_maps(np.random.default_rng(9), 10, 64, 64, 7, 20)
    a = ds.label_stats(inst, cls, 7, device=cuda, chunk=3)
    b = ds.label_stats(inst, cls, 7, device=cuda, chunk=1024)
    c = ds.label_stats(torch.from_numpy(inst).to(cuda), torch.from_numpy(cls.astype(np.int64)).to(cuda), 7, device=cuda)   # device tensors
    ref = lsr.numpy_label_stats(inst, cls, 7)
    for s in (a, b, c):
        assert np.array_equal(s.class_counts, ref["class_px"].sum(0)) and np.array_equal(s.instance_counts, ref["inst_per_class"])
        assert np.array_equal(s.n_masks, ref["n_masks"]) and s.instance_counts.shape == (10, 7)
        assert np.array_equal(s.diameters.view(np.uint64), a.diameters.view(np.uint64))
    assert _diam_dev(a.diameters, ref["diameters"]) <= DIAM_RTOL


# ---- the consumers --------------------------------------------------------------------------------------------------
def _synthetic_set(n, ncls, seed0=300):
    """The synthetic set of tests/test_gpu_train.py, rebuilt here."""
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


def test_augment_batch_rescale(cuda):
    from classpose_amd import augment, ops
    ims, labs = _synthetic_set(4, 7)
    kw = dict(scale_range=0.5, dtype=torch.float32, device=cuda)
    p0, l0 = augment.augment_batch(ims, labs, np.random.default_rng(4), "hed_only", **kw)
    p1, l1 = augment.augment_batch(ims, labs, np.random.default_rng(4), "hed_only", rescale=np.ones(4), **kw)
    assert torch.equal(p0, p1) and torch.equal(l0, l1)                      # rescale = 1 is bitwise the batch without it
    # rescale = 2: the maps are affine_inverse of the HALVED scale, with the crop room of that scale (none: 256 * 0.625 < 256)
    base = augment.sample_affine_params(np.random.default_rng(4), 4, 256, 256, 256, 0.5)
    q = augment.sample_batch_params(np.random.default_rng(4), 4, 256, 256, None, 0.5, True, 256, rescale=np.full(4, 2.0))
    inv = augment.affine_inverse(base["flip"], base["theta"], base["scale"] / 2, np.zeros((4, 2)), 256, 256, 256)
    assert np.array_equal(q.inv, inv) and np.array_equal(q.flip, base["flip"])
    p2, l2 = augment.augment_batch(ims, labs, np.random.default_rng(4), "geometry", rescale=np.full(4, 2.0), **kw)
    X, L = torch.from_numpy(ims).to(cuda), torch.from_numpy(labs).to(cuda)
    w, lw = ops.warp_affine(X, inv, (256, 256), L, 0)
    assert torch.equal(p2, ops.patchify_f32(ops.normalize_img_f32(w), torch.float32)) and torch.equal(l2, lw)
    pg, _lg = augment.augment_batch(ims, labs, np.random.default_rng(4), "geometry", **kw)
    assert not torch.equal(p2, pg)
    # a crop that a round resamples draws with ITS factor: an island in a corner, lost by a shrinking transform
    labs2 = np.full_like(labs, -100)
    labs2[:, 0:40, 0:40] = 1
    rs = np.array([2.0, 0.5, 0.6, 4.0])
    first = augment.sample_batch_params(np.random.default_rng(5), 4, 256, 256, None, 0.5, True, 256, rescale=rs)
    _w, lab_first = ops.warp_affine(X, first.inv, (256, 256), torch.from_numpy(labs2).to(cuda), -100)
    lost = torch.nonzero((lab_first == -100).flatten(1).all(1)).flatten().cpu().numpy()
    assert len(lost) and not np.any(rs[lost] == rs[:len(lost)]), "the seed is chosen so that crops behind the first ones lose their island"
    rng = np.random.default_rng(5)
    _p, l3 = augment.augment_batch(ims, labs2, rng, "geometry", label_fill=-100, rescale=rs, **kw)
    replay = np.random.default_rng(5)
    augment.sample_batch_params(replay, 4, 256, 256, None, 0.5, True, 256, rescale=rs)
    lab, empty = lab_first.clone(), lost
    for _ in range(augment.MAX_RESAMPLE):
        if not len(empty):
            break
        r = augment.sample_batch_params(replay, len(empty), 256, 256, None, 0.5, True, 256, rescale=rs[empty])
        _w, lr = ops.warp_affine(X[torch.from_numpy(empty).to(cuda)], r.inv, (256, 256), torch.from_numpy(labs2[empty]).to(cuda), -100)
        lab[torch.from_numpy(empty).to(cuda)] = lr
        empty = torch.nonzero((lab == -100).flatten(1).all(1)).flatten().cpu().numpy()
    assert torch.equal(l3, lab) and rng.random() == replay.random()
    print(f"crops {lost.tolist()} drew a new transform with their own rescale")


def test_train_class_head_oversampled_and_rescaled_equals_the_replay_by_hand(cuda, tmp_path):
    from classpose_amd import augment, synth
    from classpose_amd.train import HeadTrainer, lr_schedule, train_class_head
    ncls, bs, n_epochs, lr, seed = 7, 4, 2, 2e-3, 42
    sd = synth.make_state_dict(ncls, None, depth=1, seed=11)
    ims, labs = _synthetic_set(6, ncls)
    probs = np.array([4.0, 0.0, 1.0, 1.0, 2.0, 0.5])                        # not normalised; image 1 is never drawn
    diam = np.array([12.0, 30.0, 45.0, 20.0, 36.0, 60.0])
    runs = []
    for k in range(2):
        t = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
        seen = []

        def spy(x, y, rng, t=t, seen=seen):             # runs before the augmentation and draws nothing: the weights before each step
            seen.append((t.w.clone(), t.b.clone()))
            return x, y
        path, tl, _vl = train_class_head(t, ims, labs, batch_size=bs, n_epochs=n_epochs, learning_rate=lr, save_path=tmp_path / f"run{k}",
                                         model_name="head", random_seed=seed, transform=spy, augment="geometry", scale_range=0.5,
                                         train_probs=probs, rescale=True, diameters=diam, diam_mean=30.0)
        runs.append((t, path, tl, seen))
    t, path, tl, seen = runs[0]
    h = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    LR = lr_schedule(lr, n_epochs)
    step, drawn = 0, []
    for ep in range(n_epochs):
        rng = np.random.default_rng([seed, ep])
        order = rng.choice(6, 6, p=probs / probs.sum())
        drawn += order.tolist()
        sums, count = 0.0, 0
        for s in range(0, 6, bs):
            idx = order[s:s + bs]
            assert torch.equal(seen[step][0], h.w) and torch.equal(seen[step][1], h.b), f"weights before step {step}"
            x, y = augment.augment_batch(ims[idx], labs[idx], rng, "geometry", scale_range=0.5, label_fill=0, dtype=h.dtype, device=cuda,
                                         rescale=diam[idx] / 30.0)
            r = h.step(x, y, float(LR[ep]))
            sums += r["loss"] * len(idx)
            count += len(idx)
            step += 1
        assert tl[ep] == sums / count
    assert step == len(seen) == 4 and 1 not in drawn and len(set(drawn)) < len(drawn)          # drawn WITH replacement
    assert torch.equal(t.w, h.w) and torch.equal(t.b, h.b) and not torch.equal(t.w, seen[0][0])
    _t1, path1, tl1, _ = runs[1]
    assert np.array_equal(tl, tl1)
    for name in ("head", "checkpoint_last.pt", "checkpoint_best.pt"):
        assert (path.parent / name).read_bytes() == (path1.parent / name).read_bytes(), name
    # without the rescale the same draws warp other pixels
    t3 = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
    train_class_head(t3, ims, labs, batch_size=bs, n_epochs=n_epochs, learning_rate=lr, save_path=tmp_path / "run3", model_name="head",
                     random_seed=seed, augment="geometry", scale_range=0.5, train_probs=probs)
    assert not torch.equal(t3.w, t.w)


def test_cli_trains_from_instance_annotations_in_a_child_process(cuda, tmp_path):
    from classpose_amd import dataset_stats as ds, models, synth
    ncls = 5
    sd = synth.make_state_dict(1, None, depth=1, seed=12)               # a plain backbone: the CLI initialises the head
    torch.save(sd, tmp_path / "backbone.pt")
    ims, _labs = _synthetic_set(6, ncls)
    rng = np.random.default_rng(3)
    inst = np.zeros((6, 256, 256), np.int32)
    labs = np.zeros((6, 256, 256), np.int16)
    for k in range(6):
        if k == 4:
            continue                                                       # the one crop without a mask
        for c in range(5 + 3 * k):
            y0, x0, h, w = int(rng.integers(0, 230)), int(rng.integers(0, 230)), int(rng.integers(6, 26)), int(rng.integers(6, 26))
            inst[k, y0:y0 + h, x0:x0 + w] = 1000 * k + c + 1
            labs[k, y0:y0 + h, x0:x0 + w] = 1 + (c * c) % 4
        labs[k, 250:] = -100
    for name, a in (("X", ims), ("Y", labs), ("I", inst)):
        np.save(tmp_path / f"{name}.npy", a)
    cmd = [sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--images", str(tmp_path / "X.npy"), "--labels",
           str(tmp_path / "Y.npy"), "--instances", str(tmp_path / "I.npy"), "--pretrained_model", str(tmp_path / "backbone.pt"),
           "--nclasses", str(ncls), "--n_epochs", "2", "--batch_size", "4", "--learning_rate", "1e-3", "--auto_class_weights",
           "--oversampling_method", "custom", "--rescale", "--augment", "geometry", "--min_train_masks", "1", "--save_path",
           str(tmp_path), "--model_name", "m", "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    log = r.stderr
    counts = np.bincount(labs[labs >= 0].astype(np.int64), minlength=ncls)
    weights = ds.get_class_weights(counts)
    assert f"class weights = {weights.tolist()}" in log, log[-3000:]
    assert "1 train images with number of masks less than min_train_masks (1), removing from train set" in log
    assert "n_train=5" in log and "Custom oversampling - probability range:" in log and "diameters:" in log
    m = models.ClassposeModel(pretrained_model=str(out), device=cuda, precision="bf16", max_batch_tiles=2)
    assert m.nclasses == ncls
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["out_class.weight"].shape == (ncls * 64, 256, 1, 1) and not torch.equal(ck["out_class.weight"], torch.zeros(()))
