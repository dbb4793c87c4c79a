"""Device training of the flow head (cpx_masks_to_flows, cpx_warp_affine_pool_flow_f32, cpx_seg_loss -> ops -> augment / train ->
the train_head CLI).

Yardsticks, none of them the code under test:
  * target flows: ``oracle.dynamics.masks_to_flows`` (float64).  |got - ref| <= 2^-25 + 1e-12: the values lie in [-1, 1], a correct
    float32 rounding moves them by at most 2^-25, and 1e-12 is the agreement the diffusion tests of tests/test_gpu_postproc.py
    hold.  At most ONE pixel per label is left out, the centre the oracle reports: there the flow is the normalised difference of
    equal numbers (tests/test_flow_train_host.py::test_oracle_masks_to_flows_symmetry).
  * target warp: the numpy restatement ``flow_train_reference.warp_flow_targets``, bitwise; and the symmetry of masks_to_flows
    under a quarter turn, which pins the sign conventions of the vector matrix without cellpose.
  * seg loss and the two-head steps: torch float64 autograd on the float32 values the device read, with the rule of
    tests/test_gpu_train.py: err(device) <= max(4 * err(torch CPU float32), 2^-20), err = relative L2.
Every test prints what it measured before it asserts (run with -s)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flow_train_reference as fr
import train_reference as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -20
MTF_TOL = 2.0 ** -25 + 1e-12


def _check(name, dev_val, f32_val, f64_val, floor=FLOOR):
    e_dev, e_cpu = tr.rel_l2(dev_val, f64_val), tr.rel_l2(f32_val, f64_val)
    tol = max(4 * e_cpu, floor)
    print(f"  {name}: err(device) = {e_dev:.3e}, err(torch CPU float32) = {e_cpu:.3e}, tolerance = {tol:.3e}")
    assert e_dev <= tol, (name, e_dev, e_cpu, tol)
    return e_dev


# ---- 1. target flows ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def oracle_flows():
    """{name: (map, oracle flows float64 (2, H, W), centre mask)} -- computed once, never modified."""
    from oracle import dynamics
    out = {}
    sym = fr.symmetric_map()
    fewer = sym.copy()
    fewer[fewer > 3] = 0
    for name, m in (("symmetric", sym), ("border", fr.border_map()), ("fewer", fewer)):
        F, dbg = dynamics.masks_to_flows(m, return_debug=True)
        out[name] = (m, F, fr.centre_mask(m, dbg["centers"]))
    return out


def _compare_flows(name, got, m, F, skip):
    assert got.dtype == np.float32 and got.shape == F.shape
    assert np.all(got[:, m == 0] == 0), "the background is exactly 0"
    d = np.abs(got.astype(np.float64) - F).max(0)
    assert int(skip.sum()) <= int(m.max()) and np.all(m[skip] > 0)
    print(f"  {name}: max |device - oracle| off the centres = {d[~skip].max():.3e} (tolerance {MTF_TOL:.3e}); at the {int(skip.sum())} centres "
          f"{d[skip].max():.3e}")
    assert d[~skip].max() <= MTF_TOL, name


@pytest.mark.parametrize("name", ["symmetric", "border"])
def test_masks_to_flows_equals_the_oracle(cuda, oracle_flows, name):
    from classpose_amd import ops
    m, F, skip = oracle_flows[name]
    if name == "border":
        assert (m == 1).sum() == 2500 and 52 * 52 > 2048          # the square runs in the second diffusion launch
        assert m[0].any() and m[-1].any() and m[:, 0].any() and m[:, -1].any()
    md = torch.from_numpy(m).to(cuda)
    got = ops.masks_to_flows(md)
    again = ops.masks_to_flows(md)
    assert torch.equal(got, again), "two runs are bitwise equal"
    _compare_flows(name, got.cpu().numpy(), m, F, skip)


def test_masks_to_flows_batch_with_different_label_counts_and_an_empty_tile(cuda, oracle_flows):
    from classpose_amd import ops
    (m0, F0, s0), (m1, F1, s1) = oracle_flows["symmetric"], oracle_flows["fewer"]
    assert m0.max() == 5 and m1.max() == 3
    batch = torch.from_numpy(np.stack([m0, m1, np.zeros_like(m0)])).to(cuda)
    got = ops.masks_to_flows(batch)
    assert got.shape == (3, 2, 96, 96) and torch.equal(got, ops.masks_to_flows(batch))
    g = got.cpu().numpy()
    _compare_flows("tile 0 (5 labels)", g[0], m0, F0, s0)
    _compare_flows("tile 1 (3 labels)", g[1], m1, F1, s1)
    assert np.all(g[2] == 0), "an all-zero tile gives all-zero flows"
    pair = ops.masks_to_flows(batch[:2])                           # nT = 2
    assert torch.equal(pair, got[:2])
    zero = ops.masks_to_flows(torch.zeros((40, 56), dtype=torch.int32, device=cuda))
    assert zero.shape == (2, 40, 56) and not bool(zero.any())


def test_masks_to_flows_refuses_ids_it_has_no_table_for(cuda):
    from classpose_amd import _lib, ops
    L = _lib.lib().cpx_postproc_max_labels(16, 16)
    assert L == 16 * 16 // 11 + 2
    m = torch.zeros((16, 16), dtype=torch.int32, device=cuda)
    m[2:5, 2:5] = L - 1                                             # the largest id with a table row: fine
    ok = ops.masks_to_flows(m)
    assert bool(torch.isfinite(ok).all()) and bool((ok[:, 2:5, 2:5] != 0).any())
    m[8, 8] = L
    with pytest.raises(ValueError, match="above the"):
        ops.masks_to_flows(m)
    flows, status = ops.masks_to_flows(m, check_status=False)       # ... and nothing was written through it
    assert int(status.item()) == 1 and torch.equal(flows, ok)
    m[8, 8] = 2 ** 31 - 1
    with pytest.raises(ValueError, match="above the"):
        ops.masks_to_flows(m)
    m[8, 8] = -1
    with pytest.raises(ValueError, match="negative"):
        ops.masks_to_flows(m)
    m[9, 9] = -(2 ** 31)
    with pytest.raises(ValueError, match="negative"):
        ops.masks_to_flows(m)
    with pytest.raises(ValueError):
        ops.masks_to_flows(m.to(torch.int64))


# ---- 2. target warp -------------------------------------------------------------------------------------------------
SHAPES = [(40, 56), (72, 48)]


def _random_planes(seed=3):
    rng = np.random.default_rng(seed)
    return [np.stack([rng.random(s, dtype=np.float32), *(rng.standard_normal((2, *s), dtype=np.float32) * 0.6)]) for s in SHAPES]


def _pool(planes, dev):
    from classpose_amd import augment
    px_off, hw, _px = augment.pool_table([p.shape[1:] for p in planes])
    return (torch.from_numpy(fr.pack_planes(planes)).to(dev), torch.from_numpy(px_off).to(dev), torch.from_numpy(hw).to(dev))


def test_warp_identity_returns_the_planes(cuda):
    from classpose_amd import augment, ops
    planes = _random_planes()
    tgt, px_off, hw = _pool(planes, cuda)
    for i, p in enumerate(planes):
        out, status = ops.warp_flow_targets(tgt, px_off, hw, [i], augment.identity_maps(1), augment.identity_vecs(1), p.shape[1:])
        assert int(status.item()) == 0 and np.array_equal(out[0].cpu().numpy().view(np.int32), p.view(np.int32)), i
    # a window that leaves the source: zeros beyond it, mask channel included
    out, _ = ops.warp_flow_targets(tgt, px_off, hw, [0], augment.identity_maps(1), augment.identity_vecs(1), (64, 64))
    o = out[0].cpu().numpy()
    assert np.array_equal(o[:, :40, :56], planes[0]) and not o[:, 40:].any() and not o[:, :, 56:].any()
    with pytest.raises(ValueError, match="outside the pool"):
        ops.warp_flow_targets(tgt, px_off, hw, [2], augment.identity_maps(1), augment.identity_vecs(1), (8, 8))


def test_warp_exact_quarter_turns_and_flips_are_index_shuffles(cuda):
    """Integer inverse maps and vector matrices of 0 / +-1: the result is the numpy index shuffle of the planes with the flow pair
    permuted / negated, value for value (0 * a + b and -a + 0 are exact; a zero's sign is not compared)."""
    from classpose_amd import ops
    planes = _random_planes()
    tgt, px_off, hw = _pool(planes, cuda)
    for i, p in enumerate(planes):
        h, w = p.shape[1:]
        cases = {
            "quarter turn": ([0, 1, 0, -1, 0, h - 1], [0, 1, -1, 0], (w, h), np.stack([fr.rot90(p[0]), fr.rot90(p[2]), -fr.rot90(p[1])])),
            "quarter turn back": ([0, -1, w - 1, 1, 0, 0], [0, -1, 1, 0], (w, h), np.stack([np.rot90(p[0]), -np.rot90(p[2]), np.rot90(p[1])])),
            "half turn": ([-1, 0, w - 1, 0, -1, h - 1], [-1, 0, 0, -1], (h, w), np.stack([p[0][::-1, ::-1], -p[1][::-1, ::-1], -p[2][::-1, ::-1]])),
            "flip": ([-1, 0, w - 1, 0, 1, 0], [1, 0, 0, -1], (h, w), np.stack([p[0][:, ::-1], p[1][:, ::-1], -p[2][:, ::-1]])),
            "flip + quarter turn": ([0, -1, w - 1, -1, 0, h - 1], [0, -1, -1, 0], (w, h),
                                    np.stack([fr.rot90(p[0][:, ::-1]), -fr.rot90(p[2][:, ::-1]), -fr.rot90(p[1][:, ::-1])])),
        }
        for name, (inv, vec, out_hw, want) in cases.items():
            out, _ = ops.warp_flow_targets(tgt, px_off, hw, [i], np.array([inv], np.float64), np.array([vec], np.float64), out_hw)
            assert np.array_equal(out[0].cpu().numpy(), want), (i, name)


def test_warp_random_maps_equal_the_numpy_restatement(cuda):
    """Two image shapes in one pool, 64 x 64 crops that leave the source (both images are smaller than the crop in one direction):
    bitwise the restatement of the kernel's arithmetic, like tests/test_gpu_augment.py checks cpx_warp_affine_f32."""
    from classpose_amd import augment, ops
    planes = _random_planes(11)
    tgt, px_off, hw = _pool(planes, cuda)
    rng = np.random.default_rng(21)
    image_of = np.array([0, 1, 1, 0, 1, 0, 0, 1])
    sh = np.array([SHAPES[i][0] for i in image_of])
    sw = np.array([SHAPES[i][1] for i in image_of])
    p = augment.sample_affine_params(rng, len(image_of), sh, sw, 64, 1.0)
    p["dxy"] = p["dxy"] + rng.uniform(-12, 12, p["dxy"].shape)          # push some crops further out of their source
    assert p["flip"].any() and not p["flip"].all()
    inv = augment.affine_inverse(p["flip"], p["theta"], p["scale"], p["dxy"], sh, sw, 64)
    vec = augment.flow_vec(p["flip"], p["theta"])
    out, status = ops.warp_flow_targets(tgt, px_off, hw, image_of, inv, vec, (64, 64))
    again, _ = ops.warp_flow_targets(tgt, px_off, hw, image_of, inv, vec, (64, 64))
    want = fr.warp_flow_targets(planes, image_of, inv, vec, 64, 64)
    got = out.cpu().numpy()
    outside = [float((want[t, 0] == 0).mean()) for t in range(len(image_of))]
    print(f"  share of output pixels outside the source per crop: {np.round(outside, 2).tolist()}")
    assert max(outside) > 0.2 and int(status.item()) == 0 and torch.equal(out, again)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_warp_of_the_device_flows_equals_the_flows_of_the_turned_map(cuda, oracle_flows):
    """Sign conventions without cellpose: the device flows of rot90(m) (and of the flipped m) against the device warp -- exact integer
    maps, vec from ``augment.flow_vec`` rounded to its exact 0 / +-1 -- of the device flows of m, within 2^-23 (one float32 rounding
    of values in [-1, 1] on either side, plus the 1e-9 of the symmetry itself), the centre pixel of each label left out."""
    from classpose_amd import augment, ops
    m, _F, skip = oracle_flows["symmetric"]
    h, w = m.shape
    base = ops.masks_to_flows(torch.from_numpy(m).to(cuda))
    tgt = torch.cat([torch.from_numpy((m > 0).astype(np.float32)).to(cuda)[None], base]).contiguous()
    px_off, hw_t, _px = augment.pool_table([(h, w)])
    px_off, hw_t = torch.from_numpy(px_off).to(cuda), torch.from_numpy(hw_t).to(cuda)
    for name, mt, inv, flip, theta, sk in (
            ("quarter turn", fr.rot90(m).copy(), [0, 1, 0, -1, 0, h - 1], False, np.pi / 2, fr.rot90(skip)),
            ("flip", m[:, ::-1].copy(), [-1, 0, w - 1, 0, 1, 0], True, 0.0, skip[:, ::-1])):
        vec = augment.flow_vec([flip], [theta])
        assert np.abs(vec - np.round(vec)).max() < 1e-15
        # the linear part of the inverse map of the same draw is that of this integer map, up to the rounding of cos / sin of pi / 2
        full = augment.affine_inverse([flip], [theta], [1.0], [[0.0, 0.0]], h, w, h)
        assert np.abs(full[0, [0, 1, 3, 4]] - np.array(inv, np.float64)[[0, 1, 3, 4]]).max() < 1e-15
        warped, _ = ops.warp_flow_targets(tgt.view(-1), px_off, hw_t, [0], np.array([inv], np.float64), np.round(vec), (h, w))
        direct = ops.masks_to_flows(torch.from_numpy(mt).to(cuda))
        wn, dn = warped[0].cpu().numpy(), direct.cpu().numpy()
        assert np.array_equal(wn[0], (mt > 0).astype(np.float32))
        d = np.abs(wn[1:].astype(np.float64) - dn).max(0)
        print(f"  {name}: max |warp(flows(m)) - flows(turned m)| off the centres = {d[~sk].max():.3e}; at the centres {d[sk].max():.3e}")
        assert int(sk.sum()) <= int(m.max()) and d[~sk].max() <= 2.0 ** -23, name


# ---- 3. seg loss ----------------------------------------------------------------------------------------------------
def _seg_case(name):
    rng = np.random.default_rng({"token": 1, "small": 2, "big": 3, "extreme": 4, "zeros": 5}[name])
    n, H, W = {"token": (1, 8, 8), "small": (3, 16, 24), "big": (2, 256, 256), "extreme": (2, 16, 16), "zeros": (2, 16, 24)}[name]
    z = rng.standard_normal((n, 3, H, W), dtype=np.float32) * np.float32(3.0)
    tg = np.stack([rng.random((n, H, W), dtype=np.float32), *(np.clip(rng.standard_normal((2, n, H, W), dtype=np.float32) * 0.5, -1, 1))], 1)
    if name == "extreme":
        z = np.where(rng.random(z.shape) < 0.5, np.float32(80.0), np.float32(-80.0)).astype(np.float32)
    if name == "zeros":
        tg[:] = 0
    return torch.from_numpy(z), torch.from_numpy(np.ascontiguousarray(tg))


@pytest.mark.parametrize("name", ["token", "small", "big", "extreme", "zeros"])
def test_seg_loss_against_float64_autograd(cuda, name):
    from classpose_amd import ops
    z32, tg = _seg_case(name)
    n, _c, H, W = z32.shape
    head = fr.head_with_flow_logits(z32, ncls=3, seed=1).to(cuda)
    o = ops.seg_loss(head, tg.to(cuda))
    o2 = ops.seg_loss(head, tg.to(cuda))
    assert torch.equal(tr.tokens_to_nchw(head.cpu(), 0, 3, n, H, W), z32)          # the logits the device read
    r64, r32 = fr.seg_loss_and_grad(z32, tg, torch.float64), fr.seg_loss_and_grad(z32, tg, torch.float32)
    print(f"{name}: flow = {o.flow.item():.9g} (float64 {float(r64['flow']):.9g}), cp = {o.cp.item():.9g} (float64 {float(r64['cp']):.9g})")
    for k in ("flow", "cp", "dlogits"):
        assert bool(torch.isfinite(getattr(o, k)).all()), k
        assert torch.equal(getattr(o, k), getattr(o2, k)), f"{k}: two runs are bitwise equal"
    _check("flow", o.flow.cpu(), r32["flow"], r64["flow"])
    _check("cp", o.cp.cpu(), r32["cp"], r64["cp"])
    _check("dlogits", tr.tokens_to_nchw(o.dlogits.cpu(), 0, 3, n, H, W), r32["dlogits"], r64["dlogits"])
    # the class columns of the head buffer are noise and do not matter: other noise, same bits
    other = fr.head_with_flow_logits(z32, ncls=3, seed=2).to(cuda)
    assert not torch.equal(other[:, 192:], head[:, 192:])
    o3 = ops.seg_loss(other, tg.to(cuda))
    assert all(torch.equal(getattr(o, k), getattr(o3, k)) for k in ("flow", "cp", "dlogits"))
    # w_seg scales the gradient alone
    o4 = ops.seg_loss(head, tg.to(cuda), w_seg=0.5)
    assert torch.equal(o4.flow, o.flow) and torch.equal(o4.cp, o.cp)
    _check("dlogits at w_seg = 0.5", tr.tokens_to_nchw(o4.dlogits.cpu(), 0, 3, n, H, W), 0.5 * r32["dlogits"], 0.5 * r64["dlogits"])


# ---- 4. trainer -----------------------------------------------------------------------------------------------------
NCLS = 7


def _crops(n, seed0=300):
    """uint8 crops of the synthetic slide, class maps from its analytic fields with a -100 band, and disc instance maps."""
    from classpose_amd import synth
    ims, labs, inst = [], [], []
    for k in range(n):
        x0, y0 = 256 * (k % 4), 256 * (k // 4)
        ims.append(synth.render_region(seed0, x0, y0, 256, 256))
        lab = synth.analytic_fields(seed0, x0, y0, 256, 256, NCLS)[2].argmax(0).astype(np.int16)
        lab[(40 + 11 * k) % 200:][:24] = -100
        labs.append(lab)
        inst.append(fr.disc_crop(50 + k))
    return np.stack(ims), np.stack(labs), np.stack(inst)


@pytest.fixture(scope="module")
def data(cuda):
    """Four crops, their class maps, instance maps and the device flow targets built once from them."""
    from classpose_amd import augment
    ims, labs, inst = _crops(4)
    tg = torch.stack(augment.flow_targets_of(list(inst), cuda))
    assert tg.shape == (4, 3, 256, 256) and tg.dtype == torch.float32
    assert torch.equal(tg[:, 0], torch.from_numpy((inst > 0).astype(np.float32)).to(cuda))
    return ims, labs, inst, tg


def _trainer(cuda, precision="bf16", flow=True, **kw):
    from classpose_amd import synth
    from classpose_amd.train import HeadTrainer
    sd = synth.make_state_dict(NCLS, None, depth=2, seed=11)
    return HeadTrainer(sd, device=cuda, precision=precision, feature_batch=4, train_flow_head=flow, **kw), sd


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_twenty_steps_with_both_heads_follow_the_float64_replay(cuda, data, precision):
    ims, labs, _inst, tg = data
    t, _sd = _trainer(cuda, precision)
    steps = 20
    feat = t.features(ims)
    lrs = [float(x) for x in np.minimum(np.linspace(0, 4e-3, 10), 2e-3)] + [2e-3] * 10
    Wc0, bc0, Wf0, bf0 = t.w.cpu().clone(), t.b.cpu().clone(), t.flow.w.cpu().clone(), t.flow.b.cpu().clone()
    res = [t.step(feat, labs, lr, flow_targets=tg) for lr in lrs]
    dev_losses, dev_seg = np.array([r["loss"] for r in res]), np.array([r["seg"] for r in res])
    assert all(abs(r["loss"] - (r["seg"] + r["ce"] + r["tversky"])) <= 1e-6 * abs(r["loss"]) for r in res) and t.n_steps == steps
    lab = torch.from_numpy(labs)
    args = (feat.cpu(), lab, tg.cpu(), Wc0, bc0, Wf0, bf0, lrs)
    l64, s64, Wc64, bc64, Wf64, bf64 = fr.replay_two_heads(*args, torch.float64, t.dtype, NCLS, t.weight_decay)
    l32, s32, Wc32, bc32, Wf32, bf32 = fr.replay_two_heads(*args, torch.float32, t.dtype, NCLS, t.weight_decay)
    print(f"{precision}: loss step 1 = {dev_losses[0]:.6f} (replay {l64[0]:.6f}), step {steps} = {dev_losses[-1]:.6f} (replay {l64[-1]:.6f}); "
          f"seg {dev_seg[0]:.6f} -> {dev_seg[-1]:.6f} (replay {s64[0]:.6f} -> {s64[-1]:.6f})")
    floor = steps * FLOOR
    _check("loss curve", dev_losses, l32, l64, floor)
    _check("seg loss curve", dev_seg, s32, s64, floor)
    for name, dv, v0, v32, v64 in (("class weight", t.w, Wc0, Wc32, Wc64), ("class bias", t.b, bc0, bc32, bc64),
                                   ("flow weight", t.flow.w, Wf0, Wf32, Wf64), ("flow bias", t.flow.b, bf0, bf32, bf64)):
        _check(f"final master {name} update", dv.cpu().double() - v0.double(), v32.double() - v0.double(), v64 - v0.double(), floor)
    assert l64[-1] < l64[0] and s64[-1] < s64[0], "the chosen inputs are meant to train"
    assert dev_losses[-1] < dev_losses[0] and dev_seg[-1] < dev_seg[0]


def test_without_targets_the_class_head_is_bitwise_the_class_only_trainer(cuda, data):
    ims, labs, _inst, tg = data
    a, _ = _trainer(cuda, flow=True)
    b, _ = _trainer(cuda, flow=False)
    feat = a.features(ims)
    assert torch.equal(feat, b.features(ims))
    f0 = a.flow.w.clone()
    for lr in (0.0, 1e-3, 2e-3, 2e-3, 2e-3):
        ra, rb = a.step(feat, labs, lr), b.step(feat, labs, lr)
        assert ra == rb and "seg" not in ra
    assert torch.equal(a.w, b.w) and torch.equal(a.b, b.b) and torch.equal(a.m_w, b.m_w) and torch.equal(a.v_b, b.v_b)
    assert torch.equal(a.flow.w, f0), "the flow head does not move without targets"
    assert torch.equal(a.evaluate(feat, labs, return_head=True)["head"], b.evaluate(feat, labs, return_head=True)["head"])
    # with targets the class head still takes the very same step: its gradient does not see the flow columns
    ra, rb = a.step(feat, labs, 2e-3, flow_targets=tg), b.step(feat, labs, 2e-3)
    assert torch.equal(a.w, b.w) and torch.equal(a.b, b.b) and ra["ce"] == rb["ce"] and not torch.equal(a.flow.w, f0)
    with pytest.raises(ValueError, match="without train_flow_head"):
        b.step(feat, labs, 1e-3, flow_targets=tg)
    with pytest.raises(ValueError, match="flow_targets"):
        a.step(feat, labs, 1e-3, flow_targets=tg[:, :2])


def test_thirty_steps_on_disc_crops_lower_the_seg_loss(cuda, data):
    ims, labs, _inst, tg = data
    t, _ = _trainer(cuda)
    feat = t.features(ims)
    seg = [t.step(feat, labs, 2e-3, flow_targets=tg)["seg"] for _ in range(30)]
    print(f"seg loss: first {seg[0]:.5f}, last {seg[-1]:.5f}")
    assert np.all(np.isfinite(seg)) and seg[-1] < seg[0]


def test_the_unet_trainer_shares_the_flow_head(cuda, data):
    """UNetHeadTrainer uses the same FlowHead object: from equal flow heads and equal features, one step moves ``out`` identically."""
    from classpose_amd import synth
    from classpose_amd.train import FlowHead
    from classpose_amd.train_unet import UNetHeadTrainer
    ims, labs, _inst, tg = data
    sd = synth.make_state_dict(NCLS, None, depth=2, seed=11)
    u = UNetHeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4, feature_transformation_structure=[16, 24], train_flow_head=True)
    h, _ = _trainer(cuda)
    assert isinstance(u.flow, FlowHead) and torch.equal(u.flow.w, h.flow.w)
    feat = u.features(ims[:2])
    ru, rh = u.step(feat, labs[:2], 2e-3, flow_targets=tg[:2]), h.step(feat, labs[:2], 2e-3, flow_targets=tg[:2])
    assert ru["seg"] == rh["seg"] and torch.equal(u.flow.w, h.flow.w) and torch.equal(u.flow.b, h.flow.b)
    assert set(u.state_dict()) == set(u.sd) and not torch.equal(u.state_dict()["out.weight"], sd["out.weight"])
    assert "seg" not in u.step(feat, labs[:2], 2e-3)


# ---- 5. the checkpoint ----------------------------------------------------------------------------------------------
def test_the_saved_checkpoint_serves_inference(cuda, data, tmp_path):
    import ctypes as C
    from classpose_amd import _lib, engine, models
    from classpose_amd.train import HeadTrainer
    ims, labs, _inst, tg = data
    t, sd = _trainer(cuda)
    feat = t.features(ims)
    for _ in range(3):
        t.step(feat, labs, 2e-3, flow_targets=tg)
    t.set_diam_labels([20.0, 30.0])
    t.save(tmp_path / "both.pt")
    ck = torch.load(tmp_path / "both.pt", map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and ck["out.weight"].shape == (192, 256, 1, 1) and ck["out.bias"].shape == (192,)
    assert not torch.equal(ck["out.weight"], sd["out.weight"]) and torch.equal(ck["W2"], sd["W2"])
    assert float(ck["diam_labels"]) == 25.0 and float(ck["diam_mean"]) == float(sd["diam_mean"])
    assert all(torch.equal(ck[k], sd[k]) for k in sd if not k.startswith(("out.", "out_class.")) and k != "diam_labels")
    t.save(tmp_path / "only.pt", save_only_trainable_params=True)
    assert set(torch.load(tmp_path / "only.pt", weights_only=True)) == {"out_class.weight", "out_class.bias", "out.weight", "out.bias"}
    # the inference forward on the saved weights computes the trainer's flow and class columns, bit for bit
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    ev_head = t.evaluate(ims, labs, flow_targets=tg, return_head=True)["head"].clone()      # (a view that the next call overwrites)
    L = _lib.lib()
    ws = torch.empty(L.cpx_net_workspace_bytes(4, w.c.dtype), dtype=torch.uint8, device=cuda)
    head = torch.empty((4 * 1024, w.c.ld_head), dtype=torch.float32, device=cuda)
    _lib.check(L.cpx_net_forward(C.byref(w.c), _lib.ptr(t._patches(ims)), 4, _lib.ptr(head), _lib.ptr(ws), ws.numel(),
                                 torch.cuda.current_stream(cuda).cuda_stream), "net_forward")
    assert torch.equal(head[:, :192 + NCLS * 64], ev_head[:, :192 + NCLS * 64])
    # ClassposeModel on a training crop returns the dP and cellprob that the trainer's head columns hold: the model pads the crop and
    # cuts it into 2 x 2 overlapping sub-tiles (core.run_net), so the trainer's head runs on those same sub-tiles (patch rows in,
    # one launch of four like the model's) and its flow columns go through the same blend
    from classpose_amd import ops
    patches, til = ops.make_patches(torch.from_numpy(ims[:1]).to(cuda), dtype=t.dtype)
    assert til.ny * til.nx == 4
    th = t.head(t.features(patches))
    dP_t, cp_t, _lg = ops.blend_head(th, w.c.ld_head, NCLS, til, 1)
    m = models.ClassposeModel(pretrained_model=str(tmp_path / "both.pt"), device=cuda, precision="bf16", max_batch_tiles=1)
    _masks, flows, _cm, _styles = m.eval(ims[0])
    dP, cp = flows[1], flows[2]
    assert dP.shape == (2, 256, 256) and cp.shape == (256, 256)
    print(f"ClassposeModel against the trainer's blended head columns: max |dP difference| = {np.abs(dP - dP_t[0].cpu().numpy()).max():.3e}, "
          f"max |cellprob difference| = {np.abs(cp - cp_t[0].cpu().numpy()).max():.3e}")
    assert np.array_equal(dP, dP_t[0].cpu().numpy()) and np.array_equal(cp, cp_t[0].cpu().numpy())
    m0 = models.ClassposeModel(pretrained_model=sd, device=cuda, precision="bf16", max_batch_tiles=1)
    assert not np.array_equal(m0.eval(ims[0])[1][1], dP), "the untrained checkpoint gives other flows"
    # reloading into a trainer: the same master weights
    r = HeadTrainer(ck, device=cuda, precision="bf16", feature_batch=4, train_flow_head=True)
    assert torch.equal(r.flow.w, t.flow.w) and torch.equal(r.flow.b, t.flow.b) and torch.equal(r.w, t.w)
    assert torch.equal(r.evaluate(feat, labs, flow_targets=tg, return_head=True)["head"], ev_head)


# ---- 6. end to end --------------------------------------------------------------------------------------------------
def _two_images():
    """Two annotated images, 300 x 280 and 256 x 256: pixels from the synthetic slide, disc instances of class 1 or 2."""
    from classpose_amd import synth
    out = []
    for k, (h, w) in enumerate([(300, 280), (256, 256)]):
        im = synth.render_region(300, 64 * k, 32 * k, w, h)
        inst = np.zeros((h, w), np.int32)
        inst[:256, :256] = fr.disc_crop(70 + k) * 3                  # ids 3, 6, ...: renumbered on the way in
        lab = np.where(inst > 0, 1 + (inst // 3) % 2, 0).astype(np.int16)
        out.append((im, lab, inst))
    return out


def test_train_class_head_end_to_end_on_a_pool(cuda, tmp_path):
    import io
    import logging
    from classpose_amd import augment, synth
    from classpose_amd.train import HeadTrainer, train_class_head
    trip = _two_images()
    assert trip[0][0].shape == (300, 280, 3) and trip[1][0].shape == (256, 256, 3)
    sd = synth.make_state_dict(3, None, depth=2, seed=11)
    pool = augment.ImagePool([t[0] for t in trip], [t[1] for t in trip], device=cuda, instances=[t[2] for t in trip])
    plain = augment.ImagePool([t[0] for t in trip], [t[1] for t in trip], device=cuda)
    assert plain.pool_tgt is None and pool.nbytes - plain.nbytes == 12 * pool.pool_px and pool.pool_tgt.numel() == 3 * pool.pool_px
    assert torch.equal(plain.pool_u8, pool.pool_u8) and torch.equal(plain.pool_lab, pool.pool_lab)
    # asking for the targets changes no draw and no crop
    xa, ya, ta = augment.augment_batch_pool(pool, [0, 1, 0], np.random.default_rng(3), config="geometry", flow_targets=True)
    xb, yb = augment.augment_batch_pool(plain, [0, 1, 0], np.random.default_rng(3), config="geometry")
    assert torch.equal(xa, xb) and torch.equal(ya, yb) and ta.shape == (3, 3, 256, 256) and bool(torch.isfinite(ta).all())
    assert float(ta[:, 1:].abs().max()) <= 1.0 + 2.0 ** -20 and 0.0 <= float(ta[:, 0].min()) and float(ta[:, 0].max()) <= 1.0
    tr_ = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4, train_flow_head=True)
    buf = io.StringIO()
    handler = logging.StreamHandler(buf)
    logging.getLogger("classpose_amd.train").addHandler(handler)
    try:
        path, tl, vl = train_class_head(tr_, pool, None, pool, None, batch_size=2, n_epochs=2, learning_rate=2e-3, augment="geometry",
                                        save_path=tmp_path, model_name="both", train_flow_head=True)
    finally:
        logging.getLogger("classpose_amd.train").removeHandler(handler)
    text = buf.getvalue()
    print(text[-600:])
    assert np.all(np.isfinite(tl)) and np.all(np.isfinite(vl)) and len(tl) == 2
    assert text.count("seg=") >= 4, "the seg loss is logged per epoch, training and validation"
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert not torch.equal(ck["out.weight"], sd["out.weight"]) and not torch.equal(ck["out_class.weight"], sd["out_class.weight"])
    with pytest.raises(ValueError, match="instances"):
        train_class_head(tr_, plain, None, batch_size=2, n_epochs=1, save_path=tmp_path, model_name="x", train_flow_head=True)


def test_pre_cut_crops_warp_their_targets_like_a_pool_and_train(cuda, data, tmp_path):
    """Pre-cut crops of equal shape are a pool with a regular table: ``augment_batch(..., flow_targets=)`` returns bitwise what
    ``augment_batch_pool`` returns on a pool of the same images, and asking for the targets changes nothing else.  Then
    ``train_class_head`` on arrays with ``instances`` / ``test_instances``, from cached features and augmented."""
    from classpose_amd import augment
    from classpose_amd.train import train_class_head
    ims, labs, inst, tg = data
    pool = augment.ImagePool(list(ims), list(labs), device=cuda, instances=list(inst))
    assert torch.equal(pool.pool_tgt.view(4, 3, 256, 256), tg)
    xa, ya, ta = augment.augment_batch(ims, labs, np.random.default_rng(9), config="geometry", device=cuda, flow_targets=tg)
    xp, yp, tp = augment.augment_batch_pool(pool, np.arange(4), np.random.default_rng(9), config="geometry", flow_targets=True)
    x0, y0 = augment.augment_batch(ims, labs, np.random.default_rng(9), config="geometry", device=cuda)
    assert torch.equal(xa, xp) and torch.equal(ya, yp) and torch.equal(ta, tp) and torch.equal(xa, x0) and torch.equal(ya, y0)
    assert bool((ta[:, 1:].abs() > 0.5).any()) and not torch.equal(ta, tg)
    assert torch.equal(augment.grid_flow_targets(pool), tg), "a 256 x 256 image is its own grid window"
    for k, aug in enumerate((None, "geometry")):
        t, sd = _trainer(cuda)
        path, tl, vl = train_class_head(t, ims, labs, ims[:2], labs[:2], batch_size=2, n_epochs=2, learning_rate=2e-3, augment=aug,
                                        save_path=tmp_path / str(k), model_name="m", train_flow_head=True, instances=inst,
                                        test_instances=inst[:2])
        assert np.all(np.isfinite(tl)) and np.all(np.isfinite(vl)) and not torch.equal(t.flow.w.cpu(), sd["out.weight"].reshape(192, 256))
    with pytest.raises(ValueError, match="needs instances"):
        train_class_head(t, ims, labs, n_epochs=1, save_path=tmp_path, model_name="x", train_flow_head=True)
    with pytest.raises(ValueError, match="train_flow_head=True"):
        train_class_head(t, ims, labs, n_epochs=1, save_path=tmp_path, model_name="x", instances=inst)


def test_cli_freeze_backbone_neck_in_a_child_process(cuda, tmp_path):
    from classpose_amd import engine, synth
    sd = synth.make_state_dict(1, None, depth=2, seed=12)              # a plain backbone: the CLI initialises the class head
    torch.save(sd, tmp_path / "backbone.pt")
    trip = _two_images()
    d = tmp_path / "data"
    d.mkdir()
    imgs = np.empty(2, dtype=object)
    labs = np.empty(2, dtype=object)
    for k, (im, lab, inst) in enumerate(trip):
        imgs[k] = im
        labs[k] = np.stack([inst, lab.astype(np.int32)], -1)
    np.save(d / "images.npy", imgs, allow_pickle=True)
    np.save(d / "labels.npy", labs, allow_pickle=True)
    cmd = [sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--data_path", str(d), "--train_fraction", "1", "--freeze", "backbone",
           "neck", "--pretrained_model", str(tmp_path / "backbone.pt"), "--nclasses", "3", "--n_epochs", "2", "--batch_size", "2",
           "--learning_rate", "1e-3", "--augment", "geometry", "--save_path", str(tmp_path), "--model_name", "m", "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    assert "seg=" in r.stdout + r.stderr
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["out.weight"].shape == (192, 256, 1, 1) and not torch.equal(ck["out.weight"], sd["out.weight"])
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    assert w.ncls == 3 and w.c.n_unet_ops == 0
