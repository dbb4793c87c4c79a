"""Device training of the neck (csrc/cpx_train_neck.hip -> ops -> classpose_amd.train.NeckParams / HeadTrainer(train_neck=True) ->
the train_head CLI).  The network is synth.make_state_dict(3, None, depth=1): every shape of the neck is fixed by the architecture
except the crop count; nS = 1 is one image and two weight-gradient slabs, nS = 3 an odd image count (the 3x3 taps and the col2im
must not cross a crop's border).  Every workspace is poisoned (0xFF bytes, NaN gradients) before the call that fills it.

Bounds, u = 2^-24:
  LayerNorm backward   everything is formed in float64 and rounded once: |got - exact| <= u |exact| + 2^-40 S, S = the sum of the
                       magnitudes of the terms of that element (neck_train_reference.ln_backward), exact = the float64 formula on
                       the same stored y.  Zero rows of dout give exactly zero rows of dy.
  dW0, dW2             |got - exact| <= (L + P + 2) u sum|dY||X|: L = cpx_unet_wgrad_slab_rows() rows go through one MFMA
                       accumulator chain, P = ceil(rows / L) slab partials are added in float64 (tests/test_gpu_unet_train.py).
  dfeat, da1           a float32 dot product over Npad terms in the GEMM's order, then `taps` of them added one by one onto a zero:
                       |got - exact| <= (Npad + taps + 2) u sum|dY||W| (same header; Npad = ld_head and 1 tap, 256 and 9 taps).
  every stage is compared on the device's OWN stored tensors and OWN incoming gradient.
End to end and training: the project's rule, err(x) = ||x - q64||_2 / ||q64||_2:
    err(device) <= max(4 * err(torch CPU float32), 2^-20)
with q64 from tests/neck_train_reference.py on the same x, labels and targets (bf16 / fp16: the straight-through replay).
Every test prints what it observed before it asserts (run with -s)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_train_reference as fr
import neck_train_reference as nr
import train_reference as tr
from classpose_amd import _lib, engine, ops, synth
from classpose_amd._lib import ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
FLOOR = 2.0 ** -20
NCLS = 3
HD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_W = {}


def _weights(prec, dev):
    if prec not in _W:
        sd = synth.make_state_dict(NCLS, None, depth=1, seed=41)
        _W[prec] = (sd, engine.NetWeights.from_state_dict(sd, prec, dev))
    return _W[prec]


def _vec(sd, key, prec, dev):
    """an epilogue vector as NetWeights keeps it: rounded through the network dtype, float32"""
    return sd[key].float().to(HD[prec]).float().to(dev)


def _labels(n, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros((n, 256, 256), np.int16)
    for b in range(n):
        coarse = rng.integers(0, ncls, (16, 16))
        coarse.reshape(-1)[rng.permutation(256)[:ncls]] = np.arange(ncls)
        lab[b] = np.kron(coarse, np.ones((16, 16), np.int64))
        lab[b, 30 + 17 * b:][:9] = -100
        lab[b, 100:131, 200:223] = -100
        lab[b][rng.random((256, 256)) < 0.02] = -100
    return lab


def _targets(n, seed):
    """(n, 3, 256, 256) float32 flow-head targets: a blocky mask and smooth flows in [-1, 1]"""
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(n, 1, 16, 16, generator=g) > 0.5).float().repeat_interleave(16, 2).repeat_interleave(16, 3)
    flow = torch.tanh(F.interpolate(torch.randn(n, 2, 32, 32, generator=g), size=256, mode="bilinear")) * mask
    return torch.cat([mask, flow], 1).contiguous()


def _x_rows(nS, prec, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(nS * 1024, 1024, generator=g, device=dev).to(HD[prec])


def _check(name, dev_val, f32_val, f64_val, floor=FLOOR):
    e_dev, e_cpu = tr.rel_l2(dev_val, f64_val), tr.rel_l2(f32_val, f64_val)
    tol = max(4 * e_cpu, floor)
    print(f"  {name}: err(device) = {e_dev:.3e}, err(torch CPU float32) = {e_cpu:.3e}, tolerance = {tol:.3e}")
    assert e_dev <= tol, (name, e_dev, e_cpu, tol)


def _forward_train(w, x, dev):
    """the training tail into a 0xFF workspace and a NaN head"""
    nS = x.shape[0] // 1024
    ws = ops.neck_train_workspace(nS, w.c.dtype, dev)
    ws.fill_(0xFF)
    head = torch.full((x.shape[0], w.c.ld_head), float("nan"), dtype=torch.float32, device=dev)
    return ops.neck_forward_train(w, x, head=head, workspace=ws)


# ---- 1. forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS", [1, 3])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_forward_train_is_bitwise_the_tail_of_net_forward(cuda, prec, nS):
    sd, w = _weights(prec, cuda)
    hd, c, L = HD[prec], w.c, _lib.lib()
    g = torch.Generator(device=cuda).manual_seed(3 + nS)
    patches = torch.randn(nS * 1024, 192, generator=g, device=cuda).to(hd)
    ws = torch.full((L.cpx_net_workspace_bytes(nS, c.dtype),), 0xFF, dtype=torch.uint8, device=cuda)
    head = torch.full((nS * 1024, c.ld_head), float("nan"), dtype=torch.float32, device=cuda)
    _lib.check(L.cpx_net_forward(C.byref(c), ptr(patches), nS, ptr(head), ptr(ws), ws.numel(), torch.cuda.current_stream(cuda).cuda_stream),
               "net_forward")
    x = ops.backbone_rows(ws, nS, hd).clone()
    feat = ops.neck_features(ws, nS, hd).clone()
    assert bool(torch.isfinite(x.float()).all()) and float(x.float().abs().max()) > 0
    o = _forward_train(w, x, cuda)
    torch.cuda.synchronize(cuda)
    same_head, same_feat = torch.equal(o.head, head), torch.equal(o.feat.view(torch.uint8), feat.view(torch.uint8))
    ln1 = ops.layernorm(o.y0.contiguous(), _vec(sd, "encoder.neck.1.weight", prec, cuda), _vec(sd, "encoder.neck.1.bias", prec, cuda))
    same_ln = torch.equal(ln1.view(torch.uint8), o.a1.view(torch.uint8))
    finite = all(bool(torch.isfinite(t.float()).all()) for t in (o.y0, o.a1, o.y2))
    print(f"{prec} nS={nS}: head equal {same_head}, feat equal {same_feat}, LN(y0) == a1 {same_ln}, intermediates finite {finite}; "
          f"max |head| {float(head.abs().max()):.3f}")
    assert same_head and same_feat and same_ln and finite
    assert bool(torch.isfinite(head).all())
    assert L.cpx_net_backbone_offset(0, c.dtype) == 2 ** 64 - 1 and L.cpx_net_backbone_offset(nS, 7) == 2 ** 64 - 1


def test_forward_train_refuses_a_unet_head(cuda):
    sd = synth.make_state_dict(NCLS, [16, 24], depth=1, seed=42)
    w = engine.NetWeights.from_state_dict(sd, "bf16", cuda)
    with pytest.raises(NotImplementedError):
        ops.neck_forward_train(w, _x_rows(1, "bf16", cuda, 1))
    ws = ops.neck_train_workspace(1, w.c.dtype, cuda)
    head = torch.zeros((1024, w.c.ld_head), dtype=torch.float32, device=cuda)
    rc = _lib.lib().cpx_neck_forward_train(C.byref(w.c), ptr(_x_rows(1, "bf16", cuda, 1)), 1, ptr(head), ptr(ws), ws.numel(),
                                           torch.cuda.current_stream(cuda).cuda_stream)
    assert rc != 0


# ---- 2. LayerNorm backward ----------------------------------------------------------------------------------------
def _ln_case(rows, prec, dev, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(rows, 256, generator=g) * torch.logspace(-1, 1, rows)[:, None] + 0.5 * torch.randn(rows, 1, generator=g)).to(HD[prec])
    gamma = 1.0 + 0.3 * torch.randn(256, generator=g)
    dout = torch.randn(rows, 256, generator=g) * torch.logspace(-3, 0, 256)[None]
    dout[::7] = 0
    return y, gamma, dout


def _ln_compare(what, got, exact, S):
    got = got.double().cpu()
    err, bound = (got - exact).abs(), U * exact.abs() + 2.0 ** -40 * S
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"  {what}: worst error / bound = {worst:.3f}, max |exact| = {float(exact.abs().max()):.3e}")
    return worst


@pytest.mark.parametrize("rows", [1024, 3072])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_layernorm_backward_every_element(cuda, prec, rows):
    y, gamma, dout = _ln_case(rows, prec, cuda, rows + 5)
    L = _lib.lib()
    nb = L.cpx_layernorm_backward_workspace_bytes(rows, 256)
    assert nb > 0 and L.cpx_layernorm_backward_workspace_bytes(rows, 1024) == 0
    yd, gd, dd = y.to(cuda), gamma.to(cuda), dout.to(cuda)
    outs = []
    for fill in (0xFF, 0x00):                                          # the result does not depend on what the workspace held
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=cuda)
        dy = torch.full((rows, 256), float("nan"), dtype=torch.float32, device=cuda)
        dg, db = (torch.full((256,), float("nan"), dtype=torch.float32, device=cuda) for _ in range(2))
        _lib.check(L.cpx_layernorm_backward(ops._DT[HD[prec]], ptr(yd), ptr(gd), ptr(dd), rows, 256, 1e-6, ptr(dy), ptr(dg), ptr(db), ptr(ws),
                                            nb, torch.cuda.current_stream(cuda).cuda_stream), "layernorm_backward")
        outs.append((dy, dg, db))
    torch.cuda.synchronize(cuda)
    dy, dg, db = outs[0]
    r = nr.ln_backward(y, gamma, dout)
    print(f"LayerNorm backward {prec} rows={rows}:")
    worst = [_ln_compare("dy", dy, r["dy"], r["S_dy"]), _ln_compare("dgamma", dg, r["dgamma"], r["S_dgamma"]),
             _ln_compare("dbeta", db, r["dbeta"], r["S_dbeta"])]
    zero_rows = not bool(dy[::7].any())
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[0], outs[1]))
    print(f"  zero rows of dout give zero rows of dy: {zero_rows}; two runs bitwise equal: {same}")
    assert max(worst) <= 1.0 and zero_rows and same
    wy, wg, wb = ops.layernorm_backward(yd, gd, dd)
    assert torch.equal(wy, dy) and torch.equal(wg, dg) and torch.equal(wb, db)


# ---- 3. the backward, stage by stage ------------------------------------------------------------------------------
def _dhead(nS, ld, dev, seed, zero_crops=()):
    g = torch.Generator(device=dev).manual_seed(seed)
    ncols = 192 + NCLS * 64
    d = torch.zeros((nS * 1024, ld), dtype=torch.float32, device=dev)
    d[:, :ncols] = torch.randn(nS * 1024, ncols, generator=g, device=dev) * torch.logspace(-3, 0, ncols, device=dev)[None]
    d[::7] = 0
    for s in zero_crops:
        d[s * 1024:(s + 1) * 1024] = 0
    return d


def _run_backward(w, x, fwd, dhead, dev):
    nS = x.shape[0] // 1024
    ws, off = ops.neck_backward_workspace(nS, w.c.dtype, w.c.ld_head, dev)
    ws.fill_(0xFF)
    n_g, _o = ops.neck_grad_layout()
    grads = torch.full((n_g,), float("nan"), dtype=torch.float32, device=dev)
    ops.neck_backward(w, x, fwd, dhead, grads, ws)
    torch.cuda.synchronize(dev)
    n = x.shape[0] * 256 * 4
    inter = {k: ws[o:o + n].view(torch.float32).view(-1, 256) for k, o in zip(("dfeat", "dy2", "da1", "dy0"), off)}
    return grads, inter


def _grad_views(grads):
    _n, off = ops.neck_grad_layout()
    return {k: grads[o:o + int(np.prod(s))].view(s) for k, o, s in zip(ops.NECK_GRAD_NAMES, off, ops.NECK_GRAD_SHAPES)}


@pytest.mark.parametrize("nS", [1, 3])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_backward_stage_by_stage(cuda, prec, nS):
    sd, w = _weights(prec, cuda)
    hd, ld = HD[prec], w.c.ld_head
    assert ops.neck_grad_layout() == (256 * 1024 + 256 * 2304 + 4 * 256, [0, 262144, 262400, 262656, 852480, 852736])
    x = _x_rows(nS, prec, cuda, 7 + nS)
    fwd = _forward_train(w, x, cuda)
    dhead = _dhead(nS, ld, cuda, 11 + nS)
    grads, inter = _run_backward(w, x, fwd, dhead, cuda)
    grads2, inter2 = _run_backward(w, x, fwd, dhead, cuda)
    same = torch.equal(grads.view(torch.int32), grads2.view(torch.int32)) and \
        all(torch.equal(inter[k].view(torch.int32), inter2[k].view(torch.int32)) for k in inter)
    finite = bool(torch.isfinite(grads).all()) and all(bool(torch.isfinite(v).all()) for v in inter.values())
    print(f"neck backward {prec} nS={nS}: two runs bitwise equal {same}, everything finite {finite}")
    assert same and finite
    G = {k: v.cpu() for k, v in _grad_views(grads).items()}
    I = {k: v.double().cpu() for k, v in inter.items()}
    y0, a1, y2 = (t.double().cpu() for t in (fwd.y0, fwd.a1, fwd.y2))
    xd, dh = x.double().cpu(), dhead.double().cpu()
    rows = nS * 1024
    Lrows = _lib.lib().cpx_unet_wgrad_slab_rows()
    P = (rows + Lrows - 1) // Lrows
    worst = {}

    def bounded(name, got, exact, bound):
        err = (got.double() - exact).abs()
        worst[name] = float((err / bound.clamp_min(1e-300)).max())
        print(f"  {name}: worst error / bound = {worst[name]:.3f}, max |exact| = {float(exact.abs().max()):.3e}")

    # 1. dfeat = dhead Wh with the rounded operand (padding rows of Wh are 0)
    Wh = torch.zeros(ld, 256, dtype=torch.float64)
    Wh[:192] = sd["out.weight"].reshape(192, 256).float().to(hd).double()
    Wh[192:192 + NCLS * 64] = sd["out_class.weight"].reshape(-1, 256).float().to(hd).double()
    bounded("dfeat", I["dfeat"], dh @ Wh, (ld + 1 + 2) * U * (dh.abs() @ Wh.abs()))
    # 2. LayerNorm 2 on the stored y2 and the device's dfeat
    g2 = sd["encoder.neck.3.weight"].float().to(hd).double()
    r = nr.ln_backward(y2, g2, I["dfeat"])
    for name, got, key in (("dy2", I["dy2"], "dy"), ("dgamma2", G["gamma2"], "dgamma"), ("dbeta2", G["beta2"], "dbeta")):
        bounded(name, got, r[key], U * r[key].abs() + 2.0 ** -40 * r["S_" + key])
    # 3. the 3x3 conv on the stored a1 and the device's dy2
    W2 = sd["encoder.neck.2.weight"].float().to(hd).double()

    def conv_grads(a, wv, dy):
        a, wv = a.clone().requires_grad_(True), wv.clone().requires_grad_(True)
        F.conv2d(a.reshape(nS, 32, 32, 256).permute(0, 3, 1, 2), wv, padding=1).backward(dy.reshape(nS, 32, 32, 256).permute(0, 3, 1, 2))
        return wv.grad.permute(0, 2, 3, 1).reshape(256, 2304), a.grad

    dW2, da1 = conv_grads(a1, W2, I["dy2"])
    mW2, ma1 = conv_grads(a1.abs(), W2.abs(), I["dy2"].abs())
    bounded("dW2", G["W2"], dW2, (Lrows + P + 2) * U * mW2)
    bounded("da1", I["da1"], da1, (256 + 9 + 2) * U * ma1)
    # 4. LayerNorm 1 on the stored y0 and the device's da1
    g1 = sd["encoder.neck.1.weight"].float().to(hd).double()
    r = nr.ln_backward(y0, g1, I["da1"])
    for name, got, key in (("dy0", I["dy0"], "dy"), ("dgamma1", G["gamma1"], "dgamma"), ("dbeta1", G["beta1"], "dbeta")):
        bounded(name, got, r[key], U * r[key].abs() + 2.0 ** -40 * r["S_" + key])
    # 5. dW0 = dy0^T x
    bounded("dW0", G["W0"], I["dy0"].T @ xd, (Lrows + P + 2) * U * (I["dy0"].abs().T @ xd.abs()))
    assert max(worst.values()) <= 1.0, worst
    assert not bool(I["dfeat"][::7].any()) and not bool(I["dy2"][::7].any()), "zero rows of dhead give zero rows of dfeat and dy2"


def test_no_gradient_crosses_a_crop_border(cuda):
    """dhead zero on crops 0 and 2 of three: dy2, da1 and dy0 of those crops are exactly 0, crop 1's are not"""
    prec, nS = "bf16", 3
    _sd, w = _weights(prec, cuda)
    x = _x_rows(nS, prec, cuda, 21)
    fwd = _forward_train(w, x, cuda)
    _grads, inter = _run_backward(w, x, fwd, _dhead(nS, w.c.ld_head, cuda, 22, zero_crops=(0, 2)), cuda)
    for k in ("dfeat", "dy2", "da1", "dy0"):
        v = inter[k].view(nS, 1024, 256)
        outer, inner = bool(v[0].any()) or bool(v[2].any()), float(v[1].abs().max())
        print(f"  {k}: anything non-zero on crops 0 / 2: {outer}; max |crop 1| = {inner:.3e}")
        assert not outer and inner > 0


# ---- 4. end to end --------------------------------------------------------------------------------------------------
def _trainer(dev, prec, sd=None, **kw):
    from classpose_amd.train import HeadTrainer
    sd = synth.make_state_dict(NCLS, None, depth=1, seed=43) if sd is None else sd
    return HeadTrainer(sd, device=dev, precision=prec, **kw), sd


def _device_grads(t, x, labs, tg):
    """one step's worth of gradients, nothing updated: the six neck tensors and both heads"""
    feat, head, o = t._loss(x, labs)
    seg = t._seg_loss(head, tg)
    t._neck_backward(*t._fwd, o, seg)
    got = {k: v.clone() for k, v in _grad_views(t.neck.grads).items()}
    got["Wc"], got["bc"] = ops.head_wgrad(o.dlogits, feat)
    got["Wf"], got["bf"] = ops.head_wgrad(seg.dlogits, feat)
    loss = float(o.ce.item()) + float(o.tversky.item()) + float(seg.flow.item()) + float(seg.cp.item())
    return got, loss


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_gradients_end_to_end(cuda, prec):
    nS = 3
    t, sd = _trainer(cuda, prec, feature_batch=1, train_flow_head=True, train_neck=True)
    x = _x_rows(nS, prec, cuda, 31)
    labs, tg = _labels(nS, NCLS, 7), _targets(nS, 8)
    got, loss = _device_grads(t, x, labs, tg.to(cuda))
    P = nr.params_from_state_dict(sd)
    net = None if prec == "fp32" else HD[prec]
    lab = torch.from_numpy(labs.astype(np.int64))
    r64 = nr.loss_and_grads(P, x.cpu(), lab, tg, NCLS, torch.float64, net)
    r32 = nr.loss_and_grads(P, x.cpu(), lab, tg, NCLS, torch.float32, net)
    print(f"{prec}: loss device {loss:.6f}, float64 {float(r64['loss']):.6f}, float32 {float(r32['loss']):.6f}")
    assert abs(loss - float(r64["loss"])) <= 1e-3 * abs(float(r64["loss"]))
    for k in nr.NECK + nr.HEADS:
        _check(k, got[k].cpu(), r32["grads"][k], r64["grads"][k])


# ---- 5. training ----------------------------------------------------------------------------------------------------
def _neck_operands(t):
    """copies of the six neck operands of the trainer's NetWeights as the kernels read them (the tensors that own the device memory
    the weight struct points at)"""
    c, keep = t.weights.c, t.weights.keep
    out = []
    for p in (c.neck0_w, c.neck_ln1_w, c.neck_ln1_b, c.neck2_w, c.neck_ln2_w, c.neck_ln2_b):
        owner = [k for k in keep if isinstance(k, torch.Tensor) and k.data_ptr() == p]
        assert len(owner) == 1
        out.append(owner[0].clone())
    return out


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_twenty_steps(cuda, prec):
    """The first epochs of the reference's schedule (ten warm-up steps from lr = 0, then constant): lr = 0 changes no neck operand
    bitwise; fp32: the loss curve and the final update of every tensor follow the float64 replay by the 6d rule; the loss summed over
    the last five steps is below that of the first five."""
    from classpose_amd.train import lr_schedule
    nS, steps = 1, 20
    t, sd = _trainer(cuda, prec, feature_batch=1, train_flow_head=True, train_neck=True)
    x = _x_rows(nS, prec, cuda, 33)
    labs, tg = _labels(nS, NCLS, 9), _targets(nS, 10)
    tgd = tg.to(cuda)
    lrs = [float(v) for v in lr_schedule(2e-4, steps)[:steps]]
    assert lrs[0] == 0.0 and lrs[-1] == 2e-4
    ops0 = _neck_operands(t)
    P0 = t.neck.params.clone()
    head0 = t.evaluate(x, labs, flow_targets=tgd, return_head=True)["head"].clone()
    losses = []
    for k, lr in enumerate(lrs):
        losses.append(t.step(x, labs, lr, flow_targets=tgd)["loss"])
        if k == 0:
            same_p = torch.equal(t.neck.params.view(torch.int32), P0.view(torch.int32))
            same_o = all(torch.equal(a, b) for a, b in zip(ops0, _neck_operands(t)))
            same_h = torch.equal(t.evaluate(x, labs, flow_targets=tgd, return_head=True)["head"], head0)
            print(f"{prec}: after lr = 0 masters unchanged {same_p}, operands unchanged {same_o}, head unchanged {same_h}")
            assert same_p and same_o and same_h
    losses = np.array(losses)
    print(f"{prec}: loss step 1 = {losses[0]:.6f}, step {steps} = {losses[-1]:.6f}; first five {losses[:5].sum():.6f}, last five {losses[-5:].sum():.6f}")
    assert not torch.equal(t.neck.params, P0) and any(not torch.equal(a, b) for a, b in zip(ops0, _neck_operands(t)))
    if prec == "fp32":
        P = nr.params_from_state_dict(sd)
        lab = torch.from_numpy(labs.astype(np.int64))
        l64, p64 = nr.replay(P, x.cpu(), lab, tg, NCLS, lrs, torch.float64, None, t.weight_decay)
        l32, p32 = nr.replay(P, x.cpu(), lab, tg, NCLS, lrs, torch.float32, None, t.weight_decay)
        floor = steps * FLOOR
        _check("loss curve", losses, l32, l64, floor)
        fin = {k: t.neck.view(i).cpu() for i, k in enumerate(nr.NECK)}
        fin.update(Wc=t.w.cpu(), bc=t.b.cpu(), Wf=t.flow.w.cpu(), bf=t.flow.b.cpu())
        for k in nr.NECK + nr.HEADS:
            _check(f"final update of {k}", fin[k].double() - P[k].double(), p32[k].double() - P[k].double(), p64[k] - P[k].double(), floor)
        assert l64[-5:].sum() < l64[:5].sum(), "the chosen inputs are meant to train"
    assert losses[-5:].sum() < losses[:5].sum()


# ---- 6. off means off -----------------------------------------------------------------------------------------------
def _crops(n, seed0=300):
    ims, labs, inst = [], [], []
    for k in range(n):
        x0, y0 = 256 * (k % 4), 256 * (k // 4)
        ims.append(synth.render_region(seed0, x0, y0, 256, 256))
        lab = synth.analytic_fields(seed0, x0, y0, 256, 256, NCLS)[2].argmax(0).astype(np.int16)
        lab[(40 + 11 * k) % 200:][:24] = -100
        labs.append(lab)
        inst.append(fr.disc_crop(50 + k))
    return np.stack(ims), np.stack(labs), np.stack(inst)


def test_train_neck_false_is_the_trainer_as_before(cuda):
    from classpose_amd.train import HeadTrainer
    ims, labs, _inst = _crops(2)
    sd = synth.make_state_dict(NCLS, None, depth=1, seed=44)
    a = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=2)
    b = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=2, train_neck=False)
    assert b.neck is None
    feat = a.features(ims)
    assert torch.equal(feat, b.features(ims))
    for lr in (0.0, 1e-3, 2e-3):
        ra, rb = a.step(feat, labs, lr), b.step(feat, labs, lr)
        print(f"  lr {lr}: {ra} | {rb}")
        assert ra == rb
    assert a.step(ims, labs, 2e-3) == b.step(ims, labs, 2e-3)          # from pixels too
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) == set(sd) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(torch.equal(sb[k], sd[k]) for k in sd if k.startswith("encoder.neck.")), "no neck key changes when the neck does not train"
    from classpose_amd.train_unet import UNetHeadTrainer
    with pytest.raises(NotImplementedError, match="neck"):
        UNetHeadTrainer(sd, device=cuda, feature_transformation_structure=[16, 24], train_neck=True)


# ---- 7. the checkpoint ----------------------------------------------------------------------------------------------
def test_the_saved_checkpoint_loads_into_net_weights(cuda, tmp_path):
    from classpose_amd import augment
    from classpose_amd.train import NECK_KEYS
    ims, labs, inst = _crops(4)
    tg = torch.stack(augment.flow_targets_of(list(inst), cuda))
    t, sd = _trainer(cuda, "bf16", feature_batch=4, train_flow_head=True, train_neck=True)
    x = t.backbone_features(ims)
    assert x.shape == (4 * 1024, 1024) and x.dtype == torch.bfloat16
    r_rows = t.evaluate(x, labs, flow_targets=tg)
    r_pix = t.evaluate(ims, labs, flow_targets=tg)
    assert r_rows == r_pix, "cached backbone rows and pixels give the same losses"
    for lr in (1e-3, 2e-3, 2e-3):
        t.step(x, labs, lr, flow_targets=tg)
    t.save(tmp_path / "neck.pt")
    ck = torch.load(tmp_path / "neck.pt", map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and all(ck[k].shape == sd[k].shape and ck[k].dtype == sd[k].dtype for k in sd)
    changed = {k for k in sd if not torch.equal(ck[k], sd[k])}
    print(f"changed keys: {sorted(changed)}")
    assert changed == set(NECK_KEYS) | {"out.weight", "out.bias", "out_class.weight", "out_class.bias"}
    t.save(tmp_path / "only.pt", save_only_trainable_params=True)
    assert set(torch.load(tmp_path / "only.pt", weights_only=True)) == changed
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    ev = t.evaluate(ims, labs, flow_targets=tg, return_head=True)["head"].clone()
    L = _lib.lib()
    ws = torch.empty(L.cpx_net_workspace_bytes(4, w.c.dtype), dtype=torch.uint8, device=cuda)
    head = torch.empty((4 * 1024, w.c.ld_head), dtype=torch.float32, device=cuda)
    _lib.check(L.cpx_net_forward(C.byref(w.c), ptr(t._patches(ims)), 4, ptr(head), ptr(ws), ws.numel(),
                                 torch.cuda.current_stream(cuda).cuda_stream), "net_forward")
    same = torch.equal(head[:, :192 + NCLS * 64], ev[:, :192 + NCLS * 64])
    print(f"cpx_net_forward on the saved checkpoint equals the trainer's head bitwise: {same}")
    assert same
    # reloading into a trainer: the same masters
    r, _ = _trainer(cuda, "bf16", sd=ck, feature_batch=4, train_flow_head=True, train_neck=True)
    assert torch.equal(r.neck.params, t.neck.params)


# ---- 8. the command line --------------------------------------------------------------------------------------------
def test_cli_train_neck_in_a_child_process(cuda, tmp_path):
    sd = synth.make_state_dict(1, None, depth=1, seed=45)               # a plain backbone: the CLI initialises the class head
    torch.save(sd, tmp_path / "backbone.pt")
    d = tmp_path / "data"
    d.mkdir()
    imgs, labs = np.empty(2, dtype=object), np.empty(2, dtype=object)
    for k, (h, wd) in enumerate([(300, 280), (256, 256)]):
        inst = np.zeros((h, wd), np.int32)
        inst[:256, :256] = fr.disc_crop(70 + k)
        imgs[k] = synth.render_region(300, 64 * k, 32 * k, wd, h)
        labs[k] = np.stack([inst, np.where(inst > 0, 1 + inst % 2, 0).astype(np.int32)], -1)
    np.save(d / "images.npy", imgs, allow_pickle=True)
    np.save(d / "labels.npy", labs, allow_pickle=True)
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--data_path", str(d),
           "--train_fraction", "1", "--train_neck", "--train_flow_head", "--pretrained_model", str(tmp_path / "backbone.pt"), "--nclasses", "3",
           "--n_epochs", "2", "--batch_size", "2", "--learning_rate", "1e-3", "--save_path", str(tmp_path), "--model_name", "m",
           "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    assert "backbone rows" in r.stdout + r.stderr, "the cache holds backbone rows when the neck trains"
    ck = torch.load(out, map_location="cpu", weights_only=True)
    neck = [k for k in sd if k.startswith("encoder.neck.")]
    print(f"neck keys: {neck}")
    assert len(neck) == 6 and all(ck[k].shape == sd[k].shape and not torch.equal(ck[k], sd[k]) for k in neck)
    assert not torch.equal(ck["out.weight"], sd["out.weight"])
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    assert w.ncls == 3 and w.c.n_unet_ops == 0
