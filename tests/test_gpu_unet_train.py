"""Device training of the UNet semantic head (csrc/cpx_train_unet.hip -> ops -> classpose_amd.train_unet -> the train_head CLI).

Backward, op by op: every op's dW, db and the gradient tensors are compared with float64 autograd of F.conv2d /
F.conv_transpose2d on the device's OWN tensors -- the stored input X and output Y of the forward workspace, the incoming gradient dY
the backward left in its workspace (after the ReLU mask) and the weights of the state dict rounded to the dtype.
  dW, db   |got - exact| <= (L + P + 2) u sum|dY||X|, u = 2^-24: L = cpx_unet_wgrad_slab_rows() rows go through one MFMA
           accumulator chain, P = ceil(rows / L) slab partials are added (in float64, rounded once) -- the bound of
           test_head_wgrad_every_element.
  dX       the gradient tensor of op t's output is mask_t * sum over t's consumers j of col2im_j(dY_j W_j).  An element of dY_j W_j is
           a float32 dot product over Npad_j terms in the GEMM's order, at most 9 taps of it and one earlier consumer's contribution
           are then added one by one: |got - exact| <= sum_j (Npad_j + taps_j + 2) u sum|dY_j||W_j|.  Where the mask (stored Y > 0)
           is off the gradient is exactly 0; padded channels and padding rows are exactly 0.
End to end and training: the project's rule for a quantity q with err(x) = ||x - q64||_2 / ||q64||_2:
    err(device) <= max(4 * err(torch CPU float32), 2^-20),
q64 from the float64 restatement tests/unet_train_reference.py (pinned on the reference by tests/test_unet_train_host.py) on the
same features and labels; for bf16 / fp16 both replays round the weights and every op's output to the dtype, straight-through.
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

import train_reference as tr
import unet_train_reference as ur
from classpose_amd import _lib, engine, ops, synth, train_unet
from classpose_amd._lib import ptr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
FLOOR = 2.0 ** -20
HD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_W = {}


def _weights(ncls, fts, prec, dev):
    key = (ncls, tuple(fts), prec)
    if key not in _W:
        sd = synth.make_state_dict(ncls, list(fts), depth=1, seed=21 + len(fts))
        _W[key] = (sd, engine.NetWeights.from_state_dict(sd, prec, dev))
    return _W[key]


def _labels(n, ncls, seed):
    """blocky class maps (n, 256, 256) int16 with a -100 band, a -100 box and scattered -100 pixels; every class present"""
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


def _nchw(tok, nS, h):
    return tok.reshape(nS, h, h, -1).permute(0, 3, 1, 2).contiguous()


def _tokens(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def _check(name, dev_val, f32_val, f64_val, floor=FLOOR):
    e_dev, e_cpu = tr.rel_l2(dev_val, f64_val), tr.rel_l2(f32_val, f64_val)
    tol = max(4 * e_cpu, floor)
    print(f"  {name}: err(device) = {e_dev:.3e}, err(torch CPU float32) = {e_cpu:.3e}, tolerance = {tol:.3e}")
    assert e_dev <= tol, (name, e_dev, e_cpu, tol)
    return e_dev, e_cpu


# ---- backward, op by op ---------------------------------------------------------------------------------------------------
def _run_backward(w, feat, dl, nS, dev):
    """forward on a 0xFF workspace, then the backward with its workspace and the gradient buffer poisoned; CPU copies"""
    L = _lib.lib()
    c = w.c
    n = c.n_unet_ops
    fb = L.cpx_unet_workspace_bytes(c.unet_ops, n, nS, c.dtype)
    fws = torch.full((fb,), 0xFF, dtype=torch.uint8, device=dev)
    head = torch.zeros((nS * 1024, c.ld_head), dtype=torch.float32, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(L.cpx_unet_head_forward(c.unet_ops, n, ptr(feat), nS, ptr(head), c.ld_head, 192, c.dtype, ptr(fws), fb, st), "forward")
    bb = L.cpx_unet_backward_workspace_bytes(c.unet_ops, n, nS, c.dtype)
    assert bb > 0
    bws = torch.full((bb,), 0xFF, dtype=torch.uint8, device=dev)
    total = L.cpx_unet_param_layout(c.unet_ops, n, None, None, None, None)
    grads = torch.full((total,), float("nan"), dtype=torch.float32, device=dev)
    ops.unet_head_backward(w, feat, fws, dl, grads, bws)
    torch.cuda.synchronize(dev)
    return fws, bws, grads


def check_backward(fts, prec, nS, dev, ncls=3):
    sd, w = _weights(ncls, fts, prec, dev)
    hd, c = HD[prec], w.c
    n, out_ch = c.n_unet_ops, ncls * 64
    plan = train_unet.unet_plan(fts, out_ch)
    assert n == len(plan)
    g = torch.Generator(device=dev).manual_seed(nS * 13 + len(fts))
    feat = torch.randn(nS * 1024, 256, generator=g, device=dev).to(hd)
    dl = torch.randn(nS * 1024, out_ch, generator=g, device=dev) * torch.logspace(-3, 0, out_ch, device=dev)[None]
    dl[::7] = 0                                                        # rows of pixels without annotation
    fws, bws, grads = _run_backward(w, feat, dl, nS, dev)
    # bitwise reproducible, whatever the workspaces held
    _f2, bws2, grads2 = _run_backward(w, feat, dl, nS, dev)
    g_off, g_ld = (C.c_size_t * n)(), (C.c_int * n)()
    _lib.check(_lib.lib().cpx_unet_grad_layout(c.unet_ops, n, nS, c.dtype, g_off, g_ld), "grad_layout")
    g_end = g_off[n - 1]                                               # the last op has no gradient tensor: the tensors end where its slot would start
    assert torch.equal(grads.view(torch.int32), grads2.view(torch.int32)), "two backward passes differ"
    assert torch.equal(bws[:g_end], bws2[:g_end]), "two backward passes leave different gradient tensors"
    assert bool(torch.isfinite(grads).all())
    # padded rows / columns of every operand and bias: exactly 0 (pack o unpack keeps exactly the valid entries)
    gsd = train_unet.unpack_params(grads, fts, out_ch)
    assert torch.equal(train_unet.pack_params(gsd, fts, out_ch), grads.cpu()), "a padded gradient entry is not 0 (or transposed-conv bias copies differ)"
    a_off, a_ld = (C.c_size_t * n)(), (C.c_int * n)()
    with _lib.use_debug_library() as D:
        _lib.check(D.cpx_unet_head_layout(c.unet_ops, n, nS, c.dtype, a_off, a_ld), "head_layout")
    es = torch.finfo(hd).bits // 8
    opsl = [c.unet_ops[i] for i in range(n)]
    Lrows = _lib.lib().cpx_unet_wgrad_slab_rows()

    def out_hw(o):
        return o.h if o.kind == 0 else (o.h // 2 if o.kind == 1 else o.h * 2)

    Y, G = {}, {}                                                      # op index -> [rows][padded channels] float64 on the CPU
    for i, o in enumerate(opsl[:-1]):
        rows = nS * out_hw(o) ** 2
        rp = (rows + 127) // 128 * 128
        Y[i] = fws[a_off[i]:a_off[i] + rp * a_ld[i] * es].view(hd).reshape(rp, a_ld[i])[:rows, :o.cout].double().cpu()
        gt = bws[g_off[i]:g_off[i] + rp * g_ld[i] * 4].view(torch.float32).reshape(rp, g_ld[i])
        real = plan[i][4]
        assert not bool(gt[rows:].any()) and not bool(gt[:, real:].any()), f"op {i}: gradient padding not 0"
        G[i] = gt[:rows, :real].double().cpu()
    G[n - 1] = dl.double().cpu()
    featd = feat.double().cpu()
    contrib, cbound = {}, {}
    worst_w = worst_b = worst_x = 0.0
    for i, ((key, kind, cin_a, cin_b, cout), o) in enumerate(zip(plan, opsl)):
        h, ho = o.h, out_hw(o)
        srcs = [(o.src_a, cin_a)] + ([(o.src_b, cin_b)] if o.src_b >= 0 else [])
        X = torch.cat([_nchw(featd if t == 0 else Y[t - 1][:, :cr], nS, h) for t, cr in srcs], 1)
        dY = _nchw(G[i], nS, ho)
        wt, b = sd[key + ".weight"].to(hd).double(), sd[key + ".bias"].to(hd).double()

        def grads_of(x, wv, dy):
            x, wv, bv = x.clone().requires_grad_(True), wv.clone().requires_grad_(True), b.clone().requires_grad_(True)
            y = F.conv2d(x, wv, bv, padding=1) if kind == 0 else F.conv2d(x, wv, bv, stride=2) if kind == 1 \
                else F.conv_transpose2d(x, wv, bv, stride=2)
            y.backward(dy)
            return wv.grad, bv.grad, x.grad

        dW, db, dX = grads_of(X, wt, dY)
        mW, mb, mX = grads_of(X.abs(), wt.abs(), dY.abs())
        rows_gemm = nS * (h * h if kind == 2 else ho * ho)
        P = (rows_gemm + Lrows - 1) // Lrows
        bw, bb_ = (Lrows + P + 2) * U * mW, (Lrows + P + 2) * U * mb
        ew = (gsd[key + ".weight"].double() - dW).abs()
        eb = (gsd[key + ".bias"].double() - db).abs()
        what = f"{prec} fts {fts} nS={nS} op {i} {key}"
        assert bool((ew <= bw).all()), f"{what}: dW off by {float((ew / bw.clamp_min(1e-300)).max()):.3f} bounds"
        assert bool((eb <= bb_).all()), f"{what}: db off by {float((eb / bb_.clamp_min(1e-300)).max()):.3f} bounds"
        worst_w = max(worst_w, float((ew / bw.clamp_min(1e-300)).max()))
        worst_b = max(worst_b, float((eb / bb_.clamp_min(1e-300)).max()))
        n_pad = train_unet.param_layout(fts, out_ch)[1][i][2]
        taps = (9, 4, 1)[kind]
        c0 = 0
        for t, cr in srcs:
            if t > 0:
                contrib[t] = contrib.get(t, 0) + _tokens(dX[:, c0:c0 + cr])
                cbound[t] = cbound.get(t, 0) + (n_pad + taps + 2) * U * _tokens(mX[:, c0:c0 + cr])
            c0 += cr
    for t in range(1, n):                                              # tensor t = op t - 1's output
        i = t - 1
        exp, bd = contrib[t], cbound[t]
        real = plan[i][4]
        if opsl[i].relu:
            on = Y[i][:, :real] > 0
            assert not bool(G[i][~on].any()), f"op {i}: gradient not 0 where the stored output is <= 0"
            exp = exp * on
        ex = (G[i] - exp).abs()
        what = f"{prec} fts {fts} nS={nS} gradient of op {i} {plan[i][0]}"
        assert bool((ex <= bd).all()), f"{what}: off by {float((ex / bd.clamp_min(1e-300)).max()):.3f} bounds"
        worst_x = max(worst_x, float((ex / bd.clamp_min(1e-300)).max()))
    return worst_w, worst_b, worst_x


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("fts", [[64, 128], [20, 36], [12, 20, 36, 68]], ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("nS", [1, 3])
def test_backward_every_element(cuda, prec, fts, nS):
    ww, wb, wx = check_backward(fts, prec, nS, cuda)
    print(f"unet backward {prec} fts {fts} nS={nS}: worst err/bound dW {ww:.3f}, db {wb:.3f}, dX {wx:.3f}")


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _flat(d, keys):
    return torch.cat([d[k].double().reshape(-1) for k in keys])


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_parameter_gradients_end_to_end(cuda, prec):
    """loss -> dlogits -> every parameter gradient against float64 autograd of the restatement (bf16 / fp16: the straight-through
    replay) on the same features and labels; the yardstick is the same replay in torch CPU float32"""
    fts, ncls, nS = [20, 36], 3, 2
    hd = HD[prec]
    sd = synth.make_state_dict(ncls, fts, depth=1, seed=31)
    t = train_unet.UNetHeadTrainer(sd, device=cuda, precision=prec, feature_batch=2)
    g = torch.Generator().manual_seed(9)
    feat = torch.randn(nS * 1024, 256, generator=g).to(hd)
    labs = _labels(nS, ncls, 5)
    fd, _head, o = t._loss(feat.to(cuda), labs)
    got = train_unet.unpack_params(t.backward(fd, o.dlogits), fts, ncls * 64)
    x = _nchw(feat.double(), nS, 32)
    ste = None if prec == "fp32" else hd
    lab = torch.from_numpy(labs.astype(np.int64))
    r64 = ur.loss_and_grads(sd, x, lab, fts, ncls, dtype=torch.float64, ste=ste)
    r32 = ur.loss_and_grads(sd, x, lab, fts, ncls, dtype=torch.float32, ste=ste)
    print(f"{prec}: loss device {float(o.ce.item()) + float(o.tversky.item()):.6f}, float64 {float(r64['loss']):.6f}, float32 {float(r32['loss']):.6f}")
    keys = ur.unet_keys(fts)
    worst = (0.0, 0.0)
    for k in keys:
        worst = max(worst, _check(k, got[k], r32["grads"][k], r64["grads"][k]))
    _check("all parameters", _flat(got, keys), _flat(r32["grads"], keys), _flat(r64["grads"], keys))
    print(f"{prec}: worst per-parameter err(device) {worst[0]:.3e} (torch CPU float32 there: {worst[1]:.3e})")


# ---- training -----------------------------------------------------------------------------------------------------------------
def _replay(sd, x, lab, fts, ncls, lrs, dtype, ste, weight_decay):
    keys = ur.unet_keys(fts)
    p = {k: sd[k].to(dtype).clone() for k in keys}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v = {k: torch.zeros_like(v_) for k, v_ in p.items()}
    losses = []
    for step, lr in enumerate(lrs, 1):
        r = ur.loss_and_grads(p, x, lab, fts, ncls, dtype=dtype, ste=ste)
        losses.append(float(r["loss"]))
        for k in keys:
            tr.adamw_step(p[k], r["grads"][k].to(dtype), m[k], v[k], step, lr, weight_decay=weight_decay)
    return np.array(losses), p


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_twenty_steps(cuda, prec):
    """fp32: the loss curve and the final update follow the float64 replay by the 6d rule; bf16: the loss decreases.  Both: lr = 0
    changes nothing bitwise, and the padded parameters are exactly 0 afterwards.
    The learning rates (warm-up from 0 to 2e-4, the reference's default is 5e-5) keep the 20 steps where float32 can be a
    yardstick at all: at 2e-3 this batch is fitted to a loss of 4e-4 within 20 steps, the softmax saturates and the float32 gradient
    of ANY implementation loses three digits (torch CPU float32 against float64 at the same parameters: 3e-7 at step 1, 3e-4 at
    step 20; the device: 5e-7 and 1e-4).  A trajectory is also discontinuous where a ReLU input crosses 0: one element whose mask
    differs between two float32 implementations moves the final update by 1e-4 .. 1e-3 (seen at 2e-4 in the torch CPU float32
    replay, step 11, and at 2e-3 in the device run), which is what the yardstick term of the rule absorbs."""
    fts, ncls, nS, steps = [12, 20], 3, 1, 20
    hd = HD[prec]
    sd = synth.make_state_dict(ncls, fts, depth=1, seed=32)
    t = train_unet.UNetHeadTrainer(sd, device=cuda, precision=prec, feature_batch=1)
    g = torch.Generator().manual_seed(10)
    feat = torch.randn(nS * 1024, 256, generator=g).to(hd)
    labs = _labels(nS, ncls, 6)
    fd = feat.to(cuda)
    lrs = [float(v) for v in np.minimum(np.linspace(0, 4e-4, 10), 2e-4)] + [2e-4] * 10
    P0 = t.params.clone()
    head0 = t.evaluate(fd, labs, return_head=True)["head"].clone()
    dev_losses = []
    for k, lr in enumerate(lrs):
        dev_losses.append(t.step(fd, labs, lr)["loss"])
        if k == 0:
            assert lr == 0 and torch.equal(t.params.view(torch.int32), P0.view(torch.int32)), "lr = 0 changed a parameter"
            assert torch.equal(t.evaluate(fd, labs, return_head=True)["head"], head0), "lr = 0 changed an operand"
    dev_losses = np.array(dev_losses)
    out_ch = ncls * 64
    fin = train_unet.unpack_params(t.params, fts, out_ch)
    assert torch.equal(train_unet.pack_params(fin, fts, out_ch), t.params.cpu()), "a padded parameter moved off 0"
    assert not torch.equal(t.params, P0)
    print(f"{prec}: loss step 1 = {dev_losses[0]:.6f}, step {steps} = {dev_losses[-1]:.6f}")
    if prec != "fp32":
        assert dev_losses[-1] < dev_losses[0]
        return
    x, lab = _nchw(feat.double(), nS, 32), torch.from_numpy(labs.astype(np.int64))
    l64, p64 = _replay(sd, x, lab, fts, ncls, lrs, torch.float64, None, t.weight_decay)
    l32, p32 = _replay(sd, x, lab, fts, ncls, lrs, torch.float32, None, t.weight_decay)
    keys = ur.unet_keys(fts)
    p0 = _flat({k: sd[k] for k in keys}, keys)
    floor = steps * FLOOR
    _check("loss curve", dev_losses, l32, l64, floor)
    _check("final update of every parameter", _flat(fin, keys) - p0, _flat(p32, keys) - p0, _flat(p64, keys) - p0, floor)
    assert l64[-1] < l64[0], "the chosen inputs are meant to train"
    assert dev_losses[-1] < dev_losses[0]


# ---- the trainer in its surroundings ------------------------------------------------------------------------------------------
def _synthetic_set(n, ncls, seed0=300):
    ims, labs = [], []
    for k in range(n):
        x0, y0 = 256 * (k % 4), 256 * (k // 4)
        ims.append(synth.render_region(seed0, x0, y0, 256, 256))
        lab = synth.analytic_fields(seed0, x0, y0, 256, 256, ncls)[2].argmax(0).astype(np.int16)
        lab[(40 + 11 * k) % 200:][:24] = -100
        labs.append(lab)
    return np.stack(ims), np.stack(labs)


def test_train_class_head_and_the_saved_checkpoint(cuda, tmp_path):
    """train_class_head with a UNetHeadTrainer: cached == uncached bitwise; the saved checkpoint is a reference-layout state dict
    whose inference forward computes, bit for bit, the class columns the trainer evaluates; ClassposeModel loads it"""
    from classpose_amd import models
    from classpose_amd.train import make_trainer, train_class_head
    ncls, fts = 3, [16, 24]
    sd = synth.make_state_dict(ncls, fts, depth=1, seed=33)
    ims, labs = _synthetic_set(8, ncls)
    runs = {}
    for cached in (True, False):
        t = make_trainer(sd, device=cuda, precision="bf16", feature_batch=4)
        assert isinstance(t, train_unet.UNetHeadTrainer)
        path, tl, vl = train_class_head(t, ims[:6], labs[:6], ims[6:], labs[6:], batch_size=4, n_epochs=3, learning_rate=2e-3,
                                        cache_features=cached, save_path=tmp_path / f"c{int(cached)}", model_name="head")
        runs[cached] = (t, path, tl, vl)
    (ta, pa, tla, vla), (tb, _pb, tlb, vlb) = runs[True], runs[False]
    assert torch.equal(ta.params.view(torch.int32), tb.params.view(torch.int32))
    assert np.array_equal(tla, tlb) and np.array_equal(vla, vlb) and np.all(np.isfinite(tla)) and np.all(vla > 0)
    ck = torch.load(pa, map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and all(ck[k].shape == sd[k].shape for k in sd)
    assert all(torch.equal(ck[k], sd[k]) for k in sd if not k.startswith("out_class."))
    assert any(not torch.equal(ck[k], sd[k]) for k in sd if k.startswith("out_class."))
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    assert w.c.n_unet_ops == len(train_unet.unet_plan(fts, ncls * 64)) and w.ncls == ncls
    four = ims[:4]
    ev = ta.evaluate(four, labs[:4], return_head=True)
    patches = ta._patches(four)
    L = _lib.lib()
    nb = L.cpx_net_workspace_bytes(4, w.c.dtype) + L.cpx_unet_workspace_bytes(w.c.unet_ops, w.c.n_unet_ops, 4, w.c.dtype)
    ws = torch.empty(nb, dtype=torch.uint8, device=cuda)
    head = torch.empty((4 * 1024, w.c.ld_head), dtype=torch.float32, device=cuda)
    _lib.check(L.cpx_net_forward(C.byref(w.c), ptr(patches), 4, ptr(head), ptr(ws), nb, torch.cuda.current_stream(cuda).cuda_stream),
               "net_forward")
    assert torch.equal(head[:, 192:192 + ncls * 64], ev["head"][:, 192:192 + ncls * 64])
    assert torch.equal(head[:, :192], ev["head"][:, :192])            # the frozen flow head is untouched
    m = models.ClassposeModel(pretrained_model=str(pa), device=cuda, precision="bf16", max_batch_tiles=2)
    assert m.nclasses == ncls
    _masks, flows, class_masks, _styles = m.eval(ims[0])
    assert class_masks.shape == (256, 256) and flows[3].shape == (ncls, 256, 256)
    ta.save(tmp_path / "only.pt", save_only_trainable_params=True)
    assert set(torch.load(tmp_path / "only.pt", weights_only=True)) == {k for k in sd if k.startswith("out_class.")}


@pytest.mark.parametrize("fresh", [False, True], ids=["unet checkpoint", "fresh head"])
def test_cli_trains_in_a_child_process(cuda, tmp_path, fresh):
    from classpose_amd import models
    ncls = 3
    sd = synth.make_state_dict(1, None, depth=1, seed=34) if fresh else synth.make_state_dict(ncls, [16, 24], depth=1, seed=34)
    torch.save(sd, tmp_path / "ck.pt")
    ims, labs = _synthetic_set(8, ncls)
    np.save(tmp_path / "X.npy", ims)
    np.save(tmp_path / "Y.npy", labs)
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--images", str(tmp_path / "X.npy"),
           "--labels", str(tmp_path / "Y.npy"), "--pretrained_model", str(tmp_path / "ck.pt"), "--n_epochs", "2", "--batch_size", "4",
           "--learning_rate", "1e-3", "--save_path", str(tmp_path), "--model_name", "m", "--device", "cuda:0"]
    if fresh:
        cmd += ["--feature_transformation_structure", "16", "24", "--nclasses", str(ncls)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert engine.NetWeights.infer_structure(ck)[:2] == ([16, 24], ncls)
    m = models.ClassposeModel(pretrained_model=str(out), device=cuda, precision="bf16", max_batch_tiles=2)
    assert m.nclasses == ncls
