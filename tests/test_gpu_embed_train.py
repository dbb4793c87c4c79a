"""Training the patch embedding and the position table: cpx_blocks_backward_in, cpx_embed_backward (csrc/cpx_train_embed.hip),
train.EmbedParams / HeadTrainer(train_embed=True) and train_head --train_embed.  The network is synth.make_state_dict(3, None, depth=2) and
the helpers are those of tests/test_gpu_block_train.py.

Crop counts: nS = 1 (the smallest grid), 3 (odd: the slabs of two crops leave a remainder, dpos has three terms), and one on each side
of every change of the bf16 kernel's row split S = 8 min(nS, 4): 1 | 2 | 3 | 4 | 5 (S = 8, 16, 24, 32, 32; 128 rows per split up to 4
crops, 32 nS from 5 on), and 8, the largest count at which integer sums stay below 2^24.

Bounds, all derived and none measured:
  * integer dx and p in {-2 .. 2} (exact in bf16), rows <= 8 * 1024: every partial sum is an integer below 2^24, so dW, db and dpos are
    torch.equal to the CPU result in both gradient modes.
  * random operands, bf16 mode: only the additions round: |dW - exact| <= (L + 2) 2^-24 sum |r(dx)||p|, L = rows, exact in float64 on the
    rounded operands.
  * db, dpos (float64 sums rounded once): |got - exact| <= 2^-24 |exact| + 2^-40 sum |dx|.
  * float32 mode and everything end to end: err(device) <= max(4 err(torch CPU float32), 2^-20) in relative L2 against the float64
    reference (tests/embed_train_reference.py); for the bf16 gradient modes the CPU float32 comparator carries the same roundings.  The
    comparator is never the device.
Every output and workspace is poisoned (0xFF bytes, NaN) before the call that fills it; every test prints what it observed before it
asserts (run with -s)."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import block_train_reference as br
import embed_train_reference as er
import flow_train_reference as fr
import neck_train_reference as nr
import test_gpu_block_train as bt
from classpose_amd import _lib, engine, ops, synth
from classpose_amd._lib import ptr
from test_gpu_block_train import DEPTH, FLOOR, HD, NCLS, ROOT, _check, _forward_train, _labels, _neck_views, _patches, _rounded_params, _rows_in, _targets

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EINVAL = -22
BF, F32 = torch.bfloat16, torch.float32
CROPS = [1, 2, 3, 4, 5, 8]
MODES = {"fp32": (F32, F32), "bf16": (BF, F32), "bf16+attn": (BF, BF)}       # (grad_dtype, attn_grad_dtype) of the blocks' backward


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _views(grads):
    _n, off = ops.embed_grad_layout()
    return {k: grads[o:o + int(np.prod(s))].view(s) for k, o, s in zip(ops.EMBED_GRAD_NAMES, off, ops.EMBED_GRAD_SHAPES)}


# ---- 1. cpx_blocks_backward_in ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS", [1, 3])
@pytest.mark.parametrize("mode", list(MODES))
def test_dx_in_is_record_zero_of_dx_all(cuda, mode, nS):
    gd, ad = MODES[mode]
    sd, w = bt._weights("bf16", cuda)
    x = _rows_in(w, _patches(nS, "bf16", cuda, 40 + nS), nS, DEPTH, cuda)
    fwd = _forward_train(w, x, DEPTH, cuda)
    dy0 = torch.randn(nS * 1024, 256, generator=torch.Generator(device=cuda).manual_seed(41), device=cuda)
    params = _rounded_params(sd, "bf16", cuda)
    n, _o = ops.block_grad_layout()
    out = []
    for with_in in (False, True):
        ws = ops.blocks_backward_workspace(nS, w.c.dtype, cuda, gd, ad)
        ws.fill_(0xFF)
        grads = torch.full((DEPTH * n,), float("nan"), dtype=F32, device=cuda)
        dx_all = torch.full((DEPTH + 1, nS * 1024, 1024), float("nan"), dtype=F32, device=cuda)
        dx_in = torch.full((nS * 1024, 1024), float("nan"), dtype=F32, device=cuda) if with_in else None
        ops.blocks_backward(w, params, fwd, dy0, grads, ws, dx_all, grad_dtype=gd, attn_grad_dtype=ad, dx_in=dx_in)
        out.append((grads, dx_all, dx_in))
    only = torch.full((nS * 1024, 1024), float("nan"), dtype=F32, device=cuda)          # dx_in without dx_all
    ws = ops.blocks_backward_workspace(nS, w.c.dtype, cuda, gd, ad)
    ws.fill_(0xFF)
    g3 = ops.blocks_backward(w, params, fwd, dy0, None, ws, None, grad_dtype=gd, attn_grad_dtype=ad, dx_in=only)
    torch.cuda.synchronize(cuda)
    (g0, d0, _none), (g1, d1, din) = out
    i32 = lambda t: t.view(torch.int32)
    same_g = torch.equal(i32(g0), i32(g1)) and torch.equal(i32(g0), i32(g3))
    same_all = torch.equal(i32(d0), i32(d1))
    rec0 = torch.equal(i32(din), i32(d1[0])) and torch.equal(i32(only), i32(d1[0]))
    finite = bool(torch.isfinite(din).all()) and float(din.abs().max()) > 0
    print(f"{mode} nS={nS}: grads bitwise those of the call without dx_in {same_g}; dx_all unchanged {same_all}; dx_in == dx_all[0] {rec0}; "
          f"finite and non-zero {finite}")
    assert same_g and same_all and rec0 and finite


# ---- 2. cpx_embed_backward ----------------------------------------------------------------------------------------------
_CASE = {}


def _case(nS, kind):
    """(dx float32, p float32 holding bf16 values, and the float64 results) on the CPU, computed once per crop count"""
    if (nS, kind) not in _CASE:
        g = torch.Generator().manual_seed(1000 + 10 * nS + (kind == "int"))
        rows = nS * 1024
        if kind == "int":
            dx, p = torch.randint(-2, 3, (rows, 1024), generator=g).float(), torch.randint(-2, 3, (rows, 192), generator=g).float()
        else:
            dx = torch.randn(rows, 1024, generator=g) * torch.logspace(-3, 0, 1024)[None]
            dx[::7] = 0
            p = torch.randn(rows, 192, generator=g).to(BF).float()
        d64, p64 = dx.double(), p.double()
        r64 = dx.to(BF).double()
        c = {"dx": dx, "p": p, "W64": d64.T @ p64, "W64r": r64.T @ p64, "Wabs": r64.abs().T @ p64.abs(), "W32": dx.T @ p,
             "b64": d64.sum(0), "babs": d64.abs().sum(0), "pos64": d64.view(nS, 1024, 1024).sum(0), "posabs": d64.abs().view(nS, 1024, 1024).sum(0)}
        _CASE[(nS, kind)] = c
    return _CASE[(nS, kind)]


def _embed_run(p, dx, grad_dtype, fill=0xFF):
    dev = p.device
    ws = ops.embed_backward_workspace(p.shape[0] // 1024, ops._DT[p.dtype], dev, grad_dtype)
    ws.fill_(fill)
    grads = torch.full((ops.embed_grad_layout()[0],), float("nan"), dtype=F32, device=dev)
    ops.embed_backward(p, dx, grads, ws, grad_dtype=grad_dtype)
    torch.cuda.synchronize(dev)
    return grads


@pytest.mark.parametrize("nS", CROPS)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_embed_backward_exact_on_integers(cuda, mode, nS):
    c = _case(nS, "int")
    assert float(c["Wabs"].max()) < 2 ** 24 and float(c["babs"].max()) < 2 ** 24
    a = _embed_run(c["p"].to(cuda).to(BF), c["dx"].to(cuda), MODES[mode][0], 0xFF)
    b = _embed_run(c["p"].to(cuda).to(BF), c["dx"].to(cuda), MODES[mode][0], 0x00)
    G = {k: v.cpu() for k, v in _views(a).items()}
    eq = {"pe_w": torch.equal(G["pe_w"], c["W64"].float()), "pe_b": torch.equal(G["pe_b"], c["b64"].float()),
          "pos": torch.equal(G["pos"], c["pos64"].float())}
    same = torch.equal(a.view(torch.int32), b.view(torch.int32))
    print(f"integers, {mode} gradients, nS={nS}: equal to the CPU result {eq}; largest |dW| {float(c['W64'].abs().max()):.0f}; two runs bitwise equal {same}")
    assert all(eq.values()) and same


@pytest.mark.parametrize("nS", CROPS)
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_embed_backward_on_random_data(cuda, mode, nS):
    c = _case(nS, "rand")
    rows = nS * 1024
    a = _embed_run(c["p"].to(cuda).to(BF), c["dx"].to(cuda), MODES[mode][0], 0xFF)
    b = _embed_run(c["p"].to(cuda).to(BF), c["dx"].to(cuda), MODES[mode][0], 0x00)
    G = {k: v.cpu() for k, v in _views(a).items()}
    same = torch.equal(a.view(torch.int32), b.view(torch.int32))
    finite = bool(torch.isfinite(a).all())
    print(f"random data, {mode} gradients, nS={nS}: finite {finite}, two runs bitwise equal {same}")
    ok = [finite, same]
    if mode == "bf16":
        worst = float(((G["pe_w"].double() - c["W64r"]).abs() / ((rows + 2) * U * c["Wabs"]).clamp_min(1e-300)).max())
        print(f"  dW: worst |got - exact| / ((L + 2) 2^-24 sum |r(dx)||p|) = {worst:.4f}")
        ok.append(worst <= 1.0)
    else:
        ok.append(_check("dW", G["pe_w"], c["W32"], c["W64"]))
    for k, e, s in (("pe_b", "b64", "babs"), ("pos", "pos64", "posabs")):
        worst = float(((G[k].double() - c[e]).abs() / (U * c[e].abs() + 2.0 ** -40 * c[s]).clamp_min(1e-300)).max())
        print(f"  {k}: worst |got - exact| / (2^-24 |exact| + 2^-40 sum |dx|) = {worst:.4f}")
        ok.append(worst <= 1.0)
    zero_rows = torch.equal(G["pos"][::7], c["pos64"][::7].float()) if nS == 1 else True
    assert all(ok) and zero_rows


@pytest.mark.parametrize("prec", ["fp32", "fp16"])
def test_embed_backward_float32_mode_in_the_other_network_dtypes(cuda, prec):
    """fp32 and fp16 patch rows, widened exactly, at the odd crop count"""
    nS = 3
    c = _case(nS, "rand")
    p = c["p"].to(HD[prec])                                            # bf16 values are exact in both
    a = _embed_run(p.to(cuda), c["dx"].to(cuda), F32)
    G = {k: v.cpu() for k, v in _views(a).items()}
    ok = [_check(f"{prec} dW", G["pe_w"], c["W32"], c["W64"])]
    bits = torch.equal(a, _embed_run(c["p"].to(cuda).to(BF), c["dx"].to(cuda), F32))
    print(f"{prec} patch rows holding the same values give the bf16 rows' record bitwise: {bits}")
    assert all(ok) and bits


# ---- 3. crops do not mix ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_crops_do_not_mix(cuda, mode):
    c = _case(3, "rand")
    dx = c["dx"].clone()
    dx[:1024] = 0
    dx[2048:] = 0
    p = c["p"].to(cuda).to(BF)
    three = _views(_embed_run(p, dx.to(cuda), MODES[mode][0]))
    one = _views(_embed_run(p[1024:2048].contiguous(), dx[1024:2048].contiguous().to(cuda), MODES[mode][0]))
    pos = torch.equal(three["pos"].cpu(), dx[1024:2048])
    dw, db = torch.equal(three["pe_w"], one["pe_w"]), torch.equal(three["pe_b"], one["pe_b"])
    print(f"{mode}: dx in crop 1 of 3 only: dpos equals that crop's rows {pos}; dW equals the one-crop call's {dw}; db too {db}; "
          f"largest |dW| {float(one['pe_w'].abs().max()):.3e}")
    assert pos and dw and db and float(one["pe_w"].abs().max()) > 0


# ---- 4. refusals --------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_outputs_untouched(cuda):
    L, nS = _lib.lib(), 1
    bf, f16, f32 = _lib.DT_BF16, _lib.DT_F16, _lib.DT_F32
    n, off = ops.embed_grad_layout()
    assert n == 1024 * 192 + 1024 + 1024 * 1024 and off == [0, 1024 * 192, 1024 * 192 + 1024] and L.cpx_embed_grad_layout(None) == n
    p = torch.zeros(nS * 1024 + 8, 192, dtype=BF, device=cuda)
    dx = torch.zeros(nS * 1024 + 8, 1024, dtype=F32, device=cuda)
    nb = L.cpx_embed_backward_workspace_bytes(nS, bf, bf)
    assert nb > 0 and nb % 256 == 0 and L.cpx_embed_backward_workspace_bytes(nS, bf, f32) > 0
    sizes = {"nS 0": L.cpx_embed_backward_workspace_bytes(0, bf, f32), "nS 2^21": L.cpx_embed_backward_workspace_bytes(1 << 21, bf, f32),
             "fp16 + bf16": L.cpx_embed_backward_workspace_bytes(nS, f16, bf), "fp32 + bf16": L.cpx_embed_backward_workspace_bytes(nS, f32, bf),
             "dtype 9": L.cpx_embed_backward_workspace_bytes(nS, 9, f32), "grad fp16": L.cpx_embed_backward_workspace_bytes(nS, bf, f16)}
    print(f"workspace bytes of invalid arguments: {sizes}")
    assert not any(sizes.values())
    ws = torch.full((nb + 512,), 0xFF, dtype=torch.uint8, device=cuda)
    grads = torch.full((n + 8,), float("nan"), dtype=F32, device=cuda)
    s = _stream(cuda)
    P, D, G, W = p.data_ptr(), dx.data_ptr(), grads.data_ptr(), ws.data_ptr()
    assert W % 256 == 0 and G % 16 == 0
    cases = {"patches NULL": (bf, None, D, nS, bf, G, W, nb), "dx_in NULL": (bf, P, None, nS, bf, G, W, nb), "grads NULL": (bf, P, D, nS, bf, None, W, nb),
             "workspace NULL": (bf, P, D, nS, bf, G, None, nb), "patches + 2": (bf, P + 2, D, nS, bf, G, W, nb), "dx_in + 4": (bf, P, D + 4, nS, bf, G, W, nb),
             "grads + 4": (bf, P, D, nS, bf, G + 4, W, nb), "workspace + 128": (bf, P, D, nS, bf, G, W + 128, nb),
             "workspace short": (bf, P, D, nS, bf, G, W, nb - 1), "nS 0": (bf, P, D, 0, bf, G, W, nb), "nS -1": (bf, P, D, -1, f32, G, W, nb),
             "nS 2^21": (bf, P, D, 1 << 21, f32, G, W, 1 << 40), "fp16 + bf16": (f16, P, D, nS, bf, G, W, nb), "fp32 + bf16": (f32, P, D, nS, bf, G, W, nb),
             "dtype 9": (9, P, D, nS, f32, G, W, nb), "grad fp16": (bf, P, D, nS, f16, G, W, nb)}
    seen = {k: L.cpx_embed_backward(*a, s) for k, a in cases.items()}
    torch.cuda.synchronize(cuda)
    untouched = bool(torch.isnan(grads).all()) and bool((ws == 0xFF).all())
    print(f"return codes: {seen}; outputs untouched {untouched}")
    assert all(v == EINVAL for v in seen.values()) and untouched
    assert L.cpx_embed_backward(bf, P, D, nS, bf, G, W, nb, s) == 0
    torch.cuda.synchronize(cuda)
    assert bool((grads[:n] == 0).all()) and bool(torch.isnan(grads[n:]).all()), "zero gradients from zero dx, nothing beyond the record"
    # the wrappers and cpx_blocks_backward_in
    with pytest.raises(ValueError, match="bf16 network"):
        ops.embed_backward(p[:1024].to(torch.float16), dx[:1024], grad_dtype=BF)
    with pytest.raises(ValueError, match="dx_in must be"):
        ops.embed_backward(p[:1024], dx[:1024, :512].contiguous())
    with pytest.raises(ValueError, match="patches must be"):
        ops.embed_backward(p[:1000], dx[:1000])
    sd, w = bt._weights("bf16", cuda)
    x = _rows_in(w, _patches(1, "bf16", cuda, 44), 1, DEPTH, cuda)
    fwd = _forward_train(w, x, DEPTH, cuda)
    dy0 = torch.zeros(1024, 256, device=cuda)
    params = _rounded_params(sd, "bf16", cuda)
    g = torch.full((DEPTH * ops.block_grad_layout()[0],), float("nan"), dtype=F32, device=cuda)
    bws = ops.blocks_backward_workspace(1, w.c.dtype, cuda)
    rc = L.cpx_blocks_backward_in(C.byref(w.c), ptr(params), 1, 0, ptr(fwd.workspace), fwd.workspace.numel(), ptr(dy0), f32, f32, ptr(g), None,
                                  dx.data_ptr() + 4, ptr(bws), bws.numel(), s)
    torch.cuda.synchronize(cuda)
    print(f"cpx_blocks_backward_in with a misaligned dx_in: {rc}; grads untouched {bool(torch.isnan(g).all())}")
    assert rc == EINVAL and bool(torch.isnan(g).all())
    with pytest.raises(ValueError, match="dx_in must be"):
        ops.blocks_backward(w, params, fwd, dy0, dx_in=dx[:1024, :512].contiguous())


# ---- 5. end to end ------------------------------------------------------------------------------------------------------
def _trainer(dev, prec, sd=None, seed=53, **kw):
    from classpose_amd.train import HeadTrainer
    sd = synth.make_state_dict(NCLS, None, depth=DEPTH, seed=seed) if sd is None else sd
    return HeadTrainer(sd, device=dev, precision=prec, train_blocks=DEPTH, train_embed=True, **kw), sd


@pytest.mark.parametrize("prec,mode", [("fp32", "fp32"), ("bf16", "fp32"), ("fp16", "fp32"), ("bf16", "bf16+attn")])
def test_gradients_end_to_end(cuda, prec, mode):
    """Both blocks, the neck, both heads and the three new tensors from labels and flow targets, starting from patch rows"""
    nS = 1
    g16 = mode != "fp32"
    kw = dict(grad_precision="bf16", attn_grad_precision="bf16") if g16 else {}
    t, sd = _trainer(cuda, prec, feature_batch=1, train_flow_head=True, **kw)
    assert t.embed is not None and t.groups[-1] is t.embed and t.embed.keys == er.KEYS
    p = _patches(nS, prec, cuda, 23)
    labs, tg = _labels(nS, NCLS, 7), _targets(nS, 8)
    t.embed.grads.fill_(float("nan"))
    feat, head, o = t._loss(p, labs)
    seg = t._seg_loss(head, tg.to(cuda))
    t._neck_backward(*t._fwd, o, seg)
    t._blocks_backward()
    torch.cuda.synchronize(cuda)
    loss = float(o.ce.item()) + float(o.tversky.item()) + float(seg.flow.item()) + float(seg.cp.item())
    got_n = {k: v.clone().cpu() for k, v in _neck_views(t.neck.grads).items()}
    got_n["Wc"], got_n["bc"] = (v.cpu() for v in ops.head_wgrad(o.dlogits, feat))
    got_n["Wf"], got_n["bf"] = (v.cpu() for v in ops.head_wgrad(seg.dlogits, feat))
    net = None if prec == "fp32" else HD[prec]
    PE, PN = er.params_from_state_dict(sd), nr.params_from_state_dict(sd)
    PB = [br.params_from_state_dict(sd, j) for j in range(DEPTH)]
    lab = torch.from_numpy(labs.astype(np.int64))
    pc = p.float().cpu()
    r64 = er.loss_and_grads(PE, PB, PN, pc, lab, tg, NCLS, torch.float64, net)
    r32 = er.loss_and_grads_bf16(PE, PB, PN, pc, lab, tg, NCLS, F32, net, attn_bf16=True) if g16 else \
        er.loss_and_grads(PE, PB, PN, pc, lab, tg, NCLS, F32, net)
    print(f"{prec}, {mode} gradients: loss device {loss:.6f}, float64 {float(r64['loss']):.6f}, float32 {float(r32['loss']):.6f}")
    ok = [abs(loss - float(r64["loss"])) <= 1e-3 * abs(float(r64["loss"]))]
    for i, k in enumerate(er.NAMES):
        got = t.embed.view(i, t.embed.grads).cpu()
        assert got.shape == r64["embed"][k].shape and bool(torch.isfinite(got).all())
        ok.append(_check(k, got, r32["embed"][k], r64["embed"][k]))
    for k in nr.NECK + nr.HEADS:
        ok.append(_check(k, got_n[k], r32["neck"][k], r64["neck"][k]))
    for j in range(DEPTH):
        for ti, k in enumerate(br.NAMES):
            got = t.blocks.rel_grads[j][ti - 4] if k.startswith("rel_") else t.blocks.view(j, ti, t.blocks.grads)
            ok.append(_check(f"block {j} {k}", got.cpu(), r32["blocks"][j][k], r64["blocks"][j][k]))
    assert all(ok)


# ---- 6. training --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_twenty_steps(cuda, prec):
    """The first epochs of the reference's schedule from patch rows: lr = 0 changes nothing bitwise; two runs are bitwise equal; the loss
    goes down; fp32: the loss curve and the final update of the three tensors follow the float64 replay by the rule"""
    from classpose_amd.train import lr_schedule
    nS, steps = 1, 20
    labs, tg = _labels(nS, NCLS, 9), _targets(nS, 10)
    lrs = [float(v) for v in lr_schedule(2e-4, steps)[:steps]]
    runs = []
    for rep in range(2):
        t, sd = _trainer(cuda, prec, feature_batch=1, train_flow_head=True)
        p = t.patch_rows(_patches(nS, prec, cuda, 33))
        tgd = tg.to(cuda)
        E0, B0 = t.embed.params.clone(), t.blocks.params.clone()
        head0 = t.evaluate(p, labs, flow_targets=tgd, return_head=True)["head"].clone()
        losses = []
        for k, lr in enumerate(lrs):
            losses.append(t.step(p, labs, lr, flow_targets=tgd)["loss"])
            if k == 0:
                same_p = torch.equal(t.embed.params.view(torch.int32), E0.view(torch.int32)) and torch.equal(t.blocks.params, B0)
                same_h = torch.equal(t.evaluate(p, labs, flow_targets=tgd, return_head=True)["head"], head0)
                print(f"{prec}: after lr = 0 masters unchanged {same_p}, head unchanged {same_h}")
                assert same_p and same_h
        runs.append((np.array(losses), t.embed.params.clone(), t.blocks.params.clone()))
        if rep == 0:
            first, p_cpu = t, p.float().cpu()
    (losses, ea, ba), (losses_b, eb, bb_) = runs
    same_runs = bool((losses == losses_b).all()) and torch.equal(ea.view(torch.int32), eb.view(torch.int32)) and torch.equal(ba, bb_)
    moved = [not torch.equal(first.embed.view(i), first.embed.view(i, E0)) for i in range(3)]
    print(f"{prec}: loss step 1 = {losses[0]:.6f}, step {steps} = {losses[-1]:.6f}; first five {losses[:5].sum():.6f}, last five "
          f"{losses[-5:].sum():.6f}; two runs bitwise equal {same_runs}; pe_w, pe_b, pos moved {moved}")
    assert same_runs and all(moved) and bool(torch.isfinite(ea).all())
    t = first
    if prec == "fp32":
        PE, PN = er.params_from_state_dict(sd), nr.params_from_state_dict(sd)
        PB = [br.params_from_state_dict(sd, j) for j in range(DEPTH)]
        lab = torch.from_numpy(labs.astype(np.int64))
        l64, e64, _b, _n = er.replay(PE, PB, PN, p_cpu, lab, tg, NCLS, lrs, torch.float64, None, t.weight_decay)
        l32, e32, _b, _n = er.replay(PE, PB, PN, p_cpu, lab, tg, NCLS, lrs, F32, None, t.weight_decay)
        floor = steps * FLOOR
        ok = [_check("loss curve", losses, l32, l64, floor)]
        for i, k in enumerate(er.NAMES):
            ok.append(_check(f"final update of {k}", t.embed.view(i).cpu().double() - PE[k].double(), e32[k].double() - PE[k].double(),
                             e64[k] - PE[k].double(), floor))
        assert all(ok) and l64[-5:].sum() < l64[:5].sum()
    assert losses[-5:].sum() < losses[:5].sum()


# ---- 7. off means off ---------------------------------------------------------------------------------------------------
def test_train_embed_off_is_the_trainer_as_before(cuda):
    from classpose_amd.train import EmbedParams, HeadTrainer
    from classpose_amd.train_unet import UNetHeadTrainer
    sd = synth.make_state_dict(NCLS, None, depth=DEPTH, seed=54)
    t = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=1, train_blocks=DEPTH)
    u = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=1, train_blocks=DEPTH, train_embed=False)
    assert t.embed is None and u.embed is None and not any(isinstance(g, EmbedParams) for g in t.groups + u.groups) and len(t.groups) == len(u.groups)
    w, c = t.weights, t.weights.c
    ops0 = [bt._operand(w, q).clone() for q in (c.pe_w, c.pe_b, c.pos)]
    p = _patches(1, "bf16", cuda, 61)
    x, labs = t.backbone_features(p), _labels(1, NCLS, 11)
    for lr in (0.0, 1e-3, 2e-3):
        ra, rb = t.step(x, labs, lr), u.step(x, labs, lr)
        print(f"  lr {lr}: {ra} | {rb}")
        assert ra == rb
    same_ops = all(torch.equal(a.view(torch.uint8), bt._operand(w, q).view(torch.uint8)) for a, q in zip(ops0, (c.pe_w, c.pe_b, c.pos)))
    st = t.state_dict()
    same_sd = all(torch.equal(st[k], sd[k]) for k in er.KEYS)
    print(f"after three steps without train_embed: pe_w / pe_b / pos operands bitwise as loaded {same_ops}; state-dict entries as loaded {same_sd}")
    assert same_ops and same_sd and all(torch.equal(a, b) for a, b in zip(st.values(), u.state_dict().values()))
    for K in (0, 1):
        with pytest.raises(ValueError, match="train_embed needs train_blocks = 2"):
            HeadTrainer(sd, device=cuda, train_blocks=K, train_embed=True)
    with pytest.raises(NotImplementedError, match="train_embed"):
        UNetHeadTrainer(sd, device=cuda, feature_transformation_structure=[16, 24], train_embed=True)
    bad = dict(sd)
    bad["encoder.pos_embed"] = torch.zeros(1, 16, 16, 1024)
    with pytest.raises(ValueError, match="pos_embed"):
        EmbedParams(bad, w)


# ---- 8. the checkpoint --------------------------------------------------------------------------------------------------
def test_the_saved_checkpoint_loads_into_net_weights(cuda, tmp_path):
    from classpose_amd import augment
    ims, labs, inst = bt._crops(2)
    tg = torch.stack(augment.flow_targets_of(list(inst), cuda))
    t, sd = _trainer(cuda, "bf16", seed=55, feature_batch=2, train_flow_head=True)
    p = t.patch_rows(ims)
    assert p.shape == (2 * 1024, 192) and p.dtype == BF
    assert t.evaluate(p, labs, flow_targets=tg) == t.evaluate(ims, labs, flow_targets=tg), "cached patch rows and pixels give the same losses"
    for lr in (1e-3, 2e-3, 2e-3):
        t.step(p, labs, lr, flow_targets=tg)
    t.save(tmp_path / "embed.pt")
    t.save(tmp_path / "embed_only.pt", save_only_trainable_params=True)
    ck = torch.load(tmp_path / "embed.pt", map_location="cpu", weights_only=True)
    only = torch.load(tmp_path / "embed_only.pt", map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and all(ck[k].shape == sd[k].shape and ck[k].dtype == sd[k].dtype for k in sd)
    assert set(er.KEYS) <= set(only) and all(torch.equal(only[k], ck[k]) for k in only)
    changed = {k for k in sd if not torch.equal(ck[k], sd[k])}
    print(f"changed keys: {len(changed)}; the three new ones among them: {set(er.KEYS) <= changed}")
    assert set(er.KEYS) <= changed
    w, tw = engine.NetWeights.from_state_dict(ck, "bf16", cuda), t.weights
    same_ops = all(torch.equal(bt._operand(w, getattr(w.c, n)).view(torch.uint8), bt._operand(tw, getattr(tw.c, n)).view(torch.uint8))
                   for n in ("pe_w", "pe_b", "pos"))
    ev = t.evaluate(ims, labs, flow_targets=tg, return_head=True)["head"].clone()
    head, _x = bt._net_forward(w, t._patches(ims), 2, cuda)
    same = torch.equal(head[:, :192 + NCLS * 64], ev[:, :192 + NCLS * 64])
    print(f"pe_w / pe_b / pos of the loaded checkpoint bitwise the trainer's operands: {same_ops}; cpx_net_forward on it equals the trainer's head: {same}")
    assert same_ops and same
    r, _ = _trainer(cuda, "bf16", sd=ck, feature_batch=2, train_flow_head=True)
    assert torch.equal(r.embed.params, t.embed.params)


# ---- 9. the command line ------------------------------------------------------------------------------------------------
def test_cli_train_embed_in_a_child_process(cuda, tmp_path):
    sd = synth.make_state_dict(1, None, depth=DEPTH, seed=56)
    torch.save(sd, tmp_path / "backbone.pt")
    d = tmp_path / "data"
    d.mkdir()
    imgs, labs = np.empty(2, dtype=object), np.empty(2, dtype=object)
    for k, (h, wd) in enumerate([(512, 256), (256, 512)]):
        inst = np.zeros((h, wd), np.int32)
        inst[:256, :256] = fr.disc_crop(70 + k)
        imgs[k] = synth.render_region(300, 64 * k, 32 * k, wd, h)
        labs[k] = np.stack([inst, np.where(inst > 0, 1 + inst % 2, 0).astype(np.int32)], -1)
    np.save(d / "images.npy", imgs, allow_pickle=True)
    np.save(d / "labels.npy", labs, allow_pickle=True)
    r = subprocess.run(bt._cli(tmp_path, "--train_embed", "--train_blocks", str(DEPTH)), cwd=ROOT, capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    assert "the cache holds patch rows" in r.stdout + r.stderr
    ck = torch.load(out, map_location="cpu", weights_only=True)
    moved = {k: not torch.equal(ck[k], sd[k]) and ck[k].shape == sd[k].shape and bool(torch.isfinite(ck[k]).all()) for k in er.KEYS}
    print(f"the three tensors differ from the input's: {moved}")
    assert all(moved.values()) and engine.NetWeights.from_state_dict(ck, "bf16", cuda).ncls == 3
    r = subprocess.run(bt._cli(tmp_path, "--train_embed"), cwd=ROOT, capture_output=True, text=True)
    print(r.stderr.strip().splitlines()[-1])
    assert r.returncode != 0 and "--train_embed needs --train_blocks" in r.stderr and "only through every block" in r.stderr
    r = subprocess.run(bt._cli(tmp_path, "--train_embed", "--train_blocks", "1"), cwd=ROOT, capture_output=True, text=True)
    print(r.stderr.strip().splitlines()[-1])
    assert r.returncode != 0 and f"--train_blocks {DEPTH}" in r.stderr and "only through every block" in r.stderr
    r = subprocess.run(bt._cli(tmp_path, "--train_embed", "--train_blocks", str(DEPTH), "--feature_transformation_structure", "16", "24"), cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode != 0 and "UNet class head" in r.stderr and "--train_embed" in r.stderr
