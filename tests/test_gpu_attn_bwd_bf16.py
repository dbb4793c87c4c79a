"""The attention backward on bf16 operands: cpx_attention_backward_bf16 (csrc/cpx_attn_bwd16.hip), cpx_blocks_backward_mp,
HeadTrainer(attn_grad_precision="bf16") and train_head --attn_grad_precision bf16.  The network is synth.make_state_dict(3, None, depth=2);
the helpers are those of tests/test_gpu_block_train*.py, the restatement is tests/attn_bwd_bf16_reference.py.

Bounds, all derived and none measured on the device:
  * integer cases: every operand, every product, every partial sum and every rounded value is exactly representable (S' = 0, P = 2^-10,
    dS' = 2^-13 dP with |dP| <= 64), so any order of float32 additions is exact: torch.equal with the float64 CPU result.
  * random data, r64 the unrounded float64 backward, b64 / b32 the restatement with the roundings in float64 / float32:
      (i)  the project's rule: err(device, r64) <= max(4 err(b32, r64), 2^-20);
      (ii) the sharp one for dq, dk, dv: err(device, b64) <= err(b64, r64) / 4 -- the roundings move the result by about 2.4e-3, the order
           of the float32 sums by 1e-5 .. 6e-5 (CPU), a missing or misplaced rounding by 1.3e-3 upwards;
           for the tables (no rounded operand enters them directly): err(device, b64) <= max(4 err(b32, b64), 2^-20).
Every workspace is poisoned (0xFF, then 0x00), every output starts as NaN, and every test prints what it observed before it asserts."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import attn_bwd_bf16_reference as ab
import block_train_bf16_reference as b16
import block_train_reference as br
import flow_train_reference as fr
import test_gpu_block_train as bt
import test_gpu_block_train_batches as bb
from classpose_amd import _lib, engine, ops, synth
from classpose_amd._lib import ptr
from test_gpu_block_train import DEPTH, NCLS, ROOT, _attn_case, _check, _forward_train, _grad_views, _patches, _rounded_params, _rows_in, _table_grad

pytestmark = pytest.mark.gpu
EINVAL = -22
FLOOR = 2.0 ** -20
BF, F32 = torch.bfloat16, torch.float32
SLICES = (("dq", slice(0, 1024)), ("dk", slice(1024, 2048)), ("dv", slice(2048, 3072)))


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _attn_run(qkv, Rh, Rw, dO, dev):
    """two runs on differently poisoned workspaces -> (first result, bitwise equal)"""
    nS = qkv.shape[0] // 1024
    q, h, w, d = (t.to(dev) for t in (qkv, Rh, Rw, dO))
    out = torch.full((nS * 1024, 1024), float("nan"), dtype=q.dtype, device=dev)      # not read in this mode
    res = []
    for fill in (0xFF, 0x00):
        ws = ops.attention_backward_workspace(nS, dev)
        ws.fill_(fill)
        res.append(ops.attention_backward(q, h, w, out, d, ws, grad_dtype=BF))
    torch.cuda.synchronize(dev)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res))
    return res[0], same


# ---- 1. exact integer cases -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["q", "k"])
def test_integer_operands_are_exact(cuda, which):
    """(a) q in {-2 .. 2}, k = 0: non-zero dk, dv, dRh, dRw; (b) q = 0, k in {-2 .. 2}: non-zero dq, dv.  Tables zero, dO and v in
    {-1, 0, 1}, every channel of v summing to zero over the keys: S' = 0, P = 2^-10, delta = 0, dS' = 2^-13 dP.  Every operand
    permutation of the five products is pinned: a wrong k order changes integers"""
    g = torch.Generator().manual_seed(81 + (which == "k"))
    qkv = torch.zeros(1024, 3072)
    col = slice(0, 1024) if which == "q" else slice(1024, 2048)
    qkv[:, col] = torch.randint(-2, 3, (1024, 1024), generator=g).float()
    half = torch.randint(-1, 2, (512, 1024), generator=g).float()
    qkv[:, 2048:] = torch.cat([half, -half])[torch.randperm(1024, generator=g)]
    dO = torch.randint(-1, 2, (1024, 1024), generator=g).float()
    Z = torch.zeros(64, 64)
    assert not bool(qkv[:, 2048:].reshape(1024, 16, 64).sum(0).any())
    b64 = ab.attention_backward_bf16(qkv.double(), Z.double(), Z.double(), dO.double(), 1)
    b32 = ab.attention_backward_bf16(qkv, Z, Z, dO, 1)
    r64 = br.attention_backward(qkv.double(), Z.double(), Z.double(), dO.double(), 1)
    cpu_exact = torch.equal(b32["dqkv"].double(), b64["dqkv"]) and all(torch.equal(b64[k], r64[k]) for k in ("dqkv", "dRh", "dRw"))
    (dqkv, drh, drw), same = _attn_run(qkv.to(BF), Z.to(BF), Z.to(BF), dO, cuda)
    eq = {n: torch.equal(dqkv[:, s].cpu().double(), b64["dqkv"][:, s]) for n, s in SLICES}
    eq["dRh"], eq["dRw"] = torch.equal(drh.cpu(), b64["dRh"].float()), torch.equal(drw.cpu(), b64["dRw"].float())
    live = {n: bool(b64["dqkv"][:, s].any()) for n, s in SLICES}
    live["dRh"], live["dRw"] = bool(b64["dRh"].any()), bool(b64["dRw"].any())
    print(f"integers in {which}: CPU float32 restatement == float64 == unrounded float64: {cpu_exact}; device equal to float64: {eq}; non-zero: {live}; "
          f"two runs bitwise equal {same}; max |dqkv| {float(dqkv.abs().max()):.6g}")
    assert cpu_exact and all(eq.values()) and same
    assert live == ({"dq": False, "dk": True, "dv": True, "dRh": True, "dRw": True} if which == "q" else
                    {"dq": True, "dk": False, "dv": True, "dRh": False, "dRw": False})


# ---- 2. every output on random data -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS,qscale", [(1, 1.0), (1, 7.5), (3, 1.0)])
def test_every_output_on_random_data(cuda, nS, qscale):
    """A norm test: rules (i) and (ii) of the module's docstring take ONE relative L2 norm per tensor (dq, dk, dv, dRel_h, dRel_w);
    "every output" is each of the five tensors, not each element.  32 token rows of head 0 multiplied by 1.3 pass both rules
    (tests/test_attn_bwd_bounds_host.py); the elements are checked in tests/test_gpu_attn_bwd_every_element.py"""
    qkv, Rh, Rw, dO = _attn_case(nS, "bf16", 61, qscale)
    (dqkv, drh, drw), same = _attn_run(qkv, Rh, Rw, dO, cuda)
    r64 = br.attention_backward(qkv.double(), Rh.double(), Rw.double(), dO.double(), nS)
    b64 = ab.attention_backward_bf16(qkv.double(), Rh.double(), Rw.double(), dO.double(), nS)
    b32 = ab.attention_backward_bf16(qkv.float(), Rh.float(), Rw.float(), dO, nS)
    lg = br._logits(*br._split(qkv[:1024].double(), 1)[:2], Rh.double(), Rw.double(), 1) * br.SCALE
    print(f"bf16 attention backward qscale={qscale} nS={nS}: logits of crop 0 {float(lg.min()):.1f} .. {float(lg.max()):.1f}; two runs bitwise equal {same}")
    dev = {n: dqkv[:, s].cpu() for n, s in SLICES}
    dev["dRh"], dev["dRw"] = drh.cpu(), drw.cpu()
    pick = lambda R: {**{n: R["dqkv"][:, s] for n, s in SLICES}, "dRh": R["dRh"], "dRw": R["dRw"]}
    R64, B64, B32 = pick(r64), pick(b64), pick(b32)
    ok = []
    for n in dev:
        ok.append(_check(f"(i) {n}", dev[n], B32[n], R64[n]))
        e_dev, away, e32 = _rel(dev[n], B64[n]), _rel(B64[n], R64[n]), _rel(B32[n], B64[n])
        tol = away / 4 if n in ("dq", "dk", "dv") else max(4 * e32, FLOOR)
        print(f"  (ii) {n}: err(device, b64) = {e_dev:.3e}, err(b64, r64) = {away:.3e}, err(b32, b64) = {e32:.3e}, tolerance = {tol:.3e}")
        ok.append(e_dev <= tol)
    finite = all(bool(torch.isfinite(t).all()) for t in (dqkv, drh, drw))
    zero_dq = not bool(dqkv[::5, :1024].any())
    zero_pad = not bool(drh[63].any()) and not bool(drw[63].any())
    print(f"  finite {finite}; rows with dO = 0 give zero dq: {zero_dq}; row 63 of both table gradients zero: {zero_pad}")
    assert all(ok) and same and finite and zero_dq and zero_pad
    if qscale > 1:
        assert float(lg.abs().max()) > 40


# ---- 3. dO enters through r(dO) alone -----------------------------------------------------------------------------------------
def test_dout_enters_rounded_to_bf16_and_in_no_other_form(cuda):
    """dO = a bf16 value moved by less than half an ulp (a quarter at most, so it stays inside the rounding interval next to a power of
    two as well), or by exactly half an ulp away from zero: a tie, which goes to the even neighbour -- back to the value where its last
    bit is even, on to the next one where it is odd.  Every output is bitwise the run on dO.to(bfloat16).float()"""
    qkv, Rh, Rw, dO = _attn_case(1, "bf16", 63)
    base = dO.to(BF).float()
    ulp = torch.exp2(torch.floor(torch.log2(base.abs().clamp_min(2.0 ** -100))) - 7)
    g = torch.Generator().manual_seed(64)
    kind = torch.randint(0, 4, base.shape, generator=g)
    frac = (torch.rand(base.shape, generator=g) * 0.5 - 0.25) * (kind < 3) + 0.5 * (kind == 3) * torch.sign(base)
    moved = base + frac * ulp
    moved[base == 0] = 0
    rounded = moved.to(BF).float()
    ties = (kind == 3) & (base != 0)
    back, on = int((ties & (rounded == base)).sum()), int((ties & (rounded != base)).sum())
    off_tie = bool(((rounded == base) | ties).all())
    print(f"{int((moved != rounded).sum())} of {moved.numel()} values of dO are not bf16 values; ties that go back to an even value {back}, on to "
          f"the even neighbour of an odd one {on}; every other value rounds to where it came from {off_tie}")
    assert back > 1000 and on > 1000 and off_tie
    (a, ah, aw), same = _attn_run(qkv, Rh, Rw, moved, cuda)
    (b, bh, bw), _ = _attn_run(qkv, Rh, Rw, rounded, cuda)
    eq = torch.equal(a, b), torch.equal(ah, bh), torch.equal(aw, bw)
    print(f"dqkv, dRh, dRw bitwise equal to the run on the rounded dO: {eq}; max |dqkv| {float(a.abs().max()):.3e}")
    assert all(eq) and same and float(a.abs().max()) > 0


# ---- 4. crop border ---------------------------------------------------------------------------------------------------------
def test_does_not_cross_a_crop_border(cuda):
    qkv, Rh, Rw, dO = _attn_case(3, "bf16", 62)
    dO[:1024] = 0
    dO[2048:] = 0
    (dqkv, drh, drw), same = _attn_run(qkv, Rh, Rw, dO, cuda)
    (one, oh, ow), _ = _attn_run(qkv[1024:2048], Rh, Rw, dO[1024:2048], cuda)
    outer = bool(dqkv[:1024].any()) or bool(dqkv[2048:].any())
    inner = torch.equal(dqkv[1024:2048], one)
    tables = torch.equal(drh, oh) and torch.equal(drw, ow)
    print(f"anything non-zero on crops 0 / 2: {outer}; crop 1 bitwise its own run: {inner}; table gradients equal the one crop's: {tables}; "
          f"two runs bitwise equal {same}; max |dqkv crop 1| = {float(one.abs().max()):.3e}")
    assert not outer and inner and tables and same and float(one.abs().max()) > 0


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------
def test_refuses_what_the_header_excludes(cuda):
    """the C entry has no dtype argument (bf16 is its only element type), so fp16 / fp32 rows are refused where the dtype is known:
    ops.attention_backward, and cpx_blocks_backward_mp (test_mp_refusals_and_the_float32_switch)"""
    L, s = _lib.lib(), _stream(cuda)
    qkv, Rh, Rw, dO = (t.to(cuda) for t in _attn_case(1, "bf16", 65))
    nb = L.cpx_attention_backward_bf16_workspace_bytes(1)
    ws = torch.full((nb + 256,), 0xFF, dtype=torch.uint8, device=cuda)
    dqkv = torch.full((1024 * 3072 + 8,), float("nan"), device=cuda)
    drh, drw = torch.full((64 * 64 + 8,), float("nan"), device=cuda), torch.full((64 * 64 + 8,), float("nan"), device=cuda)
    good = [ptr(qkv), ptr(Rh), ptr(Rw), ptr(dO), 1, ptr(dqkv), ptr(drh), ptr(drw), ptr(ws), nb]
    cases = {"qkv null": (0, None), "rel_h null": (1, None), "rel_w null": (2, None), "dO null": (3, None), "dqkv null": (5, None),
             "drel_h null": (6, None), "drel_w null": (7, None), "workspace null": (8, None), "qkv misaligned": (0, ptr(qkv) + 8),
             "rel_w misaligned": (2, ptr(Rw) + 2), "dO misaligned": (3, ptr(dO) + 4), "dqkv misaligned": (5, ptr(dqkv) + 4),
             "workspace misaligned": (8, ptr(ws) + 128), "workspace one byte short": (9, nb - 1), "no crops": (4, 0), "too many crops": (4, 16384)}
    seen = {}
    for what, (i, v) in cases.items():
        args = list(good)
        args[i] = v
        seen[what] = L.cpx_attention_backward_bf16(*args, s)
    torch.cuda.synchronize(cuda)
    untouched = all(bool(torch.isnan(t).all()) for t in (dqkv, drh, drw))
    print(f"refusals: {seen}; NaN-poisoned outputs untouched: {untouched}")
    assert all(rc == EINVAL for rc in seen.values()) and untouched
    for dt in (torch.float16, torch.float32):
        with pytest.raises(ValueError, match="needs bf16 qkv"):
            ops.attention_backward(qkv.to(dt), Rh.to(dt), Rw.to(dt), dO.to(dt), dO, grad_dtype=BF)
    assert L.cpx_attention_backward_bf16(*good, s) == 0
    torch.cuda.synchronize(cuda)
    assert bool(torch.isfinite(dqkv[:1024 * 3072]).all()) and bool(torch.isnan(dqkv[1024 * 3072:]).all()) and bool(torch.isnan(drh[4096:]).all())


# ---- 6. the blocks ------------------------------------------------------------------------------------------------------------
def _run(w, params, fwd, dy0, dev, attn_dtype=BF, want_dx=True, fill=0xFF):
    K, rows = len(fwd.x), fwd.x_out.shape[0]
    ws = ops.blocks_backward_workspace(rows // 1024, w.c.dtype, dev, BF, attn_dtype)
    ws.fill_(fill)
    n, _o = ops.block_grad_layout()
    grads = torch.full((K * n,), float("nan"), dtype=F32, device=dev)
    dx = torch.full((K + 1, rows, 1024), float("nan"), dtype=F32, device=dev) if want_dx else None
    ops.blocks_backward(w, params, fwd, dy0, grads, ws, dx, grad_dtype=BF, attn_grad_dtype=attn_dtype)
    torch.cuda.synchronize(dev)
    return grads, dx


@pytest.mark.parametrize("fused", [True, False])
def test_backward_block_by_block(cuda, fused):
    """nS = 3 (a slab of two crops and a remainder), K = 2: rule (i) for every gradient of every block and every dx record, each block
    on the device's own stored tensors and incoming gradient, against the float64 replay without roundings; the comparator is the block
    restatement in float32 with the roundings of the GEMMs and of the attention backward"""
    prec, nS, net = "bf16", 3, BF
    sd, w = bb._weights_for(prec, fused, cuda)
    x = _rows_in(w, _patches(nS, prec, cuda, 13 + nS), nS, DEPTH, cuda)
    fwd = _forward_train(w, x, DEPTH, cuda)
    g = torch.Generator(device=cuda).manual_seed(17 + nS)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=cuda) * torch.logspace(-2, 0, 256, device=cuda)[None]
    params = _rounded_params(sd, prec, cuda)
    grads, dx = _run(w, params, fwd, dy0, cuda)
    finite = bool(torch.isfinite(grads).all()) and bool(torch.isfinite(dx).all())
    print(f"bf16 gradients and bf16 attention backward, fuse_ln={fused}, nS={nS}: everything finite {finite}")
    assert finite
    ok = []
    for j in (1, 0):
        P = br.params_from_state_dict(sd, j)
        xin, dout = fwd.x[j].float().cpu(), dx[j + 1].cpu()
        held = {"qkv": fwd.qkv[j].float().cpu(), "ao": fwd.ao[j].float().cpu(), "x_mid": fwd.x_mid[j].float().cpu()}
        r64 = br.block_grads(P, xin, dout, nS, torch.float64, net, fused, stored=held)
        r32 = ab.block_backward(P, xin, dout, nS, F32, net, fused, stored=held, rnd=b16.round_bf16)
        G = {k: v.cpu() for k, v in _grad_views(grads, j).items()}
        for k in br.NAMES:
            got = _table_grad(sd, j, k, G[k]) if k.startswith("rel_") else G[k]
            ok.append(_check(f"block {j} {k}", got, r32["grads"][k], r64["grads"][k]))
        ok.append(_check(f"block {j} dx", dx[j].cpu(), r32["dx"], r64["dx"]))
        assert not bool(G["rel_h"][63].any()) and not bool(G["rel_w"][63].any())
    assert all(ok)


def test_mp_refusals_and_the_float32_switch(cuda):
    """cpx_blocks_backward_mp(attn CPX_DT_F32) is cpx_blocks_backward_ex on every gradient and dx record; attn CPX_DT_BF16 without bf16
    gradient GEMMs, or on an fp16 network, is CPX_EINVAL with the outputs untouched; two bf16-attention runs are bitwise equal"""
    nS = 3
    w, o, dy0, params = bb._backward_case(cuda, "bf16", True, nS, DEPTH, 150)
    L, c, s = _lib.lib(), w.c, _stream(cuda)
    b16c, f32c, f16c = _lib.DT_BF16, _lib.DT_F32, _lib.DT_F16
    a, dxa = _run(w, params, o, dy0, cuda, F32)
    nb = L.cpx_blocks_backward_workspace_bytes_ex(nS, c.dtype, b16c)
    ws = torch.full((nb,), 0x00, dtype=torch.uint8, device=cuda)
    g2, dx2 = torch.full_like(a, float("nan")), torch.full_like(dxa, float("nan"))
    _lib.check(L.cpx_blocks_backward_ex(C.byref(c), ptr(params), nS, o.first_block, ptr(o.workspace), o.workspace.numel(), ptr(dy0), b16c, ptr(g2),
                                        ptr(dx2), ptr(ws), nb, s), "blocks_backward_ex")
    torch.cuda.synchronize(cuda)
    same_ex = torch.equal(a, g2) and torch.equal(dxa, dx2)
    g3, dx3 = torch.full_like(a, float("nan")), torch.full_like(dxa, float("nan"))
    seen = {}
    for what, (gd, ad) in {"float32 GEMMs, bf16 attention": (f32c, b16c), "fp16 attention": (b16c, f16c), "fp16 both": (f16c, f16c)}.items():
        seen[what] = L.cpx_blocks_backward_mp(C.byref(c), ptr(params), nS, o.first_block, ptr(o.workspace), o.workspace.numel(), ptr(dy0), gd, ad,
                                              ptr(g3), ptr(dx3), ptr(ws), nb, s)
    c16 = bt._weights("fp16", cuda)[1].c
    seen["fp16 network"] = L.cpx_blocks_backward_mp(C.byref(c16), ptr(params), nS, o.first_block, ptr(o.workspace), o.workspace.numel(), ptr(dy0),
                                                    b16c, b16c, ptr(g3), ptr(dx3), ptr(ws), nb, s)
    torch.cuda.synchronize(cuda)
    untouched = bool(torch.isnan(g3).all()) and bool(torch.isnan(dx3).all())
    b, dxb = _run(w, params, o, dy0, cuda, BF, fill=0xFF)
    b2, dxb2 = _run(w, params, o, dy0, cuda, BF, fill=0x00)
    same = torch.equal(b.view(torch.int32), b2.view(torch.int32)) and torch.equal(dxb.view(torch.int32), dxb2.view(torch.int32))
    away = float((b - a).norm() / a.norm())
    print(f"_mp(attn float32) equals _ex on every gradient and dx record: {same_ex}; refusals {seen}, outputs untouched {untouched}; two bf16-attention "
          f"runs bitwise equal {same}; distance of their gradients from the float32-attention ones {away:.3e}")
    assert same_ex and all(rc == EINVAL for rc in seen.values()) and untouched and same and bool(torch.isfinite(b).all()) and 0 < away < 2.0 ** -5
    with pytest.raises(ValueError, match="needs grad_dtype torch.bfloat16"):
        ops.blocks_backward(w, params, o, dy0, grad_dtype=F32, attn_grad_dtype=BF)


@pytest.mark.parametrize("slab", [0, 1])
def test_backward_of_one_hot_slab_equals_the_slab_alone(cuda, slab):
    """nS = 3, K = 1, dy0 non-zero in slab 0 (two crops) or in the one-crop remainder: the table gradients of the slabs are added in
    order (add_rel), the other slab adds exact zeros"""
    nS, K = 3, 1
    w, o, dy0, params = bb._backward_case(cuda, "bf16", True, nS, K, 160 + slab)
    hot, mask = bb._hot(dy0, [slab], nS)
    c0 = slab * bb.SLAB
    nc = min(bb.SLAB, nS - c0)
    assert int(mask.sum()) == nc * 1024 and nc == (2, 1)[slab]
    grads, dx = _run(w, params, o, hot, cuda)
    alone, dx1 = _run(w, params, bb._slab_record(w, o, c0, nc, cuda), hot[mask].contiguous(), cuda)
    G, A = _grad_views(grads, 0), _grad_views(alone, 0)
    diff = [k for k in G if not torch.equal(G[k], A[k])]
    same_dx, zero_dx = torch.equal(dx[:, mask], dx1), not bool(dx[:, ~mask].any())
    live = float(dx1.abs().max()) > 0 and all(float(v.abs().max()) > 0 for v in A.values())
    print(f"bf16 attention backward, slab {slab} ({nc} crop(s)) hot: tensors that differ from the slab alone: {diff or 'none'} of {len(G)}; the slab's dx "
          f"rows equal {same_dx}; every other dx row zero {zero_dx}")
    assert len(G) == 14 and not diff and same_dx and zero_dx and live and bool(torch.isfinite(grads).all())


# ---- 7. the trainer and the command line ----------------------------------------------------------------------------------------
def test_trainer_twenty_steps_with_and_without(cuda, tmp_path):
    from classpose_amd.train import HeadTrainer, lr_schedule
    nS, steps = 2, 20
    labs, tg = bt._labels(nS, NCLS, 9), bt._targets(nS, 10).to(cuda)
    lrs = [float(v) for v in lr_schedule(2e-4, steps)[:steps]]
    curves = {}
    for mode in ("fp32", "bf16"):
        t, sd = bt._trainer(cuda, "bf16", 1, feature_batch=nS, train_flow_head=True, grad_precision="bf16", attn_grad_precision=mode)
        assert t.grad_precision == "bf16" and t.attn_grad_precision == mode
        x = t.backbone_features(_patches(nS, "bf16", cuda, 33))
        curves[mode] = np.array([t.step(x, labs, lr, flow_targets=tg)["loss"] for lr in lrs])
    for k in range(steps):
        print(f"  step {k + 1:2d}: float32 attention backward {curves['fp32'][k]:.6f}   bf16 attention backward {curves['bf16'][k]:.6f}")
    dist = float(np.abs(curves["bf16"] - curves["fp32"]).max() / np.abs(curves["fp32"]).max())
    print(f"largest distance of the two loss curves, relative to the largest loss: {dist:.3e} (recorded, not gated)")
    for mode, c in curves.items():
        assert np.isfinite(c).all() and c[-1] < c[0], mode
    t.save(tmp_path / "attn16.pt")
    ck = torch.load(tmp_path / "attn16.pt", map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and all(ck[k].shape == sd[k].shape and ck[k].dtype == sd[k].dtype for k in sd)
    assert engine.NetWeights.from_state_dict(ck, "bf16", cuda).ncls == NCLS
    changed = [k for k in sd if k.startswith(f"encoder.blocks.{DEPTH - 1}.") and not torch.equal(ck[k], sd[k])]
    assert len(changed) == 14
    with pytest.raises(ValueError, match="needs grad_precision bf16"):
        HeadTrainer(sd, device=cuda, precision="bf16", train_blocks=1, attn_grad_precision="bf16")


def test_cli_attn_grad_precision_bf16_in_a_child_process(cuda, tmp_path):
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
    bad = subprocess.run(bt._cli(tmp_path, "--train_blocks", "1", "--attn_grad_precision", "bf16", "--precision", "bf16"), cwd=ROOT,
                         capture_output=True, text=True)
    print(f"without --grad_precision bf16: exit {bad.returncode}: {bad.stderr.strip().splitlines()[-1][:200] if bad.stderr.strip() else ''}")
    assert bad.returncode != 0 and "--attn_grad_precision bf16 needs --grad_precision bf16" in bad.stderr and not (tmp_path / "m" / "m").exists()
    r = subprocess.run(bt._cli(tmp_path, "--train_blocks", "1", "--grad_precision", "bf16", "--attn_grad_precision", "bf16", "--precision", "bf16"),
                       cwd=ROOT, capture_output=True, text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    ck = torch.load(out, map_location="cpu", weights_only=True)
    last = [k for k in sd if k.startswith(f"encoder.blocks.{DEPTH - 1}.")]
    assert len(last) == 14 and all(ck[k].shape == sd[k].shape and not torch.equal(ck[k], sd[k]) and bool(torch.isfinite(ck[k]).all()) for k in last)
    assert all(torch.equal(ck[k], sd[k]) for k in sd if k.startswith("encoder.blocks.0."))
    assert engine.NetWeights.from_state_dict(ck, "bf16", cuda).ncls == 3
