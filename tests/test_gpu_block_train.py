"""Device training of the last transformer blocks (csrc/cpx_train_blocks.hip -> ops -> classpose_amd.train.BlockParams /
HeadTrainer(train_blocks=K) -> the train_head CLI).  The network is synth.make_state_dict(3, None, depth=2): every shape is fixed by the
architecture except the crop count; nS = 1 is one crop and the smallest grid, nS = 3 an odd crop count (attention and the rel-pos
reductions must not cross a crop's border; the backward's slabs of two crops leave a remainder).  Its rel-pos tables have 27 rows, so
every table gradient in the checkpoint's shape goes back through the interpolation to 63 rows.  Every workspace is poisoned (0xFF
bytes, NaN gradients) before the call that fills it.

The project's rule wherever a float64 answer exists, err(x) = ||x - q64||_2 / ||q64||_2:
    err(device) <= max(4 * err(torch CPU float32), 2^-20)
with q64 from tests/block_train_reference.py on the same stored inputs (bf16 / fp16: the straight-through replay, LayerNorm folded as
the device folds it).  LayerNorm backward at C = 1024: the element bound of tests/test_gpu_neck_train.py,
|got - exact| <= u |exact| + 2^-40 S.  Every test prints what it observed before it asserts (run with -s)."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import block_train_reference as br
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
DEPTH = 2
HD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_W = {}


def _weights(prec, dev):
    if prec not in _W:
        sd = synth.make_state_dict(NCLS, None, depth=DEPTH, seed=52)
        _W[prec] = (sd, engine.NetWeights.from_state_dict(sd, prec, dev))
    return _W[prec]


def _operand(w, p):
    """the tensor that owns the device memory the weight struct points at"""
    owner = [k for k in w.keep if isinstance(k, torch.Tensor) and k.data_ptr() == p]
    assert len(owner) == 1
    return owner[0]


def _check(name, dev_val, f32_val, f64_val, floor=FLOOR):
    e_dev, e_cpu = tr.rel_l2(dev_val, f64_val), tr.rel_l2(f32_val, f64_val)
    tol = max(4 * e_cpu, floor)
    print(f"  {name}: err(device) = {e_dev:.3e}, err(torch CPU float32) = {e_cpu:.3e}, tolerance = {tol:.3e}")
    return e_dev <= tol


def _net_forward(w, patches, nS, dev, depth=None):
    c, L = w.c, _lib.lib()
    ws = torch.full((L.cpx_net_workspace_bytes(nS, c.dtype),), 0xFF, dtype=torch.uint8, device=dev)
    head = torch.full((nS * 1024, c.ld_head), float("nan"), dtype=torch.float32, device=dev)
    full = c.depth
    c.depth = full if depth is None else depth
    try:
        _lib.check(L.cpx_net_forward(C.byref(c), ptr(patches), nS, ptr(head), ptr(ws), ws.numel(), torch.cuda.current_stream(dev).cuda_stream),
                   "net_forward")
    finally:
        c.depth = full
    return head, ops.backbone_rows(ws, nS, patches.dtype).clone()


def _rows_in(w, patches, nS, K, dev):
    """the input rows of block depth - K: the frozen prefix of cpx_net_forward, or the patch embedding's launch for K = depth"""
    c = w.c
    if K == c.depth:
        return ops.gemm(patches, _operand(w, c.pe_w), "pos", _operand(w, c.pe_b), _operand(w, c.pos))
    return _net_forward(w, patches, nS, dev, depth=c.depth - K)[1]


def _forward_train(w, x, K, dev):
    nS = x.shape[0] // 1024
    ws = ops.blocks_train_workspace(nS, w.c.dtype, K, dev)
    ws.fill_(0xFF)
    head = torch.full((x.shape[0], w.c.ld_head), float("nan"), dtype=torch.float32, device=dev)
    return ops.blocks_forward_train(w, x, w.c.depth - K, head=head, workspace=ws)


def _patches(nS, prec, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    return torch.randn(nS * 1024, 192, generator=g, device=dev).to(HD[prec])


# ---- 1. forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS", [1, 3])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_forward_train_is_bitwise_net_forward(cuda, prec, K, nS):
    sd, w = _weights(prec, cuda)
    patches = _patches(nS, prec, cuda, 3 + nS)
    head, x_last = _net_forward(w, patches, nS, cuda)
    x = _rows_in(w, patches, nS, K, cuda)
    o = _forward_train(w, x, K, cuda)
    torch.cuda.synchronize(cuda)
    same_head, same_x = torch.equal(o.head, head), torch.equal(o.x_out.view(torch.uint8), x_last.view(torch.uint8))
    b = w.blocks[DEPTH - K]
    rel_h, rel_w = _operand(w, b.rel_h), _operand(w, b.rel_w)
    same_ao = torch.equal(ops.attention(o.qkv[0].contiguous(), rel_h, rel_w).view(torch.uint8), o.ao[0].view(torch.uint8))
    same_in = torch.equal(o.x[0].view(torch.uint8), x.view(torch.uint8))
    if prec == "fp32":
        xn = ops.layernorm(x, _operand(w, b.ln1_w), _operand(w, b.ln1_b))
        qkv = ops.gemm(xn, _operand(w, b.qkv_w), "f32", _operand(w, b.qkv_b))
    else:
        vt = torch.full((nS * 1024, 1024), float("nan"), dtype=HD[prec], device=cuda)
        args = (_operand(w, b.qkv_w), "qkv", _operand(w, b.qkv_b), vt)
        if prec == "bf16":
            qkv = ops.gemm_ln(x, *args, ops.row_stats(x), _operand(w, b.qkv_colsum))
        else:                                                          # the product library's cpx_gemm_ln / cpx_row_stats are bf16: fp16 has
            with _lib.use_debug_library():                             # its entries in the -DCPX_DEBUG build of the same sources
                qkv = ops.gemm_ln(x, *args, ops.row_stats(x), _operand(w, b.qkv_colsum))
        # that epilogue writes the V third transposed into vt [crop][channel][token] instead of the rows; the kept rows hold it
        qkv[:, 2048:] = vt.view(nS, 1024, 1024).transpose(1, 2).reshape(nS * 1024, 1024)
    same_qkv = torch.equal(qkv.view(torch.uint8), o.qkv[0].view(torch.uint8))
    finite = all(bool(torch.isfinite(t.float()).all()) for ts in (o.x, o.qkv, o.ao, o.x_mid) for t in ts)
    print(f"{prec} K={K} nS={nS}: head equal {same_head}, last block's rows equal {same_x}, stored input equal {same_in}, "
          f"qkv == stand-alone GEMM {same_qkv}, ao == cpx_attention(qkv) {same_ao}, stored tensors finite {finite}")
    assert same_head and same_x and same_in and same_qkv and same_ao and finite and bool(torch.isfinite(head).all())


# ---- 2. attention backward ----------------------------------------------------------------------------------------
def _attn_case(nS, prec, seed, qscale=1.0):
    g = torch.Generator().manual_seed(seed)
    hd = HD[prec]
    qkv = torch.randn(nS * 1024, 3072, generator=g)
    qkv[:, :1024] *= qscale
    tab = lambda: torch.cat([torch.randn(63, 64, generator=g) * 0.5, torch.zeros(1, 64)]).to(hd)
    dO = torch.randn(nS * 1024, 1024, generator=g) * torch.logspace(-2, 0, 1024)[None]
    dO[::5] = 0
    return qkv.to(hd), tab(), tab(), dO


def _attn_run(qkv, Rh, Rw, dO, dev):
    nS = qkv.shape[0] // 1024
    q, h, w, d = (t.to(dev) for t in (qkv, Rh, Rw, dO))
    out = ops.attention(q, h, w)
    res = []
    for fill in (0xFF, 0x00):
        ws = ops.attention_backward_workspace(nS, dev)
        ws.fill_(fill)
        res.append(ops.attention_backward(q, h, w, out, d, ws))
    torch.cuda.synchronize(dev)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res))
    return res[0], same


@pytest.mark.parametrize("prec,qscale,nS", [(p, q, 1) for p in ("bf16", "fp16", "fp32") for q in (1.0, 7.5)] + [("bf16", 1.0, 3)])
def test_attention_backward_every_output(cuda, prec, qscale, nS):
    """A norm test: each of dq, dk, dv, dRel_h, dRel_w enters as ONE relative L2 norm over the whole tensor, so "every output" means each
    of the five tensors, not each element (dO is scaled by logspace(-2, 0) over the channels: head 0 holds 5e-5 of a tensor's energy,
    and a fault confined to it passes here).  The elements are checked in tests/test_gpu_attn_bwd_every_element.py.
    qscale 7.5: |q . k| reaches about 7.5 * 8 * 8 = 480 before the scale, logits of about +-60.  nS = 3 with dO in every crop: the
    table gradients are sums of the partials of three crops"""
    qkv, Rh, Rw, dO = _attn_case(nS, prec, 61, qscale)
    (dqkv, drh, drw), same = _attn_run(qkv, Rh, Rw, dO, cuda)
    r64 = br.attention_backward(qkv.double(), Rh.double(), Rw.double(), dO.double(), nS)
    r32 = br.attention_backward(qkv.float(), Rh.float(), Rw.float(), dO, nS)
    lg = br._logits(*br._split(qkv.double(), nS)[:2], Rh.double(), Rw.double(), nS) * br.SCALE
    print(f"attention backward {prec} qscale={qscale} nS={nS}: logits {float(lg.min()):.1f} .. {float(lg.max()):.1f}; two runs bitwise equal {same}")
    ok = [_check(n, dqkv[:, s].cpu(), r32["dqkv"][:, s], r64["dqkv"][:, s])
          for n, s in (("dq", slice(0, 1024)), ("dk", slice(1024, 2048)), ("dv", slice(2048, 3072)))]
    ok += [_check("dRel_h", drh.cpu(), r32["dRh"], r64["dRh"]), _check("dRel_w", drw.cpu(), r32["dRw"], r64["dRw"])]
    finite = all(bool(torch.isfinite(t).all()) for t in (dqkv, drh, drw))
    zero_dq = not bool(dqkv[::5, :1024].any())
    zero_pad = not bool(drh[63].any()) and not bool(drw[63].any())
    print(f"  finite {finite}; rows with dO = 0 give zero dq: {zero_dq}; row 63 of both table gradients zero: {zero_pad}")
    assert all(ok) and same and finite and zero_dq and zero_pad
    if qscale > 1:
        assert float(lg.abs().max()) > 40


def test_attention_backward_does_not_cross_a_crop_border(cuda):
    """dO non-zero in the middle crop of three only: the dqkv rows of crops 0 and 2 are exactly zero, and crop 1's are bitwise what the
    crop gives on its own (a crop's gradient is a function of that crop alone)"""
    prec = "bf16"
    qkv, Rh, Rw, dO = _attn_case(3, prec, 62)
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


# ---- 3. GELU and LayerNorm backward -------------------------------------------------------------------------------
def test_gelu_backward(cuda):
    pts = torch.tensor([0.0, 1e-30, -1e-30, 6.0, -6.0, 40.0, -40.0, 1.0], dtype=torch.float32)
    g = torch.Generator().manual_seed(63)
    x = torch.cat([pts, torch.randn(4096 - 8, generator=g) * 3])
    dh = torch.randn(4096, generator=g)
    dh[:8] = 1
    got = ops.gelu_backward(x.to(cuda), dh.to(cuda)).cpu()
    want = br.gelu_grad(x.double()) * dh.double()
    print(f"gelu' at 0, +-1e-30, +-6, +-40: {got[:7].tolist()}")
    assert bool(torch.isfinite(got).all())
    assert got[0] == 0.5 and got[1] == 0.5 and got[2] == 0.5 and got[5] == 1.0 and got[6] == 0.0
    assert abs(float(got[3]) - 1.0) < 1e-6 and abs(float(got[4])) < 1e-6
    x32 = x.clone().requires_grad_(True)
    F.gelu(x32).backward(dh)
    assert _check("dpre", got, x32.grad, want)


def _ln_case(rows, Cn, prec, seed):
    g = torch.Generator().manual_seed(seed)
    y = (torch.randn(rows, Cn, generator=g) * torch.logspace(-1, 1, rows)[:, None] + 0.5 * torch.randn(rows, 1, generator=g)).to(HD[prec])
    gamma = 1.0 + 0.3 * torch.randn(Cn, generator=g)
    dout = torch.randn(rows, Cn, generator=g) * torch.logspace(-3, 0, Cn)[None]
    dout[::7] = 0
    return y, gamma, dout


@pytest.mark.parametrize("rows,Cn", [(1024, 1024), (3072, 1024), (1000, 1024), (1024, 256)])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_layernorm_backward_every_element(cuda, prec, rows, Cn):
    """C = 1024 (and one C = 256 case, computed the same way before and after) against the float64 formula with 6l's element bound"""
    y, gamma, dout = _ln_case(rows, Cn, prec, rows + Cn)
    L = _lib.lib()
    nb = L.cpx_layernorm_backward_bytes(rows, Cn)
    assert nb > 0 and L.cpx_layernorm_backward_bytes(rows, 512) == 0
    yd, gd, dd = y.to(cuda), gamma.to(cuda), dout.to(cuda)
    outs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((nb,), fill, dtype=torch.uint8, device=cuda)
        dy = torch.full((rows, Cn), float("nan"), dtype=torch.float32, device=cuda)
        dg, db = (torch.full((Cn,), float("nan"), dtype=torch.float32, device=cuda) for _ in range(2))
        _lib.check(L.cpx_layernorm_backward(ops._DT[HD[prec]], ptr(yd), ptr(gd), ptr(dd), rows, Cn, 1e-6, ptr(dy), ptr(dg), ptr(db), ptr(ws),
                                            nb, torch.cuda.current_stream(cuda).cuda_stream), "layernorm_backward")
        outs.append((dy, dg, db))
    torch.cuda.synchronize(cuda)
    dy, dg, db = outs[0]
    r = nr.ln_backward(y, gamma, dout)
    print(f"LayerNorm backward {prec} rows={rows} C={Cn}:")
    worst = []
    for what, got, key in (("dy", dy, "dy"), ("dgamma", dg, "dgamma"), ("dbeta", db, "dbeta")):
        err, bound = (got.double().cpu() - r[key]).abs(), U * r[key].abs() + 2.0 ** -40 * r["S_" + key]
        worst.append(float((err / bound.clamp_min(1e-300)).max()))
        print(f"  {what}: worst error / bound = {worst[-1]:.3f}")
    zero_rows = not bool(dy[::7].any())
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs[0], outs[1]))
    print(f"  zero rows of dout give zero rows of dy: {zero_rows}; two runs bitwise equal: {same}")
    assert max(worst) <= 1.0 and zero_rows and same
    wy, wg, wb = ops.layernorm_backward(yd, gd, dd)
    assert torch.equal(wy, dy) and torch.equal(wg, dg) and torch.equal(wb, db)


# ---- 4. the backward, block by block ------------------------------------------------------------------------------
def _rounded_params(sd, prec, dev):
    """K = 2 records of the unfolded parameters as the forward reads them (what BlockParams.rounded holds)"""
    n, off = ops.block_grad_layout()
    flat = torch.zeros(DEPTH * n)
    for j in range(DEPTH):
        P = br.rounded(br.params_from_state_dict(sd, j), torch.float32, None if prec == "fp32" else HD[prec])
        for t, name in enumerate(br.NAMES):
            if not name.startswith("rel_"):
                flat[j * n + off[t]:j * n + off[t] + P[name].numel()] = P[name].reshape(-1)
    return flat.to(dev)


def _grad_views(grads, j):
    n, off = ops.block_grad_layout()
    return {k: grads[j * n + o:j * n + o + int(np.prod(s))].view(s) for k, o, s in zip(ops.BLOCK_GRAD_NAMES, off, ops.BLOCK_GRAD_SHAPES)}


def _table_grad(sd, j, name, g_operand):
    """the operand table's gradient [64, 64] -> the checkpoint's shape: the transpose of the interpolation, times 1 / scale"""
    n = sd[f"encoder.blocks.{j}.attn.{'rel_pos_h' if name == 'rel_h' else 'rel_pos_w'}"].shape[0]
    return 8.0 * br.interp_matrix(n).T @ g_operand.double()[:63]


def _run_backward(w, params, fwd, dy0, dev, want_dx=True):
    K, rows = len(fwd.x), fwd.x_out.shape[0]
    ws = ops.blocks_backward_workspace(rows // 1024, w.c.dtype, dev)
    ws.fill_(0xFF)
    n, _o = ops.block_grad_layout()
    grads = torch.full((K * n,), float("nan"), dtype=torch.float32, device=dev)
    dx = torch.full((K + 1, rows, 1024), float("nan"), dtype=torch.float32, device=dev) if want_dx else None
    ops.blocks_backward(w, params, fwd, dy0, grads, ws, dx)
    torch.cuda.synchronize(dev)
    return grads, dx


@pytest.mark.parametrize("prec,nS", [("fp32", 1), ("bf16", 3), ("fp16", 1)])
def test_backward_block_by_block(cuda, prec, nS):
    """K = 2: every block's every gradient and the data gradient handed to the block below, each block on the device's own stored
    tensors (its input rows, qkv, attention output and rows after the attention residual) and own incoming gradient"""
    sd, w = _weights(prec, cuda)
    block_by_block(cuda, prec, nS, sd, w, fold=True)


def block_by_block(cuda, prec, nS, sd, w, fold):
    """``fold``: how ``w`` was built (fuse_ln), hence how the float64 replay forms qkv and lin1 (tests/test_gpu_block_train_batches.py
    runs the half types with fuse_ln=False through here)"""
    net = None if prec == "fp32" else HD[prec]
    x = _rows_in(w, _patches(nS, prec, cuda, 13 + nS), nS, DEPTH, cuda)
    fwd = _forward_train(w, x, DEPTH, cuda)
    g = torch.Generator(device=cuda).manual_seed(17 + nS)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=cuda) * torch.logspace(-2, 0, 256, device=cuda)[None]
    params = _rounded_params(sd, prec, cuda)
    grads, dx = _run_backward(w, params, fwd, dy0, cuda)
    grads2, dx2 = _run_backward(w, params, fwd, dy0, cuda)
    same = torch.equal(grads.view(torch.int32), grads2.view(torch.int32)) and torch.equal(dx.view(torch.int32), dx2.view(torch.int32))
    finite = bool(torch.isfinite(grads).all()) and bool(torch.isfinite(dx).all())
    print(f"blocks backward {prec} nS={nS}: two runs bitwise equal {same}, everything finite {finite}")
    assert same and finite
    W0 = sd["encoder.neck.0.weight"].reshape(256, 1024).float().to(HD[prec])
    ok = [_check("d x_out = dy0 W0", dx[DEPTH].cpu(), dy0.cpu() @ W0.float(), dy0.double().cpu() @ W0.double())]
    for j in (1, 0):
        P = br.params_from_state_dict(sd, j)
        xin, dout = fwd.x[j].float().cpu(), dx[j + 1].cpu()
        free = br.block_grads(P, xin, dout, nS, torch.float64, net, fold)["fwd"]
        held = {"qkv": fwd.qkv[j].float().cpu(), "ao": fwd.ao[j].float().cpu(), "x_mid": fwd.x_mid[j].float().cpu()}
        print(f" block {j}: stored rows against the replay's own: " + ", ".join(f"{k} {tr.rel_l2(v, free[k]):.3e}" for k, v in held.items()))
        r64 = br.block_grads(P, xin, dout, nS, torch.float64, net, fold, stored=held)
        r32 = br.block_grads(P, xin, dout, nS, torch.float32, net, fold, stored=held)
        G = {k: v.cpu() for k, v in _grad_views(grads, j).items()}
        for k in br.NAMES:
            got = _table_grad(sd, j, k, G[k]) if k.startswith("rel_") else G[k]
            ok.append(_check(f"block {j} {k}", got, r32["grads"][k], r64["grads"][k]))
        ok.append(_check(f"block {j} dx", dx[j].cpu(), r32["dx"], r64["dx"]))
        assert not bool(G["rel_h"][63].any()) and not bool(G["rel_w"][63].any())
    assert all(ok)


# ---- 4b. the production shape: 32 crops -----------------------------------------------------------------------------
def test_thirty_two_crops_statistics_from_the_gemms_and_two_mlp_parts(cuda):
    """bf16, K = 1, 32 crops: cpx_net_forward takes every block's row statistics from the epilogue of the GEMM before it and runs the MLP in
    two row parts of 16 384; the training forward does the same, except that its first trained block takes its statistics from
    cpx_row_stats (the same sums in another order).
    Forward bound: the two statistics differ by float32 summation order (relative 2^-24 times a few), so qkv before rounding differs by about
    1e-7 of its size and a bf16 rounding (2^-9 relative) flips on about 1e-7 / 2^-9 = 5e-5 of the elements: sqrt(5e-5) * 2^-8 = 3e-5 in
    relative L2, and the flips it causes downstream are as rare.  The bound is one bf16 ulp, 2^-8, in relative L2, on the Q and K thirds of
    qkv (cpx_net_forward leaves them in its workspace), the last block's rows and the head: an order of magnitude of room, and two orders
    below what a wrong row part or wrong statistics give (O(1)).
    Backward: the parameter gradients at 32 crops against the float64 sum of the gradients of the sixteen two-crop runs on the same rows.
    The two-crop forwards use other GEMM kernels, so the stored tensors differ by independent bf16 roundings (2^-9 relative, on every
    element at worst); a gradient entry sums at least 1024 rows of such products, so its relative L2 error stays below 2^-9, and 2^-6 is
    the bound: a dropped or doubled slab, part or crop gives at least 1 / 32."""
    prec, nS, K = "bf16", 32, 1
    sd, w = _weights(prec, cuda)
    L, c = _lib.lib(), w.c
    assert L.cpx_net_mlp_parts(nS, c.dtype) == 2 and L.cpx_gemm_uses_big_tile(nS * 1024, 1024, 1024, ops.EPI["resid"]) == 1
    patches = _patches(nS, prec, cuda, 71)
    ws = torch.full((L.cpx_net_workspace_bytes(nS, c.dtype),), 0xFF, dtype=torch.uint8, device=cuda)
    head = torch.full((nS * 1024, c.ld_head), float("nan"), dtype=torch.float32, device=cuda)
    _lib.check(L.cpx_net_forward(C.byref(c), ptr(patches), nS, ptr(head), ptr(ws), ws.numel(), torch.cuda.current_stream(cuda).cuda_stream), "net_forward")
    x_last = ops.backbone_rows(ws, nS, HD[prec]).clone()
    qkv_off = nS * 1024 * 1024 * 2 * 2                                 # cpx_net_ws: x, xn, then qkv (256-byte aligned sizes)
    qkv_ref = ws[qkv_off:qkv_off + nS * 1024 * 3072 * 2].view(HD[prec]).view(nS * 1024, 3072)[:, :2048].float()
    del ws
    x = _rows_in(w, patches, nS, K, cuda)
    o = _forward_train(w, x, K, cuda)
    torch.cuda.synchronize(cuda)
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    e_qkv, e_x, e_head = rel(o.qkv[0][:, :2048], qkv_ref), rel(o.x_out, x_last), rel(o.head, head)
    finite = all(bool(torch.isfinite(t.float()).all()) for t in (o.qkv[0], o.ao[0], o.x_mid[0], o.x_out, o.head))
    print(f"32 crops: against cpx_net_forward qkv (Q, K) {e_qkv:.3e}, last block's rows {e_x:.3e}, head {e_head:.3e} (bound {2.0 ** -8:.3e}); finite {finite}")
    g = torch.Generator(device=cuda).manual_seed(72)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=cuda) * torch.logspace(-2, 0, 256, device=cuda)[None]
    params = _rounded_params(sd, prec, cuda)[ops.block_grad_layout()[0]:].contiguous()       # block 1's record
    grads, _dx = _run_backward(w, params, o, dy0, cuda, want_dx=False)
    grads_b, _dx = _run_backward(w, params, o, dy0, cuda, want_dx=False)
    same = torch.equal(grads.view(torch.int32), grads_b.view(torch.int32))
    total = torch.zeros(grads.numel(), dtype=torch.float64, device=cuda)
    del o
    for s0 in range(0, nS, 2):
        rows = slice(s0 * 1024, (s0 + 2) * 1024)
        o2 = _forward_train(w, x[rows].contiguous(), K, cuda)
        g2, _dx = _run_backward(w, params, o2, dy0[rows].contiguous(), cuda, want_dx=False)
        total += g2.double()
    ok = [e_qkv <= 2.0 ** -8, e_x <= 2.0 ** -8, e_head <= 2.0 ** -8, finite, same, bool(torch.isfinite(grads).all())]
    G, T = _grad_views(grads, 0), _grad_views(total, 0)
    for k in br.NAMES:
        e = float((G[k].double() - T[k]).norm() / T[k].norm())
        print(f"  {k}: 32 crops against the sum of sixteen two-crop runs {e:.3e} (bound {2.0 ** -6:.3e})")
        ok.append(e <= 2.0 ** -6)
    print(f"  two runs bitwise equal {same}")
    assert all(ok)


def test_trainer_rows_for_all_blocks_are_the_patch_embedding_of_net_forward(cuda):
    """K = depth: ``backbone_features`` launches the patch embedding itself; the trainer's forward on those rows is bitwise cpx_net_forward
    on the pixels.  K < depth runs a copy of the weight struct: the trainer's own keeps its depth"""
    for K in (DEPTH, 1):
        t, _sd = _trainer(cuda, "bf16", K, feature_batch=1)
        patches = _patches(1, "bf16", cuda, 73)
        x = t.backbone_features(patches)
        assert t.weights.c.depth == DEPTH
        head, _x = _net_forward(t.weights, patches, 1, cuda)
        got = t.evaluate(x, _labels(1, NCLS, 5), return_head=True)["head"]
        same = torch.equal(got, head)
        print(f"K = {K}: the trainer's head from its own cached rows equals cpx_net_forward bitwise: {same}")
        assert same


# ---- 5. end to end ------------------------------------------------------------------------------------------------
def _labels(n, ncls, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros((n, 256, 256), np.int16)
    for b in range(n):
        coarse = rng.integers(0, ncls, (16, 16))
        coarse.reshape(-1)[rng.permutation(256)[:ncls]] = np.arange(ncls)
        lab[b] = np.kron(coarse, np.ones((16, 16), np.int64))
        lab[b, 30 + 17 * b:][:9] = -100
        lab[b][rng.random((256, 256)) < 0.02] = -100
    return lab


def _targets(n, seed):
    g = torch.Generator().manual_seed(seed)
    mask = (torch.rand(n, 1, 16, 16, generator=g) > 0.5).float().repeat_interleave(16, 2).repeat_interleave(16, 3)
    flow = torch.tanh(F.interpolate(torch.randn(n, 2, 32, 32, generator=g), size=256, mode="bilinear")) * mask
    return torch.cat([mask, flow], 1).contiguous()


def _trainer(dev, prec, K, sd=None, seed=53, **kw):
    from classpose_amd.train import HeadTrainer
    sd = synth.make_state_dict(NCLS, None, depth=DEPTH, seed=seed) if sd is None else sd
    return HeadTrainer(sd, device=dev, precision=prec, train_blocks=K, **kw), sd


def _neck_views(grads):
    _n, off = ops.neck_grad_layout()
    return {k: grads[o:o + int(np.prod(s))].view(s) for k, o, s in zip(ops.NECK_GRAD_NAMES, off, ops.NECK_GRAD_SHAPES)}


@pytest.mark.parametrize("prec", ["fp32", "bf16", "fp16"])
def test_gradients_end_to_end(cuda, prec):
    """K = 2 blocks, the neck and both heads from labels and flow targets; the rel-pos gradients in the checkpoint's [27, 64] shape,
    through the interpolated table"""
    nS, K = 1, DEPTH
    t, sd = _trainer(cuda, prec, K, feature_batch=1, train_flow_head=True)
    assert t.neck is not None, "train_blocks implies train_neck"
    x = t.backbone_features(_patches(nS, prec, cuda, 23))
    labs, tg = _labels(nS, NCLS, 7), _targets(nS, 8)
    feat, head, o = t._loss(x, labs)
    seg = t._seg_loss(head, tg.to(cuda))
    t._neck_backward(*t._fwd, o, seg)
    t._blocks_backward()
    loss = float(o.ce.item()) + float(o.tversky.item()) + float(seg.flow.item()) + float(seg.cp.item())
    got_n = {k: v.clone().cpu() for k, v in _neck_views(t.neck.grads).items()}
    got_n["Wc"], got_n["bc"] = (v.cpu() for v in ops.head_wgrad(o.dlogits, feat))
    got_n["Wf"], got_n["bf"] = (v.cpu() for v in ops.head_wgrad(seg.dlogits, feat))
    net = None if prec == "fp32" else HD[prec]
    PB, PN = [br.params_from_state_dict(sd, j) for j in range(K)], nr.params_from_state_dict(sd)
    lab = torch.from_numpy(labs.astype(np.int64))
    r64 = br.loss_and_grads(PB, PN, x.float().cpu(), lab, tg, NCLS, torch.float64, net)
    r32 = br.loss_and_grads(PB, PN, x.float().cpu(), lab, tg, NCLS, torch.float32, net)
    print(f"{prec}: loss device {loss:.6f}, float64 {float(r64['loss']):.6f}, float32 {float(r32['loss']):.6f}")
    ok = [abs(loss - float(r64["loss"])) <= 1e-3 * abs(float(r64["loss"]))]
    for k in nr.NECK + nr.HEADS:
        ok.append(_check(k, got_n[k], r32["neck"][k], r64["neck"][k]))
    for j in range(K):
        for ti, k in enumerate(br.NAMES):
            got = t.blocks.rel_grads[j][ti - 4] if k.startswith("rel_") else t.blocks.view(j, ti, t.blocks.grads)
            assert got.shape == r64["blocks"][j][k].shape
            ok.append(_check(f"block {j} {k}", got.cpu(), r32["blocks"][j][k], r64["blocks"][j][k]))
    assert all(ok)


# ---- 6. training --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_twenty_steps(cuda, prec):
    """K = 1, the first epochs of the reference's schedule: lr = 0 changes nothing bitwise; fp32: the loss curve and the final update
    of every tensor follow the float64 replay by the rule; the loss goes down; two runs are bitwise equal"""
    from classpose_amd.train import lr_schedule
    nS, steps, K = 1, 20, 1
    labs, tg = _labels(nS, NCLS, 9), _targets(nS, 10)
    lrs = [float(v) for v in lr_schedule(2e-4, steps)[:steps]]
    runs = []
    for rep in range(2):
        t, sd = _trainer(cuda, prec, K, feature_batch=1, train_flow_head=True)
        x = t.backbone_features(_patches(nS, prec, cuda, 33))
        tgd = tg.to(cuda)
        P0, R0 = t.blocks.params.clone(), [[r.clone() for r in pair] for pair in t.blocks.rel]
        head0 = t.evaluate(x, labs, flow_targets=tgd, return_head=True)["head"].clone()
        losses = []
        for k, lr in enumerate(lrs):
            losses.append(t.step(x, labs, lr, flow_targets=tgd)["loss"])
            if k == 0:
                same_p = torch.equal(t.blocks.params.view(torch.int32), P0.view(torch.int32)) and \
                    all(torch.equal(a, b) for pa, pb in zip(R0, t.blocks.rel) for a, b in zip(pa, pb))
                same_h = torch.equal(t.evaluate(x, labs, flow_targets=tgd, return_head=True)["head"], head0)
                print(f"{prec}: after lr = 0 masters unchanged {same_p}, head unchanged {same_h}")
                assert same_p and same_h
        runs.append((np.array(losses), t.blocks.params.clone(), [r.clone() for r in t.blocks.rel[0]]))
        if rep == 0:
            first, x_cpu = t, x.float().cpu()
    (losses, pa, ra), (losses_b, pb, rb) = runs
    same_runs = bool((losses == losses_b).all()) and torch.equal(pa.view(torch.int32), pb.view(torch.int32)) and all(torch.equal(a, b) for a, b in zip(ra, rb))
    print(f"{prec}: loss step 1 = {losses[0]:.6f}, step {steps} = {losses[-1]:.6f}; first five {losses[:5].sum():.6f}, last five "
          f"{losses[-5:].sum():.6f}; two runs bitwise equal {same_runs}")
    assert same_runs and not torch.equal(pa, P0)
    t = first
    if prec == "fp32":
        PB, PN = [br.params_from_state_dict(sd, DEPTH - 1)], nr.params_from_state_dict(sd)
        lab = torch.from_numpy(labs.astype(np.int64))
        l64, b64, n64 = br.replay(PB, PN, x_cpu, lab, tg, NCLS, lrs, torch.float64, None, t.weight_decay)
        l32, b32, n32 = br.replay(PB, PN, x_cpu, lab, tg, NCLS, lrs, torch.float32, None, t.weight_decay)
        floor = steps * FLOOR
        ok = [_check("loss curve", losses, l32, l64, floor)]
        for ti, k in enumerate(br.NAMES):
            fin = t.blocks.rel[0][ti - 4] if k.startswith("rel_") else t.blocks.view(0, ti)
            ok.append(_check(f"final update of {k}", fin.cpu().double() - PB[0][k].double(), b32[0][k].double() - PB[0][k].double(),
                             b64[0][k] - PB[0][k].double(), floor))
        fin = {k: t.neck.view(i).cpu() for i, k in enumerate(nr.NECK)}
        fin.update(Wc=t.w.cpu(), bc=t.b.cpu(), Wf=t.flow.w.cpu(), bf=t.flow.b.cpu())
        for k in nr.NECK + nr.HEADS:
            ok.append(_check(f"final update of {k}", fin[k].double() - PN[k].double(), n32[k].double() - PN[k].double(), n64[k] - PN[k].double(), floor))
        assert all(ok) and l64[-5:].sum() < l64[:5].sum()
    assert losses[-5:].sum() < losses[:5].sum()


# ---- 7. off means off ---------------------------------------------------------------------------------------------
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


def test_train_blocks_zero_is_the_trainer_as_before(cuda):
    from classpose_amd.train import HeadTrainer
    from classpose_amd.train_unet import UNetHeadTrainer
    ims, labs, _inst = _crops(2)
    sd = synth.make_state_dict(NCLS, None, depth=DEPTH, seed=54)
    a = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=2, train_neck=True)
    b = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=2, train_neck=True, train_blocks=0)
    assert b.blocks is None and len(a.groups) == len(b.groups)
    x = a.backbone_features(ims)
    assert torch.equal(x, b.backbone_features(ims))
    for lr in (0.0, 1e-3, 2e-3):
        ra, rb = a.step(x, labs, lr), b.step(x, labs, lr)
        print(f"  lr {lr}: {ra} | {rb}")
        assert ra == rb
    assert a.step(ims, labs, 2e-3) == b.step(ims, labs, 2e-3)
    sa, sb = a.state_dict(), b.state_dict()
    assert set(sa) == set(sb) == set(sd) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert all(torch.equal(sb[k], sd[k]) for k in sd if k.startswith("encoder.blocks.")), "no block key changes when no block trains"
    with pytest.raises(NotImplementedError, match="train_blocks"):
        UNetHeadTrainer(sd, device=cuda, feature_transformation_structure=[16, 24], train_blocks=1)
    with pytest.raises(ValueError, match="train_blocks"):
        HeadTrainer(sd, device=cuda, train_blocks=DEPTH + 1)


# ---- 8. the checkpoint --------------------------------------------------------------------------------------------
def test_the_saved_checkpoint_loads_into_net_weights(cuda, tmp_path):
    from classpose_amd import augment
    ims, labs, inst = _crops(2)
    tg = torch.stack(augment.flow_targets_of(list(inst), cuda))
    t, sd = _trainer(cuda, "bf16", 1, seed=55, feature_batch=2, train_flow_head=True)
    x = t.backbone_features(ims)
    assert x.shape == (2 * 1024, 1024) and x.dtype == torch.bfloat16
    assert t.evaluate(x, labs, flow_targets=tg) == t.evaluate(ims, labs, flow_targets=tg), "cached rows and pixels give the same losses"
    for lr in (1e-3, 2e-3, 2e-3):
        t.step(x, labs, lr, flow_targets=tg)
    t.save(tmp_path / "blocks.pt")
    ck = torch.load(tmp_path / "blocks.pt", map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and all(ck[k].shape == sd[k].shape and ck[k].dtype == sd[k].dtype for k in sd)
    changed = {k for k in sd if not torch.equal(ck[k], sd[k])}
    want = {k for k in sd if k.startswith(f"encoder.blocks.{DEPTH - 1}.") or k.startswith("encoder.neck.")} | \
        {"out.weight", "out.bias", "out_class.weight", "out_class.bias"}
    print(f"changed keys: {len(changed)}; expected {len(want)}; unexpected {sorted(changed ^ want)}")
    assert changed == want
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    ev = t.evaluate(ims, labs, flow_targets=tg, return_head=True)["head"].clone()
    head, _x = _net_forward(w, t._patches(ims), 2, cuda)
    same = torch.equal(head[:, :192 + NCLS * 64], ev[:, :192 + NCLS * 64])
    print(f"cpx_net_forward on the saved checkpoint equals the trainer's head bitwise: {same}")
    assert same
    r, _ = _trainer(cuda, "bf16", 1, sd=ck, feature_batch=2, train_flow_head=True)
    assert torch.equal(r.blocks.params, t.blocks.params) and torch.equal(r.blocks.rel[0][0], t.blocks.rel[0][0])
    from classpose_amd.models import ClassposeModel
    m = ClassposeModel(gpu=True, pretrained_model=str(tmp_path / "blocks.pt"), device=cuda, nclasses=NCLS, precision="bf16")
    assert m is not None


# ---- 9. the command line ------------------------------------------------------------------------------------------
def _cli(tmp_path, *extra):
    return ["timeout", "-k", "10", "300", sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--data_path", str(tmp_path / "data"),
            "--train_fraction", "1", "--pretrained_model", str(tmp_path / "backbone.pt"), "--nclasses", "3", "--n_epochs", "2", "--batch_size", "2",
            "--learning_rate", "1e-3", "--save_path", str(tmp_path), "--model_name", "m", "--device", "cuda:0", *extra]


def test_cli_train_blocks_in_a_child_process(cuda, tmp_path):
    sd = synth.make_state_dict(1, None, depth=DEPTH, seed=56)
    torch.save(sd, tmp_path / "backbone.pt")
    d = tmp_path / "data"
    d.mkdir()
    imgs, labs = np.empty(2, dtype=object), np.empty(2, dtype=object)
    for k, (h, wd) in enumerate([(512, 256), (256, 512)]):              # two crops each: four crops
        inst = np.zeros((h, wd), np.int32)
        inst[:256, :256] = fr.disc_crop(70 + k)
        imgs[k] = synth.render_region(300, 64 * k, 32 * k, wd, h)
        labs[k] = np.stack([inst, np.where(inst > 0, 1 + inst % 2, 0).astype(np.int32)], -1)
    np.save(d / "images.npy", imgs, allow_pickle=True)
    np.save(d / "labels.npy", labs, allow_pickle=True)
    r = subprocess.run(_cli(tmp_path, "--train_blocks", "1", "--train_flow_head"), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    assert "turns --train_neck on" in r.stdout + r.stderr and "backbone rows" in r.stdout + r.stderr
    ck = torch.load(out, map_location="cpu", weights_only=True)
    last = [k for k in sd if k.startswith(f"encoder.blocks.{DEPTH - 1}.")]
    first = [k for k in sd if k.startswith("encoder.blocks.0.")]
    print(f"{len(last)} keys of the trained block, {len(first)} of the frozen one")
    assert len(last) == 14 and all(ck[k].shape == sd[k].shape and not torch.equal(ck[k], sd[k]) for k in last)
    assert all(torch.equal(ck[k], sd[k]) for k in first)
    assert engine.NetWeights.from_state_dict(ck, "bf16", cuda).ncls == 3
    r = subprocess.run(_cli(tmp_path, "--train_blocks", "1", "--feature_transformation_structure", "16", "24"), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "UNet class head" in r.stderr and "--train_blocks" in r.stderr
    r = subprocess.run(_cli(tmp_path, "--train_blocks", str(DEPTH + 1)), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "--train_blocks" in r.stderr and "blocks" in r.stderr
    r = subprocess.run(_cli(tmp_path, "--train_blocks", "1", "--freeze", "backbone", "neck"), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "--train_blocks contradicts --freeze" in r.stderr and "--train_neck contradicts" not in r.stderr
    r = subprocess.run(_cli(tmp_path, "--freeze", "none"), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "--freeze none" in r.stderr and "is not built" in r.stderr
