"""The bf16 gradient mode of block training: cpx_gemm_tn_bf16 (csrc/cpx_gemm_tn.hip), the row-parallel column sums, the
operand rounding, the data-gradient route through cpx_gemm_half with contraction length 3072, cpx_blocks_backward_ex in both modes,
HeadTrainer(grad_precision="bf16") and train_head --grad_precision bf16.  The network is synth.make_state_dict(3, None, depth=2) and the
helpers are those of tests/test_gpu_block_train.py and tests/test_gpu_block_train_batches.py.

Bounds, all derived and none measured:
  * integer operands in {-2 .. 2}: every product and every partial sum is an integer below 2^24, so any order of float32 additions is
    exact: torch.equal with the CPU product.
  * random bf16 operands: a product of two bf16 values has 16 significant bits and is exact in float32, so only the additions round; a
    sum of L terms in any order, plus the one addition of the previous value and the final write, obeys
    |got - exact| <= (L + 2) 2^-24 (sum |a||b| + |prev|), exact in float64.
  * column sums in float64, rounded once: |got - exact| <= 2^-24 |exact| + 2^-40 sum |dy|.
  * the backward as a whole: the project's rule err(device) <= max(4 err(CPU float32), 2^-20) against the float64 replay WITHOUT
    roundings, where the CPU float32 comparator is tests/block_train_bf16_reference.py with the roundings -- never the device.
Every output and workspace is poisoned before the call that fills it; every test prints what it observed before it asserts."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import block_train_bf16_reference as b16
import block_train_reference as br
import flow_train_reference as fr
import test_gpu_block_train as bt
import test_gpu_block_train_batches as bb
from classpose_amd import _lib, engine, ops, synth
from classpose_amd._lib import ptr
from test_gpu_block_train import DEPTH, NCLS, ROOT, _check, _forward_train, _grad_views, _patches, _rounded_params, _rows_in, _table_grad

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
EINVAL = -22
BF, F32 = torch.bfloat16, torch.float32


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


# ---- 1. cpx_gemm_tn_bf16 ------------------------------------------------------------------------------------------
def _tn(a, b, out, add, ld=None):
    N, K = a.shape[1], b.shape[1]
    return _lib.lib().cpx_gemm_tn_bf16(ptr(a), ptr(b), a.shape[0], N, K, add, ptr(out), out.stride(0) if ld is None else ld, _stream(a.device))


_INT = {}


def _int_case(M, N, K):
    """integer operands and their exact float32 product, computed once"""
    if (M, N, K) not in _INT:
        g = torch.Generator().manual_seed(M + N + K)
        a, b = (torch.randint(-2, 3, (M, n), generator=g).float() for n in (N, K))
        _INT[(M, N, K)] = (a, b, a.T @ b)
    return _INT[(M, N, K)]


SHAPES = [(1024, 3072, 1024), (1024, 1024, 1024), (1024, 4096, 1024), (1024, 1024, 4096), (2048, 4096, 1024), (2048, 1024, 4096)]


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_tn_exact_on_integers(cuda, M, N, K):
    a, b, want = _int_case(M, N, K)
    ad, bd = a.to(cuda).to(BF), b.to(cuda).to(BF)
    assert float(want.abs().max()) < 2 ** 24
    out = torch.full((N, K), float("nan"), device=cuda)
    assert _tn(ad, bd, out, 0) == 0
    plain = torch.equal(out.cpu(), want)
    prev = torch.randint(-1000, 1000, (N, K), generator=torch.Generator().manual_seed(5)).float()
    acc = prev.to(cuda)
    assert _tn(ad, bd, acc, 1) == 0
    added = torch.equal(acc.cpu(), want + prev)
    pad = 64                                                            # ld_out > K: the columns beyond K keep their poison
    wide = torch.full((N, K + pad), float("nan"), device=cuda)
    assert _tn(ad, bd, wide[:, :K], 0) == 0 and wide.stride(0) == K + pad
    torch.cuda.synchronize(cuda)
    padded = torch.equal(wide[:, :K].cpu(), want) and bool(torch.isnan(wide[:, K:]).all())
    w2 = ops.gemm_tn_bf16(ad, bd)
    print(f"tn GEMM M={M} N={N} K={K}: max |product| {float(want.abs().max()):.0f}; add = 0 on NaN exact {plain}; add = 1 exact {added}; "
          f"ld_out = K + {pad} exact with the padding untouched {padded}")
    assert plain and added and padded and torch.equal(w2, out)


def _spread(shape, g):
    """bf16 values with exponents spread over 2^-8 .. 2^8"""
    return (torch.randn(shape, generator=g) * torch.exp2(torch.randint(-8, 9, shape, generator=g).float())).to(BF)


def _element_bound(got, a, b, prev, L):
    exact = a.double().T @ b.double() + prev.double()
    S = a.double().abs().T @ b.double().abs() + prev.double().abs()
    return float(((got.double() - exact).abs() / ((L + 2) * U * S).clamp_min(1e-300)).max())


@pytest.mark.parametrize("M,N,K", [(1024, 1024, 1024), (2048, 1024, 1024), (1024, 4096, 1024)])
def test_gemm_tn_every_element(cuda, M, N, K):
    g = torch.Generator().manual_seed(7 * M + N)
    a, b = _spread((M, N), g), _spread((M, K), g)
    prev = torch.randn(N, K, generator=g) * 100
    out = torch.full((N, K), float("nan"), device=cuda)
    acc = prev.to(cuda)
    assert _tn(a.to(cuda), b.to(cuda), out, 0) == 0 and _tn(a.to(cuda), b.to(cuda), acc, 1) == 0
    torch.cuda.synchronize(cuda)
    w0, w1 = _element_bound(out.cpu(), a, b, torch.zeros(N, K), M), _element_bound(acc.cpu(), a, b, prev, M)
    print(f"tn GEMM M={M} N={N} K={K}, random bf16: worst error / bound {w0:.4f} (add = 0), {w1:.4f} (add = 1)")
    assert bool(torch.isfinite(out).all()) and w0 <= 1.0 and w1 <= 1.0


def test_gemm_tn_refuses_what_the_header_excludes(cuda):
    a, b = torch.ones(128, 256, dtype=BF, device=cuda), torch.ones(128, 256, dtype=BF, device=cuda)
    out = torch.full((256 * 257 + 8,), float("nan"), device=cuda)
    L, s = _lib.lib(), _stream(cuda)
    good = (ptr(a), ptr(b), 128, 128, 128, 0, ptr(out), 128)
    cases = {"M not a multiple of 64": (2, 96), "M zero": (2, 0), "N not a multiple of 128": (3, 64), "K not a multiple of 128": (4, 192),
             "ld_out < K": (7, 127), "add neither 0 nor 1": (5, 2), "A null": (0, None), "B null": (1, None), "out null": (6, None),
             "A not 16-byte aligned": (0, ptr(a) + 2), "B not 16-byte aligned": (1, ptr(b) + 8), "out not 16-byte aligned": (6, ptr(out) + 4)}
    seen = {}
    for what, (i, v) in cases.items():
        args = list(good)
        args[i] = v
        seen[what] = L.cpx_gemm_tn_bf16(*args, s)
    torch.cuda.synchronize(cuda)
    untouched = bool(torch.isnan(out).all())
    print(f"refusals: {seen}; out keeps its poison: {untouched}")
    assert all(rc == EINVAL for rc in seen.values()) and untouched
    assert L.cpx_gemm_tn_bf16(*good, s) == 0
    torch.cuda.synchronize(cuda)
    assert torch.equal(out[:128 * 128], torch.full((128 * 128,), 128.0, device=cuda)) and bool(torch.isnan(out[128 * 128:]).all())


# ---- 2. the data-gradient route: cpx_gemm_half, float32 epilogue, contraction length 3072 -------------------------------
@pytest.mark.parametrize("M", [1024, 2048])
def test_gemm_half_contraction_3072_every_element(cuda, M):
    """da = bf16(dqkv) Wqkv: no forward GEMM has this contraction length.  The float32 epilogue always takes the 128^2 kernel."""
    L, N, Kc = _lib.lib(), 1024, 3072
    band = L.cpx_gemm_uses_big_tile(M, N, Kc, ops.EPI["f32"])
    print(f"contraction 3072, M={M}: 256^2 kernel {band}")
    assert band == 0
    g = torch.Generator().manual_seed(31 + M)
    a, wt = _spread((M, Kc), g), _spread((N, Kc), g)
    out = torch.full((M, N), float("nan"), device=cuda)
    ad, wd = a.to(cuda), wt.to(cuda)
    _lib.check(L.cpx_gemm(_lib.DT_BF16, ptr(ad), ptr(wd), M, N, Kc, ops.EPI["f32"], None, None, ptr(out), N, _stream(cuda)), "gemm")
    torch.cuda.synchronize(cuda)
    worst = _element_bound(out.cpu(), a.T.contiguous(), wt.T.contiguous(), torch.zeros(M, N), Kc)
    print(f"  worst error / bound {worst:.4f}")
    assert bool(torch.isfinite(out).all()) and worst <= 1.0


# ---- 3. column sums and the operand rounding ----------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1024, 2048])
@pytest.mark.parametrize("N", [1024, 3072, 4096])
def test_colsum_every_column(cuda, N, rows):
    g = torch.Generator().manual_seed(N + rows)
    dy = torch.randn(rows, N, generator=g) * torch.exp2(torch.randint(-10, 11, (rows, N), generator=g).float())
    db0 = torch.randn(N, generator=g) * 50
    S = dy.double().abs().sum(0)
    worst = []
    for start in (torch.zeros(N), db0):
        ws = torch.full((_lib.lib().cpx_colsum_workspace_bytes(rows, N),), 0xFF, dtype=torch.uint8, device=cuda)
        db = start.to(cuda)
        ops.colsum_add(dy.to(cuda), db, ws)
        again = ops.colsum_add(dy.to(cuda), start.to(cuda))
        exact = start.double() + dy.double().sum(0)
        worst.append(float(((db.cpu().double() - exact).abs() / (U * exact.abs() + 2.0 ** -40 * S)).max()))
        assert torch.equal(db, again), "two runs are bitwise equal"
    print(f"column sums rows={rows} N={N}: worst error / bound {worst[0]:.4f} (from zero), {worst[1]:.4f} (on top of db)")
    assert max(worst) <= 1.0
    assert _lib.lib().cpx_colsum_add(ptr(dy.to(cuda)), rows - 1, N, ptr(db), ptr(ws), ws.numel(), _stream(cuda)) == EINVAL


def test_operand_rounding_is_torch_bfloat16(cuda):
    """cpx_round_weights, the producer of every bf16 operand of the mode: round to nearest even, bit for bit x.to(torch.bfloat16)"""
    special = torch.tensor([0.0, -0.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -7 + 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -8 + 2.0 ** -23, 2.0 ** -133, 3 * 2.0 ** -134,
                            2.0 ** -134, 2.0 ** -149, -2.0 ** -140, 2.0 ** -126, 3.3895313892515355e38, -3.3895313892515355e38, 3.3961775292304446e38,
                            3.4028234663852886e38, float("inf"), -float("inf")], dtype=F32)
    g = torch.Generator().manual_seed(41)
    x = torch.cat([special, torch.randn(4096 + 3, generator=g) * torch.exp2(torch.randint(-140, 120, (4099,), generator=g).float())]).to(cuda)
    dst = torch.full((x.numel() + 8,), -1, dtype=torch.int16, device=cuda)
    ops.round_weights(x, dst.data_ptr(), _lib.DT_BF16, False)
    torch.cuda.synchronize(cuda)
    want = x.cpu().to(BF).view(torch.int16).to(cuda)
    bad = (dst[:x.numel()] != want).nonzero().flatten().tolist()
    print(f"rounding of {x.numel()} values, {len(special)} special: differing from torch {bad[:8]}; beyond the end untouched {bool((dst[x.numel():] == -1).all())}")
    assert not bad and bool((dst[x.numel():] == -1).all())


# ---- 4. the backward ------------------------------------------------------------------------------------------------------
def _run(w, params, fwd, dy0, dev, grad_dtype, want_dx=True, fill=0xFF):
    K, rows = len(fwd.x), fwd.x_out.shape[0]
    ws = ops.blocks_backward_workspace(rows // 1024, w.c.dtype, dev, grad_dtype)
    ws.fill_(fill)
    n, _o = ops.block_grad_layout()
    grads = torch.full((K * n,), float("nan"), dtype=F32, device=dev)
    dx = torch.full((K + 1, rows, 1024), float("nan"), dtype=F32, device=dev) if want_dx else None
    ops.blocks_backward(w, params, fwd, dy0, grads, ws, dx, grad_dtype=grad_dtype)
    torch.cuda.synchronize(dev)
    return grads, dx


@pytest.mark.parametrize("fused", [True, False])
def test_bf16_backward_block_by_block(cuda, fused):
    """nS = 3 (a slab of two crops and a remainder), K = 2: every gradient of every block and every dx record, each block on the device's
    own stored tensors and incoming gradient.  q64: float64 autograd without roundings; the comparator: the CPU restatement in float32
    with the roundings."""
    prec, nS, net = "bf16", 3, BF
    sd, w = bb._weights_for(prec, fused, cuda)
    x = _rows_in(w, _patches(nS, prec, cuda, 13 + nS), nS, DEPTH, cuda)
    fwd = _forward_train(w, x, DEPTH, cuda)
    g = torch.Generator(device=cuda).manual_seed(17 + nS)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=cuda) * torch.logspace(-2, 0, 256, device=cuda)[None]
    params = _rounded_params(sd, prec, cuda)
    grads, dx = _run(w, params, fwd, dy0, cuda, BF)
    finite = bool(torch.isfinite(grads).all()) and bool(torch.isfinite(dx).all())
    print(f"bf16 gradients, fuse_ln={fused}, nS={nS}: everything finite {finite}")
    assert finite
    W0 = sd["encoder.neck.0.weight"].reshape(256, 1024).float().to(net)
    ok = [_check("d x_out = bf16(dy0) W0", dx[DEPTH].cpu(), b16.top_backward(dy0.cpu(), W0.float(), b16.round_bf16), dy0.double().cpu() @ W0.double())]
    for j in (1, 0):
        P = br.params_from_state_dict(sd, j)
        xin, dout = fwd.x[j].float().cpu(), dx[j + 1].cpu()
        held = {"qkv": fwd.qkv[j].float().cpu(), "ao": fwd.ao[j].float().cpu(), "x_mid": fwd.x_mid[j].float().cpu()}
        r64 = br.block_grads(P, xin, dout, nS, torch.float64, net, fused, stored=held)
        r32 = b16.block_backward(P, xin, dout, nS, F32, net, fused, stored=held, rnd=b16.round_bf16)
        G = {k: v.cpu() for k, v in _grad_views(grads, j).items()}
        for k in br.NAMES:
            got = _table_grad(sd, j, k, G[k]) if k.startswith("rel_") else G[k]
            ok.append(_check(f"block {j} {k}", got, r32["grads"][k], r64["grads"][k]))
        ok.append(_check(f"block {j} dx", dx[j].cpu(), r32["dx"], r64["dx"]))
        assert not bool(G["rel_h"][63].any()) and not bool(G["rel_w"][63].any())
    assert all(ok)


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_fp32_mode_is_cpx_blocks_backward(cuda, prec):
    nS = 3
    sd, w = bt._weights(prec, cuda)
    L, c = _lib.lib(), w.c
    x = _rows_in(w, _patches(nS, prec, cuda, 21), nS, DEPTH, cuda)
    fwd = _forward_train(w, x, DEPTH, cuda)
    dy0 = torch.randn(nS * 1024, 256, generator=torch.Generator(device=cuda).manual_seed(22), device=cuda)
    params = _rounded_params(sd, prec, cuda)
    grads, dx = _run(w, params, fwd, dy0, cuda, F32)
    nb, nb_ex = L.cpx_blocks_backward_workspace_bytes(nS, c.dtype), L.cpx_blocks_backward_workspace_bytes_ex(nS, c.dtype, _lib.DT_F32)
    ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=cuda)
    g2, dx2 = torch.full_like(grads, float("nan")), torch.full_like(dx, float("nan"))
    _lib.check(L.cpx_blocks_backward(C.byref(c), ptr(params), nS, fwd.first_block, ptr(fwd.workspace), fwd.workspace.numel(), ptr(dy0), ptr(g2),
                                     ptr(dx2), ptr(ws), nb, _stream(cuda)), "blocks_backward")
    torch.cuda.synchronize(cuda)
    same = torch.equal(grads, g2) and torch.equal(dx, dx2)
    print(f"{prec}: cpx_blocks_backward_ex(CPX_DT_F32) equals cpx_blocks_backward on every gradient and dx record: {same}; workspace {nb_ex} == {nb}")
    assert same and nb == nb_ex and bool(torch.isfinite(grads).all())
    with pytest.raises(ValueError, match="bf16 network"):
        if prec == "fp32":
            ops.blocks_backward(w, params, fwd, dy0, grad_dtype=BF)
        else:
            ops.blocks_backward(bt._weights("fp16", cuda)[1], params, fwd, dy0, grad_dtype=BF)
    with pytest.raises(ValueError, match="grad_dtype is"):
        ops.blocks_backward(w, params, fwd, dy0, grad_dtype=torch.float16)


@pytest.mark.parametrize("slab", [0, 1])
def test_bf16_backward_of_one_hot_slab_equals_the_slab_alone(cuda, slab):
    """nS = 3, K = 1, dy0 non-zero in slab 0 (two crops) or in the one-crop remainder: the other slab adds exact zeros to every sum, so
    all 14 gradient tensors and the slab's dx rows equal the backward of the slab alone on a record holding only its rows"""
    nS, K = 3, 1
    w, o, dy0, params = bb._backward_case(cuda, "bf16", True, nS, K, 120 + slab)
    hot, mask = bb._hot(dy0, [slab], nS)
    c0 = slab * bb.SLAB
    nc = min(bb.SLAB, nS - c0)
    assert int(mask.sum()) == nc * 1024 and nc == (2, 1)[slab]
    grads, dx = _run(w, params, o, hot, cuda, BF)
    alone, dx1 = _run(w, params, bb._slab_record(w, o, c0, nc, cuda), hot[mask].contiguous(), cuda, BF)
    G, A = _grad_views(grads, 0), _grad_views(alone, 0)
    diff = [k for k in G if not torch.equal(G[k], A[k])]
    same_dx, zero_dx = torch.equal(dx[:, mask], dx1), not bool(dx[:, ~mask].any())
    live = float(dx1.abs().max()) > 0 and all(float(v.abs().max()) > 0 for v in A.values())
    print(f"bf16 gradients, slab {slab} ({nc} crop(s)) hot: tensors that differ from the slab alone: {diff or 'none'} of {len(G)}; the slab's dx rows "
          f"equal {same_dx}; every other dx row zero {zero_dx}")
    assert len(G) == 14 and not diff and same_dx and zero_dx and live and bool(torch.isfinite(grads).all())


def test_bf16_backward_is_bitwise_reproducible(cuda):
    nS = 3
    w, o, dy0, params = bb._backward_case(cuda, "bf16", True, nS, DEPTH, 140)
    a, dxa = _run(w, params, o, dy0, cuda, BF, fill=0xFF)
    b, dxb = _run(w, params, o, dy0, cuda, BF, fill=0x00)
    same = torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(dxa.view(torch.int32), dxb.view(torch.int32))
    f32, _dx = _run(w, params, o, dy0, cuda, F32, want_dx=False)
    away = float((a - f32).norm() / f32.norm())
    print(f"two bf16-mode backwards bitwise equal: {same}; distance from the float32 mode {away:.3e}")
    assert same and bool(torch.isfinite(a).all()) and 0 < away < 2.0 ** -5


# ---- 5. the trainer and the command line ----------------------------------------------------------------------------------
def test_trainer_twenty_steps_in_both_modes(cuda, tmp_path):
    from classpose_amd.train import HeadTrainer, lr_schedule
    nS, steps = 2, 20
    labs, tg = bt._labels(nS, NCLS, 9), bt._targets(nS, 10).to(cuda)
    lrs = [float(v) for v in lr_schedule(2e-4, steps)[:steps]]
    curves = {}
    for mode in ("fp32", "bf16"):
        t, sd = bt._trainer(cuda, "bf16", 1, feature_batch=nS, train_flow_head=True, grad_precision=mode)
        assert t.grad_precision == mode
        x = t.backbone_features(_patches(nS, "bf16", cuda, 33))
        curves[mode] = np.array([t.step(x, labs, lr, flow_targets=tg)["loss"] for lr in lrs])
    for k in range(steps):
        print(f"  step {k + 1:2d}: fp32 gradients {curves['fp32'][k]:.6f}   bf16 gradients {curves['bf16'][k]:.6f}")
    dist = float(np.abs(curves["bf16"] - curves["fp32"]).max() / np.abs(curves["fp32"]).max())
    print(f"largest distance of the two loss curves, relative to the largest loss: {dist:.3e}")
    for mode, c in curves.items():
        assert np.isfinite(c).all() and c[-1] < c[0], mode
    t.save(tmp_path / "bf16grad.pt")
    ck = torch.load(tmp_path / "bf16grad.pt", map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and all(ck[k].shape == sd[k].shape and ck[k].dtype == sd[k].dtype for k in sd)
    assert engine.NetWeights.from_state_dict(ck, "bf16", cuda).ncls == NCLS
    changed = [k for k in sd if k.startswith(f"encoder.blocks.{DEPTH - 1}.") and not torch.equal(ck[k], sd[k])]
    assert len(changed) == 14
    for kw, what in ((dict(precision="fp16", train_blocks=1), "loss scaling"), (dict(precision="bf16", train_blocks=0), "train_blocks > 0"),
                     (dict(precision="fp32", train_blocks=1), "no half-precision")):
        with pytest.raises(ValueError, match=what):
            HeadTrainer(sd, device=cuda, grad_precision="bf16", **kw)


def test_cli_grad_precision_bf16_in_a_child_process(cuda, tmp_path):
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
    r = subprocess.run(bt._cli(tmp_path, "--train_blocks", "1", "--grad_precision", "bf16", "--precision", "bf16"), cwd=ROOT, capture_output=True,
                       text=True)
    print(r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    ck = torch.load(out, map_location="cpu", weights_only=True)
    last = [k for k in sd if k.startswith(f"encoder.blocks.{DEPTH - 1}.")]
    assert len(last) == 14 and all(ck[k].shape == sd[k].shape and not torch.equal(ck[k], sd[k]) and bool(torch.isfinite(ck[k]).all()) for k in last)
    assert all(torch.equal(ck[k], sd[k]) for k in sd if k.startswith("encoder.blocks.0."))
    assert engine.NetWeights.from_state_dict(ck, "bf16", cuda).ncls == 3
