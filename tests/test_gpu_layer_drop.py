"""Layer drop (stochastic depth) for the trained blocks on the device: the compaction kernels (cpx_gather_crops /
cpx_scatter_crops), cpx_blocks_forward_train_drop, cpx_blocks_backward_drop, HeadTrainer(layer_drop=...) / step(keep=...) and train_head
--layer_drop.  The network is synth.make_state_dict(3, None, depth=2) and the helpers are those of tests/test_gpu_block_train.py.

Masks are written keep[block][crop], 1 = the block runs on the crop.  What is bitwise: a dropped crop's rows and gradient rows pass
through untouched; a block's kept rows are what the existing forward gives for that block alone on the gathered crops; all ones and no
mask are the existing entries.  What is not: every gradient, held to the project's rule
    err(device) <= max(4 * err(torch CPU float32), 2^-20),  err(x) = ||x - q64||_2 / ||q64||_2
against the float64 replay on the device's own stored tensors, the comparator in the bf16 gradient modes carrying the same roundings.
Crop counts: 3 (a slab of two and a remainder; the masks give slabs with two, one -- either half -- and no kept crop) and 4 (two full
slabs; block 1 keeps one whole slab and drops the other).  Every output and workspace is poisoned (0xFF bytes, NaN) before the call
that fills it; every test prints what it observed before it asserts (run with -s)."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np
import pytest
import torch

import attn_bwd_bf16_reference as ab
import block_train_bf16_reference as b16
import block_train_reference as br
import embed_train_reference as er
import flow_train_reference as fr
import layer_drop_reference as ldr
import neck_train_reference as nr
import test_gpu_block_train as bt
from classpose_amd import _lib, engine, ops, synth
from classpose_amd._lib import ptr
from test_gpu_block_train import DEPTH, FLOOR, HD, NCLS, ROOT, _check, _forward_train, _grad_views, _labels, _neck_views, _patches, _rounded_params, _rows_in, _table_grad, _targets

pytestmark = pytest.mark.gpu
EINVAL = -22
BF, F32 = torch.bfloat16, torch.float32
MASKS = {3: [[1, 0, 1], [0, 1, 1]], 4: [[0, 1, 1, 1], [1, 1, 0, 0]]}
MODES = {"fp32": ("fp32", F32, F32), "bf16": ("bf16", F32, F32), "bf16+bf16": ("bf16", BF, BF)}


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _bits(t):
    return t.contiguous().view(torch.uint8)


def _crops_of(t, idx):
    """the rows of the crops ``idx`` of full rows ``t``, compact"""
    n = t.shape[0] // 1024
    return t.view(n, 1024, -1)[torch.as_tensor(idx, dtype=torch.long, device=t.device)].reshape(len(idx) * 1024, t.shape[1])


def _forward_drop(w, x, K, keep, dev):
    nS = x.shape[0] // 1024
    ws = ops.blocks_train_workspace(nS, w.c.dtype, K, dev, drop=True)
    ws.fill_(0xFF)
    head = torch.full((x.shape[0], w.c.ld_head), float("nan"), dtype=F32, device=dev)
    return ops.blocks_forward_train(w, x, w.c.depth - K, head=head, workspace=ws, keep=None if keep is None else np.asarray(keep, np.uint8))


def _backward(w, params, fwd, dy0, dev, gd=F32, ad=F32, want_in=False):
    K, rows = len(fwd.x), fwd.x_out.shape[0]
    ws = ops.blocks_backward_workspace(rows // 1024, w.c.dtype, dev, gd, ad)
    ws.fill_(0xFF)
    n, _o = ops.block_grad_layout()
    grads = torch.full((K * n,), float("nan"), dtype=F32, device=dev)
    dx = torch.full((K + 1, rows, 1024), float("nan"), dtype=F32, device=dev)
    dx_in = torch.full((rows, 1024), float("nan"), dtype=F32, device=dev) if want_in else None
    ops.blocks_backward(w, params, fwd, dy0, grads, ws, dx, grad_dtype=gd, attn_grad_dtype=ad, dx_in=dx_in)
    torch.cuda.synchronize(dev)
    return grads, dx, dx_in


# ---- 1. compaction ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_compaction_every_element(cuda, prec):
    """5 crops; the lists [0..4] (everything), [1, 2, 4] (a gap and the last crop), [4] and [].  Every element of the gathered rows is the
    source's, the statistics are bitwise cpx_row_stats of the gathered rows, the scatter changes the listed crops and nothing else of a
    destination filled with 0xA5 bytes; a list that is unordered, repeats a crop or leaves the buffer is CPX_EINVAL and changes nothing"""
    nS, hd, L = 5, HD[prec], _lib.lib()
    g = torch.Generator(device=cuda).manual_seed(91)
    src = (torch.randn(nS * 1024, 1024, generator=g, device=cuda) * torch.logspace(-2, 2, 1024, device=cuda)[None]).to(hd)
    half = prec != "fp32"
    ok = []
    for lst in ([0, 1, 2, 3, 4], [1, 2, 4], [4], []):
        n = len(lst)
        dst = torch.full((max(n, 1) * 1024, 1024 * src.element_size()), 0xA5, dtype=torch.uint8, device=cuda).view(hd)
        st = torch.full((max(n, 1) * 1024, 4, 2), float("nan"), dtype=F32, device=cuda) if half else None
        ops.gather_crops(src, lst, dst, st)
        want = _crops_of(src, lst)
        same = torch.equal(_bits(dst[:n * 1024]), _bits(want)) and bool((_bits(dst[n * 1024:]) == 0xA5).all())
        same_st = True
        if half and n:
            if prec == "bf16":
                ref = ops.row_stats(dst[:n * 1024])
            else:                                                      # cpx_row_stats is bf16; the fp16 entry is in the -DCPX_DEBUG build
                with _lib.use_debug_library():
                    ref = ops.row_stats(dst[:n * 1024])
            same_st = torch.equal(st[:n * 1024].view(torch.int32), ref.view(torch.int32)) and bool(torch.isnan(st[n * 1024:]).all())
        elif half:
            same_st = bool(torch.isnan(st).all())
        full = torch.full((nS * 1024, 1024 * src.element_size()), 0x5A, dtype=torch.uint8, device=cuda).view(hd)
        ops.scatter_crops(dst, lst, full)
        back = all(torch.equal(_bits(_crops_of(full, [c])), _bits(_crops_of(src, [c]))) if c in lst else bool((_bits(_crops_of(full, [c])) == 0x5A).all())
                   for c in range(nS))
        print(f"{prec} crops {lst}: gathered rows bitwise the source's {same}, statistics bitwise cpx_row_stats {same_st}, scatter touches the "
              f"listed crops alone {back}")
        ok += [same, same_st, back]
    dst = torch.full((nS * 1024, 1024 * src.element_size()), 0xA5, dtype=torch.uint8, device=cuda).view(hd)
    st = torch.full((nS * 1024, 4, 2), float("nan"), dtype=F32, device=cuda)
    for bad in ([2, 1], [1, 1], [0, 5], [-1, 2], [0, 1, 2, 3, 4, 4]):
        a = np.asarray(bad, np.int32)
        pa = a.ctypes.data_as(C.POINTER(C.c_int))
        rc_g = L.cpx_gather_crops(ops._DT[hd], ptr(src), nS, pa, len(bad), ptr(dst), ptr(st) if half else None, _stream(cuda))
        rc_s = L.cpx_scatter_crops(ops._DT[hd], ptr(src), nS, pa, len(bad), ptr(dst), _stream(cuda))
        torch.cuda.synchronize(cuda)
        untouched = bool((_bits(dst) == 0xA5).all()) and bool(torch.isnan(st).all())
        print(f"  list {bad}: gather {rc_g}, scatter {rc_s}, outputs untouched {untouched}")
        ok += [rc_g == EINVAL, rc_s == EINVAL, untouched]
    first = np.asarray([0], np.int32)
    one = first.ctypes.data_as(C.POINTER(C.c_int))
    if not half:
        ok.append(L.cpx_gather_crops(ops._DT[hd], ptr(src), nS, one, 1, ptr(dst), ptr(st), _stream(cuda)) == EINVAL)      # no float32 statistics
    ok.append(L.cpx_gather_crops(ops._DT[hd], ptr(src), nS, one, 1, ptr(dst) + 8, None, _stream(cuda)) == EINVAL)          # misaligned
    ok.append(L.cpx_gather_crops(ops._DT[hd], ptr(src), nS, one, 0, None, None, _stream(cuda)) == 0)                       # an empty list is fine
    assert all(ok) and bool((_bits(dst) == 0xA5).all())


# ---- 2. forward ---------------------------------------------------------------------------------------------------------
class _Alone:
    """``w`` with a copy of its weight struct cut to ``depth`` blocks (the trainer's frozen prefix does the same): with first_block =
    depth - 1 the existing forward runs that one block"""

    def __init__(self, w, depth):
        self.c = type(w.c).from_buffer_copy(w.c)
        self.c.depth = depth


def _check_forward(w, x, keep, o, dev, exact=True):
    """every stored tensor of the masked forward ``o`` against the existing forward of each block alone on its gathered crops -- gathered
    on the host from the rows the blocks before it left (``exact``), or the block's own stored input; returns (all bitwise, worst relative
    L2 per tensor kind, the rows after the last block when ``exact``)"""
    nS = x.shape[0] // 1024
    state = x.clone()
    same, worst = [], {}
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    for j in range(DEPTH):
        idx = ldr.kept(keep, j)
        nk = len(idx)
        assert o.n_keep[j] == nk
        if nk == 0:
            continue
        xin = _crops_of(state, idx).contiguous() if exact else o.x[j][:nk * 1024].contiguous()
        ws = ops.blocks_train_workspace(nk, w.c.dtype, 1, dev)
        ws.fill_(0xFF)
        o1 = ops.blocks_forward_train(_Alone(w, j + 1), xin, j, workspace=ws)
        pairs = {"x": (o.x[j], o1.x[0]), "qkv": (o.qkv[j], o1.qkv[0]), "ao": (o.ao[j], o1.ao[0]), "x_mid": (o.x_mid[j], o1.x_mid[0])}
        for k, (got, want) in pairs.items():
            got = got[:nk * 1024]
            same.append(torch.equal(_bits(got), _bits(want)))
            cols = slice(0, 2048) if k == "qkv" else slice(None)
            worst[k] = max(worst.get(k, 0.0), rel(got[:, cols], want[:, cols]))
            assert bool(torch.isfinite(got.float()).all()), (j, k)
        state.view(nS, 1024, 1024)[torch.as_tensor(idx, device=dev)] = o1.x_out.view(nk, 1024, 1024)
        if j + 1 == DEPTH:
            worst["rows"] = rel(_crops_of(o.x_out, idx), o1.x_out)
    return all(same), worst, state


@pytest.mark.parametrize("nS", [3, 4])
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
def test_forward_under_a_mask(cuda, prec, nS):
    sd, w = bt._weights(prec, cuda)
    keep = MASKS[nS]
    x = _rows_in(w, _patches(nS, prec, cuda, 40 + nS), nS, DEPTH, cuda)
    o = _forward_drop(w, x, DEPTH, keep, cuda)
    torch.cuda.synchronize(cuda)
    assert o.n_keep == [sum(k) for k in keep] and np.array_equal(o.keep, np.asarray(keep, np.uint8))
    blocks_same, _worst, state = _check_forward(w, x, keep, o, cuda)
    out_same = torch.equal(_bits(o.x_out), _bits(state))
    # a crop dropped by every block it met leaves as it came; one dropped by the last block leaves as the block before left it
    for c in range(nS):
        if not keep[1][c] and not keep[0][c]:
            assert torch.equal(_bits(_crops_of(o.x_out, [c])), _bits(_crops_of(x, [c])))
    dropped0 = [c for c in range(nS) if not keep[0][c]]
    kept1 = ldr.kept(keep, 1)
    through = all(torch.equal(_bits(_crops_of(o.x[1][:len(kept1) * 1024], [kept1.index(c)])), _bits(_crops_of(x, [c]))) for c in dropped0 if c in kept1)
    nk = ops.neck_forward_train(w, state.contiguous())
    torch.cuda.synchronize(cuda)
    neck_same = all(torch.equal(_bits(getattr(o.neck, k)), _bits(getattr(nk, k))) for k in ("y0", "a1", "y2", "feat"))
    head_same = torch.equal(o.head, nk.head)
    print(f"{prec} nS={nS} keep={keep}: each block's kept rows bitwise the existing forward of that block alone {blocks_same}; x_out bitwise "
          f"{out_same}; crops dropped by block 0 reach block 1 as they came {through}; neck {neck_same}; head {head_same}")
    assert blocks_same and out_same and through and neck_same and head_same and bool(torch.isfinite(o.head).all())


# ---- 3. backward, block by block ----------------------------------------------------------------------------------------
def _block_by_block(dev, mode, nS, keep):
    prec, gd, ad = MODES[mode]
    net = None if prec == "fp32" else HD[prec]
    sd, w = bt._weights(prec, dev)
    x = _rows_in(w, _patches(nS, prec, dev, 13 + nS), nS, DEPTH, dev)
    fwd = _forward_drop(w, x, DEPTH, keep, dev)
    g = torch.Generator(device=dev).manual_seed(17 + nS)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=dev) * torch.logspace(-2, 0, 256, device=dev)[None]
    params = _rounded_params(sd, prec, dev)
    grads, dx, dx_in = _backward(w, params, fwd, dy0, dev, gd, ad, want_in=True)
    grads2, dx2, dx_in2 = _backward(w, params, fwd, dy0, dev, gd, ad, want_in=True)
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in ((grads, grads2), (dx, dx2), (dx_in, dx_in2)))
    finite = bool(torch.isfinite(grads).all()) and bool(torch.isfinite(dx).all())
    in_same = torch.equal(dx_in.view(torch.int32), dx[0].view(torch.int32))
    print(f"blocks backward {mode} nS={nS} keep={keep}: two runs bitwise equal {same}, everything finite {finite}, dx_in is record 0 {in_same}")
    assert same and finite and in_same
    ok = []
    for j in (1, 0):
        idx = ldr.kept(keep, j)
        nk = len(idx)
        dropped = [c for c in range(nS) if c not in idx]
        passed = all(torch.equal(_crops_of(dx[j], [c]).view(torch.int32), _crops_of(dx[j + 1], [c]).view(torch.int32)) for c in dropped)
        print(f" block {j}: kept crops {idx}; the gradient rows of the dropped crops {dropped} pass down bitwise {passed}")
        ok.append(passed)
        G = {k: v.cpu() for k, v in _grad_views(grads, j).items()}
        if nk == 0:
            ok.append(not bool(_grad_views(grads, j)["qkv_w"].any()))
            continue
        P = br.params_from_state_dict(sd, j)
        xin, dout = fwd.x[j][:nk * 1024].float().cpu(), _crops_of(dx[j + 1], idx).cpu()
        held = {k: getattr(fwd, k)[j][:nk * 1024].float().cpu() for k in ("qkv", "ao", "x_mid")}
        r64 = br.block_grads(P, xin, dout, nk, torch.float64, net, True, stored=held)
        if gd == BF:
            r32 = ab.block_backward(P, xin, dout, nk, F32, net, True, stored=held, rnd=b16.round_bf16)
        else:
            r32 = br.block_grads(P, xin, dout, nk, F32, net, True, stored=held)
        for k in br.NAMES:
            got = _table_grad(sd, j, k, G[k]) if k.startswith("rel_") else G[k]
            ok.append(_check(f"block {j} {k}", got, r32["grads"][k], r64["grads"][k]))
        ok.append(_check(f"block {j} dx of the kept crops", _crops_of(dx[j], idx).cpu(), r32["dx"], r64["dx"]))
        assert not bool(G["rel_h"][63].any()) and not bool(G["rel_w"][63].any())
    return all(ok)


@pytest.mark.parametrize("nS", [3, 4])
@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16+bf16"])
def test_backward_block_by_block_under_a_mask(cuda, mode, nS):
    """Every gradient of every block and the kept crops' dx, each block on the device's own stored (compact) tensors and own incoming
    gradient with nS = n_keep; bf16+bf16: both bf16 switches, the comparator with the roundings of the GEMMs and the attention backward"""
    assert _block_by_block(cuda, mode, nS, MASKS[nS])


# ---- 4. edge masks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["bf16", "bf16+bf16", "fp32"])
def test_a_block_that_keeps_nothing(cuda, mode):
    """keep = [[0, 0, 0], [1, 1, 1]]: block 0 launches nothing.  Its whole gradient record is exactly zero -- bf16 folds LayerNorm, so
    k_unfold_grads runs on the all-zero record and must leave zeros --, dx[0] is dx[1] bitwise, and block 1 is what it is without a mask"""
    prec, gd, ad = MODES[mode]
    nS, keep = 3, [[0, 0, 0], [1, 1, 1]]
    sd, w = bt._weights(prec, cuda)
    x = _rows_in(w, _patches(nS, prec, cuda, 45), nS, DEPTH, cuda)
    fwd = _forward_drop(w, x, DEPTH, keep, cuda)
    g = torch.Generator(device=cuda).manual_seed(46)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=cuda)
    params = _rounded_params(sd, prec, cuda)
    grads, dx, dx_in = _backward(w, params, fwd, dy0, cuda, gd, ad, want_in=True)
    n, _o = ops.block_grad_layout()
    zero = not bool(grads[:n].any())
    passed = torch.equal(dx[0].view(torch.int32), dx[1].view(torch.int32)) and torch.equal(dx_in.view(torch.int32), dx[1].view(torch.int32))
    # block 1 alone, without a mask, on the same rows (block 0 passed x through)
    one = ops.blocks_forward_train(_Alone(w, DEPTH), x, DEPTH - 1)
    same_rows = torch.equal(_bits(fwd.x_out), _bits(one.x_out)) and torch.equal(fwd.head, one.head) and torch.equal(_bits(fwd.x[1]), _bits(x))
    g1, dx1, _ = _backward(w, params[n:].contiguous(), one, dy0, cuda, gd, ad)
    same_g = torch.equal(grads[n:].view(torch.int32), g1.view(torch.int32)) and torch.equal(dx[1].view(torch.int32), dx1[0].view(torch.int32))
    print(f"{mode}: block 0's record exactly zero {zero} (bytes {int(_bits(grads[:n]).max())}); dx[0] == dx[1] == dx_in bitwise {passed}; "
          f"block 1 bitwise the unmasked K = 1 run: rows {same_rows}, gradients {same_g}")
    assert zero and passed and same_rows and same_g and fwd.n_keep == [0, 3]


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_all_ones_and_no_mask_are_the_existing_entries(cuda, prec):
    nS = 3
    sd, w = bt._weights(prec, cuda)
    x = _rows_in(w, _patches(nS, prec, cuda, 47), nS, DEPTH, cuda)
    g = torch.Generator(device=cuda).manual_seed(48)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=cuda)
    params = _rounded_params(sd, prec, cuda)
    gd = BF if prec == "bf16" else F32
    base = _forward_train(w, x, DEPTH, cuda)
    ref = _backward(w, params, base, dy0, cuda, gd, gd, want_in=True)
    held = lambda o: [t.clone() for ts in (o.x, o.qkv, o.ao, o.x_mid) for t in ts] + [o.x_out.clone(), o.head.clone()] + \
        [getattr(o.neck, k).clone() for k in ("y0", "a1", "y2", "feat")]
    want = held(base)
    L, c = _lib.lib(), w.c
    for what, keep in (("all ones", np.ones((DEPTH, nS), np.uint8)), ("keep=None", None)):
        o = _forward_drop(w, x, DEPTH, keep, cuda)
        same_f = all(torch.equal(_bits(a), _bits(b)) for a, b in zip(held(o), want))
        got = _backward(w, params, o, dy0, cuda, gd, gd, want_in=True)
        same_b = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, ref))
        print(f"{prec} {what}: head and every stored tensor bitwise the existing forward {same_f}; grads, dx_all, dx_in bitwise {same_b}")
        assert same_f and same_b and o.n_keep == [nS] * DEPTH
    # the C entries themselves with a NULL mask and the workspace of the existing forward
    ws = ops.blocks_train_workspace(nS, c.dtype, DEPTH, cuda)
    ws.fill_(0xFF)
    head = torch.full((nS * 1024, c.ld_head), float("nan"), dtype=F32, device=cuda)
    assert L.cpx_blocks_forward_train_drop(C.byref(c), ptr(x), nS, 0, None, ptr(head), ptr(ws), ws.numel(), _stream(cuda)) == 0
    ones = np.ones((DEPTH, nS), np.uint8)
    head2 = torch.full_like(head, float("nan"))
    assert L.cpx_blocks_forward_train_drop(C.byref(c), ptr(x), nS, 0, ones.ctypes.data, ptr(head2), ptr(ws), ws.numel(), _stream(cuda)) == 0
    torch.cuda.synchronize(cuda)
    assert torch.equal(head, base.head) and torch.equal(head2, base.head)
    # a mask that drops needs the staging rows: the short workspace is refused and nothing is written
    ones[1, 0] = 0
    head3 = torch.full_like(head, float("nan"))
    rc = L.cpx_blocks_forward_train_drop(C.byref(c), ptr(x), nS, 0, ones.ctypes.data, ptr(head3), ptr(ws), ws.numel(), _stream(cuda))
    torch.cuda.synchronize(cuda)
    assert rc == EINVAL and bool(torch.isnan(head3).all())
    with pytest.raises(ValueError, match="keep is a uint8 array"):
        ops.blocks_forward_train(w, x, 0, keep=np.ones((DEPTH, nS + 1), np.uint8))


# ---- 5. sixteen kept crops ----------------------------------------------------------------------------------------------
def test_sixteen_kept_crops_take_the_big_statistics_route(cuda):
    """bf16, K = 2, 17 crops; block 0 keeps all 17, block 1 drops crop 5 and runs on 16: from 16 crops up the residual GEMMs emit the row
    statistics themselves and the existing forward hands block 1 those of block 0's last GEMM, while a compacted block takes them from
    the gather (the same sums in another order).  The bounds and their reasons are those of
    test_thirty_two_crops_statistics_from_the_gemms_and_two_mlp_parts: forward, 2^-8 in relative L2 (one bf16 ulp; the statistics differ
    by float32 summation order, which flips a bf16 rounding on about 5e-5 of the elements) on qkv (Q, K), the rows and the head, against
    the existing path on the gathered crops -- block 0 on all 17 and, from the masked forward's own rows, block 1 alone on its 16; and
    against the existing two-block forward of the 16 crops, whose block 1 does take its statistics from the GEMM.  Backward: every
    gradient against the float64 sum of two-crop runs with the same mask, 2^-6 (independent bf16 roundings of the stored tensors, at
    least 1024 rows per entry; a dropped or doubled slab or crop gives at least 1 / 17)."""
    prec, nS, K = "bf16", 17, DEPTH
    sd, w = bt._weights(prec, cuda)
    L, c = _lib.lib(), w.c
    assert L.cpx_gemm_uses_big_tile(16 * 1024, 1024, 1024, ops.EPI["resid"]) == 1 and L.cpx_gemm_uses_big_tile(16 * 1024, 1024, 4096, ops.EPI["resid"]) == 1
    keep = np.ones((K, nS), np.uint8)
    keep[1, 5] = 0
    idx = ldr.kept(keep, 1)
    x = _rows_in(w, _patches(nS, prec, cuda, 75), nS, K, cuda)
    o = _forward_drop(w, x, K, keep, cuda)
    torch.cuda.synchronize(cuda)
    _same, worst, _state = _check_forward(w, x, keep, o, cuda, exact=False)
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    x16 = _crops_of(x, idx).contiguous()
    o16 = _forward_train(w, x16, K, cuda)                              # the undropped path on the 16 crops: block 1's statistics from the GEMM
    e_qkv = rel(o.qkv[1][:16 * 1024, :2048], o16.qkv[1][:, :2048])
    e_rows, e_head = rel(_crops_of(o.x_out, idx), o16.x_out), rel(_crops_of(o.head, idx), o16.head)
    passed = torch.equal(_bits(_crops_of(o.x_out, [5])), _bits(_crops_of(ops.blocks_forward_train(_Alone(w, 1), x, 0).x_out, [5])))
    finite = all(bool(torch.isfinite(t.float()).all()) for t in (o.qkv[1][:16 * 1024], o.ao[1][:16 * 1024], o.x_mid[1][:16 * 1024], o.x_out, o.head))
    print(f"17 crops, block 1 on 16: against each block alone on its gathered crops {worst}; against the two-block forward of the 16 crops "
          f"qkv (Q, K) {e_qkv:.3e}, rows {e_rows:.3e}, head {e_head:.3e} (bound {2.0 ** -8:.3e}); crop 5 leaves as block 0 left it {passed}; finite {finite}")
    ok = [v <= 2.0 ** -8 for v in worst.values()] + [e_qkv <= 2.0 ** -8, e_rows <= 2.0 ** -8, e_head <= 2.0 ** -8, passed, finite]
    del o16
    g = torch.Generator(device=cuda).manual_seed(76)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=cuda) * torch.logspace(-2, 0, 256, device=cuda)[None]
    params = _rounded_params(sd, prec, cuda)
    n, _o = ops.block_grad_layout()

    def run(fwd, dy):
        rows = fwd.x_out.shape[0]
        ws = ops.blocks_backward_workspace(rows // 1024, c.dtype, cuda)
        ws.fill_(0xFF)
        grads = torch.full((K * n,), float("nan"), dtype=F32, device=cuda)
        ops.blocks_backward(w, params, fwd, dy, grads, ws)
        return grads
    grads, grads_b = run(o, dy0), run(o, dy0)
    torch.cuda.synchronize(cuda)
    same = torch.equal(grads.view(torch.int32), grads_b.view(torch.int32))
    del o
    total = torch.zeros(grads.numel(), dtype=torch.float64, device=cuda)
    for s0 in range(0, nS, 2):
        rows = slice(s0 * 1024, min(s0 + 2, nS) * 1024)
        o2 = _forward_drop(w, x[rows].contiguous(), K, keep[:, s0:s0 + 2], cuda)
        total += run(o2, dy0[rows].contiguous()).double()
    ok += [same, bool(torch.isfinite(grads).all())]
    for j in range(K):
        G, T = _grad_views(grads, j), _grad_views(total, j)
        for k in br.NAMES:
            e = float((G[k].double() - T[k]).norm() / T[k].norm())
            print(f"  block {j} {k}: 17 crops against the sum of the two-crop runs {e:.3e} (bound {2.0 ** -6:.3e})")
            ok.append(e <= 2.0 ** -6)
    print(f"  two runs bitwise equal {same}")
    assert all(ok)


# ---- 6. the trainer -----------------------------------------------------------------------------------------------------
def _trainer(dev, prec, sd=None, seed=53, embed=False, **kw):
    from classpose_amd.train import HeadTrainer
    sd = synth.make_state_dict(NCLS, None, depth=DEPTH, seed=seed) if sd is None else sd
    return HeadTrainer(sd, device=dev, precision=prec, train_blocks=DEPTH, train_embed=embed, **kw), sd


def _state_equal(a, b):
    sa, sb = a.state_dict(), b.state_dict()
    return set(sa) == set(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)


def test_layer_drop_zero_is_the_trainer_as_before(cuda):
    labs = _labels(2, NCLS, 11)
    a, sd = _trainer(cuda, "bf16", feature_batch=2)
    b, _ = _trainer(cuda, "bf16", sd=sd, feature_batch=2, layer_drop=0.0, layer_drop_seed=9)
    x = a.backbone_features(_patches(2, "bf16", cuda, 57))
    state = b._drop_rng.bit_generator.state
    for lr in (0.0, 1e-3, 2e-3):
        ra, rb = a.step(x, labs, lr), b.step(x, labs, lr)
        assert ra == rb, (ra, rb)
    same = _state_equal(a, b) and torch.equal(a.blocks.params.view(torch.int32), b.blocks.params.view(torch.int32))
    print(f"layer_drop=0 after 3 steps: state bitwise the trainer built without the argument {same}; generator untouched "
          f"{b._drop_rng.bit_generator.state == state}")
    assert same and b._drop_rng.bit_generator.state == state and b._bfwd.keep is None
    with pytest.raises(ValueError, match=r"keep: a uint8 mask \(2, 2\)"):
        a.step(x, labs, 1e-3, keep=np.ones((DEPTH, 3), np.uint8))
    with pytest.raises(ValueError, match=r"keep: a uint8 mask \(2, 2\)"):
        a.step(x, labs, 1e-3, keep=np.ones((1, 2), np.uint8))
    assert _state_equal(a, b), "a refused mask changes nothing"
    # evaluate never drops, whatever the rate
    d, _ = _trainer(cuda, "bf16", sd=sd, feature_batch=2, layer_drop=0.9, layer_drop_seed=1)
    c0, _ = _trainer(cuda, "bf16", sd=sd, feature_batch=2)
    ev_d, ev_0 = d.evaluate(x, labs), c0.evaluate(x, labs)
    print(f"evaluate at layer_drop 0.9: {ev_d}; at 0: {ev_0}")
    assert ev_d == ev_0 and d._bfwd.keep is None


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_step_with_a_mask_end_to_end(cuda, prec):
    """train_embed on at depth 2, 2 crops, 3 classes, keep = [[1, 0], [1, 1]]: the embedding, both blocks, the neck and both heads from
    labels and flow targets, by the rule of test_gradients_end_to_end, against layer_drop_reference.loss_and_grads"""
    nS, keep = 2, np.asarray([[1, 0], [1, 1]], np.uint8)
    t, sd = _trainer(cuda, prec, embed=True, feature_batch=2, train_flow_head=True)
    p = _patches(nS, prec, cuda, 23)
    labs, tg = _labels(nS, NCLS, 7), _targets(nS, 8)
    t.embed.grads.fill_(float("nan"))
    feat, head, o = t._loss(p, labs, t._step_mask(labs, keep))
    seg = t._seg_loss(head, tg.to(cuda))
    t._neck_backward(*t._fwd, o, seg)
    t._blocks_backward()
    torch.cuda.synchronize(cuda)
    assert t._bfwd.n_keep == [1, 2]
    loss = float(o.ce.item()) + float(o.tversky.item()) + float(seg.flow.item()) + float(seg.cp.item())
    got_n = {k: v.clone().cpu() for k, v in _neck_views(t.neck.grads).items()}
    got_n["Wc"], got_n["bc"] = (v.cpu() for v in ops.head_wgrad(o.dlogits, feat))
    got_n["Wf"], got_n["bf"] = (v.cpu() for v in ops.head_wgrad(seg.dlogits, feat))
    net = None if prec == "fp32" else HD[prec]
    PE, PN = er.params_from_state_dict(sd), nr.params_from_state_dict(sd)
    PB = [br.params_from_state_dict(sd, j) for j in range(DEPTH)]
    lab = torch.from_numpy(labs.astype(np.int64))
    pc = p.float().cpu()
    r64 = ldr.loss_and_grads(PB, PN, pc, lab, tg, NCLS, keep, torch.float64, net, PE=PE)
    r32 = ldr.loss_and_grads(PB, PN, pc, lab, tg, NCLS, keep, F32, net, PE=PE)
    print(f"{prec} keep={keep.tolist()}: loss device {loss:.6f}, float64 {float(r64['loss']):.6f}, float32 {float(r32['loss']):.6f}")
    ok = [abs(loss - float(r64["loss"])) <= 1e-3 * abs(float(r64["loss"]))]
    for i, k in enumerate(er.NAMES):
        got = t.embed.view(i, t.embed.grads).cpu()
        assert bool(torch.isfinite(got).all())
        ok.append(_check(k, got, r32["embed"][k], r64["embed"][k]))
    for k in nr.NECK + nr.HEADS:
        ok.append(_check(k, got_n[k], r32["neck"][k], r64["neck"][k]))
    for j in range(DEPTH):
        for ti, k in enumerate(br.NAMES):
            got = t.blocks.rel_grads[j][ti - 4] if k.startswith("rel_") else t.blocks.view(j, ti, t.blocks.grads)
            ok.append(_check(f"block {j} {k}", got.cpu(), r32["blocks"][j][k], r64["blocks"][j][k]))
    assert all(ok)
    # the public call with the same mask reports the same losses
    r = t.step(p, labs, 0.0, flow_targets=tg.to(cuda), keep=keep)
    assert abs(r["loss"] - loss) <= 1e-6 * abs(loss)


def test_ten_steps_at_rate_04(cuda, tmp_path):
    """fp32, K = 2, one crop, rate 0.4 (blocks 0 and 1 drop with probabilities 0 and 0.4; a step that drops block 1 launches nothing for
    it and still takes its AdamW step on zero gradients): one seed twice gives bitwise equal checkpoints, another seed different ones; the float64 replay under the same masks is followed to the bound of test_twenty_steps (the project's
    rule with the floor steps * 2^-20 on the loss curve and on the final update of every block tensor); the checkpoint loads"""
    from classpose_amd.train import draw_keep_mask, lr_schedule
    prec, nS, steps = "fp32", 1, 10
    labs, tg = _labels(nS, NCLS, 9), _targets(nS, 10)
    lrs = [float(v) for v in lr_schedule(2e-4, steps)[:steps]]
    rng = np.random.default_rng(4)
    masks = [draw_keep_mask(rng, nS, DEPTH, DEPTH, 0.4) for _ in range(steps)]
    dropped = sum(int((m == 0).sum()) for m in masks)
    assert dropped > 0 and all(m[0].all() for m in masks), "block 0 of a fully trained network never drops"
    runs = []
    for seed in (4, 4, 5):
        t, sd = _trainer(cuda, prec, feature_batch=1, train_flow_head=True, layer_drop=0.4, layer_drop_seed=seed)
        x = t.backbone_features(_patches(nS, prec, cuda, 33))
        tgd = tg.to(cuda)
        losses, seen = [], []
        for lr in lrs:
            losses.append(t.step(x, labs, lr, flow_targets=tgd)["loss"])
            seen.append(t._bfwd.keep.copy() if t._bfwd.keep is not None else np.ones((DEPTH, nS), np.uint8))
        t.save(tmp_path / f"drop{len(runs)}.pt")
        runs.append((np.array(losses), torch.load(tmp_path / f"drop{len(runs)}.pt", map_location="cpu", weights_only=True), seen, t))
        if len(runs) == 1:
            x_cpu = x.float().cpu()
    (la, ca, seen_a, t), (lb, cb, _sb, _tb), (lc, cc, seen_c, _tc) = runs
    same = bool((la == lb).all()) and set(ca) == set(cb) and all(torch.equal(ca[k], cb[k]) for k in ca)
    other = any(not torch.equal(ca[k], cc[k]) for k in ca)
    drew = all(np.array_equal(a, b) for a, b in zip(seen_a, masks))
    print(f"ten steps at rate 0.4: {dropped} of {steps * DEPTH * nS} pairs dropped; the trainer drew the masks of its seed {drew}; one seed twice "
          f"bitwise equal {same}; another seed differs {other} (its masks differ {any(not np.array_equal(a, b) for a, b in zip(seen_a, seen_c))})")
    assert same and other and drew
    PB, PN = [br.params_from_state_dict(sd, j) for j in range(DEPTH)], nr.params_from_state_dict(sd)
    lab = torch.from_numpy(labs.astype(np.int64))
    l64, b64, _n64 = ldr.replay(PB, PN, x_cpu, lab, tg, NCLS, lrs, masks, torch.float64, None, t.weight_decay)
    l32, b32, _n32 = ldr.replay(PB, PN, x_cpu, lab, tg, NCLS, lrs, masks, F32, None, t.weight_decay)
    floor = steps * FLOOR
    ok = [_check("loss curve", la, l32, l64, floor)]
    for j in range(DEPTH):
        for ti, k in enumerate(br.NAMES):
            fin = t.blocks.rel[j][ti - 4] if k.startswith("rel_") else t.blocks.view(j, ti)
            ok.append(_check(f"final update of block {j} {k}", fin.cpu().double() - PB[j][k].double(), b32[j][k].double() - PB[j][k].double(),
                             b64[j][k] - PB[j][k].double(), floor))
    assert all(ok)
    w = engine.NetWeights.from_state_dict(ca, prec, cuda)
    assert w.depth == DEPTH and w.ncls == NCLS
    changed = {k for k in sd if not torch.equal(ca[k], sd[k])}
    assert all(any(k.startswith(f"encoder.blocks.{j}.") for k in changed) for j in range(DEPTH))


# ---- 7. the command line ------------------------------------------------------------------------------------------------
def test_cli_layer_drop_in_a_child_process(cuda, tmp_path):
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
    r = subprocess.run(bt._cli(tmp_path, "--train_blocks", "2", "--layer_drop", "0.4"), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    log = r.stdout + r.stderr
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    line = [ln for ln in log.splitlines() if "--layer_drop 0.4" in ln]
    print(line)
    assert line and "blocks 0 to 1 of 2" in line[0] and "0.0000, 0.4000" in line[0]
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert all(any(not torch.equal(ck[k], sd[k]) for k in sd if k.startswith(f"encoder.blocks.{j}.")) for j in range(DEPTH))
    assert engine.NetWeights.from_state_dict(ck, "bf16", cuda).ncls == 3
    r = subprocess.run(bt._cli(tmp_path, "--layer_drop", "0.4"), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode != 0 and "--layer_drop goes with --train_blocks" in r.stderr
