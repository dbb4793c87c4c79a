"""Block training (csrc/cpx_train_blocks.hip) at the crop counts the trainer really runs: tests/test_gpu_block_train.py has 1, 3 and 32
crops; HeadTrainer's default batch is 8, the last batch of an epoch is anything smaller, and --batch_size is free.  The network is the
same synth.make_state_dict(3, None, depth=2) and the helpers are that file's.

1. The training forward in every route band of cpx_gemm_half (M = crops * 1024 rows; big tile: (M / 256) * (N / 256) >= 256):
       crops    qkv (N 3072)   lin1 (N 4096)   proj / lin2 (N 1024)   row statistics   MLP parts      cases here
       1 - 3    128^2          128^2           128^2                  cpx_row_stats    1              (1, 3: the other file)
       4 - 5    128^2          256^2           128^2                  cpx_row_stats    1              4
       6 - 15   256^2          256^2           128^2                  cpx_row_stats    1              6, 8, 15
       16 - 31  256^2          256^2           256^2 + statistics     GEMM epilogues   1              16 (K = 2), 17
       >= 32    256^2          256^2           256^2 + statistics     GEMM epilogues   crops / 16     33 (16 384 + 17 408 rows)
   Every case first asserts its band through the library's own predicates, so a later change of routing reports that the premise
   moved.  Below 16 crops the result is bitwise cpx_net_forward; from 16 up the first trained block takes its statistics from
   cpx_row_stats where cpx_net_forward takes them from a GEMM epilogue, and the bound is the 32-crop test's (its docstring derives it).
2. The backward, slab by slab, exactly.  cpx_blocks_backward is linear in dy0 at fixed stored tensors and a crop's gradient depends on
   that crop alone.  With dy0 non-zero in one slab of two crops only, every other slab contributes exact zeros (zero dy gives zero GEMM
   outputs, zero LayerNorm and GELU backward, zero dS'), and every accumulation -- the RESID epilogue with aux == out, k_colsum_add,
   k_rel_finish(add = 1), add_run -- adds 0 to what it holds.  The whole-batch result therefore EQUALS (torch.equal on the float
   tensors: -0 == +0) the backward of that slab run alone, on a forward record that holds nothing but the slab's rows of the four kept
   tensors: everything else in it stays 0xFF, which also proves that the backward reads only those four.
3. bf16 / fp16 weights built with fuse_ln=False: the third code path of both entry points (LayerNorm as a kernel of its own, its output
   in the network dtype; the backward recomputes and rounds it, k_ln_fwd1024<DT, true>, and adds dgamma / dbeta per slab).  Forward
   bitwise cpx_net_forward, backward against float64 under the project's rule.

Every workspace is filled with 0xFF and every output with NaN before the call that writes it; every test prints what it observed before
it asserts (run with -s)."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

import block_train_reference as br
import test_gpu_block_train as bt
from classpose_amd import _lib, engine, ops
from classpose_amd._lib import ptr
from test_gpu_block_train import DEPTH, FLOOR, HD, _forward_train, _grad_views, _net_forward, _operand, _patches, _rounded_params, _rows_in, \
    _run_backward, _weights

pytestmark = pytest.mark.gpu
_WU = {}


def _weights_for(prec, fused, dev):
    """(state dict, weights): the other file's folded weights, or the same checkpoint built with fuse_ln=False"""
    sd, w = _weights(prec, dev)
    if fused or prec == "fp32":
        return sd, w
    if prec not in _WU:
        _WU[prec] = engine.NetWeights.from_state_dict(sd, prec, dev, fuse_ln=False)
    assert _WU[prec].c.fuse_ln == 0 and w.c.fuse_ln == 1
    return sd, _WU[prec]


# ---- 1. forward ---------------------------------------------------------------------------------------------------
def _band(nS):
    """(qkv, lin1, proj, lin2 on the 256^2 kernel; MLP row parts) as the half-precision dispatch decides them"""
    L, M = _lib.lib(), nS * 1024
    big = lambda N, K, epi: int(L.cpx_gemm_uses_big_tile(M, N, K, ops.EPI[epi]))
    return (big(3072, 1024, "qkv"), big(4096, 1024, "gelu"), big(1024, 1024, "resid"), big(1024, 4096, "resid"),
            int(L.cpx_net_mlp_parts(nS, _lib.DTYPE_CODE["bf16"])))


BANDS = {1: (0, 0, 0, 0, 1), 3: (0, 0, 0, 0, 1), 4: (0, 1, 0, 0, 1), 6: (1, 1, 0, 0, 1), 8: (1, 1, 0, 0, 1), 15: (1, 1, 0, 0, 1),
         16: (1, 1, 1, 1, 1), 17: (1, 1, 1, 1, 1), 33: (1, 1, 1, 1, 2)}


def _assert_band(nS):
    got = _band(nS)
    print(f"  routes at {nS} crops (qkv, lin1, proj, lin2 on the big tile; MLP parts): {got}, the band's {BANDS[nS]}")
    assert got == BANDS[nS], "the GEMM routing moved: this case no longer runs the band it names"
    assert nS != 33 or (nS * 1024 - 16384 == 17408 and got[4] == 2), "two parts, the second with the remainder"


def _standalone_qkv(w, b, x, prec, fused, dev):
    """the first trained block's qkv rows by the launch the network makes, on its own"""
    nS = x.shape[0] // 1024
    if prec == "fp32":
        return ops.gemm(ops.layernorm(x, _operand(w, b.ln1_w), _operand(w, b.ln1_b)), _operand(w, b.qkv_w), "f32", _operand(w, b.qkv_b))
    vt = torch.full((nS * 1024, 1024), float("nan"), dtype=HD[prec], device=dev)
    if not fused:
        xn = ops.layernorm(x, _operand(w, b.ln1_w), _operand(w, b.ln1_b))
        qkv = ops.gemm(xn, _operand(w, b.qkv_w), "qkv", _operand(w, b.qkv_b), vt)
    else:
        args = (_operand(w, b.qkv_w), "qkv", _operand(w, b.qkv_b), vt)
        if prec == "bf16":
            qkv = ops.gemm_ln(x, *args, ops.row_stats(x), _operand(w, b.qkv_colsum))
        else:                                                          # fp16: the entries of the -DCPX_DEBUG build of the same sources
            with _lib.use_debug_library():
                qkv = ops.gemm_ln(x, *args, ops.row_stats(x), _operand(w, b.qkv_colsum))
    # that epilogue writes the V third transposed into vt [crop][channel][token] instead of the rows; the kept rows hold it
    qkv[:, 2048:] = vt.view(nS, 1024, 1024).transpose(1, 2).reshape(nS * 1024, 1024)
    return qkv


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _ao_is_attention(w, o, K):
    ok = []
    for j in range(K):
        b = w.blocks[DEPTH - K + j]
        ok.append(_same_bits(ops.attention(o.qkv[j].contiguous(), _operand(w, b.rel_h), _operand(w, b.rel_w)), o.ao[j]))
    return all(ok)


def _finite(o):
    return all(bool(torch.isfinite(t.float()).all()) for ts in (o.x, o.qkv, o.ao, o.x_mid, [o.x_out, o.head]) for t in ts)


def _bitwise_forward(dev, prec, K, nS, fused):
    """the assertions of test_forward_train_is_bitwise_net_forward"""
    sd, w = _weights_for(prec, fused, dev)
    patches = _patches(nS, prec, dev, 3 + nS)
    head, x_last = _net_forward(w, patches, nS, dev)
    x = _rows_in(w, patches, nS, K, dev)
    o = _forward_train(w, x, K, dev)
    torch.cuda.synchronize(dev)
    same_head, same_x, same_in = torch.equal(o.head, head), _same_bits(o.x_out, x_last), _same_bits(o.x[0], x)
    same_qkv = _same_bits(_standalone_qkv(w, w.blocks[DEPTH - K], x, prec, fused, dev), o.qkv[0])
    same_ao, finite = _ao_is_attention(w, o, K), _finite(o)
    print(f"{prec}{'' if fused else ' fuse_ln=False'} K={K} nS={nS}: head equal {same_head}, last block's rows equal {same_x}, stored input equal "
          f"{same_in}, qkv == stand-alone GEMM {same_qkv}, ao == cpx_attention(qkv) {same_ao}, stored tensors finite {finite}")
    assert same_head and same_x and same_in and same_qkv and same_ao and finite and bool(torch.isfinite(head).all())


@pytest.mark.parametrize("prec,K,nS", [(p, K, n) for p in ("bf16", "fp16") for K in (1, 2) for n in (4, 6, 8, 15)] + [("fp32", 2, 8)])
def test_forward_train_below_sixteen_crops_is_bitwise_net_forward(cuda, prec, K, nS):
    """4: lin1 alone on the 256^2 kernel; 6: the first count with qkv on it; 8: the trainer's default; 15: the last before the statistics
    move into the GEMM epilogues.  fp32 has one GEMM kernel: one case"""
    _assert_band(nS)
    _bitwise_forward(cuda, prec, K, nS, fused=True)


@pytest.mark.parametrize("prec,nS,K", [("bf16", 16, 2), ("fp16", 16, 2), ("bf16", 17, 1), ("bf16", 33, 1)])
def test_forward_train_from_sixteen_crops_up(cuda, prec, nS, K):
    """The rule and the bound of test_thirty_two_crops_statistics_from_the_gemms_and_two_mlp_parts (tests/test_gpu_block_train.py), whose
    docstring derives it: the first trained block's statistics come from cpx_row_stats, cpx_net_forward's from the epilogue of the GEMM
    before (the patch embedding for K = 2), the same sums in another order -- relative L2 at most one ulp, 2^-8 (fp16 rounds finer: the
    same bound holds all the more), on the Q and K thirds of the first trained block's qkv, the last block's rows and the head.
    16 crops with K = 2: the second trained block reads the statistics the first one's lin2 epilogue wrote.  17: an odd count that still
    has M % 256 == 0.  33: two MLP parts of 16 384 and 17 408 rows, Mp = M - r0.
    Bitwise all the same: the first trained block's qkv against the stand-alone cpx_gemm_ln with cpx_row_stats(x) -- that is the
    launch --, and ao == cpx_attention(qkv) for every trained block.
    Observed (qkv, rows, head): bf16 16 crops K = 2 1.0e-5, 1.5e-3, 3.7e-3; fp16 3.2e-6, 2.5e-4, 5.1e-4; bf16 17 crops 8.6e-6, 2.8e-4,
    1.5e-3; 33 crops 9.2e-6, 2.6e-4, 1.4e-3.  That docstring's "the flips it causes downstream are as rare" holds for qkv only: a
    tensor that differs by e before a rounding of relative step ulp lands on the neighbouring value for a fraction e / ulp of its
    elements, sqrt(e ulp) in relative L2, which is MORE than e while e < ulp.  With ulp = 2^-7.5 for bf16: qkv 1e-5 -> the block's rows
    sqrt(1e-5 * 5.5e-3) = 2.3e-4 -> the second trained block's rows sqrt(2.8e-4 * 5.5e-3) = 1.2e-3 -> through the neck's four bf16
    tensors to the head.  Per rounding the figure saturates near ulp / sqrt 6 = 2.3e-3 (two independent roundings), and the stages add
    in squares.  All twelve figures are inside 2^-8 = 3.9e-3 as the issue states it, but the head of the K = 2 case sits at 94 % of it:
    the bound has no room for a third trained block at 16 crops or more (this network has two)."""
    _assert_band(nS)
    sd, w = _weights_for(prec, True, cuda)
    L, c = _lib.lib(), w.c
    patches = _patches(nS, prec, cuda, 80 + nS)
    full = c.depth
    refs = {}
    for depth in sorted({full - K + 1, full}):                         # the first trained block's qkv stays in the workspace of a run that ends there
        ws = torch.full((L.cpx_net_workspace_bytes(nS, c.dtype),), 0xFF, dtype=torch.uint8, device=cuda)
        head = torch.full((nS * 1024, c.ld_head), float("nan"), dtype=torch.float32, device=cuda)
        c.depth = depth
        try:
            _lib.check(L.cpx_net_forward(C.byref(c), ptr(patches), nS, ptr(head), ptr(ws), ws.numel(), torch.cuda.current_stream(cuda).cuda_stream),
                       "net_forward")
        finally:
            c.depth = full
        if depth == full - K + 1:
            qkv_off = nS * 1024 * 1024 * 2 * 2                         # cpx_net_ws: x, xn, then qkv (256-byte aligned sizes)
            refs["qk"] = ws[qkv_off:qkv_off + nS * 1024 * 3072 * 2].view(HD[prec]).view(nS * 1024, 3072)[:, :2048].clone()
        if depth == full:
            refs["head"], refs["x"] = head, ops.backbone_rows(ws, nS, HD[prec]).clone()
        del ws
    x = _rows_in(w, patches, nS, K, cuda)
    o = _forward_train(w, x, K, cuda)
    torch.cuda.synchronize(cuda)
    rel = lambda a, b: float((a.float() - b.float()).norm() / b.float().norm())
    e_qk, e_x, e_head = rel(o.qkv[0][:, :2048], refs["qk"]), rel(o.x_out, refs["x"]), rel(o.head, refs["head"])
    same_in = _same_bits(o.x[0], x)
    same_qkv = _same_bits(_standalone_qkv(w, w.blocks[DEPTH - K], x, prec, True, cuda), o.qkv[0])
    same_ao, finite = _ao_is_attention(w, o, K), _finite(o)
    print(f"{prec} K={K} nS={nS}: against cpx_net_forward qkv (Q, K) {e_qk:.3e}, last block's rows {e_x:.3e}, head {e_head:.3e} (bound "
          f"{2.0 ** -8:.3e}); stored input equal {same_in}, qkv == stand-alone GEMM with cpx_row_stats {same_qkv}, ao == cpx_attention(qkv) "
          f"{same_ao}, finite {finite}")
    assert e_qk <= 2.0 ** -8 and e_x <= 2.0 ** -8 and e_head <= 2.0 ** -8
    assert same_in and same_qkv and same_ao and finite and bool(torch.isfinite(refs["head"]).all())


# ---- 2. the backward, slab by slab --------------------------------------------------------------------------------
SLAB = 2


def _slab_record(w, o, c0, nc, dev):
    """The forward record of crops [c0, c0 + nc) of ``o`` as a stand-alone run of nc crops would lay it out, holding the rows of the
    four kept tensors of every trained block and 0xFF everywhere else (x_out, the neck's tensors, V^T, the hidden activations, the
    statistics)"""
    K, dt, hd = len(o.x), w.c.dtype, o.x[0].dtype
    ws = ops.blocks_train_workspace(nc, dt, K, dev)
    ws.fill_(0xFF)
    off = (C.c_size_t * (4 * K + 2))()
    _lib.check(_lib.lib().cpx_blocks_train_layout(nc, dt, K, off), "blocks_train_layout")
    rows, es = nc * 1024, o.x[0].element_size()
    view = lambda at, width: ws[at:at + rows * width * es].view(hd).view(rows, width)
    r = ops.BlocksForwardOut()
    r.workspace, r.first_block, r.head, r.neck = ws, o.first_block, None, None
    r.x, r.qkv, r.ao, r.x_mid = [], [], [], []
    for j in range(K):
        for i, (dst, src, width) in enumerate(((r.x, o.x, 1024), (r.qkv, o.qkv, 3072), (r.ao, o.ao, 1024), (r.x_mid, o.x_mid, 1024))):
            v = view(off[4 * j + i], width)
            v.copy_(src[j][c0 * 1024:(c0 + nc) * 1024])
            dst.append(v)
    r.x_out = view(off[4 * K], 1024)                                   # poisoned: only its row count is read
    return r


def _backward_case(dev, prec, fused, nS, K, seed):
    sd, w = _weights_for(prec, fused, dev)
    assert _lib.lib().cpx_blocks_backward_slab_crops() == SLAB
    x = _rows_in(w, _patches(nS, prec, dev, seed), nS, K, dev)
    o = _forward_train(w, x, K, dev)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    dy0 = torch.randn(nS * 1024, 256, generator=g, device=dev) * torch.logspace(-2, 0, 256, device=dev)[None]
    params = _rounded_params(sd, prec, dev)[(DEPTH - K) * ops.block_grad_layout()[0]:].contiguous()
    return w, o, dy0, params


def _hot(dy0, slabs, nS):
    """dy0 with every row outside the given slabs zero, and the row mask"""
    mask = torch.zeros(nS * 1024, dtype=torch.bool, device=dy0.device)
    for s in slabs:
        mask[s * SLAB * 1024:min((s + 1) * SLAB, nS) * 1024] = True
    return dy0 * mask[:, None], mask


ONE_HOT = [("bf16", True, 8, 2, 0), ("bf16", True, 8, 2, 1), ("bf16", True, 8, 2, 3), ("bf16", True, 7, 1, 0), ("bf16", True, 7, 1, 3),
           ("fp32", True, 8, 2, 2), ("fp16", True, 5, 1, 1), ("bf16", False, 7, 2, 1), ("bf16", False, 7, 2, 3)]


@pytest.mark.parametrize("prec,fused,nS,K,slab", ONE_HOT)
def test_backward_of_one_hot_slab_equals_the_slab_alone(cuda, prec, fused, nS, K, slab):
    """Slab 0: the later slabs must add to the result, not replace it; a middle slab and the last one: the row offsets r0 into a
    forward workspace whose per-block stride depends on nS; slab 3 of 7 crops: the one-crop remainder (crop 6), alone at nS = 1"""
    w, o, dy0, params = _backward_case(cuda, prec, fused, nS, K, 90 + 10 * nS + slab)
    hot, mask = _hot(dy0, [slab], nS)
    c0 = slab * SLAB
    nc = min(SLAB, nS - c0)
    assert int(mask.sum()) == nc * 1024 and nc == (1 if (nS, slab) == (7, 3) else SLAB)
    grads, dx = _run_backward(w, params, o, hot, cuda)
    rec = _slab_record(w, o, c0, nc, cuda)
    alone, dx1 = _run_backward(w, params, rec, hot[mask].contiguous(), cuda)
    finite = all(bool(torch.isfinite(t).all()) for t in (grads, dx, alone, dx1))
    diff = []
    for j in range(K):
        G, A = _grad_views(grads, j), _grad_views(alone, j)
        assert len(G) == 14
        diff += [f"block {j} {k}" for k in G if not torch.equal(G[k], A[k])]
        diff += [f"block {j} {k} row 63" for k in ("rel_h", "rel_w") if bool(G[k][63].any()) or tuple(G[k].shape) != (64, 64)]
    same_dx = torch.equal(dx[:, mask], dx1)
    zero_dx = not bool(dx[:, ~mask].any())
    live = float(dx1.abs().max()) > 0 and all(float(v.abs().max()) > 0 for v in _grad_views(alone, 0).values())
    print(f"{prec}{'' if fused else ' fuse_ln=False'} nS={nS} K={K}, slab {slab} ({nc} crop(s)) hot: gradient tensors that differ from the slab "
          f"alone: {diff or 'none'}; the slab's dx rows equal {same_dx}; every other dx row zero {zero_dx}; finite {finite}; "
          f"max |dx| {float(dx1.abs().max()):.3e}")
    assert not diff and same_dx and zero_dx and finite and live


@pytest.mark.parametrize("prec", ["bf16", "fp32"])
def test_backward_of_two_hot_slabs_is_the_sum_of_the_one_hot_runs(cuda, prec):
    """8 crops, K = 2, slabs 1 and 3 hot.  Rows of different slabs never mix: every dx row equals its own one-hot run.  Each gradient
    tensor against the float64 sum of the two one-hot results, relative L2 at most the project's floor 2^-20 = 16 float32 unit
    round-offs: an element sees one float32 addition (slab 3 onto slab 1), and in the folded tensors the fma and the product of
    k_unfold_grads, applied once to the sum here and once to each term there -- at most four roundings."""
    nS, K = 8, 2
    w, o, dy0, params = _backward_case(cuda, prec, True, nS, K, 171)
    (h1, m1), (h3, m3), (h13, m13) = (_hot(dy0, s, nS) for s in ([1], [3], [1, 3]))
    (g1, dx1), (g3, dx3), (g13, dx13) = (_run_backward(w, params, o, h, cuda) for h in (h1, h3, h13))
    rows = torch.equal(dx13[:, m1], dx1[:, m1]) and torch.equal(dx13[:, m3], dx3[:, m3])
    zero = not bool(dx13[:, ~m13].any()) and not bool(dx1[:, ~m1].any()) and not bool(dx3[:, ~m3].any())
    finite = all(bool(torch.isfinite(t).all()) for t in (g1, g3, g13, dx13))
    total = g1.double() + g3.double()
    print(f"{prec}: dx rows of slabs 1 and 3 equal their one-hot runs {rows}; every other dx row zero {zero}; finite {finite}")
    worst = 0.0
    for j in range(K):
        G, T, A = _grad_views(g13, j), _grad_views(total, j), _grad_views(g1, j)
        for k in G:
            e = float((G[k].double() - T[k]).norm() / T[k].norm())
            print(f"  block {j} {k}: two hot slabs against the float64 sum of the one-hot runs {e:.3e} (bound {FLOOR:.3e})")
            worst = max(worst, e)
            assert float(A[k].abs().max()) > 0 and not torch.equal(G[k], A[k]), "both slabs contribute"
    print(f"  worst {worst:.3e}")
    assert rows and zero and finite and worst <= FLOOR


# ---- 3. half precision with fuse_ln=False -------------------------------------------------------------------------
@pytest.mark.parametrize("nS", [1, 3])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_unfused_forward_train_is_bitwise_net_forward(cuda, prec, K, nS):
    """the last ``else`` of cpx_blocks_forward_train: cpx_layernorm, then the plain GEMMs"""
    _assert_band(nS)
    _bitwise_forward(cuda, prec, K, nS, fused=False)


@pytest.mark.parametrize("prec,nS", [("bf16", 3), ("fp16", 1)])
def test_unfused_backward_block_by_block(cuda, prec, nS):
    """test_backward_block_by_block on weights built with fuse_ln=False, against block_grads(..., fold=False, stored=held): the replay
    rounds the LayerNorm output through the network dtype, as the forward stores it and k_ln_fwd1024<DT, true> recomputes it; dgamma and
    dbeta come from cpx_layernorm_backward per slab (nS = 3: two slabs, add_run), not from k_unfold_grads"""
    sd, w = _weights_for(prec, False, cuda)
    bt.block_by_block(cuda, prec, nS, sd, w, fold=False)
