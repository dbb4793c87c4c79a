"""The UNet semantic head (cpx_unet_head_forward: k_conv_gather, the GEMMs, k_depth2space) op by op, every valid element,
and the network forward on a poisoned workspace.

Each case runs the head on a test-made neck output with the workspace filled with 0xFF bytes (NaN in bf16, fp16 and fp32),
reads every op's output back through cpx_unet_head_layout (the layout helper the run itself uses) and compares it with a
float64 F.conv2d / F.conv_transpose2d of the kernel's OWN input tensors, read back from the workspace, with the weights and
biases of the state dict rounded to the dtype (so the host packing of engine._build_unet_ops is under test too).  Ops are
mapped to state-dict keys in oracle.net.unet_forward's order, decoder inputs concatenated [cur, skip].

Bound: the GEMM multiplies dtype operands and accumulates in float32 over K = taps * cin (padded) terms in some order:
|acc - exact| <= K u sum|a||w| (u = 2^-24); + bias rounds once (u |acc + b|, half types only: in fp32 that IS the final
rounding); ReLU is monotone and 1-Lipschitz; the store rounds to the dtype: bound = 1/2 ulp(|ref| + d) + d with
    d = K u sum|a||w| + u |acc + b|   (fp32: d = K u sum|a||w|, the 1/2 ulp being float32's)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from classpose_amd import _lib, engine, ops, synth
from classpose_amd._lib import ptr
from oracle import numerics as nm

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SENT = -7777.25
HD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
_W = {}


def _weights(ncls, fts, prec, dev):
    key = (ncls, tuple(fts), prec)
    if key not in _W:
        sd = synth.make_state_dict(ncls, list(fts), depth=1, seed=11 + len(fts))
        _W[key] = (sd, engine.NetWeights.from_state_dict(sd, prec, dev))
    return _W[key]


def _plan(fts, out_ch):
    """unet_forward's convolutions in order: (key, kind, relu, inputs, h_in); inputs = plan indices (-1: the neck output),
    a decoder block's first conv takes [cur, skip]"""
    plan = []

    def conv(key, kind, relu, inputs, h):
        plan.append((key, kind, relu, inputs, h))
        return len(plan) - 1

    cur, h, feats = -1, 32, []
    for i in range(len(fts)):
        p = f"out_class.encoder_blocks.{i}."
        t = conv(p + "block.conv1", 0, True, [cur], h)
        t = conv(p + "block.conv2", 0, True, [t], h)
        cur = conv(p + "downconv", 1, False, [t], h)
        h //= 2
        feats.append(cur)
    feats = feats[::-1]
    p = "out_class.bottleneck_down."
    t = conv(p + "block.conv1", 0, True, [cur], h)
    t = conv(p + "block.conv2", 0, True, [t], h)
    cur = conv(p + "downconv", 1, False, [t], h)
    h //= 2
    p = "out_class.bottleneck_up."
    t = conv(p + "block.conv1", 0, True, [cur], h)
    t = conv(p + "block.conv2", 0, True, [t], h)
    cur = conv(p + "upconv", 2, False, [t], h)
    h *= 2
    n = len(fts)
    for i in range(n):
        p = f"out_class.decoder_blocks.{i}."
        t = conv(p + "block.conv1", 0, True, [cur, feats[i]], h)
        t = conv(p + "block.conv2", 0, i != n - 1, [t], h)
        cur = conv(p + "upconv", 2, False, [t], h)
        h *= 2
    assert h == 32
    return plan


def _run_head(w, feat, nS, fill, dev):
    L = _lib.lib()
    c = w.c
    dt = c.dtype
    nbytes = L.cpx_unet_workspace_bytes(c.unet_ops, c.n_unet_ops, nS, dt)
    ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    head = torch.full((nS * 1024 + 64, c.ld_head), SENT, dtype=torch.float32, device=dev)
    _lib.check(L.cpx_unet_head_forward(c.unet_ops, c.n_unet_ops, ptr(feat), nS, ptr(head), c.ld_head, 192, dt, ptr(ws), nbytes,
                                       torch.cuda.current_stream(dev).cuda_stream), "unet_head_forward")
    torch.cuda.synchronize(dev)
    return ws, head


def _layout(w, nS):
    n = w.c.n_unet_ops
    off, ld = (C.c_size_t * n)(), (C.c_int * n)()
    with _lib.use_debug_library() as L:
        _lib.check(L.cpx_unet_head_layout(w.c.unet_ops, n, nS, w.c.dtype, off, ld), "unet_head_layout")
    return list(off), list(ld)


def _tensor(ws, off, ld, rows, cols, hd):
    es = torch.finfo(hd).bits // 8
    rows_pad = (rows + 127) // 128 * 128
    return ws[off:off + rows_pad * ld * es].view(hd).reshape(rows_pad, ld)[:rows, :cols]


def _nchw(t, nS, h):
    return t.double().cpu().reshape(nS, h, h, -1).permute(0, 3, 1, 2)


def _tokens(x):
    return x.permute(0, 2, 3, 1).reshape(-1, x.shape[1])


def check_unet(ncls, fts, prec, nS, dev):
    """every op's valid outputs within the bound, padded channels exactly 0, class columns of the head == the last op
    widened, sentinels elsewhere; the same head bit for bit from a zero-filled workspace.  Returns (worst ratio, routes)."""
    sd, w = _weights(ncls, fts, prec, dev)
    hd = HD[prec]
    c = w.c
    out_ch = ncls * 64
    plan = _plan(fts, out_ch)
    assert c.n_unet_ops == len(plan)
    g = torch.Generator(device=dev).manual_seed(nS * 7 + len(fts))
    feat = torch.randn(nS * 1024, 256, generator=g, device=dev).to(hd)
    ws, head = _run_head(w, feat, nS, 0xFF, dev)
    off, ld = _layout(w, nS)
    opsl = [c.unet_ops[i] for i in range(c.n_unet_ops)]
    outs = {-1: _nchw(feat, nS, 32)}                                          # plan index -> float64 NCHW (valid channels)
    worst, routes = 0.0, []
    last = len(plan) - 1
    for i, (key, kind, relu, inputs, h) in enumerate(plan):
        o = opsl[i]
        assert (o.kind, o.relu, o.h) == (kind, int(relu), h), (key, o.kind, o.relu, o.h)
        wt = sd[key + ".weight"].to(hd).double()
        b = sd[key + ".bias"].to(hd).double()
        x = torch.cat([outs[j] for j in inputs], 1)
        taps = {0: 9, 1: 4, 2: 1}[kind]
        K = (taps * (o.cin_a + o.cin_b) + 63) // 64 * 64
        if kind == 0:
            z, az = F.conv2d(x, wt, b, padding=1), F.conv2d(x.abs(), wt.abs(), padding=1)
        elif kind == 1:
            z, az = F.conv2d(x, wt, b, stride=2), F.conv2d(x.abs(), wt.abs(), stride=2)
        else:
            z, az = F.conv_transpose2d(x, wt, b, stride=2), F.conv_transpose2d(x.abs(), wt.abs(), stride=2)
        cout, ho = z.shape[1], z.shape[2]
        rows = nS * ho * ho
        ref = z.clamp_min(0) if relu else z
        d = K * U * az + (U * z.abs() if hd != torch.float32 else 0)
        bd = 0.5 * nm.ulp(ref.abs() + d, hd) + d
        M_gemm = (nS * (h * h if kind == 2 else ho * ho) + 127) // 128 * 128
        N_gemm = ((4 * o.cout if kind == 2 else o.cout) + 127) // 128 * 128
        big = bool(_lib.lib().cpx_gemm_uses_big_tile(M_gemm, N_gemm, K, ops.EPI["relu" if relu else "bf16"])) and hd != torch.float32
        routes.append("256^2" if big else ("128^2 f32" if hd == torch.float32 else "128^2"))
        if i == last:                                     # GEMM output before depth-to-space: [rows_in][tap * cout + co]
            rin = nS * h * h
            gb = _tensor(ws, off[i], ld[i], rin, 4 * o.cout, hd)
            got = gb.reshape(nS, h, h, 2, 2, o.cout).permute(0, 1, 3, 2, 4, 5).reshape(rows, o.cout)
            last_got = got
        else:
            got = _tensor(ws, off[i], ld[i], rows, o.cout, hd)
        assert o.cout == (cout + 7) // 8 * 8, (key, o.cout, cout)
        pad = got[:, cout:]
        assert not bool(pad.float().any()), f"{key}: padded channels {cout}..{o.cout - 1} not 0 ({prec} fts {fts} nS={nS})"
        gv = got[:, :cout]
        assert bool(torch.isfinite(gv).all()), f"{key}: non-finite valid output ({prec} fts {fts} nS={nS})"
        what = f"{prec} fts {fts} nS={nS} op {i} {key} ({routes[-1]})"
        refk, bdk = _tokens(ref).to(dev), _tokens(bd).to(dev)
        nm.check(gv, refk, bdk, dtype=hd, rms_limit=None, what=what)
        worst = max(worst, float(((gv.double() - refk).abs() / bdk).max()))
        outs[i] = _nchw(gv, nS, ho)
    # the head: class columns == the last op's output widened exactly; every other column and the guard rows keep SENT
    M = nS * 1024
    cls = head[:M, 192:192 + out_ch]
    assert torch.equal(cls, last_got.float()), f"{prec} fts {fts} nS={nS}: class columns != last op widened"
    s = torch.tensor(SENT, device=dev)
    for name, t in (("columns < 192", head[:M, :192]), ("columns past the classes", head[:M, 192 + out_ch:]), ("guard rows", head[M:])):
        assert bool((t == s).all()), f"{prec} fts {fts} nS={nS}: head {name} overwritten"
    _, head0 = _run_head(w, feat, nS, 0x00, dev)
    assert torch.equal(head0, head), f"{prec} fts {fts} nS={nS}: head depends on the workspace contents"
    return worst, routes


FTS = [[64, 128], [20, 36], [12, 20, 36, 68], [64, 128, 256, 512]]


@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("fts", FTS, ids=lambda f: "-".join(map(str, f)))
@pytest.mark.parametrize("nS", [1, 3])
def test_unet_every_element(cuda, prec, fts, nS):
    worst, routes = check_unet(3, fts, prec, nS, cuda)
    print(f"unet {prec} fts {fts} nS={nS}: {len(routes)} ops, worst err/bound {worst:.3f}, routes {sorted(set(routes))}")


@pytest.mark.parametrize("prec", ["bf16", "fp16"])
def test_unet_every_element_big_tile_last_gemm(cuda, prec):
    """10 classes at 32 sub-tiles: the last transposed conv's GEMM (Mp 8192, Np 2560, Kp 640) takes the 256^2 kernel"""
    assert _lib.lib().cpx_gemm_uses_big_tile(8192, 2560, 640, ops.EPI["bf16"])
    worst, routes = check_unet(10, [64, 128], prec, 32, cuda)
    assert routes[-1] == "256^2", routes
    print(f"unet {prec} 10 classes nS=32: worst err/bound {worst:.3f}, routes {routes}")


# ---- the network forward on a poisoned workspace -------------------------------------------------------------------------
@pytest.mark.parametrize("prec", ["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("fts", [None, [64, 128]], ids=["1x1 head", "unet head"])
def test_net_forward_poisoned_workspace(cuda, prec, fts):
    """cpx_net_forward at depth 2, nS = 3 (bf16: LayerNorm folded) with the network workspace filled with 0x00 and then
    0xFF bytes: the whole head is bit for bit the same and finite (the network kernels read nothing they did not write)"""
    nS = 3
    sd = synth.make_state_dict(7, fts, depth=2, seed=5)
    w = engine.NetWeights.from_state_dict(sd, prec, cuda)
    assert bool(w.c.fuse_ln) == (prec == "bf16" or prec == "fp16")
    L = _lib.lib()
    g = torch.Generator(device=cuda).manual_seed(3)
    patches = torch.rand(nS * 1024, 192, generator=g, device=cuda).to(HD[prec])
    nbytes = L.cpx_net_workspace_bytes(nS, w.c.dtype)
    if w.c.n_unet_ops:
        nbytes += L.cpx_unet_workspace_bytes(w.c.unet_ops, w.c.n_unet_ops, nS, w.c.dtype)
    heads = []
    for fill in (0x00, 0xFF):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=cuda)
        head = torch.full((nS * 1024, w.c.ld_head), SENT, dtype=torch.float32, device=cuda)
        _lib.check(L.cpx_net_forward(C.byref(w.c), ptr(patches), nS, ptr(head), ptr(ws), nbytes,
                                     torch.cuda.current_stream(cuda).cuda_stream), "net_forward")
        torch.cuda.synchronize(cuda)
        heads.append(head)
    assert bool(torch.isfinite(heads[0]).all()) and bool(torch.isfinite(heads[1]).all())
    if not torch.equal(heads[0], heads[1]):
        bad = (heads[0] != heads[1]).nonzero()
        raise AssertionError(f"{prec} {fts}: {bad.shape[0]} head elements depend on the workspace, first {bad[0].tolist()}")
    print(f"poisoned workspace {prec} {'unet' if fts else '1x1'} head: {nbytes} bytes, head bitwise equal and finite")
