"""The float32 network path (csrc/cpx_net_f32.hip, --precision fp32) element by element.

k_gemm_f32 on INTEGER operands: with K * amax * wmax < 2^24 every partial sum is an integer a float32 accumulator holds
exactly, whatever order the MFMAs sum in, so each bitwise epilogue has a bitwise reference computed in torch float32 in
the kernel's own order from the exact accumulator (none: acc; bias: f32(acc + b); relu; resid: f32(f32(acc + b) + aux);
pos: f32(f32(acc + b) + pos[row % 1024]) with pos rows N wide).  These epilogues contain no products, so FMA contraction
(cpx_net_f32.hip is not built with -ffp-contract=off) cannot change them.  Guard columns (ld_out > N) and guard rows
must keep their sentinel.  GELU, LayerNorm and attention are checked against float64 with bounds derived from the
kernels' arithmetic that hold with or without FMA contraction (u = 2^-24); every bound is 1/2 ulp_f32(|ref| + d) + d with
d the kernel's error before its final rounding.  k_im2col3_f32 and the fp16 / fp32 patch rows must be bit exact."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from classpose_amd import _lib, ops, synth
from classpose_amd._lib import ptr
from oracle import numerics as nm
from oracle import tiling

pytestmark = pytest.mark.gpu

F32 = torch.float32
U = 2.0 ** -24
SENT = -7777.25                                  # guard sentinel (exact in float32)
CHUNK_BYTES = 1 << 30


@pytest.fixture(autouse=True)
def _no_tf32():
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = saved


def _gen(dev, seed):
    return torch.Generator(device=dev).manual_seed(seed)


def _ints(shape, amax, g, dev):
    return torch.randint(-amax, amax + 1, shape, generator=g, device=dev).float()


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _bound(ref, d):
    return 0.5 * nm.ulp(ref.abs() + d, F32) + d


def _chunks(M, N):
    rows = max(128, (CHUNK_BYTES // (N * 8)) // 128 * 128)
    for r0 in range(0, M, rows):
        yield r0, min(M, r0 + rows)


def _sentinel_kept(buf, valid_rows, valid_cols, what):
    """everything of buf outside [:valid_rows, :valid_cols] still holds SENT, bit for bit"""
    s = torch.tensor(SENT, dtype=F32, device=buf.device)
    gr = buf[valid_rows:]
    gc = buf[:valid_rows, valid_cols:]
    for name, t in (("guard rows", gr), ("guard columns", gc)):
        if t.numel():
            bad = (t != s).nonzero()
            assert bad.numel() == 0, f"{what}: {name} overwritten, first at {bad[0].tolist()} (of the guard block)"


# ---- GEMM ---------------------------------------------------------------------------------------------------------------
def _gemm_f32(A, W, epi, bias, aux, out, ld_out):
    M, K = A.shape
    N = W.shape[0]
    _lib.check(_lib.lib().cpx_gemm(_lib.DT_F32, ptr(A), ptr(W), M, N, K, ops.EPI[epi], ptr(bias), ptr(aux), ptr(out), ld_out,
                                   _stream(A.device)), f"gemm f32 {epi}")


def _operands(M, N, K, dev, seed, bias=True):
    """integer A, W with K * amax * wmax < 2^24 and a random float32 bias (|b| ~ 100): f32(acc + b) rounds"""
    g = _gen(dev, seed)
    amax = 8 if K <= 1024 else 4
    wmax = 8 if K <= 2304 else 4
    assert K * amax * wmax < 2 ** 24
    A = _ints((M, K), amax, g, dev)
    W = _ints((N, K), wmax, g, dev)
    b = (torch.randn(N, generator=g, device=dev) * 100).float() if bias else None
    return A, W, b, g


def _gelu64(z):
    return 0.5 * z * torch.special.erfc(-z / math.sqrt(2))


def _gelu_delta(x):
    """k_gemm_f32 GELU: x = f32(acc + b) is exact input here; y = 0.5f * x * (1.0f + erff(x * 0.70710678f)).
      t = fl(x c): c = f32(1/sqrt 2) (u relative) times x (one rounding): t = (x / sqrt 2)(1 + 2u)
      E = erff(t): allowed 4 ulp (twice the 2 ulp CUDA's math library guarantees for erff); ulp(E) <= 2u |E|: 8u |erf(t)|,
          and erf(t) - erf(x / sqrt 2) <= erf'(t) |t| 2u = (2 / sqrt pi) exp(-t^2) |t| 2u
      1 + E: one rounding, <= u |1 + erf|;  0.5f * x: exact;  the last product is the final rounding (the 1/2 ulp part).
    d = 0.5 |x| (8u |erf| + 2.26 u |t| exp(-t^2) + u (1 + erf)) + (second order: 1e-3 of the same).  ABSOLUTE in the erf error:
    at negative x, 1 + erf(t) cancels to ~exp(-t^2) and its relative error is unbounded, the absolute 0.5 |x| 8u is not.  FMA
    contraction can only merge a product with the following add (erff's own polynomial into the 1 + E): one rounding fewer."""
    t = x / math.sqrt(2)
    e = torch.special.erf(t)
    d = 0.5 * x.abs() * (8 * U * e.abs() + 2.26 * U * t.abs() * torch.exp(-t * t) + U * (1 + e))
    return d * 1.001


def _ref_epilogue(acc32, epi, b, aux, r0, r1):
    """float32 epilogue in the kernel's order on the exact accumulator rows r0:r1 (torch float32 adds are IEEE RNE)"""
    z = acc32 + b if b is not None else acc32
    if epi == "relu":
        return torch.clamp_min(z, 0.0)
    if epi == "resid":
        return z + aux[r0:r1]
    if epi == "pos":
        rows = torch.arange(r0, r1, device=acc32.device) % 1024
        return z + aux[rows]
    return z


def check_gemm_f32(M, N, K, epi, dev, seed, ld_out=None, guard_rows=0, inplace=False, bias=True, what=""):
    """one k_gemm_f32 launch against its float32 / float64 reference, every element; guards keep SENT.  Returns max err / bound
    (0 for the bitwise epilogues)."""
    ld = ld_out or N
    A, W, b, g = _operands(M, N, K, dev, seed, bias)
    out = torch.full((M + guard_rows, ld), SENT, dtype=F32, device=dev)
    aux = None
    if epi == "resid":
        r = torch.randn(M, N, generator=g, device=dev) * 1000
        if inplace:
            out[:M, :N] = r
            aux = out
        else:
            aux = torch.full((M, ld), float("nan"), dtype=F32, device=dev)
            aux[:, :N] = r
        resid = r
    elif epi == "pos":
        aux = torch.randn(1024, N, generator=g, device=dev) * 1000          # [1024][N]: stride N, not ld_out
    _gemm_f32(A, W, epi, b, aux, out, ld)
    worst = 0.0
    for r0, r1 in _chunks(M, N):
        acc = (A[r0:r1].double() @ W.double().T)
        assert bool((acc.abs() < 2 ** 24).all())
        acc32 = acc.float()                                                # exact
        got = out[r0:r1, :N]
        if epi == "gelu":
            x = (acc32 + b).double()
            ref = _gelu64(x)
            d = _gelu_delta(x)
            bd = _bound(ref, d)
            nm.check(got, ref, bd, dtype=F32, rms_limit=None, what=f"{what} gelu rows {r0}..")
            worst = max(worst, float(((got.double() - ref).abs() / bd).max()))
        else:
            ref = _ref_epilogue(acc32, epi, b, resid if epi == "resid" else aux, r0, r1)
            if not torch.equal(got, ref):
                bad = (got != ref).nonzero()
                i, j = bad[0].tolist()
                raise AssertionError(f"{what} {epi}: {bad.shape[0]} elements differ; first [{r0 + i}, {j}]: got {float(got[i, j])!r}, "
                                     f"ref {float(ref[i, j])!r}")
    _sentinel_kept(out, M, N, f"{what} {epi}")
    return worst


def _blocks(M, N):
    return (M // 128) * (N // 128)


EDGES = [(128, 128, 16), (384, 640, 48), (1280, 384, 16 * 7)]


@pytest.mark.parametrize("M,N,K", EDGES)
def test_gemm_f32_edges_every_epilogue(cuda, M, N, K):
    """one block and one K step; 15 and 30 blocks (the uneven branch of the XCD block remap: n_blocks % 8 != 0); every
    epilogue with ld_out = N + 128 guard columns and 64 guard rows; the residual out of place and in place (aux == out);
    pos with its [1024][N] table (rows m % 1024: M = 1280 wraps)"""
    nb = _blocks(M, N)
    worst = 0.0
    for i, (epi, inplace, bias) in enumerate([("f32", False, False), ("f32", False, True), ("relu", False, True),
                                              ("resid", False, True), ("resid", True, True), ("pos", False, True),
                                              ("gelu", False, True)]):
        w = check_gemm_f32(M, N, K, epi, cuda, 10 * M + i, ld_out=N + 128, guard_rows=64, inplace=inplace, bias=bias,
                           what=f"({M},{N},{K}) {nb} blocks {'in place' if inplace else ''}")
        worst = max(worst, w)
    print(f"gemm f32 ({M},{N},{K}): {nb} blocks (n % 8 = {nb % 8}), ld_out {N + 128}; bitwise epilogues exact, gelu worst err/bound {worst:.3f}")


@pytest.mark.parametrize("nS", [1, 3, 32])
def test_gemm_f32_network_shapes(cuda, nS):
    """the fp32 forward's GEMMs with the epilogue each takes in the float32 cpx_net_forward: patch embedding (K 192, +b +pos),
    qkv, attn.proj (residual in place), mlp.lin1 (GELU), mlp.lin2 (K 4096, residual in place), neck0, neck2 (K 2304), and
    the head at ld_head 640 and 896"""
    M = nS * 1024
    cases = [("patch", 1024, 192, "pos", False, True), ("qkv", 3072, 1024, "f32", False, True),
             ("proj", 1024, 1024, "resid", True, True), ("fc1", 4096, 1024, "gelu", False, True),
             ("fc2", 1024, 4096, "resid", True, True), ("neck0", 256, 1024, "f32", False, False),
             ("neck2", 256, 2304, "f32", False, False), ("head 640", 640, 256, "f32", False, True),
             ("head 896", 896, 256, "f32", False, True)]
    for i, (name, N, K, epi, inplace, bias) in enumerate(cases):
        w = check_gemm_f32(M, N, K, epi, cuda, 1000 * nS + i, inplace=inplace, bias=bias, guard_rows=16,
                           what=f"nS={nS} {name}")
        print(f"gemm f32 nS={nS} {name}: M {M} N {N} K {K} {epi}{' in place' if inplace else ''}, {_blocks(M, N)} blocks"
              + (f", gelu worst err/bound {w:.3f}" if epi == "gelu" else ", bit exact"))


def test_gemm_f32_gelu_every_element(cuda):
    """GELU over pre-activations spread across [-12, 12] (integer accumulators + a fractional bias), both signs, against
    float64 0.5 x (1 + erf(x / sqrt 2)) within the bound of _gelu_delta"""
    M, N, K = 2048, 1024, 1024
    g = _gen(cuda, 5)
    idx = torch.randint(0, 64, (M, K // 64, 1), generator=g, device=cuda)
    A = torch.zeros(M, K // 64, 64, device=cuda).scatter_(2, idx, torch.randint(-1, 2, (M, K // 64, 1), generator=g, device=cuda).float()).reshape(M, K)
    W = _ints((N, K), 1, g, cuda)
    b = torch.linspace(-12, 12, N, device=cuda) + torch.rand(N, generator=g, device=cuda) * 2 ** -6
    out = torch.full((M, N), SENT, dtype=F32, device=cuda)
    _gemm_f32(A, W, "gelu", b, None, out, N)
    x = ((A.double() @ W.double().T).float() + b).double()
    ref = _gelu64(x)
    d = _gelu_delta(x)
    bd = _bound(ref, d)
    nm.check(out, ref, bd, dtype=F32, rms_limit=None, what="gemm f32 gelu")
    r = (out.double() - ref).abs() / bd
    neg = x < -3
    print(f"gelu f32: worst err/bound {float(r.max()):.3f} (x < -3: {float(r[neg].max()):.3f}), "
          f"max |err| {float((out.double() - ref).abs().max()):.3g}")


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------
CONDITION = ["0", "1", "10", "100", "constant", "outlier"]


def _conditioned_rows(M, C, dev, seed):
    """row groups (cycled over the rows): |mean| / std in {0, 1, 10, 100}, constant rows, one channel at +300 sigma"""
    g = _gen(dev, seed)
    x = torch.randn(M, C, generator=g, device=dev)
    grp = torch.arange(M, device=dev) % len(CONDITION)
    for i, c in enumerate(CONDITION):
        r = grp == i
        if c in ("0", "1", "10", "100"):
            x[r] = x[r] - x[r].mean(1, keepdim=True) + float(c)
        elif c == "constant":
            x[r] = torch.randn(int(r.sum()), 1, generator=g, device=dev) * 3
        else:
            x[r, 5] += 300
    return x, grp


def _ln32_delta(x, w, b):
    """k_layernorm_f32: one wave per row, D = C / 64 values per lane.
      mean: per lane D - 1 adds, a 6-step butterfly, * (1 / C) (exact): e_m <= (D + 6) u sum|x| / C
      q = sum (x - mean_c)^2: d_i = fl(x_i - mean_c) (u), D products / FMAs per lane + 6 butterfly adds: relative (D + 9) u,
          and the shifted mean adds exactly C e_m^2 (the cross term sum (x - mean) = 0)
      var + eps = fma(q, 1 / C, eps) (one rounding: u); sqrtf and 1.0f / s are correctly rounded on gfx950 (v_sqrt_f32 with
          its +-1 ulp fix-up, the v_div_scale / v_div_fmas / v_div_fixup sequence): 2u
          -> rho = [(D + 9) u var + e_m^2] / (var + eps) / 2 + u / 2 + 2u   (relative error of rstd)
      y = (x - mean_c) rstd w + b: the subtraction, two products (or one FMA) and the add: 3u, plus the mean shift e_m rstd |w|
    d = 2 [ |x - mean| rstd |w| (rho + 3u) + e_m rstd |w| + u (|y| + |b|) ]   (2x for second-order terms)"""
    C = x.shape[1]
    D = C / 64
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    dd = xd - mean
    var = (dd * dd).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-6)
    y = dd * rstd * w.double() + b.double()
    e_m = (D + 6) * U * xd.abs().sum(1, keepdim=True) / C
    rho = ((D + 9) * U * var + e_m * e_m) / (var + 1e-6) / 2 + 2.5 * U
    aw = w.double().abs()
    d = 2 * (dd.abs() * rstd * aw * (rho + 3 * U) + e_m * rstd * aw + U * (y.abs() + b.double().abs()))
    return y, d


@pytest.mark.parametrize("C", [1024, 256])
def test_layernorm_f32_every_row(cuda, C):
    """cpx_layernorm (float32, two-pass) on every row of every conditioning group, with row counts = 1, 2, 3 mod 4 (the last
    workgroup's idle waves) and 8 guard rows after them"""
    g = _gen(cuda, C)
    w = 1 + 0.2 * torch.randn(C, generator=g, device=cuda)
    b = 0.2 * torch.randn(C, generator=g, device=cuda)
    worst = {}
    for rows in (6 * 64 + 1, 6 * 128 + 2, 6 * 256 + 3):
        assert rows % 4 in (1, 2, 3)
        x, grp = _conditioned_rows(rows, C, cuda, rows + C)
        out = torch.full((rows + 8, C), SENT, dtype=F32, device=cuda)
        _lib.check(_lib.lib().cpx_layernorm(_lib.DT_F32, ptr(x), ptr(w), ptr(b), rows, C, 1e-6, ptr(out), _stream(cuda)), "ln f32")
        ref, d = _ln32_delta(x, w, b)
        bd = _bound(ref, d)
        nm.check(out[:rows], ref, bd, dtype=F32, rms_limit=None, what=f"layernorm f32 C={C} rows={rows}")
        _sentinel_kept(out, rows, C, f"layernorm f32 C={C} rows={rows}")
        r = (out[:rows].double() - ref).abs() / bd
        for i, c in enumerate(CONDITION):
            worst[c] = max(worst.get(c, 0.0), float(r[grp == i].max()))
    print(f"layernorm f32 C={C}: worst err/bound per group " + ", ".join(f"{k}: {v:.3f}" for k, v in worst.items()))


# ---- attention ----------------------------------------------------------------------------------------------------------
def _attn_case(case, nS, dev):
    g = _gen(dev, nS * 31 + len(case))
    M = nS * 1024
    qkv = torch.randn(M, 3072, generator=g, device=dev)
    rh = torch.randn(63, 64, generator=g, device=dev) * 0.3
    rw = torch.randn(63, 64, generator=g, device=dev) * 0.3
    if case == "uniform":                        # q = 0: every logit 0 -> the output is the mean of V over the sub-tile
        qkv[:, :1024] = 0
    elif case == "spiked":                       # one key dominates every head: the online-softmax rescale path
        qkv[:, :1024] = 1.0
        qkv[700::1024, 1024:2048] = 30.0
        qkv[:, 1024:2048] *= 0.1
        rh.zero_(); rw.zero_()
    elif case == "ramp":                         # logits rising along the keys: the running maximum moves in every key tile
        t = torch.arange(M, device=dev).float() % 1024
        qkv[:, :1024] = 0.5
        qkv[:, 1024:2048] = (t / 128)[:, None] + 0.05 * qkv[:, 1024:2048]
    elif case == "wide":                         # logits spanning +-60
        qkv[:, :2048] *= 2.2
        rh *= 3; rw *= 3
    pad = lambda t: torch.cat([t * 8, torch.zeros(1, 64, device=dev)])
    return qkv, rh, rw, pad(rh), pad(rw)


def _attn32_ref_bound(qkv, rh, rw, s):
    """sub-tile s, float64: out [1024 tokens][16 heads][64] and the bound d of k_attention_f32.  Logits (x8 scaled in the kernel,
    exact) x = q.k / 8 + q.Rh + q.Rw: G = Q table^T and S = K Q^T + Gw are chains of 64 float32 FMAs (v_mfma_f32_32x32x2_f32),
    stored in float32 (LDS): eps = 66 u (|q|.|k| / 8 + |q|.|Rh| + |q|.|Rw|).  P = exp2(fma(S, c, (gh - m) c)): three roundings
    on |x| + |m| and exp2 (<= 2 ulp): 4u (|x| + |m|) + 4u; each running-max rescale alpha = exp2((m_old - m_new) c) adds 2u
    |m_old - m_new| (telescoping: <= 2u (max|x| + |m|)) + 4u, 32 key tiles: r = eps + 4u |x| + 8u max|x| + 136u.
    Relative errors r_j of P_j move out = sum P v / l by <= sum P_j r_j (|v_j| + |out|) / l.  O and l are chains through all
    1024 keys (32 tiles x (32 keys + the rescale)): <= 1060u P|V| / l and 1060u |out|; O / l: u.
        d = [(P r) |V| + |out| (P r).sum + 1060u P |V|] / l + 1061u |out|"""
    H = 16
    blk = qkv[s * 1024:(s + 1) * 1024].double().reshape(1024, 3, H, 64).permute(1, 2, 0, 3)
    q, k, v = blk[0], blk[1], blk[2]
    idx = (torch.arange(32)[:, None] - torch.arange(32)[None, :] + 31).to(qkv.device)
    Rh, Rw = rh.double()[idx], rw.double()[idx]
    qhw = q.reshape(H, 32, 32, 64)
    bh = torch.einsum("nhwc,hkc->nhwk", qhw, Rh)
    bw = torch.einsum("nhwc,wkc->nhwk", qhw, Rw)
    x = q @ k.transpose(-1, -2) * 0.125 + (bh[..., :, None] + bw[..., None, :]).reshape(H, 1024, 1024)
    aq = q.abs().reshape(H, 32, 32, 64)
    ab = torch.einsum("nhwc,hkc->nhwk", aq, Rh.abs())
    aw = torch.einsum("nhwc,wkc->nhwk", aq, Rw.abs())
    eps = 66 * U * (q.abs() @ k.abs().transpose(-1, -2) * 0.125 + (ab[..., :, None] + aw[..., None, :]).reshape(H, 1024, 1024))
    m = x.amax(-1, keepdim=True)
    xmax = x.abs().amax(-1, keepdim=True)
    P = torch.exp(x - m)
    l = P.sum(-1, keepdim=True)
    out = (P @ v) / l
    r = eps + 4 * U * x.abs() + 8 * U * xmax + 136 * U
    Pr = P * r
    d = (Pr @ v.abs() + out.abs() * Pr.sum(-1, keepdim=True) + 1060 * U * (P @ v.abs())) / l + 1061 * U * out.abs()
    tr = lambda t: t.permute(1, 0, 2).reshape(1024, 1024)
    return tr(out), tr(d)


@pytest.mark.parametrize("nS", [1, 3, 18])
def test_attention_f32_every_element(cuda, nS):
    """cpx_attention (float32, k_attention_f32): every element of every sub-tile and head against float64 within
    _attn32_ref_bound, for random, uniform (q = 0), spiked, ramp and wide (logits +-60) inputs; RMS(err / bound) over the 64
    channels of each (token, head) <= 0.5 (a systematic per-head fault -- a wrong scale, a dropped key tile -- reaches 1)"""
    for case in ["random", "uniform", "spiked", "ramp", "wide"]:
        qkv, rh, rw, ph, pw = _attn_case(case, nS, cuda)
        out = ops.attention(qkv, ph, pw)
        worst = worst_rms = 0.0
        for s in range(nS):
            ref, d = _attn32_ref_bound(qkv, rh, rw, s)
            got = out[s * 1024:(s + 1) * 1024]
            bd = _bound(ref, d)
            nm.check(got, ref, bd, dtype=F32, rms_limit=None, what=f"attention f32 {case} nS={nS} sub-tile {s}")
            rr = ((got.double() - ref).abs() / bd).reshape(1024, 16, 64)
            rms = rr.pow(2).mean(-1).sqrt()
            worst, worst_rms = max(worst, float(rr.max())), max(worst_rms, float(rms.max()))
            assert float(rms.max()) <= 0.5, (case, s, divmod(int(rms.argmax()), 16), float(rms.max()))
        print(f"attention f32 nS={nS} {case}: worst err/bound {worst:.4f}, worst (token, head) RMS {worst_rms:.4f}")


# ---- im2col and patch rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS", [1, 3])
def test_im2col3_f32_exact(cuda, nS):
    """k_im2col3_f32 (cpx_im2col3_f32_debug) == the zero-padded 3 x 3 unfold of each 32 x 32 image, k = tap * 256 + c, bit
    for bit; 32 guard rows after the output keep their sentinel"""
    M = nS * 1024
    x = torch.randn(M, 256, generator=_gen(cuda, nS), device=cuda)
    out = torch.full((M + 32, 2304), SENT, dtype=F32, device=cuda)
    with _lib.use_debug_library() as L:
        _lib.check(L.cpx_im2col3_f32_debug(ptr(x), nS, ptr(out), _stream(cuda)), "im2col3_f32")
    img = x.reshape(nS, 32, 32, 256).permute(0, 3, 1, 2)
    u = F.unfold(img, 3, padding=1)                                   # [nS][256 * 9 (c, ky, kx)][1024]
    ref = u.reshape(nS, 256, 9, 1024).permute(0, 3, 2, 1).reshape(M, 2304)
    if not torch.equal(out[:M], ref):
        bad = (out[:M] != ref).nonzero()
        i, j = bad[0].tolist()
        raise AssertionError(f"im2col3 nS={nS}: {bad.shape[0]} elements differ, first [{i}, {j}] (token {i % 1024}, tap {j // 256}, "
                             f"channel {j % 256}): got {float(out[i, j])!r}, ref {float(ref[i, j])!r}")
    _sentinel_kept(out, M, 2304, f"im2col3 nS={nS}")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("H,W,aug", [(256, 256, False), (256, 256, True), (300, 260, False), (300, 260, True)])
def test_make_patches_fp16_fp32_bit_exact(cuda, H, W, aug, dtype):
    """k_make_patches<1> / <2>: the fp16 / fp32 patch rows == the oracle's sub-tiles cast with .to(), in im2col order"""
    t = np.stack([synth.render_region(1234 + i, 300 * i, 17 * i, W, H) for i in range(2)])
    pat, _ = ops.make_patches(torch.from_numpy(t).to(cuda), 256, aug, dtype=dtype)
    x = np.concatenate([tiling.normalize_img(t[i:i + 1]) for i in range(2)])
    ref = np.concatenate([tiling.subtile_batch(x[i:i + 1], 256, aug)[0] for i in range(2)])
    nS = ref.shape[0]
    exp = torch.from_numpy(ref).reshape(nS, 3, 32, 8, 32, 8).permute(0, 2, 4, 1, 3, 5).reshape(nS * 1024, 192).to(dtype)
    got = pat.cpu()
    assert got.dtype == dtype
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero()
        i, j = bad[0].tolist()
        raise AssertionError(f"patches {dtype} {H}x{W} aug={aug}: {bad.shape[0]} differ, first row {i} col {j}: "
                             f"got {float(got[i, j])!r}, ref {float(exp[i, j])!r}")
