"""Real-valued data against float64, every element: production attention (attn2w), cpx_layernorm (two-pass) and the
LayerNorm folded into the GEMM (cpx_row_stats + one-pass variance in the epilogue), with bounds derived from each
kernel's arithmetic (u = 2^-24, the fp32 unit roundoff; u_h = 2^-8 bf16 / 2^-11 fp16, the half type's).  Every bound
is  1/2 ulp(|ref| + d) + d  with d the kernel's pre-rounding error, stated per test."""
import math

import pytest
import torch

from classpose_amd import _lib, ops
from oracle import numerics as nm

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
UH = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _no_tf32():
    saved = torch.backends.cuda.matmul.allow_tf32
    torch.backends.cuda.matmul.allow_tf32 = False
    yield
    torch.backends.cuda.matmul.allow_tf32 = saved


def _bound(ref, d, hd, base=0.5):
    return base * nm.ulp(ref.abs() + d, hd)


# ---- attention -------------------------------------------------------------------------------------------------------
def _attn_case(case, nS, hd, dev):
    g = torch.Generator(device=dev).manual_seed(nS * 31 + len(case))
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
    elif case == "wide":                         # fp16: logits spanning +-60 (q.k / 8 up to ~60, relative-position bias ~+-10)
        qkv[:, :2048] *= 2.2
        rh *= 3; rw *= 3
    qkv = qkv.to(hd)
    rh, rw = rh.to(hd), rw.to(hd)
    pad = lambda t: torch.cat([t.float() * 8, torch.zeros(1, 64, device=dev)]).to(hd)
    return qkv, rh, rw, pad(rh), pad(rw)


def _attn_ref_bound(qkv, rh, rw, s, hd):
    """sub-tile s, float64: out [1024 tokens][16 heads][64] and the bound d.  The kernel: logits x = q.k / 8 + q.Rh + q.Rw
    in fp32 (64-term dot products, <= 40 roundings deep with the scale and the sums: 40 u (|q|.|k| / 8 + |q|.|Rh| + |q|.|Rw|)),
    except that both relative-position terms pass through an fp16 scratch (G = Q table^T, csrc/cpx_attn2w.hip) in BOTH
    precisions: + 2^-11 (|q.Rh| + |q.Rw|); together eps = |dx|.  In fp16 that term dominates the whole error (measured:
    ~8x the P-rounding term on random inputs) -- the fp16 path is as exact as its bias scratch, not as its P; P = exp(x - m) in fp32 (exp2 to ~2 ulp, the scaling by log2 e: 4u |x|), rounded to the half type for
    the PV MFMA (u_h relative; fp16 below 2^-24 flushes: 2^-24 |v| absolute); O and l summed in fp32 (1024 terms, <= 40
    roundings deep), O / l (2u).  Sensitivity of out = sum P v / l to a relative error r_j of each P_j: <= 2 max r (P|V|)/l, so
        d = (u_h + 2 eps + 8u |x| + 80 u) (P|V|) / l + [fp16] 2^-24 sum|V| / l + 2u |out|."""
    H = 16
    blk = qkv[s * 1024:(s + 1) * 1024].double().reshape(1024, 3, H, 64).permute(1, 2, 0, 3)   # [3][H][L][64]
    q, k, v = blk[0], blk[1], blk[2]
    idx = (torch.arange(32)[:, None] - torch.arange(32)[None, :] + 31).to(qkv.device)
    Rh, Rw = rh.double()[idx], rw.double()[idx]                          # [32 (h)][32 (k_h)][64]
    qhw = q.reshape(H, 32, 32, 64)
    bh = torch.einsum("nhwc,hkc->nhwk", qhw, Rh)
    bw = torch.einsum("nhwc,wkc->nhwk", qhw, Rw)
    x = q @ k.transpose(-1, -2) * 0.125 + (bh[..., :, None] + bw[..., None, :]).reshape(H, 1024, 1024)
    aq = q.abs().reshape(H, 32, 32, 64)
    ab = torch.einsum("nhwc,hkc->nhwk", aq, Rh.abs())
    aw = torch.einsum("nhwc,wkc->nhwk", aq, Rw.abs())
    eps = 40 * U * (q.abs() @ k.abs().transpose(-1, -2) * 0.125 + (ab[..., :, None] + aw[..., None, :]).reshape(H, 1024, 1024))
    eps = eps + 2.0 ** -11 * (bh.abs()[..., :, None] + bw.abs()[..., None, :]).reshape(H, 1024, 1024)   # G = Q.table^T kept in fp16
    m = x.amax(-1, keepdim=True)
    P = torch.exp(x - m)
    l = P.sum(-1, keepdim=True)
    out = (P @ v) / l
    uh = UH[hd]
    d = (P * (uh + 2 * eps + 8 * U * x.abs() + 80 * U)) @ v.abs() / l + 2 * U * out.abs()
    if hd == torch.float16:
        d = d + 2.0 ** -24 * v.abs().sum(-2, keepdim=True) / l
    tr = lambda t: t.permute(1, 0, 2).reshape(1024, 1024)               # [token][head * 64 + d], the kernel's layout
    return tr(out), tr(d)


@pytest.mark.parametrize("dtn", ["bf16", "fp16"])
@pytest.mark.parametrize("nS", [1, 18, 32])
def test_attention_every_element(cuda, nS, dtn):
    """production attention (cpx_attention, attn2w), every element of every sub-tile and head against float64 with the bound
    of _attn_ref_bound, for random, uniform (q = 0), spiked, ramp and -- fp16 -- logits spanning +-60.  RMS gate per (token,
    head): the bound adds worst-case magnitudes, the real errors have partly random signs, so RMS(err / bound) over the 64
    channels of one (token, head) stays well below 1 (limit 0.5; measured worst 0.27, fp16 "wide"; 0.58 before the fp16-scratch term was in the
    bound); a systematic per-head fault (a wrong scale, a dropped key tile) pushes it to 1 and beyond."""
    hd = DT[dtn]
    cases = ["random", "uniform", "spiked", "ramp"] + (["wide"] if dtn == "fp16" else [])
    for case in cases:
        qkv, rh, rw, ph, pw = _attn_case(case, nS, hd, cuda)
        out = ops.attention(qkv, ph, pw)
        worst = 0.0
        for s in range(nS):
            ref, d = _attn_ref_bound(qkv, rh, rw, s, hd)
            got = out[s * 1024:(s + 1) * 1024]
            b = _bound(ref, d, hd)
            nm.check(got, ref, b, atol=d, rms_limit=None, what=f"attention {dtn} {case} nS={nS} sub-tile {s}")
            r = ((got.double() - ref).abs() / (b + d)).reshape(1024, 16, 64)
            rms = r.pow(2).mean(-1).sqrt()
            worst = max(worst, float(rms.max()))
            assert float(rms.max()) <= 0.5, (case, s, divmod(int(rms.argmax()), 16), float(rms.max()))
        print(f"attention {dtn} nS={nS} {case}: worst (token, head) RMS(err / bound) {worst:.3f}")


# ---- LayerNorm: two-pass kernel, and the one-pass fold -----------------------------------------------------------------
CONDITION = ["0", "1", "10", "100", "constant", "outlier"]


def _conditioned_rows(M, C, hd, dev, seed):
    """row groups (cycled over the rows): |mean| / std in {0, 1, 10, 100}, constant rows, one channel at +300 sigma"""
    g = torch.Generator(device=dev).manual_seed(seed)
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
    return x.to(hd), grp


def _ln_ref(x, w, b):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    d = xd - mean
    var = (d * d).mean(1, keepdim=True)
    rstd = 1 / torch.sqrt(var + 1e-6)
    return d * rstd * w.double() + b.double(), d, rstd


def _ln_delta(x, w, b):
    """k_layernorm (csrc/cpx_net.hip): per lane C/64 values summed in order, then a 6-step butterfly: a sum <= C/64 + 6
    roundings deep.  mean: e_m <= (C/64 + 7) u sum|x| / C; q = sum (x - mean)^2 the same depth + 2; rstd = rsqrt(q / C + eps):
    rel <= (C/64 + 9) u / 2 + 3u (v_rsq 1 ulp, the division, the eps add); y = (x - mean) rstd w + b: 4u more.
        d = 2 [ |x - mean| rstd |w| ((C/64 + 9) u / 2 + 7u) + e_m rstd |w| + u (|y| + |b|) ]  (2x for the terms' own roundings)"""
    C = x.shape[1]
    y, dd, rstd = _ln_ref(x, w, b)
    depth = C / 64
    e_m = (depth + 7) * U * x.double().abs().sum(1, keepdim=True) / C
    aw = w.double().abs()
    return y, 2 * (dd.abs() * rstd * aw * ((depth + 9) * U / 2 + 7 * U) + e_m * rstd * aw + U * (y.abs() + b.double().abs()))


@pytest.mark.parametrize("dtn", ["bf16", "fp16"])
@pytest.mark.parametrize("C", [1024, 256])
def test_layernorm_every_row_conditioning_sweep(cuda, C, dtn):
    """cpx_layernorm (two-pass) on every row of every conditioning group, within 1/2 ulp + d (_ln_delta) of float64"""
    hd = DT[dtn]
    M = 6 * 1024
    x, _ = _conditioned_rows(M, C, hd, cuda, C)
    g = torch.Generator(device=cuda).manual_seed(1)
    w = 1 + 0.2 * torch.randn(C, generator=g, device=cuda)
    b = 0.2 * torch.randn(C, generator=g, device=cuda)
    _check_ln(ops.layernorm(x, w, b, 1e-6), x, w, b, hd, f"layernorm C={C} {dtn}")


def _check_ln(out, x, w, b, hd, what):
    ref, d = _ln_delta(x, w, b)
    nm.check(out, ref, _bound(ref, d, hd), atol=d, rms_limit=None, what=what)
    return ref, d


def _fold_delta(x, W, cs, bias):
    """LayerNorm folded into the GEMM: cpx_row_stats sums x and x^2 in fp32 (16 values per lane + a 6-step butterfly: <= 22
    roundings deep, 24u), the epilogue forms mean = sum / K, var = max(sq / K - mean^2, 0) in fp32 -- ONE pass -- and
    z = rstd (acc - mean colsum) + b.  Error terms, float64:
      e_s = 24u sum|x|, e_q = 24u sum x^2;  e_mean = e_s / K + u |mean|;  e_var = e_q / K + 2 |mean| e_mean + 2u (sq / K + mean^2);
      rstd: the exact interval 1 / sqrt(max(var -+ e_var, 0) + 1e-6), + 3u rstd (v_rsq, the add);
      t = acc - mean colsum: acc of half products in fp32 over K (16 x 16 x 32 MFMAs chained over K / 32 steps: <= K / 32 + 8
      roundings) -> (K / 32 + 8) u sum_k |x||W|, + e_mean |colsum| + 2u |mean colsum| (colsum itself correctly rounded);
      z: d = |t| d_rstd + rstd e_t + 2u |z|.
    The mean^2 / var term is where the one-pass form is weak: it grows with (|mean| / std)^2 and, for constant rows
    (var = 0), rstd = 1000 multiplies the cancellation acc - mean colsum."""
    K = x.shape[1]
    xd, Wd = x.double(), W.double()
    s, sq = xd.sum(1, keepdim=True), (xd * xd).sum(1, keepdim=True)
    mean = s / K
    var = sq / K - mean * mean
    rstd = 1 / torch.sqrt(var.clamp_min(0) + 1e-6)
    e_mean = 24 * U * xd.abs().sum(1, keepdim=True) / K + U * mean.abs()
    e_var = 24 * U * sq / K + 2 * mean.abs() * e_mean + 2 * U * (sq / K + mean * mean)
    lo = 1 / torch.sqrt((var - e_var).clamp_min(0) + 1e-6)
    hi = 1 / torch.sqrt((var + e_var).clamp_min(0) + 1e-6)
    d_r = torch.maximum((lo - rstd).abs(), (hi - rstd).abs()) + 3 * U * rstd
    t = (xd - mean) @ Wd.T
    csd = cs.double()[None]
    e_t = (K / 32 + 8) * U * (xd.abs() @ Wd.abs().T) + e_mean * csd.abs() + 2 * U * (mean * csd).abs()
    z = rstd * t + bias.double()
    return z, t.abs() * d_r + rstd * e_t + 2 * U * z.abs()


def _unfused_delta(x, W, w_ln, b_ln, bias, hd):
    """two-pass LayerNorm (rounded to the half type) then the GEMM: d = (d_LN + 1/2 ulp(xn)) |W'|^T + (K/32 + 8) u |xn||W'|^T
    + u |z|, the bound the fused path has to meet at |mean| / std <= 10"""
    K = x.shape[1]
    xn, dln = _ln_delta(x, w_ln, b_ln)
    Wd = W.double()
    z = xn @ Wd.T + bias.double()
    d = (dln + 0.5 * nm.ulp(xn, hd)) @ Wd.abs().T + (K / 32 + 8) * U * (xn.abs() @ Wd.abs().T) + U * z.abs()
    return z, d


@pytest.mark.parametrize("dtn", ["bf16", "fp16"])
@pytest.mark.parametrize("rt", ["128^2", "k_gemm256p", "k_gemm4w"])
def test_folded_layernorm_conditioning_sweep(cuda, rt, dtn):
    """cpx_row_stats + the folded-LayerNorm GEMM (one-pass variance) on the 128^2, k_gemm256p and k_gemm4w routes against
    float64 LN(x) W^T + b: every element within the one-pass bound of _fold_delta in every conditioning group; for
    |mean| / std <= 10 also within the bound of the two-pass LayerNorm followed by the GEMM (_unfused_delta).  Where they
    part (printed): the one-pass term grows as (|mean| / std)^2 and with 1 / sqrt(eps) on constant rows."""
    hd = DT[dtn]
    M, N, K, epi = {"128^2": (2048, 1024, 1024, "bf16"), "k_gemm256p": (16384, 1024, 1024, "bf16"),
                    "k_gemm4w": (16384, 1024, 1024, "gelu")}[rt]
    big = bool(_lib.lib().cpx_gemm_uses_big_tile(M, N, K, ops.EPI[epi]))
    assert big == (rt != "128^2")
    g = torch.Generator(device=cuda).manual_seed(M + N)
    x, grp = _conditioned_rows(M, K, hd, cuda, M)
    W = (torch.randn(N, K, generator=g, device=cuda) / 32).to(hd)
    bias = torch.randn(N, generator=g, device=cuda)
    cs = W.double().sum(1).float()
    with _lib.use_debug_library():                # k_row_stats and the folded GEMM in the input's half type (cpx_*_dt, debug build)
        st = ops.row_stats(x)
        out = ops.gemm_ln(x, W, epi, bias, None, ln_stats=st, ln_colsum=cs)
    # the statistics themselves: per lane 8 pair sums added in turn (16 roundings) + a 6-step butterfly: <= 22 roundings deep (24u)
    xd = x.double()
    for k, v in ((0, xd), (1, xd * xd)):
        err = (st[:, 0, k].double() - v.sum(1)).abs()
        lim = 24 * U * v.abs().sum(1)
        assert bool((err <= lim).all()), (k, int((err - lim).argmax()), float((err - lim).max()))
    assert not bool(st[:, 1:].any())
    ones, zeros = torch.ones(K, device=cuda), torch.zeros(K, device=cuda)
    for r0 in range(0, M, 4096):
        sl = slice(r0, min(M, r0 + 4096))
        z, d = _fold_delta(x[sl], W, cs, bias)
        zu, du = _unfused_delta(x[sl], W, ones, zeros, bias, hd)
        if epi == "gelu":
            gl = lambda v: 0.5 * v * torch.special.erfc(-v / math.sqrt(2))
            z, d, zu, du, base = gl(z), 1.13 * d + 1e-6, gl(zu), 1.13 * du + 1e-6, 1.0
        else:
            base = 0.5
        got = out[sl]
        nm.check(got, z, _bound(z, d, hd, base), atol=d, rms_limit=None, what=f"fold {rt} {dtn} rows {r0}.. (one-pass bound)")
        gr = grp[sl]
        err = (got.double() - z).abs()
        ub = _bound(z, du, hd, base) + du
        for i, c in enumerate(CONDITION):
            r = gr == i
            ratio = float((err[r] / ub[r]).max())
            if r0 == 0:
                print(f"fold {rt} {dtn} |mean|/std={c}: max err / two-pass bound {ratio:.3g}, max one-pass d {float(d[r].max()):.3g}")
            if c in ("0", "1", "10"):
                nm.check(got[r], z[r], ub[r], rms_limit=None, what=f"fold {rt} {dtn} |mean|/std={c} vs the two-pass bound")
