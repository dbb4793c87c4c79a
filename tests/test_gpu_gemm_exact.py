"""Every GEMM route, element by element, on INTEGER operands.

With |a| <= amax, |w| <= wmax and K * amax * wmax < 2^24 every partial sum of a dot product is an integer an fp32
accumulator holds exactly, whatever order the MFMAs sum in -- so each output element has a tight reference: the exact
value (or the exact value rounded once to nearest even, oracle/numerics.round_half).  The reference GEMM itself runs in
fp32 on the same integers (exact by the same argument; TF32 is off), its epilogue in float64, in row chunks of <= 1 GiB.

Modes: (a) representable -- sparse +-1 activations (one per 64-wide K tile, so every K tile counts) against small
integer weights: every output is a half-precision integer and must match bit for bit (layout, tiles, K tiles, bias,
residual, positional rows m % 1024, q|k columns, the V^T image); (b) ties -- dense integers spread the outputs over
binades 2^0 .. 2^16 with ~1/4 of them exact ties: output == round_half(exact); (c) fp16 overflow -- biases put the
outputs around 65504 / 65519 / 65520; (d) fp16 subnormal activations; (e) GELU and the folded LayerNorm against float64
with derived bounds; (f) the [M][4][2] row statistics of the residual / positional epilogues == the exact sums of the
rounded output, slot by slot.  Every case asserts the route the dispatch takes (cpx_gemm_uses_big_tile and the known
predicates) and records it in ROUTES; the last test prints the table and asserts each route x dtype ran."""
import collections
import math

import pytest
import torch

from classpose_amd import _lib, ops
from oracle import numerics as nm

pytestmark = pytest.mark.gpu

DT = {"bf16": torch.bfloat16, "fp16": torch.float16}
ROUTES = collections.Counter()
U = 2.0 ** -24                                   # fp32 unit roundoff
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


def _sparse(M, K, g, dev, val=1.0):
    """one +-val per 64-wide K tile and row, at a random position"""
    idx = torch.randint(0, 64, (M, K // 64, 1), generator=g, device=dev)
    sgn = (torch.randint(0, 2, (M, K // 64, 1), generator=g, device=dev).float() * 2 - 1) * val
    return torch.zeros(M, K // 64, 64, device=dev).scatter_(2, idx, sgn).reshape(M, K)


def _chunks(M, N):
    rows = max(1024, (CHUNK_BYTES // (N * 8)) // 1024 * 1024)           # whole sub-tiles (the V^T image is per 1024 rows)
    for r0 in range(0, M, rows):
        yield r0, min(M, r0 + rows)


def _acc(A, W, r0, r1):
    """exact A[r0:r1] W^T as float64 (fp32 GEMM of integers < 2^24 in every partial sum)"""
    return (A[r0:r1].float() @ W.float().T).double()


def route(M, N, K, epi, ln=False, stats=False, bias=True, forced=None, dtn=None):
    """The kernel the production dispatch takes (csrc/cpx_gemm.hip: cpx_gemm_half_uses_big_tile, launch_gemm256*), asserted
    against the library's own predicate -- if the dispatch changes, this fails instead of testing another route.  The
    balanced schedule exists for the bf16 residual + statistics epilogue only (BAL_OK): fp16 takes the plain schedule."""
    big = bool(_lib.lib().cpx_gemm_uses_big_tile(M, N, K, ops.EPI[epi]))
    exp = (epi != "f32" and M % 256 == 0 and N % 256 == 0 and K >= 128 and ((K // 64) % 2 == 0 or epi == "pos")
           and (M // 256) * (N // 256) >= 256)
    assert big == exp, (M, N, K, epi, big)
    if forced:
        return forced
    if not big:
        return "128^2"
    if epi == "pos":
        return "k_gemm256"
    if epi == "qkv":
        return "k_gemm256p qkv" if (M // 256) % 64 == 0 else "k_gemm256"
    if epi == "gelu" and ln and bias and K >= 256:
        return "k_gemm4w"
    if epi == "gelu":
        return "k_gemm256p direct"
    if epi == "resid" and stats and K >= 256:
        assert dtn in DT, "the statistics route depends on the dtype"
        return "k_gemm256p balanced" if dtn == "bf16" else "k_gemm256p stats"
    return "k_gemm256p staged"


def _run(A, W, epi, bias=None, aux=None, stats=None, colsum=None, want_stats=False):
    if stats is None and not want_stats:
        return ops.gemm(A, W, epi, bias, aux), None
    with _lib.use_debug_library():                       # cpx_gemm_ln_dt: the fp16 folded / statistics entry
        r = ops.gemm_ln(A, W, epi, bias, aux, ln_stats=stats, ln_colsum=colsum, want_stats=want_stats)
    return r if want_stats else (r, None)


def _epilogue64(acc, epi, bias64, aux, r0, r1, hd):
    """float64 epilogue on the exact accumulator; returns the value BEFORE the final rounding"""
    z = acc + bias64 if bias64 is not None else acc
    if epi == "relu":
        return z.clamp_min(0)
    if epi == "resid":
        return nm.round_half(z, hd) + aux[r0:r1].double()            # the reference's double rounding
    if epi == "pos":
        rows = torch.arange(r0, r1, device=acc.device) % 1024
        return z + aux[rows].double()
    return z


def check_gemm(A, W, epi, bias=None, aux=None, hd=None, what=""):
    """run one (plain) GEMM and compare every element with round_half(exact); qkv: q|k columns and the V^T image"""
    M, K = A.shape
    N = W.shape[0]
    vT = torch.full((M // 1024, 16, 64, 1024), float("nan"), dtype=A.dtype, device=A.device) if epi == "qkv" else None
    out, _ = _run(A, W, epi, bias, vT if epi == "qkv" else aux)
    b64 = bias.double() if bias is not None else None
    for r0, r1 in _chunks(M, N):
        z = _epilogue64(_acc(A, W, r0, r1), epi, b64, aux, r0, r1, A.dtype)
        if epi == "f32":
            assert torch.equal(out[r0:r1].double(), z), what
        elif epi == "qkv":
            nm.check_exact(out[r0:r1, :2048], z[:, :2048], what=f"{what} q|k rows {r0}..")
            s0, s1 = r0 // 1024, r1 // 1024
            exp = z[:, 2048:].reshape(s1 - s0, 1024, 16, 64).permute(0, 2, 3, 1)
            nm.check_exact(vT[s0:s1].reshape(-1, 1024), exp.reshape(-1, 1024), what=f"{what} V^T sub-tiles {s0}..")
        else:
            nm.check_exact(out[r0:r1], z, what=f"{what} rows {r0}..")
    return out


def check_stats(out, st):
    """(f): slot t of row m = (sum, sum of squares) of the ROUNDED output over columns 256 t .. 256 t + 255, exactly"""
    o = out.double().reshape(out.shape[0], 4, 256)
    assert torch.equal(st[..., 0].double(), o.sum(2)), float((st[..., 0].double() - o.sum(2)).abs().max())
    assert torch.equal(st[..., 1].double(), (o * o).sum(2)), float((st[..., 1].double() - (o * o).sum(2)).abs().max())


# ---- operand families ---------------------------------------------------------------------------------------------
def operands(mode, M, N, K, hd, dev, seed):
    g = _gen(dev, seed)
    if mode == "exact":                          # (a): |out| <= 16 * 8 + 32 + 32 = 192 (64 * 2 + 64 at K = 4096): half-precision integers
        A = _sparse(M, K, g, dev)
        wmax = 8 if K <= 1024 else 2
        W = _ints((N, K), wmax, g, dev)
        bias = _ints((N,), 32, g, dev)
    elif mode == "ties":                         # (b): dense integers, outputs up to ~2^16
        amax = 32 if K <= 1024 else 16
        A = _ints((M, K), amax, g, dev)
        W = _ints((N, K), amax, g, dev)
        bias = _ints((N,), 64, g, dev)
        assert K * amax * amax < 2 ** 24
    elif mode == "overflow":                     # (c) fp16: |bias| in 65440 .. 65567 -> outputs straddle 65504 / 65520
        A = _sparse(M, K, g, dev)
        W = _ints((N, K), 4, g, dev)
        sgn = torch.where(torch.arange(N, device=dev) % 2 == 0, 1.0, -1.0)
        bias = sgn * (65440 + (torch.arange(N, device=dev) * 7) % 128).float()
    elif mode == "subnormal":                    # (d) fp16: activations k 2^-20 (subnormal below 2^-14), exact results k' 2^-20
        A = _sparse(M, K, g, dev, val=3 * 2.0 ** -20) + _sparse(M, K, g, dev, val=2.0 ** -22)
        W = _ints((N, K), 8, g, dev)
        bias = None
    else:
        raise ValueError(mode)
    return A.to(hd), W.to(hd), bias


EPIS = ["bf16", "gelu", "relu", "resid", "pos", "qkv", "f32"]


def _aux(epi, M, N, hd, dev, seed, mode):
    g = _gen(dev, seed + 1)
    if epi == "resid":
        return _ints((M, N), 32 if mode != "ties" else 1024, g, dev).to(hd)
    if epi == "pos":
        return _ints((1024, N), 32, g, dev)
    return None


def _exact_case(epi, M, N, K, hd, mode, dev, seed, what, forced=None, dtn=""):
    if epi == "qkv":
        N = 3072
    A, W, bias = operands(mode, M, N, K, hd, dev, seed)
    aux = _aux(epi, M, N, hd, dev, seed, mode)
    ROUTES[route(M, N, K, epi, forced=forced), dtn] += 1
    check_gemm(A, W, epi, bias, aux, what=f"{what} {epi} {mode}")


# ---- (a) (b) (c) (d): the route matrix ----------------------------------------------------------------------------
SHAPES = {                                      # (M, N, K) -> the kernel each takes by default
    "128^2": (2048, 1024, 1024),
    "k_gemm256p": (16384, 1024, 1024),
}


@pytest.mark.parametrize("dtn,mode", [("bf16", "exact"), ("bf16", "ties"), ("fp16", "exact"), ("fp16", "ties"),
                                      ("fp16", "overflow"), ("fp16", "subnormal")])
@pytest.mark.parametrize("variant", ["128^2 lds-dma", "128^2 register", "k_gemm256p", "k_gemm256 (persistent off)",
                                     "k_gemm256p direct (all)", "k_gemm256p staged (all)"])
def test_gemm_routes_integer_operands(cuda, variant, dtn, mode):
    hd = DT[dtn]
    small = variant.startswith("128^2")
    M, N, K = SHAPES["128^2"] if small else SHAPES["k_gemm256p"]
    epis = ["bf16", "relu", "resid", "qkv", "f32"] if small else ["bf16", "relu", "resid", "qkv"]
    with _lib.use_debug_library() as L:
        try:
            forced = None
            if variant == "128^2 register":
                L.cpx_gemm_set_variant(0); forced = "128^2 register"
            elif variant == "k_gemm256 (persistent off)":
                L.cpx_gemm_set_persistent(0); forced = "k_gemm256"
            elif variant == "k_gemm256p direct (all)":
                L.cpx_gemm_set_direct(2); forced = "k_gemm256p direct"
            elif variant == "k_gemm256p staged (all)":
                L.cpx_gemm_set_direct(0); L.cpx_gemm_set_balanced(0); forced = "k_gemm256p staged"
            for i, epi in enumerate(epis):
                f = forced
                if epi in ("resid", "qkv") and forced in ("k_gemm256p direct", "k_gemm256p staged"):
                    # no direct-store residual epilogue; qkv keeps its staged epilogue under cpx_gemm_set_direct(2) too (the direct-store
                    # form on the balanced q|k / V^T tile list wrote scattered wrong q|k elements and was retired)
                    f = None
                _exact_case(epi, M, N, K, hd, mode, cuda, 100 + i, variant, forced=f, dtn=dtn)
        finally:
            L.cpx_gemm_set_variant(1); L.cpx_gemm_set_persistent(1); L.cpx_gemm_set_direct(1); L.cpx_gemm_set_balanced(1)


# ---- the network's own GEMMs over the batch sizes that select the routes ------------------------------------------
NS = [1, 3, 8, 9, 16, 18, 25, 32, 56]


def _fold_ref(A, W, cs, bias, r0, r1):
    """(e) folded LayerNorm in float64 on exact statistics: z = rstd (acc - mean colsum) + b, and its fp32 error bound.
    The kernel: mean = sum / K (exact: K = 2^10, sum an integer), var = sq / K - mean^2 in fp32 (one product, one fma:
    <= u (sq/K + 2 mean^2)), + 1e-6 (u), v_rsq (<= 1 ulp = 2u): rel. error of rstd <= u (3 + 1.5 (sq/K + mean^2) / (var + eps));
    then rstd acc - rstd mean colsum (or (acc - mean colsum) rstd) and + b: <= 3u rstd (|acc| + |mean colsum|) + u |z|.
    Bound on z: |z - b| * rel(rstd) + 3u rstd (|acc| + |mean cs|) + u |z|, times 2 for the terms' own rounding."""
    K = A.shape[1]
    a = A[r0:r1].double()
    acc = _acc(A, W, r0, r1)
    s, sq = a.sum(1, keepdim=True), (a * a).sum(1, keepdim=True)
    mean = s / K
    var = sq / K - mean * mean
    rstd = 1.0 / torch.sqrt(var + 1e-6)
    mcs = mean * cs.double()[None]
    z = rstd * (acc - mcs) + bias.double()
    rel = U * (3 + 1.5 * (sq / K + mean * mean) / (var + 1e-6))
    dz = 2 * ((z - bias.double()).abs() * rel + 3 * U * rstd * (acc.abs() + mcs.abs()) + U * z.abs())
    return z, dz


def _gelu64(z):
    return 0.5 * z * torch.special.erfc(-z / math.sqrt(2))


def check_fold(A, W, bias, epi, stats, cs, hd, what):
    """(e): LayerNorm folded into the GEMM (+ GELU): every element within (1/2 ulp | GELU: 1 ulp + 1e-6) + the fp32
    epilogue bound of _fold_ref (GELU' <= 1.13 carries it); GELU correctly rounded in >= 99.9 % of the elements"""
    M, K = A.shape
    N = W.shape[0]
    vT = torch.zeros((M // 1024, 16, 64, 1024), dtype=hd, device=A.device) if epi == "qkv" else None
    out, _ = _run(A, W, epi, bias, vT, stats=stats, colsum=cs)
    n_cr = n = 0
    for r0, r1 in _chunks(M, N):
        z, dz = _fold_ref(A, W, cs, bias, r0, r1)
        if epi == "gelu":
            ref, dz, base = _gelu64(z), 1.13 * dz + 1e-6, 1.0
        else:
            ref, base = z, 0.5
        bound = base * nm.ulp(ref.abs() + dz, hd)
        if epi == "qkv":
            nm.check(out[r0:r1, :2048], ref[:, :2048], bound[:, :2048], atol=dz[:, :2048], what=f"{what} q|k")
            s0, s1 = r0 // 1024, r1 // 1024
            t = lambda x: x[:, 2048:].reshape(s1 - s0, 1024, 16, 64).permute(0, 2, 3, 1).reshape(-1, 1024)
            nm.check(vT[s0:s1].reshape(-1, 1024), t(ref), t(bound), atol=t(dz), what=f"{what} V^T")
        else:
            nm.check(out[r0:r1], ref, bound, atol=dz, what=what)
            if epi == "gelu":
                e = (out[r0:r1].double() - ref).abs()
                n_cr += int((e <= 0.5 * nm.ulp(ref, hd) * 1.0001 + dz).sum())
                n += e.numel()
    if n:
        assert n_cr >= 0.999 * n, (what, n - n_cr, n)


@pytest.mark.parametrize("dtn", ["bf16", "fp16"])
@pytest.mark.parametrize("nS", NS)
def test_network_gemms_every_element(cuda, nS, dtn):
    """cpx_net_forward's GEMM sequence at n_subtiles = nS with its production dispatch: patch embedding (K = 192, +bias
    +pos, statistics when the layer's residual GEMMs take the 256^2 kernel), qkv with the folded LayerNorm (q|k + V^T),
    attn.proj (residual [+ statistics]), mlp.lin1 (folded LayerNorm + GELU) and mlp.lin2 (residual [+ statistics]) in the
    MLP row parts of cpx_net_mlp_parts, cpx_row_stats where the network launches it (nS < 16), the neck (256 x 1024) and
    the head (f32).  nS < 16: proj / lin2 on the 128^2 kernel; 6 <= nS, nS % 16 != 0: qkv on k_gemm256; nS = 18:
    attn.proj = 288 tiles on 256 persistent workgroups; nS = 56: MLP parts of 16 + 16 + 24 sub-tiles."""
    hd, dev = DT[dtn], cuda
    L = _lib.lib()
    M = nS * 1024
    dt = _lib.DTYPE_CODE[dtn]
    big_stats = bool(L.cpx_gemm_uses_big_tile(M, 1024, 1024, ops.EPI["resid"]) and L.cpx_gemm_uses_big_tile(M, 1024, 4096, ops.EPI["resid"]))
    assert big_stats == (nS >= 16)
    g = _gen(dev, nS)
    # patch embedding: integer pixels x integer weights, +bias +pos (f32 table), rows m % 1024
    P, Wp, bp = operands("exact", M, 1024, 192, hd, dev, nS)
    pos = _ints((1024, 1024), 32, g, dev)
    ROUTES[route(M, 1024, 192, "pos", stats=big_stats), dtn] += 1
    if big_stats:
        out, st = _run(P, Wp, "pos", bp, pos, want_stats=True)
        check_stats(out, st)
        assert torch.equal(out, check_gemm(P, Wp, "pos", bp, pos, what=f"nS={nS} patch"))
    else:
        check_gemm(P, Wp, "pos", bp, pos, what=f"nS={nS} patch")
    # qkv: folded LayerNorm on integer rows (statistics by cpx_row_stats: exact integer sums), q|k and V^T
    x = (_ints((M, 1024), 8, g, dev) + _ints((M, 1), 4, g, dev)).to(hd)
    st = _row_stats(x)
    xd = x.double()
    assert torch.equal(st[:, 0, 0].double(), xd.sum(1)) and torch.equal(st[:, 0, 1].double(), (xd * xd).sum(1))
    assert not bool(st[:, 1:].any())
    Wq = _ints((3072, 1024), 4, g, dev).to(hd)
    cs = Wq.float().sum(1)
    bq = _ints((3072,), 8, g, dev)
    ROUTES[route(M, 3072, 1024, "qkv", ln=True), dtn] += 1
    check_fold(x, Wq, bq, "qkv", st, cs, hd, f"nS={nS} qkv")
    # attn.proj: residual (+ statistics on the 256^2 kernel)
    for name, K in (("attn.proj", 1024), ("mlp.lin2", 4096)):
        parts = L.cpx_net_mlp_parts(nS, dt) if (name == "mlp.lin2" and big_stats) else 1
        if name == "mlp.lin2":
            assert parts == (nS // 16 if nS >= 32 else 1)
        for pt in range(parts):
            r0 = pt * 16384
            Mp = 16384 if pt + 1 < parts else M - r0
            A, W, b = operands("exact", Mp, 1024, K, hd, dev, 1000 * nS + pt + K)
            res = _aux("resid", Mp, 1024, hd, dev, nS + pt + K, "exact")
            ROUTES[route(Mp, 1024, K, "resid", stats=big_stats, dtn=dtn), dtn] += 1
            if big_stats:
                out, sto = _run(A, W, "resid", b, res, want_stats=True)
                check_stats(out, sto)
                assert torch.equal(out, check_gemm(A, W, "resid", b, res, what=f"nS={nS} {name} part {pt}"))
            else:
                out = check_gemm(A, W, "resid", b, res, what=f"nS={nS} {name}")
                sto = _row_stats(out)              # the network's own cpx_row_stats launch below 16 sub-tiles
                assert not bool(sto[:, 1:].any())
                o = out.double()
                assert torch.equal(sto[:, 0, 0].double(), o.sum(1)) and torch.equal(sto[:, 0, 1].double(), (o * o).sum(1))
    # mlp.lin1: folded LayerNorm + GELU on the rows of each MLP part
    parts = L.cpx_net_mlp_parts(nS, dt) if big_stats else 1
    W1 = _ints((4096, 1024), 2, g, dev).to(hd)
    cs1 = W1.float().sum(1)
    b1 = torch.randint(-256, 257, (4096,), generator=g, device=dev).float() / 64
    for pt in range(parts):
        r0 = pt * 16384
        r1 = r0 + 16384 if pt + 1 < parts else M
        xs, sts = x[r0:r1].contiguous(), st[r0:r1].contiguous()
        ROUTES[route(r1 - r0, 4096, 1024, "gelu", ln=True), dtn] += 1
        check_fold(xs, W1, b1, "gelu", sts, cs1, hd, f"nS={nS} mlp.lin1 part {pt}")
    # neck (1x1 conv as a 256 x 1024 GEMM, plain epilogue) and the head (f32 epilogue, 640 columns)
    A, W, _ = operands("ties", M, 256, 1024, hd, dev, 7 * nS)
    ROUTES[route(M, 256, 1024, "bf16", bias=False), dtn] += 1
    check_gemm(A, W, "bf16", None, what=f"nS={nS} neck")
    A, W, b = operands("ties", M, 640, 256, hd, dev, 9 * nS)
    ROUTES[route(M, 640, 256, "f32"), dtn] += 1
    check_gemm(A, W, "f32", b, what=f"nS={nS} head")


def _row_stats(x):
    """k_row_stats in the input's half type (cpx_row_stats_dt, debug build: the product entry is bf16 only)"""
    with _lib.use_debug_library():
        return ops.row_stats(x)


@pytest.mark.parametrize("dtn", ["bf16", "fp16"])
@pytest.mark.parametrize("M,N", [(2048, 1024), (16384, 4096)])
def test_gelu_epilogue_integer_pre_activation(cuda, M, N, dtn):
    """(e) GELU on an exact pre-activation (integer accumulators + biases in 1/64 steps, z in [-40, 40]): within 1 ulp
    (+ 1e-6 absolute: the fitted GELU's own floor) of float64 erf-GELU everywhere, correctly rounded in >= 99.9 % --
    128^2 kernel and the persistent direct-store epilogue"""
    hd = DT[dtn]
    g = _gen(cuda, M + N)
    A = _sparse(M, 1024, g, cuda).to(hd)
    W = _ints((N, 1024), 2, g, cuda).to(hd)
    bias = torch.randint(-256, 257, (N,), generator=g, device=cuda).float() / 64
    ROUTES[route(M, N, 1024, "gelu", bias=True), dtn] += 1
    out, _ = _run(A, W, "gelu", bias)
    n_cr = 0
    for r0, r1 in _chunks(M, N):
        z = _acc(A, W, r0, r1) + bias.double()
        ref = _gelu64(z)
        u = nm.ulp(ref, hd)
        nm.check(out[r0:r1], ref, u, atol=1e-6, what=f"gelu {dtn}")
        n_cr += int(((out[r0:r1].double() - ref).abs() <= 0.5 * u * 1.0001 + 1e-6).sum())
    assert n_cr >= 0.999 * M * N, M * N - n_cr


@pytest.mark.parametrize("dtn", ["bf16", "fp16"])
@pytest.mark.parametrize("epi", ["bf16", "relu"])
@pytest.mark.parametrize("S,C,N", [(2, 64, 128), (1, 128, 256)])
def test_conv3x3_zero_border_integer_operands(cuda, S, C, N, epi, dtn):
    """cpx_conv3x3 (implicit GEMM on the 128^2 kernel): every element == round_half of the exact 3x3 / padding-1
    convolution of integer activations -- the zero taps outside each 32 x 32 image included"""
    hd = DT[dtn]
    g = _gen(cuda, S * C + N)
    x = _ints((S * 1024, C), 16, g, cuda).to(hd)
    Wt = _ints((N, 9 * C), 16, g, cuda).to(hd)
    bias = _ints((N,), 64, g, cuda)
    out = ops.conv3x3(x, Wt, epi, bias)
    ROUTES["conv3x3 128^2", dtn] += 1
    xi = x.double().reshape(S, 32, 32, C).permute(0, 3, 1, 2)
    w4 = Wt.double().reshape(N, 3, 3, C).permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(xi.cpu(), w4.cpu(), padding=1).to(cuda).permute(0, 2, 3, 1).reshape(S * 1024, N) + bias.double()
    if epi == "relu":
        ref = ref.clamp_min(0)
    nm.check_exact(out, ref, what=f"conv3x3 {epi} {dtn}")


def test_zz_route_table(cuda):
    """every route x dtype of the matrix above ran at least once (printed for the record).  ROUTES is filled by the tests
    above IN THE SAME PROCESS: this test summarises a run of the whole module (the file order puts it last) and fails,
    naming the routes, when run on its own or after a subset of the module."""
    common = ["128^2", "128^2 register", "k_gemm256", "k_gemm256p qkv", "k_gemm256p direct", "k_gemm256p staged", "k_gemm4w",
              "conv3x3 128^2"]
    want = {"bf16": common + ["k_gemm256p balanced"], "fp16": common + ["k_gemm256p stats"]}
    for (r, d), n in sorted(ROUTES.items()):
        print(f"route {r:22s} {d}: {n} cases")
    missing = [(r, d) for d in DT for r in want[d] if ROUTES[r, d] == 0]
    assert not missing, f"routes not exercised in this run (the module's tests fill ROUTES; run the whole file): {missing}"
    assert ROUTES["k_gemm256p balanced", "fp16"] == 0 and ROUTES["k_gemm256p stats", "bf16"] == 0
