"""Per-element error scales for the attention backward (cpx_attention_backward, cpx_attention_backward_bf16) on top of
tests/block_train_reference.py, and the check that uses them (DESIGN 6d').

``magnitudes`` returns, for every element of dq, dk, dv, dRh and dRw, the sum of the absolute values of the terms that element is the sum
of, each term weighted by the relative error its factors can carry.  Nothing in it cancels, so it is the scale a rounding error of the
element is proportional to, whatever the element's own value is (a dq row whose terms cancel keeps a large A).  With P and
scale = 0.125 of the contract (csrc/cpx_train_blocks.hip):

    dPa    = |dO| |v|^T
    Lam_ij = scale sum_d |q_id| (|k_jd| + |Rh[qy - ky + 31]_d| + |Rw[qx - kx + 31]_d|)        the size of the terms of the logit
    W_ij   = scale P_ij (dPa_ij + sum_j P_ij dPa_ij) (1 + Lam_ij)                             the size of the terms of dS'_ij, times 1 + Lam
    A(dq_id)    = sum_j W_ij |k_jd| + sum_ky (sum_kx W) |Rh[..]_d| + sum_kx (sum_ky W) |Rw[..]_d|
    A(dk_jd)    = sum_i W_ij |q_id|
    A(dv_jd)    = sum_i P_ij (1 + Lam_ij) |dO_id|
    A(dRh[r]_d) = sum over crops, heads, queries and ky with qy - ky + 31 = r of (sum_kx W) |q_d|          (dRw likewise)

The factor 1 + Lam: an absolute error e of the logit is a relative error scale e of P, and a float32 dot product of 64 channels has
e proportional to Lam / scale.  Without the factor the float32 restatement itself sits 96 units of 2^-24 A away at qscale 7.5.

``check(got, exact, A, what)`` prints the largest |got - exact| / (unit A) and where it sits, and returns it.  An element whose A is
zero (a query row with dO = 0, the padding row 63 of a table) has no term at all: there anything but the exact value is an infinite
ratio.

The hard bound of the float32 mode, ``C_F32`` = 2140 (units of 2^-24 A).  Counting roundings of the kernels, u = 2^-24, first order:
  * the logit: three dot products of 64 channels (q . k by MFMA, q . Rh and q . Rw by MFMA into Bh / Bw) and two additions, then
    (S' + off) * cexp: three more roundings on a value of at most 2 Lam / scale: scale |dS'_ij| <= (66 + 6) u Lam_ij = 72 u Lam_ij, which is
    the relative error of exp(..) (the error of the running maximum is a common factor of p and l and cancels);
  * exp2 (1 ulp = 2 u), times 1 / l: 3 u;  l itself: 16 additions per tile, 32 fmaf steps, the lane halves, the reciprocal: 50 u, plus the
    P-weighted mean of the 72 u Lam + 2 u of its terms: 72 u Lbar_i + 52 u with Lbar_i = sum_j P_ij Lam_ij;
  * dP: 64 channels, 64 u dPa;  delta = sum_j P dP: the errors of P and dP above and the same 50 u chain;
  * dS' = 0.125 (p (dP - delta)): 2 u.
  Together |dS'_ij - exact| <= u W_ij / (1 + Lam_ij) (72 (Lam_ij + 2 Lbar_i) + 64 + 2 (55 + 50 + 64) + 2)
                             <= u W_ij (72 (1 + 2 spread) + 404 / (1 + Lam_ij)),    spread = max_i (1 + Lbar_i) / (1 + min_j Lam_ij),
  which ``magnitudes`` returns: 1.5 .. 1.8 on the random cases (the host test holds it at <= 4: <= 1052 u W_ij), 32 on the spiked case,
  whose spiked key has a Lam of 60 and every other key one of 2.
  * the sums: dq 1024 keys (512 MFMA steps of two products: at most 1024 u) and 64 fmaf steps of the bias term; dk, dv 1024 queries; the
    tables 32 float32 additions of the group sum G, then float64, then one rounding: at most 1088 u on terms of size W |k|.
  c(spread) = 72 (1 + 2 spread) + 404 + 1088 (``c_f32``), ``C_F32`` = c(4) = 2140.  The float32 restatement measures 0.04 .. 1.3 on the cases of tests/test_gpu_attn_bwd_every_element.py: the
  bound is there to catch a wrong term, the 4x rule next to it to catch a wrong rounding."""
from __future__ import annotations

import torch

import block_train_reference as br

U = 2.0 ** -24


def c_f32(spread: float) -> float:
    """the chain-length constant of the hard bound |x - r64| <= c 2^-24 A of the float32 mode (derived in the module's docstring)"""
    return 72.0 * (1.0 + 2.0 * spread) + 404.0 + 1088.0


C_F32 = c_f32(4.0)
BIG = 64 * U                             # bf16 mode: the elements farther than this from b64 are counted (rounding flips of P and dS')
NAMES = ("dq", "dk", "dv", "dRh", "dRw")
SLICES = {"dq": slice(0, 1024), "dk": slice(1024, 2048), "dv": slice(2048, 3072)}


def pick(R: dict) -> dict:
    """{"dqkv", "dRh", "dRw"} of the restatements -> the five outputs by name"""
    return {**{n: R["dqkv"][:, s] for n, s in SLICES.items()}, "dRh": R["dRh"], "dRw": R["dRw"]}


def _crop(qkv, Rh, Rw, dO):
    q, k, v = br._split(qkv, 1)
    P = torch.softmax(br._logits(q, k, Rh, Rw, 1) * br.SCALE, -1)
    aq, ak, ah, aw = q.abs(), k.abs(), Rh.abs(), Rw.abs()
    lam1 = 1.0 + br._logits(aq, ak, ah, aw, 1) * br.SCALE
    spread = float(((P * lam1).sum(-1) / lam1.min(-1).values).max())
    adO = dO.abs().reshape(1, 1024, br.HEADS, br.HD).permute(0, 2, 1, 3)
    dPa = adO @ v.abs().transpose(-1, -2)
    Wt = br.SCALE * P * (dPa + (P * dPa).sum(-1, keepdim=True)) * lam1
    del dPa
    Adv = (P * lam1).transpose(-1, -2) @ adO
    del P, lam1
    Adk = Wt.transpose(-1, -2) @ aq
    w5 = Wt.reshape(1, br.HEADS, br.GRID, br.GRID, br.GRID, br.GRID)
    Wh, Ww = w5.sum(-1), w5.sum(-2)
    idx = br._rel_index()
    Adq = Wt @ ak + (torch.einsum("bnhwk,hkc->bnhwc", Wh, ah[idx]) + torch.einsum("bnhwk,wkc->bnhwc", Ww, aw[idx])).reshape(1, br.HEADS, 1024, br.HD)
    qg = aq.reshape(1, br.HEADS, br.GRID, br.GRID, br.HD)
    Ah, Aw = torch.zeros_like(Rh), torch.zeros_like(Rw)
    Ah.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->hkc", Wh, qg).reshape(-1, br.HD))
    Aw.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->wkc", Ww, qg).reshape(-1, br.HD))
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(1024, br.HEADS * br.HD)
    return rows(Adq), rows(Adk), rows(Adv), Ah, Aw, spread


def magnitudes(qkv: torch.Tensor, Rh: torch.Tensor, Rw: torch.Tensor, dO: torch.Tensor, nS: int) -> dict:
    """{"dq", "dk", "dv" [nS * 1024, 1024], "dRh", "dRw" [64, 64]} float64 and "spread" (see above), one crop at a time"""
    qkv, Rh, Rw, dO = (t.double() for t in (qkv, Rh, Rw, dO))
    parts = [_crop(qkv[c * 1024:(c + 1) * 1024], Rh, Rw, dO[c * 1024:(c + 1) * 1024]) for c in range(nS)]
    A = {n: torch.cat([p[i] for p in parts], 0) for i, n in enumerate(("dq", "dk", "dv"))}
    A["dRh"], A["dRw"] = sum(p[3] for p in parts), sum(p[4] for p in parts)
    A["spread"] = max(p[5] for p in parts)
    return A


def ratios(got: torch.Tensor, exact: torch.Tensor, A: torch.Tensor, unit: float = U) -> torch.Tensor:
    """|got - exact| / (unit A) per element; 0 where both vanish, inf where A = 0 and got differs (or got is not finite)"""
    diff = (got.double() - exact.double()).abs()
    r = diff / (unit * A)
    r = torch.where(A > 0, r, torch.where(diff == 0, torch.zeros_like(r), torch.full_like(r, float("inf"))))
    return torch.where(torch.isfinite(got.double()), r, torch.full_like(r, float("inf")))


def where(flat: int, shape) -> str:
    """the place of element ``flat`` of a [nS * 1024, 1024] gradient (crop, head, row, channel) or of a [64, 64] table"""
    row, col = divmod(int(flat), shape[1])
    if shape[1] == 1024:
        return f"crop {row // 1024} head {col // 64} row {row % 1024} channel {col % 64}"
    return f"table row {row} channel {col}"


def check(got: torch.Tensor, exact: torch.Tensor, A: torch.Tensor, what: str, unit: float = U) -> float:
    """prints and returns the worst |got - exact| / (unit A)"""
    r = ratios(got, exact, A, unit)
    at = int(r.argmax())
    worst = float(r.reshape(-1)[at])
    print(f"  {what}: worst |x - exact| / ({unit:.3g} A) = {worst:.4g} at {where(at, r.shape)} "
          f"(x = {float(got.reshape(-1)[at]):.6g}, exact = {float(exact.reshape(-1)[at]):.6g}, A = {float(A.reshape(-1)[at]):.6g})")
    return worst


def fraction_above(got: torch.Tensor, exact: torch.Tensor, A: torch.Tensor, level: float = BIG) -> float:
    """the share of the elements with |got - exact| > level * A"""
    return float((ratios(got, exact, A, 1.0) > level).double().mean())


# ---- the cases of tests/test_gpu_attn_bwd_every_element.py (built on the CPU; the host test runs the restatements on the same ones) ----
HD = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
F32_CASES = [(p, q, 1) for p in ("bf16", "fp16", "fp32") for q in (1.0, 7.5)] + [("bf16", 1.0, 3)]
BF16_CASES = [("bf16", 1.0, 1), ("bf16", 7.5, 1), ("bf16", 1.0, 3)]
DOUTS = ("scaled", "flat")


def attn_case(nS, prec, seed, qscale=1.0, dout="scaled"):
    """test_gpu_block_train._attn_case (the same generator calls in the same order: the GPU module asserts the equality); ``dout`` "flat":
    a second dO without the logspace(-2, 0) channel scaling, so that every head carries the same share of each tensor"""
    g = torch.Generator().manual_seed(seed)
    hd = HD[prec]
    qkv = torch.randn(nS * 1024, 3072, generator=g)
    qkv[:, :1024] *= qscale
    tab = lambda: torch.cat([torch.randn(63, 64, generator=g) * 0.5, torch.zeros(1, 64)]).to(hd)
    dO = torch.randn(nS * 1024, 1024, generator=g) * torch.logspace(-2, 0, 1024)[None]
    Rh, Rw = tab(), tab()
    if dout == "flat":
        dO = torch.randn(nS * 1024, 1024, generator=g) * 0.25
    dO[::5] = 0
    return qkv.to(hd), Rh, Rw, dO


def spiked_case(prec):
    """the pattern of test_attention_f32_spiked_rows for the backward: q = 1 + noise, k and v small, and per head one key of 7.5 in every
    channel: its logit is scale * 64 * 7.5 = 60 nats above the rest.  The key is 672 + 21 * head: key tiles 21 .. 30, so the running
    maximum of pass 1 is replaced late and l_run, d_run are rescaled by about e^-60"""
    g = torch.Generator().manual_seed(67)
    qkv = torch.randn(1024, 3072, generator=g) * 0.1
    qkv[:, :1024] += 1.0
    for h in range(br.HEADS):
        qkv[672 + 21 * h, 1024 + 64 * h:1024 + 64 * (h + 1)] = 7.5
    tab = lambda: torch.cat([torch.randn(63, 64, generator=g) * 0.05, torch.zeros(1, 64)]).to(HD[prec])
    Rh, Rw = tab(), tab()
    dO = torch.randn(1024, 1024, generator=g)
    dO[::5] = 0
    return qkv.to(HD[prec]), Rh, Rw, dO


def band_case(variant, nS, prec):
    """The band-masked integer case.  "h": q = 1 in channel 0 of every head and 0 elsewhere; k = 0 in channel 0, integers of -2 .. 2
    elsewhere; both tables integers of -2 .. 2 in channels 1 .. 63 of rows 0 .. 62; channel 0 of Rh is -8192 in every row but row 31,
    which holds 0, so S' is 0 for the 32 keys of the query's image row and -8192 (-1024 nats) for the other 992: P is 2^-5 or 0.
    v in {-1, 0, 1}, every channel summing to zero over each image row, dO in {-1, 0, 1}: delta = 0, dS' = 2^-8 dP with |dP| <= 64.
    "w": Rw masked, the v groups are image columns.  Every crop has its own data."""
    g = torch.Generator().manual_seed(90 + 2 * nS + (variant == "w"))
    qkv = torch.zeros(nS * 1024, 3072)
    qkv[:, 0:1024:64] = 1.0
    qkv[:, 1024:2048] = torch.randint(-2, 3, (nS * 1024, 1024), generator=g).float()
    qkv[:, 1024:2048:64] = 0.0
    half = torch.randint(-1, 2, (nS, 32, 16, 1024), generator=g).float()
    grp = torch.cat([half, -half], 2)                                   # [crop][group][member][channel], zero sum over the members
    perm = torch.stack([torch.randperm(32, generator=g) for _ in range(nS * 32)]).reshape(nS, 32, 32)
    grp = torch.gather(grp, 2, perm[..., None].expand(-1, -1, -1, 1024))
    if variant == "w":
        grp = grp.transpose(1, 2)                                       # group = kx, member = ky -> token order [ky][kx]
    qkv[:, 2048:] = grp.reshape(nS * 1024, 1024)
    tabs = []
    for masked in (variant == "h", variant == "w"):
        t = torch.zeros(64, 64)
        t[:63, 1:] = torch.randint(-2, 3, (63, 63), generator=g).float()
        if masked:
            t[:63, 0] = -8192.0
            t[31, 0] = 0.0
        tabs.append(t)
    dO = torch.randint(-1, 2, (nS * 1024, 1024), generator=g).float()
    return qkv.to(HD[prec]), tabs[0].to(HD[prec]), tabs[1].to(HD[prec]), dO


_REF = {}


def references(key, build, magnitude=True):
    """{"in": (qkv, Rh, Rw, dO), "r64", "r32", "b64", "b32" (bf16 tensors only), "A" (None without ``magnitude``)} of the case ``build()`` returns, computed once per
    ``key`` and shared by the tests of a run; nothing in it is written to afterwards"""
    if key not in _REF:
        import attn_bwd_bf16_reference as ab
        qkv, Rh, Rw, dO = build()
        nS = qkv.shape[0] // 1024
        d, f = (qkv.double(), Rh.double(), Rw.double(), dO.double()), (qkv.float(), Rh.float(), Rw.float(), dO)
        R = {"in": (qkv, Rh, Rw, dO), "A": magnitudes(qkv, Rh, Rw, dO, nS) if magnitude else None, "r64": pick(br.attention_backward(*d, nS)),
             "r32": pick(br.attention_backward(*f, nS))}
        if qkv.dtype == torch.bfloat16:
            R["b64"], R["b32"] = pick(ab.attention_backward_bf16(*d, nS)), pick(ab.attention_backward_bf16(*f, nS))
        _REF[key] = R
    return _REF[key]
