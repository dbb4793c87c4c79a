"""Per-element numerics checker for the bf16 / fp16 / fp32 kernels -- TEST INFRASTRUCTURE ONLY.

``round_half`` rounds float64 values to bf16, fp16 or float32 by round-to-nearest-even in ONE step (torch's own ``.to()``
from float64 goes through float32 first for bf16, a double rounding), with gradual underflow and overflow to +-inf; for
float32 it equals ``.float()``.  ``ulp`` is the spacing of the type at a value.  ``check`` asserts an elementwise bound and a per-block / per-row
RMS gate and, on failure, names where the error sits: the worst element, 16 x 16 block, row and column.

Everything is torch on whatever device the tensors live on (float64), so a test can build its reference on the GPU.
"""
from __future__ import annotations

import torch

# (significand bits incl. the implicit one, smallest normal exponent, largest finite value)
_FMT = {
    torch.bfloat16: (8, -126, (2.0 - 2.0 ** -7) * 2.0 ** 127),
    torch.float16: (11, -14, 65504.0),
    torch.float32: (24, -126, (2.0 - 2.0 ** -23) * 2.0 ** 127),
}

# RMS gate: a correctly rounded result has |err| <= 0.5 ulp everywhere, and for values spread over the binade
# err / ulp is ~uniform on [-0.5, 0.5]: E[e^2] = 1/12, RMS 0.289.  Truncation (the commonest wrong rounding) is uniform
# on [0, 1): RMS 0.577.  Over one 16 x 16 block (256 samples) the mean of e^2 has std 0.0052 (rounding) and 0.0186
# (truncation), so the 6-sigma bands end at RMS 0.34 and 0.47: 0.40 separates the two.
RMS_LIMIT = 0.40


def _fmt(dtype):
    if dtype not in _FMT:
        raise ValueError(f"not bf16, fp16 or float32: {dtype}")
    return _FMT[dtype]


def ulp(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of ``dtype`` at |x| (float64): 2^(e - p + 1) with e = floor(log2 |x|) clamped at the smallest normal
    exponent (subnormals share one spacing; ulp(0) is the smallest subnormal)."""
    p, emin, _ = _fmt(dtype)
    x = x.double()
    _, E = torch.frexp(x.abs())                    # |x| = m 2^E, m in [0.5, 1)  ->  e = E - 1
    e = torch.clamp(E.double() - 1, min=emin)
    e = torch.where(x == 0, torch.full_like(e, emin), e)
    return torch.exp2(e - (p - 1))


def round_half(x64: torch.Tensor, dtype) -> torch.Tensor:
    """Round float64 values to ``dtype`` (nearest, ties to even), returned as float64.  Exact: x / ulp is a float64
    scaling by a power of two and torch.round rounds halves to even.  Beyond the largest finite value -- i.e. from
    max + ulp/2 on, where RNE rounds up out of range -- the result is +-inf (fp16: 65520 -> inf, 65519.99 -> 65504)."""
    _, _, vmax = _fmt(dtype)
    x = x64.double()
    q = ulp(x, dtype)
    r = torch.round(x / q) * q
    r = torch.where(r.abs() > vmax, torch.copysign(torch.full_like(r, float("inf")), x), r)
    return torch.where(torch.isfinite(x), r, x)


def _as2d(t: torch.Tensor) -> torch.Tensor:
    if t.dim() == 2:
        return t
    if t.dim() == 1:
        return t.reshape(1, -1)
    return t.reshape(-1, t.shape[-1])


def check(got: torch.Tensor, ref64: torch.Tensor, bound, block=(16, 16), dtype=None, atol=0.0,
          rms_limit: float | None = RMS_LIMIT, what: str = "") -> dict:
    """Assert |got - ref64| <= bound + atol for EVERY element, and -- unless rms_limit is None -- that in every
    ``block`` and every row RMS(max(|err| - atol, 0) / ulp(ref)) <= rms_limit.

    got: the kernel's output (any dtype; compared as float64).  ref64: the float64 reference of the SAME operation
    (exact, or correctly rounded when the bound is 0).  bound, atol: scalars or tensors broadcastable to got, absolute;
    atol is the part of the bound that is not rounding (the RMS gate discounts it).
    dtype: the type that sets ulp (bf16, fp16 or float32; default got.dtype).  Non-finite values must match exactly (same inf sign / NaN).
    On failure the AssertionError names the worst element (index, ulps, got, ref), the worst block, row and column.
    Returns a few summary numbers (max ulps, worst block RMS) for the caller's report."""
    dtype = dtype or got.dtype
    g = _as2d(got.detach()).double()
    r = _as2d(ref64.detach()).double().to(g.device)
    assert g.shape == r.shape, (what, tuple(g.shape), tuple(r.shape))
    R, C = g.shape
    b = _as2d(torch.broadcast_to(torch.as_tensor(bound, dtype=torch.float64, device=g.device), got.shape))
    atol = _as2d(torch.broadcast_to(torch.as_tensor(atol, dtype=torch.float64, device=g.device), got.shape))
    fin = torch.isfinite(r)
    same_nonfinite = (~fin) & ((g == r) | (torch.isnan(g) & torch.isnan(r)))
    err = torch.where(fin, (g - r).abs(), torch.where(same_nonfinite, torch.zeros_like(g), torch.full_like(g, float("inf"))))
    err = torch.nan_to_num(err, nan=float("inf"))
    u = ulp(torch.where(fin, r, torch.zeros_like(r)), dtype)
    excess = err - (b + atol)                       # > 0: out of bound
    e_ulp = torch.clamp(err - atol, min=0) / u
    bad = excess > 0
    bh, bw = block
    # per-block / per-row mean square of the error in ulps (partial edge blocks padded with zeros, divided by their true size)
    Rp, Cp = -(-R // bh) * bh, -(-C // bw) * bw
    sq = torch.zeros((Rp, Cp), dtype=torch.float64, device=g.device)
    sq[:R, :C] = torch.where(torch.isfinite(e_ulp), e_ulp, torch.zeros_like(e_ulp)) ** 2
    cnt = torch.zeros_like(sq)
    cnt[:R, :C] = 1
    blk_rms = (sq.reshape(Rp // bh, bh, Cp // bw, bw).sum((1, 3)) / cnt.reshape(Rp // bh, bh, Cp // bw, bw).sum((1, 3))).sqrt()
    row_rms = sq[:R, :C].mean(1).sqrt()
    # where the failure sits: score = excess over the bound (elementwise) -- the worst block / row / column by it
    score = torch.where(torch.isfinite(excess), excess, torch.full_like(excess, 1e300))
    i = int(torch.argmax(score))
    wr, wc = divmod(i, C)
    sp = torch.full((Rp, Cp), -1e308, dtype=torch.float64, device=g.device)
    sp[:R, :C] = score
    blk_max = sp.reshape(Rp // bh, bh, Cp // bw, bw).amax((1, 3))
    info = dict(max_ulp=float(e_ulp.max()), n_bad=int(bad.sum()), worst_block_rms=float(blk_rms.max()),
                worst_row_rms=float(row_rms.max()))
    rms_bad = rms_limit is not None and (info["worst_block_rms"] > rms_limit or info["worst_row_rms"] > rms_limit)
    if bool(bad.any()) or rms_bad:
        if not bool(bad.any()):                   # the RMS gate tripped: locate by block / row RMS instead
            blk_max, row_key = blk_rms, row_rms
            col_key = (sq[:R, :C].mean(0)).sqrt()
        else:
            row_key, col_key = score.amax(1), score.amax(0)
        bi = int(torch.argmax(blk_max))
        bri, bci = divmod(bi, blk_max.shape[1])
        rr, cc = int(torch.argmax(row_key)), int(torch.argmax(col_key))
        kind = "elementwise bound" if bool(bad.any()) else f"RMS gate (limit {rms_limit} ulp)"
        msg = (f"{what}: {kind} violated -- {info['n_bad']} of {R * C} elements out of bound; "
               f"worst element [{wr}, {wc}]: got {float(g[wr, wc])!r}, ref {float(r[wr, wc])!r}, "
               f"|err| {float(err[wr, wc]):.6g} = {float(e_ulp[wr, wc]):.3f} ulp, bound {float(b[wr, wc] + atol[wr, wc]):.6g}; "
               f"worst block rows {bri * bh}..{min(bri * bh + bh, R) - 1} cols {bci * bw}..{min(bci * bw + bw, C) - 1} "
               f"(block RMS {float(blk_rms[bri, bci]):.3f} ulp); worst row {rr} (RMS {float(row_rms[rr]):.3f} ulp); worst column {cc}")
        raise AssertionError(msg)
    return info


def check_exact(got: torch.Tensor, ref64: torch.Tensor, what: str = "", block=(16, 16)) -> dict:
    """got must be BIT FOR BIT round_half(ref64) (the reference is exact in float64): bound 0, non-finite values included."""
    return check(got, round_half(ref64, got.dtype), 0.0, block=block, what=what, rms_limit=None)
