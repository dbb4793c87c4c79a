"""The per-element check of the attention backward (tests/attn_bwd_bounds.py, DESIGN 6d') on the CPU: the restatements themselves stay
inside the bounds tests/test_gpu_attn_bwd_every_element.py holds the device to, on every case of that module, and outputs that are
wrong in part of one head, in one table row, in one query's delta or in one crop's table partial are rejected by it -- while the two
norm rules the older tests use (tests/test_gpu_block_train.py, tests/test_gpu_attn_bwd_bf16.py) let most of them pass:
    (i)  err(x, r64) <= max(4 err(CPU float32, r64), 2^-20)                     err = relative L2 over the whole tensor
    (ii) bf16 mode: err(x, b64) <= err(b64, r64) / 4 for dq, dk, dv; <= max(4 err(b32, b64), 2^-20) for the tables
Every test prints what it measured before it asserts (run with -s)."""
from __future__ import annotations

import pytest
import torch

import attn_bwd_bf16_reference as ab
import attn_bwd_bounds as bd
import block_train_reference as br
import train_reference as tr
from attn_bwd_bounds import NAMES

FLOOR = 2.0 ** -20


def _random(prec, qscale, nS, dout):
    return bd.references(("random", prec, qscale, nS, dout), lambda: bd.attn_case(nS, prec, 61, qscale, dout))


def _spiked(prec):
    return bd.references(("spiked", prec), lambda: bd.spiked_case(prec))


# ---- (a), (b): the restatements inside the bounds of the GPU module ---------------------------------------------------------
def _inside(R, what, c):
    """The hard bound of the float32 mode, |x - r64| <= c 2^-24 A with c = attn_bwd_bounds.c_f32(spread) = 72 (1 + 2 spread) + 404 + 1088:
    72 per unit of Lam for the three 64-channel dot products of the logit, 404 for the exponential, the 1024-key sums l and delta and the
    64-channel dP, 1088 for the output's own sum over 1024 keys or queries and the 64 table terms (derivation: attn_bwd_bounds).  For
    spread <= 4, which holds on every random case, c = 2140."""
    worst = {n: bd.check(R["r32"][n], R["r64"][n], R["A"][n], f"{what} float32 restatement {n}") for n in NAMES}
    print(f"  spread {R['A']['spread']:.3f}, c = {c:.0f}")
    assert max(worst.values()) <= c and R["A"]["spread"] <= (c - 1564.0) / 144.0 + 1e-9
    return worst


@pytest.mark.parametrize("dout", bd.DOUTS)
@pytest.mark.parametrize("prec,qscale,nS", bd.F32_CASES)
def test_float32_restatement_is_inside_the_hard_bound(prec, qscale, nS, dout):
    R = _random(prec, qscale, nS, dout)
    assert R["A"]["spread"] <= 4.0
    _inside(R, f"{prec} qscale={qscale} nS={nS} dO {dout}:", bd.C_F32)
    if (prec, qscale, nS) in bd.BF16_CASES:
        # bf16 mode: b32 differs from b64 where a float32 rounding error moves P or dS' across a bf16 rounding boundary; the GPU module
        # allows the device four times the largest such difference and 0.2 % of the elements above 64 * 2^-24 A
        for n in NAMES:
            w = bd.check(R["b32"][n], R["b64"][n], R["A"][n], f"bf16 mode, b32 against b64, {n}", 1.0)
            frac = bd.fraction_above(R["b32"][n], R["b64"][n], R["A"][n])
            print(f"    share of the elements above 64 * 2^-24 A: {100 * frac:.4f} %")
            assert frac <= 0.0005 and w < 2.0 ** -12


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_spiked_case(prec):
    R = _spiked(prec)
    qkv, Rh, Rw, _ = R["in"]
    lg = br._logits(*br._split(qkv.double(), 1)[:2], Rh.double(), Rw.double(), 1) * br.SCALE
    top = lg.topk(2, -1)
    gap = top.values[..., 0] - top.values[..., 1]
    print(f"{prec}: the spiked key leads by {float(gap.min()):.1f} .. {float(gap.max()):.1f} nats and is key {int(top.indices[..., 0].min())} .. "
          f"{int(top.indices[..., 0].max())}")
    assert float(gap.min()) > 50 and int(top.indices[..., 0].min()) >= 21 * 32
    _inside(R, f"spiked {prec}:", bd.c_f32(R["A"]["spread"]))


@pytest.mark.parametrize("nS", [1, 3])
@pytest.mark.parametrize("variant", ["h", "w"])
def test_band_masked_case_is_exact_in_every_arithmetic(variant, nS):
    """P in {0, 2^-5}, delta = 0, dS' = 2^-8 dP: every rounded operand of the bf16 contract (r(dO), r(P), r(dS'), r(G_h), r(G_w)) is the
    value itself, every sum is a sum of integers times 2^-8 below 2^24: the four restatements agree bitwise"""
    R = bd.references(("band", variant, nS, "bf16"), lambda: bd.band_case(variant, nS, "bf16"), magnitude=False)
    qkv, Rh, Rw, dO = (t.double() for t in R["in"])
    for t in bd.band_case(variant, nS, "fp32"):
        assert torch.equal(t.to(torch.bfloat16).float(), t) and torch.equal(t.to(torch.float16).float(), t)
    for c in range(nS):
        q, k, v = br._split(qkv[c * 1024:(c + 1) * 1024], 1)
        P = torch.softmax(br._logits(q, k, Rh, Rw, 1) * br.SCALE, -1)
        dOh = dO[c * 1024:(c + 1) * 1024].reshape(1, 1024, 16, 64).permute(0, 2, 1, 3)
        dP = dOh @ v.transpose(-1, -2)
        dS = br.SCALE * P * dP
        G = dS.reshape(1, 16, 32, 32, 32, 32)
        assert sorted(P.unique().tolist()) == [0.0, 2.0 ** -5] and int((P > 0).sum()) == 16 * 1024 * 32
        assert not bool((P * dP).sum(-1).any()) and float(dP.abs().max()) <= 64
        for t in (P, dS, G.sum(-1), G.sum(-2)):
            assert torch.equal(ab.round_bf16(t), t)
        if c:
            assert not torch.equal(qkv[:1024], qkv[c * 1024:(c + 1) * 1024]) and not torch.equal(dO[:1024], dO[c * 1024:(c + 1) * 1024])
    live = {n: int((R["r64"][n] != 0).sum()) for n in NAMES}
    same = {n: all(torch.equal(R[k][n].double(), R["r64"][n]) for k in ("r32", "b32", "b64")) for n in NAMES}
    print(f"band-masked {variant} nS={nS}: non-zero elements {live}; r32 == b32 == b64 == r64 bitwise: {same}")
    assert all(same.values())
    zero, other = ("dRh", "dRw") if variant == "h" else ("dRw", "dRh")
    assert live[zero] == 0 and live[other] > 0 and live["dq"] > 900000 * nS and live["dk"] > 15000 * nS and live["dv"] > 900000 * nS


# ---- (c) mutants ----------------------------------------------------------------------------------------------------------------
def _backward_with(qkv, Rh, Rw, dO, rnd, zero_delta_last=False, bias_row_61_for_62=False):
    """attn_bwd_bf16_reference._one_crop with two faults that can be switched on: delta = 0 for query 1023 of every head; the Rh bias
    term of dq read from table row 61 where row 62 (qy - ky = 31) belongs"""
    q, k, v = br._split(qkv, 1)
    P = torch.softmax(br._logits(q, k, Rh, Rw, 1) * br.SCALE, -1)
    dOr = rnd(dO).reshape(1, 1024, br.HEADS, br.HD).permute(0, 2, 1, 3)
    dP = dOr @ v.transpose(-1, -2)
    delta = (P * dP).sum(-1, keepdim=True)
    if zero_delta_last:
        delta[:, :, 1023] = 0
    dS = br.SCALE * P * (dP - delta)
    dv = rnd(P).transpose(-1, -2) @ dOr
    dSr = rnd(dS)
    dk = dSr.transpose(-1, -2) @ q
    d5 = dS.reshape(1, br.HEADS, br.GRID, br.GRID, br.GRID, br.GRID)
    Gh, Gw = d5.sum(-1), d5.sum(-2)
    idx = br._rel_index()
    idx_h = torch.where(idx == 62, torch.full_like(idx, 61), idx) if bias_row_61_for_62 else idx
    bias = torch.einsum("bnhwk,hkc->bnhwc", rnd(Gh), Rh[idx_h]) + torch.einsum("bnhwk,wkc->bnhwc", rnd(Gw), Rw[idx])
    dq = dSr @ k + bias.reshape(1, br.HEADS, 1024, br.HD)
    qg = q.reshape(1, br.HEADS, br.GRID, br.GRID, br.HD)
    dRh, dRw = torch.zeros_like(Rh), torch.zeros_like(Rw)
    dRh.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->hkc", Gh, qg).reshape(-1, br.HD))
    dRw.index_add_(0, idx.reshape(-1), torch.einsum("bnhwk,bnhwc->wkc", Gw, qg).reshape(-1, br.HD))
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(1024, br.HEADS * br.HD)
    return {"dq": rows(dq), "dk": rows(dk), "dv": rows(dv), "dRh": dRh, "dRw": dRw}


def _old_rules(mode, X, R):
    """{name: accepted by the norm rules of the older tests}"""
    e = tr.rel_l2
    ok = {}
    for n in NAMES:
        cpu = R["r32"] if mode == "float32" else R["b32"]
        ok[n] = e(X[n], R["r64"][n]) <= max(4 * e(cpu[n], R["r64"][n]), FLOOR)
        if mode == "bf16":
            tol = e(R["b64"][n], R["r64"][n]) / 4 if n in ("dq", "dk", "dv") else max(4 * e(R["b32"][n], R["b64"][n]), FLOOR)
            ok[n] = ok[n] and e(X[n], R["b64"][n]) <= tol
    return ok


def _new_rule(mode, X, R, what):
    """{name: accepted by the per-element rules of tests/test_gpu_attn_bwd_every_element.py}"""
    ok = {}
    for n in NAMES:
        if mode == "float32":
            w, cpu = bd.check(X[n], R["r64"][n], R["A"][n], f"{what} {n}"), float(bd.ratios(R["r32"][n], R["r64"][n], R["A"][n]).max())
            ok[n] = w <= bd.C_F32 and w <= max(4 * cpu, 1.0)
        else:
            w, cpu = bd.check(X[n], R["b64"][n], R["A"][n], f"{what} {n}", 1.0), float(bd.ratios(R["b32"][n], R["b64"][n], R["A"][n], 1.0).max())
            ok[n] = w <= 4 * cpu and bd.fraction_above(X[n], R["b64"][n], R["A"][n]) <= 0.002
    return ok


def _verdict(mode, name, X, R, hit, clean=None):
    old, new = _old_rules(mode, X, R), _new_rule(mode, X, R, f"{mode} mode, {name}:")
    print(f"{mode} mode, mutant '{name}': norm rules (i){' and (ii)' if mode == 'bf16' else ''} accept {old}; per-element check accepts {new}")
    assert not any(new[n] for n in hit), (name, new)
    assert all(new[n] for n in (clean if clean is not None else [n for n in NAMES if n not in hit])), (name, new)     # and blames nothing else
    return all(old.values())


@pytest.mark.parametrize("mode", ["float32", "bf16"])
def test_mutants_of_one_crop_are_rejected(mode):
    R = _random("bf16", 1.0, 1, "scaled")
    base = R["r32"] if mode == "float32" else R["b32"]
    rnd = ab.identity if mode == "float32" else ab.round_bf16
    qkv, Rh, Rw, dO = (t.float() for t in R["in"])
    plain = _backward_with(qkv, Rh, Rw, dO, rnd)
    assert _verdict(mode, "none", base, R, ()) and _verdict(mode, "none (the copy of the restatement the faults are switched on in)", plain, R, ())
    passed_old = {}
    factor = 1.3 if mode == "bf16" else 1.0005       # the norm rule of the float32 mode has a tolerance of 1.5e-6: it sees 1.3, not 1.0005
    for n in ("dq", "dk", "dv"):
        X = {k: v.clone() for k, v in base.items()}
        X[n][1:33, :64] *= factor
        passed_old[f"rows 1..32 of head 0 of {n} times {factor}"] = _verdict(mode, f"rows 1..32 of head 0 of {n} times {factor}", X, R, (n,))
    X = _backward_with(qkv, Rh, Rw, dO, rnd, bias_row_61_for_62=True)
    passed_old["table row 61 for 62 in dq"] = _verdict(mode, "the Rh bias term of dq from table row 61 where row 62 belongs", X, R, ("dq",))
    X = _backward_with(qkv, Rh, Rw, dO, rnd, zero_delta_last=True)
    passed_old["delta = 0 for the last query"] = _verdict(mode, "delta = 0 for the last query of every head", X, R, ("dq",), ("dv",))
    print(f"{mode} mode: accepted by the norm rules on every output: {passed_old}")
    # measured here: the norm rules accept the three row mutants in both modes; they do see the wrong table row and the zero delta
    # (dq is off by 3e-3 and more in the norm), and the remainder's partial below -- those are printed, not asserted
    assert all(ok for what, ok in passed_old.items() if what.startswith("rows"))


@pytest.mark.parametrize("mode", ["float32", "bf16"])
def test_mutant_of_the_remainder_crops_table_partial_is_rejected(mode):
    """nS = 3: the blocks' backward adds the table gradients of a slab of two crops and of the one-crop remainder; the remainder's
    partial scaled by 1 + 2^-10"""
    R = _random("bf16", 1.0, 3, "scaled")
    base = R["r32"] if mode == "float32" else R["b32"]
    qkv, Rh, Rw, dO = (t.float() for t in R["in"])
    last = _backward_with(qkv[2048:], Rh, Rw, dO[2048:], ab.identity if mode == "float32" else ab.round_bf16)
    X = dict(base)
    X["dRh"], X["dRw"] = base["dRh"] + 2.0 ** -10 * last["dRh"], base["dRw"] + 2.0 ** -10 * last["dRw"]
    old = _verdict(mode, "the remainder crop's table partial times 1 + 2^-10", X, R, ("dRh", "dRw"))
    print(f"{mode} mode: accepted by the norm rules on every output: {old}")
