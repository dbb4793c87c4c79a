"""Every element of dq, dk, dv, dRel_h and dRel_w of the attention backward, in both precisions (cpx_attention_backward,
csrc/cpx_train_blocks.hip; cpx_attention_backward_bf16, csrc/cpx_attn_bwd16.hip), against the restatements of
tests/block_train_reference.py and tests/attn_bwd_bf16_reference.py on the error scale A of tests/attn_bwd_bounds.py (DESIGN 6d').
tests/test_attn_bwd_bounds_host.py holds the restatements themselves to the same bounds on the same cases and shows what the check
rejects.  The references of a case (about 2 s of CPU per crop) are computed once per run and shared.

  float32 mode, r64 the float64 restatement, r32 the same in torch CPU float32:
      |device - r64| <= c 2^-24 A                                           the derived bound (attn_bwd_bounds: c = 2140 at spread <= 4)
      max |device - r64| / A <= max(4 max |r32 - r64| / A, 2^-24)          the project's factor 4 on the worst element
  bf16 mode, b64 / b32 the restatement with the contract's roundings in float64 / float32:
      max |device - b64| / A <= 4 max |b32 - b64| / A
      at most 0.2 % of the elements above 64 * 2^-24 A (the CPU's b32: at most 0.05 %, held by the host test)
  band-masked integer cases: torch.equal with float64 on all five outputs, in both modes.
Every test prints a line ``every-element ...`` per output with the device's and the CPU's worst ratio before it asserts;
profiles/attn_bwd_every_element.txt is those lines of one run."""
from __future__ import annotations

import pytest
import torch

import attn_bwd_bounds as bd
import block_train_reference as br
import test_gpu_attn_bwd_bf16 as t16
import test_gpu_block_train as bt
from attn_bwd_bounds import NAMES

pytestmark = pytest.mark.gpu
MODES = ("float32", "bf16")


def _device(mode, inputs, dev):
    """the five outputs on the CPU by name, and whether two runs on differently poisoned workspaces were bitwise equal"""
    (dqkv, drh, drw), same = (bt._attn_run if mode == "float32" else t16._attn_run)(*inputs, dev)
    return bd.pick({"dqkv": dqkv.cpu(), "dRh": drh.cpu(), "dRw": drw.cpu()}), same


def _judge(mode, case, R, dev, spiked=False):
    ok = []
    for n in NAMES:
        A = R["A"][n]
        if mode == "float32":
            c = bd.c_f32(max(R["A"]["spread"], 4.0)) if spiked else bd.C_F32
            w = bd.check(dev[n], R["r64"][n], A, f"{case} {n} device")
            cpu = float(bd.ratios(R["r32"][n], R["r64"][n], A).max())
            print(f"every-element float32 mode {case} {n}: worst |x - r64| / (2^-24 A): device {w:.4g}, CPU float32 {cpu:.4g}; "
                  f"allowed min({c:.0f}, max(4 CPU, 1)) = {min(c, max(4 * cpu, 1.0)):.4g}")
            ok.append(w <= c and w <= max(4 * cpu, 1.0))
        else:
            w = bd.check(dev[n], R["b64"][n], A, f"{case} {n} device", 1.0)
            cpu = float(bd.ratios(R["b32"][n], R["b64"][n], A, 1.0).max())
            frac, frac_cpu = bd.fraction_above(dev[n], R["b64"][n], A), bd.fraction_above(R["b32"][n], R["b64"][n], A)
            # the spiked case: every key but one has the same tiny P, so one rounding flip of r(P) moves a dv element by more than
            # 64 * 2^-24 A and the CPU's own share is 4.5 %: there the factor 4 applies to the share as well
            cap = max(0.002, 4 * frac_cpu) if spiked else 0.002
            print(f"every-element bf16 mode {case} {n}: worst |x - b64| / A: device {w:.4g}, CPU b32 {cpu:.4g}, allowed {4 * cpu:.4g}; "
                  f"share above 64 * 2^-24 A: device {100 * frac:.4f} %, CPU {100 * frac_cpu:.4f} %, allowed {100 * cap:.2f} %")
            ok.append(w <= 4 * cpu and frac <= cap)
    return ok


def test_the_cases_are_those_of_the_norm_tests():
    for args in ((1, "bf16", 61, 7.5), (3, "fp16", 61, 1.0)):
        assert all(torch.equal(a, b) for a, b in zip(bd.attn_case(*args), bt._attn_case(*args)))
    scaled, flat = bd.attn_case(1, "fp32", 61), bd.attn_case(1, "fp32", 61, dout="flat")
    assert all(torch.equal(a, b) for a, b in zip(scaled[:3], flat[:3]))
    share = lambda d: float(d[:, :64].double().square().sum() / d.double().square().sum())
    print(f"share of head 0 in the energy of dO: scaled {share(scaled[3]):.2e}, flat {share(flat[3]):.2e}")
    assert share(scaled[3]) < 1e-3 and 0.05 < share(flat[3]) < 0.08


# ---- random data -----------------------------------------------------------------------------------------------------------------
def _random(cuda, mode, prec, qscale, nS, dout):
    R = bd.references(("random", prec, qscale, nS, dout), lambda: bd.attn_case(nS, prec, 61, qscale, dout))
    dev, same = _device(mode, R["in"], cuda)
    ok = _judge(mode, f"{prec} qscale={qscale} nS={nS} dO {dout}", R, dev)
    zero_dq = not bool(dev["dq"][::5].any())
    zero_pad = not bool(dev["dRh"][63].any()) and not bool(dev["dRw"][63].any())
    print(f"  two runs bitwise equal {same}; rows with dO = 0 give zero dq {zero_dq}; row 63 of both table gradients zero {zero_pad}")
    assert all(ok) and same and zero_dq and zero_pad


@pytest.mark.parametrize("dout", bd.DOUTS)
@pytest.mark.parametrize("prec,qscale,nS", bd.F32_CASES)
def test_float32_mode_every_element(cuda, prec, qscale, nS, dout):
    _random(cuda, "float32", prec, qscale, nS, dout)


@pytest.mark.parametrize("dout", bd.DOUTS)
@pytest.mark.parametrize("prec,qscale,nS", bd.BF16_CASES)
def test_bf16_mode_every_element(cuda, prec, qscale, nS, dout):
    _random(cuda, "bf16", prec, qscale, nS, dout)


# ---- band-masked integers --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nS", [1, 3])
@pytest.mark.parametrize("variant", ["h", "w"])
@pytest.mark.parametrize("mode", MODES)
def test_band_masked_integers_are_exact(cuda, mode, variant, nS):
    """attn_bwd_bounds.band_case: one table masks all keys but those of the query's image row ("h") or column ("w") with a logit of
    -1024 nats, so P is 2^-5 on 32 keys and 0 on 992, delta = 0 and dS' = 2^-8 dP, and k and both tables carry integers: every table row
    Rh[qy - ky + 31], Rw[qx - kx + 31] enters dq with an integer weight, the masked tiles pass through the running maximum and its
    rescale, and any float32 order of the sums is exact.  A wrong table row, a wrong sign of the offset, a stale maximum or a masked
    key that leaks changes integers.  (tests/test_attn_bwd_bounds_host.py asserts that every rounded operand is representable.)"""
    prec = "fp32" if mode == "float32" else "bf16"
    R = bd.references(("band", variant, nS, prec), lambda: bd.band_case(variant, nS, prec), magnitude=False)
    cpu_exact = all(torch.equal(R[k][n].double(), R["r64"][n]) for k in R if k[0] in "rb" for n in NAMES)
    dev, same = _device(mode, R["in"], cuda)
    eq = {n: torch.equal(dev[n].double(), R["r64"][n]) for n in NAMES}
    live = {n: int((R["r64"][n] != 0).sum()) for n in NAMES}
    off = {n: int((dev[n].double() != R["r64"][n]).sum()) for n in NAMES}
    print(f"every-element {mode} mode band-masked {variant} nS={nS}: CPU restatements bitwise equal {cpu_exact}; device equal to float64 {eq} "
          f"(elements that differ {off}); non-zero {live}; two runs bitwise equal {same}")
    zero, other = ("dRh", "dRw") if variant == "h" else ("dRw", "dRh")
    assert cpu_exact and all(eq.values()) and same
    assert live[zero] == 0 and live[other] > 0 and min(live["dq"], live["dv"]) > 900000 * nS and live["dk"] > 15000 * nS


# ---- a spiked key ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_spiked_key_every_element(cuda, mode):
    """attn_bwd_bounds.spiked_case: per head one key, in key tiles 21 .. 30, whose logit is about 60 nats above every other: pass 1 meets
    it after 21 tiles and rescales l_run and d_run by e^-60; P is 1 on it, delta = dP of it, and dS' of it is what the cancellation
    leaves.  The hard bound takes the case's own spread (32: the spiked key's Lam against the others')"""
    prec = "fp32" if mode == "float32" else "bf16"
    R = bd.references(("spiked", prec), lambda: bd.spiked_case(prec))
    qkv, Rh, Rw, _ = R["in"]
    lg = br._logits(*br._split(qkv.double(), 1)[:2], Rh.double(), Rw.double(), 1) * br.SCALE
    top = lg.topk(2, -1)
    gap = top.values[..., 0] - top.values[..., 1]
    print(f"spiked {prec}: the spiked key leads by {float(gap.min()):.1f} .. {float(gap.max()):.1f} nats, keys {int(top.indices[..., 0].min())} .. "
          f"{int(top.indices[..., 0].max())}")
    assert float(gap.min()) > 50 and int(top.indices[..., 0].min()) >= 21 * 32
    dev, same = _device(mode, R["in"], cuda)
    ok = _judge(mode, f"spiked {prec}", R, dev, spiked=True)
    assert all(ok) and same
