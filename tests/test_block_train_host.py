"""tests/block_train_reference.py against the oracle's network and against float64 autograd: the restated block forward is the
oracle's block, and the hand-written backward formulas the kernels of csrc/cpx_train_blocks.hip implement (attention with the
decomposed rel-pos bias, erf GELU, LayerNorm at C = 1024, the rel-pos interpolation's transpose) are the derivatives autograd finds."""
from __future__ import annotations

import torch
import torch.nn.functional as F

import block_train_reference as br
import neck_train_reference as nr
from classpose_amd import engine, synth
from oracle import net as onet

_SD = {}


def _sd():
    if "sd" not in _SD:
        _SD["sd"] = synth.make_state_dict(3, None, depth=1, seed=51)
    return _SD["sd"]


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_block_forward_is_the_oracles_block():
    sd = {k: v.double() for k, v in _sd().items() if v.is_floating_point()}
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 32, 32, 1024, generator=g, dtype=torch.float64)
    p = "encoder.blocks.0."
    h = F.layer_norm(x, x.shape[-1:], sd[p + "norm1.weight"], sd[p + "norm1.bias"], 1e-6)
    y = x + onet._attention(sd, p + "attn.", h, 16)
    h = F.layer_norm(y, y.shape[-1:], sd[p + "norm2.weight"], sd[p + "norm2.bias"], 1e-6)
    y = y + F.linear(F.gelu(F.linear(h, sd[p + "mlp.lin1.weight"], sd[p + "mlp.lin1.bias"])), sd[p + "mlp.lin2.weight"], sd[p + "mlp.lin2.bias"])
    P = br.params_from_state_dict(_sd(), 0)
    R = br.rounded(P, torch.float64, None)
    o = br.block_forward(R, x.reshape(2048, 1024), 2)
    err = _rel(o["out"], y.reshape(2048, 1024))
    print(f"block forward against the oracle: relative error {err:.3e}")
    assert err < 1e-12
    # folding LayerNorm into the Linear is the same function
    o2 = br.block_forward({k: v.float() for k, v in R.items()}, x.reshape(2048, 1024).float(), 2, torch.bfloat16, fold=True)
    o3 = br.block_forward({k: v.float() for k, v in R.items()}, x.reshape(2048, 1024).float(), 2, torch.bfloat16, fold=False)
    print(f"bf16 replay, folded against unfolded: {_rel(o2['out'], o3['out']):.3e}")
    assert _rel(o2["out"], o3["out"]) < 2e-2


def test_unfolded_half_forward_is_the_oracles_unfused_half_forward():
    """fold=False with a half network dtype is the network built with fuse_ln=False: LayerNorm writes its output in the network dtype and
    the GEMM reads that.  The oracle in bf16 / fp16 (torch CPU, every op's output in the dtype) does the same, so with the LayerNorm
    output rounded the two GEMMs multiply the same operands and differ by the float32 summation order alone: d = sqrt(1024) 2^-24 =
    2^-19 relative before the output rounding.  That rounding then lands on the neighbouring value for a fraction d / ulp of the
    elements, an error of one ulp each: sqrt(d ulp) in relative L2, 1.0e-4 for bf16 (relative ulp about 2^-7.5) and 3.6e-5 for fp16
    (2^-10.5).  Without the rounding of the LayerNorm output every element of the operand is off by ulp / sqrt 12 in the mean, so the
    product is too (d' = 1.6e-3 / 2.0e-4), and the output rounding adds sqrt(d' ulp): 3e-3 / 3.7e-4 together.  The bounds, 2^-11 for
    bf16 and 2^-13 for fp16, lie a factor 3 to 6 from either side.  One whole block against the oracle's, where the oracle also rounds
    the pre-activation, the softmax and both branch outputs before the residual -- a few roundings of an ulp each on top of the
    output's own: 2^-6 (bf16) and 2^-9 (fp16)."""
    sd = _sd()
    P = br.params_from_state_dict(sd, 0)
    g = torch.Generator().manual_seed(6)
    x32 = torch.randn(1024, 1024, generator=g) * torch.logspace(-0.5, 0.5, 1024)[:, None] + 0.3 * torch.randn(1024, 1, generator=g)
    p = "encoder.blocks.0."
    for hd, bound, whole in ((torch.bfloat16, 2.0 ** -11, 2.0 ** -6), (torch.float16, 2.0 ** -13, 2.0 ** -9)):
        x = x32.to(hd)
        R = br.rounded(P, torch.float32, hd)
        for ln, lin, names in (("norm1", "attn.qkv", ("ln1_g", "ln1_b", "qkv_w", "qkv_b")), ("norm2", "mlp.lin1", ("ln2_g", "ln2_b", "fc1_w", "fc1_b"))):
            h = F.layer_norm(x, (1024,), sd[p + ln + ".weight"].to(hd), sd[p + ln + ".bias"].to(hd), 1e-6)
            want = F.linear(h, sd[p + lin + ".weight"].to(hd), sd[p + lin + ".bias"].to(hd)).float()
            got = nr.ste(br._ln_linear(x.float(), *(R[n] for n in names), hd, False), hd)
            plain = nr.ste(nr.layernorm(x.float(), R[names[0]], R[names[1]]) @ R[names[2]].T + R[names[3]], hd)
            e, e_plain = _rel(got, want), _rel(plain, want)
            print(f"{hd} {lin}: unfolded replay against the oracle {e:.3e} (bound {bound:.3e}); without the rounding of LayerNorm {e_plain:.3e}")
            assert e <= bound < e_plain
        sdh = {k: v.to(hd) for k, v in sd.items() if v.is_floating_point()}
        xg = x.reshape(1, 32, 32, 1024)
        h = F.layer_norm(xg, (1024,), sdh[p + "norm1.weight"], sdh[p + "norm1.bias"], 1e-6)
        y = xg + onet._attention(sdh, p + "attn.", h, 16)
        h = F.layer_norm(y, (1024,), sdh[p + "norm2.weight"], sdh[p + "norm2.bias"], 1e-6)
        y = y + F.linear(F.gelu(F.linear(h, sdh[p + "mlp.lin1.weight"], sdh[p + "mlp.lin1.bias"])), sdh[p + "mlp.lin2.weight"], sdh[p + "mlp.lin2.bias"])
        o = br.block_forward(R, x.float(), 1, hd, fold=False)
        e = _rel(o["out"], y.reshape(1024, 1024).float())
        print(f"{hd} one block, unfolded replay against the oracle's block in the dtype: {e:.3e} (bound {whole:.3e})")
        assert e <= whole and torch.equal(o["out"].to(hd).float(), o["out"])


def test_ln_linear_without_a_network_dtype_is_unchanged():
    """net_dtype None (and float32): nothing is rounded, folded or not -- bit for bit the expression the branch held before"""
    P = br.params_from_state_dict(_sd(), 0)
    g = torch.Generator().manual_seed(7)
    for dt in (torch.float64, torch.float32):
        x = torch.randn(256, 1024, generator=g).to(dt)
        a = [P[n].to(dt) for n in ("ln1_g", "ln1_b", "qkv_w", "qkv_b")]
        want = nr.layernorm(x, a[0], a[1]) @ a[2].T + a[3]
        for net in (None, torch.float32):
            for fold in (False, True):
                assert torch.equal(br._ln_linear(x, *a, net, fold), want), (dt, net, fold)
    xx = torch.randn(256, 1024, generator=g, dtype=torch.float64).requires_grad_(True)
    a = [P[n].double() for n in ("ln2_g", "ln2_b", "fc1_w", "fc1_b")]
    w = torch.randn(256, 4096, generator=g, dtype=torch.float64)
    (br._ln_linear(xx, *a, torch.bfloat16, False) * w).sum().backward()
    got, xx.grad = xx.grad.clone(), None
    (br._ln_linear(xx, *a, None, False) * w).sum().backward()
    assert _rel(got, xx.grad) < 1e-14, "the rounding of the LayerNorm output passes the gradient straight through"


def test_rel_operand_is_the_loaded_table():
    sd = _sd()
    rel = sd["encoder.blocks.0.attn.rel_pos_h"]
    assert rel.shape[0] != 63, "the synthetic checkpoint's table is interpolated at load"
    A = br.interp_matrix(rel.shape[0])
    assert A.shape == (63, rel.shape[0])
    assert _rel(A @ rel.double(), engine.interp_rel_pos(rel.double())) < 1e-14
    for hd in (torch.bfloat16, torch.float16):
        want = torch.cat([engine.interp_rel_pos(rel.to(hd)).float() * 8.0, torch.zeros(1, 64)], 0)
        got = br.rel_operand(rel.double(), hd)
        assert torch.equal(got.float(), want) and torch.equal(want.to(hd).float(), want)
    r = rel.double().clone().requires_grad_(True)
    w = torch.randn(64, 64, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    (br.rel_operand(r, torch.bfloat16) * w).sum().backward()
    assert _rel(r.grad, 8.0 * A.T @ w[:63]) < 1e-14, "the table's gradient goes back through the transpose of the interpolation, times 1 / scale"


def test_attention_backward_formulas_are_autograd():
    g = torch.Generator().manual_seed(3)
    nS = 2
    qkv = torch.randn(nS * 1024, 3072, generator=g, dtype=torch.float64)
    qkv[:, :1024] *= 3.0                                               # logits of a few units
    Rh = torch.cat([torch.randn(63, 64, generator=g, dtype=torch.float64), torch.zeros(1, 64, dtype=torch.float64)])
    Rw = torch.cat([torch.randn(63, 64, generator=g, dtype=torch.float64), torch.zeros(1, 64, dtype=torch.float64)])
    dO = torch.randn(nS * 1024, 1024, generator=g, dtype=torch.float64)
    dO[1024:] = 0                                                      # the second crop sees no gradient
    a, rh, rw = (t.clone().requires_grad_(True) for t in (qkv, Rh, Rw))
    (br.attention(a, rh, rw, nS) * dO).sum().backward()
    r = br.attention_backward(qkv, Rh, Rw, dO, nS)
    for name, got, want in (("dqkv", r["dqkv"], a.grad), ("dRh", r["dRh"], rh.grad), ("dRw", r["dRw"], rw.grad)):
        print(f"  {name}: relative error {_rel(got, want):.3e}")
        assert _rel(got, want) < 1e-12
    assert not bool(r["dqkv"][1024:].any()), "no query of one crop sees a key of another"
    assert not bool(r["dRh"][63].any()) and not bool(r["dRw"][63].any())
    # the decomposed bias is the oracle's: attention() on oracle-convention inputs equals oracle.net's attention core
    sd = {k: v.double() for k, v in _sd().items() if v.is_floating_point()}
    p = "encoder.blocks.0.attn."
    x = torch.randn(1, 32, 32, 1024, generator=g, dtype=torch.float64)
    want = onet._attention(sd, p, x, 16).reshape(1024, 1024)
    q = F.linear(x.reshape(1024, 1024), sd[p + "qkv.weight"], sd[p + "qkv.bias"])
    got = F.linear(br.attention(q, br.rel_operand(sd[p + "rel_pos_h"], None), br.rel_operand(sd[p + "rel_pos_w"], None), 1),
                   sd[p + "proj.weight"], sd[p + "proj.bias"])
    assert _rel(got, want) < 1e-12


def test_gelu_and_layernorm_formulas_are_autograd():
    x = torch.cat([torch.linspace(-8, 8, 4001, dtype=torch.float64), torch.tensor([0.0, 1e-30, -1e-30, 6.0, -6.0, 40.0, -40.0], dtype=torch.float64)])
    a = x.clone().requires_grad_(True)
    F.gelu(a).sum().backward()
    d = br.gelu_grad(x)
    assert float((d - a.grad).abs().max()) < 1e-15 and bool(torch.isfinite(d).all())
    assert float(d[-1]) == 0.0 and float(d[-2]) == 1.0 and float(d[-7]) == 0.5
    g = torch.Generator().manual_seed(4)
    y = torch.randn(96, 1024, generator=g, dtype=torch.float64) * 2 + 0.3
    gamma, beta = 1 + 0.2 * torch.randn(1024, generator=g, dtype=torch.float64), torch.randn(1024, generator=g, dtype=torch.float64)
    dout = torch.randn(96, 1024, generator=g, dtype=torch.float64)
    yy, gg, bb = (t.clone().requires_grad_(True) for t in (y, gamma, beta))
    (F.layer_norm(yy, (1024,), gg, bb, nr.EPS) * dout).sum().backward()
    r = nr.ln_backward(y, gamma, dout)
    for got, want in ((r["dy"], yy.grad), (r["dgamma"], gg.grad), (r["dbeta"], bb.grad)):
        assert _rel(got, want) < 1e-12


def test_block_grads_folded_and_unfolded_agree_in_float64():
    """with nothing rounded the folded LayerNorm is the unfolded one: same gradients for W, b, gamma and beta"""
    P = br.params_from_state_dict(_sd(), 0)
    g = torch.Generator().manual_seed(5)
    x, dout = torch.randn(1024, 1024, generator=g), torch.randn(1024, 1024, generator=g)
    a = br.block_grads(P, x, dout, 1, torch.float64, None, fold=False)
    R = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    xx = x.double().clone().requires_grad_(True)
    Rh, Rw = br.rel_operand(R["rel_h"], None), br.rel_operand(R["rel_w"], None)
    qkv = br._xhat(xx) @ (R["qkv_w"] * R["ln1_g"][None]).T + (R["qkv_b"] + R["qkv_w"] @ R["ln1_b"])
    xm = xx + br.attention(qkv, Rh, Rw, 1) @ R["proj_w"].T + R["proj_b"]
    pre = br._xhat(xm) @ (R["fc1_w"] * R["ln2_g"][None]).T + (R["fc1_b"] + R["fc1_w"] @ R["ln2_b"])
    out = xm + F.gelu(pre) @ R["fc2_w"].T + R["fc2_b"]
    (out * dout.double()).sum().backward()
    for k in br.NAMES:
        assert _rel(R[k].grad, a["grads"][k]) < 1e-10, k
    assert _rel(xx.grad, a["dx"]) < 1e-10
