"""The production attention kernel k_attention2w (variant 2: two query rows per wave, two workgroups per CU) against the
round-2/3 kernel k_attention4p (debug variant 7) and a float64 reference: random inputs, one spiked key, a logit ramp that
forces repeated exact rescales; bf16 and fp16; partial rounds of the grid; repeatability under concurrent load."""
import pytest
import torch

from classpose_amd import _lib, ops

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def _ref64(qkv, rel, s0=0):
    """flash_forward of one sub-tile in float64 (rel: the 64 x 64 table the kernel reads, bias = table[idx] / 8)"""
    dev = qkv.device
    q, k, v = qkv[s0 * 1024:(s0 + 1) * 1024].double().reshape(1024, 3, 16, 64).permute(1, 2, 0, 3)
    idx = (torch.arange(32)[:, None] - torch.arange(32)[None, :] + 31).to(dev)
    R = rel.double()[idx] / 8
    qhw = q.reshape(16, 32, 32, 64)
    bias = (torch.einsum("nhwc,hkc->nhwk", qhw, R)[..., :, None] + torch.einsum("nhwc,wkc->nhwk", qhw, R)[..., None, :]).reshape(16, 1024, 1024)
    return (torch.softmax(q @ k.transpose(-1, -2) * 0.125 + bias, -1) @ v).transpose(0, 1).reshape(1024, 1024)


def _run(L, variant, qkv, rel):
    L.cpx_attention_set_variant(variant)
    try:
        return ops.attention(qkv, rel, rel)
    finally:
        L.cpx_attention_set_variant(2)


def _case(name, dt, dev, nS=1):
    g = torch.Generator().manual_seed({"random": 11, "spiked": 6, "ramp": 21}[name])
    if name == "random":
        qkv = (torch.randn(nS * 1024, 3072, generator=g) * 0.7)
        rel = (torch.randn(64, 64, generator=g) * 0.8)
        rel[63] = 0
    elif name == "spiked":                                   # one key dominates every row: the rescale path
        qkv = torch.randn(1024, 3072, generator=g) * 0.1
        qkv[:, :1024] = 1.0
        qkv[700, 1024:2048] = 30.0
        rel = torch.zeros(64, 64)
    else:                                                    # logits grow with the key index (~60 nats over 1024 keys): the running
        u = torch.randn(16, 64, generator=g)                 # reference is overtaken again and again
        u = u / u.norm(dim=1, keepdim=True)
        qkv = torch.randn(1024, 3072, generator=g) * 0.3
        qkv[:, :1024] += (u * 8).reshape(1, 1024)
        ramp = (torch.arange(1024).float() / 1024 * 60)[:, None, None]
        qkv[:, 1024:2048] += (u[None] * ramp).reshape(1024, 1024)
        rel = torch.zeros(64, 64)
    return qkv.to(dt).to(dev), rel.to(dt).to(dev)


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["random", "spiked", "ramp"])
def test_attn2w_error_against_float64_and_round_2_kernel(cuda, dt, name):
    qkv, rel = _case(name, dt, cuda)
    with _lib.use_debug_library() as L:
        new = _run(L, 2, qkv, rel)
        old = _run(L, 7, qkv, rel)
    assert torch.isfinite(new.float()).all()
    ref = _ref64(qkv, rel)
    e_new, e_old = _rel(new, ref), _rel(old, ref)
    assert e_new <= 1.1 * e_old + 1e-7, (e_new, e_old)
    if dt == torch.bfloat16:
        assert e_new < 4e-3, e_new
    if name == "spiked":                                     # every query ~= the spiked key's V
        assert torch.allclose(new.float()[5], qkv[700, 2048:].float(), atol=0.02)
    # per chain, every arithmetic step is k_attention4p's, in the same order
    assert torch.equal(new, old)


@pytest.mark.parametrize("nS", [1, 3, 32, 96])
def test_attn2w_subtile_counts(cuda, nS):
    """partial last rounds of the 64 n_subtiles workgroups and every XCD decode: equal to the round-2/3 kernel, and within
    bf16 rounding of float64 on the first and the last sub-tile"""
    qkv, rel = _case("random", torch.bfloat16, cuda, nS)
    with _lib.use_debug_library() as L:
        new = _run(L, 2, qkv, rel)
        old = _run(L, 7, qkv, rel)
    assert torch.equal(new, old)
    for s0 in {0, nS - 1}:
        assert _rel(new[s0 * 1024:(s0 + 1) * 1024], _ref64(qkv, rel, s0)) < 4e-3


def test_attn2w_repeatable_under_load(cuda):
    """race screen for the LDS-DMA ring behind counted vmcnt + raw barriers, two workgroups per CU: 40 launches on 32
    sub-tiles next to an uneven memory load must be bitwise identical"""
    qkv, rel = _case("random", torch.bfloat16, cuda, 32)
    noise = torch.empty((8192, 8192), device=cuda)
    side = torch.cuda.Stream(cuda)
    with _lib.use_debug_library() as L:
        L.cpx_attention_set_variant(2)
        first = ops.attention(qkv, rel, rel)
        for i in range(40):
            if i % 4 == 0:
                with torch.cuda.stream(side):
                    noise.normal_()
            assert torch.equal(ops.attention(qkv, rel, rel), first), i
        side.synchronize()
    assert torch.equal(ops.attention(qkv, rel, rel), first)     # the product library runs the same kernel
