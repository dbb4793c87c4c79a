"""Host checks of the attention backward on bf16 operands: the CPU restatement tests/attn_bwd_bf16_reference.py against the
unrounded backward, the C ABI's additive entries, and the refusals of the CLI and the trainer.  No GPU."""
from __future__ import annotations

import os
import re
import subprocess

import pytest
import torch

import attn_bwd_bf16_reference as ab
import block_train_bf16_reference as bb
import block_train_reference as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICES = (("dq", slice(0, 1024)), ("dk", slice(1024, 2048)), ("dv", slice(2048, 3072)))
_CASE = {}


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _case():
    """one crop of bf16 values, dO with zero rows; the unrounded float64 backward is computed once"""
    if not _CASE:
        g = torch.Generator().manual_seed(71)
        qkv = torch.randn(1024, 3072, generator=g).to(torch.bfloat16).double()
        tab = lambda: torch.cat([torch.randn(63, 64, generator=g) * 0.5, torch.zeros(1, 64)]).to(torch.bfloat16).double()
        Rh, Rw = tab(), tab()
        dO = (torch.randn(1024, 1024, generator=g) * torch.logspace(-2, 0, 1024)[None]).double()
        dO[::5] = 0
        _CASE.update(qkv=qkv, Rh=Rh, Rw=Rw, dO=dO, r64=br.attention_backward(qkv, Rh, Rw, dO, 1))
    return _CASE


def _dists(got, want):
    d = {n: _rel(got["dqkv"][:, s], want["dqkv"][:, s]) for n, s in SLICES}
    d["dRh"], d["dRw"] = _rel(got["dRh"], want["dRh"]), _rel(got["dRw"], want["dRw"])
    return d


def test_without_rounding_the_restatement_is_attention_backward():
    c = _case()
    got = ab.attention_backward_bf16(c["qkv"], c["Rh"], c["Rw"], c["dO"], 1, rnd=ab.identity)
    d = _dists(got, c["r64"])
    print("rnd = identity against block_train_reference.attention_backward, float64: " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    assert max(d.values()) < 1e-10


def test_with_rounding_it_differs_by_about_a_bf16_ulp_and_keeps_the_structure():
    c = _case()
    got = ab.attention_backward_bf16(c["qkv"], c["Rh"], c["Rw"], c["dO"], 1)
    d = _dists(got, c["r64"])
    only_do = ab.attention_backward_bf16(c["qkv"], c["Rh"], c["Rw"], bb.round_bf16(c["dO"]), 1, rnd=ab.identity)
    d2 = {n: _rel(only_do["dqkv"][:, s], got["dqkv"][:, s]) for n, s in SLICES}
    print("restatement (float64) against the unrounded backward: " + ", ".join(f"{k} {v:.3e}" for k, v in d.items()))
    print("a version that rounds only dO against the restatement: " + ", ".join(f"{k} {v:.3e}" for k, v in d2.items()))
    assert all(2.0 ** -13 < v < 2.0 ** -6 for v in d.values())
    assert all(v > 2.0 ** -12 for v in d2.values()), "the roundings of P and dS' are there"
    assert not bool(got["dqkv"][::5, :1024].any()), "rows with dO = 0 give exactly zero dq"
    assert not bool(got["dRh"][63].any()) and not bool(got["dRw"][63].any())
    two = ab.attention_backward_bf16(torch.cat([c["qkv"], c["qkv"]]), c["Rh"], c["Rw"], torch.cat([c["dO"], c["dO"]]), 2)
    assert torch.equal(two["dqkv"][1024:], got["dqkv"]) and torch.equal(two["dRh"], got["dRh"] + got["dRh"])


def test_the_block_restatement_substitutes_the_attention_backward_and_puts_it_back():
    from classpose_amd import synth
    P = br.params_from_state_dict(synth.make_state_dict(3, None, depth=1, seed=51), 0)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(1024, 1024, generator=g) * torch.logspace(-0.5, 0.5, 1024)[:, None]
    dout = torch.randn(1024, 1024, generator=g) * torch.logspace(-2, 0, 1024)[None]
    plain_fn = br.attention_backward
    args = (P, x, dout, 1, torch.float64, torch.bfloat16, True)
    same = ab.block_backward(*args, rnd=bb.round_bf16, attn_rnd=ab.identity)
    plain = bb.block_backward(*args, rnd=bb.round_bf16)
    got = ab.block_backward(*args, rnd=bb.round_bf16)
    assert br.attention_backward is plain_fn
    e0 = max(_rel(same["grads"][k], plain["grads"][k]) for k in br.NAMES)
    away = {k: _rel(got["grads"][k], plain["grads"][k]) for k in ("qkv_w", "rel_h", "rel_w", "ln1_g")}
    print(f"attention rounding off: worst distance from block_train_bf16_reference {e0:.3e}; on: " + ", ".join(f"{k} {v:.3e}" for k, v in away.items()))
    assert e0 < 1e-10 and all(2.0 ** -14 < v < 2.0 ** -5 for v in away.values())
    for k in ("proj_w", "proj_b", "fc1_w", "fc2_w", "ln2_g"):          # upstream of the attention backward: untouched
        assert torch.equal(got["grads"][k], plain["grads"][k]), k


def test_attention_bf16_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    counts = {"cpx_attention_backward_bf16_workspace_bytes": 1, "cpx_attention_backward_bf16": 11, "cpx_blocks_backward_workspace_bytes_mp": 4,
              "cpx_blocks_backward_mp": 14, "cpx_blocks_backward_ex": 13, "cpx_blocks_backward": 12, "cpx_attention_backward": 13,
              "cpx_blocks_backward_workspace_bytes_ex": 3}
    for name, n in counts.items():
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    L = _lib.lib()
    f32, b16, f16 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16
    mp, ex = L.cpx_blocks_backward_workspace_bytes_mp, L.cpx_blocks_backward_workspace_bytes_ex
    for dt in (f32, b16, f16):
        assert mp(3, dt, f32, f32) == ex(3, dt, f32) > 0
    assert mp(3, b16, b16, f32) == ex(3, b16, b16) > 0
    assert mp(3, b16, b16, b16) > 0 and mp(32, b16, b16, b16) == mp(3, b16, b16, b16)
    invalid = [(3, b16, f32, b16), (3, f32, f32, b16), (3, f16, f32, b16), (3, f16, b16, b16), (3, f32, b16, b16), (3, b16, b16, f16),
               (0, b16, b16, b16)]
    for a in invalid:
        assert mp(*a) == 0, a
    a16 = L.cpx_attention_backward_bf16_workspace_bytes
    assert a16(1) == L.cpx_attention_backward_workspace_bytes(1) > 0 and a16(3) == L.cpx_attention_backward_workspace_bytes(3)
    assert a16(0) == 0 and a16(-1) == 0 and a16(16384) == 0 and a16(16383) > 0


def _args(**kw):
    from classpose_amd.entrypoints import train_head
    a = train_head.build_parser().parse_args(["--images", "i.npy", "--labels", "l.npy", "--pretrained_model", "m.pt", "--save_path", "s",
                                              "--model_name", "n"])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_cli_refuses_a_bf16_attention_backward_without_bf16_gradients():
    """check_args runs before anything touches the device"""
    from classpose_amd.entrypoints import train_head
    assert _args().attn_grad_precision == "fp32"
    with pytest.raises(SystemExit, match=r"--attn_grad_precision bf16 needs --grad_precision bf16"):
        train_head.check_args(_args(attn_grad_precision="bf16"))
    with pytest.raises(SystemExit, match=r"--attn_grad_precision bf16 needs --grad_precision bf16"):
        train_head.check_args(_args(attn_grad_precision="bf16", train_blocks=1, precision="bf16"))
    with pytest.raises(SystemExit, match=r"--grad_precision bf16 goes with --train_blocks"):
        train_head.check_args(_args(attn_grad_precision="bf16", grad_precision="bf16"))
    with pytest.raises(SystemExit, match=r"loss scaling"):
        train_head.check_args(_args(attn_grad_precision="bf16", grad_precision="bf16", train_blocks=1, precision="fp16"))
    ok = _args(attn_grad_precision="bf16", grad_precision="bf16", train_blocks=1, precision="bf16")
    train_head.check_args(ok)
    assert ok.attn_grad_precision == "bf16" and ok.grad_precision == "bf16" and ok.train_neck
    plain = _args(grad_precision="bf16", train_blocks=1, precision="bf16")
    del plain.attn_grad_precision                                       # a namespace built before the flag existed
    train_head.check_args(plain)
    assert plain.attn_grad_precision == "fp32"
    with pytest.raises(SystemExit):
        train_head.build_parser().parse_args(["--attn_grad_precision", "fp16"])


def test_trainer_argument_check_names_the_reason():
    import inspect
    from classpose_amd.train import HeadTrainer, check_attn_grad_precision, check_grad_precision
    check_attn_grad_precision("fp32", "fp32")
    check_attn_grad_precision("fp32", "bf16")
    check_attn_grad_precision("bf16", "bf16")
    with pytest.raises(ValueError, match="needs grad_precision bf16"):
        check_attn_grad_precision("bf16", "fp32")
    with pytest.raises(ValueError, match="'fp32' or 'bf16'"):
        check_attn_grad_precision("fp16", "bf16")
    assert list(inspect.signature(check_grad_precision).parameters) == ["grad_precision", "train_blocks", "precision"]
    assert inspect.signature(HeadTrainer.__init__).parameters["attn_grad_precision"].default == "fp32"
    # the trainer checks its arguments before it looks at the device or the checkpoint
    with pytest.raises(ValueError, match="needs grad_precision bf16"):
        HeadTrainer({}, 3, device="cpu", precision="bf16", train_blocks=1, attn_grad_precision="bf16")
    with pytest.raises(ValueError, match="needs grad_precision bf16"):
        HeadTrainer({}, 3, device="cpu", precision="bf16", train_blocks=1, grad_precision="fp32", attn_grad_precision="bf16")


def test_ops_refuse_the_combinations_before_any_launch():
    from classpose_amd import _lib, ops
    with pytest.raises(ValueError, match="needs grad_dtype torch.bfloat16"):
        ops.blocks_backward_workspace(1, _lib.DT_BF16, "cpu", torch.float32, torch.bfloat16)
    with pytest.raises(ValueError, match="attn_grad_dtype is torch.float32 or torch.bfloat16"):
        ops.blocks_backward_workspace(1, _lib.DT_BF16, "cpu", torch.bfloat16, torch.float16)
    with pytest.raises(ValueError, match="needs a bf16 network"):
        ops.blocks_backward_workspace(1, _lib.DT_F16, "cpu", torch.bfloat16, torch.bfloat16)
    t = torch.zeros(1024, 3072, dtype=torch.float16)
    with pytest.raises(ValueError, match="needs bf16 qkv"):
        ops.attention_backward(t, t, t, t, t, grad_dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="grad_dtype is torch.float32 or torch.bfloat16"):
        ops.attention_backward(t, t, t, t, t, grad_dtype=torch.float16)
