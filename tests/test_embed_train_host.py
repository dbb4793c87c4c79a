"""Host checks of training the patch embedding and the position table: the CPU statement tests/embed_train_reference.py
against itself, the C ABI's additive entries, and the refusals of the command line.  No GPU."""
from __future__ import annotations

import os
import re
import subprocess

import pytest
import torch

import block_train_bf16_reference as b16
import embed_train_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_the_hand_backward_is_autograd_and_rounds_dx_in_dw_alone():
    g = torch.Generator().manual_seed(5)
    n = 2
    p = torch.randn(n * 1024, 192, generator=g).to(torch.bfloat16).double()
    P = {"pe_w": torch.randn(1024, 192, generator=g) * 0.05, "pe_b": torch.randn(1024, generator=g), "pos": torch.randn(1024, 1024, generator=g)}
    dx = (torch.randn(n * 1024, 1024, generator=g) * torch.logspace(-3, 0, 1024)[None]).double()
    for net in (None, torch.bfloat16):
        R = {k: v.clone().requires_grad_(True) for k, v in er.rounded(P, torch.float64, net).items()}
        x = er.embed(R, p, net)
        assert x.shape == (n * 1024, 1024)
        if net is not None:
            assert torch.equal(x.detach(), x.detach().float().to(net).double()), "the rows are values of the network dtype"
        (x * dx).sum().backward()
        hand = er.embed_backward(p, dx)
        d = {k: _rel(hand[k], R[k].grad) for k in er.NAMES}
        print(f"net dtype {net}: hand backward against autograd (straight-through): {d}")
        assert max(d.values()) < 1e-12
    r = er.embed_backward(p, dx, b16.round_bf16)
    away = _rel(r["pe_w"], hand["pe_w"])
    print(f"dW with dx rounded to bf16 against the unrounded: {away:.3e}")
    assert 2.0 ** -13 < away < 2.0 ** -6 and torch.equal(r["pe_b"], hand["pe_b"]) and torch.equal(r["pos"], hand["pos"])
    assert torch.equal(hand["pos"], dx[:1024] + dx[1024:]), "dpos is the sum over the crops, token by token"


def test_embed_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    counts = {"cpx_blocks_backward_in": 15, "cpx_embed_grad_layout": 1, "cpx_embed_backward_workspace_bytes": 3, "cpx_embed_backward": 9,
              "cpx_blocks_backward_mp": 14}
    for name, n in counts.items():
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    from classpose_amd import ops
    L = _lib.lib()
    n, off = ops.embed_grad_layout()
    assert n == 1024 * 192 + 1024 + 1024 * 1024 and off == [0, 1024 * 192, 1024 * 192 + 1024]
    assert tuple(ops.EMBED_GRAD_SHAPES) == ((1024, 192), (1024,), (1024, 1024))
    f32, bf, f16 = _lib.DT_F32, _lib.DT_BF16, _lib.DT_F16
    q = L.cpx_embed_backward_workspace_bytes
    # float32 mode: independent of the batch; bf16 mode: 768 KiB per split, S = 8 min(nS, 4)
    assert q(1, bf, f32) == q(32, bf, f32) == q(3, f16, f32) == q(3, f32, f32) > 0
    per = 1024 * 192 * 4
    assert [(q(k, bf, bf) - q(1, bf, bf)) // per for k in (1, 2, 3, 4, 5, 8, 32)] == [0, 8, 16, 24, 24, 24, 24]
    for a in ((0, bf, f32), (-1, bf, bf), (1 << 21, bf, f32), (1, f16, bf), (1, f32, bf), (1, 9, f32), (1, bf, f16)):
        assert q(*a) == 0, a
    # the workspace of the blocks' backward is what it was
    assert L.cpx_blocks_backward_workspace_bytes_mp(3, bf, bf, bf) == L.cpx_blocks_backward_workspace_bytes_ex(3, bf, bf) > 0


def _args(*extra, **kw):
    from classpose_amd.entrypoints import train_head
    a = train_head.build_parser().parse_args(["--images", "i.npy", "--labels", "l.npy", "--pretrained_model", kw.pop("model", "m.pt"), "--save_path",
                                              "s", "--model_name", "n", *extra])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_cli_refuses_train_embed_without_every_block(tmp_path):
    """check_args runs before anything touches the device; the checkpoint's depth is read from its keys"""
    from classpose_amd import synth
    from classpose_amd.entrypoints import train_head
    assert _args().train_embed is False and "--train_embed" in train_head.build_parser().format_help()
    with pytest.raises(SystemExit, match=r"--train_embed needs --train_blocks equal to the checkpoint's depth.*only through every block"):
        train_head.check_args(_args("--train_embed"))
    ck = tmp_path / "depth2.pt"
    torch.save(synth.make_state_dict(3, None, depth=2, seed=1), ck)
    assert train_head.checkpoint_depth(str(ck)) == 2 and train_head.checkpoint_depth(str(tmp_path / "missing.pt")) is None
    with pytest.raises(SystemExit, match=r"--train_embed needs --train_blocks 2, the checkpoint's depth, not --train_blocks 1.*only through every block"):
        train_head.check_args(_args("--train_embed", "--train_blocks", "1", model=str(ck)))
    with pytest.raises(SystemExit, match=r"--train_embed: .*UNet class head"):
        train_head.check_args(_args("--train_embed", "--train_blocks", "2", "--feature_transformation_structure", "16", "24", model=str(ck)))
    ok = _args("--train_embed", "--train_blocks", "2", "--grad_precision", "bf16", model=str(ck))
    train_head.check_args(ok)
    assert ok.train_embed and ok.train_blocks == 2 and ok.train_neck and ok.grad_precision == "bf16" and ok.attn_grad_precision == "fp32"
    off = _args("--train_blocks", "2", model=str(ck))
    train_head.check_args(off)
    assert off.train_embed is False


def test_freeze_none_still_exits_as_it_did():
    from classpose_amd.entrypoints import train_head
    with pytest.raises(SystemExit, match=r"--freeze none: training the backbone and training the neck is not built"):
        train_head.check_args(_args("--freeze", "none"))
    with pytest.raises(SystemExit, match=r"is not built"):
        train_head.check_args(_args("--freeze", "none", "--train_embed", "--train_blocks", "24"))
