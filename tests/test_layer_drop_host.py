"""Host checks of layer drop for the trained blocks: the restatement tests/layer_drop_reference.py against the reference's own
expression in float64, the drop probabilities and the mask draw, the refusals of the trainer and the command line, and the C ABI's
additive entries.  No GPU."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest
import torch

import block_train_reference as br
import layer_drop_reference as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(a, b):
    return float((a - b).norm() / b.norm())


def test_kept_crops_only_is_the_reference_expression_in_float64():
    """2 blocks, 3 crops; crop 1 is dropped in both blocks and block 1 keeps nothing at all in the second mask.  Values, every parameter
    gradient and dx of "the block on the kept crops, the others left alone" against x * mask + blk(x) * (1 - mask) with blk on all
    crops: 1e-12 relative (float64; the two differ by the order of the blend's additions alone)."""
    from classpose_amd import synth
    sd = synth.make_state_dict(3, None, depth=2, seed=81)
    PB = [br.params_from_state_dict(sd, j) for j in range(2)]
    g = torch.Generator().manual_seed(82)
    n = 3
    x = torch.randn(n * 1024, 1024, generator=g, dtype=torch.float64)
    dout = torch.randn(n * 1024, 1024, generator=g, dtype=torch.float64)
    for keep in ([[1, 0, 1], [0, 0, 1]], [[1, 0, 1], [0, 0, 0]]):
        res = []
        for fn in (lr.blocks_forward, lr.reference_expression):
            RB = [{k: v.clone().requires_grad_(True) for k, v in br.rounded(P, torch.float64, None).items()} for P in PB]
            xx = x.clone().requires_grad_(True)
            out = fn(RB, xx, keep)
            (out * dout).sum().backward()
            res.append((out.detach(), xx.grad, [{k: (R[k].grad if R[k].grad is not None else torch.zeros_like(R[k])) for k in R} for R in RB]))
        (o_a, dx_a, g_a), (o_b, dx_b, g_b) = res
        worst = max(_rel(o_a, o_b), _rel(dx_a, dx_b))
        for j in range(2):
            for k in br.NAMES:
                if float(g_b[j][k].norm()) == 0:
                    assert float(g_a[j][k].norm()) == 0, (j, k)
                else:
                    worst = max(worst, _rel(g_a[j][k], g_b[j][k]))
        dropped_same = torch.equal(o_a.view(n, -1)[1], x.view(n, -1)[1]) and torch.equal(dx_a.view(n, -1)[1], dout.view(n, -1)[1])
        empty = [j for j in range(2) if not any(keep[j])]
        zero = all(float(g_a[j][k].abs().max()) == 0 for j in empty for k in br.NAMES)
        print(f"keep {keep}: worst relative difference {worst:.3e}; the crop dropped twice passes x and dout through bitwise {dropped_same}; "
              f"blocks {empty} keep nothing and have zero gradients {zero}")
        assert worst < 1e-12 and dropped_same and zero
        assert float(g_a[0]["qkv_w"].norm()) > 0


def test_drop_probabilities_are_the_reference_linspace():
    from classpose_amd.train import layer_drop_probs
    p = layer_drop_probs(24, 0.4)
    want = torch.linspace(0, 0.4, 24, dtype=torch.float64).numpy()
    assert p.dtype == np.float64 and p.shape == (24,) and p[0] == 0.0 and p[-1] == 0.4
    assert np.abs(p - want).max() <= 2.0 ** -52 and np.all(np.diff(p) > 0)
    assert np.array_equal(layer_drop_probs(1, 0.4), [0.0]) and not layer_drop_probs(5, 0.0).any()
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="layer_drop"):
            layer_drop_probs(24, bad)


class _Stub:
    """a generator whose every draw is the table it was given"""

    def __init__(self, table):
        self.table, self.calls = np.asarray(table, dtype=np.float64), 0

    def random(self, shape):
        self.calls += 1
        return np.broadcast_to(self.table, shape).copy()


SEED = 1            # chosen on the CPU: its 4 000 draws put every block within 1.7 binomial standard deviations of its mean


def test_draw_keep_mask():
    from classpose_amd.train import draw_keep_mask, layer_drop_probs
    rng = np.random.default_rng(7)
    before = rng.bit_generator.state
    assert draw_keep_mask(rng, 8, 24, 24, 0.0) is None and rng.bit_generator.state == before, "rate 0 draws nothing"
    m = draw_keep_mask(rng, 8, 24, 24, 0.4)
    assert m.dtype == np.uint8 and m.shape == (24, 8) and m.flags.c_contiguous and set(np.unique(m)) <= {0, 1}
    assert rng.bit_generator.state != before
    p = layer_drop_probs(24, 0.4)
    # the comparison is strict: a draw equal to the probability keeps
    for K in (24, 4, 1):
        st = _Stub(p[24 - K:])
        assert draw_keep_mask(st, 5, 24, K, 0.4).all() and st.calls == 1
    # K < depth takes the LAST K probabilities: draws just below p[20:] drop everything (against p[:4] they would keep everything)
    below = np.nextafter(p[20:], 0)
    assert not draw_keep_mask(_Stub(below), 3, 24, 4, 0.4).any()
    assert not draw_keep_mask(_Stub(p[:4]), 3, 24, 4, 0.4).any(), "draws equal to the FIRST four probabilities lie below the last four"
    # block 0 of a fully trained network is never dropped (probability 0, strict <), not even by a draw of exactly 0
    assert draw_keep_mask(_Stub(np.zeros(24)), 3, 24, 24, 0.4)[0].all()
    n = 4000
    m = draw_keep_mask(np.random.default_rng(SEED), n, 24, 24, 0.4)
    drops = n - m.sum(axis=1)
    sigma = np.sqrt(n * p * (1 - p))
    z = np.abs(drops - n * p) / np.maximum(sigma, 1e-300)
    print(f"seed {SEED}, {n} crops: drops per block {drops.tolist()}; worst deviation {z[1:].max():.2f} sigma; share dropped {1 - m.mean():.4f}")
    assert drops[0] == 0 and z[1:].max() <= 5.0
    for bad in ((8, 24, 0, 0.4), (8, 24, 25, 0.4), (8, 24, 4, 1.0)):
        with pytest.raises(ValueError):
            draw_keep_mask(rng, *bad)


def test_trainer_refuses_before_it_touches_a_device():
    from classpose_amd.train import HeadTrainer, check_layer_drop
    for rate in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"layer_drop: a rate in \[0, 1\)"):
            HeadTrainer({}, device="cpu", train_blocks=2, layer_drop=rate)
    with pytest.raises(ValueError, match="layer_drop .* needs train_blocks > 0"):
        HeadTrainer({}, device="cpu", layer_drop=0.4)
    with pytest.raises(ValueError, match="needs train_blocks"):
        HeadTrainer({}, device="cpu", train_neck=True, layer_drop=0.4)
    check_layer_drop(0.0, 0)
    check_layer_drop(0.4, 1)


def _args(*extra, **kw):
    from classpose_amd.entrypoints import train_head
    a = train_head.build_parser().parse_args(["--images", "i.npy", "--labels", "l.npy", "--pretrained_model", kw.pop("model", "m.pt"), "--save_path",
                                              "s", "--model_name", "n", *extra])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_cli_refuses_layer_drop_without_trained_blocks():
    from classpose_amd.entrypoints import train_head
    assert _args().layer_drop == 0.0
    hlp = train_head.build_parser().format_help()
    assert "--layer_drop" in hlp and "0.4" in hlp[hlp.index("--layer_drop"):]
    with pytest.raises(SystemExit, match=r"--layer_drop goes with --train_blocks K"):
        train_head.check_args(_args("--layer_drop", "0.4"))
    with pytest.raises(SystemExit, match=r"--layer_drop goes with --train_blocks K"):
        train_head.check_args(_args("--layer_drop", "0.4", "--train_neck"))
    for bad in ("1", "-0.2", "1.5"):
        with pytest.raises(SystemExit, match=r"--layer_drop: a rate in \[0, 1\)"):
            train_head.check_args(_args("--layer_drop", bad, "--train_blocks", "2"))
    ok = _args("--layer_drop", "0.4", "--train_blocks", "2")
    train_head.check_args(ok)
    assert ok.layer_drop == 0.4 and ok.train_blocks == 2 and ok.train_neck
    off = _args("--train_blocks", "2")
    train_head.check_args(off)
    assert off.layer_drop == 0.0


def test_layer_drop_entries_are_declared_bound_and_exported():
    from classpose_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    declared = set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr))
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    exported = set(re.findall(r" T (cpx_[a-z0-9_]+)", subprocess.check_output(["nm", "-D", _lib.LIB_PATH], text=True)))
    counts = {"cpx_gather_crops": 8, "cpx_scatter_crops": 7, "cpx_blocks_train_workspace_bytes_drop": 3, "cpx_blocks_forward_train_drop": 9,
              "cpx_blocks_backward_drop": 16, "cpx_blocks_forward_train": 8, "cpx_blocks_backward_in": 15}
    for name, n in counts.items():
        assert name in declared and name in _lib.SIGNATURES and name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == n, name
    L = _lib.lib()
    bf, f16, f32 = _lib.DT_BF16, _lib.DT_F16, _lib.DT_F32
    base, drop = L.cpx_blocks_train_workspace_bytes, L.cpx_blocks_train_workspace_bytes_drop
    # one staging tensor of the batch's rows behind the workspace as it was
    for nS, dt, K, es in ((3, bf, 2, 2), (5, f16, 1, 2), (2, f32, 2, 4), (32, bf, 24, 2)):
        assert drop(nS, dt, K) - base(nS, dt, K) == nS * 1024 * 1024 * es, (nS, dt, K)
    for a in ((0, bf, 2), (3, 9, 2), (3, bf, 0)):
        assert drop(*a) == 0 == base(*a), a
