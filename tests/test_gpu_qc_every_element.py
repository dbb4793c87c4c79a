"""The GrandQC network's kernels (csrc/cpx_qc.hip: k_qc_pre, k_qc_conv<32|64>, k_qc_dw, k_qc_pool, k_qc_se, k_qc_argmax)
op by op, every element, against the float64 interpreter of tests/qc_reference.py.

The harness calls cpx_qc_forward with ONE op at a time on a persistent workspace (each call re-runs k_qc_pre and the
argmax, both harmless) and holds three things for every call:
 1. the op's destination equals the interpreter run on the DEVICE's own inputs of that op (the workspace before the
    call), element by element -- errors do not accumulate across ops;
 2. every float of the workspace outside the destination slice (for squeeze-excite: the pool scratch and the gate row too)
    is bit-identical before and after; only the input region, which the call's own k_qc_pre rewrites, is exempt and
    must hold the bits of the reference preprocessing;
 3. a second call gives the same bits.

Tolerances are derived, not tuned (u = 2^-24, K products per element, S = the operation on absolute values); the
derivations are in the docstring of tests/qc_reference.py and in DESIGN.md 6b:
 dense / depthwise pre-activation (K + 3) u S + 1e-30; ReLU adds nothing; SiLU 1.1 e_pre + (2 |v| + 8) u |silu(v)|;
 residual + u (|res| + |value|); squeeze-excite the same constants through mean (integer inputs: two roundings), reduce,
 SiLU, expand and sigmoid (e_s / 4 + (2 |s| + 8) u sigmoid(s)).  The SiLU / sigmoid terms rest on __expf being the
 hardware exp2 of fl(log2e x) with 1 ulp for the instruction (the ISA manual's figure for V_EXP_F32).
That such tolerances still expose a subtly wrong kernel on these inputs is shown without a GPU by
tests/test_qc_program_host.py::test_detection_power_*."""
import ctypes as C

import numpy as np
import pytest
import torch

import qc_reference as R
from classpose_amd import _lib, grandqc, synth
from classpose_amd._lib import CpxQcOp, ptr
from classpose_amd.grandqc import NONE
from oracle import grandqc as og

pytestmark = pytest.mark.gpu


class Harness:
    """one workspace on the device + its host mirror; ``step`` runs one op under the three conditions"""

    def __init__(self, dev, ws_host, nB, H, W, patches, input_off, logits_off, n_classes, ld_logits, wts):
        self.dev, self.nB, self.H, self.W = dev, nB, H, W
        self.input_off, self.logits_off, self.n_classes, self.ld_logits = input_off, logits_off, n_classes, ld_logits
        self.wts = wts
        self.ws = torch.from_numpy(ws_host).to(dev)
        self.ws_bytes = ws_host.size * 4
        self.patches_host = patches
        self.patches = torch.from_numpy(patches).to(dev)
        self.cls = torch.full((nB, H, W), -1, dtype=torch.int8, device=dev)
        self.logits_out = torch.full((nB, H, W, n_classes), R.SENT, dtype=torch.float32, device=dev)
        self.inp = R.Region(input_off // 4, nB * H * W, 4, 4)
        self.before = ws_host.copy()
        self.inp.view(self.before)[...] = R.pre(patches).reshape(-1, 4)      # what the call's own k_qc_pre leaves there

    def call(self, op, nB=None, H=None, W=None, ws_bytes=None, n_classes=None, ld_logits=None) -> int:
        arr = (CpxQcOp * 1)(op)
        rc = _lib.lib().cpx_qc_forward(arr, 1, ptr(self.patches), self.nB if nB is None else nB,
                                       self.H if H is None else H, self.W if W is None else W, self.input_off,
                                       self.logits_off, self.n_classes if n_classes is None else n_classes,
                                       self.ld_logits if ld_logits is None else ld_logits, ptr(self.cls),
                                       ptr(self.logits_out), ptr(self.ws), self.ws_bytes if ws_bytes is None else ws_bytes,
                                       torch.cuda.current_stream(self.dev).cuda_stream)
        torch.cuda.synchronize(self.dev)
        return rc

    def step(self, op, what: str) -> dict:
        _lib.check(self.call(op), what)
        first = self.ws.clone()
        _lib.check(self.call(op), what)
        assert torch.equal(first.view(torch.int32), self.ws.view(torch.int32)), f"{what}: not bitwise repeatable"
        after = first.cpu().numpy()
        before = self.before
        out = R.run_op(before, op, self.nB, self.wts)
        regs = R.op_regions(op, self.nB)
        got = regs["dst"].view(after).astype(np.float64)
        ref, tol = out["ref"], out["tol"]
        assert np.isfinite(ref).all() and np.isfinite(tol).all(), f"{what}: the reference itself is not finite"
        err = np.abs(got - ref)
        bad = ~(err <= tol)                                    # NaN on the device counts as wrong
        if bad.any():
            ratio = np.where(np.isfinite(err), err / tol, np.inf)
            r, c = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements out of tolerance; worst at row {r} "
                                 f"channel {c}: got {got[r, c]!r}, reference {ref[r, c]!r}, |diff| {err[r, c]:.3e}, "
                                 f"tolerance {tol[r, c]:.3e}")
        if op.kind == 2 and out["exact"]:                      # integer inputs: every partial sum is exact
            n = out["pool_rows"]
            pool = regs["pool"].view(after)
            assert np.array_equal(pool[:n].astype(np.float64), out["pool"][:n]), f"{what}: pool partial sums"
            assert np.array_equal(pool[n:].view(np.int32), regs["pool"].view(before)[n:].view(np.int32)), \
                f"{what}: pool rows beyond the slices in use were written"
        allowed = np.zeros(after.size, bool)
        for d in R.written(op, self.nB):
            d.mark(allowed)
        stray = (before.view(np.int32) != after.view(np.int32)) & ~allowed
        if stray.any():
            idx = np.flatnonzero(stray)
            raise AssertionError(f"{what}: {idx.size} floats outside the destination changed, first at float {idx[0]} "
                                 f"({before[idx[0]]!r} -> {after[idx[0]]!r}); destination {regs['dst']}")
        self.before = after
        return dict(worst=float((err / tol).max()), n=err.size)


def _run_case(cs, dev):
    h = Harness(dev, cs.ws, cs.nB, cs.H, cs.W, cs.patches, cs.input_off, cs.logits_off, cs.n_classes, cs.ld_logits, cs.wts)
    worst = 0.0
    for op, label in zip(cs.ops, cs.labels):
        worst = max(worst, h.step(op, label)["worst"])
    print(f"{len(cs.ops)} ops, worst |diff| / tolerance {worst:.3f}")
    return h


# ---- walk of the production program ---------------------------------------------------------------
@pytest.mark.parametrize("n_classes,nB,H,W,seed", [(2, 3, 64, 96, 3), (8, 2, 96, 64, 4)])
def test_walk_of_the_production_program(cuda, n_classes, nB, H, W, seed):
    """every op of QcNet.plan in order, one call each, on a workspace that starts as NaN everywhere (a read before the
    definition shows as NaN); after the last op the class map is np.argmax of the device logits bit for bit"""
    sd = synth.make_grandqc_state_dict(n_classes, seed)
    patches = np.stack([synth.render_region(40 + seed, 700 * i, 33 * i, W, H) for i in range(nB)])
    patches[0, : H // 2, : W // 3] = 245                       # a flat background region
    net = grandqc.QcNet.from_state_dict(sd, cuda)
    pl = net.plan(nB, H, W)
    ws = np.full(pl["ws_bytes"] // 4, np.nan, np.float32)
    h = Harness(cuda, ws, nB, H, W, patches, pl["input_off"], pl["logits_off"], n_classes, pl["ld_logits"],
                R.net_weights(net))
    worst = (0.0, "")
    for i, (op, name) in enumerate(zip(pl["ops"], pl["names"])):
        res = h.step(op, f"op {i} ({R.KIND[op.kind]}, {name})")
        worst = max(worst, (res["worst"], f"op {i} {name}"))
    print(f"{pl['n_ops']} ops, worst |diff| / tolerance {worst[0]:.3f} at {worst[1]}")
    after = h.before
    lg = R.Region(pl["logits_off"] // 4, nB * H * W, pl["ld_logits"], n_classes).view(after)
    out = h.logits_out.cpu().numpy().reshape(-1, n_classes)
    assert np.array_equal(out.view(np.int32), np.ascontiguousarray(lg).view(np.int32))
    assert np.array_equal(h.cls.cpu().numpy().ravel(), np.argmax(out, -1).astype(np.int8))
    # and the walk ends where the one-call forward ends
    cls, logits = net.forward(torch.from_numpy(patches).to(cuda), return_logits=True)
    assert torch.equal(logits.view(torch.int32).cpu(), h.logits_out.view(torch.int32).cpu())
    assert torch.equal(cls, h.cls)


# ---- synthetic single-op programs -----------------------------------------------------------------
@pytest.mark.parametrize("P", sorted(R.TILE_P))
def test_dense_tiles(cuda, P):
    """P = nB h_out w_out: 35 (partial first tile), 105 (three images in one 128-pixel workgroup), 128, 351 (tail in the
    third tile) x c_out 2 / 8 / 24 / 32 (32-wide tile) and 40 / 64 / 80 / 112 (64-wide tile, partial second column tile);
    the destination is the slice [4, 4 + c_out) of rows of c_out + 8 sentinels"""
    _run_case(R.case_dense_tiles(cuda, P), cuda)


@pytest.mark.parametrize("k,stride", [(1, 1), (1, 2), (3, 1), (3, 2)])
def test_dense_sources(cuda, k, stride):
    """c_a 4, 12, 16, 24, 28, 40 and 136 (nine K chunks) as the slice [4, 4 + c_a) of rows of c_a + 8 floats with NaN
    around it; inputs of 2x3 and 9x13"""
    _run_case(R.case_dense_sources(cuda, k, stride), cuda)


def test_dense_upsample_and_source_b(cuda):
    """nearest x2 upsampling of A, alone and with a source B (c_b 24 / 48) that ends its rows as the concat buffers do"""
    _run_case(R.case_dense_upsample(cuda), cuda)


def test_dense_gate_and_residual(cuda):
    """per-image gate and residual (ld_res != ld_dst), three images"""
    _run_case(R.case_dense_gate_residual(cuda), cuda)


def test_dense_activations(cuda):
    """none, ReLU, SiLU with pre-activations over about [-12, 12]"""
    _run_case(R.case_dense_acts(cuda), cuda)


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_depthwise(cuda, k, stride):
    """C 4 / 32 / 144 x inputs 2x3, 1x1 (window larger than the image), 9x13 x ld_a = C and C + 8, three images"""
    _run_case(R.case_depthwise(cuda, k, stride), cuda)


@pytest.mark.parametrize("HW", sorted(R.SE_EXACT))
def test_squeeze_excite_exact_means(cuda, HW):
    """integer inputs (|x| <= 8): every float32 partial sum is exact in any order, so the pool scratch is compared
    exactly and the mean carries two roundings; HW 35 / 1023 (one slice), 1024 / 1085 (four, short last slice),
    16384 / 16512 (sixteen, short last slice)"""
    _run_case(R.case_se_exact(cuda, HW), cuda)


def test_squeeze_excite_real_valued(cuda):
    _run_case(R.case_se_real(cuda), cuda)


def test_pre_every_level(cuda):
    """all 256 levels in every channel: bit-equal to oracle.grandqc.preprocess, fourth channel exactly +0"""
    cs = R.Case(cuda, 1, 900)
    i = np.arange(1024)
    cs.patches = np.stack([(i * 1) % 256, (i * 3 + 7) % 256, (i * 5 + 14) % 256], -1).astype(np.uint8).reshape(1, 32, 32, 3)
    assert all(len(np.unique(cs.patches[..., c])) == 256 for c in range(3))
    R.add_dense(cs, 2, 3, 4, 2)
    cs.finish()
    h = _run_case(cs, cuda)
    got = cs.input.view(h.before).reshape(32, 32, 4)
    want = og.preprocess(cs.patches[0])[0].permute(1, 2, 0).numpy()
    assert np.array_equal(got[..., :3].view(np.int32), np.ascontiguousarray(want).view(np.int32))
    assert not got[..., 3].view(np.int32).any()


@pytest.mark.parametrize("n_classes", [2, 5, 8])
def test_argmax_ties_and_padded_lanes(cuda, n_classes):
    """first maximum wins (exact ties between class 0 / a middle class and a later class), all-negative rows, padded
    lanes at +1e30 never win and never reach logits_out"""
    cs = R.Case(cuda, 2, 950 + n_classes, n_classes)
    R.add_dense(cs, 2, 3, 4, 2)
    cs.finish()
    ld, npix = cs.ld_logits, 2 * 1024
    lg = np.full((npix, ld), 1e30, np.float32)
    vals = cs.rng.integers(-3, 4, (npix, n_classes)).astype(np.float32)        # few levels: ties everywhere
    vals[0::4] -= 10.0                                                         # all-negative rows
    vals[1::8, 0] = 5.0
    vals[1::8, n_classes - 1] = 5.0                                            # first and last class tie at the maximum
    vals[2::8, n_classes // 2] = 6.0
    vals[2::8, n_classes - 1] = 6.0
    vals[3, :] = -0.0
    vals[7, :] = 0.0
    lg[:, :n_classes] = vals
    cs.logits.view(cs.ws)[...] = lg
    h = _run_case(cs, cuda)
    want = np.argmax(vals, -1).astype(np.int8)
    assert want[1] == 0 and (n_classes == 2 or want[2] == n_classes // 2)
    assert np.array_equal(want, R.argmax(cs.ws, cs.logits_off, npix, ld, n_classes))
    assert np.array_equal(h.cls.cpu().numpy().ravel(), want)
    assert np.array_equal(h.logits_out.cpu().numpy().reshape(npix, n_classes).view(np.int32), vals.view(np.int32))


# ---- contract rejections -------------------------------------------------------------------------
def _clone(op, **kw):
    o = CpxQcOp.from_buffer_copy(op)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_contract_rejections(cuda):
    """inputs the kernels would mishandle come back as a status with a message and leave the workspace alone"""
    cs = R.Case(cuda, 2, 990)
    R.add_dense(cs, 6, 4, 12, 24, k=3, up=1, c_b=24, gate=True, res=True)
    R.add_depthwise(cs, 5, 7, 32, 3, 1)
    R.add_se(cs, 5, 7, 32, 4)
    cs.finish()
    h = _run_case(cs, cuda)
    dense, dw, se = cs.ops
    end = cs.ws_bytes
    bad = {
        "H % 32": (dense, dict(H=48)),
        "c_a % 4": (_clone(dense, c_a=10), {}),
        "unknown kind": (_clone(dense, kind=3), {}),
        "destination past the workspace": (_clone(dense, dst=end - 64), {}),
        "destination past a smaller workspace": (dense, dict(ws_bytes=dense.dst + 64)),
        "depthwise ld_dst != c_a": (_clone(dw, ld_dst=40), {}),
        "squeeze-excite ld_dst != c_a": (_clone(se, ld_dst=40), {}),
        # found by reading the code: source extents and alignments were never checked
        "source A past the workspace": (_clone(dense, src_a=end - 64), {}),
        "source A misaligned": (_clone(dense, src_a=dense.src_a + 4), {}),
        "source A pitch below its channels": (_clone(dense, ld_a=8), {}),
        "source B past the workspace": (_clone(dense, src_b=end - 64), {}),
        "gate past the workspace": (_clone(dense, gate=end - 16), {}),
        "residual past the workspace": (_clone(dense, res=end - 64), {}),
        "depthwise source past the workspace": (_clone(dw, src_a=end - 64), {}),
        "depthwise destination past the workspace": (_clone(dw, dst=end - 64), {}),
        "squeeze-excite source past the workspace": (_clone(se, src_a=end - 64), {}),
        "squeeze-excite gate past the workspace": (_clone(se, dst=end - 64), {}),
        "squeeze-excite scratch past the workspace": (_clone(se, res=end - 64), {}),
        "more classes than logits lanes": (dense, dict(n_classes=5, ld_logits=4)),
    }
    L = _lib.lib()
    snap = h.ws.clone()
    for what, (op, kw) in bad.items():
        rc = h.call(op, **kw)
        msg = L.cpx_last_error()
        assert rc != 0, what
        assert msg and b"invalid argument" in msg, (what, msg)
        assert torch.equal(snap.view(torch.int32), h.ws.view(torch.int32)), what
    _lib.check(h.call(dense), "the valid op still runs")
    assert torch.equal(snap.view(torch.int32), h.ws.view(torch.int32))
