"""The GrandQC op program without a GPU: QcNet.plan's flattening (BatchNorm folding, weight packing, concat slices,
ping-pong buffers) interpreted in float64 against the float64 oracle, the program's memory invariants, and the detection
power of the synthetic single-op programs that tests/test_gpu_qc_every_element.py runs on the device."""
import numpy as np
import pytest
import torch

import qc_reference as R
from classpose_amd import grandqc, synth
from classpose_amd.grandqc import NONE
from oracle import grandqc as og


def _patches(nB, H, W, seed=45):
    p = np.stack([synth.render_region(seed, 700 * i, 33 * i, W, H) for i in range(nB)])
    p[0, : H // 2, : W // 3] = 245                            # a flat background region
    return p


def _oracle(sd, patches, dtype):
    with torch.no_grad():
        x = torch.cat([og.preprocess(p) for p in patches]).to(dtype)
        sdd = {k: (v.to(dtype) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in sd.items()}
        return og.forward(sdd, x).permute(0, 2, 3, 1).numpy().astype(np.float64)


@pytest.mark.parametrize("n_classes", [2, 8])
def test_interpreted_program_equals_float64_oracle(n_classes):
    """The program planned on the CPU and interpreted in float64 (activations never rounded) differs from the float64
    oracle only by the folded weights having been rounded to float32.  Rounding the weights alone must not cost more
    than rounding everything, so the rel-L2 limit is 4x the measured distance between the float32 and the float64
    oracle on the same inputs (measured: 5.4e-7 for 2 classes, 5.6e-7 for 8; the interpreted program is at 5.7e-8 and
    6.7e-8).  Class maps identical wherever the float64 top-2 margin exceeds 1e-3, > 99 % of the pixels."""
    nB, H, W = 2, 64, 96
    sd = synth.make_grandqc_state_dict(n_classes, 5)
    patches = _patches(nB, H, W)
    net = grandqc.QcNet(sd, "cpu")
    pl = net.plan(nB, H, W)
    assert len(pl["names"]) == pl["n_ops"]
    ws = R.interpret(list(pl["ops"]), nB, patches, pl["input_off"], pl["ws_bytes"] // 4, R.net_weights(net))
    got = R.Region(pl["logits_off"] // 4, nB * H * W, pl["ld_logits"], n_classes).view(ws).reshape(nB, H, W, n_classes)
    r64, r32 = _oracle(sd, patches, torch.float64), _oracle(sd, patches, torch.float32)
    d_oracle = np.linalg.norm(r32 - r64) / np.linalg.norm(r64)
    d_prog = np.linalg.norm(got - r64) / np.linalg.norm(r64)
    print(f"n_classes {n_classes}: oracle f32 vs f64 rel-L2 {d_oracle:.3e}, interpreted program vs f64 {d_prog:.3e}")
    assert np.isfinite(got).all()
    assert 1e-8 < d_oracle < 1e-5, d_oracle                   # the yardstick itself is float32 rounding, nothing else
    assert d_prog <= 4 * d_oracle, (d_prog, d_oracle)
    srt = np.sort(r64, -1)
    decided = (srt[..., -1] - srt[..., -2]) > 1e-3
    assert decided.mean() > 0.99
    assert np.array_equal(got.argmax(-1)[decided], r64.argmax(-1)[decided])


def test_packing_functions_are_what_qcnet_uploads():
    """the lifted module-level packers produce the bytes QcNet keeps behind its ops' pointers"""
    sd = synth.make_grandqc_state_dict(2, 7)
    net = grandqc.QcNet(sd, "cpu")
    pl = net.plan(1, 32, 32)
    names, ops = pl["names"], pl["ops"]
    i = names.index("decoder.blocks.x_1_2.conv1.0.weight")      # c_a = 40, c_b = 48: both sources padded
    o = ops[i]
    assert (o.c_a, o.c_b) == (40, 48)
    s64 = net._sd
    scale, shift = net._bn_fold("decoder.blocks.x_1_2.conv1.1", 24)
    w, b = grandqc.pack_dense_weights(s64[names[i]], scale, shift, 40, 48)
    assert w.shape == (32, 9, 48 + 48) and torch.equal(w.to(torch.float32), net.weight_tensor(o.w))
    assert torch.equal(b.to(torch.float32), net.weight_tensor(o.bias))
    # the pad lanes are zero, the real lanes are the folded weights in [cout][tap][cin] order
    ref = (s64[names[i]] * scale[:, None, None, None]).permute(0, 2, 3, 1).reshape(24, 9, 88)
    assert torch.equal(w[:24, :, :40], ref[:, :, :40]) and torch.equal(w[:24, :, 48:96], ref[:, :, 40:])
    assert not w[:, :, 40:48].any() and not w[24:].any()
    j = names.index("encoder.blocks.2.0.conv_dw.weight")
    scale, shift = net._bn_fold("encoder.blocks.2.0.bn2", 144)
    wd, bd = grandqc.pack_dw_weights(s64[names[j]], scale, shift)
    assert wd.shape == (25, 144) and torch.equal(wd.to(torch.float32), net.weight_tensor(ops[j].w))
    assert torch.equal(bd.to(torch.float32), net.weight_tensor(ops[j].bias))
    with pytest.raises(KeyError):
        net.weight_tensor(12345)


def _disjoint(a: R.Region, b: R.Region) -> bool:
    """byte ranges apart, or two channel slices of rows of one pitch whose column ranges are apart"""
    if a.end() <= b.off or b.end() <= a.off:
        return True
    if a.ld != b.ld:
        return False
    if a.off > b.off:
        a, b = b, a
    d = (b.off - a.off) % a.ld                               # b's first column relative to a's
    return d >= a.c and d + b.c <= a.ld


@pytest.mark.parametrize("nB,H,W", [(1, 32, 32), (3, 64, 96), (1, 512, 512)])
def test_program_invariants(nB, H, W):
    sd = synth.make_grandqc_state_dict(2, 3)
    net = grandqc.QcNet(sd, "cpu")
    pl = net.plan(nB, H, W)
    ops, names, ws_bytes = list(pl["ops"]), pl["names"], pl["ws_bytes"]
    n_floats = ws_bytes // 4
    inp = R.Region(pl["input_off"] // 4, nB * H * W, 4, 4)
    logits = R.Region(pl["logits_off"] // 4, nB * H * W, pl["ld_logits"], 2)
    assert pl["input_off"] % 16 == 0 and pl["logits_off"] % 16 == 0
    assert inp.end() <= n_floats and logits.off + nB * H * W * pl["ld_logits"] <= n_floats
    writer = np.full(n_floats, -2, np.int16)                # -2: never written, -1: k_qc_pre, i: op i
    inp.mark(writer, -1)
    dst_of = {-1: inp}
    for i, o in enumerate(ops):
        what = f"op {i} ({R.KIND[o.kind]}, {names[i]})"
        regs = R.op_regions(o, nB)
        # inside the workspace, 16-byte offsets, float4-loaded pitches and channel counts
        for key in ("src_a", "src_b", "gate", "res", "dst"):
            off = getattr(o, key)
            assert off == NONE or off % 16 == 0, (what, key, off)
        for key, r in regs.items():
            assert r.rows > 0 and 0 < r.c <= r.ld and r.end() <= n_floats, (what, key, r, n_floats)
        assert o.c_a % 4 == 0 and o.ld_a % 4 == 0 and o.c_b % 4 == 0 and o.ld_b % 4 == 0, what
        if o.kind != 0:
            assert o.ld_dst == o.c_a == o.c_out, what
        if o.kind == 2:
            assert regs["pool"].rows * regs["pool"].c == 16 * nB * o.c_a, what
        # the destination is apart from everything the op reads
        for key, r in regs.items():
            if key not in ("dst", "pool"):
                for d in R.written(o, nB):
                    assert _disjoint(d, r), (what, key, d, r)
        if o.kind == 2:
            assert _disjoint(regs["dst"], regs["pool"]), what
        # definition before use: every float an op reads still carries the stamp of a producer whose destination
        # tiles the region exactly (one producer for A, the gate and the residual; one per channel group for B)
        for key in ("a", "b", "gate", "res"):
            if key not in regs:
                continue
            r = regs[key]
            stamp = r.view(writer)
            assert (stamp >= -1).all(), (what, key, "reads floats nothing has written")
            assert (stamp == stamp[0]).all(), (what, key, "rows of one region come from different producers")
            producers = list(dict.fromkeys(int(s) for s in stamp[0]))
            assert key == "b" or len(producers) == 1, (what, key, producers)
            col = 0
            for p in producers:
                d = dst_of[p]
                assert (d.off, d.rows, d.ld) == (r.off + col, r.rows, r.ld), (what, key, p, d, r)
                col += d.c
            assert col == r.c, (what, key, producers)
        if o.kind == 0 and "gate" in regs:
            assert ops[int(regs["gate"].view(writer)[0, 0])].kind == 2, what
        for d in R.written(o, nB):
            d.mark(writer, i)
        dst_of[i] = regs["dst"]
    last = R.op_regions(ops[-1], nB)["dst"]
    assert (last.off, last.rows, last.ld, last.c) == (logits.off, logits.rows, logits.ld, logits.c)
    assert (inp.view(writer) == -1).all()                    # nothing overwrites the network's input


# ---- detection power of the synthetic programs -------------------------------------------------------
def _moves(cs, i, defect):
    """largest |defective - true| / tolerance over one op's elements"""
    good = R.run_op(cs.ws, cs.ops[i], cs.nB, cs.wts)
    bad = R.run_op(cs.ws, cs.ops[i], cs.nB, cs.wts, defect)
    assert np.isfinite(good["ref"]).all() and np.isfinite(good["tol"]).all(), cs.labels[i]
    return float((np.abs(bad["ref"] - good["ref"]) / good["tol"]).max())


@pytest.mark.parametrize("HW", sorted(R.SE_EXACT))
def test_detection_power_pool_slice_drops_its_last_pixel(HW):
    """integer-mean squeeze-excite tolerance: the last pixel of the last slice missing moves a gate by > 8 tolerances"""
    cs = R.case_se_exact("cpu", HW)
    assert R.run_op(cs.ws, cs.ops[0], cs.nB, cs.wts)["exact"]
    assert _moves(cs, 0, "pool_last_pixel") > 8


def test_detection_power_pool_slice_real_valued():
    cs = R.case_se_real("cpu")
    assert not R.run_op(cs.ws, cs.ops[0], cs.nB, cs.wts)["exact"]
    assert _moves(cs, 0, "pool_last_pixel") > 8


@pytest.mark.parametrize("stride", [1, 2])
def test_detection_power_depthwise_border_tap(stride):
    """depthwise tolerance: one border tap of a 5x5 window taken from inside the image instead of zero"""
    cs = R.case_depthwise("cpu", 5, stride)
    for i, o in enumerate(cs.ops):
        assert _moves(cs, i, "border_tap") > 8, cs.labels[i]


def test_detection_power_gate_of_image0_for_the_last_image():
    """dense tolerance with gate and residual"""
    cs = R.case_dense_gate_residual("cpu")
    for i in range(len(cs.ops)):
        assert _moves(cs, i, "gate_image0") > 8, cs.labels[i]


def test_detection_power_12_channel_tail_read_as_zero():
    """dense tolerance, every activation: the last four channels of a c_a % 16 == 12 source missing"""
    n = 0
    cases = [R.case_dense_sources("cpu", k, s) for k in (1, 3) for s in (1, 2)]
    for cs in cases + [R.case_dense_upsample("cpu"), R.case_dense_gate_residual("cpu")]:
        for i, o in enumerate(cs.ops):
            if o.c_a % 16 == 12:
                assert _moves(cs, i, "tail12_zero") > 8, cs.labels[i]
                n += 1
    assert n >= 16


def test_detection_power_source_b_weights_four_lanes_early():
    """dense tolerance with two sources: B's weights read from pad16(c_a) - 4"""
    cs = R.case_dense_upsample("cpu")
    n = 0
    for i, o in enumerate(cs.ops):
        if o.src_b != NONE:
            assert _moves(cs, i, "b_offset") > 8, cs.labels[i]
            n += 1
    assert n == 3


def test_detection_power_silu_and_tiles():
    """the linear / ReLU / SiLU tolerances of the tile and activation cases, with the plainest defect: the last four
    channels of their 24-channel source (its 8-channel tail) read as zero"""
    for cs in [R.case_dense_acts("cpu")] + [R.case_dense_tiles("cpu", P) for P in R.TILE_P]:
        for i, o in enumerate(cs.ops):
            good = R.run_op(cs.ws, o, cs.nB, cs.wts)
            a = R.op_regions(o, cs.nB)["a"]
            ws = cs.ws.copy()
            a.view(ws)[:, o.c_a - 4:] = 0.0
            bad = R.run_op(ws, o, cs.nB, cs.wts)
            assert (np.abs(bad["ref"] - good["ref"]) / good["tol"]).max() > 8, cs.labels[i]
    cs = R.case_dense_acts("cpu")
    v = R.run_op(cs.ws, cs.ops[2], cs.nB, cs.wts)["pre"]
    assert v.min() < -11 and v.max() > 11                    # SiLU sees about [-12, 12]


def test_interpreter_matches_torch_conv_on_synthetic_ops():
    """the interpreter's own convolution against F.conv2d in float64 (odd sizes, stride 2, two sources, upsampling)"""
    import torch.nn.functional as F
    cs = R.case_dense_upsample("cpu")
    o = cs.ops[1]                                              # c_a = 28, c_b = 24, up_a, 3x3, ReLU
    regs = R.op_regions(o, cs.nB)
    a = torch.from_numpy(regs["a"].view(cs.ws).astype(np.float64).reshape(cs.nB, 3, 2, 28)).permute(0, 3, 1, 2)
    b = torch.from_numpy(regs["b"].view(cs.ws).astype(np.float64).reshape(cs.nB, 6, 4, 24)).permute(0, 3, 1, 2)
    x = torch.cat([F.interpolate(a, scale_factor=2, mode="nearest"), b], 1)
    wp = torch.from_numpy(cs.wts(o.w).astype(np.float64)).reshape(64, 9, 32 + 32)
    w = torch.cat([wp[:40, :, :28], wp[:40, :, 32:56]], -1).reshape(40, 3, 3, 52).permute(0, 3, 1, 2)
    bias = torch.from_numpy(cs.wts(o.bias).astype(np.float64))[:40]
    want = F.relu(F.conv2d(x, w, bias, padding=1)).permute(0, 2, 3, 1).reshape(-1, 40).numpy()
    got = R.run_op(cs.ws, o, cs.nB, cs.wts)
    assert np.abs(got["ref"] - want).max() < 1e-12
    cs = R.case_depthwise("cpu", 5, 2)
    i = [j for j, o in enumerate(cs.ops) if (o.h_in, o.w_in, o.c_a, o.ld_a) == (9, 13, 32, 40)][0]
    o = cs.ops[i]
    x = torch.from_numpy(R.op_regions(o, 3)["a"].view(cs.ws).astype(np.float64).reshape(3, 9, 13, 32)).permute(0, 3, 1, 2)
    w = torch.from_numpy(cs.wts(o.w).astype(np.float64)).reshape(5, 5, 32).permute(2, 0, 1)[:, None]
    v = F.conv2d(x, w, torch.from_numpy(cs.wts(o.bias).astype(np.float64)), stride=2, padding=2, groups=32)
    want = (v * torch.sigmoid(v)).permute(0, 2, 3, 1).reshape(-1, 32).numpy()
    assert np.abs(R.run_op(cs.ws, o, 3, cs.wts)["ref"] - want).max() < 1e-12
