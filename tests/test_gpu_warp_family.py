"""The pool warps are one family: include/classpose_hip.h documents each entry as bitwise the one before it when its new inputs
are off.  The links of that chain, and where each is held:

  quality (no HBS flag, no override) == stain          test_gpu_quality.py::test_quality_pool_kernel_equals_its_parts_bitwise
  stain, mode 0 == pool without jitter                 test_gpu_stain.py::test_fused_pool_kernel_equals_its_parts_bitwise
  stain, mode 1 == pool with applied = 1               the same test
  pool of equal-sized images == warp_affine (uint8)    test_gpu_train_pool.py::test_pool_warp_equals_warp_affine_bitwise
  flow targets, vec (1, 0, 0, 1) == warp_affine (f32)  nowhere before this file

Those tests draw their maps at random or put them well inside the source.  What they leave open, and this file adds: the last link,
and every link at the edges of the code the kernels share -- a source coordinate of exactly -1 and exactly the source's width (the
two ends of the inside test), a nearest pixel of exactly 0 and exactly the width (the ends of the label rule), a map of NaN, a map
that misses the source, an image index and a table entry outside the pool -- on one ragged pool whose byte offsets make the byte
sum take its head, its body, its tail and a count below one load.  One member of the chain is tied to the numpy restatements
(tests/augment_reference.py, tests/flow_train_reference.py); everything else is torch.equal against that member.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

import augment_reference as ar
import flow_train_reference as fr

SIZES = [(1, 1), (5, 7), (64, 65), (33, 130)]          # 3 * px_off = 0, 3, 108, 12588: with the odd guard every image starts unaligned
DH, DW = 16, 20                                        # 320 pixels: one full workgroup of 256 and a partial one
FILL = -100
WARP_ABS = 8 * 2.0 ** -24 * 255                        # the bound of test_gpu_train_pool.py: a few float32 roundings of values <= 255
NAN, MISS = 7, 3                                       # the crops whose maps are NaN / miss the source


def _maps():
    """(image_of, inv): ten crops, every image used, repeats, and the edges of the shared geometry."""
    c, s = np.cos(0.5) * 1.3, np.sin(0.5) * 1.3
    ox, oy = (DW - 1) / 2, (DH - 1) / 2
    turn = lambda cx, cy, c, s: [c, s, cx - (c * ox + s * oy), -s, c, cy - (-s * ox + c * oy)]       # noqa: E731
    rows = [
        (3, [1, 0, 0, 0, 1, 0]),                        # identity
        (2, [-1, 0, 64, 0, 1, 0]),                      # a flip of the 65 columns
        (1, turn(3.1, 2.2, c, s)),                      # a turn with scale about the 5 x 7 image: the source is left on all four sides
        (2, [1, 0, 500.0, 0, 1, 0]),                    # MISS: entirely outside
        (1, [1, 0, -1, 0, 1, -1]),                      # sx = -1 at x = 0 and sx = sw = 7 at x = 8; sy = -1 and sy = sh = 5 likewise
        (1, [1, 0, -0.5, 0, 1, -0.5]),                  # floor(sx + 0.5) = 0 at x = 0 and = sw at x = 7; rows likewise
        (0, [1, 0, -1, 0, 1, -1]),                      # the 1 x 1 image: sx = -1, 0 and 1 = sw
        (3, [np.nan] * 6),                              # NAN
        (3, turn(64.3, 16.4, np.cos(2.0) * 2.1, np.sin(2.0) * 2.1)),
        (2, [1, 0, 50.25, 0, 1, 55.75]),                # the lower right corner of the 64 x 65 image and beyond
    ]
    return np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.float64)


def test_the_restatements_hold_the_edges_on_the_cpu():
    """Before they serve as the reference: a map that misses the source gives zeros / the fill, the edge maps give what the rule says.
    A NaN map does NOT go through them (their weights become NaN where the kernels skip the pixel): that crop is asserted directly."""
    image_of, inv = _maps()
    rng = np.random.default_rng(0)
    src = rng.integers(1, 251, (3, 5, 7)).astype(np.float32)
    lab = rng.integers(1, 7, (5, 7)).astype(np.int16)
    assert not ar.warp_image(src, inv[MISS], DH, DW, np.float32).any() and (ar.warp_labels(lab, inv[MISS], DH, DW, FILL) == FILL).all()
    assert (ar.warp_labels(lab, inv[NAN], DH, DW, FILL) == FILL).all() and np.isnan(ar.warp_image(src, inv[NAN], DH, DW, np.float32)).all()
    edge = ar.warp_image(src, inv[4], DH, DW, np.float32)               # sx = x - 1: column 0 is the border, 1..7 the source, 8.. outside
    assert not edge[:, :, 0].any() and not edge[:, 0].any() and np.array_equal(edge[:, 1:6, 1:8], src) and not edge[:, :, 8:].any()
    near = ar.warp_labels(lab, inv[5], DH, DW, FILL)                    # floor(x - 0.5 + 0.5) = x: columns 0..6 the source, 7.. the fill
    assert np.array_equal(near[:5, :7], lab) and (near[:, 7:] == FILL).all() and (near[5:] == FILL).all()
    for t in (2, 8):                                                    # the turns stay away from the half-integers of the label rule
        assert ar.half_integer_distance(inv[t], DH, DW) > 1e-9, t


@pytest.fixture(scope="module")
def family(cuda):
    """The pool (uint8 images, labels, float32 target planes of the same shapes) and every member of the chain on the same crops."""
    from classpose_amd import augment, ops
    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 251, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    labs = [rng.integers(0, 7, (h, w)).astype(np.int16) for h, w in SIZES]
    planes = [np.stack([rng.random((h, w), dtype=np.float32), *(rng.standard_normal((2, h, w), dtype=np.float32) * 0.6)]) for h, w in SIZES]
    px_off, hw, total = augment.pool_table(SIZES)
    buf = torch.full((77 + 3 * total + 77,), 255, dtype=torch.uint8, device=cuda)         # guards of 255 at an odd offset
    buf[77:77 + 3 * total] = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims])).to(cuda)
    d = dict(ims=ims, labs=labs, planes=planes, pool_u8=buf[77:77 + 3 * total],
             pool_lab=torch.from_numpy(np.concatenate([lab.reshape(-1) for lab in labs])).to(cuda),
             pool_tgt=torch.from_numpy(fr.pack_planes(planes)).to(cuda), px_off=torch.from_numpy(px_off).to(cuda),
             hw=torch.from_numpy(hw).to(cuda))
    d["image_of"], d["inv"] = _maps()
    d["n"] = len(d["image_of"])
    d["args"] = (d["pool_u8"], d["pool_lab"], d["px_off"], d["hw"], d["image_of"], d["inv"], (DH, DW))
    d["plain"] = ops.warp_affine_pool(*d["args"], label_fill=FILL)
    d["flow"] = ops.warp_flow_targets(d["pool_tgt"], d["px_off"], d["hw"], d["image_of"], d["inv"], augment.identity_vecs(d["n"]), (DH, DW))
    return d


@pytest.mark.gpu
def test_the_plain_pool_warp_and_the_flow_warp_equal_the_restatements(family):
    f = family
    got, got_lab, status = (x.cpu().numpy() for x in f["plain"])
    flow, fstatus = (x.cpu().numpy() for x in f["flow"])
    assert int(status[0]) == 0 and int(fstatus[0]) == 0 and got.max() <= 250                # no guard byte shows
    ok = [t for t in range(f["n"]) if t != NAN]
    want_flow = fr.warp_flow_targets(f["planes"], f["image_of"][ok], f["inv"][ok], np.tile([1.0, 0, 0, 1.0], (len(ok), 1)), DH, DW)
    for k, t in enumerate(ok):
        i = f["image_of"][t]
        r64 = ar.warp_image(f["ims"][i].transpose(2, 0, 1), f["inv"][t], DH, DW, np.float64)
        worst = float(np.abs(got[t] - r64).max())
        print(f"crop {t} of image {i} {SIZES[i]}: max |device - float64| = {worst:.3e} (bound {WARP_ABS:.3e})")
        assert worst <= WARP_ABS and bool(r64.any()) == (t != MISS), (t, worst)
        assert np.array_equal(got_lab[t], ar.warp_labels(f["labs"][i], f["inv"][t], DH, DW, FILL)), t
        assert np.array_equal(flow[t], want_flow[k]), t                 # the float32 restatement of the kernel, value for value
    for t in (NAN, MISS):
        assert not got[t].any() and (got_lab[t] == FILL).all() and not flow[t].any(), t


@pytest.mark.gpu
def test_every_link_of_the_chain_is_bitwise(family, cuda):
    from classpose_amd import ops
    f, n = family, family["n"]
    plain, plain_lab, _s = f["plain"]
    rng = np.random.default_rng(6)
    sigma, bias = (rng.uniform(-0.25, 0.25, (n, 3)).astype(np.float32) for _ in range(2))
    jit, jit_lab, _s = ops.warp_affine_pool(*f["args"], sigma, bias, np.ones(n, np.int32), False, FILL)
    # stain, mode 0 / 1 == the plain entry without / with the jitter
    m0, l0, _s = ops.warp_affine_pool_stain(*f["args"], np.zeros(n, np.int32), label_fill=FILL)
    m1, l1, _s = ops.warp_affine_pool_stain(*f["args"], np.ones(n, np.int32), sigma, bias, label_fill=FILL)
    assert torch.equal(m0, plain) and torch.equal(l0, plain_lab) and torch.equal(m1, jit) and torch.equal(l1, jit_lab)
    assert torch.equal(jit_lab, plain_lab) and not torch.equal(jit, plain)
    # quality with nothing of its own == stain, in both modes
    q0, ql0, _s = ops.warp_affine_pool_quality(*f["args"], np.zeros(n, np.int32), label_fill=FILL)
    q1, ql1, _s = ops.warp_affine_pool_quality(*f["args"], np.ones(n, np.int32), sigma, bias, label_fill=FILL)
    assert torch.equal(q0, m0) and torch.equal(ql0, l0) and torch.equal(q1, m1) and torch.equal(ql1, l1)
    # per crop, the image on its own: warp_affine (uint8) with labels, and warp_affine (float32) of the three target planes
    flow, _s = f["flow"]
    for t, i in enumerate(f["image_of"]):
        one = f["inv"][t:t + 1]
        want, want_lab = ops.warp_affine(torch.from_numpy(f["ims"][i][None]).to(cuda), one, (DH, DW), torch.from_numpy(f["labs"][i][None]).to(cuda), FILL)
        assert torch.equal(plain[t], want[0]) and torch.equal(plain_lab[t], want_lab[0]), t
        want_f, _none = ops.warp_affine(torch.from_numpy(f["planes"][i][None]).to(cuda), one, (DH, DW))
        assert torch.equal(flow[t], want_f[0]), t


@pytest.mark.gpu
def test_bad_entries_keep_their_bit_and_cost_their_own_crop_only(family):
    from classpose_amd import augment, ops
    f, n = family, family["n"]
    vec = augment.identity_vecs(n)
    bad_of = f["image_of"].copy()
    bad_of[0] = len(SIZES)                                              # bit 0: an image index outside the pool
    bad_off = f["px_off"].clone()
    bad_off[1] = f["pool_u8"].numel() // 3 - 5                          # bit 1: the 5 x 7 image (crops 2, 4, 5) would leave the pool
    for image_of, px_off, bit, gone in ((bad_of, f["px_off"], 1, [0]), (f["image_of"], bad_off, 2, [2, 4, 5])):
        keep = [t for t in range(n) if t not in gone]
        mode = np.ones(n, np.int32)
        outs = [ops.warp_affine_pool(f["pool_u8"], f["pool_lab"], px_off, f["hw"], image_of, f["inv"], (DH, DW), label_fill=FILL, check_status=False),
                ops.warp_affine_pool_stain(f["pool_u8"], f["pool_lab"], px_off, f["hw"], image_of, f["inv"], (DH, DW), 0 * mode, label_fill=FILL,
                                           check_status=False),
                ops.warp_affine_pool_quality(f["pool_u8"], f["pool_lab"], px_off, f["hw"], image_of, f["inv"], (DH, DW), label_fill=FILL,
                                             check_status=False)]
        for got, got_lab, status in outs:
            assert int(status.item()) == bit
            assert not got[gone].any() and bool((got_lab[gone] == FILL).all())
            assert torch.equal(got[keep], f["plain"][0][keep]) and torch.equal(got_lab[keep], f["plain"][1][keep])
        flow, status = ops.warp_flow_targets(f["pool_tgt"], px_off, f["hw"], image_of, f["inv"], vec, (DH, DW), check_status=False)
        assert int(status.item()) == bit and not flow[gone].any() and torch.equal(flow[keep], f["flow"][0][keep])
        with pytest.raises(ValueError, match="image index outside the pool" if bit == 1 else "outside the pool"):
            ops.warp_flow_targets(f["pool_tgt"], px_off, f["hw"], image_of, f["inv"], vec, (DH, DW))


@pytest.mark.gpu
def test_byte_sums_of_the_pool_are_numpys(family):
    from classpose_amd import ops
    f = family
    assert f["pool_u8"].data_ptr() % 2 == 1
    sums = ops.pool_byte_sums(f["pool_u8"], f["px_off"], f["hw"]).cpu().numpy()
    want = np.array([int(im.astype(np.int64).sum()) for im in f["ims"]])
    print("byte sums", sums.tolist(), "numpy", want.tolist())
    assert sums.dtype == np.int64 and np.array_equal(sums, want)
