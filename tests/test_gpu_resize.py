"""cpx_resize_linear_f32 / cpx_resize_nearest on the device against tests/resize_reference.py, on every element: bitwise for
float32 (both sides round every product and every sum to float32 and fuse nothing), integer equality for nearest.  Every
destination is pre-filled with a sentinel and followed by a guard row that must stay untouched."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import resize_reference as rr
from classpose_amd import _lib

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _field(rng, n, sh, sw):
    """standard normal x 1e3 plus a ramp: a wrong tap or weight moves a value by O(1e3)"""
    ramp = (np.arange(sh, dtype=np.float32)[:, None] * 7 + np.arange(sw, dtype=np.float32)[None, :] * 3)
    return (rng.standard_normal((n, sh, sw)) * 1e3).astype(np.float32) + ramp[None]


def _device_linear(dev, src, dh, dw, misalign=0):
    """through the raw ABI into a sentinel-filled buffer with one guard row (dw elements) after the end"""
    n, sh, sw = src.shape
    buf = torch.full((misalign + n * dh * dw + dw,), SENTINEL, dtype=torch.float32, device=dev)
    s = torch.from_numpy(src).to(dev)
    dst = buf[misalign:]
    _lib.check(_lib.lib().cpx_resize_linear_f32(s.data_ptr(), n, sh, sw, dst.data_ptr(), dh, dw,
                                                torch.cuda.current_stream(dev).cuda_stream), "resize_linear_f32")
    got = buf.cpu().numpy()
    assert np.all(got[:misalign] == SENTINEL) and np.all(got[misalign + n * dh * dw:] == SENTINEL), "wrote outside the destination"
    return got[misalign:misalign + n * dh * dw].reshape(n, dh, dw)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


SHAPES = [
    ((37, 53), (64, 80)),        # upscale: left / right clamp, unclamped top and bottom rows
    ((64, 80), (37, 53)),        # downscale
    ((64, 96), (32, 48)),        # exact 2 x: area path
    ((64, 80), (32, 53)),        # 2 x in y only: NOT the area path
    ((40, 40), (40, 40)),        # copy
    ((1, 1), (5, 7)), ((1, 9), (4, 9)), ((9, 1), (9, 4)),      # degenerate sources
    *[((7, 41), (5, dw)) for dw in (3, 63, 64, 65, 257)],        # vector tail and wave boundary
    ((10, 6), (5, 3)), ((10, 130), (5, 65)),                     # area path with a scalar tail
]


@pytest.mark.parametrize("n_planes", [1, 13])
@pytest.mark.parametrize("src_hw,dst_hw", SHAPES)
def test_linear_f32_equals_reference_bitwise(cuda, src_hw, dst_hw, n_planes):
    rng = np.random.default_rng([*src_hw, *dst_hw, n_planes])
    src = _field(rng, n_planes, *src_hw)
    want = rr.resize_linear_f32(src, *dst_hw)
    assert want.shape == (n_planes, *dst_hw) and np.isfinite(want).all()
    got = _device_linear(cuda, src, *dst_hw)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert len(bad) == 0, f"{len(bad)} elements differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}"


@pytest.mark.parametrize("src_hw,dst_hw", [((37, 53), (64, 80)), ((64, 96), (32, 48)), ((7, 41), (5, 64))])
def test_linear_f32_unaligned_destination(cuda, src_hw, dst_hw):
    """a destination 4 bytes off a 16-byte boundary must take the scalar stores and still equal the reference"""
    rng = np.random.default_rng(5)
    src = _field(rng, 3, *src_hw)
    got = _device_linear(cuda, src, *dst_hw, misalign=1)
    assert np.array_equal(_bits(got), _bits(rr.resize_linear_f32(src, *dst_hw)))


@pytest.mark.parametrize("src_hw,dst_hw", [((37, 53), (64, 80)), ((64, 80), (37, 53)), ((64, 96), (32, 48))])
def test_linear_f32_non_finite_pixels(cuda, src_hw, dst_hw):
    """single pixels of +inf, -inf and NaN (also in the clamped first / last column) spread exactly as in the reference"""
    rng = np.random.default_rng(6)
    src = _field(rng, 2, *src_hw)
    sh, sw = src_hw
    src[0, 5, 7], src[0, sh - 1, sw - 1], src[1, 0, 0], src[1, sh // 2, sw - 1] = np.inf, -np.inf, np.nan, np.inf
    want = rr.resize_linear_f32(src, *dst_hw)
    got = _device_linear(cuda, src, *dst_hw)
    assert not np.isfinite(want).all()
    assert np.array_equal(got, want, equal_nan=True)


@pytest.mark.parametrize("n_planes", [1, 13])
@pytest.mark.parametrize("src_hw,dst_hw", SHAPES)
@pytest.mark.parametrize("dtype", [np.uint16, np.uint8])
def test_nearest_equals_reference(cuda, dtype, src_hw, dst_hw, n_planes):
    rng = np.random.default_rng([*src_hw, *dst_hw, n_planes, np.dtype(dtype).itemsize])
    top = np.iinfo(dtype).max
    src = rng.integers(0, top + 1, (n_planes, *src_hw)).astype(dtype)
    src[0, 0, 0], src[-1, -1, -1] = top, top - 1          # 65535 / 255: the int16 storage must not sign-extend
    want = rr.resize_nearest(src, *dst_hw)
    dh, dw = dst_hw
    tdt = torch.int16 if dtype == np.uint16 else torch.uint8
    sent = 0x5A5A if dtype == np.uint16 else 0x5A
    buf = torch.full((n_planes * dh * dw + dw,), sent, dtype=tdt, device=cuda)
    s = torch.from_numpy(src.view(np.int16) if dtype == np.uint16 else src).to(cuda)
    _lib.check(_lib.lib().cpx_resize_nearest(s.data_ptr(), src.itemsize, n_planes, *src_hw, buf.data_ptr(), dh, dw,
                                             torch.cuda.current_stream(cuda).cuda_stream), "resize_nearest")
    got = buf.cpu().numpy().view(dtype)
    assert np.all(got[n_planes * dh * dw:] == sent), "wrote outside the destination"
    assert np.array_equal(got[:n_planes * dh * dw].reshape(n_planes, dh, dw), want)


def test_ops_wrappers_keep_leading_dims_and_reject_wrong_types(cuda):
    from classpose_amd import ops
    rng = np.random.default_rng(7)
    src = _field(rng, 6, 21, 30).reshape(2, 3, 21, 30)
    got = ops.resize_fields(torch.from_numpy(src).to(cuda), 33, 17)
    assert got.shape == (2, 3, 33, 17)
    assert np.array_equal(_bits(got.cpu().numpy()), _bits(rr.resize_linear_f32(src, 33, 17)))
    ids = rng.integers(0, 65536, (2, 21, 30)).astype(np.uint16)
    got = ops.resize_nearest(torch.from_numpy(ids.view(np.int16)).to(cuda), 33, 17)
    assert np.array_equal(ops.masks_to_numpy(got), rr.resize_nearest(ids, 33, 17))
    with pytest.raises(ValueError):
        ops.resize_fields(torch.zeros((4, 4), dtype=torch.float64, device=cuda), 2, 2)
    with pytest.raises(ValueError):
        ops.resize_nearest(torch.zeros((4, 4), dtype=torch.int32, device=cuda), 2, 2)
    with pytest.raises(_lib.CpxError):
        ops.resize_fields(torch.zeros((4, 4), dtype=torch.float32, device=cuda), 0, 2)
