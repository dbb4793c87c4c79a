"""Tile ingest and blending (csrc/cpx_pre.hip) at the edges the workload's own shapes never reach: tiles of 1 to 3 pixels,
pixel counts that are no multiple of 4, channels that normalise to 0 (x99 - x01 <= 1e-3 with ptp > 0: "mode 2", the
mostly-background tile), sub-tile sizes other than 256, tiles smaller than the sub-tile, the 16-row sub-tile grid, blends
without class channels, and resizes from / to one pixel, upscales and the half-on-one-axis case.

Every check is exact equality with oracle/tiling.py, element by element.  The C entry points are called directly into
buffers that are longer than the result and pre-filled with a sentinel: the guard behind the result must keep it (the
smallest shapes run one block, where an unguarded tail shows nowhere else)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from classpose_amd import _lib, ops
from classpose_amd._lib import ptr
from classpose_amd.engine import make_tiling, percentile_params, taper_1d
from oracle import tiling

pytestmark = pytest.mark.gpu

SENT = -7777.25                                  # float32 guard sentinel (exact)
SENT16 = 0x7B5A                                  # bit pattern of the 16-bit guards
SENT8 = 0xA5
GUARD = 1024                                     # guard elements behind every result


def _stream(dev):
    return torch.cuda.current_stream(dev).cuda_stream


def _same(got, ref, what):
    """exact equality; a failure names the number of differing elements and the first one"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    bad = np.argwhere(got != ref)
    if len(bad):
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first at {i}: got {got[i]!r}, ref {ref[i]!r}")


def _guarded(n, dtype, dev):
    """flat buffer of n result elements + GUARD sentinels (the whole buffer starts as sentinel)"""
    if dtype == torch.float32:
        return torch.full((n + GUARD,), SENT, dtype=dtype, device=dev)
    if dtype == torch.uint8:
        return torch.full((n + GUARD,), SENT8, dtype=dtype, device=dev)
    if dtype == torch.int32:
        return torch.full((n + GUARD,), -777, dtype=dtype, device=dev)
    return torch.full((n + GUARD,), SENT16, dtype=torch.int16, device=dev).view(dtype)


def _guard_kept(buf, n, what):
    tail = buf[n:]
    if tail.dtype in (torch.bfloat16, torch.float16):
        tail, want = tail.view(torch.int16), SENT16
    else:
        want = {torch.float32: SENT, torch.uint8: SENT8, torch.int32: -777}[tail.dtype]
    bad = (tail != want).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} guard elements overwritten, first at result end + {int(bad[0])}"


# ---- contents -----------------------------------------------------------------------------------------------------------
def _speck_channel(rng, n, n_lo, n_hi, base=200):
    """`base` everywhere but n_lo random pixels below it and n_hi above"""
    v = np.full(n, base, np.uint8)
    pos = rng.permutation(n)[: n_lo + n_hi]
    v[pos[:n_lo]] = rng.integers(0, base, n_lo)
    v[pos[n_lo:]] = rng.integers(base + 1, 256, n_hi)
    return v


def _mode2_room(n):
    """most specks below / above the base value that leave both percentiles ON it: sorted[lo_prev] and sorted[hi_prev + 1]
    are then the base value, so x99 - x01 == 0 (numpy 'linear': indices from engine.percentile_params)"""
    lo_prev, _ = percentile_params(n, 1)
    hi_prev, _ = percentile_params(n, 99)
    return lo_prev, max(0, n - 2 - hi_prev)


def _specks(rng, H, W):
    """about 2 % specks on 200.  Channel 0: as many as mode 2 allows on both sides; channel 1: half of that;
    channel 2: one more on the low side than mode 2 allows (x01 leaves the base value: mode 1 by the smallest margin).
    Where no speck fits (a few pixels) one is placed anyway: mode 1, not a constant channel."""
    n = H * W
    lo, hi = _mode2_room(n)
    t = np.empty((n, 3), np.uint8)
    for c, (a, b) in enumerate([(lo, hi), (lo // 2, hi // 2), (min(lo + 1, n - 1), 0)]):
        if a + b == 0 and n > 1:
            a = 1
        t[:, c] = _speck_channel(rng, n, a, b)
    return t.reshape(H, W, 3)


def _content(kind, rng, H, W):
    n = H * W
    if kind == "uniform":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "one_zero":
        t = np.full((n, 3), 255, np.uint8)
        t[rng.integers(0, n, 3), np.arange(3)] = 0
        return t.reshape(H, W, 3)
    if kind == "specks":
        return _specks(rng, H, W)
    if kind == "const_channel":
        t = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        t[..., int(rng.integers(0, 3))] = 77
        return t
    lo, hi = {"bins_0_255": (0, 255), "bins_3_4": (3, 4), "bins_252_255": (252, 255)}[kind]
    if kind == "bins_0_255":                     # a different share of 255 in every channel, 1 % and 99 % among them
        p = rng.choice([0.004, 0.01, 0.3, 0.5, 0.99, 0.996], 3)
        return np.where(rng.random((H, W, 3)) < p, 255, 0).astype(np.uint8)
    return rng.integers(lo, hi + 1, (H, W, 3), dtype=np.uint8)


KINDS = ["uniform", "one_zero", "specks", "bins_0_255", "bins_3_4", "bins_252_255", "const_channel"]
NORM_SHAPES = [(1, 1), (1, 2), (1, 3), (2, 2), (1, 7), (3, 5), (17, 13), (101, 1), (7, 143), (208, 208)]


def _ref_stats(t):
    """[x01, den, mode, x99] per (tile, channel) the way oracle.tiling.normalize_img / normalize99 decide them"""
    st = np.empty(t.shape[:1] + (3, 4), np.float32)
    for k in range(t.shape[0]):
        for c in range(3):
            x = t[k, ..., c].astype(np.float32)
            x01, x99 = np.percentile(x, 1), np.percentile(x, 99)
            mode = 0.0 if np.ptp(x) == 0 else (1.0 if x99 - x01 > 1e-3 else 2.0)
            st[k, c] = (x01, x99 - x01, mode, x99)
    return st


def _ref_norm(t):
    return np.concatenate([tiling.normalize_img(t[k:k + 1]) for k in range(len(t))])


# ---- 1. normalisation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nT", [1, 5])
@pytest.mark.parametrize("H,W", NORM_SHAPES)
def test_normalize_stats_and_pixels_every_element(cuda, H, W, nT, kind):
    """cpx_normalize_stats_u8 / cpx_normalize_apply_u8 == tiling.normalize_img per tile: stats [x01, den, mode, x99] and
    every pixel.  nT * 3 = 3 or 15 channels: a partly filled block of four waves in k_norm_stats either way."""
    rng = np.random.default_rng([H, W, nT, KINDS.index(kind)])
    t = np.stack([_content(kind, rng, H, W) for _ in range(nT)])
    ref = _ref_norm(t)
    assert np.isfinite(ref).all()
    st_ref = _ref_stats(t)
    if kind == "specks" and H * W >= 101:
        assert (st_ref[..., 2] == 2.0).any(), "the case was built to hold a mode-2 channel"
        assert all((ref[k, ..., 0] == 0).all() and np.ptp(t[k, ..., 0]) > 0 for k in range(nT))

    L, s = _lib.lib(), _stream(cuda)
    tiles = torch.from_numpy(t).to(cuda)
    stats = _guarded(nT * 12, torch.float32, cuda)
    hist = _guarded(nT * 768, torch.int32, cuda)
    lo, hi = percentile_params(H * W, 1), percentile_params(H * W, 99)
    _lib.check(L.cpx_normalize_stats_u8(ptr(tiles), nT, H, W, lo[0], lo[1], hi[0], hi[1], ptr(stats), ptr(hist), s), "stats")
    out = _guarded(nT * H * W * 3, torch.float32, cuda)
    _lib.check(L.cpx_normalize_apply_u8(ptr(tiles), ptr(stats), nT, H, W, ptr(out), s), "apply")
    what = f"{kind} {nT}x{H}x{W}"
    _same(stats[: nT * 12].cpu().numpy().reshape(nT, 3, 4), st_ref, what + " stats [x01, den, mode, x99]")
    _same(out[: nT * H * W * 3].cpu().numpy().reshape(t.shape), ref, what + " pixels")
    _guard_kept(stats, nT * 12, what + " stats")
    _guard_kept(hist, nT * 768, what + " histogram workspace")
    _guard_kept(out, nT * H * W * 3, what + " pixels")
    if kind == "specks" and H * W >= 101:
        assert (stats[: nT * 12].view(nT, 3, 4)[..., 2] == 2.0).any()


# ---- 2. / 3. the sub-tile table -------------------------------------------------------------------------------------------
def _shapes(b):
    return [(b, b), (b - 1, b + 1), (5, 3 * b + 7), (2 * b + 9, b // 2), (1, 1), (7 * b // 2, 16)]


TABLE = [(b, H, W, aug) for b in (32, 64, 224) for H, W in _shapes(b) for aug in (False, True)]
TABLE += [(256, 208, 208, False), (256, 208, 208, True)]        # a 427-pixel read at factor 0.486: smaller than the sub-tile
TABLE += [(32, 240, 16, True), (32, 400, 16, False)]            # 16 sub-tiles along y: the whole ys[16] table
TABLE_IDS = [f"b{b}-{H}x{W}-{'aug' if aug else 'plain'}" for b, H, W, aug in TABLE]
NT = 3


def _table_tiles(b, H, W):
    """tile 0 random, tile 1 with a mode-2 channel (where the tile has room for one), tile 2 with a constant channel"""
    rng = np.random.default_rng([b, H, W])
    t = rng.integers(0, 256, (NT, H, W, 3), dtype=np.uint8)
    lo, hi = _mode2_room(H * W)
    t[1, ..., 1] = _speck_channel(rng, H * W, lo, hi).reshape(H, W)
    t[2, ..., 2] = 131
    return t


def _ref_subtiles(b, H, W, aug):
    t = _table_tiles(b, H, W)
    x = _ref_norm(t)
    return t, np.concatenate([tiling.subtile_batch(x[k:k + 1], b, aug)[0] for k in range(NT)])


def test_the_table_reaches_the_16_row_grid():
    assert make_tiling(240, 16, 32, True).ny == 16 and make_tiling(240, 16, 32, True).nx == 3
    assert make_tiling(400, 16, 32, False).ny == 16


@pytest.mark.parametrize("b,H,W,aug", TABLE, ids=TABLE_IDS)
def test_subtiles_and_patch_rows_every_element(cuda, b, H, W, aug):
    """cpx_make_subtiles_f32 == tiling.subtile_batch(tiling.normalize_img(tile)); cpx_make_patches (bf16 / fp16 / fp32) ==
    the same pixels in im2col order, cast with .to(dtype)"""
    t, ref = _ref_subtiles(b, H, W, aug)
    til = make_tiling(H, W, b, aug)
    nS = NT * til.ny * til.nx
    assert ref.shape == (nS, 3, b, b)
    L, s = _lib.lib(), _stream(cuda)
    tiles = torch.from_numpy(t).to(cuda)
    stats = ops.normalize_stats(tiles)
    if H * W >= 101:
        assert stats[1, 1, 2] == 2.0 and stats[2, 2, 2] == 0.0      # both branches of norm_px pass through the writers
    what = f"bsize {b} tile {H}x{W} augment {aug}"

    n = nS * 3 * b * b
    sub = _guarded(n, torch.float32, cuda)
    _lib.check(L.cpx_make_subtiles_f32(ptr(tiles), ptr(stats), NT, C.byref(til), ptr(sub), s), "make_subtiles_f32")
    _same(sub[:n].cpu().numpy().reshape(ref.shape), ref, what + " sub-tiles")
    _guard_kept(sub, n, what + " sub-tiles")

    tb = b // 8
    rows = torch.from_numpy(ref).reshape(nS, 3, tb, 8, tb, 8).permute(0, 2, 4, 1, 3, 5).reshape(nS * tb * tb, 192)
    for code, dt in ((_lib.DT_BF16, torch.bfloat16), (_lib.DT_F16, torch.float16), (_lib.DT_F32, torch.float32)):
        pat = _guarded(n, dt, cuda)
        _lib.check(L.cpx_make_patches(ptr(tiles), ptr(stats), NT, C.byref(til), code, ptr(pat), s), "make_patches")
        _same(pat[:n].cpu().float().numpy().reshape(rows.shape), rows.to(dt).float().numpy(), f"{what} patch rows {dt}")
        _guard_kept(pat, n, f"{what} patch rows {dt}")


# ---- 3. blend -------------------------------------------------------------------------------------------------------------
NCLS_MAX = 7
BLEND_NT = 2


@functools.lru_cache(maxsize=2)
def _ref_blend(b, H, W, aug):
    """random network outputs for BLEND_NT tiles with NCLS_MAX class planes and their blend by the oracle; a case with fewer
    classes takes the first planes (every plane blends on its own)"""
    rng = np.random.default_rng([b, H, W, int(aug), 7])
    geom = tiling.subtile_batch(np.zeros((1, H, W, 3), np.float32), b, aug)[1]
    nsub = geom["ny"] * geom["nx"]
    y = rng.standard_normal((BLEND_NT * nsub, 3, b, b)).astype(np.float32)
    yc = rng.standard_normal((BLEND_NT * nsub, NCLS_MAX, b, b)).astype(np.float32)
    yf, ycf = zip(*[tiling.blend_subtiles(y[k * nsub:(k + 1) * nsub], yc[k * nsub:(k + 1) * nsub], geom, aug)
                    for k in range(BLEND_NT)])
    yf, ycf = np.stack(yf), np.stack(ycf)
    assert np.isfinite(yf).all() and np.isfinite(ycf).all()
    for a in (y, yc, yf, ycf):
        a.setflags(write=False)
    return y, yc, yf, ycf


LD_HEAD = {0: 192, 1: 320, 7: 640}                # 1 class: a pad block behind the class block; 0: no class block at all


@pytest.mark.parametrize("ncls", [0, 1, 7])
@pytest.mark.parametrize("b,H,W,aug", TABLE, ids=TABLE_IDS)
def test_blend_every_element(cuda, b, H, W, aug, ncls):
    """cpx_blend_subtiles_nchw == tiling.blend_subtiles, and the token-major cpx_blend_subtiles (the network head's layout,
    pixel shuffle folded in) == the NCHW result bit for bit.  ncls == 0: no y_class, no logits, ld_head = 192."""
    y, yc, yf, ycf = _ref_blend(b, H, W, aug)
    til = make_tiling(H, W, b, aug)
    nT, HW = BLEND_NT, H * W
    nS = nT * til.ny * til.nx
    assert y.shape[0] == nS
    L, s = _lib.lib(), _stream(cuda)
    taper = torch.from_numpy(taper_1d(b)).to(cuda)
    what = f"bsize {b} tile {H}x{W} augment {aug} ncls {ncls}"
    yd = torch.from_numpy(y.copy()).to(cuda)
    ycd = torch.from_numpy(yc[:, :ncls].copy()).to(cuda) if ncls else None

    def bufs():
        return (_guarded(nT * 2 * HW, torch.float32, cuda), _guarded(nT * HW, torch.float32, cuda),
                _guarded(nT * ncls * HW, torch.float32, cuda) if ncls else None)

    def check(dP, cp, lg, name):
        _same(dP[: nT * 2 * HW].cpu().numpy().reshape(nT, 2, H, W), yf[:, :2], f"{what} {name} dP")
        _same(cp[: nT * HW].cpu().numpy().reshape(nT, H, W), yf[:, 2], f"{what} {name} cellprob")
        _guard_kept(dP, nT * 2 * HW, f"{what} {name} dP")
        _guard_kept(cp, nT * HW, f"{what} {name} cellprob")
        if ncls:
            _same(lg[: nT * ncls * HW].cpu().numpy().reshape(nT, ncls, H, W), ycf[:, :ncls], f"{what} {name} logits")
            _guard_kept(lg, nT * ncls * HW, f"{what} {name} logits")

    dP, cp, lg = bufs()
    _lib.check(L.cpx_blend_subtiles_nchw(ptr(yd), ptr(ycd), ncls, nT, C.byref(til), ptr(taper), ptr(dP), ptr(cp), ptr(lg), s),
               "blend_nchw")
    check(dP, cp, lg, "NCHW")

    tb, ld = b // 8, LD_HEAD[ncls]
    full = np.concatenate([y, yc[:, :ncls]], 1)                       # [nS, 3 + ncls, b, b]
    head = np.full((nS, tb * tb, ld), np.nan, np.float32)             # a read of a pad column would show
    head[:, :, : (3 + ncls) * 64] = (full.reshape(nS, 3 + ncls, tb, 8, tb, 8).transpose(0, 2, 4, 1, 3, 5)
                                     .reshape(nS, tb * tb, -1))
    hd = torch.from_numpy(head).to(cuda)
    dP2, cp2, lg2 = bufs()
    _lib.check(L.cpx_blend_subtiles(ptr(hd), ld, ncls, nT, C.byref(til), ptr(taper), ptr(dP2), ptr(cp2), ptr(lg2), s), "blend")
    check(dP2, cp2, lg2, "token-major")
    assert torch.equal(dP2.view(torch.int32), dP.view(torch.int32)) and torch.equal(cp2.view(torch.int32), cp.view(torch.int32))
    if ncls:
        assert torch.equal(lg2.view(torch.int32), lg.view(torch.int32))


# ---- 4. resize ------------------------------------------------------------------------------------------------------------
RESIZE = [((1, 9), 0.5, (1, 4)), ((2, 2), 0.5, (1, 1)), ((5, 4), 0.5, (2, 2)), ((4, 5), 0.5, (2, 2)),
          ((2, 256), 0.5, (1, 128)), ((255, 3), 0.5, (128, 2)), ((3, 3), 3.0, (9, 9)), ((1, 1), 4.0, (4, 4)),
          ((9, 1), 2.5, (22, 2)), ((64, 64), 2.0, (128, 128)), ((33, 65), 0.03, (1, 2)), ((7, 300), 0.486, (3, 146))]


@pytest.mark.parametrize("nT", [1, 3])
@pytest.mark.parametrize("shape,factor,dshape", RESIZE)
def test_resize_edges_every_element(cuda, shape, factor, dshape, nT):
    """cpx_resize_linear_u8 == tiling.resize_linear_u8 (its restatement of cv2.resize INTER_LINEAR for 8UC3; parity with cv2
    unpinned): destinations and sources one pixel wide or high, upscales, the exact 2x2 decimation (area path) and the
    tiles where only ONE axis halves exactly ((5, 4) and (4, 5) -> 2x2), which are bilinear."""
    dh, dw = ops.resized_shape(shape[0], shape[1], factor)
    assert (dh, dw) == dshape
    rng = np.random.default_rng([shape[0], shape[1], nT])
    tiles = rng.integers(0, 256, (nT,) + shape + (3,), dtype=np.uint8)
    n = nT * dh * dw * 3
    buf = _guarded(n, torch.uint8, cuda)
    got = ops.resize_tile_to_target_mpp(torch.from_numpy(tiles).to(cuda), factor, out=buf[:n].view(nT, dh, dw, 3))
    assert got.data_ptr() == buf.data_ptr()
    want = np.stack([tiling.resize_linear_u8(tiles[k], dw, dh) for k in range(nT)])
    what = f"{nT}x{shape} * {factor} -> {dshape}"
    _same(got.cpu().numpy(), want, what)
    _guard_kept(buf, n, what)
