"""Helpers of the flow-head training tests (tests/test_flow_train_host.py, tests/test_gpu_flow_train.py): the test maps, the
symmetry bookkeeping of ``oracle.dynamics.masks_to_flows``, the numpy restatement of ``cpx_warp_affine_pool_flow_f32`` and the
float64 / float32 restatements of the seg loss and of a two-head training step.  Nothing here calls the code under test."""
from __future__ import annotations

import numpy as np
import torch

import augment_reference as ar
import train_reference as tr


# ---- maps -----------------------------------------------------------------------------------------------------------
def symmetric_map() -> np.ndarray:
    """96 x 96 int32: three pixel-centred discs of radius 13, 9 and 6, a pixel-centred ellipse (semi-axes 7 x 15) and a 3 x 5 bar.
    Every extent is odd, so every label has ONE centre pixel (no tie between equally near pixels)."""
    m = np.zeros((96, 96), np.int32)
    yy, xx = np.mgrid[:96, :96]
    for k, (cy, cx, r) in enumerate([(16, 16, 13), (14, 50, 9), (12, 80, 6)], 1):
        m[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k
    m[((yy - 60) / 7.0) ** 2 + ((xx - 30) / 15.0) ** 2 <= 1.0] = 4
    m[80:83, 70:75] = 5
    return m


def border_map() -> np.ndarray:
    """64 x 80 int32: a label on every border (one of them in a corner) and one 50 x 50 square, whose padded box (52 x 52 = 2704
    cells) is above DIFF_SMALL_CELLS = 2048, so it runs in the second diffusion launch."""
    m = np.zeros((64, 80), np.int32)
    m[7:57, 5:55] = 1                   # the large square
    m[0:5, 20:31] = 2                   # top border
    m[59:64, 30:39] = 3                 # bottom border
    m[20:31, 75:80] = 4                 # right border
    m[30:37, 0:3] = 5                   # left border
    m[0:3, 70:80] = 6                   # top-right corner
    return m


def disc_crop(seed: int, size: int = 256, n: int = 12) -> np.ndarray:
    """A ``size`` x ``size`` int32 instance map of up to ``n`` non-overlapping pixel-centred discs of radius 6..14."""
    rng = np.random.default_rng(seed)
    m = np.zeros((size, size), np.int32)
    yy, xx = np.mgrid[:size, :size]
    k = 0
    for _ in range(20 * n):
        r = int(rng.integers(6, 15))
        cy, cx = (int(v) for v in rng.integers(r + 1, size - r - 1, 2))
        d = (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        grown = (yy - cy) ** 2 + (xx - cx) ** 2 <= (r + 2) ** 2
        if m[grown].any():
            continue
        k += 1
        m[d] = k
        if k == n:
            break
    return m


def centre_mask(masks: np.ndarray, centers: np.ndarray) -> np.ndarray:
    """bool (H, W): True at the one centre pixel per label that ``oracle.dynamics.masks_to_flows(..., return_debug=True)`` reports
    in ``centers`` (n, 2) as (y, x).  At most ``masks.max()`` pixels, each inside its own label."""
    out = np.zeros(masks.shape, bool)
    c = np.asarray(centers).astype(np.int64).reshape(-1, 2)
    assert len(c) <= int(masks.max())
    out[c[:, 0], c[:, 1]] = True
    assert int(out.sum()) <= int(masks.max())
    return out


def rot90(a: np.ndarray) -> np.ndarray:
    """The quarter turn of the identities below: new[i, j] = old[H - 1 - j, i], i.e. ``np.rot90(a, -1)`` -- the turn that takes the
    +X direction of the map to +Y (clockwise on a screen with y down).  ``np.rot90(a)`` is its inverse, see ``rot90_ccw_flows``."""
    return np.rot90(a, -1)


def rot90_flows(F: np.ndarray) -> np.ndarray:
    """(dY, dX) (2, H, W) of a map m -> the flows of rot90(m): (rot90(F_x), -rot90(F_y)).  T'(i, j) = T(H - 1 - j, i), so
    d/di T' = dT/dx and d/dj T' = -dT/dy."""
    return np.stack([rot90(F[1]), -rot90(F[0])])


def rot90_ccw_flows(F: np.ndarray) -> np.ndarray:
    """The same for the opposite turn np.rot90(m): (-np.rot90(F_x), np.rot90(F_y))."""
    return np.stack([-np.rot90(F[1]), np.rot90(F[0])])


def fliplr_flows(F: np.ndarray) -> np.ndarray:
    """(dY, dX) of a map -> the flows of m[:, ::-1]: (F_y[:, ::-1], -F_x[:, ::-1])."""
    return np.stack([F[0][:, ::-1], -F[1][:, ::-1]])


# ---- warp -----------------------------------------------------------------------------------------------------------
def warp_flow_targets(planes, image_of, inv, vec, dh: int, dw: int) -> np.ndarray:
    """numpy restatement of cpx_warp_affine_pool_flow_f32, bit for bit: ``planes`` a list of (3, h, w) float32 arrays, crop t from
    image ``image_of[t]``: the float32 bilinear warp of cpx_warp_affine_f32 on all three planes, then in float32 with each product
    and the sum rounded on their own  fy' = v0 fy + v1 fx,  fx' = v2 fy + v3 fx,  v = float32(vec[t])."""
    out = np.zeros((len(image_of), 3, dh, dw), np.float32)
    for t, im in enumerate(image_of):
        w = ar.warp_image(np.asarray(planes[im], np.float32), inv[t], dh, dw, np.float32)
        v = np.asarray(vec[t], np.float64).astype(np.float32)
        fy, fx = w[1], w[2]
        a, b = (v[0] * fy).astype(np.float32), (v[1] * fx).astype(np.float32)
        c, d = (v[2] * fy).astype(np.float32), (v[3] * fx).astype(np.float32)
        out[t, 0], out[t, 1], out[t, 2] = w[0], (a + b).astype(np.float32), (c + d).astype(np.float32)
    return out


def pack_planes(planes) -> np.ndarray:
    """The pool layout: image i's (3, h, w) planes flattened back to back (its floats start at 3 * px_off[i])."""
    return np.concatenate([np.ascontiguousarray(p, np.float32).reshape(-1) for p in planes])


# ---- seg loss -------------------------------------------------------------------------------------------------------
def seg_loss(z: torch.Tensor, targets: torch.Tensor):
    """cellpose train._loss_fn_seg restated in torch, in the dtype of ``z`` (n, 3, H, W) = (dY, dX, cellprob) logits:
    (MSELoss(mean)(z[:, :2], 5 * targets[:, 1:]) / 2, BCEWithLogitsLoss(mean)(z[:, 2], targets[:, 0] > 0.5))."""
    t = targets.to(z.dtype)
    flow = torch.nn.MSELoss(reduction="mean")(z[:, :2], 5.0 * t[:, 1:]) / 2.0
    cp = torch.nn.BCEWithLogitsLoss(reduction="mean")(z[:, 2], (t[:, 0] > 0.5).to(z.dtype))
    return flow, cp


def seg_loss_and_grad(z32: torch.Tensor, targets: torch.Tensor, dtype=torch.float64, w_seg: float = 1.0) -> dict:
    """{"flow", "cp", "dlogits" (n, 3, H, W)} by autograd in ``dtype`` on the float32 logits / targets the device read."""
    z = z32.to(dtype).clone().requires_grad_(True)
    flow, cp = seg_loss(z, targets.to(dtype))
    (w_seg * (flow + cp)).backward()
    return {"flow": flow.detach(), "cp": cp.detach(), "dlogits": z.grad.detach()}


def head_with_flow_logits(z32: torch.Tensor, ncls: int = 3, seed: int = 0) -> torch.Tensor:
    """float32 (n, 3, H, W) flow-head logits -> a head buffer (rows, ld_head) as cpx_net_forward lays it out: the flow columns
    0..191, then ``ncls * 64`` class columns (and padding) of NOISE, which the seg loss must not read."""
    tok = tr.nchw_to_tokens(z32)
    ld = (192 + ncls * 64 + 127) // 128 * 128
    g = torch.Generator().manual_seed(seed)
    head = torch.randn(tok.shape[0], ld, generator=g) * 50.0
    head[:, :192] = tok
    return head


# ---- two-head replay ------------------------------------------------------------------------------------------------
def replay_two_heads(feat, labels, targets, Wc0, bc0, Wf0, bf0, lrs, dtype, net_dtype, ncls, weight_decay):
    """CPU replay of ``HeadTrainer.step(..., flow_targets=)`` in ``dtype``: autograd of seg + ce + tversky down to both 1x1 heads on
    the copied features, AdamW per tensor with one step counter, the master weights re-rounded to the network dtype every step as
    the device does.  Returns (losses (steps,), seg losses (steps,), Wc, bc, Wf, bf)."""
    f = feat.to(dtype)
    P = [x.to(dtype).clone() for x in (Wc0, bc0, Wf0, bf0)]
    M = [torch.zeros_like(x) for x in P]
    V = [torch.zeros_like(x) for x in P]
    n = feat.shape[0] // 1024
    tg = targets.to(dtype)
    losses, segs = [], []
    for t, lr in enumerate(lrs, 1):
        R = [x.float().to(net_dtype).to(dtype).clone().requires_grad_(True) for x in P]     # weights and biases: rounded as at load
        logits = tr.tokens_to_nchw(f @ R[0].T + R[1], 0, ncls, n, 256, 256)
        z = tr.tokens_to_nchw(f @ R[2].T + R[3], 0, 3, n, 256, 256)
        ce, tv, *_ = tr.class_loss(logits, labels)
        flow, cp = seg_loss(z, tg)
        loss = (flow + cp) + ce + tv
        loss.backward()
        losses.append(float(loss.detach()))
        segs.append(float((flow + cp).detach()))
        for i in range(4):
            tr.adamw_step(P[i], R[i].grad.to(dtype), M[i], V[i], t, lr, weight_decay=weight_decay)
    return np.array(losses), np.array(segs), *P
