"""Host side of the H&E stain-matrix perturbation: the tables the kernels are handed, the tissue mask as one
threshold, and the two-stain basis of an image -- StarDist's CoNIC stain augmentation as the reference carries it
(transforms/he_staining.py).  numpy float64 only; nothing here touches the device.

The reference refits the basis (``extract_stains``: NMF on optical density) at every draw.  It is a per-image constant, so it
is fitted once per image here (``stain_basis``) on the samples ``ops.stain_samples`` cuts out of the pool.
"""
from __future__ import annotations

import numpy as np

SUBSAMPLE = 128                 # extract_stains(subsample=128): values[::128] when there are more than 128
# extract_stains: NMF(n_components=2, init="random", random_state=0, alpha_W=0.001, alpha_H=0, l1_ratio=1), sklearn's defaults else
NMF_SEED, NMF_ALPHA_W, NMF_TOL, NMF_MAX_ITER = 0, 0.001, 1e-4, 200


def density_table() -> np.ndarray:
    """(256,) float64: ``rgb_to_density`` of every byte, ``max(-log(max(b, 1) / 255), 1e-6)``, formed with the reference's numpy
    operations so that it is bitwise the reference's."""
    x = np.maximum(np.arange(256, dtype=np.uint8), 1)
    return np.maximum(-1 * np.log(x / 255), 1e-6)


def linear_table() -> np.ndarray:
    """(256,) float64: the sRGB byte as linear light, ``c / 12.92`` up to 0.04045 and ``((c + 0.055) / 1.055) ** 2.4`` above."""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4)


# L* = 116 f(Y) - 16 scaled by 2.55 and rounded is below 200 exactly when it is below 199.5 before rounding; f is the cube
# root on this side of the scale, so the test is Y < ((199.5 / 2.55 + 16) / 116) ** 3.  No colour of the 2^24 lies within
# 1.6e-8 of it.
Y_THRESHOLD = ((199.5 / 2.55 + 16) / 116) ** 3
Y_WEIGHTS = (0.212671, 0.715160, 0.072169)


def tissue_mask(img_u8: np.ndarray) -> np.ndarray:
    """``cv2.cvtColor(x, COLOR_RGB2LAB)[..., 0] < 200`` restated as one threshold on linear luminance, in the summation order
    of the kernel: ``(0.212671 lin[R] + 0.715160 lin[G]) + 0.072169 lin[B] < Y_THRESHOLD``."""
    lin = linear_table()
    img_u8 = np.asarray(img_u8)
    y = (Y_WEIGHTS[0] * lin[img_u8[..., 0]] + Y_WEIGHTS[1] * lin[img_u8[..., 1]]) + Y_WEIGHTS[2] * lin[img_u8[..., 2]]
    return y < Y_THRESHOLD


def lightness_u8(img_u8: np.ndarray) -> np.ndarray:
    """The rounded 8-bit L of an RGB image by the documented float formula (D65, Y alone): what the threshold restates."""
    lin = linear_table()
    img_u8 = np.asarray(img_u8)
    y = (Y_WEIGHTS[0] * lin[img_u8[..., 0]] + Y_WEIGHTS[1] * lin[img_u8[..., 1]]) + Y_WEIGHTS[2] * lin[img_u8[..., 2]]
    L = np.where(y > 0.008856, 116.0 * np.cbrt(y) - 16.0, 903.3 * y)
    return np.clip(np.rint(L * 2.55), 0, 255).astype(np.uint8)


def select_samples(img_u8: np.ndarray) -> tuple[np.ndarray, int]:
    """(samples (m, 3) uint8, tissue-pixel count k) of one image: the pixels ``extract_stains`` fits on -- the tissue pixels in
    raster order, all pixels when there is none, every 128th when there are more than 128.  What ``ops.stain_samples`` returns."""
    img_u8 = np.asarray(img_u8)
    mask = tissue_mask(img_u8)
    values = img_u8[mask]
    k = len(values)
    if k == 0:
        values = img_u8.reshape(-1, 3)
    if len(values) > SUBSAMPLE:
        values = values[::SUBSAMPLE]
    return np.ascontiguousarray(values), k


def sample_capacity(px) -> np.ndarray:
    """Triples an image of ``px`` pixels may need: ``max(128, ceil(px / 128))``."""
    px = np.asarray(px, np.int64)
    return np.maximum(128, -(-px // SUBSAMPLE))


def n_selected(k, px) -> np.ndarray:
    """How many samples come back for ``k`` tissue pixels out of ``px``."""
    k, px = np.asarray(k, np.int64), np.asarray(px, np.int64)
    n = np.where(k == 0, px, k)
    return np.where(n > SUBSAMPLE, -(-n // SUBSAMPLE), n)


def _cd_update(W: np.ndarray, HHt: np.ndarray, XHt: np.ndarray) -> float:
    """One sweep of sklearn's ``_update_cdnmf_fast`` with the identity permutation: the components in sequence, the rows of a
    component at once (a row's update reads its own row only)."""
    violation = 0.0
    for t in range(W.shape[1]):
        grad = -XHt[:, t]
        for r in range(W.shape[1]):
            grad = grad + HHt[t, r] * W[:, r]
        pg = np.where(W[:, t] == 0, np.minimum(0.0, grad), grad)
        violation += float(np.abs(pg).sum())
        hess = HHt[t, t]
        if hess != 0:
            W[:, t] = np.maximum(W[:, t] - grad / hess, 0.0)
    return violation


def nmf2(X: np.ndarray) -> np.ndarray:
    """``components_`` (2, 3) of the reference's NMF fit on X (n, 3) float64: random initialisation from ``RandomState(0)``,
    coordinate descent with an L1 penalty on W alone (``n_features * alpha_W``), stopped at 200 sweeps or when the projected
    gradient falls to 1e-4 of its first value.  Restated from scikit-learn's ``_fit_coordinate_descent``."""
    X = np.ascontiguousarray(X, np.float64)
    n, f = X.shape
    avg = np.sqrt(X.mean() / 2)
    rng = np.random.RandomState(NMF_SEED)
    H = np.abs(avg * rng.standard_normal(size=(2, f)))
    W = np.abs(avg * rng.standard_normal(size=(n, 2)))
    l1_w = f * NMF_ALPHA_W
    Ht = np.ascontiguousarray(H.T)
    first = 0.0
    for it in range(1, NMF_MAX_ITER + 1):
        violation = _cd_update(W, np.dot(Ht.T, Ht), np.dot(X, Ht) - l1_w)
        violation += _cd_update(Ht, np.dot(W.T, W), np.dot(X.T, W))
        if it == 1:
            first = violation
        if first == 0 or violation / first <= NMF_TOL:
            break
    return np.ascontiguousarray(Ht.T)


def stain_basis(samples_u8: np.ndarray):
    """(H (2, 3), Hinv (3, 2)) float64 of ``extract_stains`` from the sample pixels (m, 3) uint8 it fits on: density through
    the table, the NMF, rows normalised, swapped when ``H[0, 0] < H[1, 0]``, ``np.linalg.pinv``.  (None, None) where the basis is
    not finite (a zero row): the image then stays unaugmented, as the reference's ``try / except`` returns the original."""
    samples_u8 = np.asarray(samples_u8)
    if samples_u8.dtype != np.uint8 or samples_u8.ndim != 2 or samples_u8.shape[1] != 3 or len(samples_u8) == 0:
        raise ValueError("stain_basis: samples are (m, 3) uint8, m > 0")
    H = nmf2(density_table()[samples_u8])
    with np.errstate(divide="ignore", invalid="ignore"):
        H = H / np.linalg.norm(H, axis=1, keepdims=True)
    if not np.all(np.isfinite(H)):
        return None, None
    if H[0, 0] < H[1, 0]:
        H = H[[1, 0]]
    try:
        Hinv = np.linalg.pinv(H)
    except np.linalg.LinAlgError:
        return None, None
    if not np.all(np.isfinite(Hinv)):
        return None, None
    return H, Hinv


def image_basis(img_u8: np.ndarray):
    """``stain_basis`` of a whole image (host selection of the samples): for pre-cut crops and for tests."""
    return stain_basis(select_samples(img_u8)[0])


def stain_params(H, Hinv, u_matrix, u_stains, amount_matrix: float, amount_stains: float) -> np.ndarray:
    """(14,) float64 of one crop for ``ops.he_stain``: Hinv (3, 2), ``M = max(H + amount_matrix * U, 0)`` (2, 3) -- not
    renormalised -- and the two factors ``1 + amount_stains * u`` (augment_stains, he_staining.py:149-157)."""
    M = np.maximum(np.asarray(H, np.float64) + amount_matrix * np.asarray(u_matrix, np.float64).reshape(2, 3), 0)
    fac = 1 + amount_stains * np.asarray(u_stains, np.float64).reshape(2)
    return np.concatenate([np.asarray(Hinv, np.float64).reshape(6), M.reshape(6), fac])
