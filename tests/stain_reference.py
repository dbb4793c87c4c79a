"""float64 restatement of the H&E stain perturbation as the kernels compute it (include/classpose_hip.h, section t5): the yardstick
of tests/test_stain_host.py (against the reference-minted fixture) and of tests/test_gpu_stain.py (against the device).

Per pixel, left to right and unfused: ``d = density[byte]``; ``s_j = max((d0 Hinv[0][j] + d1 Hinv[1][j] + d2 Hinv[2][j]) * f_j, 0)``;
``x_c = s_0 M[0][c] + s_1 M[1][c]``; byte = ``trunc(clip(255 exp(-x_c), 0, 255))``.
"""
from __future__ import annotations

import numpy as np

from classpose_amd import stain

WINDOW = 1e-9       # a device value may be off by one level only where 255 exp(-x) of this restatement is this close to an integer


ZERO_MARGIN = 1e-12  # a stain clamped to zero counts as robustly zero when its value before the clamp is below -ZERO_MARGIN


def he_stain_values(img_u8: np.ndarray, params: np.ndarray, with_exact: bool = False):
    """``255 * exp(-x)`` (H, W, 3) float64, before the clip and the truncation, from the 14 doubles of ``stain.stain_params``.
    ``with_exact`` also returns the mask of values that are 255 because x is EXACTLY zero in any float64 evaluation: every stain
    that meets a non-zero matrix entry was clamped from at least ``ZERO_MARGIN`` below zero (rounding moves it by 1e-22).  Such a
    value is an integer by construction, not by accident, and no rounding can shift it."""
    params = np.asarray(params, np.float64)
    Hinv, M, f = params[0:6].reshape(3, 2), params[6:12].reshape(2, 3), params[12:14]
    d = stain.density_table()[np.asarray(img_u8)]
    s, safe = [], []
    for j in range(2):
        c = d[..., 0] * Hinv[0, j] + d[..., 1] * Hinv[1, j] + d[..., 2] * Hinv[2, j]
        s.append(np.maximum(c * f[j], 0.0))
        safe.append(c * f[j] <= -ZERO_MARGIN)
    x = np.stack([s[0] * M[0, c] + s[1] * M[1, c] for c in range(3)], -1)
    v = 255.0 * np.exp(-x)
    if not with_exact:
        return v
    exact = np.stack([(safe[0] | (M[0, c] == 0)) & (safe[1] | (M[1, c] == 0)) for c in range(3)], -1) & (x == 0)
    return v, exact


def he_stain(img_u8: np.ndarray, params: np.ndarray):
    """(uint8 image, the float64 values before the truncation, the mask of exactly-255 values of ``he_stain_values``)."""
    v, exact = he_stain_values(img_u8, params, True)
    return np.clip(v, 0, 255).astype(np.uint8), v, exact


def near_integer(v: np.ndarray, exact: np.ndarray | None = None, window: float = WINDOW) -> np.ndarray:
    """Where a value lies within ``window`` of an integer, the exactly-255 values of ``he_stain_values`` excepted."""
    near = np.abs(v - np.rint(v)) <= window
    return near if exact is None else near & ~exact


def check_against(got: np.ndarray, want: np.ndarray, v64: np.ndarray, exact: np.ndarray | None = None, window: float = WINDOW) -> dict:
    """``got`` may differ from ``want`` by one level, and only where ``v64`` lies within ``window`` of an integer (and is not
    exactly 255 by construction).  Returns the counts; raises AssertionError otherwise."""
    diff = got.astype(np.int16) - want.astype(np.int16)
    differ = diff != 0
    assert np.abs(diff).max(initial=0) <= 1, f"a value is off by {int(np.abs(diff).max())} levels"
    near = near_integer(v64, exact, window)
    outside = differ & ~near
    assert not outside.any(), f"{int(outside.sum())} values differ outside the {window} window"
    return {"differ": int(differ.sum()), "in_window": int(near.sum()), "size": int(got.size)}
