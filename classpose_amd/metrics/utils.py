"""Mask loading and shape checks with the reference's names (classpose/metrics/utils.py:97-159)."""
from __future__ import annotations

import glob
import os

import numpy as np


def load_masks(path: str):
    """A ``.npy`` / ``.npz`` file (``arr_0`` of an archive) -> its array; a directory -> the list of the arrays of its
    ``*.npy`` / ``*.npz`` files in sorted order.  ``ValueError`` for an empty directory or another extension."""
    if os.path.isdir(path):
        files = sorted(glob.glob(os.path.join(path, "*.np[yz]")))
        if not files:
            raise ValueError(f"No .npy or .npz files found in {path}")
        out = []
        for f in files:
            a = np.load(f, allow_pickle=True)
            out.append(a if isinstance(a, np.ndarray) else a["arr_0"])
        return out
    if path.endswith(".npy"):
        return np.load(path, allow_pickle=True)
    if path.endswith(".npz"):
        return np.load(path, allow_pickle=True)["arr_0"]
    raise ValueError(f"Unsupported file format: {path}")


def check_and_coherce_if_necessary(masks, expected_shape_length: int):
    """Lists pass through, object arrays become lists, a single mask of ``expected_shape_length`` dimensions gains a
    leading batch axis; any other rank is a ``ValueError``."""
    if isinstance(masks, np.ndarray) and masks.dtype == object:
        return list(masks)
    if isinstance(masks, list):
        return masks
    nd = len(masks.shape)
    if nd == expected_shape_length:
        return masks[None]
    if nd != expected_shape_length + 1:
        raise ValueError(f"Masks have {nd} dimensions, expected {expected_shape_length}")
    return masks
