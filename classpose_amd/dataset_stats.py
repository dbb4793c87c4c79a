"""Dataset statistics for training from instance annotations: class weights, oversampling probabilities and
cell diameters, from one device pass over the instance and class maps (``ops.label_stats``, csrc/cpx_labelstats.hip).

The reference makes that pass on the host: ``get_class_counts`` / ``get_instance_counts`` (train_utils.py:387-436) and
``cellpose.utils.diameters`` per image (train_utils.py:256-268).  ``get_class_weights`` and ``compute_oversampling_probabilities``
are host restatements of the reference functions of the same names (train_utils.py:439-496): a handful of float64 operations on
``n_classes`` numbers, pinned on the reference's own results by tests/golden/reference_label_stats.npz.

``label_instances=True`` of ``get_instance_counts`` (``skimage.measure.label`` of every instance map before counting) and the
reference's recipe for semantic-only sets (``ndimage.label`` per class, paper_experiments/run_cellpose_semantic.py:89-100) run on
the device too: ``ops.label_components`` (csrc/cpx_components.hip) behind ``label_stats(label_instances=True)`` and
``instances_from_classes``.  scikit-image is not a dependency, so both are restatements of the documented rule that are NOT
pinned on skimage results: the tests compare with scipy.ndimage.label and a breadth-first fill (tests/components_reference.py).

``split_touching=True`` of both cuts the regions that hold several touching cells: the peaks of the exact squared distance map
are seeds and every pixel goes to the nearest seed of its own region (``ops.split_touching``, csrc/cpx_split.hip).
An integer rule of this project's own, restated by tests/split_reference.py; not scikit-image's ``peak_local_max`` + ``watershed``.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import _lib, ops
from .log import get_logger

logger = get_logger(__name__)


@dataclass
class LabelStats:
    """``class_counts`` (ncls,) int64: ``get_class_counts``; ``instance_counts`` (N, ncls) float64: ``get_instance_counts``;
    ``n_masks`` (N,) int64: ``len(cellpose.utils.diameters(masks)[1])``; ``diameters`` (N,) float64: its first value, RAW -- the
    reference's clamp ``diam[diam < 5] = 5`` (train_utils.py:268) is ``clamp_diameters``, a separate step."""
    class_counts: np.ndarray
    instance_counts: np.ndarray
    n_masks: np.ndarray
    diameters: np.ndarray


def diameters_from_mid_areas(mid_area: np.ndarray) -> np.ndarray:
    """``np.median(counts ** 0.5) / (pi ** 0.5 / 2)`` of cellpose.utils.diameters from the two middle areas of the sorted counts:
    the median of m values is the mean of those at ranks (m - 1) / 2 and m / 2.  float64 on the host; {0, 0} (no mask) gives 0."""
    a = np.asarray(mid_area, np.float64).reshape(-1, 2)
    return (np.sqrt(a[:, 0]) + np.sqrt(a[:, 1])) / 2 / (np.pi ** 0.5 / 2)


def clamp_diameters(diameters: np.ndarray, minimum: float = 5.0) -> np.ndarray:
    """train_utils.py:268: ``diam_train[diam_train < 5] = 5.0`` (a copy)."""
    d = np.array(diameters, np.float64)
    d[d < minimum] = minimum
    return d


def _chunk_to_device(x, lo: int, hi: int, dtype: torch.dtype, dev) -> torch.Tensor:
    part = x[lo:hi]
    if not isinstance(part, torch.Tensor):
        part = np.asarray(part)
        if not np.issubdtype(part.dtype, np.integer):
            raise ValueError(f"label_stats: integer maps expected, got {part.dtype}")
        info = torch.iinfo(dtype)
        if part.size and (part.min() < info.min or part.max() > info.max):
            raise ValueError(f"label_stats: values outside the range of {dtype}")
        part = torch.from_numpy(np.ascontiguousarray(part.astype(np.int32 if dtype == torch.int32 else np.int16, copy=False)))
    elif part.dtype.is_floating_point:
        raise ValueError(f"label_stats: integer maps expected, got {part.dtype}")
    return part.to(device=dev, dtype=dtype).contiguous()


def instances_from_classes(classes, connectivity: int = 4, device="cuda:0", chunk: int = 1024, split_touching: bool = False,
                           min_distance: int = 5, min_radius: int = 2):
    """Instance maps of a semantic-only set: ``classes`` (N, H, W) integer class maps (numpy or tensor; device tensors are used
    where they are) -> ``(instances, n_components)``: an int32 (N, H, W) tensor on ``device`` and the (N,) int64 numpy counts.
    Classes <= 0 become background first -- class 0 and the -100 of pixels that are not annotated -- and every connected region
    of one class becomes one instance (``ops.label_components``, ``chunk`` images per call).  ``connectivity=4`` is the default
    because it is ``ndimage.label``'s in the reference's recipe (run_cellpose_semantic.py:89-100).  The ids are in raster order
    of each region's first pixel over all classes, where the reference numbers class after class: the PARTITION is the same,
    and nothing downstream depends on the numbering.  Touching cells of one class are one instance.  Restated, not pinned on the
    reference's output (module docstring).

    ``split_touching=True`` then cuts every region at its distance peaks (``ops.split_touching`` with ``min_distance``,
    ``min_radius`` and the same ``connectivity``); the counts are those after the cut.  ``False`` is exactly the above."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("instances_from_classes runs HIP kernels: pass a cuda device (there is no CPU path)")
    if len(classes.shape) != 3:
        raise ValueError("instances_from_classes: classes are (N, H, W) maps")
    if chunk < 1:
        raise ValueError("instances_from_classes: chunk must be positive")
    if connectivity not in (4, 8):
        raise ValueError(f"instances_from_classes: connectivity must be 4 or 8, not {connectivity!r}")
    N, H, W = (int(v) for v in classes.shape)
    chunk = min(int(chunk), 65535)
    out = torch.empty((N, H, W), dtype=torch.int32, device=dev)
    counts = np.zeros(N, np.int64)
    ws = None
    if N:
        nbytes = _lib.lib().cpx_label_components_workspace_bytes(min(chunk, N), H, W)
        if nbytes == 0:
            raise ValueError(f"instances_from_classes: unsupported H={H}, W={W} (H, W >= 1, H * W <= 2^28)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        part = _chunk_to_device(classes, lo, hi, torch.int32, dev).clamp_min(0)
        lab, cnt = ops.label_components(part, connectivity, workspace=ws)
        if split_touching:
            lab, cnt = ops.split_touching(lab, min_distance, min_radius, connectivity)
        out[lo:hi] = lab
        counts[lo:hi] = cnt.cpu().numpy()
    return out, counts


def split_summary(before: torch.Tensor, after: torch.Tensor):
    """``(components, split, instances)`` of instance maps before and after ``split_touching``: how many components there were,
    how many of them were cut, and how many instances there are now.  Both (N, H, W) int32 on one device; a report, not a hot
    path (``torch.unique`` over the (image, before, after) triples)."""
    fg = before > 0
    img = torch.arange(before.shape[0], device=before.device).view(-1, 1, 1).expand_as(before)[fg].long()
    b, a = before[fg].long(), after[fg].long()
    nb, na = int(before.max()) + 1 if b.numel() else 1, int(after.max()) + 1 if b.numel() else 1
    pairs = torch.unique((img * nb + b) * na + a)
    pieces = torch.unique(pairs // na, return_counts=True)[1]
    return int(pieces.numel()), int((pieces > 1).sum()), int(pairs.numel())


def label_stats(instances, classes, n_classes: int, device="cuda:0", chunk: int = 1024, label_instances: bool = False,
                connectivity: int = 8, split_touching: bool = False, min_distance: int = 5, min_radius: int = 2) -> LabelStats:
    """Statistics of N training crops: ``instances`` / ``classes`` (N, H, W) integer numpy arrays or tensors (device tensors are
    used where they are).  The device pass runs on ``chunk`` images at a time, so its workspace (two hash tables of >= 2 * H * W
    slots and one area list per image: 2.75 MB per 256 x 256 crop) stays bounded.  Raises ``ValueError`` for a negative id or a
    class >= ``n_classes``, naming the image.

    ``label_instances=True`` is the reference's ``get_instance_counts(label_instances=True)`` (train_utils.py:407-436):
    ``instance_counts`` are counted on ``label(instances)`` -- the connected components of equal non-zero id, background 0, full
    connectivity (``connectivity=8``, skimage's default in 2-D) -- so one id on two separate blobs counts twice.
    ``class_counts``, ``n_masks`` and ``diameters`` still come from the maps as given, as in the reference, which relabels only
    inside ``get_instance_counts``.  Restated, not pinned on skimage (module docstring).

    ``split_touching=True`` goes with ``label_instances=True``: the relabelled components are cut at their distance peaks
    (``ops.split_touching`` with ``min_distance`` and ``min_radius``) before ``instance_counts`` are counted, so three touching
    cells of one id count three times.  ``False`` is exactly the above."""
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("label_stats runs HIP kernels: pass a cuda device (there is no CPU path)")
    if split_touching and not label_instances:
        raise ValueError("label_stats: split_touching goes with label_instances=True")
    if connectivity not in (4, 8):
        raise ValueError(f"label_stats: connectivity must be 4 or 8, not {connectivity!r}")
    if len(instances) != len(classes) or tuple(instances.shape) != tuple(classes.shape) or len(instances.shape) != 3:
        raise ValueError("label_stats: instances and classes are (N, H, W) maps of one shape")
    if chunk < 1:
        raise ValueError("label_stats: chunk must be positive")
    N, H, W = (int(v) for v in instances.shape)
    chunk = min(int(chunk), 65535)
    class_px = np.zeros((N, n_classes), np.int64)
    ipc = np.zeros((N, n_classes), np.int64)
    n_masks = np.zeros(N, np.int64)
    mid = np.zeros((N, 2), np.int64)
    ws = cc_ws = None
    if N:
        nbytes = _lib.lib().cpx_label_stats_workspace_bytes(min(chunk, N), H, W, int(n_classes))
        if nbytes == 0:
            raise ValueError(f"label_stats: unsupported H={H}, W={W}, n_classes={n_classes} (1 <= n_classes <= 64)")
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if label_instances:
            cc_ws = torch.empty(_lib.lib().cpx_label_components_workspace_bytes(min(chunk, N), H, W), dtype=torch.uint8, device=dev)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        inst, cls = _chunk_to_device(instances, lo, hi, torch.int32, dev), _chunk_to_device(classes, lo, hi, torch.int16, dev)
        out = ops.label_stats(inst, cls, n_classes, workspace=ws, check_status=False)
        px, ic, nm, ma, st = (t.cpu().numpy() for t in out)
        if label_instances and not st.any():
            relabelled, _ = ops.label_components(inst, connectivity, workspace=cc_ws)
            if split_touching:
                relabelled, _ = ops.split_touching(relabelled, min_distance, min_radius, connectivity)
            ic = ops.label_stats(relabelled, cls, n_classes, workspace=ws, check_status=False)[1].cpu().numpy()
        bad = np.flatnonzero(st)
        if len(bad):
            what = "a negative instance id" if st[bad[0]] & 1 else f"a class >= {n_classes}"
            raise ValueError(f"label_stats: image {lo + int(bad[0])} has {what}")
        class_px[lo:hi], ipc[lo:hi], n_masks[lo:hi], mid[lo:hi] = px, ic, nm, ma
    return LabelStats(class_counts=class_px.sum(0), instance_counts=ipc.astype(np.float64), n_masks=n_masks,
                      diameters=diameters_from_mid_areas(mid))


def get_class_weights(class_counts: np.ndarray) -> np.ndarray:
    """train_utils.py:439-467: ``sqrt(median(positive counts) / count)`` rounded to 4 decimals, 0 for an absent class."""
    class_counts = np.asarray(class_counts)
    positive = class_counts[class_counts > 0]
    if positive.size == 0:
        raise ValueError("Cannot compute class weights with no positive class counts")
    median_count = np.median(positive)
    inv_freq = np.zeros_like(class_counts, dtype=np.float64)
    inv_freq[class_counts > 0] = median_count / class_counts[class_counts > 0]
    inv_freq = inv_freq ** 0.5
    return inv_freq.round(4)


def compute_oversampling_probabilities(class_counts: np.ndarray, instance_counts: np.ndarray, power: float = 1) -> np.ndarray:
    """train_utils.py:470-496: per image ``sum_j instance_counts[i, j] / class_counts[j]`` over the classes present, the class-0
    weight forced to 0, raised to ``power`` and normalised to sum 1.  Like the reference, a set without a single instance of a
    class above 0 yields NaN (0 / 0)."""
    class_counts = np.asarray(class_counts)
    class_weights = np.zeros_like(class_counts, dtype=np.float64)
    class_weights[class_counts > 0] = 1.0 / class_counts[class_counts > 0]
    class_weights[0] = 0
    weights = np.sum(np.asarray(instance_counts) * class_weights[None], 1)
    weights = weights ** power
    return weights / weights.sum()
