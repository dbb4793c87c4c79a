"""The reference's training data directory, loaded on the host for ``train_head --data_path``.

``images.npy`` holds ``(H, W, C)`` images whose sizes may differ (an object array then), ``labels.npy`` ``(H, W, 2)`` maps with
channel 0 = instance and channel 1 = class (README.md:176-182 of the reference).  Each step below restates one rule of
``classpose/train_utils.py`` and is pinned on the reference's own results by tests/golden/reference_train_data.npz:

  * ``load_data_arrays``            <- ``load_data_arrays`` (:587-617): images of an object-dtype element become float32, labels int64;
                                       floating labels become int64 and the number of distinct values must survive;
  * ``split_labels``                <- ``_split_labels(mask_classes=True)`` (:53-77): classes as int16, a class above 0 on instance 0
                                       and class 0 on an instance above 0 both become -100;
  * ``filter_single_pixel``         <- ``_filter_labels_and_images`` (:18-50): an image with exactly one non-zero instance pixel leaves;
  * ``subsample_indices``           <- ``subsample_dataset`` (:620-632) with the index sort of ``ClassposeDataset.subset``;
  * ``split_indices``               <- ``split_dataset`` (:635-652): sklearn's ``train_test_split(train_size=f, random_state=seed)``
                                       restated (``RandomState(seed).permutation``, test first), then the same sort.

Deliberately different: the reference filters images and labels but leaves the class list it split off earlier as it was, so the
classes of every image after a dropped one belong to its neighbour (run_training.py); here the three lists drop together.
Images must be uint8, or integer-valued floats in [0, 255] (what ``load_data_arrays`` makes of uint8 object arrays): the device
pool holds bytes.  Not built: ``--make_sparse``, HDF5 data sets.
"""
from __future__ import annotations

import os
from dataclasses import dataclass

import numpy as np

from .log import get_logger

logger = get_logger(__name__)


@dataclass
class TrainData:
    """``images`` [(H, W, 3) uint8], ``instances`` [(H, W) int64], ``classes`` [(H, W) int16, -100 = not annotated], one entry per
    image; ``n_classes`` = highest class + 1."""
    images: list
    instances: list
    classes: list
    n_classes: int

    def __len__(self) -> int:
        return len(self.images)

    def subset(self, indices) -> "TrainData":
        idx = [int(i) for i in indices]
        return TrainData([self.images[i] for i in idx], [self.instances[i] for i in idx], [self.classes[i] for i in idx], self.n_classes)


def load_data_arrays(data_dir) -> tuple[list, list]:
    """(images, labels) of ``data_dir``/images.npy and labels.npy as lists of arrays, converted as the reference converts them."""
    images_path, labels_path = os.path.join(data_dir, "images.npy"), os.path.join(data_dir, "labels.npy")
    if not os.path.exists(images_path) or not os.path.exists(labels_path):
        raise FileNotFoundError(f"Images or labels not found in {data_dir}")
    images = np.load(images_path, allow_pickle=True)
    labels = np.load(labels_path, allow_pickle=True)
    if len(images) == 0 or len(images) != len(labels):
        raise ValueError(f"{data_dir}: {len(images)} images but {len(labels)} label maps")
    images = [np.asarray(im) for im in images]
    if images[0].dtype == object:
        images = [np.ascontiguousarray(im).astype(np.float32) for im in images]
    labels = [np.asarray(lab) for lab in labels]
    if labels[0].dtype == object:
        labels = [np.ascontiguousarray(lab).astype(np.int64) for lab in labels]
    if np.issubdtype(labels[0].dtype, np.floating):
        logger.info("Labels are floating, converting to int64")
        n_float = len(np.unique(np.concatenate([np.ravel(lab) for lab in labels])))
        labels = [lab.astype(np.int64) for lab in labels]
        if len(np.unique(np.concatenate([np.ravel(lab) for lab in labels]))) != n_float:
            raise ValueError("Different number of unique labels after conversion to int64 - please check labels!")
    return images, labels


def image_to_uint8(image, index: int = 0) -> np.ndarray:
    """(H, W, 3) uint8 of a uint8 image or of a float image whose values are integers in [0, 255]; anything else raises."""
    image = np.asarray(image)
    if image.ndim != 3 or image.shape[2] != 3 or image.shape[0] < 1 or image.shape[1] < 1:
        raise ValueError(f"image {index}: expected (H, W, 3), got {image.shape}")
    if image.dtype == np.uint8:
        return np.ascontiguousarray(image)
    if np.issubdtype(image.dtype, np.floating):
        if not np.all(np.isfinite(image)) or image.min() < 0 or image.max() > 255 or np.any(image != np.floor(image)):
            raise ValueError(f"image {index}: float images must hold integer values in [0, 255] (the device pool holds bytes)")
        return np.ascontiguousarray(image.astype(np.uint8))
    raise ValueError(f"image {index}: uint8 or integer-valued float expected, got {image.dtype}")


def split_labels(labels) -> tuple[list, list]:
    """(instances [(H, W) int64], classes [(H, W) int16]) of (H, W, 2) label maps, with the reference's two masking rules."""
    instances, classes = [], []
    for i, lab in enumerate(labels):
        lab = np.asarray(lab)
        if lab.ndim != 3 or lab.shape[2] != 2 or not np.issubdtype(lab.dtype, np.integer):
            raise ValueError(f"labels {i}: expected an integer (H, W, 2) map (instance, class), got {lab.shape} {lab.dtype}")
        inst = np.ascontiguousarray(lab[:, :, 0]).astype(np.int64)
        cls = lab[:, :, 1].astype(np.int16)                    # np.int16(classes[i]) of the reference
        cls[np.logical_and(inst == 0, cls > 0)] = -100          # a class where there is no instance
        cls[np.logical_and(inst > 0, cls == 0)] = -100          # an instance without a class
        instances.append(inst)
        classes.append(cls)
    return instances, classes


def filter_single_pixel(images, instances, classes):
    """Drop every image with exactly one non-zero instance pixel -- from all three lists.  Returns them and the kept indices."""
    keep = [i for i, inst in enumerate(instances) if np.count_nonzero(inst) != 1]
    if len(keep) < len(instances):
        logger.info(f"Removed {len(instances) - len(keep)} images with a single pixel instance")
    return [images[i] for i in keep], [instances[i] for i in keep], [classes[i] for i in keep], np.asarray(keep, np.int64)


def load_dataset(data_dir) -> TrainData:
    """The data directory as the trainer takes it: loaded, converted to bytes, split into instance and masked class maps,
    single-pixel images dropped, the class count inferred."""
    images, labels = load_data_arrays(data_dir)
    images = [image_to_uint8(im, i) for i, im in enumerate(images)]
    for i, (im, lab) in enumerate(zip(images, labels)):
        if lab.shape[:2] != im.shape[:2]:
            raise ValueError(f"{data_dir}: image {i} is {im.shape[:2]} but its labels are {lab.shape[:2]}")
    instances, classes = split_labels(labels)
    images, instances, classes, _keep = filter_single_pixel(images, instances, classes)
    if not images:
        raise ValueError(f"{data_dir}: no image left")
    n_classes = int(max(int(c.max()) for c in classes)) + 1
    return TrainData(images, instances, classes, n_classes)


def subsample_indices(n: int, subsample_fraction: float | None, seed: int) -> np.ndarray:
    """Sorted indices of the ``int(fraction * n)`` images the reference keeps: the head of ``default_rng(seed).shuffle(arange(n))``."""
    if subsample_fraction is None:
        return np.arange(n, dtype=np.int64)
    idx = np.arange(n, dtype=np.int32)
    np.random.default_rng(seed).shuffle(idx)
    return np.sort(idx[:int(subsample_fraction * n)]).astype(np.int64)


def split_indices(n: int, train_fraction: float, seed: int) -> tuple[np.ndarray, np.ndarray | None]:
    """(train, test) sorted indices; ``train_fraction >= 1`` keeps everything for training (test None).  sklearn's shuffle split:
    ``n_train = floor(train_fraction * n)``, the rest is the test set, taken from the FRONT of ``RandomState(seed).permutation(n)``,
    the training set after it."""
    if train_fraction >= 1.0:
        return np.arange(n, dtype=np.int64), None
    n_train = int(np.floor(train_fraction * n))
    n_test = n - n_train
    if n_train < 1 or train_fraction <= 0:
        raise ValueError(f"train_fraction={train_fraction} leaves no training image out of {n}")
    perm = np.random.RandomState(seed).permutation(n)
    return np.sort(perm[n_test:n_test + n_train]).astype(np.int64), np.sort(perm[:n_test]).astype(np.int64)


def stats_chunk(H: int, W: int, n_classes: int, budget_bytes: int) -> int:
    """Images of H x W per device pass of ``dataset_stats.label_stats`` so that its workspace stays within ``budget_bytes`` (at
    least 1: a single 1024 x 1024 image already needs 44 MB of tables)."""
    from . import _lib
    per = _lib.lib().cpx_label_stats_workspace_bytes(1, int(H), int(W), int(n_classes))
    if per == 0:
        raise ValueError(f"label statistics: unsupported H={H}, W={W}, n_classes={n_classes}")
    chunk = max(1, min(65535, int(budget_bytes) // per))
    while chunk > 1 and _lib.lib().cpx_label_stats_workspace_bytes(chunk, int(H), int(W), int(n_classes)) > budget_bytes:
        chunk -= 1
    return chunk


def ragged_label_stats(instances, classes, n_classes: int, device="cuda:0", budget_bytes: int = 1 << 30,
                       label_instances: bool = False, connectivity: int = 8):
    """``dataset_stats.label_stats`` of maps of any sizes: one call per group of equal shape, each with the ``stats_chunk`` of its
    shape, the per-image results scattered back into the order of the lists.  ``label_instances`` / ``connectivity`` are those of
    ``dataset_stats.label_stats`` (instance counts of the connected components of every instance map).  Returns a ``LabelStats``."""
    from . import dataset_stats
    N = len(instances)
    groups: dict = {}
    for i, inst in enumerate(instances):
        groups.setdefault(tuple(inst.shape), []).append(i)
    class_counts = np.zeros(n_classes, np.int64)
    ipc, n_masks, diam = np.zeros((N, n_classes), np.float64), np.zeros(N, np.int64), np.zeros(N, np.float64)
    for (H, W), idx in groups.items():
        st = dataset_stats.label_stats(np.stack([instances[i] for i in idx]), np.stack([classes[i] for i in idx]), n_classes,
                                       device=device, chunk=stats_chunk(H, W, n_classes, budget_bytes),
                                       label_instances=label_instances, connectivity=connectivity)
        class_counts += st.class_counts
        ipc[idx], n_masks[idx], diam[idx] = st.instance_counts, st.n_masks, st.diameters
    return dataset_stats.LabelStats(class_counts, ipc, n_masks, diam)
