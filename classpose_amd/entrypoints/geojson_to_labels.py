"""``python -m classpose_amd.entrypoints.geojson_to_labels``: a directory of images and a directory of GeoJSON annotations (drawn
or corrected in QuPath) -> the ``images.npy`` / ``labels.npy`` pair ``train_head --data_path`` loads (classpose_amd/train_data.py).

    python -m classpose_amd.entrypoints.geojson_to_labels --images DIR --annotations DIR --class_names N1 N2 ... --out DIR \\
        [--coordinate_offset O] [--ignore_unknown]

Images and annotation files pair by file stem; images are read by PIL.  ``labels.npy`` holds (H, W, 2) int32 maps, channel 0 =
instance (the 1-based feature index of the image's file), channel 1 = class (position + 1 in ``--class_names``); both files are
object arrays when the image sizes differ.  All images of one size are painted by ONE device call (``cpx_rasterize_polygons`` with
a ring -> image table).  This is the reference's PUMA recipe (paper_experiments/scripts/organise-datasets.py:626-652, which is
``--coordinate_offset -1``) for any directory.
"""
from __future__ import annotations

import argparse
import os
from pathlib import Path

import numpy as np

from ..log import get_logger

logger = get_logger(__name__)

IMAGE_SUFFIXES = (".png", ".tif", ".tiff", ".jpg", ".jpeg", ".bmp")
ANNOTATION_SUFFIXES = (".geojson", ".json")


def pair_by_stem(images_dir, annotations_dir) -> list[tuple[str, Path, Path]]:
    """[(stem, image path, annotation path)] sorted by stem; an image without annotations or the reverse ends the run."""
    def by_stem(d, suffixes, what):
        if not os.path.isdir(d):
            raise SystemExit(f"{d}: not a directory")
        out: dict = {}
        for p in sorted(Path(d).iterdir()):
            if p.suffix.lower() in suffixes:
                if p.stem in out:
                    raise SystemExit(f"{d}: two {what} files with the stem {p.stem!r}")
                out[p.stem] = p
        return out
    imgs = by_stem(images_dir, IMAGE_SUFFIXES, "image")
    anns = by_stem(annotations_dir, ANNOTATION_SUFFIXES, "annotation")
    if not imgs:
        raise SystemExit(f"{images_dir}: no image ({', '.join(IMAGE_SUFFIXES)})")
    lone = sorted(set(imgs) ^ set(anns))
    if lone:
        raise SystemExit(f"images and annotations do not pair by file stem: {lone[:8]}")
    return [(s, imgs[s], anns[s]) for s in sorted(imgs)]


def stack_or_objects(arrays: list) -> np.ndarray:
    """one array when every shape agrees, else the object array ``np.load(allow_pickle=True)`` gives back element by element"""
    if len({a.shape for a in arrays}) == 1:
        return np.stack(arrays)
    out = np.empty(len(arrays), dtype=object)
    for i, a in enumerate(arrays):
        out[i] = a
    return out


def labels_of(pairs, class_names, coordinate_offset: float, ignore_unknown: bool, device="cuda"):
    """(images [(H, W, 3) uint8], labels [(H, W, 2) int32]) in the order of ``pairs``"""
    import torch
    from PIL import Image
    from .. import annotations, ops
    images, anns = [], []
    for _stem, ip, ap in pairs:
        images.append(np.ascontiguousarray(np.asarray(Image.open(ip).convert("RGB"), np.uint8)))
        anns.append(annotations.load_features(ap, class_names, ignore_unknown=ignore_unknown))
    labels: list = [None] * len(pairs)
    groups: dict = {}
    for i, im in enumerate(images):
        groups.setdefault(im.shape[:2], []).append(i)
    for (H, W), idx in groups.items():
        parts = [annotations.local_rings(anns[i], [(0.0, 0.0, float(W), float(H))], 1.0, coordinate_offset) for i in idx]
        xy = np.concatenate([p[0] for p in parts])
        counts = np.concatenate([np.diff(p[1]) for p in parts])
        off = np.zeros(len(counts) + 1, np.int64)
        off[1:] = np.cumsum(counts)
        value = np.concatenate([p[2] for p in parts])
        image = np.concatenate([np.full(len(p[2]), k, np.int32) for k, p in enumerate(parts)])
        inst = ops.rasterize_polygons(xy, off, value, (H, W), ring_image=image, n_images=len(idx), device=device)
        for k, i in enumerate(idx):
            class_of = np.concatenate([np.zeros(1, np.uint8), anns[i].feature_class])
            cls = ops.ids_to_classes(inst[k], class_of)
            labels[i] = torch.stack([inst[k], cls.to(torch.int32)], dim=-1).cpu().numpy()
    return images, labels


def main(args) -> None:
    pairs = pair_by_stem(args.images, args.annotations)
    if not 1 <= len(args.class_names) <= 255:
        raise SystemExit("--class_names: between 1 and 255 names")
    images, labels = labels_of(pairs, args.class_names, args.coordinate_offset, args.ignore_unknown)
    out = Path(args.out)
    out.mkdir(parents=True, exist_ok=True)
    np.save(out / "images.npy", stack_or_objects(images), allow_pickle=True)
    np.save(out / "labels.npy", stack_or_objects(labels), allow_pickle=True)
    n_cells = sum(len(np.unique(lab[..., 0])) - 1 for lab in labels)
    logger.info(f"{len(pairs)} images, {n_cells} annotated instances -> {out / 'images.npy'}, {out / 'labels.npy'}")


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Rasterise GeoJSON annotations into the images.npy / labels.npy pair train_head --data_path loads.")
    p.add_argument("--images", required=True, help="directory of images (read by PIL)")
    p.add_argument("--annotations", required=True, help="directory of .geojson / .json files with the images' file stems")
    p.add_argument("--class_names", required=True, nargs="+", help="classification names in class order: the first is class 1")
    p.add_argument("--out", required=True, help="directory for images.npy and labels.npy")
    p.add_argument("--coordinate_offset", type=float, default=0.0, help="added to every coordinate (QuPath exports of 1-based tools: -1)")
    p.add_argument("--ignore_unknown", action="store_true", help="a feature with a name outside --class_names gets class 0 instead of an error")
    return p


def main_with_args() -> None:
    main(build_parser().parse_args())


if __name__ == "__main__":
    main_with_args()
