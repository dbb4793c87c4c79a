"""Mint the training-data fixture from the REFERENCE's own functions (run in the build container only).

    python tests/golden/make_golden_train_data.py      # rewrites tests/golden/reference_train_data.npz / .json

``classpose.train_utils`` is imported under the stub finder of make_golden.py.  Called on the CPU: ``load_data_arrays`` on three
small data directories written to a temporary folder, ``_split_labels`` and ``_filter_labels_and_images`` on what it returns (in
the order of ``_process_train_test``: split, then filter), and ``subsample_dataset`` / ``split_dataset`` on a bare
``ClassposeDataset`` with ``length`` / ``indices`` set, of which ``.indices`` is recorded.  The fixture holds data only: the inputs
as saved, and per image the instance map, the masked class map and whether the reference kept the image.
"""
from __future__ import annotations

import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
os.environ.setdefault("TQDM_DISABLE", "1")

SPLITS = [(n, seed, f) for n in (10, 37) for seed in (0, 42) for f in (0.5, 0.8)]


def _cells(rng, H, W, n):
    """(H, W, 2) int32: n rectangles with ids 1..n and classes 1..4 on a background of (0, 0)."""
    lab = np.zeros((H, W, 2), np.int32)
    for k in range(n):
        h, w = min(H, int(rng.integers(2, max(3, H // 3)))), min(W, int(rng.integers(2, max(3, W // 3))))
        y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
        lab[y:y + h, x:x + w, 0] = k + 1
        lab[y:y + h, x:x + w, 1] = 1 + k % 4
    return lab


def make_cases(rng):
    """name -> (images, labels, how they are saved)."""
    cases = {}
    # ragged sizes in an object array of uint8 / int32 arrays; both masking rules; one image with a single instance pixel
    shapes = [(20, 28), (33, 17), (9, 11), (12, 12), (1, 1), (40, 25)]
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in shapes]
    labs = [_cells(rng, h, w, 3) for h, w in shapes]
    labs[0][0:3, 0:4, 0], labs[0][0:3, 0:4, 1] = 0, 3            # a class above 0 where there is no instance
    labs[1][30:33, 0:5, 0], labs[1][30:33, 0:5, 1] = 9, 0        # an instance without a class
    labs[2][:] = 0
    labs[2][4, 5] = (7, 2)                                       # exactly one instance pixel: the image is dropped
    labs[4][:] = 0                                               # 1 x 1 and empty: zero instance pixels, kept
    cases["ragged"] = (ims, labs, "object array of arrays")
    # equal sizes saved with dtype=object: load_data_arrays turns the images into float32 and the labels into int64
    ims = [rng.integers(0, 256, (16, 16, 3), dtype=np.uint8) for _ in range(3)]
    labs = [_cells(rng, 16, 16, 4) for _ in range(3)]
    labs[1][0:2, 0:2, 0], labs[1][0:2, 0:2, 1] = 0, 2
    cases["objdtype"] = (ims, labs, "object dtype")
    # floating labels of one shape: converted to int64 under the uniqueness check
    ims = [rng.integers(0, 256, (14, 18, 3), dtype=np.uint8) for _ in range(3)]
    labs = [_cells(rng, 14, 18, 3).astype(np.float64) for _ in range(3)]
    labs[2][5:8, 5:9, 0], labs[2][5:8, 5:9, 1] = 11.0, 0.0
    cases["floatlabels"] = (ims, labs, "plain array")
    return cases


def save_case(folder, ims, labs, how):
    """Write images.npy / labels.npy the way ``how`` says.  tests/test_train_data_host.py rebuilds the directories the same way."""
    os.makedirs(folder, exist_ok=True)
    if how == "object array of arrays":
        a, b = np.empty(len(ims), object), np.empty(len(labs), object)
        for i in range(len(ims)):
            a[i], b[i] = ims[i], labs[i]
    elif how == "object dtype":
        a, b = np.array(ims, dtype=object), np.array(labs, dtype=object)
    else:
        a, b = np.stack(ims), np.stack(labs)
    np.save(os.path.join(folder, "images.npy"), a, allow_pickle=True)
    np.save(os.path.join(folder, "labels.npy"), b, allow_pickle=True)


def main():
    import make_golden
    sys.meta_path.insert(0, make_golden._Finder())
    sys.path.insert(0, make_golden.REF)
    from classpose import train_utils as rtu
    from classpose.dataset import ClassposeDataset

    rng = np.random.default_rng(20261018)
    arrays, meta = {}, {"cases": [], "splits": []}
    with tempfile.TemporaryDirectory() as tmp:
        for name, (ims, labs, how) in make_cases(rng).items():
            save_case(os.path.join(tmp, name), ims, labs, how)
            images, labels = rtu.load_data_arrays(os.path.join(tmp, name))
            images = [np.transpose(im, (2, 0, 1)) for im in images]                   # process_and_build_dataset
            labels = [np.transpose(lab, (2, 0, 1)) for lab in labels]
            inst, classes = rtu._split_labels(labels)
            kept_images, kept_inst = rtu._filter_labels_and_images(images, inst)
            kept = [any(y is k for k in kept_inst) for y in inst]
            assert sum(kept) == len(kept_images) == len(kept_inst)
            for i in range(len(ims)):
                arrays[f"{name}_image_{i}"], arrays[f"{name}_labels_{i}"] = ims[i], labs[i]
                arrays[f"{name}_loaded_image_{i}"] = np.transpose(images[i], (1, 2, 0))
                arrays[f"{name}_inst_{i}"] = np.asarray(inst[i][0], np.int64)
                arrays[f"{name}_cls_{i}"] = classes[i][0]
                assert classes[i][0].dtype == np.int16
            meta["cases"].append(dict(name=name, n=len(ims), saved_as=how, kept=[bool(k) for k in kept],
                                      loaded_image_dtype=str(images[0].dtype), loaded_label_dtype=str(labels[0].dtype),
                                      max_class=int(max(c.max() for c in classes))))
            print(name, "kept", kept, images[0].dtype, labels[0].dtype)
    assert meta["cases"][0]["kept"] == [True, True, False, True, True, True]
    for n, seed, f in SPLITS:
        ds = ClassposeDataset()
        ds.length, ds.indices = n, np.arange(n, dtype=np.int32)
        sub = rtu.subsample_dataset(ds, f, seed)
        tr, te = rtu.split_dataset(ds, f, seed)
        sub_tr, sub_te = rtu.split_dataset(sub, f, seed)                              # run_training.py: subsample, then split
        key = f"split_{n}_{seed}_{f}"
        for what, d in (("sub", sub), ("train", tr), ("test", te), ("sub_train", sub_tr), ("sub_test", sub_te)):
            arrays[f"{key}_{what}"] = np.asarray(d.indices, np.int64)
            assert len(d) == len(d.indices)
        meta["splits"].append(dict(n=n, seed=seed, fraction=f, key=key))
        print(key, "sub", len(sub), "train", len(tr), "test", len(te), "sub_train", len(sub_tr))
    np.savez_compressed(os.path.join(HERE, "reference_train_data.npz"), **arrays)
    with open(os.path.join(HERE, "reference_train_data.json"), "w") as f:
        json.dump(meta, f, indent=1)
    print("wrote reference_train_data.npz", os.path.getsize(os.path.join(HERE, "reference_train_data.npz")), "bytes")


if __name__ == "__main__":
    main()
