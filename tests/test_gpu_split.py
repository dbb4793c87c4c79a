"""Splitting touching cells on the device (csrc/cpx_split.hip -> ops.distance_sq / ops.split_touching ->
dataset_stats.instances_from_classes(split_touching=True) -> train_head --split_touching_cells).  The distance map, the seed lists,
the labels and the counts must EQUAL the CPU restatement of the rule (tests/split_reference.py) on every pixel; there is no
tolerance.  The outcome of the scenes is proven on the CPU by tests/test_split_host.py."""
import argparse

import numpy as np
import pytest
import torch

import split_reference as sr

pytestmark = pytest.mark.gpu


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} pixels differ, first at (image, row, col) {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}" if len(bad) else ""


def _split(maps: np.ndarray, dev, *params, **kw):
    from classpose_amd import ops
    src = torch.from_numpy(np.array(maps)).to(dev)
    labels, counts, seeds = ops.split_touching(src, *params, return_seeds=True, **kw)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(labels.shape) == maps.shape and tuple(counts.shape) == maps.shape[:1]
    assert torch.equal(src.cpu(), torch.from_numpy(np.array(maps)))               # the input is only read
    return labels.cpu().numpy(), counts.cpu().numpy(), [s.cpu().numpy() for s in seeds]


@pytest.mark.parametrize("name", list(sr.CASES))
def test_distance_map_equals_the_restatement(cuda, name):
    from classpose_amd import ops
    maps = sr.CASES[name]
    src = torch.from_numpy(np.array(maps)).to(cuda)
    got = ops.distance_sq(src)
    assert got.dtype == torch.int32 and tuple(got.shape) == maps.shape
    got = got.cpu().numpy()
    want = sr.expected(name)[3]
    assert np.array_equal(got, want), _first_difference(got, want)
    assert torch.equal(src.cpu(), torch.from_numpy(np.array(maps)))
    if name.startswith("size_"):
        H, W = maps.shape[1:]
        assert (got[1] == H * H + W * W).all()                                   # one instance fills the image: no site at all


@pytest.mark.parametrize("min_distance,min_radius", sr.PARAMETERS)
@pytest.mark.parametrize("name", list(sr.CASES))
def test_seeds_labels_and_counts_equal_the_restatement(cuda, name, min_distance, min_radius):
    for connectivity in (8, 4):
        want, want_counts, want_seeds, _d2 = sr.expected(name, min_distance, min_radius, connectivity)
        got, counts, seeds = _split(sr.CASES[name], cuda, min_distance, min_radius, connectivity)
        print(f"{name} d={min_distance} r={min_radius} c={connectivity}: counts {counts.tolist()}, reference {want_counts.tolist()}, "
              f"seeds {[len(s) for s in seeds]}")
        for k, (s, w) in enumerate(zip(seeds, want_seeds)):
            assert s.dtype == np.int32 and np.array_equal(s, w), (k, s.tolist()[:16], w.tolist()[:16])
        assert np.array_equal(counts, want_counts), (counts.tolist(), want_counts.tolist())
        assert np.array_equal(got, want), _first_difference(got, want)


def test_the_scenes_reproduce(cuda):
    counts = {name: _split(sr.CASES[name], cuda)[1].tolist() for name in ("two_discs", "ellipse", "disc_grid", "thin", "twin_peaks")}
    assert counts == {"two_discs": [2], "ellipse": [1], "disc_grid": [9], "thin": [2], "twin_peaks": [1]}
    m = sr.CASES["two_discs"][0]
    labels, _counts, seeds = _split(sr.CASES["two_discs"], cuda)
    xs = np.mgrid[:m.shape[0], :m.shape[1]][1]
    assert np.array_equal(labels[0], np.where(m != 0, np.where(xs <= 30, 1, 2), 0))
    assert seeds[0].tolist() == [24 * 60 + 23, 24 * 60 + 37]
    labels, _counts, seeds = _split(sr.CASES["thin"], cuda)
    assert np.array_equal(labels[0], sr.CASES["thin"][0]) and seeds[0].tolist() == [34 * 90 + 3]
    assert _split(sr.CASES["twin_peaks"], cuda)[2][0].tolist() == [9 * 80 + 62]
    assert _split(sr.CASES["twin_peaks_vertical"], cuda)[2][0].tolist() == [62 * 20 + 9]


def test_an_image_splits_alone_as_in_a_batch(cuda):
    batch = sr.CASES["size_130x70"]
    assert np.array_equal(batch[0], sr.CASES["single_130x70"][0])
    for params in ((5, 2, 8), (1, 1, 4)):
        got, counts, seeds = _split(batch, cuda, *params)
        for order in ([2, 0, 1], [0]):
            again, counts2, seeds2 = _split(batch[order], cuda, *params)
            assert np.array_equal(again, got[order]) and np.array_equal(counts2, counts[order])
            assert all(np.array_equal(seeds2[i], seeds[k]) for i, k in enumerate(order))


def _raw_call(src, params, cap, dev, guard=64, stream=None):
    """the entry itself with guard words around every output: (status, n_seeds, labels, counts, seeds) as numpy"""
    from classpose_amd import _lib
    L = _lib.lib()
    n, H, W = src.shape
    need = L.cpx_split_workspace_bytes(n, H, W, cap)
    ws = torch.full((need + guard,), 0xA5, dtype=torch.uint8, device=dev)
    sizes = dict(labels=n * H * W, counts=n, seeds=n * cap, n_seeds=n, status=n)
    bufs = {k: torch.full((guard + v + guard,), -7, dtype=torch.int32, device=dev) for k, v in sizes.items()}
    at = {k: b.data_ptr() + 4 * guard for k, b in bufs.items()}
    torch.cuda.synchronize()
    handle = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream.cuda_stream
    _lib.check(L.cpx_split_touching(src.data_ptr(), n, H, W, *params, cap, at["labels"], at["counts"], at["seeds"], at["n_seeds"],
                                    at["status"], ws.data_ptr(), need, handle), "split_touching")
    torch.cuda.synchronize()
    assert (ws[need:] == 0xA5).all()                                              # nothing behind the bytes it was given
    out = {}
    for k, b in bufs.items():
        h = b.cpu().numpy()
        assert (h[:guard] == -7).all() and (h[-guard:] == -7).all(), k          # nothing written outside an output
        out[k] = h[guard:-guard]
    return out["status"], out["n_seeds"], out["labels"].reshape(n, H, W), out["counts"], out["seeds"].reshape(n, cap)


def test_a_seed_list_that_overflows_voids_its_image_and_the_wrapper_repeats(cuda):
    maps = sr.CASES["size_65x67"]
    want, want_counts, want_seeds, _d2 = sr.expected("size_65x67", 1, 1, 8)
    totals = [len(s) for s in want_seeds]
    assert totals[1] == 1 and totals[0] > 30 and totals[2] > 300
    src = torch.from_numpy(np.array(maps)).to(cuda)
    cap = totals[0]                                                             # fits images 0 and 1 exactly, not image 2
    status, n_seeds, labels, counts, seeds = _raw_call(src, (1, 1, 8), cap, cuda)
    assert status.tolist() == [0, 0, 1] and n_seeds.tolist() == totals           # the true total, also where it does not fit
    assert not labels[2].any() and counts[2] == 0                                # void
    for k in (0, 1):
        assert np.array_equal(labels[k], want[k]) and counts[k] == want_counts[k] and np.array_equal(seeds[k, :totals[k]], want_seeds[k])
    status, n_seeds, labels, counts, seeds = _raw_call(src, (1, 1, 8), max(totals), cuda)
    assert status.tolist() == [0, 0, 0] and np.array_equal(labels, want) and np.array_equal(seeds[2], want_seeds[2])
    for cap in (1, totals[2] - 1):                                               # the wrapper: one repeat with the reported total
        got, counts, seeds = _split(maps, cuda, 1, 1, 8, seed_cap=cap)
        assert np.array_equal(got, want) and np.array_equal(counts, want_counts)
        assert all(np.array_equal(s, w) for s, w in zip(seeds, want_seeds))


def test_an_id_without_a_table_slot_is_refused(cuda):
    from classpose_amd import ops
    maps = np.zeros((2, 5, 6), np.int32)
    maps[0, 1:4, 1:4] = 30                                                      # 30 = H * W: the largest id with a slot
    maps[1, 2, 2] = 31
    src = torch.from_numpy(maps).to(cuda)
    status, _n_seeds, labels, counts, _seeds = _raw_call(src, (5, 2, 8), 30, cuda)
    assert status.tolist() == [0, 2] and counts.tolist() == [1, 0] and np.array_equal(labels[0], (maps[0] != 0).astype(np.int32))
    with pytest.raises(ValueError, match="image 1 has an instance id outside"):
        ops.split_touching(src)
    maps[1, 2, 2] = -4
    with pytest.raises(ValueError, match="image 1 has an instance id outside"):
        ops.split_touching(torch.from_numpy(maps).to(cuda))


def test_two_calls_give_identical_bits_on_any_stream(cuda):
    maps = np.concatenate([sr.CASES["size_130x70"], sr.CASES["seams"][:, :, :70]])
    src = torch.from_numpy(np.array(maps)).to(cuda)
    stream = torch.cuda.Stream(device=cuda)
    first = _raw_call(src, (1, 1, 8), 2048, cuda)
    assert not first[0].any() and first[1].max() > 700
    for st in (None, stream, stream):
        again = _raw_call(src, (1, 1, 8), 2048, cuda, stream=st)
        for a, b in zip(first[:4], again[:4]):
            assert a.tobytes() == b.tobytes()
        for k, total in enumerate(first[1]):
            assert first[4][k, :total].tobytes() == again[4][k, :total].tobytes()
    assert torch.equal(src.cpu(), torch.from_numpy(np.array(maps)))


def test_wrappers_take_empty_batches_and_views(cuda):
    from classpose_amd import ops
    empty = torch.zeros((0, 5, 7), dtype=torch.int32, device=cuda)
    assert tuple(ops.distance_sq(empty).shape) == (0, 5, 7)
    labels, counts, seeds = ops.split_touching(empty, return_seeds=True)
    assert tuple(labels.shape) == (0, 5, 7) and tuple(counts.shape) == (0,) and seeds == []
    full = sr.CASES["seams"]
    view = torch.from_numpy(np.array(full)).to(cuda)[:, 20:120, 40:130]                      # not contiguous
    want = sr.split_image(full[0, 20:120, 40:130])
    got, counts = ops.split_touching(view)
    assert np.array_equal(got.cpu().numpy()[0], want[0]) and int(counts[0]) == want[1]
    assert np.array_equal(ops.distance_sq(view).cpu().numpy()[0], want[3])
    with pytest.raises(ValueError, match="min_distance"):
        ops.split_touching(view, min_distance=0)
    with pytest.raises(ValueError, match="min_radius"):
        ops.split_touching(view, min_radius=0)
    with pytest.raises(ValueError, match="connectivity"):
        ops.split_touching(view, connectivity=6)
    with pytest.raises(ValueError, match="unsupported"):
        ops.distance_sq(torch.zeros((1, 32768, 1), dtype=torch.int32, device=cuda))


# ---- from class maps to statistics -----------------------------------------------------------------------------------------------
def _touching_disc_classes():
    """(2, 96, 130) class maps of touching discs and, built by hand, the instance maps a pathologist would draw:
    image 0: the 3 x 3 grid of class 2 (nine cells, cut on the grid lines), the two discs of class 1 (cut on their bisector) and
    one disc of class 3 alone; image 1: the two discs of class 3 and not-annotated margins."""
    cls = np.zeros((2, 96, 130), np.int16)
    true = np.zeros((2, 96, 130), np.int32)
    grid = sr.disc_grid()                                                       # 67 x 67
    ys, xs = np.mgrid[:67, :67]
    cells = np.where(grid != 0, 1 + 3 * np.clip((ys - 4) // 20, 0, 2) + np.clip((xs - 4) // 20, 0, 2), 0)
    cls[0, 2:69, 1:68] = grid * 2
    true[0, 2:69, 1:68] = cells
    pair = sr.two_discs(H=24, W=38, cy=12, cx=11)                               # centres at columns 11 and 25: the cut is after 18
    halves = np.where(pair != 0, np.where(np.mgrid[:24, :38][1] <= 18, 10, 11), 0)
    cls[0, 70:94, 5:43] = pair
    true[0, 70:94, 5:43] = halves
    sr.disc(cls[0], 40, 100, 12, 3)
    true[0][cls[0] == 3] = 12
    cls[1, 30:54, 50:88] = pair * 3
    true[1, 30:54, 50:88] = halves
    cls[1, :8] = -100
    cls[1, :, 120:] = -100
    return cls, true


def test_class_maps_of_touching_discs_give_the_true_statistics(cuda):
    from classpose_amd import dataset_stats as ds
    cls, true = _touching_disc_classes()
    ncls = 4
    want = ds.label_stats(true, cls, ncls, device=cuda)
    assert want.n_masks.tolist() == [12, 2]
    merged, merged_counts = ds.instances_from_classes(cls, device=cuda)
    assert merged_counts.tolist() == [3, 1]                                      # what the labeller alone makes of them
    inst, counts = ds.instances_from_classes(cls, device=cuda, split_touching=True, chunk=1)
    assert inst.dtype == torch.int32 and inst.is_cuda and counts.dtype == np.int64 and counts.tolist() == [12, 2]
    assert np.array_equal(sr.partition_id(inst.cpu().numpy()[0]), sr.partition_id(true[0]))
    assert np.array_equal(sr.partition_id(inst.cpu().numpy()[1]), sr.partition_id(true[1]))
    got = ds.label_stats(inst, cls, ncls, device=cuda)
    assert np.array_equal(got.n_masks, want.n_masks) and np.array_equal(got.diameters, want.diameters)
    assert np.array_equal(got.instance_counts, want.instance_counts) and np.array_equal(got.class_counts, want.class_counts)
    assert ds.split_summary(merged, inst) == (4, 3, 14)
    off, off_counts = ds.instances_from_classes(cls, device=cuda, split_touching=False)
    assert torch.equal(off, merged) and off_counts.tolist() == [3, 1]
    # label_stats(label_instances=True): merged ids in, the cut applied before the instances are counted
    plain = ds.label_stats(merged, cls, ncls, device=cuda, label_instances=True, connectivity=4)
    cut = ds.label_stats(merged, cls, ncls, device=cuda, label_instances=True, connectivity=4, split_touching=True)
    assert plain.instance_counts[:, 1:].tolist() == [[1, 1, 1], [0, 0, 1]] and cut.instance_counts[:, 1:].tolist() == [[2, 9, 1], [0, 0, 2]]
    assert np.array_equal(cut.instance_counts, want.instance_counts)
    assert np.array_equal(cut.n_masks, plain.n_masks) and np.array_equal(cut.diameters, plain.diameters)


def test_train_head_derives_split_instances_and_reports_them(cuda, monkeypatch):
    from classpose_amd import dataset_stats as ds
    from classpose_amd.entrypoints import train_head
    cls, true = _touching_disc_classes()
    said = []
    monkeypatch.setattr(train_head.logger, "info", lambda msg, *a, **k: said.append(str(msg)))
    args = argparse.Namespace(device="cuda:0", instance_connectivity=None, split_touching_cells=True, split_min_distance=None,
                              split_min_radius=None)
    inst = train_head._derive_instances(cls, args, "--labels")
    assert torch.equal(inst, ds.instances_from_classes(cls, device=cuda, split_touching=True)[0])
    assert any("cut 3 of 4 components into pieces, 14 instances in all (min_distance 5, min_radius 2)" in s for s in said), said
    del said[:]
    args.split_touching_cells = False
    assert torch.equal(train_head._derive_instances(cls, args, "--labels"), ds.instances_from_classes(cls, device=cuda)[0])
    assert len(said) == 1 and "derived 4 instances from 2 class maps" in said[0]
    args.split_touching_cells, args.split_min_distance, args.split_min_radius = True, 30, 2
    wide = train_head._derive_instances(cls, args, "--labels")                  # a window wider than a cell: the grid's rows merge
    assert int(wide.max()) < 12 and any("min_distance 30" in s for s in said)


def test_train_head_with_split_cells_trains_as_with_the_split_maps_given(cuda, tmp_path, monkeypatch):
    import components_reference as cr
    from classpose_amd import dataset_stats as ds, synth, train
    from classpose_amd.entrypoints import train_head
    ncls = 5
    torch.save(synth.make_state_dict(1, None, depth=1, seed=12), tmp_path / "backbone.pt")
    ims = np.stack([synth.render_region(300, 256 * k, 0, 256, 256) for k in range(4)])
    labs = np.stack([cr._blobs((256, 256), 700 + k, 25, nval=4) for k in range(4)]).astype(np.int16)
    labs[:, 250:] = -100
    np.save(tmp_path / "X.npy", ims)
    np.save(tmp_path / "Y.npy", labs)
    merged, merged_counts = ds.instances_from_classes(labs, device=cuda)
    derived, counts = ds.instances_from_classes(labs, device=cuda, split_touching=True, min_distance=7)
    assert counts.sum() > merged_counts.sum()                                    # overlapping discs of one class: some are cut
    np.save(tmp_path / "I.npy", derived.cpu().numpy())
    losses, said, warned = [], [], []
    real = train.train_class_head

    def recording(*a, **kw):
        out = real(*a, **kw)
        losses.append(np.asarray(out[1], np.float64))
        return out
    monkeypatch.setattr(train, "train_class_head", recording)
    info, warning = train_head.logger.info, train_head.logger.warning
    monkeypatch.setattr(train_head.logger, "info", lambda msg, *a, **k: (said.append(str(msg)), info(msg, *a, **k))[1])
    monkeypatch.setattr(train_head.logger, "warning", lambda msg, *a, **k: (warned.append(str(msg)), warning(msg, *a, **k))[1])
    common = ["--images", str(tmp_path / "X.npy"), "--labels", str(tmp_path / "Y.npy"), "--pretrained_model", str(tmp_path / "backbone.pt"),
              "--nclasses", str(ncls), "--n_epochs", "2", "--batch_size", "2", "--learning_rate", "1e-3", "--auto_class_weights",
              "--oversampling_method", "custom", "--rescale", "--augment", "geometry", "--train_flow_head", "--device", "cuda:0"]
    parser = train_head.build_parser()
    train_head.main(parser.parse_args(common + ["--instances_from_labels", "--split_touching_cells", "--split_min_distance", "7",
                                                "--save_path", str(tmp_path / "a"), "--model_name", "m"]))
    n_comp, n_split, n_inst = ds.split_summary(merged, derived)
    assert n_split > 0 and any(f"cut {n_split} of {n_comp} components into pieces, {n_inst} instances in all (min_distance 7, min_radius 2)" in s
                               for s in said), said
    assert not any("merge into one instance" in s for s in warned)
    train_head.main(parser.parse_args(common + ["--instances", str(tmp_path / "I.npy"), "--save_path", str(tmp_path / "b"), "--model_name", "m"]))
    assert len(losses) == 2 and len(losses[0]) == 2 and np.all(np.isfinite(losses[0]))
    assert losses[0].tobytes() == losses[1].tobytes(), (losses[0].tolist(), losses[1].tolist())
    cka = torch.load(tmp_path / "a" / "m" / "m", map_location="cpu", weights_only=True)
    ckb = torch.load(tmp_path / "b" / "m" / "m", map_location="cpu", weights_only=True)
    assert torch.equal(cka["out.weight"], ckb["out.weight"]) and torch.equal(cka["out_class.weight"], ckb["out_class.weight"])
    del warned[:]
    train_head.main(parser.parse_args(common + ["--instances_from_labels", "--n_epochs", "1", "--save_path", str(tmp_path / "c"), "--model_name", "m"]))
    assert any("touching cells of one class merge into one instance" in s for s in warned)       # without the flag: the old warning
