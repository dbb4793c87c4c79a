"""Connected-component labelling on the device (csrc/cpx_components.hip -> ops.label_components -> dataset_stats.instances_from_classes /
label_stats(label_instances=True) -> train_head --instances_from_labels).  Every pixel and every count must EQUAL the CPU statement
of the rule (tests/components_reference.py: scipy per value, renumbered explicitly by first raster index); there is no tolerance."""
import numpy as np
import pytest
import torch

import components_reference as cr

pytestmark = pytest.mark.gpu


def _run(maps: np.ndarray, connectivity: int, dev, **kw):
    from classpose_amd import ops
    labels, counts = ops.label_components(torch.from_numpy(np.array(maps)).to(dev), connectivity, **kw)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int32 and counts.dtype == torch.int32 and tuple(labels.shape) == maps.shape and tuple(counts.shape) == maps.shape[:1]
    return labels.cpu().numpy(), counts.cpu().numpy()


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} pixels differ, first at (image, row, col) {bad[0].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}" if len(bad) else ""


@pytest.mark.parametrize("connectivity", [4, 8])
@pytest.mark.parametrize("name", list(cr.CASES))
def test_labels_and_counts_equal_the_reference(cuda, name, connectivity):
    want, want_counts = cr.expected(name, connectivity)
    got, counts = _run(cr.CASES[name], connectivity, cuda)
    print(f"{name} {connectivity}: counts {counts.tolist()[:8]}, reference {want_counts.tolist()[:8]}")
    assert np.array_equal(counts, want_counts), (counts.tolist(), want_counts.tolist())
    assert np.array_equal(got, want), _first_difference(got, want)
    if name in cr.KNOWN_COUNTS:
        assert counts.tolist() == cr.KNOWN_COUNTS[name][connectivity]


def test_batch_numbering_restarts_in_every_image(cuda):
    maps = cr.CASES["batch5"]
    for connectivity in (4, 8):
        got, counts = _run(maps, connectivity, cuda)
        assert counts.tolist() == [0, 1, 7, 4000, 1]
        for k in range(5):
            assert got[k].max() == counts[k] and np.array_equal(np.unique(got[k][maps[k] != 0]), np.arange(1, counts[k] + 1))
            assert not got[k][maps[k] == 0].any()
        # an image labels the same alone as inside the batch, wherever it stands in it
        order = [3, 0, 4, 2, 1]
        again, counts2 = _run(maps[order], connectivity, cuda)
        assert np.array_equal(again, got[order]) and np.array_equal(counts2, counts[order])
        alone, c1 = _run(maps[3:4], connectivity, cuda)
        assert np.array_equal(alone[0], got[3]) and c1.tolist() == [4000]


def test_rasterised_cell_field(cuda):
    from classpose_amd import ops
    xy, off, val = cr.cell_field(11, 512, 300)
    inst = ops.rasterize_polygons(xy, off, val, (512, 512), device=cuda)
    host = inst.cpu().numpy()
    assert host.max() == 300 and len(np.unique(host)) > 250                       # overlapping cells: later ids cover earlier ones
    for connectivity in (4, 8):
        labels, counts = ops.label_components(inst, connectivity)
        want, n = cr.label_scipy(host[0], connectivity)
        assert int(counts[0]) == n >= len(np.unique(host)) - 1                    # a covered cell may fall apart, none can merge
        got = labels.cpu().numpy()[0]
        assert np.array_equal(got, want), _first_difference(got[None], want[None])


def test_reproducible_on_a_second_stream_and_nothing_written_outside(cuda):
    from classpose_amd import _lib
    maps = np.concatenate([cr.CASES["random_density_05"][:3], cr.CASES["size_300x520"][:, :200, :333]])
    want = np.stack([cr.label_scipy(m, 8)[0] for m in maps])
    n, H, W = maps.shape
    L = _lib.lib()
    need = L.cpx_label_components_workspace_bytes(n, H, W)
    guard = 64
    src = torch.from_numpy(np.array(maps)).to(cuda)
    stream = torch.cuda.Stream(device=cuda)
    results = []
    ws_exact = torch.empty(need, dtype=torch.uint8, device=cuda)
    ws_large = torch.full((need + 4096 + guard,), 0xFF, dtype=torch.uint8, device=cuda)
    for ws, ws_bytes in ((ws_exact, need), (ws_exact, need), (ws_large, need + 4096)):
        out = torch.full((guard + n * H * W + guard,), -7, dtype=torch.int32, device=cuda)
        cnt = torch.full((guard + n + guard,), -7, dtype=torch.int32, device=cuda)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            _lib.check(L.cpx_label_components(src.data_ptr(), n, H, W, 8, out.data_ptr() + 4 * guard, cnt.data_ptr() + 4 * guard,
                                              ws.data_ptr(), ws_bytes, stream.cuda_stream), "label_components")
        stream.synchronize()
        o, c = out.cpu().numpy(), cnt.cpu().numpy()
        assert (o[:guard] == -7).all() and (o[-guard:] == -7).all() and (c[:guard] == -7).all() and (c[-guard:] == -7).all()
        results.append((o[guard:-guard].reshape(n, H, W), c[guard:-guard]))
    assert (ws_large[need + 4096:] == 0xFF).all()                                 # nothing behind the bytes it was given
    assert torch.equal(src.cpu(), torch.from_numpy(np.array(maps)))   # the input is only read
    for o, c in results:
        assert np.array_equal(o, want) and np.array_equal(c, want.reshape(n, -1).max(1))
        assert o.tobytes() == results[0][0].tobytes() and c.tobytes() == results[0][1].tobytes()


def test_wrapper_reuses_a_workspace_and_takes_an_empty_batch(cuda):
    from classpose_amd import _lib, ops
    maps = cr.CASES["touching"]
    need = _lib.lib().cpx_label_components_workspace_bytes(*maps.shape)
    ws = torch.empty(need + 100, dtype=torch.uint8, device=cuda)
    a = _run(maps, 4, cuda, workspace=ws)
    b = _run(maps, 4, cuda, workspace=torch.empty(8, dtype=torch.uint8, device=cuda))        # too small: replaced inside
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], cr.expected("touching", 4)[0])
    labels, counts = ops.label_components(torch.zeros((0, 5, 7), dtype=torch.int32, device=cuda))
    assert tuple(labels.shape) == (0, 5, 7) and tuple(counts.shape) == (0,)
    view = torch.from_numpy(np.array(cr.CASES["size_300x520"])).to(cuda)[:, 10:200, 7:300]       # not contiguous
    got, _ = ops.label_components(view, 8)
    assert np.array_equal(got.cpu().numpy()[1], cr.label_scipy(cr.CASES["size_300x520"][1, 10:200, 7:300], 8)[0])


def _class_maps():
    """(6, 256, 256) class maps of 4 classes: discs, some touching, with regions that are not annotated (-100)"""
    maps = np.stack([cr._blobs((256, 256), 900 + k, 45, nval=4) for k in range(6)]).astype(np.int16)
    for k in range(6):
        maps[k, (30 + 37 * k) % 220:][:20] = -100
        maps[k, 100:140, 10 * k:10 * k + 25] = -100
    return maps


def test_instances_from_classes_partition(cuda):
    from classpose_amd import dataset_stats as ds
    classes = _class_maps()
    inst, counts = ds.instances_from_classes(classes, device=cuda, chunk=4)                     # two chunks: 4 + 2
    assert inst.dtype == torch.int32 and inst.is_cuda and tuple(inst.shape) == classes.shape and counts.dtype == np.int64
    got = inst.cpu().numpy()
    for k in range(6):
        want, n = cr.label_scipy(np.maximum(classes[k], 0), 4)
        assert counts[k] == n and np.array_equal(got[k], want), k
        assert not got[k][classes[k] <= 0].any()
    inst8, counts8 = ds.instances_from_classes(torch.from_numpy(classes).to(cuda), connectivity=8, device=cuda)
    assert (counts8 <= counts).all() and counts8.sum() < counts.sum()
    assert np.array_equal(inst8.cpu().numpy()[2], cr.label_scipy(np.maximum(classes[2], 0), 8)[0])


def test_label_stats_with_relabelled_instances(cuda):
    from classpose_amd import dataset_stats as ds, train_data
    ncls = 4
    inst = np.zeros((3, 96, 130), np.int32)
    cls = np.zeros((3, 96, 130), np.int16)
    inst[0, 5:15, 5:15] = 7; inst[0, 40:50, 60:70] = 7; cls[0, 5:15, 5:15] = 1; cls[0, 40:50, 60:70] = 1       # one id, two blobs
    inst[0, 60:80, 10:40] = 3; cls[0, 60:80, 10:25] = 2; cls[0, 60:80, 25:40] = 3                              # one blob, two classes
    inst[1, 10:20, 10:20] = 1; inst[1, 20:30, 20:30] = 1; cls[1, 10:30, 10:30] = 2                             # corner contact: one 8-connected
    inst[1, 50:60, 50:60] = 5; cls[1, 50:60, 50:60] = 3
    inst[2, 0:4, :] = 9; inst[2, 8:12, :] = 9; inst[2, 16:20, :] = 9; cls[2, 0:20, :] = 1; cls[2, 90:, :] = -100
    plain = ds.label_stats(inst, cls, ncls, device=cuda)
    for connectivity in (8, 4):
        st = ds.label_stats(inst, cls, ncls, device=cuda, label_instances=True, connectivity=connectivity, chunk=2)
        want = cr.instance_counts_relabelled(inst, cls, ncls, connectivity)
        assert np.array_equal(st.instance_counts, want), (st.instance_counts, want)
        assert np.array_equal(st.class_counts, plain.class_counts) and np.array_equal(st.n_masks, plain.n_masks)
        assert np.array_equal(st.diameters, plain.diameters)
    want8 = cr.instance_counts_relabelled(inst, cls, ncls, 8)
    assert not np.array_equal(want8, plain.instance_counts) and not np.array_equal(want8, cr.instance_counts_relabelled(inst, cls, ncls, 4))
    assert want8[0].tolist() == [1, 2, 1, 1] and plain.instance_counts[0].tolist() == [1, 1, 1, 1]
    assert ds.label_stats(inst, cls, ncls, device=cuda).instance_counts.tolist() == plain.instance_counts.tolist()        # default: off
    rag = train_data.ragged_label_stats(list(inst), list(cls), ncls, device=cuda, label_instances=True)
    assert np.array_equal(rag.instance_counts, want8)


def test_train_head_from_class_only_maps_end_to_end(cuda, tmp_path, monkeypatch):
    from classpose_amd import dataset_stats as ds, synth, train
    from classpose_amd.entrypoints import train_head
    ncls = 5
    torch.save(synth.make_state_dict(1, None, depth=1, seed=12), tmp_path / "backbone.pt")
    ims = np.stack([synth.render_region(300, 256 * k, 0, 256, 256) for k in range(4)])
    labs = np.stack([cr._blobs((256, 256), 700 + k, 25, nval=4) for k in range(4)]).astype(np.int16)
    labs[:, 250:] = -100
    np.save(tmp_path / "X.npy", ims)
    np.save(tmp_path / "Y.npy", labs)
    derived, counts = ds.instances_from_classes(labs, device=cuda)
    assert counts.min() >= 3
    np.save(tmp_path / "I.npy", derived.cpu().numpy())
    losses = []
    real = train.train_class_head

    def recording(*a, **kw):
        out = real(*a, **kw)
        losses.append(np.asarray(out[1], np.float64))
        return out
    monkeypatch.setattr(train, "train_class_head", recording)
    common = ["--images", str(tmp_path / "X.npy"), "--labels", str(tmp_path / "Y.npy"), "--pretrained_model", str(tmp_path / "backbone.pt"),
              "--nclasses", str(ncls), "--n_epochs", "2", "--batch_size", "2", "--learning_rate", "1e-3", "--auto_class_weights",
              "--oversampling_method", "custom", "--rescale", "--augment", "geometry", "--train_flow_head", "--device", "cuda:0"]
    parser = train_head.build_parser()
    train_head.main(parser.parse_args(common + ["--instances_from_labels", "--save_path", str(tmp_path / "a"), "--model_name", "m"]))
    train_head.main(parser.parse_args(common + ["--instances", str(tmp_path / "I.npy"), "--save_path", str(tmp_path / "b"), "--model_name", "m"]))
    assert len(losses) == 2 and len(losses[0]) == 2 and np.all(np.isfinite(losses[0]))
    assert losses[0].tobytes() == losses[1].tobytes(), (losses[0].tolist(), losses[1].tolist())
    cka = torch.load(tmp_path / "a" / "m" / "m", map_location="cpu", weights_only=True)
    ckb = torch.load(tmp_path / "b" / "m" / "m", map_location="cpu", weights_only=True)
    assert cka["out.weight"].shape == (192, 256, 1, 1) and cka["out_class.weight"].shape[0] == ncls * 64
    assert torch.equal(cka["out.weight"], ckb["out.weight"]) and torch.equal(cka["out_class.weight"], ckb["out_class.weight"])
