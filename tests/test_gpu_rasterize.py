"""GPU: cpx_rasterize_polygons / cpx_ids_to_classes (csrc/cpx_rasterize.hip) against the exact-integer CPU statement of the rule
(tests/rasterize_reference.py): EQUALITY of every pixel, no tolerance.  Every coordinate is a multiple of 1/16, where the
kernel's float64 predicate is exact.  Every case runs twice into fresh maps and the two runs are compared bit for bit; the maps
carry a sentinel-filled guard image on either side, which no call may touch.

The shared cases put rings on both sides of what the kernel's decomposition has: the wave (64), the small-ring limits (256
vertices, 4096 box pixels), the edge chunk of the large-ring path (512), box sides of 1 / 63 / 64 / 65 / 129.  The last test closes
the loop with the device polygoniser: cells -> rings -> cells."""
import numpy as np
import pytest
import torch
from scipy import ndimage

import rasterize_reference as rr
from classpose_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 0x5A5A5A5A


def _device(cuda, xy, off, val, shape, img=None, n_images=1, base=None, as_tensors=False):
    """ops.rasterize_polygons twice into fresh, guarded maps -> the (n_images, H, W) result of the first run"""
    H, W = shape
    runs = []
    for _ in range(2):
        buf = torch.full((n_images + 2, H, W), GUARD, dtype=torch.int32, device=cuda)
        out = buf[1:n_images + 1]
        out.copy_(torch.zeros_like(out) if base is None else torch.from_numpy(base).to(cuda))
        args = [xy, off, val]
        if as_tensors:
            args = [torch.from_numpy(a).to(cuda) for a in args]
            img_arg = None if img is None else torch.from_numpy(img).to(cuda)
        else:
            img_arg = img
        res = ops.rasterize_polygons(*args, shape, ring_image=img_arg, n_images=n_images, out=out)
        torch.cuda.synchronize()
        assert res.data_ptr() == out.data_ptr()
        host = buf.cpu().numpy()
        assert (host[0] == GUARD).all() and (host[-1] == GUARD).all(), "written outside the maps"
        runs.append(host[1:-1].copy())
    assert np.array_equal(runs[0], runs[1]), "two runs differ"
    return runs[0]


@pytest.mark.parametrize("name", list(rr.CASES))
def test_device_equals_exact_rule(cuda, name):
    rings, shape = rr.CASES[name]
    xy, off, val, _ = rr.pack(rings, values=[7] * len(rings))
    want = rr.rasterize(xy, off, val, shape)
    got = _device(cuda, xy, off, val, shape)
    assert np.array_equal(got, want), f"{int((got != want).sum())} pixels differ"
    if name.startswith(("two_vertices", "outside")):
        assert not got.any()
    elif name == "collinear":
        assert np.argwhere(got[0]).tolist() == [[i, i] for i in range(3, 21)]
    else:
        assert got.any()


def test_closed_equals_unclosed_and_device_resident_arguments(cuda):
    a = rr.pack(rr.SINGLE["triangle"])
    b = rr.pack(rr.SINGLE["triangle_closed"])
    ma, mb = _device(cuda, *a[:3], rr.SHAPE), _device(cuda, *b[:3], rr.SHAPE, as_tensors=True)
    assert np.array_equal(ma, mb) and ma.any()


# ---- painter's order -----------------------------------------------------------------------------------------------------------
def test_later_feature_wins_multipolygon_hole_and_three_images(cuda):
    sq = lambda x, y, s: [(x, y), (x + s, y), (x + s, y + s), (x, y + s)]
    rings = [sq(4, 4, 20), sq(14, 14, 20),                               # features 1, 2 overlap: 2 wins
             sq(40, 4, 6), sq(50.5, 4.25, 8),                            # feature 3: a MultiPolygon of two parts
             sq(40, 30, 20), sq(45, 35, 10),                             # feature 4: a shell and its hole -- both paint
             rr.star(300, 30.5, 30.25, 29.0, 11.0),                      # feature 5, a large-path ring under everything later
             sq(2, 50, 9)]                                               # feature 6 over the star
    values = [1, 2, 3, 3, 4, 4, 5, 6]
    images = [0, 0, 1, 1, 2, 2, 0, 0]
    xy, off, val, img = rr.pack(rings, values, images)
    want = rr.rasterize(xy, off, val, (64, 72), img, 3)
    got = _device(cuda, xy, off, val, (64, 72), img, 3)
    assert np.array_equal(got, want)
    assert got[0, 20, 20] == 2 and got[0, 30, 30] == 5 and got[0, 5, 22] == 1 and got[0, 55, 5] == 6
    assert set(np.unique(got[1])) == {0, 3} and got[1, 8, 54] == 3
    assert got[2, 40, 50] == 4 and set(np.unique(got[2])) == {0, 4}          # the hole is filled
    # the same rings in reversed order give the same maps: the maximum decides, not the order of the work
    order = np.arange(len(rings))[::-1]
    xy2, off2, val2, img2 = rr.pack([rings[i] for i in order], [values[i] for i in order], [images[i] for i in order])
    assert np.array_equal(_device(cuda, xy2, off2, val2, (64, 72), img2, 3), want)
    # ring_image = None is image 0
    xy3, off3, val3, _ = rr.pack(rings[:2], values[:2])
    assert np.array_equal(_device(cuda, xy3, off3, val3, (64, 72))[0], rr.rasterize(xy3, off3, val3, (64, 72))[0])


def test_second_call_composes_onto_a_nonzero_map(cuda):
    rng = np.random.default_rng(3)
    base = rng.integers(0, 6, (2, 48, 56)).astype(np.int32)
    rings = [rr.TRIANGLE, rr.SINGLE["concave_u"][0], rr.star(280, 27.5, 24.25, 22.0, 9.0)]
    xy, off, val, img = rr.pack(rings, [3, 9, 4], [0, 1, 1])
    want = rr.rasterize(xy, off, val, (48, 56), img, 2, out=base)
    got = _device(cuda, xy, off, val, (48, 56), img, 2, base=base)
    assert np.array_equal(got, want)
    assert (got >= base).all() and (got != base).any() and (got[0][base[0] > 3] == base[0][base[0] > 3]).all()


def test_no_rings_is_a_no_op(cuda):
    out = torch.full((1, 8, 8), 5, dtype=torch.int32, device=cuda)
    res = ops.rasterize_polygons(np.zeros((0, 2)), np.zeros(1, np.int64), np.zeros(0, np.int32), (8, 8), out=out)
    assert res is out and (out == 5).all().item()
    assert not ops.rasterize_polygons(np.zeros((0, 2)), np.zeros(1, np.int64), np.zeros(0, np.int32), (8, 8), device=cuda).any().item()
    with pytest.raises(ValueError, match="NaN"):
        ops.rasterize_polygons(torch.full((3, 2), float("nan"), dtype=torch.float64, device=cuda), torch.tensor([0, 3], device=cuda),
                               torch.ones(1, dtype=torch.int32, device=cuda), (8, 8))
    with pytest.raises(ValueError, match="> 0"):
        ops.rasterize_polygons(torch.zeros((3, 2), dtype=torch.float64, device=cuda), torch.tensor([0, 3], device=cuda),
                               torch.zeros(1, dtype=torch.int32, device=cuda), (8, 8))


def test_ids_to_classes_is_a_table_lookup(cuda):
    rng = np.random.default_rng(11)
    n_ids = 1000
    inst = rng.integers(0, n_ids + 1, (3, 37, 53)).astype(np.int32)
    inst[0, 0, 0], inst[0, 0, 1] = 0, n_ids
    table = rng.integers(0, 256, n_ids + 1).astype(np.uint8)
    table[0], table[n_ids] = 0, 255
    d = torch.from_numpy(inst).to(cuda)
    got = ops.ids_to_classes(d, table)
    assert got.dtype == torch.uint8 and got.shape == d.shape
    assert np.array_equal(got.cpu().numpy(), table[inst]) and got[0, 0, 1].item() == 255 and got[0, 0, 0].item() == 0
    assert np.array_equal(ops.ids_to_classes(d, torch.from_numpy(table).to(cuda)).cpu().numpy(), table[inst])
    assert np.array_equal(ops.ids_to_classes(d, table).cpu().numpy(), got.cpu().numpy())
    with pytest.raises(ValueError, match="ids span"):
        ops.ids_to_classes(d, table[:-1])
    with pytest.raises(ValueError, match="ids span"):
        ops.ids_to_classes(-d, table)


# ---- the round trip with the polygoniser -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cell_maps():
    return np.stack([rr.ragged_cells(seed) for seed in (0, 1, 2)])


def _filled(maps, kept):
    """per map: binary_fill_holes of every kept label's mask, painted with the label"""
    want = np.zeros(maps.shape, np.int32)
    for t, labels in enumerate(kept):
        for l in labels:
            want[t][ndimage.binary_fill_holes(maps[t] == l)] = l
    return want


def test_round_trip_with_the_polygoniser(cuda, cell_maps):
    """cells -> device polygoniser at scale 1 -> rings -> device rasteriser: every cell the polygoniser keeps comes back as
    binary_fill_holes of its mask, exactly.  The same is asserted first for the CPU pair (oracle.polygons.post_process_tile and
    the exact rasteriser); at least 80 % of the cells must be kept, so dropping them cannot pass."""
    import polygon_shapes as ps
    from oracle import polygons as opoly
    from test_gpu_polygons_edges import _poly
    nT, H, W = cell_maps.shape
    n_cells = sum(int(m.max()) for m in cell_maps)
    assert n_cells >= 250
    # the CPU pair
    rings, values, images, kept_cpu = [], [], [], []
    for t in range(nT):
        cells = opoly.post_process_tile(cell_maps[t].astype(np.int32), None, (0.0, 0.0), 1.0)
        kept_cpu.append([c["label"] for c in cells])
        for c in cells:
            rings.append(c["coords"]); values.append(c["label"]); images.append(t)
    xy, off, val, img = rr.pack(rings, values, images)
    cpu = rr.rasterize(xy, off, val, (H, W), img, nT)
    n_cpu = sum(len(k) for k in kept_cpu)
    assert np.array_equal(cpu, _filled(cell_maps, kept_cpu))
    # the device pair
    recs = [ps.records(m) for m in cell_maps]
    res = _poly(cuda, cell_maps, recs)
    d_rings, d_values, d_images, kept_dev = [], [], [], []
    for t in range(nT):
        keep = [(int(r["label"]), c) for r, c in zip(recs[t], res.tiles[t]) if c["valid"] and c["n_pts"] >= 4]
        kept_dev.append([l for l, _ in keep])
        for l, c in keep:
            d_rings.append(res.xy[c["offset"]:c["offset"] + c["n_pts"]]); d_values.append(l); d_images.append(t)
    n_dev = sum(len(k) for k in kept_dev)
    print(f"round trip: {n_cells} cells, the CPU pair keeps {n_cpu}, the device pair {n_dev}")
    assert kept_dev == kept_cpu
    assert n_cpu >= 0.8 * n_cells and n_dev >= 0.8 * n_cells
    dxy, doff, dval, dimg = rr.pack(d_rings, d_values, d_images)
    got = _device(cuda, dxy, doff, dval, (H, W), dimg, nT)
    assert np.array_equal(got, _filled(cell_maps, kept_dev))
    assert np.array_equal(got, cpu)
