"""CPU: the host side of the per-cell class confidence (--cell_confidence): the numpy reference on hand-built maps, the
measurement formulas, the native GeoJSON writer with extra measurements, the parsers, and the way the confidence rows travel
through the tile loop's ordering, selection and exchange."""
import ctypes as C
import json
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import cell_confidence_reference as ref
from classpose_amd import _lib, confidence, geojson, parallel

Q = 1 << 24


# ---- the reference, on maps small enough to work out by hand ------------------------------------------------------------------
def test_reference_on_hand_built_maps():
    # one 2 x 3 tile, two cells: label 1 = pixels 0, 1, 3; label 2 = pixel 2; pixels 4, 5: background and an id past rec_counts
    masks = np.array([[[1, 1, 2], [1, 0, 3]]], np.uint16)
    ln3 = np.float32(np.log(3.0))
    lg = np.zeros((1, 2, 2, 3), np.float32)
    lg[0, :, 0, 0] = [0.0, 0.0]               # p = (1/2, 1/2); the first maximum wins: votes class 0
    lg[0, :, 0, 1] = [ln3, 0.0]               # p = (3/4, 1/4) up to the float32 rounding of ln 3
    lg[0, :, 1, 0] = [-80.0, 80.0]            # p = (0, 1) exactly: exp(-160) / (1 + exp(-160)) rounds to 0 quanta
    lg[0, :, 0, 2] = [np.nan, 5.0]            # a NaN beats every number: votes class 0, adds nothing to the sums
    lg[0, :, 1, 2] = [9.0, 9.0]               # id 3 > rec_counts = 2: background
    cp = np.zeros((1, 2, 3), np.float32)
    cp[0, 0, 1] = 80.0                        # sigmoid = 1 exactly in float64 (1 + exp(-80) == 1)
    cp[0, 1, 0] = np.inf                      # non-finite: adds 0
    cp[0, 0, 2] = -np.float32(np.log(3.0))    # sigmoid = 1/4 up to rounding
    votes, prob_q, cellprob_q, valid = ref.instance_confidence(masks, lg, cp, [2], 4)
    assert valid.tolist() == [[True, True, False, False]]
    assert votes[0].tolist() == [[2, 1], [1, 0], [0, 0], [0, 0]]
    e3 = np.exp(np.float64(ln3))
    q34, q14 = int(np.rint(e3 / (e3 + 1.0) * Q)), int(np.rint(1.0 / (e3 + 1.0) * Q))
    assert abs(q34 - 3 * Q // 4) <= 1 and abs(q14 - Q // 4) <= 1
    assert prob_q[0].tolist() == [[Q // 2 + q34 + 0, Q // 2 + q14 + Q], [0, 0], [0, 0], [0, 0]]
    assert cellprob_q[0].tolist() == [Q // 2 + Q + 0, q14, 0, 0]          # label 1: sigmoid(0), sigmoid(80), inf -> 0
    # round half to even on the quantum: p * 2^24 = k + 0.5 goes to the even neighbour
    assert ref.softmax_q(np.array([[0.0], [0.0]], np.float32)).tolist() == [[Q // 2], [Q // 2]]
    assert np.rint(np.array([0.5, 1.5, 2.5])).tolist() == [0.0, 2.0, 2.0]
    # two +inf logits: the first wins the vote, nothing is added
    z = np.array([[1.0], [np.inf], [np.inf]], np.float32)
    assert int(np.argmax(z, 0)[0]) == 1 and ref.softmax_q(z).sum() == 0
    # max_rec below rec_counts: ids above max_rec are background
    v2, p2, c2, ok2 = ref.instance_confidence(masks, lg, cp, [2], 1)
    assert ok2.tolist() == [[True]] and v2[0].tolist() == [[2, 1]] and c2[0].tolist() == [Q // 2 + Q]
    # parts are optional
    v3, p3, c3, _ = ref.instance_confidence(masks, None, cp, [2], 4)
    assert v3.shape == (1, 4, 0) and np.array_equal(c3, cellprob_q)


# ---- measurement formulas -----------------------------------------------------------------------------------------------------------
def test_measurements_names_order_and_values():
    labels = ["tumour", "stroma", 'imm"une']                     # class values 1, 2, 3; value 0 -> labels[-1], like cell_dict
    votes = np.array([[0, 7, 3, 0], [5, 0, 0, 0], [1, 1, 1, 0]], np.int64)
    prob_q = (np.array([[0.1, 0.6, 0.25, 0.05], [1.0, 0.0, 0.0, 0.0], [1 / 3, 1 / 3, 1 / 3, 0.0]]) * Q).round().astype(np.uint64) * \
        votes.sum(1, keepdims=True).astype(np.uint64)
    cellprob_q = np.array([10 * Q, 5 * Q // 2, 0], np.uint64)
    cls = np.array([1, 0, 2])
    names, vals = confidence.measurements(votes, prob_q, cellprob_q, cls, "summary", labels)
    assert names == ["class_vote_fraction", "class_probability", "detection_probability"]
    assert vals.dtype == np.float64 and vals.shape == (3, 3)
    n = votes.sum(1).astype(np.float64)
    want = np.stack([votes[np.arange(3), cls] / n, prob_q[np.arange(3), cls].astype(np.float64) / (n * Q),
                     cellprob_q.astype(np.float64) / (n * Q)], 1)
    assert np.array_equal(vals, want)
    assert vals[0].tolist() == [0.7, float(np.uint64(round(0.6 * Q)) * np.uint64(10)) / (10.0 * Q), 1.0]
    assert vals[1].tolist() == [1.0, 1.0, 0.5] and vals[2, 0] == 1 / 3 and vals[2, 2] == 0.0
    names_f, vals_f = confidence.measurements(votes, prob_q, cellprob_q, cls, "full", labels)
    assert names_f == names + ['probability: imm"une', "probability: tumour", "probability: stroma", 'probability: imm"une']
    assert names_f[3] == "probability: " + geojson.cell_dict([[0, 0]], 0, labels, 1, 1, [0, 0])["label"]
    assert np.array_equal(vals_f[:, :3], vals) and np.array_equal(vals_f[:, 3:], prob_q.astype(np.float64) / (n * Q)[:, None])
    # no class head: detection_probability alone in either mode, the pixel counts from area=
    for mode in ("summary", "full"):
        nm, v = confidence.measurements(None, None, cellprob_q, np.zeros(3, int), mode, None, area=[10, 5, 3])
        assert nm == ["detection_probability"] and v[:, 0].tolist() == [1.0, 0.5, 0.0]
    with pytest.raises(ValueError):
        confidence.measurements(votes, prob_q, cellprob_q, cls, "everything", labels)
    with pytest.raises(ValueError):
        confidence.measurements(votes, prob_q, cellprob_q, np.array([1, 4, 2]), "summary", labels)
    # rows survive the packing that carries them beside the cell table
    rows = confidence.pack_rows(votes, prob_q, cellprob_q, votes.sum(1))
    assert rows.dtype == np.uint64 and rows.shape == (3, confidence.row_width(4))
    v, p, c, a = confidence.unpack_rows(rows)
    assert np.array_equal(v, votes) and np.array_equal(p, prob_q) and np.array_equal(c, cellprob_q) and a.tolist() == [10, 5, 3]
    assert confidence.unpack_rows(confidence.pack_rows(np.zeros((3, 0)), np.zeros((3, 0)), cellprob_q, [10, 5, 3]))[0].shape == (3, 0)
    # no cells at all: empty tables of the right width
    assert confidence.pack_rows(np.zeros((0, 4)), np.zeros((0, 4)), np.zeros(0), np.zeros(0)).shape == (0, confidence.row_width(4))
    empty = confidence.stats_table(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 4)), np.zeros((0, 4), np.uint64), np.zeros(0, np.uint64))
    assert empty.shape == (0,) and empty["votes"].shape == (0, 4) and empty.dtype.names == confidence.STATS_FIELDS
    one = confidence.stats_table([1], [2], [4], [[1, 0, 3, 0]], [[Q, 0, 3 * Q, 0]], [2 * Q])
    assert one["prob"].tolist() == [[0.25, 0.0, 0.75, 0.0]] and one["detection"].tolist() == [0.5] and one["area"].tolist() == [4]


# ---- writer -------------------------------------------------------------------------------------------------------------------------------
_MASK = lambda t: re.sub(r'"id": "[0-9a-f]{8}-[0-9a-f]{4}-4[0-9a-f]{3}-[89ab][0-9a-f]{3}-[0-9a-f]{12}"', '"id": "X"', t)   # noqa: E731


def _cells(n, rng):
    from classpose_amd.entrypoints.predict_wsi import CELL_ROW
    cells = np.zeros(n, CELL_ROW)
    cells["n_pts"] = rng.integers(3, 7, n)
    cells["cls"] = rng.integers(0, 3, n)
    cells["area"] = rng.uniform(10, 500, n)
    cells["perimeter"] = rng.uniform(10, 90, n)
    cells["cx"] = rng.uniform(0, 1e5, n)
    cells["cy"] = rng.uniform(0, 1e5, n)
    xy = rng.integers(0, 40000, (int(cells["n_pts"].sum()), 2)).astype(np.float64) * 0.5
    return cells, xy, np.concatenate([[0], np.cumsum(cells["n_pts"])])


def test_writer_with_extras_is_bytewise_json_dump(tmp_path):
    rng = np.random.default_rng(5)
    n = 20
    cells, xy, offs = _cells(n, rng)
    labels = ["a", 'b "quoted" \\ name', "ünï"]
    names = ["class_vote_fraction", "class_probability", "detection_probability"] + ["probability: " + l for l in labels]
    extra = rng.uniform(0, 1, (n, len(names)))
    special = [1.0, 0.0, 1 / 3, 5e-324, 0.5, 2 / 3, 1e-5, 0.1 + 0.2, 16777215 / 16777216, 1e-4]
    extra.reshape(-1)[: len(special)] = special
    extra[7] = [0.0, 1.0, 1 / 3, 5e-324, 1.0, 0.0]
    keep = [int(k) for k in rng.permutation(n)] + [3, 3, 0]                 # repeats, as overlapping ROIs produce them
    for bounds in [(0.0, 0.0), (12.5, -7.25)]:
        feats, plain = [], []
        for i in keep:
            c = cells[i]
            centroid = np.round([c["cx"], c["cy"]], 2).tolist()
            cd = geojson.cell_dict(xy[offs[i]:offs[i + 1]].tolist(), int(c["cls"]), labels, c["area"], c["perimeter"], centroid)
            f = geojson.to_geojson_polygon(cd, extra_measurements=list(zip(names, extra[i])))
            g = geojson.to_geojson_polygon(dict(cd))
            assert [m["name"] for m in f["properties"]["measurements"]] == ["area", "perimeter", "centroidX", "centroidY"] + names
            feats.append(geojson.apply_bounds_offset_to_feature(f, *bounds) if bounds != (0.0, 0.0) else f)
            plain.append(geojson.apply_bounds_offset_to_feature(g, *bounds) if bounds != (0.0, 0.0) else g)
        want_c = json.dumps({"type": "FeatureCollection", "features": feats})
        want_p = json.dumps({"type": "FeatureCollection", "features": geojson.polygons_to_centroids(plain)})
        geojson.write_feature_collections(tmp_path / "c.json", tmp_path / "p.json", cells, xy, keep, labels, bounds, n_threads=3,
                                          extra_names=names, extra=extra)
        got_c, got_p = open(tmp_path / "c.json").read(), open(tmp_path / "p.json").read()
        assert _MASK(got_c) == _MASK(want_c)
        assert _MASK(got_p) == _MASK(want_p)                                # the centroids file does not carry the extras
        assert '"value": 5e-324}' in got_c and '"value": 0.3333333333333333}' in got_c
        assert json.dumps('probability: b "quoted" \\ name') in got_c
        # the same cells without extras: the centroids file is the same file
        geojson.write_feature_collections(tmp_path / "c0.json", tmp_path / "p0.json", cells, xy, keep, labels, bounds, n_threads=3)
        assert _MASK(open(tmp_path / "p0.json").read()) == _MASK(got_p)
    with pytest.raises(ValueError):
        geojson.write_feature_collections(tmp_path / "c.json", tmp_path / "p.json", cells, xy, keep, labels, extra_names=names,
                                          extra=extra[:, :2])


def test_writer_ex_without_extras_equals_the_plain_writer(tmp_path):
    rng = np.random.default_rng(6)
    n = 20
    cells, xy, offs = _cells(n, rng)
    L = _lib.lib()
    keep = np.arange(n, dtype=np.int64)
    cen = np.ascontiguousarray(geojson.rounded_centroids(cells))
    table = [t.encode("ascii") for t in geojson.class_json_table(["a", "b", "c"], 3)]
    arr = (C.c_char_p * len(table))(*table)
    offs = np.ascontiguousarray(offs.astype(np.int64))

    def args(a, b):
        return (str(tmp_path / a).encode(), str(tmp_path / b).encode(), cells.ctypes.data, n, cen.ctypes.data, xy.ctypes.data,
                offs.ctypes.data, keep.ctypes.data, n, arr, len(table), 3.0, -2.0, 2)
    _lib.check(L.cpx_write_geojson(*args("c1.json", "p1.json")))
    _lib.check(L.cpx_write_geojson_ex(*args("c2.json", "p2.json"), None, 0, None))
    for a, b in (("c1.json", "c2.json"), ("p1.json", "p2.json")):
        assert _MASK(open(tmp_path / a).read()) == _MASK(open(tmp_path / b).read())
    assert L.cpx_write_geojson_ex(*args("c3.json", "p3.json"), None, 2, None) == -22           # names missing: CPX_EINVAL
    assert L.cpx_write_geojson_ex(*args("c3.json", "p3.json"), None, -1, None) == -22


# ---- parsers ------------------------------------------------------------------------------------------------------------------------------
def test_parsers_keep_the_namespace_unless_the_flag_is_given(capsys):
    from classpose_amd.entrypoints import predict_wsi, predict_wsi_cpsam
    for mod, base in ((predict_wsi, ["--model_config", "m", "--slide_path", "s", "--output_folder", "o"]),
                      (predict_wsi_cpsam, ["--slide_path", "s", "--output_folder", "o"])):
        p = mod.build_parser()
        a = p.parse_args(base)
        assert "cell_confidence" not in vars(a) and getattr(a, "cell_confidence", None) is None
        for mode in ("summary", "full"):
            assert vars(p.parse_args(base + ["--cell_confidence", mode]))["cell_confidence"] == mode
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--cell_confidence", "everything"])
        with pytest.raises(SystemExit):
            p.parse_args(base + ["--cell_confidence"])
        assert "reference" in " ".join(p.format_help().split()).split("--cell_confidence", 2)[-1]
    capsys.readouterr()


# ---- ordering, selection, exchange ----------------------------------------------------------------------------------------------------
def test_rows_follow_their_cells_through_order_and_selection():
    from classpose_amd.entrypoints import predict_wsi as pw
    rng = np.random.default_rng(7)
    n = 12
    cells, xy, offs = _cells(n, rng)
    cells["area"] = np.arange(n) + 100.0                                    # the cell's identity
    tiles = np.array([4, 4, 1, 1, 1, 7, 0, 0, 3, 3, 3, 2], np.int64)        # as ranks and fallback paths deliver them
    extra = confidence.pack_rows(np.arange(n)[:, None] * np.array([[1, 2]]) + 1, np.arange(n)[:, None] * np.array([[3, 5]]),
                                 np.arange(n) * 7, np.arange(n) * 3 + 2)
    c2, xy2, e2 = pw.canonical_cell_order(cells, xy, tiles, extra)
    order = np.argsort(tiles, kind="stable")
    assert np.array_equal(c2["area"], cells["area"][order]) and not np.array_equal(order, np.arange(n))
    ident = (c2["area"] - 100).astype(np.int64)
    assert np.array_equal(e2, extra[ident]) and e2.dtype == np.uint64
    assert np.array_equal(e2[:, 4], ident.astype(np.uint64) * np.uint64(7))
    c3, xy3 = pw.canonical_cell_order(cells, xy, tiles)                      # without rows: what it was
    assert np.array_equal(c3, c2) and np.array_equal(xy3, xy2)
    # already ordered: passed through, rows included
    c4, xy4, e4 = pw.canonical_cell_order(c2, xy2, np.sort(tiles), e2)
    assert c4 is c2 and e4 is e2
    # the keep indices of de-duplication and the filters (np.repeat duplicates included) pick rows and cells alike
    keep = np.repeat(np.array([0, 2, 5, 11, 7]), [1, 2, 0, 1, 3])
    votes, prob_q, cq, area = confidence.unpack_rows(e2)
    names, vals = confidence.measurements(votes, prob_q, cq, np.zeros(n, int), "summary", ["x", "y"])
    assert np.array_equal(vals[keep][:, 0], (votes[:, 0] / votes.sum(1))[keep])
    assert np.array_equal(e2[keep][:, 5], (ident[keep] * 3 + 2).astype(np.uint64))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gather_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    parallel.init_distributed("gloo")
    from classpose_amd.entrypoints import predict_wsi as pw
    n = 3 + 2 * rank
    cells = np.zeros(n, pw.CELL_ROW)
    cells["area"] = 100 * rank + np.arange(n); cells["n_pts"] = 4; cells["cls"] = rank + 1
    xy = np.arange(n * 4 * 2, dtype=np.float64).reshape(-1, 2) + 1000 * rank
    tiles = np.arange(n, dtype=np.int64) * world + rank
    extra = (np.arange(n * 6, dtype=np.uint64).reshape(n, 6) + np.uint64(1000 * rank)) | (np.uint64(1) << np.uint64(40 + rank))
    c, v, t, e = pw.gather_cells(cells, xy, torch.device("cpu"), tiles, extra)
    parallel.barrier()
    q.put((rank, c.copy(), t.copy(), e.copy()))
    torch.distributed.destroy_process_group()


def test_confidence_rows_all_gather_over_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    ps = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = sorted([q.get(timeout=120) for _ in ps], key=lambda t: t[0])
    for p in ps:
        p.join(60)
        assert p.exitcode == 0
    want = np.concatenate([(np.arange(n * 6, dtype=np.uint64).reshape(n, 6) + np.uint64(1000 * r)) | (np.uint64(1) << np.uint64(40 + r))
                           for r, n in ((0, 3), (1, 5))])
    for r, c, t, e in res:
        assert len(c) == len(t) == 8 and e.dtype == np.uint64 and np.array_equal(e, want)
        assert list(c["cls"]) == [1] * 3 + [2] * 5
