"""GPU: per-cell class confidence (cpx_instance_confidence, csrc/cpx_confidence.hip) against the numpy float64 restatement
in tests/cell_confidence_reference.py, at shapes far below the workload's, then through the engine, the CLI and eval.

Bounds.  ``votes`` are integer counts: equal.  ``prob_q`` / ``cellprob_q`` are sums of per-pixel values rounded to 2^-24:
within n quanta of the reference, n the instance's pixel count -- one quantum per pixel, the most a last-bit difference
between the device's and numpy's float64 ``exp`` can move a rounded value (p * 2^24 moves by ~2^24 * 2^-52, so a rounding
can flip only at a tie).  A derived bound, not a measured one; equality is what is expected, and every test prints the
largest difference it saw."""
import ctypes as C
import json
import re

import numpy as np
import pytest
import torch

import cell_confidence_reference as ref
from classpose_amd import _lib, confidence, engine, ops, synth
from classpose_amd._lib import ptr

pytestmark = pytest.mark.gpu

Q = 1 << 24
GUARD = 64                       # sentinel elements before and after every output buffer
S32, S64 = -1234567, -987654321012345


def _run(dev, masks, logits, cellprob, rec_counts, max_rec, ncls=None, L=None):
    """the raw entry into sentinel-filled buffers with guard bands -> (rc, votes, prob_q, cellprob_q, guards_ok) as numpy"""
    L = L or _lib.lib()
    nT, H, W = masks.shape
    ncls = (0 if logits is None else logits.shape[1]) if ncls is None else ncls
    k = max(ncls, 1)
    d_m = torch.from_numpy(np.ascontiguousarray(masks).view(np.int16)).to(dev)
    d_l = None if logits is None else torch.from_numpy(np.ascontiguousarray(logits, dtype=np.float32)).to(dev)
    d_c = None if cellprob is None else torch.from_numpy(np.ascontiguousarray(cellprob, dtype=np.float32)).to(dev)
    d_n = torch.tensor(list(rec_counts), dtype=torch.int32, device=dev)
    bv = torch.full((2 * GUARD + nT * max_rec * k,), S32, dtype=torch.int32, device=dev)
    bp = torch.full((2 * GUARD + nT * max_rec * k,), S64, dtype=torch.int64, device=dev)
    bc = torch.full((2 * GUARD + nT * max_rec,), S64, dtype=torch.int64, device=dev)
    need = L.cpx_instance_confidence_workspace_bytes(nT, ncls, H, W, max_rec)
    ws = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
    rc = L.cpx_instance_confidence(ptr(d_m), ptr(d_l), ptr(d_c), ptr(d_n), nT, ncls, H, W, max_rec, ptr(bv[GUARD:]), ptr(bp[GUARD:]),
                                   ptr(bc[GUARD:]), ptr(ws), need, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    guards = all(bool((b[:GUARD] == s).all()) and bool((b[-GUARD:] == s).all()) for b, s in ((bv, S32), (bp, S64), (bc, S64)))
    return (rc, bv[GUARD:-GUARD].cpu().numpy().reshape(nT, max_rec, k), bp[GUARD:-GUARD].cpu().numpy().reshape(nT, max_rec, k),
            bc[GUARD:-GUARD].cpu().numpy().reshape(nT, max_rec), guards)


def _check(dev, masks, logits, cellprob, rec_counts, max_rec, what, exact=False, L=None):
    """entry == reference on the defined rows (votes exactly, sums within n quanta), sentinel everywhere else"""
    rc, v, p, c, guards = _run(dev, masks, logits, cellprob, rec_counts, max_rec, L=L)
    assert rc == 0, _lib.lib().cpx_last_error()
    assert guards, "a guard band was written"
    rv, rp, rcq, valid = ref.instance_confidence(masks, logits, cellprob, rec_counts, max_rec)
    nT = masks.shape[0]
    area = np.stack([np.bincount(masks[t].reshape(-1).astype(np.int64), minlength=max_rec + 2)[1:max_rec + 1] for t in range(nT)])
    worst = 0
    if logits is not None and logits.shape[1] > 1:
        assert np.array_equal(v[valid], rv[valid]), f"{what}: votes differ"
        assert (v[~valid] == S32).all() and (p[~valid] == S64).all(), f"{what}: a class row past rec_counts was written"
        d = np.abs(p.astype(np.int64) - rp.astype(np.int64))[valid]
        worst = max(worst, int(d.max()) if d.size else 0)
        assert (d <= area[valid][:, None]).all(), f"{what}: prob_q off by up to {d.max()} quanta"
    else:
        assert (v == S32).all() and (p == S64).all(), f"{what}: the class buffers were touched without a class part"
    if cellprob is not None:
        assert (c[~valid] == S64).all(), f"{what}: a detection row past rec_counts was written"
        d = np.abs(c.astype(np.int64) - rcq.astype(np.int64))[valid]
        worst = max(worst, int(d.max()) if d.size else 0)
        assert (d <= area[valid]).all(), f"{what}: cellprob_q off by up to {d.max()} quanta"
    else:
        assert (c == S64).all(), f"{what}: cellprob_q was touched without a detection part"
    print(f"{what}: largest |device - reference| = {worst} quanta")
    if exact:
        assert worst == 0
    return v, p, c, valid


def _random_maps(rng, nT, H, W, n_inst):
    """Voronoi cells of n_inst random seeds, eroded by a random background: instances of many sizes that cross workgroups"""
    yy, xx = np.mgrid[:H, :W]
    out = np.zeros((nT, H, W), np.uint16)
    for t in range(nT):
        sy, sx = rng.integers(0, H, n_inst), rng.integers(0, W, n_inst)
        d = (yy[None] - sy[:, None, None]) ** 2 + (xx[None] - sx[:, None, None]) ** 2
        lab = d.argmin(0) + 1
        lab[(d.min(0) > 36) | (rng.random((H, W)) < 0.1)] = 0
        out[t] = lab
    return out


@pytest.fixture(scope="module")
def fields():
    rng = np.random.default_rng(2024)
    masks = _random_maps(rng, 3, 64, 64, 40)
    return masks, {k: (rng.normal(0, 3, (3, k, 64, 64))).astype(np.float32) for k in (2, 7, 32)}, rng.normal(0, 4, (3, 64, 64)).astype(np.float32)


@pytest.mark.parametrize("ncls", [2, 7, 32])
def test_random_maps(cuda, fields, ncls):
    masks, lg, cp = fields
    assert all(len(np.unique(masks[t])) >= 36 for t in range(3))
    v, p, c, valid = _check(cuda, masks, lg[ncls], cp, [40, 40, 40], 44, f"random maps, {ncls} classes")
    assert valid.sum() == 120 and (v[valid].sum(1) > 0).sum() >= 100


def test_odd_size_partial_last_workgroup(cuda):
    rng = np.random.default_rng(3)
    masks = _random_maps(rng, 2, 40, 72, 30)            # 2 880 pixels: eleven workgroups and a quarter
    masks[:, -1, -8:] = 30                              # ... and the quarter has cells in it, up to the last pixel
    assert (40 * 72) % 256 != 0
    _check(cuda, masks, rng.normal(0, 3, (2, 5, 40, 72)).astype(np.float32), rng.normal(0, 3, (2, 40, 72)).astype(np.float32),
           [30, 30], 30, "40 x 72")


def test_one_instance_over_the_whole_tile(cuda):
    rng = np.random.default_rng(4)
    masks = np.ones((1, 64, 64), np.uint16)
    v, p, c, _ = _check(cuda, masks, rng.normal(0, 2, (1, 7, 64, 64)).astype(np.float32), rng.normal(0, 2, (1, 64, 64)).astype(np.float32),
                        [1], 3, "one instance, 16 workgroups")
    assert v[0, 0].sum() == 4096


@pytest.mark.parametrize("ncls", [2, 32])
def test_lds_table_full_goes_to_global_atomics(cuda, ncls):
    """every pixel its own instance: a workgroup's 256 pixels bring 256 x (ncls + 1) table keys to 512 slots, so most
    contributions find no slot in 8 probes and take the direct path; with 32 classes the arg-max cycles through them"""
    rng = np.random.default_rng(5)
    masks = (np.arange(1024, dtype=np.uint16) + 1).reshape(1, 32, 32)
    lg = rng.normal(0, 1, (1, ncls, 32, 32)).astype(np.float32)
    win = np.arange(1024).reshape(32, 32) % ncls
    np.put_along_axis(lg[0], win[None], 6.0, 0)
    assert 256 * (ncls + 1) > 512
    v, p, c, _ = _check(cuda, masks, lg, rng.normal(0, 3, (1, 32, 32)).astype(np.float32), [1024], 1024, f"1 024 labels, {ncls} classes")
    assert np.array_equal(v[0].argmax(1), win.reshape(-1)) and (v[0].sum(1) == 1).all()


def test_saturation_is_exact(cuda):
    rng = np.random.default_rng(6)
    masks = _random_maps(rng, 1, 64, 64, 20)
    win = rng.integers(0, 5, 21)
    lg = np.full((1, 5, 64, 64), -80.0, np.float32)
    np.put_along_axis(lg[0], win[masks[0]][None], 80.0, 0)
    cp = np.full((1, 64, 64), 80.0, np.float32)
    v, p, c, valid = _check(cuda, masks, lg, cp, [20], 20, "logits +-80", exact=True)
    n = np.bincount(masks[0].reshape(-1), minlength=21)[1:]
    for r in range(20):
        want = np.zeros(5, np.int64)
        want[win[r + 1]] = n[r] * Q
        assert np.array_equal(p[0, r], want) and c[0, r] == n[r] * Q and v[0, r, win[r + 1]] == n[r]


def test_non_finite_pixels_vote_and_add_nothing(cuda):
    masks = np.zeros((1, 8, 64), np.uint16)
    masks[0, 2, 3:11] = 1
    masks[0, 5, 20:24] = 2
    lg = np.zeros((1, 4, 8, 64), np.float32)
    lg[0, :, 2, 3] = [0.0, np.nan, 9.0, np.nan]          # the first NaN wins: class 1
    lg[0, :, 2, 4] = [1.0, np.inf, 0.0, 0.0]             # +inf wins: class 1
    lg[0, :, 2, 5] = [1.0, -np.inf, 0.0, 3.0]            # -inf loses: class 3
    lg[0, :, 2, 6] = [0.0, 0.0, np.inf, np.inf]          # two +inf: the first, class 2
    lg[0, :, 2, 7] = [2.0, 0.0, 0.0, 0.0]                # finite: class 0
    lg[0, :, 5, 20] = [np.nan, np.nan, np.nan, np.nan]   # class 0
    cp = np.ones((1, 8, 64), np.float32)
    cp[0, 2, 3], cp[0, 2, 4], cp[0, 5, 21] = np.nan, np.inf, -np.inf
    v, p, c, _ = _check(cuda, masks, lg, cp, [2], 2, "NaN / inf pixels", exact=True)
    assert v[0].tolist() == [[4, 2, 1, 1], [4, 0, 0, 0]]
    fin = ref.softmax_q(lg[0, :, 2, 7:11].reshape(4, -1)).sum(1)
    assert np.array_equal(p[0, 0].astype(np.uint64), fin)                    # the four non-finite pixels added 0 to every class
    assert p[0, 1].tolist() == [3 * (Q // 4)] * 4
    one = int(ref.sigmoid_q(np.ones(1, np.float32))[0])
    assert c[0].tolist() == [6 * one, 3 * one]


def test_ids_out_of_range_are_background(cuda):
    rng = np.random.default_rng(7)
    masks = _random_maps(rng, 2, 32, 64, 12)             # ids 1 .. 12
    masks[0, 0, :5] = [8, 9, 11, 65535, 40000]           # tile 0: rec_counts 7, max_rec 10: 8 = rec_counts + 1, 11 = max_rec + 1
    masks[1, 3, :4] = [11, 12, 65535, 10]                # tile 1: rec_counts 30 > max_rec
    lg, cp = rng.normal(0, 2, (2, 3, 32, 64)).astype(np.float32), rng.normal(0, 2, (2, 32, 64)).astype(np.float32)
    v, p, c, valid = _check(cuda, masks, lg, cp, [7, 30], 10, "ids past rec_counts and max_rec")
    assert valid.sum(1).tolist() == [7, 10]
    clean = masks.copy()
    clean[0][clean[0] > 7] = 0
    clean[1][clean[1] > 10] = 0
    v2, p2, c2, _ = _check(cuda, clean, lg, cp, [7, 30], 10, "the same with those pixels as background")
    assert np.array_equal(v, v2) and np.array_equal(p, p2) and np.array_equal(c, c2)
    # a negative count defines no row
    rc, v3, p3, c3, guards = _run(cuda, masks, lg, cp, [-5, 0], 10)
    assert rc == 0 and guards and (v3 == S32).all() and (p3 == S64).all() and (c3 == S64).all()


def test_optional_parts_and_argument_checks(cuda):
    rng = np.random.default_rng(8)
    masks = _random_maps(rng, 1, 32, 32, 6)
    lg, cp = rng.normal(0, 2, (1, 4, 32, 32)).astype(np.float32), rng.normal(0, 2, (1, 32, 32)).astype(np.float32)
    _check(cuda, masks, None, cp, [6], 6, "logits = NULL")
    _check(cuda, masks, lg[:, :1], cp, [6], 6, "ncls = 1")
    _check(cuda, masks, lg, None, [6], 6, "cellprob = NULL")
    for bad in (33, -1):
        rc, v, p, c, guards = _run(cuda, masks, np.zeros((1, 33, 32, 32), np.float32), cp, [6], 6, ncls=bad)
        assert rc == -22 and guards and (v == S32).all() and (p == S64).all() and (c == S64).all()
    rc, v, p, c, _ = _run(cuda, masks, None, None, [6], 6)                   # neither part
    assert rc == -22 and (c == S64).all()
    with pytest.raises(ValueError):
        ops.instance_confidence(torch.zeros((1, 32, 32), dtype=torch.int16, device=cuda), None,
                                torch.zeros((1, 16, 32), dtype=torch.float32, device=cuda), torch.zeros(1, dtype=torch.int32, device=cuda), 4)


def test_two_runs_and_both_footprints_give_the_same_bits(cuda, fields):
    masks, lg, cp = fields
    a = _run(cuda, masks, lg[7], cp, [40, 40, 40], 44)
    b = _run(cuda, masks, lg[7], cp, [40, 40, 40], 44)
    assert a[0] == b[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:4]))
    with _lib.use_debug_library() as D:                  # the 16 x 16 footprint the benchmark compares (debug build only)
        try:
            D.cpx_confidence_set_footprint(1)
            c = _run(cuda, masks, lg[7], cp, [40, 40, 40], 44, L=D)
            odd = _random_maps(np.random.default_rng(9), 1, 40, 72, 30)
            _check(cuda, odd, lg[7][:1, :, :40, :].repeat(2, 3)[..., :72].copy(), None, [30], 30, "16 x 16 footprint, 40 x 72", L=D)
        finally:
            D.cpx_confidence_set_footprint(0)
    assert c[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1:4], c[1:4]))


# ---- against the chain, the engine, the CLI, eval --------------------------------------------------------------------------------------
def _analytic(n, ncls, seed, noise):
    rng = np.random.default_rng(seed)
    f = [synth.analytic_fields(seed + k, 40 * k, 0, 256, 256, ncls) for k in range(n)]
    dP, cp = np.stack([a[0] for a in f]), np.stack([a[1] for a in f])
    lg = np.stack([a[2] for a in f]) + rng.normal(0, noise, (n, ncls, 256, 256)).astype(np.float32)
    return dP, cp, lg.astype(np.float32)


def test_against_the_chain(cuda):
    """the new pass sees the vote the product already makes: per record, sum_c votes == area and the first arg-max == cls"""
    L = _lib.lib()
    nT, ncls, H, W = 2, 7, 256, 256
    dP, cp, lg = (torch.from_numpy(a).to(cuda) for a in _analytic(nT, ncls, 300, 3.0))
    max_rec = L.cpx_postproc_max_labels(H, W)
    masks = torch.empty((nT, H, W), dtype=torch.int16, device=cuda)
    cm = torch.empty((nT, H, W), dtype=torch.uint8, device=cuda)
    nlab = torch.empty(nT, dtype=torch.int32, device=cuda)
    recs = torch.zeros(nT * max_rec * engine.RECORD_DTYPE.itemsize, dtype=torch.uint8, device=cuda)
    cnt = torch.empty(nT, dtype=torch.int32, device=cuda)
    ws = torch.empty(L.cpx_postproc_workspace_bytes(nT, H, W), dtype=torch.uint8, device=cuda)
    st = torch.cuda.current_stream(cuda).cuda_stream
    _lib.check(L.cpx_compute_masks_records(ptr(dP), ptr(cp), ptr(lg), nT, ncls, H, W, 0.0, 0.4, 200, 15, 0.4, ptr(masks), ptr(cm),
                                           ptr(nlab), max_rec, ptr(recs), ptr(cnt), ptr(ws), st))
    votes, prob_q, cq = ops.instance_confidence(masks, lg, cp, cnt, max_rec)
    counts = cnt.cpu().numpy()
    assert counts.min() >= 10
    r = recs.cpu().numpy().view(engine.RECORD_DTYPE).reshape(nT, max_rec)
    v = votes.cpu().numpy()
    seen = set()
    for t in range(nT):
        k = int(counts[t])
        assert np.array_equal(r[t, :k]["label"], np.arange(1, k + 1))
        assert np.array_equal(v[t, :k].sum(1), r[t, :k]["area"])
        assert np.array_equal(v[t, :k].argmax(1), r[t, :k]["cls"])
        seen |= set(np.round(v[t, :k].max(1) / v[t, :k].sum(1), 3))
    assert len(seen) > 3                                # the noise makes the votes split: not every cell is unanimous
    # and the sums are the reference's on the chain's own map
    rv, rp, rc_, valid = ref.instance_confidence(masks.cpu().numpy().view(np.uint16), lg.cpu().numpy(), cp.cpu().numpy(), counts, max_rec)
    area = rv.sum(2)
    assert np.array_equal(v[valid], rv[valid])
    d = np.abs(prob_q.cpu().numpy() - rp.astype(np.int64))[valid]
    dc = np.abs(cq.cpu().numpy() - rc_.astype(np.int64))[valid]
    print(f"against the chain: largest |device - reference| = {max(d.max(), dc.max())} quanta")
    assert (d <= area[valid][:, None]).all() and (dc <= area[valid]).all()


def test_engine_confidence_switch(cuda):
    L = _lib.lib()
    sd = synth.make_state_dict(7, None, depth=1, seed=3)
    w = engine.NetWeights.from_state_dict(sd, "bf16", cuda)
    eng = engine.Engine(w, 256, batch_tiles=2)
    tiles = torch.from_numpy(np.stack([synth.render_region(300 + k, 40 * k, 0, 256, 256) for k in range(2)])).to(cuda)
    inj = tuple(torch.from_numpy(a).to(cuda) for a in _analytic(2, 7, 300, 3.0))
    poly = (1.0, [(0.0, 0.0), (512.0, 0.0)])
    got = {}
    for conf in (False, True, True, False):             # two slots in turn: each sees both settings
        n0 = L.cpx_postproc_launch_count()
        out = eng.run(tiles, inject=inj, polygons=poly, confidence=conf)
        launches = L.cpx_postproc_launch_count() - n0
        torch.cuda.synchronize()
        total = int(out.n_pts_total.item())
        snap = (out.masks.cpu().numpy().copy(), out.class_masks.cpu().numpy().copy(), eng.fetch_records(2, out).tobytes(),
                eng.fetch_polygons(2, out)[0].tobytes(), out.xy_pool[:total].cpu().numpy().copy(), launches)
        if conf:
            assert out.votes is not None and out.prob_q is not None and out.cellprob_q is not None
            v, p, c = ops.instance_confidence(out.masks, out.logits if inj is None else inj[2], inj[1], out.rec_counts, eng.max_rec)
            for t in range(2):
                k = int(out.rec_counts[t])
                assert k > 5
                assert torch.equal(out.votes[t, :k], v[t, :k]) and torch.equal(out.prob_q[t, :k], p[t, :k]) and \
                    torch.equal(out.cellprob_q[t, :k], c[t, :k])
            tb, lb = np.array([0, 1, 1]), np.array([2, 1, 4])
            fv, fp, fc = eng.fetch_confidence(out, tb, lb)
            assert np.array_equal(fv, v[tb, lb - 1].cpu().numpy()) and np.array_equal(fp.view(np.int64), p[tb, lb - 1].cpu().numpy())
        else:
            assert out.votes is None and out.prob_q is None and out.cellprob_q is None
        got.setdefault(conf, []).append(snap)
    for a, b in zip(got[False], got[True]):
        assert all(np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y for x, y in zip(a, b))
    assert got[False][0][5] == got[True][0][5] > 0      # the chain's launch count is what it was


def test_cli_cell_confidence_full(cuda, tmp_path, monkeypatch):
    monkeypatch.setenv("CLASSPOSE_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("CLASSPOSE_SYNTHETIC_DEPTH", "1")
    monkeypatch.setenv("CLASSPOSE_AMD_PLUGINS", "classpose_amd.synth:flow")
    monkeypatch.setenv("CLASSPOSE_MODEL_DIR", str(tmp_path / "nomodels"))
    from classpose_amd import hooks
    from classpose_amd.entrypoints import predict_wsi
    texts = {}
    try:
        for name, extra in (("plain", []), ("full", ["--cell_confidence", "full"]), ("fallback", ["--cell_confidence", "full"])):
            hooks.reset()
            if name == "fallback":                      # the vertex pool "overflows": every batch goes to the host polygoniser
                monkeypatch.setattr(engine.Engine, "fetch_polygons", lambda self, n, out: None)
            out = tmp_path / name
            predict_wsi.main(predict_wsi.build_parser().parse_args([
                "--model_config", "conic", "--slide_path", "synthetic://512x512?mpp=0.5&seed=77", "--output_folder", str(out),
                "--tile_size", "256", "--overlap", "32", "--device", "cuda:0"] + extra))
            texts[name] = (open(next(out.glob("*contours.geojson"))).read(), open(next(out.glob("*centroids.geojson"))).read())
    finally:
        hooks.reset()
    mask = lambda t: re.sub(r'"id": "[0-9a-f-]{36}"', '"id": "X"', t)                                   # noqa: E731
    labels = ["Neutrophil", "Epithelial", "Lymphocyte", "Plasma cell", "Eosinophil", "Connective"]
    names = ["class_vote_fraction", "class_probability", "detection_probability"] + \
        ["probability: " + labels[c - 1] for c in range(7)]
    added = "".join(r', \{"name": %s, "value": [^}]*\}' % re.escape(json.dumps(n)) for n in names)
    assert mask(re.sub(added, "", texts["full"][0])) == mask(texts["plain"][0])
    assert mask(texts["full"][1]) == mask(texts["plain"][1])
    # the host-polygoniser fallback carries the same rows to the same cells
    assert mask(texts["fallback"][0]) == mask(texts["full"][0]) and mask(texts["fallback"][1]) == mask(texts["full"][1])
    feats = json.loads(texts["full"][0])["features"]
    assert len(feats) > 5
    for f in feats:
        m = f["properties"]["measurements"]
        assert [x["name"] for x in m] == ["area", "perimeter", "centroidX", "centroidY"] + names
        vals = np.array([x["value"] for x in m[4:]])
        assert ((vals >= 0) & (vals <= 1)).all()
        # class_vote_fraction * n is an integer for some pixel count n: the fraction is votes / n exactly
        assert any(abs(vals[0] * n - round(vals[0] * n)) < 1e-9 for n in range(1, 4000))
        assert abs(vals[3:].sum() - 1.0) <= 7 * 2.0 ** -24
        cls = labels.index(f["properties"]["classification"]["name"]) + 1
        # class_probability is the cell's own class's column (class value 0 shares the last label's name)
        assert vals[1] == vals[3 + cls] or (cls == 6 and vals[1] == vals[3])


@pytest.mark.parametrize("injected", [False, True])
def test_eval_cell_confidence(cuda, monkeypatch, injected):
    """``injected``: the engine's dynamics take analytic fields (random weights alone find no cell in a rendered tile, and a
    table without rows checks little); eval itself is what it is"""
    from classpose_amd.models import ClassposeModel
    sd = synth.make_state_dict(7, None, depth=1, seed=2)
    model = ClassposeModel(gpu=True, pretrained_model=sd, device=cuda, nclasses=7, precision="bf16")
    tile = synth.render_region(5, 0, 0, 256, 256)
    if injected:
        f = synth.analytic_fields(5, 0, 0, 256, 256, 7)
        noise = np.random.default_rng(1).normal(0, 3, f[2].shape).astype(np.float32)
        inj = tuple(torch.from_numpy(np.stack([a, a])).to(cuda) for a in (f[0], f[1], f[2] + noise))
        run = engine.Engine.run
        monkeypatch.setattr(engine.Engine, "run", lambda self, tiles, **kw: run(self, tiles, inject=tuple(a[:len(tiles)].contiguous() for a in inj), **kw))
    plain = model.eval([tile, tile])
    assert len(plain) == 4 and (plain[0][0].max() > 10) == injected
    masks, flows, class_masks, styles, conf = model.eval([tile, tile], cell_confidence=True)
    assert np.array_equal(masks[0], plain[0][0]) and np.array_equal(class_masks[0], plain[2][0])
    single = model.eval(tile, cell_confidence=True)
    assert len(single) == 5 and len(model.eval(tile)) == 4
    for m, cm, t in ((masks[0], class_masks[0], conf[0]), (single[0], single[2], single[4])):
        ids = np.unique(m)
        ids = ids[ids > 0]
        assert t.dtype.names == ("label", "cls", "area", "votes", "prob", "detection") and t["votes"].shape == (len(ids), 7)
        assert np.array_equal(t["label"], ids)
        assert np.array_equal(t["area"], np.bincount(m.reshape(-1))[1:]) and np.array_equal(t["votes"].sum(1), t["area"])
        first = np.array([np.flatnonzero(m.reshape(-1) == i)[0] for i in ids], dtype=np.int64)
        assert np.array_equal(t["cls"], cm.reshape(-1)[first])
        if len(ids):
            assert np.all(np.abs(t["prob"].sum(1) - 1) <= 7 * 2.0 ** -24) and np.all((t["detection"] > 0) & (t["detection"] <= 1))
    assert np.array_equal(conf[0], conf[1])


def test_cpsam_cli_writes_detection_probability_alone(cuda, tmp_path, monkeypatch):
    """the class-less entry: no vote table, so the pixel counts come from the records; either mode writes the one measurement"""
    monkeypatch.setenv("CLASSPOSE_SYNTHETIC_WEIGHTS", "1")
    monkeypatch.setenv("CLASSPOSE_SYNTHETIC_DEPTH", "1")
    monkeypatch.setenv("CLASSPOSE_AMD_PLUGINS", "classpose_amd.synth:flow")
    from classpose_amd import hooks
    from classpose_amd.entrypoints import predict_wsi_cpsam
    hooks.reset()
    try:
        predict_wsi_cpsam.main(predict_wsi_cpsam.build_parser().parse_args([
            "--model_path", str(tmp_path / "cpsam"), "--slide_path", "synthetic://512x512?mpp=0.5&seed=3", "--output_folder", str(tmp_path),
            "--tile_size", "256", "--overlap", "32", "--device", "cuda:0", "--cell_confidence", "full"]))
    finally:
        hooks.reset()
    feats = json.load(open(next(tmp_path.glob("*contours.geojson"))))["features"]
    cent = json.load(open(next(tmp_path.glob("*centroids.geojson"))))["features"]
    assert len(feats) > 5 and len(cent) == len(feats)
    vals = []
    for f, c in zip(feats, cent):
        assert [m["name"] for m in f["properties"]["measurements"]] == ["area", "perimeter", "centroidX", "centroidY", "detection_probability"]
        assert [m["name"] for m in c["properties"]["measurements"]] == ["area", "perimeter", "centroidX", "centroidY"]
        vals.append(f["properties"]["measurements"][4]["value"])
    vals = np.array(vals)
    assert ((vals > 0) & (vals <= 1)).all()
    # the injected cellprob is +6 inside a nucleus: a cell of such pixels alone has exactly the quantised sigmoid(6)
    assert (vals == float(ref.sigmoid_q(np.full(1, 6.0, np.float32))[0]) / Q).mean() > 0.5
