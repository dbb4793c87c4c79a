"""Device training of the 1x1 class head (csrc/cpx_train.hip -> ops -> classpose_amd.train -> the train_head CLI).

Yardstick: the float64 restatement of tests/train_reference.py (pinned on the reference's own functions by
tests/test_train_host.py), always evaluated on the SAME float32 logits / features the device read -- never the code under test.

Tolerance rule for a quantity q, with err(x) = ||x - q64||_2 / ||q64||_2:
    err(device) <= max(4 * err(torch CPU float32), 2^-20).
The margin of 4 covers a different summation order and expf; the floor is 16 float32 unit round-offs for a ~10-operation
per-element chain.  Every test prints the errors it observed before it asserts (run with -s to see them).

cpx_head_wgrad has a per-element bound instead: |dW - dW64| <= (L + P + 2) * 2^-24 * sum |a b| with L = 512, the longest serial
accumulation chain of the kernel (one slab of rows through the MFMA accumulator), and P = ceil(rows / 512), the number of slab
partials reduced -- the standard bound for recursive summation (the kernel adds the partials in float64 and rounds once, so it
has room to spare).
"""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import train_reference as tr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FLOOR = 2.0 ** -20


def _fixture():
    with open(os.path.join(GOLD, "reference_train.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_train.npz")), meta


def _head_from_logits(logits32: torch.Tensor, dev, seed=0):
    """float32 logits (n, C, H, W) -> a head buffer (rows, ld_head) as cpx_net_forward lays it out (192 flow columns of noise first)."""
    n, C, H, W = logits32.shape
    tok = tr.nchw_to_tokens(logits32)
    ld = (192 + C * 64 + 127) // 128 * 128
    g = torch.Generator().manual_seed(seed)
    head = torch.randn(tok.shape[0], ld, generator=g)
    head[:, 192:192 + C * 64] = tok
    return head.to(dev)


def _check(name, dev_val, f32_val, f64_val, floor=FLOOR):
    e_dev, e_cpu = tr.rel_l2(dev_val, f64_val), tr.rel_l2(f32_val, f64_val)
    tol = max(4 * e_cpu, floor)
    print(f"  {name}: err(device) = {e_dev:.3e}, err(torch CPU float32) = {e_cpu:.3e}, tolerance = {tol:.3e}")
    assert e_dev <= tol, (name, e_dev, e_cpu, tol)
    return e_dev


def _run_loss_case(dev, logits32, labels, cw, tag):
    from classpose_amd import ops
    n, C, H, W = logits32.shape
    head = _head_from_logits(logits32, dev)
    lab = torch.from_numpy(labels).to(dev)
    cwt = None if cw is None else torch.from_numpy(np.float32(cw))
    o = ops.class_loss(head, lab, C, 192, None if cwt is None else cwt.to(dev))
    o2 = ops.class_loss(head, lab, C, 192, None if cwt is None else cwt.to(dev))
    back = tr.tokens_to_nchw(head.cpu(), 192, C, n, H, W)           # the logits the device read, copied back
    assert torch.equal(back, logits32)
    cw32 = None if cwt is None else cwt.double()                    # the float32 weights the device read
    r64 = tr.loss_and_grad(back, torch.from_numpy(labels), cw32)
    r32 = tr.loss_and_grad_f32(back, torch.from_numpy(labels), cw32)
    print(f"{tag}: ce = {o.ce.item():.9g}, tversky = {o.tversky.item():.9g}")
    raw = tr.raw_tversky(r64["tp"], r64["fp"], r64["fn"])
    present = raw != 1.0
    edge = float(torch.minimum(raw[present], 1 - raw[present]).min())
    print(f"  distance of the raw Tversky losses from the clip edges >= {edge:.3f}; absent (image, class) pairs: {int((~present).sum())}")
    assert edge >= 0.1
    _check("ce", o.ce.cpu(), r32["ce"], r64["ce"])
    _check("tversky", o.tversky.cpu(), r32["tversky"], r64["tversky"])
    for k in ("tp", "fp", "fn"):
        _check(k, getattr(o, k).cpu(), r32[k], r64[k])
    g_dev = tr.tokens_to_nchw(o.dlogits.cpu(), 0, C, n, H, W)
    _check("dlogits", g_dev, r32["dlogits"], r64["dlogits"])
    assert torch.equal(o.n_annot.cpu().long(), torch.from_numpy((labels != -100).reshape(n, -1).sum(1)))
    # not-annotated pixels: exactly zero rows
    assert torch.all(g_dev.permute(0, 2, 3, 1)[torch.from_numpy(labels == -100)] == 0)
    # two runs are bitwise equal
    for k in ("ce", "tversky", "tp", "fp", "fn", "dlogits"):
        assert torch.equal(getattr(o, k), getattr(o2, k)), k
    return o, r64, head, lab


@pytest.mark.parametrize("name", ["c7", "c7w", "c10", "c10w"])
def test_class_loss_fixture_cases(cuda, name):
    arr, meta = _fixture()
    c = next(x for x in meta["cases"] if x["name"] == name)
    logits32 = torch.from_numpy(arr[name + "_logits"])
    cw = arr[name + "_weights"] if c["weights"] else None
    o, r64, head, lab = _run_loss_case(cuda, logits32, arr[name + "_labels"], cw, name)
    # the reference's own numbers: the floor, plus 2^-23 where class weights enter (float64 there, rounded to float32 here:
    # numerator and denominator of a weighted mean each move by at most 2^-24 relative)
    rt = FLOOR + (2.0 ** -23 if cw is not None else 0.0)
    assert abs(o.ce.item() - c["ce"]) <= rt * abs(c["ce"])
    assert abs(o.tversky.item() - c["tversky"]) <= rt * abs(c["tversky"])


@pytest.mark.parametrize("name", ["c7w", "c10", "c10w"])
def test_absent_class_has_exactly_zero_gradient_share(cuda, name):
    """With the cross-entropy switched off, the rows of an image do not change by one bit when the weight of a class that is
    absent from it is multiplied by 1000: its Tversky term (raw loss exactly 1, clipped) passes no gradient."""
    from classpose_amd import ops
    arr, meta = _fixture()
    c = next(x for x in meta["cases"] if x["name"] == name)
    b, k = c["absent"]
    C, n = c["ncls"], c["nI"]
    head = _head_from_logits(torch.from_numpy(arr[name + "_logits"]), cuda)
    lab = torch.from_numpy(arr[name + "_labels"]).to(cuda)
    assert not (arr[name + "_labels"][b] == k).any()
    w1 = torch.ones(C)
    w2 = w1.clone()
    w2[k] = 1000.0
    o1 = ops.class_loss(head, lab, C, 192, w1.to(cuda), w_ce=0.0)
    o2 = ops.class_loss(head, lab, C, 192, w2.to(cuda), w_ce=0.0)
    T = (c["H"] // 8) * (c["W"] // 8)
    rows = slice(b * T, (b + 1) * T)
    assert torch.equal(o1.dlogits[rows], o2.dlogits[rows]) and o1.dlogits[rows].abs().max() > 0
    others = [i for i in range(n) if i != b and (arr[name + "_labels"][i] == k).any()]
    assert others and not torch.equal(o1.dlogits[others[0] * T:(others[0] + 1) * T], o2.dlogits[others[0] * T:(others[0] + 1) * T])
    # an image annotated as class 0 everywhere: only class 0's term has a gradient
    z = c["all_zero"]
    if z is not None:
        w3 = torch.ones(C) * 7.0
        w3[0] = 1.0
        o3 = ops.class_loss(head, lab, C, 192, w3.to(cuda), w_ce=0.0)
        assert torch.equal(o1.dlogits[z * T:(z + 1) * T], o3.dlogits[z * T:(z + 1) * T])


def _big_case(ncls, n=32, seed=0):
    rng = np.random.default_rng(1000 + ncls + seed)
    coarse = rng.integers(0, ncls, (n, 32, 32))
    lab = np.kron(coarse, np.ones((1, 8, 8), np.int64)).astype(np.int16)
    lab[1][lab[1] == 3] = 4                                   # class 3 absent from image 1
    lab[2] = 0                                                # image 2 annotated as background everywhere
    for b in range(n):
        y0 = int(rng.integers(0, 200))
        lab[b, y0:y0 + 20] = -100                             # a band without annotation
        lab[b][rng.random((256, 256)) < 0.02] = -100
    onehot = np.eye(ncls, dtype=np.float32)[np.where(lab < 0, 0, lab)].transpose(0, 3, 1, 2)
    logits = rng.standard_normal((n, ncls, 256, 256), dtype=np.float32) * 1.5
    logits += 2.0 * onehot * (rng.random((n, 1, 256, 256)) < 0.7)
    return torch.from_numpy(logits), lab


@pytest.mark.parametrize("ncls", [7, 10])
def test_class_loss_32_crops(cuda, ncls):
    logits32, lab = _big_case(ncls)
    cw = np.linspace(0.5, 2.0, ncls) if ncls == 10 else None
    _run_loss_case(cuda, logits32, lab, cw, f"32 crops x {ncls} classes at 256^2")


def _many_class_case(ncls=20, n=3, size=64):
    rng = np.random.default_rng(77)
    lab = np.kron(rng.integers(0, ncls, (n, size // 8, size // 8)), np.ones((1, 8, 8), np.int64)).astype(np.int16)
    lab[:, 10:14] = -100
    onehot = np.eye(ncls, dtype=np.float32)[np.where(lab < 0, 0, lab)].transpose(0, 3, 1, 2)
    logits = rng.standard_normal((n, ncls, size, size), dtype=np.float32) + 4.0 * onehot * (rng.random((n, 1, size, size)) < 0.8)
    return torch.from_numpy(logits), lab


def test_class_loss_more_than_16_classes(cuda):
    """Above 16 classes the kernels keep nothing per class in registers (run-time class loops): the same checks on that path."""
    logits32, lab = _many_class_case()
    _run_loss_case(cuda, logits32, lab, np.linspace(0.5, 1.5, 20), "3 crops x 20 classes at 64^2")


def test_class_loss_flags_an_image_without_annotation(cuda):
    from classpose_amd import ops
    logits32, lab = _big_case(7, n=3)
    lab[1] = -100
    head = _head_from_logits(logits32, cuda)
    with pytest.raises(ValueError, match="image 1 has no annotated pixel"):
        ops.class_loss(head, torch.from_numpy(lab).to(cuda), 7)
    lab[1] = 0
    lab[2, 5, 5] = 7
    with pytest.raises(ValueError, match="image 2 has a label outside"):
        ops.class_loss(head, torch.from_numpy(lab).to(cuda), 7)


@pytest.mark.parametrize("rows,dtype", [(1024, torch.bfloat16), (3072, torch.bfloat16), (3000, torch.bfloat16), (32768, torch.bfloat16),
                                        (1000, torch.float32), (3072, torch.float16)])
def test_head_wgrad_every_element(cuda, rows, dtype):
    from classpose_amd import _lib, ops
    L = _lib.lib().cpx_head_wgrad_slab_rows()
    assert L == 512
    P = (rows + L - 1) // L
    N = 448 if rows != 3072 else 640
    g = torch.Generator().manual_seed(rows)
    dl = torch.randn(rows, N, generator=g) * torch.logspace(-4, 0, N)[None]
    dl[::7] = 0                                                       # rows of pixels without annotation
    feat = torch.randn(rows, 256, generator=g).to(dtype)
    dW, db = ops.head_wgrad(dl.to(cuda), feat.to(cuda))
    dW2, db2 = ops.head_wgrad(dl.to(cuda), feat.to(cuda))
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    a, f = dl.double(), feat.double()
    ref, mag = a.T @ f, a.abs().T @ f.abs()
    bound = (L + P + 2) * 2.0 ** -24 * mag
    err = (dW.cpu().double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"rows {rows}, {dtype}: L = {L}, P = {P}, worst |dW - dW64| / bound = {worst:.3e}, rel-L2 = {tr.rel_l2(dW.cpu(), ref):.3e}")
    assert torch.all(err <= bound)
    refb, magb = a.sum(0), a.abs().sum(0)
    errb = (db.cpu().double() - refb).abs()
    print(f"  db: worst |db - db64| / bound = {float((errb / ((L + P + 2) * 2.0 ** -24 * magb)).max()):.3e}")
    assert torch.all(errb <= (L + P + 2) * 2.0 ** -24 * magb)


@pytest.mark.parametrize("weight_decay", [0.1, 0.0])
def test_adamw_against_the_float64_replay(cuda, weight_decay):
    from classpose_amd import ops
    arr, meta = _fixture()
    p0 = torch.from_numpy(arr["adamw_p0"]).float()
    grads = torch.from_numpy(arr["adamw_grads"]).float()
    lrs = arr["adamw_lrs"]
    ref = tr.adamw_replay(p0, grads, lrs, weight_decay=weight_decay)               # float64 on the float32 inputs the device reads
    if weight_decay == 0.1:                                                        # ... and that replay IS torch's AdamW (fixture)
        fix = tr.adamw_replay(arr["adamw_p0"], arr["adamw_grads"], lrs, weight_decay=0.1)
        assert tr.rel_l2(fix[-1], arr["adamw_traj"][-1]) <= 1e-14
    pc = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pc], lr=1e-3, weight_decay=weight_decay)
    p = p0.clone().to(cuda)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for t, (g, lr) in enumerate(zip(grads, lrs), 1):
        ops.adamw_step(p, g.to(cuda), m, v, t, float(lr), weight_decay=weight_decay)
        for grp in opt.param_groups:
            grp["lr"] = float(lr)
        pc.grad = g.clone()
        opt.step()
        if lr == 0:
            assert torch.equal(p.cpu(), p0), "lr = 0 must leave the parameters unchanged"
            continue
        upd64 = ref[t - 1] - p0.double()
        _check(f"step {t} accumulated update (weight_decay {weight_decay})", p.cpu().double() - p0.double(),
               pc.detach().double() - p0.double(), upd64)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32])
def test_patchify_f32_is_the_rounded_gather(cuda, dtype):
    from classpose_amd import ops
    g = torch.Generator().manual_seed(5)
    X = torch.randn(3, 3, 256, 256, generator=g) * 3
    got = ops.patchify_f32(X.to(cuda), dtype).cpu()
    want = X.to(dtype).reshape(3, 3, 32, 8, 32, 8).permute(0, 2, 4, 1, 3, 5).reshape(3 * 1024, 192)     # k = c*64 + i*8 + j
    bits = torch.int32 if dtype == torch.float32 else torch.int16
    assert torch.equal(got.view(bits), want.contiguous().view(bits))


def _synthetic_set(n, ncls, seed0=300):
    """uint8 crops of the synthetic slide and labels from its analytic class map: nucleus class / background / a -100 band."""
    from classpose_amd import synth
    ims, labs = [], []
    for k in range(n):
        x0, y0 = 256 * (k % 4), 256 * (k // 4)
        ims.append(synth.render_region(seed0, x0, y0, 256, 256))
        lg = synth.analytic_fields(seed0, x0, y0, 256, 256, ncls)[2]
        lab = lg.argmax(0).astype(np.int16)
        lab[(40 + 11 * k) % 200:][:24] = -100
        labs.append(lab)
    return np.stack(ims), np.stack(labs)


@pytest.fixture(scope="module")
def trainers(cuda):
    from classpose_amd import synth
    from classpose_amd.train import HeadTrainer
    made = {}

    def get(precision, ncls=7, **kw):
        key = (precision, ncls, tuple(sorted(kw.items())))
        if key not in made:
            sd = synth.make_state_dict(ncls, None, depth=2, seed=11)
            made[key] = HeadTrainer(sd, device=cuda, precision=precision, feature_batch=4, **kw)
        return made[key]
    return get


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_features_and_head_reproduce_the_forward(cuda, trainers, precision):
    """The exposed neck features followed by the head GEMM are the class columns cpx_net_forward wrote: same launch, same operands."""
    t = trainers(precision)
    ims, _ = _synthetic_set(4, 7)
    feat = t.features(ims)
    forward_head = t._head_fb.clone()                    # what cpx_net_forward wrote for these four crops (feature_batch = 4)
    head = t.head(feat)
    assert head.shape == forward_head.shape and torch.equal(head, forward_head)
    assert feat.dtype == t.dtype and feat.shape == (4096, 256) and bool(torch.isfinite(feat.float()).all())
    # a crop's features do not depend on how the crops are batched (3 crops: one padded launch; 4 + 1: two launches)
    assert torch.equal(t.features(ims[:3]), feat[:3072])
    five = t.features(np.concatenate([ims, ims[:1]]))
    assert torch.equal(five[:4096], feat) and torch.equal(five[4096:], feat[:1024])
    # float32 crops: normalise + patchify is what the uint8 path does
    from classpose_amd import ops
    x = ops.normalize_img(torch.from_numpy(ims).to(cuda)).permute(0, 3, 1, 2).contiguous()
    assert torch.equal(t.features(x.cpu().numpy()), feat)


def _replay(feat, labels, W0, b0, lrs, dtype, net_dtype, ncls, weight_decay):
    """CPU replay of HeadTrainer.step in ``dtype`` (float64: the yardstick; float32: sets the tolerance): autograd + AdamW on the
    copied features, the master weights re-rounded to the network dtype each step as the device does."""
    f = feat.to(dtype)
    W, b = W0.to(dtype).clone(), b0.to(dtype).clone()
    mW, vW, mb, vb = (torch.zeros_like(x) for x in (W, W, b, b))
    n = feat.shape[0] // 1024
    losses = []
    for t, lr in enumerate(lrs, 1):
        Wr = W.float().to(net_dtype).to(dtype).clone().requires_grad_(True)
        br = b.float().to(net_dtype).to(dtype).clone().requires_grad_(True)
        logits = tr.tokens_to_nchw(f @ Wr.T + br, 0, ncls, n, 256, 256)
        ce, tv, *_ = tr.class_loss(logits, labels)
        loss = ce + tv
        loss.backward()
        losses.append(float(loss))
        tr.adamw_step(W, Wr.grad.to(dtype), mW, vW, t, lr, weight_decay=weight_decay)
        tr.adamw_step(b, br.grad.to(dtype), mb, vb, t, lr, weight_decay=weight_decay)
    return np.array(losses), W, b


@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_twenty_steps_follow_the_float64_replay(cuda, precision):
    from classpose_amd import synth
    from classpose_amd.train import HeadTrainer
    ncls, steps = 7, 20
    sd = synth.make_state_dict(ncls, None, depth=2, seed=11)
    t = HeadTrainer(sd, device=cuda, precision=precision, feature_batch=4)
    ims, labs = _synthetic_set(8, ncls)
    feat = t.features(ims)
    lrs = [float(x) for x in np.minimum(np.linspace(0, 4e-3, 10), 2e-3)] + [2e-3] * 10
    W0, b0 = t.w.cpu().clone(), t.b.cpu().clone()
    dev_losses = np.array([t.step(feat, labs, lr)["loss"] for lr in lrs])
    lab = torch.from_numpy(labs)
    l64, W64, b64 = _replay(feat.cpu(), lab, W0, b0, lrs, torch.float64, t.dtype, ncls, t.weight_decay)
    l32, W32, b32 = _replay(feat.cpu(), lab, W0, b0, lrs, torch.float32, t.dtype, ncls, t.weight_decay)
    print(f"{precision}: loss step 1 = {dev_losses[0]:.6f} (replay {l64[0]:.6f}), step {steps} = {dev_losses[-1]:.6f} (replay {l64[-1]:.6f})")
    floor = steps * FLOOR
    _check("loss curve", dev_losses, l32, l64, floor)
    _check("final master weight update", t.w.cpu().double() - W0.double(), W32.double() - W0.double(), W64 - W0.double(), floor)
    _check("final master bias update", t.b.cpu().double() - b0.double(), b32.double() - b0.double(), b64 - b0.double(), floor)
    if l64[-1] < l64[0]:
        assert dev_losses[-1] < dev_losses[0]
    assert l64[-1] < l64[0], "the chosen inputs are meant to train"


def test_train_class_head_cached_equals_uncached_and_the_checkpoint_serves_inference(cuda, tmp_path):
    import ctypes as C
    from classpose_amd import _lib, engine, models, ops, synth
    from classpose_amd.train import HeadTrainer, train_class_head
    ncls = 7
    sd = synth.make_state_dict(ncls, None, depth=2, seed=11)
    ims, labs = _synthetic_set(8, ncls)
    runs = {}
    for cached in (True, False):
        t = HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=4)
        path, tl, vl = train_class_head(t, ims[:6], labs[:6], ims[6:], labs[6:], batch_size=4, n_epochs=4, learning_rate=2e-3,
                                        cache_features=cached, save_path=tmp_path / f"c{int(cached)}", model_name="head")
        runs[cached] = (t, path, tl, vl)
    (ta, pa, tla, vla), (tb, pb, tlb, vlb) = runs[True], runs[False]
    assert torch.equal(ta.w, tb.w) and torch.equal(ta.b, tb.b)
    assert np.array_equal(tla, tlb) and np.array_equal(vla, vlb) and len(tla) == 4 and np.all(np.isfinite(tla)) and np.all(vla > 0)
    assert not torch.equal(ta.w.cpu(), sd["out_class.weight"].reshape(-1, 256))
    for name in ("head", "checkpoint_last.pt", "checkpoint_best.pt"):
        assert (pa.parent / name).exists()
    # the saved checkpoint: reference key layout, loads as a 1x1 head, and the inference forward computes the trainer's logits
    ck = torch.load(pa, map_location="cpu", weights_only=True)
    assert set(ck) == set(sd) and ck["out_class.weight"].shape == (ncls * 64, 256, 1, 1)
    assert all(torch.equal(ck[k], sd[k]) for k in sd if not k.startswith("out_class."))
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    assert w.c.n_unet_ops == 0 and w.ncls == ncls
    four = ims[:4]
    ev = ta.evaluate(four, labs[:4], return_head=True)
    patches = ta._patches(four)
    L = _lib.lib()
    ws = torch.empty(L.cpx_net_workspace_bytes(4, w.c.dtype), dtype=torch.uint8, device=cuda)
    head = torch.empty((4 * 1024, w.c.ld_head), dtype=torch.float32, device=cuda)
    _lib.check(L.cpx_net_forward(C.byref(w.c), _lib.ptr(patches), 4, _lib.ptr(head), _lib.ptr(ws), ws.numel(),
                                 torch.cuda.current_stream(cuda).cuda_stream), "net_forward")
    assert torch.equal(head[:, 192:192 + ncls * 64], ev["head"][:, 192:192 + ncls * 64])
    assert torch.equal(head[:, :192], ev["head"][:, :192])            # the frozen flow head is untouched
    # smoke: ClassposeModel accepts the checkpoint and returns class maps of the trained class count
    m = models.ClassposeModel(pretrained_model=str(pa), device=cuda, precision="bf16", max_batch_tiles=2)
    assert m.nclasses == ncls
    masks, flows, class_masks, _styles = m.eval(ims[0])
    assert class_masks.shape == (256, 256) and flows[3].shape == (ncls, 256, 256) and 0 <= class_masks.min() and class_masks.max() < ncls
    # save_only_trainable_params keeps the two trained tensors
    ta.save(tmp_path / "only.pt", save_only_trainable_params=True)
    assert set(torch.load(tmp_path / "only.pt", weights_only=True)) == {"out_class.weight", "out_class.bias"}


def test_cli_trains_in_a_child_process(cuda, tmp_path):
    from classpose_amd import engine, synth
    ncls = 5
    sd = synth.make_state_dict(1, None, depth=2, seed=12)              # a plain backbone: the CLI initialises the head
    torch.save(sd, tmp_path / "backbone.pt")
    ims, labs = _synthetic_set(16, ncls)
    np.save(tmp_path / "X.npy", ims)
    np.save(tmp_path / "Y.npy", labs)
    cmd = [sys.executable, "-m", "classpose_amd.entrypoints.train_head", "--images", str(tmp_path / "X.npy"), "--labels",
           str(tmp_path / "Y.npy"), "--test_images", str(tmp_path / "X.npy"), "--test_labels", str(tmp_path / "Y.npy"),
           "--pretrained_model", str(tmp_path / "backbone.pt"), "--nclasses", str(ncls), "--n_epochs", "3", "--batch_size", "8",
           "--learning_rate", "1e-3", "--class_weights", "0.5", "1", "1", "2", "1", "--save_path", str(tmp_path), "--model_name", "m",
           "--device", "cuda:0"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = tmp_path / "m" / "m"
    assert r.stdout.strip().splitlines()[-1] == str(out) and out.exists()
    ck = torch.load(out, map_location="cpu", weights_only=True)
    assert ck["out_class.weight"].shape == (ncls * 64, 256, 1, 1) and ck["W3"].shape == (ncls * 64, ncls, 8, 8)
    w = engine.NetWeights.from_state_dict(ck, "bf16", cuda)
    assert w.ncls == ncls and w.c.n_unet_ops == 0
