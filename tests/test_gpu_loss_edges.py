"""The loss kernels and AdamW of csrc/cpx_train.hip at the shapes and values the older tests (tests/test_gpu_train.py,
tests/test_gpu_flow_train.py: square images of 32^2, 64^2 and 256^2, at most 32 of them) never reach: the second chunk of 256 images of
k_loss_finish / k_seg_finish, H != W in lane_label, a last workgroup of fewer than 64 tokens behind a full one, both sides of the
16-class switch between the register and the general kernels and the 64-class limit, a Tversky term inside the clip, saturated and
all-equal logits -- and every element of both gradients against float64 where those tests take one norm.

ops.class_loss, per element of dlogits.  The kernel computes d = p (G - S) + wy (p - [c == y]) with p = expf(z_c - lse),
G = the Tversky factor of the pixel's (image, class), S = sum_c p_c G_c, wy = w[y] w_ce / sum w[y].  Its error scales with
    A_c = p_c f_c (|G_c| + Sa) + wy (p_c f_c + |p_c - [c == y]|),    f_c = 1 + |z_c - lse|,    Sa = sum_c p_c f_c |G_c|
(f: an absolute error e of the exponent is a relative error e of p; a p below 2^-126, the smallest normal float32, has no relative
precision and counts as 2^-126 / u).  In units of u = 2^-24: the exponent (z_c - max) - ls, ls = logf(s), carries the sum of ncls
exponentials (ncls + 1), expf and logf (2 each) and the two differences, rounded at |z_c - max| <= f_c + ln 64 <= 4.2 f_c:
e_p = ncls + 9 per p.  (The kernels keep max and ls apart: lse = max + ls rounded at the size of the logits was a relative error of 2^-18 of every p at logits of +-80, the same
for all pixels with the same logits, and put tp 2.3e-6 away where the rule of tests/test_gpu_train.py allows 9.5e-7 -- the case
"plus or minus 80" below found it.)  d holds p twice (p and S) and G, whose float64 sums of tp, fp, fn inherit the e_p of their terms
through a derivative of condition <= 4; the class sum S adds ncls and the remaining products and sums 8:
    |d - d64| <= K u A,   K = 6 (ncls + 9) + ncls + 8,
and beside it the project's factor 4 on the worst element: max |d - d64| / (u A) <= max(4 max |torch CPU float32 - d64| / (u A), 1).
Rows of pixels without annotation are exactly zero, two runs are bitwise equal, the loss values follow the rule of
tests/test_gpu_train.py.  The float64 formula that A is built from is itself compared with autograd (1e-12) in every case.

ops.seg_loss, per element: the flow planes d = (z - 5 t) g: two roundings on the scale of the operands (the product and the difference;
one where the compiler contracts them) and two on the scale of the result (times g, and g's own rounding to float32):
    |d - d64| <= 2 u (|z| + 5 |t|) g + 2 u |d64|;
the cellprob plane d = (sig - y) g: expf (2 u), 1 + e, the division, then the difference and the product with the rounded g:
    |d - d64| <= u g (5 sig + 3 |sig - y|) + 2^-126 g      (2^-126: below it float32 has no relative precision; expf(-100) lies there)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

import flow_train_reference as fr
import test_gpu_train as tt
import train_reference as tr

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ALPHA, GAMMA, EPS = 0.3, 1.33, 1e-6

SHAPES = [(1, 8, 8, 2),          # one token
          (3, 8, 24, 7),         # H != W
          (2, 40, 24, 10),       # 15 tokens
          (1, 72, 64, 7),        # 72 tokens: a full workgroup and one of 8
          (300, 8, 8, 7),        # image chunks 256 + 44, n_bc = 2100
          (257, 16, 8, 10),      # image chunks 256 + 1
          (2, 16, 24, 16),       # the last class count of the register kernels
          (2, 16, 24, 17),       # the first class count of the general kernels
          (2, 16, 24, 64)]       # the general kernels' class limit


def _class_case(nI, H, W, ncls, seed):
    """labels in blocks of 4 x 4 pixels (so a token holds up to four classes) with a band of two rows and 5 % scattered pixels of -100"""
    rng = np.random.default_rng(seed)
    lab = np.kron(rng.integers(0, ncls, (nI, H // 4, W // 4)), np.ones((1, 4, 4), np.int64)).astype(np.int16)
    lab[:, H // 4:H // 4 + 2] = -100
    lab[rng.random((nI, H, W)) < 0.05] = -100
    onehot = np.eye(ncls, dtype=np.float32)[np.where(lab < 0, 0, lab)].transpose(0, 3, 1, 2)
    logits = rng.standard_normal((nI, ncls, H, W), dtype=np.float32) * np.float32(1.5)
    logits += np.float32(2.0) * onehot * (rng.random((nI, 1, H, W)) < 0.7)
    return torch.from_numpy(logits.astype(np.float32)), lab


def _formula64(z32, labels, cw, w_ce=1.0, w_tv=1.0):
    """the kernel's formula in float64 on the float32 logits -> (d, A, L): d loss / d logits, its error scale, the largest |lse|"""
    z = z32.double()
    n, C, H, W = z.shape
    lab = torch.from_numpy(labels).long()
    use = lab != -100
    onehot = torch.nn.functional.one_hot(torch.where(use, lab, torch.zeros_like(lab)), C).permute(0, 3, 1, 2).double()
    usef = use.double()[:, None]
    lse = torch.logsumexp(z, 1, keepdim=True)
    p, f = torch.exp(z - lse), 1.0 + (z - lse).abs()
    w = torch.ones(C, dtype=torch.float64) if cw is None else torch.as_tensor(cw).double()
    tp, fp, fn = (p * onehot * usef).sum((2, 3)), (p * (1 - onehot) * usef).sum((2, 3)), ((1 - p) * onehot * usef).sum((2, 3))
    D = tp + ALPHA * fp + (1 - ALPHA) * fn
    raw = 1.0 - tp / D
    inside = (raw >= EPS) & (raw <= 1 - EPS)
    ig = 1.0 / GAMMA
    dl = torch.where(inside, ig * raw.clamp_min(1e-300).pow(ig - 1.0) * w[None] * w_tv / (n * C), torch.zeros_like(raw))
    ga = dl * (-(ALPHA * fp + (1 - ALPHA) * fn) / D ** 2 - (1 - ALPHA) * tp / D ** 2)
    gb = dl * ALPHA * tp / D ** 2
    G = ga[:, :, None, None] * onehot + gb[:, :, None, None] * (1 - onehot)
    S, Sa = (p * G).sum(1, keepdim=True), (p * f * G.abs()).sum(1, keepdim=True)
    wy = (w[torch.where(use, lab, torch.zeros_like(lab))] * use.double())[:, None] * (w_ce / float((w[lab[use]]).sum()))
    d = (p * (G - S) + wy * (p - onehot)) * usef
    A = (p * f * (G.abs() + Sa) + wy * (p * f + (p - onehot).abs())) * usef
    A = A + 2.0 ** -126 / U * (G.abs() + Sa + wy) * usef              # a p below 2^-126 has no relative precision in float32 (logits of -80)
    return d, A, float(lse.abs().max())


def _check_class(dev, z32, labels, cw, tag, w_ce=1.0, w_tv=1.0):
    from classpose_amd import ops
    n, C, H, W = z32.shape
    head = tt._head_from_logits(z32, dev)
    lab = torch.from_numpy(labels).to(dev)
    cwt = None if cw is None else torch.from_numpy(np.float32(cw))
    run = lambda: ops.class_loss(head, lab, C, 192, None if cwt is None else cwt.to(dev), w_ce=w_ce, w_tv=w_tv)
    o, o2 = run(), run()
    assert torch.equal(tr.tokens_to_nchw(head.cpu(), 192, C, n, H, W), z32)                  # the logits the device read
    cw64 = None if cwt is None else cwt.double()
    r64 = tr.loss_and_grad(z32, torch.from_numpy(labels), cw64, w_ce=w_ce, w_tv=w_tv)
    r32 = tr.loss_and_grad_f32(z32, torch.from_numpy(labels), cw64, w_ce=w_ce, w_tv=w_tv)
    d64, A, L = _formula64(z32, labels, cw64, w_ce, w_tv)
    form = float((d64 - r64["dlogits"]).abs().max() / r64["dlogits"].abs().max().clamp_min(1e-300))
    print(f"{tag}: ce = {o.ce.item():.9g}, tversky = {o.tversky.item():.9g}; the float64 formula against autograd {form:.2e}; largest |lse| {L:.1f}")
    assert form <= 1e-12
    for k in ("ce", "tversky", "tp", "fp", "fn"):
        tt._check(k, getattr(o, k).cpu(), r32[k], r64[k])
    assert torch.equal(o.n_annot.cpu().long(), torch.from_numpy((labels != -100).reshape(n, -1).sum(1)))
    g_dev = tr.tokens_to_nchw(o.dlogits.cpu(), 0, C, n, H, W)
    K = 6 * (C + 9) + C + 8
    ratio = lambda x: torch.where(A > 0, (x.double() - r64["dlogits"]).abs() / (U * A).clamp_min(1e-300),
                                  torch.where(x.double() == r64["dlogits"], 0.0, float("inf")).double())
    r_dev, r_cpu = ratio(g_dev), ratio(r32["dlogits"])
    at = np.unravel_index(int(r_dev.argmax()), r_dev.shape)
    w_dev, w_cpu = float(r_dev.max()), float(r_cpu.max())
    print(f"  dlogits, worst |d - d64| / (2^-24 A): device {w_dev:.3f} at (image, class, y, x) = {tuple(int(i) for i in at)}, torch CPU float32 {w_cpu:.3f}; "
          f"allowed min(K = {K:.0f}, max(4 CPU, 1)) = {min(K, max(4 * w_cpu, 1.0)):.3f}; relative L2 {tr.rel_l2(g_dev, r64['dlogits']):.2e}")
    assert bool(torch.isfinite(g_dev).all()) and w_dev <= K and w_dev <= max(4 * w_cpu, 1.0)
    assert torch.all(g_dev.permute(0, 2, 3, 1)[torch.from_numpy(labels == -100)] == 0)        # not annotated: exactly zero
    for k in ("ce", "tversky", "tp", "fp", "fn", "dlogits", "n_annot"):
        assert torch.equal(getattr(o, k), getattr(o2, k)), k
    return o, r64


@pytest.mark.parametrize("weights", [False, True])
@pytest.mark.parametrize("nI,H,W,ncls", SHAPES)
def test_class_loss_shapes(cuda, nI, H, W, ncls, weights):
    z32, lab = _class_case(nI, H, W, ncls, 500 + nI + H + ncls)
    T = (H // 8) * (W // 8)
    assert (lab == -100).any() and all((lab[b] != -100).any() for b in range(nI))
    _check_class(cuda, z32, lab, np.linspace(0.5, 2.0, ncls) if weights else None, f"{nI} images of {H} x {W} ({T} tokens), {ncls} classes")


@pytest.mark.parametrize("what", ["plus or minus 80", "all equal"])
def test_class_loss_saturated_and_equal_logits(cuda, what):
    _z, lab = _class_case(2, 16, 24, 7, 41)
    rng = np.random.default_rng(42)
    if what == "all equal":
        z32 = torch.full((2, 7, 16, 24), 3.0)
    else:
        z32 = torch.from_numpy(np.where(rng.random((2, 7, 16, 24)) < 0.5, np.float32(80.0), np.float32(-80.0)).astype(np.float32))
    _check_class(cuda, z32, lab, np.linspace(0.5, 2.0, 7), f"logits {what}")


def test_class_loss_a_perfectly_predicted_image_is_clipped(cuda):
    """image 0: +40 on the labelled class: p = 1 there, e^-40 elsewhere, raw Tversky loss of about 1e-17 < eps for every class -- the
    clip passes no gradient: with the cross-entropy off its rows are exactly zero while image 1 (random logits) has a gradient"""
    z32, lab = _class_case(2, 16, 24, 7, 43)
    onehot = np.eye(7, dtype=np.float32)[np.where(lab[0] < 0, 0, lab[0])].transpose(2, 0, 1)
    z32[0] = torch.from_numpy(40.0 * onehot)
    assert all((lab[0] == c).any() for c in range(7))
    o, r64 = _check_class(cuda, z32, lab, None, "image 0 predicted perfectly, w_ce = 0", w_ce=0.0)
    raw = tr.raw_tversky(r64["tp"], r64["fp"], r64["fn"])
    T = 2 * 3
    print(f"  raw Tversky losses of image 0: {float(raw[0].min()):.2e} .. {float(raw[0].max()):.2e}; of image 1: {float(raw[1].min()):.3f} .. {float(raw[1].max()):.3f}")
    assert float(raw[0].max()) < EPS and float(raw[1].min()) > 0.1
    assert not bool(o.dlogits[:T].any()) and float(o.dlogits[T:].abs().max()) > 0 and not bool(r64["dlogits"][0].any())
    o2, _ = _check_class(cuda, z32, lab, None, "image 0 predicted perfectly, w_ce = 1")
    assert float(o2.dlogits[:T].abs().max()) > 0


def test_class_loss_flags_image_299(cuda):
    """status[1], the first flagged image, is found in the second chunk of 256 images"""
    from classpose_amd import ops
    z32, lab = _class_case(300, 8, 8, 7, 44)
    head = tt._head_from_logits(z32, cuda)
    empty = lab.copy()
    empty[299] = -100
    with pytest.raises(ValueError, match="image 299 has no annotated pixel"):
        ops.class_loss(head, torch.from_numpy(empty).to(cuda), 7)
    o = ops.class_loss(head, torch.from_numpy(empty).to(cuda), 7, check_status=False)
    assert int(o.status[1]) == 299 and int(o.status[0]) != 0 and int(o.n_annot[299]) == 0
    bad = lab.copy()
    bad[299, 7, 7] = 7
    with pytest.raises(ValueError, match="image 299 has a label outside"):
        ops.class_loss(head, torch.from_numpy(bad).to(cuda), 7)
    o = ops.class_loss(head, torch.from_numpy(lab).to(cuda), 7, check_status=False)
    assert int(o.status[0]) == 0 and int(o.status[1]) == -1


# ---- seg loss ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", ["random", "plus or minus 100"])
@pytest.mark.parametrize("nI,H,W", [(300, 8, 8), (2, 8, 24), (1, 72, 64)])
def test_seg_loss_shapes(cuda, nI, H, W, logits):
    from classpose_amd import ops
    rng = np.random.default_rng(600 + nI + H)
    z = rng.standard_normal((nI, 3, H, W), dtype=np.float32) * np.float32(3.0)
    if logits != "random":
        z = np.where(rng.random(z.shape) < 0.5, np.float32(100.0), np.float32(-100.0)).astype(np.float32)
    tg = np.stack([rng.random((nI, H, W), dtype=np.float32), *(np.clip(rng.standard_normal((2, nI, H, W), dtype=np.float32) * 0.5, -1, 1))], 1)
    half = rng.random((nI, H, W)) < 0.25
    tg[:, 0][half] = np.float32(0.5)                                  # exactly 0.5 is background: the mask is t > 0.5
    z32, tg = torch.from_numpy(z), torch.from_numpy(np.ascontiguousarray(tg))
    head = fr.head_with_flow_logits(z32, ncls=3, seed=1).to(cuda)
    o, o2 = ops.seg_loss(head, tg.to(cuda)), ops.seg_loss(head, tg.to(cuda))
    assert torch.equal(tr.tokens_to_nchw(head.cpu(), 0, 3, nI, H, W), z32)
    r64, r32 = fr.seg_loss_and_grad(z32, tg, torch.float64), fr.seg_loss_and_grad(z32, tg, torch.float32)
    print(f"{nI} images of {H} x {W}, logits {logits}: flow = {o.flow.item():.9g} (float64 {float(r64['flow']):.9g}), cp = {o.cp.item():.9g} "
          f"(float64 {float(r64['cp']):.9g}); pixels with a mask target of exactly 0.5: {int(half.sum())}")
    for k in ("flow", "cp", "dlogits"):
        assert bool(torch.isfinite(getattr(o, k)).all()) and torch.equal(getattr(o, k), getattr(o2, k)), k
    tt._check("flow", o.flow.cpu(), r32["flow"], r64["flow"])
    tt._check("cp", o.cp.cpu(), r32["cp"], r64["cp"])
    d = tr.tokens_to_nchw(o.dlogits.cpu(), 0, 3, nI, H, W).double()
    n = float(nI * H * W)
    zz, t = z32.double(), tg.double()
    g_flow, g_cp = 1.0 / (2.0 * n), 1.0 / n
    y = (t[:, 0] > 0.5).double()
    sig = torch.sigmoid(zz[:, 2])
    want = torch.cat([(zz[:, :2] - 5.0 * t[:, 1:]) * g_flow, ((sig - y) * g_cp)[:, None]], 1)
    form = float((want - r64["dlogits"]).abs().max())
    bound = torch.cat([2 * U * (zz[:, :2].abs() + 5.0 * t[:, 1:].abs()) * g_flow + 2 * U * want[:, :2].abs(),
                       (U * g_cp * (5 * sig + 3 * (sig - y).abs()) + 2.0 ** -126 * g_cp)[:, None]], 1)
    err = (d - r64["dlogits"]).abs()
    worst = [float((err[:, k] / bound[:, k]).max()) for k in range(3)]
    at_half = bool((y[torch.from_numpy(half)] == 0).all())
    print(f"  worst |d - d64| / bound: dY {worst[0]:.3f}, dX {worst[1]:.3f}, cellprob {worst[2]:.3f}; the float64 formula against autograd {form:.1e}; "
          f"targets of 0.5 count as background {at_half}")
    assert form <= 1e-18 + 1e-12 * float(want.abs().max()) and at_half and max(worst) <= 1.0


# ---- AdamW -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grad", ["random", "zero", "1e30"])
@pytest.mark.parametrize("step", [1, 10000])
@pytest.mark.parametrize("n", [1, 255, 257])
def test_adamw_sizes_steps_and_gradients(cuda, n, step, grad):
    """one step of n parameters (one lane, one short of a workgroup, one over) from the state of step - 1 against the float64 replay
    and torch.optim.AdamW, by the rule of test_adamw_against_the_float64_replay.  A gradient of 1e30: g^2 overflows the float32 second
    moment in torch and on the device alike (the float64 replay moves by lr where they do not move): the device must equal torch"""
    from classpose_amd import ops
    g = torch.Generator().manual_seed(1000 * n + step)
    p0 = torch.randn(n, generator=g)
    gr = {"random": torch.randn(n, generator=g) * 0.1, "zero": torch.zeros(n), "1e30": torch.full((n,), 1e30)}[grad]
    m0 = torch.zeros(n) if step == 1 else torch.randn(n, generator=g) * 0.05
    v0 = torch.zeros(n) if step == 1 else torch.rand(n, generator=g) * 0.01
    lr, wd = 1e-3, 0.1
    p64, m64, v64 = p0.double().clone(), m0.double().clone(), v0.double().clone()
    tr.adamw_step(p64, gr.double(), m64, v64, step, lr, weight_decay=wd)
    pc = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pc], lr=lr, weight_decay=wd)
    opt.state[pc] = {"step": torch.tensor(float(step - 1)), "exp_avg": m0.clone(), "exp_avg_sq": v0.clone()}
    pc.grad = gr.clone()
    opt.step()
    p, m, v = p0.clone().to(cuda), m0.clone().to(cuda), v0.clone().to(cuda)
    sentinel = torch.full((n + 64,), 7.0, device=cuda)
    sentinel[:n] = p
    ops.adamw_step(sentinel[:n], gr.to(cuda), m, v, step, lr, weight_decay=wd)
    p = sentinel[:n].cpu()
    assert bool((sentinel[n:] == 7.0).all())                                         # nothing behind the last parameter is written
    near = float((p.double() - pc.detach().double()).abs().max() / p0.abs().max())
    print(f"n = {n}, step {step}, gradient {grad}: largest |device - torch CPU float32| / max |p| = {near:.2e}")
    assert bool(torch.isfinite(p).all()) and near <= 4 * U
    if grad == "1e30":
        assert bool(torch.isinf(v).all()) and bool(torch.isinf(opt.state[pc]["exp_avg_sq"]).all())
    else:
        tt._check("update", p.double() - p0.double(), pc.detach().double() - p0.double(), p64 - p0.double())
        tt._check("exp_avg", m.cpu(), opt.state[pc]["exp_avg"], m64)
        tt._check("exp_avg_sq", v.cpu(), opt.state[pc]["exp_avg_sq"], v64)
