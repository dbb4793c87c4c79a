"""The parameter groups of the trainers (train.LinearHead, train.NeckParams, train_unet.UNetParams): for every combination of
groups, what ``save(..., save_only_trainable_params=True)`` writes is the union of the groups' ``keys``, every one of those tensors
moves in a step, and nothing else in ``state_dict()`` does.  Depth-1 network, bf16, 2 crops, 2 steps."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NCLS = 3
FTS = [16, 24]
CLASS_KEYS = {"out_class.weight", "out_class.bias"}
FLOW_KEYS = {"out.weight", "out.bias"}
NECK_KEYS = {"encoder.neck.0.weight", "encoder.neck.1.weight", "encoder.neck.1.bias", "encoder.neck.2.weight", "encoder.neck.3.weight",
             "encoder.neck.3.bias"}
CONFIGS = {"1x1": (False, {}, CLASS_KEYS),
           "1x1+flow": (False, dict(train_flow_head=True), CLASS_KEYS | FLOW_KEYS),
           "1x1+flow+neck": (False, dict(train_flow_head=True, train_neck=True), CLASS_KEYS | FLOW_KEYS | NECK_KEYS),
           "unet": (True, {}, None),
           "unet+flow": (True, dict(train_flow_head=True), FLOW_KEYS)}


def _trainer(cuda, unet, kw):
    from classpose_amd import synth
    from classpose_amd.train import HeadTrainer
    from classpose_amd.train_unet import UNetHeadTrainer
    sd = synth.make_state_dict(NCLS, None, depth=1, seed=41)
    if unet:
        return UNetHeadTrainer(sd, device=cuda, precision="bf16", feature_batch=2, feature_transformation_structure=FTS, **kw)
    return HeadTrainer(sd, device=cuda, precision="bf16", feature_batch=2, **kw)


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    ims = torch.randn(2, 3, 256, 256, generator=torch.Generator().manual_seed(1))
    labs = np.kron(rng.integers(0, NCLS, (2, 16, 16)), np.ones((1, 16, 16), np.int64)).astype(np.int16)
    labs[:, 40:49] = -100
    g = torch.Generator().manual_seed(6)
    mask = (torch.rand(2, 1, 16, 16, generator=g) > 0.5).float().repeat_interleave(16, 2).repeat_interleave(16, 3)
    flow = torch.tanh(torch.randn(2, 2, 256, 256, generator=g)) * mask
    return ims, labs, torch.cat([mask, flow], 1).contiguous()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_saved_keys_are_the_groups_keys_and_only_they_move(cuda, data, name, tmp_path):
    from classpose_amd.train_unet import unet_plan
    ims, labs, tg = data
    unet, kw, expected = CONFIGS[name]
    if unet:
        expected = {k + s for k, *_ in unet_plan(FTS, NCLS * 64) for s in (".weight", ".bias")} | (expected or set())
    t = _trainer(cuda, unet, kw)
    loaded = {k: torch.as_tensor(v).clone() for k, v in t.sd.items()}            # the checkpoint as loaded
    x = t.backbone_features(ims) if t.neck is not None else t.features(ims)
    for _ in range(2):
        t.step(x, labs, 1e-3, **(dict(flow_targets=tg) if t.flow is not None else {}))
    assert t.n_steps == 2 and [g for g in (t.flow, t.neck) if g is not None] == t.groups[1:]
    union = {k for g in t.groups for k in g.keys}
    assert sum(len(g.keys) for g in t.groups) == len(union), "two groups own one key"
    t.save(tmp_path / "trainable.pt", save_only_trainable_params=True)
    saved = torch.load(tmp_path / "trainable.pt", map_location="cpu", weights_only=True)
    assert set(saved) == union == expected
    after = t.state_dict()
    assert set(after) == set(loaded)
    for k, v in after.items():
        if k in expected:
            assert not torch.equal(v, loaded[k].reshape(v.shape)), f"{k} trains but did not move"
            assert torch.equal(saved[k], v), f"{k}: the saved tensor is not state_dict()'s"
        else:
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(loaded[k])), f"{k} does not train but changed"


def test_the_compatibility_names_are_views_of_the_groups(cuda):
    t = _trainer(cuda, False, dict(train_flow_head=True, train_neck=True))
    assert len(t.groups) == 3 and t.groups[1] is t.flow and t.groups[2] is t.neck
    assert t.w is t.groups[0].w and t.b is t.groups[0].b and t.m_w is t.groups[0].m_w
    u = _trainer(cuda, True, {})
    assert u.params is u.groups[0].params and u.grads is u.groups[0].grads and u.layout is u.groups[0].layout
