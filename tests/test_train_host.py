"""Host-side checks of the head-training feature (no GPU): the float64 restatement of the two losses (tests/train_reference.py,
the yardstick of tests/test_gpu_train.py) against the fixture minted from the reference's own functions
(tests/golden/make_golden_train.py), the learning-rate schedule, the AdamW restatement, the checkpoint layout and the CLI parser."""
import json
import os
import re

import numpy as np
import pytest
import torch

import train_reference as tr
from classpose_amd import _lib, engine, synth
from classpose_amd import train as cptrain
from classpose_amd.entrypoints import train_head as cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "reference_train.json")) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLD, "reference_train.npz")), meta


def test_fixture_covers_the_cases_the_feature_promises(gold):
    arr, meta = gold
    cases = {c["name"]: c for c in meta["cases"]}
    assert {c["ncls"] for c in cases.values()} == {7, 10}
    assert {c["weights"] for c in cases.values()} == {True, False}
    assert any(c["absent"] for c in cases.values()) and any(c["all_zero"] is not None for c in cases.values())
    for c in cases.values():
        lab = arr[c["name"] + "_labels"]
        assert (lab == -100).any() and c["min_clip_edge_distance"] >= 0.1
    assert meta["all_ignored_image_tversky_is_nan"] and meta["all_ignored_batch_ce_is_nan"]


def test_restatement_equals_the_reference_losses_and_gradient(gold):
    arr, meta = gold
    for c in meta["cases"]:
        n = c["name"]
        logits = torch.from_numpy(arr[n + "_logits"]).double()
        labels = torch.from_numpy(arr[n + "_labels"])
        cw = arr[n + "_weights"] if c["weights"] else None
        r = tr.loss_and_grad(logits, labels, cw)
        assert abs(float(r["ce"]) - c["ce"]) <= 1e-12 * abs(c["ce"]), n
        assert abs(float(r["tversky"]) - c["tversky"]) <= 1e-12 * abs(c["tversky"]), n
        assert abs(float(r["loss"]) - c["loss"]) <= 1e-12 * abs(c["loss"]), n
        assert tr.rel_l2(r["dlogits"], arr[n + "_dlogits"]) <= 1e-12, n
        # not-annotated pixels carry no gradient; an absent class (raw loss exactly 1) carries no Tversky gradient
        g = r["dlogits"].numpy()
        assert np.all(g.transpose(0, 2, 3, 1)[arr[n + "_labels"] == -100] == 0)
        raw = tr.raw_tversky(r["tp"], r["fp"], r["fn"]).numpy()
        assert int((raw == 1.0).sum()) == c["n_absent"]


def test_token_layout_round_trip():
    x = torch.arange(2 * 3 * 16 * 24, dtype=torch.float32).reshape(2, 3, 16, 24)
    tok = tr.nchw_to_tokens(x)
    assert tok.shape == (2 * 2 * 3, 3 * 64)
    assert tok[1 * 6 + 1 * 3 + 2, 2 * 64 + 5 * 8 + 7] == x[1, 2, 8 + 5, 16 + 7]
    assert torch.equal(tr.tokens_to_nchw(tok, 0, 3, 2, 16, 24), x)


def test_lr_schedule_equals_the_reference(gold):
    arr, meta = gold
    for e in meta["lr"]:
        mine = cptrain.lr_schedule(e["learning_rate"], e["n_epochs"])
        ref = arr[f"lr_{e['n_epochs']}"]
        assert mine.shape == ref.shape == (e["n"],) and np.array_equal(mine, ref)
    assert cptrain.lr_schedule(1e-3, 5)[0] == 0.0 and len(cptrain.lr_schedule(1e-3, 5)) == 10


def test_adamw_restatement_equals_torch(gold):
    arr, meta = gold
    traj = tr.adamw_replay(arr["adamw_p0"], arr["adamw_grads"], arr["adamw_lrs"], weight_decay=meta["adamw"]["weight_decay"])
    for mine, ref in zip(traj, arr["adamw_traj"]):
        assert tr.rel_l2(mine, ref) <= 1e-14
    assert np.array_equal(traj[0].numpy(), arr["adamw_p0"])          # lr = 0 in the first epoch: nothing moves


def test_state_dict_keeps_the_reference_layout(tmp_path):
    sd = synth.make_state_dict(7, None, depth=1, seed=2)
    out, ncls = cptrain.prepare_state_dict(dict(sd))
    assert ncls == 7 and set(out) == set(sd)
    # a plain Cellpose-SAM backbone gets a seeded 1x1 head in the reference's layout
    plain = synth.make_state_dict(1, None, depth=1, seed=2)
    assert "out_class.weight" not in plain
    with pytest.raises(ValueError):
        cptrain.prepare_state_dict(dict(plain))
    a, n = cptrain.prepare_state_dict(dict(plain), nclasses=5, head_seed=3)
    b, _ = cptrain.prepare_state_dict(dict(plain), nclasses=5, head_seed=3)
    assert n == 5 and a["out_class.weight"].shape == (320, 256, 1, 1) and a["out_class.bias"].shape == (320,)
    assert a["W3"].shape == (320, 5, 8, 8) and torch.equal(a["out_class.weight"], b["out_class.weight"])
    assert float(a["out_class.weight"].abs().max()) <= 1 / 16
    fts, n_classes, depth = engine.NetWeights.infer_structure(a)
    assert fts is None and n_classes == 5 and depth == 1
    w = engine.NetWeights.from_state_dict(a, "fp32", "cpu")           # host-side packing accepts it as a 1x1 head
    assert w.c.n_unet_ops == 0 and w.c.n_head_cols == 192 + 320
    with pytest.raises(ValueError):
        cptrain.prepare_state_dict(dict(sd), nclasses=9)
    unet = synth.make_state_dict(3, [32, 64], depth=1, seed=2)
    with pytest.raises(NotImplementedError):
        cptrain.prepare_state_dict(unet)
    # a path works like a dict
    p = tmp_path / "ck.pt"
    torch.save(sd, p)
    out2, _ = cptrain.prepare_state_dict(p)
    assert all(torch.equal(out2[k], sd[k]) for k in sd)


def test_dataset_checks_name_the_image():
    im = np.zeros((3, 256, 256, 3), np.uint8)
    lab = np.zeros((3, 256, 256), np.int16)
    lab[2] = -100
    with pytest.raises(ValueError, match="image 2 has no annotated pixel"):
        cptrain._check_dataset(im, lab, "training")
    with pytest.raises(ValueError):
        cptrain._check_dataset(im[:, :128], lab, "training")
    with pytest.raises(ValueError):
        cptrain._check_dataset(im, lab.astype(np.float32), "training")


def test_cli_arguments():
    a = cli.build_parser().parse_args("--images X.npy --labels Y.npy --pretrained_model C --save_path D --model_name N".split())
    assert (a.n_epochs, a.batch_size, a.learning_rate, a.weight_decay) == (100, 8, 5e-5, 0.1)
    assert a.cache_features and a.precision == "bf16" and a.nclasses is None and a.class_weights is None and a.device == "cuda:0"
    a = cli.build_parser().parse_args("--images X --labels Y --test_images TX --test_labels TY --pretrained_model C --nclasses 7 "
                                      "--n_epochs 3 --batch_size 4 --learning_rate 1e-3 --weight_decay 0 --class_weights 1 2 3 4 5 6 7 "
                                      "--precision fp32 --no-cache_features --save_path D --model_name N --device cuda:1".split())
    assert not a.cache_features and a.class_weights == [1, 2, 3, 4, 5, 6, 7] and a.nclasses == 7 and a.precision == "fp32"
    assert (a.test_images, a.test_labels, a.n_epochs, a.weight_decay, a.device) == ("TX", "TY", 3, 0.0, "cuda:1")
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--images", "X"])


def test_training_entry_points_are_declared_exported_and_bound():
    names = {"cpx_net_neck_offset", "cpx_patchify_f32", "cpx_class_loss_workspace_bytes", "cpx_class_loss", "cpx_head_wgrad_slab_rows",
             "cpx_head_wgrad_workspace_bytes", "cpx_head_wgrad", "cpx_adamw_step"}
    hdr = open(os.path.join(ROOT, "include", "classpose_hip.h")).read()
    assert names <= set(re.findall(r"\b(cpx_[a-z0-9_]+)\s*\(", hdr)) and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert L.cpx_head_wgrad_slab_rows() == 512
    # host-only queries: sizes and offsets need no device
    assert L.cpx_net_neck_offset(0, 0) == 0 and L.cpx_net_neck_offset(8, 3) == 0
    for dt, es in ((_lib.DT_BF16, 2), (_lib.DT_F16, 2), (_lib.DT_F32, 4)):
        off = L.cpx_net_neck_offset(8, dt)
        assert off > 0 and off % 256 == 0 and off + 8 * 1024 * 256 * es <= L.cpx_net_workspace_bytes(8, dt)
    assert L.cpx_class_loss_workspace_bytes(32, 256, 256, 7) >= 32 * 16 * 25 * 8
    assert L.cpx_class_loss_workspace_bytes(1, 250, 256, 7) == 0 and L.cpx_class_loss_workspace_bytes(1, 256, 256, 65) == 0
    assert L.cpx_head_wgrad_workspace_bytes(1000, 448) >= 2 * 448 * 256 * 4 + 2 * 448 * 8
    assert L.cpx_head_wgrad_workspace_bytes(1000, 100) == 0
