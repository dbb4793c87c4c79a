"""GPU: a plain ``bench.py`` run prints the headline line only, and ``--dump-outputs`` writes the last timed step's outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_headline_and_dumped_outputs(cuda, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CPX_DIST_BACKEND")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "wsi_tiles_per_sec" and line["unit"] == "tiles/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 2 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(8 / (line["ms_per_step"] * 1e-3), rel=1e-6)
    assert not {"roofline", "side_lines", "cpu_baseline"} & set(line)          # what only --full measures

    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert sorted(got) == ["cellprob", "class_masks", "dP", "logits", "masks", "nlabels", "records"]
    assert sum(a.nbytes for a in got.values()) <= 64 * 10**6
    assert all(a.dtype == (np.float64 if n == "records" else np.float32) for n, a in got.items())
    assert got["masks"].shape == (8, 256, 256) and got["dP"].shape == (8, 2, 256, 256) and got["logits"].shape == (8, 7, 256, 256)
    assert all(np.isfinite(a).all() for a in got.values())
    # ids 1..nlabels per tile; one record per cell
    assert np.array_equal(got["masks"].reshape(8, -1).max(1), got["nlabels"]) and got["nlabels"].sum() > 0
    rec = got["records"]
    assert rec.shape == (int(got["nlabels"].sum()), 10)
    assert np.array_equal(np.bincount(rec[:, 0].astype(int), minlength=8), got["nlabels"].astype(int))
