"""GPU tier: the plain `bench.py` run - timed steps and the result line only - and what `--dump-outputs` writes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_plain_run_and_dump_outputs(dev, tmp_path):
    """A plain run times exactly --steps steps and prints one line without the --full records; --dump-outputs writes the last
    timed step's loss / nll / argmax and the model state it left as float32 .npy files, under 64 MB in all."""
    out_dir = str(tmp_path / "dump")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LASR_FORCE_OVERLAP"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--batch", "8",
                          "--dump-outputs", out_dir], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "audio-seconds/sec" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    for k in ("roofline", "cpu_baseline", "trainer", "comm"):
        assert k not in d, k
    files = sorted(os.listdir(out_dir))
    assert files == ["argmax.npy", "buffers.npy", "grads.npy", "loss.npy", "nll.npy", "params.npy"], files
    total = 0
    arrs = {}
    for f in files:
        a = np.load(os.path.join(out_dir, f))
        assert a.dtype == np.float32, (f, a.dtype)
        assert np.isfinite(a).all(), f
        arrs[f[:-4]] = a
        total += os.path.getsize(os.path.join(out_dir, f))
    assert total <= 64 * 2 ** 20
    assert arrs["loss"].shape == (1,) and abs(float(arrs["loss"][0]) - d["final_loss"]) <= 1e-6 * abs(d["final_loss"])
    assert arrs["nll"].shape == (8,)
    assert arrs["argmax"].shape[0] == 8 and (arrs["argmax"] >= 0).all() and (arrs["argmax"] < d["config"]["n_class"]).all()
    assert arrs["params"].shape == arrs["grads"].shape and arrs["params"].size > 1000000
