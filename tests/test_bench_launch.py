"""bench.py's launcher contract (CPU, no GPU touched): `--gpus N` without a launcher starts N ranks
itself; under a launcher whose WORLD_SIZE differs from N it exits non-zero before any work.  And its output
contract: the `--dump-outputs` writer (CPU), and a plain run's result line and dumps on the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True,
                          env=env, timeout=timeout, cwd=ROOT)


def test_bench_gpus2_spawns_two_ranks():
    r = _run(["--gpus", "2", "--launch-check"])
    assert r.returncode == 0, r.stderr[-2000:]
    line = [x for x in r.stdout.splitlines() if x.startswith("{")][-1]
    d = json.loads(line)
    assert d["world"] == 2 and d["ranks_seen"] == 2 and d["local_world"] == 2


def test_bench_mismatched_launcher_exits_nonzero():
    r = _run(["--gpus", "4", "--launch-check"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"}, timeout=60)
    assert r.returncode != 0
    assert "WORLD_SIZE=2" in r.stderr


def test_dump_outputs_float32_and_fixed_sample(tmp_path):
    """--dump-outputs' writer: float32 files (float64 kept), an array above the cap written as the same
    seeded sample on every call, a small one whole."""
    import torch

    import bench
    n = bench.DUMP_MAX_ELEMS + 12345
    big = torch.arange(n, dtype=torch.float32).to(torch.bfloat16)
    arrays = {"big": big, "small": torch.tensor([[1.5, -2.0]], dtype=torch.bfloat16),
              "wide": torch.tensor([1.0 / 3.0], dtype=torch.float64)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in arrays}
    assert a["big"].dtype == np.float32 and a["big"].shape == (bench.DUMP_MAX_ELEMS,)
    assert np.all(np.diff(a["big"]) >= 0) and np.isin(a["big"][::4099], big.float().numpy()).all()
    assert a["small"].dtype == np.float32 and a["small"].tolist() == [1.5, -2.0]
    assert a["wide"].dtype == np.float64 and a["wide"][0] == 1.0 / 3.0
    for k in arrays:
        assert np.array_equal(a[k], np.load(tmp_path / "b" / f"{k}.npy")), k
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64e6


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_repeat(gpu, tmp_path):
    """A plain run prints the headline keys and nothing that needs runs of its own; --steps sets the timed
    steps; two runs with the same arguments dump the same arrays (identical inputs, same kernels)."""
    outs = []
    for tag in ("a", "b"):
        r = _run(["--gpus", "1", "--config", "tiny", "--steps", "2", "--warmup", "1",
                  "--dump-outputs", str(tmp_path / tag)], timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1]))
    d = outs[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in d, k
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["unit"] == "images/sec" and d["higher_is_better"] is True
    assert not [k for k in d if k.startswith("cpu_baseline")]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad_norm.npy", "loss.npy", "projector_grad.npy", "projector_param.npy"]
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
        assert np.array_equal(a, b), f
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == pytest.approx(d["loss"], abs=1e-4)
