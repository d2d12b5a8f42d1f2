"""bench.py's launcher contract, checked without a GPU: `--gpus N` is never silently ignored."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=300)


def test_gpus_flag_fails_loudly_when_devices_are_missing():
    n = torch.cuda.device_count() + 1 if torch.cuda.is_available() else 2
    r = _run(["--gpus", str(n), "--steps", "1", "--warmup", "0"])
    assert r.returncode != 0
    assert f"--gpus {n} requested but only" in r.stderr
    assert "{" not in r.stdout, "no bench line may be printed for a run that did not get its GPUs"


def test_world_size_must_match_gpus_flag():
    r = _run(["--gpus", "1", "--steps", "1", "--warmup", "0"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0
    assert "WORLD_SIZE=2 but --gpus 1" in r.stderr


def test_help_names_full_and_dump_outputs():
    r = _run(["--help"])
    assert r.returncode == 0
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_writes_every_row_below_the_limit(tmp_path):
    import numpy as np
    bench = _bench_module()
    packed = torch.arange(50 * 5, dtype=torch.float32).reshape(50, 5)
    bench.dump_outputs(str(tmp_path), {"image": packed[:, :3], "depth": packed[:, 3], "weights_sum": packed[:, 4]})
    assert sorted(os.listdir(tmp_path)) == ["depth.npy", "image.npy", "weights_sum.npy"]
    assert np.array_equal(np.load(tmp_path / "image.npy"), packed[:, :3].numpy())
    assert np.array_equal(np.load(tmp_path / "depth.npy"), packed[:, 3].numpy())
    assert np.load(tmp_path / "weights_sum.npy").dtype == np.float32


def test_dump_outputs_samples_the_same_rows_of_every_array_above_the_limit(tmp_path, monkeypatch):
    import numpy as np
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1000)
    img = torch.arange(200 * 3, dtype=torch.float32).reshape(200, 3)
    depth = torch.arange(200, dtype=torch.float32) * 0.5
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), {"image": img, "depth": depth})
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 1000 // (16 + 8) and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))            # fixed, seeded sample
    idx = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "image.npy"), img.numpy()[idx])
    assert np.array_equal(np.load(tmp_path / "a" / "depth.npy"), depth.numpy()[idx])
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 1000 + 3 * 128   # (+ .npy headers)
