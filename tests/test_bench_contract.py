"""bench.py: the SURVEY 8(d) byte formula on CPU, and the one-JSON-line contract of the plain and the --full run on the GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_algorithmic_bytes_formula():
    sys.path.insert(0, ROOT)
    import bench
    # smallCapture S = 92 -> B = 225 + 4928 e; tiny S = 76 -> 193 + 4480 e; 20x20 S = 128 -> 297 + 12800 e
    assert bench.algorithmic_bytes(11, 14, 4) == 225 + 4928 * 4 == 19937
    assert bench.algorithmic_bytes(11, 14, 1) == 225 + 4928
    assert bench.algorithmic_bytes(7, 20, 2) == 193 + 4480 * 2
    assert bench.algorithmic_bytes(20, 20, 4) == 297 + 12800 * 4
    assert bench.WORKLOADS["small16384"] == ("smallCapture", 16384)          # BASELINE configs[2], the default workload
    r = bench.reference_ratio("smallCapture")
    assert r is None or r > 10                                                # port / reference speed ratio, if the file is present


@pytest.mark.parametrize("flag", ["--float32-e2e", "--fixed-sweep"])
def test_options_of_full_only_passes_are_refused_without_full(flag):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), flag], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 2 and "--full" in out.stderr and not out.stdout.strip()


FULL_ONLY = ("roofline", "roofline_emit_team", "cpu_baseline", "ppo", "ppo_config5")


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_nothing_of_full():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "30", "--warmup", "5", "--workload", "tiny4096"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == "env-steps/s (4-agent tinyCapture)" and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "u32" and d["steps"] == 30 and d["warmup"] == 5 and d["n_gpus"] == 1
    assert abs(d["value"] - 4096 / (d["ms_per_step"] / 1e3)) <= 1e-6 * d["value"]
    assert not [k for k in FULL_ONLY if k in d]


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_keys():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "30", "--warmup", "5", "--workload", "tiny4096",
                          "--full", "--no-ppo", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in d, k
    assert d["steps"] == 30 and d["warmup"] == 5 and d["n_gpus"] == 1 and d["unit"] == "env-steps/s" and d["vs_baseline"] is None
    assert abs(d["value"] - 4096 / (d["ms_per_step"] / 1e3)) <= 1e-6 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9
    assert r["algorithmic_bytes_per_launch"] == 4096 * 4 * 8 * 7 * 20 * 4
    # the headline figure is the all-bytes-to-HBM one (sweep direction fixed); the cache-assisted figure of the default path in
    # this loop is reported beside it and can only be faster
    assert "expand_alt 0" in r["measured_with"] and r["cache_assisted"]["GBps"] > 0 and "workload" in d["config"]
    assert d["tick_all_bytes_to_hbm"]["us_per_tick"] > 0
    assert d["roofline_emit_team"]["bound"] == "hbm" and "cpu_baseline" not in d and "ppo" not in d      # the --no-* options hold


def _fake_step(n, h, w, obs_dtype):
    import torch
    g = torch.Generator().manual_seed(0)
    obs = torch.randint(0, 2, (n, 4, 8, h, w), generator=g).to(obs_dtype)
    info = {"legal_actions": torch.randint(0, 32, (n, 4), generator=g, dtype=torch.uint8),
            "score_change": torch.randint(-5, 5, (n,), generator=g, dtype=torch.int32),
            "score": torch.randint(-20, 20, (n,), generator=g, dtype=torch.int32),
            "agent": torch.randint(0, 1 << 30, (n, 4), generator=g, dtype=torch.int32)}
    return obs, torch.randn(n, 2, generator=g, dtype=torch.float64), torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8), info


@pytest.mark.parametrize("n,h,w,dtype", [(16384, 11, 14, "float32"), (8192, 20, 20, "bfloat16"), (300, 7, 20, "uint8")])
def test_dump_outputs_writes_float_arrays_of_one_fixed_env_sample_under_64_mb(tmp_path, n, h, w, dtype):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    step = _fake_step(n, h, w, getattr(torch, dtype))
    r = bench.dump_outputs(str(tmp_path / "a"), step, n)
    bench.dump_outputs(str(tmp_path / "b"), step, n)
    names = {"env_index", "obs", "reward", "done", "legal_actions", "score_change", "score", "agent"}
    assert {p.name for p in (tmp_path / "a").iterdir()} == {x + ".npy" for x in names}
    assert sum(p.stat().st_size for p in (tmp_path / "a").iterdir()) <= 64e6
    idx = np.load(tmp_path / "a" / "env_index.npy")
    assert idx.dtype == np.float64 and len(idx) == r["envs"] and (r["envs"] < n) == (n > 300)     # 300 envs fit whole, the others not
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n
    sel = torch.from_numpy(idx.astype(np.int64))
    full = {"obs": step[0], "reward": step[1], "done": step[2], **step[3]}
    for name in names:
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype in (np.float32, np.float64) and a.tobytes() == b.tobytes(), name     # the same sample every time
        if name != "env_index":
            assert a.shape == (len(idx),) + tuple(full[name].shape[1:]) and (a == full[name][sel].double().numpy()).all(), name


@pytest.mark.gpu
def test_bench_dump_outputs_are_the_same_from_run_to_run(tmp_path):
    import numpy as np
    lines = []
    for run in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "7", "--warmup", "3", "--workload", "tiny4096",
                              "--no-ppo", "--no-cpu-baseline", "--no-emit", "--no-unidirectional", "--dump-outputs", str(tmp_path / run)],
                             capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        lines.append(json.loads([l for l in out.stdout.splitlines() if l.strip().startswith("{")][0]))
    for d in lines:
        assert d["steps"] == 7 and d["ms_per_step"] > 0 and d["dump_outputs"]["of_envs"] == 4096
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert "obs.npy" in files and "reward.npy" in files and files == sorted(p.name for p in (tmp_path / "b").iterdir())
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape and a.tobytes() == b.tobytes(), f
    obs = np.load(tmp_path / "a" / "obs.npy")
    assert obs.shape[1:] == (4, 8, 7, 20) and obs.any()
