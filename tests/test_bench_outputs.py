"""bench.py's plain run and --dump-outputs: the dump helper on CPU tensors (dtypes, the seeded
sample of a large output), the options a plain run switches off, and on the GPU one small plain
run whose dumped RDM and flags equal the engine's own output for the same seeded echo."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench():
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_outputs_dtypes_and_whole_arrays(tmp_path):
    import torch
    bench = _bench()
    g = torch.Generator().manual_seed(7)
    rdm = torch.rand((2, 5, 7), generator=g)
    flag = (torch.rand((2, 5, 7), generator=g) < 0.3).to(torch.uint8)
    z = torch.view_as_complex(torch.rand((3, 4, 2), generator=g))
    est = torch.rand((6, 3), generator=g, dtype=torch.float64)
    count = torch.tensor([[1 << 30, 0], [3, 1]], dtype=torch.int32)
    bench.dump_outputs(str(tmp_path), {"rdm": rdm, "flag": flag, "z": z, "est": est, "count": count})
    got = {n: np.load(tmp_path / (n + ".npy")) for n in ("rdm", "flag", "z", "est", "count")}
    assert got["rdm"].dtype == np.float32 and np.array_equal(got["rdm"], rdm.numpy())
    assert got["flag"].dtype == np.float32 and np.array_equal(got["flag"], flag.numpy())
    assert got["z"].dtype == np.float32 and got["z"].shape == (3, 4, 2)
    assert np.array_equal(got["z"][..., 0] + 1j * got["z"][..., 1], z.numpy())
    assert got["est"].dtype == np.float64 and np.array_equal(got["est"], est.numpy())
    assert got["count"].dtype == np.float64 and np.array_equal(got["count"], count.numpy())


def test_dump_outputs_samples_a_large_output(tmp_path, monkeypatch):
    import torch
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 4096)            # 2 arrays: 1024 float32 each
    big = torch.arange(50000, dtype=torch.float32).reshape(50, 1000)
    small = torch.arange(100, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (1024,) and np.array_equal(a, b)            # the same sample in every run
    assert np.all(np.diff(a) >= 0) and a.min() >= 0 and a.max() < 50000
    assert len(np.unique(a)) > 900                                # spread over the array, not a prefix
    assert a.max() > 45000 and a.min() < 5000
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small.numpy())
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 2 * 4096 + 2 * 128                            # the budget, plus the .npy headers


def test_plain_run_switches_off_the_secondary_measurements(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "2", "--host-path"])
    a = bench.parse()
    assert (a.full, a.cpu_seconds, a.lane_steps, a.host_path, a.dump_outputs) == (False, 0, 0, False, None)
    assert (a.steps, a.warmup) == (3, 2)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--host-path", "--dump-outputs", "d"])
    a = bench.parse()
    assert (a.full, a.cpu_seconds, a.lane_steps, a.host_path, a.dump_outputs) == (True, 10.0, 2, True, "d")


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    import torch
    from rsp import presets, synth
    from rsp.engine import Engine
    P, R, B = 64, 1024, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--P", str(P),
                        "--R", str(R), "--batch", str(B), "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=150, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0
    assert out["value"] > 0 and out["unit"] == "CPI/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    # a plain run: no CPU baseline, no per-kernel pass, no host path
    assert out["cpu_baseline"] is None and "kernels" not in out["roofline"] and "host_path" not in out
    # the dump is what a caller of the timed path receives for the same seeded echo (seed 1003:
    # config c3, first CPI 0)
    spec = presets.v2(P, R)
    cf = presets.default_cfar(spec)
    eng = Engine(spec, device=0)
    echo = synth.echo_torch(spec, B, seed=1003, device=torch.device("cuda", 0))
    rdm = torch.empty((B, spec.P, spec.R_out), dtype=torch.float32, device="cuda:0")
    flag = torch.empty((B, spec.P, spec.R_out), dtype=torch.uint8, device="cuda:0")
    eng.run_dev(echo, rdm=rdm, flag=flag, cfar=cf)
    torch.cuda.synchronize()
    got_rdm, got_flag = np.load(tmp_path / "rdm.npy"), np.load(tmp_path / "flag.npy")
    assert got_rdm.dtype == np.float32 and got_flag.dtype == np.float32
    assert np.array_equal(got_rdm, rdm.cpu().numpy())
    assert np.array_equal(got_flag, flag.cpu().numpy())
    assert got_flag.any()
    eng.close()
