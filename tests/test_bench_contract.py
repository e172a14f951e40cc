"""bench.py driver-contract tests: single-rank and multi-rank (gloo, CPU) runs must
produce the one-line JSON with the required fields and sane values."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_FIELDS = ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                   "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                   "dtype", "data", "config")


def _last_json_line(out: str):
    for line in reversed(out.strip().splitlines()):
        line = line.strip()
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(f"no JSON line in output:\n{out[-2000:]}")


@pytest.mark.timeout(240)
def test_bench_single_rank():
    out = subprocess.run(
        [sys.executable, "bench.py", "--steps", "3", "--warmup", "1", "--full"],
        cwd=REPO, capture_output=True, text=True, timeout=220)
    assert out.returncode == 0, out.stderr[-2000:]
    res = _last_json_line(out.stdout)
    for f in REQUIRED_FIELDS:
        assert f in res, f"missing field {f}"
    assert res["metric"] == "podgangs_per_sec"
    assert res["n_gpus"] == 1 and res["steps"] == 3 and res["warmup"] == 1
    assert res["value"] > 0 and res["higher_is_better"] is True
    assert res["scaling"] == "weak" and res["data"] == "synthetic"
    assert res["p50_time_to_running_ms"] > 0
    # headline is the deployable (wire) shape, with the in-process number nested
    assert res["config"]["transport"] == "http"
    assert res["inproc"]["value"] > 0
    assert res["calibration"]["spin_ms"] > 0


@pytest.mark.timeout(300)
@pytest.mark.parametrize("gang_size", [1, 2, 4, 8])
def test_bench_gang_size_matrix(gang_size):
    """Every gang size of the driver's scaling sweep produces a valid record
    (be ready for the 8-GPU sweep on first contact)."""
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", str(gang_size), "--steps", "2",
         "--warmup", "0", "--gangs-per-step", "2", "--transport", "inproc"],
        cwd=REPO, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    res = _last_json_line(out.stdout)
    assert res["n_gpus"] == gang_size
    assert res["config"]["gang_size"] == gang_size
    assert res["value"] > 0 and res["p50_time_to_running_ms"] > 0


@pytest.mark.timeout(300)
def test_bench_two_ranks_gloo():
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29517", "bench.py", "--gpus", "2",
         "--steps", "3", "--warmup", "1", "--full"],
        cwd=REPO, capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    res = _last_json_line(out.stdout)
    assert res["n_gpus"] == 2
    assert res["config"]["gang_size"] == 2
    assert res["value"] > 0


@pytest.mark.timeout(240)
def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times only the headline (wire) plane; --dump-outputs writes the
    last timed step's placements, one row of sorted GPU ids per gang."""
    import numpy as np
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1",
         "--gangs-per-step", "3", "--dump-outputs", str(tmp_path / "out")],
        cwd=REPO, capture_output=True, text=True, timeout=220)
    assert out.returncode == 0, out.stderr[-2000:]
    res = _last_json_line(out.stdout)
    for f in REQUIRED_FIELDS:
        assert f in res, f"missing field {f}"
    assert res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["config"]["transport"] == "http"
    assert "inproc" not in res and "calibration" not in res
    ids = np.load(tmp_path / "out" / "gang_gpu_ids.npy")
    assert ids.dtype == np.float32 and ids.shape == (3, 2)
    # a gang of 2 on the 2-GPU node holds each GPU once
    assert (ids == np.array([0.0, 1.0], dtype=np.float32)).all()


@pytest.mark.gpu
@pytest.mark.timeout(240)
def test_bench_dumps_payload_product(tmp_path):
    """payload_gemm.npy is the payload kernel's product at the payload shape on the
    seeded inputs: within the fp32-accumulation bound K * 2^-24 * |A| @ |B|^T of the
    float64 product of the same bf16-rounded inputs."""
    import numpy as np
    import torch
    import bench
    m, n, k = 256, 384, 512
    out = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "0",
         "--payload", f"{m}x{n}x{k}x1", "--dump-outputs", str(tmp_path)],
        cwd=REPO, capture_output=True, text=True, timeout=220)
    assert out.returncode == 0, out.stderr[-2000:]
    got = np.load(tmp_path / "payload_gemm.npy")
    assert got.dtype == np.float32 and got.shape == (m, n)
    gen = torch.Generator().manual_seed(bench.DUMP_SEED)
    a = torch.randn(m, k, generator=gen).to(torch.bfloat16).double()
    bt = torch.randn(n, k, generator=gen).to(torch.bfloat16).double()
    ref = a @ bt.t()
    bound = k * 2.0 ** -24 * (a.abs() @ bt.abs().t())
    err = (torch.from_numpy(got).double() - ref).abs()
    print(f"max err {err.max().item():.3e}, min slack {(bound - err).min().item():.3e}")
    assert (err <= bound).all()
    ids = np.load(tmp_path / "gang_gpu_ids.npy")
    assert ids.dtype == np.float32 and ids.shape == (4, 1) and (ids == 0).all()
