"""bench.py's plain / --full split and --dump-outputs: a plain run reports the headline only, --full
adds the comparator and toy-MLP side figures without changing what the headline computes, and
--dump-outputs writes the last timed step's parameters and losses, identical from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_KEYS = ("ref_samples_per_s", "speedup_vs_torch", "mlp_us_per_step", "mlp_bf16_us_per_step")
HEAD_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(args, timeout=240):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", *args], cwd=REPO, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [json.loads(l[l.index('{"metric"'):]) for l in p.stdout.splitlines() if '{"metric"' in l]
    assert len(lines) == 1
    return lines[0]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _check_dump(rec, out, steps):
    assert all(rec[k] is not None for k in HEAD_KEYS)
    assert rec["steps"] == steps and rec["value"] > 0
    # ms_per_step is the timed window over the K timed steps (both figures are rounded in the line)
    assert rec["ms_per_step"] == pytest.approx(1e-3 * rec["timing"]["headline"]["window_us"] / steps, abs=1e-5)
    assert set(out) == {"params", "losses"} == set(rec["dumped_outputs"])
    for name, a in out.items():
        assert a.dtype == np.float32 and a.size > 0 and np.isfinite(a).all(), name
        assert list(a.shape) == rec["dumped_outputs"][name]


def test_bench_cpu_plain_run_is_lean_and_dumps(tmp_path):
    """CPU/gloo stock loop, one rank: no side measurement without --full; the dump holds the 21
    parameters of Linear(20, 1) and the last step's loss, and a second run writes the same bytes."""
    args = ["--device", "cpu", "--engine", "reference", "--steps", "12", "--warmup", "3"]
    recs = [_bench(args + ["--dump-outputs", str(tmp_path / n)]) for n in ("a", "b")]
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    _check_dump(recs[0], a, 12)
    assert a["params"].shape == (21,) and a["losses"].shape == (1,)
    assert not any(k in recs[0] for k in SIDE_KEYS) and recs[0]["vs_baseline"] is None
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k


def test_dump_outputs_samples_large_arrays(tmp_path):
    """An array over its share of the 64 MB limit is cut to a fixed sample; small ones are kept whole."""
    import torch

    import bench

    big = torch.arange(1 << 16, dtype=torch.float32)
    old = bench.DUMP_LIMIT_BYTES
    bench.DUMP_LIMIT_BYTES = 2 * 4096  # two arrays: 4096 bytes (1024 floats) each
    try:
        s1 = bench._dump_outputs(str(tmp_path / "a"), {"big": big, "small": torch.ones(3, dtype=torch.float64)})
        s2 = bench._dump_outputs(str(tmp_path / "b"), {"big": big, "small": torch.ones(3, dtype=torch.float64)})
    finally:
        bench.DUMP_LIMIT_BYTES = old
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert s1 == s2 == {"big": [1024], "small": [3]}
    assert a["big"].dtype == np.float32 and a["small"].dtype == np.float64
    assert (a["big"] == b["big"]).all() and (np.diff(a["big"]) > 0).all()  # same, ordered sample of the input
    assert sum(v.nbytes for v in a.values()) <= 2 * 4096


@pytest.fixture(scope="module")
def gpu_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_out")
    args = ["--steps", "20", "--warmup", "5"]
    plain = _bench(args + ["--dump-outputs", str(d / "plain")])
    full = _bench(args + ["--full", "--dump-outputs", str(d / "full")])
    return plain, full, _load(d / "plain"), _load(d / "full")


@pytest.mark.gpu
def test_bench_gpu_plain_vs_full(gpu_runs):
    """The driver command on the persistent engine: the plain line has no side measurement, the
    --full line has all of them, and both name the same engine for the headline."""
    plain, full, _, _ = gpu_runs
    assert not any(k in plain for k in SIDE_KEYS) and plain["vs_baseline"] is None
    assert all(full.get(k) for k in SIDE_KEYS) and full["vs_baseline"] == full["speedup_vs_torch"]
    assert plain["engine_path"] == full["engine_path"] == "persistent" and "fallback" not in plain
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k]


@pytest.mark.gpu
def test_bench_gpu_dump_outputs_repeat(gpu_runs):
    """Same arguments, same inputs: two processes leave bit-identical parameters and losses (the side
    measurements of --full run after the dump's copies are taken), 20 losses for the 20 timed steps."""
    plain, full, a, b = gpu_runs
    _check_dump(plain, a, 20)
    _check_dump(full, b, 20)
    assert a["params"].shape == (21,) and a["losses"].shape == (20,)
    assert a["losses"][-1] == np.float32(plain["final_loss"])
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
