"""bench.py command line on CPU (StubEngine): the result line's contract and
the --dump-outputs / --full options."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent


def _run_bench(*extra: str) -> dict:
    # hide any GPU: this is the host-side contract, seconds with the stub
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    proc = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--steps", "3",
         "--warmup", "1", *extra],
        capture_output=True, text=True, timeout=240, cwd=REPO, env=env)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [l for l in proc.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_and_full(tmp_path):
    """One run with both options: the result line keeps its fields, --steps
    sets the timed step count, and the dump holds the last step's per-agent
    replies as float arrays."""
    out_dir = tmp_path / "dump"
    out = _run_bench("--full", "--dump-outputs", str(out_dir))
    assert out["metric"] == "agent-cycles/sec" and out["unit"] == "cycles/s"
    assert out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 3 and out["warmup"] == 1
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value and ms_per_step describe the same timed window
    agents = out["config"]["agents_per_gpu"]
    assert abs(out["value"] * out["ms_per_step"] / 1000 - agents) < 0.05 * agents

    assert sorted(p.name for p in out_dir.iterdir()) == [
        "token_counts.npy", "tokens.npy"]
    tokens = np.load(out_dir / "tokens.npy")
    counts = np.load(out_dir / "token_counts.npy")
    assert tokens.dtype == np.float32 and counts.dtype == np.float32
    assert tokens.shape[0] == agents and tokens.shape[1] > 0
    assert counts.shape == (agents, 2)
    assert (counts[:, 1] > 0).all()          # every agent replied
    assert (tokens[:, 0] >= 0).all()         # no empty reply row
    assert tokens.min() >= -1 and tokens.max() < 151936
    assert tokens.nbytes + counts.nbytes < 64 * 2**20
