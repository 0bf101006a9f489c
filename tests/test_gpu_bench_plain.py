"""GPU (one device): a plain `python bench.py` run times its steps and prints the headline only, and `--dump-outputs DIR`
writes the proof of the last timed step -- the same words from two runs with the same arguments (the inputs are seeded)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain(out_dir, steps):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ZKHIP_BENCH_PLUMBING_ONLY", "ZKHIP_BENCH_DRYRUN_1GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                        "--log-rows", "14", "--width", "40", "--inflight", "2", "--dump-outputs", str(out_dir)],
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_proof(tmp_path):
    a = _plain(tmp_path / "a", 3)
    assert a["steps"] == 3 and a["warmup"] == 1 and a["n_gpus"] == 1
    assert a["unit"] == "proofs/s" and a["higher_is_better"] is True and a["dtype"] == "u32"
    assert a["value"] > 0 and a["ms_per_step"] > 0
    assert abs(a["value"] * a["ms_per_step"] - 1e3) < 0.02 * 1e3   # one step = one proof
    # what only --full measures is absent
    for k in ("roofline", "stage_ms_single_stream", "cpu_baseline", "aggregate", "guest_flow"):
        assert k not in a
    pa = np.load(tmp_path / "a" / "proof.npy")
    assert pa.dtype == np.float64 and pa.size * 4 == a["config"]["proof_bytes"]
    assert (pa == np.floor(pa)).all() and pa.min() >= 0 and pa.max() < 2.0 ** 32
    b = _plain(tmp_path / "b", 3)
    assert np.array_equal(pa, np.load(tmp_path / "b" / "proof.npy"))
