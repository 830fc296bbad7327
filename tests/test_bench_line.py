"""GPU box: bench.py's plain single-GPU line (headline only: no extras, no CPU baseline) and --dump-outputs, the output set
of the last timed step checked against the CPU oracle on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_line_and_dump_outputs(tmp_path):
    B, N, M, steps = 1024, 20, 5, 3
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
           "--batch", str(B), "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["unit"] == "solves/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["value"] > 0 and abs(d["value"] - B * steps / (d["ms_per_step"] * steps * 1e-3)) < 1e-6 * d["value"]
    for k in ("cpu_baseline", "c5", "schedule_hint", "pipelined_budget", "stream_of_batches", "extras_status"):
        assert k not in d, k                                  # extras run only under --full

    shapes = {"X": (B, N + 1, 9), "U": (B, N, 5), "s": (B, N + 1), "status": (B,), "iters": (B,), "cost": (B,), "err": (B,)}
    r = {k: np.load(os.path.join(tmp_path, k + ".npy")) for k in shapes}
    assert sorted(os.listdir(tmp_path)) == sorted(k + ".npy" for k in shapes)
    for k, shp in shapes.items():
        assert r[k].shape == shp and r[k].dtype == np.float64, (k, r[k].shape, r[k].dtype)
    assert (r["status"] == 0).all() and d["solver"]["max_iters"] == int(r["iters"].max())

    # the same seeded batch (bench.py's default seed) through the CPU oracle: tolerance as in test_gpu_certificates
    from oracle import synth, coracle, nlp
    n = 32
    s = synth.make_batch(B, N=N, M=M, config_id=3)
    par = nlp.WholeBodyParams(N=N)
    xi = np.clip(s["x_init"][:n], par.xlim[0], par.xlim[1])
    o = coracle.solve_batch(par, xi, s["traj_ref"][:n], s["u_ref"][:n], np.zeros((n, N, 5)), s["obs"][:n])
    assert (o["status"] == 0).all()
    assert np.abs(r["X"][:n] - o["X"]).max() < 2e-5 and np.abs(r["U"][:n] - o["U"]).max() < 2e-5
    assert np.abs(r["cost"][:n] / o["cost"] - 1).max() < 1e-9
