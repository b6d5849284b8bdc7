"""bench.py's guards for the first real multi-GPU run (round-4 verdict, item 4) - the parts that need no GPU: the host-side deadline and
the failure path leave ONE JSON line carrying "error" on rank 0's stdout and end the process with a fresh non-zero exit; other ranks
say so on stderr only.  (The collective timeout, the pre-check of the gathered matrix and a rank that dies are rehearsed on the GPU box:
tools/rehearse.sh -> profiles/r05_bench_gloo_rehearsal.txt.)  Also the command line: --steps, and (on the GPU) what a plain run
prints and what --dump-outputs writes."""
import json
import os
import subprocess
import sys

import pytest
from conftest import ROOT

CODE = """
import sys, time
sys.path.insert(0, {root!r})
import bench
{body}
"""


def run(body):
    return subprocess.run([sys.executable, "-c", CODE.format(root=ROOT, body=body)], capture_output=True, text=True, timeout=300)


def test_deadline_fires_with_an_error_line_and_a_nonzero_exit():
    out = run("d = bench.Deadline(0.3, 0, 4); d.phase = 'timed steps'; time.sleep(30)")
    assert out.returncode == 3
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["value"] is None and line["n_gpus"] == 4 and "timed steps" in line["error"] and "not finished" in line["error"]
    out = run("d = bench.Deadline(0.3, 2, 4); time.sleep(30)")          # another rank: stderr only, same exit
    assert out.returncode == 3 and out.stdout.strip() == "" and "rank 2 of 4" in out.stderr


def test_deadline_cancelled_in_time_is_silent():
    out = run("d = bench.Deadline(0.5, 0, 1); d.cancel(); time.sleep(1.0); print('done')")
    assert out.returncode == 0 and out.stdout.strip() == "done"


def test_fail_prints_the_error_line_on_rank_zero_only():
    out = run("bench.fail(0, 8, 'pre-check of the gathered interaction matrix failed: x')")
    assert out.returncode == 4
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["n_gpus"] == 8 and line["value"] is None and "pre-check" in line["error"]
    out = run("bench.fail(3, 8, 'boom')")
    assert out.returncode == 4 and out.stdout.strip() == "" and "boom" in out.stderr


def test_collective_timeout_and_deadline_come_from_the_environment():
    env = dict(os.environ, BENCH_COLLECTIVE_TIMEOUT_S="15", BENCH_DEADLINE_S="77")
    out = subprocess.run([sys.executable, "-c", CODE.format(root=ROOT, body="print(bench.COLLECTIVE_TIMEOUT_S, bench.DEADLINE_S)")],
                         capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0 and out.stdout.split() == ["15.0", "77.0"]


def test_steps_below_one_are_refused_before_any_work():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 2 and "--steps must be >= 1" in out.stderr and out.stdout.strip() == ""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(dev, tmp_path):
    """A plain run: the headline fields, none of the --full legs, and the last timed step's outputs under --dump-outputs -
    W, on which the device greedy loop reproduces the reference's visit order on this cloud (G19), and the slab sample."""
    import numpy as np
    import torch
    from dipole_normal_prop_amd import field_utils as fu
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "pairs/s"
    assert line["higher_is_better"] is True and line["dtype"] == "f32" and line["full"] is False
    assert not {"other_configs", "cpu_baseline", "sharded_driver", "trace_matches_reference_G19"} & set(line)
    W = np.load(tmp_path / "interaction_matrix.npy")
    dE = np.load(tmp_path / "patch_fields_sample.npy")
    assert W.dtype == np.float64 and W.shape == (256, 256) and np.isfinite(W).all()
    assert dE.dtype == np.float32 and dE.shape == (256, 8192, 3) and np.isfinite(dE).all()
    assert W.nbytes + dE.nbytes <= 64 << 20
    g19 = np.load(os.path.join(ROOT, "tests", "golden", "G19_headline_sphere_patch_propagation.npz"))
    order, _, _ = fu._greedy_on_device(torch.from_numpy(W).to(dev), torch.full((1,), int(g19["order"][0]), dtype=torch.int64, device=dev))
    assert np.array_equal(order.cpu().numpy(), g19["order"])
