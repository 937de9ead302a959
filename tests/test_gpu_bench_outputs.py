"""`bench.py --dump-outputs DIR` on the GPU: a plain run (no `--full`) of the stream workload at a small
batch times exactly `--steps` steps, leaves the keys of the other legs null, and writes the last timed
step's outputs as float32 / float64 `.npy` files that are identical from run to run and equal the
oracle's chain over the same scans."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE_TOL = 1e-4  # BASELINE.json north_star: <= 1e-4 m / <= 1e-4 rad
B, STEPS = 6, 3
ARGV = ["--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--batch", str(B), "--contexts", "2", "--workers", "1"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Two plain runs with the same arguments, side by side: [(JSON line, dump directory)]."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    dirs = [str(tmp_path_factory.mktemp("dump")) for _ in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "bench.py"), *ARGV, "--dump-outputs", d],
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, cwd=ROOT) for d in dirs]
    out = []
    for p, d in zip(procs, dirs):
        so, se = p.communicate(timeout=120)
        assert p.returncode == 0, se[-3000:]
        lines = [l for l in so.splitlines() if l.strip()]
        assert len(lines) == 1, so
        out.append((json.loads(lines[0]), d))
    return out


def test_plain_line(runs):
    for line, _ in runs:
        assert line["steps"] == STEPS and line["unit"] == "scans/s" and line["higher_is_better"] is True
        assert line["ms_per_step"] > 0
        # value = scans per step / seconds per step (both rounded in the line)
        assert line["value"] == pytest.approx(B * 1e3 / line["ms_per_step"], rel=1e-2)
        for key in ("pose_delta_vs_cpu", "sustained", "single_sequence", "segmented", "roofline", "cpu_baseline"):
            assert line[key] is None, key
        assert line["engine_aborts"] == {"timed": 0}


def test_dumps_are_reproducible_and_match_the_oracle(runs, oracle, synth):
    (_, da), (_, db) = runs
    names = sorted(os.listdir(da))
    assert names == sorted(os.listdir(db))
    for want in ("pose.npy", "para.npy", "stats.npy", "counts.npy", "orb_stats.npy", "orb_T.npy", "laser_cloud.npy", "sharp.npy",
                 "less_sharp.npy", "flat.npy", "less_flat.npy", "sample_scans.npy"):
        assert want in names
    a = {n[:-4]: np.load(os.path.join(da, n)) for n in names}
    total = 0
    for n in names:
        b = np.load(os.path.join(db, n))
        assert a[n[:-4]].dtype in (np.float32, np.float64), n
        assert a[n[:-4]].shape == b.shape and np.array_equal(a[n[:-4]], b), n
        total += b.nbytes
    assert total <= 64 << 20
    scans = synth.make_sequence(B)
    feats = [oracle.scan_registration(s) for s in scans]
    pose, rel, st = oracle.odometry_chain(feats)
    assert list(a["sample_scans"]) == list(range(B))  # up to eight scans: all of them
    for name in ("laser_cloud", "sharp", "less_sharp", "flat", "less_flat"):
        ref = np.concatenate([getattr(f, name) for f in feats])
        assert a[name].shape == ref.shape and np.array_equal(a[name][:, :3], ref[:, :3]), name
        assert np.allclose(a[name][:, 3], ref[:, 3], atol=1e-6), name
    for k in range(1, B):
        assert np.max(np.abs(a["pose"][k] - pose[k])) < POSE_TOL, k
        assert np.max(np.abs(a["para"][k] - rel[k])) < POSE_TOL, k
        assert np.array_equal(a["stats"][k][:4], st[k][:4]), k
