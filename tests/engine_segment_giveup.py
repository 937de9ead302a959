"""Child process of test_gpu_engine_segments.test_give_up_under_the_dispatcher, started with
LISLAM_ENGINE_WAIT_US=1 (every bounded device wait of the engine expires at once): two batches
pending on the dispatcher at shape (3, 5) with segments on.  Each launch gives up in its first
segment, the chain ends there and is re-run on the per-round schedule when it settles: status 1 and
the per-round schedule's outputs, array for array."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    assert os.environ.get("LISLAM_ENGINE_WAIT_US") == "1"
    pkg = importlib.import_module("intensity_based_lidar_slam_for_me-_amd")
    if os.environ.get("LISLAM_ALT_LIB"):  # developer A/B: a variant build of the library
        pkg.native.load(os.environ["LISLAM_ALT_LIB"])
    nat = pkg.native
    S = 6
    ctxs = [pkg.Context(n_scans=64, width=1024) for _ in range(2)]
    bats = []
    try:
        for c in ctxs:
            c.set_engine_shape(3, 5)
            c.set_engine_segment(2)
        bats = [pkg.Batch(c, S) for c in ctxs]
        refs = []
        for c, b, start in zip(ctxs, bats, (70, 400)):
            b.upload(pkg.synth.make_sequence(S, start=start))
            b.extract(S)
            c.set_odometry_schedule(c.ENGINE_OFF)  # the per-round schedule: no device waits
            b.odometry(S, S - 1)
            refs.append([[b.download(w, k) for k in range(S)] for w in (nat.OUT_PARA, nat.OUT_POSE, nat.OUT_STATS)])
            c.set_odometry_schedule(c.ENGINE_ON)
        for b in bats:  # both pending before either is read
            b.odometry(S, S - 1)
        for b, ref in zip(bats, refs):
            got = [[b.download(w, k) for k in range(S)] for w in (nat.OUT_PARA, nat.OUT_POSE, nat.OUT_STATS)]
            status = b.odometry_status()
            assert b.odometry_engine() == 2 and status == 1, (b.odometry_engine(), status)
            assert b.odometry_status() == 0  # read and cleared
            for g, r in zip(got, ref):
                for k in range(S):
                    assert np.array_equal(g[k], r[k]), (k, g[k], r[k])
    finally:
        for b in bats:
            b.close()
        for c in ctxs:
            c.close()
    print("give-up recovered")


if __name__ == "__main__":
    main()
