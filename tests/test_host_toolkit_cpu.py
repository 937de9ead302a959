"""csrc/lislam_host.hpp on the host alone: tests/cpp/host_toolkit.cpp (its own main, no HIP call) built
with the address and undefined-behaviour sanitizers on the host side and run as a child process; it
compares every status and error text of the shared formatter and feed checks with literals."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "intensity_based_lidar_slam_for_me-_amd", "csrc")


def test_host_toolkit_under_sanitizers():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "tests", "cpp", "host_toolkit.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "host_toolkit")
        subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-value",
                        "-Werror=format", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                        "-fno-sanitize-recover=undefined", "-I", CSRC, src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.strip() == "host toolkit ok"
