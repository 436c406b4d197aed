"""hybvio_amd/csrc/lds_layout.hpp, the one description of the EKF kernels' dynamic-LDS carves that launchers and kernels share:
tests/cpp/test_lds_layout.cpp is built with the host compiler alone (the header includes no HIP header) and checks every layout over
the state sizes, row counts and track lengths the kernels serve, plus byte counts worked out by hand. No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lds_layouts():
    src = os.path.join(ROOT, "tests", "cpp", "test_lds_layout.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_lds_layout")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all lds layout tests passed" in r.stdout
