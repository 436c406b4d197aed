"""The dynamic-LDS layout of the upright 2-point kernel (hybvio_amd/csrc/ransac_lds.hpp: upright2p_lds):
tests/cpp/test_upright2p_lds.cpp is built with the host compiler alone and checks the sections, the closed-form total and that the
largest shape fits a compute unit. No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_upright2p_lds_layout():
    src = os.path.join(ROOT, "tests", "cpp", "test_upright2p_lds.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_upright2p_lds")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all upright2p lds layout tests passed" in r.stdout
