"""hybvio_amd/csrc/hv_mt19937.hpp, the arithmetic and the three-phase twist schedule the device generators run (rng.hip):
tests/cpp/test_mt19937_schedule.cpp is built with the host compiler alone (the header includes no HIP header), runs the schedule with
64 simulated lanes that do all reads of a phase before its writes, and compares against <random>'s std::mt19937 over several twists,
seeds and positions, plus the standard's known answer. No GPU."""
import os
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mt19937_schedule():
    src = os.path.join(ROOT, "tests", "cpp", "test_mt19937_schedule.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_mt19937_schedule")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all mt19937 schedule tests passed" in r.stdout
