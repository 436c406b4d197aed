"""hybvio_amd/csrc/hv_stage.hpp, the staging of every host-pointer entry in the context's arena: tests/cpp/test_stage.cpp is built with
the host compiler alone (the header includes no HIP header) against the counting allocator and runtime operations that log their
calls, and run plain and under the address / undefined-behaviour sanitizers. Source checks keep the header free of HIP and the
staging copies' byte counts in it. No GPU."""
import glob
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybvio_amd", "csrc")


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_stage(sanitize):
    src = os.path.join(ROOT, "tests", "cpp", "test_stage.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_stage")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *sanitize, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "live blocks at exit: 0" in r.stdout
    assert "all stage tests passed" in r.stdout


def test_stage_header_includes_no_hip_header():
    with open(os.path.join(CSRC, "hv_stage.hpp"), encoding="utf-8") as f:
        text = f.read()
    assert "hip_runtime" not in text and not re.search(r"#include\s*[<\"]hip/", text)


def test_ekf_owns_no_staging():
    """Ekf::Fixed holds no staging member, and nobody aliases the hybrid visit's apply mask."""
    with open(os.path.join(CSRC, "ekf_host.hpp"), encoding="utf-8") as f:
        text = f.read()
    fixed = text[text.index("struct Fixed {"):text.index("} fixed;")]
    assert not re.search(r"\b(sH|sv|sr|schi2|simu|sstatus|sdrop|sactive|sH_cap)\b", fixed)
    users = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, encoding="utf-8") as f:
            users += [os.path.basename(path)] * len(re.findall(r"visit\.apply\b", f.read()))
    assert users == ["ekf_visit.hip"] * 2, users         # ekf_hybrid_insert_kernel's output, the update's flags
