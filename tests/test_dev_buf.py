"""hybvio_amd/csrc/dev_buf.hpp, the owning type of every device buffer of the library: tests/cpp/test_dev_buf.cpp is built with the
host compiler alone (the header includes no HIP header) against a counting allocator that can fail the k-th allocation, and run plain
and under the address / undefined-behaviour sanitizers. A source check keeps the raw allocator calls in the one file that defines
dev_alloc / dev_free. No GPU."""
import glob
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hybvio_amd", "csrc")


@pytest.mark.parametrize("sanitize", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]], ids=["plain", "asan_ubsan"])
def test_dev_buf(sanitize):
    src = os.path.join(ROOT, "tests", "cpp", "test_dev_buf.cpp")
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "test_dev_buf")
        subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *sanitize, "-o", exe, src])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "live blocks at exit: 0" in r.stdout
    assert "all dev_buf tests passed" in r.stdout


def test_raw_device_allocation_stays_in_one_file():
    users = set()
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, encoding="utf-8") as f:
            if re.search(r"\bhipMalloc\s*\(|\bhipFree\s*\(", f.read()):
                users.add(os.path.basename(path))
    assert users == {"capi.hip"}, users
    with open(os.path.join(CSRC, "capi.hip"), encoding="utf-8") as f:
        text = f.read()
    assert len(re.findall(r"\bhipMalloc\s*\(", text)) == 1 and len(re.findall(r"\bhipFree\s*\(", text)) == 1
    assert re.search(r"int dev_alloc\(void \*\*p, size_t bytes\)\s*{[^}]*hipMalloc\(", text)
    assert re.search(r"void dev_free\(void \*p\)\s*{[^}]*hipFree\(", text)
    with open(os.path.join(CSRC, "dev_buf.hpp"), encoding="utf-8") as f:
        assert "hip_runtime" not in f.read()
