"""csrc/host_api.h is the one interface header shared by the host binding (g++) and the kernel
translation units (hipcc): it must stay readable by the host compiler alone — plain C++17, no
device code, no builtins — and be safe to include more than once."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "perceiver_io_amd", "csrc")
ROCM_INC = "/opt/rocm/include"

pytestmark = pytest.mark.skipif(shutil.which("g++") is None or not os.path.isdir(ROCM_INC),
                                reason="needs g++ and the ROCm headers")


@pytest.mark.parametrize("times", [1, 2])
def test_host_api_header_parses_with_the_host_compiler(tmp_path, times):
    src = tmp_path / "include_host_api.cpp"
    src.write_text('#include "host_api.h"\n' * times)
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__=1", "-isystem", ROCM_INC,
                        "-I", CSRC, str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
