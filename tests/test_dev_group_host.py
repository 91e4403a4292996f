"""The reallocation policy of a frame's buffer groups (web-rwkv-gguf_amd/csrc/wrk_dev_group.h), on the CPU.

tests/host/dev_group_main.cpp includes the header alone, stands in for hipMalloc / hipFree / hipStreamSynchronize with malloc and free
(with a settable failure and a live-allocation count) and asserts the policy: what the first ensure does, that a request the group
already serves touches nothing, when the owner's drop callback runs, the dimensions and the layout after growth, the empty state after
a failed allocation, and that release frees everything.  It is built with the host compiler under the address and undefined-behaviour
sanitizers, so a piece that does not lie inside the allocation fails the run.  The sanitizer runtimes are linked into the program:
it is a stand-alone executable and runs the same whatever libraries the environment preloads."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rocm_include():
    for d in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if d and os.path.exists(os.path.join(d, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(d, "include")
    pytest.fail("no ROCm headers (hip/hip_runtime_api.h) under $ROCM_PATH or /opt/rocm")


def test_group_policy(tmp_path):
    cxx = shutil.which("g++")
    assert cxx, "the host compiler g++ is required"
    exe = str(tmp_path / "dev_group")
    cmd = [cxx, "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + _rocm_include(), "-I" + os.path.join(ROOT, "web-rwkv-gguf_amd", "csrc"),
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan", "-Wall", "-Werror", "-g",
           os.path.join(ROOT, "tests", "host", "dev_group_main.cpp"), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, ran.stdout + ran.stderr
    assert "dev_group: ok" in ran.stdout
