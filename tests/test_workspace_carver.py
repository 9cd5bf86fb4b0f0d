"""The workspace carver (csrc/tr_workspace.h) under AddressSanitizer and UBSan: tests/cpp/carver_check.cpp is
a stand-alone host program (no HIP) that declares layouts, binds them into heap blocks of exactly
bytes() and writes both ends of every piece.  Built with the host compiler and run as a child
process; nothing is preloaded."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tensor_regression_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "carver_check.cpp")


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_carver_layouts_under_sanitizers(tmp_path):
    cxx = _host_compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (g++ / clang++) on this machine")
    exe = str(tmp_path / "carver_check")
    # the sanitizer runtimes are linked into the program itself (clang's default; asked of g++)
    static = [] if "clang" in os.path.basename(cxx) else ["-static-libasan", "-static-libubsan"]
    cc = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", *static, "-I", CSRC, SRC, "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.strip() == "carver ok" and run.stderr == ""
