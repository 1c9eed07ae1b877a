"""The C++ host shim's exact search past k 256 (option "exact_wide"): tests/cpp/wide_test.cpp,
compiled here against include/ and hnsw_amd/libmhnsw.so and run on the GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(tmp_path):
    exe = str(tmp_path / "wide_test")
    lib = os.path.join(ROOT, "hnsw_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "wide_test.cpp"), os.path.join(lib, "libmhnsw.so"),
                           "-Wl,-rpath," + lib])
    return exe


def test_cpp_wide_builds(tmp_path):
    out = subprocess.run(["ldd", _build(tmp_path)], capture_output=True, text=True)
    assert "libmhnsw.so" in out.stdout


@pytest.mark.gpu
def test_cpp_wide(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
