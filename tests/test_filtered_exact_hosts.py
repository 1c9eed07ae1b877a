"""The filtered exact search's host surfaces: include/mhnsw.h declares the two
entry points and hnsw_amd._lib binds them; the C++ header's
Graph<K>::SearchFilteredExact compiles against include/ and hnsw_amd/libmhnsw.so
(tests/cpp/filter_exact_test.cpp) and, on the GPU, runs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mhnsw_search_filtered_exact", "mhnsw_search_filtered_exact_device")


def test_header_declares_and_binding_binds(H):
    src = open(os.path.join(ROOT, "include", "mhnsw.h")).read()
    lib = H.load()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert name in H.SIGNATURES and hasattr(lib, name), name
    res, args = H.SIGNATURES[NAMES[0]]
    assert res is C.c_int and len(args) == 9      # h, queries, B, dim, k, filter_of, keys, dist, n
    res, args = H.SIGNATURES[NAMES[1]]
    assert res is C.c_int and len(args) == 10 and args[5] is C.c_int  # ... k, filter, keys, dist, n, stream


def test_python_hosts_take_a_mode(H):
    for fn in (H.Graph.search_filtered_arrays, H.Graph.SearchFiltered):
        assert inspect.signature(fn).parameters["mode"].default == H.MODE_BEAM
    assert hasattr(H.Graph, "search_filtered_exact_device")
    assert hasattr(H.ExactIndex, "SearchFiltered") and hasattr(H.ExactAdapter, "SearchFiltered")
    from hnsw_amd import facets

    assert facets.MODE_EXACT == H.MODE_EXACT
    assert inspect.signature(facets.FacetedGraph.Search).parameters["mode"].default == facets.MODE_COMPAT


def _build(tmp_path):
    exe = str(tmp_path / "filter_exact_test")
    lib = os.path.join(ROOT, "hnsw_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "filter_exact_test.cpp"),
                           os.path.join(lib, "libmhnsw.so"), "-Wl,-rpath," + lib])
    return exe


def test_cpp_filtered_exact_builds(tmp_path):
    out = subprocess.run(["ldd", _build(tmp_path)], capture_output=True, text=True)
    assert "libmhnsw.so" in out.stdout


@pytest.mark.gpu
def test_cpp_filtered_exact(tmp_path):
    r = subprocess.run([_build(tmp_path)], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "PASS" in r.stdout
