"""CPU: the in-place update's surface -- mhnsw.h declares the three calls, _lib.py binds them
with matching arity, and the Python host exports its methods."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"mhnsw_update": 6, "mhnsw_update_device": 6, "mhnsw_export_edge_dist": 3}


def _header():
    with open(os.path.join(ROOT, "include", "mhnsw.h")) as f:
        return f.read()


def test_header_declares_the_calls():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name, nargs in CALLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    assert "out_found" in text


def test_lib_binds_the_calls():
    from hnsw_amd import _lib

    for name, nargs in CALLS.items():
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.C.c_int and len(args) == nargs, name


def test_host_exports_the_methods():
    import hnsw_amd

    for name in ("Update", "Upsert", "update_arrays", "update_device", "export_edge_dist"):
        assert callable(getattr(hnsw_amd.Graph, name)), name
