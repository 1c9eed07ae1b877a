"""CPU: the wide exact search's surface -- mhnsw.h states the k limits and names the options,
api.cpp knows every option the header names, and the Python host passes the option on."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTIONS = ("exact_wide", "exact_wide_min_k", "wide_force_fallback", "wide_fallback_bytes")
READ_ONLY = ("last_wide_queries", "last_wide_fallback_queries", "last_wide_hits", "last_wide_rank", "last_wide_room",
             "last_wide_sample_ns", "last_wide_radius_ns", "last_wide_range_ns", "last_wide_emit_ns",
             "last_wide_fallback_ns")


def _read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_header_states_the_limits_and_options():
    text = re.sub(r"\s*\n \*\s*", " ", _read("include", "mhnsw.h"))
    assert "exact mode supports k <= 256" in text
    assert "exact mode supports k <= 4096" in text
    for name in OPTIONS + READ_ONLY:
        assert name in text, name


def test_engine_knows_the_options():
    api = _read("hnsw_amd", "csrc", "api.cpp")
    for name in OPTIONS:
        assert api.count('n == "%s"' % name) == 2, name  # set and get
    for name in READ_ONLY:
        stem = name[len("last_wide_"):-len("_ns")] if name.endswith("_ns") else None
        assert ('"%s"' % name in api) or ('"%s"' % stem in api), name
    host = _read("hnsw_amd", "csrc", "search_host.cpp")
    assert '"exact mode supports k <= 4096"' in host and '"exact mode supports k <= 256"' in host
    assert "wide.hip" in _read("hnsw_amd", "csrc", "Makefile")


def test_host_passes_the_option():
    import hnsw_amd

    assert "wide" in inspect.signature(hnsw_amd.ExactIndex.__init__).parameters
    assert inspect.signature(hnsw_amd.ExactIndex.__init__).parameters["wide"].default is False
    assert "options" in inspect.signature(hnsw_amd.Graph.__init__).parameters  # Graph(..., exact_wide=1)
