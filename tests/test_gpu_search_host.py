"""GPU: the search host path (hnsw_amd/csrc/search_host.cpp) -- what the plain,
filtered and negatives entry points share on one handle and what no other test
pins: the staged scratch buffers across the entry families, which of two
argument faults each entry point reports, the timing flags every search leaves,
and the sticky error word of the *_device calls.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, D, SEED = 600, 16, 5  # (N >= engine.hpp H1_BN = 256: the exact mode runs its fused path)


def _data():
    rng = np.random.default_rng(33)
    X = rng.normal(size=(N, D)).astype(np.float32)
    Q = rng.normal(size=(70, D)).astype(np.float32)
    NEG = rng.normal(size=(6, D)).astype(np.float32)
    allowed = np.flatnonzero(rng.random(N) < 0.5) * 3 + 1
    return X, Q, NEG, allowed


def _graph(H, X, allowed, build_mode=None, **kw):
    """the batched-build cosine graph of X (keys 3 i + 1) and its one filter"""
    bm = H.BUILD_BATCH if build_mode is None else build_mode
    g = H.Graph(M=8, Ml=0.25, EfSearch=kw.pop("EfSearch", 32), Distance=H.CosineDistance, Rng=SEED, build_mode=bm, **kw)
    if len(X):
        g.add_arrays(np.arange(len(X), dtype=np.int64) * 3 + 1, X)
    return g, (g.Filter(allowed.tolist()) if bm != H.BUILD_FLAT else None)


def _same(got, want, what):
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what


def test_scratch_reuse_across_entry_families(H):
    X, Q, NEG, allowed = _data()
    negs = [NEG[0:2], [], NEG[2:3], [], NEG[3:6]]
    calls = [
        ("beam 70", lambda g, f: g.search_arrays(Q, 10, mode=H.MODE_BEAM)),
        ("filtered 3", lambda g, f: g.search_filtered_arrays(Q[:3], 5, f)),
        ("negatives 5", lambda g, f: g.search_negatives_arrays(Q[10:15], negs, 4, 0.5, mode=H.MODE_BEAM)),
        ("compat 1", lambda g, f: g.search_arrays(Q[7], 1, mode=H.MODE_COMPAT)),
        ("exact 33", lambda g, f: g.search_arrays(Q[:33], 7, mode=H.MODE_EXACT)),
        ("filtered 70", lambda g, f: g.search_filtered_arrays(Q, 10, f)),
    ]
    g, f = _graph(H, X, allowed)
    try:
        got = [call(g, f) for _, call in calls]
    finally:
        g.close()
    for (what, call), res in zip(calls, got):
        g, f = _graph(H, X, allowed)
        try:
            want = call(g, f)
        finally:
            g.close()
        assert (want[2] == want[0].shape[1]).all(), what  # (every list full: nothing compared is padding)
        _same(res, want, what)


class _Raw:
    """the four search entry points called directly, with any B / dim / k / mode /
    ef / route / filter_of -> the HnswError's message, or None for MHNSW_OK"""

    def __init__(self, H, g, torch):
        self.H, self.g, self.t = H, g, torch
        self.n = None

    def _out(self, B, k, device):
        B, k = max(B, 1), max(k, 1)
        if device:
            t = self.t
            return (t.zeros(B, k, dtype=t.int64, device="cuda"), t.zeros(B, k, dtype=t.float32, device="cuda"),
                    t.full((B,), 99, dtype=t.int32, device="cuda"))
        return np.zeros((B, k), np.int64), np.zeros((B, k), np.float32), np.full(B, 99, np.int32)

    def _run(self, fn, on, device):
        try:
            self.g._check(fn())
        except self.H.HnswError as e:
            return str(e)
        if device:
            self.t.cuda.synchronize()
            self.g.device_status()
            on = on.cpu().numpy()
        self.n = on
        return None

    def plain(self, device, B, dim, k, mode, ef=0, entry_key=None):
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        lib, h = self.H.load(), self.g._h
        ok, od, on = self._out(B, k, device)
        if device:
            q = self.t.ones(max(B, 1), dim, dtype=self.t.float32, device="cuda")
            return self._run(lambda: lib.mhnsw_search_device(h, q.data_ptr(), B, dim, k, mode, ef, ok.data_ptr(),
                                                             od.data_ptr(), on.data_ptr(), None), on, True)
        q = np.ones((max(B, 1), dim), np.float32)
        ek = None if entry_key is None else C.byref(C.c_int64(entry_key))
        return self._run(lambda: lib.mhnsw_search(h, P(q, C.c_float), B, dim, k, mode, ef, ek, P(ok, C.c_int64),
                                                  P(od, C.c_float), P(on, C.c_int32)), on, False)

    def filtered(self, device, B, dim, k, ef=0, route=0, fid=-1, null_filter=False):
        P = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        lib, h = self.H.load(), self.g._h
        ok, od, on = self._out(B, k, device)
        if device:
            q = self.t.ones(max(B, 1), dim, dtype=self.t.float32, device="cuda")
            fo = self.t.full((max(B, 1),), fid, dtype=self.t.int32, device="cuda")
            return self._run(lambda: lib.mhnsw_search_filtered_device(
                h, q.data_ptr(), B, dim, k, ef, route, None if null_filter else fo.data_ptr(), ok.data_ptr(),
                od.data_ptr(), on.data_ptr(), None), on, True)
        q = np.ones((max(B, 1), dim), np.float32)
        fo = np.full(max(B, 1), fid, np.int32)
        return self._run(lambda: lib.mhnsw_search_filtered(
            h, P(q, C.c_float), B, dim, k, ef, route, None if null_filter else P(fo, C.c_int32), P(ok, C.c_int64),
            P(od, C.c_float), P(on, C.c_int32)), on, False)


K0 = "k must be greater than 0, got 0"
DIM1 = f"embedding dimension mismatch: {D} != 5"
DIMB = f"embedding dimension mismatch for query 0: {D} != 5"
FLAT = "flat index (build_mode 2) supports exact search only"
EF128 = "filtered search supports max(ef,k) <= 128"
ROUTE = "filtered search supports route <= 2048"
NOFILTER = "filter_of must be non-NULL"
EFSEARCH = "EfSearch must be greater than 0, got 0"


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_error_precedence(H, device):
    """calls that carry two faults: each entry point reports the one its checks
    reach first.  Plain: validate, k, dimension, mode, flat index, B <= 0, empty
    index, entry key.  Filtered: validate, k, dimension, flat index, (ef default)
    max(ef, k) > 128, route, B <= 0, NULL filter_of, the filter ids (host
    pointers only), empty index."""
    import torch

    X, _, _, allowed = _data()
    g, f = _graph(H, X, allowed)
    flat, _ = _graph(H, X[:40], allowed, build_mode=H.BUILD_FLAT)
    empty, _ = _graph(H, X[:0], allowed[:0])
    eflat, _ = _graph(H, X[:0], allowed[:0], build_mode=H.BUILD_FLAT)
    try:
        r, rf, re, ref = (_Raw(H, x, torch) for x in (g, flat, empty, eflat))
        BEAM, EXACT = H.MODE_BEAM, H.MODE_EXACT
        # ---- plain
        assert r.plain(device, 4, 5, 0, 9) == K0
        assert r.plain(device, 1, 5, 3, 9) == DIM1
        assert r.plain(device, 4, 5, 3, 9) == DIMB
        assert r.plain(device, 0, 5, 3, BEAM) == DIMB  # (the dimension before B <= 0)
        assert rf.plain(device, 4, D, 3, 9) == "unknown search mode 9"
        assert rf.plain(device, 4, 5, 3, BEAM) == DIMB
        assert rf.plain(device, 0, D, 3, BEAM) == FLAT
        assert r.plain(device, 0, D, 3, -1) == "unknown search mode -1"
        assert r.plain(device, 0, D, 3, BEAM, ef=4000) is None  # (B <= 0 before the beam mode's ef limit)
        assert re.plain(device, 4, 5, 0, 9) == K0  # (an empty index has no dimension yet)
        assert re.plain(device, 4, 5, 3, 9) == "unknown search mode 9"
        assert ref.plain(device, 4, 5, 3, BEAM) == FLAT
        assert re.plain(device, 4, 5, 3, BEAM, ef=4000) is None and (re.n == 0).all()
        assert re.plain(device, 4, 5, 300, EXACT) is None and (re.n == 0).all()  # (before exact mode's k limit)
        if not device:  # (the entry key is the host call's alone)
            assert r.plain(False, 0, D, 3, BEAM, entry_key=-77) is None
            assert re.plain(False, 4, 5, 3, BEAM, entry_key=-77) is None and (re.n == 0).all()
            assert r.plain(False, 4, D, 3, BEAM, ef=4000, entry_key=-77) == "entry key -77 not in top layer"
            assert r.plain(False, 4, D, 300, EXACT, entry_key=-77) == "entry key -77 not in top layer"
        assert r.plain(device, 4, D, 3, BEAM, ef=4000) == "beam mode supports max(ef,k) <= 2048"
        assert r.plain(device, 4, D, 300, EXACT) == "exact mode supports k <= 256"
        # ---- filtered
        bad = 777  # (a free slot)
        assert r.filtered(device, 4, 5, 0) == K0
        assert r.filtered(device, 1, 5, 3, ef=200) == DIM1
        assert rf.filtered(device, 4, 5, 3) == DIMB
        assert rf.filtered(device, 4, D, 3, ef=200) == FLAT
        assert ref.filtered(device, 4, D, 3, ef=200) == FLAT
        assert r.filtered(device, 0, D, 3, ef=200) == EF128
        assert r.filtered(device, 4, D, 200, route=4096) == EF128
        assert r.filtered(device, 4, D, 3, route=4096, fid=bad) == ROUTE
        assert r.filtered(device, 0, D, 3, route=4096, null_filter=True) == ROUTE
        assert r.filtered(device, 0, D, 3, null_filter=True) is None
        assert r.filtered(device, 4, D, 3, null_filter=True) == NOFILTER
        assert re.filtered(device, 4, D, 3, null_filter=True) == NOFILTER
        assert re.filtered(device, 4, D, 3, ef=200) == EF128
        if device:  # (device ids are the kernel's to check, and no kernel runs on an empty index)
            assert re.filtered(True, 4, D, 3, fid=bad) is None and (re.n == 0).all()
        else:
            assert r.filtered(False, 4, D, 3, fid=bad) == f"unknown filter {bad}"
            assert re.filtered(False, 4, D, 3, fid=bad) == f"unknown filter {bad}"
        assert re.filtered(device, 4, D, 3) is None and (re.n == 0).all()
        assert r.filtered(device, 4, D, 3, fid=f.id) is None and (r.n == 3).all()
        # the handle's EfSearch is the ef of a call that names none, before the width check
        g.EfSearch = 200
        g._sync()
        assert r.filtered(device, 0, D, 3) == EF128
        assert r.filtered(device, 0, D, 3, ef=64) is None
        # validate comes first everywhere
        g.EfSearch = 0
        g._sync()
        assert r.plain(device, 4, 5, 0, 9) == EFSEARCH
        assert r.filtered(device, 4, 5, 0, ef=200) == EFSEARCH
    finally:
        for x in (g, flat, empty, eflat):
            x.close()


def test_timing_state(H):
    """have_timing / have_gemm_timing as each search leaves them: last_kernel_ms()
    and option last_gemm_ns (the exact path's score GEMM) succeed or fail"""
    X, Q, _, allowed = _data()
    g, f = _graph(H, X, allowed)

    def gemm():
        try:
            return g.get_option("last_gemm_ns") >= 0
        except H.HnswError:
            return False

    def state():
        try:
            ms = g.last_kernel_ms() >= 0
        except H.HnswError:
            ms = False
        return ms, gemm()

    try:
        assert state() == (False, False)
        g.search_arrays(Q[:8], 5, mode=H.MODE_BEAM)
        assert state() == (True, False)
        g.search_arrays(Q[:8], 5, mode=H.MODE_EXACT)
        assert state() == (True, True)
        # a failing filtered call leaves both; a failing plain call clears the GEMM's after validate
        with pytest.raises(H.HnswError, match="k must be greater than 0"):
            g.search_filtered_arrays(Q[:8], 0, f)
        assert state() == (True, True)
        with pytest.raises(H.HnswError, match="k must be greater than 0"):
            g.search_arrays(Q[:8], 0, mode=H.MODE_BEAM)
        assert state() == (True, False)
        g.search_arrays(Q[:8], 5, mode=H.MODE_EXACT)
        assert state() == (True, True)
        g.search_filtered_arrays(Q[:8], 5, f)
        assert state() == (True, False)
        g.search_arrays(Q[:8], 5, mode=H.MODE_EXACT)
        g.search_arrays(Q[:8], 5, mode=H.MODE_COMPAT)
        assert state() == (True, False)
    finally:
        g.close()


def test_sticky_word_is_the_device_calls_alone(H):
    import torch

    X, Q, _, allowed = _data()
    g, f = _graph(H, X, allowed)
    try:
        B, k = 8, 5
        want = g.search_arrays(Q[:B], k, mode=H.MODE_BEAM)
        Qd = torch.tensor(Q[:B], device="cuda")
        fo = torch.full((B,), 777, dtype=torch.int32, device="cuda")  # (a free slot)
        ok = torch.empty(B, k, dtype=torch.int64, device="cuda")
        od = torch.empty(B, k, dtype=torch.float32, device="cuda")
        on = torch.full((B,), 99, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        g.search_filtered_device(Qd.data_ptr(), B, D, k, fo.data_ptr(), ok.data_ptr(), od.data_ptr(), on.data_ptr())
        _same(g.search_arrays(Q[:B], k, mode=H.MODE_BEAM), want, "host search after a reporting device search")
        with pytest.raises(H.HnswError, match="unknown filter in filter_of") as e:
            g.device_status()
        assert e.value.code == H._lib.EINVAL
        g.device_status()
        assert (on.cpu().numpy() == 0).all()
    finally:
        g.close()
