"""CPU: the Analyzer's and Relink's symbols are exported, and mhnsw_hops checks its arguments
before it uses the handle or the device (no device is needed: the calls below pass no handle)."""
import ctypes as C

import numpy as np
import pytest

NEW = ("mhnsw_quality_metrics", "mhnsw_degree_histogram", "mhnsw_hops", "mhnsw_reachability", "mhnsw_unreachable_keys",
       "mhnsw_relink")


def test_symbols_exported(H):
    lib = H.load()
    for name in NEW:
        assert name in H.SIGNATURES and hasattr(lib, name), name
    for name in ("Analyzer", "GraphQualityMetrics", "GraphReachability"):
        assert hasattr(H, name), name
    assert hasattr(H.Graph, "Relink") and hasattr(H.Graph, "relink_arrays")
    assert [f for f in H.GraphQualityMetrics.__dataclass_fields__] == [
        "NodeCount", "AvgConnectivity", "ConnectivityStdDev", "DistortionRatio", "LayerBalance", "GraphHeight"]


def _hops(H, keys, n, depth, out):
    lib = H.load()
    kp = None if keys is None else keys.ctypes.data_as(C.POINTER(C.c_int64))
    op = None if out is None else out.ctypes.data_as(C.POINTER(C.c_int32))
    rc = lib.mhnsw_hops(None, kp, n, depth, op)
    return rc, lib.mhnsw_last_error(None).decode()


@pytest.mark.parametrize("keys,out,n,depth,code,msg", [
    (False, True, 4, 10, "EINVAL", "keys and out must be non-NULL"),
    (True, False, 4, 10, "EINVAL", "keys and out must be non-NULL"),
    (True, True, 0, 10, "EINVAL", "hops needs at least 1 key"),
    (True, True, -3, 10, "EINVAL", "hops needs at least 1 key"),
    (True, True, 129, 10, "EUNSUPPORTED", "hops supports at most 128 keys"),
    (True, True, 4, 0, "EINVAL", "max_depth must be in [1, 64], got 0"),
    (True, True, 4, 65, "EINVAL", "max_depth must be in [1, 64], got 65"),
])
def test_hops_argument_checks(H, keys, out, n, depth, code, msg):
    k = np.arange(130, dtype=np.int64) if keys else None
    o = np.full(130 * 130, 7, np.int32) if out else None
    rc, err = _hops(H, k, n, depth, o)
    assert rc == getattr(H._lib, code) and err == msg
    assert o is None or (o == 7).all()  # nothing written
