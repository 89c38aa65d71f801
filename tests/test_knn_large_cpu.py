"""singa_knn_graph_large on the cross-compiled library, without a launch: it validates before any HIP call, its header and its
binding table name the same symbols, and singa_knn_graph keeps its refusal above 2,048 atoms."""
import ctypes

import pytest
import torch

from tests.test_capi_exports import declared_symbols


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    from singa_amd import _capi
    __graft_entry__.build()
    return _capi.bind(__graft_entry__.LIB)


def test_header_matches_binding_table():
    from singa_amd import _capi
    assert sorted(_capi.KNN_LARGE_EXPORTS) == declared_symbols("singa_hip_knn_large.h") == ["singa_knn_graph_large"]


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)                                      # never dereferenced: every call below returns before a launch
    assert lib.singa_knn_graph_large(None, p, p, 1, 1, 48, p, p, None) == -1          # SINGA_E_NULL
    assert lib.singa_knn_graph_large(p, p, p, 1, 1, 48, p, None, None) == -1
    for k in (0, 65):
        assert lib.singa_knn_graph_large(p, p, p, 1, 1, k, p, p, None) == -3          # SINGA_E_SHAPE
        assert b"k must be 1 .. 64" in lib.singa_last_error_string()
    assert lib.singa_knn_graph_large(p, p, p, 1, 2 ** 30, 48, p, p, None) == -3       # 3 * N beyond an int32 count
    assert lib.singa_knn_graph_large(p, p, p, 0, 0, 48, p, p, None) == 0
    assert lib.singa_knn_graph_large(p, p, p, 3, 0, 48, p, p, None) == 0
    assert lib.singa_knn_graph(p, p, p, 1, 1, 48, 2049, p, p, None) == -3             # the drop-in entry point keeps its limit
    assert b"2048" in lib.singa_last_error_string()


def test_k_above_64_is_refused_before_the_launch():
    from singa_amd import ops
    pos, batch, ptr = torch.zeros(3, 3), torch.zeros(3, dtype=torch.long), torch.tensor([0, 3])
    with pytest.raises(ValueError, match="k <= 64"):
        ops.knn_graph(pos, 65, batch, ptr, 2049)
    with pytest.raises(ValueError, match="k <= 64"):
        ops.knn_graph(pos, 65, batch, ptr, 3, route="large")
    with pytest.raises(ValueError, match="route"):
        ops.knn_graph(pos, 48, batch, ptr, 3, route="medium")
