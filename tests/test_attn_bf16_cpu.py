"""The dense attention core with bf16 operands (include/singa_hip_attn_bf16.h) on the cross-compiled library, without a launch: the
header, the binding table and the library name the same two symbols, and the argument checks return before any HIP call."""
import ctypes

import pytest

from tests.test_capi_exports import declared_symbols

NAMES = ["singa_attn_bf16_bwd", "singa_attn_bf16_fwd"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    from singa_amd import _capi
    __graft_entry__.build()
    return _capi.bind(__graft_entry__.LIB)


def test_header_table_and_library_name_the_same_symbols(lib):
    from singa_amd import _capi
    assert sorted(_capi.ATTN_BF16_EXPORTS) == declared_symbols("singa_hip_attn_bf16.h") == NAMES
    for name in [n for n in dir(_capi) if n.endswith("EXPORTS") and n != "ATTN_BF16_EXPORTS"]:
        assert not set(_capi.ATTN_BF16_EXPORTS) & set(getattr(_capi, name)), name
    assert all(hasattr(lib, name) for name in NAMES)              # (ctypes resolves the symbol on access)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_argument_errors_without_a_launch(lib, direction):
    buf = (ctypes.c_int64 * 8)()
    p = ctypes.addressof(buf)                                      # never dereferenced: every call below returns before a launch
    nptr = 2 if direction == "fwd" else 7                          # ctx, lse | ctx, lse, g_ctx, g_q, g_k, g_v, dsum
    maps = [None] * (1 if direction == "fwd" else 2)

    def call(first=p, BH=8, heads=4, DK=32, DV=64):
        return getattr(lib, f"singa_attn_bf16_{direction}")(first, p, p, p, 0, 0, *[p] * nptr, BH, 33, 33, heads, DK, DV, 0, 0, 0, 0,
                                                           0.125, *maps, None)
    assert call(first=None) == -1                                  # SINGA_E_NULL
    for kw in ({"DK": 64}, {"DV": 32}, {"BH": 6}, {"heads": 0}):
        assert call(**kw) == -3, kw                                # SINGA_E_SHAPE
    assert b"attn_bf16" in lib.singa_last_error_string()
    assert call(BH=0) == 0                                         # nothing to do: no launch either
