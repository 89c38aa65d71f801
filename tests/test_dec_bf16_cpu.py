"""The row-tiled decoder step on the bf16 matrix cores (include/singa_hip_dec_bf16.h) on the cross-compiled library, without a
launch: the header, the binding table and the library name the same symbols, the argument checks return before any HIP call, and
the Python switch refuses bf16 without the row-tiled step before it touches a tensor."""
import ctypes

import pytest

from tests.test_capi_exports import declared_symbols

NAMES = ["singa_dec_bf16_pack", "singa_dec_bf16_tile_cross_attn", "singa_dec_bf16_tile_ffn", "singa_dec_bf16_tile_self_attn"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    from singa_amd import _capi
    __graft_entry__.build()
    return _capi.bind(__graft_entry__.LIB)


def test_header_table_and_library_name_the_same_symbols(lib):
    from singa_amd import _capi
    assert sorted(_capi.DEC_BF16_EXPORTS) == declared_symbols("singa_hip_dec_bf16.h") == NAMES
    for name in [n for n in dir(_capi) if n.endswith("EXPORTS") and n != "DEC_BF16_EXPORTS"]:
        assert not set(_capi.DEC_BF16_EXPORTS) & set(getattr(_capi, name)), name
    assert all(hasattr(lib, name) for name in NAMES)              # (ctypes resolves the symbol on access)


@pytest.mark.parametrize("entry", ["pack", "self_attn", "cross_attn", "ffn"])
def test_argument_errors_without_a_launch(lib, entry):
    buf = (ctypes.c_int64 * 8)()
    p = (ctypes.addressof(buf) + 15) & ~15                         # never dereferenced: every call below returns before a launch
    if entry == "pack":
        call = lambda first=p, K=256, N=512: lib.singa_dec_bf16_pack(first, K, N, p, None)
        bad = ({"K": 48}, {"N": 24}, {"K": 0})
    elif entry == "self_attn":
        call = lambda first=p, R=34, beams=17, P=256, per_row=0, anc=None: lib.singa_dec_bf16_tile_self_attn(
            first, *[p] * 9, per_row, R, beams, P, p, 1e-5, anc, None)
        bad = ({"P": 257}, {"P": 0}, {"R": 33}, {"beams": 0}, {"per_row": 1, "anc": p})
    elif entry == "cross_attn":
        call = lambda first=p, R=34, beams=17, S=65: lib.singa_dec_bf16_tile_cross_attn(first, *[p] * 9, R, beams, S, p, 1e-5, None)
        bad = ({"S": 0}, {"R": 33}, {"beams": 0})
    else:
        call = lambda first=p, R=17: lib.singa_dec_bf16_tile_ffn(first, *[p] * 6, R, p, 1e-5, None)
        bad = ({"R": -1},)
    assert call(first=None) == -1                                  # SINGA_E_NULL
    for kw in bad:
        assert call(**kw) == -3, kw                                # SINGA_E_SHAPE
    assert b"dec_bf16" in lib.singa_last_error_string()
    if entry != "pack":
        assert call(R=0) == 0                                      # nothing to do: no launch either


def test_bf16_without_tiles_is_refused_before_any_launch():
    from singa_amd import ops
    from singa_amd.model.Sampling import check_decoder_precision
    with pytest.raises(ValueError, match="tiles=True"):            # (no argument is looked at before the switch is)
        ops.dec_layer_step(None, None, None, None, None, None, None, None, 1, precision="bf16")
    with pytest.raises(ValueError, match="tiles=True"):
        check_decoder_precision("sample", "bf16", False)
    assert check_decoder_precision("sample", "bf16", True) == "bf16" and check_decoder_precision("sample", "f32", False) == "f32"
