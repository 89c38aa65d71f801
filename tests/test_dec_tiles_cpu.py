"""The row-tiled decoder step (include/singa_hip_dec_tiles.h), the part that runs without a GPU: the header against its binding
table and the built library, the argument errors of the three entry points (all raised before any device call), and
`KVDecoder(tiles=True)`'s refusal of what the tile kernels are not built for."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["singa_dec_tile_cross_attn", "singa_dec_tile_ffn", "singa_dec_tile_self_attn"]
NULL, SHAPE = -1, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_dec_tiles_table_matches_header_and_library(lib):
    from singa_amd import _capi
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", strip("singa_hip_dec_tiles.h"))))
    assert declared == sorted(_capi.DEC_TILES_EXPORTS) == NAMES
    tables = [n for n in dir(_capi) if n.endswith("EXPORTS") and n != "DEC_TILES_EXPORTS"]
    assert len(tables) >= 13
    for name in tables:
        assert not set(_capi.DEC_TILES_EXPORTS) & set(getattr(_capi, name)), name
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):            # declared in its own header only
        if other != "singa_hip_dec_tiles.h":
            text = strip(other)
            assert not any(re.search(r"\b%s\b" % n, text) for n in NAMES), other
    import __graft_entry__
    assert "singa_hip_dec_tiles.h" in open(__graft_entry__.__file__).read()    # a dependency of the build


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    err = lambda: lib.singa_last_error_string()

    def self_attn(ptrs=None, per_row=0, R=10, beams=5, P=8):
        a = [p] * 11 if ptrs is None else ptrs             # x wqkv_t bqkv wo_t bo gamma beta k_cache v_cache pos | y
        return lib.singa_dec_tile_self_attn(*a[:10], per_row, R, beams, P, a[10], 1e-5, None)

    def cross_attn(ptrs=None, R=10, beams=5, S=7):
        a = [p] * 11 if ptrs is None else ptrs             # y wq_t bq ck cv pad wo_t bo gamma beta | z
        return lib.singa_dec_tile_cross_attn(*a[:10], R, beams, S, a[10], 1e-5, None)

    def ffn(ptrs=None, R=10):
        a = [p] * 8 if ptrs is None else ptrs              # z w1_t b1 w2_t b2 gamma beta | out
        return lib.singa_dec_tile_ffn(*a[:7], R, a[7], 1e-5, None)

    for fn, n, name in ((self_attn, 11, b"dec_tile_self_attn"), (cross_attn, 11, b"dec_tile_cross_attn"), (ffn, 8, b"dec_tile_ffn")):
        for i in range(n):                                 # each operand missing in turn
            ptrs = [p] * n
            ptrs[i] = None
            assert fn(ptrs=ptrs) == NULL, (name, i)
            assert name + b":" in err() and b"null" in err()
    for per_row in (0, 1):
        for bad, word in ((dict(P=0), b"256 cached positions"), (dict(P=257), b"256 cached positions"), (dict(beams=0), b"proteins x beams"),
                          (dict(R=11), b"proteins x beams"), (dict(R=-5), b"proteins x beams")):
            assert self_attn(per_row=per_row, **bad) == SHAPE, bad
            assert b"dec_tile_self_attn:" in err() and word in err(), (bad, err())
    for bad, word in ((dict(S=0), b"encoder position"), (dict(S=-3), b"encoder position"), (dict(beams=0), b"proteins x beams"),
                      (dict(R=11), b"proteins x beams")):
        assert cross_attn(**bad) == SHAPE, bad
        assert b"dec_tile_cross_attn:" in err() and word in err(), (bad, err())
    assert ffn(R=-1) == SHAPE and b"dec_tile_ffn:" in err()
    # no rows: a successful no-op, at the limits as well; more than 1024 encoder positions pass the checks
    assert self_attn(R=0) == 0 and self_attn(R=0, P=256, per_row=1) == 0 and self_attn(R=0, P=1, beams=33) == 0
    assert cross_attn(R=0) == 0 and cross_attn(R=0, S=1) == 0 and cross_attn(R=0, S=1500) == 0
    assert ffn(R=0) == 0


def _decoder(hidden=256, key=128, heads=4, ffn=1024):
    attn = SimpleNamespace(hidden_channels=hidden, key_channels=key, num_heads=heads)
    layer = SimpleNamespace(dec_self_attn=attn, pos_ffn=SimpleNamespace(conv1=SimpleNamespace(out_channels=ffn)))
    return SimpleNamespace(layers=[layer], num_props=0)


def test_entry_points_refuse_tiles_before_the_encoder_runs():
    """`sample` and `beam_search` call `check_tiles` ahead of `encode_pockets`: the same refusals as `KVDecoder`'s, earlier."""
    from singa_amd.model.Sampling import check_tiles
    check_tiles("sample", _decoder(), 201, None)
    check_tiles("sample", _decoder(), 256, True)
    for dec, positions, fused, word in ((_decoder(), 201, False, "fused=False"), (_decoder(hidden=128), 201, None, "geometry"),
                                        (_decoder(ffn=512), 201, True, "geometry"), (_decoder(), 257, None, "256 positions")):
        with pytest.raises(ValueError, match=word):
            check_tiles("sample", dec, positions, fused)


@pytest.mark.parametrize("what, kw", [("fused=False", dict(fused=False)), ("hidden 128", dict(hidden=128)), ("2 heads", dict(heads=2)),
                                      ("key 64", dict(key=64)), ("ffn 512", dict(ffn=512)), ("257 positions", dict(positions=257))])
def test_kvdecoder_refuses_tiles_before_any_launch(what, kw):
    """tiles=True is a form of the fused step: with fused=False, another decoder geometry or more than 256 positions the
    constructor raises before it touches a tensor (the operands here are `meta` tensors: nothing could be launched on them)."""
    import torch
    from singa_amd.model.BeamSearch import KVDecoder
    kw = dict(kw)
    fused, positions = kw.pop("fused", True), kw.pop("positions", 64)
    enc = torch.empty(2, 1100, 256, device="meta")
    pad = torch.empty(2, 1, 1100, dtype=torch.bool, device="meta")
    with pytest.raises(ValueError, match="tiles=True"):
        KVDecoder(_decoder(**kw), None, enc, pad, 5, positions, 30, fused=fused, search_buffers=False, tiles=True)
