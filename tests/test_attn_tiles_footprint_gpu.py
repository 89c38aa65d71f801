"""-m gpu: the write footprint of the entry points of include/singa_hip_attn_tiles.h, in the manner of
tests/test_abi_footprint_gpu.py: every view of a call lies inside one poisoned allocation (tests.helpers.Arena), the call runs
over quiet-NaN poison and over 1e30, and  (a) no guard or gap word changed,  (b) every promised element was written,  (c) the two
runs agree bit for bit,  (d) the values are right - the tile map against the rule in numpy, the tiled attention against
`singa_attn_fwd` / `singa_attn_bwd` on the same views (torch.equal).  The mask's batches lie 16 bytes further apart than T * S,
the tile map is written into views of its own, the token-major call reads and writes the column blocks of one [B, T, 512] buffer.

test_attn_tiles_table_matches_header_and_library needs no GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from singa_amd import _capi
from tests.helpers import arena_runs
from tests.test_attn_tiles_gpu import pack, rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["singa_attn_tiled_bwd", "singa_attn_tiled_fwd", "singa_attn_tiles"]
B, HEADS, T = 2, 4, 70
BH = B * HEADS
SCALE = 32 ** -0.5


def test_attn_tiles_table_matches_header_and_library():
    import __graft_entry__
    __graft_entry__.build()
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", strip("singa_hip_attn_tiles.h"))))
    assert declared == sorted(_capi.ATTN_TILES_EXPORTS) == NAMES
    for name in [n for n in dir(_capi) if n.endswith("EXPORTS") and n != "ATTN_TILES_EXPORTS"]:
        assert not set(_capi.ATTN_TILES_EXPORTS) & set(getattr(_capi, name)), name
    raw = ctypes.CDLL(__graft_entry__.LIB)
    assert all(hasattr(raw, n) for n in declared)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):            # declared in its own header only
        if other != "singa_hip_attn_tiles.h":
            text = strip(other)
            assert not any(re.search(r"\b%s\b" % n, text) for n in NAMES), other
    assert "singa_hip_attn_tiles.h" in open(__graft_entry__.__file__).read()   # a dependency of the build


def test_argument_errors_without_gpu():
    import __graft_entry__
    __graft_entry__.build()
    lib = _capi.bind(__graft_entry__.LIB)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    assert lib.singa_attn_tiles(None, 0, 0, p, p, 2, 3, 4, None) == -1 and b"attn_tiles" in lib.singa_last_error_string()
    assert lib.singa_attn_tiles(p, 0, 0, None, p, 2, 3, 4, None) == -1
    assert lib.singa_attn_tiles(p, 0, 0, p, None, 2, 3, 4, None) == -1
    assert lib.singa_attn_tiles(p, -1, 0, p, p, 2, 3, 4, None) == -3
    assert lib.singa_attn_tiles(p, 0, 0, p, p, 0, 3, 4, None) == 0                                   # no batch: nothing to do
    fwd = lambda q, dk: lib.singa_attn_tiled_fwd(q, p, p, p, 0, 0, p, p, 8, 3, 4, 4, dk, 64, 0, 0, 0, 0, SCALE, p, None)
    assert fwd(None, 32) == -1 and b"attn_tiled_fwd" in lib.singa_last_error_string()
    assert fwd(p, 16) == -3
    bwd = lambda q, dk: lib.singa_attn_tiled_bwd(q, p, p, p, 0, 0, p, p, p, p, p, p, p, 8, 3, 4, 4, dk, 64, 0, 0, 0, 0, SCALE, p, p,
                                                 None)
    assert bwd(None, 32) == -1 and b"attn_tiled_bwd" in lib.singa_last_error_string()
    assert bwd(p, 16) == -3


def _p(v):
    return ctypes.c_void_p(v.ptr)


def _case(ar, lib, st):
    g = torch.Generator().manual_seed(77)
    mask = torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1).unsqueeze(0).repeat(B, 1, 1)
    mask[0, :, 69:] = True
    mask[1, :, 66:] = True
    ok = lambda code, what: _ok(lib, code, what)
    vm = ar.view("mask", (B, T, T), torch.uint8, strides=(T * T + 16, T, 1), data=mask.to(torch.uint8))
    qt = (T + 31) // 32
    rows = ar.view("tile_rows", (B, qt, 1), torch.int32, role="out")
    cols = ar.view("tile_cols", (B, qt, 1), torch.int32, role="out")
    ok(lib.singa_attn_tiles(_p(vm), T * T + 16, T, _p(rows), _p(cols), B, T, T, st), "attn_tiles")
    # one mask row for all queries (row stride 0), S = 100: two runs of valid keys in batch 0
    S2 = 100
    pad = torch.ones(B, S2, dtype=torch.bool)
    pad[0, :30], pad[0, 64:70], pad[1, :] = False, False, False
    vp = ar.view("pad", (B, S2), torch.uint8, strides=(S2 + 16, 1), data=pad.to(torch.uint8))
    prow = ar.view("pad_rows", (B, qt, 1), torch.int32, role="out")
    pcol = ar.view("pad_cols", (B, 4, 1), torch.int32, role="out")
    ok(lib.singa_attn_tiles(_p(vp), S2 + 16, 0, _p(prow), _p(pcol), B, T, S2, st), "attn_tiles")

    fused = torch.randn(B, T, 512, generator=g)                                # q | k | v, token-major, one projection buffer
    go = torch.randn(B, T, HEADS, 64, generator=g)
    vf, vgo = ar.view("qkv", fused.shape, data=fused), ar.view("g_ctx", go.shape, data=go)
    blocks = lambda base: [ctypes.c_void_p(base + 4 * off) for off in (0, 128, 256)]
    head = (*blocks(vf.ptr), _p(vm), T * T + 16, T)
    tail = (BH, T, T, HEADS, 32, 64, 1, 512, 512, 512, SCALE)
    for tag in ("tiled.", "plain."):
        ctx, lse = ar.view(tag + "ctx", (B, T, HEADS, 64), role="out"), ar.view(tag + "lse", (BH, T, 2), role="out")
        gf = ar.view(tag + "g_qkv", fused.shape, role="out")
        ds = ar.view(tag + "dsum", (BH, T), role="out")
        if tag == "tiled.":
            ok(lib.singa_attn_tiled_fwd(*head, _p(ctx), _p(lse), *tail, _p(rows), st), "attn_tiled_fwd")
            ok(lib.singa_attn_tiled_bwd(*head, _p(ctx), _p(lse), _p(vgo), *blocks(gf.ptr), _p(ds), *tail, _p(rows), _p(cols), st),
               "attn_tiled_bwd")
        else:
            ok(lib.singa_attn_fwd(*head, _p(ctx), _p(lse), *tail, st), "attn_fwd")
            ok(lib.singa_attn_bwd(*head, _p(ctx), _p(lse), _p(vgo), *blocks(gf.ptr), _p(ds), *tail, st), "attn_bwd")
    return mask, pad.unsqueeze(1), S2


def _ok(lib, code, what):
    assert code == 0, (what, code, lib.singa_last_error_string())


@pytest.mark.gpu
def test_footprint():
    from singa_amd import _lib
    _lib.ensure_init(torch.cuda.current_device())
    lib = _lib.lib()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan, big, differ, (mask, pad, S2) = arena_runs(lambda ar: _case(ar, lib, st), "cuda")
    assert not nan.stray and not big.stray, ("words outside the promised views changed: {view: (count, first offset)}", nan.stray, big.stray)
    assert not nan.unwritten and not big.unwritten, ("promised elements never written: {view: count}", nan.unwritten, big.unwritten)
    assert not differ, ("outputs that depend on what memory held before the call", differ)
    o = nan.out
    u32 = lambda t: t.numpy().view(np.uint32)
    bits = rule(mask, T, T)
    assert int(bits.sum()) == 12                                               # 6 of 9 pairs per batch
    assert np.array_equal(u32(o["tile_rows"]), pack(bits)) and np.array_equal(u32(o["tile_cols"]), pack(bits.transpose(0, 2, 1)))
    bits = rule(pad, T, S2)
    assert int(bits.sum()) == 3 * 2 + 3 * 4
    assert np.array_equal(u32(o["pad_rows"]), pack(bits)) and np.array_equal(u32(o["pad_cols"]), pack(bits.transpose(0, 2, 1)))
    for key in ("ctx", "lse", "g_qkv", "dsum"):
        assert torch.equal(o["tiled." + key], o["plain." + key]), key
