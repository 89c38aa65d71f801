"""-m gpu: dense attention over the score tiles the mask leaves standing (include/singa_hip_attn_tiles.h), through the C ABI.

Two things, per mask:  (a) the tile map of `singa_attn_tiles` is the rule of the header, restated in numpy: both orientations of
the bits and the number of computed pairs;  (b) `singa_attn_tiled_fwd` / `singa_attn_tiled_bwd` give what `singa_attn_fwd` /
`singa_attn_bwd` give on the same inputs - `torch.equal` on ctx, lse, gq, gk, gv and dsum, no tolerance - head-major, token-major
and token-major on pitched operands (q in a padded buffer of its own, k | v as column blocks of one buffer).
Head geometry 32 / 64 channels, 4 heads, B = 2.

The cross-attention case of the issue names the valid keys [0, 37) u [64, 70) of S = 100 and expects key tiles 1 and 3 to be
dead; keys 32..36 lie in tile 1, so under the rule only tile 3 is.  `cross` keeps the keys as named, `cross_dead13` ([0, 30) u
[64, 70)) is the mask that leaves tiles 1 and 3 without a valid key.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

B, HEADS, DK, DV = 2, 4, 32, 64
BH = B * HEADS
SCALE = DK ** -0.5
LAYOUTS = ("head_major", "token_major", "token_major_pitched")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _causal_pad(T, tails):
    m = torch.triu(torch.ones(T, T, dtype=torch.bool), diagonal=1).unsqueeze(0).repeat(B, 1, 1)
    for b, n in enumerate(tails):
        m[b, :, n:] = True
    return m


def _runs(S, runs_per_batch):
    m = torch.ones(B, 1, S, dtype=torch.bool)
    for b, runs in enumerate(runs_per_batch):
        for lo, hi in runs:
            m[b, 0, lo:hi] = False
    return m


def _dead_row():
    T, S = 40, 100
    m = torch.rand(B, T, S, generator=_gen(3)) < 0.4
    m[0, 32:, 32:] = True            # query tile 1 of batch 0: key tiles 1..3 masked in every element, no dead row -> cleared
    m[0, 5, :] = True                # query tile 0 of batch 0 holds a row masked in all keys -> keeps all four bits
    m[1, :, 64:96] = True            # batch 1: key tile 2 dead for both query tiles
    return m


def _one_per_tile():
    T, S = 70, 100
    g = _gen(4)
    m = torch.rand(B, T, S, generator=g) < 0.9
    for b in range(B):
        for qt in range(3):
            for kt in range(4):
                q = qt * 32 + int(torch.randint(0, min(32, T - qt * 32), (1,), generator=g))
                k = kt * 32 + int(torch.randint(0, min(32, S - kt * 32), (1,), generator=g))
                m[b, q, k] = False
    return m


# name -> (T, S, mask [B, T | 1, S]; one row: passed with row stride 0, computed pairs expected (None: whatever the rule says))
CASES = {
    "causal_pad": lambda: (70, 70, _causal_pad(70, (69, 66)), 12),                      # 6 of 9 pairs per batch
    "cross": lambda: (40, 100, _runs(100, ([(0, 37), (64, 70)], [(0, 100)])), 2 * 3 + 2 * 4),
    "cross_dead13": lambda: (40, 100, _runs(100, ([(0, 30), (64, 70)], [(0, 100)])), 2 * 2 + 2 * 4),
    "dead_row": lambda: (40, 100, _dead_row(), 4 + 1 + 3 + 3),
    "one_per_tile": lambda: (70, 100, _one_per_tile(), B * 3 * 4),
    "short_keys": lambda: (40, 20, _runs(20, ([(0, 13)], [(2, 20)])), B * 2),
    "one_query": lambda: (1, 70, _runs(70, ([(0, 20), (64, 66)], [(40, 70)])), 2 + 2),
    "one_query_one_tile": lambda: (1, 70, _runs(70, ([(0, 20)], [(33, 34)])), 1 + 1),
    "batch_all_masked": lambda: (40, 100, _runs(100, ([], [(0, 10)])), 2 * 4 + 2 * 1),   # row stride 0, its one row dead: all bits
}


def rule(mask, T, S):
    """The header's rule in numpy: bits [B, qtiles, ktiles] (True = compute)."""
    m = np.broadcast_to(mask.numpy(), (mask.shape[0], T, S))
    qt, kt = (T + 31) // 32, (S + 31) // 32
    pad = np.ones((m.shape[0], qt * 32, kt * 32), dtype=bool)           # keys >= S count as masked; rows >= T are not looked at
    pad[:, :T, :S] = m
    all_masked = pad.reshape(-1, qt, 32, kt, 32).all(axis=(2, 4))
    dead_row = np.zeros((m.shape[0], qt * 32), dtype=bool)
    dead_row[:, :T] = m.all(axis=2)
    return ~all_masked | dead_row.reshape(-1, qt, 32).any(axis=2)[:, :, None]


def pack(bits):
    """[B, n, m] bool -> u32 [B, n, ceil(m / 32)], bit j % 32 of word j / 32"""
    b, n, m = bits.shape
    w = (m + 31) // 32
    padded = np.zeros((b, n, w * 32), dtype=np.uint64)
    padded[:, :, :m] = bits
    return (padded.reshape(b, n, w, 32) << np.arange(32, dtype=np.uint64)).sum(axis=3).astype(np.uint32)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Lib:
    def __init__(self):
        from singa_amd import _lib
        _lib.ensure_init(torch.cuda.current_device())
        self.lib = _lib.lib()

    def ok(self, code, what):
        assert code == 0, (what, code, self.lib.singa_last_error_string())

    @property
    def st(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.fixture(scope="module")
def L():
    return Lib()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """One case's operands on the device, head-major, made once and never written: (T, S, mask u8 [B, T | 1, S], q, k, v, go, want)"""
    T, S, mask, want = CASES[name]()
    g = _gen(sum(map(ord, name)))
    q, k, v = torch.randn(BH, T, DK, generator=g), torch.randn(BH, S, DK, generator=g), torch.randn(BH, S, DV, generator=g)
    go = torch.randn(BH, T, DV, generator=g)
    return T, S, mask, want, mask.to(torch.uint8).cuda(), q.cuda(), k.cuda(), v.cuda(), go.cuda()


def tile_map(L, mask_dev, T, S):
    qt, kt = (T + 31) // 32, (S + 31) // 32
    rows = torch.full((B, qt, (kt + 31) // 32), -1, dtype=torch.int32, device="cuda")
    cols = torch.full((B, kt, (qt + 31) // 32), -1, dtype=torch.int32, device="cuda")
    mst = 0 if mask_dev.shape[1] == 1 else mask_dev.stride(1)
    L.ok(L.lib.singa_attn_tiles(_p(mask_dev), mask_dev.stride(0), mst, _p(rows), _p(cols), B, T, S, L.st), "attn_tiles")
    return rows, cols, mst


@pytest.mark.parametrize("name", sorted(CASES))
def test_map_is_the_rule(L, name):
    T, S, mask, want, mask_dev = inputs(name)[:5]
    rows, cols, _ = tile_map(L, mask_dev, T, S)
    bits = rule(mask, T, S)
    got_r, got_c = rows.cpu().numpy().view(np.uint32), cols.cpu().numpy().view(np.uint32)
    count = lambda w: int(np.unpackbits(w.view(np.uint8)).sum())
    print(f"{name}: computed pairs {int(bits.sum())} of {bits.size}; rows {count(got_r)}, cols {count(got_c)}")
    assert np.array_equal(got_r, pack(bits))
    assert np.array_equal(got_c, pack(bits.transpose(0, 2, 1)))
    assert count(got_r) == count(got_c) == int(bits.sum())
    if want is not None:
        assert int(bits.sum()) == want
    if name == "one_per_tile":
        assert bits.all()
    if name == "dead_row":
        assert bits[0, 0].all() and bits[0, 1].tolist() == [True, False, False, False] and not bits[1, :, 2].any()
    if name == "batch_all_masked":
        assert bits[0].all()


def _tm(t):
    """[B * heads, T, D] -> token-major [B, T, heads, D]"""
    return t.view(B, HEADS, t.shape[1], t.shape[2]).transpose(1, 2).contiguous()


def _block(rows, width, pitch, off):
    """A [B, rows, HEADS, width / HEADS] column block at column `off` of a NaN-filled [B, rows, pitch] buffer"""
    buf = torch.full((B, rows, pitch), float("nan"), device="cuda")
    return buf, buf[:, :, off:off + width].view(B, rows, HEADS, width // HEADS)


def operands(name, layout):
    T, S, _, _, mask_dev, q, k, v, go = inputs(name)
    if layout == "head_major":
        return dict(q=q, k=k, v=v, go=go, tm=0, ld=(0, 0, 0), like=lambda: (torch.full_like(q, float("nan")),
                    torch.full_like(k, float("nan")), torch.full_like(v, float("nan"))), ctx_shape=(BH, T, DV))
    tq, tk, tv, tgo = _tm(q), _tm(k), _tm(v), _tm(go)
    if layout == "token_major":
        return dict(q=tq, k=tk, v=tv, go=tgo, tm=1, ld=(0, 0, 0), like=lambda: (torch.full_like(tq, float("nan")),
                    torch.full_like(tk, float("nan")), torch.full_like(tv, float("nan"))), ctx_shape=(B, T, HEADS, DV))
    PQ, PKV = HEADS * DK + 16, HEADS * (DK + DV) + 8          # q: a padded buffer of its own; k | v: column blocks of one buffer
    _, pq = _block(T, HEADS * DK, PQ, 0)
    kvbuf, pk = _block(S, HEADS * DK, PKV, 0)
    pv = kvbuf[:, :, HEADS * DK:HEADS * (DK + DV)].view(B, S, HEADS, DV)
    pq.copy_(tq), pk.copy_(tk), pv.copy_(tv)

    def like():
        _, gq = _block(T, HEADS * DK, PQ, 0)
        gbuf, gk = _block(S, HEADS * DK, PKV, 0)
        return gq, gk, gbuf[:, :, HEADS * DK:HEADS * (DK + DV)].view(B, S, HEADS, DV)
    return dict(q=pq, k=pk, v=pv, go=tgo, tm=1, ld=(PQ, PKV, PKV), like=like, ctx_shape=(B, T, HEADS, DV))


def run(L, name, layout, tiled):
    T, S, _, _, mask_dev = inputs(name)[:5]
    o = operands(name, layout)
    rows, cols, mst = tile_map(L, mask_dev, T, S)
    ctx = torch.full(o["ctx_shape"], float("nan"), device="cuda")
    lse = torch.full((BH, T, 2), float("nan"), device="cuda")
    head = (_p(o["q"]), _p(o["k"]), _p(o["v"]), _p(mask_dev), mask_dev.stride(0), mst)
    tail = (BH, T, S, HEADS, DK, DV, o["tm"], *o["ld"], SCALE)
    if tiled:
        L.ok(L.lib.singa_attn_tiled_fwd(*head, _p(ctx), _p(lse), *tail, _p(rows), L.st), "attn_tiled_fwd")
    else:
        L.ok(L.lib.singa_attn_fwd(*head, _p(ctx), _p(lse), *tail, L.st), "attn_fwd")
    gq, gk, gv = o["like"]()
    dsum = torch.full((BH, T), float("nan"), device="cuda")
    if tiled:
        L.ok(L.lib.singa_attn_tiled_bwd(*head, _p(ctx), _p(lse), _p(o["go"]), _p(gq), _p(gk), _p(gv), _p(dsum), *tail, _p(rows),
                                        _p(cols), L.st), "attn_tiled_bwd")
    else:
        L.ok(L.lib.singa_attn_bwd(*head, _p(ctx), _p(lse), _p(o["go"]), _p(gq), _p(gk), _p(gv), _p(dsum), *tail, L.st), "attn_bwd")
    torch.cuda.synchronize()
    return dict(ctx=ctx, lse=lse, gq=gq, gk=gk, gv=gv, dsum=dsum), cols


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_tiled_equals_untiled(L, name, layout):
    T, S, mask = inputs(name)[:3]
    want, _ = run(L, name, layout, tiled=False)
    got, cols = run(L, name, layout, tiled=True)
    for key in ("ctx", "lse", "gq", "gk", "gv", "dsum"):
        assert not bool(torch.isnan(want[key]).any()), key
        assert torch.equal(got[key], want[key]), (key, int((got[key] != want[key]).sum()))
    # a key tile without any computed pair: exact zeros in its dK / dV rows
    dead = (cols.cpu().numpy().view(np.uint32) == 0).all(axis=2)                       # [B, ktiles]
    if name in ("cross", "cross_dead13", "dead_row", "one_query", "one_query_one_tile"):
        assert dead.any()
    hm = (lambda t: t) if layout == "head_major" else (lambda t: t.transpose(1, 2).reshape(BH, t.shape[1], t.shape[3]))
    for b, kt in zip(*np.nonzero(dead)):
        for key in ("gk", "gv"):
            rows_ = hm(got[key])[b * HEADS:(b + 1) * HEADS, kt * 32:min(S, kt * 32 + 32)]
            assert rows_.numel() and float(rows_.abs().max()) == 0.0, (key, b, kt)
    if name == "dead_row":                                # the row masked in all keys: uniform weights, max -1e9, 1 / sum = 1 / S
        st = got["lse"][:HEADS, 5]
        one_over_s = (torch.ones((), device="cuda") / S).item()
        print("dead row lse", st.tolist(), "1 / S", one_over_s)
        assert bool((st[:, 0] == -1e9).all()) and bool((st[:, 1] == one_over_s).all())
