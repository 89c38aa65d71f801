"""-m gpu: the row-tiled decoder step (include/singa_hip_dec_tiles.h: singa_dec_tile_self_attn / _cross_attn / _ffn through
`ops.dec_layer_step(tiles=True)` and `KVDecoder(tiles=True)`).

Kernel level, one decoder layer of the shipped geometry against the float64 reference of tests/test_decode_kernels_gpu.py (the
layer evaluated on the whole sequence with a causal mask), errors by tests.helpers.rowwise_err under that file's bound TOL = 2e-5:
all 256 cache positions for pockets of 1 .. 1500 atoms (1025 and 1500 are beyond k17's limit; 63 / 65 and 1024 / 1025 lie on both
sides of a chunk boundary of the running softmax), tile boundaries (1, 16, 17, 33 rows per pocket), rows that do not depend - to
the bit - on their neighbours in the tile, one position per row, the write footprint, and graph replay = eager.

End to end on the `beam_b2_k6_eos` golden model: `sample(tiles=True)` against the CPU oracle decision by decision with the
settings and bounds of tests/test_sampling_gpu.py; `score`, `sample_stream`, `sample_distinct` and `beam_search_device` with
`tiles=True` against each other bit for bit; and a pocket of 1,100 atoms, which only this path decodes with the step kernels.

One tile height is built (16 rows), so the comparison "TR = 16 against TR = 32, bit for bit" has nothing to compare; what it
would show - a row's bits do not depend on its tile - is what `test_rows_do_not_depend_on_their_neighbours` asserts.

Measured on MI355X (profiles/dec_tiles/README.md has every figure): against float64, outputs 4.7e-7 .. 5.7e-7, key cache
5.4e-7 .. 6.2e-7, value cache 4.5e-7 .. 5.2e-7 over all cases (k17: 2.2e-7 .. 3.8e-7; bound 2e-5); end to end 1,255 - 2,560 live
decisions per setting, 0 - 0.54 % ambiguous, no mismatch, log-probabilities within 1.93e-6 of the oracle's (4 x = 7.7e-6 <= EPS);
logits of the two paths within 8.1e-7 row-wise; the 1,100-atom pocket: 33 live decisions, 1 ambiguous, no mismatch.
"""
import ctypes
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import singa_oracle as O
from tests.helpers import arena_runs, golden, rowwise_err, smi_voc
from tests.test_decode_kernels_gpu import TOL, make_layer

pytestmark = pytest.mark.gpu
DEV = "cuda"
I64, U8, I32 = torch.int64, torch.uint8, torch.int32


@pytest.fixture(scope="module", autouse=True)
def stream_pool_left_as_found():
    """torch hands streams out of a pool of 32 per device, round robin, and every captured generation below takes one
    (`capture_steps`' warm-up stream).  Which pool stream a later module's first `ops.branch_stream()` becomes - and with it the
    hardware queue that stream shares with others - depends on how many were taken before it; tests/test_stream_overlap_gpu.py
    needs that stream to run BESIDE the current one.  So this module leaves the pool's cursor where it found it: one full turn
    of the ring on the way in, and on the way out as many draws as bring the cursor back."""
    ring = [torch.cuda.Stream() for _ in range(32)]
    yield
    for _ in range(32):
        if torch.cuda.Stream() == ring[-1]:
            break


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def same(a, b):
    a, b = torch.as_tensor(a).cpu().contiguous(), torch.as_tensor(b).cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


# ------------------------------------------------------------------------------------------------ one layer, any shape
def make_kv(layer, enc, pad, beams, P, tiles=True):
    """A one-layer KVDecoder: the transposed weights and the projected encoder keys / values exactly as generation has them."""
    from singa_amd.model.BeamSearch import KVDecoder
    dec = SimpleNamespace(layers=[layer], num_props=0)
    with torch.no_grad():
        kv = KVDecoder(dec, None, enc.to(DEV), pad.to(DEV), beams, P, 1, fused=True, search_buffers=False, tiles=tiles)
    assert kv.fused and kv.tiles == tiles
    return kv


def inputs(B, beams, n, S, seed):
    """x [B * beams, n, 256], enc [B, S, 256], pad [B, 1, S]: pocket 1 ragged, the last pocket (if B > 2) fully padded - as
    `inputs` of tests/test_decode_kernels_gpu.py makes them."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * beams, n, 256, generator=g)
    enc = torch.randn(B, S, 256, generator=g)
    pad = torch.zeros(B, 1, S, dtype=torch.bool)
    if B > 1:
        pad[1, 0, max(1, (2 * S) // 3):] = True
    if B > 2:
        pad[2] = True
    return x, enc, pad


def reference(sd, x, enc, pad, beams):
    """x [R, n, 256] f64 -> (layer output [R, n, 256], K [R, 4, n, 32], V [R, 4, n, 64]): one causal attention over all
    positions, the encoder rows of pocket r // beams."""
    n = x.shape[1]
    causal = torch.triu(torch.ones(n, n, dtype=torch.bool), 1).unsqueeze(0).expand(x.shape[0], n, n)
    enc_r = enc.double().repeat_interleave(beams, 0)
    mask = pad.repeat_interleave(beams, 0).expand(x.shape[0], n, pad.shape[2])
    with torch.no_grad():
        y = O.dense_mha(sd, "l.dec_self_attn", x, x, x, causal)
        y = O.dense_mha(sd, "l.dec_enc_attn", y, enc_r, enc_r, mask)
        out = O.pos_ffn(sd, "l.pos_ffn", y)
        k = O.lin(sd, "l.dec_self_attn.W_K", x).view(x.shape[0], n, 4, 32).transpose(1, 2)
        v = O.lin(sd, "l.dec_self_attn.W_V", x).view(x.shape[0], n, 4, 64).transpose(1, 2)
    return out, k, v


def decode(kv, x):
    """All of x's positions through the step kernels -> outputs [R, n, 256] (CPU)."""
    xd = x.to(DEV)
    with torch.no_grad():
        outs = [kv.advance(xd[:, pos].contiguous()) for pos in range(x.shape[1])]
    torch.cuda.synchronize()
    return torch.stack(outs, 1).cpu()


def check(tag, got, kv, want, wk, wv):
    n = want.shape[1]
    e_out = rowwise_err(got.reshape(-1, 256), want.reshape(-1, 256), f"{tag} outputs (row = decoder row * {n} + position)")
    e_k = rowwise_err(kv.k[0, :, :, :n].cpu().reshape(-1, 32), wk.reshape(-1, 32), f"{tag} key cache")
    e_v = rowwise_err(kv.v[0, :, :, :n].cpu().reshape(-1, 64), wv.reshape(-1, 64), f"{tag} value cache")
    assert e_out <= TOL and e_k <= TOL and e_v <= TOL, (tag, e_out, e_k, e_v)


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("S", [1, 63, 65, 300, 1024, 1025, 1500])
def test_all_256_positions_against_float64(S):
    """Every cache position 0..255 for 3 pockets x 5 rows (one partial tile per pocket, rows 5 of 16), a ragged and a fully
    padded pocket; 1025 and 1500 encoder positions are beyond what k17 takes."""
    B, beams, P = 3, 5, 256
    layer, sd = make_layer(S)
    x, enc, pad = inputs(B, beams, P, S, 1000 + S)
    kv = make_kv(layer, enc, pad, beams, P)
    assert kv.P == 256 and kv.R == 15 and bool(pad[2].all()) and not bool(pad[0].any())
    got = decode(kv, x)
    assert int(kv.pos) == 256                              # the last slot of the cache was written
    want, wk, wv = reference(sd, x.double(), enc, pad, beams)
    check(f"tiles S={S}", got, kv, want, wk, wv)


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("beams", [1, 16, 17, 33])
def test_tile_boundaries(beams):
    """1 row (15 of a tile's rows missing), exactly one tile, one tile + 1 row, two tiles + 1 row per pocket."""
    B, S, n = 2, 65, 40
    layer, sd = make_layer(100 + beams)
    x, enc, pad = inputs(B, beams, n, S, 2000 + beams)
    kv = make_kv(layer, enc, pad, beams, n)
    got = decode(kv, x)
    want, wk, wv = reference(sd, x.double(), enc, pad, beams)
    check(f"tiles beams={beams}", got, kv, want, wk, wv)


# ---------------------------------------------------------------------------------------------------------------- 3
def test_rows_do_not_depend_on_their_neighbours():
    """The same 7 rows per pocket (inputs, hence caches) once as the pocket's only rows and once at scattered places among 33
    rows of other data - in the first, the second and the third tile, at other offsets inside them: the same bits in their
    outputs and cache rows at every position."""
    B, S, n = 2, 65, 24
    where = torch.tensor([1, 4, 15, 16, 22, 31, 32])
    layer, _ = make_layer(31)
    x7, enc, pad = inputs(B, 7, n, S, 3007)
    x33 = torch.randn(B * 33, n, 256, generator=torch.Generator().manual_seed(3033))
    rows33 = torch.cat([b * 33 + where for b in range(B)])
    x33[rows33] = x7
    kv7, kv33 = make_kv(layer, enc, pad, 7, n), make_kv(layer, enc, pad, 33, n)
    got7, got33 = decode(kv7, x7), decode(kv33, x33)
    assert same(got33[rows33], got7)
    assert same(kv33.k[0, rows33.to(DEV)], kv7.k[0]) and same(kv33.v[0, rows33.to(DEV)], kv7.v[0])
    other = torch.ones(B * 33, dtype=torch.bool)
    other[rows33] = False
    assert not same(got33[other][:B * 7], got7)            # (the comparison above is not one of constants)


# ---------------------------------------------------------------------------------------------------------------- 4
def _self_attn_direct(kv, x, k, v, pos, per_row, y):
    from singa_amd import _capi, _lib, ops
    a = kv.w[0]["self"]
    code = _lib.lib().singa_dec_tile_self_attn(
        ops._p(x), ops._p(a["wqkv_t"]), ops._p(a["bqkv"]), ops._p(a["wo_t"]), ops._p(a["bo"]), ops._p(a["gamma"]), ops._p(a["beta"]),
        ops._p(k), ops._p(v), ops._p(pos), per_row, x.shape[0], kv.beams, k.shape[2], ops._p(y), a["eps"], ops._stream())
    _capi.check(_lib.lib(), code, "singa_dec_tile_self_attn")


def test_per_row_positions():
    from singa_amd import ops
    B, beams, P, S = 2, 9, 40, 65
    R = B * beams
    layer, sd = make_layer(41)
    x, enc, pad = inputs(B, beams, P, S, 4001)
    # (a) the same position in every row: the bits of the one-position form, step by step
    kva, kvb = make_kv(layer, enc, pad, beams, P), make_kv(layer, enc, pad, beams, P)
    xd = x.to(DEV)
    with torch.no_grad():
        for pos in range(P):
            one = kva.advance(xd[:, pos].contiguous())
            per = kvb.advance(xd[:, pos].contiguous(), row_pos=torch.full((R,), pos, dtype=I64, device=DEV))
            assert same(one, per), pos
    assert same(kva.k, kvb.k) and same(kva.v, kvb.v)
    # (b) every row at a position of its own, on caches that hold the rows' whole sequences: a row sees its own prefix only
    want, _, _ = reference(sd, x.double(), enc, pad, beams)
    rp = torch.tensor([-1, 0, 3, P - 1, P, 7, 1, 38, 20, 5, -3, 12, 39, 2, P + 7, 31, 17, 0], dtype=I64)
    assert len(rp) == R
    live = (rp >= 0) & (rp < P)
    at = rp.clamp(0, P - 1)
    x_at = x[torch.arange(R), at].contiguous()
    k0, v0 = kva.k.clone(), kva.v.clone()
    with torch.no_grad():
        out = ops.dec_layer_step(x_at.to(DEV), kva.w[0], kva.k[0], kva.v[0], rp.to(DEV), kva.cross_k[0], kva.cross_v[0], kva.pad_u8,
                                 beams, per_row=True, tiles=True).cpu()
    err = rowwise_err(out[live], want[torch.arange(R), at][live], "tiles per-row positions: outputs of the live rows")
    assert err <= TOL, err
    # what was appended is what was there (same inputs at the same positions), to rounding; dead rows' caches keep their bits
    assert same(kva.k[0, (~live).to(DEV)], k0[0, (~live).to(DEV)]) and same(kva.v[0, (~live).to(DEV)], v0[0, (~live).to(DEV)])
    assert same(kva.k, k0) and same(kva.v, v0)             # a live row re-appends the very bits it appended in (a)
    # the self-attention launch alone, outputs and caches over a canary: rows at -1, -3, P and P + 7 keep it
    canary = 1234.5
    y = torch.full((R, 256), canary, device=DEV)
    kc, vc = torch.full_like(kva.k[0], canary), torch.full_like(kva.v[0], canary)
    _self_attn_direct(kva, x_at.to(DEV), kc, vc, rp.to(DEV), 1, y)
    torch.cuda.synchronize()
    y, kc, vc = y.cpu(), kc.cpu(), vc.cpu()
    assert bool((y[~live] == canary).all()) and bool((kc[~live] == canary).all()) and bool((vc[~live] == canary).all())
    assert bool((y[live] != canary).all())
    for r in torch.nonzero(live)[:, 0].tolist():
        keep = torch.ones(P, dtype=torch.bool)
        keep[rp[r]] = False
        assert bool((kc[r][:, keep] == canary).all()) and bool((vc[r][:, keep] == canary).all()), r
        assert same(kc[r][:, rp[r]], k0[0, r][:, rp[r]]) and same(vc[r][:, rp[r]], v0[0, r][:, rp[r]]), r


# ---------------------------------------------------------------------------------------------------------------- 5
def _footprint(fn):
    """Both runs of one case (tests.helpers.arena_runs: NaN and 1e30 canaries), then: no word outside the promised views changed,
    every promised element written, the two runs bit-identical, values within their bound."""
    nan, big, differ, verify = arena_runs(fn, DEV)
    rows = verify(nan.out)
    assert not nan.stray and not big.stray, ("words outside the promised views changed: {view: (count, first offset)}", nan.stray, big.stray)
    assert not nan.unwritten and not big.unwritten, ("promised elements never written: {view: count}", nan.unwritten, big.unwritten)
    assert not differ, ("outputs that depend on what memory held before the call", differ)
    for label, got, want, bound in rows:
        err = rowwise_err(got, want, f"footprint {label} (bound {bound:.0e})")
        assert err <= bound, (label, err)


def _fp_tools():
    from tests.test_abi_footprint_gpu import Env, _dec_weights, _ln, _views, d64, gen, p, rn
    return Env(), _dec_weights, _ln, _views, d64, gen, p, rn


SHAPES = [(3, 5), (2, 17), (1, 1)]                         # partial tiles only; a full tile + 1 row; R = 1


@pytest.mark.parametrize("per_row", [0, 1])
@pytest.mark.parametrize("B, beams", SHAPES)
def test_footprint_self_attn(B, beams, per_row):
    """Of the caches only position pos of every live row changes; the slots behind it hold NaN and must not be read; y is
    written in exactly the live rows.  per_row: rows 0 and R - 1 lie outside the cache (R > 1)."""
    E, _dec_weights, _ln, _views, d64, gen, p, rn = _fp_tools()
    R, P = B * beams, 67
    g = gen(400 + R)
    w = _dec_weights(g, [("wqkv_t", (256, 512)), ("bqkv", (512,)), ("wo_t", (256, 256)), ("bo", (256,)), ("gamma", (256,)), ("beta", (256,))])
    x = rn(g, R, 256)
    kc, vc = rn(g, R, 4, P, 32), rn(g, R, 4, P, 64)
    pos = torch.randint(0, P, (R,), generator=g) if per_row else torch.full((1,), 41, dtype=I64)
    if per_row and R > 1:
        pos[0], pos[R - 1] = -1, P
    rp = pos if per_row else pos.expand(R)
    live = (rp >= 0) & (rp < P)

    kd, vd = kc.clone(), vc.clone()
    for r in range(R):                                     # behind a row's position: NaN, which must not be read
        kd[r, :, max(int(rp[r]), 0) + 1:], vd[r, :, max(int(rp[r]), 0) + 1:] = float("nan"), float("nan")

    def fn(ar):
        vx = ar.view("x", x.shape, data=x)
        vw = _views(ar, list(w.items()))
        vk, vv = ar.view("k_cache", kc.shape, data=kd, role="inout"), ar.view("v_cache", vc.shape, data=vd, role="inout")
        vpos = ar.view("pos", pos.shape, I64, data=pos)
        y = ar.view("y", (R, 256), role="out", promised=live.view(R, 1))
        E.ok(E.lib.singa_dec_tile_self_attn(p(vx), *[p(vw[k]) for k in ("wqkv_t", "bqkv", "wo_t", "bo", "gamma", "beta")], p(vk), p(vv),
                                            p(vpos), per_row, R, beams, P, p(y), 1e-5, E.st), "dec_tile_self_attn")

        def verify(o):
            d = {k_: d64(t) for k_, t in w.items()}
            qkv = d64(x) @ d["wqkv_t"] + d["bqkv"]
            qn, kn, vn = qkv[:, :128].view(R, 4, 32), qkv[:, 128:256].view(R, 4, 32), qkv[:, 256:].view(R, 4, 64)
            rows = []
            for r in range(R):
                keep = torch.ones(P, dtype=torch.bool)
                if live[r]:
                    keep[rp[r]] = False
                for name, init in (("k_cache", kd), ("v_cache", vd)):
                    assert torch.equal(o[name][r][:, keep].view(I32), init[r][:, keep].view(I32)), (name, r)
                if not live[r]:
                    continue
                t = int(rp[r])
                K = torch.cat([d64(kc)[r, :, :t], kn[r].unsqueeze(1)], 1)
                V = torch.cat([d64(vc)[r, :, :t], vn[r].unsqueeze(1)], 1)
                att = torch.softmax(torch.einsum("hd,hpd->hp", qn[r], K) / math.sqrt(32), -1)
                ctx = torch.einsum("hp,hpd->hd", att, V).reshape(256)
                rows.append((_ln(ctx @ d["wo_t"] + d["bo"] + d64(x)[r], d["gamma"], d["beta"]), kn[r].reshape(-1), vn[r].reshape(-1),
                             o["y"][r], o["k_cache"][r][:, t].reshape(-1), o["v_cache"][r][:, t].reshape(-1)))
            col = lambda i: torch.stack([row[i] for row in rows])
            return [("self_attn y", col(3), col(0), 2e-5), ("k_cache[pos]", col(4), col(1), 2e-5), ("v_cache[pos]", col(5), col(2), 2e-5)]
        return verify
    _footprint(fn)


@pytest.mark.parametrize("S", [77, 1100])
@pytest.mark.parametrize("B, beams", SHAPES)
def test_footprint_cross_attn(B, beams, S):
    E, _dec_weights, _ln, _views, d64, gen, p, rn = _fp_tools()
    R = B * beams
    g = gen(500 + R + S)
    w = _dec_weights(g, [("wq_t", (256, 128)), ("bq", (128,)), ("wo_t", (256, 256)), ("bo", (256,)), ("gamma", (256,)), ("beta", (256,))])
    y, ck, cv = rn(g, R, 256), rn(g, B, 4, 32, S), rn(g, B, 4, S, 64)
    pad = torch.zeros(B, S, dtype=U8)
    if B > 1:
        pad[1, 2 * S // 3:] = 1
    if B > 2:
        pad[2] = 1

    def fn(ar):
        vy, vck, vcv, vpad = ar.view("y", y.shape, data=y), ar.view("ck", ck.shape, data=ck), ar.view("cv", cv.shape, data=cv), \
            ar.view("pad", pad.shape, U8, data=pad)
        vw = _views(ar, list(w.items()))
        z = ar.view("z", (R, 256), role="out")
        E.ok(E.lib.singa_dec_tile_cross_attn(p(vy), p(vw["wq_t"]), p(vw["bq"]), p(vck), p(vcv), p(vpad), p(vw["wo_t"]), p(vw["bo"]),
                                             p(vw["gamma"]), p(vw["beta"]), R, beams, S, p(z), 1e-5, E.st), "dec_tile_cross_attn")

        def verify(o):
            d = {k_: d64(t) for k_, t in w.items()}
            qn = (d64(y) @ d["wq_t"] + d["bq"]).view(R, 4, 32)
            prot = torch.arange(R) // beams
            sc = torch.einsum("rhd,rhds->rhs", qn, d64(ck)[prot]) / math.sqrt(32)
            sc = sc.masked_fill(pad.bool()[prot].unsqueeze(1), -1e9)
            ctx = torch.einsum("rhs,rhsd->rhd", torch.softmax(sc, -1), d64(cv)[prot]).reshape(R, 256)
            return [("cross_attn z", o["z"], _ln(ctx @ d["wo_t"] + d["bo"] + d64(y), d["gamma"], d["beta"]), 2e-5)]
        return verify
    _footprint(fn)


@pytest.mark.parametrize("R", [15, 17, 1])
def test_footprint_ffn(R):
    E, _dec_weights, _ln, _views, d64, gen, p, rn = _fp_tools()
    g = gen(600 + R)
    w = _dec_weights(g, [("w1_t", (256, 1024)), ("b1", (1024,)), ("w2_t", (1024, 256)), ("b2", (256,)), ("gamma", (256,)), ("beta", (256,))])
    z = rn(g, R, 256)

    def fn(ar):
        vz = ar.view("z", z.shape, data=z)
        vw = _views(ar, list(w.items()))
        out = ar.view("out", (R, 256), role="out")
        E.ok(E.lib.singa_dec_tile_ffn(p(vz), *[p(vw[k]) for k in ("w1_t", "b1", "w2_t", "b2", "gamma", "beta")], R, p(out), 1e-5, E.st),
             "dec_tile_ffn")

        def verify(o):
            d = {k_: d64(t) for k_, t in w.items()}
            h = torch.relu(d64(z) @ d["w1_t"] + d["b1"])
            return [("ffn out", o["out"], _ln(h @ d["w2_t"] + d["b2"] + d64(z), d["gamma"], d["beta"]), 2e-5)]
        return verify
    _footprint(fn)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_captured_equals_eager():
    """20 steps of KVDecoder(tiles=True).advance replayed from one HIP graph (the position is a device scalar that the step itself
    advances) against 20 eager steps: the same bits in every output row and in the caches."""
    from singa_amd.model.BeamSearch import capture_steps
    B, beams, P, S, n = 2, 17, 32, 65, 20
    layer, _ = make_layer(61)
    x, enc, pad = inputs(B, beams, n, S, 6001)
    kv = make_kv(layer, enc, pad, beams, P)
    eager = decode(kv, x)
    k_eager, v_eager = kv.k.clone(), kv.v.clone()
    kv.k.zero_(), kv.v.zero_(), kv.reset()
    xd = x.to(DEV)
    x_in, out = xd[:, 0].contiguous(), torch.empty(B * beams, 256, device=DEV)

    def body():
        out.copy_(kv.advance(x_in))
    with torch.no_grad():
        replay, = capture_steps(kv.reset, [body], 2)
        kv.reset(), kv.k.zero_(), kv.v.zero_()
        outs = []
        for pos in range(n):
            x_in.copy_(xd[:, pos])
            replay()
            outs.append(out.clone())
    torch.cuda.synchronize()
    assert int(kv.pos) == n
    assert same(torch.stack(outs, 1), eager)
    assert same(kv.k, k_eager) and same(kv.v, v_eager)


# ---------------------------------------------------------------------------------------------------------------- 7
@pytest.fixture(scope="module")
def setup():
    from tests.test_beam_gpu import build_model
    from tests.test_sampling_gpu import example_of
    z = golden("beam_b2_k6_eos.npz")
    model, sd, _ = build_model(z)                            # `sd` (the oracle's weights) carries the golden's gains too
    return z, model, sd, example_of(z)


def _settings():
    from tests.test_sampling_gpu import IDS, SETTINGS
    return dict(argvalues=SETTINGS, ids=IDS)


@pytest.mark.parametrize("setting", **_settings())
def test_sample_matches_oracle_decision_by_decision(setup, setting):
    """2 pockets x 32 rows, 40 steps, the settings of tests/test_sampling_gpu.py and its bounds: no mismatch among the unambiguous
    decisions, at most 2 % left out as ambiguous (decided from the oracle's numbers alone), EPS >= 4 x the largest deviation of
    a log-probability."""
    from tests.sampling_rule import EPS
    from tests.test_sampling_gpu import oracle_check, run, well_formed
    z, model, sd, ex = setup
    tokens, u, prop, tr = run(z, model, setting=setting, ex=ex, tiles=True)
    assert tr["path"] == "tiles"
    lengths, tok_logp = tr["lengths"].cpu().numpy(), tr["token_logp"].cpu().numpy()
    well_formed(tokens, lengths)
    res = oracle_check(z, sd, tokens, u, prop, setting)
    dev = float(np.abs(tok_logp.astype(np.float64) - res["logp"])[:, 1:].max())
    share = res["ambiguous"] / res["live"]
    print(f"tiles, setting {setting}: {res['live']} live decisions, {res['ambiguous']} ambiguous ({100 * share:.2f} %), "
          f"{len(res['bad'])} mismatches, max |device logp - oracle logp| {dev:.3e}, steps {tr['steps']}")
    assert not res["bad"], res["bad"][:10]
    assert share <= 0.02, share
    assert EPS >= 4 * dev, dev


@pytest.fixture(scope="module")
def drawn(setup):
    from tests.test_sampling_gpu import run
    z, model, sd, ex = setup
    tokens, u, prop, tr = run(z, model, ex=ex, tiles=True)
    return tokens, u, {k: tr[k].cpu() for k in ("lengths", "sum_logp", "token_logp")}


def test_score_reproduces_the_drawn_rows(setup, drawn):
    from singa_amd.model.Sampling import score
    z, model, sd, ex = setup
    voc = smi_voc()
    eos, B, per = voc.index("$"), 2, 32
    tokens, _, tr = drawn
    lengths, sums, tlp = tr["lengths"].numpy(), tr["sum_logp"].numpy(), tr["token_logp"].numpy()
    mols = [[] for _ in range(B)]
    for r in range(B * per):
        n = int(lengths[r])
        if tokens[r, n] == eos:
            mols[r // per].append((r, [int(t) for t in tokens[r, 1:n]]))
    assert all(len(m) >= 4 for m in mols)
    sc = score(model, voc, [[m for _, m in mb] for mb in mols], B, ex, torch.as_tensor(z["prop"][:1]).float(), device=DEV,
               max_length=tokens.shape[1], tiles=True)
    assert sc["path"] == "tiles"
    for b in range(B):
        for i, (r, m) in enumerate(mols[b]):
            assert sc["length"][b][i] == len(m) + 1 == lengths[r]
            assert bits(np.float32(sc["sum_logp"][b][i])) == bits(sums[r]), (b, r)
            assert np.array_equal(bits(sc["token_logp"][b][i]), bits(tlp[r, 1:1 + len(m) + 1])), (b, r)


@pytest.mark.parametrize("R", [1, 5, 37])
def test_stream_equals_sample_bit_for_bit(setup, drawn, R):
    from singa_amd.model.Sampling import sample_stream
    z, model, sd, ex = setup
    tokens, u, tr = drawn
    st = {}
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(2, 1).to(DEV)
    got = sample_stream(model, smi_voc(), 32, 2, tokens.shape[1], ex, prop, R, device=DEV, uniforms=u, trace=st, tiles=True)
    torch.cuda.synchronize()
    assert st["path"] == "tiles"
    assert np.array_equal(got.cpu().numpy(), tokens)
    for k in ("lengths", "sum_logp", "token_logp"):
        assert same(st[k], tr[k]), k


def test_distinct_and_device_beam_sums_are_scores_bits(setup):
    from singa_amd.model.BeamSearch import beam_search_device
    from singa_amd.model.Sampling import sample_distinct, score
    z, model, sd, ex = setup
    voc = [str(v) for v in smi_voc()]
    eos, B, T = voc.index("$"), 2, 41
    prop1 = torch.as_tensor(z["prop"][:1]).float()
    # sampling without replacement
    k = 24
    tr = {}
    out = sample_distinct(model, voc, k, B, T, ex, prop1.repeat(B * k, 1).to(DEV), device=DEV, suppress=("&", "^"), seed=4, trace=tr,
                          tiles=True).cpu().numpy().reshape(B, k, T)
    assert tr["path"] == "tiles" and bool(tr["valid"].all())
    lengths, sums = tr["lengths"].cpu().numpy().reshape(B, k), tr["sum_logp"].cpu().numpy().reshape(B, k)
    mols = [[] for _ in range(B)]
    for b in range(B):
        assert len({tuple(r) for r in out[b]}) == k
        for r in range(k):
            n = int(lengths[b, r])
            if out[b, r, n] == eos:
                mols[b].append((r, [int(t) for t in out[b, r, 1:n]]))
    assert all(len(m) >= 1 for m in mols)
    sc = score(model, voc, [[m for _, m in mb] for mb in mols], B, ex, prop1, device=DEV, max_length=T, tiles=True)
    for b in range(B):
        for i, (r, m) in enumerate(mols[b]):
            assert bits(np.float32(sc["sum_logp"][b][i])) == bits(sums[b, r]), ("distinct", b, r)
    # beam search selected on the device
    nb, topk, Tb = 5, 2, 12
    tr = {}
    beam_search_device(model, voc, nb, B, Tb, topk, ex, prop1.repeat(B * nb, 1).to(DEV), device=DEV, grammar="smiles", trace=tr, tiles=True)
    assert tr["path"] == "tiles"
    hyp = [[[int(v) for v in x[1:]] for _, x in tr["hyps"][b].beams] for b in range(B)]
    assert all(len(h) >= 1 for h in hyp)
    sc = score(model, voc, hyp, B, ex, prop1, device=DEV, max_length=Tb, grammar="smiles", tiles=True)
    for b in range(B):
        for i, m in enumerate(hyp[b]):
            assert sc["length"][b][i] == len(m) + 1
            assert bits(np.float32(sc["sum_logp"][b][i])) == bits(np.float32(tr["hyp_sum_logp"][b][i])), ("beam", b, i)


def _teacher_forced_logits(model, ex, tokens, prop, per, **kw):
    """The logits of every step of `tokens` [rows, T] through a KVDecoder of the model (`kw`: fused / tiles): [rows, T - 1, V]."""
    from singa_amd.model.BeamSearch import KVDecoder, encode_pockets
    tf = model.model
    B = tokens.shape[0] // per
    num = 1 if tf.decoder.num_props else 0
    T = tokens.shape[1]
    with torch.no_grad():
        kv = KVDecoder(tf.decoder, tf.projection, *encode_pockets(tf, ex, B), per, T - 1 + num, len(smi_voc()), search_buffers=False, **kw)
        if num:
            kv.advance(kv.prop_input(prop.to(DEV).float()))
        tok = torch.as_tensor(tokens).to(DEV)
        out = [tf.projection(kv.advance(kv.token_input(tok[:, t].contiguous()))) for t in range(T - 1)]
    torch.cuda.synchronize()
    return torch.stack(out, 1).cpu(), kv


def test_logits_of_the_two_paths(setup, drawn):
    """The same tokens through k17 and through the tile kernels: every step's logits within 2e-5 row-wise."""
    z, model, sd, ex = setup
    tokens = drawn[0]
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(tokens.shape[0], 1)
    a, kva = _teacher_forced_logits(model, ex, tokens, prop, 32, fused=True)
    b, kvb = _teacher_forced_logits(model, ex, tokens, prop, 32, fused=True, tiles=True)
    assert kva.fused and not kva.tiles and kvb.tiles
    V = a.shape[-1]
    err = rowwise_err(b.reshape(-1, V), a.reshape(-1, V), "logits, tiles against k17 (row = decoder row * 40 + step)")
    assert err <= 2e-5, err


# ---------------------------------------------------------------------------------------------------------------- 8
def big_pocket(z, atoms=1100):
    """One synthetic pocket of `atoms` atoms: the golden's atom features and Laplacian rows drawn with replacement, positions
    on a jittered grid (no two atoms coincide), the kNN list drawn on the device."""
    from singa_amd.config import Config
    g = torch.Generator().manual_seed(8)
    pick = torch.randint(0, len(z["feat"]), (atoms,), generator=g)
    side = math.ceil(atoms ** (1 / 3))
    grid = torch.stack(torch.meshgrid(*[torch.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:atoms].float()
    ex = Config()
    ex.protein_element_batch = torch.zeros(atoms, dtype=torch.long, device=DEV)
    ex.protein_atom_feature = torch.as_tensor(z["feat"]).float()[pick].to(DEV)
    ex.protein_pos = (1.5 * grid + 0.2 * torch.rand(atoms, 3, generator=g)).to(DEV)
    ex.protein_atom_laplacian = torch.as_tensor(z["lap"]).float()[pick].to(DEV)
    return ex


def test_pocket_above_the_old_limit(setup):
    """1,100 atoms, 4 rows, 12 steps.  `sample_stream` and `sample_distinct` run (without `tiles` they raise), and `sample(tiles=
    True)` agrees with the library path, the only other one there: the library path's logits on the drawn tokens, the rule of
    tests/sampling_rule.py applied to them and to the uniforms the kernel read - no mismatch among the decisions that
    `sampling_rule.choose` does not flag as ambiguous at EPS."""
    from singa_amd.model.Sampling import sample, sample_distinct, sample_stream
    from tests.sampling_rule import EPS, check_against_oracle
    from tests.test_sampling_gpu import cpu_uniforms
    z, model, sd, _ = setup
    ex, voc = big_pocket(z), smi_voc()
    per, T = 4, 13
    prop = torch.as_tensor(z["prop"][:1]).float()
    u = cpu_uniforms(T, per, 8)
    for fn, args in ((sample_stream, (prop.to(DEV), 2)), (sample_distinct, (prop.repeat(per, 1).to(DEV),))):
        with pytest.raises(ValueError, match="1024 pocket atoms"):
            fn(model, voc, per, 1, T, ex, *args, device=DEV)
    with pytest.raises(ValueError, match="1024 pocket atoms"):
        sample(model, voc, per, 1, T, ex, prop.repeat(per, 1).to(DEV), device=DEV, uniforms=u, fused=True)
    tr = {}
    tokens = sample(model, voc, per, 1, T, ex, prop.repeat(per, 1).to(DEV), device=DEV, uniforms=u, trace=tr, tiles=True).cpu().numpy()
    assert tr["path"] == "tiles"
    st = {}
    streamed = sample_stream(model, voc, per, 1, T, ex, prop.to(DEV), 2, device=DEV, uniforms=u, trace=st, tiles=True).cpu().numpy()
    assert st["path"] == "tiles" and np.array_equal(streamed, tokens) and same(st["sum_logp"], tr["sum_logp"])
    dt = {}
    distinct = sample_distinct(model, voc, per, 1, T, ex, prop.repeat(per, 1).to(DEV), device=DEV, suppress=("&", "^"), seed=1, trace=dt,
                               tiles=True).cpu().numpy()
    assert dt["path"] == "tiles" and len({tuple(r) for r in distinct}) == per
    lib = {}
    sample(model, voc, per, 1, T, ex, prop.repeat(per, 1).to(DEV), device=DEV, uniforms=u, trace=lib, fused=False)
    assert lib["path"] == "library"                         # what `fused=None` falls to here without `tiles`
    logits, kv = _teacher_forced_logits(model, ex, tokens, prop.repeat(per, 1), per, fused=False)
    assert not kv.fused
    res = check_against_oracle(tokens, u.numpy(), logits.double().numpy(), voc.index("$"), 1.0, 0, 1.0, eps=EPS)
    dev = float(np.abs(tr["token_logp"].cpu().numpy().astype(np.float64) - res["logp"])[:, 1:].max())
    print(f"1100 atoms: {res['live']} live decisions, {res['ambiguous']} ambiguous, {len(res['bad'])} mismatches against the library "
          f"path's logits, max |tiles logp - library logp| {dev:.3e}")
    assert res["live"] >= per and not res["bad"], res["bad"]
