"""-m gpu: the row-tiled decoder step with its weight products on the bf16 matrix cores (k20b, include/singa_hip_dec_bf16.h) through
`ops.dec_layer_step(..., tiles=True, precision="bf16")` up to `sample(..., tiles=True, decoder_precision="bf16")`.  The reference
is one decoder layer in float64 with the kernels' rounding points: weights and each product's left operand rounded to bf16 (ties to
even), everything else float64.  An activation the kernel computed in f32 can round to the other neighbour than the float64 value
does, so the bounds are 4 x the largest error measured on an MI355X, capped at 2^-6 (profiles/dec_bf16/README.md)."""
import math

import pytest
import torch

from tests.test_dec_tiles_gpu import make_kv, same
from tests.test_decode_kernels_gpu import make_layer

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, P = 2, 256
# {inputs representable in bf16: largest max |error| / max |reference| of (outputs, appended key rows, appended value rows)} over the
# grid below; the appended rows are f32 sums of exact products.  The f32 tile path against plain float64: 6.8e-7 / 8.0e-7 / 8.2e-7.
MEASURED = {True: (1.344e-03, 2.793e-07, 2.661e-07), False: (1.086e-03, 2.793e-07, 2.661e-07)}
CAP = 2.0 ** -6
BOUND = {rep: tuple(min(4 * v, CAP) for v in MEASURED[rep]) for rep in MEASURED}


def r16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def ln(v, p):
    m = v.mean(-1, keepdim=True)
    return (v - m) / torch.sqrt(((v - m) ** 2).mean(-1, keepdim=True) + p["eps"]) * p["gamma"] + p["beta"]


def reference(w, x, kc, vc, rp, ck, cv, pad, beams, rnd, anc=None):
    """One layer step in float64 -> (out [R, 256], new key rows [R, 4, 32], new value rows [R, 4, 64]); `rnd`: the rounding of operands."""
    mm = lambda a, p, n: rnd(a) @ rnd(p[n])
    R = x.shape[0]
    a, c, f = w["self"], w["cross"], w["ffn"]
    qkv = mm(x, a, "wqkv_t") + a["bqkv"]
    q, kn, vn = qkv[:, :128].view(R, 4, 32), qkv[:, 128:256].view(R, 4, 32), qkv[:, 256:].view(R, 4, 64)
    ctx = torch.zeros(R, 256, dtype=torch.float64)
    for r in range(R):
        t = int(rp[r])
        if not 0 <= t < P:
            continue
        src = anc[:t, r].long() if anc is not None else torch.full((t,), r)
        K = torch.cat([kc[src, :, torch.arange(t)].permute(1, 0, 2), kn[r].unsqueeze(1)], 1)
        V = torch.cat([vc[src, :, torch.arange(t)].permute(1, 0, 2), vn[r].unsqueeze(1)], 1)
        att = torch.softmax(torch.einsum("hd,hpd->hp", q[r], K) / math.sqrt(32), -1)
        ctx[r] = torch.einsum("hp,hpd->hd", att, V).reshape(256)
    y = ln(mm(ctx, a, "wo_t") + a["bo"] + x, a)
    prot = torch.arange(R) // beams
    sc = torch.einsum("rhd,rhds->rhs", (mm(y, c, "wq_t") + c["bq"]).view(R, 4, 32), ck[prot]) / math.sqrt(32)
    ctx = torch.einsum("rhs,rhsd->rhd", torch.softmax(sc.masked_fill(pad.bool()[prot][:, None], -1e9), -1), cv[prot]).reshape(R, 256)
    z = ln(mm(ctx, c, "wo_t") + c["bo"] + y, c)
    return ln(mm(torch.relu(mm(z, f, "w1_t") + f["b1"]), f, "w2_t") + f["b2"] + z, f), kn, vn


def to64(w):
    return {b: {n: v.double().cpu() if torch.is_tensor(v) else v for n, v in p.items() if n != "bf16"} for b, p in w.items()}


def step(kv, x, kc, vc, rp, beams, mode, precision, anc=None):
    """One `ops.dec_layer_step` on copies of the caches -> (out, k_cache, v_cache) on the CPU."""
    from singa_amd import ops
    kd, vd = kc.to(DEV), vc.to(DEV)
    pos = rp.to(DEV) if mode == "per_row" else rp[:1].to(DEV)
    with torch.no_grad():
        out = ops.dec_layer_step(x.to(DEV), kv.w[0], kd, vd, pos, kv.cross_k[0], kv.cross_v[0], kv.pad_u8, beams, per_row=mode == "per_row",
                                 tiles=True, anc=None if anc is None else anc.to(DEV), precision=precision)
    torch.cuda.synchronize()
    return out.cpu(), kd.cpu(), vd.cpu()


def make_case(layer, beams, S, seed, rep):
    from singa_amd import ops
    R = B * beams
    g = torch.Generator().manual_seed(seed)
    enc, pad = torch.randn(B, S, 256, generator=g), torch.zeros(B, 1, S, dtype=torch.bool)
    pad[0, 0, max(1, 2 * S // 3):], pad[1] = True, True              # pocket 0 ragged, pocket 1 fully padded
    kv = make_kv(layer, enc, pad, beams, P)
    ops.dec_bf16_pack_layer(kv.w[0])
    x, kc, vc = torch.randn(R, 256, generator=g), torch.randn(R, 4, P, 32, generator=g), torch.randn(R, 4, P, 64, generator=g)
    if rep:
        x, kc, vc = r16(x), r16(kc), r16(vc)
        kv.cross_k[0].copy_(r16(kv.cross_k[0])), kv.cross_v[0].copy_(r16(kv.cross_v[0]))
    return kv, x, kc, vc, g


@pytest.fixture(scope="module")
def layer():
    return make_layer(2020)[0]


def rel(got, want):
    return float((got.double() - want).abs().max() / want.abs().max())


@pytest.mark.parametrize("mode", ["one", "per_row", "anc"])
@pytest.mark.parametrize("ip, pos", enumerate([0, 1, 63, 64, 255]))
@pytest.mark.parametrize("ib, beams", enumerate([1, 16, 17, 33]))
def test_layer_step_against_float64(layer, ib, beams, ip, pos, mode):
    """Tile shapes x cache positions x (one position | one per row, some outside [0, P) | an ancestry table); S cycles 1, 64, 65, 130."""
    S, R = (1, 64, 65, 130)[(ib + ip) % 4], B * beams
    for rep in (True, False):
        kv, x, kc, vc, g = make_case(layer, beams, S, 100 * ib + 10 * ip + len(mode), rep)
        rp, anc = torch.full((R,), pos), None
        if mode == "per_row":
            rp = torch.tensor([(pos, 0, 1, 63, 64, 255)[r % 6] for r in range(R)])
            rp[R - 1] = P
            if R > 2:
                rp[1] = -1
        if mode == "anc":
            anc = torch.stack([torch.cat([b * beams + torch.randperm(beams, generator=g) for b in range(B)]) for _ in range(P)]).int()
        live = (rp >= 0) & (rp < P)
        w64, ops64 = to64(kv.w[0]), [t.double() for t in (x, kc, vc)] + [rp] + [t.double().cpu() for t in (kv.cross_k[0], kv.cross_v[0])]
        pad = kv.pad_u8.cpu()
        want = reference(w64, *ops64, pad, beams, r16, anc)
        plain = reference(w64, *ops64, pad, beams, lambda t: t, anc)
        rows = torch.nonzero(live)[:, 0]
        new = lambda c: torch.stack([c[r, :, rp[r]] for r in rows])
        errs = {}
        for precision, ref in (("bf16", want), ("f32", plain)):
            out, kd, vd = step(kv, x, kc, vc, rp, beams, mode, precision, anc)
            errs[precision] = (rel(out[live], ref[0][live]), rel(new(kd), ref[1][live]), rel(new(vd), ref[2][live]))
            keep = torch.ones(R, P, dtype=torch.bool)
            keep[rows, rp[rows]] = False                               # everything but the appended rows keeps its bits
            assert same(kd.transpose(1, 2)[keep], kc.transpose(1, 2)[keep]) and same(vd.transpose(1, 2)[keep], vc.transpose(1, 2)[keep])
        print(f"dec_bf16 beams={beams} pos={pos} {mode} S={S} representable={rep}: bf16 out/k/v "
              + " ".join(f"{e:.3e}" for e in errs["bf16"]) + "  f32 " + " ".join(f"{e:.3e}" for e in errs["f32"]))
        assert all(e <= b for e, b in zip(errs["bf16"], BOUND[rep])), (rep, errs["bf16"], BOUND[rep])


def bare_kv(layer, wv, x_rows):
    """The layer with every weight matrix and bias zero, LayerNorm affine (1, 0), and `wv` as the last columns of q | k | v."""
    from singa_amd import ops
    kv, x, kc, vc, _ = make_case(layer, x_rows // B, 1, 5, True)
    for p in kv.w[0].values():
        for n, v in list(p.items()):
            if torch.is_tensor(v):                                     # (new tensors: some entries are views of the layer's parameters)
                p[n] = torch.ones_like(v) if n == "gamma" else torch.zeros_like(v)
    kv.w[0]["self"]["wqkv_t"][:, 512 - wv.shape[1]:] = wv.to(DEV)
    ops.dec_bf16_pack_layer(kv.w[0])
    return kv, kc, vc


def test_weights_are_rounded(layer):
    """Value projection (1 + 2^-10) I, representable x: the appended value row is x (the weight rounded to 1), not what f32 appends."""
    x = r16(torch.randn(B, 256, generator=torch.Generator().manual_seed(1)))
    kv, kc, vc = bare_kv(layer, (1 + 2.0 ** -10) * torch.eye(256), B)
    rp = torch.zeros(B, dtype=torch.int64)
    _, _, vb = step(kv, x, kc, vc, rp, 1, "one", "bf16")
    _, _, vf = step(kv, x, kc, vc, rp, 1, "one", "f32")
    assert float((vb[:, :, 0].reshape(B, 256) - x).abs().max()) <= 1e-6 * float(x.abs().max())
    assert not same(vb[:, :, 0], vf[:, :, 0])


def test_exact_projection_appends_the_f32_bits(layer):
    """Small integers in x and in the key / value projection: every product and sum is exact in both paths, the cache rows agree to the bit."""
    g = torch.Generator().manual_seed(2)
    R = B * 17
    x = torch.randint(-4, 5, (R, 256), generator=g).float()
    kv, kc, vc = bare_kv(layer, torch.randint(-2, 3, (256, 384), generator=g).float(), R)
    rp = torch.full((R,), 3)
    _, kb, vb = step(kv, x, kc, vc, rp, 17, "one", "bf16")
    _, kf, vf = step(kv, x, kc, vc, rp, 17, "one", "f32")
    assert same(kb, kf) and same(vb, vf) and not same(kb[:, :, 3], kc[:, :, 3])


@pytest.mark.parametrize("pos", [0, 70])
def test_a_row_does_not_depend_on_its_tile(layer, pos):
    """The same row alone in its pocket, as row 0 and as row 16 of a pocket of 17: the same bits in its outputs and cache rows."""
    got = []
    for beams, at in ((1, 0), (17, 0), (17, 16)):
        kv, x, kc, vc, _ = make_case(layer, beams, 65, 31, False)
        one = make_case(layer, 1, 65, 77, False)
        x[at], kc[at], vc[at] = one[1][0], one[2][0], one[3][0]
        out, kd, vd = step(kv, x, kc, vc, torch.full((B * beams,), pos), beams, "one", "bf16")
        got.append((out[at], kd[at], vd[at]))
    for other in got[1:]:
        assert all(same(a, b) for a, b in zip(got[0], other))


def test_entry_points_of_a_step(layer, monkeypatch):
    """Three launches per layer under either precision: with the switch off they are today's, with it on the three bf16 ones."""
    from singa_amd import _lib
    kv, x, kc, vc, _ = make_case(layer, 5, 65, 9, False)
    real, called = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            if name.startswith("singa_dec"):
                called.append(name)
            return getattr(real, name)
    monkeypatch.setattr(_lib, "lib", lambda: Counting())
    step(kv, x, kc, vc, torch.zeros(10, dtype=torch.int64), 5, "one", "f32")
    assert called == ["singa_dec_tile_self_attn", "singa_dec_tile_cross_attn", "singa_dec_tile_ffn"]
    del called[:]
    step(kv, x, kc, vc, torch.zeros(10, dtype=torch.int64), 5, "one", "bf16")
    assert called == ["singa_dec_bf16_tile_self_attn", "singa_dec_bf16_tile_cross_attn", "singa_dec_bf16_tile_ffn"]


@pytest.fixture(scope="module")
def pockets():
    from singa_amd import generate as GEN, graph as G
    from singa_amd.config import load_config
    from tests.test_beam_gpu import build_model
    model = build_model()[0]
    ex, n = GEN.pocket_example(model, load_config(lmax=2), G.collate([G.example_graph(i) for i in range(len(G.EXAMPLE_NAMES))]).to(DEV))
    return model, ex, n


def test_sample_parses_and_score_returns_its_bits(pockets):
    from singa_amd.model.Sampling import sample, score
    from tests.helpers import smi_voc
    from tests.test_dec_tiles_gpu import bits
    from tests.test_grammar_gpu import all_parse
    import numpy as np
    model, ex, n = pockets
    voc, per, T = smi_voc(), 8, 41
    prop, tr = torch.ones(n * per, 3, device=DEV), {}
    tokens = sample(model, voc, per, n, T, ex, prop, device=DEV, generator=torch.Generator(device=DEV).manual_seed(3), trace=tr,
                    grammar="smiles", suppress=("&", "^"), tiles=True, decoder_precision="bf16").cpu().numpy()
    assert tr["path"] == "tiles" and all(all_parse(tokens))
    lengths, sums = tr["lengths"].cpu().numpy(), tr["sum_logp"].cpu().numpy()
    mols = [[[int(t) for t in tokens[r, 1:lengths[r]]] for r in range(b * per, (b + 1) * per)] for b in range(n)]
    sc = score(model, voc, mols, n, ex, prop[:1].cpu(), device=DEV, max_length=T, grammar="smiles", tiles=True, decoder_precision="bf16")
    for b in range(n):
        for i in range(per):
            assert bits(np.float32(sc["sum_logp"][b][i])) == bits(sums[b * per + i]), (b, i)


def test_distinct_ancestry_equals_copy(pockets):
    from singa_amd.model.Sampling import sample_distinct
    from tests.helpers import smi_voc
    model, ex, n = pockets
    res = []
    for cache in ("copy", "ancestry"):
        tr = {}
        out = sample_distinct(model, smi_voc(), 20, n, 41, ex, torch.ones(n * 20, 3, device=DEV), device=DEV, suppress=("&", "^"), seed=4,
                              trace=tr, tiles=True, cache=cache, decoder_precision="bf16")
        res.append((out.cpu(), tr["sum_logp"].cpu(), tr["gumbel"].cpu()))
    assert all(same(a, b) for a, b in zip(*res))
