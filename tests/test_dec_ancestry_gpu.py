"""-m gpu: ancestry-indexed key / value caches (include/singa_hip_ancestry.h).  1: one decoder layer through the table, k17 and
tiles, against the float64 layer reference and bound of tests/test_dec_tiles_gpu.py / test_decode_kernels_gpu.py and against the
plain entry point on the gathered cache, bit for bit; slot s holds the float32-rounded keys / values of a random sequence x[s],
so the table describes the sequence x[anc[p][r], p].  2: the table update against numpy, twice in a row.  3: `sample_distinct`
and `beam_search_device`, cache="ancestry" against "copy", bit for bit.  The refusals: tests/test_dec_ancestry_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from tests.helpers import golden, rowwise_err, smi_voc
from tests.test_dec_tiles_gpu import inputs, make_kv, reference
from tests.test_dec_tiles_gpu import stream_pool_left_as_found  # noqa: F401  (autouse: the captured generations below take streams)
from tests.test_decode_kernels_gpu import TOL, make_layer

pytestmark = pytest.mark.gpu
DEV = "cuda"
P1, POSITIONS = 130, (0, 1, 63, 64, 65, 129)


@functools.lru_cache(maxsize=None)
def layer_case(B, beams):
    """Layer, inputs and every slot's float64 keys / values, once per shape."""
    layer, sd = make_layer(71)
    x, enc, pad = inputs(B, beams, P1, 65, 7100 + beams)
    _, wk, wv = reference(sd, x.double(), enc, pad, beams)
    return layer, sd, x, enc, pad, wk.float().contiguous(), wv.float().contiguous()


def table(kind, B, beams, P, seed):
    """anc [P, R] int32: per position a random slot of the row's pocket, the pocket's last slot for all its rows, or the row."""
    base = (torch.arange(B) * beams).repeat_interleave(beams)
    off = {"random": torch.randint(0, beams, (P, B * beams), generator=torch.Generator().manual_seed(seed)),
           "one": torch.full((P, B * beams), beams - 1), "identity": torch.arange(beams).repeat(B).expand(P, -1)}[kind]
    return (base + off).to(torch.int32).contiguous()


@pytest.mark.parametrize("kind", ["random", "one", "identity"])
@pytest.mark.parametrize("B,beams", [(1, 1), (2, 3), (2, 17)])
@pytest.mark.parametrize("tiles", [False, True], ids=["k17", "tiles"])
def test_self_attention_through_the_table(tiles, B, beams, kind):
    from singa_amd import ops
    layer, sd, x, enc, pad, kc, vc = layer_case(B, beams)
    R = B * beams
    kv = make_kv(layer, enc, pad, beams, P1, tiles=tiles)
    anc = table(kind, B, beams, P1, 100 * beams + len(kind))
    at, pp = anc.long().t(), torch.arange(P1)                          # at[r, p] = anc[p][r]
    xg_all = x[at, pp]                                                 # the sequence the table gives row r
    hh = torch.arange(4)[None, :, None]
    kg, vg = kc[at[:, None, :], hh, pp[None, None, :]].contiguous(), vc[at[:, None, :], hh, pp[None, None, :]].contiguous()
    xq = torch.randn(R, 256, generator=torch.Generator().manual_seed(5))    # the new position's input

    def step(k, v, pos, table_):
        with torch.no_grad():
            out = ops.dec_layer_step(xq.to(DEV), kv.w[0], k, v, torch.tensor([pos], device=DEV), kv.cross_k[0], kv.cross_v[0],
                                     kv.pad_u8, beams, tiles=tiles, anc=table_)
        return out.cpu()

    for pos in POSITIONS:
        k1, v1, k2, v2 = (t.clone().to(DEV) for t in (kc, vc, kg, vg))
        got, plain = step(k1, v1, pos, anc.to(DEV)), step(k2, v2, pos, None)
        xg = torch.cat([xg_all[:, :pos], xq[:, None]], 1).double()
        want, wk, wv = reference(sd, xg, enc, pad, beams)
        tag = f"{'tiles' if tiles else 'k17'} {B}x{beams} {kind} pos {pos}"
        errs = (rowwise_err(got, want[:, pos], tag + " output"), rowwise_err(k1[:, :, pos].cpu().reshape(R, -1), wk[:, :, pos].reshape(R, -1), tag + " key"),
                rowwise_err(v1[:, :, pos].cpu().reshape(R, -1), wv[:, :, pos].reshape(R, -1), tag + " value"))
        assert max(errs) <= TOL, (tag, errs)
        assert torch.equal(got, plain), tag
        for new, old, ref in ((k1.cpu(), kc, k2.cpu()), (v1.cpu(), vc, v2.cpu())):
            assert torch.equal(new[:, :, pos], ref[:, :, pos]) and not torch.equal(new[:, :, pos], old[:, :, pos]), tag
            new[:, :, pos] = old[:, :, pos]
            assert torch.equal(new, old), tag                          # nothing but (row, pos) was written


@pytest.mark.parametrize("n", [0, 1, 39, 40])
@pytest.mark.parametrize("k", [1, 5, 70])
def test_table_update_against_numpy(k, n):
    """`n` = *pos behind the step's increment: t = n - 1 was just appended (0: nothing to do; 40 = P: the table's last row)."""
    from singa_amd import ops
    B, P = 2, 40
    R = B * k
    rng = np.random.default_rng(10 * k + n)
    base = np.repeat(np.arange(B) * k, k)
    anc = (base + rng.integers(0, k, (P, R))).astype(np.int32)
    dev_anc, pos = torch.as_tensor(anc).to(DEV), torch.tensor([n], device=DEV)
    for launch in range(2):
        src = base + rng.integers(0, k, R)
        if k > 1:
            src[0], src[1], src[2 % k], src[k - 1] = 1, 1, 1, k - 1    # slot 1: parent of a lower slot and of several; a dead slot
        if launch == 1:
            src[R - 1] = 0 if B > 1 else -1                            # a parent outside the row's pocket leaves the row alone
        want = anc.copy()
        ok = (src >= base) & (src < base + k)
        if n >= 1:
            want[:n - 1, ok] = anc[:n - 1, src[ok]]
            want[n - 1, ok] = src[ok]
        ops.anc_follow(dev_anc, torch.as_tensor(src).to(DEV), pos, k)
        anc = want
        assert np.array_equal(dev_anc.cpu().numpy(), want), (k, n, launch)


B2, K2, T2 = 2, 20, 40


@pytest.fixture(scope="module")
def setup():
    from tests.test_beam_gpu import build_model
    from tests.test_sampling_gpu import example_of
    z = golden("beam_b2_k6_eos.npz")
    return build_model(z)[0], example_of(z), [str(v) for v in smi_voc()], torch.as_tensor(z["prop"][:1]).float().repeat(B2 * K2, 1).to(DEV)


def both(fn, keys):
    """fn(cache=..., trace=...) with "copy" and with "ancestry": the same tokens, steps and bits in trace[keys] -> the traces."""
    ca, an = {}, {}
    assert torch.equal(fn(cache="copy", trace=ca).cpu(), fn(cache="ancestry", trace=an).cpu())
    for key in keys:
        assert torch.equal(torch.as_tensor(ca[key]).cpu(), torch.as_tensor(an[key]).cpu()), key
    assert ca["steps"] == an["steps"]
    return ca, an


@pytest.mark.parametrize("tiles,grammar,prefix,graph", [
    (False, None, None, True), (True, None, None, True), (False, "smiles", None, True), (True, "smiles", None, True),
    (True, "smiles", "c1cc", True), (False, None, None, False)])
def test_sample_distinct_equals_the_copy_path(setup, tiles, grammar, prefix, graph):
    from singa_amd import smiles
    from singa_amd.model.Sampling import sample_distinct
    model, ex, voc, prop = setup
    forced = None if prefix is None else smiles.encode([prefix] * B2, voc, T2)
    tr, _ = both(functools.partial(sample_distinct, model, voc, K2, B2, T2, ex, prop, device=DEV, suppress=("&", "^"), grammar=grammar,
                                   seed=9, forced=forced, tiles=tiles, graph=graph),
                 ("gumbel", "prop_logp", "sum_logp", "token_logp", "lengths", "valid"))
    assert tr["steps"] >= 8 and int(tr["valid"].sum()) > B2            # the rows were re-ranked for a while


@pytest.mark.parametrize("grammar", [None, "smiles"])
def test_beam_search_device_equals_the_copy_path(setup, grammar):
    from singa_amd.model.BeamSearch import beam_search_device
    model, ex, voc, prop = setup
    a, b = both(functools.partial(beam_search_device, model, voc, K2, B2, T2, 3, ex, prop, device=DEV, grammar=grammar), ("valid",))
    for pa, pb in zip(a["hyps"], b["hyps"]):
        assert [s for s, _ in pa.beams] == [s for s, _ in pb.beams]
        assert all(np.array_equal(x, y) for (_, x), (_, y) in zip(pa.beams, pb.beams))
    assert all(np.array_equal(np.float32(x), np.float32(y)) for x, y in zip(a["hyp_sum_logp"], b["hyp_sum_logp"]))
