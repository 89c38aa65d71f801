"""-m gpu: sampled generation (singa_amd/model/Sampling.py, kernel `singa_sample_token`).

The kernel against the float64 restatement of its rule (tests/sampling_rule.py) on synthetic logits; `sample` end to end
against the CPU oracle DECISION BY DECISION: the returned sequences are fed, teacher-forced, through the oracle's encoder /
decoder, and for every live (row, position) the rule is applied to the oracle's logits and the very uniform the kernel
read - so a disagreement cannot cascade and nothing is statistical.  A decision is left out only when, in the oracle's
numbers alone, one of its thresholds is closer than EPS = 1e-5 (sampling_rule.choose); at most 2 % of a setting's live
decisions may be left out.

What EPS has to cover is the deviation of the device's fp32 log-probabilities from the oracle's; the test measures it over
all live decisions and asserts EPS >= 4 x the largest.  Measured on MI355X (profiles/sampling/accuracy.txt): 2.06e-6 (per
setting 1.68e-6, 1.91e-6, 1.66e-6, 2.06e-6, greedy 1.22e-6), i.e. 4 x = 8.2e-6 <= EPS; 0 - 0.54 % of the live decisions of a
setting are left out, none of the others disagrees.

The 41-token runs stay inside the first 64 cache positions; `test_sample_matches_oracle_beyond_64_tokens` repeats the check on
130-token sequences that cannot end ('&', '^', '$' suppressed).  Measured on MI355X: 1032 live decisions per setting, 1 and 3
of them ambiguous (0.10 % / 0.29 %), no mismatch, largest log-probability deviation 1.40e-6 / 2.16e-6 (4 x = 8.7e-6 <= EPS).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import golden, smi_voc
from tests.sampling_rule import EPS, check_against_oracle, choose, logp_bound, oracle_logits
from tests.test_beam_gpu import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(1.0, 0, 1.0), (0.8, 20, 1.0), (1.0, 0, 0.9), (0.7, 10, 0.95), (0.0, 0, 1.0)]
IDS = ["plain", "t0.8-k20", "p0.9", "t0.7-k10-p0.95", "greedy"]


def cpu_uniforms(T, rows, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.rand(rows, generator=g) for _ in range(T)])


def example_of(z, order=None):
    """The pockets of a beam golden as `sample` / `beam_search` take them; `order` lists the pockets in another order."""
    from singa_amd.config import Config
    batch, knn = torch.as_tensor(z["batch"]).long(), torch.as_tensor(z["knn"]).long()
    feat, pos, lap = (torch.as_tensor(z[k]).float() for k in ("feat", "pos", "lap"))
    if order is not None:
        perm = torch.cat([torch.nonzero(batch == b)[:, 0] for b in order])
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(len(perm))
        new_id = torch.empty(len(order), dtype=torch.long)
        new_id[torch.as_tensor(order)] = torch.arange(len(order))
        feat, pos, lap, batch = feat[perm], pos[perm], lap[perm], new_id[batch[perm]]
        knn = inv[knn]
        knn = knn[:, torch.sort(knn[0], stable=True)[1]]
    ex = Config()
    ex.protein_element_batch, ex.protein_atom_feature, ex.protein_pos = batch.to(DEV), feat.to(DEV), pos.to(DEV)
    ex.protein_atom_laplacian, ex.protein_knn = lap.to(DEV), knn.to(DEV)
    return ex


@pytest.fixture(scope="module")
def setup():
    z = golden("beam_b2_k6_eos.npz")
    model, sd, _ = build_model(z)                            # `sd` (the oracle's weights) carries the golden's gains too
    return z, model, sd


def run(z, model, per=32, T=41, setting=(1.0, 0, 1.0), seed=0, ex=None, u=None, **kw):
    from singa_amd.model.Sampling import sample
    B = len(z["names"])
    rows = B * per
    u = cpu_uniforms(T, rows, seed) if u is None else u
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(rows, 1)
    tr = {}
    tau, k, p = setting
    out = sample(model, smi_voc(), per, B, T, ex if ex is not None else example_of(z), prop.to(DEV), device=DEV,
                 temperature=tau, top_k=k, top_p=p, uniforms=u, trace=tr, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), u, prop, tr


def oracle_check(z, sd, tokens, u, prop, setting, order=None, suppress=()):
    B = len(z["names"])
    allowed = None
    if suppress:
        allowed = np.ones(len(smi_voc()), np.uint8)
        allowed[[smi_voc().index(s) for s in suppress]] = 0
    ex = example_of(z, order)
    c = lambda t: t.cpu()
    logits = oracle_logits(sd, smi_voc(), tokens, c(ex.protein_atom_feature), c(ex.protein_pos), c(ex.protein_element_batch),
                           c(ex.protein_atom_laplacian), c(ex.protein_knn), prop, B)
    return check_against_oracle(tokens, u.numpy(), logits, smi_voc().index("$"), *setting, allowed=allowed)


def well_formed(tokens, lengths=None):
    voc = smi_voc()
    sos, eos, pad = voc.index("&"), voc.index("$"), voc.index("^")
    T = tokens.shape[1]
    assert (tokens[:, 0] == sos).all()
    for r, row in enumerate(tokens):
        ends = np.flatnonzero(row == eos)
        n = int(ends[0]) if len(ends) else T - 1
        assert (row[n + 1:] == pad).all(), (r, row)             # '^' after '$', nothing else
        if lengths is not None:
            assert int(lengths[r]) == n, (r, int(lengths[r]), n)


# ---------------------------------------------------------------------------------------------------------------- 1
def kernel_call(zl, u, tau, top_k, top_p, allowed=None, finished=None, eos=1, pad=0):
    from singa_amd import ops
    R, V = zl.shape
    T = 3
    state = {"tokens": torch.full((R, T), -7, dtype=torch.int64, device=DEV), "next": torch.full((R,), -7, dtype=torch.int64, device=DEV),
             "finished": torch.zeros(R, dtype=torch.uint8, device=DEV), "length": torch.zeros(R, dtype=torch.int32, device=DEV),
             "sum_logp": torch.zeros(R, device=DEV), "live": torch.full((1,), R, dtype=torch.int32, device=DEV),
             "tok_logp": torch.zeros(R, T, device=DEV)}
    if finished is not None:
        state["finished"].copy_(torch.as_tensor(finished, dtype=torch.uint8))
    uu = torch.full((T, R), 0.5)
    uu[1] = torch.as_tensor(u)
    pos = torch.tensor([6], dtype=torch.int64, device=DEV)      # step 1 with pos_offset 5: reads uniforms[1], writes column 2
    al = None if allowed is None else torch.as_tensor(allowed, dtype=torch.uint8).to(DEV)
    ops.sample_token(torch.as_tensor(zl).to(DEV), uu.to(DEV), pos, 5, state, tau, top_k, top_p, eos, pad, al)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in state.items()}


@pytest.mark.parametrize("V", [2, 64, 116, 117, 1024])
def test_kernel_matches_the_rule(V):
    rs = np.random.RandomState(V)
    R = 96
    zl = rs.uniform(-10, 10, (R, V)).astype(np.float32)
    for r in range(0, 24):                                       # exact ties, also between the largest values
        i, j = rs.randint(V), rs.randint(V)
        zl[r, i] = zl[r, j] = zl[r].max() if r % 2 else zl[r, j]
    zl[24:30] = -10.0                                            # the mass sits on one token
    zl[np.arange(24, 30), rs.randint(V, size=6)] = 10.0
    zl[30] = 3.25                                                # all equal
    u = rs.rand(R).astype(np.float32)
    u[::7] = 0.0
    u[3::7] = np.float32(1) - np.float32(2.0 ** -24)
    u[5::7] = np.float32(1) - np.float32(2.0 ** -23)
    finished = np.zeros(R, np.uint8)
    finished[90:] = 1
    allowed = (rs.rand(V) < 0.7).astype(np.uint8)
    allowed[rs.randint(V)] = 1
    eos, pad = 1 % V, 0
    worst, cases, left_out = 0.0, 0, 0
    for tau in (0.0, 0.5, 1.0, 2.0):
        for top_k in (0, 1, 5, V, V + 3):
            for top_p in (1.0, 0.9, 0.5, 1e-6):
                for al in (None, allowed):
                    if al is not None and (top_k, top_p) not in ((0, 1.0), (5, 0.9)):
                        continue
                    got = kernel_call(zl, u, tau, top_k, top_p, al, finished, eos, pad)
                    assert (got["tokens"][:, :2] == -7).all()                     # only column t + 1 is written
                    for r in range(R):
                        if finished[r]:
                            assert got["tokens"][r, 2] == pad and got["next"][r] == pad and got["sum_logp"][r] == 0
                            assert got["length"][r] == 0
                            continue
                        tok, logp, amb = choose(zl[r], float(u[r]), tau, top_k, top_p, al, eps=EPS)
                        cases += 1
                        if amb:
                            left_out += 1
                            continue
                        g = int(got["tokens"][r, 2])
                        assert g == tok, (V, r, tau, top_k, top_p, al is not None, float(u[r]), g, tok)
                        assert got["next"][r] == tok and got["length"][r] == 1
                        assert got["finished"][r] == (1 if tok == eos else 0)
                        err = abs(float(got["sum_logp"][r]) - logp)
                        worst = max(worst, err)
                        assert err <= logp_bound(V, 10.0), (V, r, err)
                        assert got["tok_logp"][r, 2] == got["sum_logp"][r]
                    n_eos = int(((got["tokens"][:90, 2] == eos)).sum())
                    assert int(got["live"][0]) == R - n_eos
    print(f"V={V}: {cases} decisions, {left_out} ambiguous at eps {EPS}, worst |logp - float64| {worst:.3e} "
          f"(bound {logp_bound(V, 10.0):.3e})")
    # what is left out is a property of these inputs alone (float64 rule, no device number): u one or two fp32 steps below
    # 1 on rows whose mass is concentrated puts a cumulative F_i within EPS of u - about 3 % of the cases (2.7 - 3.4 %)
    assert left_out <= 0.05 * cases


# ------------------------------------------------------------------------------------------------------------ 2, 3
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_sample_matches_oracle_decision_by_decision(setup, setting):
    z, model, sd = setup
    tokens, u, prop, tr = run(z, model, setting=setting)
    lengths, sum_logp, tok_logp = (tr[k].cpu().numpy() for k in ("lengths", "sum_logp", "token_logp"))
    well_formed(tokens, lengths)
    res = oracle_check(z, sd, tokens, u, prop, setting)
    dev = float(np.abs(tok_logp.astype(np.float64) - res["logp"])[:, 1:].max())
    share = res["ambiguous"] / res["live"]
    print(f"setting {setting}: {res['live']} live decisions, {res['ambiguous']} ambiguous ({100 * share:.2f} %), "
          f"{len(res['bad'])} mismatches, max |device logp - oracle logp| {dev:.3e}, steps {tr['steps']}, path {tr['path']}")
    assert not res["bad"], res["bad"][:10]
    assert share <= 0.02, share
    assert EPS >= 4 * dev, dev
    assert np.array_equal(lengths, res["lengths"])
    want = res["logp"].sum(1)
    assert np.allclose(sum_logp, want, rtol=1e-4, atol=1e-5), float(np.abs(sum_logp - want).max())
    assert len(set(lengths.tolist())) > 1 or setting[0] == 0.0   # rows finish at different lengths


@pytest.mark.parametrize("setting", [(1.0, 0, 1.0), (0.8, 20, 0.9)], ids=["plain", "t0.8-k20-p0.9"])
def test_sample_matches_oracle_beyond_64_tokens(setup, setting):
    """The decision-by-decision check on sequences of 130 tokens: '&', '^' and '$' are suppressed, so no row finishes and
    every row decodes cache positions up to 129 - the second and third 64-lane pass of the self-attention's score loop,
    which the 41-token runs above never enter.  Same conditions as there; in addition at least 8 rows must have 60
    compared (live, unambiguous) decisions at token columns >= 64, so the test cannot pass by finishing early."""
    z, model, sd = setup
    sup = ("&", "^", "$")
    tokens, u, prop, tr = run(z, model, per=4, T=130, setting=setting, suppress=sup)
    lengths, tok_logp = (tr[k].cpu().numpy() for k in ("lengths", "token_logp"))
    voc = smi_voc()
    assert tokens.shape == (8, 130) and not np.isin(tokens[:, 1:], [voc.index(c) for c in sup]).any()
    assert tr["path"] == "k17" and tr["steps"] == 129 and (lengths == 129).all()
    res = oracle_check(z, sd, tokens, u, prop, setting, suppress=sup)
    dev = float(np.abs(tok_logp.astype(np.float64) - res["logp"])[:, 1:].max())
    dev_late = float(np.abs(tok_logp.astype(np.float64) - res["logp"])[:, 64:].max())
    share = res["ambiguous"] / res["live"]
    late = res["checked"][:, 64:].sum(1)
    print(f"setting {setting}, T = 130: {res['live']} live decisions, {res['ambiguous']} ambiguous ({100 * share:.2f} %), "
          f"{len(res['bad'])} mismatches, max |device logp - oracle logp| {dev:.3e} (columns >= 64: {dev_late:.3e}), "
          f"compared decisions at columns >= 64 per row {late.tolist()}")
    assert not res["bad"], res["bad"][:10]
    assert share <= 0.02, share
    assert EPS >= 4 * dev, dev
    assert np.array_equal(lengths, res["lengths"])
    assert int((late >= 60).sum()) >= 8, late.tolist()


# ---------------------------------------------------------------------------------------------------------------- 4
def test_determinism_and_independence(setup):
    z, model, sd = setup
    from singa_amd.model.Sampling import sample
    setting = (1.0, 0, 1.0)
    a, u, prop, tr = run(z, model)
    assert np.array_equal(a, run(z, model)[0])
    assert np.array_equal(a, run(z, model, graph=False)[0])
    assert tr["path"] == "k17"
    lib, _, _, tr_l = run(z, model, fused=False)
    assert tr_l["path"] == "library"
    if not np.array_equal(a, lib):                               # every disagreement must be an ambiguous decision, by the oracle
        for tk in (a, lib):
            assert not oracle_check(z, sd, tk, u, prop, setting)["bad"]
    assert not np.array_equal(a, run(z, model, seed=1)[0])
    for b in range(2):
        assert len({tuple(r) for r in a[32 * b:32 * b + 32]}) > 1
    # the generator draws the uniforms: same seed, same tokens; a device generator works too
    B, rows = 2, 64
    outs = []
    for _ in range(2):
        g = torch.Generator(device=DEV).manual_seed(5)
        outs.append(sample(model, smi_voc(), 32, B, 41, example_of(z), prop.to(DEV), device=DEV, generator=g).cpu().numpy())
    assert np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], a)
    # the pockets in the other order: the same rows in the other order
    swapped, _, _, _ = run(z, model, ex=example_of(z, [1, 0]), u=torch.cat([u[:, 32:], u[:, :32]], 1))
    back = np.concatenate([swapped[32:], swapped[:32]])
    if not np.array_equal(a, back):
        assert not oracle_check(z, sd, swapped, torch.cat([u[:, 32:], u[:, :32]], 1), prop, setting, order=[1, 0])["bad"]
        differ = np.flatnonzero((a != back).any(1))
        assert len(differ) <= 2, differ                          # fp32 noise at an ambiguous decision, not a mixed-up pocket


def test_suppress_and_memory_guard(setup):
    z, model, _ = setup
    voc = smi_voc()
    tokens, _, _, _ = run(z, model, suppress=("&", "^", "$"))
    assert not np.isin(tokens[:, 1:], [voc.index(c) for c in "&^$"]).any()
    with pytest.raises(ValueError, match="rows"):
        run(z, model, per=1_000_000, T=41, u=torch.zeros(1, 1))


# ---------------------------------------------------------------------------------------------------------------- 5
def test_beam_search_unchanged_after_sampling(setup):
    from singa_amd.config import Config
    from singa_amd.model.BeamSearch import beam_search
    z2, model2, _ = setup
    run(z2, model2)
    z = golden("beam_b1_k20.npz")
    model, _, _ = build_model(z)
    run(z, model, per=8, T=21)
    t = lambda k, dt=torch.float32: torch.as_tensor(z[k]).to(dt).to(DEV)
    ex = Config()
    ex.protein_element_batch, ex.protein_atom_feature, ex.protein_pos = t("batch", torch.long), t("feat"), t("pos")
    ex.protein_atom_laplacian, ex.protein_knn = t("lap"), t("knn", torch.long)
    tr = {}
    out = beam_search(model, smi_voc(), int(z["num_beams"]), len(z["names"]), int(z["max_length"]), int(z["topk"]), ex,
                      t("prop"), device=DEV, trace=tr)
    assert np.array_equal(tr["last_beams"], z["last_beams"])
    assert out.shape == z["decoded"].shape and np.array_equal(out.cpu().numpy(), z["decoded"])


# ---------------------------------------------------------------------------------------------------------------- 6
def test_scale_2048_rows():
    z = golden("beam_b1_k20.npz")
    model, _, _ = build_model(z)
    T = 201
    u = cpu_uniforms(T, 2048, seed=3)
    big, _, _, tr = run(z, model, per=2048, T=T, u=u, fused=True)
    assert big.shape == (2048, T) and tr["path"] == "k17"
    well_formed(big, tr["lengths"].cpu().numpy())
    small, _, _, _ = run(z, model, per=20, T=T, u=u[:, :20].contiguous(), fused=True)
    assert np.array_equal(big[:20], small)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_gen_entry_point():
    def gen():
        cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "golden", "--mode", "sample", "--num-samples", "8",
               "--seed", "1"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
        out = r.stdout.decode().splitlines()
        assert any("random initial weights" in l for l in out if l.startswith("#"))
        return [l for l in out if not l.startswith("#")]
    a, b = gen(), gen()
    assert a == b
    names = {}
    for line in a:
        name, smiles, length, logp = line.split("\t")
        assert 0 < int(length) <= 200 and float(logp) <= 0.0
        assert not set(smiles) & set("&$")
        names[name] = names.get(name, 0) + 1
    assert len(names) == 3 and set(names.values()) == {8}
