"""-m gpu: forced tokens in sampling (`singa_sample_token_forced`, `sample(..., forced=...)`, `score`, `gen.py --prefix` /
`--mode score`).

One step of the kernel in every regime against the unforced entry points (free rows: bit for bit) and against numpy / float64
(forced rows, rank), without and under the grammar; then `sample` with forced prefixes against the CPU oracle decision by
decision (tests/forced_rule.py: a forced column is no decision, its log-probability is compared like any other), the round
trip draw -> score, `score` against the oracle, forced columns past 64 cache positions, grammar and prefix together, and the
command line.  Tolerances are those of tests/test_sampling_gpu.py: EPS / 4 for a device log-probability against the oracle's
(2.06e-6 was measured there), the fp32 bound of a V-term log-sum-exp against float64 on synthetic logits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import grammar_rule as G
from tests.forced_rule import PREFIXES, PREFIX_TOKENS, check_forced_against_oracle, is_forced, rank_of
from tests.helpers import golden, smi_voc
from tests.sampling_rule import EPS, logp_bound, oracle_logits
from tests.test_beam_gpu import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("tokens", "next", "finished", "length", "sum_logp", "tok_logp")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def new_state(R, T, finished, states=None):
    """canaries everywhere a step must not write"""
    st = {"tokens": torch.full((R, T), -7, dtype=torch.int64, device=DEV), "next": torch.full((R,), -7, dtype=torch.int64, device=DEV),
          "finished": torch.as_tensor(finished, dtype=torch.uint8).to(DEV), "length": torch.zeros(R, dtype=torch.int32, device=DEV),
          "sum_logp": torch.zeros(R, device=DEV), "live": torch.full((1,), R - int(np.sum(finished)), dtype=torch.int32, device=DEV),
          "tok_logp": torch.full((R, T), 9.0, device=DEV)}
    if states is not None:
        st["grammar"] = torch.as_tensor(np.asarray(states, np.int32)).to(DEV)
        st["allowed_logp"] = torch.full((R, T), 9.0, device=DEV)
    return st


def host(st):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in st.items()}


def float64_logp(z, tok):
    z = z.astype(np.float64)
    return z[tok] - (z.max() + np.log(np.exp(z - z.max()).sum()))


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("V", [2, 64, 116, 117, 1024])
def test_one_step_every_regime(V):
    from singa_amd import ops
    rs = np.random.RandomState(V)
    R, T = 96, 3
    zl = rs.uniform(-10, 10, (R, V)).astype(np.float32)             # as tests/test_sampling_gpu.py::test_kernel_matches_the_rule
    for r in range(0, 24):                                          # exact ties, also between the largest values
        i, j = rs.randint(V), rs.randint(V)
        zl[r, i] = zl[r, j] = zl[r].max() if r % 2 else zl[r, j]
    zl[24:30] = -10.0                                               # the mass sits on one token
    zl[np.arange(24, 30), rs.randint(V, size=6)] = 10.0
    zl[30] = 3.25                                                   # all equal
    u = rs.rand(R).astype(np.float32)
    u[::7] = 0.0
    finished = np.zeros(R, np.uint8)
    finished[90:] = 1
    allowed = (rs.rand(V) < 0.7).astype(np.uint8)
    allowed[rs.randint(V)] = 1
    eos, pad = 1 % V, 0
    # column 2 is the one step 1 reads: free on a third of the rows, a random token on a third (among them a token `allowed`
    # masks out, eos, and V and V + 5, which are free), the arg-max or the arg-min on the rest; columns 0 and 1 hold tokens
    # that nothing may read
    forced = rs.randint(0, V, size=(R, T)).astype(np.int64)
    forced[0::3, 2] = -1
    forced[1::3, 2] = rs.randint(0, V, size=len(forced[1::3]))
    forced[2::6, 2] = zl[2::6].argmax(1)
    forced[5::6, 2] = zl[5::6].argmin(1)
    masked = np.flatnonzero(allowed == 0)
    assert len(masked) or V == 2
    forced[1, 2], forced[4, 2], forced[7, 2], forced[10, 2] = (masked[0] if len(masked) else 0), eos, V, V + 5
    forced[25, 2] = eos                                             # a forced token of probability ~ e^-20 ...
    forced[28, 2] = zl[28].argmax()                                 # ... and one of probability ~ 1
    given = is_forced(forced[:, 2], V)
    assert given[[1, 4]].all() and not given[[0, 3, 7, 10]].any()
    zl_d, f_d = torch.as_tensor(zl).to(DEV), torch.as_tensor(forced).to(DEV)
    uu = torch.full((T, R), 0.5)
    uu[1] = torch.as_tensor(u)
    uu = uu.to(DEV)
    pos = torch.tensor([6], dtype=torch.int64, device=DEV)          # step 1 with pos_offset 5: reads uniforms[1], writes column 2
    worst = 0.0
    for tau in (0.0, 1.0):
        for top_k, top_p in ((0, 1.0), (5, 0.9)):
            for al in (None, allowed):
                al_d = None if al is None else torch.as_tensor(al).to(DEV)
                ref = new_state(R, T, finished)
                ops.sample_token(zl_d, uu, pos, 5, ref, tau, top_k, top_p, eos, pad, al_d)
                ref = host(ref)
                st = new_state(R, T, finished)
                st["rank"] = torch.full((R, T), -99, dtype=torch.int32, device=DEV)
                ops.sample_token_forced(zl_d, uu, pos, 5, st, f_d, None, tau, top_k, top_p, eos, pad, al_d)
                got = host(st)
                ctx = (V, tau, top_k, top_p, al is not None)
                assert torch.equal(f_d.cpu(), torch.as_tensor(forced)), ctx                       # forced is only read
                assert (got["tokens"][:, :2] == -7).all() and (bits(got["tok_logp"][:, :2]) == bits(np.float32(9.0))).all(), ctx
                assert (got["rank"][:, :2] == -99).all(), ctx                                     # only column t + 1 is written
                free = ~given | (finished == 1)
                for k in KEYS:                                      # free and finished rows: the unforced entry point, bit for bit
                    assert np.array_equal(bits(got[k][free]), bits(ref[k][free])), (ctx, k)
                n_eos = 0
                for r in range(R):
                    if finished[r]:
                        assert got["tokens"][r, 2] == pad and got["rank"][r, 2] == 0 and got["length"][r] == 0, (ctx, r)
                        continue
                    tok = int(got["tokens"][r, 2])
                    n_eos += tok == eos
                    assert got["rank"][r, 2] == rank_of(zl[r], tok), (ctx, r, tok)                # exact: the same fp32 numbers
                    if not given[r]:
                        continue
                    assert tok == forced[r, 2] and got["next"][r] == tok and got["length"][r] == 1, (ctx, r)
                    assert got["finished"][r] == (tok == eos), (ctx, r)
                    err = abs(float(got["tok_logp"][r, 2]) - float64_logp(zl[r], tok))
                    worst = max(worst, err)
                    assert err <= logp_bound(V, 10.0), (ctx, r, err)
                    assert bits(got["sum_logp"])[r] == bits(got["tok_logp"])[r, 2], (ctx, r)
                assert int(got["live"][0]) == 90 - n_eos, ctx
                assert n_eos >= 2
    print(f"V={V}: worst |forced logp - float64| {worst:.3e} (bound {logp_bound(V, 10.0):.3e})")


# ---------------------------------------------------------------------------------------------------------------- 2
def test_one_step_under_the_grammar():
    """The grid of states of tests/test_grammar_gpu.py::test_one_step_matches_the_rule; every third row free, every third
    forced to a random token of any class, every third to the classes in turn - allowed by the rule or not."""
    from singa_amd import ops, smiles
    voc = smi_voc()
    cls, eos, pad = smiles.classify(voc), voc.index("$"), voc.index("^")
    V = len(cls)
    states = [G.pack(prev, depth, ring, here) for prev in range(1, 9) for depth in (0, 1, 2, 63)
              for ring in (0, 1, 0b100100, 0x1ff) for here in (0, ring & 0b101, ring)]
    assert len(states) == 384
    R = 384 + 16
    states = np.array(states + states[5:21], np.int32)
    finished = np.zeros(R, np.uint8)
    finished[384:] = 1
    rs = np.random.RandomState(7)
    zl = rs.uniform(-10, 10, (R, V)).astype(np.float32)
    u = rs.rand(R).astype(np.float32)
    glob = (rs.rand(V) < 0.8).astype(np.uint8)
    glob[eos] = 1
    one_of = [int(np.flatnonzero((cls & 15) == c)[0]) for c in range(8)] + [voc.index("3"), voc.index("9")]
    cls_d, zl_d = torch.as_tensor(cls).to(DEV), torch.as_tensor(zl).to(DEV)
    pos = torch.tensor([6], dtype=torch.int64, device=DEV)
    refused = inside = empty_free = 0
    for rem in (0, 2, 12):
        T = rem + 3
        forced = np.full((R, T), -1, np.int64)
        forced[1::3, 2] = rs.randint(0, V, size=len(forced[1::3]))
        forced[2::3, 2] = [one_of[(i + rem) % len(one_of)] for i in range(len(forced[2::3]))]
        given = is_forced(forced[:, 2], V)
        f_d = torch.as_tensor(forced).to(DEV)
        uu = torch.full((T, R), 0.5)
        uu[1] = torch.as_tensor(u)
        uu = uu.to(DEV)
        gram = G.allows(states[:, None], cls[None, :], rem)
        for al in (None, glob):
            masks = gram if al is None else gram & al.astype(bool)[None, :]
            al_d = None if al is None else torch.as_tensor(al).to(DEV)
            for setting in ((1.0, 0, 1.0), (0.7, 10, 0.95)):
                ref = new_state(R, T, finished, states)
                ops.sample_token_grammar(zl_d, uu, pos, 5, ref, cls_d, *setting, eos, pad, al_d)
                ref = host(ref)
                st = new_state(R, T, finished, states)
                st["rank"] = torch.full((R, T), -99, dtype=torch.int32, device=DEV)
                ops.sample_token_forced(zl_d, uu, pos, 5, st, f_d, cls_d, *setting, eos, pad, al_d)
                got = host(st)
                ctx = (rem, al is not None, setting)
                cols = [0, 1] + list(range(3, T))
                assert (got["tokens"][:, cols] == -7).all() and (got["rank"][:, cols] == -99).all(), ctx
                assert (got["tok_logp"][:, cols] == 9.0).all() and (got["allowed_logp"][:, cols] == 9.0).all(), ctx
                free = ~given | (finished == 1)
                for k in KEYS + ("grammar", "allowed_logp"):
                    assert np.array_equal(bits(got[k][free]), bits(ref[k][free])), (ctx, k)
                # the mass on the effective mask does not depend on what is forced
                assert np.array_equal(bits(got["allowed_logp"][:, 2]), bits(ref["allowed_logp"][:, 2])), ctx
                n_eos = 0
                for r in range(R):
                    if finished[r]:
                        assert got["rank"][r, 2] == 0 and got["grammar"][r] == states[r], (ctx, r)
                        continue
                    tok = int(got["tokens"][r, 2])
                    if not given[r] and not masks[r].any():         # a free row with an empty mask: `pad`, and no rank
                        assert tok == pad and got["rank"][r, 2] == -1 and got["finished"][r] == 0, (ctx, r)
                        empty_free += 1
                        continue
                    n_eos += tok == eos
                    assert got["rank"][r, 2] == rank_of(zl[r], tok), (ctx, r, tok)
                    if not given[r]:
                        continue
                    assert tok == forced[r, 2] and got["next"][r] == tok and got["length"][r] == 1, (ctx, r)
                    assert got["finished"][r] == (tok == eos), (ctx, r)
                    assert got["grammar"][r] == int(G.transition(states[r], int(cls[tok]))), (ctx, r, tok)   # allowed or not
                    refused += not masks[r][tok]
                    inside += bool(masks[r][tok])
                    assert abs(float(got["tok_logp"][r, 2]) - float64_logp(zl[r], tok)) <= logp_bound(V, 10.0), (ctx, r)
                assert int(got["live"][0]) == 384 - n_eos, ctx
    print(f"forced tokens inside the mask {inside}, outside {refused}; free rows with an empty mask {empty_free}")
    assert refused > 300 and inside > 300 and empty_free > 0


# ------------------------------------------------------------------------------------------------------- 3 .. 7: `sample`
@pytest.fixture(scope="module")
def setup():
    z = golden("beam_b2_k6_eos.npz")
    model, sd, _ = build_model(z)
    return z, model, sd


def oracle_of(z, sd, tokens, prop):
    from tests.test_sampling_gpu import example_of
    ex = example_of(z)
    c = lambda t: t.cpu()
    return oracle_logits(sd, smi_voc(), tokens, c(ex.protein_atom_feature), c(ex.protein_pos), c(ex.protein_element_batch),
                         c(ex.protein_atom_laplacian), c(ex.protein_knn), prop, len(z["names"]))


@pytest.mark.parametrize("setting", [(1.0, 0, 1.0), (0.7, 10, 0.95)], ids=["plain", "t0.7-k10-p0.95"])
def test_prefix_then_free_matches_oracle(setup, setting):
    """16 rows per pocket, T = 41, prefixes of 0, 1, 5 and 12 tokens cycling over the rows.  The 0.02 cap on the ambiguous
    share is a condition on the inputs: the same rows drawn on the CPU from the oracle's own logits with `choose` (seed 0,
    these prefixes) have 808 / 549 free decisions in the two settings, none of them ambiguous at EPS (share 0.00 %)."""
    from singa_amd import smiles
    from tests.test_sampling_gpu import run
    z, model, sd = setup
    voc = smi_voc()
    rows, T = 32, 41
    forced = smiles.encode([PREFIXES[r % 4] for r in range(rows)], voc, T)
    assert [int(is_forced(forced[r, 1:], len(voc)).sum()) for r in range(4)] == list(PREFIX_TOKENS)
    tokens, u, prop, tr = run(z, model, per=16, T=T, setting=setting, forced=forced)
    lengths, tok_logp, rank = (tr[k].cpu().numpy() for k in ("lengths", "token_logp", "rank"))
    given = is_forced(forced, len(voc))
    assert np.array_equal(tokens[given], forced[given])                                     # forced columns equal the prefix
    logits = oracle_of(z, sd, tokens, prop)
    res = check_forced_against_oracle(tokens, forced, u.numpy(), logits, voc.index("$"), *setting)
    live = res["logp"] != 0
    dev = float(np.abs(tok_logp.astype(np.float64) - res["logp"])[:, 1:].max())
    dev_forced = float(np.abs(tok_logp.astype(np.float64) - res["logp"])[res["forced_live"]].max())
    share = res["ambiguous"] / res["free"]
    print(f"setting {setting}: {res['free']} free decisions, {res['ambiguous']} ambiguous ({100 * share:.2f} %), "
          f"{len(res['bad'])} mismatches, {int(res['forced_live'].sum())} forced columns, max |device logp - oracle logp| {dev:.3e} "
          f"(forced columns {dev_forced:.3e})")
    assert not res["forced_bad"] and not res["bad"], (res["forced_bad"][:10], res["bad"][:10])
    assert share <= 0.02, share
    assert dev <= EPS / 4, dev
    assert np.array_equal(lengths, res["lengths"])
    assert int(res["forced_live"].sum()) == 8 * sum(PREFIX_TOKENS)
    for r, t in zip(*np.nonzero(live)):                             # rank against the oracle's numbers, where the gap is clear
        zz = logits[r, t - 1]
        gap = np.abs(zz - zz[tokens[r, t]])
        gap[tokens[r, t]] = np.inf
        if gap.min() > EPS:
            assert rank[r, t] == rank_of(zz, tokens[r, t]), (r, t)


# ---------------------------------------------------------------------------------------------------------------- 4
def test_round_trip_draw_then_score(setup):
    from tests.test_sampling_gpu import run
    z, model, sd = setup
    voc = smi_voc()
    eos = voc.index("$")
    tokens, u, prop, tr = run(z, model)                              # 32 rows per pocket, k17 path, graph
    assert tr["path"] == "k17"
    drawn = {k: tr[k].cpu().numpy() for k in ("lengths", "token_logp", "sum_logp")}
    forced = tokens.copy()
    for r, n in enumerate(drawn["lengths"]):
        forced[r, 1 + n:] = -1                                      # nothing behind the row's '$'
    assert (drawn["lengths"] < 40).any() and ((forced == eos).sum(1) <= 1).all()
    for kw in (dict(), dict(graph=False)):
        again, _, _, tr2 = run(z, model, seed=1, forced=forced, **kw)                        # other uniforms: nothing is drawn
        assert np.array_equal(again, tokens), kw
        assert np.array_equal(tr2["lengths"].cpu().numpy(), drawn["lengths"]), kw
        for k in ("token_logp", "sum_logp"):
            assert np.array_equal(bits(tr2[k].cpu().numpy()), bits(drawn[k])), (kw, k)
    lib, _, _, tr3 = run(z, model, seed=1, forced=forced, fused=False)
    assert tr3["path"] == "library" and np.array_equal(lib, tokens)
    dev = float(np.abs(tr3["token_logp"].cpu().numpy().astype(np.float64) - drawn["token_logp"]).max())
    print(f"library path against k17: max |token_logp difference| {dev:.3e}")
    assert dev <= EPS / 4, dev


# ---------------------------------------------------------------------------------------------------------------- 5
MOLECULES = (["CCO", "CC(=O)Nc1ccc(O)cc1", "C[C@H](N)C(=O)O"],
             ["c1ccccc1", "CN1CCC[C@H]1c1cccnc1", "O=C(O)c1ccccc1OC(C)=O", "C1CC1", "N#Cc1ccccc1", "ClCCBr", "C[N+](C)(C)CC([O-])=O"])


def test_score_against_oracle(setup):
    from singa_amd import smiles
    from singa_amd.model.Sampling import score
    from tests.test_sampling_gpu import example_of
    z, model, sd = setup
    voc = smi_voc()
    pad = voc.index("^")
    prop1 = torch.as_tensor(z["prop"][:1]).float()
    res = score(model, voc, MOLECULES, 2, example_of(z), prop1, device=DEV)
    assert [len(x) for x in res["sum_logp"]] == [3, 7] == [len(x) for x in res["rank"]]       # filler rows are absent
    assert "allowed_logp" not in res
    per = 7
    T = max(len(smiles.tokenize(m, voc)) for ms in MOLECULES for m in ms) + 2
    items = [m for ms in MOLECULES for m in list(ms) + [""] * (per - len(ms))]
    tokens = smiles.encode(items, voc, T, end=True)
    tokens[tokens < 0] = pad
    logits = oracle_of(z, sd, tokens, prop1.repeat(2 * per, 1))
    clear = top1 = 0
    for b, ms in enumerate(MOLECULES):
        for i, m in enumerate(ms):
            r, n = b * per + i, len(smiles.tokenize(m, voc)) + 1
            assert res["length"][b][i] == n and len(res["token_logp"][b][i]) == n == len(res["rank"][b][i])
            want = np.array([logits[r, t, tokens[r, t + 1]] - (logits[r, t].max() + np.log(np.exp(logits[r, t] - logits[r, t].max()).sum()))
                             for t in range(n)])
            assert np.abs(res["token_logp"][b][i] - want).max() <= EPS / 4, (b, i)
            assert np.allclose(res["sum_logp"][b][i], want.sum(), rtol=1e-4, atol=1e-5), (b, i, res["sum_logp"][b][i], want.sum())
            for t in range(n):
                zz, tok = logits[r, t], tokens[r, t + 1]
                others = np.delete(zz, tok).max()
                if abs(zz[tok] - others) > EPS:                     # rank == 0 exactly where the token is the oracle's arg-max
                    clear += 1
                    top1 += zz[tok] > others
                    assert (res["rank"][b][i][t] == 0) == (zz[tok] > others), (b, i, t)
    print(f"{clear} tokens with a clear gap, {top1} of them the oracle's arg-max")
    assert clear > 60 and top1 > 0
    # the order of the molecules within a pocket does not matter
    back = score(model, voc, [ms[::-1] for ms in MOLECULES], 2, example_of(z), prop1, device=DEV)
    for b in range(2):
        assert np.abs(np.array(back["sum_logp"][b][::-1]) - np.array(res["sum_logp"][b])).max() <= EPS / 4
        for x, y in zip(back["token_logp"][b][::-1], res["token_logp"][b]):
            assert np.abs(x - y).max() <= EPS / 4
    g = score(model, voc, MOLECULES, 2, example_of(z), prop1, device=DEV, grammar="smiles")
    assert [len(x) for x in g["allowed_logp"]] == [3, 7] and np.array_equal(g["sum_logp"][1], res["sum_logp"][1])
    with pytest.raises(ValueError, match="position 2"):
        score(model, voc, [["CCXC"], ["C"]], 2, example_of(z), prop1, device=DEV)
    with pytest.raises(ValueError, match="row 1, column 2"):
        score(model, voc, [["C"], ["C)"]], 2, example_of(z), prop1, device=DEV, grammar="smiles")


# ---------------------------------------------------------------------------------------------------------------- 6
def test_forced_columns_past_64_positions(setup):
    """A forced prefix of 70 tokens, one per pocket (the [batch_size, max_length] form), 4 rows each, T = 130, '$' suppressed in
    the free part: forced columns 64 .. 70 are decoded by the second 64-lane pass of the self-attention's score loop."""
    from singa_amd import smiles
    from tests.test_sampling_gpu import run
    z, model, sd = setup
    voc = smi_voc()
    sup = ("&", "^", "$")
    forced = smiles.encode(["CC(=O)N" * 10, "CCOCN" * 14], voc, 130)
    assert (is_forced(forced, len(voc)).sum(1) == 71).all()
    setting = (1.0, 0, 1.0)
    tokens, u, prop, tr = run(z, model, per=4, T=130, setting=setting, suppress=sup, forced=forced)
    tok_logp = tr["token_logp"].cpu().numpy()
    assert tokens.shape == (8, 130) and tr["path"] == "k17" and (tr["lengths"].cpu().numpy() == 129).all()
    full = np.repeat(forced, 4, 0)
    assert np.array_equal(tokens[:, :71], full[:, :71])
    allowed = np.ones(len(voc), np.uint8)
    allowed[[voc.index(s) for s in sup]] = 0
    res = check_forced_against_oracle(tokens, full, u.numpy(), oracle_of(z, sd, tokens, prop), voc.index("$"), *setting, allowed=allowed)
    late = res["forced_live"].copy()
    late[:, :64] = False
    assert (late.sum(1) == 7).all()                                  # all 8 rows have forced columns there
    err = np.abs(tok_logp.astype(np.float64) - res["logp"])
    print(f"forced columns >= 64: max |device logp - oracle logp| {err[late].max():.3e}; all columns {err[:, 1:].max():.3e}; "
          f"{res['free']} free decisions, {res['ambiguous']} ambiguous, {len(res['bad'])} mismatches")
    assert err[late].max() <= EPS / 4
    assert not res["bad"] and not res["forced_bad"]


# ---------------------------------------------------------------------------------------------------------------- 7
def test_grammar_and_prefix_together(setup, monkeypatch):
    from singa_amd import ops, smiles
    from singa_amd.model import Sampling
    from tests.test_sampling_gpu import run
    z, model, sd = setup
    voc = smi_voc()
    eos = voc.index("$")
    pre = smiles.tokenize("c1ccc(", voc)
    tokens, _, _, tr = run(z, model, per=32, T=24, grammar="smiles", forced=smiles.encode(["c1ccc("] * 2, voc, 24))
    assert tokens.shape == (64, 24)
    texts = set()
    for row in tokens:
        toks = G.row_text(row, voc, eos)
        assert toks is not None and toks[:len(pre)] == pre and G.parses(toks), row
        texts.add("".join(toks))
    assert len(texts) > 16
    launched = []
    monkeypatch.setattr(ops, "sample_token_forced", lambda *a, **k: launched.append("step"))
    monkeypatch.setattr(Sampling, "KVDecoder", lambda *a, **k: launched.append("decoder"))
    monkeypatch.setattr(model.model.encoder, "forward", lambda *a, **k: launched.append("encoder"))
    with pytest.raises(ValueError, match="row 0, column 2"):
        run(z, model, per=32, T=24, grammar="smiles", forced=smiles.encode(["C)"] * 2, voc, 24))
    assert not launched


# ---------------------------------------------------------------------------------------------------------------- 8
def test_gen_prefix_and_score_mode(tmp_path):
    """Text does not always determine the tokens: the shipped vocabulary holds '[V]' twice, and a drawn second '[V]' is scored
    as the first.  The fourth column is therefore compared on the lines without '[V]' - with 13 free columns of a random-weight
    model about (1 - 2 / 116) ^ 13 = 80 % of them, at least half is demanded - and the other three columns on all."""
    def gen(*args):
        cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "golden", "--seed", "1", "--max-length", "20", *args]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
        assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
        return [l for l in r.stdout.decode().splitlines() if not l.startswith("#")]
    draw = ("--mode", "sample", "--prefix", "c1ccc(", "--grammar", "smiles", "--num-samples", "8")
    a = gen(*draw)
    assert a == gen(*draw) and len(a) == 24
    voc = smi_voc()
    for line in a:
        name, text, length, logp = line.split("\t")
        assert text.startswith("c1ccc(") and G.parses(G.tokenize(text, voc)), text
    path = tmp_path / "molecules.tsv"
    order = a[16:] + a[:8] + a[8:16]                                 # pockets interleaved differently: the output follows the input
    path.write_text("\n".join("\t".join(l.split("\t")[:2]) for l in order) + "\n")
    scored = gen("--mode", "score", "--molecules", str(path))
    assert [l.split("\t")[:3] for l in scored] == [l.split("\t")[:3] for l in order]
    unique = [i for i, l in enumerate(order) if "[V]" not in l]
    assert len(unique) >= 12 and [scored[i] for i in unique] == [order[i] for i in unique]
