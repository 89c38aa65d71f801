"""-m gpu: grammar-constrained sampling (`singa_sample_token_grammar`, `sample(..., grammar="smiles")`, `gen.py --grammar`).

The kernel against the numpy restatement of the rule (tests/grammar_rule.py) combined with the float64 restatement of the
token choice (tests/sampling_rule.py): one step from a grid of states, whole sequences launch by launch, the write
footprint, then `sample` end to end against the CPU oracle decision by decision, as tests/test_sampling_gpu.py does for the
unconstrained draw, with the per-step mask rebuilt from the returned tokens.  What the rule produced is judged by a parser
written separately from it (grammar_rule.parses).  Tolerances: a decision is left out only when one of its thresholds is
closer than EPS in the float64 numbers alone (at most 2 % of a setting's decisions); log-probabilities hold the fp32 bound of
a V-term log-sum-exp (sampling_rule.logp_bound), `allowed_logp` - two log-sum-exps - twice that."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import grammar_rule as G
from tests.helpers import arena_runs, smi_voc
from tests.sampling_rule import EPS, choose, logp_bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(1.0, 0, 1.0), (0.7, 10, 0.95), (2.0, 5, 0.5), (0.0, 0, 1.0)]


def shipped():
    from singa_amd import smiles
    voc = smi_voc()
    return smiles.classify(voc), voc.index("$"), voc.index("^")


def wide():
    """200 class bytes whose structure tokens sit in the second and third register group of a lane (indices >= 64, >= 128)"""
    cls = np.full(200, G.ATOM, np.uint8)
    cls[[0, 1, 99, 160]] = G.NONE
    cls[[2, 3, 70, 140]] = G.BOND
    cls[[7, 135]] = G.DOT
    cls[64:69] = [G.RING | d << 4 for d in range(5)]
    cls[128:132] = [G.RING | d << 4 for d in range(5, 9)]
    cls[100], cls[150], cls[190] = G.OPEN, G.CLOSE, G.EOS
    return cls, 190, 0


def new_state(R, T, states, finished=None):
    st = {"tokens": torch.full((R, T), -7, dtype=torch.int64, device=DEV), "next": torch.full((R,), -7, dtype=torch.int64, device=DEV),
          "finished": torch.zeros(R, dtype=torch.uint8, device=DEV), "length": torch.zeros(R, dtype=torch.int32, device=DEV),
          "sum_logp": torch.zeros(R, device=DEV), "live": torch.zeros(1, dtype=torch.int32, device=DEV),
          "tok_logp": torch.full((R, T), 9.0, device=DEV), "allowed_logp": torch.full((R, T), 9.0, device=DEV),
          "grammar": torch.as_tensor(np.asarray(states, np.int32)).to(DEV)}
    if finished is not None:
        st["finished"].copy_(torch.as_tensor(finished, dtype=torch.uint8))
    st["live"].fill_(R - int(st["finished"].sum()))
    return st


def float64_step(z, u, setting, mask):
    """One row: -> (token or None for an empty mask, log-probability of it, ambiguous, log of the mass on the mask)"""
    z = z.astype(np.float64)
    lse = z.max() + np.log(np.exp(z - z.max()).sum())
    if not mask.any():
        return None, None, False, -np.inf
    tok, lp, amb = choose(z, float(u), *setting, mask, eps=EPS)
    zm = z[mask]
    return tok, lp, amb, zm.max() + np.log(np.exp(zm - zm.max()).sum()) - lse


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("vocab", [shipped, wide], ids=["V116", "V200"])
def test_one_step_matches_the_rule(vocab):
    from singa_amd import ops
    cls, eos, pad = vocab()
    V = len(cls)
    states = [G.pack(prev, depth, ring, here) for prev in range(1, 9) for depth in (0, 1, 2, 63)
              for ring in (0, 1, 0b100100, 0x1ff) for here in (0, ring & 0b101, ring)]
    assert len(states) == 384
    R = 384 + 16                                                    # the last 16 rows are finished
    states = np.array(states + states[5:21], np.int32)
    finished = np.zeros(R, np.uint8)
    finished[384:] = 1
    rs = np.random.RandomState(V)
    zl = rs.uniform(-10, 10, (R, V)).astype(np.float32)
    u = rs.rand(R).astype(np.float32)
    glob = (rs.rand(V) < 0.8).astype(np.uint8)
    glob[eos] = 1
    cls_d = torch.as_tensor(cls).to(DEV)
    zl_d = torch.as_tensor(zl).to(DEV)
    pos = torch.tensor([6], dtype=torch.int64, device=DEV)          # step 1 with pos_offset 5: reads uniforms[1], writes column 2
    cases = left_out = empty = 0
    worst_lp = worst_alp = 0.0
    for rem in (0, 1, 2, 3, 5, 12, 30):
        T = rem + 3
        uu = torch.full((T, R), 0.5)
        uu[1] = torch.as_tensor(u)
        uu = uu.to(DEV)
        gram = G.allows(states[:, None], cls[None, :], rem)         # [R, V]
        for al in (None, glob):
            masks = gram if al is None else gram & al.astype(bool)[None, :]
            for setting in SETTINGS:
                st = new_state(R, T, states, finished)
                ops.sample_token_grammar(zl_d, uu, pos, 5, st, cls_d, *setting, eos, pad,
                                         None if al is None else torch.as_tensor(al).to(DEV))
                torch.cuda.synchronize()
                got = {k: v.cpu().numpy() for k, v in st.items()}
                assert (got["tokens"][:, [0, 1] + list(range(3, T))] == -7).all()          # only column t + 1 is written
                assert (got["tok_logp"][:, :2] == 9.0).all() and (got["allowed_logp"][:, :2] == 9.0).all()
                n_eos = 0
                for r in range(R):
                    ctx = (V, rem, al is not None, setting, r, int(states[r]))
                    if finished[r]:
                        assert got["tokens"][r, 2] == pad and got["next"][r] == pad and got["length"][r] == 0, ctx
                        assert got["grammar"][r] == states[r] and got["tok_logp"][r, 2] == 0 and got["allowed_logp"][r, 2] == 0, ctx
                        continue
                    tok, lp, amb, alp = float64_step(zl[r], u[r], setting, masks[r])
                    if tok is None:                                 # empty mask: `pad`, still live, state kept
                        empty += 1
                        assert got["tokens"][r, 2] == pad and got["finished"][r] == 0 and got["grammar"][r] == states[r], ctx
                        assert got["allowed_logp"][r, 2] == -np.inf, ctx
                        continue
                    a_err = abs(float(got["allowed_logp"][r, 2]) - alp)
                    worst_alp = max(worst_alp, a_err)
                    assert a_err <= 2 * logp_bound(V, 10.0), (ctx, a_err)
                    g = int(got["tokens"][r, 2])
                    assert masks[r][g], (ctx, g)                    # whatever fp32 decides, never a masked token
                    n_eos += g == eos
                    assert got["grammar"][r] == int(G.transition(states[r], int(cls[g]))), (ctx, g)
                    cases += 1
                    if amb:
                        left_out += 1
                        continue
                    assert g == tok, (ctx, g, tok)
                    assert got["next"][r] == tok and got["length"][r] == 1 and got["finished"][r] == (tok == eos), ctx
                    err = abs(float(got["tok_logp"][r, 2]) - lp)
                    worst_lp = max(worst_lp, err)
                    assert err <= logp_bound(V, 10.0), (ctx, err)
                    assert got["sum_logp"][r] == got["tok_logp"][r, 2], ctx
                assert int(got["live"][0]) == 384 - n_eos
    print(f"V={V}: {cases} decisions, {left_out} ambiguous at eps {EPS}, {empty} rows with an empty mask, worst |tok_logp - float64| "
          f"{worst_lp:.3e} (bound {logp_bound(V, 10.0):.3e}), worst |allowed_logp - float64| {worst_alp:.3e}")
    assert cases > 5000 and empty > 0
    assert left_out <= 0.02 * cases


# ---------------------------------------------------------------------------------------------------------------- 2
def run_sequences(T, R=256, seed=0, setting=(1.0, 0, 1.0)):
    """R rows decoded launch by launch from fresh logits per step, biased towards the structure tokens"""
    from singa_amd import ops
    cls, eos, pad = shipped()
    voc = smi_voc()
    V = len(cls)
    rs = np.random.RandomState(seed + T)
    zl = rs.uniform(-3, 3, (T - 1, R, V)).astype(np.float32)
    zl[:, :, np.isin(cls & 15, (G.BOND, G.OPEN, G.CLOSE, G.RING, G.DOT))] += 2.5
    u = rs.rand(T - 1, R).astype(np.float32)
    st = new_state(R, T, np.full(R, G.FRESH, np.int32))
    st["tokens"].fill_(pad)
    st["tokens"][:, 0] = voc.index("&")
    cls_d, zl_d, u_d = torch.as_tensor(cls).to(DEV), torch.as_tensor(zl).to(DEV), torch.as_tensor(u).to(DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    for t in range(T - 1):
        ops.sample_token_grammar(zl_d[t], u_d, pos, 0, st, cls_d, *setting, eos, pad, None)
        pos += 1
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in st.items()}, zl, u, cls, eos, pad, voc


@pytest.mark.parametrize("T", [12, 41])
def test_sequences_end_in_time_and_parse(T):
    setting = (1.0, 0, 1.0)
    got, zl, u, cls, eos, pad, voc = run_sequences(T)
    tokens = got["tokens"]
    R = tokens.shape[0]
    assert int(got["live"][0]) == 0 and got["finished"].all()
    texts = set()
    for r in range(R):
        toks = G.row_text(tokens[r], voc, eos)
        assert toks is not None, tokens[r]
        assert G.parses(toks), "".join(toks)
        assert (tokens[r, 2 + len(toks):] == pad).all() and got["length"][r] == len(toks) + 1
        texts.add("".join(toks))
    assert any("(" in s for s in texts) and any("1" in s for s in texts) and len(texts) > R // 2
    # the rule replayed on the returned tokens reproduces every unambiguous decision
    states, on = G.replay(tokens, cls, eos)
    live = amb = 0
    for t in range(T - 1):
        masks = G.allows(states[:, t, None], cls[None, :], T - 2 - t)
        for r in np.flatnonzero(on[:, t]):
            tok, lp, a, alp = float64_step(zl[t, r], u[t, r], setting, masks[r])
            g = int(tokens[r, t + 1])
            live += 1
            amb += a
            assert masks[r][g], (r, t, g)
            assert a or g == tok, (r, t, g, tok)
            assert abs(float(got["allowed_logp"][r, t + 1]) - alp) <= 2 * logp_bound(len(cls), 5.5), (r, t)
    last = on.sum(1) - 1                                            # the step that drew '$': it leaves the state as it was
    assert np.array_equal(got["grammar"], states[np.arange(R), last])
    print(f"T={T}: {live} live decisions, {amb} ambiguous")
    assert amb <= 0.02 * live


def test_three_columns_hold_one_atom():
    got, _, _, cls, eos, _, voc = run_sequences(3)
    tokens = got["tokens"]
    assert (tokens[:, 0] == voc.index("&")).all() and ((cls[tokens[:, 1]] & 15) == G.ATOM).all() and (tokens[:, 2] == eos).all()
    assert int(got["live"][0]) == 0 and len(set(tokens[:, 1].tolist())) > 10


# ---------------------------------------------------------------------------------------------------------------- 3
def test_write_footprint():
    """Over NaN and 1e30 poison: one live step writes column t + 1 of tokens / tok_logp / allowed_logp and the per-row words
    and nothing else, a step outside 0 .. T - 2 writes nothing, and the two runs agree bit for bit."""
    from singa_amd import _lib
    lib = _lib.lib()
    _lib.ensure_init(torch.cuda.current_device())
    cls, eos, pad = shipped()
    V, R, T, off, t = len(cls), 7, 9, 10, 3
    g = torch.Generator().manual_seed(11)
    logits = (torch.rand(R, V, generator=g) * 8 - 4)
    uni = torch.rand(T - 1, R, generator=g)
    allowed = torch.ones(V, dtype=torch.uint8)
    allowed[[20, 25]] = 0
    states = [G.FRESH, G.pack(G.ATOM), G.pack(G.ATOM, 1, 1, 1), G.pack(G.OPEN, 1), G.pack(G.CLOSE), G.pack(G.ATOM), G.pack(G.RING, 0, 2, 2)]
    logits[4, eos] = 30.0                                             # row 4 (after ')', nothing open) draws '$'
    fin0 = torch.tensor([0, 1, 0, 0, 0, 0, 0], dtype=torch.uint8)
    init = dict(finished=fin0, length=torch.tensor([2, 3, 2, 2, 2, 1, 2], dtype=torch.int32), sum_logp=-torch.rand(R, generator=g) * 5,
                tokens=torch.randint(4, V, (R, T), generator=g), next=torch.randint(4, V, (R,), generator=g),
                live=torch.tensor([6], dtype=torch.int32), tok_logp=-torch.rand(R, T, generator=g),
                gstate=torch.tensor(states, dtype=torch.int32), allowed_logp=-torch.rand(R, T, generator=g))
    p = lambda v: None if v is None else v.ptr
    stream = torch.cuda.current_stream().cuda_stream

    def case(ar):
        vl, vu = ar.view("logits", logits.shape, data=logits), ar.view("uniforms", uni.shape, data=uni)
        va, vc = ar.view("allowed", (V,), torch.uint8, data=allowed), ar.view("cls", (V,), torch.uint8, data=torch.as_tensor(cls))
        for tag, step in (("live.", t), ("past.", T - 1), ("before.", -1)):
            vpos = ar.view(tag + "pos", (1,), torch.int64, data=[off + step])
            st = {k: ar.view(tag + k, v.shape, v.dtype, data=v, role="inout") for k, v in init.items()}
            code = lib.singa_sample_token_grammar(p(vl), p(vu), p(va), p(vc), p(vpos), off, R, V, T, 0.8, 12, 0.9, eos, pad,
                                                  p(st["finished"]), p(st["length"]), p(st["sum_logp"]), p(st["tokens"]),
                                                  p(st["next"]), p(st["live"]), p(st["tok_logp"]), p(st["gstate"]),
                                                  p(st["allowed_logp"]), stream)
            assert code == 0, lib.singa_last_error_string()
        return True

    rep_nan, rep_big, differ, _ = arena_runs(case, DEV, capacity=8 << 20)
    assert not differ, differ
    for rep in (rep_nan, rep_big):
        assert not rep.stray, rep.stray
        o = rep.out
        for tag in ("past.", "before."):
            for k, v in init.items():
                assert torch.equal(o[tag + k].view(-1), v.view(-1)), (tag, k)
        col = torch.zeros(T, dtype=torch.bool)
        col[t + 1] = True
        for k in ("tokens", "tok_logp", "allowed_logp"):
            assert torch.equal(o["live." + k][:, ~col], init[k][:, ~col]), k
        toks = o["live.tokens"][:, t + 1]
        assert toks[1] == pad and o["live.tok_logp"][1, t + 1] == 0 and o["live.allowed_logp"][1, t + 1] == 0
        assert o["live.gstate"][1] == states[1] and o["live.length"][1] == 3
        assert toks[4] == eos and o["live.finished"].tolist() == [0, 1, 0, 0, 1, 0, 0] and int(o["live.live"][0]) == 5
        for r in (0, 2, 3, 4, 5, 6):
            m = G.mask(states[r], cls, T - 2 - t) & allowed.numpy().astype(bool)
            assert m[int(toks[r])], (r, int(toks[r]))
            assert int(o["live.gstate"][r]) == int(G.transition(states[r], int(cls[int(toks[r])])))
            assert o["live.length"][r] == init["length"][r] + 1 and o["live.next"][r] == toks[r]
            assert o["live.allowed_logp"][r, t + 1] <= 0 and o["live.tok_logp"][r, t + 1] <= 0     # row 4: 30 against <= 4, -0.0 in fp32


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.fixture(scope="module")
def setup():
    from tests.helpers import golden
    from tests.test_beam_gpu import build_model
    z = golden("beam_b2_k6_eos.npz")
    model, sd, _ = build_model(z)
    return z, model, sd


def oracle_check_grammar(z, sd, tokens, u, prop, setting, cls):
    """tests/sampling_rule.check_against_oracle with the mask of every step rebuilt from the row's own tokens"""
    from tests.sampling_rule import oracle_logits
    from tests.test_sampling_gpu import example_of
    voc = smi_voc()
    eos = voc.index("$")
    ex = example_of(z)
    c = lambda t: t.cpu()
    logits = oracle_logits(sd, voc, tokens, c(ex.protein_atom_feature), c(ex.protein_pos), c(ex.protein_element_batch),
                           c(ex.protein_atom_laplacian), c(ex.protein_knn), prop, len(z["names"]))
    u = np.asarray(u, np.float64)
    R, T = tokens.shape
    live = amb = 0
    bad, lp, alp = [], np.zeros((R, T)), np.zeros((R, T))
    states, on = G.replay(tokens, cls, eos)
    for t in range(T - 1):
        masks = G.allows(states[:, t, None], cls[None, :], T - 2 - t)
        for r in np.flatnonzero(on[:, t]):
            m, zz = masks[r], logits[r, t]
            want, _, a = choose(zz, u[t, r], *setting, m, eps=EPS, exact_ties=False)
            got = int(tokens[r, t + 1])
            lse = zz.max() + np.log(np.exp(zz - zz.max()).sum())
            lp[r, t + 1] = zz[got] - lse
            alp[r, t + 1] = np.log(np.exp(zz[m] - zz.max()).sum()) + zz.max() - lse
            live += 1
            amb += a
            if not a and got != want:
                bad.append((r, t, got, want))
    return {"live": live, "ambiguous": amb, "bad": bad, "logp": lp, "allowed_logp": alp}


def all_parse(tokens):
    voc = smi_voc()
    texts = [G.row_text(row, voc, voc.index("$")) for row in tokens]
    return [t is not None and G.parses(t) for t in texts]


@pytest.mark.parametrize("setting", [(1.0, 0, 1.0), (0.7, 10, 0.95)], ids=["plain", "t0.7-k10-p0.95"])
def test_sample_with_grammar_end_to_end(setup, setting):
    from tests.test_sampling_gpu import run, well_formed
    z, model, sd = setup
    cls = shipped()[0]
    tokens, u, prop, tr = run(z, model, setting=setting, grammar="smiles")
    assert tokens.shape == (64, 41)
    lengths, tok_logp, alp = (tr[k].cpu().numpy() for k in ("lengths", "token_logp", "allowed_logp"))
    well_formed(tokens, lengths)
    assert all(all_parse(tokens))                                   # every row ends and parses
    assert (lengths <= 40).all()
    res = oracle_check_grammar(z, sd, tokens, u.numpy(), prop, setting, cls)
    dev = float(np.abs(tok_logp.astype(np.float64) - res["logp"])[:, 1:].max())
    dev_a = float(np.abs(alp.astype(np.float64) - res["allowed_logp"])[:, 1:].max())
    share = res["ambiguous"] / res["live"]
    print(f"grammar, setting {setting}: {res['live']} live decisions, {res['ambiguous']} ambiguous ({100 * share:.2f} %), "
          f"{len(res['bad'])} mismatches, max |device logp - oracle logp| {dev:.3e}, allowed_logp {dev_a:.3e}, steps {tr['steps']}")
    assert not res["bad"], res["bad"][:10]
    assert share <= 0.02, share
    assert EPS >= 4 * dev, dev
    assert EPS >= 2 * dev_a, dev_a                                  # two log-sum-exps of the same logits: twice tok_logp's share
    assert res["live"] == int(lengths.sum())
    # graph replay equals eager; the library path differs from k17 at ambiguous decisions only
    assert np.array_equal(tokens, run(z, model, setting=setting, grammar="smiles", graph=False)[0])
    assert tr["path"] == "k17"
    lib, _, _, tr_l = run(z, model, setting=setting, grammar="smiles", fused=False)
    assert tr_l["path"] == "library" and all(all_parse(lib))
    if not np.array_equal(tokens, lib):
        assert not oracle_check_grammar(z, sd, lib, u.numpy(), prop, setting, cls)["bad"]
    # the unconstrained draw from the same uniforms: unchanged by the new argument, and not all of it parses
    plain, _, _, tr_p = run(z, model, setting=setting)
    assert np.array_equal(plain, run(z, model, setting=setting, grammar=None)[0]) and "allowed_logp" not in tr_p
    assert not all(all_parse(plain))


# ---------------------------------------------------------------------------------------------------------------- 5
def test_gen_entry_point_with_grammar():
    cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "golden", "--mode", "sample", "--grammar", "smiles",
           "--num-samples", "8", "--max-length", "41", "--seed", "1"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    lines = [l for l in r.stdout.decode().splitlines() if not l.startswith("#")]
    assert len(lines) == 24
    voc = smi_voc()
    for line in lines:
        name, text, length, logp = line.split("\t")
        toks = G.tokenize(text, voc)
        assert G.parses(toks), text
        assert len(toks) + 1 == int(length) <= 40 and float(logp) <= 0.0
