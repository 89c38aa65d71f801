"""-m gpu: valence-aware sampling (`singa_sample_token_valence`, `grammar="valence"` of `sample`, `score`, `sample_stream` and
`gen.py`).

The kernel against the numpy restatement of the rule (tests/valence_rule.py) combined with the float64 restatement of the
token choice (tests/sampling_rule.py), as tests/test_grammar_gpu.py does for the SMILES rule and with its settings and
tolerances: one step from states that CPU walks reached, whole sequences launch by launch, the write footprint, then the
Python layer end to end.  What the rule produced is judged by the parser of tests/grammar_rule.py and by the graph builder of
tests/valence_rule.py, which knows nothing of the rule's state."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import grammar_rule as G
from tests import valence_rule as VR
from tests.helpers import arena_runs, smi_voc
from tests.sampling_rule import EPS, logp_bound
from tests.test_grammar_gpu import SETTINGS, float64_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def operands(voc):
    from singa_amd import smiles
    cap = smiles.capacity(voc)
    return smiles.classify_orders(voc), cap, voc.index("$"), voc.index("^"), {t: int(c) for t, c in zip(voc, cap)}


def new_state(R, T, states, finished=None, molecules=None):
    """the device state of R rows in front of a step: states [R, 3] (the state word and the two valence words)"""
    M = R if molecules is None else molecules
    states = np.asarray(states)
    st = {"tokens": torch.full((M, T), -7, dtype=torch.int64, device=DEV), "next": torch.full((R,), -7, dtype=torch.int64, device=DEV),
          "finished": torch.zeros(R, dtype=torch.uint8, device=DEV), "length": torch.zeros(M, dtype=torch.int32, device=DEV),
          "sum_logp": torch.zeros(M, device=DEV), "live": torch.zeros(1, dtype=torch.int32, device=DEV),
          "tok_logp": torch.full((M, T), 9.0, device=DEV), "allowed_logp": torch.full((M, T), 9.0, device=DEV),
          "grammar": torch.as_tensor(states[:, 0].astype(np.int32)).to(DEV),
          "valence": torch.as_tensor(np.ascontiguousarray(states[:, 1:3]).astype(np.int32)).to(DEV)}
    if finished is not None:
        st["finished"].copy_(torch.as_tensor(finished, dtype=torch.uint8))
    st["live"].fill_(R - int(st["finished"].sum()))
    return st


def step_states(cls, cap, eos):
    """384 states that walks under the rule reach (the three words), covering every prev code, att 0, the depth limit and nine
    open rings; the rest is drawn from the same walks"""
    pools = [VR.walks(41, 64, 1, cls, cap, eos, keep_states=True)["states"],
             VR.walks(81, 48, 2, cls, cap, eos, keep_states=True, weights={G.OPEN: 60.0, G.CLOSE: 1.0, G.EOS: 0.1})["states"],
             VR.walks(81, 48, 3, cls, cap, eos, keep_states=True, weights={G.RING: 60.0, G.EOS: 0.1})["states"]]
    pool = np.unique(np.concatenate(pools)[:, :3], axis=0)
    prev, depth, ring, _ = G.fields(pool[:, 0])
    att = pool[:, 1] & 7
    must = [prev == p for p in range(1, 9)] + [(att == 0) & (prev != G.START), depth == 10, depth == 9, ring == 0x1ff,
                                                (ring != 0) & (att == 0), (pool[:, 1] >> 3 & 3) == 2, (pool[:, 1] >> 5 & 1) == 1]
    rs = np.random.RandomState(5)
    take = []
    for m in must:
        idx = np.flatnonzero(m)
        assert len(idx), "the walks did not reach a state the test is about"
        take += rs.choice(idx, min(len(idx), 6), replace=False).tolist()
    rest = np.setdiff1d(np.arange(len(pool)), take)
    take = sorted(set(take)) + rs.choice(rest, 384 - len(set(take)), replace=False).tolist()
    assert len(take) == 384
    return pool[take]


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("vocab", ["V116", "V200"])
def test_one_step_matches_the_rule(vocab):
    from singa_amd import ops
    voc = smi_voc() if vocab == "V116" else VR.wide_vocabulary()
    cls, cap, eos, pad, _ = operands(voc)
    V = len(voc)
    live_states = step_states(cls, cap, eos)
    R = 384 + 16                                                    # the last 16 rows are finished
    states = np.concatenate([live_states, live_states[5:21]])
    finished = np.zeros(R, np.uint8)
    finished[384:] = 1
    rs = np.random.RandomState(V)
    zl = rs.uniform(-10, 10, (R, V)).astype(np.float32)
    u = rs.rand(R).astype(np.float32)
    glob = (rs.rand(V) < 0.8).astype(np.uint8)
    glob[eos] = 1
    REMS = (0, 1, 2, 3, 5, 12, 30)
    # the float64 restatement alone, before anything runs on the device: the masks, the choices, and the share of decisions
    # that these logits and uniforms leave ambiguous
    want, cases = {}, 0
    left_out = empty = 0
    for rem in REMS:
        gram = VR.allows(states[:, None, 0], states[:, None, 1], states[:, None, 2], cls[None], cap[None], rem)       # [R, V]
        nxt = VR.transition(states[:, None, 0], states[:, None, 1], states[:, None, 2], cls[None], cap[None])
        for al in (None, glob):
            masks = gram if al is None else gram & al.astype(bool)[None, :]
            for setting in SETTINGS:
                rows = [float64_step(zl[r], u[r], setting, masks[r]) for r in range(384)]
                want[rem, al is not None, setting] = masks, rows, nxt
                cases += sum(t is not None for t, _, _, _ in rows)
                left_out += sum(bool(a) for t, _, a, _ in rows if t is not None)
                empty += sum(t is None for t, _, _, _ in rows)
    print(f"V={V}: {cases} decisions, {left_out} ambiguous at eps {EPS}, {empty} rows with an empty mask")
    assert cases > 5000 and empty > 0
    assert left_out <= 0.02 * cases

    cls_d, cap_d, zl_d = torch.as_tensor(cls).to(DEV), torch.as_tensor(cap).to(DEV), torch.as_tensor(zl).to(DEV)
    pos = torch.tensor([6], dtype=torch.int64, device=DEV)          # step 1 with pos_offset 5: reads uniforms[1], writes column 2
    worst_lp = worst_alp = 0.0
    for (rem, with_al, setting), (masks, rows, nxt) in want.items():
        T = rem + 3
        uu = torch.full((T, R), 0.5)
        uu[1] = torch.as_tensor(u)
        st = new_state(R, T, states, finished)
        ops.sample_token(zl_d, uu.to(DEV), pos, 5, st, *setting, eos, pad, torch.as_tensor(glob).to(DEV) if with_al else None,
                         cls=cls_d, cap=cap_d, vstate=st["valence"])
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in st.items()}
        words = np.concatenate([got["grammar"][:, None], got["valence"]], 1)
        assert (got["tokens"][:, [0, 1] + list(range(3, T))] == -7).all()          # only column t + 1 is written
        assert (got["tok_logp"][:, :2] == 9.0).all() and (got["allowed_logp"][:, :2] == 9.0).all()
        n_eos = 0
        for r in range(R):
            ctx = (V, rem, with_al, setting, r, [int(x) for x in states[r]])
            if finished[r]:
                assert got["tokens"][r, 2] == pad and got["next"][r] == pad and got["length"][r] == 0, ctx
                assert np.array_equal(words[r], states[r]) and got["tok_logp"][r, 2] == 0 and got["allowed_logp"][r, 2] == 0, ctx
                continue
            tok, lp, amb, alp = rows[r]
            if tok is None:                                         # empty mask: `pad`, still live, all three words kept
                assert got["tokens"][r, 2] == pad and got["finished"][r] == 0 and np.array_equal(words[r], states[r]), ctx
                assert got["allowed_logp"][r, 2] == -np.inf, ctx
                continue
            a_err = abs(float(got["allowed_logp"][r, 2]) - alp)
            worst_alp = max(worst_alp, a_err)
            assert a_err <= 2 * logp_bound(V, 10.0), (ctx, a_err)
            g = int(got["tokens"][r, 2])
            assert masks[r][g], (ctx, g)                            # whatever fp32 decides, never a masked token
            n_eos += g == eos
            assert [int(words[r, i]) for i in range(3)] == [int(nxt[i][r, g]) for i in range(3)], (ctx, g)
            if amb:
                continue
            assert g == tok, (ctx, g, tok)
            assert got["next"][r] == tok and got["length"][r] == 1 and got["finished"][r] == (tok == eos), ctx
            err = abs(float(got["tok_logp"][r, 2]) - lp)
            worst_lp = max(worst_lp, err)
            assert err <= logp_bound(V, 10.0), (ctx, err)
            assert got["sum_logp"][r] == got["tok_logp"][r, 2], ctx
        assert int(got["live"][0]) == 384 - n_eos
    print(f"V={V}: worst |tok_logp - float64| {worst_lp:.3e} (bound {logp_bound(V, 10.0):.3e}), worst |allowed_logp - float64| "
          f"{worst_alp:.3e}")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("T", [12, 41])
def test_sequences_end_parse_and_hold_capacity(T):
    """256 rows decoded launch by launch from fresh logits per step, biased towards the structure tokens"""
    from singa_amd import ops
    voc = smi_voc()
    cls, cap, eos, pad, capacity = operands(voc)
    R, V = 256, len(voc)
    rs = np.random.RandomState(T)
    zl = rs.uniform(-3, 3, (T - 1, R, V)).astype(np.float32)
    zl[:, :, np.isin(cls & 15, (G.BOND, G.OPEN, G.CLOSE, G.RING, G.DOT))] += 2.5
    st = new_state(R, T, np.tile([G.FRESH, -1, 0x2aaaaaaa], (R, 1)))  # fresh rows: the valence words may hold anything
    st["tokens"].fill_(pad)
    st["tokens"][:, 0] = voc.index("&")
    cls_d, cap_d, zl_d = torch.as_tensor(cls).to(DEV), torch.as_tensor(cap).to(DEV), torch.as_tensor(zl).to(DEV)
    u_d = torch.as_tensor(rs.rand(T - 1, R).astype(np.float32)).to(DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    for t in range(T - 1):
        ops.sample_token(zl_d[t], u_d, pos, 0, st, 1.0, 0, 1.0, eos, pad, None, cls=cls_d, cap=cap_d, vstate=st["valence"])
        pos += 1
    torch.cuda.synchronize()
    tokens = st["tokens"].cpu().numpy()
    assert int(st["live"].item()) == 0 and bool(st["finished"].all())
    texts = set()
    for r in range(R):
        toks = G.row_text(tokens[r], voc, eos)
        assert toks is not None, tokens[r]                          # '$' in time
        assert G.parses(toks), "".join(toks)
        assert not VR.over_capacity(toks, capacity), ("".join(toks), VR.over_capacity(toks, capacity))
        texts.add("".join(toks))
    assert any("(" in s for s in texts) and any("1" in s for s in texts) and any("=" in s for s in texts) and len(texts) > R // 2
    states, on = VR.replay(tokens, cls, cap, eos)                   # the device's final words are the restatement's
    last = on.sum(1) - 1
    got = np.concatenate([st["grammar"].cpu().numpy()[:, None], st["valence"].cpu().numpy()], 1)
    assert np.array_equal(got, states[np.arange(R), last])


# ---------------------------------------------------------------------------------------------------------------- 3
def test_write_footprint():
    """Over NaN and 1e30 poison, through the C entry point: one live step writes column t + 1 of tokens / tok_logp / allowed_logp
    / rank and the live rows' words and nothing else, a step outside 0 .. T - 2 writes nothing, the two runs agree bit for bit."""
    from singa_amd import _lib
    lib = _lib.lib()
    _lib.ensure_init(torch.cuda.current_device())
    voc = smi_voc()
    cls, cap, eos, pad, _ = operands(voc)
    V, R, T, off, t = len(voc), 7, 9, 10, 3
    g = torch.Generator().manual_seed(11)
    logits = (torch.rand(R, V, generator=g) * 8 - 4)
    uni = torch.rand(T - 1, R, generator=g)
    allowed = torch.ones(V, dtype=torch.uint8)
    allowed[[20, 25]] = 0
    states = [(G.FRESH, 77, 99), (G.pack(G.ATOM),) + VR.vpack(3), (G.pack(G.ATOM, 1, 1, 1),) + VR.vpack(2, stack=[3]),
              (G.pack(G.OPEN, 1),) + VR.vpack(3, first=1, stack=[3]), (G.pack(G.CLOSE),) + VR.vpack(2), (G.pack(G.ATOM),) + VR.vpack(0),
              (G.pack(G.RING, 0, 2, 2),) + VR.vpack(2, rord=2)]
    logits[4, eos] = 30.0                                             # row 4 (after ')', nothing open) draws '$'
    forced = torch.full((R, T), -1, dtype=torch.int64)
    forced[6, t + 1] = voc.index("C")                                 # row 6 is given its token
    fin0 = torch.tensor([0, 1, 0, 0, 0, 0, 0], dtype=torch.uint8)
    init = dict(finished=fin0, length=torch.tensor([2, 3, 2, 2, 2, 1, 2], dtype=torch.int32), sum_logp=-torch.rand(R, generator=g) * 5,
                tokens=torch.randint(4, V, (R, T), generator=g), next=torch.randint(4, V, (R,), generator=g),
                live=torch.tensor([6], dtype=torch.int32), tok_logp=-torch.rand(R, T, generator=g),
                gstate=torch.tensor([s[0] for s in states], dtype=torch.int32),
                vstate=torch.tensor([s[1:] for s in states], dtype=torch.int32), allowed_logp=-torch.rand(R, T, generator=g),
                rank=torch.randint(0, V, (R, T), generator=g).to(torch.int32))
    p = lambda v: None if v is None else v.ptr
    stream = torch.cuda.current_stream().cuda_stream

    def case(ar):
        vl, vu = ar.view("logits", logits.shape, data=logits), ar.view("uniforms", uni.shape, data=uni)
        va, vc = ar.view("allowed", (V,), torch.uint8, data=allowed), ar.view("cls", (V,), torch.uint8, data=torch.as_tensor(cls))
        vk, vf = ar.view("cap", (V,), torch.uint8, data=torch.as_tensor(cap)), ar.view("forced", (R, T), torch.int64, data=forced)
        for tag, step in (("live.", t), ("past.", T - 1), ("before.", -1)):
            vpos = ar.view(tag + "pos", (1,), torch.int64, data=[off + step])
            st = {k: ar.view(tag + k, v.shape, v.dtype, data=v, role="inout") for k, v in init.items()}
            code = lib.singa_sample_token_valence(p(vl), p(vu), p(va), p(vc), p(vk), p(vpos), None, off, R, 0, V, T, 0.8, 12, 0.9, eos,
                                                  pad, p(st["finished"]), p(st["length"]), p(st["sum_logp"]), p(st["tokens"]),
                                                  p(st["next"]), p(st["live"]), p(st["tok_logp"]), p(st["gstate"]), p(st["vstate"]),
                                                  p(st["allowed_logp"]), p(vf), p(st["rank"]), stream)
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
        for k in ("tokens", "tok_logp", "allowed_logp", "rank"):
            assert torch.equal(o["live." + k][:, ~col], init[k][:, ~col]), k
        toks = o["live.tokens"][:, t + 1]
        assert toks[1] == pad and o["live.tok_logp"][1, t + 1] == 0 and o["live.allowed_logp"][1, t + 1] == 0
        assert o["live.gstate"][1] == states[1][0] and o["live.vstate"][1].tolist() == list(states[1][1:]) and o["live.length"][1] == 3
        ended = (toks == eos) & (fin0 == 0)                           # row 5 may draw '$' as well: '.' and '$' are all it has
        assert toks[4] == eos and torch.equal(o["live.finished"], fin0 | ended.to(torch.uint8))
        assert int(o["live.live"][0]) == 6 - int(ended.sum())
        assert toks[6] == voc.index("C")
        for r in (0, 2, 3, 4, 5, 6):
            i = int(toks[r])
            m = VR.allows(*states[r], cls, cap, T - 2 - t) & allowed.numpy().astype(bool)
            assert m[i] or r == 6, (r, i)
            want = VR.transition(*states[r], int(cls[i]), int(cap[i]))
            assert [int(o["live.gstate"][r])] + o["live.vstate"][r].tolist() == [int(w) for w in want], r
            assert o["live.length"][r] == init["length"][r] + 1 and o["live.next"][r] == toks[r]
            assert o["live.allowed_logp"][r, t + 1] <= 0 and o["live.tok_logp"][r, t + 1] <= 0
        assert (cls[int(toks[5])] & 15) in (G.DOT, G.EOS)          # row 5 (att = 0, nothing open): no bond can start here


# ---------------------------------------------------------------------------------------------------------------- 4
@pytest.fixture(scope="module")
def setup():
    from tests.helpers import golden
    from tests.test_beam_gpu import build_model
    z = golden("beam_b2_k6_eos.npz")
    model, sd, _ = build_model(z)
    return z, model, sd


def judged(tokens):
    """per row: ends, parses and holds every atom's capacity"""
    voc = smi_voc()
    capacity = operands(voc)[4]
    texts = [G.row_text(row, voc, voc.index("$")) for row in tokens]
    return [t is not None and G.parses(t) and not VR.over_capacity(t, capacity) for t in texts], texts


def bits(t):
    return torch.as_tensor(t).contiguous().view(torch.int32) if torch.as_tensor(t).dtype == torch.float32 else torch.as_tensor(t)


@pytest.mark.parametrize("setting", [(1.0, 0, 1.0), (0.7, 10, 0.95)], ids=["plain", "t0.7-k10-p0.95"])
def test_sample_score_and_stream_end_to_end(setup, setting):
    from singa_amd.model.Sampling import sample_stream, score
    from tests.test_sampling_gpu import example_of, run, well_formed
    z, model, sd = setup
    voc = smi_voc()
    capacity = operands(voc)[4]
    tokens, u, prop, tr = run(z, model, setting=setting, grammar="valence")
    assert tokens.shape == (64, 41) and tr["path"] == "k17"
    lengths, tok_logp, alp, sums = (tr[k].cpu().numpy() for k in ("lengths", "token_logp", "allowed_logp", "sum_logp"))
    well_formed(tokens, lengths)
    ok, texts = judged(tokens)
    assert all(ok), [("".join(t), VR.over_capacity(t, capacity)) for t, k in zip(texts, ok) if not k][:5]
    assert (lengths <= 40).all() and (alp <= 0).all() and (tok_logp[:, 1:] <= alp[:, 1:] + 2 * logp_bound(116, 30.0)).all()
    assert np.array_equal(tokens, run(z, model, setting=setting, grammar="valence", graph=False)[0])       # replay equals eager
    # what this grammar removes: the rows that the syntax alone leaves over capacity, from the same uniforms
    plain = run(z, model, setting=setting, grammar="smiles")[0]
    over = [bool(VR.over_capacity(t, capacity)) for t in judged(plain)[1]]
    print(f"setting {setting}: {sum(over)} of {len(over)} rows of grammar='smiles' hold an atom over its capacity "
          f"({100 * np.mean(over):.1f} %), 0 of grammar='valence'")
    # `score` of the drawn molecules: the same kernels in the same order, bit for bit
    B, per = 2, 32
    ids = [[int(x) for x in row[1:n]] for row, n in zip(tokens, lengths)]       # ids, not strings: the vocabulary holds '[V]' twice
    res = score(model, voc, [ids[b * per:(b + 1) * per] for b in range(B)], B, example_of(z),
                torch.as_tensor(z["prop"][:1]).float(), device=DEV, max_length=41, grammar="valence")
    for b in range(B):
        for i in range(per):
            r, n = b * per + i, int(lengths[b * per + i])
            assert res["length"][b][i] == n
            assert np.float32(res["sum_logp"][b][i]).tobytes() == sums[r].tobytes(), (r, res["sum_logp"][b][i], sums[r])
            assert res["token_logp"][b][i].tobytes() == tok_logp[r, 1:1 + n].tobytes(), r
            assert res["allowed_logp"][b][i].tobytes() == alp[r, 1:1 + n].tobytes(), r
    # `sample_stream` on any row budget: the same molecules and the same traced arrays, bit for bit
    prop1 = torch.as_tensor(z["prop"][:1]).float().repeat(B, 1).to(DEV)
    tau, k, p = setting
    for R in (1, 5, 37):
        st = {}
        got = sample_stream(model, voc, per, B, 41, example_of(z), prop1, R, device=DEV, temperature=tau, top_k=k, top_p=p,
                            uniforms=u, trace=st, grammar="valence")
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), tokens), R
        for key in ("lengths", "sum_logp", "token_logp", "allowed_logp"):
            assert torch.equal(bits(st[key].cpu()), bits(tr[key].cpu())), (R, key)


def test_forced_scaffold_is_continued(setup):
    from singa_amd import smiles
    from tests.test_sampling_gpu import run
    z, model, sd = setup
    voc = smi_voc()
    forced = smiles.encode(["c1ccc("] * 2, voc, 41)
    tokens, _, _, tr = run(z, model, grammar="valence", forced=forced, seed=3)
    ok, texts = judged(tokens)
    assert all(ok) and all("".join(t).startswith("c1ccc(") for t in texts)
    assert len({"".join(t) for t in texts}) > 16
    with pytest.raises(ValueError, match=r"row 0, column 3, token '='.*valence"):
        run(z, model, grammar="valence", forced=smiles.encode(["F(="] * 2, voc, 41))


def test_gen_entry_point_with_the_valence_grammar():
    cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "golden", "--mode", "sample", "--grammar", "valence",
           "--num-samples", "8", "--max-length", "41", "--seed", "1"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    lines = [l for l in r.stdout.decode().splitlines() if not l.startswith("#")]
    assert len(lines) == 24
    voc = smi_voc()
    capacity = operands(voc)[4]
    for line in lines:
        name, text, length, logp = line.split("\t")
        toks = G.tokenize(text, voc)
        assert G.parses(toks) and not VR.over_capacity(toks, capacity), text
        assert len(toks) + 1 == int(length) <= 40 and float(logp) <= 0.0
