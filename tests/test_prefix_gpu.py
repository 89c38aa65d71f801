"""-m gpu: forced tokens in continuous sampling, sampling without replacement and the device beam search
(`singa_sample_token_stream_forced`, `singa_swor_expand_forced`, `singa_forced_beam_expand`; include/singa_hip_prefix.h states
the rule), and `score(..., rows_per_pocket=...)`.

Kernel level: the streamed choice with forced tokens against `ops.sample_token(forced=...)` on one row per molecule, bit for
bit under every rule; one forced expansion of the stochastic beam against the unforced one; whole forced runs against the
float64 restatement (tests/prefix_rule.py) with the comparison and the EPS_G of tests/test_swor_gpu.py - every pocket, after
the restatement itself has shown that no run is ambiguous; the forced beam expansion and the unchanged selection against
tests/beam_rule.py with one-hot masks, as tests/test_beam_device_gpu.py compares; the write footprints.  End to end on a beam
golden: `sample_stream(forced=...)` is `sample(forced=...)`, `score(rows_per_pocket=...)` is `score`, distinct completions of a
scaffold, forced beam searches, and the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import beam_rule as BR
from tests import grammar_rule as G
from tests import prefix_rule as PR
from tests import swor_rule as R
from tests import test_beam_device_gpu as TB
from tests import test_stream_gpu as TS
from tests import test_swor_gpu as TW
from tests import valence_rule as VR
from tests.helpers import golden, smi_voc
from tests.sampling_rule import logp_bound
from tests.test_beam_gpu import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")
OFF = TS.OFF
EPS_G = TW.EPS_G                                                            # 1e-5: tests/test_swor_gpu.py's measured figure
bits, same = TW.bits, TS.same


# ------------------------------------------------------------------------------------------------ 1: the streamed choice
def rule_operands(rule):
    from singa_amd import smiles
    voc = smi_voc()
    if rule is None:
        return None, None
    cls = smiles.classify_orders(voc) if rule == "valence" else smiles.classify(voc)
    cap = torch.as_tensor(smiles.capacity(voc)).to(DEV) if rule == "valence" else None
    return torch.as_tensor(cls).to(DEV), cap


def forced_matrix(M, T, V, sos, eos, seed):
    """Molecule j: a forced run of j % T tokens from column 1 (T - 1: through the last column); every seventh an empty molecule
    ('$' in column 1), every eleventh a run that ends in its '$'."""
    rs = np.random.RandomState(seed)
    F = np.full((M, T), -1, np.int64)
    F[:, 0] = sos
    body = [v for v in range(V) if v != eos]
    for j in range(M):
        n = j % T
        F[j, 1:1 + n] = rs.choice(body, size=n)
        if j % 7 == 3:
            F[j, 1:] = -1
            F[j, 1] = eos
        elif j % 11 == 5 and n >= 2:
            F[j, n] = eos
    return F


def lockstep_reference(table, u, T, sos, eos, pad, cls, cap, F):
    """`ops.sample_token(forced=...)` on one row per molecule, step by step -> the final state"""
    from singa_amd import ops, smiles
    M = table.shape[0]
    i32 = dict(dtype=torch.int32, device=DEV)
    st = {"tokens": torch.full((M, T), pad, dtype=torch.int64, device=DEV), "next": torch.full((M,), sos, dtype=torch.int64, device=DEV),
          "finished": torch.zeros(M, dtype=torch.uint8, device=DEV), "length": torch.zeros(M, **i32), "sum_logp": torch.zeros(M, device=DEV),
          "live": torch.full((1,), M, **i32), "tok_logp": torch.zeros(M, T, device=DEV), "rank": torch.zeros(M, T, **i32)}
    st["tokens"][:, 0] = sos
    if cls is not None:
        st["grammar"] = torch.full((M,), smiles.FRESH, **i32)
        st["allowed_logp"] = torch.zeros(M, T, device=DEV)
    vst = torch.zeros(M, 2, **i32) if cap is not None else None
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    for t in range(T - 1):
        pos.fill_(OFF + t)
        ops.sample_token(table[:, t].contiguous(), u, pos, OFF, st, 1.0, 0, 1.0, eos, pad, None, cls=cls, forced=F, cap=cap, vstate=vst)
    return st


@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("V", [2, 116, 1024])
def test_stream_forced_equals_lockstep_forced(V, R):
    from singa_amd import ops, smiles
    B, T = 3, 6
    sos, eos, pad, _ = TS.marks(V)
    for rule in ((None,) if V != 116 else ("smiles", "valence")):
        cls, cap = rule_operands(rule)
        for n in sorted({1, R, 4 * R + 1}):
            M, rows = B * n, B * R
            table = TS.logit_table(M, T, V, eos, seed=V + 7 * R + n)
            u = torch.rand(T, M, generator=torch.Generator().manual_seed(n)).to(DEV)
            F_host = forced_matrix(M, T, V, sos, eos, seed=M)
            F = torch.as_tensor(F_host).to(DEV)
            ref = lockstep_reference(table, u, T, sos, eos, pad, cls, cap, F)
            st = TS.stream_state(B, R, n, T, sos, pad, cls is not None)
            st["rank"] = torch.zeros(M, T, dtype=torch.int32, device=DEV)
            vst = torch.zeros(rows, 2, dtype=torch.int32, device=DEV) if cap is not None else None
            limit = (-(-n // R) + 1) * (T - 1) + 2
            for s in range(limit):
                if int(st["live"].sum()) == 0:
                    break
                mol, t = st["mol"].clone(), st["pos"] - OFF
                live = mol >= 0
                logits = table[mol.clamp(min=0).long(), t.clamp(0, T - 2)].contiguous()
                logits[~live] = float("nan")                                   # a retired row's logits are not read
                ops.sample_token_stream(logits, u, st["pos"], st["mol"], OFF, st, 1.0, 0, 1.0, eos, pad, None, cls=cls, cap=cap,
                                        vstate=vst, forced=F)
                ops.stream_refill(st["pos"], st["mol"], OFF, st, R, n, T, sos, eos, smiles.FRESH, cls is not None)
            assert int(st["live"].sum()) == 0, (rule, n)
            assert torch.equal(F.cpu(), torch.as_tensor(F_host))                # forced is only read
            for k in ("tokens", "tok_logp", "length", "sum_logp", "rank") + (("allowed_logp",) if cls is not None else ()):
                assert same(st[k], ref[k]), (k, rule, n)
            given = (F_host[:, 1:] >= 0) & (F_host[:, 1:] < V)
            got = st["tokens"].cpu().numpy()
            assert np.array_equal(got[:, 1:][given], F_host[:, 1:][given])      # whatever the rule thinks of the token
            empty = given[:, 0] & (F_host[:, 1] == eos)
            assert (st["length"].cpu().numpy()[empty] == 1).all() and (got[empty, 2:] == pad).all()
            if M >= 6:
                assert int((st["length"] == T - 1).sum()) > 0                   # some were forced through the last column


# ------------------------------------------------------------------------------------------------ 2: one forced expansion
@pytest.mark.parametrize("V", [116, 1024])
def test_swor_expand_forced_single_step(V):
    from singa_amd import ops, smiles
    voc = smi_voc()
    B, k, T, t = 4, 5, 8, 2
    rows = B * k
    if V == len(voc):
        sos, eos, pad = voc.index("&"), voc.index("$"), voc.index("^")
        cls = torch.as_tensor(smiles.classify(voc)).to(DEV)
        f0, f2 = voc.index(")"), voc.index("N")                                # ')' at depth 0: the rule refuses it
    else:
        sos, eos, pad, cls, f0, f2 = 0, 2, 1, None, 700, 5
    rs = np.random.RandomState(V)
    g = -np.sort(rs.rand(B, k).astype(np.float32) * 3, axis=1)
    g[:2, k - 1] = NEG                                                         # dead slots
    fin = np.zeros((B, k), np.uint8)
    fin[:, 1] = 1                                                              # finished rows
    st = TW.new_state(B, k, V, T, sos, pad, grammar=int(smiles.pack(1)) if cls is not None else None)     # prev = ATOM
    st["gumbel"].copy_(torch.as_tensor(g.reshape(-1)))
    st["prop_logp"].copy_(torch.as_tensor(np.where(np.isfinite(g), g - 1.5, NEG).astype(np.float32).reshape(-1)))
    st["hash"].copy_(torch.as_tensor(rs.randint(0, 2 ** 62, rows)))
    st["finished"].copy_(torch.as_tensor(fin.reshape(-1)))
    logits = torch.as_tensor(rs.uniform(-8, 8, (rows, V)).astype(np.float32)).to(DEV)
    strm = TW.words([3, 4, 5, 2 ** 32 - 1])
    pos = torch.tensor([OFF + t], dtype=torch.int64, device=DEV)
    F = np.full((B, T), -1, np.int64)
    F[:, t], F[:, t + 2] = 1, 3                                                # neighbouring columns: not this step's
    F[0, t + 1], F[2, t + 1], F[3, t + 1] = f0, f2, V + 3                      # pockets 1 and 3 are free
    free_F = np.where(np.arange(T)[None] == t + 1, -1, F)
    F_d, free_d = torch.as_tensor(F).to(DEV), torch.as_tensor(free_F).to(DEV)
    names = ("cand", "cand_logp", "cand_phi")

    def expand(al, c, forced=None):
        for n in names:
            st[n].fill_(7.0)
        state = st if c is not None else {n: v for n, v in st.items() if n != "grammar"}
        ops.swor_expand(logits, pos, OFF, state, k, strm, 0.8, 11, pad, al, c, forced=forced)
        torch.cuda.synchronize()
        return {n: st[n].cpu().numpy().reshape(B, k, V) for n in names}

    nomask = expand(None, None)
    for closed in (None, f0, f2):
        al = None
        if closed is not None:
            al = torch.ones(V, dtype=torch.uint8, device=DEV)
            al[closed] = 0
        base = expand(al, cls)
        got = expand(al, cls, F_d)
        assert torch.equal(F_d.cpu(), torch.as_tensor(F))
        for n in names:
            assert np.array_equal(bits(expand(al, cls, free_d)[n]), bits(base[n])), (n, closed)     # all free: singa_swor_expand
        for b, f in ((0, f0), (1, None), (2, f2), (3, None)):
            for i in range(k):
                row = {n: got[n][b, i] for n in names}
                if f is None or not np.isfinite(g[b, i]) or fin[b, i]:                              # free, dead, finished: as unforced
                    for n in names:
                        assert np.array_equal(bits(row[n]), bits(base[n][b, i])), (n, closed, b, i)
                    continue
                others = np.arange(V) != f
                for n in names:
                    assert (row[n][others] == NEG).all(), (n, closed, b, i)
                assert bits(row["cand"][f:f + 1])[0] == bits(g[b, i:i + 1])[0], (closed, b, i)
                assert bits(row["cand_phi"][f:f + 1])[0] == bits((g[b, i:i + 1] - np.float32(1.5)))[0], (closed, b, i)
                assert bits(row["cand_logp"][f:f + 1])[0] == bits(nomask["cand_logp"][b, i, f:f + 1])[0], (closed, b, i)


# ------------------------------------------------------------------------------------------------ 3: runs against the restatement
def toy_run_forced(table, k, T, seed, streams, sos, eos, pad, allowed, forced, tau=1.0):
    """tests/test_swor_gpu.toy_run with the forced matrix"""
    from singa_amd import ops
    V, B = table.shape[0], len(streams)
    st = TW.new_state(B, k, V, T, sos, pad)
    table_d = torch.as_tensor(table).to(DEV)
    al = None if allowed is None else torch.as_tensor(allowed).to(DEV)
    F = torch.as_tensor(np.asarray(forced, np.int64)).to(DEV)
    work, strm = ops.swor_work(B * k, T, DEV), TW.words(streams)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    lives = []
    for t in range(T - 1):
        pos.fill_(t + 3)
        ops.swor_expand(table_d.index_select(0, st["next"]).contiguous(), pos, 3, st, k, strm, tau, seed, pad, al, forced=F)
        ops.swor_select(pos, 3, st, k, work, eos, pad)
        lives.append(st["live"].clone())
    torch.cuda.synchronize()
    out = {n: v.cpu().numpy().reshape((B, k) + tuple(v.shape[1:])) for n, v in st.items() if n not in ("live", "cand", "cand_logp", "cand_phi")}
    out["hash"] = out["hash"].view(np.uint64)
    out["valid"] = out["gumbel"] > NEG
    out["lives"] = torch.stack(lives).cpu().numpy()
    return out


def compare_with_rule(dev, want, prefixes, bound, ctx):
    """every pocket of a run: the device's rows are the rule's rows; -> the largest |G_device - G_rule|"""
    worst = 0.0
    for b, p in enumerate(prefixes):
        n = int(want["valid"][b].sum())
        assert int(dev["valid"][b].sum()) == n, (ctx, b)
        at = {tuple(r): i for i, r in enumerate(want["tokens"][b, :n])}
        assert len(at) == n
        for r in range(n):
            assert tuple(dev["tokens"][b, r]) in at, (ctx, b, r)
            assert list(dev["tokens"][b, r, 1:1 + len(p)]) == list(p), (ctx, b, r)
            i = at[tuple(dev["tokens"][b, r])]
            worst = max(worst, abs(float(dev["gumbel"][b, r]) - want["gumbel"][b, i]))
            assert abs(float(dev["prop_logp"][b, r]) - want["prop_logp"][b, i]) <= bound, (ctx, b, r)
            assert abs(float(dev["sum_logp"][b, r]) - want["sum_logp"][b, i]) <= bound, (ctx, b, r)
            assert dev["hash"][b, r] == want["hash"][b, i] and dev["length"][b, r] == want["length"][b, i], (ctx, b, r)
            assert bool(dev["finished"][b, r]) == bool(want["finished"][b, i]), (ctx, b, r)
    return worst


@pytest.mark.parametrize("V", [64, 65, 117])
def test_forced_runs_are_the_rules_top_k(V):
    """216 pocket runs over the three vocabularies: prefixes of 1 and 4 tokens and a pocket without one, in two arrangements.
    No pocket is left out: the restatement finds every run unambiguous (gap >= EPS_G), which is asserted first."""
    sos, eos, pad, allowed = TW.toy_vocab(V)
    T, streams = 10, [1, 2, 2 ** 32 - 1]
    table = R.toy_table(V, 100 + V, sos, eos, pad)
    bound = logp_bound(V, float(np.abs(table).max())) * T
    worst, runs = 0.0, 0
    for k in (1, 3, 64, 65):
        for lens in ((1, 4, 0), (4, 0, 1)):
            prefixes = PR.toy_prefixes(V, lens)
            forced = PR.prefix_matrix(prefixes, T, sos)
            for seed in TW.SEEDS:
                want = PR.run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed, forced=forced)
                assert (want["gap"] >= EPS_G).all(), (V, k, lens, seed, want["gap"])
                dev = toy_run_forced(table, k, T, seed, streams, sos, eos, pad, allowed, forced)
                TW.check_invariants(dev, T, pad, eos)
                worst = max(worst, compare_with_rule(dev, want, prefixes, bound, (V, k, lens, seed)))
                runs += len(streams)
    print(f"V={V}: {runs} pocket runs, all compared, largest |G_device - G_rule| {worst:.3e}, EPS_G {EPS_G:.0e}")
    assert runs == 72 and EPS_G >= 4 * worst, worst


def test_forced_run_wide_vocabulary():
    V, k, T = 1024, 3, 6
    sos, eos, pad, allowed = TW.toy_vocab(V)
    table = R.toy_table(V, 200 + V, sos, eos, pad)
    streams, seed = [3, 2 ** 31], 6
    prefixes = PR.toy_prefixes(V, (2, 2))
    forced = PR.prefix_matrix(prefixes, T, sos)
    want = PR.run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed, forced=forced)
    assert (want["gap"] >= EPS_G).all(), want["gap"]
    dev = toy_run_forced(table, k, T, seed, streams, sos, eos, pad, allowed, forced)
    TW.check_invariants(dev, T, pad, eos)
    worst = compare_with_rule(dev, want, prefixes, logp_bound(V, float(np.abs(table).max())) * T, (V, k))
    assert EPS_G >= 4 * worst, worst


def test_nesting_under_a_prefix():
    V, T = 65, 12
    sos, eos, pad, allowed = TW.toy_vocab(V)
    table = R.toy_table(V, V, sos, eos, pad)
    forced = PR.prefix_matrix(PR.toy_prefixes(V, (3, 0)), T, sos)
    small = toy_run_forced(table, 8, T, 77, [3, 4], sos, eos, pad, allowed, forced)
    big = toy_run_forced(table, 32, T, 77, [3, 4], sos, eos, pad, allowed, forced)
    TW.check_invariants(small, T, pad, eos), TW.check_invariants(big, T, pad, eos)
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp", "hash", "length", "finished"):
        assert np.array_equal(bits(small[key]), bits(big[key][:, :8])), key


# ------------------------------------------------------------------------------------------------ 4: the forced beam expansion
BEAM_LENS = {1: (0, 2), 3: (3, 0), 6: (2, 3), 70: (3, 2)}                     # prefix tokens per pocket, by k
BEAM_PREFIX = ["C", "(", "N"]                                                 # every head of it is a prefix both rules accept


@pytest.mark.parametrize("grammar", [None, "smiles", "valence"])
@pytest.mark.parametrize("V", [7, 116])
@pytest.mark.parametrize("k", [1, 3, 6, 70])
def test_forced_beam_kernels_match_the_rule_at_every_step(k, V, grammar):
    from singa_amd import ops
    B, T = 2, 8
    voc, sos, eos, pad = TB.vocabulary(V)
    cls, cap = TB.operands(voc, grammar)
    forced = PR.prefix_matrix([[voc.index(x) for x in (["C", "N"] if n == 2 else BEAM_PREFIX[:n])] for n in BEAM_LENS[k]], T, sos)
    run = BR.Search(B, k, V, T, sos, eos, pad, cls=cls, cap=cap)
    rs = np.random.RandomState(1000 * k + V)
    tables, snaps = [], []
    for t in range(T - 1):
        masks = PR.beam_masks(run, forced)
        for attempt in range(400):                                             # redrawn until the ranked candidates are well apart
            z = (2.5 * rs.randn(B * k, V)).astype(np.float32)
            cand = run.expand(z, masks)
            if TB.ranked_gaps_ok(run, cand):
                break
        else:
            raise AssertionError(f"no fair logits for step {t} in 400 draws")
        run.select(cand)
        run.t += 1
        tables.append(z)
        snaps.append(run.snapshot())
        for b, n in enumerate(BEAM_LENS[k]):
            if t < n:
                assert run.live[b] == 1                                        # one live slot through the prefix
    st = TB.new_state(B, k, V, T, sos, pad, grammar)
    cls_d = None if cls is None else torch.as_tensor(cls).to(DEV)
    cap_d = None if cap is None else torch.as_tensor(cap).to(DEV)
    F = torch.as_tensor(forced).to(DEV)
    work = ops.beam_work(B * k, T, DEV)
    len_pow = torch.tensor([1.0] + [float(n ** 0.7) for n in range(1, T)], dtype=torch.float64, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    logits = torch.as_tensor(np.stack(tables)).to(DEV)
    for t in range(T - 1):
        pos.fill_(t + 3)
        ops.beam_expand(logits[t].contiguous(), pos, 3, st, k, None, cls_d, cap_d, forced=F)
        ops.beam_select(pos, 3, st, k, work, len_pow, eos, pad, cls_d, cap_d)
        torch.cuda.synchronize()
        TB.compare(t, {n: v.cpu().numpy() for n, v in st.items()}, snaps[t], B, k, T, grammar)
    assert torch.equal(F.cpu(), torch.as_tensor(forced))
    run.finish()
    for b, n in enumerate(BEAM_LENS[k]):
        want = [voc.index(x) for x in (["C", "N"] if n == 2 else BEAM_PREFIX[:n])]
        assert len(run.hyps[b].items) >= 1
        assert all(list(toks[1:1 + n]) == want for _, _, toks, _ in run.hyps[b].items), b


# ------------------------------------------------------------------------------------------------ 5: write footprints
def test_footprint_stream_forced():
    """As tests/test_stream_gpu.py's choice case: one column of the live rows' molecules - `rank` among them -, their sums and
    lengths, the live rows' next / grammar words; `forced` comes back unchanged."""
    from singa_amd import _lib, ops, smiles
    voc = smi_voc()
    V, T, B, Rr, n = len(voc), 6, 2, 4, 6
    sos, eos, pad, cls = TS.marks(V)
    M, rows = B * n, B * Rr
    lib = _lib.lib()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: ctypes.c_void_p(v.ptr)
    atom = voc.index("C")
    mol = torch.tensor([2, 3, -1, 4, -1, -1, -1, -1], dtype=torch.int32)
    pos = torch.tensor([3, 5, 2, 2, 4, 1, 3, 5], dtype=torch.int64)         # steps 2, 4 (the last column), -, 1
    live = mol >= 0
    j, t = mol[live].long(), pos[live] - OFF
    table = TS.logit_table(rows, 2, V, eos, seed=5)[:, 0]
    table[~live.to(DEV)] = float("nan")
    u = torch.rand(T, M, generator=torch.Generator().manual_seed(2))
    forced = torch.randint(0, V, (M, T), generator=torch.Generator().manual_seed(3))      # what no live row reads is arbitrary
    forced[2, 3], forced[3, 5], forced[4, 2] = voc.index("N"), eos, -1                     # forced, forced to '$', free
    tokens = torch.full((M, T), pad, dtype=torch.int64)
    tokens[:, 0] = sos
    tok_logp, alp, rank = torch.zeros(M, T), torch.zeros(M, T), torch.full((M, T), 9, dtype=torch.int32)
    for jj, tt in zip(j, t):
        tokens[jj, 1:tt + 1], tok_logp[jj, 1:tt + 1], alp[jj, 1:tt + 1] = atom, -1.5, -0.25
    length, sums = torch.zeros(M, dtype=torch.int32), torch.zeros(M)
    length[j], sums[j] = t.int(), -1.5 * t.float()
    nxt = torch.full((rows,), atom, dtype=torch.int64)
    gs = torch.full((rows,), int(smiles.pack(1)), dtype=torch.int32)
    dense = {"tokens": tokens, "tok_logp": tok_logp, "allowed_logp": alp, "length": length, "sum_logp": sums, "next": nxt, "grammar": gs,
             "rank": rank}
    dense = {k: v.clone().to(DEV) for k, v in dense.items()}
    ops.sample_token_stream(table, u.to(DEV), pos.to(DEV), mol.to(DEV), OFF, dense, 1.0, 0, 1.0, eos, pad, None, cls=cls,
                            forced=forced.to(DEV))
    torch.cuda.synchronize()
    assert dense["tokens"][2, 3] == voc.index("N") and dense["tokens"][3, 5] == eos
    col = torch.zeros(M, T, dtype=torch.bool)
    col[j, t + 1] = True
    per_mol = torch.zeros(M, dtype=torch.bool)
    per_mol[j] = True

    def choice(ar):
        i = {"logits": ar.view("logits", (rows, V), data=table), "u": ar.view("u", (T, M), data=u),
             "cls": ar.view("cls", (V,), torch.uint8, data=cls), "pos": ar.view("pos", (rows,), torch.int64, data=pos),
             "mol": ar.view("mol", (rows,), torch.int32, data=mol), "forced": ar.view("forced", (M, T), torch.int64, data=forced)}
        o = {"tokens": ar.view("tokens", (M, T), torch.int64, data=tokens, role="inout", promised=col),
             "tok_logp": ar.view("tok_logp", (M, T), data=tok_logp, role="inout", promised=col),
             "allowed_logp": ar.view("allowed_logp", (M, T), data=alp, role="inout", promised=col),
             "rank": ar.view("rank", (M, T), torch.int32, data=rank, role="inout", promised=col),
             "length": ar.view("length", (M,), torch.int32, data=length, role="inout", promised=per_mol),
             "sum_logp": ar.view("sum_logp", (M,), data=sums, role="inout", promised=per_mol),
             "next": ar.view("next", (rows,), torch.int64, data=nxt, role="inout", promised=live),
             "grammar": ar.view("grammar", (rows,), torch.int32, data=gs, role="inout", promised=live)}
        code = lib.singa_sample_token_stream_forced(p(i["logits"]), p(i["u"]), None, p(i["cls"]), None, p(i["pos"]), p(i["mol"]), OFF,
                                                    rows, M, V, T, 1.0, 0, 1.0, eos, pad, p(o["length"]), p(o["sum_logp"]),
                                                    p(o["tokens"]), p(o["next"]), p(o["tok_logp"]), p(o["grammar"]), None,
                                                    p(o["allowed_logp"]), p(i["forced"]), p(o["rank"]), stream())
        assert code == 0, lib.singa_last_error_string()

    for rep in TS.arena_pair(choice):
        for k, want in dense.items():
            assert same(rep.out[k], want.cpu()), k


def test_footprint_swor_expand_forced():
    """After 4 steps of a toy run (finished, live and dead rows): cand, cand_logp and cand_phi are written in full and nothing
    else is, `forced` comes back unchanged, and the results are the dense op's."""
    from singa_amd import _lib, ops
    V, k, B, T, steps = 5, 40, 2, 9, 4
    st, table, strm, al, pos, (sos, eos, pad) = TW.mid_run_state(V, k, B, T, steps)
    rows = B * k
    fin, dead = st["finished"].bool(), st["gumbel"] == NEG
    assert int(fin.sum()) > 0 and int(dead.sum()) > 0 and int((~fin & ~dead).sum()) > 0
    logits = table.index_select(0, st["next"]).contiguous()
    forced = torch.full((B, T), 4, dtype=torch.int64)
    forced[0, steps + 1], forced[1, steps + 1] = 3, -1                         # pocket 0 forced, pocket 1 free
    dense = {n: v.clone() for n, v in st.items()}
    ops.swor_expand(logits, pos, 0, dense, k, strm, 1.0, 5, pad, al, forced=forced.to(DEV))
    torch.cuda.synchronize()
    lib = _lib.lib()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: ctypes.c_void_p(v.ptr)

    def expand(ar):
        i = {n: ar.view(n, st[n].shape, st[n].dtype, data=st[n]) for n in ("gumbel", "prop_logp", "hash", "finished")}
        lg, a, s, ps = ar.view("logits", logits.shape, data=logits), ar.view("allowed", (V,), torch.uint8, data=al), \
            ar.view("streams", (B,), torch.int32, data=strm), ar.view("pos", (1,), torch.int64, data=pos)
        f = ar.view("forced", (B, T), torch.int64, data=forced)
        o = {n: ar.view(n, (rows, V), role="out") for n in ("cand", "cand_logp", "cand_phi")}
        code = lib.singa_swor_expand_forced(p(lg), p(a), None, p(ps), 0, rows, k, V, T, 1.0, 5, p(s), pad, p(i["gumbel"]),
                                            p(i["prop_logp"]), p(i["hash"]), p(i["finished"]), None, p(o["cand"]), p(o["cand_logp"]),
                                            p(o["cand_phi"]), p(f), stream())
        assert code == 0, lib.singa_last_error_string()

    for rep in TW.arena_pair(expand):
        for n in ("cand", "cand_logp", "cand_phi"):
            assert torch.equal(rep.out[n].view(torch.int32), dense[n].cpu().view(torch.int32)), n
    live0 = (~fin & ~dead)[:k].cpu()
    assert (dense["cand"][:k].cpu()[live0][:, [0, 1, 2, 4]] == NEG).all() and (dense["cand"][:k].cpu()[live0][:, 3] > NEG).all()


def test_footprint_forced_beam_expand():
    """cand of the pockets that are not done is written in full - a done pocket's rows are not written -, nothing else is."""
    from singa_amd import _lib, ops
    voc, sos, eos, pad = TB.vocabulary(7)
    V, B, k, T = 7, 3, 3, 8
    rows = B * k
    st = TB.new_state(B, k, V, T, sos, pad, None)
    st["score"].copy_(torch.tensor([0.0, -1.0, NEG, -0.5, NEG, NEG, -2.0, -3.0, -4.0]))
    st["done"].copy_(torch.tensor([0, 1, 0], dtype=torch.uint8))
    logits = torch.randn(rows, V, generator=torch.Generator().manual_seed(1)).to(DEV)
    pos = torch.tensor([5], dtype=torch.int64, device=DEV)                    # step 2 with pos_offset 3
    forced = torch.full((B, T), 2, dtype=torch.int64)
    forced[0, 3], forced[2, 3] = voc.index("N"), -1
    dense = {n: v.clone() for n, v in st.items()}
    dense["cand"].fill_(5.0)
    ops.beam_expand(logits, pos, 3, dense, k, None, None, None, forced=forced.to(DEV))
    torch.cuda.synchronize()
    want = dense["cand"].cpu()
    assert (want[3:6] == 5.0).all() and (want[2] == NEG).all() and int((want[0] > NEG).sum()) == 1 and (want[6:] > NEG).all()
    lib = _lib.lib()
    p = lambda v: ctypes.c_void_p(v.ptr)
    written = torch.tensor([1, 1, 1, 0, 0, 0, 1, 1, 1], dtype=torch.bool)[:, None]

    def expand(ar):
        lg, ps = ar.view("logits", (rows, V), data=logits), ar.view("pos", (1,), torch.int64, data=pos)
        sc, dn = ar.view("score", (rows,), data=st["score"]), ar.view("done", (B,), torch.uint8, data=st["done"])
        f = ar.view("forced", (B, T), torch.int64, data=forced)
        c = ar.view("cand", (rows, V), role="out", promised=written)
        code = lib.singa_forced_beam_expand(p(lg), None, None, None, p(ps), 3, rows, k, V, T, p(sc), None, None, p(dn), p(c), p(f),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == 0, lib.singa_last_error_string()

    for rep in TW.arena_pair(expand):
        got = rep.out["cand"]
        assert torch.equal(got[written[:, 0]].view(torch.int32), want[written[:, 0]].view(torch.int32))


# ------------------------------------------------------------------------------------------------ 6: with the model
@pytest.fixture(scope="module")
def setup():
    from tests.test_sampling_gpu import example_of
    z = golden("beam_b2_k6_eos.npz")
    model, _, _ = build_model(z)
    return z, model, example_of(z)


PER, T6 = 10, 24
WHOLE = "CC(=O)Nc1ccccc1"


def mixed_forced(B, per, T):
    """prefixes "", "C", "c1ccc(" and a whole molecule with its '$', cycling over the molecules"""
    from singa_amd import smiles
    voc = smi_voc()
    kinds = ["", "C", "c1ccc(", WHOLE]
    F = smiles.encode([kinds[r % 4] for r in range(B * per)], voc, T)
    whole = smiles.encode([WHOLE], voc, T, end=True)[0]
    F[3::4] = whole
    return F


@pytest.fixture(scope="module")
def lockstep(setup):
    """`sample(forced=F)` once per grammar: tokens, uniforms and the trace on the host"""
    from tests.test_sampling_gpu import run
    z, model, ex = setup
    out = {}
    for grammar in (None, "smiles", "valence"):
        tokens, u, _, tr = run(z, model, per=PER, T=T6, seed=11, ex=ex, grammar=grammar, forced=mixed_forced(2, PER, T6))
        out[grammar] = tokens, u, {k: v.cpu() for k, v in tr.items() if torch.is_tensor(v)}
    return out


@pytest.mark.parametrize("R", [1, 5, 37])
@pytest.mark.parametrize("grammar", [None, "smiles", "valence"])
def test_sample_stream_forced_equals_sample_forced(setup, lockstep, grammar, R):
    tokens, u, tr = lockstep[grammar]
    F = mixed_forced(2, PER, T6)
    keys = ("lengths", "sum_logp", "token_logp", "rank") + (("allowed_logp",) if grammar else ())
    for graph in ((True, False) if R == 5 else (True,)):                        # replay equals eager
        got, st = TS.stream(setup, PER, R, T6, u, grammar=grammar, forced=F, graph=graph)
        assert np.array_equal(got, tokens), graph
        for k in keys:
            assert same(st[k].cpu(), tr[k]), (k, graph)
    given = (F >= 0) & (F < len(smi_voc()))
    assert np.array_equal(tokens[given], F[given])
    if R == 5:                                                                  # one prefix per pocket, repeated per molecule
        per_pocket = F[[1, PER]]                                                # "C" and "c1ccc("
        a, _ = TS.stream(setup, PER, R, T6, u, grammar=grammar, forced=per_pocket)
        b, _ = TS.stream(setup, PER, R, T6, u, grammar=grammar, forced=np.repeat(per_pocket, PER, 0))
        assert np.array_equal(a, b) and (a[:PER, 1] == per_pocket[0, 1]).all()


LIBRARY = (["CCO", "CC(=O)Nc1ccc(O)cc1", "", "C[C@H](N)C(=O)O", "c1ccccc1", "ClCCBr", "N#Cc1ccccc1"],
           ["CN1CCC[C@H]1c1cccnc1", "C1CC1", "O=C(O)c1ccccc1OC(C)=O"])


@pytest.mark.parametrize("grammar", [None, "valence"])
def test_score_on_a_row_budget_equals_score(setup, grammar):
    from singa_amd.model.Sampling import score
    z, model, ex = setup
    voc = smi_voc()
    prop = torch.as_tensor(z["prop"][:1]).float()
    want = score(model, voc, LIBRARY, 2, ex, prop, device=DEV, grammar=grammar)
    assert [len(x) for x in want["sum_logp"]] == [7, 3] and want["length"][0][2] == 1
    for R in (1, 4):
        got = score(model, voc, LIBRARY, 2, ex, prop, device=DEV, grammar=grammar, rows_per_pocket=R)
        assert set(got) == set(want)
        for key in want:
            for b in range(2):
                assert len(got[key][b]) == len(want[key][b])
                for x, y in zip(got[key][b], want[key][b]):
                    if isinstance(y, np.ndarray):
                        assert x.dtype == y.dtype and np.array_equal(bits(x), bits(y)), (key, R, b)
                    else:
                        assert type(x) is type(y) and np.array_equal(bits(np.float32(x)), bits(np.float32(y))) and x == y, (key, R, b)
    with pytest.raises(ValueError, match="one prompt per pocket"):
        score(model, voc, LIBRARY, 2, ex, prop.repeat(14, 1), device=DEV, rows_per_pocket=4)


def distinct(setup, k, T, forced, grammar="smiles", graph=True, seed=4):
    from singa_amd.model.Sampling import sample_distinct
    z, model, ex = setup
    B = len(z["names"])
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(B * k, 1).to(DEV)
    tr = {}
    out = sample_distinct(model, smi_voc(), k, B, T, ex, prop, device=DEV, suppress=("&", "^"), grammar=grammar, seed=seed,
                          graph=graph, trace=tr, forced=forced)
    torch.cuda.synchronize()
    res = {n: v.cpu().numpy().reshape((B, k) + tuple(v.shape[1:])) for n, v in tr.items() if torch.is_tensor(v)}
    res["tokens"], res["steps"] = out.cpu().numpy().reshape(B, k, T), tr["steps"]
    return res


def test_distinct_completions_of_a_scaffold(setup):
    from singa_amd import smiles
    from singa_amd.model.Sampling import score
    z, model, ex = setup
    voc = smi_voc()
    eos = voc.index("$")
    B, k, T = 2, 12, 24
    pre = smiles.tokenize("c1ccc(", voc)
    forced = smiles.encode(["c1ccc("] * B, voc, T)
    res = distinct(setup, k, T, forced)
    mols = [[] for _ in range(B)]
    for b in range(B):
        rows = [r for r in range(k) if res["valid"][b, r]]
        assert len(rows) >= 2 and len({tuple(res["tokens"][b, r]) for r in rows}) == len(rows)
        g = res["gumbel"][b, rows]
        assert (g <= 0).all() and (np.diff(g) <= 0).all()
        for r in rows:
            text = G.row_text(res["tokens"][b, r], voc, eos)
            assert text is not None and text[:len(pre)] == pre and G.parses(text), res["tokens"][b, r]
            mols[b].append((r, [int(t) for t in res["tokens"][b, r, 1:int(res["lengths"][b, r])]]))
    sc = score(model, voc, [[m for _, m in mb] for mb in mols], B, ex, torch.as_tensor(z["prop"][:1]).float(), device=DEV, max_length=T)
    for b in range(B):
        for i, (r, m) in enumerate(mols[b]):
            ln = len(m) + 1
            assert sc["length"][b][i] == ln == res["lengths"][b, r]
            assert bits(np.float32(sc["sum_logp"][b][i])) == bits(res["sum_logp"][b, r]), (b, r)
            assert np.array_equal(bits(sc["token_logp"][b][i]), bits(res["token_logp"][b, r, 1:1 + ln])), (b, r)
    eager = distinct(setup, k, T, forced, graph=False)
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp", "token_logp", "lengths"):
        assert np.array_equal(bits(res[key]), bits(eager[key])), key
    small, big = distinct(setup, 8, T, forced), distinct(setup, 32, T, forced)
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp", "token_logp", "lengths"):
        assert np.array_equal(bits(small[key]), bits(big[key][:, :8])), key


def test_distinct_all_free_and_the_neighbours(setup):
    """A forced matrix without a forced column gives the bits of forced=None; `sample`, `beam_search` and
    `sample_distinct(forced=None)` give the same bits before and after a forced call."""
    from singa_amd import smiles
    from singa_amd.model.BeamSearch import beam_search
    from singa_amd.model.Sampling import sample
    z, model, ex = setup
    voc = smi_voc()
    B, T = 2, 16

    def neighbours():
        u = torch.rand(T, B * 4, generator=torch.Generator().manual_seed(3))
        prop = torch.as_tensor(z["prop"][:1]).float()
        tr = {}
        s = sample(model, voc, 4, B, T, ex, prop.repeat(B * 4, 1).to(DEV), device=DEV, uniforms=u, trace=tr)
        bm = beam_search(model, voc, int(z["num_beams"]), B, int(z["max_length"]), int(z["topk"]), ex,
                         torch.as_tensor(z["prop"]).float().to(DEV), device=DEV)
        d = distinct(setup, 6, T, None, grammar=None)
        return s.cpu().numpy(), tr["sum_logp"].cpu().numpy(), bm.cpu().numpy(), d["tokens"], d["gumbel"], d["sum_logp"]

    before = neighbours()
    free = np.full((B, T), -1, np.int64)
    free[:, 0] = voc.index("&")
    a = distinct(setup, 6, T, free, grammar=None)
    for got, want in ((a["tokens"], before[3]), (a["gumbel"], before[4]), (a["sum_logp"], before[5])):
        assert np.array_equal(bits(got), bits(want))
    distinct(setup, 6, T, smiles.encode(["CC", "c1ccc("], voc, T))
    for x, y in zip(before, neighbours()):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(before[2], z["decoded"])
    with pytest.raises(ValueError, match="pocket 1, column 2"):
        distinct(setup, 6, T, smiles.encode(["C", "C)"], voc, T))
    with pytest.raises(ValueError, match="one prefix per pocket"):
        distinct(setup, 6, T, smiles.encode(["C"] * 12, voc, T))


@pytest.mark.parametrize("grammar", [None, "smiles", "valence"])
def test_forced_device_beam_search(setup, grammar):
    from singa_amd import smiles
    from singa_amd.model.BeamSearch import beam_search_device
    from singa_amd.model.Sampling import score
    z, model, ex = setup
    voc = [str(v) for v in smi_voc()]
    eos = voc.index("$")
    capacity = {t: int(c) for t, c in zip(voc, smiles.capacity(voc))}
    B, k, topk, T = 2, 5, 2, 16
    texts = ["c1ccc(", "CC"]
    prefixes = [[voc.index(x) for x in smiles.tokenize(t, voc)] for t in texts]
    forced = smiles.encode(texts, voc, T)
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(B * k, 1).to(DEV)
    runs = []
    for graph in (True, False):
        tr = {}
        out = beam_search_device(model, voc, k, B, T, topk, ex, prop, device=DEV, grammar=grammar, graph=graph, trace=tr, forced=forced)
        runs.append((out.cpu().numpy(), tr))
    (out, tr), (out_e, tr_e) = runs
    assert np.array_equal(out, out_e) and tr["steps"] == tr_e["steps"]
    mols, ended = [], []
    for b in range(B):
        assert len(tr["hyps"][b]) >= 1 and len(tr["hyps"][b]) == len(tr_e["hyps"][b])
        for (s, x), (s_e, x_e), total, total_e in zip(tr["hyps"][b].beams, tr_e["hyps"][b].beams, tr["hyp_sum_logp"][b],
                                                      tr_e["hyp_sum_logp"][b]):
            assert s == s_e and np.array_equal(x, x_e) and TB.bits(total) == TB.bits(total_e)
        mols.append([[int(v) for v in x[1:]] for _, x in tr["hyps"][b].beams])
        for m in mols[b]:
            assert m[:len(prefixes[b])] == prefixes[b], (b, m)
            if grammar is not None:
                text = [voc[v] for v in m]
                assert len(m) <= T - 2 and G.parses(text), "".join(text)
                if grammar == "valence":
                    assert not VR.over_capacity(text, capacity), "".join(text)
    for r, row in enumerate(out):
        if tr["valid"][r]:
            assert list(row[1:1 + len(prefixes[r // topk])]) == prefixes[r // topk]
    # a hypothesis the search ended carries its '$' in the sum: `score`'s bits.  Without a grammar a pocket that is not done
    # at the last step adds its live beams unfinished (T - 1 tokens, no '$'): those are `sample`'s sums with every column forced.
    prop1 = torch.as_tensor(z["prop"][:1]).float()
    keep = [[i for i, m in enumerate(mols[b]) if len(m) <= T - 2] for b in range(B)]
    assert grammar is None or all(len(keep[b]) == len(mols[b]) for b in range(B))
    if any(keep):
        sc = score(model, voc, [[mols[b][i] for i in keep[b]] for b in range(B)], B, ex, prop1, device=DEV, max_length=T, grammar=grammar)
        for b in range(B):
            for n, i in enumerate(keep[b]):
                assert sc["length"][b][n] == len(mols[b][i]) + 1
                assert TB.bits(sc["sum_logp"][b][n]) == TB.bits(tr["hyp_sum_logp"][b][i]), (b, i)
    rest = [[i for i in range(len(mols[b])) if i not in keep[b]] for b in range(B)]
    per = max(len(r) for r in rest)
    if per:
        from singa_amd.model.Sampling import sample
        full = np.full((B * per, T), -1, np.int64)
        full[:, 0], full[:, 1] = voc.index("&"), eos                            # rows without a hypothesis: empty molecules
        for b in range(B):
            for n, i in enumerate(rest[b]):
                assert len(mols[b][i]) == T - 1
                full[b * per + n, 1:] = mols[b][i]
        tr2 = {}
        sample(model, voc, per, B, T, ex, prop1.repeat(B * per, 1).to(DEV), device=DEV, uniforms=torch.zeros(T, B * per), forced=full,
               trace=tr2)
        sums = tr2["sum_logp"].cpu().numpy()
        for b in range(B):
            for n, i in enumerate(rest[b]):
                assert TB.bits(sums[b * per + n]) == TB.bits(tr["hyp_sum_logp"][b][i]), (b, i)
    with pytest.raises(ValueError, match=r"pocket 0, column 2, token '\$'"):
        beam_search_device(model, voc, k, B, T, topk, ex, prop, device=DEV, grammar=grammar, forced=smiles.encode(["C", "C"], voc, T, end=True))


def test_device_beam_search_without_forced_reproduces_the_golden():
    from singa_amd.model.BeamSearch import beam_search_device
    z = golden("beam_b2_k4.npz")
    model, _, _ = build_model(z)
    out = beam_search_device(model, smi_voc(), int(z["num_beams"]), len(z["names"]), int(z["max_length"]), int(z["topk"]),
                             TB.example_from(z), torch.as_tensor(z["prop"]).float().to(DEV), device=DEV, forced=None)
    assert out.shape == z["decoded"].shape and np.array_equal(out.cpu().numpy(), z["decoded"])


# ------------------------------------------------------------------------------------------------ 7: the command line
def gen(*args):
    cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "golden", "--seed", "1", "--max-length", "24", *args]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    return [l for l in r.stdout.decode().splitlines() if not l.startswith("#")]


def test_gen_distinct_with_a_prefix():
    voc = smi_voc()
    per = {}
    for line in gen("--mode", "distinct", "--prefix", "c1ccc(", "--grammar", "smiles", "--num-samples", "6"):
        name, text, length, logp = line.split("\t")
        assert text.startswith("c1ccc(") and G.parses(G.tokenize(text, voc)) and float(logp) <= 0.0, text
        per.setdefault(name, []).append(text)
    assert len(per) == 3 and all(len(t) == 6 and len(set(t)) == 6 for t in per.values()), per


def test_gen_device_beam_with_a_prefix():
    beam = gen("--mode", "beam", "--beam-select", "device", "--num-beams", "5", "--prefix", "c1ccc(", "--grammar", "smiles")
    assert len(beam) == 3 and all(l.split("\t")[1].startswith("c1ccc(") for l in beam)


def test_gen_score_on_a_row_budget(tmp_path):
    from singa_amd import graph as Gr
    names = list(Gr.EXAMPLE_NAMES)
    mols = ["c1ccc(O)cc1", "CCO", "CC(=O)Nc1ccccc1", "C1CC1", "N#Cc1ccccc1", "ClCCBr", "CC(C)C", "c1ccncc1", "OCC(O)CO", "C=CC=C", "CS(C)=O"]
    wanted = [(names[i % 3 if i < 9 else 0], m) for i, m in enumerate(mols)]                # ragged: 5, 3 and 3 molecules
    path = tmp_path / "molecules.tsv"
    path.write_text("\n".join(f"{n}\t{m}" for n, m in wanted) + "\n")
    plain = gen("--mode", "score", "--molecules", str(path))
    assert [l.split("\t")[:2] for l in plain] == [list(w) for w in wanted] and all(float(l.split("\t")[3]) < 0 for l in plain)
    assert gen("--mode", "score", "--molecules", str(path), "--rows-per-pocket", "4") == plain
