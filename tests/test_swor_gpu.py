"""-m gpu: sampling without replacement (`singa_swor_expand` / `_select` / `_follow`, `sample_distinct`, `gen.py --mode
distinct`; include/singa_hip_swor.h states the rule).

Kernel level, a first-order Markov toy model (logits = table[previous token]) driven through `ops.swor_*` against the float64
restatement of the rule (tests/swor_rule.py): a tree smaller than k is exhausted leaf by leaf, k = 8 is the head of k = 32 bit
for bit, and the device's k rows are the rule's k rows.  A pocket of a run is left out of the last comparison only if, in the
rule's own float64 numbers, the k-th and the (k + 1)-th candidate of some step are closer than EPS_G - the device then may
rightly keep the other one.  What EPS_G has to cover is the deviation of the device's fp32 G from the rule's; the test
measures it over all matched rows and asserts EPS_G >= 4 x the largest.  Measured on MI355X (profiles/sampling/
swor_accuracy.txt): 3.3e-7 / 1.02e-6 / 8.3e-7 / 9.5e-7 at V = 2 / 64 / 65 / 117, 1.12e-6 at V = 1024, so EPS_G = 1e-5; phi and sum_logp are held to
the fp32 bound of a V-term log-sum-exp per column (tests/sampling_rule.logp_bound), as in the exhaustion test.

Then the cache move (`swor_follow`) and the write footprint of the three launching entry points between poisoned guard bands
(tests.helpers.Arena, as tests/test_abi_footprint_gpu.py), and `sample_distinct` end to end on the pockets of a beam golden:
distinct well-formed rows whose log-probabilities are `score`'s bit for bit, nesting through the decoder, captured against
eager, streams, the grammar, the neighbouring entry points, and the command line."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import grammar_rule as G
from tests import swor_rule as R
from tests.helpers import Arena, golden, smi_voc
from tests.sampling_rule import logp_bound
from tests.test_beam_gpu import build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS_G = 1e-5            # the next power of ten above 4 x the largest |G_device - G_rule| measured: 4 x 1.12e-6 = 4.5e-6
SEEDS = (1, 2, 3)
NEG = float("-inf")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def new_state(B, k, V, T, sos, pad, grammar=None):
    rows = B * k
    f32 = dict(dtype=torch.float32, device=DEV)
    st = {"gumbel": torch.full((rows,), NEG, **f32), "prop_logp": torch.full((rows,), NEG, **f32), "sum_logp": torch.zeros(rows, **f32),
          "hash": torch.zeros(rows, dtype=torch.int64, device=DEV), "finished": torch.zeros(rows, dtype=torch.uint8, device=DEV),
          "length": torch.zeros(rows, dtype=torch.int32, device=DEV), "tokens": torch.full((rows, T), pad, dtype=torch.int64, device=DEV),
          "tok_logp": torch.zeros(rows, T, **f32), "next": torch.full((rows,), sos, dtype=torch.int64, device=DEV),
          "src": torch.zeros(rows, dtype=torch.int64, device=DEV), "live": torch.ones(B, dtype=torch.int32, device=DEV),
          "cand": torch.empty(rows, V, **f32), "cand_logp": torch.empty(rows, V, **f32), "cand_phi": torch.empty(rows, V, **f32)}
    st["gumbel"].view(B, k)[:, 0] = 0
    st["prop_logp"].view(B, k)[:, 0] = 0
    st["tokens"][:, 0] = sos
    if grammar is not None:
        st["grammar"] = torch.full((rows,), grammar, dtype=torch.int32, device=DEV)
    return st


def words(streams):
    return torch.as_tensor(np.asarray(streams, np.int64).astype(np.uint32).view(np.int32)).to(DEV)


def toy_run(table, k, T, seed, streams, sos, eos, pad, tau=1.0, allowed=None):
    """The toy model through ops.swor_expand / swor_select, T - 1 steps -> the final state as numpy arrays [B, k, ...]."""
    from singa_amd import ops
    V, B = table.shape[0], len(streams)
    st = new_state(B, k, V, T, sos, pad)
    table_d = torch.as_tensor(table).to(DEV)
    al = None if allowed is None else torch.as_tensor(allowed).to(DEV)
    work, strm = ops.swor_work(B * k, T, DEV), words(streams)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    lives = []
    for t in range(T - 1):
        pos.fill_(t + 3)                                               # pos_offset 3: the step is read from the device
        ops.swor_expand(table_d.index_select(0, st["next"]).contiguous(), pos, 3, st, k, strm, tau, seed, pad, al)
        ops.swor_select(pos, 3, st, k, work, eos, pad)
        lives.append(st["live"].clone())
    torch.cuda.synchronize()
    out = {n: v.cpu().numpy().reshape((B, k) + tuple(v.shape[1:])) for n, v in st.items() if n not in ("live", "cand", "cand_logp", "cand_phi")}
    out["hash"] = out["hash"].view(np.uint64)
    out["valid"] = out["gumbel"] > NEG
    out["lives"] = torch.stack(lives).cpu().numpy()
    return out


def toy_vocab(V):
    """(sos, eos, pad, allowed): '&' and '^' are never drawn; V = 2 has no room for them - token 0 doubles as both"""
    if V == 2:
        return 0, 1, 0, None
    allowed = np.ones(V, np.uint8)
    allowed[:2] = 0
    return 0, 2, 1, allowed


def check_invariants(dev, T, pad, eos):
    """what holds for every run: G descending, dead slots trail and are blank, rows distinct, live counted"""
    g, valid = dev["gumbel"], dev["valid"]
    for b in range(g.shape[0]):
        n = int(valid[b].sum())
        assert valid[b, :n].all() and not valid[b, n:].any(), b
        assert (np.diff(g[b, :n]) <= 0).all(), b
        assert (dev["tokens"][b, n:, 1:] == pad).all() and (dev["length"][b, n:] == 0).all() and (dev["finished"][b, n:] == 0).all()
        assert len({tuple(r) for r in dev["tokens"][b, :n]}) == n, b
        assert int(dev["lives"][-1][b]) == int((valid[b] & (dev["finished"][b] == 0)).sum()), b
        for r in range(n):
            row, ln = dev["tokens"][b, r], int(dev["length"][b, r])
            assert (row[ln + 1:] == pad).all() and bool(dev["finished"][b, r]) == (ln > 0 and row[ln] == eos and ln < T), (b, r)


# ---------------------------------------------------------------------------------------------------------------- 1
def test_exhaustion_every_leaf_once():
    sos, eos, pad, allowed = toy_vocab(5)
    V, T, k = 5, 6, 64
    table = R.toy_table(V, 5, sos, eos, pad, scale=1.5)
    streams = [0, 1, 2 ** 32 - 1]
    dev = toy_run(table, k, T, 9, streams, sos, eos, pad, allowed=allowed)
    check_invariants(dev, T, pad, eos)
    bound = logp_bound(V, float(np.abs(table).max())) * T
    t64 = table.astype(np.float64)
    logq = np.where(allowed.astype(bool), t64, -np.inf)
    logq = logq - R.lse(logq)
    logp = t64 - R.lse(t64)
    worst = 0.0
    for b in range(len(streams)):
        n = int(dev["valid"][b].sum())
        assert n == 63                                                  # 31 finished strings over two atoms, 32 of full length
        leaves = set()
        for r in range(n):
            row, ln = dev["tokens"][b, r], int(dev["length"][b, r])
            leaves.add(tuple(row))
            phi = sum(logq[row[c], row[c + 1]] for c in range(ln))
            slp = sum(logp[row[c], row[c + 1]] for c in range(ln))
            worst = max(worst, abs(dev["prop_logp"][b, r] - phi), abs(dev["sum_logp"][b, r] - slp))
            assert abs(dev["prop_logp"][b, r] - phi) <= bound and abs(dev["sum_logp"][b, r] - slp) <= bound, (b, r)
        assert len(leaves) == 63
        total = np.exp(dev["prop_logp"][b, :n].astype(np.float64)).sum()
        assert abs(total - 1.0) <= bound, (b, total)
    print(f"exhaustion: worst |phi - float64| {worst:.3e} (bound {bound:.3e})")


# ---------------------------------------------------------------------------------------------------------------- 2
@pytest.mark.parametrize("V", [64, 65, 117])
def test_nesting_k8_is_the_head_of_k32(V):
    sos, eos, pad, allowed = toy_vocab(V)
    table = R.toy_table(V, V, sos, eos, pad)
    small = toy_run(table, 8, 12, 77, [3, 4], sos, eos, pad, allowed=allowed)
    big = toy_run(table, 32, 12, 77, [3, 4], sos, eos, pad, allowed=allowed)
    check_invariants(small, 12, pad, eos), check_invariants(big, 12, pad, eos)
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp", "hash", "length", "finished"):
        assert np.array_equal(bits(small[key]), bits(big[key][:, :8])), key


# ---------------------------------------------------------------------------------------------------------------- 3
@pytest.mark.parametrize("V", [2, 64, 65, 117])
def test_device_rows_are_the_rules_top_k(V):
    sos, eos, pad, allowed = toy_vocab(V)
    T = 10
    table = R.toy_table(V, 100 + V, sos, eos, pad)
    worst, runs, clear, early = 0.0, 0, 0, 0
    bound = logp_bound(V, float(np.abs(table).max())) * T
    for k in (1, 3, 64, 65, 300):
        for streams in ([7], [1, 2, 2 ** 32 - 1]):
            for seed in SEEDS:
                dev = toy_run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed)
                check_invariants(dev, T, pad, eos)
                want = R.run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed)
                for b in range(len(streams)):
                    runs += 1
                    if want["gap"][b] < EPS_G:
                        continue
                    clear += 1
                    ctx = (V, k, streams[b], seed)
                    n = int(want["valid"][b].sum())
                    assert int(dev["valid"][b].sum()) == n, ctx
                    at = {tuple(r): i for i, r in enumerate(want["tokens"][b, :n])}
                    assert len(at) == n
                    for r in range(n):
                        assert tuple(dev["tokens"][b, r]) in at, (ctx, r)
                        i = at[tuple(dev["tokens"][b, r])]
                        worst = max(worst, abs(float(dev["gumbel"][b, r]) - want["gumbel"][b, i]))
                        assert abs(float(dev["prop_logp"][b, r]) - want["prop_logp"][b, i]) <= bound, (ctx, r)
                        assert abs(float(dev["sum_logp"][b, r]) - want["sum_logp"][b, i]) <= bound, (ctx, r)
                        assert dev["hash"][b, r] == want["hash"][b, i] and dev["length"][b, r] == want["length"][b, i], (ctx, r)
                        assert bool(dev["finished"][b, r]) == bool(want["finished"][b, i]), (ctx, r)
                    early += int((want["finished"][b, :n] & (want["length"][b, :n] < T - 1)).sum())
    print(f"V={V}: {runs} pocket runs, {clear} unambiguous, largest |G_device - G_rule| {worst:.3e}, EPS_G {EPS_G:.0e}")
    assert clear >= 0.9 * runs, (clear, runs)
    assert EPS_G >= 4 * worst, worst
    assert early > 0                                                    # some rows did finish early


@pytest.mark.parametrize("V,k,T", [(300, 65, 6), (1024, 3, 6), (1024, 2048, 4)], ids=["V300-k65", "V1024-k3", "V1024-k2048"])
def test_large_vocabularies_and_the_limits(V, k, T):
    """The instantiations for V > 128 (4, 8 and 16 tokens per lane) and the header's limits - V = 1024, k = 2048, k V = 2^21
    candidates per pocket - against the rule, as above."""
    sos, eos, pad, allowed = toy_vocab(V)
    table = R.toy_table(V, 200 + V, sos, eos, pad)
    streams, seed = ([3, 2 ** 31], 6) if k < 2048 else ([2 ** 31], 6)        # (the rule's 2^21 candidates per pocket take seconds)
    dev = toy_run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed)
    check_invariants(dev, T, pad, eos)
    want = R.run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed)
    bound = logp_bound(V, float(np.abs(table).max())) * T
    worst = 0.0
    assert (want["gap"] >= EPS_G).all(), want["gap"]                     # (chosen on the CPU so that both pockets are unambiguous)
    for b in range(len(streams)):
        n = int(want["valid"][b].sum())
        assert int(dev["valid"][b].sum()) == n == k
        at = {tuple(r): i for i, r in enumerate(want["tokens"][b, :n])}
        for r in range(n):
            i = at[tuple(dev["tokens"][b, r])]
            worst = max(worst, abs(float(dev["gumbel"][b, r]) - want["gumbel"][b, i]))
            assert abs(float(dev["prop_logp"][b, r]) - want["prop_logp"][b, i]) <= bound
            assert abs(float(dev["sum_logp"][b, r]) - want["sum_logp"][b, i]) <= bound
            assert dev["hash"][b, r] == want["hash"][b, i]
    print(f"V={V} k={k}: largest |G_device - G_rule| {worst:.3e}")
    assert EPS_G >= 4 * worst, worst


# ---------------------------------------------------------------------------------------------------------------- 4
def follow_case(pos_value, src, gumbel, finished, pad_row=8, pad_layer=16):
    """caches of row-coded values behind padded row and layer pitches; -> (k, v destination, expected, untouched source)"""
    from singa_amd import ops
    n, R_, H, P, dk, dv = 2, len(src), 4, 256, 32, 64
    out = []
    bufs = {}
    for name, d in (("k", dk), ("v", dv)):
        row, lay = H * P * d + pad_row, R_ * (H * P * d + pad_row) + pad_layer
        for side, fill in (("src", None), ("dst", -1.0)):
            full = torch.full((n * lay + 4,), -2.0, device=DEV)
            view = full[4:].as_strided((n, R_, H, P, d), (lay, row, P * d, d, 1))
            if fill is None:
                view.copy_(torch.arange(n * R_ * H * P * d, dtype=torch.float32).reshape(n, R_, H, P, d) + (0.5 if name == "v" else 0.0))
            else:
                view.fill_(fill)
            bufs[name, side] = (full, view, full.clone())
    pos = torch.tensor([pos_value], dtype=torch.int64, device=DEV)
    ops.swor_follow(bufs["k", "src"][1], bufs["v", "src"][1], bufs["k", "dst"][1], bufs["v", "dst"][1],
                    torch.as_tensor(src, dtype=torch.int64).to(DEV), torch.as_tensor(gumbel, dtype=torch.float32).to(DEV),
                    torch.as_tensor(finished, dtype=torch.uint8).to(DEV), pos)
    torch.cuda.synchronize()
    moved = [r for r in range(R_) if gumbel[r] > NEG and not finished[r]]
    for name in ("k", "v"):
        full_s, view_s, before_s = bufs[name, "src"]
        assert torch.equal(full_s, before_s), (name, "the source changed")
        full_d, view_d, before_d = bufs[name, "dst"]
        want = before_d.clone()
        want_view = want[4:].as_strided(view_d.shape, view_d.stride())
        for r in moved:
            want_view[:, r, :, :pos_value] = view_s[:, src[r], :, :pos_value]
        assert torch.equal(full_d, want), (name, pos_value, "destination: the gather below pos, nothing else")
        out.append(len(moved))
    return out


@pytest.mark.parametrize("pos_value", [0, 1, 63, 64, 255])
def test_follow_moves_the_prefixes(pos_value):
    alive, no = [0.0] * 6, [0] * 6
    assert follow_case(pos_value, [3, 0, 5, 1, 2, 4], alive, no) == [6, 6]                       # a permutation
    assert follow_case(pos_value, [0, 0, 0, 2, 2, 5], alive, no) == [6, 6]                       # duplicates
    assert follow_case(pos_value, [1, 1, 0, 4, 4, 3], [0.0, -1.5, -2.0, -3.0, NEG, NEG], [0, 1, 0, 1, 0, 0]) == [2, 2]   # finished, dead


# ---------------------------------------------------------------------------------------------------------------- 5
def arena_pair(fn):
    """`fn(arena)` under both canaries, as tests.helpers.arena_runs; -> the two reports after the footprint assertions"""
    reps = []
    for canary in ("nan", "big"):
        ar = Arena(DEV, canary, capacity=16 << 20)
        fn(ar)
        reps.append(ar.report())
    for rep in reps:
        assert not rep.stray, ("words outside the promised views changed", rep.stray)
        assert not rep.unwritten, ("promised elements never written", rep.unwritten)
    differ = [n for n in reps[0].bits if not torch.equal(reps[0].bits[n], reps[1].bits[n])]
    assert not differ, ("outputs that depend on what memory held before the call", differ)
    return reps


def mid_run_state(V, k, B, T, steps, grammar=False):
    """the toy model's state after `steps` steps (dense tensors), for the footprint cases"""
    from singa_amd import ops
    sos, eos, pad, allowed = toy_vocab(V)
    table = torch.as_tensor(R.toy_table(V, 31, sos, eos, pad)).to(DEV)
    st = new_state(B, k, V, T, sos, pad)
    work, strm, pos = ops.swor_work(B * k, T, DEV), words(range(B)), torch.zeros(1, dtype=torch.int64, device=DEV)
    al = torch.as_tensor(allowed).to(DEV)
    for t in range(steps):
        pos.fill_(t)
        ops.swor_expand(table.index_select(0, st["next"]).contiguous(), pos, 0, st, k, strm, 1.0, 5, pad, al)
        ops.swor_select(pos, 0, st, k, work, eos, pad)
    pos.fill_(steps)
    return st, table, strm, al, pos, (sos, eos, pad)


def test_footprint_expand_and_select():
    """Both launching entry points of a step on views between poisoned guard bands, after 4 steps of a run (finished and live
    rows, and - k = 40 slots against 3 ^ 4 leaves and less - dead ones too): expand writes cand, cand_logp and cand_phi in full
    and nothing else; select writes the state, next, src and live in full, columns 0 .. t + 1 of tokens / tok_logp, and nothing
    outside `work`.  The results equal the dense ops' bit for bit."""
    from singa_amd import _lib, ops
    V, k, B, T, steps = 5, 40, 2, 9, 4
    st, table, strm, al, pos, (sos, eos, pad) = mid_run_state(V, k, B, T, steps)
    rows = B * k
    fin, dead = st["finished"].bool(), st["gumbel"] == NEG
    assert int(fin.sum()) > 0 and int(dead.sum()) > 0 and int((~fin & ~dead).sum()) > 0
    logits = table.index_select(0, st["next"]).contiguous()
    dense = {n: v.clone() for n, v in st.items()}
    ops.swor_expand(logits, pos, 0, dense, k, strm, 1.0, 5, pad, al)
    after_expand = {n: dense[n].clone() for n in ("cand", "cand_logp", "cand_phi")}
    ops.swor_select(pos, 0, dense, k, ops.swor_work(rows, T, DEV), eos, pad)
    torch.cuda.synchronize()
    lib = _lib.lib()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: ctypes.c_void_p(v.ptr)

    def expand(ar):
        i = {n: ar.view(n, st[n].shape, st[n].dtype, data=st[n]) for n in ("gumbel", "prop_logp", "hash", "finished")}
        lg, a, s, ps = ar.view("logits", logits.shape, data=logits), ar.view("allowed", (V,), torch.uint8, data=al), \
            ar.view("streams", (B,), torch.int32, data=strm), ar.view("pos", (1,), torch.int64, data=pos)
        o = {n: ar.view(n, (rows, V), role="out") for n in ("cand", "cand_logp", "cand_phi")}
        code = lib.singa_swor_expand(p(lg), p(a), None, p(ps), 0, rows, k, V, T, 1.0, 5, p(s), pad, p(i["gumbel"]), p(i["prop_logp"]),
                                     p(i["hash"]), p(i["finished"]), None, p(o["cand"]), p(o["cand_logp"]), p(o["cand_phi"]), stream())
        assert code == 0, lib.singa_last_error_string()

    for rep in arena_pair(expand):
        for n, want in after_expand.items():
            assert torch.equal(rep.out[n].view(torch.int32), want.cpu().view(torch.int32)), n

    cols = torch.arange(T) <= steps + 1
    nbytes = lib.singa_swor_work(rows, T)

    def select(ar):
        c = {n: ar.view(n, (rows, V), data=after_expand[n]) for n in ("cand", "cand_logp", "cand_phi")}
        ps = ar.view("pos", (1,), torch.int64, data=pos)
        s = {n: ar.view(n, st[n].shape, st[n].dtype, data=st[n], role="inout") for n in ("gumbel", "prop_logp", "sum_logp", "hash",
                                                                                        "finished", "length")}
        tk = ar.view("tokens", (rows, T), torch.int64, data=st["tokens"], role="inout", promised=cols)
        tl = ar.view("tok_logp", (rows, T), data=st["tok_logp"], role="inout", promised=cols)
        o = {n: ar.view(n, st[n].shape, st[n].dtype, role="out") for n in ("next", "src", "live")}
        w = ar.view("work", (nbytes,), torch.uint8, role="scratch")
        assert w.ptr % 16 == 0
        code = lib.singa_swor_select(p(c["cand"]), p(c["cand_logp"]), p(c["cand_phi"]), None, p(ps), 0, rows, k, V, T, eos, pad,
                                     p(s["gumbel"]), p(s["prop_logp"]), p(s["sum_logp"]), p(s["hash"]), p(s["finished"]), p(s["length"]),
                                     None, p(tk), p(tl), p(o["next"]), p(o["src"]), p(o["live"]), p(w), stream())
        assert code == 0, lib.singa_last_error_string()

    for rep in arena_pair(select):
        for n in ("gumbel", "prop_logp", "sum_logp", "hash", "finished", "length", "tokens", "tok_logp", "next", "src", "live"):
            got, want = rep.out[n], dense[n].cpu()
            same = torch.equal(got, want) if got.dtype != torch.float32 else torch.equal(got.view(torch.int32), want.view(torch.int32))
            assert same, n


def test_footprint_follow():
    """singa_swor_follow on padded pitches inside an arena: only positions below pos of the rows that are neither dead nor
    finished change in the destination - no pad word, no guard, no source word."""
    from singa_amd import _lib
    lib = _lib.lib()
    n, R_, H, P, dk, dv, pos_value = 2, 5, 4, 16, 32, 64, 9
    src, gumbel, finished = [2, 2, 0, 4, 1], [0.0, -1.0, NEG, -2.0, -3.0], [0, 0, 0, 1, 0]
    moved = torch.tensor([g > NEG and not f for g, f in zip(gumbel, finished)])
    data = {d: torch.arange(n * R_ * H * P * d, dtype=torch.float32).reshape(n, R_, H, P, d) for d in (dk, dv)}

    def call(ar):
        v = {}
        for name, d in (("k", dk), ("v", dv)):
            row, lay = H * P * d + 12, R_ * (H * P * d + 12) + 20
            strides = (lay, row, P * d, d, 1)
            v[name, "s"] = ar.view(name + "_src", (n, R_, H, P, d), strides=strides, data=data[d])
            promised = (moved.view(1, R_, 1, 1, 1) & (torch.arange(P) < pos_value).view(1, 1, 1, P, 1)).expand(n, R_, H, P, d)
            v[name, "d"] = ar.view(name + "_dst", (n, R_, H, P, d), strides=strides, role="out", promised=promised)
            v[name, "ld"] = (row, lay)
        s, g, f, ps = ar.view("src", (R_,), torch.int64, data=torch.tensor(src)), ar.view("gumbel", (R_,), data=torch.tensor(gumbel)), \
            ar.view("finished", (R_,), torch.uint8, data=torch.tensor(finished)), ar.view("pos", (1,), torch.int64, data=torch.tensor([pos_value]))
        pp = lambda x: ctypes.c_void_p(x.ptr)
        code = lib.singa_swor_follow(pp(v["k", "s"]), pp(v["v", "s"]), pp(v["k", "d"]), pp(v["v", "d"]), pp(s), pp(g), pp(f), pp(ps), n, R_,
                                     H, P, dk, dv, v["k", "ld"][0], v["k", "ld"][1], v["v", "ld"][0], v["v", "ld"][1],
                                     ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert code == 0, lib.singa_last_error_string()

    for rep in arena_pair(call):
        for name, d in (("k", dk), ("v", dv)):
            got = rep.out[name + "_dst"]
            for r in range(R_):
                if moved[r]:
                    assert torch.equal(got[:, r, :, :pos_value], data[d][:, src[r], :, :pos_value]), (name, r)


# ---------------------------------------------------------------------------------------------------------------- 6
@pytest.fixture(scope="module")
def setup():
    from tests.test_sampling_gpu import example_of
    z = golden("beam_b2_k6_eos.npz")
    model, sd, _ = build_model(z)
    return z, model, example_of(z)


def distinct(setup, k, T, seed=4, streams=None, graph=True, grammar=None):
    from singa_amd.model.Sampling import sample_distinct
    z, model, ex = setup
    B = len(z["names"])
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(B * k, 1).to(DEV)
    tr = {}
    out = sample_distinct(model, smi_voc(), k, B, T, ex, prop, device=DEV, suppress=("&", "^"), grammar=grammar, seed=seed,
                          streams=streams, graph=graph, trace=tr)
    torch.cuda.synchronize()
    res = {n: v.cpu().numpy().reshape((B, k) + tuple(v.shape[1:])) for n, v in tr.items() if torch.is_tensor(v)}
    res["tokens"], res["steps"] = out.cpu().numpy().reshape(B, k, T), tr["steps"]
    return res


@pytest.fixture(scope="module")
def run48(setup):
    return distinct(setup, 48, 41)


def test_rows_are_distinct_and_scored_as_score_scores_them(setup, run48):
    from singa_amd import smiles
    from singa_amd.model.Sampling import sample, score
    from tests.test_sampling_gpu import well_formed
    z, model, ex = setup
    voc = smi_voc()
    eos = voc.index("$")
    res, B, k, T = run48, len(z["names"]), 48, 41
    assert res["valid"].all()                                           # 116 tokens, 40 columns: the tree has more than 48 leaves
    well_formed(res["tokens"].reshape(B * k, T), res["lengths"].reshape(-1))
    mols, open_rows = [[] for _ in range(B)], []
    for b in range(B):
        assert len({tuple(r) for r in res["tokens"][b]}) == k
        assert (np.diff(res["gumbel"][b]) <= 0).all()
        for r in range(k):
            ln = int(res["lengths"][b, r])
            if res["tokens"][b, r, ln] == eos:
                mols[b].append((r, [int(t) for t in res["tokens"][b, r, 1:ln]]))
            else:
                open_rows.append((b, r))
    assert sum(len(m) for m in mols) > 0                                # (the golden's gains make '$' likely: rows do end)
    prop = torch.as_tensor(z["prop"][:1]).float()
    sc = score(model, voc, [[m for _, m in mb] for mb in mols], B, ex, prop, device=DEV, max_length=T)
    for b in range(B):
        for i, (r, m) in enumerate(mols[b]):
            ln = len(m) + 1
            assert sc["length"][b][i] == ln == res["lengths"][b, r]
            assert bits(np.float32(sc["sum_logp"][b][i])) == bits(res["sum_logp"][b, r]), (b, r)
            assert np.array_equal(bits(sc["token_logp"][b][i]), bits(res["token_logp"][b, r, 1:1 + ln])), (b, r)
    if open_rows:                                                       # rows that reached the last column: every column forced
        forced = np.full((B * k, T), -1, np.int64)
        forced[:, 0] = voc.index("&")
        for b, r in open_rows:
            forced[b * k + r] = res["tokens"][b, r]
        smiles.check_forced(forced, voc, T, None)
        tr = {}
        sample(model, voc, k, B, T, ex, prop.repeat(B * k, 1).to(DEV), device=DEV, uniforms=torch.zeros(T, B * k), forced=forced, trace=tr)
        slp, tlp = tr["sum_logp"].cpu().numpy().reshape(B, k), tr["token_logp"].cpu().numpy().reshape(B, k, T)
        for b, r in open_rows:
            assert bits(slp[b, r]) == bits(res["sum_logp"][b, r]) and np.array_equal(bits(tlp[b, r]), bits(res["token_logp"][b, r])), (b, r)
    print(f"{sum(len(m) for m in mols)} finished rows scored by score(), {len(open_rows)} open rows by forced sampling")


def test_nesting_through_the_decoder(setup):
    small, big = distinct(setup, 8, 20), distinct(setup, 32, 20)
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp", "token_logp", "lengths"):
        assert np.array_equal(bits(small[key]), bits(big[key][:, :8])), key


def test_graph_eager_repeat_and_streams(setup):
    a = distinct(setup, 12, 20, streams=[5, 9])
    for other in (distinct(setup, 12, 20, streams=[5, 9], graph=False), distinct(setup, 12, 20, streams=[5, 9])):
        for key in ("tokens", "gumbel", "prop_logp", "sum_logp"):
            assert np.array_equal(bits(a[key]), bits(other[key])), key
    c = distinct(setup, 12, 20, streams=[5, 10])                        # the neighbour draws from another stream
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp"):
        assert np.array_equal(bits(a[key][0]), bits(c[key][0])), key
    assert not np.array_equal(a["tokens"][1], c["tokens"][1])
    assert not np.array_equal(a["tokens"], distinct(setup, 12, 20, seed=5, streams=[5, 9])["tokens"])


def one_pocket(z, b):
    """pocket b of a beam golden alone, as `example_of` builds the whole batch"""
    from singa_amd.config import Config
    batch, knn = torch.as_tensor(z["batch"]).long(), torch.as_tensor(z["knn"]).long()
    idx = torch.nonzero(batch == b)[:, 0]
    new = torch.full((len(batch),), -1, dtype=torch.long)
    new[idx] = torch.arange(len(idx))
    knn = new[knn[:, (batch[knn[0]] == b) & (batch[knn[1]] == b)]]
    ex = Config()
    ex.protein_element_batch = torch.zeros(len(idx), dtype=torch.long, device=DEV)
    ex.protein_atom_feature, ex.protein_pos = torch.as_tensor(z["feat"]).float()[idx].to(DEV), torch.as_tensor(z["pos"]).float()[idx].to(DEV)
    ex.protein_atom_laplacian, ex.protein_knn = torch.as_tensor(z["lap"]).float()[idx].to(DEV), knn.to(DEV)
    return ex


def test_a_pocket_alone_and_with_another_neighbour(setup):
    """The issue's sense of "its neighbour changes": each pocket run alone (no neighbour, another padding of the encoder's
    batch) and with the pockets swapped, under its own stream.  The pocket's logits then come from another batch shape, so
    the bits may differ: the same molecules in the same order, G within 20 steps x the 1e-5 that tests/sampling_rule.EPS
    allows a device log-probability per step - given that the run's own selection margins are wider than that, which is
    asserted first (a model or seed for which they are not fails there, not by chance)."""
    from singa_amd.model.Sampling import sample_distinct
    from tests.sampling_rule import EPS
    from tests.test_sampling_gpu import example_of
    z, model, _ = setup
    k, T, streams = 12, 20, [5, 9]
    both = distinct(setup, k, T, streams=streams)
    # the margin by which this run's selections were decided: a run with one slot more has the k-slot run as its head, and its
    # slot k + 1 is at least as good as the k-slot run's best loser, so G[k - 1] - G[k] after a step is a lower bound of that
    # step's gap.  Two runs whose G differ by up to T x EPS each can only select differently inside 2 x T x EPS.
    ex, hist = example_of(z), []
    sample_distinct(model, smi_voc(), k + 1, 2, T, ex, torch.as_tensor(z["prop"][:1]).float().repeat(2 * (k + 1), 1).to(DEV),
                    device=DEV, suppress=("&", "^"), seed=4, streams=streams, trace={"gumbel_history": hist})
    g = torch.stack(hist).cpu().numpy().reshape(len(hist), 2, k + 1)
    assert np.array_equal(bits(g[-1][:, :k]), bits(both["gumbel"]))
    margin = np.where(np.isfinite(g[:, :, k]), g[:, :, k - 1] - g[:, :, k], np.inf).min()
    print(f"smallest selection margin of the run: {margin:.3e} (needed: {2 * T * EPS:.1e})")
    assert margin > 2 * T * EPS, margin
    swapped = distinct((z, model, example_of(z, order=[1, 0])), k, T, streams=streams[::-1])
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(k, 1).to(DEV)
    for b in range(2):
        tr = {}
        out = sample_distinct(model, smi_voc(), k, 1, T, one_pocket(z, b), prop, device=DEV, suppress=("&", "^"), seed=4,
                              streams=[streams[b]], trace=tr)
        for tokens, g in ((out.cpu().numpy(), tr["gumbel"].cpu().numpy()), (swapped["tokens"][1 - b], swapped["gumbel"][1 - b])):
            assert np.array_equal(tokens, both["tokens"][b]), b
            assert np.abs(g - both["gumbel"][b]).max() <= T * EPS, b


def test_grammar_rows_end_and_parse(setup):
    voc = smi_voc()
    eos = voc.index("$")
    res = distinct(setup, 24, 24, grammar="smiles")
    assert res["valid"].any(1).all()
    for b in range(res["tokens"].shape[0]):
        rows = [tuple(r) for r, ok in zip(res["tokens"][b], res["valid"][b]) if ok]
        assert len(set(rows)) == len(rows) >= 12
        for row in rows:
            text = G.row_text(row, voc, eos)
            assert text is not None and G.parses(text), row


def test_neighbouring_entry_points_are_unchanged(setup):
    """`sample` and `beam_search` before and after a `sample_distinct` call in the same process: the same tokens."""
    from singa_amd.model.BeamSearch import beam_search
    from singa_amd.model.Sampling import sample
    z, model, ex = setup
    B = len(z["names"])

    def both():
        u = torch.rand(16, B * 4, generator=torch.Generator().manual_seed(3))
        prop = torch.as_tensor(z["prop"][:1]).float()
        tr = {}
        s = sample(model, smi_voc(), 4, B, 16, ex, prop.repeat(B * 4, 1).to(DEV), device=DEV, uniforms=u, trace=tr)
        bm = beam_search(model, smi_voc(), int(z["num_beams"]), B, int(z["max_length"]), int(z["topk"]), ex,
                         torch.as_tensor(z["prop"]).float().to(DEV), device=DEV)
        return s.cpu().numpy(), tr["sum_logp"].cpu().numpy(), bm.cpu().numpy()

    before = both()
    distinct(setup, 8, 12)
    after = both()
    for x, y in zip(before, after):
        assert np.array_equal(bits(x), bits(y))
    assert np.array_equal(before[2], z["decoded"])


def test_sample_distinct_refuses_before_any_launch(setup):
    from singa_amd.model.Sampling import sample_distinct
    z, model, ex = setup
    B = len(z["names"])
    for kw, what in ((dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"), (dict(k=2049), "2048"),
                     (dict(T=300), "k17"), (dict(streams=[1]), "streams")):
        k, T = kw.pop("k", 4), kw.pop("T", 12)
        with pytest.raises(ValueError, match=what):
            sample_distinct(model, smi_voc(), k, B, T, ex, None, device=DEV, **kw)


def test_gen_entry_point_distinct():
    cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "golden", "--mode", "distinct", "--num-samples", "6",
           "--max-length", "24", "--grammar", "smiles", "--temperature", "0.9", "--seed", "2"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    lines = [l for l in r.stdout.decode().splitlines() if not l.startswith("#")]
    per = {}
    for line in lines:
        name, text, length, logp = line.split("\t")
        assert 0 < int(length) <= 23 and float(logp) <= 0.0 and not set(text) & set("&$^")
        per.setdefault(name, []).append(text)
    assert len(per) == 3
    for name, texts in per.items():
        assert len(texts) == 6 and len(set(texts)) == 6, (name, texts)
