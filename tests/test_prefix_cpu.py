"""Forced tokens in `sample_stream`, `sample_distinct` and `beam_search_device` (include/singa_hip_prefix.h), the part that runs
without a GPU: the header against its binding table and the built library, the argument errors of the three entry points,
`smiles.check_prefix`, the float64 restatement of the forced stochastic-beam rule (tests/prefix_rule.py) against
tests/swor_rule.py and by exhaustion of a small tree, the forced beam rule as `beam_rule.Search.expand` with one-hot masks on
whole searches, and gen.py's argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import beam_rule as BR
from tests import prefix_rule as PR
from tests import swor_rule as R
from tests.helpers import smi_voc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["singa_forced_beam_expand", "singa_sample_token_stream_forced", "singa_swor_expand_forced"]
NULL, SHAPE = -1, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_prefix_table_matches_header_and_library(lib):
    from singa_amd import _capi
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", strip("singa_hip_prefix.h"))))
    assert declared == sorted(_capi.PREFIX_EXPORTS) == NAMES
    tables = [n for n in dir(_capi) if n.endswith("EXPORTS") and n != "PREFIX_EXPORTS"]
    assert len(tables) >= 9                                                    # EXPORTS, LAB, GEN, FORCE, SWOR, STREAM, VALENCE, BEAM, UNITS
    for name in tables:
        assert not set(_capi.PREFIX_EXPORTS) & set(getattr(_capi, name)), name
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):            # declared in its own header only
        if other != "singa_hip_prefix.h":
            text = strip(other)
            assert not any(re.search(r"\b%s\b" % n, text) for n in NAMES), other
    import __graft_entry__
    assert "singa_hip_prefix.h" in open(__graft_entry__.__file__).read()       # a dependency of the build


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    err = lambda: lib.singa_last_error_string()

    def choice(rows=4, M=8, V=116, T=8, tau=1.0, top_k=0, top_p=1.0, eos=3, pad=4, logits=p, mol=p, pos=p, cls=None, cap=None,
               gstate=None, vstate=None, alp=None, tokens=p, length=p, forced=p, rank=None):
        return lib.singa_sample_token_stream_forced(logits, p, None, cls, cap, pos, mol, 1, rows, M, V, T, tau, top_k, top_p, eos, pad,
                                                    length, p, tokens, p, None, gstate, vstate, alp, forced, rank, None)

    for null in (dict(forced=None), dict(forced=None, rank=p), dict(logits=None), dict(mol=None), dict(pos=None), dict(tokens=None),
                 dict(length=None), dict(cls=p), dict(gstate=p), dict(alp=p), dict(cls=p, gstate=p, cap=p), dict(cls=p, gstate=p, vstate=p),
                 dict(cap=p, vstate=p)):
        assert choice(**null) == NULL, null
        assert b"sample_token_stream_forced" in err()
    for bad, word in ((dict(V=0), b"vocabulary"), (dict(V=1025), b"vocabulary"), (dict(T=1), b"T >= 2"),
                      (dict(T=2, cls=p, gstate=p), b"T >= 2"), (dict(M=0), b"molecules"), (dict(eos=116), b"eos"), (dict(pad=-1), b"pad"),
                      (dict(rows=-1), b"T >= 2"), (dict(tau=-1.0), b"temperature"), (dict(top_k=-1), b"top_k"), (dict(top_p=0.0), b"top_p")):
        assert choice(**bad) == SHAPE, bad
        assert b"sample_token_stream_forced" in err() and word in err(), (bad, err())
    assert choice(rows=0) == 0 and choice(rows=0, V=1024, T=2) == 0 and choice(rows=0, T=3, cls=p, gstate=p) == 0
    assert choice(rows=0, rank=p) == 0 and choice(rows=0, T=3, cls=p, gstate=p, alp=p, rank=p) == 0     # rank is optional
    assert choice(rows=0, T=3, cls=p, gstate=p, cap=p, vstate=p) == 0 and choice(rows=0, T=3, cls=p, gstate=p, cap=p, vstate=p, rank=p) == 0

    def swor(rows=4, k=2, V=116, T=8, tau=1.0, pad=4, logits=p, cls=None, gstate=None, cand=p, streams=p, forced=p):
        return lib.singa_swor_expand_forced(logits, None, cls, p, 1, rows, k, V, T, tau, 7, streams, pad, p, p, p, p, gstate, cand, p, p,
                                            forced, None)

    def beam(rows=4, k=2, V=116, T=8, logits=p, cls=None, cap=None, gstate=None, vstate=None, cand=p, done=p, forced=p):
        return lib.singa_forced_beam_expand(logits, None, cls, cap, p, 1, rows, k, V, T, p, gstate, vstate, done, cand, forced, None)

    for call, name, kmax in ((swor, b"swor_expand_forced", 2048), (beam, b"forced_beam_expand", 1024)):
        for null in (dict(forced=None), dict(cand=None), dict(logits=None), dict(cls=p), dict(gstate=p)):
            assert call(**null) == NULL, (name, null)
            assert name in err()
        for bad in (dict(V=0), dict(V=1025), dict(k=0), dict(k=kmax + 1, rows=kmax + 1), dict(rows=5), dict(rows=-2), dict(T=1),
                    dict(T=2, cls=p, gstate=p)):
            assert call(**bad) == SHAPE, (name, bad)
            assert name in err()
        assert call(rows=0) == 0 and call(rows=0, k=kmax, V=1024, T=2) == 0 and call(rows=0, T=3, cls=p, gstate=p) == 0
        assert call(rows=0, forced=None) == NULL                                                    # before the rows are looked at
    assert swor(streams=None) == NULL and swor(pad=116) == SHAPE and swor(pad=-1) == SHAPE
    for tau in (0.0, -1.0, float("nan")):
        assert swor(tau=tau) == SHAPE and b"temperature" in err()
    for null in (dict(cls=p, gstate=p, vstate=p), dict(cls=p, gstate=p, cap=p), dict(cap=p, vstate=p), dict(done=None)):
        assert beam(**null) == NULL, null
    assert beam(T=2, cls=p, gstate=p, cap=p, vstate=p) == SHAPE and beam(rows=0, T=3, cls=p, gstate=p, cap=p, vstate=p) == 0


# ------------------------------------------------------------------------------------------------ check_prefix
def test_check_prefix_controls(lib):
    from singa_amd import smiles
    voc = smi_voc()
    T = 12
    ok = smiles.encode(["", "C", "c1ccc("], voc, T)
    for grammar in (None, "smiles", "valence"):
        got = smiles.check_prefix(ok, voc, 3, T, grammar)
        assert got.dtype == np.int64 and got.flags["C_CONTIGUOUS"] and np.array_equal(got, ok)
        smiles.check_prefix(np.where(ok < 0, 116, ok), voc, 3, T, grammar)     # any value outside the vocabulary is free
        with pytest.raises(ValueError, match=r"pocket 1, column 2, token '\$'"):
            smiles.check_prefix(np.stack([ok[1], smiles.encode(["C"], voc, T, end=True)[0]]), voc, 2, T, grammar)
        with pytest.raises(ValueError, match=r"pocket 0, column 1, token '\$'"):    # `score`'s empty row is no prefix either
            smiles.check_prefix(smiles.encode([""], voc, T, end=True), voc, 1, T, grammar)
        gap = smiles.encode(["CC", "CCCC"], voc, T)
        gap[1, 2] = -1
        with pytest.raises(ValueError, match="pocket 1, column 3, token 'C'.*free column 2"):
            smiles.check_prefix(gap, voc, 2, T, grammar)
        for shape_of in (ok[:2], ok[:, :T - 1], ok[0], ok.astype(np.float32)):
            with pytest.raises(ValueError, match="one prefix per pocket"):
                smiles.check_prefix(shape_of, voc, 3, T, grammar)
    # no room left: every column behind '&' forced
    full = smiles.encode(["C" * 11], voc, T)
    with pytest.raises(ValueError, match="pocket 0, column 11, token 'C'.*no free column"):
        smiles.check_prefix(full, voc, 1, T, None)
    smiles.check_prefix(smiles.encode(["C" * 10], voc, T), voc, 1, T, None)   # one free column is enough without a grammar ...
    with pytest.raises(ValueError, match=r"pocket 0, column 10, token '\('"):  # ... under one the branch and the '$' need theirs
        smiles.check_prefix(smiles.encode(["C" * 9 + "("], voc, T), voc, 1, T, "smiles")
    # a token the rule refuses, and a prefix that cannot be finished in the columns left
    for text, col, tok in (("C)", 2, r"\)"), ("C11", 3, "1"), ("(", 1, r"\(")):
        for grammar in ("smiles", "valence"):
            with pytest.raises(ValueError, match=f"pocket 1, column {col}, token '{tok}'"):
                smiles.check_prefix(smiles.encode(["C", text], voc, T), voc, 2, T, grammar)
        smiles.check_prefix(smiles.encode(["C", text], voc, T), voc, 2, T, None)
    with pytest.raises(ValueError, match="pocket 0, column 5, token 'C'.*valence"):      # F(C)C: fluorine has one bond
        smiles.check_prefix(smiles.encode(["F(C)C"], voc, T), voc, 1, T, "valence")
    smiles.check_prefix(smiles.encode(["F(C)C"], voc, T), voc, 1, T, "smiles")
    with pytest.raises(ValueError, match=r"pocket 0, column 2, token '\('.*2 columns left"):
        smiles.check_prefix(smiles.encode(["C("], voc, 5), voc, 1, 5, "smiles")
    smiles.check_prefix(smiles.encode(["C("], voc, 6), voc, 1, 6, "smiles")
    with pytest.raises(ValueError, match="unknown grammar"):
        smiles.check_prefix(ok, voc, 3, T, "selfies")


# ------------------------------------------------------------------------------------------------ the forced stochastic-beam rule
def toy(V):
    allowed = np.ones(V, np.uint8)
    allowed[:2] = 0
    return 0, 2, 1, allowed                                                    # sos, eos, pad: as tests/test_swor_gpu.toy_vocab


def test_all_free_is_the_unforced_rule_exactly():
    for V, k, T, seed, streams in ((9, 7, 6, 11, [5, 6]), (64, 3, 10, 2, [1, 2, 2 ** 32 - 1]), (5, 64, 6, 9, [0])):
        sos, eos, pad, allowed = toy(V)
        table = R.toy_table(V, V, sos, eos, pad)
        want = R.run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed)
        for forced in (None, np.full((len(streams), T), -1), np.full((len(streams), T), V)):
            got = PR.run(table, k, T, seed, streams, sos, eos, pad, allowed=allowed, forced=forced)
            for key, a in want.items():
                assert np.array_equal(a, got[key]), (V, key)


def test_G_and_phi_stay_zero_through_a_prefix():
    V, k, T = 9, 7, 8
    sos, eos, pad, allowed = toy(V)
    table = R.toy_table(V, 3, sos, eos, pad)
    prefixes = [[3, 4, 5], [], [0, 7]]                                         # token 0 is one `allowed` would refuse
    forced = PR.prefix_matrix(prefixes, T, sos)
    out = PR.run(table, k, T, 11, [5, 6, 7], sos, eos, pad, allowed=allowed, forced=forced)
    for b, p in enumerate(prefixes):
        for t in range(len(p)):
            G, phi = out["history"][t]
            assert G[b, 0] == 0.0 and phi[b, 0] == 0.0 and not np.isfinite(G[b, 1:]).any(), (b, t)     # exactly: one live slot
        if p:
            G, _ = out["history"][len(p)]
            assert np.isfinite(G[b]).sum() > 1 and (G[b][np.isfinite(G[b])] <= 0).all()
        n = int(out["valid"][b].sum())
        assert n == k and (out["tokens"][b, :n, 1:1 + len(p)] == np.array(p, np.int64)).all()
    free = PR.run(table, k, T, 11, [6], sos, eos, pad, allowed=allowed)
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp"):                  # the pocket without a prefix: the unforced run
        assert np.array_equal(out[key][1], free[key][0]), key


@pytest.mark.parametrize("prefix,leaves", [([3, 4], 15), ([4], 31)])
def test_exhaustion_under_a_prefix(prefix, leaves):
    """The toy tree of tests/test_swor_gpu.py::test_exhaustion_every_leaf_once (V = 5, T = 6, three drawable tokens, k = 64)
    under a prefix of n tokens: 2 ^ (5 - n) - 1 strings that end early and 2 ^ (5 - n) of full length remain... counted with
    '$' as one of the three: sum over the free columns.  Each leaf once, proposal mass 1 - conditional on the prefix."""
    sos, eos, pad, allowed = toy(5)
    V, T, k = 5, 6, 64
    table = R.toy_table(V, 5, sos, eos, pad, scale=1.5)
    out = PR.run(table, k, T, 9, [0, 1, 2 ** 32 - 1], sos, eos, pad, allowed=allowed, forced=PR.prefix_matrix([prefix] * 3, T, sos))
    t64 = table.astype(np.float64)
    logq = np.where(allowed.astype(bool), t64, -np.inf)
    logq = logq - R.lse(logq)
    for b in range(3):
        n = int(out["valid"][b].sum())
        assert n == leaves
        rows = out["tokens"][b, :n]
        assert len({tuple(r) for r in rows}) == n and (rows[:, 1:1 + len(prefix)] == prefix).all()
        assert abs(np.exp(out["prop_logp"][b, :n]).sum() - 1.0) < 1e-12
        for r in range(n):
            ln = int(out["length"][b, r])
            phi = sum(logq[rows[r, c], rows[r, c + 1]] for c in range(len(prefix), ln))     # the free columns alone
            assert abs(out["prop_logp"][b, r] - phi) < 1e-12


# ------------------------------------------------------------------------------------------------ the forced beam rule
@pytest.mark.parametrize("grammar", [None, "smiles", "valence"])
def test_forced_beam_searches_keep_the_prefix(grammar):
    from singa_amd import smiles
    voc = [str(v) for v in smi_voc()]
    V, sos, eos, pad = len(voc), voc.index("&"), voc.index("$"), voc.index("^")
    cls = None if grammar is None else smiles.classify_orders(voc) if grammar == "valence" else smiles.classify(voc)
    cap = smiles.capacity(voc) if grammar == "valence" else None
    B, T = 3, 12
    prefixes = [smiles.tokenize(x, voc) for x in ("c1ccc(", "", "CC")]
    forced = smiles.encode(["c1ccc(", "", "CC"], voc, T)
    stored = 0
    for k in (1, 3, 6):
        rs = np.random.RandomState(k)
        run = BR.Search(B, k, V, T, sos, eos, pad, cls=cls, cap=cap)
        for t in range(T - 1):
            z = rs.randn(B * k, V).astype(np.float32)
            z[:, eos] += rs.choice([-2.0, 3.0], size=B * k)
            run.select(run.expand(z, PR.beam_masks(run, forced)))
            run.t += 1
            for b, p in enumerate(prefixes):
                if t < len(p):                                                 # one live slot through the prefix
                    assert run.live[b] == 1 and (run.score[b, 1:] == BR.NEG).all() and run.score[b, 0] > BR.NEG, (k, b, t)
                    assert len(run.hyps[b].items) == 0
                live = run.score[b] > BR.NEG
                n = min(t + 1, len(p))
                assert (run.tokens[b, live, 1:1 + n] == [voc.index(x) for x in p[:n]]).all(), (k, b, t)
        run.finish()
        for b, p in enumerate(prefixes):
            assert len(run.hyps[b].items) >= 1
            for score, total, toks, stamp in run.hyps[b].items:
                assert [voc[x] for x in toks[1:1 + len(p)]] == p, (k, b)
                stored += 1
                if grammar is not None:
                    from tests import grammar_rule as G
                    assert G.parses([voc[x] for x in toks[1:]])
    assert stored > 9


# ------------------------------------------------------------------------------------------------ the entry points, the command line
def test_entry_points_refuse_cpu_tensors_and_bad_prefixes_first():
    import torch

    from singa_amd import smiles
    from singa_amd.config import Config
    from singa_amd.model import BeamSearch, Sampling
    voc = smi_voc()
    ex = Config()
    ex.protein_atom_feature = torch.zeros(4, 8)
    forced = smiles.encode(["C"], voc, 8)
    for fn in (Sampling.sample_distinct, Sampling.sample_stream):
        with pytest.raises(RuntimeError, match="GPU only"):
            fn(None, voc, 2, 1, 8, ex, device="cuda", forced=forced)
    with pytest.raises(RuntimeError, match="GPU only"):
        BeamSearch.beam_search_device(None, voc, 2, 1, 8, 1, ex, device="cuda", forced=forced)
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.score(None, voc, [["CC"]], 1, ex, device="cuda", rows_per_pocket=4)
    with pytest.raises(ValueError, match="valence"):                           # as before: pinned by tests/test_valence_cpu.py
        Sampling.sample_distinct(None, voc, 2, 1, 8, ex, device="cuda", grammar="valence", forced=forced)


def test_gen_argument_checks():
    import gen
    a = gen.parse_args(["--mode", "distinct", "--prefix", "c1ccc(", "--grammar", "smiles"])
    assert a.prefix == "c1ccc(" and a.mode == "distinct"
    assert gen.parse_args(["--mode", "beam", "--beam-select", "device", "--prefix", "CC"]).prefix == "CC"
    assert gen.parse_args(["--mode", "beam", "--grammar", "valence", "--prefix", "CC"]).prefix == "CC"
    a = gen.parse_args(["--mode", "sample", "--rows-per-pocket", "8", "--prefix", "CC"])
    assert a.rows_per_pocket == 8 and a.prefix == "CC"
    assert gen.parse_args(["--mode", "score", "--molecules", "x.tsv", "--rows-per-pocket", "4"]).rows_per_pocket == 4
    for argv, word in ((["--mode", "beam", "--prefix", "CC"], "--beam-select device"),
                       (["--mode", "score", "--molecules", "x.tsv", "--prefix", "CC"], "--prefix"),
                       (["--mode", "distinct", "--rows-per-pocket", "4"], "--rows-per-pocket"),
                       (["--mode", "beam", "--rows-per-pocket", "4"], "--rows-per-pocket")):
        with pytest.raises(SystemExit):
            gen.parse_args(argv)
    for word in ("--prefix", "--rows-per-pocket", "singa_hip_prefix.h"):
        assert word in gen.__doc__
