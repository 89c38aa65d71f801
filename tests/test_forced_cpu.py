"""Forced tokens in sampling, the part that runs without a GPU: the header against its binding table and the built library,
the argument errors of `singa_sample_token_forced`, `smiles.tokenize` / `encode` / `check_forced` (the last against the
independent parser of tests/grammar_rule.py on random walks cut at random points), and the refusal of CPU tensors."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import grammar_rule as G
from tests.helpers import smi_voc
from tests.test_grammar_cpu import biased_walks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_force_table_matches_header_and_library(lib):
    from singa_amd import _capi
    text = open(os.path.join(ROOT, "include", "singa_hip_force.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_capi.FORCE_EXPORTS) == ["singa_sample_token_forced"]
    assert not set(_capi.FORCE_EXPORTS) & (set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS) | set(_capi.GEN_EXPORTS))
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)
    for other in ("singa_hip.h", "singa_hip_gen.h", "singa_hip_lab.h"):       # declared in its own header only
        assert "singa_sample_token_forced(" not in re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", other)).read(),
                                                          flags=re.S)


def test_sample_token_forced_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    shape = lib.singa_edge_mlp_fwd(*([p] * 11), 1, 1, 1, 1, None)       # a known SINGA_E_SHAPE
    assert shape not in (0, -1)

    def call(V=116, tau=1.0, top_k=0, top_p=1.0, T=8, eos=3, pad=4, rows=4, logits=p, live=p, cls=p, gstate=p, alp=None,
             forced=p, rank=None):
        return lib.singa_sample_token_forced(logits, p, None, cls, p, 2, rows, V, T, tau, top_k, top_p, eos, pad, p, p, p, p, p,
                                             live, None, gstate, alp, forced, rank, None)

    for null in (dict(logits=None), dict(live=None), dict(forced=None), dict(cls=None), dict(gstate=None),
                 dict(forced=None, cls=None, gstate=None), dict(cls=None, gstate=None, alp=p)):
        assert call(**null) == -1, null
        assert b"sample_token_forced" in lib.singa_last_error_string()
    for gram in (dict(), dict(cls=None, gstate=None)):                  # the shape errors, with and without the grammar
        for bad in (dict(V=0), dict(V=1025), dict(top_p=0.0), dict(top_p=1.5), dict(tau=-0.5), dict(top_k=-1), dict(T=1),
                    dict(eos=116), dict(pad=-1), dict(tau=float("nan")), dict(top_p=float("nan")), dict(rows=-1)):
            assert call(**bad, **gram) == shape, (bad, gram)
        assert b"sample_token_forced" in lib.singa_last_error_string()
    assert call(T=2) == shape and call(T=2, rows=0) == shape            # T = 2: refused with the grammar ...
    assert call(T=2, rows=0, cls=None, gstate=None) == 0                # ... accepted without it
    assert call(rows=0) == 0 and call(rows=0, T=3, alp=p, rank=p) == 0 and call(rows=0, cls=None, gstate=None, rank=p) == 0


# ------------------------------------------------------------------------------------------------ tokenize, encode
def test_tokenize_agrees_with_the_test_tokenizer():
    from singa_amd import smiles
    voc = smi_voc()
    for v in voc:
        assert smiles.tokenize(v, voc) == G.tokenize(v, voc) == [v]
    rs = np.random.RandomState(0)
    for _ in range(500):
        toks = [voc[i] for i in rs.randint(len(voc), size=rs.randint(0, 30))]
        text = "".join(toks)
        assert smiles.tokenize(text, voc) == G.tokenize(text, voc), text
    assert smiles.tokenize("C[nH]Cl1Br", voc) == ["C", "[nH]", "Cl", "1", "Br"] and smiles.tokenize("", voc) == []
    for text, where in (("CC%10", "position 2"), ("CC[NH", "position 2"), ("CCXC", "position 2"), ("C[Xx]", "position 1")):
        with pytest.raises(ValueError, match=where):
            smiles.tokenize(text, voc)


def test_encode_layout_and_limits():
    from singa_amd import smiles
    voc = smi_voc()
    ix = voc.index
    out = smiles.encode(["CCl", ["c", "1"], [ix("N")], ""], voc, 6, end=True)
    assert out.dtype == np.int64 and out.shape == (4, 6)
    assert out.tolist() == [[ix("&"), ix("C"), ix("Cl"), ix("$"), -1, -1], [ix("&"), ix("c"), ix("1"), ix("$"), -1, -1],
                            [ix("&"), ix("N"), ix("$"), -1, -1, -1], [ix("&"), ix("$"), -1, -1, -1, -1]]
    out = smiles.encode(["CCl", ""], voc, 6, end=False)
    assert out.tolist() == [[ix("&"), ix("C"), ix("Cl"), -1, -1, -1], [ix("&"), -1, -1, -1, -1, -1]]
    assert smiles.encode([], voc, 6).shape == (0, 6)
    # the edges: n + 1 <= max_length - 1 with the end token, n <= max_length - 1 without
    assert smiles.encode(["CCCC"], voc, 6, end=True)[0, 5] == ix("$")
    with pytest.raises(ValueError, match="item 1"):
        smiles.encode(["C", "CCCCC"], voc, 6, end=True)
    assert smiles.encode(["CCCCC"], voc, 6, end=False)[0].tolist() == [ix("&")] + [ix("C")] * 5
    with pytest.raises(ValueError, match="item 0"):
        smiles.encode(["CCCCCC"], voc, 6, end=False)
    with pytest.raises(ValueError, match="item 0, token 1"):
        smiles.encode([["C", "Xx"]], voc, 6)
    with pytest.raises(ValueError, match="item 0, token 0"):
        smiles.encode([[116]], voc, 6)


# ------------------------------------------------------------------------------------------------ check_forced
def test_check_forced_controls(lib):
    from singa_amd import smiles
    voc = smi_voc()
    ix = voc.index
    T = 12
    ok = smiles.encode(["", "C", "c1ccc(", "C(=O)"], voc, T)
    for grammar in (None, "smiles"):
        got = smiles.check_forced(ok, voc, T, grammar)
        assert got.dtype == np.int64 and np.array_equal(got, ok)
        smiles.check_forced(smiles.encode(["CC(=O)Nc1ccccc1", ""], voc, 20, end=True), voc, 20, grammar)   # a molecule; an empty row
        free0 = ok.copy()
        free0[:, 0] = -1
        smiles.check_forced(free0, voc, T, grammar)
        smiles.check_forced(np.where(ok < 0, 116, ok), voc, T, grammar)        # any value outside the vocabulary is free
    for text, col, tok in (("C)", 2, r"\)"), ("C11", 3, "1"), ("(", 1, r"\("), ("C(1", 3, "1"), ("C.$", 3, r"\$")):
        bad = smiles.encode(["C", text], voc, T)
        with pytest.raises(ValueError, match=f"row 1, column {col}, token '{tok}'"):
            smiles.check_forced(bad, voc, T, "smiles")
    smiles.check_forced(smiles.encode(["C)", "C11", "("], voc, T), voc, T, None)  # without a grammar only the shape is checked
    # a ring bond closed on the atom after the one that opened it is outside the rule's scope (include/singa_hip_gen.h): syntax only
    smiles.check_forced(smiles.encode(["C1C1"], voc, T), voc, T, "smiles")
    for grammar in (None, "smiles"):
        gap = smiles.encode(["CC", "CCCC"], voc, T)
        gap[1, 2] = -1
        with pytest.raises(ValueError, match="row 1, column 3, token 'C'.*free column 2"):
            smiles.check_forced(gap, voc, T, grammar)
        col0 = smiles.encode(["C", "C"], voc, T)
        col0[1, 0] = ix("C")
        with pytest.raises(ValueError, match="row 1, column 0, token 'C'"):
            smiles.check_forced(col0, voc, T, grammar)
        late = smiles.encode(["C", "C"], voc, T, end=True)
        late[0, 3] = ix("C")
        with pytest.raises(ValueError, match=r"row 0, column 3, token 'C'.*'\$'"):
            smiles.check_forced(late, voc, T, grammar)
        with pytest.raises(ValueError, match="max_length"):
            smiles.check_forced(ok, voc, T + 1, grammar)
        with pytest.raises(ValueError, match="integer"):
            smiles.check_forced(ok.astype(np.float32), voc, T, grammar)
    # 'C(' needs an atom, ')' and '$' behind it: 6 columns hold it, 5 do not
    smiles.check_forced(smiles.encode(["C("], voc, 6), voc, 6, "smiles")
    with pytest.raises(ValueError, match=r"row 0, column 2, token '\('.*2 columns left"):
        smiles.check_forced(smiles.encode(["C("], voc, 5), voc, 5, "smiles")
    smiles.check_forced(smiles.encode(["C("], voc, 5), voc, 5, None)
    with pytest.raises(ValueError, match="unknown grammar"):
        smiles.check_forced(ok, voc, T, "selfies")


@pytest.mark.parametrize("T", [12, 41])
def test_check_forced_agrees_with_the_parser_on_cut_walks(lib, T):
    """2,000 random walks under the rule (1,000 per length), cut at a random point: every such prefix is accepted, and so is
    the whole walk with its '$'; a prefix is then spoiled with one random token, and `check_forced` accepts the result exactly
    if the numpy restatement of the rule does, token by token - and, for whole strings, exactly if the parser does."""
    from singa_amd import smiles
    voc = smi_voc()
    cls = smiles.classify(voc)
    eos = voc.index("$")
    walks, _ = biased_walks(T, 1000, 100 + T, voc, cls)
    rs = np.random.RandomState(T)
    n_tok = np.array([int(np.flatnonzero(w == eos)[0]) - 1 for w in walks])
    cut = np.array([rs.randint(0, n + 1) for n in n_tok])
    pref = np.full_like(walks, -1)
    pref[:, 0] = walks[:, 0]
    for r in range(len(walks)):
        pref[r, 1:1 + cut[r]] = walks[r, 1:1 + cut[r]]
    smiles.check_forced(pref, voc, T, "smiles")                              # every cut prefix
    whole = np.where(np.arange(T)[None, :] <= (n_tok + 1)[:, None], walks, -1)
    smiles.check_forced(whole, voc, T, "smiles")                             # every walk with its '$'
    accepted = refused = 0
    for r in range(len(walks)):
        if cut[r] == 0:
            continue
        row = pref[r:r + 1].copy()
        at = rs.randint(1, cut[r] + 1)
        row[0, at] = rs.choice(np.flatnonzero((cls & 15) != G.NONE))
        st, want = G.FRESH, True
        for t in range(0 if cut[r] == 1 and row[0, 1] == eos else cut[r]):      # '$' alone: the empty row `score` pads with
            c = int(cls[row[0, t + 1]])
            if not G.allows(st, c, T - 2 - t) or (c & 15) == G.EOS and t + 1 < cut[r]:
                want = False
                break
            st = int(G.transition(st, c))
        try:
            smiles.check_forced(row, voc, T, "smiles")
            got = True
        except ValueError:
            got = False
        assert got == want, (r, [voc[i] for i in row[0, 1:1 + cut[r]]])
        accepted += got
        refused += not got
    # whole strings, spoiled or not, against the parser: accepted with '$' exactly if they parse (and fit)
    for r in range(0, len(walks), 4):
        toks = [voc[i] for i in walks[r, 1:1 + n_tok[r]]]
        if rs.rand() < 0.5 and len(toks) > 1:
            toks[rs.randint(len(toks))] = voc[rs.choice(np.flatnonzero((cls & 15) != G.NONE))]
        if "$" in toks:
            continue
        try:
            smiles.check_forced(smiles.encode([toks], voc, T, end=True), voc, T, "smiles")
            got = True
        except ValueError:
            got = False
        assert got == G.parses(toks), "".join(toks)
    print(f"T={T}: {accepted} spoiled prefixes accepted, {refused} refused")
    assert accepted > 50 and refused > 50


def test_sample_and_score_refuse_cpu_tensors():
    import torch

    from singa_amd import smiles
    from singa_amd.config import Config
    from singa_amd.model import Sampling
    voc = smi_voc()
    ex = Config()
    ex.protein_atom_feature = torch.zeros(4, 8)
    forced = smiles.encode(["C"], voc, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.sample(None, voc, 1, 1, 8, ex, device="cuda", forced=forced)
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.sample(None, voc, 1, 1, 8, ex, device="cpu", forced=forced)
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.score(None, voc, [["CC"]], 1, ex, device="cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.score(None, voc, [["CC"]], 1, ex, device="cpu")
