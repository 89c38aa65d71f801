"""Valence-aware sampling, the part that runs without a GPU: the valence header against its binding table and the built
library, the argument errors of both entry points, the capacities of the shipped vocabulary, the C++ rule
(`singa_valence_rule_host`: the very inline functions the kernel evaluates) against its numpy restatement
(tests/valence_rule.py) on states reached by random walks and on hand-made edge states, random walks under the rule judged by
the parser of tests/grammar_rule.py and by a graph builder that knows nothing of the rule's state, the same walks under the
plain SMILES rule as the control, and the argument checks of the Python layer."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import grammar_rule as G
from tests import valence_rule as VR
from tests.helpers import smi_voc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def operands(voc):
    """-> (class bytes, capacities, index of '$', token -> capacity) as the host prepares them"""
    from singa_amd import smiles
    cls, cap = smiles.classify_orders(voc), smiles.capacity(voc)
    return cls, cap, voc.index("$"), {t: int(c) for t, c in zip(voc, cap)}


def host_step(lib, st, v0, v1, c, cap, rem):
    """singa_valence_rule_host on flat arrays -> (ok, next state, next word 0, next word 1)"""
    n = len(st)
    st, rem = np.ascontiguousarray(st, np.int32), np.ascontiguousarray(rem, np.int32)
    v = np.ascontiguousarray(np.stack([v0, v1], -1), np.int32)
    c, cap = np.ascontiguousarray(c, np.uint8), np.ascontiguousarray(cap, np.uint8)
    ok, ns, nv = np.full(n, 7, np.uint8), np.full(n, -1, np.int32), np.full((n, 2), -1, np.int32)
    assert lib.singa_valence_rule_host(vp(c), vp(cap), vp(st), vp(v), vp(rem), n, vp(ok), vp(ns), vp(nv)) == 0
    return ok, ns, nv[:, 0], nv[:, 1]


def test_valence_table_matches_header_and_library(lib):
    from singa_amd import _capi
    text = open(os.path.join(ROOT, "include", "singa_hip_valence.h")).read()
    assert "NECESSARY" in text and "aromaticity" in text and "duplicate ring bonds" in text     # the header states its scope
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_capi.VALENCE_EXPORTS) == ["singa_sample_token_valence", "singa_valence_rule_host"]
    others = (_capi.EXPORTS, _capi.LAB_EXPORTS, _capi.GEN_EXPORTS, _capi.FORCE_EXPORTS, _capi.SWOR_EXPORTS, _capi.STREAM_EXPORTS)
    assert not any(set(_capi.VALENCE_EXPORTS) & set(t) for t in others)
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks
    shape = lib.singa_edge_mlp_fwd(*([p] * 11), 1, 1, 1, 1, None)       # a known SINGA_E_SHAPE
    assert shape not in (0, -1)

    def call(V=116, tau=1.0, top_k=0, top_p=1.0, T=8, eos=3, pad=4, rows=4, molecules=0, logits=p, live=p, finished=p, cls=p, cap=p,
             gstate=p, vstate=p, alp=None, mol=None, forced=None, rank=None):
        return lib.singa_sample_token_valence(logits, p, None, cls, cap, p, mol, 2, rows, molecules, V, T, tau, top_k, top_p, eos, pad,
                                              finished, p, p, p, p, live, None, gstate, vstate, alp, forced, rank, None)

    for null in (dict(logits=None), dict(live=None), dict(finished=None), dict(cls=None), dict(gstate=None), dict(cap=None),
                 dict(vstate=None), dict(rank=p)):
        assert call(**null) == -1, null
    assert b"sample_token_valence" in lib.singa_last_error_string()
    for bad in (dict(V=0), dict(V=1025), dict(top_p=0.0), dict(top_p=1.5), dict(tau=-0.5), dict(top_k=-1), dict(T=2), dict(T=1),
                dict(eos=116), dict(pad=-1), dict(tau=float("nan")), dict(top_p=float("nan")), dict(rows=-1),
                dict(mol=p, molecules=0), dict(mol=p, molecules=4, forced=p)):
        assert call(**bad) == shape, bad
    assert b"sample_token_valence" in lib.singa_last_error_string()
    assert call(rows=0) == 0 and call(rows=0, T=3, alp=p, forced=p, rank=p) == 0       # valid arguments and no rows
    assert call(rows=0, mol=p, molecules=4, live=None, finished=None) == 0              # the stream form needs neither
    q = np.zeros(2, np.int32).ctypes.data_as(ctypes.c_void_p)
    for i in range(9):
        if i != 5:
            args = [q] * 5 + [1] + [q] * 3
            args[i] = None
            assert lib.singa_valence_rule_host(*args) == -1, i
    assert lib.singa_valence_rule_host(q, q, q, q, q, -1, q, q, q) == shape
    assert lib.singa_valence_rule_host(q, q, q, q, q, 0, q, q, q) == 0


def test_capacity_of_the_shipped_vocabulary():
    from singa_amd import smiles
    voc = smi_voc()
    cap, cls = smiles.capacity(voc), smiles.classify(voc)
    assert cap.dtype == np.uint8 and cap.shape == (116,) and cap.max() <= 7
    want = {"C": 4, "F": 1, "[nH]": 2, "[N+]": 4, "[O-]": 1, "B": 3, "N": 3, "O": 2, "P": 5, "S": 6, "Cl": 1, "Br": 1, "I": 1, "c": 4,
            "n": 3, "o": 2, "s": 6, "p": 5, "[B-]": 4, "[C-]": 3, "[CH-]": 2, "[C@@H]": 3, "[NH3+]": 1, "[Si]": 4, "[se]": 6,
            "[SeH]": 5, "[As]": 5, "[Na]": 7, "[Fe--]": 7, "[2H]": 7, "[125I]": 1, "[Zn++]": 7, "[S@@+]": 7, "[n-]": 2, "[OH+]": 2}
    assert {t: int(cap[voc.index(t)]) for t in want} == want
    assert (cap[(cls & 15) != smiles.ATOM] == 0).all()
    atoms = np.flatnonzero((cls & 15) == smiles.ATOM)
    assert len(atoms) == 96                                         # every ATOM token gets a value: the table's, or 7
    table = {"B": 3, "C": 4, "Si": 4, "N": 3, "O": 2, "P": 5, "As": 5, "S": 6, "Se": 6, "F": 1, "Cl": 1, "Br": 1, "I": 1}
    for i in atoms:
        el = re.fullmatch(r"\[?\d*([A-Z][a-z]?|se|as|[bcnops]).*", voc[i]).group(1).capitalize()
        assert (cap[i] == 7) if el not in table else (0 <= cap[i] <= 7 and abs(int(cap[i]) - table[el]) <= 3), voc[i]
    assert smiles.capacity(["[Cl-]", "[N+]", "[O-]", "[B-]", "[Si-]", "[C+]", "[CH3-]", "[CH4--]", "[13CH3]", "[Xx]", "[C@@?]", "(", "[N+2]",
                            "[O--]"]).tolist() == [0, 4, 1, 4, 3, 3, 0, 0, 1, 7, 7, 0, 5, 0]
    orders = smiles.classify_orders(voc)
    assert np.array_equal(orders, VR.class_bytes(voc))
    assert [int(orders[voc.index(t)]) >> 4 for t in ("-", "=", "#", "/", "\\")] == [0, 1, 2, 0, 0]
    assert np.array_equal(orders & 15, cls & 15) and np.array_equal(orders[(cls & 15) != smiles.BOND], cls[(cls & 15) != smiles.BOND])
    assert smiles.GRAMMARS == ("smiles", "valence")


EDGE_REM = (0, 5, 30)


def edge_states():
    """hand-made (state, word 0, word 1): depth 9 and 10, nine open rings, att 0 and 7, a START row with garbage"""
    out = []
    for prev in range(1, 9):
        for depth in (0, 1, 9, 10):
            for ring, here in ((0, 0), (1, 1), (0x1ff, 0), (0x1ff, 0x100), (0b100100, 0b100)):
                for att in (0, 1, 7):
                    for pend, first, rord in ((0, 0, 0), (2, 0, 0x1ff), (3, 1, 0b100)):
                        for fill in (0, 7):
                            stack = [fill] * depth
                            if depth and first:
                                stack[-1] = att
                            out.append((G.pack(prev, depth, ring, here),) + VR.vpack(att, pend, first, rord, stack))
    out += [(G.FRESH, 0x7fff, 0x3fffffff), (G.FRESH, -1, -1), (G.FRESH, 0, 0), (G.pack(G.START, 0, 0, 0), 12345, 54321)]
    return np.array(out, np.int64)


def test_host_rule_equals_the_restatement(lib):
    """`ok`, `next_state` and `next_vstate` of the library's rule against the numpy restatement, on every (state, token, rem)
    with the states that random walks reach (both vocabularies, three lengths) x every token of the vocabulary x the rem of
    the walk and a grid of others, and on the hand-made edge states x every token x a rem grid."""
    total = {True: 0, False: 0}
    for voc in (smi_voc(), VR.wide_vocabulary()):
        cls, cap, eos, _ = operands(voc)
        V = len(voc)
        reached = np.concatenate([VR.walks(T, rows, 7 * T, cls, cap, eos, keep_states=True)["states"]
                                  for T, rows in ((5, 30), (12, 40), (41, 32))])
        reached = np.unique(reached, axis=0)
        sets = [(reached, (None, 2, 30))]
        if V == 116:
            sets.append((edge_states(), EDGE_REM))
        for states, rems in sets:
            for rem in rems:
                st, v0, v1 = (np.repeat(states[:, i], V) for i in range(3))
                r = np.repeat(reached[:, 3], V) if rem is None else np.full(len(st), rem)
                c, k = np.tile(cls, len(states)), np.tile(cap, len(states))
                got = host_step(lib, st, v0, v1, c, k, r)
                want = VR.step(st, v0, v1, c, k, r)
                bad = np.flatnonzero(np.any([g != w for g, w in zip(got, want)], 0))
                assert not len(bad), [(hex(int(st[i])), oct(int(v0[i])), oct(int(v1[i])), voc[i % V], int(r[i]),
                                       [int(g[i]) for g in got], [int(w[i]) for w in want]) for i in bad[:5]]
                total[states is not reached] += len(st)
    print(f"{total[False]} (state, token, rem) triples from states the walks reached, {total[True]} from the edge states")
    assert total[False] >= 1_000_000
    # a START row reads its valence words as 0, whatever they hold
    cls, cap, eos, _ = operands(smi_voc())
    c = cls[smi_voc().index("C")]
    a, b = host_step(lib, [G.FRESH] * 2, [0, -1], [0, 0x2aaaaaaa], [c] * 2, [4] * 2, [5] * 2), None
    assert a[0].tolist() == [1, 1] and a[1][0] == a[1][1] and a[2][0] == a[2][1] == 4 and a[3][0] == a[3][1] == 0


WALKS = [(3, 150), (4, 150), (5, 150), (12, 300), (41, 200), (201, 30)]


@pytest.mark.parametrize("vocab", ["V116", "V200"])
@pytest.mark.parametrize("T,rows", WALKS)
def test_random_walks_end_parse_and_hold_capacity(vocab, T, rows):
    voc = smi_voc() if vocab == "V116" else VR.wide_vocabulary()
    cls, cap, eos, capacity = operands(voc)
    w = VR.walks(T, rows, T, cls, cap, eos)
    assert w["fewest"] >= 1                                         # at every live step some token is allowed
    assert w["stuck"] == 0                                          # where '$' is not allowed, some allowed token lowers `need`
    texts = VR.texts_of(w["tokens"], voc, eos)
    for toks in texts:
        assert toks is not None                                     # '$' by column T - 1
        assert G.parses(toks), "".join(toks)
        assert not VR.over_capacity(toks, capacity), ("".join(toks), VR.over_capacity(toks, capacity))
    if T >= 12:
        flat = ["".join(t) for t in texts]
        assert any("(" in s for s in flat) and any("1" in s for s in flat) and any("=" in s for s in flat)
        assert len(set(flat)) > rows // 2
    # the control: the same walks under the plain SMILES rule leave atoms over capacity
    plain = VR.texts_of(VR.walks(T, rows, T, cls, cap, eos, rule="smiles")["tokens"], voc, eos)
    share = np.mean([bool(VR.over_capacity(t, capacity)) for t in plain])
    print(f"{vocab}, T = {T}: {100 * share:.1f} % of the rows of the plain SMILES rule hold an atom over its capacity")
    if T >= 12:
        assert share > 0.2


def test_checker_controls():
    cap = operands(smi_voc())[3]
    assert VR.bond_sums(G.tokenize("C(=O)(C)C1CC1")) == [("C", 4), ("O", 2), ("C", 1), ("C", 3), ("C", 2), ("C", 2)]
    assert VR.bond_sums(G.tokenize("C=1CC1.C#N")) == [("C", 3), ("C", 2), ("C", 3), ("C", 3), ("N", 3)]
    for text, atom in (("F(C)C", 0), ("O(C)(C)C", 0), ("C1CF1", 2), ("C(=O)(=O)(=O)C", 0), ("C=C=1CC=1", 1), ("N#1CC1", 0)):
        over = VR.over_capacity(G.tokenize(text), cap)
        assert over and over[0][0] == atom, (text, over)
    for text in ("O=c1cccc[nH]1", "CS(=O)(=O)N", "C[N+](C)(C)C", "C1CC1(F)F", "C(C)(C)(C)C", "N#CC#N"):
        assert not VR.over_capacity(G.tokenize(text), cap), text


def host_walk(lib, text, voc, T):
    """Walk `text` through the library's rule from the fresh state with rem = T - 2 - t -> the column of the first refused
    token (None: the whole text and its '$' are accepted)"""
    cls, cap, eos, _ = operands(voc)
    s = (G.FRESH, 0, 0)
    toks = G.tokenize(text, voc) + ["$"]
    for t, tok in enumerate(toks):
        i = voc.index(tok)
        ok, st, v0, v1 = host_step(lib, [s[0]], [s[1]], [s[2]], [cls[i]], [cap[i]], [T - 2 - t])
        if not ok[0]:
            return t + 1
        s = (int(st[0]), int(v0[0]), int(v1[0]))
    return None


def test_known_strings(lib):
    """refused at the column at which the atom would go over its capacity (or could no longer be closed), accepted otherwise"""
    voc = smi_voc()
    nest = "C(" * 11 + "C" + ")" * 11
    for text, column in (("F(C)C", 5), ("O(C)(C)C", 8), ("C1CF1", 4), ("C(=O)(=O)(=O)C", 10), ("C#1CC1", 3), (nest, 22),
                         ("F(=O)", 3), ("C=C=1CC=1", 5), ("[NH3+](C)C", 5), ("C1CC1=1", 7)):
        assert host_walk(lib, text, voc, 41) == column, text
    for text in ("O=c1cccc[nH]1", "CS(=O)(=O)N", "C[N+](C)(C)C", "C1CC1(F)F", "C(" * 10 + "C" + ")" * 10, "C=1CC1", "N#CC#N", "F(C)",
                 "C12CC1.C2", "C.C"):
        assert host_walk(lib, text, voc, 41) is None, text
    assert host_walk(lib, "C1CC1", voc, 7) is None and host_walk(lib, "C1CC1", voc, 6) == 4      # no column to spare


def test_check_forced_walks_the_valence_rule(lib):
    """The prefix `F(` alone is NOT refused, and must not be: F has att = 1 and OPEN needs att >= 1, so `F(C)` (fluoromethane)
    is a valid row under the rule as include/singa_hip_valence.h states it.  What is refused is the second bond on F: the last
    C of `F(C)C` (column 5) and the '=' of `F(=` (column 3), both of which the SMILES rule alone lets pass."""
    from singa_amd import smiles
    voc = smi_voc()
    ok = smiles.encode(["C1CC1(F)F", "F(C)"], voc, 41)
    assert np.array_equal(smiles.check_forced(ok, voc, 41, "valence"), ok)
    for text, column, token in (("F(C)C", 5, "C"), ("F(=", 3, "=")):
        f = smiles.encode(["CC", text], voc, 41)
        smiles.check_forced(f, voc, 41, "smiles")                       # the syntax alone lets it pass
        with pytest.raises(ValueError, match=rf"row 1, column {column}, token '{re.escape(token)}'.*valence"):
            smiles.check_forced(f, voc, 41, "valence")
    whole = smiles.encode(["C(=O)(=O)(=O)C"], voc, 41, end=True)
    with pytest.raises(ValueError, match=r"row 0, column 10, token '\('"):
        smiles.check_forced(whole, voc, 41, "valence")


def test_sample_argument_check():
    from singa_amd import smiles
    voc = smi_voc()
    assert np.array_equal(smiles.check_arguments("valence", voc, 3, ("&", "^")), smiles.classify_orders(voc))
    assert np.array_equal(smiles.check_arguments("smiles", voc, 3), smiles.classify(voc))
    cap = smiles.capacity(voc)
    anchors = [v for v, c in zip(voc, cap) if c >= 4]
    with pytest.raises(ValueError, match="capacity >= 4"):
        smiles.check_arguments("valence", voc, 41, anchors)
    with pytest.raises(ValueError, match="capacity >= 4"):
        smiles.check_arguments("valence", [v for v in voc if v not in anchors], 41)
    smiles.check_arguments("valence", voc, 41, anchors[1:])             # one anchor left
    smiles.check_arguments("smiles", voc, 41, anchors)                  # the SMILES rule needs none
    for kw, what in ((dict(max_length=2), "max_length"), (dict(suppress=("$",)), r"'\$'"), (dict(suppress=(")",)), r"'\)'")):
        with pytest.raises(ValueError, match=what):
            smiles.check_arguments(**dict(dict(grammar="valence", voc=voc, max_length=41, suppress=()), **kw))
    with pytest.raises(ValueError, match="unknown grammar.*valence"):
        smiles.check_arguments("selfies", voc, 41)


def test_sample_distinct_refuses_the_valence_grammar():
    """before any device work: neither the model nor the example is touched"""
    from singa_amd.model.Sampling import sample_distinct
    with pytest.raises(ValueError, match="unsupported"):
        sample_distinct(None, smi_voc(), 4, 1, 41, None, grammar="valence")


def test_signatures_keep_their_defaults():
    import inspect

    from singa_amd import ops
    from singa_amd.model import Sampling
    for fn in (Sampling.sample, Sampling.score, Sampling.sample_stream, Sampling.sample_distinct):
        assert inspect.signature(fn).parameters["grammar"].default is None
    for fn in (ops.sample_token, ops.sample_token_stream):
        p = inspect.signature(fn).parameters
        assert p["cap"].default is None and p["vstate"].default is None
