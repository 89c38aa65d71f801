"""Grammar-constrained sampling, the part that runs without a GPU: the generation header against its binding table and the
built library, the argument errors of `singa_sample_token_grammar`, the token classes of the shipped vocabulary, the C++ rule
(`singa_smiles_rule_host`: the very inline functions the kernel evaluates) against its numpy restatement on a grid of
states, random walks under the rule against an independent parser, and the argument check of `sample(grammar=...)`."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import grammar_rule as G
from tests.helpers import smi_voc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_gen_table_matches_header_and_library(lib):
    from singa_amd import _capi
    text = open(os.path.join(ROOT, "include", "singa_hip_gen.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_capi.GEN_EXPORTS) == ["singa_sample_token_grammar", "singa_smiles_rule_host"]
    assert not set(_capi.GEN_EXPORTS) & (set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS))
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)


def test_sample_token_grammar_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks
    shape = lib.singa_edge_mlp_fwd(*([p] * 11), 1, 1, 1, 1, None)       # a known SINGA_E_SHAPE
    assert shape not in (0, -1)

    def call(V=116, tau=1.0, top_k=0, top_p=1.0, T=8, eos=3, pad=4, rows=4, logits=p, live=p, cls=p, gstate=p, alp=None):
        return lib.singa_sample_token_grammar(logits, p, None, cls, p, 2, rows, V, T, tau, top_k, top_p, eos, pad, p, p, p, p, p,
                                              live, None, gstate, alp, None)

    for null in (dict(logits=None), dict(live=None), dict(cls=None), dict(gstate=None)):
        assert call(**null) == -1, null
    assert b"sample_token_grammar" in lib.singa_last_error_string()
    for bad in (dict(V=0), dict(V=1025), dict(top_p=0.0), dict(top_p=1.5), dict(tau=-0.5), dict(top_k=-1), dict(T=2), dict(T=1),
                dict(eos=116), dict(pad=-1), dict(tau=float("nan")), dict(top_p=float("nan")), dict(rows=-1)):
        assert call(**bad) == shape, bad
    assert b"sample_token_grammar" in lib.singa_last_error_string()
    assert call(rows=0) == 0 and call(rows=0, T=3, alp=p) == 0           # valid arguments and no rows: nothing to launch
    z = np.zeros(1, np.int32)
    q = z.ctypes.data_as(ctypes.c_void_p)
    assert lib.singa_smiles_rule_host(None, q, q, 1, q, q) == -1 and lib.singa_smiles_rule_host(q, q, q, -1, q, q) == shape
    assert lib.singa_smiles_rule_host(q, q, q, 0, q, q) == 0


def test_classify_the_shipped_vocabulary():
    from singa_amd import smiles
    voc = smi_voc()
    cls = smiles.classify(voc)
    assert cls.dtype == np.uint8 and cls.shape == (116,)
    counts = np.bincount(cls & 15, minlength=8)
    assert counts.tolist() == [2, 96, 5, 1, 1, 9, 1, 1]             # NONE ATOM BOND OPEN CLOSE RING DOT EOS
    assert {voc[i] for i in np.flatnonzero((cls & 15) == smiles.NONE)} == {"&", "^"}
    assert {voc[i] for i in np.flatnonzero((cls & 15) == smiles.BOND)} == {"-", "=", "#", "/", "\\"}
    for i in np.flatnonzero((cls & 15) == smiles.RING):
        assert cls[i] >> 4 == int(voc[i]) - 1
    assert (cls[(cls & 15) != smiles.RING] >> 4 == 0).all()
    assert smiles.classify(["%", ":", "Cl", "[nH]", "X", "0", "[]"]).tolist() == [0, smiles.BOND, smiles.ATOM, smiles.ATOM, 0, 0, 0]
    assert smiles.FRESH == G.FRESH == 7 and smiles.unpack(smiles.pack(5, 63, 0x1ff, 0x155)) == (5, 63, 0x1ff, 0x155)
    assert (smiles.NONE, smiles.ATOM, smiles.BOND, smiles.OPEN, smiles.CLOSE, smiles.RING, smiles.DOT, smiles.EOS, smiles.START,
            smiles.BONDX) == (G.NONE, G.ATOM, G.BOND, G.OPEN, G.CLOSE, G.RING, G.DOT, G.EOS, G.START, G.BONDX)


def test_acceptor_controls():
    for s in G.ACCEPT:
        assert G.parses(s), s
    for s in G.REJECT:
        assert not G.parses(s), s
    assert G.tokenize("C[nH]Cl1", smi_voc()) == ["C", "[nH]", "Cl", "1"] == G.tokenize("C[nH]Cl1")


def test_host_rule_equals_the_restatement_on_the_grid(lib):
    """`ok` and `next_state` of the library's rule against the numpy restatement: all prev codes x depth {0, 1, 2, 62, 63} x all
    512 ring masks x here in {0, ring, ring & 0b101010101, ring & 0b000110011} x rem 0..20 x every class and digit (and the
    class bytes no vocabulary produces: digit index 9, class 8)."""
    tokens = np.array([G.NONE, G.ATOM, G.BOND, G.OPEN, G.CLOSE, G.DOT, G.EOS] + [G.RING | d << 4 for d in range(10)] + [8],
                      np.uint8)
    ring = np.arange(512)
    n = 0
    for prev in range(1, 9):
        for depth in (0, 1, 2, 62, 63):
            for hsel in (0, 0x1ff, 0b101010101, 0b000110011):
                st1 = G.pack(prev, depth, ring, ring & hsel).astype(np.int32)                  # [512]
                st, c, rem = np.meshgrid(st1, tokens, np.arange(21, dtype=np.int32), indexing="ij")
                st, c, rem = (np.ascontiguousarray(a.reshape(-1)) for a in (st, c, rem))
                ok = np.full(st.shape, 7, np.uint8)
                nxt = np.full(st.shape, -1, np.int32)
                vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
                assert lib.singa_smiles_rule_host(vp(c), vp(st), vp(rem), len(st), vp(ok), vp(nxt)) == 0
                want_ok, want_next = G.step(st, c, rem)
                bad = np.flatnonzero((ok != want_ok) | (nxt != want_next))
                assert not len(bad), (prev, depth, hsel, [(int(st[i]), int(c[i]), int(rem[i]), int(ok[i]), int(nxt[i]))
                                                         for i in bad[:5]])
                n += len(st)
    assert n == 8 * 5 * 4 * 512 * 18 * 21


def biased_walks(T, rows, seed, voc, cls):
    """Random walks under the rule, biased towards '(', digits, bonds, ')' and '.': -> token rows [rows, T], and the
    smallest number of allowed tokens seen at any live step."""
    rs = np.random.RandomState(seed)
    w = np.ones(len(voc))
    w[np.isin(cls & 15, (G.BOND, G.OPEN, G.CLOSE, G.RING, G.DOT))] = 12.0
    w[(cls & 15) == G.EOS] = 3.0
    out = np.full((rows, T), voc.index("^"), np.int64)
    out[:, 0] = voc.index("&")
    fewest = len(voc)
    for r in range(rows):
        st = G.FRESH
        for t in range(T - 1):
            m = G.mask(st, cls, T - 2 - t)
            fewest = min(fewest, int(m.sum()))
            if not m.any():
                break
            p = w * m
            tok = int(rs.choice(len(voc), p=p / p.sum()))
            out[r, t + 1] = tok
            if tok == voc.index("$"):
                break
            st = int(G.transition(st, int(cls[tok])))
    return out, fewest


@pytest.mark.parametrize("T,rows", [(3, 200), (4, 200), (5, 200), (12, 300), (41, 150), (201, 25)])
def test_random_walks_end_in_time_and_parse(T, rows):
    from singa_amd import smiles
    voc = smi_voc()
    cls = smiles.classify(voc)
    tokens, fewest = biased_walks(T, rows, T, voc, cls)
    assert fewest >= 1                                              # some token is allowed at every step
    eos = voc.index("$")
    texts = set()
    for row in tokens:
        toks = G.row_text(row, voc, eos)
        assert toks is not None, row                                # '$' by column T - 1
        assert G.parses(toks), "".join(toks)
        texts.add("".join(toks))
    if T >= 12:
        assert any("(" in s for s in texts) and any("1" in s for s in texts) and len(texts) > rows // 2


def test_bondx_case():
    """'(' bond digit: without the BONDX code a digit could follow the bond symbol of a branch (`C(-2`)."""
    from singa_amd import smiles
    voc = smi_voc()
    cls = smiles.classify(voc)
    st = G.FRESH
    for tok in ("C", "(", "-"):
        assert G.mask(st, cls, 30)[voc.index(tok)]
        st = int(G.transition(st, int(cls[voc.index(tok)])))
    assert G.fields(st)[0] == G.BONDX
    m = G.mask(st, cls, 30)
    assert not m[voc.index("2")] and m[voc.index("C")] and {voc[i] for i in np.flatnonzero(m)} == \
        {v for v, c in zip(voc, cls & 15) if c == G.ATOM}


def test_sample_argument_check():
    from singa_amd import smiles
    voc = smi_voc()
    atoms = [v for v, c in zip(voc, smiles.classify(voc) & 15) if c == smiles.ATOM]
    assert smiles.check_arguments(None, voc, 2) is None
    assert np.array_equal(smiles.check_arguments("smiles", voc, 3, ("&", "^")), smiles.classify(voc))
    for kw, what in ((dict(grammar="selfies"), "unknown grammar"), (dict(max_length=2), "max_length"),
                     (dict(voc=[v for v in voc if v != "$"]), r"'\$'"), (dict(suppress=atoms), "atom"),
                     (dict(suppress=("$",)), r"'\$'"), (dict(suppress=(")",)), r"'\)'")):
        args = dict(grammar="smiles", voc=voc, max_length=41, suppress=())
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            smiles.check_arguments(**args)
    smiles.check_arguments("smiles", voc, 41, ("(", ")"))           # both gone: no branches, fine
    smiles.check_arguments("smiles", voc, 41, atoms[1:])            # one atom left


def test_sample_signature_keeps_its_defaults():
    import inspect

    from singa_amd.model.Sampling import sample
    assert inspect.signature(sample).parameters["grammar"].default is None
