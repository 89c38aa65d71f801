"""-m gpu: the row front end that `sample_token_kernel`, `swor_expand_kernel` and `beam_expand_kernel` share (RowFront in
singa_amd/csrc/singa_hip.hip), at kernel level: the same seeded logits through `ops.sample_token` (forced), `ops.swor_expand`
and `ops.beam_expand`.

What the public contract rests on - a beam hypothesis' sum and a `sample_distinct` row's sum are what `score(...)` reports - is
that every consumer's z - lse carries the same bits, and that all three see the same effective mask.  R = 5 rows (two
workgroups, the second partly filled), T = 4 at step 0, one slot per pocket, beam score 0 and swor gumbel / prop_logp 0, so that
beam's cand and swor's cand_logp are the bare z - lse.

`allowed_logp` is compared with float64 to a relative 1e-5.  Its fp32 error is absolute - two roundings at the magnitude of
lse, two logf - so a relative bound only means something where the value is not close to 0: the `allowed` mask of the rule
cases leaves out every row's best token, and the logits are redrawn (judged by the float64 numbers alone) until every
non-empty mask's log-mass is below -0.25."""
import ctypes

import numpy as np
import pytest
import torch

from tests import grammar_rule as G
from tests import valence_rule as VR
from tests.helpers import smi_voc
from tests.test_grammar_gpu import wide

pytestmark = pytest.mark.gpu
DEV = "cuda"
R, T = 5, 4
REM = T - 2                                                         # step 0: columns left after the token


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def beam_cand(z, allowed, cls=None, cap=None, gstate=None, vstate=None, T=T):
    from singa_amd import ops
    V = z.shape[1]
    st = {"score": torch.zeros(R, device=DEV), "done": torch.zeros(R, dtype=torch.uint8, device=DEV),
          "tokens": torch.zeros(R, T, dtype=torch.int64, device=DEV), "cand": torch.full((R, V), 7.0, device=DEV)}
    if cls is not None:
        st["grammar"] = dev(gstate.astype(np.int32))
    if cap is not None:
        st["vstate"] = dev(vstate.astype(np.int32))
    ops.beam_expand(dev(z), torch.zeros(1, dtype=torch.int64, device=DEV), 0, st, 1, None if allowed is None else dev(allowed),
                    None if cls is None else dev(cls), None if cap is None else dev(cap))
    return st["cand"].cpu().numpy()


def swor_cand_logp(z, allowed, cls=None, gstate=None, T=T):
    from singa_amd import ops
    V = z.shape[1]
    st = {"gumbel": torch.zeros(R, device=DEV), "prop_logp": torch.zeros(R, device=DEV),
          "hash": torch.arange(R, dtype=torch.int64, device=DEV), "finished": torch.zeros(R, dtype=torch.uint8, device=DEV),
          "tokens": torch.zeros(R, T, dtype=torch.int64, device=DEV)}
    st.update({n: torch.full((R, V), 7.0, device=DEV) for n in ("cand", "cand_logp", "cand_phi")})
    if cls is not None:
        st["grammar"] = dev(gstate.astype(np.int32))
    ops.swor_expand(dev(z), torch.zeros(1, dtype=torch.int64, device=DEV), 0, st, 1, torch.arange(R, dtype=torch.int32, device=DEV),
                    1.0, 11, 0, None if allowed is None else dev(allowed), None if cls is None else dev(cls))
    return st["cand_logp"].cpu().numpy()


def sampled(z, allowed, forced=None, cls=None, cap=None, gstate=None, vstate=None, T=T):
    """one `ops.sample_token` launch at step 0 -> (tok_logp[:, 1], allowed_logp[:, 1] or None)"""
    from singa_amd import ops
    st = {"tokens": torch.zeros(R, T, dtype=torch.int64, device=DEV), "next": torch.zeros(R, dtype=torch.int64, device=DEV),
          "finished": torch.zeros(R, dtype=torch.uint8, device=DEV), "length": torch.zeros(R, dtype=torch.int32, device=DEV),
          "sum_logp": torch.zeros(R, device=DEV), "live": torch.full((1,), R, dtype=torch.int32, device=DEV),
          "tok_logp": torch.full((R, T), 9.0, device=DEV)}
    if cls is not None:
        st["grammar"], st["allowed_logp"] = dev(gstate.astype(np.int32)), torch.full((R, T), 9.0, device=DEV)
    f = None
    if forced is not None:
        f = torch.full((R, T), -1, dtype=torch.int64, device=DEV)
        f[:, 1] = dev(np.asarray(forced, np.int64))
    ops.sample_token(dev(z), torch.full((T, R), 0.5, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV), 0, st, 1.0, 0, 1.0,
                     0, 0, None if allowed is None else dev(allowed), None if cls is None else dev(cls), f,
                     None if cap is None else dev(cap), None if cap is None else dev(vstate.astype(np.int32)))
    alp = st["allowed_logp"][:, 1].cpu().numpy() if cls is not None else None
    return st["tok_logp"][:, 1].cpu().numpy(), alp


# ---------------------------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("V", [2, 64, 65, 116, 129, 1024])         # every NPL; for NPL 2 and 4 the lane edges i < V
def test_z_minus_lse_carries_the_same_bits_in_all_three(V):
    rs = np.random.RandomState(V)
    z = (2.5 * rs.randn(R, V)).astype(np.float32)
    allowed = np.ones(V, np.uint8)
    allowed[rs.choice(V, min(3, V - 1), replace=False)] = 0
    beam, swor = beam_cand(z, allowed), swor_cand_logp(z, allowed)
    assert np.array_equal(bits(beam), bits(swor))                   # every row and token, the -inf pattern included
    assert np.array_equal(np.isfinite(beam), np.broadcast_to(allowed.astype(bool), (R, V)))
    ok = np.flatnonzero(allowed)
    picks = (np.full(R, ok[0]), np.full(R, ok[-1]), ok[rs.randint(0, len(ok), R)])
    for forced in picks:                                            # the lowest, the highest and a random allowed token per row
        lp, _ = sampled(z, allowed, forced)
        assert np.array_equal(bits(lp), bits(beam[np.arange(R), forced])), (V, forced)


# ---------------------------------------------------------------------------------------------------------------- 2
def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def shipped_operands():
    from singa_amd import smiles
    voc = [str(v) for v in smi_voc()]
    return smiles.classify(voc), smiles.classify_orders(voc), smiles.capacity(voc)


def wide_operands():
    cls = wide()[0]
    return cls, cls, np.random.RandomState(200).randint(0, 8, 200).astype(np.uint8)


def walk(lib, cls, cap, toks):
    """the rule state after the tokens `toks` of a fresh row, from the library's host twins (cap: the valence rule)"""
    st, v = np.array([G.FRESH], np.int32), np.zeros((1, 2), np.int32)
    rem, ok = np.array([30], np.int32), np.zeros(1, np.uint8)
    for tok in toks:
        c, ns, nv = np.array([cls[tok]], np.uint8), np.zeros(1, np.int32), np.zeros((1, 2), np.int32)
        if cap is None:
            assert lib.singa_smiles_rule_host(vp(c), vp(st), vp(rem), 1, vp(ok), vp(ns)) == 0
        else:
            cp = np.array([cap[tok]], np.uint8)
            assert lib.singa_valence_rule_host(vp(c), vp(cp), vp(st), vp(v), vp(rem), 1, vp(ok), vp(ns), vp(nv)) == 0
        assert ok[0] == 1, (toks, tok)
        st, v = ns, nv
    return int(st[0]), v[0].copy()


def rule_states(lib, cls, cap):
    """fresh, after an atom, inside a branch, with an open ring, and a branch beside an open ring -> gstate [R], vstate [R, 2]"""
    first = lambda byte: int(np.flatnonzero(np.asarray(cls) == byte)[0])
    atoms = np.flatnonzero((np.asarray(cls) & 15) == G.ATOM)
    atom = int(atoms[0] if cap is None else atoms[np.asarray(cap)[atoms] >= 4][0])
    opn, ring = first(G.OPEN), first(G.RING)                        # '(' and the digit 1
    got = [walk(lib, cls, cap, toks) for toks in ([], [atom], [atom, opn], [atom, ring], [atom, ring, atom, opn, atom])]
    assert len(got) == R
    return np.array([g for g, _ in got], np.int64), np.stack([v for _, v in got]).astype(np.int64)


def log_mass(z, masks):
    z = z.astype(np.float64)
    e = np.exp(z - z.max(1, keepdims=True))
    with np.errstate(divide="ignore"):
        return np.log((e * masks).sum(1)) - np.log(e.sum(1))


@pytest.mark.parametrize("T", [4, 12], ids=["rem2", "rem10"])
@pytest.mark.parametrize("rule", ["smiles", "valence"])
@pytest.mark.parametrize("vocab", [shipped_operands, wide_operands], ids=["V116", "V200"])
def test_all_three_see_the_mask_of_the_rule(vocab, rule, T):
    from singa_amd import _lib
    lib = _lib.lib()
    cls_s, cls_v, cap = vocab()
    cls, cap = (cls_v, cap) if rule == "valence" else (cls_s, None)
    V, rem = len(cls), T - 2
    gs, vs = rule_states(lib, cls, cap)
    if cap is None:
        want = G.allows(gs[:, None], np.asarray(cls, np.int64)[None, :], rem)
    else:
        want = VR.allows(gs[:, None], vs[:, 0][:, None], vs[:, 1][:, None], np.asarray(cls, np.int64)[None, :],
                         np.asarray(cap, np.int64)[None, :] & 7, rem)
    assert want.any(1).sum() >= 3 and not want.all(1).any()          # the states do tell the rule's masks apart
    assert len({m.tobytes() for m in want}) >= 3
    beam = beam_cand(np.zeros((R, V), np.float32), None, cls, cap, gs, vs, T)
    assert np.array_equal(np.isfinite(beam), want)                  # the rule alone: the restatement's mask exactly
    for seed in range(50):                                          # (see the module docstring: fair inputs for a relative bound)
        z = (2.5 * np.random.RandomState(1000 * V + seed).randn(R, V)).astype(np.float32)
        allowed = np.ones(V, np.uint8)
        allowed[z.argmax(1)] = 0
        masks = want & allowed.astype(bool)[None, :]
        mass = log_mass(z, masks)
        if (mass[masks.any(1)] < -0.25).all():
            break
    else:
        raise AssertionError("no fair logits in 50 draws")
    beam = beam_cand(z, allowed, cls, cap, gs, vs, T)
    assert np.array_equal(np.isfinite(beam), masks)
    if cap is None:
        assert np.array_equal(bits(swor_cand_logp(z, allowed, cls, gs, T)), bits(beam))     # swor: no valence form
    _, alp = sampled(z, allowed, None, cls, cap, gs, vs, T)
    empty = ~masks.any(1)
    print(f"V={V} {rule} rem={rem}: allowed tokens per row {masks.sum(1).tolist()}, float64 log-mass {np.round(mass, 4).tolist()}, "
          f"worst relative error {np.max(np.abs(alp[~empty] - mass[~empty]) / np.abs(mass[~empty])) if (~empty).any() else 0:.2e}")
    assert (alp[empty] == -np.inf).all()
    assert (np.abs(alp[~empty] - mass[~empty]) <= 1e-5 * np.abs(mass[~empty])).all(), (alp, mass)
