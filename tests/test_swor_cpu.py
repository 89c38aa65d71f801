"""Sampling without replacement, the part that runs without a GPU: the header against its binding table and the built
library, `singa_swor_noise_host` against the numpy Philox / hash / uniform of tests/swor_rule.py bit for bit, the argument
errors of the entry points, the rule's inclusion frequencies against the analytic Plackett-Luce values, and `swor_weights`."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import swor_rule as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["singa_swor_expand", "singa_swor_follow", "singa_swor_noise_host", "singa_swor_select", "singa_swor_work"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_swor_table_matches_header_and_library(lib):
    from singa_amd import _capi
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", strip("singa_hip_swor.h"))))
    assert declared == sorted(_capi.SWOR_EXPORTS) == NAMES
    others = set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS) | set(_capi.GEN_EXPORTS) | set(_capi.FORCE_EXPORTS)
    assert not set(_capi.SWOR_EXPORTS) & others
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)
    for other in ("singa_hip.h", "singa_hip_gen.h", "singa_hip_lab.h", "singa_hip_force.h"):   # declared in its own header only
        assert "singa_swor_" not in strip(other)
    import __graft_entry__
    assert "singa_hip_swor.h" in open(__graft_entry__.__file__).read()                       # a dependency of the build


def test_philox_known_answers():
    """Random123's known-answer vectors for philox4x32-10 (first output word)."""
    assert int(R.philox(0, 0, 0, 0)) == 0x6627E8D5
    assert int(R.philox(2 ** 64 - 1, 2 ** 64 - 1, 0xFFFFFFFF, 0xFFFFFFFF)) == 0x408F276D
    assert int(R.philox(0x299F31D0A4093822, 0x85A308D3243F6A88, 0x13198A2E, 0x03707344)) == 0xD16CFE09


def test_noise_host_equals_numpy_bit_for_bit(lib):
    rs = np.random.RandomState(0)
    n = 10000
    word = lambda: rs.randint(0, 2 ** 32, n, dtype=np.uint64)
    hsh = (word() << np.uint64(32)) | word()
    v = rs.randint(0, 1024, n).astype(np.int32)
    strm = word().astype(np.uint32)
    hsh[:4], v[:4], strm[:4] = [0, 2 ** 64 - 1, 0, 1], [0, 1023, 5, 0], [0, 2 ** 32 - 1, 0, 7]
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for seed in (0, 1, 0x3707344AA4093822, 2 ** 64 - 1):
        x, u, child = np.zeros(n, np.uint32), np.zeros(n, np.float32), np.zeros(n, np.uint64)
        assert lib.singa_swor_noise_host(seed, ptr(hsh), ptr(v), ptr(strm), n, ptr(x), ptr(u), ptr(child)) == 0
        assert np.array_equal(x, R.philox(seed, hsh, v, strm)), seed
        assert np.array_equal(u.view(np.uint32), R.uniform(x).view(np.uint32)), seed
        assert np.array_equal(child, R.child_hash(hsh, v)), seed
        assert (u > 0).all() and (u < 1).all()
    # the uniform's edges: the smallest word, the largest (whose float32 sum rounds to 2^24, i.e. u = 1, taken back), a tie
    edge = np.array([0, 0xFFFFFFFF, 0xFFFFFE00, 0x80000100, 0x000001FF], np.uint32)
    ue = R.uniform(edge)
    assert ue[0] == np.float32(2.0 ** -25) and ue[1] == np.float32(1 - 2.0 ** -24) and (ue < 1).all()
    assert lib.singa_swor_noise_host(0, ptr(hsh), ptr(v), ptr(strm), 3, None, None, None) == 0     # every output is optional
    assert lib.singa_swor_noise_host(0, None, ptr(v), ptr(strm), 3, None, None, None) == -1
    assert lib.singa_swor_noise_host(0, ptr(hsh), ptr(v), ptr(strm), -1, None, None, None) == -3


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    NULL, SHAPE = -1, -3
    err = lambda: lib.singa_last_error_string()

    def expand(rows=4, k=2, V=116, T=8, tau=1.0, pad=4, logits=p, cls=None, gstate=None, cand=p, streams=p):
        return lib.singa_swor_expand(logits, None, cls, p, 1, rows, k, V, T, tau, 7, streams, pad, p, p, p, p, gstate, cand, p, p, None)

    def select(rows=4, k=2, V=116, T=8, eos=3, pad=4, cand=p, cls=None, gstate=None, work=p, live=p):
        return lib.singa_swor_select(cand, p, p, cls, p, 1, rows, k, V, T, eos, pad, p, p, p, p, p, p, gstate, p, p, p, p, live, work,
                                     None)

    for call in (expand, select):
        for null in (dict(cand=None), dict(cls=p), dict(gstate=p)):
            assert call(**null) == NULL, (call.__name__, null)
        for bad in (dict(V=0), dict(V=1025), dict(k=0), dict(k=2049, rows=2049), dict(rows=5), dict(rows=-2), dict(T=1), dict(pad=116),
                    dict(pad=-1), dict(T=2, cls=p, gstate=p)):
            assert call(**bad) == SHAPE, (call.__name__, bad)
            assert b"swor_" in err()
        assert call(rows=0) == 0 and call(rows=0, k=2048, V=1024, T=2) == 0 and call(rows=0, T=3, cls=p, gstate=p) == 0
    assert expand(logits=None) == NULL and expand(streams=None) == NULL and select(work=None) == NULL and select(live=None) == NULL
    for tau in (0.0, -1.0, float("nan")):
        assert expand(tau=tau) == SHAPE and b"temperature" in err()
    assert select(eos=116) == SHAPE and select(eos=-1) == SHAPE
    assert select(work=ctypes.c_void_p(p.value + 4)) == SHAPE and b"aligned" in err()

    assert lib.singa_swor_work(-1, 8) == -1 and lib.singa_swor_work(4, 1) == -1 and lib.singa_swor_work(0, 2) == 0
    for rows, T in ((1, 2), (7, 41), (2048, 257)):                        # holds every field of the new row state, 16-byte aligned
        n = lib.singa_swor_work(rows, T)
        assert n % 16 == 0 and rows * (T * 12 + 29) <= n <= rows * (T * 12 + 29) + 9 * 16

    q = ctypes.c_void_p((p.value + 15) // 16 * 16)
    q2 = ctypes.c_void_p(q.value + 16)

    def follow(ks=q, kd=q2, vs=q, vd=q2, src=q, layers=2, rows=4, heads=4, P=8, dk=32, dv=64, krow=None, klay=None, vrow=None, vlay=None):
        krow, vrow = heads * P * dk if krow is None else krow, heads * P * dv if vrow is None else vrow
        klay, vlay = rows * krow if klay is None else klay, rows * vrow if vlay is None else vlay
        return lib.singa_swor_follow(ks, vs, kd, vd, src, q, q, q, layers, rows, heads, P, dk, dv, krow, klay, vrow, vlay, None)

    assert follow(ks=None) == NULL and follow(src=None) == NULL
    for bad in (dict(dk=30), dict(dv=2), dict(dk=0), dict(heads=0), dict(P=0), dict(rows=-1), dict(layers=-1), dict(krow=4 * 8 * 32 - 4),
                dict(vrow=4 * 8 * 64 + 2), dict(klay=4 * 4 * 8 * 32 - 4), dict(vlay=3), dict(kd=q), dict(vd=q), dict(layers=70000),
                dict(ks=ctypes.c_void_p(q.value + 4)), dict(vd=ctypes.c_void_p(q.value + 8)), dict(heads=4096, P=4096, dk=64, dv=128)):
        assert follow(**bad) == SHAPE, bad
        assert b"swor_follow" in err()
    assert follow(rows=0) == 0 and follow(layers=0) == 0


def test_rule_inclusion_frequencies_are_plackett_luce():
    """A tree of three leaves - '$' (0.5), 'a$' (0.2), 'ab' (0.3) - and k = 2 over 20,000 seeds: how often each leaf is among
    the two returned, against sampling two of three without replacement; the second level is reached only through the
    conditioning on the parent's G.  4 standard errors of a binomial frequency."""
    sos, pad, a, b, eos = 0, 1, 2, 3, 4
    V, T, n = 5, 3, 20000
    off = np.float32(-1e4)
    table = np.full((V, V), off, np.float32)
    table[sos, [a, eos]] = np.log([0.5, 0.5]).astype(np.float32)
    table[a, [eos, b]] = np.log([0.4, 0.6]).astype(np.float32)
    table[b, eos] = 0.0
    allowed = np.array([0, 0, 1, 1, 1], np.uint8)
    seeds = np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(12345)
    out = R.run(table, 2, T, seeds, np.zeros(n, np.int64), sos, eos, pad, allowed=allowed)
    assert out["valid"].all()
    leaves = {(eos, pad): 0.5, (a, eos): 0.2, (a, b): 0.3}
    want = R.plackett_luce_inclusion(list(leaves.values()))
    toks = out["tokens"][:, :, 1:]
    assert (toks[:, 0] != toks[:, 1]).any(1).all()                        # the two of a run are distinct
    assert (out["gumbel"][:, 0] >= out["gumbel"][:, 1]).all()
    for (leaf, p), w in zip(leaves.items(), want):
        hit = (toks == np.array(leaf)).all(2)
        freq = hit.any(1).mean()
        se = np.sqrt(w * (1 - w) / n)
        print(f"leaf {leaf}: p {p}, inclusion {freq:.4f}, Plackett-Luce {w:.4f}, 4 se {4 * se:.4f}")
        assert abs(freq - w) <= 4 * se, (leaf, freq, w)
        assert np.allclose(out["prop_logp"][hit], np.log(p), atol=1e-6) and np.allclose(out["sum_logp"][hit], np.log(p), atol=1e-6)
    # the first of the two is a plain sample: frequencies of the leaf at rank 0 are the probabilities themselves
    for leaf, p in leaves.items():
        freq = (toks[:, 0] == np.array(leaf)).all(1).mean()
        assert abs(freq - p) <= 4 * np.sqrt(p * (1 - p) / n), (leaf, freq, p)


def test_rule_is_nested_and_keyed_by_the_prefix():
    """k = 3 is the head of k = 7 (same seed), and a pocket's result depends on its stream alone, not on its neighbours."""
    V, T = 9, 6
    table = R.toy_table(V, 3, 0, 2, 1)
    allowed = np.ones(V, np.uint8)
    allowed[:2] = 0
    big = R.run(table, 7, T, 11, [5, 6], 0, 2, 1, allowed=allowed)
    small = R.run(table, 3, T, 11, [5, 6], 0, 2, 1, allowed=allowed)
    alone = R.run(table, 7, T, 11, [6], 0, 2, 1, allowed=allowed)
    for key in ("tokens", "gumbel", "prop_logp", "sum_logp"):
        assert np.array_equal(small[key], big[key][:, :3]), key
        assert np.array_equal(alone[key][0], big[key][1]), key
    assert not np.array_equal(big["tokens"][0], big["tokens"][1])


def test_swor_weights_on_hand_computed_values():
    from singa_amd.model.Sampling import swor_weights
    phi = np.log(np.array([[0.5, 0.25, 0.125, 1.0], [0.2, 0.1, 1.0, 1.0]]))
    g = np.array([[1.0, 0.5, -0.25, -np.inf], [0.0, -np.inf, -np.inf, -np.inf]])
    valid = np.array([[1, 1, 1, 0], [1, 0, 0, 0]])
    w = swor_weights(phi, g, valid)
    kappa = -0.25
    q = lambda p: 1.0 - np.exp(-p * np.exp(-kappa))                          # exp(phi - kappa) = p e^-kappa
    assert np.allclose(w[0], [1 / q(0.5), 1 / q(0.25), 0.0, 0.0], rtol=1e-12)
    assert np.array_equal(w[1], [0.0, 0.0, 0.0, 0.0])                         # a lone survivor is the threshold itself
    assert abs(1 / q(0.5) - 2.11074) < 1e-5                                   # 1 / (1 - exp(-0.5 e^0.25)), by hand
    with pytest.raises(ValueError, match="pockets, k"):
        swor_weights(phi[0], g[0], valid[0])


def test_sample_distinct_refuses_bad_arguments_before_any_launch():
    import torch

    from singa_amd.config import Config
    from singa_amd.model import Sampling
    from tests.helpers import smi_voc
    voc = smi_voc()
    ex = Config()
    ex.protein_atom_feature = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.sample_distinct(None, voc, 2, 1, 8, ex, device="cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.sample_distinct(None, voc, 2, 1, 8, ex, device="cpu")
