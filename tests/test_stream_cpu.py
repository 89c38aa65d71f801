"""Continuous sampling, the part that runs without a GPU: the header against its binding table and the built library, the
argument errors of the entry points, the hand-over's host twin (`singa_stream_refill_host`, one source with the kernel)
against the numpy restatement of tests/stream_rule.py, and `sample_stream`'s refusal of a CPU device."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests.stream_rule import live_after, stream_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["singa_dec_self_attn_rows", "singa_sample_token_stream", "singa_stream_refill", "singa_stream_refill_host"]
NULL, SHAPE = -1, -3


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_stream_table_matches_header_and_library(lib):
    from singa_amd import _capi
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", strip("singa_hip_stream.h"))))
    assert declared == sorted(_capi.STREAM_EXPORTS) == NAMES
    others = set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS) | set(_capi.GEN_EXPORTS) | set(_capi.FORCE_EXPORTS) | set(_capi.SWOR_EXPORTS)
    assert not set(_capi.STREAM_EXPORTS) & others
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)
    for other in ("singa_hip.h", "singa_hip_gen.h", "singa_hip_lab.h", "singa_hip_force.h", "singa_hip_swor.h"):
        text = strip(other)                                                # declared in its own header only
        assert not any(re.search(r"\b%s\b" % n, text) for n in NAMES), other
    import __graft_entry__
    assert "singa_hip_stream.h" in open(__graft_entry__.__file__).read()   # a dependency of the build


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    err = lambda: lib.singa_last_error_string()

    def choice(rows=4, M=8, V=116, T=8, tau=1.0, top_k=0, top_p=1.0, eos=3, pad=4, logits=p, mol=p, pos=p, cls=None, gstate=None,
               alp=None, tokens=p, length=p):
        return lib.singa_sample_token_stream(logits, p, None, cls, pos, mol, 1, rows, M, V, T, tau, top_k, top_p, eos, pad, length, p,
                                             tokens, p, None, gstate, alp, None)

    for null in (dict(logits=None), dict(mol=None), dict(pos=None), dict(tokens=None), dict(length=None), dict(cls=p), dict(gstate=p),
                 dict(alp=p)):
        assert choice(**null) == NULL, null
        assert b"sample_token_stream" in err()
    for bad, word in ((dict(V=0), b"vocabulary"), (dict(V=1025), b"vocabulary"), (dict(T=1), b"T >= 2"),
                      (dict(T=2, cls=p, gstate=p), b"T >= 2"), (dict(M=0), b"molecules"), (dict(eos=116), b"eos"), (dict(pad=-1), b"pad"),
                      (dict(rows=-1), b"T >= 2"), (dict(tau=-1.0), b"temperature"), (dict(top_k=-1), b"top_k"), (dict(top_p=0.0), b"top_p")):
        assert choice(**bad) == SHAPE, bad
        assert b"sample_token_stream" in err() and word in err(), (bad, err())
    assert choice(rows=0) == 0 and choice(rows=0, V=1024, T=2) == 0 and choice(rows=0, T=3, cls=p, gstate=p) == 0

    def refill(fn, pockets=2, R=3, n=5, T=8, pos=p, mol=p, nxt=p, gstate=None, issued=p, live=p, row_of=p, start=p):
        args = (pockets, R, n, T, 1, 0, 3, 7, pos, mol, nxt, gstate, issued, live, row_of, start)
        return fn(*args, None) if fn is lib.singa_stream_refill else fn(*args)

    for fn, name in ((lib.singa_stream_refill, b"stream_refill:"), (lib.singa_stream_refill_host, b"stream_refill_host:")):
        for null in (dict(pos=None), dict(mol=None), dict(nxt=None), dict(issued=None), dict(live=None), dict(row_of=None),
                     dict(start=None)):
            assert refill(fn, **null) == NULL, null
            assert name in err()
        for bad, word in ((dict(R=0), b"R:"), (dict(R=2049), b"R:"), (dict(n=0), b"num_samples"), (dict(T=1), b"T >= 2"),
                          (dict(T=2, gstate=p), b"T >= 2"), (dict(pockets=-1), b"pockets"), (dict(pockets=2 ** 20, n=2 ** 12), b"pockets")):
            assert refill(fn, **bad) == SHAPE, bad
            assert name in err() and word in err(), (bad, err())
        assert refill(fn, pockets=0) == 0 and refill(fn, pockets=0, R=2048, T=2) == 0

    def attn(x=p, pos=p, y=p, R=4, P=8):
        return lib.singa_dec_self_attn_rows(x, p, p, p, p, p, p, p, p, pos, R, P, y, 1e-5, None)

    assert attn(x=None) == NULL and attn(pos=None) == NULL and attn(y=None) == NULL and b"dec_self_attn_rows" in err()
    assert attn(P=0) == SHAPE and attn(P=257) == SHAPE and b"256 cached positions" in err()
    assert attn(R=0) == 0


def drive_host(lib, counts, R, T, grammar=False):
    """Steps of the rule with the host twin doing the hand-over and this function the choices: molecule j draws `eos` in its
    step counts[j] - 1, anything else before (counts[j] = T - 1 draws no `eos` at all: the last column ends it).  Returns the
    state after every step and the final one."""
    counts = np.asarray(counts)
    B, n = counts.shape
    sos, eos, other, off, fresh = 0, 3, 5, 1, 7
    first = min(R, n)
    mol = np.full((B, R), -1, np.int32)
    mol[:, :first] = np.arange(B)[:, None] * n + np.arange(first)[None]
    row_of = np.zeros((B, n), np.int32)
    row_of[:, :first] = np.arange(B)[:, None] * R + np.arange(first)[None]
    st = dict(pos=np.full(B * R, off, np.int64), mol=mol.reshape(-1), next=np.full(B * R, sos, np.int64),
              gstate=np.full(B * R, fresh, np.int32), issued=np.full(B, first, np.int32), live=np.full(B, first, np.int32),
              row_of=row_of.reshape(-1), start_step=np.zeros(B * n, np.int32))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    flat, history = counts.reshape(-1), []
    for step in range((-(-n // R) + 1) * (T - 1) + 2):
        rows = np.flatnonzero(st["mol"] >= 0)
        t = st["pos"][rows] - off
        last = t + 1 == flat[st["mol"][rows]]
        st["next"][rows] = np.where(last & (t + 1 < T - 1), eos, other)
        st["gstate"][rows] = 99                                            # "the state after the token"
        assert lib.singa_stream_refill_host(B, R, n, T, off, sos, eos, fresh, ptr(st["pos"]), ptr(st["mol"]), ptr(st["next"]),
                                            ptr(st["gstate"]) if grammar else None, ptr(st["issued"]), ptr(st["live"]),
                                            ptr(st["row_of"]), ptr(st["start_step"])) == 0
        history.append({k: v.copy() for k, v in st.items()})
        if st["live"].sum() == 0 and step >= 1 and history[-2]["live"].sum() == 0:
            break
    return history, (sos, eos, other, off, fresh)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [1, 3, 64, 65, 2048])
def test_host_twin_against_the_rule(lib, B, R):
    T = 7
    issued_sets = []
    for n in sorted({1, max(R - 1, 1), R, 4 * R + 1}):
        rs = np.random.RandomState(1000 * B + R + n)
        counts = rs.randint(1, T, (B, n))                                  # 1 .. T - 1 steps, the last column among them
        want_row, want_start, total = stream_rule(counts, R)
        history, (sos, eos, other, off, fresh) = drive_host(lib, counts, R, T, grammar=(n % 2 == 0))
        end = history[-1]
        assert np.array_equal(end["row_of"], want_row), (B, R, n)
        assert np.array_equal(end["start_step"], want_start), (B, R, n)
        assert (end["mol"] == -1).all() and (end["live"] == 0).all() and (end["issued"] == n).all()
        assert len(history) == total + 1                                   # live is zero after `total` steps, and not before
        assert all(np.array_equal(h, history[total - 1][k]) for k, h in history[-1].items())      # further steps change nothing
        for s, h in enumerate(history[:total]):
            assert np.array_equal(h["live"], live_after(counts, R, s + 1)), (s, h["live"])
            assert ((h["pos"] >= off) & (h["pos"] <= off + T - 2)).all()    # every row, retired ones too, names a cache position
            held = h["mol"][h["mol"] >= 0]
            assert len(set(held)) == len(held) and np.array_equal(h["row_of"][held], np.flatnonzero(h["mol"] >= 0))
            fresh_rows = np.flatnonzero((h["mol"] >= 0) & (h["pos"] == off))
            assert (h["next"][fresh_rows] == sos).all() and (h["start_step"][h["mol"][fresh_rows]] == s + 1).all()
            if n % 2 == 0:
                assert (h["gstate"][fresh_rows] == fresh).all()
        # every molecule is issued exactly once: the rows' histories name each molecule, in one row only
        seen = np.zeros(B * n, int)
        first = np.full((B, R), -1)
        first[:, :min(R, n)] = np.arange(B)[:, None] * n + np.arange(min(R, n))[None]
        prev = first.reshape(-1)
        np.add.at(seen, prev[prev >= 0], 1)
        for h in history:
            new = (h["mol"] != prev) & (h["mol"] >= 0)
            np.add.at(seen, h["mol"][new], 1)
            prev = h["mol"]
        assert (seen == 1).all(), (B, R, n)
        issued_sets.append((n, np.flatnonzero(seen)))
    # the set of issued molecules does not depend on R: it is every molecule, for every n
    for n, got in issued_sets:
        assert np.array_equal(got, np.arange(B * n))


def test_host_twin_leaves_a_dead_pocket_alone(lib):
    """A pocket without a live row writes nothing, and a retired row is not touched."""
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    pos, mol = np.array([5, 3, 9, 2], np.int64), np.array([-1, -1, 4, -1], np.int32)
    nxt, gs = np.array([3, 3, 5, 3], np.int64), np.array([11, 12, 13, 14], np.int32)
    issued, live = np.array([77, 3], np.int32), np.array([55, 1], np.int32)
    row_of, start = np.array([0, 1, 2, 2, 3, 2], np.int32), np.array([0, 0, 4, 4, 0, 8], np.int32)
    before = [a.copy() for a in (pos, mol, nxt, gs, issued, live, row_of, start)]
    assert lib.singa_stream_refill_host(2, 2, 3, 12, 1, 0, 3, 7, ptr(pos), ptr(mol), ptr(nxt), ptr(gs), ptr(issued), ptr(live),
                                        ptr(row_of), ptr(start)) == 0
    before[0][2] = 10                                                      # the one live row moved on by one position
    for a, b in zip((pos, mol, nxt, gs, issued, live, row_of, start), before):
        assert np.array_equal(a, b)


def test_sample_stream_refuses_a_cpu_device():
    import torch

    from singa_amd.config import Config
    from singa_amd.model import Sampling
    from tests.helpers import smi_voc
    ex = Config()
    ex.protein_atom_feature = torch.zeros(4, 8)
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.sample_stream(None, smi_voc(), 2, 1, 8, ex, device="cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        Sampling.sample_stream(None, smi_voc(), 2, 1, 8, ex, device="cpu")
