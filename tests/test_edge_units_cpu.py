"""The kNN edge MLPs once per undirected edge, the part that runs without a GPU: the unit list `KnnEdges` builds (every row in
exactly one unit, mates are opposite directions with the same attribute bits, self loops and padding rows alone, fixed
shapes), the header against its binding table and the built library, and the argument errors of the entry points."""
import ctypes
import os
import re

import pytest
import torch

from singa_amd.model import CProMG as CP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["singa_edge_mlp_units_bwd", "singa_edge_mlp_units_fwd"]


def knn_list(pos, sizes, k):
    """[2, N * k] (centre, neighbour): the k nearest other nodes of the same graph, -1 in the slots a small graph cannot fill."""
    N = pos.shape[0]
    ei = torch.full((2, N * k), -1, dtype=torch.int64)
    start = 0
    for n in sizes:
        d = (pos[start:start + n, None] - pos[None, start:start + n]).norm(dim=2)
        d.fill_diagonal_(float("inf"))
        kk = min(k, n - 1)
        nb = d.argsort(dim=1)[:, :kk] + start
        for i in range(n):
            s = (start + i) * k
            ei[0, s:s + kk] = start + i
            ei[1, s:s + kk] = nb[i]
        start += n
    return ei


def make(sizes, k, seed, pad_atoms=0):
    g = torch.Generator().manual_seed(seed)
    n_real = sum(sizes)
    pos = torch.randn(n_real + pad_atoms, 3, generator=g) * 3.0
    smear = CP.GaussianSmearing(stop=15, num_gaussians=64, device="cpu")
    knn = knn_list(pos[:n_real], sizes, k)
    return CP.KnnEdges(pos, knn, smear), n_real, knn


def check_units(e, n_real):
    E = e.row.numel()
    a, b = e.unit_a, e.unit_b
    assert a.dtype == b.dtype == torch.int32 and a.shape == b.shape == (E,)
    assert e.tensors()[-2] is a and e.tensors()[-1] is b
    n = int((a >= 0).sum())
    assert bool((a[:n] >= 0).all()) and bool((a[n:] == -1).all()) and bool((b[n:] == -1).all())      # units first, a null tail
    a, b = a[:n].long(), b[:n].long()
    assert bool((a[1:] > a[:-1]).all())                                                  # in row order
    named = torch.cat([a, b[b != a]])
    assert torch.equal(torch.sort(named).values, torch.arange(E))                        # every row, exactly once
    mated = b != a
    assert torch.equal(e.row[a[mated]], e.col[b[mated]]) and torch.equal(e.col[a[mated]], e.row[b[mated]])
    assert bool((e.row[a[mated]] < e.col[a[mated]]).all())
    assert torch.equal(e.attr[a].view(torch.int32), e.attr[b].view(torch.int32))         # the same bits
    alone = (e.row == e.col) | (e.row >= n_real) | (e.col >= n_real)                     # self loops, padding rows
    assert bool((~mated)[alone[a]].all()) and not bool(alone[b[mated]].any())
    assert int(mated.sum()) * 2 + int(alone.sum()) == E                                  # and nothing else is alone
    return n


@pytest.mark.parametrize("sizes, k", [((5, 40, 3, 120), 8), ((300, 17), 48), ((2, 1, 9), 4)])
def test_units_of_knn_edges(sizes, k):
    e, n_real, knn = make(sizes, k, seed=sum(sizes) + k)
    assert bool((knn < 0).any())                                                         # a graph below k + 1 nodes: absent slots
    fwd = set(map(tuple, knn[:, knn[0] >= 0].t().tolist()))
    assert any((j, i) not in fwd for i, j in fwd)                                        # non-mutual neighbours
    n = check_units(e, n_real)
    assert n == (e.row.numel() - n_real) // 2 + n_real                                   # E0 / 2 + N of E0 + N rows


def test_units_of_padded_edge_lists_have_fixed_shapes():
    shapes = []
    for sizes, seed, pad in (((5, 40, 3, 60), 3, 72), ((30, 50, 20), 4, 80)):
        n_real = sum(sizes)
        cap = 1600                                                                       # the same capacity for both batches
        g = torch.Generator().manual_seed(seed)
        pos = torch.randn(n_real + pad, 3, generator=g) * 3.0
        smear = CP.GaussianSmearing(stop=15, num_gaussians=64, device="cpu")
        e = CP.KnnEdges(pos, knn_list(pos[:n_real], sizes, 8), smear, cap=cap, n_real=n_real)
        assert e.n_edges < cap and e.row.numel() == cap                                  # padding edges were added
        n = check_units(e, n_real)
        assert n < cap                                                                   # a null tail behind the units
        shapes.append([tuple(t.shape) for t in e.tensors()[4:]])
    assert shapes[0] == shapes[1]


def test_units_of_a_list_with_repeats_are_singletons():
    sizes, k = (12, 7), 4
    pos = torch.randn(19, 3, generator=torch.Generator().manual_seed(9))
    knn = knn_list(pos, sizes, k)
    e = CP.KnnEdges(pos, torch.cat([knn, knn, knn], 1), CP.GaussianSmearing(stop=15, num_gaussians=64, device="cpu"))
    E = e.row.numel()
    assert torch.equal(e.unit_a.long(), torch.arange(E)) and torch.equal(e.unit_b, e.unit_a)


# ------------------------------------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


def test_units_table_matches_header_and_library(lib):
    from singa_amd import _capi
    strip = lambda name: re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(singa_[a-z0-9_]+)\s*\(", strip("singa_hip_units.h"))))
    assert declared == sorted(_capi.UNITS_EXPORTS) == NAMES
    others = set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS) | set(_capi.GEN_EXPORTS) | set(_capi.FORCE_EXPORTS) | \
        set(_capi.SWOR_EXPORTS) | set(_capi.STREAM_EXPORTS) | set(_capi.VALENCE_EXPORTS) | set(_capi.BEAM_EXPORTS)
    assert not set(_capi.UNITS_EXPORTS) & others
    raw = ctypes.CDLL(lib._name)
    assert all(hasattr(raw, n) for n in declared)
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):                      # declared in its own header only
        if other != "singa_hip_units.h":
            assert "singa_edge_mlp_units" not in strip(other), other
    import __graft_entry__
    assert "singa_hip_units.h" in open(__graft_entry__.__file__).read()                 # a dependency of the build


def test_argument_errors_without_gpu(lib):
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)                 # never dereferenced: every call below fails its checks or has no rows
    assert p.value % 16 == 0
    off = ctypes.c_void_p(p.value + 4)
    NULL, SHAPE = -1, -3
    err = lambda: lib.singa_last_error_string()

    def fwd(E=0, CIN=64, HK=32, HV=64, **ptr):
        names = ["attr", "unit_a", "unit_b", "w1tk", "b1k", "w2tk", "b2k", "w1tv", "b1v", "w2tv", "b2v", "wk", "wv"]
        return lib.singa_edge_mlp_units_fwd(*[ptr.get(n, p) for n in names], E, CIN, HK, HV, None)

    def bwd(E=0, CIN=64, H=32, **ptr):
        names = ["attr", "unit_a", "unit_b", "g_out", "w1t", "b1", "w2", "part"]
        return lib.singa_edge_mlp_units_bwd(*[ptr.get(n, p) for n in names], E, CIN, H, None)

    for call, names, aligned in ((fwd, ["attr", "unit_a", "unit_b", "w1tk", "b1k", "w2tk", "b2k", "w1tv", "b1v", "w2tv", "b2v", "wk", "wv"],
                                  ["attr", "wk", "wv"]),
                                 (bwd, ["attr", "unit_a", "unit_b", "g_out", "w1t", "b1", "w2", "part"], ["attr", "g_out"])):
        assert call() == 0                                                               # no rows: nothing to do
        for n in names:
            assert call(E=4, **{n: None}) == NULL, (call.__name__, n)
            assert b"edge_mlp_units_" in err()
        for n in aligned:
            assert call(E=4, **{n: off}) == SHAPE and b"aligned" in err(), (call.__name__, n)
        assert call(E=-1) == SHAPE and call(CIN=32) == SHAPE and b"edge_mlp_units_" in err()
    assert fwd(HK=64) == SHAPE and fwd(HV=32) == SHAPE
    assert bwd(H=16) == SHAPE and bwd(H=128) == SHAPE and bwd(H=64) == 0
