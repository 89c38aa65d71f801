"""-m gpu: n2 for graphs of 2,049 .. 32,768 atoms (singa_lap_pe_xl through ops.lap_pe_xl) against numpy's fp64 eigvalsh of the
same Laplacian, basis-free, with the bounds of tests/test_lap_large_gpu.py; repeatability; and the routing of
graph.laplacian_pe_batched.  The pure paths are the class singa_lap_pe_large gives up on (eigenvalues ~1e-6 apart)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0


def _lap_np(ei, n):
    a = np.zeros((n, n))
    a[ei[0], ei[1]] = 1.0
    dinv = np.clip(a.sum(0), 1, None) ** -0.5
    lap = np.eye(n) - dinv[:, None] * a * dinv[None, :]
    return 0.5 * (lap + lap.T)


def _sym_edges(pairs):
    a, b = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])])


def _path(n, at=0):
    return [(at + i, at + i + 1) for i in range(n - 1)]


# the graphs as (atoms, edges, goes by the book); every case is ONE call over some of them
_rs = np.random.RandomState(5)
GRAPHS = {
    "path": (2049, _sym_edges(_path(2049)), True),
    "shuffled": (2049, _rs.permutation(2049)[_sym_edges(_path(2049))], True),
    "chords": (2300, _sym_edges(_path(2300) + [(int(a), int(b)) for a, b in _rs.randint(0, 2300, (1000, 2)) if a != b]), True),
    "fragments": (2500, _sym_edges([p for c in range(50) for p in _path(50, 50 * c)]), True),
    # a 2,000-atom component with chords + two fragments of 200, numbering interleaved: three null vectors, then a solve
    "interleaved": (2400, _rs.permutation(2400)[_sym_edges(
        _path(2000) + [(int(a), int(b)) for a, b in _rs.randint(0, 2000, (600, 2)) if a != b] + _path(200, 2000) + _path(200, 2200))], True),
    "hub": (2100, _sym_edges(_path(2100) + [(0, 50 * i + 25) for i in range(40)]), False),     # atom 0: more than an ELL row holds
}
CASES = {name: [name] for name in GRAPHS}
CASES["two"] = ["chords", "path"]
_REF = {}


def _reference(name):
    """(Laplacian, ascending eigenvalues) of a graph, computed once."""
    if name not in _REF:
        n, e, _ = GRAPHS[name]
        lap = _lap_np(e, n)
        _REF[name] = (lap, np.linalg.eigvalsh(lap))
    return _REF[name]


def _check(v, name):
    lap, w = _reference(name)
    assert np.isfinite(v).all()
    assert np.abs(v.T @ v - np.eye(8)).max() < 2e-6, name
    ritz = v.T @ lap @ v
    assert np.abs(lap @ v - v @ ritz).max() < 2e-6, name
    assert np.abs(np.linalg.eigvalsh(ritz) - w[1:9]).max() < 2e-6, name
    assert (v.max(0) >= (-v).max(0) - 1e-6).all()


def _encode(names):
    """One ops.lap_pe_xl call over the named graphs, placed with gaps into a sentinel-filled `out`."""
    from singa_amd import ops
    gs = [GRAPHS[nm] for nm in names]
    num = [n for n, _, _ in gs]
    start = np.cumsum([3] + [n + 2 for n in num])[:-1]
    n_total = int(start[-1] + num[-1] + 4)
    ei = np.concatenate([e for _, e, _ in gs], 1)
    t = lambda a, dt=torch.int32: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    out = torch.full((n_total, 8), SENTINEL, device=DEV)
    got, status = ops.lap_pe_xl(t(ei[0]), t(ei[1]), t(np.concatenate([[0], np.cumsum([e.shape[1] for _, e, _ in gs])])),
                                t(num, torch.long), t(start, torch.long), n_total, max(num), 8, out=out)
    return got.cpu(), status.cpu().numpy(), start


@pytest.mark.parametrize("case", sorted(CASES))
def test_lap_pe_xl_against_numpy(case):
    """Status 0 and the bounds for every graph that goes by the book, rows outside the graphs untouched; the hub graph sets status
    1, leaves its rows alone, and meets the same bounds through graph.laplacian_pe_batched (the dense route)."""
    from singa_amd import graph as G
    got, status, start = _encode(CASES[case])
    pe = got.double().numpy()
    inside = np.zeros(pe.shape[0], bool)
    for name, s, st in zip(CASES[case], start, status):
        n, e, ok = GRAPHS[name]
        inside[s:s + n] = True
        assert st == (0 if ok else 1), (name, st)
        v = pe[s:s + n]
        if not ok:
            assert (v == SENTINEL).all()
            v = G.laplacian_pe_batched(torch.tensor(e, device=DEV), torch.zeros(n, dtype=torch.long, device=DEV), 1).cpu().double().numpy()
        _check(v, name)
    assert (pe[~inside] == SENTINEL).all()


def test_lap_pe_xl_repeats_bit_for_bit():
    assert torch.equal(_encode(["path"])[0], _encode(["path"])[0])


def test_small_graphs_keep_their_route_beside_an_xl_one(monkeypatch):
    """graph.laplacian_pe_batched on three bundled-size graphs + the 2,049-atom path, the dense route patched to raise: the small
    graphs' rows are bit-equal to the rows of the batch without the large graph, the large graph's columns orthonormal."""
    from singa_amd import graph as G

    def no_dense(*a, **k):
        raise AssertionError("the dense route was taken")
    monkeypatch.setattr(G, "_laplacian_pe_dense", no_dense)
    gs = [(300, _sym_edges(_path(300))), (41, _sym_edges([(i, (i + 1) % 41) for i in range(41)])),
          (5, _sym_edges([(0, 1), (1, 2), (3, 4)])), GRAPHS["path"][:2]]
    res = []
    for sub in (gs, gs[:3]):
        off = np.cumsum([0] + [n for n, _ in sub])
        ei = torch.tensor(np.concatenate([e + o for (_, e), o in zip(sub, off)], 1), device=DEV)
        bt = torch.repeat_interleave(torch.arange(len(sub)), torch.tensor([n for n, _ in sub])).to(DEV)
        res.append(G.laplacian_pe_batched(ei, bt, len(sub)).cpu())
    assert res[0].shape == (346 + 2049, 8) and torch.equal(res[0][:346], res[1])
    v = res[0][346:].double()
    assert float((v.T @ v - torch.eye(8, dtype=torch.float64)).abs().max()) < 2e-6
