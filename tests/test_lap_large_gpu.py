"""-m gpu: n2 for graphs of 897 .. 2,048 atoms (singa_lap_pe_large through ops.lap_pe_large) against numpy's fp64 eigh of the same
Laplacian, basis-free, with the bounds of test_kernels_gpu.test_lap_eig_batched_against_numpy; and the per-graph routing of
graph.laplacian_pe_batched.  In the cases that need a solve (one component) eigenvalues 8 and 9 of the committed inputs are
at least 1e-4 apart (checked with numpy: 1.2e-3 at 897, 1.1e-3 at 2,048, 2.9e-4 at 900 atoms, 4.0e-4 for the hub graph); in the
fragment cases both are exact zeros of the same null space, which the residual check covers as it stands."""
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


# every case: the graphs of ONE launch as (atoms, edges, goes by the book)
_rs = np.random.RandomState(3)
_NONE = np.zeros((2, 0), np.int64)
CASES = {}
for _name, _n, _chords in (("897", 897, 400), ("2048", 2048, 900), ("900", 900, 400), ("hub", 1000, 400)):
    _pairs = [(i, i + 1) for i in range(_n - 1)] + [(int(a), int(b)) for a, b in _rs.randint(0, _n, (_chords, 2)) if a != b]
    if _name == "hub":                                       # atom 0 bonded to 40 atoms: more than an ELL row holds
        _pairs += [(0, 20 * i + 10) for i in range(40)]
    CASES[_name] = [(_n, _sym_edges(_pairs), _name != "hub")]
# 2,047 atoms in 45 path fragments of 20 .. 60 atoms: zero is 45-fold
_sizes = _rs.randint(20, 61, 45)
while _sizes.sum() != 2047:
    _i = _rs.randint(45)
    _sizes[_i] = min(60, max(20, _sizes[_i] + (1 if _sizes.sum() < 2047 else -1)))
_off = np.concatenate([[0], np.cumsum(_sizes)])
CASES["fragments"] = [(2047, _sym_edges([(_off[c] + i, _off[c] + i + 1) for c in range(45) for i in range(_sizes[c] - 1)]), True)]
# 1,500 atoms: a 1,000-atom component and 25 fragments of 20, atom indices shuffled over all of them
_perm = _rs.permutation(1500)
_pairs = [(i, i + 1) for i in range(999)] + [(int(a), int(b)) for a, b in _rs.randint(0, 1000, (300, 2)) if a != b]
_pairs += [(1000 + 20 * c + i, 1000 + 20 * c + i + 1) for c in range(25) for i in range(19)]
CASES["interleaved"] = [(1500, _perm[_sym_edges(_pairs)], True)]
CASES["mixed"] = [CASES.pop("900")[0], (5, _sym_edges([(0, 1), (1, 2), (3, 4)]), True), (1, _NONE, True), (12, _NONE, True)]


@pytest.mark.parametrize("case", sorted(CASES))
def test_lap_pe_large_against_numpy(case):
    """ops.lap_pe_large directly, `out` filled with a sentinel first and the graphs placed with gaps between them: status 0 and
    the bounds for every graph that goes by the book, rows outside the graphs untouched; the hub graph sets its status, leaves
    its rows alone, and meets the same bounds through graph.laplacian_pe_batched (the dense route)."""
    from singa_amd import graph as G, ops
    gs = CASES[case]
    num = [n for n, _, _ in gs]
    start = np.cumsum([3] + [n + 2 for n in num])[:-1]
    n_total = int(start[-1] + num[-1] + 4)
    ecount = [e.shape[1] for _, e, _ in gs]
    ei = np.concatenate([e for _, e, _ in gs], 1)
    t = lambda a, dt=torch.int32: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    out = torch.full((n_total, 8), SENTINEL, device=DEV)
    got, status = ops.lap_pe_large(t(ei[0]), t(ei[1]), t(np.concatenate([[0], np.cumsum(ecount)])), t(num, torch.long),
                                   t(start, torch.long), n_total, max(num), 8, out=out)
    pe, status = got.cpu().double().numpy(), status.cpu().numpy()
    inside = np.zeros(n_total, bool)
    for (n, e, ok), s, st in zip(gs, start, status):
        inside[s:s + n] = True
        assert (st == 0) == ok, (n, st)
        v = pe[s:s + n]
        if not ok:
            assert (v == SENTINEL).all()
            bt = torch.zeros(n, dtype=torch.long, device=DEV)
            v = G.laplacian_pe_batched(t(e, torch.long), bt, 1).cpu().double().numpy()
        assert np.isfinite(v).all()
        lap = _lap_np(e, n)
        w = np.linalg.eigvalsh(lap)
        kk = min(8, n - 1)
        assert np.abs(v[:, kk:]).max(initial=0.0) == 0.0                      # columns the graph is too small for
        if kk == 0:
            continue
        v = v[:, :kk]
        assert np.abs(v.T @ v - np.eye(kk)).max() < 2e-6, n
        ritz = v.T @ lap @ v
        assert np.abs(lap @ v - v @ ritz).max() < 2e-6, n
        assert np.abs(np.linalg.eigvalsh(ritz) - w[1:kk + 1]).max() < 2e-6, n
        assert (v.max(0) >= (-v).max(0) - 1e-6).all()
    assert (pe[~inside] == SENTINEL).all()


def test_small_graphs_keep_their_route_beside_a_large_one():
    """graph.laplacian_pe_batched on three bundled-size graphs + the 897-atom graph: the small graphs' rows are bit-equal to the
    rows of the batch without the large graph, and the large graph's rows are an encoding (orthonormal columns)."""
    from singa_amd import graph as G
    gs = [(300, _sym_edges([(i, i + 1) for i in range(299)])), (41, _sym_edges([(i, (i + 1) % 41) for i in range(41)])),
          (5, _sym_edges([(0, 1), (1, 2), (3, 4)])), CASES["897"][0][:2]]
    res = []
    for sub in (gs, gs[:3]):
        off = np.cumsum([0] + [n for n, _ in sub])
        ei = torch.tensor(np.concatenate([e + o for (_, e), o in zip(sub, off)], 1), device=DEV)
        bt = torch.repeat_interleave(torch.arange(len(sub)), torch.tensor([n for n, _ in sub])).to(DEV)
        res.append(G.laplacian_pe_batched(ei, bt, len(sub)).cpu())
    assert res[0].shape == (346 + 897, 8) and torch.equal(res[0][:346], res[1])
    v = res[0][346:].double()
    assert float((v.T @ v - torch.eye(8, dtype=torch.float64)).abs().max()) < 2e-6
