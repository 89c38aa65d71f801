"""-m gpu: the filtered subspace iteration under both Laplacian kernels (lap_fsi_iterate) at the smallest shapes at which its
pieces can go wrong: a block of 16 vectors in a space barely larger than the block, and fewer rows than threads.  Two graphs:
a 33-atom ring with 16 chords (one component: the large kernel writes one zero and solves for 8 pairs) and 40 atoms in two
components, a chorded ring of 25 and a chorded path of 15 (the large kernel projects two null vectors out and the zeros merge
in front of 7 Ritz values).  Both go through ops.lap_pe_large, and through the small kernel's sparse route forced on beside the
300-atom path (ld = 300 >= 266: the iteration's matrices need 4 * ld >= 1,064 doubles of LDS).  Bounds: the basis-free ones of
test_lap_large_gpu / test_kernels_gpu.test_lap_eig_batched_against_numpy.
Inputs: checked with numpy that eigenvalues 8 and 9 are 5.1e-2 (ring) and 3.6e-2 (two components) apart, far above 1e-4; and
checked on the parent commit that singa_lap_pe_large returns status 0 for both (profiles/lap_fsi_shared/README.md).
The ring's chords are chosen for that status.  With 32 non-zero eigenvalues the block's 16th Ritz value is the middle of the
spectrum (~1), so once the block has turned towards the Ritz vectors the degree-24 filter amplifies its lowest mode ~1e13
times more than its 16th, and the Gram matrix's smallest Cholesky pivot lands next to the 1e-26 of the trace that the pivot rule
asks for: a ring with four chords, (0, 7) (3, 19) (11, 28) (14, 22), and two with 6 and 12 chords give up on the parent commit
(status 2: the caller's dense route answers), as most sparse 33-atom rings do.  The 16 chords below raise the smallest non-zero
eigenvalue to 0.13 and go by the book, on the parent commit and on this one with the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77.0


def _sym_edges(pairs):
    a, b = np.asarray(pairs, dtype=np.int64).reshape(-1, 2).T
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])])


def _lap_np(ei, n):
    a = np.zeros((n, n))
    a[ei[0], ei[1]] = 1.0
    dinv = np.clip(a.sum(0), 1, None) ** -0.5
    lap = np.eye(n) - dinv[:, None] * a * dinv[None, :]
    return 0.5 * (lap + lap.T)


GRAPHS = {
    "ring33": (33, _sym_edges([(i, (i + 1) % 33) for i in range(33)]
                              + [(0, 26), (1, 26), (2, 7), (3, 8), (3, 31), (6, 12), (6, 21), (7, 14), (7, 20), (10, 25), (12, 26),
                                 (13, 15), (15, 28), (20, 23), (21, 25), (22, 32)])),
    "two40": (40, _sym_edges([(i, (i + 1) % 25) for i in range(25)] + [(0, 9), (4, 17), (12, 21)]
                             + [(25 + i, 26 + i) for i in range(14)] + [(25, 31), (28, 38)])),
}
PATH300 = (300, _sym_edges([(i, i + 1) for i in range(299)]))


def _check(v, n, e):
    """The basis-free bounds for one graph's rows v [n, 8] (float64)."""
    assert np.isfinite(v).all()
    lap = _lap_np(e, n)
    w = np.linalg.eigvalsh(lap)
    assert w[9] - w[8] >= 1e-4
    assert np.abs(v.T @ v - np.eye(8)).max() < 2e-6, n
    ritz = v.T @ lap @ v
    assert np.abs(lap @ v - v @ ritz).max() < 2e-6, n
    assert np.abs(np.linalg.eigvalsh(ritz) - w[1:9]).max() < 2e-6, n
    assert (v.max(0) >= (-v).max(0) - 1e-6).all()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_large_kernel_block_barely_fits(name):
    """ops.lap_pe_large on one graph placed between sentinel rows: status 0, the bounds, the other rows untouched."""
    from singa_amd import ops
    n, e = GRAPHS[name]
    t = lambda a, dt=torch.int32: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    out = torch.full((n + 7, 8), SENTINEL, device=DEV)
    got, status = ops.lap_pe_large(t(e[0]), t(e[1]), t([0, e.shape[1]]), t([n], torch.long), t([3], torch.long), n + 7, n, 8, out=out)
    pe = got.cpu().double().numpy()
    assert int(status[0]) == 0
    _check(pe[3:3 + n], n, e)
    assert (pe[:3] == SENTINEL).all() and (pe[3 + n:] == SENTINEL).all()


def test_small_kernel_sparse_route_block_barely_fits():
    """graph.laplacian_pe_batched on the 300-atom path and both graphs with the sparse route forced on every graph of more than 32
    atoms: the bounds for each graph."""
    from singa_amd import _lib, graph as G
    gs = [PATH300] + [GRAPHS[k] for k in sorted(GRAPHS)]
    off = np.cumsum([0] + [n for n, _ in gs])
    ei = torch.tensor(np.concatenate([e + o for (_, e), o in zip(gs, off)], 1), device=DEV)
    bt = torch.repeat_interleave(torch.arange(len(gs)), torch.tensor([n for n, _ in gs])).to(DEV)
    _lib.lib().singa_lap_pe_fsi_min(1)
    try:
        pe = G.laplacian_pe_batched(ei, bt, len(gs)).cpu().double().numpy()
    finally:
        _lib.lib().singa_lap_pe_fsi_min(384)
    assert pe.shape == (373, 8)
    for (n, e), o in zip(gs[1:], off[1:]):
        _check(pe[o:o + n], n, e)
