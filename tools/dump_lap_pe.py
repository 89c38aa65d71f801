"""Writes the Laplacian encodings of a fixed list of batches to an .npz, so that two commits can be compared bit for bit (GPU
only):  python tools/dump_lap_pe.py OUT.npz

  eig_<big>      graph.laplacian_pe_batched on the big = 0, 800, -800 and -1 batches of
                 tests/test_kernels_gpu.py::test_lap_eig_batched_against_numpy (big < 0: the sparse route forced on)
  large_<case>   ops.lap_pe_large on every case of tests/test_lap_large_gpu.py: `out` and `status`
  small_<name>   ops.lap_pe_large on the graphs of tests/test_lap_fsi_small_gpu.py: `out` and `status`
  small_sparse   graph.laplacian_pe_batched on that test's batch with the sparse route forced on

Runs on any commit that has ops.lap_pe_large when this file and tests/test_lap_fsi_small_gpu.py are copied into it;
profiles/lap_fsi_shared/README.md holds a comparison made with it."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
DEV = "cuda:0"


def collate(gs):
    off = np.cumsum([0] + [n for n, _ in gs])
    ei = torch.tensor(np.concatenate([e + o for (_, e), o in zip(gs, off)], 1), device=DEV)
    bt = torch.repeat_interleave(torch.arange(len(gs)), torch.tensor([n for n, _ in gs])).to(DEV)
    return ei, bt, len(gs)


def large(ops, gs):
    """The launch of test_lap_pe_large_against_numpy: graphs placed with gaps, `out` filled with a sentinel first."""
    num = [n for n, _ in gs]
    start = np.cumsum([3] + [n + 2 for n in num])[:-1]
    n_total = int(start[-1] + num[-1] + 4)
    ei = np.concatenate([e for _, e in gs], 1)
    t = lambda a, dt=torch.int32: torch.tensor(np.asarray(a), dtype=dt, device=DEV)
    out = torch.full((n_total, 8), -77.0, device=DEV)
    got, status = ops.lap_pe_large(t(ei[0]), t(ei[1]), t(np.concatenate([[0], np.cumsum([e.shape[1] for _, e in gs])])),
                                   t(num, torch.long), t(start, torch.long), n_total, max(num), 8, out=out)
    return got.cpu().numpy(), status.cpu().numpy()


def main():
    assert torch.cuda.is_available(), "dump_lap_pe needs a GPU"
    from singa_amd import _lib, graph as G, ops
    from tests import test_lap_fsi_small_gpu as S, test_lap_large_gpu as L
    _sym_edges = L._sym_edges
    res = {}
    # the graphs of test_lap_eig_batched_against_numpy, drawn in its order (the 1,000-atom batch is drawn and not run)
    rs = np.random.RandomState(0)
    graphs = [(300, _sym_edges([(i, i + 1) for i in range(299)])),
              (470, _sym_edges([(i, (i + 1) % 470) for i in range(470)] + [(i, (i * 7 + 3) % 470) for i in range(0, 470, 5)])),
              (240, _sym_edges([(8 * c + i, 8 * c + i + 1) for c in range(30) for i in range(7)])),
              (5, _sym_edges([(0, 1), (1, 2), (3, 4)])), (1, np.zeros((2, 0), np.int64)), (12, np.zeros((2, 0), np.int64)),
              (9, _sym_edges([(i, i + 1) for i in range(8)])),
              (10, np.concatenate([np.array([[0, 1, 2, 2, 5, 6, 7, 3, 3], [1, 2, 3, 3, 6, 7, 5, 0, 0]], np.int64),
                                   _sym_edges([(8, 9), (8, 9), (4, 8)])], 1)),
              (60, _sym_edges([(i, i + 3) for i in range(57)]))]
    try:
        for big in (0, 800, 1000, -800, -1):
            _lib.lib().singa_lap_pe_fsi_min(1 if big < 0 else 384)
            gs = list(graphs)
            if big not in (0, -1):
                n = abs(big)
                pairs = [(i, i + 1) for i in range(n - 1)] + [(int(a), int(b)) for a, b in rs.randint(0, n, (400, 2)) if a != b]
                gs = [(n, _sym_edges(pairs)), gs[0], gs[3]]
            if big != 1000:
                res[f"eig_{big}"] = G.laplacian_pe_batched(*collate(gs)).cpu().numpy()
        _lib.lib().singa_lap_pe_fsi_min(1)
        res["small_sparse"] = G.laplacian_pe_batched(*collate([S.PATH300] + [S.GRAPHS[k] for k in sorted(S.GRAPHS)])).cpu().numpy()
    finally:
        _lib.lib().singa_lap_pe_fsi_min(384)
    for case in sorted(L.CASES):
        res[f"large_{case}"], res[f"large_{case}_status"] = large(ops, [g[:2] for g in L.CASES[case]])
    for name in sorted(S.GRAPHS):
        res[f"small_{name}"], res[f"small_{name}_status"] = large(ops, [S.GRAPHS[name]])
    torch.cuda.synchronize()
    np.savez(sys.argv[1], **res)
    print("wrote", sys.argv[1], {k: (v.shape, v.tolist()) if k.endswith("_status") else v.shape for k, v in res.items()})


if __name__ == "__main__":
    main()
