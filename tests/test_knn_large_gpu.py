"""-m gpu: singa_knn_graph_large (include/singa_hip_knn_large.h), the kNN graph kernel that streams its candidates and so takes
molecules of any size.  The order by (fp32 squared distance, atom index) is total, so the output is unique: every comparison
here is torch.equal on the int64 [2, N * k] lists, against a stable argsort on the CPU in the kernel's fp32 arithmetic."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def reference(pos, sizes, k):
    """Per molecule: fp32 differences, (dx*dx + dy*dy) + dz*dz, self at infinity, stable ascending argsort, first k; -1 elsewhere."""
    N = pos.shape[0]
    out = torch.full((2, N, k), -1, dtype=torch.int64)
    lo = 0
    for n in sizes:
        if n > 1:
            p = pos[lo:lo + n]
            df = p[:, None, :] - p[None, :, :]
            d2 = (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]
            d2.fill_diagonal_(float("inf"))
            kk = min(k, n - 1)
            out[0, lo:lo + n, :kk] = torch.arange(lo, lo + n)[:, None]
            out[1, lo:lo + n, :kk] = torch.sort(d2, dim=1, stable=True).indices[:, :kk] + lo
        lo += n
    return out.view(2, N * k)


def line(n, order):
    """n atoms on a line, 1 A apart.  up: numbered towards the far end; down: from it; far_first: as down, with atom 0 moved
    behind atom n - 1 - from atom 0 every later atom is nearer than all before it, whichever way the tiles are walked from it:
    each batch is admitted whole."""
    x = torch.arange(n, dtype=torch.float32)
    if order != "up":
        x = float(n) - x
        if order == "far_first":
            x[0] = 0.0
    return torch.stack([x, torch.zeros(n), torch.zeros(n)], 1)


CASES = {
    # absent slots, an empty and a single-atom molecule, 7 atoms of no molecule, molecules below one batch, exact ties
    "ragged": ([70, 5, 1, 0, 33, 49], 48, 7, "lattice"),
    # the first size singa_knn_graph refuses: one atom past a batch (and a tile) boundary
    "2049": ([2049], 48, 0, "random"),
    # several tiles, a ragged last tile and last batch, a small companion in the same launch
    "4100+31": ([4100, 31], 30, 0, "random"),
    # more than 8,192 atoms in the launch: two centres per wavefront; workgroups that straddle two molecules
    "4x2050": ([2050] * 4, 30, 0, "random"),
    # every distance ties: the order is the index alone, and a <= in the threshold would show
    "point": ([2304], 48, 0, "point"),
    # the best and the worst admission orders, k at its upper limit
    "line_up": ([2304], 64, 0, "up"),
    "line_down": ([2304], 64, 0, "down"),
    "line_far_first": ([2304], 64, 0, "far_first"),
}


@pytest.mark.parametrize("case", list(CASES))
def test_knn_graph_large_equals_cpu_argsort(case):
    from singa_amd import ops
    sizes, k, extra, kind = CASES[case]
    B, n_real = len(sizes), sum(sizes)
    g = torch.Generator().manual_seed(11)
    if kind in ("up", "down", "far_first"):
        pos = line(n_real, kind)
    elif kind == "point":
        pos = torch.full((n_real, 3), 1.25)
    else:
        pos = torch.rand(n_real + extra, 3, generator=g) * 30.0
        if kind == "lattice":                            # a 2 x 2 x 2 lattice corner inside molecule 0: exact ties
            pos[:8] = torch.tensor([[x, y, z] for x in (1.0, 2.0) for y in (1.0, 2.0) for z in (1.0, 2.0)])
    batch = torch.cat([torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)), torch.full((extra,), B)])
    ptr = torch.tensor([0] + sizes).cumsum(0)
    want = reference(pos, sizes, k)
    own = ops.knn_graph(pos.to(DEV), k, batch.to(DEV), ptr.to(DEV), max(sizes), route="large").cpu()
    bad = (own != want).view(2, -1, k).any(2).any(0).nonzero().view(-1)
    print(f"{case}: {bad.numel()} of {pos.shape[0]} centres differ" + (f", first {bad[:8].tolist()}" if bad.numel() else ""))
    assert torch.equal(own, want)
    if max(sizes) <= 2048:                               # both kernels accept the batch: the same integers
        assert torch.equal(ops.knn_graph(pos.to(DEV), k, batch.to(DEV), ptr.to(DEV), max(sizes), route="small").cpu(), want)


def test_prepare_and_forward_with_a_2100_atom_pocket():
    """The public path: a collated batch with a 2,100-atom pocket goes through SINGA.prepare (refused before the streaming
    kernel), the protein encoder's edges are the oracle's kNN edge set, and a forward pass at l_max 2 is finite."""
    from oracle import singa_oracle as O
    from singa_amd import graph as G
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    big = G.synthetic_graph(0, n_protein=2100, n_ligand=30, e_pp=17000, e_ll=64, e_x=118, with_lap=False)
    cpu = G.collate([big, G.synthetic_graph(1, with_lap=False)])
    cfg = load_config(lmax=2)
    g = torch.Generator().manual_seed(3)
    for nt in (G.PA, G.LA):                              # the encodings are an input here (the dense eigensolver's turn above 2,048)
        cpu.nodes[nt]["lap_pe"] = torch.randn(cpu[nt]["x"].shape[0], cfg.model.encoder.lap_dim, generator=g)
    pos, bt = cpu[G.PA]["pos"], cpu[G.PA]["batch"]
    batch = cpu.to(DEV)
    model = SINGA(cfg, device=DEV)
    model.eval()
    prep = model.prepare(batch)
    e = prep["p"]["edges"]
    row, col, _ = O.knn_edges(pos, O.knn_graph(pos, 48, bt), 15.0, 64)
    N = pos.shape[0]
    assert torch.equal(torch.sort(e.row.cpu() * N + e.col.cpu()).values, torch.sort(row * N + col).values)
    with torch.no_grad():
        logits = model(batch)
    assert torch.isfinite(logits).all()
