"""-m gpu: the kNN edge MLPs once per undirected edge (include/singa_hip_units.h) against the float64 CPU evaluation of
Linear -> softplus - ln 2 -> Linear on the DIRECTED rows (the reference and the bounds of test_edge_mlp_pair_matches_module_path:
outputs at 2e-6 of the maximum, the eight parameter gradients at 2e-5 of the norm), bit for bit against the directed kernels,
its write footprint, and through MultiHeadAttention with the path switched on and off.

The unit lists are synthetic: a random permutation decides which rows are mates (they land in other tiles, other workgroups),
rows without a mate sit at random places of the list, and the attribute row of a unit's first row is copied onto its mate."""
import math

import pytest
import torch

from tests.helpers import cpu_f64

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = torch.nn.functional
SENTINEL = 12345.0


def unit_list(n_units, n_single, n_dropped, seed):
    """-> (E, unit_a, unit_b [E] int32 with a -1 tail, named [E] bool).  n_dropped units are left out of the list: their
    rows are named by no unit."""
    g = torch.Generator().manual_seed(seed)
    E = 2 * (n_units - n_single) + n_single
    rows = torch.randperm(E, generator=g)
    a = torch.cat([rows[:n_single], rows[n_single::2]])
    b = torch.cat([rows[:n_single], rows[n_single + 1::2]])
    order = torch.randperm(n_units, generator=g)[:n_units - n_dropped]
    a, b = a[order], b[order]
    ua, ub = torch.full((E,), -1, dtype=torch.int32), torch.full((E,), -1, dtype=torch.int32)
    ua[:a.numel()], ub[:b.numel()] = a.to(torch.int32), b.to(torch.int32)
    named = torch.zeros(E, dtype=torch.bool)
    named[a], named[b] = True, True
    return E, ua, ub, named


def problem(n_units, n_single, n_dropped, seed):
    E, ua, ub, named = unit_list(n_units, n_single, n_dropped, seed)
    torch.manual_seed(seed)
    attr = torch.randn(E, 64)
    n = int((ua >= 0).sum())
    attr[ub[:n].long()] = attr[ua[:n].long()]                       # a unit's two rows carry the same attributes
    nets = [(torch.nn.Linear(64, H, device=DEV), torch.nn.Linear(H, H, device=DEV)) for H in (32, 64)]
    keep = named[:, None].float()                                   # rows no unit names take no part: no gradient flows from them
    gk, gv = torch.randn(E, 32) * keep, torch.randn(E, 64) * keep
    return E, ua.to(DEV), ub.to(DEV), named.to(DEV), attr.to(DEV), nets, gk.to(DEV), gv.to(DEV)


def ref(a, w1k, b1k, w2k, b2k, w1v, b1v, w2v, b2v):                 # CP:41-48: Linear -> softplus - ln 2 -> Linear, both nets
    return [F.linear(F.softplus(F.linear(a, w1k, b1k)) - math.log(2.0), w2k, b2k),
            F.linear(F.softplus(F.linear(a, w1v, b1v)) - math.log(2.0), w2v, b2v)]


CASES = {"1": (1, 0, 0), "31": (31, 7, 0), "33": (33, 8, 0), "1000": (1000, 250, 0), "past_the_range_cap": (65537, 16000, 0),
         "all_singletons": (100, 100, 0), "rows_no_unit_names": (1000, 250, 37)}


@pytest.mark.parametrize("case", list(CASES))
def test_unit_path_matches_directed_rows(case):
    from singa_amd import _lib, ops
    n_units, n_single, n_dropped = CASES[case]
    E, ua, ub, named, attr, nets, gk, gv = problem(n_units, n_single, n_dropped, seed=n_units + n_single)
    n = int((ua >= 0).sum())
    assert n == n_units - n_dropped and (n < E or n_single == n_units)         # a null tail behind the units, or none at all
    if case == "past_the_range_cap":                 # the regime of test_edge_mlp_pair_past_the_range_cap: the ranges wrap
        for H in (32, 64):
            parts = _lib.lib().singa_edge_mlp_bwd_nparts(E, H)
            assert parts == _lib.lib().singa_edge_mlp_bwd_nparts(2 * E, H) and n > 128 * parts
    params = [p for l1, l2 in nets for p in (l1.weight, l1.bias, l2.weight, l2.bias)]
    want, want_g = cpu_f64(ref, [attr] + params, [gk, gv], wrt=range(1, 9))
    assert ops.USE_EDGE_UNITS
    got = ops.edge_mlp_pair(attr, nets[0], nets[1], units=(ua, ub))
    got_g = torch.autograd.grad(list(got), params, [gk, gv])
    directed = ops.edge_mlp_pair(attr, nets[0], nets[1])
    rows = named.cpu()
    figures = []
    for name, a, b, d in zip(("wk", "wv"), got, want, directed):
        assert torch.equal(a[named], d[named]), name                            # the bits of the directed kernel
        figures.append((name, float((a.detach().cpu()[rows] - b[rows]).abs().max()), 2e-6 * max(1.0, float(b[rows].abs().max()))))
    names = [f"d {net}.{p}" for net in ("k_net", "v_net") for p in ("w1", "b1", "w2", "b2")]
    for name, a, b in zip(names, got_g, want_g):
        figures.append((name, float((a.cpu() - b).norm()), 2e-5 * max(1e-6, float(b.norm()))))
    print(f"{case}: E = {E}, {n} units; " + ", ".join(f"{nm} {e:.2e} (bound {t:.2e})" for nm, e, t in figures))
    bad = [f for f in figures if not f[1] < f[2]]
    assert not bad, bad


def test_unit_entry_points_write_what_they_name():
    """wk / wv rows that no unit names keep what they held; every partial row of the backward pass is written."""
    from singa_amd import _lib
    from singa_amd.ops import _p, _stream
    lib = _lib.lib()
    E, ua, ub, named, attr, nets, gk, gv = problem(1000, 250, 37, seed=5)
    assert int((~named).sum()) > 0
    ws = [t.detach().contiguous() for l1, l2 in nets for t in (l1.weight, l1.bias, l2.weight, l2.bias)]
    wk, wv = torch.full((E, 32), SENTINEL, device=DEV), torch.full((E, 64), SENTINEL, device=DEV)
    assert lib.singa_edge_mlp_units_fwd(_p(attr), _p(ua), _p(ub), *[_p(t) for t in ws], _p(wk), _p(wv), E, 64, 32, 64, _stream()) == 0
    dk, dv = torch.empty(E, 32, device=DEV), torch.empty(E, 64, device=DEV)
    assert lib.singa_edge_mlp_fwd(_p(attr), *[_p(t) for t in ws], _p(dk), _p(dv), E, 64, 32, 64, _stream()) == 0
    for out, d in ((wk, dk), (wv, dv)):
        assert bool((out[~named] == SENTINEL).all()) and torch.equal(out[named], d[named])
    for H, g, (w1, b1, w2, _) in ((32, gk, ws[:4]), (64, gv, ws[4:])):
        parts = lib.singa_edge_mlp_bwd_nparts(E, H)
        assert parts > (int((ua >= 0).sum()) + 127) // 128                     # workgroups that find no unit at all
        part = torch.full((parts, H * 64 + H + H * H + H), float("nan"), device=DEV)
        assert lib.singa_edge_mlp_units_bwd(_p(attr), _p(ua), _p(ub), _p(g), _p(w1), _p(b1), _p(w2), _p(part), E, 64, H, _stream()) == 0
        assert not bool(torch.isnan(part).any())
        idle = part[(int((ua >= 0).sum()) + 127) // 128:]
        assert float(idle.abs().max()) == 0.0                                    # zeros, written


def test_attention_module_with_units_on_and_off():
    from singa_amd import ops
    from singa_amd.model import CProMG as CP
    torch.manual_seed(11)
    sizes = (70, 45)
    N = sum(sizes)
    pos = torch.randn(N, 3, device=DEV) * 4.0
    batch = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(sizes)]).to(DEV)
    edges = CP.KnnEdges(pos, CP.knn_graph(pos, 8, batch, len(sizes)), CP.GaussianSmearing(stop=15, num_gaussians=64, device=DEV))
    n = int((edges.unit_a >= 0).sum())
    assert n == (edges.row.numel() - N) // 2 + N and torch.equal(edges.attr[edges.unit_a[:n].long()], edges.attr[edges.unit_b[:n].long()])
    mha = CP.MultiHeadAttention(256, 64, 128, num_heads=4, device=DEV)
    x = torch.randn(N, 256, device=DEV, requires_grad=True)
    gy = torch.randn(N, 256, device=DEV)
    params = [p for p in mha.parameters()]
    runs = []
    try:
        for on in (True, False):
            ops.USE_EDGE_UNITS = on
            y = mha(x, edges)
            runs.append((y.detach(), torch.autograd.grad(y, [x] + params, gy, allow_unused=True)))
    finally:
        ops.USE_EDGE_UNITS = True
    (y1, g1), (y0, g0) = runs
    assert torch.equal(y1, y0)
    names = ["input"] + [n for n, _ in mha.named_parameters()]
    for name, a, b in zip(names, g1, g0):
        assert (a is None) == (b is None), name
        if a is not None:
            assert float((a - b).norm()) <= 2e-5 * float(b.norm()), name
