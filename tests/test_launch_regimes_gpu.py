"""-m gpu: the training kernels in the launch regimes the product runs in and the small-shape kernel tests never reach -
past their grid caps (grid-stride loops that wrap, per-part partial rows that hold several strides, node runs longer
than the minimum), on degenerate segment layouts, and the column-sum kernels checked exactly.

Every case asserts that its regime was reached (the library's own sizing function has saturated and the size exceeds
what the capped grid covers in one stride), evaluates the torch formulation of the existing small-shape test of the
same kernel in float64 on the CPU, and compares outputs and ALL gradients per row (tests.helpers.rowwise_err: one wrong
tail edge or one skipped stride is not diluted by the row count) with the bound the small-shape test uses.  Measured on
MI355X every figure stays below a quarter of its bound.  A gather_rotate kernel that stops after its first grid stride, or an
rmsnorm backward that forgets all strides but the last in its partial rows, fails here and passes tests/test_kernels_gpu.py.

The no-edges layouts failed before this module existed: the five segment ops handed the address of an empty tensor (0) to
the library, which refuses null pointers; singa_amd.ops now answers an empty edge set without a launch.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import singa_oracle as O
from oracle import so3_tables as T
from singa_amd import so3
from tests.helpers import cpu_f64, rowwise_err
from tests.test_kernels_gpu import rad_row_index, rand_rot

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = torch.nn.functional


def _ops():
    from singa_amd import ops
    return ops


def _lib():
    from singa_amd import _lib as L
    return L.lib()


def dev_leaf(t):
    return t.detach().float().to(DEV).requires_grad_(True)


def check_rows(tag, pairs):
    """pairs: (name, got, want, bound).  Prints every figure, then asserts all of them."""
    bad = []
    for name, got, want, tol in pairs:
        e = rowwise_err(got, want, f"{tag} {name} (bound {tol:.0e})")
        if not e <= tol:
            bad.append((name, e, tol))
    assert not bad, (tag, bad)


def wigner_fwd_inv(wr, L, M=2):
    """The rotation matrices the kernels apply, rebuilt from the reduced Wigner rows `wr` [E, WSZ] THEY read (float64 copies
    of the float32 records: the Wigner kernel has its own test): fwd [E, KR, K] (rotate, EF:485-505) and inv [E, K, KR]
    (rotate_inv with its rescale) as oracle.Frame holds them."""
    wr = wr.detach().cpu().double()
    E, K = wr.shape[0], (L + 1) ** 2
    rows, off = [], 0
    for l in range(L + 1):
        nr, nc = 2 * min(l, M) + 1, 2 * l + 1
        full = torch.zeros(E, nr, K, dtype=torch.float64)
        full[:, :, l * l:(l + 1) ** 2] = wr[:, off:off + nr * nc].reshape(E, nr, nc)
        rows.append(full)
        off += nr * nc
    fwd = torch.cat(rows, 1)
    inv = fwd.transpose(1, 2) * torch.as_tensor(np.asarray(T.rotate_inv_rescale(L, M)), dtype=torch.float64)
    return fwd, inv


# --------------------------------------------------------------------------------------------------- gather_rotate (k3-k6)
@pytest.mark.parametrize("L", [2, 6])
@pytest.mark.parametrize("E", [8193, 16421])
def test_gather_rotate_past_the_grid_cap(E, L):
    """Forward and d-rad run on grid_for(E) workgroups - capped at 8192 (grid_for's default cap in singa_hip.hip, not
    exported) - and walk the edges with e += gridDim.x: from E = 8193 on a workgroup handles more than one edge.  Hetero
    edge set (Ns != Nd), one hub node of 2000 edges on each side, ~10 % of the nodes of each side without edges."""
    assert E > 8192                                        # grid_for(E) in singa_gather_rotate_fwd / _bwd: cap 256 * 32
    ops = _ops()
    rs = np.random.RandomState(E + L)
    C, Ns, Nd = 16, 600, 900
    lay = so3.layout(L, 2)
    live_s, live_d = rs.permutation(Ns)[:int(0.9 * Ns)], rs.permutation(Nd)[:int(0.9 * Nd)]
    src, dst = live_s[rs.randint(0, len(live_s), E)], live_d[rs.randint(0, len(live_d), E)]
    dst[:2000], src[-2000:] = live_d[0], live_s[0]
    es = ops.EdgeSet(torch.tensor(np.stack([src, dst]), dtype=torch.int64).to(DEV), Ns, Nd)
    src_s, dst_s = es.src64.cpu(), es.dst64.cpu()          # the destination-sorted order the kernels work in
    deg_s, deg_d = torch.bincount(src_s, minlength=Ns), torch.bincount(dst_s, minlength=Nd)
    assert int(deg_d.max()) >= 2000 and int(deg_s.max()) >= 2000
    assert int((deg_s == 0).sum()) >= Ns // 10 and int((deg_d == 0).sum()) >= Nd // 10
    wr = ops.wigner_rows(rand_rot(rs, E).to(DEV), L)
    fwd, _ = wigner_fwd_inv(wr, L)
    xs = torch.tensor(rs.randn(Ns, lay.K, C), dtype=torch.float32)
    xd = torch.tensor(rs.randn(Nd, lay.K, C), dtype=torch.float32)
    rad = torch.tensor(rs.randn(E, lay.rad_rows * 2 * C), dtype=torch.float32)
    g = torch.tensor(rs.randn(E, lay.KR * 2 * C), dtype=torch.float32)
    to_m, rri = torch.as_tensor(lay.to_m), rad_row_index(lay)

    def ref(xs_, xd_, rad_):
        return (torch.bmm(fwd, torch.cat([xs_[src_s], xd_[dst_s]], 2))[:, to_m]
                * rad_.view(E, lay.rad_rows, 2 * C)[:, rri]).reshape(E, -1)
    want, (w_xs, w_xd, w_rad) = cpu_f64(ref, (xs, xd, rad), g)
    xs_g, xd_g, rad_g = dev_leaf(xs), dev_leaf(xd), dev_leaf(rad)
    out = ops.gather_rotate(xs_g, xd_g, rad_g, wr, es, L)
    out.backward(g.to(DEV))
    check_rows(f"gather_rotate E={E} L={L}", [("out", out, want, 2e-5), ("d x_src", xs_g.grad, w_xs, 2e-5),
                                              ("d x_dst", xd_g.grad, w_xd, 2e-5), ("d rad", rad_g.grad, w_rad, 2e-5)])


# --------------------------------------------------------------------------------------------------------- so3_rmsnorm (k12)
@pytest.mark.parametrize("L", [2, 6])
@pytest.mark.parametrize("N", [32769, 65541])
def test_so3_rmsnorm_past_the_wave_cap(N, L):
    """rmsnorm_fwd4 / bwd4: one wavefront per four nodes, at most singa_so3_rmsnorm_nparts = 8192 wavefronts; beyond 32768
    nodes a wavefront walks several strides and its gw_part / gb_part row holds the sum over all of them."""
    ops, lib = _ops(), _lib()
    nparts = lib.singa_so3_rmsnorm_nparts(N)
    assert nparts == lib.singa_so3_rmsnorm_nparts(2 * N) and N > 4 * nparts        # saturated, and more than one stride
    rs = np.random.RandomState(N % 1000 + L)
    C, K = 16, (L + 1) ** 2
    x = torch.tensor(rs.randn(N, K, C) * 2 + 0.3, dtype=torch.float32)
    w = torch.tensor(1 + 0.1 * rs.randn(L + 1, C), dtype=torch.float32)
    b = torch.tensor(0.1 * rs.randn(C), dtype=torch.float32)
    g = torch.tensor(rs.randn(N, K, C), dtype=torch.float32)
    g2 = torch.tensor(rs.randn(N, K, C), dtype=torch.float32)
    want, (w_x, w_w, w_b) = cpu_f64(lambda x_, w_, b_: O.rms_norm({"n.affine_weight": w_, "n.affine_bias": b_}, "n", x_, L),
                                    (x, w, b), g)
    xg, wg, bg = dev_leaf(x), dev_leaf(w), dev_leaf(b)
    y = ops.so3_rmsnorm(xg, wg, bg, L)
    y.backward(g.to(DEV))
    tag = f"so3_rmsnorm N={N} L={L}"
    check_rows(tag, [("y", y, want, 1e-5), ("d x", xg.grad, w_x, 2e-5), ("d weight", wg.grad, w_w, 2e-5),
                     ("d bias", bg.grad, w_b, 2e-5)])
    # the norm + residual node: the backward kernel adds the skip's gradient itself
    xs, ws, bs = dev_leaf(x), dev_leaf(w), dev_leaf(b)
    y2, skip = ops.so3_rmsnorm_skip(xs, ws, bs, L)
    assert torch.equal(y2, y) and torch.equal(skip, xs)
    torch.autograd.backward([y2, skip], [g.to(DEV), g2.to(DEV)])
    check_rows(tag + " skip", [("d x", xs.grad, w_x + g2.double(), 2e-5), ("d weight", ws.grad, w_w, 2e-5),
                               ("d bias", bs.grad, w_b, 2e-5)])


# ------------------------------------------------------------------------------------------------------- edge_head (k9a + k8)
def sep_s2_act64(gate, x, L, M):
    """oracle.sep_s2_act (SeparableS2Activation, EF:1736-1773) with the grid matrices in the inputs' dtype (the oracle pins
    them to float32)."""
    to, fr = (torch.as_tensor(np.asarray(a), dtype=x.dtype) for a in T.s2_grid_mats(L, M))
    grid = F.silu(torch.einsum("bai,zic->zbac", to, x))
    y = torch.einsum("bai,zbac->zic", fr, grid)
    return torch.cat([F.silu(gate).unsqueeze(1), y[:, 1:]], 1)


@pytest.mark.parametrize("E", [16385, 32771])
def test_edge_head_past_the_slot_cap(E):
    """alpha_logits_fwd / bwd: singa_alpha_logits_nslots caps the grid at 16384 edge slots; beyond that a slot walks several
    edges and its partial row of (d ln_w, d ln_b, d alpha_dot) sums them."""
    ops, lib = _ops(), _lib()
    nslots = lib.singa_alpha_logits_nslots(E)
    assert nslots == lib.singa_alpha_logits_nslots(2 * E) and E > nslots
    rs = np.random.RandomState(E % 1000)
    L, heads, A, C = 2, 7, 32, 128
    lay = so3.layout(L, 2)
    h0 = torch.tensor(rs.randn(E, heads * A + C + lay.seg_rows[0] * C), dtype=torch.float32)
    h1 = torch.tensor(rs.randn(E, lay.seg_rows[1] * C), dtype=torch.float32)
    h2 = torch.tensor(rs.randn(E, lay.seg_rows[2] * C), dtype=torch.float32)
    w = torch.tensor(1 + 0.2 * rs.randn(A), dtype=torch.float32)
    b = torch.tensor(0.2 * rs.randn(A), dtype=torch.float32)
    dot = torch.tensor(rs.randn(heads, A) * 0.2, dtype=torch.float32)
    g1 = torch.tensor(rs.randn(E, heads), dtype=torch.float32)
    to_m = torch.as_tensor(lay.to_m)
    g2 = torch.tensor(rs.randn(E, lay.KR * C), dtype=torch.float32)

    def ref(h0_, h1_, h2_, w_, b_, dot_):
        a = F.layer_norm(h0_[:, :heads * A].reshape(-1, heads, A), (A,), w_, b_, 1e-5)
        a = 0.6 * a + 0.4 * a * (2 * torch.sigmoid(a) - 1)
        xm = torch.cat([h0_[:, heads * A + C:].view(E, -1, C), h1_.view(E, -1, C), h2_.view(E, -1, C)], 1)
        act = sep_s2_act64(h0_[:, heads * A:heads * A + C], xm[:, torch.argsort(to_m)], L, 2)[:, to_m].reshape(E, -1)
        return [(a * dot_).sum(-1), act]
    (w_logits, w_act), w_g = cpu_f64(ref, (h0, h1, h2, w, b, dot), [g1, g2])
    dev = [dev_leaf(t) for t in (h0, h1, h2, w, b, dot)]
    logits, act = ops.edge_head(*dev, heads, A, C, L)
    torch.autograd.backward([logits, act], [g1.to(DEV), g2.to(DEV)])
    names = ("d h0", "d h1", "d h2", "d ln_w", "d ln_b", "d alpha_dot")
    check_rows(f"edge_head E={E}", [("logits", logits, w_logits, 2e-5), ("act", act, w_act, 2e-5)] +
               [(n, d.grad, r, 1e-4) for n, d, r in zip(names, dev, w_g)])


# --------------------------------------------------------------------------------------------------------- edge_mlp_pair (k15c)
@pytest.mark.parametrize("E", [65537, 140003])
def test_edge_mlp_pair_past_the_range_cap(E):
    """edge_mlp_mfma_bwd: singa_edge_mlp_bwd_nparts caps the edge ranges (128 edges each) at 512 for H = 32 and 256 for
    H = 64; beyond 65536 edges BOTH nets' ranges wrap and every partial row sums several ranges."""
    ops, lib = _ops(), _lib()
    for H in (32, 64):
        n = lib.singa_edge_mlp_bwd_nparts(E, H)
        assert n == lib.singa_edge_mlp_bwd_nparts(2 * E, H) and E > 128 * n
    torch.manual_seed(E)
    attr = torch.randn(E, 64, device=DEV)
    nets = [(torch.nn.Linear(64, H, device=DEV), torch.nn.Linear(H, H, device=DEV)) for H in (32, 64)]
    gk, gv = torch.randn(E, 32, device=DEV), torch.randn(E, 64, device=DEV)
    params = [p for l1, l2 in nets for p in (l1.weight, l1.bias, l2.weight, l2.bias)]

    def ref(a, w1k, b1k, w2k, b2k, w1v, b1v, w2v, b2v):       # CP:41-48: Linear -> softplus - ln 2 -> Linear, both nets
        return [F.linear(F.softplus(F.linear(a, w1k, b1k)) - math.log(2.0), w2k, b2k),
                F.linear(F.softplus(F.linear(a, w1v, b1v)) - math.log(2.0), w2v, b2v)]
    want, want_g = cpu_f64(ref, [attr] + params, [gk, gv], wrt=range(1, 9))
    got = ops.edge_mlp_pair(attr, nets[0], nets[1])
    got_g = torch.autograd.grad(list(got), params, [gk, gv])
    names = [f"d {net}.{p}" for net in ("k_net", "v_net") for p in ("w1", "b1", "w2", "b2")]
    check_rows(f"edge_mlp_pair E={E}", [("wk", got[0], want[0], 2e-6), ("wv", got[1], want[1], 2e-6)] +
               [(n, a, b, 2e-5) for n, a, b in zip(names, got_g, want_g)])


# ------------------------------------------------------------------------------------------------- so3_linear through k11s
# L = 4 (the flagship workload's degree) only: L = 6 at these N is ~3 GB of float64 per tensor on the CPU side, and with L = 2
# as well this test alone took 19 s of float64 CPU reference, three times the whole of tests/test_kernels_gpu.py
@pytest.mark.parametrize("L", [4])
@pytest.mark.parametrize("N", [12289, 16401, "sized-by-the-library"])
@pytest.mark.parametrize("cin,cout", [(16, 512), (512, 16), (112, 16)])
def test_so3_linear_skinny_long_node_runs(cin, cout, N, L):
    """so3_skinny_expand / _reduce (both singa_so3_skinny_variant settings): a workgroup handles 8 nodes until the node count
    exceeds 8 x its target grid; beyond that the runs grow (and the MFMA variant rounds them to 16-node tiles).  N is not a
    multiple of 16, so the last run and the last tile are partial.

    The expand kernels aim at 1536 runs, their MFMA variant at 2048 (so3_skinny_npb's targets in singa_so3_skinny_expand, not
    exported): N = 12289 lengthens the runs of the first, N = 16401 of both.  The reduction's target is what the device runs
    in one round (so3_skinny_reduce_runs: occupancy x compute units, exported through singa_so3_skinny_nparts): 256 and 512
    without a device, but on an MI355X 1366 for 112 channels at L = 4 (12289 nodes make runs of 9) and 2051 at L = 2 (16401
    nodes still make runs of 8).  The third size is therefore taken from the sizing function itself: the first
    N = 12289 + 2048 k with more than 9 nodes per run."""
    ops, lib = _ops(), _lib()
    wide = max(cin, cout)
    per_run = lambda n: n / lib.singa_so3_skinny_nparts(n, L, wide)
    if isinstance(N, str):
        N = 12289
        while per_run(N) <= 9:
            N += 2048
        if N == 12289:                                     # the fixed sizes are in the reduction's regime already (asserted there)
            return
        assert per_run(N) > 8 and N < 200000
    else:
        # more than the minimum 8 nodes per workgroup: in the expand kernels by N alone, in the reduction by its sizing
        # function - or the library-sized case of this (cin, cout, L) takes over, which then must not return early
        assert N > 8 * 1536 and (per_run(N) > 8 or per_run(12289) <= 9)
    assert N % 16
    print(f"so3_linear {cin}->{cout} L={L}: N = {N}, {per_run(N):.2f} nodes per reduction run")
    K = (L + 1) ** 2
    g = torch.Generator().manual_seed(N + L + cin)
    x = torch.randn(N, K, cin, generator=g)
    w = torch.randn(L + 1, cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    gy = torch.randn(N, K, cout, generator=g)
    want, (w_x, w_w, w_b) = cpu_f64(lambda x_, w_, b_: O.so3_linear({"p.weight": w_, "p.bias": b_}, "p", x_, L), (x, w, b), gy)
    assert ops.USE_SKINNY_SO3
    for valu in (0, 1):
        lib.singa_so3_skinny_variant(valu)
        try:
            xd, wd, bd = dev_leaf(x), dev_leaf(w), dev_leaf(b)
            got = ops.so3_linear(xd, wd, bd, L)
            got.backward(gy.to(DEV))
            check_rows(f"so3_linear {cin}->{cout} N={N} L={L} variant={valu}",
                       [("out", got, want, 2e-6), ("d x", xd.grad, w_x, 5e-6), ("d weight", wd.grad, w_w, 1e-5),
                        ("d bias", bd.grad, w_b, 1e-5)])
        finally:
            lib.singa_so3_skinny_variant(0)


# ----------------------------------------------------------------------------------------------- degenerate segment layouts
def segment_layouts():
    """(name, N, sorted segment ids): layouts the random graphs of the small-shape tests cannot produce."""
    rs = np.random.RandomState(12)
    return [("first-and-last-empty", 12, np.sort(rs.randint(1, 11, 300))), ("all-on-one-node", 9, np.full(200, 4)),
            ("one-node", 1, np.zeros(70, np.int64)), ("no-edges", 5, np.zeros(0, np.int64))]


LAYOUTS = segment_layouts()
LAYOUT_IDS = [l[0] for l in LAYOUTS]


def row_ptr_of(ids, N):
    rp = torch.zeros(N + 1, dtype=torch.int64)
    rp[1:] = torch.bincount(torch.as_tensor(ids, dtype=torch.int64), minlength=N).cumsum(0)
    return rp.to(torch.int32).to(DEV)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_segment_softmax_and_wsum_degenerate_layouts(layout):
    name, N, ids = layout
    ops = _ops()
    E = len(ids)
    if E:
        assert ids[0] > 0 and ids[-1] < N - 1 or len(set(ids.tolist())) == 1
    rs = np.random.RandomState(N)
    dst, rp = torch.as_tensor(ids, dtype=torch.int64), row_ptr_of(ids, N)
    for H, eps in ((7, 1e-16), (4, 0.0)):
        x = torch.tensor(rs.randn(E, H) * 4, dtype=torch.float32)
        g = torch.tensor(rs.randn(E, H), dtype=torch.float32)
        want, (w_x,) = cpu_f64(lambda x_: O.seg_softmax(x_, dst, N, eps), (x,), g)
        xg = dev_leaf(x)
        y = ops.segment_softmax(xg, rp, eps)
        y.backward(g.to(DEV))
        assert y.shape == (E, H) and xg.grad.shape == (E, H)
        assert float((y.detach().cpu().double() - want).abs().max() if E else 0.0) < 1e-6
        # d x: the small-shape test's 1e-5 is a GLOBAL relative norm.  Per edge row (H values, many of them ~1e-7 of the
        # segment's mass at logits of spread 4) it is below what float32 can give: the same formulation (oracle.seg_softmax +
        # autograd) evaluated in float32 on the CPU has rowwise_err 3.7e-5 (H = 4) / 2.0e-5 (H = 7) against float64 on the
        # first-and-last-empty layout, 2.8e-6 / 1.1e-6 on the other two (global: 5e-7).  Bound = 4 x 3.7e-5.
        check_rows(f"segment_softmax {name} H={H}", [("y", y, want, 1e-5), ("d x", xg.grad, w_x, 1.5e-4)])
    H, Fv = 4, 64
    w = torch.tensor(rs.rand(E, H), dtype=torch.float32)
    v = torch.tensor(rs.randn(E, H, Fv), dtype=torch.float32)
    g = torch.tensor(rs.randn(N, H, Fv), dtype=torch.float32)
    want, (w_w, w_v) = cpu_f64(lambda w_, v_: O.seg_sum(w_.unsqueeze(-1) * v_, dst, N), (w, v), g)
    wg, vg = dev_leaf(w), dev_leaf(v)
    out = ops.segment_wsum(wg, vg, rp)
    out.backward(g.to(DEV))
    assert out.shape == (N, H, Fv) and wg.grad.shape == w.shape and vg.grad.shape == v.shape
    if E == 0:
        assert float(out.detach().abs().max()) == 0.0
    check_rows(f"segment_wsum {name}", [("out", out, want, 1e-5), ("d w", wg.grad, w_w, 1e-5), ("d v", vg.grad, w_v, 1e-6)])


@pytest.mark.parametrize("L", [2, 6])
@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_rotate_back_scatter_degenerate_layouts(layout, L):
    name, Nd, ids = layout
    ops = _ops()
    E, Ns, CH, heads = len(ids), 7, 112, 7
    rs = np.random.RandomState(Nd + L)
    lay = so3.layout(L, 2)
    ei = torch.tensor(np.stack([rs.randint(0, Ns, E), ids]), dtype=torch.int64)
    es = ops.EdgeSet(ei.to(DEV), Ns, Nd)
    dst = es.dst64.cpu()
    assert torch.equal(dst, torch.as_tensor(ids, dtype=torch.int64))
    wr = ops.wigner_rows(rand_rot(rs, E).to(DEV), L) if E else torch.zeros(0, lay.WSZ, device=DEV)
    _, inv = wigner_fwd_inv(wr, L)
    to_l = torch.argsort(torch.as_tensor(lay.to_m))
    parts = [torch.tensor(rs.randn(E, r * CH), dtype=torch.float32) for r in lay.seg_rows]
    alpha = torch.tensor(rs.rand(E, heads), dtype=torch.float32)
    g = torch.tensor(rs.randn(Nd, lay.K, CH), dtype=torch.float32)

    def ref(p0, p1, p2, al):
        msg = torch.cat([p.view(E, r, CH) for p, r in zip((p0, p1, p2), lay.seg_rows)], 1)[:, to_l]
        msg = (msg.view(E, lay.KR, heads, CH // heads) * al.view(E, 1, heads, 1)).reshape(E, lay.KR, CH)
        return O.seg_sum(torch.bmm(inv, msg), dst, Nd)
    want, w_g = cpu_f64(ref, (*parts, alpha), g)
    dev = [dev_leaf(t) for t in (*parts, alpha)]
    out = ops.rotate_back_scatter(dev[0], dev[1], dev[2], dev[3], wr, es, heads, L)
    out.backward(g.to(DEV))
    assert out.shape == (Nd, lay.K, CH) and all(d.grad.shape == d.shape for d in dev)
    if E == 0:
        assert float(out.detach().abs().max()) == 0.0
    else:
        empty = torch.bincount(dst, minlength=Nd) == 0
        assert float(out.detach()[empty.to(DEV)].abs().max() if bool(empty.any()) else 0.0) == 0.0     # nodes without edges: exact zeros
    check_rows(f"rotate_back_scatter {name} L={L}", [("out", out, want, 2e-5)] +
               [(f"d y{i}", d.grad, r, 2e-5) for i, (d, r) in enumerate(zip(dev[:3], w_g[:3]))] +
               [("d alpha", dev[3].grad, w_g[3], 5e-5)])


class AttentionEdges:
    """The edge bundle ops.edge_logits / ops.gather_wsum read: row-sorted edges, CSR / CSC pointers, the column-sorted order."""

    def __init__(self, row, col, N):
        row, col = torch.as_tensor(row, dtype=torch.int64), torch.as_tensor(col, dtype=torch.int64)
        self.row_ptr = row_ptr_of(row, N)
        self.col_ptr = row_ptr_of(col, N)
        self.row32, self.col32 = row.to(torch.int32).to(DEV), col.to(torch.int32).to(DEV)
        self.eperm = torch.argsort(col, stable=True).to(torch.int32).to(DEV)


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_graph_attention_degenerate_layouts(layout):
    """edge_logits / gather_wsum (CP:59-74) with the segment layout on the row side and, transposed, on the column side."""
    name, N, ids = layout
    ops = _ops()
    E, H, D, Fv = len(ids), 4, 32, 64
    rs = np.random.RandomState(N + 40)
    scale = 1.0 / math.sqrt(D)
    t = lambda *s: torch.tensor(rs.randn(*s), dtype=torch.float32)
    for side in ("rows", "columns"):
        other = rs.randint(0, N, E)
        if side == "rows":
            row, col = np.asarray(ids), other
        else:
            o = np.argsort(other, kind="stable")
            row, col = other[o], np.asarray(ids)[o]
        e = AttentionEdges(row, col, N)
        row_t, col_t = torch.as_tensor(row, dtype=torch.int64), torch.as_tensor(col, dtype=torch.int64)
        q, hk, wk, wkl, bkl = t(N, H, D), t(N, H, D), t(E, D), t(D, D), t(D)
        g = t(E, H)
        want, w_g = cpu_f64(lambda q_, hk_, wk_, wkl_, bkl_:
                            (q_[row_t] * F.linear(wk_.unsqueeze(1) * hk_[col_t], wkl_, bkl_)).sum(-1) * scale,
                            (q, hk, wk, wkl, bkl), g)
        dev = [dev_leaf(x) for x in (q, hk, wk, wkl, bkl)]
        qg, hkg, wkg, wklg, bklg = dev
        out = ops.edge_logits(torch.matmul(qg, wklg), wkg, hkg, (qg * bklg).sum(-1) * scale, e, scale)
        out.backward(g.to(DEV))
        assert out.shape == (E, H)
        check_rows(f"edge_logits {name} on {side}", [("out", out, want, 1e-5)] +
                   [(f"d {n}", d.grad, r, 2e-5) for n, d, r in zip(("q", "hk", "wk", "wk_lin.weight", "wk_lin.bias"), dev, w_g)])
        alpha, hv, wv, wvl = torch.tensor(rs.rand(E, H), dtype=torch.float32), t(N, H, Fv), t(E, Fv), t(Fv, Fv)
        g = t(N, H, Fv)
        want, w_g = cpu_f64(lambda a_, hv_, wv_, wvl_: torch.zeros(N, H, Fv, dtype=a_.dtype).index_add_(
            0, row_t, a_.unsqueeze(-1) * F.linear(wv_.unsqueeze(1) * hv_[col_t], wvl_)), (alpha, hv, wv, wvl), g)
        dev = [dev_leaf(x) for x in (alpha, hv, wv, wvl)]
        out = F.linear(ops.gather_wsum(dev[0], dev[2], dev[1], e), dev[3], None)
        out.backward(g.to(DEV))
        assert out.shape == (N, H, Fv)
        if E == 0:
            assert float(out.detach().abs().max()) == 0.0
        check_rows(f"gather_wsum {name} on {side}", [("out", out, want, 1e-5)] +
                   [(f"d {n}", d.grad, r, 2e-5) for n, d, r in zip(("alpha", "hv", "wv", "wv_lin.weight"), dev, w_g)])


# ------------------------------------------------------------------------------------------------------ column sums, exactly
# Integer-valued float32 inputs from -8 .. 8: every partial sum is an integer below 2^24 (300001 rows x 8 = 2.4e6), so the
# float32 result is exact in any summation order and one dropped, doubled or misplaced row changes it.
COLSUM_M = [1, 16, 17, 2048, 2049, 4097, 8193, 16384, 16385, 40000, 300001]


def int_valued(shape, gen):
    return torch.randint(-8, 9, shape, generator=gen).float()


def first_pass_rows(M):
    """The rows per first-pass slab (colsum_first_r in singa_hip.hip: 16 .. 128) and the number of passes, recovered from
    the exported workspace size singa_colsum_work(M, 1) = ceil(M / r) + ceil(ceil(M / r) / 128) + 2."""
    ceil = lambda a, b: -(-a // b)
    work = _lib().singa_colsum_work(M, 1) - 2
    fits = [r for r in (16, 32, 64, 128) if ceil(M, r) + ceil(ceil(M, r), 128) == work]
    assert len(fits) == 1 or (M <= 16 and 16 in fits), (M, work, fits)
    r = fits[0]
    s1 = ceil(M, r)
    return r, 1 if s1 == 1 else (2 if s1 <= 128 else 3)


def test_colsum_sizes_cover_every_first_pass_class():
    classes = {first_pass_rows(M) for M in COLSUM_M if M > 16}
    assert {r for r, _ in classes} == {16, 32, 64, 128}
    assert {p for _, p in classes} == {2, 3} and first_pass_rows(16)[1] == 1
    assert first_pass_rows(16384) == (128, 2) and first_pass_rows(16385) == (128, 3)


@pytest.mark.parametrize("M", COLSUM_M)
def test_colsum_is_exact(M):
    ops = _ops()
    gen = torch.Generator().manual_seed(M)
    for n in (1, 7, 256, 1028):
        if M > 16385 and n > 256:                          # the two largest M only with n <= 256 (memory and CPU time)
            continue
        for ld in ((n, n + 5) if n in (7, 256) else (n,)): # ld > n: a column block of a wider tensor
            wide = int_valued((M, ld), gen)
            x = wide.to(DEV)[:, ld - n:]
            assert x.stride(0) == ld and x.shape == (M, n)
            got = ops.colsum(x)
            want = wide[:, ld - n:].to(torch.int64).sum(0)
            assert int(want.abs().max()) < 2 ** 24
            assert got.shape == (n,) and torch.equal(got.cpu().to(torch.int64), want), (M, n, ld)
            assert torch.equal(got.cpu(), want.float())


def colsum_multi_jobs():
    """The job mix of tests/test_kernels_emul.py::test_colsum_multi: single- and multi-slab jobs, strided sources, several
    destination segments per job, an M = 0 job, the float4 path (n >= 1024, segment starts at multiples of 4), and more
    than 36 jobs / 72 segments, so several launches are needed.  -> (shapes [(M, n, ld)], segment starts per job)."""
    rs = np.random.RandomState(3)
    shapes = [(1, 5, 5), (17, 3, 3), (700, 33, 40), (5000, 300, 300), (40000, 7, 9), (0, 4, 4)] + \
             [(int(rs.randint(1, 3000)), int(rs.randint(1, 70)), 80) for _ in range(90)]
    vec_cuts = {(49, 4096, 4096): [0, 1024, 3072], (64, 2048, 2048): [0], (300, 1024, 1028): [0, 512], (16, 1536, 1536): [0, 4]}
    shapes += list(vec_cuts)
    cuts = []
    for M, n, ld in shapes:
        c = sorted(set([0] + ([int(v) for v in rs.randint(1, n, size=rs.randint(0, 3))] if n > 1 else [])))
        cuts.append(vec_cuts.get((M, n, ld), c))
    return shapes, cuts


def test_colsum_multi_is_exact_and_replays():
    """singa_colsum_multi ADDS the column sums into pre-filled destinations; the job table rides in the kernel arguments, so
    a captured call replays with the host tables gone (the property the engine's gradient sink relies on)."""
    ops, lib = _ops(), _lib()
    shapes, cuts = colsum_multi_jobs()
    assert len(shapes) > 36 and sum(len(c) for c in cuts) > 72 and any(M == 0 for M, _, _ in shapes)
    assert any(lib.singa_colsum_multi_work(M, n) > 0 for M, n, _ in shapes)               # multi-slab jobs
    assert any(lib.singa_colsum_multi_work(M, n) == 0 and M > 0 for M, n, _ in shapes)    # single-slab jobs
    gen = torch.Generator().manual_seed(9)
    xs, dsts, init, sums = [], [], [], []
    for (M, n, ld), c in zip(shapes, cuts):
        x = int_valued((M, ld), gen)
        xs.append(x.to(DEV))
        tot = x[:, :n].to(torch.int64).sum(0)
        ends = c[1:] + [n]
        init.append([torch.randint(-8, 9, (b - a,), generator=gen) for a, b in zip(c, ends)])
        sums.append([tot[a:b] for a, b in zip(c, ends)])
        dsts.append([i.float().to(DEV) for i in init[-1]])
    ops._dev(xs[0])
    nj, ns = len(shapes), sum(len(c) for c in cuts)
    X, LD, MM, NN = (ctypes.c_void_p * nj)(), (ctypes.c_longlong * nj)(), (ctypes.c_longlong * nj)(), (ctypes.c_int * nj)()
    S0, C0, D = (ctypes.c_int * nj)(), (ctypes.c_int * ns)(), (ctypes.c_void_p * ns)()
    q = work = 0
    for k, ((M, n, ld), x) in enumerate(zip(shapes, xs)):
        X[k], LD[k], MM[k], NN[k], S0[k] = x.data_ptr(), ld, M, n, q
        work += lib.singa_colsum_multi_work(M, n)
        for c0, d in zip(cuts[k], dsts[k]):
            C0[q], D[q] = c0, d.data_ptr()
            q += 1
    w = torch.zeros(work + 4, device=DEV)

    def call():
        code = lib.singa_colsum_multi(nj, X, LD, MM, NN, S0, ns, C0, D, ctypes.c_void_p(w.data_ptr()), work + 4,
                                      ops._stream())
        assert code == 0, lib.singa_last_error_string()

    def check(times):
        torch.cuda.synchronize()
        for k in range(nj):
            for d, i, s in zip(dsts[k], init[k], sums[k]):
                assert torch.equal(d.cpu().to(torch.int64), i + times * s), (shapes[k], times)

    call()
    check(1)                                               # eager: initial + sums
    # capture: a warm-up call on a side stream EXECUTES (destinations = initial + 2 x sums); the capture itself executes
    # nothing; the destinations are then reset to their initial integers, the host tables are wiped, and two replays must
    # leave exactly initial + 2 x sums
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    check(2)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        call()
    check(2)
    for k in range(nj):
        for d, i in zip(dsts[k], init[k]):
            d.copy_(i.float())
    for tbl in (MM, NN, LD, S0, C0):
        ctypes.memset(tbl, 0, ctypes.sizeof(tbl))
    graph.replay()
    graph.replay()
    check(2)


def test_param_colsum_through_the_gradient_sink_is_exact():
    """ops.param_colsum as the backward functions use it: without the sink it returns the column blocks' sums; with the
    sink on, the sums are queued and _GradSink.flush adds them into the parameters' .grad buffers in one multi-job call."""
    ops = _ops()
    gen = torch.Generator().manual_seed(21)
    M, widths = 40000, (32, 224, 4)
    src = int_valued((M, sum(widths)), gen)
    tot = src.to(torch.int64).sum(0)
    params = [torch.zeros(wd, device=DEV, requires_grad=True) for wd in widths]
    offs = [0, widths[0], widths[0] + widths[1]]
    targets = [(o, wd, p) for o, wd, p in zip(offs, widths, params)]
    got = ops.param_colsum(src.to(DEV), targets)
    for o, wd, gt in zip(offs, widths, got):
        assert torch.equal(gt.cpu().to(torch.int64), tot[o:o + wd])
    start = [torch.randint(-8, 9, (wd,), generator=gen) for wd in widths]
    for p, s in zip(params, start):
        p.grad = s.float().to(DEV)
    ops._GradSink.on = True
    try:
        assert ops.param_colsum(src.to(DEV), targets) == [None, None, None]
        ops._GradSink.flush()
    finally:
        ops._GradSink.on = False
        ops._GradSink.jobs = []
    for o, wd, p, s in zip(offs, widths, params, start):
        assert torch.equal(p.grad.cpu().to(torch.int64), s + tot[o:o + wd])
