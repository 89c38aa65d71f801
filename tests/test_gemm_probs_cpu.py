"""CPU checks of the GEMM problem builder of singa_amd/ops.py (`_prob`, `_cprob`, `_so3_linear_probs`, `_dw_grads`): the
singa_gemm_t / singa_cgemm_t records it derives from tensor views against records written out by hand - base pointer plus
4 * element offset, pitches and extents typed in, the way the call sites used to spell them - and the descriptions it must
refuse.  The builder reads only data_ptr(), shapes and strides, so CPU tensors do; nothing is launched (`_dw_grads` runs
with the launch and the column sum replaced by recorders)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from singa_amd import _capi, ops  # noqa: E402


def same(got, want, struct=_capi.Gemm):
    """Field by field over the whole struct; a field that is missing, None or 0 is the struct's zero."""
    names = [f[0] for f in struct._fields_]
    assert set(got) <= set(names) and set(want) <= set(names)
    for f in names:
        assert (got.get(f) or 0) == (want.get(f) or 0), f"field {f}: {got.get(f)} != {want.get(f)}"


def same_list(got, want, struct=_capi.Gemm):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        same(g, w, struct)


def rand(*shape):
    return torch.randn(*shape, dtype=torch.float32)


@pytest.fixture
def recorded(monkeypatch):
    """ops._dw_grads without a device: launches and column sums are recorded, not run."""
    rec = dict(launches=[], colsums=[])
    for kind in ("gemm", "cgemm"):
        monkeypatch.setattr(ops, "_" + kind, lambda items, a_rc, b_rc, splits=1, precision="f32", kind=kind:
                            rec["launches"].append((kind, items, a_rc, b_rc, splits, precision)))

    def colsum(src, targets):
        rec["colsums"].append((src, targets))
        return [torch.zeros(n) for _, n, _ in targets]
    monkeypatch.setattr(ops, "param_colsum", colsum)
    return rec


def test_so2_column_blocks():
    """(1, 1): the three blocks of one m-primary edge matrix X [E, n0 + n1 + n2] into the column blocks of H."""
    E, ins, outs = 40, (24, 32, 16), (48, 64, 32)
    X, H, b0 = rand(E, sum(ins)), rand(E, sum(outs)), rand(outs[0])
    ws = [rand(o, k) for o, k in zip(outs, ins)]
    got = [ops._prob(x, w, h, True, True, bias=b) for x, w, h, b in zip(X.split(ins, 1), ws, H.split(outs, 1), (b0, None, None))]
    want, ai, ci = [], 0, 0
    for w, k, o, b in zip(ws, ins, outs, (b0, None, None)):
        want.append(dict(a=X.data_ptr() + 4 * ai, lda=X.stride(0), b=w.data_ptr(), ldb=w.stride(0),
                         c=H.data_ptr() + 4 * ci, ldc=H.stride(0), bias=b.data_ptr() if b is not None else None,
                         I=E, J=o, R=k))
        ai, ci = ai + k, ci + o
    same_list(got, want)
    assert want[1]["a"] == X.data_ptr() + 4 * 24 and want[1]["lda"] == 72 and want[2]["c"] == H.data_ptr() + 4 * 112


@pytest.mark.parametrize("L", [2, 4, 6])
def test_so3_linear_per_degree_lists(L, recorded):
    """SO3_LinearV2 on [N, K, C] rows: forward (1, 1) with bias and addend, input gradient (1, 0), and the weight gradient's
    split (0, 0) form with grouped rows on both operands and one slab per degree."""
    N, K, cin, cout = 7, (L + 1) ** 2, 16, 32
    x, out, addend, g, gx = rand(N, K, cin), rand(N, K, cout), rand(N, K, cout), rand(N, K, cout), rand(N, K, cin)
    weight, bias = rand(L + 1, cout, cin), rand(cout)
    want = []
    for l in range(L + 1):
        n = 2 * l + 1
        want.append(dict(a=x.data_ptr() + 4 * l * l * cin, lda=cin, a_group=n, a_group_ld=K * cin,
                         b=weight.data_ptr() + 4 * l * cout * cin, ldb=cin,
                         c=out.data_ptr() + 4 * l * l * cout, ldc=cout, c_group=n, c_group_ld=K * cout,
                         bias=bias.data_ptr() if l == 0 else None, addend=addend.data_ptr() + 4 * l * l * cout,
                         I=N * n, J=cout, R=cin))
    same_list(ops._so3_linear_probs(x, weight, out, L, True, bias, addend), want)
    want = []
    for l in range(L + 1):
        n = 2 * l + 1
        want.append(dict(a=g.data_ptr() + 4 * l * l * cout, lda=cout, a_group=n, a_group_ld=K * cout,
                         b=weight.data_ptr() + 4 * l * cout * cin, ldb=cin,
                         c=gx.data_ptr() + 4 * l * l * cin, ldc=cin, c_group=n, c_group_ld=K * cin,
                         I=N * n, J=cin, R=cout))
    same_list(ops._so3_linear_probs(g, weight, gx, L, False), want)

    S, sz = 3, cout * cin
    (gw,), gb = ops._dw_grads([(gl, xl, weight, None) for gl, xl in zip(ops._degrees(g, L), ops._degrees(x, L))], S)
    (kind, items, a_rc, b_rc, splits, precision), = recorded["launches"]
    (part, targets), = recorded["colsums"]
    assert (kind, a_rc, b_rc, splits, precision) == ("gemm", False, False, S, "f32") and tuple(part.shape) == (S, (L + 1) * sz)
    want = []
    for l in range(L + 1):
        n = 2 * l + 1
        want.append(dict(a=g.data_ptr() + 4 * l * l * cout, lda=cout, a_group=n, a_group_ld=K * cout,
                         b=x.data_ptr() + 4 * l * l * cin, ldb=cin, b_group=n, b_group_ld=K * cin,
                         c=part.data_ptr() + 4 * l * sz, ldc=cin, I=cout, J=cin, R=N * n, c_split_stride=(L + 1) * sz))
    same_list(items, want)
    assert len(targets) == 1 and targets[0][:2] == (0, (L + 1) * sz) and targets[0][2] is weight
    assert gw.shape == weight.shape and gb == []


def test_grouped_linear3_head_blocks(recorded):
    """One problem per (layer, head): h's column block of the head times the head's [og, ig] weight block into the head's
    column block of the layer's [N, heads, og] output; the weight gradients' slabs fill each layer's parameter head by head."""
    N, heads, ig, og = 50, 4, 8, 12
    h, w, o = rand(N, heads * ig), rand(heads * og, ig), rand(N, heads, og)
    got = [ops._prob(hh, wh, oh, True, True) for hh, wh, oh in zip(h.split(ig, 1), w.split(og, 0), o.unbind(1))]
    want = [dict(a=h.data_ptr() + 4 * g * ig, lda=h.stride(0), b=w.data_ptr() + 4 * g * og * ig, ldb=ig,
                 c=o.data_ptr() + 4 * g * og, ldc=heads * og, I=N, J=og, R=ig) for g in range(heads)]
    same_list(got, want)

    params = [rand(heads * og, ig, 1) for _ in range(3)]               # Conv1d weights
    gs = [rand(N, heads * og) for _ in range(3)]
    S, tot = 2, 3 * heads * og * ig
    gws, _ = ops._dw_grads([(gg, hh, p, None) for g, p in zip(gs, params) for gg, hh in zip(g.split(og, 1), h.split(ig, 1))], S)
    items, (part, targets) = recorded["launches"][0][1], recorded["colsums"][0]
    want, off = [], 0
    for g in gs:
        for hd in range(heads):
            want.append(dict(a=g.data_ptr() + 4 * hd * og, lda=g.stride(0), b=h.data_ptr() + 4 * hd * ig, ldb=h.stride(0),
                             c=part.data_ptr() + 4 * off, ldc=ig, I=og, J=ig, R=N, c_split_stride=tot))
            off += og * ig
    same_list(items, want)
    sz = heads * og * ig
    assert [t[:2] for t in targets] == [(0, sz), (sz, sz), (2 * sz, sz)] and all(t[2] is p for t, p in zip(targets, params))
    assert [tuple(gw.shape) for gw in gws] == [(heads * og, ig, 1)] * 3


def test_complex_problems_in_three_forms(recorded):
    """An m > 0 block of an SO(2) convolution: X block [x_+ | x_-] (column halves), fc weight [Wr; Wi] (row halves), result
    [out_r | out_i]; I, J, R in complex units."""
    E, K, N, ai, ci = 24, 16, 20, 8, 12
    X, H, w = rand(E, ai + 2 * K + 4), rand(E, ci + 2 * N), rand(2 * N, K)
    x, h = X[:, ai:ai + 2 * K], H[:, ci:ci + 2 * N]
    same(ops._cprob(x.chunk(2, 1), w.chunk(2, 0), h.chunk(2, 1), True, True, 1.0),
         dict(a=X.data_ptr() + 4 * ai, lda=X.stride(0), a_im=K, b=w.data_ptr(), ldb=K, b_im=N * K,
              c=H.data_ptr() + 4 * ci, ldc=H.stride(0), c_im=N, I=E, J=N, R=K, sigma=1.0), _capi.CGemm)
    g, gX = rand(E, 2 * N), rand(E, ai + 2 * K + 4)
    same(ops._cprob(g.chunk(2, 1), w.chunk(2, 0), gX[:, ai:ai + 2 * K].chunk(2, 1), True, False, -1.0),
         dict(a=g.data_ptr(), lda=g.stride(0), a_im=N, b=w.data_ptr(), ldb=K, b_im=N * K,
              c=gX.data_ptr() + 4 * ai, ldc=gX.stride(0), c_im=K, I=E, J=K, R=N, sigma=-1.0), _capi.CGemm)
    # (0, 0): two blocks into the slabs of one buffer, the fc weights' own layout
    K2, N2, S = 8, 12, 5
    x2, g2, w2 = X[:, ai + 2 * K - 12:ai + 2 * K + 4], rand(E, 2 * N2), rand(2 * N2, K2)
    (gw, gw2), _ = ops._dw_grads([(g, x, w, None), (g2, x2, w2, None)], S, cplx=True)
    (kind, items, a_rc, b_rc, splits, precision), = recorded["launches"]
    (part, targets), = recorded["colsums"]
    rowc = 2 * N * K + 2 * N2 * K2
    assert (kind, a_rc, b_rc, splits, precision) == ("cgemm", False, False, S, "f32") and tuple(part.shape) == (S, rowc)
    same_list(items, [dict(a=g.data_ptr(), lda=g.stride(0), a_im=N, b=X.data_ptr() + 4 * ai, ldb=X.stride(0), b_im=K,
                           c=part.data_ptr(), ldc=K, c_im=N * K, I=N, J=K, R=E, sigma=-1.0, c_split_stride=rowc),
                      dict(a=g2.data_ptr(), lda=g2.stride(0), a_im=N2, b=X.data_ptr() + 4 * (ai + 2 * K - 12), ldb=X.stride(0),
                           b_im=K2, c=part.data_ptr() + 4 * 2 * N * K, ldc=K2, c_im=N2 * K2, I=N2, J=K2, R=E, sigma=-1.0,
                           c_split_stride=rowc)], _capi.CGemm)
    assert [t[:2] for t in targets] == [(0, 2 * N * K), (2 * N * K, 2 * N2 * K2)]
    assert gw.shape == w.shape and gw2.shape == w2.shape


def test_weight_gradient_with_bias_sums(recorded):
    """(0, 0) with asum: dW = g^T x into [S, N K] slabs, the per-split column sums of g (the bias gradient) behind them."""
    M, N, K = 300, 16, 24
    g, x, w, b = rand(M, N), rand(M, 40)[:, 8:8 + K], rand(N, K), rand(N)
    gw, gb = ops._tn_grad(g, x, w, b)
    (kind, items, a_rc, b_rc, S, precision), = recorded["launches"]
    (part, targets), = recorded["colsums"]
    row = N * K + N
    assert S == ops._tn_splits(M, N, K) and tuple(part.shape) == (S, row) and (a_rc, b_rc, precision) == (False, False, "f32")
    same_list(items, [dict(a=g.data_ptr(), lda=g.stride(0), b=x.data_ptr(), ldb=x.stride(0), c=part.data_ptr(), ldc=K,
                           I=N, J=K, R=M, c_split_stride=row, asum=part.data_ptr() + 4 * N * K, asum_stride=row)])
    assert [t[:2] for t in targets] == [(0, N * K), (N * K, N)] and targets[0][2] is w and targets[1][2] is b
    assert gw.shape == w.shape and gb.shape == b.shape
    # several problems: all slabs first, then the asum rows in the problems' order (the fused Q | K | V projections)
    recorded["launches"].clear(), recorded["colsums"].clear()
    ns, G = (16, 8, 12), rand(M, 36)
    ws, bs = [rand(n, K) for n in ns], [rand(n) for n in ns]
    ops._dw_grads([(gg, x, w, b) for gg, w, b in zip(G.split(ns, 1), ws, bs)], 4)
    items, (part, targets) = recorded["launches"][0][1], recorded["colsums"][0]
    tot, row = sum(ns), sum(ns) * K + sum(ns)
    want, off, poff = [], 0, 0
    for n in ns:
        want.append(dict(a=G.data_ptr() + 4 * off, lda=36, b=x.data_ptr(), ldb=x.stride(0), c=part.data_ptr() + 4 * poff, ldc=K,
                         I=n, J=K, R=M, c_split_stride=row, asum=part.data_ptr() + 4 * (tot * K + off), asum_stride=row))
        off, poff = off + n, poff + n * K
    same_list(items, want)
    assert [t[:2] for t in targets] == [(0, 16 * K), (16 * K, 8 * K), (24 * K, 12 * K), (36 * K, 16), (36 * K + 16, 8), (36 * K + 24, 12)]


def test_no_rows_gives_zeros_without_a_launch(recorded):
    w, b = rand(16, 8), rand(16)
    (gw,), (gb,) = ops._dw_grads([(rand(0, 16), rand(0, 8), w, b)], 1)
    assert not recorded["launches"] and not recorded["colsums"]
    assert gw.shape == w.shape and gb.shape == b.shape and not gw.any() and not gb.any()


def test_builder_refuses_what_the_kernel_cannot_address():
    A, B, C = rand(32, 16), rand(24, 16), rand(32, 24)
    ops._prob(A, B, C, True, True)                                           # y = x W^T: fine
    for a, b, c in ((A, rand(24, 20), C), (A, B, rand(32, 28)), (rand(28, 16), B, C)):      # R, J, I disagree
        with pytest.raises(RuntimeError, match="disagree"):
            ops._prob(a, b, c, True, True)
    with pytest.raises(RuntimeError, match="disagree"):
        ops._prob(A, B, C, True, False)                                      # the same views in the wrong operand form
    with pytest.raises(RuntimeError, match="disagree"):
        ops._prob(rand(5, 3, 16), B, rand(5, 4, 24), True, True)             # grouped rows: 15 rows of A, 20 of C
    with pytest.raises(RuntimeError, match="not contiguous"):
        ops._prob(rand(16, 32).t(), B, C, True, True)                        # inner stride 32
    wide = rand(32, 24)
    with pytest.raises(RuntimeError, match="not 16-byte aligned"):
        ops._prob(wide[:, 1:17], B, C, True, True)                           # base one float off
    with pytest.raises(RuntimeError, match="pitches are not multiples of 4"):
        ops._prob(rand(32, 18)[:, :16], B, C, True, True)                    # row pitch 18 floats
    with pytest.raises(RuntimeError, match="pitches are not multiples of 4"):
        ops._prob(A, B, rand(8, 4, 26)[:, :, :24], True, True)               # grouped result, pitches 104 and 26
    with pytest.raises(RuntimeError, match="addend"):
        ops._prob(A, B, C, True, True, addend=rand(32, 28)[:, :24])          # not laid out like C
    with pytest.raises(RuntimeError, match="slabs"):
        ops._prob(rand(40, 32), rand(40, 24), rand(3, 32, 28)[:, :, :24], False, False)    # partial slabs must be dense
    # complex: extents in complex units, parts a multiple of 4 floats apart
    x, w, h = rand(24, 32), rand(40, 16), rand(24, 40)
    ops._cprob(x.chunk(2, 1), w.chunk(2, 0), h.chunk(2, 1), True, True, 1.0)
    with pytest.raises(RuntimeError, match="disagree"):
        ops._cprob(x.chunk(2, 1), w.chunk(2, 0), rand(24, 48).chunk(2, 1), True, True, 1.0)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops._cprob((x[:, 0:12], x[:, 14:26]), (w[:20, :12], w[20:, :12]), h.chunk(2, 1), True, True, 1.0)
