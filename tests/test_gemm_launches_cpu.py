"""CPU checks of WHICH launches the GEMM-backed autograd functions of singa_amd/ops.py make, forward and backward, and in which
order: the whole sequence of each function - entry point, operand form, problem count, split count and every field of every
singa_gemm_t record - against a sequence written out by hand, under "f32" and under "bf16" (the same sequence through the other
entry point).  The bound library is replaced by a recorder, `_stream`, `_dev` and `param_colsum` as in tests/test_precision_cpu.py
and tests/test_gemm_probs_cpu.py; the functions read only data_ptr(), shapes and strides before they launch, so CPU tensors do
and nothing real is launched.  A pointer into a tensor the test holds is spelled base + 4 * element offset; one into a buffer
the function allocates itself is an `own(name, offset)`: whatever address the first launch that names it shows, and the SAME
buffer in every later launch (the FFN's hidden activation is the C of its first launch, the A of its second, the mask of its
fourth)."""
import pytest
import torch

from singa_amd import _capi, _lib, ops

F32 = "singa_gemm_f32"
FIELDS = [f for f, _ in _capi.Gemm._fields_]
precisions = pytest.mark.parametrize("precision", ["f32", "bf16"])


class own:
    """`off` floats behind the start of the buffer that the function under test allocates and this expectation calls `name`."""

    def __init__(self, name, off=0):
        self.name, self.off = name, off


def at(t, off=0):
    return t.data_ptr() + 4 * off


class _Recorder:
    """Stands in for the bound library: (entry point, records as dicts, n, a_rc, b_rc, splits) per launch."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(arr, n, a_rc, b_rc, splits, stream):
            assert type(arr)._type_ is _capi.Gemm and len(arr) == n
            self.calls.append((name, [{f: getattr(g, f) for f in FIELDS} for g in arr], n, a_rc, b_rc, splits))
            return 0
        return entry


@pytest.fixture
def calls(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_dev", lambda *t: None)
    monkeypatch.setattr(ops, "param_colsum", lambda src, targets: [torch.zeros(n) for _, n, _ in targets])
    return rec.calls


def check(calls, want, precision):
    """want: [(entry point under "f32", a_rc, b_rc, n, splits, [record])]; a field a record leaves out is the struct's zero."""
    assert [(c[0], c[3], c[4], c[2], c[5]) for c in calls] == \
        [(name.replace("gemm_f32", "gemm_" + precision), a_rc, b_rc, n, splits) for name, a_rc, b_rc, n, splits, _ in want]
    owned = {}
    for k, ((_, got, *_), (*_, recs)) in enumerate(zip(calls, want)):
        assert len(got) == len(recs), f"launch {k}"
        for i, (g, w) in enumerate(zip(got, recs)):
            assert set(w) <= set(FIELDS)
            for f in FIELDS:
                have, exp = g[f] or 0, w.get(f) or 0
                if isinstance(exp, own):
                    assert have, f"launch {k}, record {i}, field {f}: no pointer"
                    have, exp = have - 4 * exp.off, owned.setdefault(exp.name, have - 4 * exp.off)
                assert have == exp, f"launch {k}, record {i}, field {f}: {have} != {exp}"


def rand(*shape, grad=True):
    return torch.randn(*shape, dtype=torch.float32).requires_grad_(grad)


@precisions
def test_linear_own_with_bias_and_addend(calls, precision):
    """y = x W^T + b + addend in one launch; the weight gradient (the bias gradient in its launch) in front of the input gradient."""
    x, w, b, ad, g = rand(3, 10, 24), rand(16, 24), rand(16), rand(3, 10, 16), rand(3, 10, 16, grad=False)
    y = ops._LinearOwn.apply(x, w, b, ad, precision)
    y.backward(g)
    check(calls, [
        (F32, 1, 1, 1, 1, [dict(a=at(x), lda=24, b=at(w), ldb=24, c=at(y), ldc=16, bias=at(b), addend=at(ad), I=30, J=16, R=24)]),
        (F32, 0, 0, 1, 1, [dict(a=at(g), lda=16, b=at(x), ldb=24, c=own("part"), ldc=24, I=16, J=24, R=30, c_split_stride=400,
                                asum=own("part", 384), asum_stride=400)]),
        (F32, 1, 0, 1, 1, [dict(a=at(g), lda=16, b=at(w), ldb=24, c=own("gx"), ldc=24, I=30, J=24, R=16)]),
    ], precision)
    assert y.shape == (3, 10, 16) and x.grad.shape == x.shape and w.grad.shape == w.shape and ad.grad.shape == ad.shape


@precisions
def test_linear_nn(calls, precision):
    """y = x W for W [K, N] as it lies: (1, 0) forward, the input gradient in the (1, 1) form, dW = x^T g."""
    x, w, g = rand(3, 10, 24), rand(24, 16), rand(3, 10, 16, grad=False)
    y = ops._LinearNN.apply(x, w, precision)
    y.backward(g)
    check(calls, [
        (F32, 1, 0, 1, 1, [dict(a=at(x), lda=24, b=at(w), ldb=16, c=at(y), ldc=16, I=30, J=16, R=24)]),
        (F32, 1, 1, 1, 1, [dict(a=at(g), lda=16, b=at(w), ldb=16, c=own("gx"), ldc=24, I=30, J=24, R=16)]),
        (F32, 0, 0, 1, 1, [dict(a=at(x), lda=24, b=at(g), ldb=16, c=own("part"), ldc=16, I=24, J=16, R=30, c_split_stride=384)]),
    ], precision)
    assert y.shape == (3, 10, 16) and x.grad.shape == x.shape and w.grad.shape == w.shape


@precisions
def test_linear_multi_two_layers(calls, precision):
    """Two layers on the same rows into the column blocks of one buffer; the gradients arrive as column blocks of one buffer, as
    the attention writes them: one input-gradient product over all 24 output columns, one split launch for both weights."""
    x, (w0, b0), (w1, b1) = rand(3, 10, 24), (rand(16, 24), rand(16)), (rand(8, 24), rand(8))
    G = rand(3, 10, 24, grad=False)
    y0, y1 = ops._LinearMulti.apply(x, precision, w0, b0, w1, b1)
    torch.autograd.backward([y0, y1], [G[..., :16], G[..., 16:]])
    assert at(y1) == at(y0, 16) and y0.stride() == y1.stride() == (240, 24, 1)
    check(calls, [
        (F32, 1, 1, 2, 1, [dict(a=at(x), lda=24, b=at(w0), ldb=24, c=at(y0), ldc=24, bias=at(b0), I=30, J=16, R=24),
                           dict(a=at(x), lda=24, b=at(w1), ldb=24, c=at(y0, 16), ldc=24, bias=at(b1), I=30, J=8, R=24)]),
        (F32, 1, 0, 1, 1, [dict(a=at(G), lda=24, b=own("wcat"), ldb=24, c=own("gx"), ldc=24, I=30, J=24, R=24)]),
        (F32, 0, 0, 2, 1, [dict(a=at(G), lda=24, b=at(x), ldb=24, c=own("part"), ldc=24, I=16, J=24, R=30, c_split_stride=600,
                                asum=own("part", 576), asum_stride=600),
                           dict(a=at(G, 16), lda=24, b=at(x), ldb=24, c=own("part", 384), ldc=24, I=8, J=24, R=30, c_split_stride=600,
                                asum=own("part", 592), asum_stride=600)]),
    ], precision)
    assert x.grad.shape == x.shape and all(p.grad.shape == p.shape for p in (w0, b0, w1, b1))


@precisions
def test_pos_ffn(calls, precision):
    """Two launches forward, four backward: each weight gradient in front of the input gradient it goes with; the hidden
    activation h is written once and read three times, its gradient dh written once and read twice."""
    x, w1, b1, w2, b2, g = rand(3, 10, 24), rand(32, 24), rand(32), rand(24, 32), rand(24), rand(3, 10, 24, grad=False)
    y = ops.pos_ffn(x, w1, b1, w2, b2, precision)
    y.backward(g)
    check(calls, [
        (F32, 1, 1, 1, 1, [dict(a=at(x), lda=24, b=at(w1), ldb=24, c=own("h"), ldc=32, bias=at(b1), relu=1, I=30, J=32, R=24)]),
        (F32, 1, 1, 1, 1, [dict(a=own("h"), lda=32, b=at(w2), ldb=32, c=at(y), ldc=24, bias=at(b2), I=30, J=24, R=32)]),
        (F32, 0, 0, 1, 1, [dict(a=at(g), lda=24, b=own("h"), ldb=32, c=own("part2"), ldc=32, I=24, J=32, R=30, c_split_stride=792,
                                asum=own("part2", 768), asum_stride=792)]),
        (F32, 1, 0, 1, 1, [dict(a=at(g), lda=24, b=at(w2), ldb=32, c=own("dh"), ldc=32, mask=own("h"), I=30, J=32, R=24)]),
        (F32, 0, 0, 1, 1, [dict(a=own("dh"), lda=32, b=at(x), ldb=24, c=own("part1"), ldc=24, I=32, J=24, R=30, c_split_stride=800,
                                asum=own("part1", 768), asum_stride=800)]),
        (F32, 1, 0, 1, 1, [dict(a=own("dh"), lda=32, b=at(w1), ldb=24, c=own("gx"), ldc=24, I=30, J=24, R=32)]),
    ], precision)
    assert y.shape == (3, 10, 24) and x.grad.shape == x.shape and all(p.grad.shape == p.shape for p in (w1, b1, w2, b2))


@precisions
def test_grouped_linear3(calls, precision):
    """One problem per (layer, head) forward; the input gradient as three launches of four problems, each adding the one before it
    in its epilogue; all twelve weight-gradient blocks from one split launch."""
    N, heads, ig, ogs = 50, 4, 8, (12, 12, 24)
    h = rand(N, heads * ig)
    ws = [rand(heads * og, ig, 1) for og in ogs]
    gs = [rand(N, heads, og, grad=False) for og in ogs]
    outs = ops._GroupedLinear3.apply(h, *ws, heads, precision)
    torch.autograd.backward(outs, gs)
    want = [(F32, 1, 1, 12, 1, [dict(a=at(h, hd * ig), lda=32, b=at(w, hd * og * ig), ldb=8, c=at(o, hd * og), ldc=heads * og,
                                     I=N, J=og, R=ig) for w, o, og in zip(ws, outs, ogs) for hd in range(heads)])]
    for k, (g, w, og) in enumerate(zip(gs, ws, ogs)):
        want.append((F32, 1, 0, 4, 1, [dict(a=at(g, hd * og), lda=heads * og, b=at(w, hd * og * ig), ldb=8, c=own(f"gh{k}", hd * ig),
                                            ldc=32, addend=own(f"gh{k - 1}", hd * ig) if k else None, I=N, J=ig, R=og)
                                       for hd in range(heads)]))
    recs, off = [], 0
    for g, og in zip(gs, ogs):
        for hd in range(heads):
            recs.append(dict(a=at(g, hd * og), lda=heads * og, b=at(h, hd * ig), ldb=32, c=own("part", off), ldc=8, I=og, J=ig, R=N,
                             c_split_stride=1536))
            off += og * ig
    want.append((F32, 0, 0, 12, 1, recs))
    assert off == 1536
    check(calls, want, precision)
    assert [tuple(o.shape) for o in outs] == [(N, heads, og) for og in ogs]
    assert h.grad.shape == h.shape and all(w.grad.shape == w.shape for w in ws)


@precisions
def test_gemm_nt_forward(calls, precision):
    x, w, b = rand(30, 24, grad=False), rand(16, 24, grad=False), rand(16, grad=False)
    y = ops.gemm_nt(x, w, b, precision=precision)
    check(calls, [(F32, 1, 1, 1, 1, [dict(a=at(x), lda=24, b=at(w), ldb=24, c=at(y), ldc=16, bias=at(b), I=30, J=16, R=24)])],
          precision)
    assert y.shape == (30, 16)
    calls.clear()
    X, out = rand(30, 40, grad=False), torch.empty(30, 16)               # a column block of wider rows, the caller's result buffer
    assert ops.gemm_nt(X[:, 8:32], w, out=out, precision=precision) is out
    check(calls, [(F32, 1, 1, 1, 1, [dict(a=at(X, 8), lda=40, b=at(w), ldb=24, c=at(out), ldc=16, I=30, J=16, R=24)])], precision)


def test_so3_linear(calls):
    """SO3_LinearV2 (f32 only) on [N, 9, C] rows, a width pair the MFMA kernel takes: one problem per degree each way, the 2l + 1
    rows of every node a grouped row set; the weight gradient's operands both grouped, one slab per degree."""
    N, L, K, cin, cout = 7, 2, 9, 16, 32
    x, weight, bias, g = rand(N, K, cin), rand(L + 1, cout, cin), rand(cout), rand(N, K, cout, grad=False)
    out = ops._SO3Linear.apply(x, weight, bias, L, None)
    out.backward(g)
    fwd, dx, dw = [], [], []
    for l in range(L + 1):
        n = 2 * l + 1
        fwd.append(dict(a=at(x, l * l * cin), lda=cin, a_group=n, a_group_ld=K * cin, b=at(weight, l * cout * cin), ldb=cin,
                        c=at(out, l * l * cout), ldc=cout, c_group=n, c_group_ld=K * cout, bias=at(bias) if l == 0 else None,
                        I=N * n, J=cout, R=cin))
        dx.append(dict(a=at(g, l * l * cout), lda=cout, a_group=n, a_group_ld=K * cout, b=at(weight, l * cout * cin), ldb=cin,
                       c=own("gx", l * l * cin), ldc=cin, c_group=n, c_group_ld=K * cin, I=N * n, J=cin, R=cout))
        dw.append(dict(a=at(g, l * l * cout), lda=cout, a_group=n, a_group_ld=K * cout, b=at(x, l * l * cin), ldb=cin, b_group=n,
                       b_group_ld=K * cin, c=own("part", l * cout * cin), ldc=cin, I=cout, J=cin, R=N * n, c_split_stride=1536))
    check(calls, [(F32, 1, 1, 3, 1, fwd), (F32, 1, 0, 3, 1, dx), (F32, 0, 0, 3, 1, dw)], "f32")
    assert x.grad.shape == x.shape and weight.grad.shape == weight.shape and bias.grad.shape == bias.shape
