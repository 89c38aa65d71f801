"""-m gpu: the dense attention core with bf16 operands (k19b, include/singa_hip_attn_bf16.h) through `ops.attention(...,
precision="bf16")` up to `SINGA(..., attention_precision="bf16")`.  The reference is the plain float64 evaluation - matmul,
masked_fill(-1e9), softmax, matmul under autograd; `r` rounds to bf16 (ties to even)."""
import math

import pytest
import torch

from tests import test_embedding_precision_gpu as EP
from tests import test_precision_gpu as PG

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, H = 2, 4
SCALE = 1.0 / math.sqrt(32.0)


def r(x):
    return x.to(torch.bfloat16).float()


def make_mask(kind, T, S):
    """pad: [B, 1, S] expanded over the queries (row stride 0).  causal: pad | causal as [B, T, S], one row masked in every key.
    dead: pad whose keys 32 .. 63 are masked for every query, so that a whole key tile is skipped under a tile map."""
    pad = torch.zeros(B, S, dtype=torch.bool)
    if S > 1:
        pad[0, S - S // 4:], pad[1, S - S // 3:] = True, True
    if kind == "dead":
        pad[:, 32:64] = True
    if kind != "causal":
        return pad.to(DEV)[:, None, :].expand(B, T, S)              # (expanded on the device: a copy would lose the stride 0)
    m = pad[:, None, :] | torch.triu(torch.ones(T, S, dtype=torch.bool), 1)
    m[0, T // 2] = True
    return m.to(DEV)


def laid_out(layout, q, k, v):
    """The canonical [B, H, rows, D] operands in the layout under test, made by differentiable views: head-major, dense
    token-major, or q | k | v as column blocks of one [B, T, 512] buffer."""
    if layout == "head":
        return [t.reshape(B * H, t.shape[2], t.shape[3]) for t in (q, k, v)], False
    tm = [t.permute(0, 2, 1, 3).contiguous() for t in (q, k, v)]
    if layout == "fused":
        buf = torch.cat([t.flatten(2) for t in tm], 2)              # [B, T, 128 | 128 | 256]
        tm = [buf[:, :, a:b].view(B, -1, H, d) for a, b, d in ((0, 128, 32), (128, 256, 32), (256, 512, 64))]
    return tm, True


def run(layout, mask, q, k, v, g, precision, tiles):
    from singa_amd import ops
    q, k, v = [t.to(DEV).requires_grad_() for t in (q, k, v)]
    ops_in, tm = laid_out(layout, q, k, v)
    T, S = q.shape[2], k.shape[2]
    out = ops.attention(*ops_in, mask, SCALE, H, token_major=tm, tiles=ops.attn_tiles(mask, T, S) if tiles else None, precision=precision)
    out = out.permute(0, 2, 1, 3) if tm else out.view(B, H, T, 64)
    out.backward(g.to(DEV))
    return [t.detach().cpu() for t in (out, q.grad, k.grad, v.grad)]


def reference(mask, q, k, v, g):
    q, k, v = [t.double().requires_grad_() for t in (q, k, v)]
    s = (q @ k.transpose(2, 3) * SCALE).masked_fill(mask.cpu()[:, None], -1e9)
    out = torch.softmax(s, -1) @ v
    out.backward(g.double())
    return [out.detach(), q.grad, k.grad, v.grad]


def errors(got, want, scales):
    """ctx: max |error| / max |reference|; dq, dk, dv: |error|_2 / |reference|_2 (a reference that is zero throughout - the
    single key of S = 1 has dS = 0 - is measured against the size its terms have: scale |g| |v| |other operand|)."""
    ctx = float((got[0].double() - want[0]).abs().max() / want[0].abs().max())
    grads = [float((a.double() - b).norm() / (b.norm() if float(b.norm()) > 0 else s)) for a, b, s in zip(got[1:], want[1:], scales)]
    return ctx, max(grads)


# Largest error against the float64 reference over the cases below, measured on an MI355X (profiles/attn_bf16/README.md); the
# bounds are 4 x these (the error depends on the draw), and none may exceed 2^-6 = four bf16 unit roundoffs.
#                                                        ctx          gradients
#   q, k, v, dO representable in bf16 (rounded: p~, P, dS)   1.275e-03    1.906e-03
#   unrounded (rounded: all operands)                        5.885e-03    4.421e-03
MEASURED = {True: (1.275e-03, 1.906e-03), False: (5.885e-03, 4.421e-03)}
CAP = 2.0 ** -6
BOUND = {rep: tuple(min(4 * x, CAP) for x in MEASURED[rep]) for rep in MEASURED}

# the whole product shape x mask x layout: pad | causal on square shapes only, the dead tile at S = 97 only, the fused buffer at
# T = S only - 24 combinations
CASES = [(T, S, kind, layout) for T, S in ((1, 1), (31, 33), (32, 32), (33, 97), (70, 70)) for kind in ("pad", "causal", "dead")
         for layout in ("head", "token", "fused")
         if (kind != "causal" or T == S) and (kind != "dead" or S == 97) and (layout != "fused" or T == S)]


@pytest.mark.parametrize("representable", [True, False])
@pytest.mark.parametrize("T,S,kind,layout", CASES)
def test_forward_and_backward_against_float64(T, S, kind, layout, representable):
    gen = torch.Generator().manual_seed(1000 * T + S + len(kind))
    q, k, v, g = [torch.randn(B, H, n, d, generator=gen) for n, d in ((T, 32), (S, 32), (S, 64), (T, 64))]
    if representable:
        q, k, v, g = r(q), r(k), r(v), r(g)
    mask = make_mask(kind, T, S)
    want = reference(mask, q, k, v, g)
    full, tiled = [run(layout, mask, q, k, v, g, "bf16", t) for t in (False, True)]
    for a, b in zip(full, tiled):
        assert torch.equal(a, b)                                   # a skipped tile contributes exact zeros
    gv = SCALE * float(g.norm()) * float(v.norm())
    scales = (gv * float(k.norm()), gv * float(q.norm()), float(g.norm()))
    ctx, grad = errors(full, want, scales)
    ctx32, grad32 = errors(run(layout, mask, q, k, v, g, "f32", True), want, scales)
    print(f"T={T} S={S} {kind} {layout} representable={representable}: ctx {ctx:.3e} grad {grad:.3e} (f32 path: {ctx32:.3e} {grad32:.3e})")
    assert ctx32 <= 1e-5 and grad32 <= 1e-5
    assert ctx <= BOUND[representable][0] and grad <= BOUND[representable][1]


@pytest.mark.parametrize("S,n", [(33, 16), (64, 32), (97, 64)])
@pytest.mark.parametrize("tiles", [False, True])
def test_rounding_of_v_and_the_context_gradient_is_exact(S, n, tiles):
    """q = 0 and a padding mask that leaves n keys: every unmasked p~ is 1 and P = 1 / n, both representable, so ctx is the mean of
    r(v) over the unmasked keys, dv is (1 / n) sum_t r(g) on them and an exact zero on the others, and dk = dS^T q is exactly zero.
    A kernel that does not round v or dO misses the first two by about 1e-3."""
    T = 33
    gen = torch.Generator().manual_seed(S)
    k, v, g = [torch.randn(B, H, rows, d, generator=gen) for rows, d in ((S, 32), (S, 64), (T, 64))]
    q = torch.zeros(B, H, T, 32)
    mask = (torch.arange(S) >= n).to(DEV)[None, None, :].expand(B, T, S)
    out, _, dk, dv = run("head", mask, q, k, v, g, "bf16", tiles)
    tol = 1e-6 * float(v.abs().max())
    want_ctx = r(v)[:, :, :n].double().mean(2, keepdim=True).expand(B, H, T, 64)
    assert float((out.double() - want_ctx).abs().max()) <= tol
    want_dv = (r(g).double().sum(2, keepdim=True) / n).expand(B, H, n, 64)
    assert float((dv[:, :, :n].double() - want_dv).abs().max()) <= tol
    assert bool((dv[:, :, n:] == 0).all()) and bool((dk == 0).all())


def _counted(monkeypatch):
    from singa_amd import _lib
    n = {}
    for name in ("singa_attn_fwd", "singa_attn_bwd", "singa_attn_tiled_fwd", "singa_attn_tiled_bwd", "singa_attn_bf16_fwd", "singa_attn_bf16_bwd"):
        def counted(*args, _inner=getattr(_lib.lib(), name), _name=name):
            n[_name] = n.get(_name, 0) + 1
            return _inner(*args)
        monkeypatch.setattr(_lib.lib(), name, counted)
    return n


# Relative error of the step with attention_precision="bf16" against the f32 step on the golden 3-graph batch at L = 2, measured on
# an MI355X (profiles/attn_bf16/README.md):   logits 3.179e-04   loss 1.072e-05   total gradient norm 3.686e-05
# The bound is 4 x these, as CLOSE of tests/test_precision_gpu.py.
STEP_CLOSE = {"logits": 4 * 3.179e-04, "loss": 4 * 1.072e-05, "grad_norm": 4 * 3.686e-05}


def test_switch_reaches_every_dense_attention_and_the_step_stays_close(monkeypatch):
    batch = PG._batch(2)
    n = _counted(monkeypatch)
    steps, calls = {}, {}
    for key, kw in (("f32", {}), ("attn", {"attention_precision": "bf16"})):
        n.clear()
        steps[key] = PG._step(EP._model(2, **kw), batch)
        calls[key] = dict(n)
    fwd = sum(c for name, c in calls["f32"].items() if name.endswith("fwd"))
    bwd = sum(c for name, c in calls["f32"].items() if name.endswith("bwd"))
    assert fwd >= 1 and bwd == fwd and not any("bf16" in name for name in calls["f32"])
    assert calls["attn"] == {"singa_attn_bf16_fwd": fwd, "singa_attn_bf16_bwd": bwd}
    (lo_f, loss_f, gn_f), (lo_b, loss_b, gn_b) = steps["f32"], steps["attn"]
    err = {"logits": float((lo_b.double() - lo_f.double()).norm() / lo_f.double().norm()),
           "loss": abs(loss_b - loss_f) / abs(loss_f), "grad_norm": abs(gn_b - gn_f) / gn_f}
    print("attention_precision bf16 against f32, L=2: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert 0 < v <= STEP_CLOSE[k], (k, v, STEP_CLOSE[k])
