"""-m gpu: `embedding_precision="bf16"` from ops.so2_conv3m up to train.py (ops._gemm -> singa_gemm_bf16 for the m = 0 block,
ops._cgemm -> singa_cgemm_bf16 for the complex blocks; the complex kernel itself is tests/test_cgemm_bf16_gpu.py's).  Backward
follows the switch, the recomputing node runs the same launches, the switch reaches the SO(2) convolutions and nothing else and
is independent of `precision`; the step stays close to the f32 step, replays as it runs eagerly, and trains."""
import functools
import glob
import os
import subprocess
import sys

import pytest
import torch

from tests.helpers import NAMES, golden, product_batch, state_from_spec
from tests.test_gemm_gpu import _f64, _tol, check
from tests.test_recompute_gpu import attention_case

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN, NO, TN = (True, True), (True, False), (False, False)      # operand forms of the forward, dX and dW launches


def _r(t):
    return t.detach().cpu().bfloat16().double()


# ============================================================================================== the convolution's six launches
N0, N1, N2 = 36, 48, 24                  # input widths: m = 0, then [x_+ | x_-] of 24 and of 12 complex inputs
O0, O1, O2 = 40, 40, 24                  # outputs: 40, then [re | im] of 20 and of 12 complex outputs


def _conv_case(E):
    g = torch.Generator().manual_seed(300 + E)
    rn = lambda *s, scale=1.0: torch.randn(*s, generator=g) * scale
    tensors = [rn(E, N0 + N1 + N2), rn(O0, N0, scale=N0 ** -0.5), rn(O0), rn(O1, N1 // 2, scale=(N1 // 2) ** -0.5),
               rn(O2, N2 // 2, scale=(N2 // 2) ** -0.5)]
    return tensors, [rn(E, o) for o in (O0, O1, O2)]


def _conv_run(tensors, gys, precision):
    from singa_amd import ops
    t = [v.to(DEV).requires_grad_(True) for v in tensors]
    ys = ops.so2_conv3m(*t, N0, N1, **({} if precision is None else {"precision": precision}))
    torch.autograd.backward(ys, [g.to(DEV) for g in gys])
    torch.cuda.synchronize()
    return [y.detach() for y in ys], [v.grad for v in t]


@pytest.mark.parametrize("E", [1, 37, 300])
def test_so2_conv3m_forward_and_backward_follow_the_switch(E):
    """Outputs, dX and the three weight gradients against float64 on bf16-rounded X, weights and incoming gradients, within the
    f32 GEMM tests' tolerance of the matching operand form; db0 bit-equal to the f32 path's; everything else not bit-equal; the
    keyword left out is "f32"."""
    tensors, gys = _conv_case(E)
    ys32, g32 = _conv_run(tensors, gys, "f32")
    ys_none, g_none = _conv_run(tensors, gys, None)
    assert all(torch.equal(a, b) for a, b in zip(ys32 + g32, ys_none + g_none))
    ys, (dx, dw0, db0, dw1, dw2) = _conv_run(tensors, gys, "bf16")
    X, w0, b0, w1, w2 = tensors
    x0, x1, x2 = (_r(v) for v in X.split((N0, N1, N2), 1))
    g0, g1, g2 = (_r(v) for v in gys)
    check(ys[0], x0 @ _r(w0).t() + _f64(b0), *_tol("float", NN, N0))
    check(dx[:, :N0], g0 @ _r(w0), *_tol("float", NO, O0))
    check(dw0, g0.t() @ x0, *_tol("float", TN, E))
    col = N0
    for y, x, gy, w, dw in ((ys[1], x1, g1, w1, dw1), (ys[2], x2, g2, w2, dw2)):
        (xr, xi), (gr, gi), (wr, wi) = x.chunk(2, 1), gy.chunk(2, 1), _r(w).chunk(2, 0)
        K, N = xr.shape[1], wr.shape[0]                       # complex inputs and outputs
        check(y, torch.cat([xr @ wr.t() - xi @ wi.t(), xr @ wi.t() + xi @ wr.t()], 1), *_tol("float", NN, K, cplx=True))
        check(dx[:, col:col + 2 * K], torch.cat([gr @ wr + gi @ wi, gi @ wr - gr @ wi], 1), *_tol("float", NO, N, cplx=True))
        check(dw, torch.cat([gr.t() @ xr + gi.t() @ xi, gi.t() @ xr - gr.t() @ xi], 0), *_tol("float", TN, E, cplx=True))
        col += 2 * K
    assert torch.equal(db0, g32[2])                           # column sums of g0: the unrounded f32 registers
    for name, a, b in zip(("y0", "y1", "y2", "dX", "dw0", "dw1", "dw2"), ys + [dx, dw0, dw1, dw2], ys32 + [g32[0], g32[1], g32[3], g32[4]]):
        assert not torch.equal(a, b), name


def test_recomputing_node_equals_the_chain_under_bf16():
    """edge_head -> so2_conv3m against edge_head_conv_recompute, both bf16, L = 2: outputs and all ten gradients bit for bit - and
    the convolution's outputs are not the f32 chain's."""
    from singa_amd import ops
    L, E = 2, 300
    (heads, A, Ch, lay), tensors, gl, gys = attention_case(L, E)
    n0, n1 = lay.seg_rows[0] * Ch, lay.seg_rows[1] * Ch

    def run(recompute, precision):
        t = [v.to(DEV).requires_grad_(True) for v in tensors]
        if recompute:
            outs = ops.edge_head_conv_recompute(*t, heads, A, Ch, L, precision=precision)
        else:
            logits, act = ops.edge_head(*t[:6], heads, A, Ch, L)
            outs = (logits,) + tuple(ops.so2_conv3m(act, t[6], t[7], t[8], t[9], n0, n1, precision=precision))
        sum((o * g.to(DEV)).sum() for o, g in zip(outs, [gl] + gys)).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], [v.grad for v in t]

    want_o, want_g = run(False, "bf16")
    got_o, got_g = run(True, "bf16")
    for a, b in zip(got_o + got_g, want_o + want_g):
        assert a is not None and b is not None and a.shape == b.shape and torch.equal(a, b)
    f32_o, _ = run(True, "f32")
    assert torch.equal(f32_o[0], got_o[0]) and not any(torch.equal(a, b) for a, b in zip(f32_o[1:], got_o[1:]))


# ====================================================================================================== the whole model
def _model(L, precision="f32", embedding_precision="f32", **kw):
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    if embedding_precision != "f32":
        kw["embedding_precision"] = embedding_precision
    model = SINGA(load_config(lmax=L), device=DEV, precision=precision, **kw)
    model.load_state_dict(state_from_spec(f"singa_L{L}"), strict=False)
    return model.eval()                                     # dropout off


@functools.lru_cache(maxsize=None)
def _batch(L):
    return product_batch(NAMES, golden(f"singa_L{L}_B3.npz"))


def _step(model, batch):
    model.zero_grad(set_to_none=True)
    logits = model(batch)
    loss = torch.nn.functional.cross_entropy(logits, batch["ligand_data"]["smiIndices_tgt"].reshape(-1))
    loss.backward()
    torch.cuda.synchronize()
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))
    return logits.detach(), float(loss), gn


@functools.lru_cache(maxsize=None)
def _f32_step(L):
    """The f32 step (both switches at their defaults: the code path of the commit before the switch), computed once."""
    return _step(_model(L), _batch(L))


class _Count:
    """Wraps ops._gemm and ops._cgemm: launches by (kind, precision, operand form)."""

    def __init__(self, monkeypatch):
        from singa_amd import ops
        self.n = {}
        for kind, name in (("real", "_gemm"), ("complex", "_cgemm")):
            monkeypatch.setattr(ops, name, self._counted(kind, getattr(ops, name)))

    def _counted(self, kind, inner):
        def counted(items, a_rc, b_rc, splits=1, precision="f32"):
            key = (kind, precision, (bool(a_rc), bool(b_rc)))
            self.n[key] = self.n.get(key, 0) + 1
            return inner(items, a_rc, b_rc, splits, precision)
        return counted

    def take(self):
        n, self.n = self.n, {}
        return n


def _bf16(n, kind=None):
    return sum(v for k, v in n.items() if k[1] == "bf16" and kind in (None, k[0]))


def test_switch_reaches_the_so2_convolutions_only(monkeypatch):
    """L = 2 on the golden batch, launches counted by (real / complex, precision, form).  Embedding switch alone: the embedding
    launches bf16 complex and bf16 real GEMMs in all three forms and still f32 real ones (SO3 linears, radial functions), no f32
    complex one; the whole step launches no bf16 GEMM beyond the embedding's (the transformer has none) and as many GEMMs as the
    f32 step; the embedding's outputs differ from f32's.  Both switches: the transformer's bf16 count is the count under
    precision="bf16" alone.  Defaults: nothing is bf16."""
    from singa_amd.graph import LA, PA
    batch = _batch(2)
    count = _Count(monkeypatch)

    def embedding_alone(model):
        model.zero_grad(set_to_none=True)
        model.prepare(batch)
        e = model.embedding(batch)
        outs = [t for nt in (PA, LA) for t in vars(e[nt]).values() if torch.is_tensor(t) and t.is_floating_point()]
        sum(t.sum() for t in outs if t.requires_grad).backward()
        torch.cuda.synchronize()
        return outs, count.take()

    def whole_step(model):
        logits, _, _ = _step(model, batch)
        return logits, count.take()

    off, emb, both, trans = _model(2), _model(2, "f32", "bf16"), _model(2, "bf16", "bf16"), _model(2, "bf16")
    outs_off, n_eoff = embedding_alone(off)
    logits_off, n_off = whole_step(off)
    assert n_eoff and n_off and _bf16(n_eoff) == 0 and _bf16(n_off) == 0
    assert sum(v for k, v in n_off.items() if k[0] == "complex") >= 3

    outs_emb, n_eemb = embedding_alone(emb)
    for form in (NN, NO, TN):
        assert n_eemb.get(("complex", "bf16", form), 0) >= 1 and n_eemb.get(("real", "bf16", form), 0) >= 1, n_eemb
        assert n_eemb.get(("real", "f32", form), 0) >= 1, n_eemb
        assert n_eemb.get(("complex", "f32", form), 0) == 0, n_eemb
    assert sum(n_eemb.values()) == sum(n_eoff.values())
    # every complex launch belongs to an SO(2) convolution, and each convolution pass makes one real launch beside it
    assert _bf16(n_eemb, "real") == _bf16(n_eemb, "complex") == sum(v for k, v in n_eoff.items() if k[0] == "complex")
    assert len(outs_off) == len(outs_emb) >= 2 and not any(torch.equal(a, b) for a, b in zip(outs_off, outs_emb))
    logits_emb, n_emb = whole_step(emb)
    assert _bf16(n_emb) == _bf16(n_eemb)                               # the transformer launches no bf16 GEMM
    assert sum(n_emb.values()) == sum(n_off.values())
    assert not torch.equal(logits_emb, logits_off)

    _, n_trans = whole_step(trans)
    assert _bf16(n_trans, "complex") == 0 and _bf16(n_trans, "real") >= 3
    _, n_both = whole_step(both)
    assert _bf16(n_both, "complex") == _bf16(n_emb, "complex")
    assert _bf16(n_both, "real") - _bf16(n_emb, "real") == _bf16(n_trans, "real")
    assert sum(n_both.values()) == sum(n_off.values())


# Relative error against the f32 step on the golden 3-graph batch with the weights of oracle/weights.py, measured on an MI355X
# (profiles/bf16_embed/README.md):
#                                                               logits      loss        total gradient norm
#   embedding_precision="bf16"                          L = 2   3.953e-05   1.682e-06   1.770e-06
#                                                       L = 4   3.971e-05   7.007e-07   8.057e-06
#   precision="bf16", embedding_precision="bf16"        L = 2   4.787e-03   7.400e-05   2.441e-04
#                                                       L = 4   4.633e-03   3.780e-04   9.846e-04
# The bound is 4 x the larger of the two per setting and quantity: the error depends on weights and inputs, and these weights
# are one draw.
CLOSE = {("f32", "bf16"): {"logits": 4 * 3.971e-05, "loss": 4 * 1.682e-06, "grad_norm": 4 * 8.057e-06},
         ("bf16", "bf16"): {"logits": 4 * 4.787e-03, "loss": 4 * 3.780e-04, "grad_norm": 4 * 9.846e-04}}


def closeness(L, setting):
    """Relative errors of the step under `setting` = (precision, embedding_precision) against the f32 step."""
    lo_f, loss_f, gn_f = _f32_step(L)
    lo_b, loss_b, gn_b = _step(_model(L, *setting), _batch(L))
    return {"logits": float((lo_b.double() - lo_f.double()).norm() / lo_f.double().norm()),
            "loss": abs(loss_b - loss_f) / abs(loss_f), "grad_norm": abs(gn_b - gn_f) / gn_f}


@pytest.mark.parametrize("setting", [("f32", "bf16"), ("bf16", "bf16")], ids=["embedding_only", "both"])
@pytest.mark.parametrize("L", [2, 4])
def test_bf16_embedding_step_is_close_to_the_f32_step(L, setting):
    """Guards the plumbing (a layout slip is an O(1) error and tests/test_cgemm_bf16_gpu.py's business), not the arithmetic."""
    err = closeness(L, setting)
    print(f"precision {setting[0]}, embedding precision {setting[1]} against f32, L={L}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert 0 < v <= CLOSE[setting][k], (k, v, CLOSE[setting][k])


def test_replayed_bf16_embedding_steps_equal_eager_ones():
    """TrainStep in graph mode with embedding_precision="bf16": three replayed steps give the losses and the parameters of three
    eager steps of the same model, bit for bit.  The eager engine first makes its gradient-only pass, as in
    tests/test_precision_gpu.py::test_replayed_bf16_steps_equal_eager_ones (see there)."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = _batch(2)
    runs = []
    for use_graph in (False, True):
        model = _model(2, "f32", "bf16")
        eng = TrainStep(model, Adam(model.parameters(), lr=1e-4, betas=(0.99, 0.999)), None, use_graph=use_graph)
        try:
            if not use_graph:
                eng._prepared(batch)
                eng._fwd_bwd(batch)
                eng.opt.zero_grad(set_to_none=True)
                assert eng._sink_params is not None and not getattr(eng.opt, "_built", False)
            losses = [eng.step(batch).detach().clone() for _ in range(3)]
            torch.cuda.synchronize()
            assert float(eng.opt.step_t) == 3.0                  # neither that pass nor the capture's warm-up took a step
            runs.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}))
        finally:
            if hasattr(eng, "release"):
                eng.release()
    (le, pe), (lg, pg) = runs
    print("eager", [float(v) for v in le], "replayed", [float(v) for v in lg])
    assert all(torch.equal(a, b) for a, b in zip(le, lg))
    differ = [n for n in pe if not torch.equal(pe[n], pg[n])]
    assert not differ, (len(differ), differ[:6])
    assert float(le[0]) != _f32_step(2)[1]                      # and they are not the f32 steps


def test_both_switches_train():
    """20 Adam steps on the three golden graphs at L = 2 from the same state: every loss finite, and with both switches on the
    loss falls by at least half of what the f32 run's falls by."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = _batch(2)
    falls = {}
    for setting in (("f32", "f32"), ("bf16", "bf16")):
        model = _model(2, *setting)
        eng = TrainStep(model, Adam(model.parameters(), lr=1e-4, betas=(0.99, 0.999)), None, use_graph=True)
        try:
            losses = [float(eng.step(batch).detach()) for _ in range(20)]
        finally:
            if hasattr(eng, "release"):
                eng.release()
        assert all(l == l and abs(l) != float("inf") for l in losses), losses
        falls[setting] = losses[0] - losses[-1]
        print(setting, "loss", losses[0], "->", losses[-1])
    assert falls["f32", "f32"] > 0 and falls["bf16", "bf16"] >= 0.5 * falls["f32", "f32"], falls


def test_train_entry_point_with_bf16_embedding(tmp_path):
    """train.py --embedding-precision bf16 runs three iterations, logs the setting once and writes a checkpoint with the f32
    run's keys, shapes and dtypes; no tensor in it is bf16."""
    cks = {}
    for ep in ("f32", "bf16"):
        logdir = str(tmp_path / ep)
        cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data", "golden", "--lmax", "2", "--batch-size", "3", "--logdir", logdir,
               "--max-iters", "3", "--embedding-precision", ep]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-2000:]
        assert sum("embedding precision bf16: " in l for l in out.splitlines()) == (1 if ep == "bf16" else 0), out[-2000:]
        assert sum("precision f32" in l for l in out.splitlines()) == 1, out[-2000:]     # the transformer's line, unchanged
        ck = glob.glob(os.path.join(logdir, "*", "checkpoints", "3.pt"))
        assert ck, "checkpoint of the last iteration missing"
        cks[ep] = torch.load(ck[0], map_location="cpu")

    def layout(tree, prefix=""):
        if torch.is_tensor(tree):
            return {prefix: (tree.dtype, tuple(tree.shape))}
        if isinstance(tree, dict):
            return {k2: v2 for k, v in tree.items() for k2, v2 in layout(v, f"{prefix}/{k}").items()}
        if isinstance(tree, (list, tuple)):
            return {k2: v2 for i, v in enumerate(tree) for k2, v2 in layout(v, f"{prefix}/{i}").items()}
        return {prefix: type(tree)}
    a, b = layout(cks["f32"]), layout(cks["bf16"])
    assert a == b and any(v[0] == torch.float32 for v in a.values() if isinstance(v, tuple))
    assert not any(isinstance(v, tuple) and v[0] == torch.bfloat16 for v in b.values())
