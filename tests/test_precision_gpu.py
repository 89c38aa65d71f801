"""-m gpu: `precision="bf16"` from the autograd functions up to train.py (ops._gemm -> singa_gemm_bf16; the kernel itself is
tests/test_gemm_bf16_gpu.py's).  Backward follows the flag; the flag reaches the CProMG transformer and nothing else; the step
stays close to the f32 step, replays as it runs eagerly, and trains."""
import functools
import glob
import os
import subprocess
import sys

import pytest
import torch

from tests.helpers import NAMES, golden, product_batch, state_from_spec
from tests.test_gemm_gpu import _f64, _tol, check

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NN, NO, TN = (True, True), (True, False), (False, False)      # operand forms of the forward, dX and dW launches


def _r(t):
    return t.detach().cpu().bfloat16().double()


def _leaf(t):
    return t.to(DEV).requires_grad_(True)


def _linear_case(M, K, N, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g)], torch.randn(M, N, generator=g)


@pytest.mark.parametrize("M", [1, 37, 300])
def test_linear_forward_and_backward_follow_the_flag(M):
    """y, dx, dW against float64 on bf16-rounded operands (x, W and the incoming gradient g) within the f32 GEMM tests' tolerance;
    db bit-equal to the f32 path's."""
    from singa_amd import ops
    K, N = 68, 132
    (x, w, b), gy = _linear_case(M, K, N, M)
    grads = {}
    for precision in ("f32", "bf16"):
        t = [_leaf(v) for v in (x, w, b)]
        y = ops.linear(*t, precision=precision)
        y.backward(gy.to(DEV))
        grads[precision] = (y.detach(), *[v.grad for v in t])
    y, dx, dw, db = grads["bf16"]
    check(y, _r(x) @ _r(w).t() + _f64(b), *_tol("float", NN, K))
    check(dx, _r(gy) @ _r(w), *_tol("float", NO, N))
    check(dw, _r(gy).t() @ _r(x), *_tol("float", TN, M))
    assert torch.equal(db, grads["f32"][3])
    assert not torch.equal(y, grads["f32"][0]) and not torch.equal(dx, grads["f32"][1]) and not torch.equal(dw, grads["f32"][2])


@pytest.mark.parametrize("M", [1, 37, 300])
def test_pos_ffn_forward_and_backward_follow_the_flag(M):
    """relu(x W1^T + b1) W2^T + b2.  Rounding to bf16 is not continuous, so each product is referred to the operands the GPU
    itself rounded: the hidden tensor h and its gradient dh are taken from bf16 launches of the same two products on their own
    (same kernel, same tile plan: the same bits as inside pos_ffn)."""
    from singa_amd import ops
    K, H, N = 68, 132, 36
    g = torch.Generator().manual_seed(100 + M)
    x, w1, b1 = torch.randn(M, K, generator=g), torch.randn(H, K, generator=g) / K ** 0.5, torch.randn(H, generator=g)
    w2, b2, gy = torch.randn(N, H, generator=g) / H ** 0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    out = {}
    for precision in ("f32", "bf16"):
        t = [_leaf(v) for v in (x, w1, b1, w2, b2)]
        y = ops.pos_ffn(*t, precision=precision)
        y.backward(gy.to(DEV))
        out[precision] = (y.detach(), *[v.grad for v in t])
    y, dx, dw1, db1, dw2, db2 = out["bf16"]
    h = torch.relu(ops.linear(x.to(DEV), w1.to(DEV), b1.to(DEV), precision="bf16")).detach().requires_grad_(True)
    ops.linear(h, w2.to(DEV), None, precision="bf16").backward(gy.to(DEV))
    dh = h.grad * (h.detach() > 0)
    check(y, _r(h) @ _r(w2).t() + _f64(b2), *_tol("float", NN, H))
    check(dw2, _r(gy).t() @ _r(h), *_tol("float", TN, M))
    check(dx, _r(dh) @ _r(w1), *_tol("float", NO, H))
    check(dw1, _r(dh).t() @ _r(x), *_tol("float", TN, M))
    assert torch.equal(db2, out["f32"][5])                                # column sums of g: the unrounded f32 registers
    ref1 = _f64(dh).sum(0)
    assert float((_f64(db1) - ref1).abs().max()) <= 2e-6 * M ** 0.5 + 1e-6 * float(ref1.abs().max())
    assert not torch.equal(y, out["f32"][0]) and not torch.equal(dx, out["f32"][1]) and not torch.equal(dw1, out["f32"][2])


@pytest.mark.parametrize("M", [1, 37, 300])
def test_grouped_linear3_forward_and_backward_follow_the_flag(M):
    """The three grouped projections: outputs and weight gradients per (layer, head) block; the input gradient is the three
    layers' contributions chained through the epilogue's addend - the sum of the three products' allowances plus two f32
    additions (2^-23 of the largest value each)."""
    from singa_amd import ops
    heads, ig, ogs = 4, 64, (32, 32, 64)
    g = torch.Generator().manual_seed(200 + M)
    h = torch.randn(M, heads * ig, generator=g)
    ws = [torch.randn(heads * og, ig, 1, generator=g) / ig ** 0.5 for og in ogs]
    gys = [torch.randn(M, heads, og, generator=g) for og in ogs]
    out = {}
    for precision in ("f32", "bf16"):
        hd, wd = _leaf(h), [_leaf(w) for w in ws]
        ys = ops.grouped_linear3(hd, *wd, heads, precision=precision)
        torch.autograd.backward(ys, [gy.to(DEV) for gy in gys])
        out[precision] = ([y.detach() for y in ys], hd.grad, [w.grad for w in wd])
    ys, dh, dws = out["bf16"]
    hb = _r(h).view(M, heads, ig)
    dh_ref, allow = torch.zeros(M, heads, ig, dtype=torch.float64), 0.0
    for y, dw, w, gy, og in zip(ys, dws, ws, gys, ogs):
        wb = _r(w).view(heads, og, ig)
        check(y, torch.einsum("mhi,hoi->mho", hb, wb), *_tol("float", NN, ig))
        check(dw.view(heads, og, ig), torch.einsum("mho,mhi->hoi", _r(gy), hb), *_tol("float", TN, M))
        part = torch.einsum("mho,hoi->mhi", _r(gy), wb)
        tol, slack, extra = _tol("float", NO, og)
        allow += tol * float(part.abs().max()) + slack + extra
        dh_ref += part
    assert float((_f64(dh).view(M, heads, ig) - dh_ref).abs().max()) <= allow + 2 * 2.0 ** -23 * float(dh_ref.abs().max())
    assert not torch.equal(ys[0], out["f32"][0][0]) and not torch.equal(dh, out["f32"][1]) and not torch.equal(dws[2], out["f32"][2][2])


# ====================================================================================================== the whole model
def _model(L, precision):
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    model = SINGA(load_config(lmax=L), device=DEV, precision=precision)
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


class _Count:
    """Wraps ops._gemm: launches by (precision, operand form)."""

    def __init__(self, monkeypatch):
        from singa_amd import ops
        self.n = {}
        inner = ops._gemm

        def counted(items, a_rc, b_rc, splits=1, precision="f32"):
            key = (precision, (bool(a_rc), bool(b_rc)))
            self.n[key] = self.n.get(key, 0) + 1
            return inner(items, a_rc, b_rc, splits, precision)
        monkeypatch.setattr(ops, "_gemm", counted)

    def take(self):
        n, self.n = self.n, {}
        return n


def test_flag_reaches_the_transformer_only(monkeypatch):
    """Same weights, flag off and on: the embedding's outputs are the same bits and it launches no bf16 GEMM, forward or
    backward; the transformer launches bf16 GEMMs in all three forms - forward (1, 1), dX (1, 0), dW (0, 0) - (no shape class is
    routed back to f32 in ops._gemm), the step makes as many launches as the f32 step, and the logits differ from its."""
    from singa_amd.graph import LA, PA
    batch = _batch(2)
    off, on = _model(2, "f32"), _model(2, "bf16")
    count = _Count(monkeypatch)
    embeds = []
    for model in (off, on):
        model.zero_grad(set_to_none=True)
        model.prepare(batch)
        e = model.embedding(batch)
        outs = [t for nt in (PA, LA) for t in vars(e[nt]).values() if torch.is_tensor(t) and t.is_floating_point()]
        sum(t.sum() for t in outs if t.requires_grad).backward()
        torch.cuda.synchronize()
        embeds.append(outs)
        n = count.take()
        assert n and not any(k[0] == "bf16" for k in n), n           # the embedding does launch real GEMMs, all of them f32
    assert len(embeds[0]) == len(embeds[1]) >= 2
    assert all(torch.equal(a, b) for a, b in zip(*embeds))
    logits_off, _, _ = _step(off, batch)
    n_off = count.take()
    assert not any(k[0] == "bf16" for k in n_off), n_off
    logits_on, _, _ = _step(on, batch)
    n_on = count.take()
    for form in (NN, NO, TN):
        assert n_on.get(("bf16", form), 0) >= 1, n_on
    assert sum(v for k, v in n_on.items()) == sum(n_off.values())
    assert not torch.equal(logits_on, logits_off)


# Relative error of the bf16 step against the f32 step on the golden 3-graph batch with the weights of oracle/weights.py,
# measured on an MI355X (profiles/bf16/README.md):      logits      loss        total gradient norm
#                                               L = 2   4.762e-03   4.972e-05   2.628e-04
#                                               L = 4   4.610e-03   3.639e-04   9.002e-04
# The bound is 4 x the larger of the two per quantity: the error depends on weights and inputs, and these weights are one draw.
CLOSE = {"logits": 4 * 4.762e-03, "loss": 4 * 3.639e-04, "grad_norm": 4 * 9.002e-04}


@pytest.mark.parametrize("L", [2, 4])
def test_bf16_step_is_close_to_the_f32_step(L):
    """Guards the plumbing (a layout slip is an O(1) error and tests/test_gemm_bf16_gpu.py's business), not the arithmetic."""
    batch = _batch(L)
    lo_f, loss_f, gn_f = _step(_model(L, "f32"), batch)
    lo_b, loss_b, gn_b = _step(_model(L, "bf16"), batch)
    err = {"logits": float((lo_b.double() - lo_f.double()).norm() / lo_f.double().norm()),
           "loss": abs(loss_b - loss_f) / abs(loss_f), "grad_norm": abs(gn_b - gn_f) / gn_f}
    print(f"bf16 against f32, L={L}: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert 0 < v <= CLOSE[k], (k, v, CLOSE[k])


def test_replayed_bf16_steps_equal_eager_ones():
    """TrainStep in graph mode with precision="bf16": three replayed steps give the losses and the parameters of three eager
    steps of the same model, bit for bit (the captured step simply holds the other kernel).

    As in tests/test_update_parity_gpu.py, the eager engine first runs ONE gradient-only pass (no optimizer): an engine's
    first pass only finds out which parameters get their gradients accumulated in place (ops._GradSink) and hands every
    gradient to autograd, which adds them up in another order.  The capture's warm-up is that pass for the replayed engine; an
    eager engine without it takes its first public step the other way, and its parameters differ in their last bits from then
    on (in f32 too; bf16's rounding of the next forward's operands carries them into the loss)."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = _batch(2)
    runs = []
    for use_graph in (False, True):
        model = _model(2, "bf16")
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


def test_replayed_bf16_steps_repeat():
    """Two replayed bf16 runs from the same state: the same losses and parameters, bit for bit; and step 1's loss is the eager
    step's."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = _batch(2)
    runs = []
    for _ in range(2):
        model = _model(2, "bf16")
        eng = TrainStep(model, Adam(model.parameters(), lr=1e-4, betas=(0.99, 0.999)), None, use_graph=True)
        try:
            losses = [eng.step(batch).detach().clone() for _ in range(3)]
            torch.cuda.synchronize()
            runs.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}))
        finally:
            eng.release()
    (la, pa), (lb, pb) = runs
    assert all(torch.equal(a, b) for a, b in zip(la, lb)) and all(torch.equal(pa[n], pb[n]) for n in pa)
    assert float(la[0]) == _step(_model(2, "bf16"), batch)[1]


def test_bf16_trains():
    """20 Adam steps on the three golden graphs at L = 2 from the same state: every loss finite, and the bf16 run's loss falls by
    at least half of what the f32 run's falls by."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = _batch(2)
    falls = {}
    for precision in ("f32", "bf16"):
        model = _model(2, precision)
        eng = TrainStep(model, Adam(model.parameters(), lr=1e-4, betas=(0.99, 0.999)), None, use_graph=True)
        try:
            losses = [float(eng.step(batch).detach()) for _ in range(20)]
        finally:
            if hasattr(eng, "release"):
                eng.release()
        assert all(l == l and abs(l) != float("inf") for l in losses), losses
        falls[precision] = losses[0] - losses[-1]
        print(precision, "loss", losses[0], "->", losses[-1])
    assert falls["f32"] > 0 and falls["bf16"] >= 0.5 * falls["f32"], falls


def test_train_entry_point_with_bf16(tmp_path):
    """train.py --precision bf16 runs, logs the setting once and writes a checkpoint with the f32 run's keys and dtypes."""
    cks = {}
    for precision in ("f32", "bf16"):
        logdir = str(tmp_path / precision)
        cmd = [sys.executable, os.path.join(ROOT, "train.py"), "--data", "golden", "--lmax", "2", "--batch-size", "3", "--logdir", logdir,
               "--max-iters", "3", "--precision", precision]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600, cwd=ROOT)
        out = r.stdout.decode()
        assert r.returncode == 0, out[-2000:]
        assert sum(f"precision {precision}" in l for l in out.splitlines()) == 1, out[-2000:]
        ck = glob.glob(os.path.join(logdir, "*", "checkpoints", "3.pt"))
        assert ck, "checkpoint of the last iteration missing"
        cks[precision] = torch.load(ck[0], map_location="cpu")

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
