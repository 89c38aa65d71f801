"""-m gpu: activation recomputation in the embedding (`SINGA(config, device, recompute=True)`).

The flag trades time for memory and must change nothing else.  Both recomputing nodes run the very launches of the nodes they
stand for - ops.edge_head_conv_recompute those of edge_head -> so2_conv3m, ops.ffn_recompute those of so3_linear -> ffn_tail -
on the same inputs in the same order, so they are compared with torch.equal, under the default matrix-core k11s variant and
under the lane-broadcast one (singa_so3_skinny_variant(1)); the feed-forward node also against the float64 oracle with the
default chain's own error as the yardstick.  Whole steps: bit-equality (eager loss and gradients under both variants, parameters
after three bucketed replayed steps), and the oracle parity of tests/test_workloads_gpu.py under the default variant.  Memory:
what the forward pass holds with the flag off minus on is the sum of the tensors that are no longer saved, computed from the
batch's shapes.

(A fused kernel that forms the hidden tensor in registers and never writes it was built for the feed-forward node and measured:
two launches of it cost 4.44 ms against 3.88 ms for two expand + activation pairs at config 3, 12.43 ms against 9.65 ms at the
config-5 share (profiles/recompute/README.md), so the node repeats the existing launches instead.)"""
import contextlib
import functools

import pytest
import torch

from oracle import singa_oracle as O
from singa_amd import so3
from tests.helpers import cpu_f64, named_grads, oracle_relu_ties, pinned_relu_ties, rel_err
from tests.test_launch_regimes_gpu import sep_s2_act64

pytestmark = pytest.mark.gpu
DEV = "cuda"
C = 512


def _ops():
    from singa_amd import ops
    return ops


def _lib():
    from singa_amd import _lib as L
    return L.lib()


@contextlib.contextmanager
def skinny_variant(valu):
    """The lane-broadcast (1) or the matrix-core (0, default) k11s kernels; the switch is restored on the way out."""
    _lib().singa_so3_skinny_variant(valu)
    try:
        yield
    finally:
        _lib().singa_so3_skinny_variant(0)


# ====================================================================================================== the attention node
def attention_case(L, E, seed=3):
    heads, A, Ch, V = 7, 32, 128, 16
    lay = so3.layout(L, 2)
    g = torch.Generator().manual_seed(100 * L + E + seed)
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    h0 = rn(E, heads * A + Ch + lay.seg_rows[0] * Ch)
    h1, h2 = rn(E, lay.seg_rows[1] * Ch), rn(E, lay.seg_rows[2] * Ch)
    ln_w, ln_b, dot = 1 + rn(A, scale=0.2), rn(A, scale=0.2), rn(heads, A, scale=0.2)
    out = heads * V
    n0, n1, n2 = (r * Ch for r in lay.seg_rows)
    w0, b0 = rn((L + 1) * out, n0, scale=n0 ** -0.5), rn((L + 1) * out)
    w1 = rn(2 * out * L, n1 // 2, scale=(n1 // 2) ** -0.5)
    w2 = rn(2 * out * (L - 1), n2 // 2, scale=(n2 // 2) ** -0.5)
    gl = rn(E, heads)
    gys = [rn(E, w.shape[0]) for w in (w0, w1, w2)]
    return (heads, A, Ch, lay), [h0, h1, h2, ln_w, ln_b, dot, w0, b0, w1, w2], gl, gys


@pytest.mark.parametrize("E", [0, 1, 300])
@pytest.mark.parametrize("L", [2, 4, 6])
def test_attention_node_equals_the_chain(L, E):
    """edge_head -> so2_conv3m against the recomputing node: outputs and all ten gradients, bit for bit."""
    ops = _ops()
    (heads, A, Ch, lay), tensors, gl, gys = attention_case(L, E)
    n0, n1 = lay.seg_rows[0] * Ch, lay.seg_rows[1] * Ch
    names = ["h0", "h1", "h2", "ln_w", "ln_b", "alpha_dot", "w0", "b0", "w1", "w2"]

    def run(recompute):
        t = [v.to(DEV).requires_grad_(True) for v in tensors]
        if recompute:
            outs = ops.edge_head_conv_recompute(*t, heads, A, Ch, L)
        else:
            logits, act = ops.edge_head(*t[:6], heads, A, Ch, L)
            outs = (logits,) + tuple(ops.so2_conv3m(act, t[6], t[7], t[8], t[9], n0, n1))
        loss = sum((o * g.to(DEV)).sum() for o, g in zip(outs, [gl] + gys))
        loss.backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs], [v.grad for v in t]

    want_o, want_g = run(False)
    got_o, got_g = run(True)
    for n, a, b in zip(["logits", "y0", "y1", "y2"], got_o, want_o):
        assert a.shape == b.shape and torch.equal(a, b), (n, L, E)
    for n, a, b in zip(names, got_g, want_g):
        assert a is not None and b is not None and a.shape == b.shape and torch.equal(a, b), (n, L, E)


# ==================================================================================================== the feed-forward node
def ffn_case(L, N):
    g = torch.Generator().manual_seed(77 * L + N)
    K = (L + 1) ** 2
    rn = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale)
    return [rn(N, K, 16), rn(N, C), rn(L + 1, C, 16, scale=0.25), rn(C), rn(L + 1, 16, C, scale=C ** -0.5), rn(16, scale=0.1),
            rn(N, K, 16)], rn(N, K, 16)


FFN_NAMES = ["x", "gate", "W1", "b1", "W2", "b2", "residual"]
# the bounds the existing tests put on these tensors: test_so3_linear_matches_oracle (d input 5e-6, d weight 1e-5, d bias 1e-5) for
# the first linear's, test_ffn_tail_matches_oracle for the output (2e-5) and the rest
FFN_BOUNDS = {"out": 2e-5, "x": 5e-6, "gate": 2e-5, "W1": 1e-5, "b1": 1e-5, "W2": 2e-5, "b2": 1e-5, "residual": 1e-6}


def ffn_run(recompute, tensors, gy, L):
    ops = _ops()
    x, gate, w1, b1, w2, b2, res = t = [v.to(DEV).requires_grad_(True) for v in tensors]
    if recompute:
        out = ops.ffn_recompute(x, gate, w1, b1, w2, b2, L, res)
    else:
        out = ops.ffn_tail(ops.so3_linear(x, w1, b1, L), gate, w2, b2, L, res)
    out.backward(gy.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), [v.grad for v in t]


@pytest.mark.parametrize("valu", [1, 0])
@pytest.mark.parametrize("N", [0, 37])
@pytest.mark.parametrize("L", [2, 4, 6])
def test_ffn_node_equals_the_chain(L, N, valu):
    """so3_linear -> ffn_tail against the recomputing node, under the lane-broadcast and under the default variant: output and
    all seven gradients, bit for bit."""
    tensors, gy = ffn_case(L, N)
    with skinny_variant(valu):
        want_o, want_g = ffn_run(False, tensors, gy, L)
        got_o, got_g = ffn_run(True, tensors, gy, L)
    assert got_o.shape == want_o.shape and torch.equal(got_o, want_o)
    for n, a, b in zip(FFN_NAMES, got_g, want_g):
        assert a is not None and b is not None and a.shape == b.shape and torch.equal(a, b), (n, L, N)


@pytest.mark.parametrize("N", [0, 37])
@pytest.mark.parametrize("L", [2, 4, 6])
def test_ffn_node_matches_oracle_default_variant(L, N):
    """Default (matrix-core) variant: the recomputing node against the float64 oracle.  Its relative error on each tensor may be
    at most the larger of the bound the existing tests put on that tensor and twice the default chain's own error, measured
    here on the same inputs.  (With the node on the chain's own launches the two errors are equal.)"""
    tensors, gy = ffn_case(L, N)

    def oracle(x, gate, w1, b1, w2, b2, res):
        h = O.so3_linear({"a.weight": w1, "a.bias": b1}, "a", x, L)
        return O.so3_linear({"b.weight": w2, "b.bias": b2}, "b", sep_s2_act64(gate, h, L, L), L) + res
    want_o, want_g = cpu_f64(oracle, tensors, gy)
    base_o, base_g = ffn_run(False, tensors, gy, L)
    got_o, got_g = ffn_run(True, tensors, gy, L)
    bad = []
    for n, got, base, want in zip(["out"] + FFN_NAMES, [got_o] + got_g, [base_o] + base_g, [want_o] + want_g):
        assert got.shape == want.shape, n
        e_got, e_base = rel_err(got.cpu(), want), rel_err(base.cpu(), want)
        bound = max(FFN_BOUNDS[n], 2 * e_base)
        print(f"ffn node L={L} N={N} {n}: recompute {e_got:.2e}, default chain {e_base:.2e}, bound {bound:.2e}")
        if not e_got <= bound:
            bad.append((n, e_got, e_base, bound))
    assert not bad, bad


# ============================================================================================================ whole steps
def example_graphs(n=3, seed=11):
    """The bundled example graphs with their edge-frame draws pinned (`rot_rand`), so that no run draws frames of its own."""
    from singa_amd import graph as G
    gen = torch.Generator().manual_seed(seed)
    gs = []
    for i in range(n):
        g = G.example_graph(i)
        g.extras["rot_rand"] = {k: torch.rand(g[et]["edge_index"].shape[1], 3, generator=gen)
                                for k, et in (("pp", G.E_PP), ("ll", G.E_LL), ("lp", G.E_LP))}
        gs.append(g)
    return gs


def make_model(L, recompute, seed=7):
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    torch.manual_seed(seed)
    return SINGA(load_config(lmax=L), device=DEV, recompute=recompute).eval()          # eval: dropout off


def eager_step(model, batch):
    model.zero_grad(set_to_none=True)
    logits = model(batch)
    loss = torch.nn.functional.cross_entropy(logits, batch["ligand_data"]["smiIndices_tgt"].reshape(-1))
    loss.backward()
    return logits.detach(), loss.detach(), named_grads(model)


@pytest.mark.parametrize("L", [2, 6])
def test_step_bits_lane_broadcast(L):
    """Recompute on against off, same seed and state: an eager step gives the same loss and the same gradient of every parameter
    (under the default and under the lane-broadcast variant), three bucketed replayed TrainStep steps the same parameters
    (lane-broadcast variant) - torch.equal.  The state_dict keys (and the initial values) are those of the default model."""
    from singa_amd import graph as G
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = G.collate(example_graphs()).to(DEV)
    off, on = make_model(L, False), make_model(L, True)
    sd_off, sd_on = off.state_dict(), on.state_dict()
    assert list(sd_off) == list(sd_on)
    assert all(torch.equal(sd_off[k], sd_on[k]) for k in sd_off)
    assert on.embedding.recompute and not off.embedding.recompute
    init = {n: p.detach().clone() for n, p in off.named_parameters()}
    _, loss_off, g_off = eager_step(off, batch)
    _, loss_on, g_on = eager_step(on, batch)
    assert torch.equal(loss_on, loss_off), (float(loss_on), float(loss_off))
    differ = [n for n in g_off if not torch.equal(g_on[n], g_off[n])]
    assert set(g_on) == set(g_off) and not differ, (len(differ), differ[:6])
    with skinny_variant(1):
        _, loss_off, g_off = eager_step(off, batch)
        _, loss_on, g_on = eager_step(on, batch)
        assert torch.equal(loss_on, loss_off), (float(loss_on), float(loss_off))
        assert set(g_on) == set(g_off) and len(g_off) == 634
        differ = [n for n in g_off if not torch.equal(g_on[n], g_off[n])]
        assert not differ, (len(differ), differ[:6])
        finals = []
        for model in (off, on):
            model.zero_grad(set_to_none=True)
            eng = TrainStep(model, Adam(model.parameters(), lr=1e-4), None, use_graph=True, bucket=True)
            try:
                for _ in range(3):
                    eng.step(batch)
                torch.cuda.synchronize()
                finals.append({n: p.detach().clone() for n, p in model.named_parameters()})
            finally:
                eng.release()
        moved = sum(not torch.equal(finals[0][n], init[n]) for n in finals[0])
        assert moved > 600, moved                                        # the steps did update the parameters
        differ = [n for n in finals[0] if not torch.equal(finals[0][n], finals[1][n])]
        assert not differ, (len(differ), differ[:6])


@functools.lru_cache(maxsize=None)
def oracle_step(L):
    """The CPU oracle's step on the example graphs from the state of make_model(L, .): (state with gradients, loss, logits, ties)."""
    graphs = example_graphs()
    model = make_model(L, False)
    sd = {k: v.detach().cpu().clone().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    del model
    b, rots, lap_p, lap_l = O.batch_from_graphs(graphs)
    with oracle_relu_ties() as ties:
        loss_o = O.train_step_loss(sd, b, rots, L, lap_p, lap_l)
    loss_o.backward()
    with torch.no_grad():
        n = len(graphs)
        bp = torch.repeat_interleave(torch.arange(n), b["ptr_p"][1:] - b["ptr_p"][:-1])
        bl = torch.repeat_interleave(torch.arange(n), b["ptr_l"][1:] - b["ptr_l"][:-1])
        ref = O.singa_forward(sd, b, rots, L, O.knn_graph(b["pos_p"], 48, bp), O.knn_graph(b["pos_l"], 30, bl), lap_p, lap_l)
    return sd, loss_o.detach(), ref, ties.records


@pytest.mark.parametrize("L", [2, 6])
def test_recompute_step_matches_oracle(L):
    """Default variant: the recompute step against the CPU oracle with the criteria and tolerances of
    tests/test_workloads_gpu.py::test_workload_step_matches_oracle (logits, loss, every parameter's gradient and the total
    gradient norm at 1e-4, ReLU gates at fp32 ties pinned to the oracle's choice)."""
    from singa_amd import graph as G
    sd, loss_o, ref, records = oracle_step(L)
    model = make_model(L, True)
    batch = G.collate(example_graphs()).to(DEV)
    with pinned_relu_ties(records=records) as pins:
        logits, loss, _ = eager_step(model, batch)
    assert pins.call == 18 and pins.flipped <= 16, (pins.call, pins.flipped)
    assert abs(float(loss) - float(loss_o)) < 1e-4 * abs(float(loss_o)), (float(loss), float(loss_o))
    assert rel_err(logits.cpu(), ref) < 1e-4
    total = float(torch.sqrt(sum((v.grad.double() ** 2).sum() for v in sd.values() if v.grad is not None)))
    bad, errs, n_checked = [], [], 0
    for name, p in model.named_parameters():
        go = sd[name].grad
        if go is None or float(go.norm()) == 0.0:
            assert p.grad is None or float(p.grad.norm()) == 0.0, name
            continue
        assert p.grad is not None, name
        n_checked += 1
        err = float((p.grad.detach().cpu().double() - go.double()).norm() / go.double().norm())
        if float(go.norm()) > 1e-7 * total:
            errs.append((err, name))
            if err > 1e-4:
                bad.append((name, err, float(go.norm())))
    print(f"recompute step L={L}: {pins.flipped} ReLU gates pinned; largest per-parameter gradient errors: "
          + ", ".join(f"{n} {e:.1e}" for e, n in sorted(errs, reverse=True)[:6]))
    assert n_checked == 634, n_checked
    assert not bad, bad[:8]
    gn = float(torch.sqrt(sum((p.grad.double() ** 2).sum() for p in model.parameters() if p.grad is not None)))
    assert abs(gn - total) < 1e-4 * total, (gn, total)


def test_flag_is_refused_where_the_kernels_do_not_fit():
    from singa_amd.config import load_config
    from singa_amd.model.Embedding import EquivariantEmbedding
    cfg = load_config(lmax=2).embedding
    cfg.ffn_hidden_channels = 256
    with pytest.raises(ValueError, match="ffn_hidden_channels"):
        EquivariantEmbedding(cfg, device=DEV, recompute=True)
    EquivariantEmbedding(cfg, device=DEV)                                 # the default path takes any width


# ================================================================================================================= memory
def saved_bytes(batch, L, layers):
    """What the flag keeps out of the autograd graph, from the batch's own shapes: both [N, K, 512] tensors of every
    feed-forward call and the [E, KR*128] activation of every attention call.  Calls: `layers` over the union of the protein
    and the ligand graph, one over the ligand->protein edges / the protein atoms, one over the protein->ligand edges / the ligand
    atoms (the hetero passes' dead layers only renormalise).  -> (bytes, number of tensors)."""
    from singa_amd import graph as G
    n_p, n_l = batch[G.PA]["x"].shape[0], batch[G.LA]["x"].shape[0]
    e = {et: batch[et]["edge_index"].shape[1] for et in (G.E_PP, G.E_LL, G.E_LP, G.E_PL)}
    K, KR = (L + 1) ** 2, so3.layout(L, 2).KR
    ffn_nodes = [n_p + n_l] * layers + [n_p, n_l]
    att_edges = [e[G.E_PP] + e[G.E_LL]] * layers + [e[G.E_LP], e[G.E_PL]]
    return sum(2 * n * K * 512 * 4 for n in ffn_nodes) + sum(m * KR * 128 * 4 for m in att_edges), 2 * len(ffn_nodes) + len(att_edges)


def test_forward_holds_less_by_the_unsaved_tensors():
    from singa_amd import graph as G
    L = 4
    batch = G.collate(example_graphs(1)).to(DEV)
    held, peak = {}, {}
    for mode in (False, True):
        model = make_model(L, mode)
        eager_step(model, batch)                                         # caches (edge sets, grid tables, streams) exist now
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        logits = model(batch)
        torch.cuda.synchronize()
        held[mode] = torch.cuda.memory_allocated() - before
        del logits
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        eager_step(model, batch)
        torch.cuda.synchronize()
        peak[mode] = torch.cuda.max_memory_allocated()
        del model
    S, n_tensors = saved_bytes(batch, L, 3)
    diff = held[False] - held[True]
    print(f"forward holds {held[False] / 2**20:.1f} MiB off, {held[True] / 2**20:.1f} MiB on: {diff / 2**20:.1f} MiB less; "
          f"S = {S / 2**20:.1f} MiB in {n_tensors} tensors; step peak {peak[False] / 2**20:.1f} -> {peak[True] / 2**20:.1f} MiB")
    assert abs(diff - S) <= n_tensors * 2 * 2 ** 20, (diff, S)
    assert peak[True] < peak[False]
