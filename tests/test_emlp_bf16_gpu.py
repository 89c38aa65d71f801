"""-m gpu: the kNN edge MLPs with bf16 operands (k15e, include/singa_hip_emlp_bf16.h) from the two entry points up to
`SINGA(..., edge_mlp_precision="bf16")`.  The reference is the float64 evaluation of the unit contract; `r` rounds the operands of
its products - not at all for the bounds, to bf16 (`.bfloat16().double()`, ties to even) for the exact-integer cases, where every
product and sum is exact in f32 and the kernels must give the reference's bits."""
import math

import pytest
import torch

from tests import test_embedding_precision_gpu as EP
from tests import test_precision_gpu as PG

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 12345.0
F = torch.nn.functional


def _bf(t):
    return t.bfloat16().double()


def unit_list(E, seed):
    """A shuffled unit list over E rows with a -1 tail: real pairs, rows without a mate (b == a), one unit whose b is no row
    (it must act as "no mate"), and rows that no unit names.  -> unit_a, unit_b [E] int32, (a, effective b) of the units."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randperm(E, generator=g).tolist()
    rows = rows[E // 8:]                                            # the first E / 8 rows: named by no unit
    single, rest = rows[:max(1, E // 4)], rows[max(1, E // 4):]
    units = [(a, a, a) for a in single] + [(a, b, b) for a, b in zip(rest[0::2], rest[1::2])]
    units += [(rest[-1], E + 5, rest[-1])] if len(rest) % 2 else []          # (a, b as listed, b as it acts)
    units = [units[k] for k in torch.randperm(len(units), generator=g).tolist()]
    ua, ub = torch.full((E,), -1, dtype=torch.int32), torch.full((E,), -1, dtype=torch.int32)
    ua[:len(units)], ub[:len(units)] = torch.tensor([u[0] for u in units], dtype=torch.int32), torch.tensor([u[1] for u in units], dtype=torch.int32)
    return ua, ub, torch.tensor([u[0] for u in units]), torch.tensor([u[2] for u in units])


def reference(x, g, w1, b1, w2, b2, r):
    """One net on the units' rows in float64: x [U, 64], g [U, H] = g_out[a] + g_out[b]; r rounds the operands of the products."""
    x, g, w1, b1, w2, b2 = [t.double() for t in (x, g, w1, b1, w2, b2)]
    pre = r(x) @ r(w1).t() + b1
    h = F.softplus(pre) - math.log(2.0)
    gp = (r(g) @ r(w2)) * torch.sigmoid(pre)
    return r(h) @ r(w2).t() + b2, [r(gp).t() @ r(x), gp.sum(0), r(g).t() @ r(h), g.sum(0)]


def run(attr, gs, nets, ua, ub, tag="_bf16"):
    """The three launches through the C ABI -> (wk, wv) over a sentinel, [dW1, db1, dW2, db2] per net from fully written parts."""
    from singa_amd import _lib
    from singa_amd.ops import _p, _stream
    lib, E = _lib.lib(), attr.shape[0]
    attr, ua, ub = attr.to(DEV), ua.to(DEV), ub.to(DEV)
    ws = [t.to(DEV).contiguous() for net in nets for t in net]
    outs = [torch.full((E, H), SENTINEL, device=DEV) for H in (32, 64)]
    fwd, bwd = getattr(lib, f"singa_edge_mlp{tag}_units_fwd"), getattr(lib, f"singa_edge_mlp{tag}_units_bwd")
    assert fwd(_p(attr), _p(ua), _p(ub), *[_p(t) for t in ws], _p(outs[0]), _p(outs[1]), E, 64, 32, 64, _stream()) == 0
    grads = []
    for H, g, (w1, b1, w2, _) in ((32, gs[0], ws[:4]), (64, gs[1], ws[4:])):
        part = torch.full((lib.singa_edge_mlp_bwd_nparts(E, H), H * 64 + H + H * H + H), float("nan"), device=DEV)
        g = g.to(DEV)
        assert bwd(_p(attr), _p(ua), _p(ub), _p(g), _p(w1), _p(b1), _p(w2), _p(part), E, 64, H, _stream()) == 0
        assert not bool(torch.isnan(part).any())                               # every partial row is written
        s = part.double().sum(0).cpu()
        o1, o2, o3 = H * 64, H * 64 + H, H * 64 + H + H * H
        grads.append([s[:o1].view(H, 64), s[o1:o2], s[o2:o3].view(H, H), s[o3:]])
    return [o.cpu() for o in outs], grads


def compare(attr, gs, nets, ua, ub, a, b, r, outs, grads):
    """-> [(name, got, want)] of the named rows' outputs and the eight gradients; rows no unit names must hold the sentinel."""
    named = torch.zeros(attr.shape[0], dtype=torch.bool)
    named[a], named[b] = True, True
    pairs = []
    for net, g, out, gr, nm in zip(nets, gs, outs, grads, "kv"):
        assert bool((out[~named] == SENTINEL).all()), "a row that no unit names was written"
        gu = g[a].double() + torch.where((b != a)[:, None], g[b].double(), torch.zeros((), dtype=torch.float64))
        want_o, want_g = reference(attr[a], gu, *net, r)
        assert torch.equal(out[a], out[b])                                      # a unit's two rows: the same registers
        pairs.append((f"w{nm}", out[a].double(), want_o))
        pairs += [(f"d{nm}.{p}", x, y) for p, x, y in zip(("w1", "b1", "w2", "b2"), gr, want_g)]
    return pairs


def draw(E, seed, round_weights):
    g = torch.Generator().manual_seed(seed)
    rb = (lambda t: t.bfloat16().float()) if round_weights else (lambda t: t)
    attr = torch.randn(E, 64, generator=g).bfloat16().float()                   # exactly representable: no rounding of attr
    nets = [[rb(torch.randn(H, 64, generator=g) / 8), torch.randn(H, generator=g), rb(torch.randn(H, H, generator=g) / H ** 0.5),
             torch.randn(H, generator=g)] for H in (32, 64)]
    gs = [torch.randn(E, H, generator=g) for H in (32, 64)]
    if round_weights:                     # ... and gradients whose unit sums are representable: h and g_pre alone are rounded
        gs = [torch.randint(-8, 9, (E, H), generator=g).float() / 8 for H in (32, 64)]
    return attr, gs, nets


# Largest error against the float64 reference with UNROUNDED operands over the cases below, measured on an MI355X
# (profiles/emlp_bf16/README.md) - outputs: max |error| / max |reference|, gradients: |error|_2 / |reference|_2.
#                                                                         outputs     gradients
#   attr representable (rounded: W1, W2, h, g, g_pre)                     3.026e-03   3.188e-03
#   weights and gradients representable as well (rounded: h, g_pre)       1.444e-03   1.636e-03
# The bounds are 4 x these: the error depends on the draw.
BOUND = {False: (4 * 3.026e-03, 4 * 3.188e-03), True: (4 * 1.444e-03, 4 * 1.636e-03)}


@pytest.mark.parametrize("E,round_weights", [(1, False), (31, False), (32, False), (33, False), (97, False), (97, True)])
def test_forward_and_backward_against_float64(E, round_weights):
    attr, gs, nets = draw(E, 7 * E + round_weights, round_weights)
    ua, ub, a, b = unit_list(E, E)
    outs, grads = run(attr, gs, nets, ua, ub)
    worst = [0.0, 0.0]
    for name, got, want in compare(attr, gs, nets, ua, ub, a, b, lambda t: t, outs, grads):
        k = 0 if name[0] == "w" else 1
        err = float((got - want).abs().max() / want.abs().max()) if k == 0 else float((got - want).norm() / want.norm())
        worst[k] = max(worst[k], err)
        print(f"E={E} round_weights={round_weights} {name}: {err:.3e}")
        assert err <= BOUND[round_weights][k], (name, err, BOUND[round_weights][k])
    print(f"E={E} round_weights={round_weights} worst: outputs {worst[0]:.3e}, gradients {worst[1]:.3e}")


@pytest.mark.parametrize("mode", ["identity", "saturated", "ties"])
def test_exact_integers(mode):
    """Small-integer operands and a first bias that makes the activation trivial, so that every product and f32 sum of both GEMMs
    and of all four gradients is exact: the kernels give the bits of the float64 evaluation on bf16-rounded operands, and a wrong
    fragment map or reduction order is an O(1) error.  identity: pre >= 128, softplus is the identity and sigmoid is 1 in f32.
    saturated: pre <= -128, h is -ln 2 everywhere and g_pre is 0.  ties: every attribute lies halfway between two bf16 neighbours
    (1 + 2^-8 goes down to 1, 1 + 3 * 2^-8 goes up to 1 + 2^-6: to even) and W1 = +-64 makes the difference an integer."""
    E = 97
    g = torch.Generator().manual_seed(len(mode))
    ri = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float()
    attr = ri(-2, 2, E, 64)
    scale, b1 = (64.0, 8192.0) if mode == "ties" else (1.0, -256.0 if mode == "saturated" else 256.0)
    if mode == "ties":
        attr = (1 + (2 * ri(0, 1, E, 64) + 1) * 2.0 ** -8) * (2 * ri(0, 1, E, 64) - 1)
        assert bool((_bf(attr) != attr.double()).all()) and float(_bf(torch.tensor(1 + 2.0 ** -8))) == 1.0
        assert float(_bf(torch.tensor(1 + 3 * 2.0 ** -8))) == 1 + 2.0 ** -6
    nets = [[scale * ri(-1, 1, H, 64), torch.full((H,), b1), ri(-1, 1, H, H), ri(-3, 3, H)] for H in (32, 64)]
    gs = [ri(-2, 2, E, H) for H in (32, 64)]
    ua, ub, a, b = unit_list(E, 3)
    outs, grads = run(attr, gs, nets, ua, ub)
    for name, got, want in compare(attr, gs, nets, ua, ub, a, b, _bf, outs, grads):
        assert float(want.abs().max()) > 0 or name.endswith(("w1", "b1"))      # (saturated: g_pre is 0)
        assert torch.equal(got.float(), want.float()), (mode, name, float((got - want).abs().max()))


@pytest.mark.parametrize("representable", [False, True])
def test_bias_gradients_come_from_unrounded_values(representable):
    """db2 is the f32 kernel's within the f32 summation order (n 2^-23 sum |x| for two orders of n terms) for any g; so is db1 where
    the rounding of the operands changes nothing (all of them representable), although g_pre itself is not: the sums take the
    unrounded registers.  A sum of rounded values would be off by about 2^-9 |x|_2, several times the allowance."""
    E = 97
    attr, gs, nets = draw(E, 5, representable)
    ua, ub, a, b = unit_list(E, 9)
    _, got = run(attr, gs, nets, ua, ub)
    _, want = run(attr, gs, nets, ua, ub, tag="")
    for net, g, gr, wr in zip(nets, gs, got, want):
        gu = g[a].double() + torch.where((b != a)[:, None], g[b].double(), torch.zeros((), dtype=torch.float64))
        H = gu.shape[1]
        pre = attr[a].double() @ net[0].double().t() + net[1].double()
        gp = (gu @ net[2].double()) * torch.sigmoid(pre)
        allow2 = E * 2.0 ** -23 * gu.abs().sum(0)
        assert bool(((gr[3] - wr[3]).abs() <= allow2).all()), float(((gr[3] - wr[3]).abs() / allow2).max())
        if representable:                   # + the two kernels' f32 sums inside pre (64 terms) and gh (H terms)
            allow1 = (E + 64 + H) * 2.0 ** -23 * gp.abs().sum(0)
            assert bool(((gr[1] - wr[1]).abs() <= allow1).all()), float(((gr[1] - wr[1]).abs() / allow1).max())


def _counted(monkeypatch):
    from singa_amd import _lib
    n = {}
    for name in ("singa_edge_mlp_units_fwd", "singa_edge_mlp_units_bwd", "singa_edge_mlp_bf16_units_fwd", "singa_edge_mlp_bf16_units_bwd"):
        def counted(*args, _inner=getattr(_lib.lib(), name), _name=name):
            n[_name] = n.get(_name, 0) + 1
            return _inner(*args)
        monkeypatch.setattr(_lib.lib(), name, counted)
    return n


# Relative error of the step with edge_mlp_precision="bf16" against the f32 step on the golden 3-graph batch at L = 2, measured on
# an MI355X (profiles/emlp_bf16/README.md):   logits 2.230e-05   loss 5.256e-07   total gradient norm 2.538e-06
# The bound is 4 x these, as CLOSE of tests/test_precision_gpu.py.
STEP_CLOSE = {"logits": 4 * 2.230e-05, "loss": 4 * 5.256e-07, "grad_norm": 4 * 2.538e-06}


def test_switch_reaches_the_edge_mlps_and_the_step_stays_close(monkeypatch):
    """The golden batch at L = 2: edge_mlp_precision="bf16" takes the new entry points for every launch the f32 step makes through
    the f32 ones (forward, and backward of both nets), precision="bf16" alone takes none of them, and the step stays close."""
    batch = PG._batch(2)
    n = _counted(monkeypatch)
    steps, calls = {}, {}
    for key, kw in (("f32", {}), ("gemm", {"precision": "bf16"}), ("emlp", {"edge_mlp_precision": "bf16"})):
        n.clear()
        steps[key] = PG._step(EP._model(2, **kw), batch)
        calls[key] = dict(n)
    f, b = "singa_edge_mlp_units_fwd", "singa_edge_mlp_units_bwd"
    assert calls["f32"].get(f, 0) >= 1 and calls["f32"][b] == 2 * calls["f32"][f] and calls["gemm"] == calls["f32"]
    assert calls["emlp"] == {f.replace("units", "bf16_units"): calls["f32"][f], b.replace("units", "bf16_units"): calls["f32"][b]}
    (lo_f, loss_f, gn_f), (lo_b, loss_b, gn_b) = steps["f32"], steps["emlp"]
    assert not torch.equal(lo_b, lo_f)
    err = {"logits": float((lo_b.double() - lo_f.double()).norm() / lo_f.double().norm()),
           "loss": abs(loss_b - loss_f) / abs(loss_f), "grad_norm": abs(gn_b - gn_f) / gn_f}
    print("edge_mlp_precision bf16 against f32, L=2: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert 0 < v <= STEP_CLOSE[k], (k, v, STEP_CLOSE[k])


def test_argument_errors_without_a_launch():
    from singa_amd import _lib, ops
    from singa_amd.ops import _p
    lib = _lib.lib()
    t = torch.zeros(64, 64, device=DEV)
    u = torch.zeros(64, dtype=torch.int32, device=DEV)
    fwd = lambda first, cin, hv: lib.singa_edge_mlp_bf16_units_fwd(first, _p(u), _p(u), *[_p(t)] * 8, _p(t), _p(t), 64, cin, 32, hv, None)
    bwd = lambda first, cin, h: lib.singa_edge_mlp_bf16_units_bwd(first, _p(u), _p(u), _p(t), _p(t), _p(t), _p(t), _p(t), 64, cin, h, None)
    assert fwd(None, 64, 64) == -1 and bwd(None, 64, 64) == -1                  # SINGA_E_NULL
    shape = [fwd(_p(t), 32, 64), fwd(_p(t), 64, 48), bwd(_p(t), 32, 64), bwd(_p(t), 64, 48)]
    assert len(set(shape)) == 1 and shape[0] not in (0, -1), shape               # SINGA_E_SHAPE
    nets = [(torch.nn.Linear(64, H, device=DEV), torch.nn.Linear(H, H, device=DEV)) for H in (32, 64)]
    with pytest.raises(ValueError, match="unit"):
        ops.edge_mlp_pair(t, nets[0], nets[1], precision="bf16")
