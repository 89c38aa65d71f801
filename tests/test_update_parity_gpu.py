"""-m gpu: the UPDATE half of the training step - singa_adam_step, singa_grad_norm, the clipping coefficient, the device-side
learning rate and step count, the warm-up's snapshot and restore, resuming from a checkpoint - per element, with MOVING
parameters.  (tests/test_replay_parity_gpu.py pins the other half, the gradients, at lr = 0; its fixtures are used here: the
lmax = 2 model, two-graph batches of 45 to 80 protein atoms, its sequence over three captures.)

Protocol: step 0 runs at lr = 0 on every engine (the optimizer is built, the first capture taken, the eager engine reaches its
in-place gradient path); then param_groups[0]['lr'] is set to the reference's 1e-4 - after the capture - and every public
step() is bracketed by clones of all 724 parameters, both moments, the step count and, after the step, .grad.  The criterion is
tests/adam_rule.check_step: the float64 rule on the bracketing values with the k the step should have and the rate in force.

a. every step against the rule, eager / use_graph / use_graph + bucket; the 90 gradient-free tensors keep their bits and have
   no state; the step count equals the number of public steps (warm-ups leave nothing behind);
b. a real ReduceLROnPlateau(factor 0.5, patience 0, as train.py:147) halves the rate between two replays of one capture,
   directly before a step that captures and directly before a switch back to an older capture: the rule holds with the new
   rate in the very next step, and `captures` does not grow when only the rate changes;
c. max_grad_norm = half the first batch's norm: .grad after the step is the clipped gradient, so the rule applies unchanged,
   and the reported norm is the float64 norm of .grad / coef at 1e-6;
d. the bucketed engine and an eager engine on a copy of the model over the same staged batches and rate changes: all
   parameters, both moments and the step count torch.equal after each of seven steps;
e. resume: three steps, state_dict() of model and optimizer (torch layout, lr included) into a fresh model, Adam and TrainStep
   - whose capture then happens at k = 4 with live moments - and three more steps, against six uninterrupted ones: the same
   bits in every parameter and moment.

Measured on an MI355X (16,055,008 elements in the 634 active tensors): (d) and (e) hold BIT FOR BIT - every parameter, both
moments and the step count torch.equal after each of the seven steps / after the six - and are asserted so.  (a)-(c): the
parameter's error reaches 0.998 ... 1.000 of its bound in every moving step (the bound's leading term, 1/2 ulp of p, is what a
correct kernel's final rounding uses up); the update proper, read off the 14,001 elements that still are exactly 0 in the
first moving step (k = 2): 2.7e-6 relative (bound 3.7e-5; the kernel cases' 2.8e-6); moments where g and m do not oppose and
nothing underflows: m 1.5e-7, v 1.7e-7 (bound 2.4e-7); from k = 3 on 35 to 48 % of the elements have g m < 0 and 2,000 to
3,800 a v' below 2^-126 (see adam_rule.check_step for both).  Reported norm against .grad / coef: 6.9e-8 at worst.
Tried and not kept: TrainStep._replay without sync_hyper() fails (a) in both graph modes, (c) bucketed, (d) and (e), and no
test from before this file; Adam.restore that leaves step_t advanced fails the same five."""
import copy
import math

import pytest
import torch

from tests import adam_rule as R
from tests.helpers import named_grads
from tests.test_replay_parity_gpu import _batch, _engine, _model

pytestmark = pytest.mark.gpu
LR = 1e-4
MODES = {"eager": dict(use_graph=False), "graph": dict(use_graph=True), "bucket": dict(use_graph=True, bucket=True)}


@pytest.fixture(scope="module")
def batches():
    sizes = [(46, 230), (45, 226), (47, 234), (45, 224)]
    b = [_batch(80 + 3 * i, n, e) for i, (n, e) in enumerate(sizes)]
    return b, _batch(200, 80, 400)


def _snap(eng):
    """({name: (p, m, v)} - clones; m = v = None for a tensor without optimizer state - , the step count)."""
    torch.cuda.synchronize()
    opt = eng.opt
    built = getattr(opt, "_built", False)
    mom = {id(p): (m, v) for p, m, v in zip(opt.active, opt.exp_avg, opt.exp_avg_sq)} if built else {}
    out = {}
    for n, p in eng.model.named_parameters():
        m, v = mom.get(id(p), (None, None))
        out[n] = (p.detach().clone(), None if m is None else m.clone(), None if v is None else v.clone())
    return out, (float(opt.step_t) if built else 0.0)


def _checked_step(eng, batch, k, label):
    """One public step between two snapshots, held to the rule -> (snapshot after, .grad after)."""
    before, k0 = _snap(eng)
    g = eng.opt.param_groups[0]
    lr, betas, eps = g["lr"], g["betas"], g["eps"]
    eng.step(batch)
    after, k1 = _snap(eng)
    grads = named_grads(eng.model)
    assert (k0, k1) == (float(k - 1), float(k)), (label, k0, k1, k)
    assert len(before) == 724 and len(grads) == 634, (len(before), len(grads))
    for n, (p, m, v) in after.items():
        if n in grads:
            assert m is not None and v is not None, n
        else:                                                   # never receives a gradient: initial bits, no state
            assert m is None and v is None and torch.equal(p, before[n][0]), n
    zero = lambda n, t: torch.zeros_like(before[n][0]) if t is None else t        # (before the first step: no moments yet)
    b4 = {n: (before[n][0], zero(n, before[n][1]), zero(n, before[n][2])) for n in grads}
    R.check_step(b4, {n: after[n] for n in grads}, grads, k, lr, betas, eps, label=label)
    return after, grads


def _plateau(opt):
    """ReduceLROnPlateau as train.py:147 builds it, its best metric set: every further step(1.0) halves the rate."""
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=0.5, patience=0)
    sched.step(1.0)
    return sched


def _halve(scheds, opts):
    for s in scheds:
        s.step(1.0)
    lrs = {o.param_groups[0]["lr"] for o in opts}
    assert len(lrs) == 1
    return lrs.pop()


# ------------------------------------------------------------------------------------------------ a, b
def _plan(mode, batches):
    """(batches, the steps a rate change falls directly before, `captures` after every step)."""
    b, wide = batches
    if mode == "graph":          # (one capture at a time: a new shape captures again)
        return [b[0], b[0], b[0], wide, wide, b[0]], {2: "between two replays of one capture", 3: "before a capture",
                                                      5: "before a capture"}, [1, 1, 1, 2, 2, 3]
    seq = [b[0], wide, b[1], wide, b[2], wide, b[3], b[3]]
    why = {2: "before a capture", 3: "before a switch back to an older capture", 7: "between two replays of one capture"}
    return seq, why, ([1, 2, 3, 3, 3, 3, 3, 3] if mode == "bucket" else [0] * 8)


@pytest.mark.parametrize("mode", list(MODES))
def test_every_step_follows_the_rule_with_the_rate_in_force(batches, mode):
    seq, changes, captures = _plan(mode, batches)
    model = _model()
    first = {n: p.detach().clone() for n, p in model.named_parameters()}
    eng = _engine(model, **MODES[mode])
    sched, lr, moved = None, 0.0, []
    for i, x in enumerate(seq):
        if i == 1:
            eng.opt.param_groups[0]["lr"] = lr = LR                     # after the first capture
            sched = _plateau(eng.opt)
        if i in changes:
            lr = _halve([sched], [eng.opt])
            assert lr == LR * 0.5 ** sorted(changes).index(i) / 2, (i, lr)
        before_captures = eng.captures
        after, _ = _checked_step(eng, x, i + 1, f"{mode} step {i}" + (f" (rate halved {changes[i]})" if i in changes else ""))
        assert eng.captures == captures[i], (i, eng.captures, captures)
        if i in changes and "replays" in changes[i]:
            assert eng.captures == before_captures                        # only the rate changed
        moved.append(sum(not torch.equal(after[n][0], first[n]) for n in first))
    assert moved[0] == 0 and 0 < moved[1] <= moved[-1] <= 634, moved              # lr = 0 froze them; then they move
    state = eng.opt.state_dict()["state"]
    names = [n for n, _ in model.named_parameters()]
    assert len(state) == 634 and all(float(st["step"]) == len(seq) for st in state.values())
    assert sorted(names[i] for i in state) == sorted(n for n in names if after[n][1] is not None)
    if mode != "eager":
        eng.release()


# ------------------------------------------------------------------------------------------------ c
@pytest.fixture(scope="module")
def first_norm(batches):
    eng = _engine(_model(), use_graph=False)
    eng.step(batches[0][0])
    return float(eng.grad_norm)


@pytest.mark.parametrize("mode", ["eager", "bucket"])
def test_clipping_while_moving(batches, first_norm, mode):
    max_norm = 0.5 * first_norm
    eng = _engine(_model(), max_grad_norm=max_norm, **MODES[mode])
    clipped = []
    for i, x in enumerate(batches[0][:3]):
        if i == 1:
            eng.opt.param_groups[0]["lr"] = LR
        _, grads = _checked_step(eng, x, i + 1, f"clipped, {mode} step {i}")
        norm = eng.grad_norm.detach().float().cpu()
        coef = float((max_norm / (norm + 1e-6)).clamp(max=1.0))                 # float32, as TrainStep._update forms it
        norm64 = math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads.values())) / coef
        err = abs(float(norm) - norm64) / norm64
        print(f"clipped, {mode} step {i}: reported norm {float(norm)!r}, float64 norm of .grad / coef {norm64!r} ({err:.2e}), coef {coef!r}")
        assert err <= 1e-6, (float(norm), norm64)
        clipped.append(coef < 1.0)
    assert clipped[0] and clipped[1], clipped                  # in force while the parameters move (step 0: coef = 1/2)
    if mode != "eager":
        assert eng.captures == 1
        eng.release()


# ------------------------------------------------------------------------------------------------ d
def _opt_state(eng):
    torch.cuda.synchronize()
    names = {id(p): n for n, p in eng.model.named_parameters()}
    out = {"step_t": eng.opt.step_t.clone()}
    for n, p in eng.model.named_parameters():
        out["p " + n] = p.detach().clone()
    for p, m, v in zip(eng.opt.active, eng.opt.exp_avg, eng.opt.exp_avg_sq):
        out["m " + names[id(p)]], out["v " + names[id(p)]] = m.clone(), v.clone()
    return out


def _first_difference(a, b):
    assert list(a) == list(b)
    for key in a:
        if not torch.equal(a[key], b[key]):
            d = (a[key].double() - b[key].double()).abs()
            return key, float(d.max()), float(d.max() / b[key].double().abs().max().clamp_min(1e-300))
    return None


def test_bucketed_replay_equals_eager_bit_for_bit(batches):
    """Same kernels on the same bits: the gradients were measured bit-equal with frozen parameters (634 of 634,
    tests/test_replay_parity_gpu.py), the Adam launch is one kernel over them.  The eager engine first runs ONE gradient-only
    pass (no optimizer) over the first staged batch, so that all of its seven public steps accumulate parameter gradients in
    place as the captures do (its first pass only finds out which parameters are produced that way)."""
    b, wide = batches
    seq = [b[0], wide, b[1], wide, b[2], wide, b[3]]
    run, ref = _engine(_model(), **MODES["bucket"]), _engine(_model(), use_graph=False)
    scheds = None
    for i, x in enumerate(seq):
        pb = run._stage(x)
        if i == 0:
            ref._prepared(pb)
            ref._fwd_bwd(pb)
            ref.opt.zero_grad(set_to_none=True)
            assert ref._sink_params is not None and not getattr(ref.opt, "_built", False)
        if i == 1:
            for e in (run, ref):
                e.opt.param_groups[0]["lr"] = LR
            scheds = [_plateau(run.opt), _plateau(ref.opt)]
        if i in (2, 3, 5):
            assert _halve(scheds, [run.opt, ref.opt]) < LR
        run.step(pb)
        ref.step(pb)
        got, want = _opt_state(run), _opt_state(ref)
        assert float(got["step_t"]) == i + 1
        diff = _first_difference(got, want)
        assert diff is None, (f"step {i}: first tensor that differs, largest absolute and relative difference", diff)
    assert run.captures == 3 and len(run._sink_params) == len(ref._sink_params)
    run.release()


# ------------------------------------------------------------------------------------------------ e
def test_resume_continues_the_uninterrupted_run_bit_for_bit(batches):
    """Both runs follow the protocol (step 0 at lr = 0, then 1e-4); the checkpoint is taken from a run of its own."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = batches[0][0]

    def run(steps):
        eng = _engine(_model(), **MODES["graph"])
        for i in range(steps):
            if i == 1:
                eng.opt.param_groups[0]["lr"] = LR
            eng.step(batch)
        torch.cuda.synchronize()
        assert eng.captures == 1
        return eng

    eng = run(6)
    want = _opt_state(eng)
    eng.release()
    eng = run(3)
    ckpt = copy.deepcopy({"model": eng.model.state_dict(), "opt": eng.opt.state_dict()})
    eng.release()
    del eng
    assert ckpt["opt"]["param_groups"][0]["lr"] == LR and len(ckpt["opt"]["state"]) == 634
    assert all(float(st["step"]) == 3.0 for st in ckpt["opt"]["state"].values())

    model = _model(seed=6)                                                      # other initial values: everything comes from the checkpoint
    model.load_state_dict(ckpt["model"])
    opt = Adam(model.parameters(), lr=7e-4)
    opt.load_state_dict(ckpt["opt"])
    assert opt.param_groups[0]["lr"] == LR
    res = TrainStep(model, opt, None, **MODES["graph"])
    for i in range(3, 6):
        _checked_step(res, batch, i + 1, f"resumed step {i}")                   # the first one: k = 4, captured with live moments
    assert res.captures == 1
    got = _opt_state(res)
    diff = _first_difference(got, want)
    assert diff is None, ("first tensor that differs, largest absolute and relative difference", diff)
    res.release()
