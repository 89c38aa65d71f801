"""-m gpu: the mode every throughput figure comes from - TrainStep(use_graph=True, bucket=True): ragged batches padded to a
size class and replayed from a few captured HIP graphs - checked PER PARAMETER instead of by its loss.

Parameters are frozen throughout (learning rate 0: the Adam kernel subtracts 0 * x, checked bit for bit), so the gradient of
a batch is a fixed quantity, `exp_avg` is an exact linear function of the gradients that reached the optimizer, and the
public `step()` path - optimizer graph included - can be used everywhere.

1. determinism and history independence, bit level: the same batch replayed twice, after a larger batch of its capture, and
   after a batch of another class gives the same bits (loss and all 634 gradients);
2. the replayed gradients against an eager engine on a copy of the model, (a) on the same padded batch, (b) on the batch itself;
3. the Adam moments after a sequence that switches between three captures against the eager engine's;
4. gradient clipping (max_grad_norm finite) inside the captured optimizer graph;
5. train mode: the positional-encoding dropout (Q9) is redrawn per replay, a seeded run is reproducible, p = 0 equals eval;
6. two batches with equal atom / edge totals and different graph counts;
7. the ragged and the isolated-atoms batch of tests/test_edge_cases_gpu.py behind a larger batch of their class.

Criterion wherever two runs may round differently (another launch geometry: padded against unpadded rows): the per-parameter
one of tests/test_padding_gpu.py, helpers.grad_mismatches, with the reference's decision at tied ReLU gates pinned to the
replay's (`_pin_ties`).  All batches carry their edge-frame draws (`rot_rand`, Q6), so no
run draws frames of its own.

Measured on an MI355X: checks 1, 2(a) and 5 hold bit for bit (2(a): 634 of 634 gradients and the loss torch.equal between
the replay and the eager engine on the same padded batch, in both layouts), so they are asserted with torch.equal; 2(b), against
the unpadded batch: no gradient bit-equal, largest relative difference 3.4e-6."""
import numpy as np
import pytest
import torch

from tests.helpers import (bit_equal_report, grad_mismatches, named_grads, pinned_relu_ties, relu_gate_flips,
                           relu_gate_log)

pytestmark = pytest.mark.gpu
DEV = "cuda"
KW = dict(n_ligand=12, e_ll=24, e_x=30)


def _batch(first, n_protein, e_pp, n=2, **kw):
    from singa_amd import graph as G
    return G.synthetic_batch(n, first_id=first, n_protein=n_protein, e_pp=e_pp, **{**KW, **kw}).to(DEV)


def _model(seed=5, train=False):
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    torch.manual_seed(seed)
    model = SINGA(load_config(lmax=2), device=DEV)
    return model.train() if train else model.eval()


def _engine(model, **kw):
    """A TrainStep over `model` with frozen parameters: lr = 0 before the first step."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    opt = Adam(model.parameters(), lr=1e-4)
    opt.param_groups[0]["lr"] = 0.0
    return TrainStep(model, opt, None, **kw)


def _step(eng, batch):
    """One public step -> (loss, gradients), both cloned."""
    loss = eng.step(batch).detach().clone()
    return loss, named_grads(eng.model)


def _eager_reference(seed=5):
    """An eager engine on a copy of the model (same seed, same frozen parameters).  From its second step on parameter
    gradients take the same in-place accumulation path (`ops._GradSink`) as inside a capture."""
    return _engine(_model(seed), use_graph=False)


class _Replay:
    """A bucketed graph engine whose steps also return the ReLU gates of the replayed pass (relu_gate_log: 18 masks per
    capture, rewritten by its replays)."""

    def __init__(self, model=None, **kw):
        self.eng = _engine(model or _model(), use_graph=True, bucket=True, **kw)
        self.log, self.by_sig, self.seen = relu_gate_log(capturing=True), {}, 0

    def __enter__(self):
        self.log.__enter__()
        return self

    def __exit__(self, *exc):
        self.eng.release()
        return self.log.__exit__(*exc)

    def step(self, batch):
        loss, grads = _step(self.eng, batch)
        if len(self.log.masks) > self.seen:                      # this step captured
            assert len(self.log.masks) == self.seen + 18
            self.seen = len(self.log.masks)
            self.by_sig[self.eng._active] = self.log.masks[-18:]
        return loss, grads, [m.clone() for m in self.by_sig[self.eng._active]]


def _pin_ties(want, ref_masks, got, batch, spare):
    """The eager reference `want` of 2(b) with the replayed run's decision at TIED ReLU gates.  The replay (padded rows) and
    the eager run (the batch itself) round differently (measured: 3e-6 on the gradients), so a PoswiseFeedForward
    pre-activation within rounding of zero is positive in one and negative in the other; the gate is a step function, and ONE
    such gate moves its unit's row of conv1's gradient by 2e-4 of the whole tensor whichever run is right (measured on the
    three-graph batch of check 6: unit 766 of decoder layer 3 carried 5.455e-4 of a 5.540e-4 difference; the losses were
    bit-equal).  As for the oracle comparisons ("ReLU ties") the reference is run again with those gates
    pinned to the other side's choice; at most 16 of them, the cap tests/test_workloads_gpu.py uses - two runs of the same code
    that disagree on more gates than that disagree on more than rounding.  `spare()`: an eager engine for that second run."""
    flips = relu_gate_flips(ref_masks, got[2])
    n = int(flips["on"].numel())
    assert n <= 16, n
    if n:
        with pinned_relu_ties(records=flips) as pins:
            want = _step(spare(), batch)
        assert pins.call == 18 and pins.flipped == n, (pins.call, pins.flipped, n)
    print(f"{n} tied ReLU gates pinned to the replay's choice")
    return want


def _eager_unpadded(ref, batch, got):
    """2(b)'s reference for the replayed result `got` = (loss, gradients, gates): the eager engine `ref` on the batch itself."""
    with relu_gate_log() as log:
        want = _step(ref, batch)
    return _pin_ties(want, log.take(), got, batch, lambda: ref)


def _assert_same_bits(got, want):
    assert torch.equal(got[0], want[0]), (float(got[0]), float(want[0]))
    assert set(got[1]) == set(want[1])
    differ = [n for n, g in want[1].items() if not torch.equal(got[1][n], g)]
    assert not differ, (len(differ), differ[:6])
    if len(got) > 2 and len(want) > 2:
        assert all(torch.equal(a, b) for a, b in zip(got[2], want[2]))


# ------------------------------------------------------------------------------------------------ 1 and 2: one shared run
@pytest.fixture(scope="module")
def history():
    """The bucketed engine's run of checks 1 and 2 (three captures)."""
    bs = dict(first=_batch(80, 46, 230), large=_batch(86, 47, 234), small=_batch(89, 45, 224), wide=_batch(200, 80, 400))
    model = _model()
    before = [p.detach().clone() for p in model.parameters()]
    h = {}
    with _Replay(model) as run:
        eng = run.eng
        run.step(bs["first"])
        h["A"] = run.step(bs["small"])
        h["A_again"] = run.step(bs["small"])
        run.step(bs["large"])
        h["A_after_large"] = run.step(bs["small"])
        h["captures_narrow"] = eng.captures
        h["staged_narrow"] = eng._stage(bs["small"])              # the padded batch that step replayed
        run.step(bs["wide"])
        h["B"] = run.step(bs["small"])
        h["staged_wide"] = eng._stage(bs["small"])
        run.step(bs["wide"])
        h["B_again"] = run.step(bs["small"])
        h["captures_wide"] = eng.captures
        torch.cuda.synchronize()
        h["params_unchanged"] = all(torch.equal(p, q) for p, q in zip(model.parameters(), before))
        h["n_sink"] = len(eng._sink_params)
    h["batches"] = bs
    return h


@pytest.fixture(scope="module")
def references(history):
    """The eager references of check 2 for `small` as `history` replayed it: on the two padded batches and on the batch itself."""
    h, bs, r = history, history["batches"], {}
    ref = _eager_reference()
    _step(ref, bs["first"])
    assert len(ref._sink_params) == h["n_sink"]
    r["padded_narrow"] = _step(ref, h["staged_narrow"])
    r["padded_wide"] = _step(ref, h["staged_wide"])
    r["unpadded_narrow"] = _eager_unpadded(ref, bs["small"], h["A_after_large"])
    r["unpadded_wide"] = _eager_unpadded(ref, bs["small"], h["B"])
    return r


def test_learning_rate_zero_freezes_the_parameters(history):
    assert history["params_unchanged"]
    assert len(history["A"][1]) == 634                      # 634 of the 724 tensors carry gradients


def test_replay_is_deterministic(history):
    """The same batch replayed twice: the library has no float atomics and its reductions run in a fixed order."""
    _assert_same_bits(history["A_again"], history["A"])


def test_replay_is_independent_of_the_previous_batch(history):
    """`small` behind the larger `large` in the same capture: nothing of `large` (padded rows of the static buffers, gradient
    buffers accumulated in place, kNN slots) reaches it."""
    assert history["captures_narrow"] == 1
    _assert_same_bits(history["A_after_large"], history["A"])


def test_replay_is_independent_of_a_capture_switch(history):
    """`wide` opens a second class and widens the dense layout, so `small`'s class is captured again; from then on `small`
    behind `wide` (another capture's .grad set and gradient-address table in between) repeats its bits."""
    assert history["captures_wide"] == 3
    _assert_same_bits(history["B_again"], history["B"])
    assert not grad_mismatches(history["B"][1], history["A"][1])          # (the wider layout changes rounding only)


@pytest.mark.parametrize("layout", ["narrow", "wide"])
def test_replay_equals_eager_on_the_same_padded_batch(history, references, layout):
    """2(a): same shapes, same kernels, same gradient-accumulation path; only the launch context (replayed graph against
    eager launches) differs - and every bit agrees."""
    got = history["A_after_large" if layout == "narrow" else "B"]
    want = references["padded_" + layout]
    same, n, worst = bit_equal_report(got[1], want[1], f"replay vs eager, same padded batch ({layout})")
    print(f"loss {float(got[0])!r} vs {float(want[0])!r}")
    assert not grad_mismatches(got[1], want[1])
    _assert_same_bits(got, want)


@pytest.mark.parametrize("layout", ["narrow", "wide"])
def test_replay_equals_eager_on_the_unpadded_batch(history, references, layout):
    """2(b): with padded-against-unpadded (test_padding_gpu) and eager-against-oracle (test_workloads_gpu) this closes the
    chain from the replayed step to the oracle."""
    got = history["A_after_large" if layout == "narrow" else "B"]
    want = references["unpadded_" + layout]
    bit_equal_report(got[1], want[1], f"replay vs eager, unpadded batch ({layout})")
    assert abs(float(got[0]) - float(want[0])) < 1e-5 * float(want[0])
    assert not grad_mismatches(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 3: optimizer state
def test_adam_moments_across_capture_switches_match_eager():
    """Seven steps over three captures with frozen parameters: exp_avg is a fixed linear combination of the seven gradients,
    exp_avg_sq a quadratic one.  A stale gradient-address table feeds another capture's gradients into the moments;
    an unswapped .grad set shows another batch's gradients to whoever reads .grad after the step."""
    sizes = [(46, 230), (45, 226), (47, 234), (45, 224)]
    b = [_batch(80 + 3 * i, n, e) for i, (n, e) in enumerate(sizes)]
    wide = _batch(200, 80, 400)
    seq = [b[0], wide, b[1], wide, b[2], wide, b[3]]

    def state(eng):
        torch.cuda.synchronize()
        return {i: {k: v.clone() for k, v in st.items()} for i, st in eng.opt.state_dict()["state"].items()}

    with _Replay() as run:
        steps = [run.step(x) for x in seq]
        got, captures = state(run.eng), run.eng.captures
    assert captures == 3
    ref, spare = _eager_reference(), []

    def spare_engine():                       # (the moments of `ref` must see every batch exactly once)
        if not spare:
            spare.append(_eager_reference())
        return spare[0]

    for i, (x, step) in enumerate(zip(seq, steps)):
        # after EVERY step .grad is the gradient of that step's batch: the set of the capture that just ran (check 2(b))
        with relu_gate_log() as log:
            w = _step(ref, x)
        w = _pin_ties(w, log.take(), step, x, spare_engine)
        assert not grad_mismatches(step[1], w[1]), i
    want = state(ref)
    assert set(got) == set(want) and len(want) == 634
    assert all(float(got[i]["step"]) == float(want[i]["step"]) == 7.0 for i in want)
    for key, rel in (("exp_avg", 2e-4), ("exp_avg_sq", 4e-4)):
        bad = grad_mismatches({str(i): st[key] for i, st in got.items()}, {str(i): st[key] for i, st in want.items()}, rel)
        assert not bad, (key, bad[:6])


# ------------------------------------------------------------------------------------------------ 4: gradient clipping
@pytest.fixture(scope="module")
def unclipped():
    """One batch, its unclipped eager gradient g, the float64 norm of g and the norm the engine reported."""
    batch = _batch(80, 46, 230)
    eng = _engine(_model(), use_graph=False)
    _, g = _step(eng, batch)
    norm64 = float(torch.sqrt(sum((v.double() ** 2).sum() for v in g.values())))
    return batch, g, norm64, float(eng.grad_norm)


@pytest.mark.parametrize("mode", ["eager", "graph", "bucket"])
def test_gradient_clipping(unclipped, mode):
    """max_grad_norm = half the batch's gradient norm: after one step from zero moments exp_avg = (1 - beta1) * coef * g with
    coef = max_norm / (norm + 1e-6) (torch's clip_grad_norm_), the reported norm is the unclipped one, and a second
    step repeats the first one's bits - the in-place scaling of .grad does not compound."""
    batch, g, norm64, reported = unclipped
    max_norm = 0.5 * reported
    model = _model()
    eng = _engine(model, use_graph=mode != "eager", bucket=mode == "bucket", max_grad_norm=max_norm)
    names = {id(p): n for n, p in model.named_parameters()}
    _, g1 = _step(eng, batch)
    norm1 = eng.grad_norm.detach().clone()
    exp_avg = {names[id(p)]: m.clone() for p, m in zip(eng.opt.active, eng.opt.exp_avg)}
    _, g2 = _step(eng, batch)
    norm2 = eng.grad_norm.detach().clone()
    print(f"{mode}: reported norm {float(norm1)!r}, float64 norm of the eager gradient {norm64!r}")
    assert abs(float(norm1) - norm64) <= 1e-6 * norm64, (float(norm1), norm64)
    coef = max_norm / (norm64 + 1e-6)
    beta1 = eng.opt.param_groups[0]["betas"][0]
    bad = grad_mismatches(exp_avg, {n: (1.0 - beta1) * coef * v.double() for n, v in g.items()})
    assert not bad, bad[:6]
    assert not grad_mismatches(g1, {n: coef * v.double() for n, v in g.items()})       # .grad holds the clipped gradient
    if mode == "eager":            # (its first step finds the in-place accumulated parameters, its second one uses that path)
        assert abs(float(norm1) - float(norm2)) <= 1e-6 * norm64 and not grad_mismatches(g2, g1)
    else:
        assert torch.equal(norm1, norm2)
        assert [n for n in g1 if not torch.equal(g1[n], g2[n])] == []
        assert eng.captures == 1
        eng.release()


# ------------------------------------------------------------------------------------------------ 5: train mode
def _train_mode_run(use_graph=True, train=True, p=None, seed=7, steps=4):
    model = _model(seed, train=train)                     # torch.manual_seed(seed), then the model
    if p is not None:
        model.model.decoder.pos_emb.dropout.p = p       # the switch of train.py --no-dropout
    eng = _engine(model, use_graph=use_graph, bucket=use_graph)
    batch = _batch(80, 46, 230)
    losses = torch.stack([eng.step(batch).detach().clone() for _ in range(steps)])
    grads = named_grads(model)
    if use_graph:
        assert eng.captures == 1
        eng.release()
    return losses.cpu(), grads


@pytest.fixture(scope="module")
def train_runs():
    return {"graph": _train_mode_run(), "graph_again": _train_mode_run(), "eager": _train_mode_run(use_graph=False)}


def test_dropout_mask_is_redrawn_on_every_replay(train_runs):
    for mode in ("graph", "eager"):
        losses = train_runs[mode][0]
        assert torch.isfinite(losses).all() and len(set(losses.tolist())) > 1, (mode, losses.tolist())


def test_seeded_replayed_run_is_reproducible(train_runs):
    a, b = train_runs["graph"], train_runs["graph_again"]
    assert torch.equal(a[0], b[0]), (a[0].tolist(), b[0].tolist())
    assert [n for n in a[1] if not torch.equal(a[1][n], b[1][n])] == [] and set(a[1]) == set(b[1])


def test_train_mode_without_dropout_equals_eval_mode():
    off, ev = _train_mode_run(p=0.0), _train_mode_run(train=False)
    assert torch.equal(off[0], ev[0]), (off[0].tolist(), ev[0].tolist())
    assert len(set(off[0].tolist())) == 1
    assert [n for n in ev[1] if not torch.equal(off[1][n], ev[1][n])] == [] and set(off[1]) == set(ev[1])


# ------------------------------------------------------------------------------------------------ 6: graph count
def test_graph_count_is_part_of_the_size_class():
    """Two graphs of 69 protein atoms and three of 46: the same atom and edge totals (bonded edges come in pairs, so 345 asked
    for per graph are 344: 688 against 690, one size class), and with `two` first the dense layout is 80 wide for both -
    everything but the number of graphs says "same capture", while pointer, token and property tensors are [B(+1), ...].
    Without the graph count in the signature `three` was loaded into `two`'s capture and the step died on "a padded batch
    does not fit the buffers of its own size class"."""
    from singa_amd import graph as G
    two = _batch(300, 69, 345, n=2, n_ligand=18, e_ll=36, e_x=45)
    three = _batch(310, 46, 230, n=3)
    assert G.batch_sizes(two) == (138, 36, 688, 72, 90) and G.batch_sizes(three) == (138, 36, 690, 72, 90)
    with _Replay() as run:
        got_two = run.step(two)
        s2, s3 = (run.eng._stage(x).extras["pad"]["sig"] for x in (two, three))
        assert [(a, b) for a, b in zip(s2, s3) if a != b] == [(2, 3)], (s2, s3)     # they collide but for the graph count
        got_three = run.step(three)
        assert run.eng.captures == 2
    ref = _eager_reference()
    for got, batch in ((got_two, two), (got_three, three)):
        want = _eager_unpadded(ref, batch, got)
        assert abs(float(got[0]) - float(want[0])) < 1e-5 * float(want[0])
        assert not grad_mismatches(got[1], want[1])


# ------------------------------------------------------------------------------------------------ 7: awkward batches
def _awkward(case, grow=0):
    """The batch `case` of tests/test_edge_cases_gpu.py, its last graph `grow` protein atoms larger; edge-frame draws pinned."""
    from singa_amd import graph as G
    from tests.test_edge_cases_gpu import CASES, make_arrays
    kws = [dict(kw) for kw in CASES[case]]
    kws[-1]["n_p"] += grow
    b = G.collate([G.from_arrays(make_arrays(**kw), with_lap=False) for kw in kws])
    rng = np.random.default_rng(17)
    b.extras["rot_rand"] = {k: torch.tensor(rng.random((b[et]["edge_index"].shape[1], 3)), dtype=torch.float32)
                            for k, et in (("pp", G.E_PP), ("ll", G.E_LL), ("lp", G.E_LP))}
    return b.to(DEV)


@pytest.mark.parametrize("case,grow", [("ragged", 6), ("isolated_atoms", 4)])
def test_awkward_batch_behind_a_larger_one_of_its_class(case, grow):
    """A ligand smaller than the kNN degree / atoms without any edge, replayed from the capture a larger batch of the same
    class opened: empty segments and absent kNN slots reach the backward kernels behind the larger batch's rows."""
    larger, batch = _awkward(case, grow), _awkward(case)
    with _Replay() as run:
        run.step(larger)
        got = run.step(batch)
        assert run.eng.captures == 1
    ref = _eager_reference()
    _step(ref, larger)
    want = _eager_unpadded(ref, batch, got)
    assert len(want[1]) == 634
    assert abs(float(got[0]) - float(want[0])) < 1e-5 * float(want[0])
    assert not grad_mismatches(got[1], want[1])
