"""-m gpu: the two-stream passes - Part 3 of the embedding beside Part 4 (EquivariantEmbedding._forward), the ligand encoder
beside the protein encoder (Transformer._encoders_two_streams) - against the same passes on ONE stream, and against themselves
with one of the two streams held back on purpose.

Both forks claim "same arithmetic in the same order inside each pass; autograd mirrors the split in the backward pass".  At the
small shapes of a test one stream is always far ahead of the other, so a read of a buffer the other stream has not finished
writing, a gradient flush that overtakes the second stream's backward nodes, or an allocator block handed out again across the
fork passes as long as the timing is kind.  Here the timing is made unkind the way PyTorch's own stream tests do it:
`torch.cuda._sleep(cycles)` - a plain kernel, captured into a HIP graph like any other - is enqueued on a chosen stream at a
chosen point, by monkeypatching only (`inject`):

  fwd-aux   on the second stream whenever a pass asks for it (`ops.branch_stream`): the head of Part 3 and of the ligand encoder;
  fwd-cur   on the current stream right after the fork: in front of Part 4 and of the protein encoder;
  bwd-aux   in the backward pass of an identity (`_Hold`) behind the LAST forward operation of the second stream's branch (Part
            3's result, the ligand encoder's output): the first thing that stream does in the backward pass;
  bwd-cur   the same behind Part 4's result and the protein encoder's output.

Calibration (`calibration`, once per session, nothing hard-coded): one `_sleep` between two events gives cycles per ms; one
undelayed eager step of the test batch between two events gives the step time; the delay is MARGIN = 2 x that step time, so the
stream that is not held back can run the whole step - every launch the host issues - before the held-back stream's writes land.
Measured on an MI355X in two sessions (profiles/stream_overlap/README.md): 2,389,007 / 2,389,472 `_sleep` cycles per ms; the
undelayed eager step of the test batch 48.1 / 84.8 ms (host-bound: it varies with the load of the host); so delays of 96.2 / 169.6
ms = 2.30e8 / 4.05e8 cycles.

0. self-check: a toy two-stream function reads, on the current stream, a tensor the second stream writes behind the delay;
   without its wait_stream it returns the stale contents, with it the new ones - the delay is long enough to expose a hazard;
1. fork against no fork, eager: {hetero, encoders} in {on/off, off/on, on/on} against off/off for the four precision pairs,
   with the gradient sink off (an engine's first step: a plain backward()) and on (its second step), bit for bit;
2. the four delays change nothing, eager, sink on, one backward() and the engine's two-phase backward (two flushes); nor does
   a fifth, bwd-tail: the delay in front of one of the last 16 launches of each run of second-stream launches in the backward
   pass (`launch_log`), which is where `_GradSink.flush()` could overtake a node that hands nothing back to autograd;
3. the four delays change nothing in a captured step: three replays equal each other and the undelayed eager step;
4. five engines built from one seed, three replayed steps with lr > 0 under f32 / bf16: one parameter hash;
5. NaN-filled allocations between fork and join, shaped like everything Part 3 reads, behind a delayed Part 3: a block handed
   back too early would be overwritten before the delayed branch reads it.

All comparisons are torch.equal on the loss and on every named gradient.  No test retries or runs a step more often than stated."""
import hashlib
import math

import pytest
import torch

from tests.helpers import bit_equal_report, named_grads

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 2.0                                    # delay = MARGIN x the undelayed eager step
POINTS = ["fwd-aux", "fwd-cur", "bwd-aux", "bwd-cur"]
PAIRS = [("f32", "f32"), ("bf16", "f32"), ("f32", "bf16"), ("bf16", "bf16")]          # (precision, embedding_precision)
ON = (True, True)                               # (overlap_hetero_passes, overlap_encoders)


# ------------------------------------------------------------------------------------------------ batch, model, engine
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


@pytest.fixture(scope="module", autouse=True)
def _shared_runs():
    """The shared engines and results (`_once`) live as long as this module's tests."""
    yield
    _CACHE.clear()
    torch.cuda.empty_cache()


def _batch():
    """Two graphs of 40 protein and 12 ligand atoms with 30 interaction edges each: Part 3 and Part 4 both launch their GEMMs."""
    def make():
        from singa_amd import graph as G
        b = G.synthetic_batch(2, first_id=80, n_protein=40, e_pp=120, n_ligand=12, e_ll=24, e_x=30).to(DEV)
        assert set(b.extras["rot_rand"]) == {"pp", "ll", "lp"}                 # the edge-frame draws travel with the batch
        assert b[G.E_LP]["edge_index"].shape[1] >= 32 and b[G.E_PL]["edge_index"].shape[1] >= 32
        return b
    return _once("batch", make)


def _model(pair=PAIRS[0], overlap=ON, seed=5):
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    torch.manual_seed(seed)
    model = SINGA(load_config(lmax=2), device=DEV, precision=pair[0], embedding_precision=pair[1]).eval()
    assert model.embedding.skip_dead_hetero_layers
    model.embedding.overlap_hetero_passes, model.model.overlap_encoders = overlap
    return model


def _engine(model, lr=0.0, **kw):
    """A TrainStep over `model`; lr = 0 freezes the parameters (tests/test_replay_parity_gpu.py)."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    opt = Adam(model.parameters(), lr=1e-4)
    opt.param_groups[0]["lr"] = lr
    return TrainStep(model, opt, None, **kw)


def _step(eng, batch):
    loss = eng.step(batch).detach().clone()
    return loss, named_grads(eng.model)


def _split_step(eng, batch):
    """One eager forward + backward in the engine's split mode (TrainStep._fwd_bwd with two_phase: loss -> transformer and the
    embedding's outputs, flush, embedding outputs -> embedding parameters, flush), without the all-reduce between the phases."""
    eng._prepared(batch)
    eng.opt.zero_grad(set_to_none=True)
    eng._sink_begin()
    try:
        from singa_amd import ops
        assert ops._GradSink.on
        loss, boundary = eng._phase_a(batch, True)
        eng._phase_b(boundary)
    finally:
        eng._sink_end(False)
    return loss.detach().clone(), named_grads(eng.model)


def _same_bits(got, want, label):
    same, n, worst = bit_equal_report(got[1], want[1], label)
    print(f"{label}: loss {float(got[0])!r} vs {float(want[0])!r}")
    differ = [k for k, g in want[1].items() if not torch.equal(got[1][k], g)]
    assert torch.equal(got[0], want[0]), (label, float(got[0]), float(want[0]))
    assert not differ, (label, len(differ), n, worst, differ[:6])


# ------------------------------------------------------------------------------------------------ the delay harness
def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def calibration():
    """{cycles_per_ms, step_ms, delay_ms, cycles}: measured once per session (see the module docstring)."""
    def make():
        torch.cuda._sleep(1000)                                                   # (first launch: module load)
        probe = 2_000_000
        _timed(lambda: torch.cuda._sleep(probe))
        cycles_per_ms = probe / _timed(lambda: torch.cuda._sleep(probe))
        ref = _eager(PAIRS[0], ON)                                                # two steps done: warm
        step_ms = max(_timed(lambda: ref["eng"].step(_batch())) for _ in range(2))
        delay_ms = MARGIN * step_ms
        cal = dict(cycles_per_ms=cycles_per_ms, step_ms=step_ms, delay_ms=delay_ms, cycles=int(delay_ms * cycles_per_ms))
        print(f"calibration: {cycles_per_ms:.0f} _sleep cycles per ms; undelayed eager step {step_ms:.1f} ms; "
              f"delay {MARGIN} x step = {delay_ms:.1f} ms = {cal['cycles']} cycles")
        assert cal["cycles"] > 0 and math.isfinite(delay_ms)
        return cal
    return _once("calibration", make)


def _on_second_stream():
    """Is the current stream the models' second stream?  (Read from the table: asking `ops.branch_stream()` on that stream
    would have it replaced.)"""
    from singa_amd import ops
    return any(torch.cuda.current_stream() == s for s in ops._branch_streams.values())


class _Hold(torch.autograd.Function):
    """Identity whose backward enqueues the delay on the stream autograd runs it on: the stream of its forward."""

    @staticmethod
    def forward(ctx, x, inj):
        ctx.inj = inj
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        ctx.inj.sleep()
        return g, None


def _float_tensors(obj, out, depth=0):
    """Every floating-point tensor reachable from `obj` through containers, SO3_Embedding-like holders and closures."""
    if torch.is_tensor(obj):
        if obj.is_floating_point() and obj.is_cuda:
            out.append(obj)
    elif depth > 4:
        return
    elif isinstance(obj, dict):
        for v in obj.values():
            _float_tensors(v, out, depth + 1)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _float_tensors(v, out, depth + 1)
    elif hasattr(obj, "embedding") and torch.is_tensor(getattr(obj, "embedding")):
        out.append(obj.embedding)
    elif callable(obj) and getattr(obj, "__closure__", None):
        for cell in obj.__closure__:
            _float_tensors(cell.cell_contents, out, depth + 1)


class inject:
    """Context manager: one delay point (or none) patched into `model`'s two forks.  poison=True: between fork and join of the
    embedding (from the fwd-cur hook, before and after Part 4 enqueues its work) the current stream allocates one NaN-filled
    tensor per floating-point tensor Part 3 reads - the closure `_hetero_pass(deferred=True)` returned and all it captured,
    the shared dict's embeddings, the Wigner tables - with the shapes found at the call.  `.fired`: (point, on the second stream?)
    per enqueued delay."""

    def __init__(self, model, point=None, cycles=0, poison=False):
        assert point is None or point in POINTS + ["bwd-tail"]           # (bwd-tail: placed by a launch_log, not here)
        self.model, self.point, self.cycles, self.poison = model, point, int(cycles), poison
        self.fired, self.poisoned, self.keep = [], 0, []

    def sleep(self):
        torch.cuda._sleep(self.cycles)
        self.fired.append((self.point, _on_second_stream()))

    def _poison(self, shapes):
        for shape, dtype in shapes:
            self.keep.append(torch.full(shape, float("nan"), device=DEV, dtype=dtype))
        self.poisoned += len(shapes)

    def __enter__(self):
        from singa_amd import ops
        emb, tr, point = self.model.embedding, self.model.model, self.point
        self._branch, hetero_pass, enc1, enc2 = ops.branch_stream, emb._hetero_pass, tr.encoder.forward, tr.encoder2.forward
        self._undo = [(ops, "branch_stream", None), (emb, "_hetero_pass", "del"), (tr.encoder, "forward", "del"),
                      (tr.encoder2, "forward", "del")]
        reads = []

        def branch_stream(device=None):
            s = self._branch(device)
            if point == "fwd-aux":
                with torch.cuda.stream(s):
                    self.sleep()
            return s

        def hetero(g, x_dict, *a, deferred=False, **kw):
            if deferred:                                              # Part 3: everything that changes the dict, and a closure
                compute = hetero_pass(g, x_dict, *a, deferred=True, **kw)
                if self.poison:
                    found = []
                    _float_tensors([compute, x_dict, vars(emb.SO3_rotation[0])], found)
                    reads[:] = [(tuple(t.shape), t.dtype) for t in found]
                if point != "bwd-aux":
                    return compute

                def held():                                           # (called under the second stream)
                    x = compute()
                    x.embedding = _Hold.apply(x.embedding, self)
                    return x
                return held
            forked = emb.overlap_hetero_passes                        # Part 4, between fork and join
            if forked and point == "fwd-cur":
                self.sleep()
            if forked and self.poison:
                self._poison(reads)
            x = hetero_pass(g, x_dict, *a, **kw)
            if forked and self.poison:
                self._poison(reads)
            if forked and point == "bwd-cur":
                x.embedding = _Hold.apply(x.embedding, self)
            return x

        def encoder(*a, **kw):
            if tr.overlap_encoders and point == "fwd-cur":
                self.sleep()
            out = enc1(*a, **kw)
            if tr.overlap_encoders and point == "bwd-cur":
                out = (_Hold.apply(out[0], self),) + tuple(out[1:])
            return out

        def encoder2(*a, **kw):                                       # (called under the second stream when forked)
            out = enc2(*a, **kw)
            if tr.overlap_encoders and point == "bwd-aux":
                out = (_Hold.apply(out[0], self),) + tuple(out[1:])
            return out

        ops.branch_stream = branch_stream
        emb._hetero_pass, tr.encoder.forward, tr.encoder2.forward = hetero, encoder, encoder2
        return self

    def __exit__(self, *exc):
        from singa_amd import ops
        ops.branch_stream = self._branch
        for obj, name, how in self._undo[1:]:
            delattr(obj, name)                                        # the instance attribute: the class's method is back
        self.keep.clear()
        return False

    def check(self, steps):
        """Both forks were held back in each of `steps` passes, on the stream the point names."""
        if self.point is not None:
            assert self.fired == [(self.point, self.point.endswith("aux"))] * (2 * steps), self.fired


class launch_log:
    """Context manager around `ops._stream`, which every launch of the library asks for its stream right before it is
    enqueued: `.aux[i]` tells whether launch i of the backward pass(es) went to the second stream.  sleep_at: launch numbers
    in front of which `inj` enqueues its delay (they must be second-stream launches)."""

    def __init__(self, sleep_at=(), inj=None):
        self.sleep_at, self.inj, self.aux = set(sleep_at), inj, []

    def __enter__(self):
        from singa_amd import ops
        self._orig = ops._stream

        def _stream():
            if torch._C._current_graph_task_id() != -1:              # inside a backward pass
                on_aux = _on_second_stream()
                if len(self.aux) in self.sleep_at:
                    assert on_aux
                    self.inj.sleep()
                self.aux.append(on_aux)
            return self._orig()

        ops._stream = _stream
        return self

    def __exit__(self, *exc):
        from singa_amd import ops
        ops._stream = self._orig
        return False

    def groups(self):
        """[(first, last)] of every run of consecutive second-stream launches."""
        out, start = [], None
        for i, a in enumerate(self.aux + [False]):
            if a and start is None:
                start = i
            elif not a and start is not None:
                out.append((start, i - 1))
                start = None
        return out


# ------------------------------------------------------------------------------------------------ shared eager runs
def _eager(pair, overlap):
    """One eager engine per (precision pair, overlap setting) with frozen parameters and its first two steps: `off` - the
    gradient sink is off in an engine's first step (it records which parameters take part; a plain backward()) - and `on`,
    the second step (`ops._GradSink` on, as inside a capture).  Later steps of the same engine (delayed ones) see the same
    parameters: lr = 0."""
    def make():
        eng = _engine(_model(pair, overlap), use_graph=False)
        off = _step(eng, _batch())
        assert eng._sink_params
        on = _step(eng, _batch())
        return dict(eng=eng, off=off, on=on)
    return _once(("eager", pair, overlap), make)


def _delayed(pair, point, step=_step, batch=None, poison=False):
    ref = _eager(pair, ON)
    with inject(ref["eng"].model, point, calibration()["cycles"] if point else 0, poison) as inj:
        got = step(ref["eng"], _batch() if batch is None else batch)
    inj.check(1)
    return got, inj


def _staged():
    """The test batch padded to its size class, as a bucketed engine replays it."""
    def make():
        eng = _engine(_eager(PAIRS[0], ON)["eng"].model, use_graph=True, bucket=True)
        return eng._stage(_batch())
    return _once("staged", make)


def _eager_padded(pair):
    return _once(("padded", pair), lambda: _step(_eager(pair, ON)["eng"], _staged()))


# ------------------------------------------------------------------------------------------------ 0: the harness can fail
def _toy(wait, cycles):
    """Writes a tensor on the models' second stream behind the delay, reads it on the current one."""
    from singa_amd import ops
    cur, aux = torch.cuda.current_stream(), ops.branch_stream()
    buf = torch.zeros(1 << 16, device=DEV)
    torch.cuda.synchronize()
    aux.wait_stream(cur)
    with torch.cuda.stream(aux):
        torch.cuda._sleep(cycles)
        buf.fill_(1.0)
    if wait:
        cur.wait_stream(aux)
    out = buf.clone()
    torch.cuda.synchronize()
    return out


def test_delay_exposes_a_missing_wait():
    """Without its wait_stream the toy returns the STALE zeros (every one of them: the delayed fill has not begun when the
    read runs), with it the ones.  Wrong data, not a fault.  If this fails the delay is too short - or the second stream does
    not run beside the current one - and the tests below prove nothing."""
    cal = calibration()
    stale, fresh = _toy(False, cal["cycles"]), _toy(True, cal["cycles"])
    print(f"unsynchronised read: {int((stale == 0).sum())} of {stale.numel()} stale; synchronised: {int((fresh == 1).sum())} new")
    assert bool((stale == 0).all())
    assert bool((fresh == 1).all())


def test_branch_stream_is_never_the_current_stream():
    """torch hands streams out of a pool of 32, round robin, so the stream of a capture or of a warm-up made long after the
    models' second stream can be that very stream (seen in a whole-suite process); the fork then ran on ONE stream and the
    capture recorded one branch.  `ops.branch_stream` replaces a second stream that is the current one."""
    from singa_amd import ops
    first = ops.branch_stream()
    assert first != torch.cuda.current_stream()
    with torch.cuda.stream(first):
        second = ops.branch_stream()
        assert second != first and second != torch.cuda.current_stream()
    assert ops.branch_stream() == second


# ------------------------------------------------------------------------------------------------ 1: fork against no fork
@pytest.mark.parametrize("sink", ["off", "on"])
@pytest.mark.parametrize("overlap", [(True, False), (False, True), (True, True)], ids=["hetero", "encoders", "both"])
@pytest.mark.parametrize("pair", PAIRS, ids=["/".join(p) for p in PAIRS])
def test_fork_equals_one_stream(pair, overlap, sink):
    want, got = _eager(pair, (False, False))[sink], _eager(pair, overlap)[sink]
    assert len(want[1]) == 634
    _same_bits(got, want, f"{'/'.join(pair)} overlap {overlap} sink {sink} vs one stream")


# ------------------------------------------------------------------------------------------------ 2: delays, eager
@pytest.mark.parametrize("mode", ["one_backward", "two_phase"])
@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[2]], ids=["f32/f32", "f32/bf16"])
def test_delay_changes_nothing_eager(pair, point, mode):
    if mode == "one_backward":
        want = _eager(pair, ON)["on"]
        got, _ = _delayed(pair, point)
    else:
        want = _once(("split", pair), lambda: _split_step(_eager(pair, ON)["eng"], _batch()))
        got, _ = _delayed(pair, point, step=_split_step)
    _same_bits(got, want, f"{'/'.join(pair)} {mode} {point} vs undelayed")


TAIL = [1, 2, 3, 4, 6, 8, 12, 16]


def _logged(pair, mode):
    """The undelayed step of `mode` under a launch_log -> (result, log)."""
    def make():
        with launch_log() as log:
            got = (_split_step if mode == "two_phase" else _step)(_eager(pair, ON)["eng"], _batch())
        return got, log
    return _once(("logged", pair, mode), make)


@pytest.mark.parametrize("back", TAIL)
@pytest.mark.parametrize("mode", ["one_backward", "two_phase"])
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[2]], ids=["f32/f32", "f32/bf16"])
def test_delay_in_the_tail_of_a_backward_branch_changes_nothing(pair, mode, back):
    """bwd-aux holds back the HEAD of the second stream's backward branch; the stream is a queue, so every node of the branch
    that hands a gradient to a node of the current stream orders all launches in front of it too.  What `_GradSink.flush()`
    could overtake is the TAIL: launches behind the branch's last such hand-over, of nodes that return nothing to autograd
    (parameter gradients taken by the sink, `_BlockWeight.backward`'s in-place add).  The backward pass's launches are logged
    in an undelayed step; then the delay goes in front of the `back`-th launch from the end of every run of consecutive
    second-stream launches (the ligand encoder's backward, Part 3's): wherever the last hand-over lies among the last 16
    launches, one of the cases holds back everything behind it and nothing in front of it."""
    want, dry = _logged(pair, mode)
    groups = dry.groups()
    print(f"{len(dry.aux)} launches in the backward pass, second-stream runs (first, last): {groups}")
    assert 2 <= len(groups) <= 16, groups
    at = sorted({max(first, last - (back - 1)) for first, last in groups})
    eng = _eager(pair, ON)["eng"]
    inj = inject(eng.model, "bwd-tail", calibration()["cycles"])
    with inj, launch_log(at, inj) as log:
        got = (_split_step if mode == "two_phase" else _step)(eng, _batch())
    assert log.aux == dry.aux
    assert inj.fired == [("bwd-tail", True)] * len(at), inj.fired
    _same_bits(got, want, f"{'/'.join(pair)} {mode} delay {back} launches from the end of {len(groups)} runs vs undelayed")
    if mode == "one_backward":
        _same_bits(want, _eager(pair, ON)["on"], "the logged step vs the plain one")


# ------------------------------------------------------------------------------------------------ 3: delays, captured
@pytest.mark.parametrize("point", POINTS)
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[2]], ids=["f32/f32", "f32/bf16"])
def test_delay_changes_nothing_captured(pair, point):
    want = _eager_padded(pair)
    model = _model(pair, ON)
    eng = _engine(model, use_graph=True, bucket=True)
    try:
        with inject(model, point, calibration()["cycles"]) as inj:
            runs = [_step(eng, _batch()) for _ in range(3)]
        inj.check(3)                                     # two warm-up passes and the captured one: the replays run the recording
        assert eng.captures == 1
        assert eng._stage(_batch()).extras["pad"]["sig"] == _staged().extras["pad"]["sig"]
    finally:
        eng.release()
    for i, got in enumerate(runs[1:], 2):
        _same_bits(got, runs[0], f"{'/'.join(pair)} {point}: replay {i} vs replay 1")
    _same_bits(runs[0], want, f"{'/'.join(pair)} {point}: replay vs undelayed eager step")


# ------------------------------------------------------------------------------------------------ 4: repeat from a seed
def test_replayed_run_repeats_from_its_seed():
    """The small-shape form of profiles/bf16_embed/determinism.txt: f32 / bf16, both forks on, lr > 0."""
    hashes = []
    for _ in range(5):
        model = _model(PAIRS[2], ON, seed=11)
        eng = _engine(model, lr=1e-4, use_graph=True, bucket=True)
        try:
            losses = [float(eng.step(_batch()).detach()) for _ in range(3)]
            torch.cuda.synchronize()
            h = hashlib.sha256()
            for _, p in model.named_parameters():
                h.update(p.detach().cpu().numpy().tobytes())
            hashes.append((h.hexdigest()[:16], losses))
        finally:
            eng.release()
    print(hashes)
    assert len(set(losses[0] for _, losses in hashes)) == 1 and hashes[0][1][0] != hashes[0][1][2]     # (the steps moved it)
    assert len(set(h for h, _ in hashes)) == 1, hashes


# ------------------------------------------------------------------------------------------------ 5: allocator reuse
@pytest.mark.parametrize("pair", [PAIRS[0], PAIRS[2]], ids=["f32/f32", "f32/bf16"])
def test_crossing_tensors_survive_allocator_reuse(pair):
    got, inj = _delayed(pair, "fwd-aux", poison=True)
    print(f"{inj.poisoned} NaN-filled allocations between fork and join")
    assert inj.poisoned >= 8
    _same_bits(got, _eager(pair, ON)["on"], f"{'/'.join(pair)} fwd-aux + NaN allocations vs undelayed")
