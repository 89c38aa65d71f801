"""Shared test helpers (CPU side): golden loading + synthetic weights."""
import os

import numpy as np
import torch

from oracle import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NAMES = ["3wi2_4tpp", "4agq_5a7b", "5cp5_4nue"]


def state_from_spec(tag):
    z = np.load(os.path.join(GOLDEN, f"param_spec_{tag}.npz"))
    spec = [(str(n), tuple(int(v) for v in str(s).split(",")) if str(s) else (), float(m), float(sd))
            for n, s, m, sd in zip(z["names"], z["shapes"], z["mean"], z["std"])]
    return W.synth_state(spec)


def golden(name):
    return np.load(os.path.join(GOLDEN, name))


def rel_err(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).norm() / (b.norm() + 1e-30))


def rowwise_err(got, want, report=None):
    """max over rows r of |got_r - want_r| / max(|want_r|, median_r |want_r|), both as float64 on the CPU, reshaped to
    [rows, -1] (rows = the leading axis: edges, nodes, decoder rows, parameter rows; a 1-D tensor is ONE row).  An error
    confined to a few rows is not diluted by the row count as in one global relative norm; the median floor keeps a
    near-zero reference row from deciding the test.  `report`: a label - prints the value and the row it was found in."""
    got = torch.as_tensor(got).detach().cpu().double()
    want = torch.as_tensor(want).detach().cpu().double()
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    if want.numel() == 0:
        return 0.0
    rows = want.shape[0] if want.dim() > 1 else 1
    got, want = got.reshape(rows, -1), want.reshape(rows, -1)
    ref = want.norm(dim=1)
    err = (got - want).norm(dim=1) / torch.maximum(ref, ref.median()).clamp_min(1e-300)
    err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))        # NaN / inf in `got`: a failure
    worst = int(err.argmax())
    if report is not None:
        print(f"{report}: rowwise_err {float(err[worst]):.3e} at row {worst} of {rows}")
    return float(err[worst])


def cpu_f64(fn, inputs, grad_outs, wrt=None, device=None):
    """Evaluate `fn` on float64 CPU copies of `inputs` (the CPU reference of a kernel: same formula as the reference's
    torch code, computed away from the GPU) and return (outputs, gradients w.r.t. inputs[wrt]) - as float64 CPU tensors, or
    as float32 tensors on `device`."""
    ins = [t.detach().cpu().double().requires_grad_(True) if (torch.is_tensor(t) and t.is_floating_point()) else
           (t.cpu() if torch.is_tensor(t) else t) for t in inputs]
    outs = fn(*ins)
    single = torch.is_tensor(outs)
    outs_l = [outs] if single else list(outs)
    gos = [g.detach().cpu().double() for g in ([grad_outs] if torch.is_tensor(grad_outs) else grad_outs)]
    idx = range(len(ins)) if wrt is None else wrt
    grads = torch.autograd.grad(outs_l, [ins[i] for i in idx], gos)
    to = (lambda t: t.detach()) if device is None else (lambda t: t.detach().float().to(device))
    return (to(outs) if single else [to(o) for o in outs_l]), [to(g) for g in grads]


def product_batch(names, z=None, device="cuda", with_lap=False):
    """Golden graphs as a singa_amd HeteroGraph batch; `z` (a golden npz) pins rot-mats / kNN lists / lap-PE."""
    import os as _os

    from singa_amd import graph as G
    b = G.collate([G.load_npz(_os.path.join(GOLDEN, f"graph_{n}.npz"), with_lap=with_lap) for n in names])
    if z is not None:
        b.extras["edge_rot_mat"] = {k: torch.tensor(z[f"rot_{k}"]) for k in ("pp", "ll", "lp")}
        if "knn_p" in z.files:
            b.extras["knn"] = {G.PA: torch.tensor(z["knn_p"]), G.LA: torch.tensor(z["knn_l"])}
            b.nodes[G.PA]["lap_pe"], b.nodes[G.LA]["lap_pe"] = torch.tensor(z["lap_p"]), torch.tensor(z["lap_l"])
    return b.to(device)


BEAM_CASES = ["b1_k20", "b2_k4", "b2_k6_eos", "b2_k5_flat"]
SMI_VOC = None


def smi_voc():
    global SMI_VOC
    if SMI_VOC is None:
        import yaml
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        SMI_VOC = list(yaml.safe_load(open(os.path.join(root, "config", "train.yml")))["model"]["decoder"]["smiVoc"])
    return SMI_VOC


def apply_beam_gains(weight, z):
    """The two documented rescalings of the vocabulary projection a beam golden was made with (oracle/make_golden_beam.py)."""
    with torch.no_grad():
        weight.mul_(float(z["proj_gain"]))
        weight[smi_voc().index("$")] *= float(z["eos_gain"])


def grad_sample_errors(named_grads, z, tol):
    """Compare the element-wise gradient samples of a singa_L*_B3 golden (up to 512 evenly spaced elements of every
    parameter's gradient, oracle/make_golden.py) with `named_grads` = {name: grad or None}.  Returns the list of
    parameters whose samples differ by more than `tol` relative (L2 over the parameter's samples)."""
    bad, off = [], 0
    flat = z["grad_samples"]
    for n, ref in zip(z["grad_names"], z["grad_norms"]):
        if ref < 0:
            continue
        gr = named_grads[str(n)]
        idx = W.sample_index(gr.numel())
        want = torch.as_tensor(flat[off:off + len(idx)], dtype=torch.float64)
        off += len(idx)
        got = gr.detach().reshape(-1).cpu()[torch.as_tensor(idx)].double()
        err = float((got - want).norm() / (want.norm() + 1e-12))
        if err > tol and float((got - want).abs().max()) > 1e-7:
            bad.append((str(n), err))
    assert off == len(flat), (off, len(flat))
    return bad


def named_grads(model):
    """{name: clone of .grad} of every parameter that has one, after a device synchronisation.  Clones: under a bucketed
    TrainStep `.grad` lives in a capture's memory pool, and the next replay overwrites it."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def grad_mismatches(got, want, rel=2e-4):
    """The per-parameter criterion of tests/test_padding_gpu.py on two {name: tensor} sets:
    |got - want| <= rel * |want| + (rel / 2e-4) * 1e-7 * |all of want| (2-norms, formed in float64; the floor is for the
    mathematically zero gradients of the dense attentions' key biases, which are rounding noise on both sides).  Both sides must
    hold the same names.  Returns [(name, relative error)] of the parameters that break it."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    total = float(torch.sqrt(sum((w.double() ** 2).sum() for w in want.values())))
    bad = []
    for n, w in want.items():
        w = w.double()
        d = float((got[n].double().to(w.device) - w).norm())
        if not d <= rel * float(w.norm()) + (rel / 2e-4) * 1e-7 * total:
            bad.append((n, d / (float(w.norm()) + 1e-300)))
    return bad


def bit_equal_report(got, want, label=None):
    """(number of parameters whose tensors are torch.equal, number of parameters, largest |got - want| / |want| among the
    rest that carry a gradient: norm above 1e-7 of the total) of two {name: tensor} sets with the same names; `label`:
    prints the three."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    total = float(torch.sqrt(sum((w.double() ** 2).sum() for w in want.values())))
    same, worst = 0, 0.0
    for n, w in want.items():
        if torch.equal(got[n], w):
            same += 1
        elif float(w.double().norm()) > 1e-7 * total:
            worst = max(worst, float((got[n].double() - w.double()).norm() / w.double().norm()))
    if label is not None:
        print(f"{label}: {same} of {len(want)} parameters bit-equal, largest relative difference {worst:.3e}")
    return same, len(want), worst


class pinned_relu_ties:
    """Context manager for the golden SINGA step: pins every PoswiseFeedForward ReLU gate whose pre-activation the REFERENCE
    saw within 1e-4 of its layer's scale from zero to the reference's recorded choice
    (tests/golden/singa_L<L>_B3_relu_ties.npz, written by oracle/make_relu_ties.py; ~800 of 10.5 M gates).  Such a
    pre-activation is positive or negative depending on the summation order of the GEMM in front of it, the gate is a step
    function, and ONE differing gate moves some parameter gradients by ~5e-3 (measured, tools/lab/xf_trace.py: 3 gates
    differed between two builds whose embedding outputs agreed to 2.6e-7, and the protein-side input gradient of the
    transformer moved by 1e-3) - which side the reference took is a property of its run.  Only the saved activation the
    backward mask reads is touched (0 <-> 1e-30), and only in the test: the forward result is the product's own.
    `.flipped` counts the gates where the product had decided the other way."""

    def __init__(self, L=None, records=None):
        """L: the golden's fixture; or records = oracle_relu_ties(...).records (HIP vs the CPU oracle on any batch)."""
        z = golden(f"singa_L{L}_B3_relu_ties.npz") if records is None else records
        self.layer = torch.as_tensor(z["layer"]).long()
        self.flat = torch.as_tensor(z["row"]).long() * 1024 + torch.as_tensor(z["unit"]).long()
        self.on = torch.as_tensor(z["on"])
        self.rows = [int(r) for r in z["rows"]]
        self.call = self.flipped = 0

    def __enter__(self):
        from singa_amd import ops
        self._orig = ops._PosFFN.forward
        orig = self._orig

        def fwd(ctx, *args):
            y = orig(ctx, *args)
            h = ctx.to_save[3]
            assert self.call < len(self.rows) and tuple(h.shape) == (self.rows[self.call], 1024), (self.call, h.shape)
            sel = self.layer == self.call
            idx, want = self.flat[sel].to(h.device), self.on[sel].to(h.device)
            cur = h.view(-1)[idx]
            self.flipped += int(((cur > 0) != want).sum())
            h.view(-1)[idx] = torch.where(want, cur.clamp_min(1e-30), torch.zeros_like(cur))
            self.call += 1
            return y

        ops._PosFFN.forward = staticmethod(fwd)
        return self

    def __exit__(self, *exc):
        from singa_amd import ops
        ops._PosFFN.forward = staticmethod(self._orig)
        return False


class relu_gate_log:
    """Context manager: records the ReLU gates (saved activation > 0, [rows, 1024] bool) of every PoswiseFeedForward call, in
    call order, in `.masks`.  capturing=True records only the calls made under HIP-graph capture: those masks are part of the
    captured graph (one compare kernel per call, the step's own numbers are untouched), live in its memory pool and are
    rewritten by every replay - `take()` copies the last pass's 18 out after a step."""

    def __init__(self, capturing=False):
        self.capturing, self.masks = capturing, []

    def __enter__(self):
        from singa_amd import ops
        self._orig = ops._PosFFN.forward
        orig = self._orig

        def fwd(ctx, *args):
            y = orig(ctx, *args)
            if torch.cuda.is_current_stream_capturing() == self.capturing:
                self.masks.append(ctx.to_save[3] > 0)
            return y

        ops._PosFFN.forward = staticmethod(fwd)
        return self

    def __exit__(self, *exc):
        from singa_amd import ops
        ops._PosFFN.forward = staticmethod(self._orig)
        return False

    def take(self, calls=18):
        torch.cuda.synchronize()
        assert len(self.masks) >= calls and len(self.masks) % calls == 0, len(self.masks)
        return [m.clone() for m in self.masks[-calls:]]


def relu_gate_flips(ref_masks, run_masks):
    """The gates two runs of the SAME code on the same batch decided differently (`relu_gate_log` masks; the run's batch may
    carry padding atoms behind the reference's rows), as `pinned_relu_ties(records=...)` takes them: pinned to the run's
    choice.  Two such runs differ by rounding only, so a gate flips only where its pre-activation is within rounding of zero
    - the tie of DESIGN section 2, "ReLU ties" - and ONE flipped gate moves its unit's row of conv1's gradient by a finite
    amount whichever side is right."""
    assert len(ref_masks) == len(run_masks)
    layer, row, unit, on = [], [], [], []
    for i, (e, r) in enumerate(zip(ref_masks, run_masks)):
        assert r.shape[0] >= e.shape[0] and r.shape[1] == e.shape[1] == 1024
        r = r[:e.shape[0]]
        idx = (e != r).nonzero()
        layer.append(torch.full((idx.shape[0],), i))
        row.append(idx[:, 0].cpu())
        unit.append(idx[:, 1].cpu())
        on.append(r[idx[:, 0], idx[:, 1]].cpu())
    return {"layer": torch.cat(layer), "row": torch.cat(row), "unit": torch.cat(unit), "on": torch.cat(on),
            "rows": [int(e.shape[0]) for e in ref_masks]}


class oracle_relu_ties:
    """Context manager around a run of the CPU oracle: records, for every PoswiseFeedForward call (oracle.pos_ffn, CP:170-191),
    the ReLU gates whose pre-activation lies within `window` of the call's scale from zero, with the oracle's choice - the
    same record oracle/make_relu_ties.py takes from the reference for the goldens; `.records` feeds pinned_relu_ties."""

    def __init__(self, window=1e-4):
        self.window, self.calls = window, []

    def __enter__(self):
        import oracle.singa_oracle as O
        self._O, self._orig = O, O.pos_ffn

        def pos_ffn(sd, p, x):
            with torch.no_grad():
                pre = torch.nn.functional.linear(x.detach(), sd[p + ".conv1.weight"].detach()[:, :, 0],
                                                 sd[p + ".conv1.bias"].detach()).reshape(-1, 1024)
                near = (pre.abs() < self.window * pre.pow(2).mean().sqrt()).nonzero()
                self.calls.append((pre.shape[0], near[:, 0], near[:, 1], pre[near[:, 0], near[:, 1]] > 0))
            return self._orig(sd, p, x)

        O.pos_ffn = pos_ffn
        return self

    def __exit__(self, *exc):
        self._O.pos_ffn = self._orig
        return False

    @property
    def records(self):
        return {"layer": torch.cat([torch.full((len(c[1]),), i) for i, c in enumerate(self.calls)]),
                "row": torch.cat([c[1] for c in self.calls]), "unit": torch.cat([c[2] for c in self.calls]),
                "on": torch.cat([c[3] for c in self.calls]), "rows": [c[0] for c in self.calls]}


class _ReluPinned(torch.autograd.Function):
    """relu whose backward mask is overridden at given flat positions (test-only: the reference's choice at fp32 ties)."""

    @staticmethod
    def forward(ctx, pre, idx, on):
        mask = pre > 0
        mask.view(-1)[idx] = on
        ctx.save_for_backward(mask)
        return pre.clamp_min(0)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


class oracle_pinned_relu_ties:
    """pinned_relu_ties for the CPU ORACLE (oracle.pos_ffn): the backward mask of the recorded near-zero gates follows the
    reference's run.  `.flipped` counts the gates where the oracle had decided the other way."""

    def __init__(self, L=None, records=None):
        """L: the golden's fixture; or records = relu_gate_flips(...) of two oracle runs (tests/symmetry.py)."""
        z = golden(f"singa_L{L}_B3_relu_ties.npz") if records is None else records
        self.layer = torch.as_tensor(z["layer"]).long()
        self.flat = torch.as_tensor(z["row"]).long() * 1024 + torch.as_tensor(z["unit"]).long()
        self.on = torch.as_tensor(z["on"])
        self.rows = [int(r) for r in z["rows"]]
        self.call = self.flipped = 0

    def __enter__(self):
        import oracle.singa_oracle as O
        self._O, self._orig = O, O.pos_ffn
        F = torch.nn.functional

        def pos_ffn(sd, p, x):
            pre = F.linear(x, sd[p + ".conv1.weight"][:, :, 0], sd[p + ".conv1.bias"])
            flat = pre.reshape(-1, 1024)
            assert flat.shape[0] == self.rows[self.call], (self.call, flat.shape)
            sel = self.layer == self.call
            idx, on = self.flat[sel], self.on[sel]
            self.flipped += int(((flat.detach().reshape(-1)[idx] > 0) != on).sum())
            self.call += 1
            h = _ReluPinned.apply(flat, idx, on).view_as(pre)
            return O.layer_norm(sd, p + ".layer_norm", F.linear(h, sd[p + ".conv2.weight"][:, :, 0], sd[p + ".conv2.bias"]) + x)

        O.pos_ffn = pos_ffn
        return self

    def __exit__(self, *exc):
        self._O.pos_ffn = self._orig
        return False


# ------------------------------------------------------------------------------------------ write footprints of C ABI calls
# The C ABI (include/singa_hip.h) works on caller-owned, possibly strided views.  An Arena carves all views of ONE call out of
# one allocation, with poisoned guard bands around every view and poison in every gap of a strided view, so that a stray
# write lands in memory of our own where it can be seen, a stray read that feeds a result shows up in the result, and nothing
# faults.  Two canaries (two runs of the same call) tell "never written" from "written with the old value".
ARENA_GUARD = 4096                                     # elements before and behind every view (16 KB of floats)
_INT_VIEW = {torch.float32: torch.int32, torch.float64: torch.int64, torch.int32: torch.int32, torch.int64: torch.int64,
             torch.uint8: torch.uint8}
# bit patterns, as the integer type of the same width
_CANARY = {"nan": {torch.float32: 0x7FC0BEEF, torch.float64: 0x7FF8DEADBEEFCAFE},          # quiet NaNs with a payload
           "big": {torch.float32: 0x7149F2CA, torch.float64: 0x7E37E43C8800759C}}          # 1e30, 1e300
_CANARY_INT = {torch.int32: -0x7452F00D, torch.int64: -0x7452F00D7452F00D, torch.uint8: 0xA5}   # outside any valid index / flag


class ArenaView:
    """One view of an Arena: `.t` is the strided tensor handed to the call, `.ptr` its address."""

    def __init__(self, name, region, t, promised, role, snap):
        self.name, self.region, self.t, self.promised, self.role, self.snap = name, region, t, promised, role, snap

    @property
    def ptr(self):
        return self.t.data_ptr()


class Arena:
    """canary: "nan" or "big" (floating-point poison; integer buffers use one out-of-range pattern in both).

    view(name, shape, ...) places a view and returns its ArenaView; roles:
      "in"      read-only input, filled with `data`; its gaps and guards are poison, and it must come back unchanged;
      "out"     every element (or every element of `promised`, a bool mask of the view's shape) must be written; the rest of the
                view, its gaps and its guards must keep their bits;
      "inout"   starts from `data` (accumulators, caches); compared by the caller against `initial (op) result`;
      "scratch" memory the header calls uninitialised: poisoned, may be written anywhere inside the view.
    report() -> ArenaReport after the call has finished."""

    def __init__(self, device, canary, capacity=64 << 20, guard=ARENA_GUARD):
        assert canary in _CANARY
        self.device, self.canary, self.guard = torch.device(device), canary, guard
        self.buf = torch.empty(capacity, dtype=torch.uint8, device=self.device)          # the ONE allocation
        self.top, self.views = 0, {}

    def poison(self, dtype):
        return _CANARY[self.canary][dtype] if dtype.is_floating_point else _CANARY_INT[dtype]

    def view(self, name, shape, dtype=torch.float32, strides=None, data=None, role="in", promised=None):
        assert name not in self.views and role in ("in", "out", "inout", "scratch")
        shape = tuple(int(s) for s in shape)
        if strides is None:
            strides, acc = [], 1
            for s in reversed(shape):
                strides.insert(0, acc)
                acc *= max(s, 1)
        strides = tuple(int(s) for s in strides)
        numel = int(np.prod(shape)) if shape else 1
        span = 1 + sum((s - 1) * st for s, st in zip(shape, strides)) if numel else 0
        item = torch.empty(0, dtype=dtype).element_size()
        n = span + 2 * self.guard
        start = -(-self.top // 256) * 256
        assert start + n * item <= self.buf.numel(), "arena capacity"
        self.top = start + n * item
        region = self.buf[start:start + n * item].view(dtype)
        bits = region.view(_INT_VIEW[dtype])
        bits.fill_(self.poison(dtype))
        t = region.as_strided(shape, strides, region.storage_offset() + self.guard)
        idx = torch.arange(n, device=self.device).as_strided(shape, strides, self.guard)
        assert idx.unique().numel() == numel, "overlapping strides"
        if role == "in" or role == "inout":
            assert data is not None
            t.copy_(torch.as_tensor(data).to(device=self.device, dtype=dtype).reshape(shape))
        mask = torch.zeros(n, dtype=torch.bool, device=self.device)
        if role == "scratch":
            mask[self.guard:self.guard + span] = True
        elif promised is None:
            mask[idx.reshape(-1)] = True
        else:
            mask[idx[torch.as_tensor(promised, device=self.device).expand(shape)]] = True
        v = ArenaView(name, region, t, mask, role, bits.clone())
        self.views[name] = v
        return v

    def report(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize()
        rep = ArenaReport()
        for name, v in self.views.items():
            bits = v.region.view(_INT_VIEW[v.region.dtype])
            changed = bits != v.snap
            stray = int((changed & ~v.promised).sum())
            if stray:
                where = int((changed & ~v.promised).nonzero()[0]) - self.guard
                rep.stray[name] = (stray, where)                    # words outside the promise whose bits changed, first offset
            if v.role == "in" and int((changed & v.promised).sum()):
                rep.stray[name] = (int(changed.sum()), "input modified")
            if v.role == "out":
                left = int(((bits == self.poison(v.region.dtype)) & v.promised).sum())
                if left:
                    rep.unwritten[name] = left
            if v.role in ("out", "inout"):
                rep.bits[name] = bits[v.promised].cpu()
                rep.out[name] = v.t.detach().clone().cpu()
        return rep


class ArenaReport:
    def __init__(self):
        self.stray, self.unwritten, self.bits, self.out = {}, {}, {}, {}


def arena_runs(case, device, **kw):
    """Run `case(arena)` (which places its views and makes the call) once per canary -> (report_nan, report_big, names of the
    outputs whose promised elements are not bit-identical between the two runs, what `case` returned in the first run)."""
    reps, ret = [], None
    for canary in ("nan", "big"):
        ar = Arena(device, canary, **kw)
        r = case(ar)
        ret = r if ret is None else ret
        reps.append(ar.report())
    differ = [n for n in reps[0].bits if not torch.equal(reps[0].bits[n], reps[1].bits[n])]
    return reps[0], reps[1], differ, ret


# The clauses of singa_s2act_sep_fwd's pairing rule (two channels per thread where gate, every segment and `out` start 8-byte
# aligned and every pitch is even), defeated one at a time; "paired" satisfies all of them.
S2_LANE_LAYOUTS = ("paired", "gate + 1", "ldg odd", "segment + 1", "segment pitch odd", "out + 1")


def s2_lane_layout(name, rows, C, E, alloc):
    """The operands of one singa_s2act_sep_fwd call laid out as `name` (one of S2_LANE_LAYOUTS) asks, each in a NaN-filled buffer of
    its own.  alloc(n) -> (flat float32 buffer of n NaNs - numpy or torch -, its address, 8-byte aligned).  -> dict: `gate`
    [E, C] and `x` (one [E, r * C] view per segment) to fill; `out` [E, KIN * C] to read, `margins` (the floats in front of and
    behind it); `items` for _capi.segs, `gate_ptr`, `ldg`, `out_ptr`."""
    assert name in S2_LANE_LAYOUTS
    last, kc = len(rows) - 1, sum(rows) * C

    def block(width, off, ld, tail=0):
        buf, addr = alloc(off + E * ld + tail)
        assert addr % 8 == 0
        return buf, buf[off:off + E * ld].reshape(E, ld)[:, :width], addr + 4 * off

    ldg = C + 2 + (name == "ldg odd")
    _, gate, gate_ptr = block(C, 2 + (name == "gate + 1"), ldg)
    lds = [r * C + 2 + (name == "segment pitch odd" and k == last) for k, r in enumerate(rows)]
    segs = [block(r * C, 2 + (name == "segment + 1" and k == last), ld) for k, (r, ld) in enumerate(zip(rows, lds))]
    off = 2 + (name == "out + 1")
    obuf, out, out_ptr = block(kc, off, kc, tail=3)
    return dict(gate=gate, x=[s[1] for s in segs], out=out, margins=(obuf[:off], obuf[off + E * kc:]),
                items=[(s[2], ld, r) for s, ld, r in zip(segs, lds, rows)], gate_ptr=gate_ptr, ldg=ldg, out_ptr=out_ptr)
