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

        def fwd(ctx, x, w1, b1, w2, b2):
            y = orig(ctx, x, w1, b1, w2, b2)
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

    def __init__(self, L):
        z = golden(f"singa_L{L}_B3_relu_ties.npz")
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
