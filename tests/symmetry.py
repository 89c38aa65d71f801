"""Transformations under which the step's result is fixed by mathematics alone (test helper, like tests/beam_rule.py).

Every transformation works on the plain array dict of a tests/golden/graph_*.npz fixture - what both
oracle.singa_oracle.load_graph_npz and singa_amd.graph.from_arrays read - and on the uniform draws `rot_rand` of the edge
frames (EF:2301; {'pp','ll','lp'}: [E,3]).  It returns

    (transformed dict, transformed draws, expect)

where `expect` maps the ORIGINAL run's embedding outputs {protein_atoms, ligand_atoms, lp_edge, pl_edge} ([N, K, C]) to what
the transformed run must give.  `in_batch` returns lists of dicts and draws (a batch) and, in place of `expect`, the function
that picks the graph's rows out of the batch's outputs.

A Case ties one transformation to the two runs that are compared: `base` and `run` are (list of dicts, list of draws) - a
list because both runners below take a batch - `expect` acts on base's outputs, `pick` on run's.

Both runners build their frames from the draws: the oracle with oracle.edge_rot_mat, the product through
`extras['rot_rand']`, i.e. with its own frame kernel and Wigner rows - never from a pinned `edge_rot_mat`.
"""
import collections
import os

import numpy as np
import torch

from oracle import singa_oracle as O
from tests.helpers import GOLDEN, golden, rel_err, rowwise_err

PA, LA = O.PA, O.LA
OUTS = (PA, LA, "lp_edge", "pl_edge")
NODE_OF = {PA: "p", LA: "l", "lp_edge": "p", "pl_edge": "l"}          # lp_edge lives on the protein atoms, pl_edge on the ligand's
FRAMES = ("pp", "ll", "lp")                                           # the pl pass reuses the lp frames edge by edge (Q5)
EDGE_ENDS = {"pp": ("p", "p"), "ll": ("l", "l"), "lp": ("l", "p"), "pl": ("p", "l")}
T_EXACT = np.array([128.0, -64.0, 32.0], np.float32)
T_GENERIC = np.array([100.0, -50.0, 25.0], np.float32)
LATTICE = 2.0 ** -10

Case = collections.namedtuple("Case", "name base run expect pick")


def identity(out):
    return out


def load(name):
    """(array dict, draws the reference took) of a bundled graph."""
    z = np.load(os.path.join(GOLDEN, f"graph_{name}.npz"))
    rr = golden(f"rot_rand_{name}.npz")
    return {k: z[k] for k in z.files}, {k: rr[k] for k in FRAMES}


# ------------------------------------------------------------------------------------------------ the transformations
def roll(d, rand, seed=11):
    """New draws: every edge frame is rolled about its edge by another angle."""
    rng = np.random.default_rng(seed)
    return d, {k: rng.random(rand[k].shape).astype(np.float32) for k in FRAMES}, identity


def shuffle_edges(d, rand, seed=12):
    """Every edge list in another order; ei_pl takes ei_lp's permutation (Q5: the goldens have ei_pl == ei_lp.flip(0), and
    the pl pass reuses the lp frames by position); the draws move with their edges."""
    rng = np.random.default_rng(seed)
    perm = {k: rng.permutation(rand[k].shape[0]) for k in FRAMES}
    out = dict(d)
    for k in FRAMES:
        out[f"ei_{k}"] = d[f"ei_{k}"][:, perm[k]]
    out["ei_pl"] = d["ei_pl"][:, perm["lp"]]
    return out, {k: rand[k][perm[k]] for k in FRAMES}, identity


def relabel(d, rand, seed=13):
    """Another numbering of the atoms of each type; edge indices rewritten, edge order (and so the draws) kept."""
    rng = np.random.default_rng(seed)
    order = {s: rng.permutation(d[f"z_{s}"].shape[0]) for s in ("p", "l")}        # new atom i is old atom order[i]
    new_of = {s: np.argsort(order[s]) for s in order}
    out = dict(d)
    for s in ("p", "l"):
        for k in ("x", "pos", "z"):
            out[f"{k}_{s}"] = d[f"{k}_{s}"][order[s]]
    for k, (a, b) in EDGE_ENDS.items():
        out[f"ei_{k}"] = np.stack([new_of[a][d[f"ei_{k}"][0]], new_of[b][d[f"ei_{k}"][1]]])

    def expect(o):
        return {k: v[torch.as_tensor(order[NODE_OF[k]], device=v.device)] for k, v in o.items()}
    expect.order, expect.new_of = order, new_of
    return out, rand, expect


def _moved(d, fn):
    out = dict(d)
    for s in ("p", "l"):
        out[f"pos_{s}"] = fn(d[f"pos_{s}"])
    return out


def snap(d):
    """Positions rounded to multiples of 2^-10: the base of `shift_exact`."""
    return _moved(d, lambda p: (np.round(p.astype(np.float64) / LATTICE) * LATTICE).astype(np.float32))


def shift_exact(d, rand):
    """snap(d) moved by (128, -64, 32): every coordinate stays exactly representable in float32, so every coordinate
    DIFFERENCE of the moved graph has the bits of the unmoved one's."""
    base = snap(d)
    out = _moved(base, lambda p: p + T_EXACT)
    for s in ("p", "l"):
        assert out[f"pos_{s}"].dtype == np.float32
        assert np.array_equal(out[f"pos_{s}"] - T_EXACT, base[f"pos_{s}"])
    return out, rand, identity


def shift(d, rand):
    return _moved(d, lambda p: p + T_GENERIC), rand, identity


def rotation(kind, seed=14):
    """3x3 float64 proper rotation: 'generic' (seeded QR draw, det +1), 'cyclic' ((x,y,z) -> (y,z,x)), 'rz90'."""
    if kind == "generic":
        q, r = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
        q = q * np.sign(np.diag(r))
        if np.linalg.det(q) < 0:
            q[:, 0] = -q[:, 0]
    elif kind == "cyclic":
        q = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    else:
        assert kind == "rz90"
        q = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    assert abs(np.linalg.det(q) - 1.0) < 1e-12 and np.abs(q @ q.T - np.eye(3)).max() < 1e-12
    return q


def wigner(Q, L):
    """[K,K] float64: D with out(Q x) = D out(x) - oracle.wigner_dense(Q) evaluated in float64 (= wigner_dense(Q^T)^T)."""
    return O.wigner_dense(torch.as_tensor(Q, dtype=torch.float64).unsqueeze(0), L)[0]


def rotate(d, rand, Q, L, transposed=False):
    """Positions Q x.  The draws are kept, so the frames of the rotated graph are the rotated frames rolled as well.
    transposed=True pairs the run with D^T: the WRONG convention, for the test that the right one is told apart."""
    D = wigner(Q, L)
    D = D.T.contiguous() if transposed else D

    def expect(o):
        return {k: torch.einsum("ij,njc->nic", D.to(v.device), v.double()) for k, v in o.items()}
    return _moved(d, lambda p: (p.astype(np.float64) @ Q.T).astype(np.float32)), rand, expect


def in_batch(d, rand, other, other_rand, slot):
    """The graph as number `slot` of a batch of two with `other`; returns the batch and the picker of the graph's rows."""
    n = {s: (d[f"z_{s}"].shape[0], other[f"z_{s}"].shape[0]) for s in ("p", "l")}
    dicts, rands = ([d, other], [rand, other_rand]) if slot == 0 else ([other, d], [other_rand, rand])

    def pick(o):
        lo = {s: 0 if slot == 0 else n[s][1] for s in n}
        return {k: v[lo[NODE_OF[k]]:lo[NODE_OF[k]] + n[NODE_OF[k]][0]] for k, v in o.items()}
    return dicts, rands, pick


def embedding_cases(L, name="4agq_5a7b", companion="5cp5_4nue", full=False):
    """The cases of the embedding tests: at every L roll, shuffle_edges, relabel, shift_exact, in_batch (first and second of
    two) and the cyclic rotation; full=True (L = 2) adds the generic shift and the other two rotations."""
    d, r = load(name)
    od, orr = load(companion)
    one = ([d], [r])

    def single(nm, t, base=one):
        return Case(nm, base, ([t[0]], [t[1]]), t[2], identity)
    cases = [single("roll", roll(d, r)), single("shuffle_edges", shuffle_edges(d, r)), single("relabel", relabel(d, r)),
             single("shift_exact", shift_exact(d, r), ([snap(d)], [r]))]
    for slot, nm in ((0, "in_batch_first"), (1, "in_batch_second")):
        ds, rs, pick = in_batch(d, r, od, orr, slot)
        cases.append(Case(nm, one, (ds, rs), identity, pick))
    cases.append(single("rotate_cyclic", rotate(d, r, rotation("cyclic"), L)))
    if full:
        cases += [single("shift", shift(d, r)), single("rotate_generic", rotate(d, r, rotation("generic"), L)),
                  single("rotate_rz90", rotate(d, r, rotation("rz90"), L))]
    return {c.name: c for c in cases}


# ------------------------------------------------------------------------------------------------ defects
def output_defects(got, want):
    """{(output, block, metric): error} of two embedding output dicts, separately for the l = 0 row and the l > 0 rows
    (at L = 2 the norm of the whole output hides an l > 0 defect five times larger), plus the whole output's rel_err."""
    out = {}
    for k in OUTS:
        g, w = got[k].detach().cpu().double(), want[k].detach().cpu().double()
        out[(k, "all", "rel")] = rel_err(g, w)
        for blk, sl in (("l0", slice(0, 1)), ("l>0", slice(1, None))):
            out[(k, blk, "rel")] = rel_err(g[:, sl], w[:, sl])
            out[(k, blk, "row")] = rowwise_err(g[:, sl], w[:, sl])
    return out


def grad_defect(got, want):
    """(largest |got - want| / |want| over the parameters whose gradient is above 1e-7 of the total norm, its name)."""
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:8]
    total = float(torch.sqrt(sum((w.double() ** 2).sum() for w in want.values())))
    worst, name = 0.0, None
    for n, w in want.items():
        if float(w.double().norm()) > 1e-7 * total:
            e = rel_err(got[n].detach().cpu(), w.detach().cpu())
            if not e <= worst:
                worst, name = (e if e == e else float("inf")), n
    return worst, name


# ------------------------------------------------------------------------------------------------ the oracle's side
def _torch_dict(d):
    g = {k: torch.as_tensor(np.asarray(v)) for k, v in d.items()}
    g["props"] = g["props"].to(torch.float64)
    return g


def oracle_inputs(dicts, rands):
    """(collated oracle batch, frames from the draws)."""
    g = O.collate([_torch_dict(d) for d in dicts])
    rnd = {k: torch.cat([torch.as_tensor(np.asarray(r[k])) for r in rands], 0) for k in FRAMES}
    vec = {"pp": g["pos_p"][g["ei_pp"][0]] - g["pos_p"][g["ei_pp"][1]],
           "ll": g["pos_l"][g["ei_ll"][0]] - g["pos_l"][g["ei_ll"][1]],
           "lp": g["pos_l"][g["ei_lp"][0]] - g["pos_p"][g["ei_lp"][1]]}
    return g, {k: O.edge_rot_mat(vec[k], rnd[k]) for k in FRAMES}


def invariant_loss(out):
    """(out[PA]**2).sum() + (out[LA]**2).sum(): unchanged by every transformation here, rotation included (D is orthogonal)."""
    return (out[PA] ** 2).sum() + (out[LA] ** 2).sum()


def oracle_embedding(sd, L, dicts, rands, pick=identity, grads=False):
    """The four outputs (after `pick`) and, with grads, {name: gradient of invariant_loss}."""
    g, rots = oracle_inputs(dicts, rands)
    sd = {k: v.detach().clone().requires_grad_(grads and v.dtype.is_floating_point) for k, v in sd.items()}
    with torch.set_grad_enabled(grads):
        full = O.embedding_forward(sd, g, rots, L)
        out = pick({k: full[k] for k in OUTS})
        if grads:
            invariant_loss(out).backward()
    return {k: v.detach() for k, v in out.items()}, {k: v.grad for k, v in sd.items() if v.grad is not None}


class oracle_gate_log:
    """relu_gate_log for the CPU oracle: the ReLU gates ([rows, 1024] bool) of every oracle.pos_ffn call, in call order."""

    def __init__(self):
        self.masks = []

    def __enter__(self):
        self._orig = O.pos_ffn

        def pos_ffn(sd, p, x):
            # the same call on the same shapes as oracle.pos_ffn and oracle_pinned_relu_ties make: the same bits at a tie
            pre = torch.nn.functional.linear(x, sd[p + ".conv1.weight"][:, :, 0], sd[p + ".conv1.bias"])
            self.masks.append(pre.detach().reshape(-1, 1024) > 0)
            return self._orig(sd, p, x)

        O.pos_ffn = pos_ffn
        return self

    def __exit__(self, *exc):
        O.pos_ffn = self._orig
        return False


def oracle_step(sd, L, dicts, rands, knn_p, knn_l, lap_p, lap_l, grads=False, ctx=None):
    """(logits, loss, {name: gradient}) of the full step; `ctx`: a context manager around the run (gate log / pinned gates).
    Autograd records every run, with or without a backward pass: torch takes another route through F.linear without it, and
    a ReLU gate at a tie may then fall the other way than in the run whose gradients are compared."""
    import contextlib
    g, rots = oracle_inputs(dicts, rands)
    sd = {k: v.detach().clone().requires_grad_(v.dtype.is_floating_point) for k, v in sd.items()}
    c = lambda t: torch.as_tensor(np.asarray(t.detach().cpu() if torch.is_tensor(t) else t))
    with (ctx if ctx is not None else contextlib.nullcontext()):
        logits = O.singa_forward(sd, g, rots, L, c(knn_p), c(knn_l), c(lap_p), c(lap_l))
        loss = torch.nn.functional.cross_entropy(logits, g["tok_tgt"].reshape(-1))
        if grads:
            loss.backward()
    return logits.detach(), float(loss.detach()), {k: v.grad for k, v in sd.items() if v.grad is not None}


# ------------------------------------------------------------------------------------------------ batches of several graphs
def node_maps(sizes, order):
    """Graphs of `sizes` atoms collated in the order `order` (slot i holds old graph order[i]): new index of every old node."""
    old_ptr = np.concatenate([[0], np.cumsum(sizes)])
    new_sizes = [sizes[i] for i in order]
    new_ptr = np.concatenate([[0], np.cumsum(new_sizes)])
    new_of = np.empty(int(old_ptr[-1]), np.int64)
    for slot, i in enumerate(order):
        new_of[old_ptr[i]:old_ptr[i + 1]] = np.arange(sizes[i]) + new_ptr[slot]
    return new_of


def remap_knn(knn, new_of):
    """A raw kNN list [2, E] in another numbering, its entries regrouped by centre node."""
    k = new_of[np.asarray(knn)]
    return k[:, np.argsort(k[0], kind="stable")]


def remap_rows(x, new_of):
    out = np.empty_like(np.asarray(x))
    out[new_of] = np.asarray(x)
    return out
