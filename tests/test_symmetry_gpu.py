"""-m gpu: the HIP step under the transformations of tests/symmetry.py - frame roll, edge order, atom numbering, batch
companion, shift, rotation, graph order.  No second implementation is compared against: the transformed run is compared with
the mapped untransformed run of the SAME code, which the mathematics fixes to rounding (about 3e-7 at L = 2: two to three
orders of magnitude below the 1e-4 of the oracle comparisons).  The product builds its frames from `extras['rot_rand']`,
i.e. with its own frame kernel and Wigner rows on every new draw.

The bound.  For each case and quantity the CPU oracle runs on the same two inputs; its defect is d_oracle.  nu is the
oracle's defect under shuffle_edges for that quantity - a transformation that only changes the summation order.  Asserted:
d_hip <= R * max(d_oracle, nu).  Both sides evaluate one formula in fp32 with different summation orders, so R is a small
constant: it started at 4 and was set once, after the first run on an MI355X, to the next power of two above the largest
ratio measured (1.56 -> R = 2; profiles/symmetry/README.md); it is never above 16.  The loss is one fp32 number, so its nu is floored at
one ulp (2^-23).  Under the exact lattice shift every coordinate difference keeps its bits: whatever is run-to-run bit-equal
on the HIP path must be bit-equal there too.

The full model is NOT rotation invariant, by the reference's design (GAN.py hands the transformer every l > 0 coefficient), so
rotation is an embedding-level case only."""
import functools

import numpy as np
import pytest
import torch

from oracle import singa_oracle as O
from tests import symmetry as S
from tests.helpers import (NAMES, bit_equal_report, golden, named_grads, oracle_pinned_relu_ties, pinned_relu_ties, rel_err,
                           relu_gate_flips, relu_gate_log, rowwise_err, state_from_spec)

pytestmark = pytest.mark.gpu
DEV = "cuda"
R = 2.0                # largest ratio measured on an MI355X: 1.56 (profiles/symmetry/README.md)
EPS32 = 2.0 ** -23
SHORT = {S.PA: "P", S.LA: "L", "lp_edge": "lp", "pl_edge": "pl"}
EVERY_L = ["roll", "shuffle_edges", "relabel", "shift_exact", "in_batch_first", "in_batch_second", "rotate_cyclic"]
L2_ONLY = ["shift", "rotate_generic", "rotate_rz90"]


def check(label, d_hip, d_or, nu):
    """Print every (quantity, d_oracle, d_hip, ratio) of a case and assert the ratio rule on all of them."""
    bad = []
    for q in d_hip:
        floor = max(d_or[q], nu[q])
        ratio = d_hip[q] / floor if floor > 0 else (0.0 if d_hip[q] == 0 else float("inf"))
        print(f"SYM | {label} | {q} | {d_or[q]:.2e} | {d_hip[q]:.2e} | {ratio:.2f}")
        if not ratio <= R:
            bad.append((q, d_or[q], nu[q], d_hip[q], ratio))
    assert not bad, (label, bad)


def flat(defects):
    return {f"{SHORT[k]}.{blk}.{m}": v for (k, blk, m), v in defects.items() if blk != "all"}


# =================================================================================================== embedding
@functools.lru_cache(maxsize=None)
def _emb(L):
    from tests.test_model_gpu import build_embedding
    return build_embedding(L)


@functools.lru_cache(maxsize=None)
def _sd(tag):
    return state_from_spec(tag)


def _product_batch(dicts, rands, knn=None, lap=None):
    """Collated product batch whose frames come from the draws; knn / lap: pinned ({'p','l'} arrays) or the product's own."""
    from singa_amd import graph as G
    gs = []
    for d, r in zip(dicts, rands):
        g = G.from_arrays(d, with_lap=False)
        g.extras["rot_rand"] = {k: torch.as_tensor(np.asarray(r[k])) for k in S.FRAMES}
        gs.append(g)
    b = G.collate(gs)
    if knn is not None:
        b.extras["knn"] = {G.PA: torch.as_tensor(np.asarray(knn["p"])), G.LA: torch.as_tensor(np.asarray(knn["l"]))}
    if lap is not None:
        b.nodes[G.PA]["lap_pe"], b.nodes[G.LA]["lap_pe"] = (torch.as_tensor(np.asarray(lap[s])) for s in ("p", "l"))
    assert "edge_rot_mat" not in b.extras
    return b.to(DEV)


def hip_embedding(L, dicts, rands, pick=S.identity):
    emb = _emb(L)
    emb.zero_grad(set_to_none=True)
    res = emb(_product_batch(dicts, rands))
    out = pick({k: res[k].embedding for k in S.OUTS})
    S.invariant_loss(out).backward()
    torch.cuda.synchronize()
    return ({k: v.detach().cpu() for k, v in out.items()},
            {n: p.grad.detach().cpu().clone() for n, p in emb.named_parameters() if p.grad is not None})


@functools.lru_cache(maxsize=None)
def _bases(L, snapped):
    """Untransformed runs: (oracle (outputs, grads), HIP (outputs, grads), HIP run-to-run bit-equal: outputs, grads)."""
    c = S.embedding_cases(L)["shift_exact" if snapped else "roll"]
    first, again = hip_embedding(L, *c.base), hip_embedding(L, *c.base)
    eq_out = all(torch.equal(first[0][k], again[0][k]) for k in S.OUTS)
    eq_grad = all(torch.equal(first[1][n], again[1][n]) for n in first[1])
    print(f"L={L}: HIP embedding run to run: outputs {'bit-equal' if eq_out else 'DIFFER'}, "
          f"gradients {'bit-equal' if eq_grad else 'DIFFER'}")
    return S.oracle_embedding(_sd(f"embed_L{L}"), L, *c.base, grads=True), first, eq_out, eq_grad


def _defects(base, run, expect):
    d = flat(S.output_defects(run[0], expect(base[0])))
    d["grad"] = S.grad_defect(run[1], base[1])[0]
    return d


@functools.lru_cache(maxsize=None)
def _oracle_defects(L, name):
    c = S.embedding_cases(L, full=(L == 2))[name]
    run = S.oracle_embedding(_sd(f"embed_L{L}"), L, *c.run, c.pick, grads=True)
    return _defects(_bases(L, name == "shift_exact")[0], run, c.expect)


@pytest.mark.parametrize("L,name", [(L, n) for L in (2, 4, 6) for n in EVERY_L] + [(2, n) for n in L2_ONLY])
def test_embedding_symmetry(L, name):
    c = S.embedding_cases(L, full=(L == 2))[name]
    _, base, eq_out, eq_grad = _bases(L, name == "shift_exact")
    run = hip_embedding(L, *c.run, c.pick)
    want = c.expect(base[0])
    d_hip, d_or, nu = _defects(base, run, c.expect), _oracle_defects(L, name), _oracle_defects(L, "shuffle_edges")
    if name in ("shift_exact", "relabel", "in_batch_first", "in_batch_second"):
        so, no, _ = bit_equal_report(run[0], {k: want[k].to(run[0][k].dtype) for k in want}, f"L={L} {name} outputs")
        sg, ng, _ = bit_equal_report(run[1], base[1], f"L={L} {name} gradients")
        if name == "shift_exact":
            assert not eq_out or so == no, "outputs depend on the absolute position"
            assert not eq_grad or sg == ng, "gradients depend on the absolute position"
    check(f"embed L={L} {name}", d_hip, d_or, nu)


# =================================================================================================== full step, L = 2
@functools.lru_cache(maxsize=None)
def _model():
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    model = SINGA(load_config(lmax=2), device=DEV)
    missing, unexpected = model.load_state_dict(_sd("singa_L2"), strict=False)
    assert not unexpected and all(("offset" in m) or m.endswith("pos_emb.pe") or "batch_norm" in m for m in missing), missing
    return model.eval()


@functools.lru_cache(maxsize=None)
def _graphs():
    loaded = [S.load(n) for n in NAMES]
    return [d for d, _ in loaded], [r for _, r in loaded]


@functools.lru_cache(maxsize=None)
def _pins():
    z = golden("singa_L2_B3.npz")
    return {"p": z["knn_p"], "l": z["knn_l"]}, {"p": z["lap_p"], "l": z["lap_l"]}


def hip_step(dicts, rands, knn=None, lap=None, grads=False, ctx=None):
    """(logits, loss, gradients, prepared batch) of one eager step; ctx: gate log / pinned gates around the run."""
    import contextlib
    model = _model()
    model.zero_grad(set_to_none=True)
    b = _product_batch(dicts, rands, knn, lap)
    model.prepare(b)
    with (ctx if ctx is not None else contextlib.nullcontext()):
        logits = model(b)
        loss = torch.nn.functional.cross_entropy(logits, b["ligand_data"]["smiIndices_tgt"].reshape(-1))
        if grads:
            loss.backward()
    gr = {n: g.cpu() for n, g in named_grads(model).items()} if grads else {}
    return logits.detach().cpu(), float(loss.detach()), gr, b


def oracle_step(dicts, rands, knn, lap, grads=False, ctx=None):
    return S.oracle_step(_sd("singa_L2"), 2, dicts, rands, knn["p"], knn["l"], lap["p"], lap["l"], grads, ctx)


def step_defects(base, run, back=S.identity, grads=False):
    d = {"logits.rel": rel_err(back(run[0]), base[0]), "logits.row": rowwise_err(back(run[0]), base[0]),
         "loss": abs(run[1] - base[1]) / abs(base[1])}
    if grads:
        d["grad"] = S.grad_defect(run[2], base[2])[0]
    return d


def _pinned_to(base_masks, masks, pins_for, rerun):
    """Second run of a transformed step with the ReLU gates it decided differently from the untransformed run (`masks` against
    `base_masks`) pinned to the untransformed run's choice ("ReLU ties"): (that run, gates pinned)."""
    flips = relu_gate_flips(masks, base_masks)
    n = int(flips["on"].numel())
    assert n <= 16, n                          # the cap of the other tie-pinning tests: more is more than rounding
    pins = pins_for(records=flips)
    run = rerun(pins)
    assert pins.call == 18 and pins.flipped == n, (pins.call, pins.flipped, n)
    return run, n


@functools.lru_cache(maxsize=None)
def _pinned_base(side):
    """The untransformed step with gradients and its ReLU gates, golden kNN lists and encodings pinned."""
    dicts, rands = _graphs()
    if side == "hip":
        log = relu_gate_log()
        return hip_step(dicts, rands, *_pins(), grads=True, ctx=log), log.take()
    log = S.oracle_gate_log()
    return oracle_step(dicts, rands, *_pins(), grads=True, ctx=log), log.masks


def _with_grads(side, dicts, rands):
    """Defects of a transformed step of the pinned batch, gradients included, tied gates following the untransformed run."""
    base, masks = _pinned_base(side)
    if side == "hip":
        log = relu_gate_log()
        hip_step(dicts, rands, *_pins(), ctx=log)
        run, n = _pinned_to(masks, log.take(), pinned_relu_ties,
                            lambda pins: hip_step(dicts, rands, *_pins(), grads=True, ctx=pins))
    else:
        log = S.oracle_gate_log()
        oracle_step(dicts, rands, *_pins(), ctx=log)
        run, n = _pinned_to(masks, log.masks, oracle_pinned_relu_ties,
                            lambda pins: oracle_step(dicts, rands, *_pins(), grads=True, ctx=pins))
    print(f"{side}: {n} tied ReLU gates pinned to the untransformed run's choice")
    return step_defects(base, run, grads=True)


@functools.lru_cache(maxsize=None)
def _step_nu():
    """The oracle's full-step defect under shuffle_edges (gradients with the tied gates pinned), the loss floored at one ulp."""
    dicts, rands = _graphs()
    sh = [S.shuffle_edges(d, r, seed=30 + i) for i, (d, r) in enumerate(zip(dicts, rands))]
    nu = _with_grads("oracle", [t[0] for t in sh], [t[1] for t in sh])
    nu["loss"] = max(nu["loss"], EPS32)
    return nu


def _nu(keys):
    return {k: _step_nu()[k] for k in keys}


def test_step_under_frame_roll():
    """New draws for every edge frame: logits, loss and every parameter's gradient."""
    dicts, rands = _graphs()
    rolled = [S.roll(d, r, seed=20 + i)[1] for i, (d, r) in enumerate(zip(dicts, rands))]
    d_hip, d_or = _with_grads("hip", dicts, rolled), _with_grads("oracle", dicts, rolled)
    check("step roll", d_hip, d_or, _nu(d_hip))


def test_step_under_shift():
    dicts, rands = _graphs()
    moved = [S.shift(d, r)[0] for d, r in zip(dicts, rands)]
    d_hip = step_defects(_pinned_base("hip")[0], hip_step(moved, rands, *_pins()))
    d_or = step_defects(_pinned_base("oracle")[0], oracle_step(moved, rands, *_pins()))
    check("step shift", d_hip, d_or, _nu(d_hip))


def test_step_under_reversed_graph_order():
    """The batch's graphs in reverse order (kNN lists and encodings renumbered with them); logit rows mapped back."""
    dicts, rands = _graphs()
    knn, lap = _pins()
    new_of = {s: S.node_maps([d[f"z_{s}"].shape[0] for d in dicts], [2, 1, 0]) for s in ("p", "l")}
    knn_r = {s: S.remap_knn(knn[s], new_of[s]) for s in new_of}
    lap_r = {s: S.remap_rows(lap[s], new_of[s]) for s in new_of}
    back = lambda lg: lg.view(3, -1, lg.shape[-1]).flip(0).reshape(lg.shape)
    d_hip = step_defects(_pinned_base("hip")[0], hip_step(dicts[::-1], rands[::-1], knn_r, lap_r), back)
    d_or = step_defects(_pinned_base("oracle")[0], oracle_step(dicts[::-1], rands[::-1], knn_r, lap_r), back)
    check("step reversed", d_hip, d_or, _nu(d_hip))


# ---------------------------------------------------------------------------------- the product's own kNN lists and encodings
def _own_choices(b):
    """What SINGA.prepare chose for a batch: the undirected kNN edges (self loops dropped) as [2, E] and the encodings."""
    from singa_amd import graph as G
    prep = b.extras["prepared"]
    knn, lap = {}, {}
    for s, nt in (("p", G.PA), ("l", G.LA)):
        e = prep[s]["edges"]
        row, col = e.row.cpu(), e.col.cpu()
        knn[s] = torch.stack([row, col])[:, row != col].numpy()
        lap[s] = b[nt]["lap_pe"].detach().cpu().numpy()
    return knn, lap


def _edge_keys(knn, n, new_of=None):
    k = knn if new_of is None else new_of[knn]
    return np.sort(k[0] * n + k[1])


def _assert_laplacian_subspace(lap, dicts):
    """Per graph: orthonormal columns spanning an invariant subspace of the oracle's Laplacian with Ritz values = eigenvalues
    1..8 (the check of test_laplacian_pe_batched_on_gpu_against_oracle_spectrum): signed eigenvectors of a repeated
    eigenvalue - a bonded pocket has dozens of components - are a free choice, the subspace property is not."""
    for s, ek in (("p", "ei_pp"), ("l", "ei_ll")):
        lo = 0
        for d in dicts:
            n = d[f"z_{s}"].shape[0]
            v = lap[s][lo:lo + n].astype(np.float64)
            lo += n
            lapm, w = O.laplacian_spectrum(d[ek], n)
            assert np.abs(v.T @ v - np.eye(8)).max() < 1e-5
            ritz = v.T @ lapm @ v
            assert np.abs(lapm @ v - v @ ritz).max() < 1e-5
            assert np.abs(np.linalg.eigvalsh(ritz) - w[1:9]).max() < 1e-5


def test_step_under_exact_shift_with_own_knn():
    """The lattice shift with the product's own kNN lists and Laplacian encodings: same edge sets, valid encodings, and -
    where the step is bit-equal run to run - bit-equal logits, loss and gradients."""
    dicts, rands = _graphs()
    snapped = [S.snap(d) for d in dicts]
    moved = [S.shift_exact(d, r)[0] for d, r in zip(dicts, rands)]
    base, again, run = (hip_step(x, rands, grads=True) for x in (snapped, snapped, moved))
    (knn0, lap0), (knn1, lap1) = _own_choices(base[3]), _own_choices(run[3])
    for s in ("p", "l"):
        n = lap0[s].shape[0]
        assert np.array_equal(_edge_keys(knn0[s], n), _edge_keys(knn1[s], n)), f"kNN edge set of '{s}' moved with the origin"
    _assert_laplacian_subspace(lap0, snapped)
    _assert_laplacian_subspace(lap1, moved)
    print("step shift_exact: encodings " + ("bit-equal" if all(np.array_equal(lap0[s], lap1[s]) for s in lap0) else "differ"))
    rr_fwd = torch.equal(base[0], again[0]) and base[1] == again[1]
    rr_grad = bit_equal_report(again[2], base[2], "step run to run")[0] == len(base[2])
    print(f"step run to run: logits and loss {'bit-equal' if rr_fwd else 'DIFFER'}")
    same, n, _ = bit_equal_report(run[2], base[2], "step shift_exact gradients")
    fwd_same = torch.equal(run[0], base[0]) and run[1] == base[1]
    print(f"step shift_exact: logits and loss {'bit-equal' if fwd_same else 'differ'}")
    assert not rr_fwd or fwd_same, "logits or loss depend on the absolute position"
    assert not rr_grad or same == n, "gradients depend on the absolute position"
    d_or = step_defects(oracle_step(snapped, rands, knn0, lap0, grads=True), oracle_step(moved, rands, knn1, lap1, grads=True),
                        grads=True)
    d_hip = step_defects(base, run, grads=True)
    check("step shift_exact", d_hip, d_or, _nu(d_hip))


def test_step_under_relabel_with_own_knn():
    """Another numbering of every graph's atoms, the product choosing kNN lists and encodings itself: the same edge set in
    the new numbering and valid encodings.  The encoding of a many-fold eigenvalue is a free choice that may follow the
    numbering (measured: it does, logits move by 1.2e-2 on both sides), so logits and loss are first held to the oracle's
    defect on the product's own choices of both runs, then - with the first run's encodings carried over - to rounding."""
    dicts, rands = _graphs()
    rel = [S.relabel(d, r, seed=40 + i) for i, (d, r) in enumerate(zip(dicts, rands))]
    moved = [t[0] for t in rel]
    base, run = hip_step(dicts, rands), hip_step(moved, rands)
    (knn0, lap0), (knn1, lap1) = _own_choices(base[3]), _own_choices(run[3])
    maps = {}
    for s in ("p", "l"):
        ptr = np.concatenate([[0], np.cumsum([d[f"z_{s}"].shape[0] for d in dicts])])
        maps[s] = np.concatenate([ptr[i] + t[2].new_of[s] for i, t in enumerate(rel)])        # new index of every old atom
        n = int(ptr[-1])
        assert np.array_equal(_edge_keys(knn0[s], n, maps[s]), _edge_keys(knn1[s], n)), f"kNN edge set of '{s}' follows the numbering"
    _assert_laplacian_subspace(lap0, dicts)
    _assert_laplacian_subspace(lap1, moved)
    print(f"step relabel: logits {'bit-equal' if torch.equal(run[0], base[0]) else 'differ'}")
    keys = ["logits.rel", "logits.row", "loss"]
    o_base = oracle_step(dicts, rands, knn0, lap0)
    check("step relabel", step_defects(base, run), step_defects(o_base, oracle_step(moved, rands, knn1, lap1)), _nu(keys))
    # the sharp half: the untransformed run's encodings carried over to the new numbering (the kNN lists stay the product's
    # own) - what is left is the numbering alone, and the logits must agree to rounding
    carried = {s: S.remap_rows(lap0[s], maps[s]) for s in maps}
    run = hip_step(moved, rands, lap=carried)
    knn2 = _own_choices(run[3])[0]
    assert all(np.array_equal(_edge_keys(knn2[s], len(maps[s])), _edge_keys(knn1[s], len(maps[s]))) for s in maps)
    check("step relabel, encodings carried over", step_defects(base, run),
          step_defects(o_base, oracle_step(moved, rands, knn2, carried)), _nu(keys))
