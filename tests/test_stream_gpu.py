"""Continuous sampling on the GPU (`singa_amd.model.Sampling.sample_stream`; include/singa_hip_stream.h states the rule): the
choice and the hand-over kernels alone against the per-row ops and tests/stream_rule.py, their write footprints, the per-row
self-attention against the scalar one, and the defining property end to end - `sample_stream` equals `sample` bit for bit
whatever the row budget."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.helpers import Arena, golden, smi_voc
from tests.stream_rule import live_after, stream_rule
from tests.test_beam_gpu import build_model
from tests.test_sampling_gpu import cpu_uniforms, example_of, run, well_formed

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = 1                                                                     # pos_offset of the kernel tests


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def arena_pair(fn):
    """`fn(arena)` under both canaries -> the two reports, after the footprint assertions"""
    reps = []
    for canary in ("nan", "big"):
        ar = Arena(DEV, canary, capacity=16 << 20)
        fn(ar)
        reps.append(ar.report())
    for rep in reps:
        assert not rep.stray, ("words outside the promised views changed", rep.stray)
        assert not rep.unwritten, ("promised elements never written", rep.unwritten)
    differ = [n for n in reps[0].bits if not torch.equal(reps[0].bits[n], reps[1].bits[n])]
    assert not differ, ("outputs that depend on what memory held before the call", differ)
    return reps


# ---------------------------------------------------------------------------------------------------------------- 1
def marks(V):
    """(sos, eos, pad, class bytes or None): the real vocabulary where V is its size (then the grammar runs too)"""
    voc = smi_voc()
    if V == len(voc):
        from singa_amd import smiles
        return voc.index("&"), voc.index("$"), voc.index("^"), torch.as_tensor(smiles.classify(voc)).to(DEV)
    return 0, 1, 0, None


def logit_table(M, T, V, eos, seed):
    """[M, T - 1, V] f32: the logits molecule j sees at step t, `eos` carrying roughly a third of the mass"""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(M, T - 1, V, generator=g) * 2
    z[:, :, eos] = -float("inf")
    z[:, :, eos] = torch.logsumexp(z, -1) - float(np.log(2.0)) if V > 1 else 0.0
    return z.to(DEV)


def reference_run(table, u, T, sos, eos, pad, cls):
    """`ops.sample_token` / `sample_token_grammar` on one row per molecule, step by step -> the final state and sum_logp /
    length after every step"""
    from singa_amd import ops, smiles
    M, _, V = table.shape
    st = {"tokens": torch.full((M, T), pad, dtype=torch.int64, device=DEV), "next": torch.full((M,), sos, dtype=torch.int64, device=DEV),
          "finished": torch.zeros(M, dtype=torch.uint8, device=DEV), "length": torch.zeros(M, dtype=torch.int32, device=DEV),
          "sum_logp": torch.zeros(M, device=DEV), "live": torch.full((1,), M, dtype=torch.int32, device=DEV),
          "tok_logp": torch.zeros(M, T, device=DEV)}
    st["tokens"][:, 0] = sos
    if cls is not None:
        st["grammar"] = torch.full((M,), smiles.FRESH, dtype=torch.int32, device=DEV)
        st["allowed_logp"] = torch.zeros(M, T, device=DEV)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    sums, lens = [], []
    for t in range(T - 1):
        pos.fill_(OFF + t)
        ops.sample_token(table[:, t].contiguous(), u, pos, OFF, st, 1.0, 0, 1.0, eos, pad, None, cls=cls)
        sums.append(st["sum_logp"].clone()), lens.append(st["length"].clone())
    return st, sums, lens


def stream_state(B, R, n, T, sos, pad, grammar):
    from singa_amd import smiles
    M, rows, first = B * n, B * R, min(R, n)
    mol0 = np.full((B, R), -1, np.int32)
    mol0[:, :first] = np.arange(B)[:, None] * n + np.arange(first)[None]
    row0 = np.zeros((B, n), np.int32)
    row0[:, :first] = np.arange(B)[:, None] * R + np.arange(first)[None]
    i32 = dict(dtype=torch.int32, device=DEV)
    st = {"tokens": torch.full((M, T), pad, dtype=torch.int64, device=DEV), "tok_logp": torch.zeros(M, T, device=DEV),
          "length": torch.zeros(M, **i32), "sum_logp": torch.zeros(M, device=DEV), "row_of": torch.as_tensor(row0.reshape(-1)).to(DEV),
          "start_step": torch.zeros(M, **i32), "next": torch.full((rows,), sos, dtype=torch.int64, device=DEV),
          "pos": torch.full((rows,), OFF, dtype=torch.int64, device=DEV), "mol": torch.as_tensor(mol0.reshape(-1)).to(DEV),
          "issued": torch.full((B,), first, **i32), "live": torch.full((B,), first, **i32)}
    st["tokens"][:, 0] = sos
    if grammar:
        st["grammar"] = torch.full((rows,), smiles.FRESH, **i32)
        st["allowed_logp"] = torch.zeros(M, T, device=DEV)
    return st


@pytest.mark.parametrize("R", [1, 3, 70])
@pytest.mark.parametrize("V", [2, 116, 1024])
def test_kernels_step_by_step(V, R):
    from singa_amd import ops, smiles
    B, T = 3, 6
    sos, eos, pad, cls = marks(V)
    assert (cls is not None) == (V == 116)
    for n in sorted({1, R, 4 * R + 1}):
        M = B * n
        table = logit_table(M, T, V, eos, seed=V + 7 * R + n)
        u = torch.rand(T, M, generator=torch.Generator().manual_seed(n)).to(DEV)
        ref, ref_sums, ref_lens = reference_run(table, u, T, sos, eos, pad, cls)
        torch.cuda.synchronize()
        counts = ref["length"].cpu().numpy().reshape(B, n)
        ended = (ref["tokens"] == eos).any(1).cpu().numpy()
        if V > 2 and M >= 15:
            assert 0 < ended.sum() and len(set(counts.reshape(-1))) >= 3     # the run has something to hand over at odd times
        want_row, want_start, total = stream_rule(counts, R)
        st = stream_state(B, R, n, T, sos, pad, cls is not None)
        expect = {k: st[k].clone() for k in ("tokens", "tok_logp", "length", "sum_logp") + (("allowed_logp",) if cls is not None else ())}
        for s in range(total + 2):
            mol, t = st["mol"].clone(), st["pos"] - OFF
            live = mol >= 0
            j = mol[live].long()
            logits = table[mol.clamp(min=0).long(), t.clamp(0, T - 2)].contiguous()
            logits[~live] = float("nan")                                   # a retired row's logits are not read
            ops.sample_token_stream(logits, u, st["pos"], st["mol"], OFF, st, 1.0, 0, 1.0, eos, pad, None, cls=cls)
            # the per-molecule outputs after the choice: the reference's column t + 1, its sums after step t
            tl = t[live]
            for k in ("tokens", "tok_logp") + (("allowed_logp",) if cls is not None else ()):
                expect[k][j, tl + 1] = ref[k][j, tl + 1]
            if len(j):
                expect["sum_logp"][j] = torch.stack(ref_sums)[tl, j]
                expect["length"][j] = torch.stack(ref_lens)[tl, j]
            for k, want in expect.items():
                assert same(st[k], want), (k, n, s)
            assert torch.equal(st["next"][live], ref["tokens"][j, tl + 1])
            ops.stream_refill(st["pos"], st["mol"], OFF, st, R, n, T, sos, eos, smiles.FRESH, cls is not None)
            torch.cuda.synchronize()
            # the rows after the hand-over: molecule j sits in row_of[j] during the steps start[j] .. start[j] + count[j] - 1
            after = s + 1
            held = np.flatnonzero((want_start <= after) & (want_start + counts.reshape(-1) > after))
            want_mol = np.full(B * R, -1, np.int32)
            want_mol[want_row[held]] = held
            assert np.array_equal(st["mol"].cpu().numpy(), want_mol), (n, s)
            pos = st["pos"].cpu().numpy()
            assert np.array_equal(pos[want_row[held]], OFF + after - want_start[held]), (n, s)
            assert ((pos >= OFF) & (pos <= OFF + T - 2)).all()
            assert np.array_equal(st["live"].cpu().numpy(), live_after(counts, R, after)), (n, s)
            handed = want_start <= after
            assert np.array_equal(st["issued"].cpu().numpy(), handed.reshape(B, n).sum(1))
            assert np.array_equal(st["row_of"].cpu().numpy()[handed], want_row[handed])
            assert np.array_equal(st["start_step"].cpu().numpy()[handed], want_start[handed])
            fresh = torch.as_tensor(np.isin(np.arange(B * R), want_row[held][want_start[held] == after])).to(DEV)
            assert (st["next"][fresh] == sos).all()
            if cls is not None:
                assert (st["grammar"][fresh] == smiles.FRESH).all()
            if s == total - 1:
                done = {k: v.clone() for k, v in st.items()}
                assert int(st["live"].sum()) == 0
        for k, v in st.items():                                            # two further steps changed nothing
            assert same(v, done[k]), k
        for k in expect:
            assert same(st[k], ref[k]), (k, n)
        assert same(st["length"], ref["length"]) and same(st["sum_logp"], ref["sum_logp"])


# ---------------------------------------------------------------------------------------------------------------- 2
def test_footprint_choice_and_refill():
    """The choice writes one column of the live rows' molecules, their sums and lengths, and the live rows' next / grammar
    words; the hand-over writes what the host twin writes - a retired row and a pocket without a live row are not touched."""
    from singa_amd import _lib, ops, smiles
    voc = smi_voc()
    V, T, B, R, n = len(voc), 6, 2, 4, 6
    sos, eos, pad, cls = marks(V)
    M, rows = B * n, B * R
    lib = _lib.lib()
    stream = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda v: ctypes.c_void_p(v.ptr)
    atom = voc.index("C")
    mol = torch.tensor([2, 3, -1, 4, -1, -1, -1, -1], dtype=torch.int32)
    pos = torch.tensor([3, 5, 2, 2, 4, 1, 3, 5], dtype=torch.int64)         # steps 2, 4 (the last column), -, 1
    live = mol >= 0
    j, t = mol[live].long(), pos[live] - OFF
    table = logit_table(rows, 2, V, eos, seed=5)[:, 0]
    table[~live.to(DEV)] = float("nan")
    u = torch.rand(T, M, generator=torch.Generator().manual_seed(2))
    tokens = torch.full((M, T), pad, dtype=torch.int64)
    tokens[:, 0] = sos
    tok_logp, alp = torch.zeros(M, T), torch.zeros(M, T)
    for jj, tt in zip(j, t):                                               # a prefix of atoms in front of the column to write
        tokens[jj, 1:tt + 1], tok_logp[jj, 1:tt + 1], alp[jj, 1:tt + 1] = atom, -1.5, -0.25
    length, sums = torch.zeros(M, dtype=torch.int32), torch.zeros(M)
    length[j], sums[j] = t.int(), -1.5 * t.float()
    nxt = torch.full((rows,), atom, dtype=torch.int64)
    after_atom = int(smiles.pack(1))                                       # prev = ATOM
    gs = torch.full((rows,), after_atom, dtype=torch.int32)
    dense = {"tokens": tokens, "tok_logp": tok_logp, "allowed_logp": alp, "length": length, "sum_logp": sums, "next": nxt, "grammar": gs}
    dense = {k: v.clone().to(DEV) for k, v in dense.items()}
    ops.sample_token_stream(table, u.to(DEV), pos.to(DEV), mol.to(DEV), OFF, dense, 1.0, 0, 1.0, eos, pad, None, cls=cls)
    torch.cuda.synchronize()
    col = torch.zeros(M, T, dtype=torch.bool)
    col[j, t + 1] = True
    per_mol = torch.zeros(M, dtype=torch.bool)
    per_mol[j] = True

    def choice(ar):
        i = {"logits": ar.view("logits", (rows, V), data=table), "u": ar.view("u", (T, M), data=u),
             "cls": ar.view("cls", (V,), torch.uint8, data=cls), "pos": ar.view("pos", (rows,), torch.int64, data=pos),
             "mol": ar.view("mol", (rows,), torch.int32, data=mol)}
        o = {"tokens": ar.view("tokens", (M, T), torch.int64, data=tokens, role="inout", promised=col),
             "tok_logp": ar.view("tok_logp", (M, T), data=tok_logp, role="inout", promised=col),
             "allowed_logp": ar.view("allowed_logp", (M, T), data=alp, role="inout", promised=col),
             "length": ar.view("length", (M,), torch.int32, data=length, role="inout", promised=per_mol),
             "sum_logp": ar.view("sum_logp", (M,), data=sums, role="inout", promised=per_mol),
             "next": ar.view("next", (rows,), torch.int64, data=nxt, role="inout", promised=live),
             "grammar": ar.view("grammar", (rows,), torch.int32, data=gs, role="inout", promised=live)}
        code = lib.singa_sample_token_stream(p(i["logits"]), p(i["u"]), None, p(i["cls"]), p(i["pos"]), p(i["mol"]), OFF, rows, M, V,
                                             T, 1.0, 0, 1.0, eos, pad, p(o["length"]), p(o["sum_logp"]), p(o["tokens"]), p(o["next"]),
                                             p(o["tok_logp"]), p(o["grammar"]), p(o["allowed_logp"]), stream())
        assert code == 0, lib.singa_last_error_string()

    for rep in arena_pair(choice):
        for k, want in dense.items():
            assert same(rep.out[k], want.cpu()), k
    assert (dense["length"].cpu()[j] == t.int() + 1).all()

    # the hand-over: pocket 0 has handed out 5 of its 6 molecules; row 0 has drawn '$' (takes molecule 5), row 1 has written
    # the last column (nothing left: retires), row 2 is retired, row 3 goes on; pocket 1 has no live row
    nxt2 = torch.tensor([eos, atom, eos, atom, eos, eos, eos, eos], dtype=torch.int64)
    issued, live2 = torch.tensor([5, 6], dtype=torch.int32), torch.tensor([3, 0], dtype=torch.int32)
    row_of = torch.tensor([0, 1, 0, 1, 3, 2, 4, 5, 6, 7, 4, 5], dtype=torch.int32)
    start = torch.tensor([0, 0, 4, 3, 6, 0, 0, 0, 0, 0, 3, 3], dtype=torch.int32)
    gs2 = torch.arange(100, 100 + rows, dtype=torch.int32)
    host = {"pos": pos.numpy().copy(), "mol": mol.numpy().copy(), "next": nxt2.numpy().copy(), "grammar": gs2.numpy().copy(),
            "issued": issued.numpy().copy(), "live": live2.numpy().copy(), "row_of": row_of.numpy().copy(),
            "start_step": start.numpy().copy()}
    before = {k: v.copy() for k, v in host.items()}
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert lib.singa_stream_refill_host(B, R, n, T, OFF, sos, eos, smiles.FRESH, *(hp(host[k]) for k in host)) == 0
    hand = {k: v.copy() for k, v in before.items()}
    hand["mol"][:2], hand["pos"][0], hand["pos"][3], hand["next"][0], hand["grammar"][0] = [5, -1], OFF, 3, sos, smiles.FRESH
    hand["issued"][0], hand["live"][0], hand["row_of"][5], hand["start_step"][5] = 6, 2, 0, 4 + 2 + 1
    for k in host:
        assert np.array_equal(host[k], hand[k]), (k, host[k], hand[k])
    src = {"pos": pos, "mol": mol, "next": nxt2, "grammar": gs2, "issued": issued, "live": live2, "row_of": row_of, "start_step": start}

    def refill(ar):
        v = {k: ar.view(k, src[k].shape, src[k].dtype, data=src[k], role="inout", promised=torch.as_tensor(host[k] != before[k]))
             for k in src}
        code = lib.singa_stream_refill(B, R, n, T, OFF, sos, eos, smiles.FRESH, *(p(v[k]) for k in src), stream())
        assert code == 0, lib.singa_last_error_string()

    for rep in arena_pair(refill):
        for k in src:
            assert np.array_equal(rep.out[k].numpy(), host[k]), k


def attn_weights(seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: (torch.randn(*s, generator=g) * 0.1).to(DEV)
    return dict(wqkv_t=r(256, 512), bqkv=r(512), wo_t=r(256, 256), bo=r(256), gamma=1 + r(256), beta=r(256))


def self_attn(rows_form, x, w, kc, vc, pos, y, P):
    from singa_amd import _lib
    _lib.ensure_init(torch.cuda.current_device())
    lib = _lib.lib()
    fn = lib.singa_dec_self_attn_rows if rows_form else lib.singa_dec_self_attn
    ptr = lambda t: ctypes.c_void_p(t if isinstance(t, int) else t.data_ptr())
    code = fn(ptr(x), ptr(w["wqkv_t"]), ptr(w["bqkv"]), ptr(w["wo_t"]), ptr(w["bo"]), ptr(w["gamma"]), ptr(w["beta"]), ptr(kc), ptr(vc),
              ptr(pos), x.shape[0], P, ptr(y), 1e-5, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert code == 0, lib.singa_last_error_string()


def test_footprint_self_attn_rows():
    """One cache position per row and the row of y are written; a row whose position lies outside the cache is left alone."""
    Rr, P = 5, 16
    w = attn_weights()
    g = torch.Generator().manual_seed(1)
    x, k0, v0 = torch.randn(Rr, 256, generator=g), torch.randn(Rr, 4, P, 32, generator=g), torch.randn(Rr, 4, P, 64, generator=g)
    pos = torch.tensor([0, 15, P, 7, -1], dtype=torch.int64)
    ok = (pos >= 0) & (pos < P)
    at = torch.zeros(Rr, 4, P, 1, dtype=torch.bool)
    at[torch.arange(Rr)[ok], :, pos[ok]] = True
    want = {}

    def call(ar):
        xv, pv = ar.view("x", (Rr, 256), data=x), ar.view("pos", (Rr,), torch.int64, data=pos)
        kc = ar.view("k", (Rr, 4, P, 32), data=k0, role="inout", promised=at)
        vc = ar.view("v", (Rr, 4, P, 64), data=v0, role="inout", promised=at)
        y = ar.view("y", (Rr, 256), role="out", promised=ok[:, None])
        self_attn(True, xv.t, w, kc.ptr, vc.ptr, pv.t, y.ptr, P)

    reps = arena_pair(call)
    for r in np.flatnonzero(ok.numpy()):                                    # and the written rows are the scalar kernel's
        kc, vc, y = k0.clone().to(DEV), v0.clone().to(DEV), torch.zeros(Rr, 256, device=DEV)
        self_attn(False, x.to(DEV), w, kc, vc, pos[r:r + 1].to(DEV), y, P)
        torch.cuda.synchronize()
        for rep in reps:
            assert same(rep.out["y"][r], y[r].cpu()) and same(rep.out["k"][r], kc[r].cpu()) and same(rep.out["v"][r], vc[r].cpu()), r


# ---------------------------------------------------------------------------------------------------------------- 3
def test_self_attn_rows_equals_scalar():
    Rr, P = 6, 256
    w = attn_weights(3)
    g = torch.Generator().manual_seed(4)
    x = torch.randn(Rr, 256, generator=g).to(DEV)
    k0, v0 = torch.randn(Rr, 4, P, 32, generator=g).to(DEV), torch.randn(Rr, 4, P, 64, generator=g).to(DEV)

    def scalar(at):
        kc, vc, y = k0.clone(), v0.clone(), torch.zeros(Rr, 256, device=DEV)
        self_attn(False, x, w, kc, vc, torch.tensor([at], dtype=torch.int64, device=DEV), y, P)
        return kc, vc, y

    ref = {at: scalar(at) for at in (0, 17, 63, 64, 255)}
    for at in (0, 63, 64, 255):                                            # all rows at one position
        kc, vc, y = k0.clone(), v0.clone(), torch.zeros(Rr, 256, device=DEV)
        self_attn(True, x, w, kc, vc, torch.full((Rr,), at, dtype=torch.int64, device=DEV), y, P)
        torch.cuda.synchronize()
        for got, want in zip((kc, vc, y), ref[at]):
            assert same(got, want), at
    mixed = [255, 0, 64, 17, 63, 0]                                         # rows at different positions
    kc, vc, y = k0.clone(), v0.clone(), torch.zeros(Rr, 256, device=DEV)
    self_attn(True, x, w, kc, vc, torch.tensor(mixed, dtype=torch.int64, device=DEV), y, P)
    torch.cuda.synchronize()
    for r, at in enumerate(mixed):
        for got, want in zip((kc, vc, y), ref[at]):
            assert same(got[r], want[r]), (r, at)


# ---------------------------------------------------------------------------------------------------------------- 4
PER, T4 = 37, 41
CASES = {"plain": dict(setting=(1.0, 0, 1.0)), "t0.7-k10-p0.95": dict(setting=(0.7, 10, 0.95)), "greedy": dict(setting=(0.0, 0, 1.0)),
         "grammar": dict(setting=(1.0, 0, 1.0), grammar="smiles")}
KEYS = ("lengths", "sum_logp", "token_logp")


@pytest.fixture(scope="module")
def setup():
    z = golden("beam_b2_k6_eos.npz")
    model, _, _ = build_model(z)
    return z, model, example_of(z)


@pytest.fixture(scope="module")
def reference(setup):
    """`sample` with PER rows per pocket, once per case: tokens, the uniforms and the trace on the host"""
    z, model, ex = setup
    out = {}
    for name, kw in CASES.items():
        tokens, u, _, tr = run(z, model, per=PER, T=T4, seed=11, ex=ex, **kw)
        out[name] = tokens, u, {k: v.cpu() for k, v in tr.items() if torch.is_tensor(v)}
    return out


def stream(setup, per, R, T, u, setting=(1.0, 0, 1.0), **kw):
    from singa_amd.model.Sampling import sample_stream
    z, model, ex = setup
    B = len(z["names"])
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(B, 1).to(DEV)
    tr = {}
    tau, k, p = setting
    out = sample_stream(model, smi_voc(), per, B, T, ex, prop, R, device=DEV, temperature=tau, top_k=k, top_p=p, uniforms=u, trace=tr, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), tr


def test_reference_run_has_something_to_hand_over(reference):
    """The condition under which the comparison below means something, on `sample`'s output alone."""
    tokens, _, tr = reference["plain"]
    eos = smi_voc().index("$")
    early = (tokens[:, :-1] == eos).any(1)
    lengths = tr["lengths"].numpy().reshape(-1, PER)
    print("rows ended early:", int(early.sum()), "of", len(early), "distinct lengths per pocket:", [len(set(l)) for l in lengths])
    assert early.mean() >= 0.25
    assert all(len(set(l)) >= 3 for l in lengths)


@pytest.mark.parametrize("R", [1, 5, 37, 64])
@pytest.mark.parametrize("case", list(CASES))
def test_stream_equals_sample_bit_for_bit(setup, reference, case, R):
    tokens, u, tr = reference[case]
    got, st = stream(setup, PER, R, T4, u, **CASES[case])
    assert np.array_equal(got, tokens)
    for k in KEYS + (("allowed_logp",) if "grammar" in CASES[case] else ()):
        assert same(st[k].cpu(), tr[k]), k
    counts = tr["lengths"].numpy().reshape(-1, PER)
    row_of, start, total = stream_rule(counts, R)
    assert np.array_equal(st["row_of"].cpu().numpy(), row_of) and np.array_equal(st["start_step"].cpu().numpy(), start)
    assert total <= st["steps"] < total + 16 and st["path"] == "k17"       # the loop polls every 16 steps
    if R == 5:
        assert (start > 0).mean() > 0.5


# ---------------------------------------------------------------------------------------------------------------- 5
def test_graph_off_repeat_and_generator(setup, reference):
    tokens, u, _ = reference["plain"]
    assert np.array_equal(stream(setup, PER, 5, T4, u, graph=False)[0], tokens)
    assert np.array_equal(stream(setup, PER, 5, T4, u)[0], tokens) and np.array_equal(stream(setup, PER, 5, T4, u)[0], tokens)
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)
    a, tra = stream(setup, PER, 5, T4, None, generator=gen())
    b, trb = stream(setup, PER, 8, T4, None, generator=gen())
    assert np.array_equal(a, b) and same(tra["uniforms"].cpu(), trb["uniforms"].cpu()) and not np.array_equal(a, tokens)


# ---------------------------------------------------------------------------------------------------------------- 6
def test_more_molecules_than_rows(setup, reference):
    tokens, u, _ = reference["plain"]
    n, B = 600, 2
    big = torch.rand(T4, B * n, generator=torch.Generator().manual_seed(9))
    for b in range(B):
        big[:, b * n:b * n + PER] = u[:, b * PER:(b + 1) * PER]
    got, tr = stream(setup, n, 16, T4, big)
    assert got.shape == (B * n, T4)
    well_formed(got, tr["lengths"].cpu().numpy())
    for b in range(B):
        assert np.array_equal(got[b * n:b * n + PER], tokens[b * PER:(b + 1) * PER])
    row_of, start, _ = stream_rule(tr["lengths"].cpu().numpy().reshape(B, n), 16)
    assert np.array_equal(tr["row_of"].cpu().numpy(), row_of) and np.array_equal(tr["start_step"].cpu().numpy(), start)


# ---------------------------------------------------------------------------------------------------------------- 7
def test_refusals(setup):
    from singa_amd.model.Sampling import sample_stream
    z, model, ex = setup
    B, voc = len(z["names"]), smi_voc()
    prop = torch.as_tensor(z["prop"][:1]).float().repeat(B, 1).to(DEV)
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match="one prompt per pocket"):
        sample_stream(model, voc, 4, B, 21, ex, prop.repeat(4, 1), 4, device=DEV)
    for R in (0, 2049):
        with pytest.raises(ValueError, match="rows_per_pocket"):
            sample_stream(model, voc, 4, B, 21, ex, prop, R, device=DEV)
    with pytest.raises(ValueError, match="256 positions"):
        sample_stream(model, voc, 4, B, 300, ex, prop, 4, device=DEV)
    with pytest.raises(ValueError, match="bytes are free"):
        sample_stream(model, voc, 10 ** 9, B, 41, ex, prop, 4, device=DEV, uniforms=torch.zeros(1, 1))
    with pytest.raises(ValueError, match="bytes are free"):
        sample_stream(model, voc, 2048, 4096, 201, ex, prop.repeat(2048, 1), 2048, device=DEV, uniforms=torch.zeros(1, 1))
    with pytest.raises(TypeError):
        sample_stream(model, voc, 4, B, 21, ex, prop, 4, device=DEV, forced=torch.zeros(B, 21))
    assert torch.cuda.memory_allocated() == before                        # refused before anything was allocated


# ---------------------------------------------------------------------------------------------------------------- 8
def test_neighbours_unchanged(setup, reference):
    from singa_amd.model.Sampling import sample_distinct, score
    z, model, ex = setup
    B, voc = len(z["names"]), smi_voc()
    tokens, u, tr = reference["plain"]
    prop = torch.as_tensor(z["prop"][:1]).float()

    def neighbours():
        sc = score(model, voc, [["CCO", "c1ccccc1"], ["CC(=O)N"]], B, ex, prop, device=DEV)
        t2 = {}
        d = sample_distinct(model, voc, 6, B, 21, ex, prop.repeat(B * 6, 1).to(DEV), device=DEV, seed=3, trace=t2)
        return sc["sum_logp"], d.cpu().numpy(), t2["gumbel"].cpu()

    a = neighbours()
    stream(setup, PER, 5, T4, u)
    b = neighbours()
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and same(a[2], b[2])
    again, _, _, tr2 = run(z, model, per=PER, T=T4, ex=ex, u=u)
    assert np.array_equal(again, tokens) and same(tr2["sum_logp"].cpu(), tr["sum_logp"])


# ---------------------------------------------------------------------------------------------------------------- 9
def test_gen_entry_point_rows_per_pocket():
    cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "golden", "--mode", "sample", "--num-samples", "20",
           "--rows-per-pocket", "8", "--max-length", "41", "--seed", "1"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    lines = [l for l in r.stdout.decode().splitlines() if not l.startswith("#")]
    names = {}
    for line in lines:
        name, text, length, logp = line.split("\t")
        assert 0 < int(length) <= 40 and float(logp) <= 0.0 and not set(text) & set("&$")
        names[name] = names.get(name, 0) + 1
    assert len(names) == 3 and set(names.values()) == {20}
