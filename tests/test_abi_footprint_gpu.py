"""-m gpu: the write footprint of every C ABI entry point (include/singa_hip.h), called directly on strided views.

singa_amd.ops hands the library a fresh dense output per call, so the rest of the suite cannot see an element a kernel should
write and does not, a write outside a view, or a result that depends on what an output, a scratch buffer or the gap of a
strided input held before.  Here every view of a call lies inside one allocation of our own (tests.helpers.Arena) between
poisoned guard bands, with every gap poisoned, and the call runs twice - once over quiet-NaN poison, once over 1e30.  Per
case:  (a) no guard or gap word changed,  (b) every promised element was written,  (c) the two runs agree bit for bit,
(d) the values match a float64 evaluation of the same formula under tests.helpers.rowwise_err with the bound of the kernel's
existing direct test (integers: equality).  Strided variants are additionally held to torch.equal with the dense call.
Only sizes and pointers the header allows are passed: the guard bands exist so that a defect lands in our own memory.

test_every_entry_point_has_a_case needs no GPU: a new entry point without a case fails it.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from oracle import singa_oracle as O
from singa_amd import _capi, so3
from tests.helpers import arena_runs, cpu_f64, rowwise_err

F = torch.nn.functional
I32, I64, U8, F64 = torch.int32, torch.int64, torch.uint8, torch.float64

CASES = {}


def case(*entries):
    def deco(fn):
        CASES[fn.__name__] = (fn, entries)
        return fn
    return deco


class Env:
    """The library, the device its views live on and the stream argument: the GPU build here; tests/test_kernels_emul.py
    drives the cases its sequential CPU build of the same source can run through Env(lib, dev="cpu")."""

    def __init__(self, lib=None, dev="cuda"):
        if lib is None:
            from singa_amd import _lib
            _lib.ensure_init(torch.cuda.current_device())
            lib = _lib.lib()
        self.lib, self.dev = lib, dev

    @property
    def st(self):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream) if self.dev == "cuda" else None

    def ok(self, code, what):
        assert code == 0, (what, code, self.lib.singa_last_error_string())


def run_case(name, env=None):
    """Both runs of one case, every figure printed, then all four assertions."""
    fn, _ = CASES[name]
    env = env or Env()
    nan, big, differ, verify = arena_runs(lambda ar: fn(ar, env), env.dev)
    bad, failed = [], None
    try:
        rows = verify(nan.out)
    except AssertionError as exc:                          # reported after the footprint, which usually explains it
        rows, failed = [], exc
    for label, got, want, bound in rows:
        err = rowwise_err(got, want, f"{name} {label} (bound {bound:.0e})")
        if not err <= bound:
            bad.append((label, err, bound))
    assert not nan.stray and not big.stray, ("words outside the promised views changed: {view: (count, first offset)}", nan.stray, big.stray)
    assert not nan.unwritten and not big.unwritten, ("promised elements never written: {view: count}", nan.unwritten, big.unwritten)
    assert not differ, ("outputs that depend on what memory held before the call", differ)
    if failed is not None:
        raise failed
    assert not bad, bad


def idle_rows_are_zero(part, nwork):
    """Partial-sum buffers whose sizing function rounds up (singa_ln_silu_nparts, singa_ln256_nparts, singa_alpha_logits_nslots)
    announce more rows than the `nwork` rows / edges of the problem can give work to - each of those contributes to one
    partial row - so at least nparts - nwork rows are idle, and an idle row holds exact zeros.  (The other sizers - rowdot,
    edge_mlp_bwd, so3_rmsnorm, so3_skinny - announce ceil(work / work per row) rows: none is idle at any size.)"""
    nparts = part.shape[0]
    assert nparts > nwork, (nparts, nwork)
    nzero = int((part.reshape(nparts, -1) == 0).all(1).sum())
    assert nzero >= nparts - nwork, (nzero, nparts, nwork)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def ru(g, *shape):
    return torch.rand(*shape, generator=g)


def p(v):
    return ctypes.c_void_p(v.ptr) if v is not None else None


def row_ptr_of(ids, N):
    rp = torch.zeros(N + 1, dtype=I64)
    rp[1:] = torch.bincount(torch.as_tensor(ids, dtype=I64), minlength=N).cumsum(0)
    return rp.to(I32)


def holes(g, N, E, lo=1):
    """E sorted segment ids in [0, N) that leave the first, the last and a few middle nodes without edges"""
    live = torch.tensor([n for n in range(lo, N - 1) if n % 4 != 2])
    ids = torch.sort(live[torch.randint(0, len(live), (E,), generator=g)]).values
    assert int(ids[0]) > 0 and int(ids[-1]) < N - 1 and len(set(range(lo, N - 1)) - set(ids.tolist())) > 0
    return ids


def wigner_records(g, E, L):
    """float32 reduced Wigner records [E, WSZ] of random frames (the CPU oracle's; the Wigner kernel has its own case)"""
    from tests.test_kernels_gpu import reduced_rows
    rot = O.edge_rot_mat(rn(g, E, 3), ru(g, E, 3))
    return reduced_rows(O.wigner_dense(rot, L), L).float().contiguous()


def d64(t):
    return t.detach().cpu().double()


# ----------------------------------------------------------------------------------------------------------- k1, k2
@case("singa_edge_frames")
def edge_frames(ar, E):
    """stats is an accumulator: started at (100, 0.999), it must come back as (shortest edge, 0.999 exactly) - the minimum
    decided by the data, the maximum by what was there (random helpers stay below 0.99)."""
    g = gen(1)
    n = 1003
    vec, rnd = rn(g, n, 3, scale=2.0), ru(g, n, 3)
    v, r = ar.view("vec", (n, 3), data=vec), ar.view("rnd", (n, 3), data=rnd)
    rot = ar.view("rot", (n, 3, 3), role="out")
    stats = ar.view("stats", (2,), data=[100.0, 0.999], role="inout")
    E.ok(E.lib.singa_edge_frames(p(v), p(r), p(rot), p(stats), n, E.st), "edge_frames")

    def verify(out):
        want_min = float(vec.double().norm(dim=1).min())
        assert abs(float(out["stats"][0]) - want_min) <= 1e-6 * want_min and float(out["stats"][1]) == float(torch.tensor(0.999))
        return [("rot", out["rot"], O.edge_rot_mat(vec.double(), rnd.double()), 1e-6)]
    return verify


@case("singa_wigner_rows")
def wigner_rows(ar, E):
    """Records are WSZ = 36 / 116 / 236 floats (the 35 / 115 / 235 coefficients padded to 16 bytes); the kernel writes the pad
    float as 0, so the whole record is promised."""
    from tests.test_kernels_gpu import reduced_rows
    outs = []
    for L in (2, 4, 6):
        g = gen(L)
        n = 77
        rot = O.edge_rot_mat(rn(g, n, 3), ru(g, n, 3)).float()
        wsz = so3.layout(L, 2).WSZ
        r = ar.view(f"rot{L}", (n, 3, 3), data=rot)
        w = ar.view(f"wr{L}", (n, wsz), role="out")
        E.ok(E.lib.singa_wigner_rows(p(r), p(w), n, L, 2, E.st), "wigner_rows")
        outs.append((L, rot))

    def verify(out):
        res = []
        for L, rot in outs:
            want = reduced_rows(O.wigner_dense(rot.double(), L), L)
            raw = sum((2 * min(l, 2) + 1) * (2 * l + 1) for l in range(L + 1))
            assert raw % 4 and float(out[f"wr{L}"][:, raw:].abs().max()) == 0.0          # the pad floats: exact zeros
            res.append((f"wr L={L}", out[f"wr{L}"], want, 3e-5))
        return res
    return verify


# --------------------------------------------------------------------------------------------------------------- k3-k6
def _gather_rotate_setup(L=4, C=16, Ns=13, Nd=11, n=41):
    from tests.test_kernels_gpu import rad_row_index
    from tests.test_launch_regimes_gpu import wigner_fwd_inv
    g = gen(30 + L)
    lay = so3.layout(L, 2)
    dst = holes(g, Nd, n)
    src = holes(g, Ns, n)[torch.randperm(n, generator=g)]              # sources without edges too: first, last, middle
    wr = wigner_records(g, n, L)
    xs, xd = rn(g, Ns, lay.K, C), rn(g, Nd, lay.K, C)
    rad = rn(g, n, lay.rad_rows, 2 * C)
    fwd, _ = wigner_fwd_inv(wr, L)
    to_m, rri = torch.as_tensor(lay.to_m), rad_row_index(lay)

    def ref(xs_, xd_, rad_):
        return torch.bmm(fwd, torch.cat([xs_[src], xd_[dst]], 2))[:, to_m] * rad_[:, rri]
    return g, lay, src, dst, wr, xs, xd, rad, ref


@case("singa_gather_rotate_fwd")
def gather_rotate_fwd(ar, E):
    L, C = 4, 16
    g, lay, src, dst, wr, xs, xd, rad, ref = _gather_rotate_setup(L, C)
    n = len(src)
    v = [ar.view(k, t.shape, t.dtype, data=t) for k, t in (("xs", xs), ("xd", xd), ("src", src.to(I32)), ("dst", dst.to(I32)),
                                                            ("wr", wr), ("rad", rad))]
    out = ar.view("out", (n, lay.KR, 2 * C), role="out")
    E.ok(E.lib.singa_gather_rotate_fwd(*[p(t) for t in v], p(out), n, C, L, 2, E.st), "gather_rotate_fwd")
    out1 = ar.view("out_norad", (n, lay.KR, 2 * C), role="out")                                     # rad = NULL: no multiply
    E.ok(E.lib.singa_gather_rotate_fwd(*[p(t) for t in v[:5]], None, p(out1), n, C, L, 2, E.st), "gather_rotate_fwd")
    return lambda o: [("out", o["out"], ref(d64(xs), d64(xd), d64(rad)), 2e-5),
                      ("out, rad = NULL", o["out_norad"], ref(d64(xs), d64(xd), torch.ones_like(d64(rad))), 2e-5)]


@case("singa_gather_rotate_bwd")
def gather_rotate_bwd(ar, E):
    """Source and destination nodes without edges (first, last, middle) must receive zero gradient rows."""
    L, C = 4, 16
    g, lay, src, dst, wr, xs, xd, rad, ref = _gather_rotate_setup(L, C)
    n, Ns, Nd = len(src), xs.shape[0], xd.shape[0]
    go = rn(g, n, lay.KR, 2 * C)
    eperm = torch.argsort(src, stable=True)
    ins = [("g", go), ("xs", xs), ("xd", xd), ("src", src.to(I32)), ("dst", dst.to(I32)), ("wr", wr), ("rad", rad),
           ("row_ptr", row_ptr_of(dst, Nd)), ("col_ptr", row_ptr_of(src, Ns)), ("eperm", eperm.to(I32))]
    v = [ar.view(k, t.shape, t.dtype, data=t) for k, t in ins]
    outs = [ar.view("g_rad", rad.shape, role="out"), ar.view("gx_src", xs.shape, role="out"), ar.view("gx_dst", xd.shape, role="out")]
    E.ok(E.lib.singa_gather_rotate_bwd(*[p(t) for t in v], *[p(t) for t in outs], n, Ns, Nd, C, L, 2, E.st), "gather_rotate_bwd")

    def verify(o):
        _, (w_xs, w_xd, w_rad) = cpu_f64(ref, (xs, xd, rad), go)
        idle = torch.bincount(src, minlength=Ns) == 0
        assert bool(idle[0]) and bool(idle[-1]) and float(o["gx_src"][idle].abs().max()) == 0.0
        idle = torch.bincount(dst, minlength=Nd) == 0
        assert bool(idle[0]) and bool(idle[-1]) and float(o["gx_dst"][idle].abs().max()) == 0.0
        return [("d rad", o["g_rad"], w_rad, 2e-5), ("d x_src", o["gx_src"], w_xs, 2e-5), ("d x_dst", o["gx_dst"], w_xd, 2e-5)]
    return verify


# ------------------------------------------------------------------------------------------------------------ k10 / k13
def _scatter_setup(L, CH, heads, Nd=10, n=29, m0=False):
    from tests.test_launch_regimes_gpu import wigner_fwd_inv
    g = gen(50 + L + CH)
    lay = so3.layout(L, 2)
    dst = holes(g, Nd, n)
    wr = wigner_records(g, n, L)
    rows = [lay.m_size[0]] if m0 else list(lay.seg_rows)
    parts = [rn(g, n, r * CH) for r in rows]
    alpha = None if m0 else ru(g, n, heads)
    _, inv = wigner_fwd_inv(wr, L)
    to_l = torch.argsort(torch.as_tensor(lay.to_m))
    scale = 0.37 if m0 else 1.0

    def ref(*ts):
        msg = torch.cat([t.view(n, r, CH) for t, r in zip(ts, rows)], 1)
        if m0:
            msg = torch.cat([msg, msg.new_zeros(n, lay.KR - rows[0], CH)], 1)
        msg = msg[:, to_l]
        if not m0:
            msg = (msg.view(n, lay.KR, heads, CH // heads) * ts[-1].view(n, 1, heads, 1)).reshape(n, lay.KR, CH)
        return O.seg_sum(torch.bmm(inv, msg), dst, Nd) * scale
    return g, lay, dst, wr, rows, parts, alpha, scale, ref


def _seg_views(ar, tag, parts, rows, CH, extra, role="in"):
    """one view per segment with ld = rows * CH + extra floats between edges -> (views, singa_seg_t array)"""
    vs = [ar.view(f"{tag}{i}", t.shape, strides=(r * CH + extra, 1), data=t if role == "in" else None, role=role)
          for i, (t, r) in enumerate(zip(parts, rows))]
    return vs, _capi.segs([(v.ptr, r * CH + extra, r) for v, r in zip(vs, rows)])[0]


@case("singa_rotate_back_scatter_fwd")
def rotate_back_scatter_fwd(ar, E):
    """msg in three segments with ld > rows * CH (column blocks of wider tensors); destination nodes without edges at the start,
    in the middle and at the end come out as exact zeros; the dense layout gives the same bits.  And the m = 0 form (k13)."""
    res = []
    for L, CH, heads, m0 in ((2, 112, 7, False), (4, 16, 1, True)):
        g, lay, dst, wr, rows, parts, alpha, scale, ref = _scatter_setup(L, CH, heads, m0=m0)
        n, Nd, t = len(dst), 10, f"m0={int(m0)}."
        w, rp = ar.view(t + "wr", wr.shape, data=wr), ar.view(t + "rp", (Nd + 1,), I32, data=row_ptr_of(dst, Nd))
        al = ar.view(t + "alpha", alpha.shape, data=alpha) if alpha is not None else None
        for extra in (8, 0):
            _, seg = _seg_views(ar, f"{t}msg{extra}_", parts, rows, CH, extra)
            out = ar.view(f"{t}out{extra}", (Nd, lay.K, CH), role="out")
            E.ok(E.lib.singa_rotate_back_scatter_fwd(seg, len(rows), p(al), p(w), p(rp), p(out), Nd, CH, heads, L, 2, int(m0),
                                                     scale, E.st), "rotate_back_scatter_fwd")
        res.append((t, dst, parts, alpha, ref))

    def verify(o):
        rows_ = []
        for t, dst, parts, alpha, ref in res:
            got = o[t + "out8"]
            assert torch.equal(got, o[t + "out0"])
            idle = torch.bincount(dst, minlength=10) == 0
            assert float(got[idle].abs().max()) == 0.0
            ins = [d64(x) for x in parts] + ([d64(alpha)] if alpha is not None else [])
            rows_.append((t + "out", got, ref(*ins), 2e-5))
        return rows_
    return verify


@case("singa_rotate_back_scatter_bwd")
def rotate_back_scatter_bwd(ar, E):
    """g_msg in three segments with ld > rows * CH, g_alpha_part [E, CH]; the m = 0 form with msg = alpha = g_alpha_part = NULL."""
    res = []
    for L, CH, heads, m0 in ((2, 112, 7, False), (4, 16, 1, True)):
        g, lay, dst, wr, rows, parts, alpha, scale, ref = _scatter_setup(L, CH, heads, m0=m0)
        n, Nd, t = len(dst), 10, f"m0={int(m0)}."
        go = rn(g, Nd, lay.K, CH)
        gv = ar.view(t + "g", go.shape, data=go)
        w, rp = ar.view(t + "wr", wr.shape, data=wr), ar.view(t + "rp", (Nd + 1,), I32, data=row_ptr_of(dst, Nd))
        al = ar.view(t + "alpha", alpha.shape, data=alpha) if alpha is not None else None
        seg = None if m0 else _seg_views(ar, t + "msg", parts, rows, CH, 12)[1]
        for extra in (8, 0):
            _, gseg = _seg_views(ar, f"{t}gmsg{extra}_", parts, rows, CH, extra, role="out")
            gap = ar.view(f"{t}gap{extra}", (n, CH), role="out") if not m0 else None
            E.ok(E.lib.singa_rotate_back_scatter_bwd(p(gv), seg, gseg, len(rows), p(al), p(w), p(rp), p(gap), Nd, CH, heads, L, 2,
                                                     int(m0), scale, E.st), "rotate_back_scatter_bwd")
        res.append((t, m0, heads, CH, go, parts, alpha, ref))

    def verify(o):
        rows_ = []
        for t, m0, heads, CH, go, parts, alpha, ref in res:
            ins = list(parts) + ([alpha] if alpha is not None else [])
            _, grads = cpu_f64(ref, ins, go)
            for i in range(len(parts)):
                assert torch.equal(o[f"{t}gmsg8_{i}"], o[f"{t}gmsg0_{i}"])
                rows_.append((f"{t}d msg{i}", o[f"{t}gmsg8_{i}"], grads[i], 2e-5))
            if not m0:
                assert torch.equal(o[t + "gap8"], o[t + "gap0"])
                rows_.append((t + "d alpha", o[t + "gap8"].view(-1, heads, CH // heads).double().sum(-1), grads[-1], 5e-5))
        return rows_
    return verify


# ------------------------------------------------------------------------------------------------------------------ k9a
HEADS, A_ = 7, 32


def _alpha_setup(n=203):
    g = gen(70)
    h0 = rn(g, n, HEADS * A_)
    w, b, dot = 1 + 0.2 * rn(g, A_), 0.2 * rn(g, A_), 0.2 * rn(g, HEADS, A_)

    def ref(h0_, w_, b_, dot_):
        a = F.layer_norm(h0_.reshape(-1, HEADS, A_), (A_,), w_, b_, 1e-5)
        a = 0.6 * a + 0.4 * a * (2 * torch.sigmoid(a) - 1)
        return (a * dot_).sum(-1)
    return g, n, h0, w, b, dot, ref


def _alpha_inputs(ar, h0, w, b, dot, ld):
    return [ar.view("h0", h0.shape, strides=(ld, 1), data=h0), ld, ar.view("ln_w", w.shape, data=w), ar.view("ln_b", b.shape, data=b),
            ar.view("dot", dot.shape, data=dot)]


@case("singa_alpha_logits_fwd")
def alpha_logits_fwd(ar, E):
    g, n, h0, w, b, dot, ref = _alpha_setup()
    h, ld, vw, vb, vd = _alpha_inputs(ar, h0, w, b, dot, HEADS * A_ + 36)
    out = ar.view("logits", (n, HEADS), role="out")
    E.ok(E.lib.singa_alpha_logits_fwd(p(h), ld, p(vw), p(vb), p(vd), p(out), n, HEADS, A_, 1e-5, E.st), "alpha_logits_fwd")
    hd = ar.view("h0_dense", h0.shape, data=h0)
    outd = ar.view("logits_dense", (n, HEADS), role="out")
    E.ok(E.lib.singa_alpha_logits_fwd(p(hd), HEADS * A_, p(vw), p(vb), p(vd), p(outd), n, HEADS, A_, 1e-5, E.st), "alpha_logits_fwd")

    def verify(o):
        assert torch.equal(o["logits"], o["logits_dense"])
        return [("logits", o["logits"], ref(d64(h0), d64(w), d64(b), d64(dot)), 2e-5)]
    return verify


def _alpha_bwd(ar, E, strided):
    g, n, h0, w, b, dot, ref = _alpha_setup()
    gl = rn(g, n, HEADS)
    h, ld, vw, vb, vd = _alpha_inputs(ar, h0, w, b, dot, HEADS * A_ + 36)
    vg = ar.view("g_logits", gl.shape, data=gl)
    nslots = E.lib.singa_alpha_logits_nslots(n)
    width = (2 + HEADS) * A_
    gx = ar.view("g_x", h0.shape, role="out")
    part = ar.view("part", (nslots, width), role="out")
    E.ok(E.lib.singa_alpha_logits_bwd(p(h), ld, p(vw), p(vb), p(vd), p(vg), p(gx), p(part), n, HEADS, A_, 1e-5, E.st), "alpha_logits_bwd")
    hd = ar.view("h0_dense", h0.shape, data=h0)
    gxd, partd = ar.view("g_x_dense", h0.shape, role="out"), ar.view("part_dense", (nslots, width), role="out")
    E.ok(E.lib.singa_alpha_logits_bwd(p(hd), HEADS * A_, p(vw), p(vb), p(vd), p(vg), p(gxd), p(partd), n, HEADS, A_, 1e-5, E.st),
         "alpha_logits_bwd")
    if strided:
        ld_gx = HEADS * A_ + 132
        gxs = ar.view("g_x_ld", h0.shape, strides=(ld_gx, 1), role="out")
        parts = ar.view("part_ld", (nslots, width), role="out")
        E.ok(E.lib.singa_alpha_logits_bwd_ld(p(h), ld, p(vw), p(vb), p(vd), p(vg), p(gxs), ld_gx, p(parts), n, HEADS, A_, 1e-5, E.st),
             "alpha_logits_bwd_ld")

    def verify(o):
        _, (w_h, w_w, w_b, w_d) = cpu_f64(ref, (h0, w, b, dot), gl)
        k = "_ld" if strided else ""
        assert torch.equal(o["g_x"], o["g_x_dense"]) and torch.equal(o["part"], o["part_dense"])          # h0 with ld > heads * A
        if strided:
            assert torch.equal(o["g_x_ld"], o["g_x"]) and torch.equal(o["part_ld"], o["part"])
        idle_rows_are_zero(o["part" + k], n)
        tot = o["part" + k].double().sum(0)
        return [("d x", o["g_x" + k], w_h, 1e-4), ("d ln_w", tot[:A_], w_w, 1e-4), ("d ln_b", tot[A_:2 * A_], w_b, 1e-4),
                ("d alpha_dot", tot[2 * A_:].view(HEADS, A_), w_d, 1e-4)]
    return verify


@case("singa_alpha_logits_bwd")
def alpha_logits_bwd(ar, E):
    """every one of the singa_alpha_logits_nslots(E) partial rows is written (callers reduce over all of them), the idle ones
    (E = 203 edges, 208 slots) as zeros; h0 with ld > heads * A gives the same bits as the dense call"""
    return _alpha_bwd(ar, E, False)


@case("singa_alpha_logits_bwd_ld")
def alpha_logits_bwd_ld(ar, E):
    """g_x as a column block of a wider tensor (ld_gx > heads * A): the same bits as the dense call, the other columns untouched"""
    return _alpha_bwd(ar, E, True)


# ------------------------------------------------------------------------------------------------------------- k9, k15
def _softmax_setups():
    """(tag, H, eps, dense_segments, N, ids): thread per (segment, head) on short segments, wavefront per segment (H = 4) on
    segments of tens of edges; nodes without edges at the start, in the middle, at the end"""
    g = gen(80)
    return g, [("h7", 7, 1e-16, 0, 14, holes(g, 14, 53)), ("h4dense", 4, 0.0, 1, 9, holes(g, 9, 301))]


@case("singa_segment_softmax_fwd")
def segment_softmax_fwd(ar, E):
    g, setups = _softmax_setups()
    keep = []
    for tag, H, eps, dense, N, ids in setups:
        x = rn(g, len(ids), H, scale=4.0)
        vx, rp = ar.view(tag + "x", x.shape, data=x), ar.view(tag + "rp", (N + 1,), I32, data=row_ptr_of(ids, N))
        out = ar.view(tag + "y", x.shape, role="out")
        E.ok(E.lib.singa_segment_softmax_fwd(p(vx), p(rp), p(out), N, H, eps, dense, E.st), "segment_softmax_fwd")
        keep.append((tag, x, ids, N, eps))
    return lambda o: [(t + " y", o[t + "y"], O.seg_softmax(d64(x), ids, N, eps), 1e-5) for t, x, ids, N, eps in keep]


@case("singa_segment_softmax_bwd")
def segment_softmax_bwd(ar, E):
    """(bound of d x: the per-row figure of tests/test_launch_regimes_gpu.py, 1.5e-4)"""
    g, setups = _softmax_setups()
    keep = []
    for tag, H, eps, dense, N, ids in setups:
        x, gy = rn(g, len(ids), H, scale=4.0), rn(g, len(ids), H)
        y = O.seg_softmax(x.double(), ids, N, eps).float()
        vy, vg = ar.view(tag + "y", y.shape, data=y), ar.view(tag + "gy", gy.shape, data=gy)
        rp = ar.view(tag + "rp", (N + 1,), I32, data=row_ptr_of(ids, N))
        out = ar.view(tag + "gx", x.shape, role="out")
        E.ok(E.lib.singa_segment_softmax_bwd(p(vy), p(vg), p(rp), p(out), N, H, dense, E.st), "segment_softmax_bwd")
        keep.append((tag, x, gy, ids, N, eps))
    return lambda o: [(t + " d x", o[t + "gx"], cpu_f64(lambda x_: O.seg_softmax(x_, ids, N, eps), (x,), gy)[1][0], 1.5e-4)
                      for t, x, gy, ids, N, eps in keep]


def _wsum_setup():
    g = gen(90)
    N, H, Fv = 11, 4, 64
    ids = holes(g, N, 157)
    return g, N, H, Fv, ids, ru(g, len(ids), H), rn(g, len(ids), H, Fv), (lambda w_, v_: O.seg_sum(w_.unsqueeze(-1) * v_, ids, N))


@case("singa_segment_wsum_fwd")
def segment_wsum_fwd(ar, E):
    g, N, H, Fv, ids, w, v, ref = _wsum_setup()
    vw, vv, rp = ar.view("w", w.shape, data=w), ar.view("v", v.shape, data=v), ar.view("rp", (N + 1,), I32, data=row_ptr_of(ids, N))
    out = ar.view("out", (N, H, Fv), role="out")
    E.ok(E.lib.singa_segment_wsum_fwd(p(vw), p(vv), p(rp), p(out), N, H, Fv, E.st), "segment_wsum_fwd")

    def verify(o):
        assert float(o["out"][torch.bincount(ids, minlength=N) == 0].abs().max()) == 0.0
        return [("out", o["out"], ref(d64(w), d64(v)), 1e-5)]
    return verify


@case("singa_segment_wsum_bwd")
def segment_wsum_bwd(ar, E):
    g, N, H, Fv, ids, w, v, ref = _wsum_setup()
    go = rn(g, N, H, Fv)
    vg, vw, vv = ar.view("g", go.shape, data=go), ar.view("w", w.shape, data=w), ar.view("v", v.shape, data=v)
    rp = ar.view("rp", (N + 1,), I32, data=row_ptr_of(ids, N))
    gw, gv = ar.view("gw", w.shape, role="out"), ar.view("gv", v.shape, role="out")
    E.ok(E.lib.singa_segment_wsum_bwd(p(vg), p(vw), p(vv), p(rp), p(gw), p(gv), N, H, Fv, E.st), "segment_wsum_bwd")

    def verify(o):
        _, (w_w, w_v) = cpu_f64(ref, (w, v), go)
        return [("d w", o["gw"], w_w, 1e-5), ("d v", o["gv"], w_v, 1e-6)]
    return verify


# -------------------------------------------------------------------------------------------------------------------- k8
def _s2_edge_setup(L=2, C=128, n=37):
    """the attention grid on m-primary rows in three segments; gate = a column block (ldg > C)"""
    from tests.test_launch_regimes_gpu import sep_s2_act64
    g = gen(100 + L)
    lay = so3.layout(L, 2)
    rows = list(lay.seg_rows)
    parts = [rn(g, n, r * C) for r in rows]
    gate = rn(g, n, C)
    to_m = torch.as_tensor(lay.to_m)

    def ref(gate_, *ps):
        xm = torch.cat([t.view(n, r, C) for t, r in zip(ps, rows)], 1)
        return sep_s2_act64(gate_, xm[:, torch.argsort(to_m)], L, 2)[:, to_m]
    return g, lay, rows, parts, gate, ref


def _s2_tables(ar, L, M, m_primary):
    return [ar.view(f"tab{k}", t.shape, data=t) for k, t in
            enumerate(torch.tensor(np.ascontiguousarray(t), dtype=torch.float32) for t in so3.s2_grid_factors(L, M, m_primary))]


def _s2_grid_mats(ar, L, M, lay):
    to, fr = so3.s2_grid(L, M)
    to, fr = (torch.tensor(np.ascontiguousarray(t[:, lay.to_m]), dtype=torch.float32) for t in (to, fr))
    return ar.view("to_grid", to.shape, data=to), ar.view("from_grid", fr.shape, data=fr), to.shape[0], to.shape[1]


@case("singa_s2act_fwd")
def s2act_fwd(ar, E):
    """segmented x with ld > rows * C and gate with ldg > C: the same bits as the call on dense segments and a dense gate"""
    L, C = 2, 128
    g, lay, rows, parts, gate, ref = _s2_edge_setup(L, C)
    n = gate.shape[0]
    _, seg = _seg_views(ar, "x", parts, rows, C, 20)
    gt = ar.view("gate", gate.shape, strides=(C + 12, 1), data=gate)
    to, fr, G, KIN = _s2_grid_mats(ar, L, 2, lay)
    out = ar.view("out", (n, KIN, C), role="out")
    E.ok(E.lib.singa_s2act_fwd(seg, 3, p(gt), C + 12, p(to), p(fr), p(out), n, C, KIN, G, E.st), "s2act_fwd")
    _, segd = _seg_views(ar, "xd", parts, rows, C, 0)
    gtd = ar.view("gate_d", gate.shape, data=gate)
    outd = ar.view("out_dense", (n, KIN, C), role="out")
    E.ok(E.lib.singa_s2act_fwd(segd, 3, p(gtd), C, p(to), p(fr), p(outd), n, C, KIN, G, E.st), "s2act_fwd")

    def verify(o):
        assert torch.equal(o["out"], o["out_dense"])
        return [("out", o["out"], ref(d64(gate), *[d64(t) for t in parts]), 2e-5)]
    return verify


@case("singa_s2act_bwd")
def s2act_bwd(ar, E):
    """segmented x with ld > rows * C and gate with ldg > C: the same bits as the call on dense segments and a dense gate"""
    L, C = 2, 128
    g, lay, rows, parts, gate, ref = _s2_edge_setup(L, C)
    n = gate.shape[0]
    _, seg = _seg_views(ar, "x", parts, rows, C, 20)
    gt = ar.view("gate", gate.shape, strides=(C + 12, 1), data=gate)
    to, fr, G, KIN = _s2_grid_mats(ar, L, 2, lay)
    go = rn(g, n, KIN, C)
    vg = ar.view("g_out", go.shape, data=go)
    gx, gg = ar.view("gx", (n, KIN, C), role="out"), ar.view("g_gate", (n, C), role="out")
    E.ok(E.lib.singa_s2act_bwd(seg, 3, p(gt), C + 12, p(to), p(fr), p(vg), p(gx), p(gg), n, C, KIN, G, E.st), "s2act_bwd")
    _, segd = _seg_views(ar, "xd", parts, rows, C, 0)
    gtd = ar.view("gate_d", gate.shape, data=gate)
    gxd, ggd = ar.view("gx_dense", (n, KIN, C), role="out"), ar.view("g_gate_dense", (n, C), role="out")
    E.ok(E.lib.singa_s2act_bwd(segd, 3, p(gtd), C, p(to), p(fr), p(vg), p(gxd), p(ggd), n, C, KIN, G, E.st), "s2act_bwd")

    def verify(o):
        assert torch.equal(o["gx"], o["gx_dense"]) and torch.equal(o["g_gate"], o["g_gate_dense"])
        _, grads = cpu_f64(ref, (gate, *parts), go)
        want = torch.cat([t.view(n, r, C) for t, r in zip(grads[1:], rows)], 1)
        return [("d x", o["gx"], want, 5e-5), ("d gate", o["g_gate"], grads[0], 1e-5)]
    return verify


def _s2_node_setup(L=2, C=512, n=5):
    from tests.test_launch_regimes_gpu import sep_s2_act64
    g = gen(120 + L)
    K = (L + 1) ** 2
    return g, K, rn(g, n, K, C), rn(g, n, C), (lambda gate_, x_: sep_s2_act64(gate_, x_, L, L))


@case("singa_s2act_sep_fwd")
def s2act_sep_fwd(ar, E):
    """edge flavour (nseg = 3, C = 128, segmented x, ldg > C) and node flavour (nseg = 1, C = 512)"""
    L, C = 2, 128
    g, lay, rows, parts, gate, ref = _s2_edge_setup(L, C)
    n = gate.shape[0]
    _, seg = _seg_views(ar, "x", parts, rows, C, 20)
    gt = ar.view("gate", gate.shape, strides=(C + 12, 1), data=gate)
    P, Q, Az = _s2_tables(ar, L, 2, True)
    out = ar.view("out", (n, lay.KR, C), role="out")
    E.ok(E.lib.singa_s2act_sep_fwd(seg, 3, p(gt), C + 12, p(P), p(Q), p(Az), p(out), n, C, L, E.st), "s2act_sep_fwd")
    _, segd = _seg_views(ar, "xd", parts, rows, C, 0)
    gtd = ar.view("gate_d", gate.shape, data=gate)
    outd = ar.view("out_dense", (n, lay.KR, C), role="out")
    E.ok(E.lib.singa_s2act_sep_fwd(segd, 3, p(gtd), C, p(P), p(Q), p(Az), p(outd), n, C, L, E.st), "s2act_sep_fwd")
    # node flavour
    g2, K, x, gate2, ref2 = _s2_node_setup(L)
    N2, C2 = x.shape[0], x.shape[2]
    vx = ar.view("nx", x.shape, data=x)
    vg2 = ar.view("ngate", gate2.shape, strides=(C2 + 16, 1), data=gate2)
    tabs = [ar.view(f"ntab{k}", t.shape, data=t) for k, t in
            enumerate(torch.tensor(np.ascontiguousarray(t), dtype=torch.float32) for t in so3.s2_grid_factors(L, L, False))]
    nout = ar.view("nout", x.shape, role="out")
    segn, _ = _capi.segs([(vx.ptr, K * C2, K)])
    E.ok(E.lib.singa_s2act_sep_fwd(segn, 1, p(vg2), C2 + 16, *[p(t) for t in tabs], p(nout), N2, C2, L, E.st), "s2act_sep_fwd(node)")

    def verify(o):
        assert torch.equal(o["out"], o["out_dense"])
        return [("edge out", o["out"], ref(d64(gate), *[d64(t) for t in parts]), 2e-5),
                ("node out", o["nout"], ref2(d64(gate2), d64(x)), 2e-5)]
    return verify


def _s2_sep_bwd(ar, E, seg_form):
    L, C = 2, 128
    g, lay, rows, parts, gate, ref = _s2_edge_setup(L, C)
    n = gate.shape[0]
    _, seg = _seg_views(ar, "x", parts, rows, C, 20)
    gt = ar.view("gate", gate.shape, strides=(C + 12, 1), data=gate)
    P, Q, Az = _s2_tables(ar, L, 2, True)
    go = rn(g, n, lay.KR, C)
    vg = ar.view("g_out", go.shape, data=go)
    gx, gg = ar.view("gx", (n, lay.KR, C), role="out"), ar.view("g_gate", (n, C), role="out")
    E.ok(E.lib.singa_s2act_sep_bwd(seg, 3, p(gt), C + 12, p(P), p(Q), p(Az), p(vg), p(gx), p(gg), n, C, L, E.st), "s2act_sep_bwd")
    if seg_form:
        _, gseg = _seg_views(ar, "gxs", parts, rows, C, 24, role="out")
        ggs = ar.view("g_gate_ld", (n, C), strides=(C + 28, 1), role="out")
        E.ok(E.lib.singa_s2act_sep_bwd_seg(seg, 3, p(gt), C + 12, p(P), p(Q), p(Az), p(vg), gseg, p(ggs), C + 28, n, C, L, E.st),
             "s2act_sep_bwd_seg")

    def verify(o):
        _, grads = cpu_f64(ref, (gate, *parts), go)
        want = torch.cat([t.view(n, r, C) for t, r in zip(grads[1:], rows)], 1)
        if seg_form:
            got = torch.cat([o[f"gxs{i}"].view(n, r, C) for i, r in enumerate(rows)], 1)
            assert torch.equal(got, o["gx"]) and torch.equal(o["g_gate_ld"], o["g_gate"])
            return [("d x (segments)", got, want, 5e-5), ("d gate (ld_gg)", o["g_gate_ld"], grads[0], 1e-5)]
        return [("d x", o["gx"], want, 5e-5), ("d gate", o["g_gate"], grads[0], 1e-5)]
    return verify


@case("singa_s2act_sep_bwd")
def s2act_sep_bwd(ar, E):
    return _s2_sep_bwd(ar, E, False)


@case("singa_s2act_sep_bwd_seg")
def s2act_sep_bwd_seg(ar, E):
    """gx in three segments with ld > rows * C and g_gate with ld_gg > C (column blocks of the SO(2) convolution's output
    gradients): the same bits as singa_s2act_sep_bwd, the other columns untouched"""
    return _s2_sep_bwd(ar, E, True)


@case("singa_s2act_ffn_bwd")
def s2act_ffn_bwd(ar, E):
    """gate as a column block (ldg > C): the same bits as the call on a dense gate"""
    L = 2
    g, K, x, gate, ref = _s2_node_setup(L, n=7)
    N, C = x.shape[0], x.shape[2]
    gs, W2 = rn(g, N, K, 16), rn(g, L + 1, 16, C, scale=C ** -0.5)
    deg = torch.as_tensor(so3.layout(L, L).degree)
    vx, vgate = ar.view("x", x.shape, data=x), ar.view("gate", gate.shape, strides=(C + 16, 1), data=gate)
    P, Q, _ = [ar.view(f"tab{k}", t.shape, data=t) for k, t in
               enumerate(torch.tensor(np.ascontiguousarray(t), dtype=torch.float32) for t in so3.s2_grid_factors(L, L, False))]
    vgs, vw = ar.view("g_small", gs.shape, data=gs), ar.view("W2", W2.shape, data=W2)
    gx, gg = ar.view("gx", x.shape, role="out"), ar.view("g_gate", gate.shape, role="out")
    E.ok(E.lib.singa_s2act_ffn_bwd(p(vx), p(vgate), C + 16, p(P), p(Q), p(vgs), p(vw), p(gx), p(gg), N, C, L, E.st), "s2act_ffn_bwd")
    vgated = ar.view("gate_d", gate.shape, data=gate)
    gxd, ggd = ar.view("gx_dense", x.shape, role="out"), ar.view("g_gate_dense", gate.shape, role="out")
    E.ok(E.lib.singa_s2act_ffn_bwd(p(vx), p(vgated), C, p(P), p(Q), p(vgs), p(vw), p(gxd), p(ggd), N, C, L, E.st), "s2act_ffn_bwd")

    def verify(o):
        assert torch.equal(o["gx"], o["gx_dense"]) and torch.equal(o["g_gate"], o["g_gate_dense"])
        gy = torch.einsum("nku,kuc->nkc", d64(gs), d64(W2)[deg])
        _, (w_gate, w_x) = cpu_f64(ref, (gate, x), gy)
        return [("d x", o["gx"], w_x, 5e-5), ("d gate", o["g_gate"], w_gate, 2e-5)]
    return verify


# ------------------------------------------------------------------------------------------------------------------- k12
def _rms_setup(L=4, C=16, N=37):
    g = gen(130)
    K = (L + 1) ** 2
    x, w, b = rn(g, N, K, C, scale=2.0) + 0.3, 1 + 0.1 * rn(g, L + 1, C), 0.1 * rn(g, C)
    return g, L, C, N, K, x, w, b, (lambda x_, w_, b_: O.rms_norm({"n.affine_weight": w_, "n.affine_bias": b_}, "n", x_, L))


@case("singa_so3_rmsnorm_fwd")
def so3_rmsnorm_fwd(ar, E):
    g, L, C, N, K, x, w, b, ref = _rms_setup()
    vx, vw, vb = ar.view("x", x.shape, data=x), ar.view("w", w.shape, data=w), ar.view("b", b.shape, data=b)
    y = ar.view("y", x.shape, role="out")
    E.ok(E.lib.singa_so3_rmsnorm_fwd(p(vx), p(vw), p(vb), p(y), N, C, L, 1e-5, E.st), "so3_rmsnorm_fwd")
    return lambda o: [("y", o["y"], ref(d64(x), d64(w), d64(b)), 1e-5)]


def _rms_bwd(ar, E, add):
    g, L, C, N, K, x, w, b, ref = _rms_setup()
    gy, ga = rn(g, N, K, C), rn(g, N, K, C)
    vx, vw, vg = ar.view("x", x.shape, data=x), ar.view("w", w.shape, data=w), ar.view("gy", gy.shape, data=gy)
    nparts = E.lib.singa_so3_rmsnorm_nparts(N)
    gx, gwp, gbp = ar.view("gx", x.shape, role="out"), ar.view("gw_part", (nparts, L + 1, C), role="out"), ar.view("gb_part", (nparts, C), role="out")
    if add:
        va = ar.view("g_add", ga.shape, data=ga)
        E.ok(E.lib.singa_so3_rmsnorm_bwd_add(p(vx), p(vw), p(vg), p(va), p(gx), p(gwp), p(gbp), N, C, L, 1e-5, E.st), "so3_rmsnorm_bwd_add")
    else:
        E.ok(E.lib.singa_so3_rmsnorm_bwd(p(vx), p(vw), p(vg), p(gx), p(gwp), p(gbp), N, C, L, 1e-5, E.st), "so3_rmsnorm_bwd")

    def verify(o):
        _, (w_x, w_w, w_b) = cpu_f64(ref, (x, w, b), gy)
        return [("d x", o["gx"], w_x + d64(ga) if add else w_x, 2e-5), ("d weight", o["gw_part"].double().sum(0), w_w, 2e-5),
                ("d bias", o["gb_part"].double().sum(0), w_b, 2e-5)]
    return verify


@case("singa_so3_rmsnorm_bwd")
def so3_rmsnorm_bwd(ar, E):
    """all singa_so3_rmsnorm_nparts(N) partial rows are written"""
    return _rms_bwd(ar, E, False)


@case("singa_so3_rmsnorm_bwd_add")
def so3_rmsnorm_bwd_add(ar, E):
    return _rms_bwd(ar, E, True)


# ----------------------------------------------------------------------------------------------------------- column sums
def ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


@case("singa_colsum")
def colsum(ar, E):
    """ld > n, uninitialised work; integer-valued inputs, so the sums are exact in any order"""
    g = gen(140)
    keep = []
    for M, n, ld in ((1, 5, 8), (333, 7, 12), (2049, 33, 40), (4097, 257, 260)):
        x = ints(g, M, n)
        t = f"M{M}."
        vx = ar.view(t + "x", x.shape, strides=(ld, 1), data=x)
        work = ar.view(t + "work", (max(E.lib.singa_colsum_work(M, n), 1),), role="scratch")
        out = ar.view(t + "out", (n,), role="out")
        E.ok(E.lib.singa_colsum(p(vx), ld, M, n, p(work), p(out), E.st), "colsum")
        keep.append((t, x))

    def verify(o):
        for t, x in keep:
            assert torch.equal(o[t + "out"].to(I64), x.to(I64).sum(0)), t
        return []
    return verify


@case("singa_colsum_multi")
def colsum_multi(ar, E):
    """Adds into pre-filled destinations: several segments per job, strided sources, an M = 0 job, the float4 path; what lies in
    front of and behind every destination segment stays as it was."""
    g = gen(150)
    jobs = [((17, 3, 4), [0]), ((700, 33, 40), [0, 5, 20]), ((5000, 300, 300), [0, 128]), ((0, 4, 4), [0]), ((300, 1024, 1028), [0, 512]),
            ((40000, 7, 9), [0, 3])]
    nj, ns = len(jobs), sum(len(c) for _, c in jobs)
    X, LD, MM, NN = (ctypes.c_void_p * nj)(), (ctypes.c_longlong * nj)(), (ctypes.c_longlong * nj)(), (ctypes.c_int * nj)()
    S0, C0, D = (ctypes.c_int * nj)(), (ctypes.c_int * ns)(), (ctypes.c_void_p * ns)()
    q = work = 0
    keep = []
    for k, ((M, n, ld), cuts) in enumerate(jobs):
        x = ints(g, M, n)
        vx = ar.view(f"x{k}", (max(M, 1), n), strides=(ld, 1), data=x if M else ints(g, 1, n))
        X[k], LD[k], MM[k], NN[k], S0[k] = vx.ptr, ld, M, n, q
        work += E.lib.singa_colsum_multi_work(M, n)
        for c0, c1 in zip(cuts, cuts[1:] + [n]):
            init = ints(g, c1 - c0)
            d = ar.view(f"dst{k}_{c0}", (c1 - c0,), data=init, role="inout")
            C0[q], D[q] = c0, d.ptr
            keep.append((f"dst{k}_{c0}", init.to(I64) + x[:, c0:c1].to(I64).sum(0)))
            q += 1
    w = ar.view("work", (work + 4,), role="scratch")
    E.ok(E.lib.singa_colsum_multi(nj, X, LD, MM, NN, S0, ns, C0, D, p(w), work + 4, E.st), "colsum_multi")

    def verify(o):
        for name, want in keep:
            assert torch.equal(o[name].to(I64), want), name
        return []
    return verify


# ------------------------------------------------------------------------------------------------------------------ k11s
def _skinny_setup(L=4, C=512, N=13):
    g = gen(160)
    K = (L + 1) ** 2
    deg = torch.as_tensor(so3.layout(L, L).degree)
    return g, L, C, N, K, deg, rn(g, N, K, 16)


def _skinny_variants(E):
    return (0, 1) if E.dev == "cuda" else (1,)          # 0: the matrix-core kernels (GPU only), 1: the lane-broadcast ones


@case("singa_so3_skinny_expand")
def so3_skinny_expand(ar, E):
    """both W stride forms (weight[l][c][u] with bias, weight[l][u][c] without), both kernel variants"""
    g, L, C, N, K, deg, small = _skinny_setup()
    w_cu, w_uc, bias = rn(g, L + 1, C, 16, scale=0.25), rn(g, L + 1, 16, C, scale=0.25), rn(g, C)
    vs, v1, v2, vb = (ar.view(k, t.shape, data=t) for k, t in (("small", small), ("w_cu", w_cu), ("w_uc", w_uc), ("bias", bias)))
    try:
        for var in _skinny_variants(E):
            E.ok(E.lib.singa_so3_skinny_variant(var), "variant")
            b1, b2 = ar.view(f"big_cu{var}", (N, K, C), role="out"), ar.view(f"big_uc{var}", (N, K, C), role="out")
            E.ok(E.lib.singa_so3_skinny_expand(p(vs), p(v1), C * 16, 16, 1, p(vb), p(b1), N, C, L, E.st), "so3_skinny_expand")
            E.ok(E.lib.singa_so3_skinny_expand(p(vs), p(v2), 16 * C, 1, C, None, p(b2), N, C, L, E.st), "so3_skinny_expand")
    finally:
        E.lib.singa_so3_skinny_variant(0 if E.dev == "cuda" else 1)

    def verify(o):
        want1 = torch.einsum("nku,kcu->nkc", d64(small), d64(w_cu)[deg])
        want1[:, 0] += d64(bias)
        want2 = torch.einsum("nku,kuc->nkc", d64(small), d64(w_uc)[deg])
        return [r for var in _skinny_variants(E) for r in ((f"[l][c][u] + bias, variant {var}", o[f"big_cu{var}"], want1, 2e-6),
                                                           (f"[l][u][c], variant {var}", o[f"big_uc{var}"], want2, 5e-6))]
    return verify


@case("singa_so3_skinny_reduce")
def so3_skinny_reduce(ar, E):
    """all singa_so3_skinny_nparts rows are written, in both row layouts, with and without the bias row"""
    g, L, C, N, K, deg, small = _skinny_setup()
    big = rn(g, N, K, C)
    vs, vb = ar.view("small", small.shape, data=small), ar.view("big", big.shape, data=big)
    nparts = E.lib.singa_so3_skinny_nparts(N, L, C)
    wsz = (L + 1) * 16 * C
    try:
        for var in _skinny_variants(E):
            E.ok(E.lib.singa_so3_skinny_variant(var), "variant")
            for out_cu, bias_row in ((1, 1), (0, 0)):
                part = ar.view(f"part{var}{out_cu}", (nparts, wsz + (C if bias_row else 0)), role="out")
                E.ok(E.lib.singa_so3_skinny_reduce(p(vs), p(vb), p(part), N, C, L, out_cu, bias_row, E.st), "so3_skinny_reduce")
    finally:
        E.lib.singa_so3_skinny_variant(0 if E.dev == "cuda" else 1)

    def verify(o):
        onehot = torch.eye(L + 1, dtype=F64)[deg]
        ref_uc = torch.einsum("kl,nku,nkc->luc", onehot, d64(small), d64(big))
        rows = []
        for var in _skinny_variants(E):
            tot = o[f"part{var}1"].double().sum(0)
            rows += [(f"[l][c][u], variant {var}", tot[:wsz].view(L + 1, C, 16), ref_uc.transpose(1, 2), 1e-5),
                     (f"bias row, variant {var}", tot[wsz:], d64(big)[:, 0].sum(0), 1e-5),
                     (f"[l][u][c], variant {var}", o[f"part{var}0"].double().sum(0).view(L + 1, 16, C), ref_uc, 1e-5)]
        return rows
    return verify


# ------------------------------------------------------------------------------------------- dense pointwise kernels
def _ln_silu_setup():
    g = gen(170)
    M, C = 333, 16
    return g, M, C, rn(g, M, C, scale=2.0) + 0.3, rn(g, C), rn(g, C), (lambda x_, ga, be: F.silu(F.layer_norm(x_, (C,), ga, be, 1e-5)))


@case("singa_ln_silu_fwd")
def ln_silu_fwd(ar, E):
    g, M, C, x, ga, be, ref = _ln_silu_setup()
    vx, vg, vb = ar.view("x", x.shape, data=x), ar.view("gamma", ga.shape, data=ga), ar.view("beta", be.shape, data=be)
    out = ar.view("out", x.shape, role="out")
    E.ok(E.lib.singa_ln_silu_fwd(p(vx), p(vg), p(vb), p(out), M, C, 1e-5, E.st), "ln_silu_fwd")
    return lambda o: [("out", o["out"], ref(d64(x), d64(ga), d64(be)), 1e-5)]


@case("singa_ln_silu_bwd")
def ln_silu_bwd(ar, E):
    """M = 333 rows, singa_ln_silu_nparts = 384 partial rows: the idle ones hold zeros"""
    g, M, C, x, ga, be, ref = _ln_silu_setup()
    go = rn(g, M, C)
    vx, vg, vb, vgo = (ar.view(k, t.shape, data=t) for k, t in (("x", x), ("gamma", ga), ("beta", be), ("g_out", go)))
    gx = ar.view("g_x", x.shape, role="out")
    part = ar.view("part", (E.lib.singa_ln_silu_nparts(M), 2 * C), role="out")
    E.ok(E.lib.singa_ln_silu_bwd(p(vx), p(vg), p(vb), p(vgo), p(gx), p(part), M, C, 1e-5, E.st), "ln_silu_bwd")

    def verify(o):
        _, (w_x, w_g, w_b) = cpu_f64(ref, (x, ga, be), go)
        idle_rows_are_zero(o["part"], M)
        tot = o["part"].double().sum(0)
        return [("d x", o["g_x"], w_x, 1e-4), ("d gamma", tot[:C], w_g, 1e-4), ("d beta", tot[C:], w_b, 1e-4)]
    return verify


def _ssp_setup():
    g = gen(180)
    M, n = 203, 64
    return g, M, n, rn(g, M, n, scale=6.0), rn(g, n), (lambda u_, b_: F.softplus(u_ + b_) - math.log(2.0))


@case("singa_bias_ssp_fwd")
def bias_ssp_fwd(ar, E):
    g, M, n, u, b, ref = _ssp_setup()
    vu, vb = ar.view("u", u.shape, data=u), ar.view("b", b.shape, data=b)
    y = ar.view("y", u.shape, role="out")
    E.ok(E.lib.singa_bias_ssp_fwd(p(vu), p(vb), p(y), M, n, E.st), "bias_ssp_fwd")
    return lambda o: [("y", o["y"], ref(d64(u), d64(b)), 1e-5)]


@case("singa_bias_ssp_bwd")
def bias_ssp_bwd(ar, E):
    g, M, n, u, b, ref = _ssp_setup()
    go = rn(g, M, n)
    vu, vb, vg = ar.view("u", u.shape, data=u), ar.view("b", b.shape, data=b), ar.view("g", go.shape, data=go)
    gu = ar.view("gu", u.shape, role="out")
    E.ok(E.lib.singa_bias_ssp_bwd(p(vu), p(vb), p(vg), p(gu), M, n, E.st), "bias_ssp_bwd")
    return lambda o: [("gu", o["gu"], cpu_f64(ref, (u, b), go)[1][0], 1e-4)]


def _ln256_setup():
    g = gen(190)
    M = 37
    a, r, ga, be = rn(g, M, 256, scale=3.0), rn(g, M, 256), rn(g, 256), rn(g, 256)
    return g, M, a, r, ga, be


@case("singa_ln256_fwd")
def ln256_fwd(ar, E):
    """with the residual and with r = NULL"""
    g, M, a, r, ga, be = _ln256_setup()
    va, vr, vg, vb = (ar.view(k, t.shape, data=t) for k, t in (("a", a), ("r", r), ("gamma", ga), ("beta", be)))
    y, y0 = ar.view("y", a.shape, role="out"), ar.view("y_nores", a.shape, role="out")
    E.ok(E.lib.singa_ln256_fwd(p(va), p(vr), p(vg), p(vb), p(y), M, 256, 1e-5, E.st), "ln256_fwd")
    E.ok(E.lib.singa_ln256_fwd(p(va), None, p(vg), p(vb), p(y0), M, 256, 1e-5, E.st), "ln256_fwd")
    return lambda o: [("y", o["y"], F.layer_norm(d64(a) + d64(r), (256,), d64(ga), d64(be), 1e-5), 2e-5),
                      ("y, r = NULL", o["y_nores"], F.layer_norm(d64(a), (256,), d64(ga), d64(be), 1e-5), 2e-5)]


@case("singa_ln256_bwd")
def ln256_bwd(ar, E):
    """M = 37 rows, singa_ln256_nparts = 40 partial rows: the idle ones hold zeros"""
    g, M, a, r, ga, be = _ln256_setup()
    go = rn(g, M, 256)
    va, vr, vg, vgo = (ar.view(k, t.shape, data=t) for k, t in (("a", a), ("r", r), ("gamma", ga), ("g", go)))
    gs = ar.view("gs", a.shape, role="out")
    part = ar.view("part", (E.lib.singa_ln256_nparts(M), 512), role="out")
    E.ok(E.lib.singa_ln256_bwd(p(va), p(vr), p(vg), p(vgo), p(gs), p(part), M, 256, 1e-5, E.st), "ln256_bwd")

    def verify(o):
        _, (w_a, w_g, w_b) = cpu_f64(lambda a_, ga_, be_: F.layer_norm(a_ + r.double(), (256,), ga_, be_, 1e-5), (a, ga, be), go)
        idle_rows_are_zero(o["part"], M)
        tot = o["part"].double().sum(0)
        return [("gs", o["gs"], w_a, 1e-4), ("d gamma", tot[:256], w_g, 1e-4), ("d beta", tot[256:], w_b, 1e-4)]
    return verify


def _rowdot_setup():
    g = gen(200)
    M = 1037
    return g, M, rn(g, M, 32), rn(g, 32), (lambda x_, b_: 0.25 * (x_ * b_).sum(-1))


@case("singa_rowdot_fwd")
def rowdot_fwd(ar, E):
    g, M, x, b, ref = _rowdot_setup()
    vx, vb = ar.view("x", x.shape, data=x), ar.view("b", b.shape, data=b)
    out = ar.view("out", (M,), role="out")
    E.ok(E.lib.singa_rowdot_fwd(p(vx), p(vb), p(out), M, 32, 0.25, E.st), "rowdot_fwd")
    return lambda o: [("out", o["out"], ref(d64(x), d64(b)), 2e-6)]                 # 1-D: one row, the existing test's global norm


@case("singa_rowdot_bwd")
def rowdot_bwd(ar, E):
    g, M, x, b, ref = _rowdot_setup()
    go = rn(g, M)
    vg, vx, vb = ar.view("g", go.shape, data=go), ar.view("x", x.shape, data=x), ar.view("b", b.shape, data=b)
    gx = ar.view("gx", x.shape, role="out")
    part = ar.view("part", (E.lib.singa_rowdot_nparts(M), 32), role="out")
    E.ok(E.lib.singa_rowdot_bwd(p(vg), p(vx), p(vb), p(gx), p(part), M, 32, 0.25, E.st), "rowdot_bwd")

    def verify(o):
        _, (w_x, w_b) = cpu_f64(ref, (x, b), go)
        return [("d x", o["gx"], w_x, 2e-6), ("d b", o["part"].double().sum(0), w_b, 1e-5)]
    return verify


def _block_setup():
    g = gen(210)
    h, k = 47, 36
    w = rn(g, 2 * h, k)
    ref = lambda w_: torch.cat([torch.cat([w_[:h], -w_[h:]], 1), torch.cat([w_[h:], w_[:h]], 1)], 0)
    return g, h, k, w, ref


@case("singa_block_weight_fwd")
def block_weight_fwd(ar, E):
    g, h, k, w, ref = _block_setup()
    vw, out = ar.view("w", w.shape, data=w), ar.view("out", (2 * h, 2 * k), role="out")
    E.ok(E.lib.singa_block_weight_fwd(p(vw), p(out), h, k, E.st), "block_weight_fwd")

    def verify(o):
        assert torch.equal(o["out"], ref(w))
        return []
    return verify


@case("singa_block_weight_bwd")
def block_weight_bwd(ar, E):
    """accumulate = 0 writes g_w; accumulate != 0 adds to what g_w holds (started from known non-zero contents)"""
    g, h, k, w, ref = _block_setup()
    G, init = rn(g, 2 * h, 2 * k), rn(g, 2 * h, k)
    vG = ar.view("G", G.shape, data=G)
    gw, acc = ar.view("g_w", w.shape, role="out"), ar.view("g_w_acc", w.shape, data=init, role="inout")
    E.ok(E.lib.singa_block_weight_bwd(p(vG), p(gw), h, k, 0, E.st), "block_weight_bwd")
    E.ok(E.lib.singa_block_weight_bwd(p(vG), p(acc), h, k, 1, E.st), "block_weight_bwd")

    def verify(o):
        _, (want,) = cpu_f64(ref, (w,), G)
        return [("g_w", o["g_w"], want, 1e-6), ("initial + g_w", o["g_w_acc"], d64(init) + want, 1e-6)]
    return verify


# ------------------------------------------------------------------------------------------------------------------ k15b
def _gatt_setup():
    """row-sorted edges with centre nodes without edges (first, last, middle) and nodes that are never a `col`"""
    g = gen(220)
    N, H, D, Fv, n = 13, 4, 32, 64, 157
    row = holes(g, N, n)
    col = holes(g, N, n)[torch.randperm(n, generator=g)]
    eperm = torch.argsort(col, stable=True)
    idx = [("row_ptr", row_ptr_of(row, N)), ("col", col.to(I32)), ("col_ptr", row_ptr_of(col, N)), ("eperm", eperm.to(I32)),
           ("row", row.to(I32))]
    return g, N, H, D, Fv, n, row, col, idx


def _views(ar, items):
    return {k: ar.view(k, t.shape, t.dtype, data=t) for k, t in items}


@case("singa_edge_logits_fwd")
def edge_logits_fwd(ar, E):
    g, N, H, D, Fv, n, row, col, idx = _gatt_setup()
    qp, wk, hk, ct = rn(g, N, H, D), rn(g, n, D), rn(g, N, H, D), rn(g, N, H)
    v = _views(ar, [("qp", qp), ("wk", wk), ("hk", hk), ("cterm", ct)] + idx[:2])
    qk = ar.view("qk", (n, H), role="out")
    scale = D ** -0.5
    E.ok(E.lib.singa_edge_logits_fwd(p(v["qp"]), p(v["wk"]), p(v["hk"]), p(v["cterm"]), p(v["row_ptr"]), p(v["col"]), p(qk), N, H, D,
                                     scale, E.st), "edge_logits_fwd")
    return lambda o: [("qk", o["qk"], scale * (d64(qp)[row] * d64(wk).unsqueeze(1) * d64(hk)[col]).sum(-1) + d64(ct)[row], 1e-5)]


@case("singa_edge_logits_bwd")
def edge_logits_bwd(ar, E):
    """nodes without edges and nodes that are never a `col` receive zero rows in g_qp / g_cterm and g_hk"""
    g, N, H, D, Fv, n, row, col, idx = _gatt_setup()
    qp, wk, hk, go = rn(g, N, H, D), rn(g, n, D), rn(g, N, H, D), rn(g, n, H)
    v = _views(ar, [("g", go), ("qp", qp), ("wk", wk), ("hk", hk)] + idx)
    outs = [ar.view(k, s, role="out") for k, s in (("g_qp", qp.shape), ("g_wk", wk.shape), ("g_hk", hk.shape), ("g_cterm", (N, H)))]
    scale = D ** -0.5
    E.ok(E.lib.singa_edge_logits_bwd(*[p(v[k]) for k in ("g", "qp", "wk", "hk", "row_ptr", "col", "col_ptr", "eperm", "row")],
                                     *[p(t) for t in outs], N, H, D, scale, E.st), "edge_logits_bwd")

    def verify(o):
        ct = torch.zeros(N, H)
        _, grads = cpu_f64(lambda q_, w_, h_, c_: scale * (q_[row] * w_.unsqueeze(1) * h_[col]).sum(-1) + c_[row], (qp, wk, hk, ct), go)
        assert float(o["g_hk"][torch.bincount(col, minlength=N) == 0].abs().max()) == 0.0
        assert float(o["g_qp"][torch.bincount(row, minlength=N) == 0].abs().max()) == 0.0
        return [(k, o[k], w, 2e-5) for k, w in zip(("g_qp", "g_wk", "g_hk", "g_cterm"), grads)]
    return verify


@case("singa_gather_wsum_fwd")
def gather_wsum_fwd(ar, E):
    g, N, H, D, Fv, n, row, col, idx = _gatt_setup()
    al, wv, hv = ru(g, n, H), rn(g, n, Fv), rn(g, N, H, Fv)
    v = _views(ar, [("alpha", al), ("wv", wv), ("hv", hv)] + idx[:2])
    out = ar.view("out", (N, H, Fv), role="out")
    E.ok(E.lib.singa_gather_wsum_fwd(p(v["alpha"]), p(v["wv"]), p(v["hv"]), p(v["row_ptr"]), p(v["col"]), p(out), N, H, Fv, E.st),
         "gather_wsum_fwd")

    def verify(o):
        want = torch.zeros(N, H, Fv, dtype=F64).index_add_(0, row, d64(al).unsqueeze(-1) * d64(wv).unsqueeze(1) * d64(hv)[col])
        assert float(o["out"][torch.bincount(row, minlength=N) == 0].abs().max()) == 0.0
        return [("out", o["out"], want, 1e-5)]
    return verify


@case("singa_gather_wsum_bwd")
def gather_wsum_bwd(ar, E):
    g, N, H, D, Fv, n, row, col, idx = _gatt_setup()
    al, wv, hv, go = ru(g, n, H), rn(g, n, Fv), rn(g, N, H, Fv), rn(g, N, H, Fv)
    v = _views(ar, [("g", go), ("alpha", al), ("wv", wv), ("hv", hv)] + idx)
    outs = [ar.view(k, s, role="out") for k, s in (("g_alpha", al.shape), ("g_wv", wv.shape), ("g_hv", hv.shape))]
    E.ok(E.lib.singa_gather_wsum_bwd(*[p(v[k]) for k in ("g", "alpha", "wv", "hv", "row_ptr", "col", "col_ptr", "eperm", "row")],
                                     *[p(t) for t in outs], N, H, Fv, E.st), "gather_wsum_bwd")

    def verify(o):
        _, grads = cpu_f64(lambda a_, w_, h_: torch.zeros(N, H, Fv, dtype=a_.dtype).index_add_(
            0, row, a_.unsqueeze(-1) * w_.unsqueeze(1) * h_[col]), (al, wv, hv), go)
        assert float(o["g_hv"][torch.bincount(col, minlength=N) == 0].abs().max()) == 0.0
        return [(k, o[k], w, 2e-5) for k, w in zip(("g_alpha", "g_wv", "g_hv"), grads)]
    return verify


# ------------------------------------------------------------------------------------------------------------------ k15c
def _mlp_setup(n=203):
    g = gen(230)
    attr = rn(g, n, 64)
    nets = []
    for H in (32, 64):
        nets.append([rn(g, H, 64, scale=1 / 8), rn(g, H, scale=0.1), rn(g, H, H, scale=H ** -0.5), rn(g, H, scale=0.1)])
    ref = lambda a, w1, b1, w2, b2: F.linear(F.softplus(F.linear(a, w1, b1)) - math.log(2.0), w2, b2)
    return g, n, attr, nets, ref


@case("singa_edge_mlp_fwd")
def edge_mlp_fwd(ar, E):
    g, n, attr, nets, ref = _mlp_setup()
    va = ar.view("attr", attr.shape, data=attr)
    ws = [ar.view(f"w{i}{j}", t.shape, data=t) for i, net in enumerate(nets) for j, t in enumerate(net)]
    wk, wv = ar.view("wk", (n, 32), role="out"), ar.view("wv", (n, 64), role="out")
    E.ok(E.lib.singa_edge_mlp_fwd(p(va), *[p(t) for t in ws], p(wk), p(wv), n, 64, 32, 64, E.st), "edge_mlp_fwd")
    return lambda o: [("wk", o["wk"], ref(d64(attr), *[d64(t) for t in nets[0]]), 2e-6),
                      ("wv", o["wv"], ref(d64(attr), *[d64(t) for t in nets[1]]), 2e-6)]


@case("singa_edge_mlp_bwd")
def edge_mlp_bwd(ar, E):
    """both nets; all singa_edge_mlp_bwd_nparts(E, H) partial rows are written"""
    g, n, attr, nets, ref = _mlp_setup()
    va = ar.view("attr", attr.shape, data=attr)
    keep = []
    for H, net in zip((32, 64), nets):
        go = rn(g, n, H)
        vg = ar.view(f"g{H}", go.shape, data=go)
        w1, b1, w2 = (ar.view(f"{k}{H}", t.shape, data=t) for k, t in zip(("w1", "b1", "w2"), net[:3]))
        part = ar.view(f"part{H}", (E.lib.singa_edge_mlp_bwd_nparts(n, H), H * 64 + H + H * H + H), role="out")
        E.ok(E.lib.singa_edge_mlp_bwd(p(va), p(vg), p(w1), p(b1), p(w2), p(part), n, 64, H, E.st), "edge_mlp_bwd")
        keep.append((H, net, go))

    def verify(o):
        rows = []
        for H, net, go in keep:
            _, grads = cpu_f64(ref, [attr] + net, go, wrt=range(1, 5))
            tot = o[f"part{H}"].double().sum(0)
            cuts = [0, H * 64, H * 64 + H, H * 64 + H + H * H, H * 64 + 2 * H + H * H]
            rows += [(f"H={H} d {k}", tot[a:b].view(w.shape), w, 2e-5)
                     for k, a, b, w in zip(("W1", "b1", "W2", "b2"), cuts, cuts[1:], grads)]
        return rows
    return verify


# ------------------------------------------------------------------------------------------------------------- k18, k19
def _mask_views(ar, tag, B, T, S, g):
    """(view, stride_b, stride_t, bool mask [B, T, S]) in both forms: a full [B, T, S] mask whose batches are 16 bytes further
    apart than T * S, and a padding mask [B, S] with mask_stride_t = 0; column 0 is never masked"""
    full = ru(g, B, T, S) < 0.3
    full[:, :, 0] = False
    padm = ru(g, B, S) < 0.3
    padm[:, 0] = False
    vf = ar.view(tag + "mask_full", (B, T, S), U8, strides=(T * S + 16, S, 1), data=full.to(U8))
    vp = ar.view(tag + "mask_pad", (B, S), U8, strides=(S + 16, 1), data=padm.to(U8))
    return [(vf, T * S + 16, S, full), (vp, S + 16, 0, padm.unsqueeze(1).expand(B, T, S))]


def _msoftmax_ref(s, mask, heads, scale):
    BH, T, S = s.shape
    return torch.softmax((s.view(-1, heads, T, S) * scale).masked_fill(mask.unsqueeze(1), -1e9), -1).view(BH, T, S)


@case("singa_masked_softmax_fwd")
def masked_softmax_fwd(ar, E):
    g = gen(240)
    B, heads, T, S = 2, 4, 37, 53
    s = rn(g, B * heads, T, S, scale=5.0)
    vs = ar.view("s", s.shape, data=s)
    keep = []
    for i, (vm, sb, stt, m) in enumerate(_mask_views(ar, "", B, T, S, g)):
        out = ar.view(f"p{i}", s.shape, role="out")
        E.ok(E.lib.singa_masked_softmax_fwd(p(vs), p(vm), sb, stt, p(out), B * heads, T, S, heads, 32 ** -0.5, E.st), "masked_softmax_fwd")
        keep.append((i, m))
    return lambda o: [(f"p, mask_stride_t = {'S' if i == 0 else 0}", o[f"p{i}"].view(-1, S),
                       _msoftmax_ref(d64(s), m, heads, 32 ** -0.5).view(-1, S), 1e-6) for i, m in keep]


@case("singa_masked_softmax_bwd")
def masked_softmax_bwd(ar, E):
    g = gen(241)
    B, heads, T, S = 2, 4, 37, 53
    s, gp = rn(g, B * heads, T, S, scale=5.0), rn(g, B * heads, T, S)
    vg = ar.view("gp", gp.shape, data=gp)
    keep = []
    for i, (vm, sb, stt, m) in enumerate(_mask_views(ar, "", B, T, S, g)):
        pr = _msoftmax_ref(s.double(), m, heads, 32 ** -0.5).float()
        vp = ar.view(f"p{i}", pr.shape, data=pr)
        out = ar.view(f"gs{i}", s.shape, role="out")
        E.ok(E.lib.singa_masked_softmax_bwd(p(vp), p(vg), p(vm), sb, stt, p(out), B * heads, T, S, heads, 32 ** -0.5, E.st),
             "masked_softmax_bwd")
        keep.append((i, m))

    def verify(o):
        rows = []
        for i, m in keep:
            _, (want,) = cpu_f64(lambda s_: _msoftmax_ref(s_, m, heads, 32 ** -0.5), (s,), gp)
            assert float(o[f"gs{i}"][m.repeat_interleave(heads, 0)].abs().max()) == 0.0          # zero at masked positions
            rows.append((f"gs, mask_stride_t = {'S' if i == 0 else 0}", o[f"gs{i}"].view(-1, S), want.view(-1, S), 1e-5))
        return rows
    return verify


ATT = dict(B=2, heads=4, T=37, DK=32, DV=64)


def _attn_setup(seed):
    g = gen(seed)
    B, heads, T = ATT["B"], ATT["heads"], ATT["T"]
    q, k, v = rn(g, B * heads, T, 32), rn(g, B * heads, T, 32), rn(g, B * heads, T, 64)
    scale = 32 ** -0.5

    def ref(q_, k_, v_, mask):
        sc = (torch.bmm(q_, k_.transpose(1, 2)) * scale).view(B, heads, T, T).masked_fill(mask.unsqueeze(1), -1e9)
        return torch.bmm(torch.softmax(sc, -1).view(B * heads, T, T), v_)

    def lse(q_, k_, mask):
        sc = (torch.bmm(q_, k_.transpose(1, 2)) * scale).view(B, heads, T, T).masked_fill(mask.unsqueeze(1), -1e9).view(B * heads, T, T)
        mx = sc.max(-1).values
        return torch.stack([mx, 1.0 / torch.exp(sc - mx.unsqueeze(-1)).sum(-1)], -1)
    return g, B, heads, T, q, k, v, scale, ref, lse


def _tm(t, B, heads):
    """[B * heads, T, D] -> token-major [B, T, heads, D]"""
    return t.view(B, heads, t.shape[1], t.shape[2]).transpose(1, 2).contiguous()


def _hm(t, B, heads):
    """token-major [B, T, heads, D] (or [B, T, heads * D]) -> [B * heads, T, D]"""
    t = t.reshape(B, t.shape[1], heads, -1)
    return t.transpose(1, 2).reshape(B * heads, t.shape[1], t.shape[3])


@case("singa_attn_fwd")
def attn_fwd(ar, E):
    """dense (both mask forms), token-major, and token-major on ONE fused [B, T, 512] projection buffer (ld_q = ld_k = ld_v =
    512): the same bits in all layouts"""
    g, B, heads, T, q, k, v, scale, ref, lse = _attn_setup(250)
    BH = B * heads
    masks = _mask_views(ar, "", B, T, T, g)
    vq, vk, vv = ar.view("q", q.shape, data=q), ar.view("k", k.shape, data=k), ar.view("v", v.shape, data=v)

    def call(tag, pq, pk, pv, m, tm, ld):
        vm, sb, stt, _ = m
        ctx, ls = ar.view(tag + "ctx", (BH, T, 64) if not tm else (B, T, heads, 64), role="out"), ar.view(tag + "lse", (BH, T, 2), role="out")
        E.ok(E.lib.singa_attn_fwd(pq, pk, pv, p(vm), sb, stt, p(ctx), p(ls), BH, T, T, heads, 32, 64, tm, ld[0], ld[1], ld[2], scale, E.st),
             "attn_fwd " + tag)
    call("dense.", p(vq), p(vk), p(vv), masks[0], 0, (0, 0, 0))
    call("pad.", p(vq), p(vk), p(vv), masks[1], 0, (0, 0, 0))
    tq, tk, tv = (ar.view("t" + n_, t.shape, data=t) for n_, t in (("q", _tm(q, B, heads)), ("k", _tm(k, B, heads)), ("v", _tm(v, B, heads))))
    call("tm.", p(tq), p(tk), p(tv), masks[0], 1, (0, 0, 0))
    fused = torch.cat([_tm(t, B, heads).reshape(B, T, -1) for t in (q, k, v)], 2)
    assert fused.shape == (B, T, 512)
    vf = ar.view("qkv", fused.shape, data=fused)
    call("fused.", ctypes.c_void_p(vf.ptr), ctypes.c_void_p(vf.ptr + 4 * 128), ctypes.c_void_p(vf.ptr + 4 * 256), masks[0], 1, (512, 512, 512))

    def verify(o):
        for tag in ("tm.", "fused."):
            assert torch.equal(_hm(o[tag + "ctx"], B, heads), o["dense.ctx"]) and torch.equal(o[tag + "lse"], o["dense.lse"]), tag
        rows = []
        for tag, m in (("dense.", masks[0][3]), ("pad.", masks[1][3])):
            rows += [(tag + "ctx", o[tag + "ctx"].reshape(-1, 64), ref(d64(q), d64(k), d64(v), m).reshape(-1, 64), 1e-5),
                     (tag + "lse", o[tag + "lse"].reshape(-1, 2), lse(d64(q), d64(k), m).reshape(-1, 2), 1e-5)]
        return rows
    return verify


@case("singa_attn_bwd")
def attn_bwd(ar, E):
    """dense (both mask forms), token-major, and token-major with g_q | g_k | g_v as the column blocks of ONE [B, T, 512] buffer:
    the three blocks agree with the dense call bit for bit; dsum is uninitialised scratch"""
    g, B, heads, T, q, k, v, scale, ref, lse = _attn_setup(251)
    BH = B * heads
    masks = _mask_views(ar, "", B, T, T, g)
    gc = rn(g, BH, T, 64)
    vq, vk, vv, vgc = (ar.view(n_, t.shape, data=t) for n_, t in (("q", q), ("k", k), ("v", v), ("g_ctx", gc)))
    saved = {}
    for i, m in enumerate(masks):
        c = ref(q.double(), k.double(), v.double(), m[3]).float()
        l = lse(q.double(), k.double(), m[3]).float()
        saved[i] = (c, l, ar.view(f"ctx{i}", c.shape, data=c), ar.view(f"lse{i}", l.shape, data=l))

    def call(tag, ins, outs, mi, tm, ld, vctx, vg):
        vm, sb, stt, _ = masks[mi]
        ds = ar.view(tag + "dsum", (BH, T), role="scratch")
        E.ok(E.lib.singa_attn_bwd(*ins, p(vm), sb, stt, p(vctx), p(saved[mi][3]), p(vg), *outs, p(ds), BH, T, T, heads, 32, 64, tm,
                                  ld[0], ld[1], ld[2], scale, E.st), "attn_bwd " + tag)

    def outs3(tag, tm):
        shp = lambda d: (B, T, heads, d) if tm else (BH, T, d)
        return [p(ar.view(tag + n_, shp(d), role="out")) for n_, d in (("g_q", 32), ("g_k", 32), ("g_v", 64))]
    call("dense.", [p(vq), p(vk), p(vv)], outs3("dense.", 0), 0, 0, (0, 0, 0), saved[0][2], vgc)
    call("pad.", [p(vq), p(vk), p(vv)], outs3("pad.", 0), 1, 0, (0, 0, 0), saved[1][2], vgc)
    tq, tk, tv = (ar.view("t" + n_, t.shape, data=t) for n_, t in (("q", _tm(q, B, heads)), ("k", _tm(k, B, heads)), ("v", _tm(v, B, heads))))
    tctx = ar.view("tctx", (B, T, heads, 64), data=_tm(saved[0][0], B, heads))
    tg = ar.view("tg_ctx", (B, T, heads, 64), data=_tm(gc, B, heads))
    call("tm.", [p(tq), p(tk), p(tv)], outs3("tm.", 1), 0, 1, (0, 0, 0), tctx, tg)
    fused = torch.cat([_tm(t, B, heads).reshape(B, T, -1) for t in (q, k, v)], 2)
    vf = ar.view("qkv", fused.shape, data=fused)
    gf = ar.view("g_qkv", fused.shape, role="out")
    blocks = lambda base: [ctypes.c_void_p(base + 4 * off) for off in (0, 128, 256)]
    call("fused.", blocks(vf.ptr), blocks(gf.ptr), 0, 1, (512, 512, 512), tctx, tg)

    def verify(o):
        fq, fk, fv = o["g_qkv"].split([128, 128, 256], 2)
        for n_, blk in (("g_q", fq), ("g_k", fk), ("g_v", fv)):
            assert torch.equal(_hm(o["tm." + n_], B, heads), o["dense." + n_]), n_
            assert torch.equal(_hm(blk, B, heads), o["dense." + n_]), n_
        rows = []
        for tag, mi in (("dense.", 0), ("pad.", 1)):
            _, grads = cpu_f64(lambda q_, k_, v_: ref(q_, k_, v_, masks[mi][3]), (q, k, v), gc)
            rows += [(tag + n_, o[tag + n_], w, 2e-5) for n_, w in zip(("g_q", "g_k", "g_v"), grads)]
        return rows
    return verify


# ------------------------------------------------------------------------------------------------------------------- k17
DEC = dict(B=3, beams=5, P=67, pos=41, S=77)


def _ln(x, gamma, beta, eps=1e-5):
    return F.layer_norm(x, (256,), gamma, beta, eps)


def _dec_weights(g, shapes):
    return {k: rn(g, *s, scale=(s[0] ** -0.5 if len(s) == 2 else 0.1)) + (1.0 if k == "gamma" else 0.0) for k, s in shapes}


@case("singa_dec_self_attn")
def dec_self_attn(ar, E):
    """Of k_cache / v_cache only position *pos of every row changes, bit for bit; the slots behind *pos hold NaN and must not be
    read."""
    g = gen(260)
    R, P, pos = DEC["B"] * DEC["beams"], DEC["P"], DEC["pos"]
    w = _dec_weights(g, [("wqkv_t", (256, 512)), ("bqkv", (512,)), ("wo_t", (256, 256)), ("bo", (256,)), ("gamma", (256,)), ("beta", (256,))])
    x = rn(g, R, 256)
    kc, vc = rn(g, R, 4, P, 32), rn(g, R, 4, P, 64)
    kc[:, :, pos + 1:], vc[:, :, pos + 1:] = float("nan"), float("nan")
    vx = ar.view("x", x.shape, data=x)
    vw = _views(ar, list(w.items()))
    vk, vv = ar.view("k_cache", kc.shape, data=kc, role="inout"), ar.view("v_cache", vc.shape, data=vc, role="inout")
    vpos = ar.view("pos", (1,), I64, data=[pos])
    y = ar.view("y", (R, 256), role="out")
    E.ok(E.lib.singa_dec_self_attn(p(vx), *[p(vw[k]) for k in ("wqkv_t", "bqkv", "wo_t", "bo", "gamma", "beta")], p(vk), p(vv), p(vpos),
                                   R, P, p(y), 1e-5, E.st), "dec_self_attn")

    def verify(o):
        d = {k_: d64(t) for k_, t in w.items()}
        qkv = d64(x) @ d["wqkv_t"] + d["bqkv"]
        qn, kn, vn = qkv[:, :128].view(R, 4, 32), qkv[:, 128:256].view(R, 4, 32), qkv[:, 256:].view(R, 4, 64)
        K = torch.cat([d64(kc)[:, :, :pos], kn.unsqueeze(2)], 2)
        V = torch.cat([d64(vc)[:, :, :pos], vn.unsqueeze(2)], 2)
        att = torch.softmax(torch.einsum("rhd,rhpd->rhp", qn, K) / math.sqrt(32), -1)
        ctx = torch.einsum("rhp,rhpd->rhd", att, V).reshape(R, 256)
        want = _ln(ctx @ d["wo_t"] + d["bo"] + d64(x), d["gamma"], d["beta"])
        for name, init in (("k_cache", kc), ("v_cache", vc)):
            keep = torch.ones(P, dtype=torch.bool)
            keep[pos] = False
            assert torch.equal(o[name][:, :, keep].view(I32), init[:, :, keep].view(I32)), name
        return [("y", o["y"], want, 2e-5), ("k_cache[*pos]", o["k_cache"][:, :, pos].reshape(R, -1), kn.reshape(R, -1), 2e-5),
                ("v_cache[*pos]", o["v_cache"][:, :, pos].reshape(R, -1), vn.reshape(R, -1), 2e-5)]
    return verify


@case("singa_dec_cross_attn")
def dec_cross_attn(ar, E):
    """rows = proteins x beams (row r reads protein r / beams), a ragged and a fully padded protein"""
    g = gen(261)
    B, beams, S = DEC["B"], DEC["beams"], DEC["S"]
    R = B * beams
    w = _dec_weights(g, [("wq_t", (256, 128)), ("bq", (128,)), ("wo_t", (256, 256)), ("bo", (256,)), ("gamma", (256,)), ("beta", (256,))])
    y, ck, cv = rn(g, R, 256), rn(g, B, 4, 32, S), rn(g, B, 4, S, 64)
    pad = torch.zeros(B, S, dtype=U8)
    pad[1, 2 * S // 3:] = 1
    pad[2] = 1
    vy, vck, vcv, vpad = ar.view("y", y.shape, data=y), ar.view("ck", ck.shape, data=ck), ar.view("cv", cv.shape, data=cv), \
        ar.view("pad", pad.shape, U8, data=pad)
    vw = _views(ar, list(w.items()))
    z = ar.view("z", (R, 256), role="out")
    E.ok(E.lib.singa_dec_cross_attn(p(vy), p(vw["wq_t"]), p(vw["bq"]), p(vck), p(vcv), p(vpad), p(vw["wo_t"]), p(vw["bo"]), p(vw["gamma"]),
                                    p(vw["beta"]), R, beams, S, p(z), 1e-5, E.st), "dec_cross_attn")

    def verify(o):
        d = {k_: d64(t) for k_, t in w.items()}
        qn = (d64(y) @ d["wq_t"] + d["bq"]).view(R, 4, 32)
        prot = torch.arange(R) // beams
        sc = torch.einsum("rhd,rhds->rhs", qn, d64(ck)[prot]) / math.sqrt(32)
        sc = sc.masked_fill(pad.bool()[prot].unsqueeze(1), -1e9)
        ctx = torch.einsum("rhs,rhsd->rhd", torch.softmax(sc, -1), d64(cv)[prot]).reshape(R, 256)
        return [("z", o["z"], _ln(ctx @ d["wo_t"] + d["bo"] + d64(y), d["gamma"], d["beta"]), 2e-5)]
    return verify


@case("singa_dec_ffn")
def dec_ffn(ar, E):
    g = gen(262)
    R = DEC["B"] * DEC["beams"]
    w = _dec_weights(g, [("w1_t", (256, 1024)), ("b1", (1024,)), ("w2_t", (1024, 256)), ("b2", (256,)), ("gamma", (256,)), ("beta", (256,))])
    z = rn(g, R, 256)
    vz = ar.view("z", z.shape, data=z)
    vw = _views(ar, list(w.items()))
    out = ar.view("out", (R, 256), role="out")
    E.ok(E.lib.singa_dec_ffn(p(vz), *[p(vw[k]) for k in ("w1_t", "b1", "w2_t", "b2", "gamma", "beta")], R, p(out), 1e-5, E.st), "dec_ffn")

    def verify(o):
        d = {k_: d64(t) for k_, t in w.items()}
        h = torch.relu(d64(z) @ d["w1_t"] + d["b1"])
        return [("out", o["out"], _ln(h @ d["w2_t"] + d["b2"] + d64(z), d["gamma"], d["beta"]), 2e-5)]
    return verify


# -------------------------------------------------------------------------------------------------------- token choice
@case("singa_sample_token")
def sample_token(ar, E):
    """Three launches on state arrays that start from known non-zero contents: a live step with finished rows and a row that
    draws `eos` (every array = initial (op) result), the same with tok_logp = NULL, and a step outside 0 .. T - 2, which must
    leave every array as it was."""
    from tests.sampling_rule import choose, logp_bound
    g = gen(270)
    R, V, T, eos, padt, off = 6, 37, 7, 3, 0, 10
    tau, top_k, top_p = 0.8, 12, 0.9
    logits = rn(g, R, V, scale=2.0)
    logits[4, eos] = 30.0                                             # row 4 draws eos
    uni = ru(g, T - 1, R)
    allowed = torch.ones(V, dtype=U8)
    allowed[[5, 11]] = 0
    fin0 = torch.tensor([0, 1, 0, 0, 0, 1], dtype=U8)
    init = dict(finished=fin0, length=torch.tensor([2, 3, 2, 2, 2, 1], dtype=I32), sum_logp=-ru(g, R) * 5,
                tokens=torch.randint(4, V, (R, T), generator=g), next=torch.randint(4, V, (R,), generator=g),
                live=torch.tensor([4], dtype=I32), tok_logp=-ru(g, R, T))
    vl, vu, va = ar.view("logits", logits.shape, data=logits), ar.view("uniforms", uni.shape, data=uni), ar.view("allowed", (V,), U8, data=allowed)
    runs = []
    for tag, t, with_lp in (("live.", 2, True), ("nolp.", 2, False), ("out_of_range.", T - 1, True), ("before.", -1, True)):
        vpos = ar.view(tag + "pos", (1,), I64, data=[off + t])
        st = {k: ar.view(tag + k, v_.shape, v_.dtype, data=v_, role="inout") for k, v_ in init.items() if with_lp or k != "tok_logp"}
        E.ok(E.lib.singa_sample_token(p(vl), p(vu), p(va), p(vpos), off, R, V, T, tau, top_k, top_p, eos, padt, p(st["finished"]),
                                      p(st["length"]), p(st["sum_logp"]), p(st["tokens"]), p(st["next"]), p(st["live"]),
                                      p(st.get("tok_logp")), E.st), "sample_token")
        runs.append((tag, t, with_lp))

    def verify(o):
        for tag, t, with_lp in runs:
            keys = [k for k in init if with_lp or k != "tok_logp"]
            if not 0 <= t <= T - 2:
                for k in keys:
                    assert torch.equal(o[tag + k].view(-1), init[k].view(-1)), (tag, k)
                continue
            want = {k: init[k].clone() for k in keys}
            lp_tol = logp_bound(V, 30.0)
            for r in range(R):
                if fin0[r]:
                    want["tokens"][r, t + 1] = want["next"][r] = padt
                    if with_lp:
                        want["tok_logp"][r, t + 1] = 0.0
                    continue
                tok, lp, amb = choose(logits[r].double().numpy(), float(uni[t, r]), tau, top_k, top_p, allowed.numpy(), eps=1e-5)
                assert not amb
                want["tokens"][r, t + 1] = want["next"][r] = tok
                want["length"][r] += 1
                want["sum_logp"][r] += lp
                if with_lp:
                    want["tok_logp"][r, t + 1] = lp
                if tok == eos:
                    want["finished"][r] = 1
                    want["live"][0] -= 1
            assert int(want["finished"][4]) == 1 and int(want["live"][0]) == 3
            for k in keys:
                if want[k].is_floating_point():
                    assert float((o[tag + k].double() - want[k].double()).abs().max()) <= lp_tol + 1e-6, (tag, k)
                    untouched = o[tag + k].double() == init[k].double()
                    assert bool(untouched[want[k] == init[k]].all()), (tag, k)        # what the step does not own keeps its bits
                else:
                    assert torch.equal(o[tag + k], want[k]), (tag, k)
        return []
    return verify


# -------------------------------------------------------------------------------------------------------------- n1, n2
@case("singa_knn_graph")
def knn_graph(ar, E):
    """molecules smaller than k + 1 atoms (-1 slots), a single atom, an empty molecule, atoms of no molecule (all -1)"""
    g = gen(280)
    sizes, k, extra = [20, 5, 1, 0, 9], 6, 3
    B, n_real = len(sizes), sum(sizes)
    N = n_real + extra
    pos = ru(g, N, 3) * 30.0
    batch = torch.cat([torch.repeat_interleave(torch.arange(B), torch.tensor(sizes)), torch.full((extra,), B)])
    ptr = torch.tensor([0] + sizes).cumsum(0)
    want_r, want_c = torch.full((N, k), -1, dtype=I64), torch.full((N, k), -1, dtype=I64)
    for b in range(B):
        ids = torch.arange(int(ptr[b]), int(ptr[b + 1]))
        if ids.numel() == 0:
            continue
        d = torch.cdist(pos[ids].double(), pos[ids].double())
        d.fill_diagonal_(float("inf"))
        srt, order = torch.sort(d, 1)
        kk = min(k, ids.numel() - 1)
        assert ids.numel() == 1 or float((srt[:, 1:kk + 1] - srt[:, :kk]).min()) > 1e-4        # no near ties: the order is decided
        want_r[ids, :kk] = ids.unsqueeze(1)
        want_c[ids, :kk] = ids[order[:, :kk]]
    vp, vb, vptr = ar.view("pos", pos.shape, data=pos), ar.view("batch", (N,), I32, data=batch), ar.view("ptr", (B + 1,), I64, data=ptr)
    row, col = ar.view("row", (N * k,), I64, role="out"), ar.view("col", (N * k,), I64, role="out")
    E.ok(E.lib.singa_knn_graph(p(vp), p(vb), p(vptr), B, N, k, 24, p(row), p(col), E.st), "knn_graph")

    def verify(o):
        assert torch.equal(o["row"].view(N, k), want_r) and torch.equal(o["col"].view(N, k), want_c)
        return []
    return verify


@case("singa_knn_edge_attr")
def knn_edge_attr(ar, E):
    """nodes without edges, a heavy node, inert padding edges behind the n_real real ones: their rows are written as zeros"""
    g = gen(281)
    N, n_real, extra, G = 11, 150, 9, 64
    row = holes(g, N - 2, n_real)
    row[40:90] = 4
    row = torch.cat([torch.sort(row).values, torch.full((extra,), N - 2)])
    ln = ru(g, n_real) * 14.0
    offset = torch.linspace(0, 15, G)
    coeff = -0.5 / float(offset[1] - offset[0]) ** 2
    seg = torch.searchsorted(row, torch.arange(N + 1)).to(I32)
    E0 = row.numel()
    vl, vs, vo = ar.view("len", ln.shape, data=ln), ar.view("ptr", (N + 1,), I32, data=seg), ar.view("offset", (G,), data=offset)
    out = ar.view("out", (E0 + N, G), role="out")
    E.ok(E.lib.singa_knn_edge_attr(p(vl), p(vs), n_real, p(vo), coeff, p(out), N, G, E.st), "knn_edge_attr")

    def verify(o):
        ea = torch.cat([torch.exp(coeff * (d64(ln).unsqueeze(1) - d64(offset)) ** 2), torch.zeros(extra, G, dtype=F64)])
        deg = torch.zeros(N, G, dtype=F64).index_add_(0, row, ea)
        order = torch.argsort(torch.cat([row, torch.arange(N)]), stable=True)
        want = torch.cat([-ea, deg])[order]
        pad_rows = (order >= n_real) & (order < E0)
        assert int(pad_rows.sum()) == extra and float(o["out"][pad_rows].abs().max()) == 0.0
        return [("out", o["out"], want, 2e-6)]
    return verify


@case("singa_lap_pe")
def lap_pe(ar, E):
    """Graphs with fewer than kout + 1 atoms (zero columns), a single atom, a graph without edges, a graph of no atoms; A and
    work are uninitialised scratch; rows of `out` that belong to no graph (one lies between two graphs here) are not written."""
    from tests.test_kernels_gpu import _lap_np, _sym_edges
    kout, ld = 8, 23
    graphs = [(21, _sym_edges([(i, i + 1) for i in range(20)] + [(0, 7), (3, 15)])), (5, _sym_edges([(0, 1), (1, 2), (3, 4)])),
              (1, np.zeros((2, 0), np.int64)), (4, np.zeros((2, 0), np.int64)), (0, np.zeros((2, 0), np.int64)),
              (9, _sym_edges([(i, i + 1) for i in range(8)]))]
    B = len(graphs)
    first, off = [], 0
    for i, (n, _) in enumerate(graphs):
        first.append(off)
        off += n + (1 if i == 1 else 0)                               # one row of no graph behind graph 1
    total = off
    esrc = np.concatenate([e[0] for _, e in graphs]).astype(np.int32)
    edst = np.concatenate([e[1] for _, e in graphs]).astype(np.int32)
    eptr = np.concatenate([[0], np.cumsum([e.shape[1] for _, e in graphs])]).astype(np.int32)
    promised = torch.zeros(total, kout, dtype=torch.bool)
    for f, (n, _) in zip(first, graphs):
        promised[f:f + n] = True
    v = _views(ar, [("esrc", torch.tensor(esrc) if len(esrc) else torch.zeros(1, dtype=I32)), ("edst", torch.tensor(edst)),
                    ("eptr", torch.tensor(eptr)), ("nnodes", torch.tensor([n for n, _ in graphs], dtype=I32)),
                    ("first", torch.tensor(first, dtype=I32))])
    A = ar.view("A", (B, ld, ld), F64, role="scratch")
    work = ar.view("work", (max(E.lib.singa_lap_pe_work(B, ld), 1),), F64, role="scratch")
    out = ar.view("out", (total, kout), role="out", promised=promised)
    E.ok(E.lib.singa_lap_pe(p(A), p(v["esrc"]), p(v["edst"]), p(v["eptr"]), p(v["nnodes"]), p(v["first"]), p(work), p(out), B, ld, kout,
                            E.st), "lap_pe")

    def verify(o):
        pe = o["out"].double().numpy()
        for f, (n, e) in zip(first, graphs):
            if n == 0:
                continue
            vv = pe[f:f + n]
            kk = min(kout, n - 1)
            assert np.abs(vv[:, kk:]).max(initial=0.0) == 0.0                      # columns the graph is too small for: zeros
            if kk == 0:
                continue
            lap = _lap_np(e, n)
            w = np.linalg.eigvalsh(lap)
            vv = vv[:, :kk]
            assert np.abs(vv.T @ vv - np.eye(kk)).max() < 2e-6, n
            ritz = vv.T @ lap @ vv
            assert np.abs(lap @ vv - vv @ ritz).max() < 2e-6, n
            assert np.abs(np.linalg.eigvalsh(ritz) - w[1:kk + 1]).max() < 2e-6, n
            assert (vv.max(0) >= (-vv).max(0) - 1e-6).all()
        return []
    return verify


# ------------------------------------------------------------------------------------------------- optimizer kernels
def _chunk_table(sizes, chunk):
    ct, co = [], []
    for i, n in enumerate(sizes):
        for o_ in range(0, n, chunk):
            ct.append(i)
            co.append(o_)
    return torch.tensor(ct, dtype=I32), torch.tensor(co, dtype=I64)


@case("singa_adam_step")
def adam_step(ar, E):
    """p, m, v and the step count are accumulators: all start from known non-zero contents (step = 3)"""
    g = gen(290)
    sizes, chunk = [5, 1030, 257], 256
    ct, co = _chunk_table(sizes, chunk)
    b1, b2, eps, lr, step = 0.9, 0.999, 1e-8, 1e-3, 3.0
    T = {k: [rn(g, n) * s + o_ for n in sizes] for k, s, o_ in (("p", 1.0, 0.0), ("g", 0.1, 0.0), ("m", 0.05, 0.0))}
    T["v"] = [ru(g, n) * 1e-2 for n in sizes]
    vt = {k: [ar.view(f"{k}{i}", t.shape, data=t, role="in" if k == "g" else "inout") for i, t in enumerate(ts)] for k, ts in T.items()}
    tabs = {k: ar.view(k + "_ptrs", (len(sizes),), I64, data=[v_.ptr for v_ in vs]) for k, vs in vt.items()}
    vsz, vct, vco = ar.view("sizes", (len(sizes),), I64, data=sizes), ar.view("ct", ct.shape, I32, data=ct), ar.view("co", co.shape, I64, data=co)
    vstep, vlr = ar.view("step", (1,), data=[step], role="inout"), ar.view("lr", (1,), data=[lr])
    E.ok(E.lib.singa_adam_step(p(tabs["p"]), p(tabs["g"]), p(tabs["m"]), p(tabs["v"]), p(vsz), p(vct), p(vco), len(ct), chunk, p(vstep),
                               p(vlr), b1, b2, eps, E.st), "adam_step")

    def verify(o):
        assert float(o["step"][0]) == step + 1
        rows = []
        k = step + 1
        for i in range(len(sizes)):
            p0, g0, m0, v0 = (d64(T[key][i]) for key in "pgmv")
            m1, v1 = b1 * m0 + (1 - b1) * g0, b2 * v0 + (1 - b2) * g0 * g0
            p1 = p0 - float(torch.tensor(lr)) / (1 - b1 ** k) * m1 / (v1.sqrt() / math.sqrt(1 - b2 ** k) + eps)
            rows += [(f"p{i}", o[f"p{i}"], p1, 1e-6), (f"m{i}", o[f"m{i}"], m1, 1e-6), (f"v{i}", o[f"v{i}"], v1, 1e-6)]
        return rows
    return verify


@case("singa_grad_norm")
def grad_norm(ar, E):
    """partial (nchunks floats) is uninitialised scratch"""
    g = gen(291)
    sizes, chunk = [5, 1030, 257], 256
    ct, co = _chunk_table(sizes, chunk)
    gs = [rn(g, n) for n in sizes]
    vg = [ar.view(f"g{i}", t.shape, data=t) for i, t in enumerate(gs)]
    tab = ar.view("g_ptrs", (len(sizes),), I64, data=[v_.ptr for v_ in vg])
    vsz, vct, vco = ar.view("sizes", (len(sizes),), I64, data=sizes), ar.view("ct", ct.shape, I32, data=ct), ar.view("co", co.shape, I64, data=co)
    part, out = ar.view("partial", (len(ct),), role="scratch"), ar.view("out", (1,), role="out")
    E.ok(E.lib.singa_grad_norm(p(tab), p(vsz), p(vct), p(vco), len(ct), chunk, p(part), p(out), E.st), "grad_norm")
    return lambda o: [("norm", o["out"], torch.cat([d64(t) for t in gs]).norm().view(1), 1e-6)]


# ------------------------------------------------------------------------------------------------------ k7 / k11, k7c
def small_ints(g, *shape):
    return torch.randint(-3, 4, shape, generator=g).float()


@case("singa_gemm_f32")
def gemm_f32(ar, E):
    """All three operand forms on small integers (exact in any summation order, as in tests/test_gemm_gpu.py: equality):
    (1, 1) with row-pitched A and B, C in groups of 5 rows (ldc > J, c_group_ld > 5 ldc), bias, an addend at C's pitches, relu;
    (1, 0) with ldc > J and a mask at the same pitch;  (0, 0) in one piece with ldc > J, and with splits = 3, whose slabs the
    header makes dense (ldc = J), c_split_stride > I * J apart, asum_stride > I.  Both macro-tile shapes."""
    g = gen(300)
    M, N, K, S = 130, 40, 36, 3
    x, w, b, dy, ad, hm = small_ints(g, M, K), small_ints(g, N, K), small_ints(g, N), small_ints(g, M, N), small_ints(g, M, N), small_ints(g, M, K)
    vx = ar.view("x", x.shape, strides=(K + 4, 1), data=x)
    vw = ar.view("w", w.shape, strides=(K + 8, 1), data=w)
    vb = ar.view("b", b.shape, data=b)
    vdy = ar.view("dy", dy.shape, strides=(N + 4, 1), data=dy)
    ldc, grp = N + 4, 5
    gld = grp * ldc + 8
    gshape, gstr = (M // grp, grp, N), (gld, ldc, 1)
    vad = ar.view("addend", gshape, strides=gstr, data=ad.view(gshape))
    vhm = ar.view("mask", hm.shape, strides=(K + 12, 1), data=hm)
    try:
        for cfg in (0, 3):
            E.ok(E.lib.singa_gemm_force_cfg(cfg), "force_cfg")
            t = f"cfg{cfg}."
            y = ar.view(t + "y", gshape, strides=gstr, role="out")
            arr, n = _capi.gemm_probs([dict(a=vx.ptr, lda=K + 4, b=vw.ptr, ldb=K + 8, c=y.ptr, ldc=ldc, I=M, J=N, R=K, c_group=grp,
                                            c_group_ld=gld, bias=vb.ptr, addend=vad.ptr, relu=1)])
            E.ok(E.lib.singa_gemm_f32(arr, n, 1, 1, 1, E.st), "gemm (1,1)")
            dx = ar.view(t + "dx", (M, K), strides=(K + 12, 1), role="out")
            arr, n = _capi.gemm_probs([dict(a=vdy.ptr, lda=N + 4, b=vw.ptr, ldb=K + 8, c=dx.ptr, ldc=K + 12, I=M, J=K, R=N, mask=vhm.ptr)])
            E.ok(E.lib.singa_gemm_f32(arr, n, 1, 0, 1, E.st), "gemm (1,0)")
            slabs = ar.view(t + "dw", (S, N, K), strides=(N * K + 16, K, 1), role="out")
            asum = ar.view(t + "asum", (S, N), strides=(N + 4, 1), role="out")
            arr, n = _capi.gemm_probs([dict(a=vdy.ptr, lda=N + 4, b=vx.ptr, ldb=K + 4, c=slabs.ptr, ldc=K, I=N, J=K, R=M,
                                            c_split_stride=N * K + 16, asum=asum.ptr, asum_stride=N + 4)])
            E.ok(E.lib.singa_gemm_f32(arr, n, 0, 0, S, E.st), "gemm (0,0)")
            dw1, asum1 = ar.view(t + "dw1", (N, K), strides=(K + 8, 1), role="out"), ar.view(t + "asum1", (N,), role="out")
            arr, n = _capi.gemm_probs([dict(a=vdy.ptr, lda=N + 4, b=vx.ptr, ldb=K + 4, c=dw1.ptr, ldc=K + 8, I=N, J=K, R=M,
                                            asum=asum1.ptr, asum_stride=N)])
            E.ok(E.lib.singa_gemm_f32(arr, n, 0, 0, 1, E.st), "gemm (0,0), one split")
    finally:
        E.lib.singa_gemm_force_cfg(-1)

    def verify(o):
        for cfg in (0, 3):
            t = f"cfg{cfg}."
            assert torch.equal(o[t + "y"].reshape(M, N), torch.relu(x @ w.t() + b + ad)), t
            assert torch.equal(o[t + "dx"], (dy @ w) * (hm > 0)), t
            assert torch.equal(o[t + "dw"].sum(0), dy.t() @ x) and torch.equal(o[t + "asum"].sum(0), dy.sum(0)), t
            assert torch.equal(o[t + "dw1"], dy.t() @ x) and torch.equal(o[t + "asum1"], dy.sum(0)), t
        return []
    return verify


@case("singa_cgemm3m_f32")
def cgemm3m_f32(ar, E):
    """All three forms on small integers (exact: equality), every operand row-pitched, the imaginary parts a_im / b_im / c_im
    elements behind the real ones, (0, 0) in one piece with ldc > J, and with splits = 3 as dense slabs c_split_stride > 2 I J
    apart."""
    g = gen(310)
    M, N, K, S = 130, 36, 20, 3
    x, w, dy = small_ints(g, M, 2 * K), small_ints(g, 2 * N, K), small_ints(g, M, 2 * N)
    lx, lw, ly = 2 * K + 4, K + 4, 2 * N + 8
    vx, vw, vdy = ar.view("x", x.shape, strides=(lx, 1), data=x), ar.view("w", w.shape, strides=(lw, 1), data=w), \
        ar.view("dy", dy.shape, strides=(ly, 1), data=dy)
    y = ar.view("y", (M, 2 * N), strides=(2 * N + 4, 1), role="out")
    arr, n = _capi.gemm_probs([dict(a=vx.ptr, lda=lx, a_im=K, b=vw.ptr, ldb=lw, b_im=N * lw, c=y.ptr, ldc=2 * N + 4, c_im=N, I=M, J=N, R=K,
                                    sigma=1.0)], _capi.CGemm)
    E.ok(E.lib.singa_cgemm3m_f32(arr, n, 1, 1, 1, E.st), "cgemm (1,1)")
    dx = ar.view("dx", (M, 2 * K), strides=(2 * K + 12, 1), role="out")
    arr, n = _capi.gemm_probs([dict(a=vdy.ptr, lda=ly, a_im=N, b=vw.ptr, ldb=lw, b_im=N * lw, c=dx.ptr, ldc=2 * K + 12, c_im=K, I=M, J=K,
                                    R=N, sigma=-1.0)], _capi.CGemm)
    E.ok(E.lib.singa_cgemm3m_f32(arr, n, 1, 0, 1, E.st), "cgemm (1,0)")
    slabs = ar.view("dw", (S, 2 * N, K), strides=(2 * N * K + 16, K, 1), role="out")
    arr, n = _capi.gemm_probs([dict(a=vdy.ptr, lda=ly, a_im=N, b=vx.ptr, ldb=lx, b_im=K, c=slabs.ptr, ldc=K, c_im=N * K, I=N, J=K, R=M,
                                    sigma=-1.0, c_split_stride=2 * N * K + 16)], _capi.CGemm)
    E.ok(E.lib.singa_cgemm3m_f32(arr, n, 0, 0, S, E.st), "cgemm (0,0)")
    dw1 = ar.view("dw1", (2 * N, K), strides=(K + 8, 1), role="out")
    arr, n = _capi.gemm_probs([dict(a=vdy.ptr, lda=ly, a_im=N, b=vx.ptr, ldb=lx, b_im=K, c=dw1.ptr, ldc=K + 8, c_im=N * (K + 8), I=N, J=K,
                                    R=M, sigma=-1.0)], _capi.CGemm)
    E.ok(E.lib.singa_cgemm3m_f32(arr, n, 0, 0, 1, E.st), "cgemm (0,0), one split")

    def verify(o):
        xr, xi, wr, wi, gr, gi = x[:, :K], x[:, K:], w[:N], w[N:], dy[:, :N], dy[:, N:]
        assert torch.equal(o["y"], torch.cat([xr @ wr.t() - xi @ wi.t(), xr @ wi.t() + xi @ wr.t()], 1))
        assert torch.equal(o["dx"], torch.cat([gr @ wr + gi @ wi, gi @ wr - gr @ wi], 1))
        want_dw = torch.cat([gr.t() @ xr + gi.t() @ xi, gi.t() @ xr - gr.t() @ xi], 0)
        assert torch.equal(o["dw"].sum(0), want_dw) and torch.equal(o["dw1"], want_dw)
        return []
    return verify


# ------------------------------------------------------------------------------------------------------------ the tests
# Entry points without a case: closed.  Only functions that enqueue nothing, and the measurement and tuning knobs.
EXEMPT = {
    "singa_version", "singa_last_error_string", "singa_init", "singa_dims",
    # sizers
    "singa_alpha_logits_nslots", "singa_ln256_nparts", "singa_ln_silu_nparts", "singa_so3_rmsnorm_nparts", "singa_edge_mlp_bwd_nparts",
    "singa_so3_skinny_nparts", "singa_rowdot_nparts", "singa_colsum_work", "singa_colsum_multi_work", "singa_lap_pe_work",
    # measurement
    "singa_prof_enable", "singa_prof_hint_edges", "singa_prof_collect", "singa_prof_collect_tagged", "singa_prof_stamps",
    "singa_prof_read_stamps", "singa_prof_reset", "singa_calib_copy", "singa_calib_copy16",
    # the force / variant / threshold setters the existing tests use
    "singa_so3_skinny_variant", "singa_gemm_occupancy", "singa_gemm_force_cfg", "singa_lap_pe_fsi_min",
}


def test_every_entry_point_has_a_case():
    bound = set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS)
    covered = {e for _, entries in CASES.values() for e in entries}
    assert covered <= bound, sorted(covered - bound)
    assert not covered & EXEMPT, sorted(covered & EXEMPT)
    assert EXEMPT <= bound, sorted(EXEMPT - bound)
    missing = bound - covered - EXEMPT
    assert not missing, f"C ABI entry points without a footprint case: {sorted(missing)}"
    for name in EXEMPT:                                     # the list stays what it says it is
        assert name in ("singa_version", "singa_last_error_string", "singa_init", "singa_dims") or name.endswith(
            ("_nparts", "_nslots", "_work")) or name.startswith(("singa_prof_", "singa_calib_")) or name in _capi.LAB_EXPORTS, name


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_footprint(name):
    run_case(name)
