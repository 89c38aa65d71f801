"""The optimizer update in float64 - torch.optim.Adam's rule without weight decay and amsgrad (reference utils/misc.py
get_optimizer, train.py:126-127) - the per-element criterion every optimizer test holds a step to, and the case table the
kernel tests (tests/test_adam_cpu.py on the sequential CPU build, tests/test_adam_gpu.py on the device) share.

    m' = b1 m + (1 - b1) g,   v' = b2 v + (1 - b2) g^2,   p' = p - lr / (1 - b1^k) * m' / (sqrt(v') / sqrt(1 - b2^k) + eps)

with k the step count AFTER the step.  `expected` evaluates it with the float32-ROUNDED b1, b2, eps and lr, because those are
what the C ABI receives (three float arguments and a float device scalar): measured on the CPU build of the kernel, the
float64 rule with exact against float32-rounded betas differs by up to 6e-6 of the update at k = 2 ... 1000 (b2 = 0.999 is
0.99900001287 in float32, and 1 - b2^k amplifies that) - more than the kernel's own error.  exact=True keeps the given values:
that form equals torch.optim.Adam on float64 parameters (tests/test_adam_cpu.py).

The bound on the update is derived, not tuned (`update_bound`); where it leaves the issue's plain relative form the reason is
written at `check_step`."""
import ctypes
import math

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24                                           # largest relative error of one float32 rounding


def f32(x):
    return float(np.float32(x))


def hyper(lr, betas, eps, exact=False):
    if exact:
        return float(lr), float(betas[0]), float(betas[1]), float(eps)
    return f32(lr), f32(betas[0]), f32(betas[1]), f32(eps)


def expected(p, g, m, v, k, lr, betas, eps, exact=False):
    """(p', m', v', delta = p' - p) of one step that ends at step count k; float64 tensors in and out."""
    lr, b1, b2, eps = hyper(lr, betas, eps, exact)
    p, g, m, v = (torch.as_tensor(t).to(F64) for t in (p, g, m, v))
    m1 = b1 * m + (1.0 - b1) * g
    v1 = b2 * v + (1.0 - b2) * g * g
    delta = -(lr / (1.0 - b1 ** k)) * m1 / (v1.sqrt() / math.sqrt(1.0 - b2 ** k) + eps)
    return p + delta, m1, v1, delta


def update_bound(k, betas):
    """Relative error of the float32 kernel's update: 2^-23 * (1 / (1 - b1^k) + 1/2 / (1 - b2^k) + 8).  The only
    ill-conditioned operations in the kernel are 1 - powf(b, k): an error of one ulp of a value below 1 (2^-24 ... 2^-23),
    divided by the difference; the root halves b2's share.  The 8 covers the seven remaining roundings (m', v', the root, two
    divisions, + eps, the product with the step size), each 2^-24, with v''s halved.  (0.99, 0.999): 7e-5 at k = 1, 3.7e-5 at
    k = 2, 1.1e-6 once both powers are negligible."""
    b1, b2 = f32(betas[0]), f32(betas[1])
    return 2.0 ** -23 * (1.0 / (1.0 - b1 ** k) + 0.5 / (1.0 - b2 ** k) + 8.0)


MOMENT_BOUND = 4 * U
FLUSH = 2.0 ** -126                                      # float32's smallest normal: the device flushes smaller results to zero


def ulp32(x):
    """Spacing of float32 at the float64 values x (0 at 0; the subnormal spacing below the normal range)."""
    x32 = x.to(torch.float32).abs()
    _, e = torch.frexp(x32)                                # x32 = mantissa in [0.5, 1) * 2^e
    ulp = torch.ldexp(torch.ones_like(x), (e - 24).clamp_min(-149).to(torch.int32))
    return torch.where(x32 == 0, torch.zeros_like(x), ulp)


def _flat(ts, dev):
    ts = [torch.as_tensor(t).detach().to(dev).reshape(-1) for t in ts]
    return torch.cat(ts).to(F64) if ts else torch.zeros(0, dtype=F64, device=dev)


def check_step(before, after, grad, k, lr, betas=(0.99, 0.999), eps=1e-8, label="", do_assert=True):
    """The per-element assertion.  before / after: {name: (p, m, v)} around ONE optimizer step, grad: {name: g} the step
    consumed, k the step count after it, lr the rate in force.  Element-wise, against `expected` on the float32 inputs:

      |m_after - m'| <= 4 * 2^-24 * (b1 |m| + (1 - b1) |g|)      (measured on the CPU build: 1.5e-7)
      |v_after - v'| <= 4 * 2^-24 * v'
      |p_after - (p + delta)| <= 1/2 ulp32(p + delta) + update_bound(k) * |delta| * (b1 |m| + (1 - b1) |g|) / |m'|

    The first term of the last line is the unavoidable final rounding into p: it dominates for parameters of O(1) and
    vanishes for zero-initialised biases, where the second term is what is tested.  b1 |m| + (1 - b1) |g| IS |m'| - and the
    three bounds are plainly relative, 4 * 2^-24 and update_bound(k) - whenever g and m do not have opposite signs (always at
    k = 1).  Where they do, m' is a difference of two float32 products: no float32 evaluation of it (torch's lerp included)
    has an error relative to the result, only to its terms, and delta, linear in m', inherits that factor - so the bounds
    there are relative to the terms.  v' is a sum of non-negative terms.

    Underflow: this model's gradients reach 1e-20 and below (the key biases of the dense attentions are rounding noise), so
    (1 - b2) g^2 leaves float32's normal range, where a rounding error is no longer relative and the device flushes to zero
    (measured on an MI355X without these terms: elements of exp_avg and exp_avg_sq of the attention's weight_k_net /
    weight_v_net whose error EQUALLED the expected value - the kernel had stored 0).  Each moment is at most four such results, so m and
    v get the absolute term 4 * 2^-126, and p what follows from it: lr / (1 - b1^k) * 4 * 2^-126 / D through m', |delta| *
    sqrt(4 * 2^-126 / (1 - b2^k)) / D through the root of v', with D = sqrt(v') / sqrt(1 - b2^k) + eps, and 2^-126 for the
    update itself.  All of it is below 5e-38 * max(1, lr / eps): nothing for any element a test could otherwise fail on.

    Prints the worst tensor, element and ratio (error / bound) of p, m and v in the manner of helpers.rowwise_err, and the
    largest plainly relative errors; returns them; asserts all three ratios <= 1."""
    names = list(grad)
    assert names and set(before) == set(after) == set(names)
    dev = torch.as_tensor(grad[names[0]]).device
    lr32, b1, b2, _ = hyper(lr, betas, eps)
    sizes = [int(torch.as_tensor(grad[n]).numel()) for n in names]
    g = _flat([grad[n] for n in names], dev)
    p0, m0, v0 = (_flat([before[n][i] for n in names], dev) for i in range(3))
    p1, m1, v1 = (_flat([after[n][i] for n in names], dev) for i in range(3))
    assert p0.numel() == g.numel() == m0.numel() == v0.numel() == p1.numel() == m1.numel() == v1.numel() == sum(sizes)
    wp, wm, wv, delta = expected(p0, g, m0, v0, k, lr, betas, eps)
    terms = b1 * m0.abs() + (1.0 - b1) * g.abs()
    cond = torch.where(wm == 0, torch.ones_like(wm), terms / wm.abs().clamp_min(1e-300))
    tiny = 1e-300
    den = (wv.sqrt() / math.sqrt(1.0 - b2 ** k) + f32(eps)).clamp_min(tiny)
    under_p = FLUSH + (lr32 / (1.0 - b1 ** k)) * 4 * FLUSH / den + delta.abs() * cond * (math.sqrt(4 * FLUSH / (1.0 - b2 ** k)) / den)
    bounds = {"p": 0.5 * ulp32(wp) + update_bound(k, betas) * delta.abs() * cond + under_p, "m": MOMENT_BOUND * terms + 4 * FLUSH,
              "v": MOMENT_BOUND * wv + 4 * FLUSH}
    errs = {"p": (p1 - wp).abs(), "m": (m1 - wm).abs(), "v": (v1 - wv).abs()}
    starts = np.concatenate([[0], np.cumsum(sizes)])
    out = {"k": k}
    for key in ("p", "m", "v"):
        err, bound = errs[key], bounds[key]
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))           # NaN / inf: a failure
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(tiny))         # (bound 0: exact or a failure)
        i = int(ratio.argmax()) if ratio.numel() else 0
        t = int(np.searchsorted(starts, i, side="right") - 1)
        out[key] = float(ratio[i]) if ratio.numel() else 0.0
        out[key + "_at"] = (names[t], i - int(starts[t]))
        if ratio.numel():
            out[key + "_got_want"] = (float({"p": p1, "m": m1, "v": v1}[key][i]), float({"p": wp, "m": wm, "v": wv}[key][i]))
    # the plainly relative figures: where m' is no difference and every quantity is well inside the normal range; the
    # update's where p starts from exactly 0 (p after the step is then the update in full float32 precision)
    plain = ((g * m0) >= 0) & (wv > 2.0 ** -100) & (wm.abs() > 2.0 ** -100)
    worst = lambda e, w, sel: float((e[sel] / w[sel]).max()) if bool(sel.any()) else 0.0
    out["rel_update"] = worst(errs["p"], delta.abs(), plain & (p0 == 0) & (delta.abs() > 2.0 ** -100))
    out["rel_m"], out["rel_v"] = worst(errs["m"], wm.abs(), plain), worst(errs["v"], wv, plain)
    out["opposed"] = int(((g * m0) < 0).sum())
    print(f"{label} k={k} lr={lr32:.3e}: error/bound p {out['p']:.3f} at {out['p_at']}, m {out['m']:.3f} at {out['m_at']}, "
          f"v {out['v']:.3f} at {out['v_at']}; relative: update from p = 0 {out['rel_update']:.2e}, m {out['rel_m']:.2e}, "
          f"v {out['rel_v']:.2e}; update bound {update_bound(k, betas):.2e}; {out['opposed']} of {g.numel()} elements with g m < 0, "
          f"{int((p0 == 0).sum())} with p = 0, {int((wv < FLUSH).sum() - (wv == 0).sum())} with 0 < v' < 2^-126")
    if do_assert:
        assert out["p"] <= 1.0 and out["m"] <= 1.0 and out["v"] <= 1.0, (label, out)
    return out


# ------------------------------------------------------------------------------------------------ the kernel cases
CHUNK = 4096                                             # singa_amd.optim.CHUNK
SIZES = [1, 255, 256, 257, 0, 4095, 4096, 4097, 3 * 4096, 3 * 4096 + 1]       # (a tensor of size 0 among the others: no chunk)
STEP_COUNTS = [1, 2, 3, 10, 100, 1000, 100000]
BETAS = [(0.99, 0.999), (0.9, 0.999)]
EPS = [1e-8, 1e-6]
LRS = [1e-4, 1e-1]
GUARD = 1024
SENTINEL = 1.0e30


def chunk_table(sizes, chunk):
    """The (tensor, offset) work list exactly as singa_amd.optim.Adam._build makes it."""
    ct, co = [], []
    for i, n in enumerate(sizes):
        for off in range(0, n, chunk):
            ct.append(i)
            co.append(off)
    return ct, co


def log_uniform(rs, n, lo, hi, signed=True):
    x = 10.0 ** rs.uniform(math.log10(lo), math.log10(hi), n)
    return x * rs.choice([-1.0, 1.0], n) if signed else x


def make_state(seed, k, betas, p_normal, sizes=SIZES):
    """Flat float32 arrays p, g, m, v over all tensors laid end to end (every tensor's data ADJACENT to its neighbours', so
    a chunk that runs past its tensor's end lands in the next one), and the element classes:
      0  |g| signed log-uniform over 1e-12 ... 1e2 (straddles eps), history h = g * (0.5 ... 2): g and m of one sign
      1  as 0 with the sign of the history drawn independently: g and m may oppose
      2  g = m = v = 0 exactly: p must keep its bits
      3  g = 0, m, v != 0: the moments decay and p still moves
    Step count k is reached in ONE launch: the buffers hold step = k - 1 and the moments of a history of constant size,
    m = (1 - b1^(k-1)) h, v = (1 - b2^(k-1)) h^2 (zero at k = 1: the first step)."""
    rs = np.random.RandomState(seed)
    n = sum(sizes)
    cls = rs.choice([0, 1, 2, 3], n, p=[0.6, 0.2, 0.1, 0.1])
    cls[:8] = [0, 1, 2, 3, 3, 2, 1, 0]                          # (the one-element tensor and the next one's head: all classes)
    g = log_uniform(rs, n, 1e-12, 1e2)
    h = g * 10.0 ** rs.uniform(-0.3, 0.3, n)
    h = np.where(cls == 1, np.abs(h) * rs.choice([-1.0, 1.0], n), h)
    h = np.where(cls == 3, log_uniform(rs, n, 1e-12, 1e2), h)
    g = np.where(cls >= 2, 0.0, g)
    h = np.where(cls == 2, 0.0, h)
    b1, b2 = f32(betas[0]), f32(betas[1])
    m = (1.0 - b1 ** (k - 1)) * h
    v = (1.0 - b2 ** (k - 1)) * h * h
    p = rs.randn(n) if p_normal else np.zeros(n)
    return tuple(np.asarray(a, np.float32) for a in (p, g, m, v)) + (cls,)


def launch_adam(lib, dev, stream, state, k, lr, betas, eps, chunk, sizes=SIZES):
    """One singa_adam_step launch through the C ABI over `state` (make_state) on device `dev` -> (before, after, grad) as
    check_step takes them plus the step count read back; asserts the guard bands around the four allocations intact."""
    n = sum(sizes)
    bufs = {}
    for key, a in zip("pgmv", state[:4]):
        buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32)
        buf[GUARD:GUARD + n] = torch.from_numpy(a)
        bufs[key] = buf.to(dev)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    i64 = lambda xs: torch.tensor([int(x) for x in xs], dtype=torch.int64).to(dev)
    ptrs = {key: i64([b.data_ptr() + 4 * (GUARD + int(s)) for s in starts[:-1]]) for key, b in bufs.items()}
    ct, co = chunk_table(sizes, chunk)
    vct, vco, vsz = torch.tensor(ct, dtype=torch.int32).to(dev), i64(co), i64(sizes)
    step = torch.tensor([float(k - 1)], dtype=torch.float32).to(dev)
    lr_t = torch.tensor([lr], dtype=torch.float32).to(dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    code = lib.singa_adam_step(vp(ptrs["p"]), vp(ptrs["g"]), vp(ptrs["m"]), vp(ptrs["v"]), vp(vsz), vp(vct), vp(vco), len(ct),
                               chunk, vp(step), vp(lr_t), betas[0], betas[1], eps, stream)
    assert code == 0, (code, lib.singa_last_error_string())
    if torch.device(dev).type == "cuda":
        torch.cuda.synchronize()
    outs = {key: b.cpu() for key, b in bufs.items()}
    for key, b in outs.items():
        assert bool((b[:GUARD] == SENTINEL).all()) and bool((b[GUARD + n:] == SENTINEL).all()), f"guard band of {key} written"
    assert torch.equal(outs["g"][GUARD:GUARD + n], torch.from_numpy(state[1])), "the gradient was modified"
    cut = lambda a: {f"t{i}": a[int(s):int(e)] for i, (s, e) in enumerate(zip(starts[:-1], starts[1:]))}
    b4 = [cut(torch.from_numpy(a)) for a in state[:4]]
    af = {key: cut(outs[key][GUARD:GUARD + n]) for key in "pmv"}
    before = {t: (b4[0][t], b4[2][t], b4[3][t]) for t in b4[0]}
    after = {t: (af["p"][t], af["m"][t], af["v"][t]) for t in b4[0]}
    return before, after, b4[1], float(step.cpu()[0])


def run_kernel_cases(lib, dev, stream, k, betas):
    """Every (eps, lr, chunk, initial p) combination at one (k, betas): check_step on each launch, the exact-zero and the
    g = 0 classes, the step count.  Returns the largest plainly relative errors of the update (p0 = 0 launches: p after the
    launch IS the update in full float32 precision) and of the moments."""
    worst = {"rel_update": 0.0, "rel_m": 0.0, "rel_v": 0.0, "p": 0.0}
    seed = 1000 * BETAS.index(tuple(betas)) + STEP_COUNTS.index(k)
    for p_normal in (False, True):
        state = make_state(seed, k, betas, p_normal)
        cls = torch.from_numpy(state[4])
        for eps in EPS:
            for lr in LRS:
                for chunk in (CHUNK, 256):
                    before, after, grad, step = launch_adam(lib, dev, stream, state, k, lr, betas, eps, chunk)
                    label = f"betas={betas} eps={eps:g} chunk={chunk} p0={'N(0,1)' if p_normal else '0'}"
                    assert step == float(k), (label, step)
                    r = check_step(before, after, grad, k, lr, betas, eps, label=label)
                    cat = lambda d, i: torch.cat([d[t][i] for t in d])
                    p0, p1, m1, v1 = cat(before, 0), cat(after, 0), cat(after, 1), cat(after, 2)
                    zero = cls == 2
                    assert torch.equal(p1[zero].view(torch.int32), p0[zero].view(torch.int32)), label     # bit for bit
                    assert float(m1[zero].abs().max()) == 0.0 and float(v1[zero].abs().max()) == 0.0, label
                    if k > 1 and not p_normal:
                        decay = cls == 3
                        assert bool((p1[decay] != 0).all()), label                    # g = 0, m != 0: p still moves
                        assert bool((m1[decay].abs() < cat(before, 1)[decay].abs()).all()), label
                    if not p_normal:
                        worst["rel_update"] = max(worst["rel_update"], r["rel_update"])
                    for key in ("rel_m", "rel_v", "p"):
                        worst[key] = max(worst[key], r[key])
    print(f"betas={betas} k={k}: worst relative error of the update {worst['rel_update']:.2e} (bound {update_bound(k, betas):.2e}), "
          f"of m {worst['rel_m']:.2e}, of v {worst['rel_v']:.2e}")
    return worst
