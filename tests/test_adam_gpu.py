"""-m gpu: singa_adam_step on the device against the float64 rule of tests/adam_rule.py, per element, through the C ABI - the
case table of tests/test_adam_cpu.py (see there), where powf is the device library's - and singa_grad_norm (workgroup-
synchronised: device only) against the float64 norm.

Measured, largest relative error of the update from p = 0 per k, both betas (CPU build / MI355X):
    k        1        2        3        10       100      1000     100000
    CPU      2.6e-7   3.7e-6   3.3e-6   4.0e-7   3.4e-7   3.1e-7   2.5e-7
    MI355X   2.6e-7   3.7e-6   3.5e-6   4.0e-7   3.4e-7   3.1e-7   2.5e-7
    bound    7.2e-5   3.7e-5   2.5e-5   8.2e-6   1.8e-6   1.2e-6   1.1e-6     (betas (0.99, 0.999); (0.9, 0.999): 6.2e-5 ... 1.1e-6)
(the device library's powf shows at k = 3, betas (0.9, 0.999) only: 3.49e-6 against 3.28e-6; every other figure agrees to the
digits printed).  Moments, CPU and MI355X alike: m 1.1e-7, v 1.3e-7 (bound 2.4e-7).  Norm, over the 24 cases below: largest
relative error 4.2e-8, exact on the one-large-element and the all-zero contents (bound 1e-6).
The bounds are adam_rule's derived ones, not these figures."""
import ctypes

import numpy as np
import pytest
import torch

from tests import adam_rule as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def lib():
    from singa_amd import _lib
    _lib.ensure_init(torch.cuda.current_device())
    return _lib.lib()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("betas", R.BETAS)
@pytest.mark.parametrize("k", R.STEP_COUNTS)
def test_adam_kernel_against_the_rule(lib, k, betas):
    R.run_kernel_cases(lib, DEV, _stream(), k, betas)


# ------------------------------------------------------------------------------------------------ singa_grad_norm
NORM_BOUND = 1e-6        # the footprint case's and the clipping test's: a partial is at most chunk / 256 + 8 float32 additions of
#                          non-negative terms (17 + 8 at chunk 4096: 25 * 2^-24 = 1.5e-6 on the SQUARE), the finish runs in
#                          double precision, and the root halves the error: 7.5e-7
WIDE = [70001, 300]                                       # chunk 256: 276 partials, the finishing kernel's threads add two
SIZE_LISTS = {"edges_4096": (R.SIZES, 4096), "edges_256": (R.SIZES, 256), "wide_256": (WIDE, 256), "wide_4096": (WIDE, 4096),
              "256_chunks": ([255 * 256, 256], 256), "257_chunks": ([255 * 256, 255, 1], 256)}


def _contents(kind, n, seed):
    rs = np.random.RandomState(seed)
    if kind == "log_uniform":       # squares stay inside float32's normal range, sums below 3e38
        return R.log_uniform(rs, n, 1e-15, 1e15)
    if kind == "one_large":
        g = np.full(n, 1e-15) * rs.choice([-1.0, 1.0], n)
        g[rs.randint(n)] = 1e15
        return g
    if kind == "small":             # nothing dominates: every addition counts
        return R.log_uniform(rs, n, 1e-2, 1e0)
    assert kind == "zeros"
    return np.zeros(n)


def _grad_norm(lib, g, sizes, chunk):
    n = sum(sizes)
    buf = torch.full((n + 2 * R.GUARD,), R.SENTINEL, dtype=torch.float32)
    buf[R.GUARD:R.GUARD + n] = torch.from_numpy(g)
    buf = buf.to(DEV)
    starts = np.concatenate([[0], np.cumsum(sizes)])
    i64 = lambda xs: torch.tensor([int(x) for x in xs], dtype=torch.int64, device=DEV)
    ptrs = i64([buf.data_ptr() + 4 * (R.GUARD + int(s)) for s in starts[:-1]])
    ct, co = R.chunk_table(sizes, chunk)
    vct, vco, vsz = torch.tensor(ct, dtype=torch.int32, device=DEV), i64(co), i64(sizes)
    partial = torch.full((len(ct) + 64,), float("nan"), dtype=torch.float32, device=DEV)          # uninitialised scratch
    out = torch.full((1 + 64,), float("nan"), dtype=torch.float32, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    code = lib.singa_grad_norm(vp(ptrs), vp(vsz), vp(vct), vp(vco), len(ct), chunk, vp(partial), vp(out), _stream())
    assert code == 0, (code, lib.singa_last_error_string())
    torch.cuda.synchronize()
    assert bool(torch.isnan(partial[len(ct):]).all()) and bool(torch.isnan(out[1:]).all()), "written past partial / out"
    assert bool(torch.isfinite(partial[:len(ct)]).all())
    assert torch.equal(buf.cpu()[R.GUARD:R.GUARD + n], torch.from_numpy(g))
    return float(out[0]), len(ct)


@pytest.mark.parametrize("kind", ["log_uniform", "one_large", "small", "zeros"])
@pytest.mark.parametrize("table", list(SIZE_LISTS))
def test_grad_norm_against_float64(lib, table, kind):
    sizes, chunk = SIZE_LISTS[table]
    g = _contents(kind, sum(sizes), 11 + list(SIZE_LISTS).index(table)).astype(np.float32)
    got, nchunks = _grad_norm(lib, g, sizes, chunk)
    if table.endswith("_chunks"):
        assert nchunks == int(table.split("_")[0])
    if table == "wide_256":
        assert nchunks > 256 and sum(sizes) > 65536
    want = float(np.sqrt((g.astype(np.float64) ** 2).sum()))
    err = abs(got - want) / want if want else abs(got)
    print(f"grad_norm {table} {kind}: {nchunks} chunks, got {got!r}, float64 {want!r}, relative error {err:.2e}")
    if kind == "zeros":
        assert got == 0.0
    else:
        assert err <= NORM_BOUND, (got, want, err)
