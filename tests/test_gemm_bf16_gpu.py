"""-m gpu: singa_gemm_bf16 (k7b, include/singa_hip_bf16.h) through the C ABI - the real GEMM with operands rounded to bf16
inside the kernel and f32 accumulation.  Exact on small integers (bf16-exact operands, sums far below 2^24: any fragment or
transpose slip is an O(1) error against tolerance 0), the rounding rule against float64 products of bf16-rounded operands within
the f32 tests' own tolerance, the epilogue, asum bit-equal to singa_gemm_f32's, the argument errors and the write footprint.

Sizes: rows of a reduction-contiguous A are free (36, 130, 257); every extent that is an operand's or the result's contiguous
axis has to be a multiple of 4 floats (both entry points refuse anything else), so J - and I in the (0, 0) form - take 36, 132
and 260: ragged against every tile shape all the same."""
import pytest
import torch

from tests.test_gemm_gpu import FORMS, _f64, _tol, check, tile_shape  # noqa: F401  (tile_shape: the fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (36, 130, 257)
COLS = (36, 132, 260)
REDUCTIONS = (4, 28, 32, 36, 64, 100)       # the K tail alone; one, two and three K steps of 32, full and ragged


def _ints(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randint(-4, 5, s, generator=g).float()


def _floats(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def _rounded(t):
    return t.bfloat16().double()


def _problem(mk, form, I, J, R, S=1, edit=None):
    """One problem in the given operand form -> (record, the tensors it points to, [S, I, J] result pre-filled with NaN, float64
    product of the bf16-rounded operands).  edit(a, b): changes the host operands (a [I, R] or [R, I], b [J, R] or [R, J])."""
    a_rc, b_rc = form
    a, b = (mk(I, R) if a_rc else mk(R, I)), (mk(J, R) if b_rc else mk(R, J))
    if edit is not None:
        edit(a, b)
    ad, bd = a.to(DEV), b.to(DEV)
    out = torch.full((S, I, J), float("nan"), device=DEV)
    ref = (_rounded(a) if a_rc else _rounded(a).t()) @ (_rounded(b).t() if b_rc else _rounded(b))
    rec = dict(a=ad.data_ptr(), lda=ad.stride(0), b=bd.data_ptr(), ldb=bd.stride(0), c=out.data_ptr(), ldc=J, I=I, J=J, R=R,
               c_split_stride=I * J)
    return rec, (ad, bd), out, ref


def _bf16(recs, form, splits=1):
    from singa_amd import ops
    ops._gemm(recs, *form, splits, precision="bf16")


def _extents(form, narrow=None):
    """(I, J) pairs: ragged against the 128 x 128 and 64 x 64 tiles; narrow = "J" / "I": at most 32 columns / rows (the
    128 x 32 / 32 x 128 tiles)."""
    rows = ROWS if form[0] else COLS
    if narrow == "J":
        return [(rows[0], 20), (rows[2], 32)]
    if narrow == "I":
        return [(20, COLS[0]), (32, COLS[2])]
    return [(i, j) for i in rows for j in COLS]


@pytest.mark.parametrize("tile_shape", [0, 3], indirect=True)
@pytest.mark.parametrize("form", FORMS)
def test_exact_on_integers_128_and_64_tiles(form, tile_shape):
    mk = _ints(11 + tile_shape)
    for I, J in _extents(form):
        for R in REDUCTIONS:
            rec, keep, out, ref = _problem(mk, form, I, J, R)
            _bf16([rec], form)
            assert torch.equal(_f64(out[0]), ref), (I, J, R)


@pytest.mark.parametrize("narrow", ["J", "I"])
@pytest.mark.parametrize("form", FORMS)
def test_exact_on_integers_narrow_tiles(form, narrow):
    mk = _ints(13)
    for I, J in _extents(form, narrow):
        for R in REDUCTIONS:
            rec, keep, out, ref = _problem(mk, form, I, J, R)
            _bf16([rec], form)
            assert torch.equal(_f64(out[0]), ref), (I, J, R)


@pytest.mark.parametrize("tile_shape", [0, 3], indirect=True)
@pytest.mark.parametrize("form", FORMS)
def test_exact_two_problems_per_launch(form, tile_shape):
    """Different shapes (the sequential tile order) and equal row counts (the interleaved one); the reductions differ."""
    mk = _ints(17)
    for rows in ((100, 36), (100, 100)):
        cases = [_problem(mk, form, I, J, R) for I, J, R in zip(rows, (72, 40), (36, 68))]
        _bf16([c[0] for c in cases], form)
        for rec, keep, out, ref in cases:
            assert torch.equal(_f64(out[0]), ref)


@pytest.mark.parametrize("form", [(True, True), (True, False)])
def test_exact_grouped_a_rows(form):
    """A = the 5 coefficient rows k0 .. k0 + 4 of every node of an [N, K, C] tensor: row i -> (i / 5) * K C + (i % 5) * C."""
    mk = _ints(19)
    N, K, C, k0, g, J = 53, 9, 36, 4, 5, 40
    x = mk(N, K, C)
    b = mk(J, C) if form[1] else mk(C, J)
    xd, bd = x.to(DEV), b.to(DEV)
    out = torch.full((N * g, J), float("nan"), device=DEV)
    a = x[:, k0:k0 + g].reshape(N * g, C)
    ref = _f64(a) @ (_f64(b).t() if form[1] else _f64(b))
    _bf16([dict(a=xd.data_ptr() + 4 * k0 * C, lda=C, a_group=g, a_group_ld=K * C, b=bd.data_ptr(), ldb=bd.stride(0),
                c=out.data_ptr(), ldc=J, I=N * g, J=J, R=C)], form)
    assert torch.equal(_f64(out), ref)


@pytest.mark.parametrize("tile_shape", [0, 3], indirect=True)
def test_exact_split_reduction_and_empty_trailing_split(tile_shape):
    """(0, 0) form: one split and three; R = 40 in 3 splits of 32 leaves the last split no rows - its slab and its asum row are
    zeros."""
    form = (False, False)
    mk = _ints(23)
    for R, S in ((100, 1), (100, 3), (40, 3)):
        rec, keep, out, ref = _problem(mk, form, 36, 132, R, S=S)
        asum = torch.full((S, 36), float("nan"), device=DEV)
        _bf16([dict(rec, asum=asum.data_ptr(), asum_stride=36)], form, S)
        assert torch.equal(_f64(out).sum(0), ref), (R, S)
        assert torch.equal(_f64(asum).sum(0), _f64(keep[0]).sum(0))
        if (R, S) == (40, 3):
            assert not out[2].any() and not asum[2].any()


@pytest.mark.parametrize("tile_shape", [0, 3], indirect=True)
@pytest.mark.parametrize("form", FORMS)
def test_rounding_rule_random_operands(form, tile_shape):
    """Random f32 operands against the float64 product of the operands rounded to bf16 (torch's round-to-nearest-even): only
    the f32 accumulation order separates the two, so the f32 tests' tolerance holds as it is."""
    mk = _floats(29 + tile_shape)
    for I, J in ((ROWS[1] if form[0] else COLS[1], COLS[0]), (ROWS[2] if form[0] else COLS[2], COLS[1])):
        for R in (36, 100):
            rec, keep, out, ref = _problem(mk, form, I, J, R)
            _bf16([rec], form)
            check(out[0], ref, *_tol("float", form, R))


TIES = [(1 + 2.0 ** -8, 1.0), (1 + 3 * 2.0 ** -8, 1 + 2.0 ** -6), (-(1 + 2.0 ** -8), -1.0), (1 + 2.0 ** -8 + 2.0 ** -20, 1 + 2.0 ** -7),
        (3 + 2.0 ** -7, 3.0), (3 + 3 * 2.0 ** -7, 3 + 2.0 ** -5)]


@pytest.mark.parametrize("form", FORMS)
def test_rounding_ties_go_to_even(form):
    """Operands exactly half way between two bf16 values, times 1: 1 + 2^-8 gives 1, 1 + 3 * 2^-8 gives 1 + 2^-6 (and a value just
    above a tie goes up).  Each tie is the only non-zero of its A row / B column, so the output element IS the rounded value -
    once with the tie on the A side, once on the B side."""
    n = 8
    vals = torch.tensor([v for v, _ in TIES] + [1.0, 1.0])
    want = torch.tensor([w for _, w in TIES] + [1.0, 1.0], dtype=torch.float64)
    for side in (0, 1):
        a_op, b_op = (torch.diag(vals), torch.eye(n)) if side == 0 else (torch.eye(n), torch.diag(vals))      # [i, r] and [r, j]
        a = (a_op if form[0] else a_op.t()).contiguous().to(DEV)
        b = (b_op.t() if form[1] else b_op).contiguous().to(DEV)
        out = torch.full((n, n), float("nan"), device=DEV)
        _bf16([dict(a=a.data_ptr(), lda=n, b=b.data_ptr(), ldb=n, c=out.data_ptr(), ldc=n, I=n, J=n, R=n)], form)
        assert torch.equal(_f64(out), torch.diag(want)), (form, side)


@pytest.mark.parametrize("form", FORMS)
def test_inf_and_nan_poison_their_own_row_and_column(form):
    """One inf in A's row 3 and one NaN in B's column 8: output row 3 and column 8 are not finite, everything else is the
    product as if they were not there (ragged tile, two K steps)."""
    I, J, R = 40, 36, 36
    ai, ar, bj, br = 3, 5, 8, 33

    def edit(a, b):
        if form[0]:
            a[ai, ar] = float("inf")
        else:
            a[ar, ai] = float("inf")
        if form[1]:
            b[bj, br] = float("nan")
        else:
            b[br, bj] = float("nan")
    rec, keep, out, ref = _problem(_floats(31), form, I, J, R, edit=edit)
    _bf16([rec], form)
    got = _f64(out[0])
    rows = torch.arange(I) != ai
    cols = torch.arange(J) != bj
    assert not torch.isfinite(got[ai]).any() and torch.isnan(got[:, bj]).all()
    clean, clean_ref = got[rows][:, cols], ref[rows][:, cols]
    assert torch.isfinite(clean).all()
    tol, slack, extra = _tol("float", form, R)
    assert float((clean - clean_ref).abs().max()) <= tol * float(clean_ref.abs().max()) + slack + extra


@pytest.mark.parametrize("tile_shape", [0, 3], indirect=True)
def test_epilogue_options(tile_shape):
    """bias + addend + ReLU, and the positive-mask epilogue, on ragged tiles: exact on integers, and on random floats against
    the same reference as the bare product."""
    M, N, K = 333, 200, 72
    for kind, mk in (("int", _ints(37)), ("float", _floats(37))):
        x, w, b, ad, hm, dy = mk(M, K), mk(N, K), mk(N), mk(M, N), mk(M, K), mk(M, N)
        xd, wd, bd, add, hmd, dyd = (t.to(DEV) for t in (x, w, b, ad, hm, dy))
        y = torch.full((M, N), float("nan"), device=DEV)
        _bf16([dict(a=xd.data_ptr(), lda=K, b=wd.data_ptr(), ldb=K, c=y.data_ptr(), ldc=N, bias=bd.data_ptr(),
                    addend=add.data_ptr(), relu=1, I=M, J=N, R=K)], (True, True))
        check(y, torch.relu(_rounded(x) @ _rounded(w).t() + _f64(b) + _f64(ad)), *_tol(kind, (True, True), K))
        dx = torch.full((M, K), float("nan"), device=DEV)
        _bf16([dict(a=dyd.data_ptr(), lda=N, b=wd.data_ptr(), ldb=K, c=dx.data_ptr(), ldc=K, I=M, J=K, R=N, mask=hmd.data_ptr())],
              (True, False))
        check(dx, (_rounded(dy) @ _rounded(w)) * (_f64(hm) > 0), *_tol(kind, (True, False), N))


@pytest.mark.parametrize("tile_shape", [0, 3], indirect=True)
@pytest.mark.parametrize("S", [1, 3])
def test_asum_is_bit_equal_to_the_f32_kernels(S, tile_shape):
    """asum comes from the unrounded f32 registers: the same bits as singa_gemm_f32 for the same operands and splits."""
    from singa_amd import ops
    I, J, R = 132, 36, 1000
    rec, keep, out, ref = _problem(_floats(41), (False, False), I, J, R, S=S)
    sums = []
    for precision in ("f32", "bf16"):
        asum = torch.full((S, I), float("nan"), device=DEV)
        ops._gemm([dict(rec, asum=asum.data_ptr(), asum_stride=I)], False, False, S, precision=precision)
        sums.append(asum.cpu())
    assert torch.isfinite(sums[0]).all() and torch.equal(sums[0], sums[1])
    check(out.sum(0), ref, *_tol("float", (False, False), R))


def test_argument_errors_give_the_f32_entry_points_codes():
    """The cases of test_gemm_argument_errors (and a few more of the shared checks): the same return code from both entry
    points, before any launch."""
    from singa_amd import _capi, _lib, ops
    lib = _lib.lib()
    z = torch.zeros(64, 64, device=DEV)
    ok = dict(a=z.data_ptr(), lda=64, b=z.data_ptr(), ldb=64, c=z.data_ptr(), ldc=64, I=8, J=4, R=8)
    cases = [([dict(a=0, b=0, c=0, I=1, J=1, R=4)], True, True, 1),               # null operands
             ([dict(ok, R=6)], True, True, 1),                                    # K = 6 is not a multiple of 4 floats
             ([dict(ok, J=6)], True, True, 1), ([dict(ok, ldc=62)], True, True, 1), ([dict(ok, I=-1)], True, True, 1),
             ([ok], False, True, 1), ([ok], True, True, 0), ([ok] * 13, True, True, 1),
             ([dict(ok, bias=z.data_ptr(), c_split_stride=64)], False, False, 2),
             ([dict(ok, asum=z.data_ptr(), asum_stride=8)], True, True, 1)]
    for items, a_rc, b_rc, splits in cases:
        codes = []
        for entry in (lib.singa_gemm_f32, lib.singa_gemm_bf16):
            arr, n = _capi.gemm_probs(items) if len(items) <= 12 else (_capi.gemm_probs(items[:12])[0], len(items))
            codes.append(entry(arr, n, int(a_rc), int(b_rc), splits, None))
        assert codes[0] != 0 and codes[0] == codes[1], (items, codes)
    x, w = torch.zeros(8, 6, device=DEV), torch.zeros(4, 6, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 4"):
        ops.gemm_nt(x, w, precision="bf16")
    with pytest.raises(RuntimeError):
        ops._gemm([dict(a=0, b=0, c=0, I=1, J=1, R=4)], True, True, precision="bf16")


@pytest.mark.parametrize("tile_shape", [0, 3], indirect=True)
@pytest.mark.parametrize("form", FORMS)
def test_write_footprint(form, tile_shape):
    """The result lies between two guard bands inside one buffer pre-filled with NaN (C) and a sentinel (guards): every element
    of C is written, nothing else, for ragged I and J."""
    I, J, R, G = (130 if form[0] else 132), 36, 68, 4096
    rec, keep, out, ref = _problem(_ints(43), form, I, J, R)
    buf = torch.full((2 * G + I * J,), 777.0, device=DEV)
    c = buf[G:G + I * J].view(I, J)
    c.fill_(float("nan"))
    _bf16([dict(rec, c=c.data_ptr())], form)
    assert bool((buf[:G] == 777.0).all()) and bool((buf[G + I * J:] == 777.0).all())
    assert torch.equal(_f64(c), ref)
