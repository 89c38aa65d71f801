"""-m gpu: singa_cgemm_bf16 (k7d, include/singa_hip_bf16.h) through ops._cgemm(..., precision="bf16") - the complex product with
operands rounded to bf16 inside the kernel, four real products, f32 accumulation.  Exact on small integers (bf16-exact
operands, sums far below 2^24: a swapped part, a lost sign, a fragment or transpose slip is an O(1) error against tolerance 0),
the rounding rule against the float64 four-product formula on bf16-rounded operands within the f32 complex tests' own
tolerance, ties, poisoning, the write footprint and the argument errors.

Layouts are the model's: A = [re | im] column halves (a_im = R, or I when output-contiguous); B = [re; im] row halves in the
(1, 1) and (1, 0) forms (b_im = J R), column halves in the (0, 0) form; C = [re | im] column halves, or row halves in (0, 0).
Rows of a reduction-contiguous A are free (36, 130, 257); in the (0, 0) form I is a contiguous axis and takes 36, 132, 260."""
import pytest
import torch

from tests.test_gemm_bf16_gpu import TIES
from tests.test_gemm_gpu import FORMS, _f64, _tol, check

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROWS = (36, 130, 257)
ROWS4 = (36, 132, 260)
# complex columns: narrower than a wavefront's 32-column block; ragged against 64; 96 and 132 leave the last tile's second column
# block padding only
COLS = (20, 36, 68, 96, 132)
REDUCTIONS = (4, 28, 32, 36, 64, 100)       # the K tail alone; one, two and three K steps of 32 (complex), full and ragged
SIGMAS = (1.0, -1.0)


def _ints(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randint(-4, 5, s, generator=g).float()


def _floats(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def _rounded(t):
    return t.bfloat16().double()


def _reference(ar, ai, br, bi, sigma):
    """The four-product formula in float64 on bf16-rounded operands -> (re, im)."""
    a, b, c, d = (_rounded(t) for t in (ar, ai, br, bi))
    return a @ c - sigma * (b @ d), b @ c + sigma * (a @ d)


class _Problem:
    """One problem from the logical parts ar, ai [I, R] and br, bi [R, J] (host tensors) in the operand form's memory layout.
    gap: elements (columns, or rows in the (0, 0) form) between C's parts and behind the imaginary one, sentinel-filled; guard:
    sentinel elements in front of and behind every slab set."""
    SENTINEL = 777.0

    def __init__(self, form, ar, ai, br, bi, sigma, S=1, gap=0, guard=0):
        a_rc, b_rc = form
        (I, R), J = ar.shape, br.shape[1]
        self.I, self.J, self.R, self.S, self.a_rc = I, J, R, S, a_rc
        a = torch.cat([ar, ai], 1) if a_rc else torch.cat([ar.t(), ai.t()], 1)
        if b_rc:
            b, b_im = torch.cat([br.t(), bi.t()], 0), J * R
        elif a_rc:
            b, b_im = torch.cat([br, bi], 0), R * J
        else:
            b, b_im = torch.cat([br, bi], 1), J
        self.keep = (a.contiguous().to(DEV), b.contiguous().to(DEV))
        shape = (S, I, 2 * (J + gap)) if a_rc else (S, 2 * (I + gap), J)
        n = shape[0] * shape[1] * shape[2]
        self.buf = torch.full((2 * guard + n,), self.SENTINEL, device=DEV)
        self.guard = guard
        self.c = self.buf[guard:guard + n].view(shape)
        re, im = self.parts(self.c)
        re.fill_(float("nan"))
        im.fill_(float("nan"))
        self.rec = dict(a=self.keep[0].data_ptr(), lda=self.keep[0].stride(0), a_im=R if a_rc else I, b=self.keep[1].data_ptr(),
                        ldb=self.keep[1].stride(0), b_im=b_im, c=self.c.data_ptr(), ldc=shape[2],
                        c_im=(J + gap) if a_rc else (I + gap) * J, I=I, J=J, R=R, sigma=sigma, c_split_stride=shape[1] * shape[2])
        self.ref = _reference(ar, ai, br, bi, sigma)

    def parts(self, c):
        """The views (re, im), each [S, I, J], of a result buffer."""
        if self.a_rc:
            w = c.shape[2] // 2
            return c[:, :, :self.J], c[:, :, w:w + self.J]
        h = c.shape[1] // 2
        return c[:, :self.I], c[:, h:h + self.I]

    def result(self):
        """(re, im) in float64, summed over the splits."""
        re, im = self.parts(self.c)
        return _f64(re).sum(0), _f64(im).sum(0)

    def untouched(self):
        """True if every element outside C's two parts still holds the sentinel."""
        c = self.c.clone()
        re, im = self.parts(c)
        re.fill_(self.SENTINEL)
        im.fill_(self.SENTINEL)
        n = c.numel()
        return bool((c == self.SENTINEL).all()) and bool((self.buf[:self.guard] == self.SENTINEL).all()) and \
            bool((self.buf[self.guard + n:] == self.SENTINEL).all())


def _random(mk, form, I, J, R, sigma, **kw):
    return _Problem(form, mk(I, R), mk(I, R), mk(R, J), mk(R, J), sigma, **kw)


def _bf16(problems, form, splits=1):
    from singa_amd import ops
    ops._cgemm([p.rec for p in problems], *form, splits, precision="bf16")


def _assert_exact(p, what=None):
    (re, im), (rre, rim) = p.result(), p.ref
    assert torch.equal(re, rre) and torch.equal(im, rim), what


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("form", FORMS)
def test_exact_on_integers(form, sigma):
    mk = _ints(11)
    for I in (ROWS if form[0] else ROWS4):
        for J in COLS:
            for R in REDUCTIONS:
                p = _random(mk, form, I, J, R, sigma)
                _bf16([p], form)
                _assert_exact(p, (I, J, R))


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("form", FORMS)
def test_each_product_lands_in_its_part_with_its_sign(form, sigma):
    """A real-only or imaginary-only times B real-only or imaginary-only: (a)(c) -> re = a c; (a)(i sigma d) -> im = sigma a d;
    (i b)(c) -> im = b c; (i b)(i sigma d) -> re = -sigma b d; the other part is zero."""
    mk = _ints(13)
    I, J, R = (132, 68, 36)
    for a_imag in (False, True):
        for b_imag in (False, True):
            x, y = mk(I, R), mk(R, J)
            zx, zy = torch.zeros(I, R), torch.zeros(R, J)
            p = _Problem(form, zx if a_imag else x, x if a_imag else zx, zy if b_imag else y, y if b_imag else zy, sigma)
            _bf16([p], form)
            re, im = p.result()
            prod = x.double() @ y.double()
            assert prod.abs().max() > 0
            if a_imag == b_imag:
                want_re, want_im = (-sigma * prod if a_imag else prod), torch.zeros_like(prod)
            else:
                want_re, want_im = torch.zeros_like(prod), (sigma * prod if b_imag else prod)
            assert torch.equal(re, want_re) and torch.equal(im, want_im), (a_imag, b_imag)


@pytest.mark.parametrize("rows", [(132, 132, 132, 132), (132, 36, 260, 36)], ids=["same_rows", "different_rows"])
@pytest.mark.parametrize("count", [2, 4])
@pytest.mark.parametrize("form", FORMS)
def test_exact_several_problems_per_launch(form, count, rows):
    """Two and four problems per launch, in the interleaved (equal rows) and in the sequential tile order; the column counts and
    the reductions differ."""
    mk = _ints(17)
    ps = [_random(mk, form, I, J, R, 1.0 if form[1] else -1.0)
          for I, J, R in list(zip(rows, (68, 20, 132, 36), (20, 36, 68, 100)))[:count]]
    _bf16(ps, form)
    for p in ps:
        _assert_exact(p)


def test_exact_split_reduction_and_empty_trailing_split():
    """(0, 0) form: one split and three; R = 40 in 3 splits of 32 leaves the last split no rows - its slab is zeros."""
    form = (False, False)
    mk = _ints(23)
    for R, S in ((100, 1), (100, 3), (40, 3)):
        p = _random(mk, form, 36, 132, R, -1.0, S=S)
        _bf16([p], form, S)
        _assert_exact(p, (R, S))
        if (R, S) == (40, 3):
            assert not p.c[2].any()


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("form", FORMS)
def test_rounding_rule_random_operands(form, sigma):
    """Random f32 operands against the float64 four-product formula on operands rounded to bf16: only the f32 accumulation
    order separates the two, so the f32 complex tests' tolerance holds as it is."""
    mk = _floats(29)
    rows = ROWS if form[0] else ROWS4
    for I, J in ((rows[1], COLS[1]), (rows[2], COLS[4])):
        for R in (36, 100):
            p = _random(mk, form, I, J, R, sigma)
            _bf16([p], form)
            re, im = p.result()
            check(torch.cat([re, im]), torch.cat(p.ref), *_tol("float", form, R, cplx=True))


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("form", FORMS)
def test_rounding_ties_go_to_even(form, sigma):
    """Operands exactly half way between two bf16 values, times 1, as the only non-zero of their A row / B column: the output
    element IS the rounded value.  The tie sits on A's real part, A's imaginary part, B's real part, B's imaginary part."""
    n = 8
    vals = torch.diag(torch.tensor([v for v, _ in TIES] + [1.0, 1.0]))
    want = torch.diag(torch.tensor([w for _, w in TIES] + [1.0, 1.0], dtype=torch.float64))
    eye, zero = torch.eye(n), torch.zeros(n, n)
    none = torch.zeros(n, n, dtype=torch.float64)
    for place, args, (wre, wim) in (("A re", (vals, zero, eye, zero), (want, none)), ("A im", (zero, vals, eye, zero), (none, want)),
                                    ("B re", (eye, zero, vals, zero), (want, none)),
                                    ("B im", (eye, zero, zero, vals), (none, sigma * want))):
        p = _Problem(form, *args, sigma)
        _bf16([p], form)
        re, im = p.result()
        assert torch.equal(re, wre) and torch.equal(im, wim), place


@pytest.mark.parametrize("form", FORMS)
def test_inf_and_nan_poison_their_own_row_and_column(form):
    """One inf in the real part of A's row 3 and one NaN in the imaginary part of B's column 8: row 3 and column 8 of BOTH
    result parts are not finite, everything else is the product as if they were not there (ragged tile, two K steps)."""
    I, J, R = 40, 36, 36
    ai_, ar_, bj, br_ = 3, 5, 8, 33
    mk = _floats(31)
    a_re, a_im, b_re, b_im = mk(I, R), mk(I, R), mk(R, J), mk(R, J)
    sigma = 1.0 if form[1] else -1.0
    clean_re, clean_im = _reference(a_re, a_im, b_re, b_im, sigma)
    a_re[ai_, ar_] = float("inf")
    b_im[br_, bj] = float("nan")
    p = _Problem(form, a_re, a_im, b_re, b_im, sigma)
    _bf16([p], form)
    rows, cols = torch.arange(I) != ai_, torch.arange(J) != bj
    tol, slack, extra = _tol("float", form, R, cplx=True)
    for got, ref in zip(p.result(), (clean_re, clean_im)):
        assert not torch.isfinite(got[ai_]).any() and torch.isnan(got[:, bj]).all()
        clean, clean_ref = got[rows][:, cols], ref[rows][:, cols]
        assert torch.isfinite(clean).all()
        assert float((clean - clean_ref).abs().max()) <= tol * float(clean_ref.abs().max()) + slack + extra


@pytest.mark.parametrize("gap", [0, 4])
@pytest.mark.parametrize("form", FORMS)
def test_write_footprint(form, gap):
    """C's two parts between guard bands in one buffer: the parts pre-filled with NaN, the guards - and, gap > 0 (c_im > J), the
    elements between and behind the parts - with a sentinel.  Every element of C is written and nothing else, for ragged I, J."""
    I, J, R = (130 if form[0] else 132), 36, 68
    p = _random(_ints(43), form, I, J, R, 1.0 if form[1] else -1.0, gap=gap, guard=4096)
    _bf16([p], form)
    assert p.untouched()
    _assert_exact(p)


def test_argument_errors_give_the_f32_entry_points_codes():
    """The cases of test_complex_gemm_argument_errors: the same non-zero return code from both entry points."""
    from singa_amd import _capi, _lib, ops
    lib = _lib.lib()
    z = torch.zeros(64, 64, device=DEV)
    ok = dict(a=z.data_ptr(), lda=64, a_im=32, b=z.data_ptr(), ldb=32, b_im=32 * 32, c=z.data_ptr(), ldc=64, c_im=32, I=64, J=32, R=32,
              sigma=1.0)
    ops._cgemm([ok], True, True, precision="bf16")
    cases = [([{**ok, **bad}], True, True) for bad in (dict(sigma=0.5), dict(a_im=30), dict(R=30), dict(a=0), dict(ldc=62))]
    cases += [([ok], False, True), ([ok] * 5, True, True)]
    for items, a_rc, b_rc in cases:
        codes = []
        for entry in (lib.singa_cgemm3m_f32, lib.singa_cgemm_bf16):
            arr, n = _capi.gemm_probs(items[:4], _capi.CGemm)[0], len(items)
            codes.append(entry(arr, n, int(a_rc), int(b_rc), 1, None))
        assert codes[0] != 0 and codes[0] == codes[1], (items, codes)
        with pytest.raises(RuntimeError):
            ops._cgemm(items, a_rc, b_rc, precision="bf16")
