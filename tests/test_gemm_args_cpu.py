"""The argument checks of `singa_gemm_f32` and `singa_cgemm3m_f32` through the built library, without a GPU: the return code and
the text of `singa_last_error_string()` for every check either entry point makes, and the calls that return SINGA_OK without
a launch.  No pointer is dereferenced and nothing is launched: every call fails a check or has no tile."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import _capi
    return _capi.bind(__graft_entry__.LIB)


# a valid record of each entry point (8 x 8 x 8, complex: in complex units); pointers: T = some 16-byte aligned address,
# None = null, MIS = that address + 4
T, MIS, NAN, BIG = True, "misaligned", float("nan"), 1 << 20
G, C = "gemm_f32", "cgemm3m_f32"
VALID = {G: dict(a=T, b=T, c=T, lda=8, ldb=8, ldc=8, I=8, J=8, R=8),
         C: dict(a=T, b=T, c=T, lda=16, ldb=8, ldc=16, a_im=8, b_im=64, c_im=8, I=8, J=8, R=8, sigma=1.0)}
AXES = 'contiguous axes must be multiples of 4 floats and 16-byte aligned'
RESULT = "the result's columns, pitches and base must be multiples of 4 floats / 16 bytes"
SLABS = 'split reductions write dense [I, J] partial slabs (c_split_stride apart), no epilogue options'
MASK = "mask / addend have the result's layout (a mask: plain rows only) and are 16-byte aligned"
ASUM = 'asum goes with the (0, 0) form, plain A rows, a slab of at least I floats per split'
CAXES = 'contiguous axes, pitches and part offsets must be multiples of 4 floats, bases 16-byte aligned'
FORM01 = 'A output-contiguous with B reduction-contiguous is not built'

# (entry point, launch arguments that differ from `(probs, len(probs), 1, 1, splits=1)` - form = (a_r_contig, b_r_contig) -, one
# dict per problem with the fields that differ from VALID, return code, text behind "<entry>: " or None for SINGA_OK), recorded
# from the library as it was when each entry point carried all of its checks and its own tile planning.
GEMM_ARGUMENTS = [
    # singa_gemm_f32: one bad argument at a time
    (G, dict(probs=None), [dict()], -3, '1..SINGA_GEMM_MAX problems per launch'),
    (G, dict(n=0), [dict()], -3, '1..SINGA_GEMM_MAX problems per launch'),
    (G, dict(), [dict()] * 13, -3, '1..SINGA_GEMM_MAX problems per launch'),
    (G, dict(splits=0), [dict()], -3, 'splits must be >= 1'),
    (G, dict(splits=-2), [dict()], -3, 'splits must be >= 1'),
    (G, dict(form=(0, 1)), [dict()], -3, FORM01),
    (G, dict(), [dict(a=None)], -1, 'null operand'),
    (G, dict(), [dict(b=None)], -1, 'null operand'),
    (G, dict(), [dict(c=None)], -1, 'null operand'),
    (G, dict(), [dict(I=-1)], -3, 'negative size'),
    (G, dict(), [dict(J=-4)], -3, 'negative size'),
    (G, dict(), [dict(R=-4)], -3, 'negative size'),
    (G, dict(), [dict(R=6)], -3, AXES),
    (G, dict(form=(1, 0)), [dict(J=6)], -3, AXES),
    (G, dict(form=(0, 0)), [dict(I=6)], -3, AXES),
    (G, dict(), [dict(lda=6)], -3, AXES),
    (G, dict(), [dict(ldb=6)], -3, AXES),
    (G, dict(), [dict(a_group_ld=2)], -3, AXES),
    (G, dict(), [dict(b_group_ld=2)], -3, AXES),
    (G, dict(), [dict(a=MIS)], -3, AXES),
    (G, dict(), [dict(b=MIS)], -3, AXES),
    (G, dict(), [dict(b_group=2)], -3, 'a reduction-contiguous B has plain rows'),
    (G, dict(form=(1, 0)), [dict(b_group=2, I=0)], 0, None),
    (G, dict(), [dict(J=6)], -3, RESULT),
    (G, dict(), [dict(ldc=6)], -3, RESULT),
    (G, dict(), [dict(c_group_ld=2)], -3, RESULT),
    (G, dict(), [dict(c_split_stride=2)], -3, RESULT),
    (G, dict(), [dict(c=MIS)], -3, RESULT),
    (G, dict(), [dict(bias=MIS)], -3, RESULT),
    (G, dict(splits=2), [dict(c_split_stride=64, bias=T)], -3, SLABS),
    (G, dict(splits=2), [dict(c_split_stride=64, ldc=12)], -3, SLABS),
    (G, dict(splits=2), [dict(c_split_stride=64, c_group=2)], -3, SLABS),
    (G, dict(splits=2), [dict(c_split_stride=64, mask=T)], -3, SLABS),
    (G, dict(splits=2), [dict(c_split_stride=64, addend=T)], -3, SLABS),
    (G, dict(splits=2), [dict(c_split_stride=64, relu=1)], -3, SLABS),
    (G, dict(splits=2), [dict(c_split_stride=60)], -3, SLABS),
    (G, dict(splits=2), [dict()], -3, SLABS),
    (G, dict(), [dict(mask=T, c_group=2)], -3, MASK),
    (G, dict(), [dict(mask=MIS)], -3, MASK),
    (G, dict(), [dict(addend=MIS)], -3, MASK),
    (G, dict(), [dict(asum=T, asum_stride=8)], -3, ASUM),
    (G, dict(form=(0, 0)), [dict(asum=T, asum_stride=8, a_group=2)], -3, ASUM),
    (G, dict(form=(0, 0)), [dict(asum=T, asum_stride=4)], -3, ASUM),
    (G, dict(splits=32), [dict(I=BIG, J=BIG, ldc=BIG, c_split_stride=BIG * BIG)], -3, 'too many tiles'),
    (G, dict(splits=1 << 30), [dict(c_split_stride=64), dict(c_split_stride=64)], -3, 'too many tiles'),
    # ... pairs: the check that comes first wins; every problem is checked before anything is planned
    (G, dict(probs=None, splits=0), [dict()], -3, '1..SINGA_GEMM_MAX problems per launch'),
    (G, dict(n=0, splits=0), [dict()], -3, '1..SINGA_GEMM_MAX problems per launch'),
    (G, dict(n=0, form=(0, 1)), [dict()], -3, '1..SINGA_GEMM_MAX problems per launch'),
    (G, dict(splits=0, form=(0, 1)), [dict()], -3, 'splits must be >= 1'),
    (G, dict(form=(0, 1)), [dict(a=None)], -3, FORM01),
    (G, dict(), [dict(a=None, I=-1)], -1, 'null operand'),
    (G, dict(), [dict(I=-1, R=6)], -3, 'negative size'),
    (G, dict(), [dict(R=6, b_group=2)], -3, AXES),
    (G, dict(), [dict(b_group=2, J=6)], -3, 'a reduction-contiguous B has plain rows'),
    (G, dict(splits=2), [dict(ldc=6, bias=T)], -3, RESULT),
    (G, dict(splits=2), [dict(bias=T, mask=MIS)], -3, SLABS),
    (G, dict(), [dict(mask=MIS, asum=T)], -3, MASK),
    (G, dict(), [dict(asum=T, asum_stride=8, I=0)], -3, ASUM),
    (G, dict(splits=32), [dict(I=BIG, J=BIG, ldc=BIG, c_split_stride=BIG * BIG, asum=T, asum_stride=BIG)], -3, ASUM),
    (G, dict(), [dict(), dict(b=None)], -1, 'null operand'),
    (G, dict(), [dict(I=0), dict(R=-4)], -3, 'negative size'),
    (G, dict(), [dict(J=6), dict(a=None)], -3, RESULT),
    # ... nothing to launch: every problem has I = 0 or J = 0 (SINGA_GEMM_MAX = 12 problems at the most)
    (G, dict(), [dict(I=0)], 0, None),
    (G, dict(), [dict(J=0)], 0, None),
    (G, dict(form=(1, 0)), [dict(I=0), dict(J=0)], 0, None),
    (G, dict(form=(0, 0), splits=3), [dict(I=0, c_split_stride=0)], 0, None),
    (G, dict(), [dict(I=0)] * 12, 0, None),
    (G, dict(), [dict(I=0, R=0), dict(J=0, R=0)], 0, None),
    # singa_cgemm3m_f32 (SINGA_CGEMM_MAX = 4)
    (C, dict(probs=None), [dict()], -3, '1..SINGA_CGEMM_MAX problems per launch'),
    (C, dict(n=0), [dict()], -3, '1..SINGA_CGEMM_MAX problems per launch'),
    (C, dict(), [dict()] * 5, -3, '1..SINGA_CGEMM_MAX problems per launch'),
    (C, dict(splits=0), [dict()], -3, 'splits must be >= 1'),
    (C, dict(form=(0, 1)), [dict()], -3, FORM01),
    (C, dict(), [dict(a=None)], -1, 'null operand'),
    (C, dict(), [dict(b=None)], -1, 'null operand'),
    (C, dict(), [dict(c=None)], -1, 'null operand'),
    (C, dict(), [dict(I=-1)], -3, 'negative size'),
    (C, dict(), [dict(J=-4)], -3, 'negative size'),
    (C, dict(), [dict(R=-4)], -3, 'negative size'),
    (C, dict(), [dict(R=6)], -3, CAXES),
    (C, dict(form=(1, 0)), [dict(J=6)], -3, CAXES),
    (C, dict(form=(0, 0)), [dict(I=6)], -3, CAXES),
    (C, dict(), [dict(J=6)], -3, CAXES),
    (C, dict(), [dict(lda=18)], -3, CAXES),
    (C, dict(), [dict(ldb=6)], -3, CAXES),
    (C, dict(), [dict(ldc=18)], -3, CAXES),
    (C, dict(), [dict(a_im=6)], -3, CAXES),
    (C, dict(), [dict(b_im=62)], -3, CAXES),
    (C, dict(), [dict(c_im=6)], -3, CAXES),
    (C, dict(), [dict(c_split_stride=2)], -3, CAXES),
    (C, dict(), [dict(a=MIS)], -3, CAXES),
    (C, dict(), [dict(b=MIS)], -3, CAXES),
    (C, dict(), [dict(c=MIS)], -3, CAXES),
    (C, dict(), [dict(sigma=0.5)], -3, 'sigma is +1 or -1'),
    (C, dict(), [dict(sigma=0.0)], -3, 'sigma is +1 or -1'),
    (C, dict(), [dict(sigma=NAN)], -3, 'sigma is +1 or -1'),
    (C, dict(splits=2), [dict()], -3, 'split reductions need c_split_stride'),
    (C, dict(splits=2), [dict(c_split_stride=-4)], -3, 'split reductions need c_split_stride'),
    (C, dict(splits=16), [dict(I=BIG, J=BIG, ldc=2 * BIG, c_im=BIG, c_split_stride=2 * BIG * BIG)], -3, 'too many tiles'),
    # ... pairs
    (C, dict(probs=None, splits=0), [dict()], -3, '1..SINGA_CGEMM_MAX problems per launch'),
    (C, dict(n=0, splits=0), [dict()], -3, '1..SINGA_CGEMM_MAX problems per launch'),
    (C, dict(splits=0, form=(0, 1)), [dict()], -3, 'splits must be >= 1'),
    (C, dict(form=(0, 1)), [dict(c=None)], -3, FORM01),
    (C, dict(), [dict(c=None, R=-4)], -1, 'null operand'),
    (C, dict(), [dict(R=-4, a_im=6)], -3, 'negative size'),
    (C, dict(), [dict(a_im=6, sigma=0.5)], -3, CAXES),
    (C, dict(splits=2), [dict(sigma=0.5)], -3, 'sigma is +1 or -1'),
    (C, dict(splits=2), [dict(I=0)], -3, 'split reductions need c_split_stride'),
    (C, dict(), [dict(), dict(sigma=2.0)], -3, 'sigma is +1 or -1'),
    (C, dict(), [dict(I=0), dict(a=None)], -1, 'null operand'),
    (C, dict(splits=16), [dict(I=BIG, J=BIG, ldc=2 * BIG, c_im=BIG, c_split_stride=2 * BIG * BIG), dict(sigma=0.5)], -3, 'sigma is +1 or -1'),
    # ... nothing to launch
    (C, dict(), [dict(I=0)], 0, None),
    (C, dict(), [dict(J=0)], 0, None),
    (C, dict(form=(1, 0)), [dict(I=0), dict(J=0)], 0, None),
    (C, dict(form=(0, 0), splits=3), [dict(J=0, c_split_stride=128)], 0, None),
    (C, dict(), [dict(I=0)] * 4, 0, None),
]


@pytest.mark.parametrize("entry,launch,probs,code,text", GEMM_ARGUMENTS, ids=[f"{e}-{i}" for i, (e, *_) in enumerate(GEMM_ARGUMENTS)])
def test_gemm_entry_points_report_arguments_as_recorded(lib, entry, launch, probs, code, text):
    """Same code and same text, byte for byte, for every row of the table: one bad argument at a time, pairs that pin the order
    of the checks, the problem-count limits, and the launches that have no tile."""
    from singa_amd import _capi
    buf = (ctypes.c_char * 80)()
    p = (ctypes.addressof(buf) + 15) // 16 * 16
    items = [{k: p if v is True else p + 4 if v == MIS else v for k, v in {**VALID[entry], **bad}.items()} for bad in probs]
    arr, n = _capi.gemm_probs(items, _capi.Gemm if entry == G else _capi.CGemm)
    a_rc, b_rc = launch.get("form", (1, 1))
    lib.singa_init(None, 0)                                  # (an error of its own: the text below must be this call's)
    got = getattr(lib, "singa_" + entry)(arr if launch.get("probs", T) else None, launch.get("n", n), a_rc, b_rc,
                                         launch.get("splits", 1), None)
    assert got == code
    if text is not None:
        assert lib.singa_last_error_string() == f"{entry}: {text}".encode()
