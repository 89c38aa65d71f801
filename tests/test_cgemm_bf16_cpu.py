"""Without a GPU: singa_cgemm_bf16 (include/singa_hip_bf16.h) is exported, declared and bound; its argument checks are
singa_cgemm3m_f32's and run before any HIP call; the embedding's precision switch refuses unknown values before any device
work; ops._cgemm's f32 call marshals what it did and "bf16" differs in the entry point only; the CPU emulation build exports the
symbol and refuses."""
import ctypes
import os
import re

import pytest
import torch

from singa_amd import _capi, _lib, ops
from tests.test_kernels_emul import emul  # noqa: F401  (the fixture: the library built against tests/emul)
from tests.test_precision_cpu import no_library  # noqa: F401  (the fixture: asking for the library is an error)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__
    __graft_entry__.build()
    return _capi.bind(__graft_entry__.LIB)


def test_the_library_exports_the_header_declares_and_the_table_lists_it(lib):
    assert isinstance(lib.singa_cgemm_bf16, ctypes._CFuncPtr)
    assert "singa_cgemm_bf16" in _capi.BF16_EXPORTS
    assert _capi._BF16_SIGS["singa_cgemm_bf16"] == (_capi._SIGS["singa_cgemm3m_f32"][0], ctypes.c_int32)
    with open(os.path.join(ROOT, "include", "singa_hip_bf16.h")) as f:
        text = f.read()
    assert re.search(r"\bint\s+singa_cgemm_bf16\s*\(\s*const\s+singa_cgemm_t\s*\*\s*probs\s*,\s*int\s+n\s*,\s*int\s+a_r_contig\s*,"
                     r"\s*int\s+b_r_contig\s*,\s*int\s+splits\s*,\s*void\s*\*\s*stream\s*\)\s*;", text)
    # the training ABI's own table does not grow
    assert "singa_cgemm_bf16" not in _capi.EXPORTS


def test_argument_checks_are_the_f32_entry_points_and_come_before_any_hip_call(lib):
    """No GPU here: a call that got as far as a launch would fail differently (or not at all) - every case returns the same
    non-zero code, with the same text behind the entry point's name, from both complex entry points."""
    buf = (ctypes.c_float * 64)()
    t = (ctypes.addressof(buf) + 15) & ~15
    ok = dict(a=t, lda=64, a_im=32, b=t, ldb=32, b_im=32 * 32, c=t, ldc=64, c_im=32, I=64, J=32, R=32, sigma=1.0)
    cases = [("null records", None, 1, (1, 1)), ("n = 0", [ok], 0, (1, 1)), ("n = SINGA_CGEMM_MAX + 1", [ok] * 4, 5, (1, 1)),
             ("form (0, 1)", [ok], 1, (0, 1)), ("sigma = 0.5", [dict(ok, sigma=0.5)], 1, (1, 1)),
             ("a_im = 30", [dict(ok, a_im=30)], 1, (1, 1)), ("R = 30", [dict(ok, R=30)], 1, (1, 1)),
             ("ldc = 62", [dict(ok, ldc=62)], 1, (1, 1))]
    for what, items, n, form in cases:
        got = []
        for name in ("singa_cgemm3m_f32", "singa_cgemm_bf16"):
            arr = _capi.gemm_probs(items, _capi.CGemm)[0] if items is not None else None
            code = getattr(lib, name)(arr, n, form[0], form[1], 1, None)
            text = lib.singa_last_error_string().decode()
            assert text.startswith(name[len("singa_"):] + ": "), (what, text)
            got.append((code, text.split(": ", 1)[1]))
        assert got[0][0] != 0 and got[0] == got[1], (what, got)


def test_unknown_precision_is_refused_before_any_device_work(no_library):  # noqa: F811
    from singa_amd.config import load_config
    from singa_amd.model.Embedding import EquivariantEmbedding
    from singa_amd.model.GAN import SINGA
    cfg = load_config(lmax=2)
    with pytest.raises(ValueError, match="precision"):
        SINGA(cfg, "cuda", embedding_precision="fp16")              # (no module is built: "cuda" is never touched)
    with pytest.raises(ValueError, match="precision"):
        EquivariantEmbedding(cfg.embedding, "cuda", precision="fp16")
    z = torch.zeros(8, 16)
    rec = dict(a=z.data_ptr(), lda=16, a_im=8, b=z.data_ptr(), ldb=8, b_im=32, c=z.data_ptr(), ldc=16, c_im=8, I=8, J=4, R=8, sigma=1.0)
    with pytest.raises(ValueError, match="precision"):
        ops._cgemm([rec], True, True, precision="x")
    with pytest.raises(ValueError, match="precision"):
        ops.so2_conv3m(z, z, z, z, z, 4, 4, precision="x")


class _Recorder:
    """Stands in for the bound library: records (entry point, records as dicts, scalar arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(arr, n, a_rc, b_rc, splits, stream):
            struct = type(arr)._type_
            self.calls.append((name, struct.__name__, [{f: getattr(g, f) for f, _ in struct._fields_} for g in arr], n, a_rc, b_rc, splits))
            return 0
        return entry


def test_f32_call_marshals_what_it_did_and_bf16_differs_in_the_entry_point_only(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    x, w, y = torch.randn(40, 48), torch.randn(32, 24), torch.empty(40, 32)
    items = [ops._cprob(x.chunk(2, 1), w.chunk(2, 0), y.chunk(2, 1), True, True, 1.0)]
    ops._cgemm(items, True, True)                                   # the keyword left out: the call made before it existed
    ops._cgemm(items, True, True, 1, "f32")
    ops._cgemm(items, True, True, precision="bf16")
    want = {f: 0 for f, _ in _capi.CGemm._fields_}
    want.update(a=x.data_ptr(), b=w.data_ptr(), c=y.data_ptr(), lda=48, ldb=24, ldc=32, a_im=24, b_im=16 * 24, c_im=16, I=40, J=16,
                R=24, sigma=1.0)
    norm = lambda r: {k: (v or 0) for k, v in r.items()}
    assert [c[0] for c in rec.calls] == ["singa_cgemm3m_f32", "singa_cgemm3m_f32", "singa_cgemm_bf16"]
    for name, struct, recs, n, a_rc, b_rc, splits in rec.calls:
        assert struct == "CGemm" and (n, a_rc, b_rc, splits) == (1, 1, 1, 1) and [norm(r) for r in recs] == [want]
    # the complex weight gradients' split launch takes the same road
    rec.calls.clear()
    monkeypatch.setattr(ops, "param_colsum", lambda src, targets: [torch.zeros(n) for _, n, _ in targets])
    g = torch.randn(40, 32)
    ops._dw_grads([(g, x, torch.nn.Parameter(w.clone()), None)], 3, cplx=True)
    for precision in ("f32", "bf16"):
        ops._dw_grads([(g, x, torch.nn.Parameter(w.clone()), None)], 3, cplx=True, precision=precision)
    (n0, _, r0, *s0), (n1, _, r1, *s1), (n2, _, r2, *s2) = rec.calls
    assert (n0, n1, n2) == ("singa_cgemm3m_f32", "singa_cgemm3m_f32", "singa_cgemm_bf16") and s0 == s1 == s2 == [1, 0, 0, 3]
    strip = lambda rs: [{k: v for k, v in r.items() if k != "c"} for r in rs]      # (each call's own partial buffer)
    assert strip(r0) == strip(r1) == strip(r2) and r0[0]["sigma"] == -1.0


def test_so2_conv3m_sends_all_six_launches_where_the_precision_says(monkeypatch):
    """Forward and backward of one convolution through the recording stand-in: under "bf16" the three real and the three complex
    launches name the bf16 entry points, with the records of the f32 launches; without the keyword none does."""
    monkeypatch.setattr(ops, "_stream", lambda: None)
    monkeypatch.setattr(ops, "_dev", lambda *t: None)
    monkeypatch.setattr(ops, "param_colsum", lambda src, targets: [torch.zeros(n) for _, n, _ in targets])
    names = {}
    for precision in (None, "f32", "bf16"):
        rec = _Recorder()
        monkeypatch.setattr(_lib, "lib", lambda rec=rec: rec)
        X = torch.randn(37, 36 + 48 + 24, requires_grad=True)
        w0, b0, w1, w2 = (torch.randn(*s, requires_grad=True) for s in ((40, 36), (40,), (40, 24), (24, 12)))
        kw = {} if precision is None else {"precision": precision}
        hs = ops.so2_conv3m(X, w0, b0, w1, w2, 36, 48, **kw)
        torch.autograd.backward(hs, [torch.ones_like(h) for h in hs])
        names[precision] = [(c[0], c[1], c[3:]) for c in rec.calls]
    f32 = ["singa_gemm_f32", "singa_cgemm3m_f32"]
    assert [n for n, _, _ in names[None]] == f32 + f32 + f32 and names[None] == names["f32"]
    assert names["bf16"] == [(n.replace("cgemm3m_f32", "cgemm_bf16").replace("gemm_f32", "gemm_bf16"), s, a) for n, s, a in names["f32"]]


def test_emulation_build_exports_the_entry_point_and_refuses(emul):  # noqa: F811
    z = torch.zeros(8, 16)
    arr, n = _capi.gemm_probs([dict(a=z.data_ptr(), lda=16, a_im=8, b=z.data_ptr(), ldb=8, b_im=32, c=z.data_ptr(), ldc=16, c_im=8,
                                    I=8, J=4, R=8, sigma=1.0)], _capi.CGemm)
    assert isinstance(emul.singa_cgemm_bf16, ctypes._CFuncPtr)
    assert emul.singa_cgemm_bf16(arr, n, 1, 1, 1, None) == -3        # SINGA_E_SHAPE, as singa_gemm_bf16 there
    assert b"cgemm_bf16: not part of the emulation build" in emul.singa_last_error_string()
