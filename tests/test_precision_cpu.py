"""Without a GPU: the precision switch's argument checks, the f32 call's unchanged marshalling, and the entry point in the CPU
emulation build (which has no bf16 matrix-core stand-in: it exports singa_gemm_bf16 and refuses)."""
import ctypes

import pytest
import torch

from singa_amd import _capi, _lib, ops
from tests.test_kernels_emul import emul  # noqa: F401  (the fixture: the library built against tests/emul)


@pytest.fixture
def no_library(monkeypatch):
    def lib():
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(_lib, "lib", lib)


def test_unknown_precision_is_refused_before_any_device_work(no_library):
    from singa_amd.config import load_config
    from singa_amd.model.CProMG import Transformer
    from singa_amd.model.GAN import SINGA
    cfg = load_config(lmax=2)
    with pytest.raises(ValueError, match="precision"):
        SINGA(cfg, device="cuda", precision="fp16")                 # (no module is built: "cuda" is never touched)
    with pytest.raises(ValueError, match="precision"):
        Transformer(cfg.model, cfg.model.featurizer_feat_dim, device="cuda", precision="fp16")
    z = torch.zeros(8, 8)
    rec = dict(a=z.data_ptr(), lda=8, b=z.data_ptr(), ldb=8, c=z.data_ptr(), ldc=8, I=8, J=8, R=8)
    with pytest.raises(ValueError, match="precision"):
        ops._gemm([rec], True, True, precision="x")
    with pytest.raises(ValueError, match="precision"):
        ops.check_precision("fp16")


class _Recorder:
    """Stands in for the bound library: records (entry point, records as dicts, scalar arguments)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(arr, n, a_rc, b_rc, splits, stream):
            recs = [{f: getattr(g, f) for f, _ in _capi.Gemm._fields_} for g in arr]
            self.calls.append((name, recs, n, a_rc, b_rc, splits))
            return 0
        return entry


def test_f32_call_marshals_what_it_did_and_bf16_differs_in_the_entry_point_only(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    monkeypatch.setattr(ops, "_stream", lambda: None)
    x, w, y, b = torch.randn(40, 24), torch.randn(16, 24), torch.empty(40, 16), torch.randn(16)
    items = [ops._prob(x, w, y, True, True, bias=b, relu=True)]
    ops._gemm(items, True, True)                                    # the keyword left out: the call made before it existed
    ops._gemm(items, True, True, 1, "f32")
    ops._gemm(items, True, True, precision="bf16")
    want = {f: 0 for f, _ in _capi.Gemm._fields_}
    want.update(a=x.data_ptr(), b=w.data_ptr(), c=y.data_ptr(), bias=b.data_ptr(), lda=24, ldb=24, ldc=16, I=40, J=16, R=24, relu=1)
    norm = lambda r: {k: (v or 0) for k, v in r.items()}
    assert [c[0] for c in rec.calls] == ["singa_gemm_f32", "singa_gemm_f32", "singa_gemm_bf16"]
    for name, recs, n, a_rc, b_rc, splits in rec.calls:
        assert (n, a_rc, b_rc, splits) == (1, 1, 1, 1) and [norm(r) for r in recs] == [want]
    # the weight gradient's split launch takes the same road
    rec.calls.clear()
    monkeypatch.setattr(ops, "param_colsum", lambda src, targets: [torch.zeros(n) for _, n, _ in targets])
    g = torch.randn(40, 16)
    for precision in ("f32", "bf16"):
        ops._tn_grad(g, x, torch.nn.Parameter(w.clone()), torch.nn.Parameter(b.clone()), precision=precision)
    (n0, r0, *s0), (n1, r1, *s1) = rec.calls
    assert (n0, n1) == ("singa_gemm_f32", "singa_gemm_bf16") and s0 == s1 and s0[1:3] == [0, 0]
    strip = lambda rs: [{k: v for k, v in r.items() if k not in ("c", "asum")} for r in rs]      # (each call's own partial buffer)
    assert strip(r0) == strip(r1) and r0[0]["asum"] and r1[0]["asum"]


def test_emulation_build_exports_the_entry_point_and_refuses(emul):  # noqa: F811
    z = torch.zeros(8, 8)
    arr, n = _capi.gemm_probs([dict(a=z.data_ptr(), lda=8, b=z.data_ptr(), ldb=8, c=z.data_ptr(), ldc=8, I=8, J=8, R=8)])
    assert emul.singa_gemm_bf16(arr, n, 1, 1, 1, None) == -3         # SINGA_E_SHAPE, as the other matrix-core-only entry points
    assert b"gemm_bf16: not part of the emulation build" in emul.singa_last_error_string()
    assert isinstance(emul.singa_gemm_bf16, ctypes._CFuncPtr)
