"""lmax 3 without a GPU: the CPU oracle against the reference's own tensors at this degree (tools/make_golden_lmax.py), the kernel source under the sequential emulation, the sizes singa_dims reports, and the one function that
refuses an embedding section before anything is launched.

The oracle and emulation cases are the test bodies of tests/test_oracle_golden.py and tests/test_kernels_emul.py, called with
L = 3: same shapes, same references, same tolerances.  (rmsnorm and the matrix-core kernels use cross-lane operations the
emulation does not have; tests/test_lmax_odd_gpu.py covers them.)"""
import ctypes

import pytest

from singa_amd import so3
from tests import test_kernels_emul as KE
from tests import test_oracle_golden as TG
from tests.golden_lmax import ODD, reads_split_goldens
from tests.helpers import NAMES
from tests.test_kernels_emul import emul  # noqa: F401  (the module-scoped build of the kernel source under tests/emul)


@pytest.fixture(autouse=True)
def _split_goldens(monkeypatch):
    reads_split_goldens(monkeypatch, TG)


# ------------------------------------------------------------------------------------------ the oracle pins the fixtures
@pytest.mark.parametrize("L", ODD)
@pytest.mark.parametrize("name", NAMES)
def test_oracle_embedding_forward_and_grads(L, name):
    TG.test_embedding_forward_and_grads(L, name)


@pytest.mark.parametrize("L", ODD)
def test_oracle_block0_intermediates(L):
    TG.test_block0_intermediates(L)


@pytest.mark.parametrize("L", ODD)
def test_oracle_singa_step(L):
    TG.test_singa_step(L)


@pytest.mark.parametrize("L", ODD)
def test_relu_tie_fixture_is_consistent(L):
    TG.test_relu_tie_fixture_is_consistent(L)


# ------------------------------------------------------------------------------------ the kernel source, thread by thread
@pytest.mark.parametrize("L", ODD)
def test_wigner_rows(emul, L):  # noqa: F811
    KE.test_wigner_rows(emul, L)


@pytest.mark.parametrize("L", ODD)
def test_gather_rotate(emul, L):  # noqa: F811
    KE.test_gather_rotate(emul, L)


@pytest.mark.parametrize("L,CH,heads,m0", [(3, 112, 7, 0), (3, 16, 1, 1)], ids=["L3-full", "L3-edge-degree"])
def test_rotate_back_scatter(emul, L, CH, heads, m0):  # noqa: F811
    """Both forms, forward and backward; rand_graph's 29 edges over 8 destinations leave one empty and fill others unevenly."""
    KE.test_rotate_back_scatter(emul, L, CH, heads, m0)


@pytest.mark.parametrize("L,M,C,edge", [(3, 2, 128, True), (3, 3, 512, False)])
def test_s2act_dense(emul, L, M, C, edge):  # noqa: F811
    KE.test_s2act(emul, L, M, C, edge)


@pytest.mark.parametrize("L,edge", [(3, True), (3, False)])
def test_s2act_separable(emul, L, edge):  # noqa: F811
    KE.test_s2act_separable(emul, L, edge)


@pytest.mark.parametrize("L,edge", [(3, True), (3, False)])
def test_s2act_separable_lane_layouts(emul, L, edge):  # noqa: F811
    KE.test_s2act_separable_lane_layouts(emul, L, edge)


@pytest.mark.parametrize("L,C", [(3, 512), (3, 112)])
def test_so3_skinny_kernels(emul, L, C):  # noqa: F811
    KE.test_so3_skinny_kernels(emul, L, C)


# ------------------------------------------------------------------------------------------------------------ singa_dims
@pytest.mark.parametrize("L,want", [(3, (14, 72, 9))])
def test_dims_of_lmax_3(emul, L, want):  # noqa: F811
    kr, wsz, rr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert emul.singa_dims(L, 2, ctypes.byref(kr), ctypes.byref(wsz), ctypes.byref(rr)) == 0
    assert (kr.value, wsz.value, rr.value) == want
    lay = so3.layout(L, 2)
    assert want == (lay.KR, lay.WSZ, lay.rad_rows)


@pytest.mark.parametrize("L,M", [(5, 2), (7, 2), (1, 2), (3, 1)])
def test_dims_refuses_what_is_not_built(emul, L, M):  # noqa: F811
    assert emul.singa_dims(L, M, None, None, None) == -2                              # SINGA_E_LMAX
    assert b"lmax in {2, 3, 4, 6} at mmax = 2" in emul.singa_last_error_string()   # one text for every site


# ------------------------------------------------------------------------------------------------------------ validation
def _cfg(lmax=6):
    from singa_amd.config import load_config
    return load_config(lmax=lmax)


@pytest.mark.parametrize("L", [2, 3, 4, 6])
def test_supported_degrees_pass_validation_and_construct(L):
    from singa_amd.config import validate_embedding_config
    from singa_amd.model.Embedding import EquivariantEmbedding
    cfg = _cfg(L)
    assert validate_embedding_config(cfg.embedding) == (L, 2)
    assert cfg.model.featurizer_feat_dim == (L + 1) ** 2 * 16
    emb = EquivariantEmbedding(cfg.embedding, device="cpu")
    assert emb.lmax_list == [L] and emb.mmax_list == [2]


REFUSED = [("lmax_list", [1]), ("lmax_list", [5]), ("lmax_list", [7]), ("lmax_list", [0]), ("lmax_list", [4, 6]), ("lmax_list", []),
           ("lmax_list", [3.5]), ("mmax_list", [1]), ("mmax_list", [3]), ("mmax_list", [2, 2]), ("sphere_channels", 32),
           ("attn_hidden_channels", 64), ("num_heads", 8), ("attn_value_channels", 8), ("use_atom_edge_embedding", False),
           ("share_atom_edge_embedding", False), ("alpha_drop", 0.1), ("proj_drop", 0.1), ("drop_path_rate", 0.05)]


@pytest.mark.parametrize("key,value", REFUSED, ids=[f"{k}={v}" for k, v in REFUSED])
def test_refused_keys_are_named_before_anything_is_built(key, value):
    from singa_amd.config import validate_embedding_config
    from singa_amd.model.Embedding import EquivariantEmbedding
    from singa_amd.model.GAN import SINGA
    cfg = _cfg(4)
    cfg.embedding[key] = value
    for build in (lambda: validate_embedding_config(cfg.embedding), lambda: EquivariantEmbedding(cfg.embedding, device="cpu"),
                  lambda: SINGA(cfg, device="cpu")):
        with pytest.raises(ValueError, match=rf"embedding\.{key}|embedding\.\S+ / embedding\.{key}") as exc:
            build()
        assert f"embedding.{key}" in str(exc.value)


def test_entry_points_name_the_degrees():
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for script in ("train.py", "gen.py"):
        out = subprocess.run([sys.executable, os.path.join(root, script), "--help"], capture_output=True, text=True, cwd=root)
        assert out.returncode == 0, out.stderr[-400:]
        assert "embedding.lmax_list (2, 3, 4 or 6)" in " ".join(out.stdout.split())
