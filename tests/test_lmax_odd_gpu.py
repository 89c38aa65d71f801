"""-m gpu: lmax 3 through every SO(3) kernel and the whole step.

Kernel level, model level and the rotation case are the test bodies of tests/test_kernels_gpu.py, tests/test_s2_lanes_gpu.py,
tests/test_launch_regimes_gpu.py, tests/test_model_gpu.py and tests/test_symmetry_gpu.py, called with L = 3: same shapes,
same references (the CPU oracle; the reference's own tensors of tools/make_golden_lmax.py), same tolerances.  The other ways
through the same kernels (recompute, the replayed step, the bf16 SO(2) convolutions, the protein-only embedding of generation)
run on the golden batch."""
import pytest
import torch

from oracle import singa_oracle as O
from singa_amd import so3
from tests import test_embedding_precision_gpu as EP
from tests import test_kernels_gpu as KG
from tests import test_launch_regimes_gpu as LR
from tests import test_model_gpu as MG
from tests import test_s2_lanes_gpu as SL
from tests import test_symmetry_gpu as SY
from tests.golden_lmax import ODD, golden, reads_split_goldens
from tests.helpers import NAMES, cpu_f64, named_grads, product_batch, rel_err, state_from_spec

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(autouse=True)
def _split_goldens(monkeypatch):
    reads_split_goldens(monkeypatch, MG)


# ================================================================================================================ kernels
@pytest.mark.parametrize("L", ODD)
def test_wigner_rows(L):
    KG.test_wigner_rows(L)


@pytest.mark.parametrize("L", ODD)
@pytest.mark.parametrize("homo", [True, False])
def test_gather_rotate_fwd_bwd(L, homo):
    KG.test_gather_rotate_fwd_bwd(L, homo)


@pytest.mark.parametrize("L", ODD)
def test_rotate_back_scatter_fwd_bwd(L):
    """(one destination with 40 edges, others empty)"""
    KG.test_rotate_back_scatter_fwd_bwd(L)


@pytest.mark.parametrize("L", ODD)
def test_edge_degree_scatter(L):
    KG.test_edge_degree_scatter(L)


@pytest.mark.parametrize("L", ODD)
def test_s2act_edge_and_node(L):
    KG.test_s2act_edge_and_node(L)


@pytest.mark.parametrize("L,edge", [(3, True), (3, False)])
def test_s2act_one_channel_form_equals_two_channel_form(L, edge):
    """Where both forward forms are built: the layouts that miss the pairing rule by one clause (an operand 4 bytes off, an odd
    pitch) reach the one-channel kernel and give the bits of the two-channel one."""
    SL.test_one_channel_form_equals_two_channel_form(L, edge)


@pytest.mark.parametrize("L", ODD)
def test_ffn_tail_matches_oracle(L):
    KG.test_ffn_tail_matches_oracle(L)


@pytest.mark.parametrize("L", ODD)
def test_so3_rmsnorm(L):
    """(forward, the plain backward and the backward that adds the skip's gradient)"""
    KG.test_so3_rmsnorm(L)


@pytest.mark.parametrize("L", ODD)
@pytest.mark.parametrize("N", [1, 15, 17])
@pytest.mark.parametrize("cin,cout", [(16, 512), (512, 16), (112, 16)])
def test_so3_linear_skinny_short_runs(cin, cout, N, L):
    """so3_skinny_expand / _reduce in the matrix-core variant (the default) and the lane-broadcast one: one node, one short of a
    16-node tile, one past it (two runs of the reduction, a second tile of one node in the expansion).  The criteria of
    tests/test_launch_regimes_gpu.py::test_so3_linear_skinny_long_node_runs."""
    ops, lib = LR._ops(), LR._lib()
    K = (L + 1) ** 2
    g = torch.Generator().manual_seed(N + L + cin)
    x = torch.randn(N, K, cin, generator=g)
    w = torch.randn(L + 1, cout, cin, generator=g) / cin ** 0.5
    b = torch.randn(cout, generator=g)
    gy = torch.randn(N, K, cout, generator=g)
    want, (w_x, w_w, w_b) = cpu_f64(lambda x_, w_, b_: O.so3_linear({"p.weight": w_, "p.bias": b_}, "p", x_, L), (x, w, b), gy)
    assert ops.USE_SKINNY_SO3
    for valu in (0, 1):
        lib.singa_so3_skinny_variant(valu)
        try:
            xd, wd, bd = LR.dev_leaf(x), LR.dev_leaf(w), LR.dev_leaf(b)
            got = ops.so3_linear(xd, wd, bd, L)
            got.backward(gy.to(DEV))
            LR.check_rows(f"so3_linear {cin}->{cout} N={N} L={L} variant={valu}",
                          [("out", got, want, 2e-6), ("d x", xd.grad, w_x, 5e-6), ("d weight", wd.grad, w_w, 1e-5),
                           ("d bias", bd.grad, w_b, 1e-5)])
        finally:
            lib.singa_so3_skinny_variant(0)


@pytest.mark.parametrize("L", ODD)
def test_so3_linear_skinny_long_node_runs(L):
    """112 -> 16 channels with more than the minimum 8 nodes per run of the reduction: the node count comes from the library's own
    sizing (singa_so3_skinny_nparts), the first 12289 + 2048 k that lengthens the runs; not a multiple of 16."""
    lib = LR._lib()
    N = 12289
    while N / lib.singa_so3_skinny_nparts(N, L, 112) <= 8 and N < 60000:
        N += 2048
    assert N / lib.singa_so3_skinny_nparts(N, L, 112) > 8, N
    LR.test_so3_linear_skinny_long_node_runs(112, 16, N, L)


# ================================================================================================================== model
@pytest.mark.parametrize("L", ODD)
@pytest.mark.parametrize("name", NAMES)
def test_embedding_matches_reference(L, name):
    MG.test_embedding_matches_reference(L, name)


@pytest.mark.parametrize("L", ODD)
def test_block0_intermediates_match_reference(L):
    MG.test_block0_intermediates_match_reference(L)


@pytest.mark.parametrize("L", ODD)
def test_singa_step_matches_reference(L):
    """logits, loss and the total gradient norm at 1e-4, every parameter's gradient samples at 1e-4, at most 16 gates pinned"""
    MG.test_singa_step_matches_reference(L)


# ================================================================================== other ways through the same kernels
def _eager(model, batch):
    model.zero_grad(set_to_none=True)
    logits = model(batch)
    loss = torch.nn.functional.cross_entropy(logits, batch["ligand_data"]["smiIndices_tgt"].reshape(-1))
    loss.backward()
    return logits.detach(), loss.detach(), named_grads(model)


@pytest.mark.parametrize("L", ODD)
def test_recompute_is_bit_identical(L):
    batch = EP._batch(L)
    lo_off, loss_off, g_off = _eager(EP._model(L), batch)
    on = EP._model(L, recompute=True)
    assert on.embedding.recompute
    lo_on, loss_on, g_on = _eager(on, batch)
    assert torch.equal(lo_on, lo_off) and torch.equal(loss_on, loss_off), (float(loss_on), float(loss_off))
    differ = [n for n in g_off if not torch.equal(g_on[n], g_off[n])]
    assert set(g_on) == set(g_off) and len(g_off) == 634 and not differ, (len(g_off), len(differ), differ[:6])


def test_replayed_steps_equal_eager_ones():
    """TrainStep in graph mode at L = 3: two replayed steps give the losses and the parameters of two eager steps of the same
    model, bit for bit.  The eager engine first makes its gradient-only pass (tests/test_update_parity_gpu.py: from its second
    pass on an eager engine accumulates parameter gradients the way a capture does)."""
    from singa_amd.engine import TrainStep
    from singa_amd.optim import Adam
    batch = EP._batch(3)
    runs = []
    for use_graph in (False, True):
        model = EP._model(3)
        init = {n: p.detach().clone() for n, p in model.named_parameters()}
        eng = TrainStep(model, Adam(model.parameters(), lr=1e-4, betas=(0.99, 0.999)), None, use_graph=use_graph)
        try:
            if not use_graph:
                eng._prepared(batch)
                eng._fwd_bwd(batch)
                eng.opt.zero_grad(set_to_none=True)
                assert eng._sink_params is not None and not getattr(eng.opt, "_built", False)
            losses = [eng.step(batch).detach().clone() for _ in range(2)]
            torch.cuda.synchronize()
            assert float(eng.opt.step_t) == 2.0                  # neither that pass nor the capture's warm-up took a step
            runs.append((losses, {n: p.detach().clone() for n, p in model.named_parameters()}))
        finally:
            if hasattr(eng, "release"):
                eng.release()
    (le, pe), (lg, pg) = runs
    print("eager", [float(v) for v in le], "replayed", [float(v) for v in lg])
    assert sum(not torch.equal(pe[n], init[n]) for n in pe) > 600                 # the steps did update the parameters
    assert all(torch.equal(a, b) for a, b in zip(le, lg))
    differ = [n for n in pe if not torch.equal(pe[n], pg[n])]
    assert not differ, (len(differ), differ[:6])


def test_bf16_embedding_step_is_close_to_the_f32_step():
    """embedding_precision="bf16" at L = 3 within the bound tests/test_embedding_precision_gpu.py holds L = 2 and 4 to"""
    setting = ("f32", "bf16")
    err = EP.closeness(3, setting)
    print("embedding precision bf16 against f32, L=3: " + ", ".join(f"{k} {v:.3e}" for k, v in err.items()))
    for k, v in err.items():
        assert 0 < v <= EP.CLOSE[setting][k], (k, v, EP.CLOSE[setting][k])


def test_gen_mode_embedding_matches_the_oracles_protein_pass():
    """`embedding(g, gen_mode=True)`, generation's only dependence on the degree: the protein-protein pass alone, against the
    oracle's protein output on the same frames."""
    from singa_amd.graph import PA
    L, name = 3, NAMES[1]
    z = golden(f"embed_L{L}_{name}.npz")
    emb = MG.build_embedding(L)
    g = product_batch([name], None)
    g.extras["edge_rot_mat"] = {"pp": torch.tensor(z["rot_pp"]).to(DEV)}
    with torch.no_grad():
        out = emb(g, gen_mode=True)
        # Part 1 of O.embedding_forward from the oracle's own pieces (its output[PA] also carries what Parts 3 and 4 do to the
        # shared dict, Q4): l = 0 initialisation + edge-degree embedding, the homogeneous blocks, the final norm
        sd, og = state_from_spec(f"embed_L{L}"), O.load_graph_npz(f"tests/golden/graph_{name}.npz")
        hp, fr = O.hyper(sd, "", L), O.Frame(torch.as_tensor(z["rot_pp"]), L, 2)
        ei, pos, zt = og["ei_pp"], og["pos_p"], og["z_p"]
        xe = torch.cat([O.gaussian((pos[ei[0]] - pos[ei[1]]).norm(dim=-1), 10.0, 16, 20.0), sd["source_embedding.weight"][zt[ei[0]]],
                        sd["target_embedding.weight"][zt[ei[1]]]], 1)
        x = torch.zeros(zt.shape[0], (L + 1) ** 2, 16)
        x[:, 0] = (sd["sphere_embedding.weight"][zt] + sd["sphere_embedding_2.weight"][O.barcode(og["x_p"])]).long().float()
        x = x + O.edge_degree(sd, "edge_degree_embedding", xe, ei[1], zt.shape[0], fr, 16)
        for i in range(hp["n_layers"]):
            x = O.block_homo(sd, f"blocks.{i}", x, xe, ei[0], ei[1], fr, hp)
        ref = O.rms_norm(sd, "norm", x, L)
    assert list(out.keys()) == [PA]
    assert out[PA].embedding.shape == (zt.shape[0], so3.layout(L, L).K, 16) and hp["n_layers"] == 3
    assert rel_err(out[PA].embedding.cpu(), ref) < 1e-4


# =============================================================================================================== rotation
@pytest.mark.parametrize("L", ODD)
def test_embedding_under_rotation(L):
    """The cyclic rotation of tests/symmetry.py: inputs turned by Q, outputs compared with D(Q) applied to the unturned run's;
    the bound is that suite's (a small multiple of the oracle's defect on the same pair of inputs)."""
    SY.test_embedding_symmetry(L, "rotate_cyclic")
