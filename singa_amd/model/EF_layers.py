"""MI355X-native equivariant layers with the reference's module surface (reference model/EF_layers.py = "EF").

Class names, constructor keywords, parameter names (state-dict keys) and forward signatures follow the reference so
that `TransBlockV2`, `SO2EquivariantGraphAttention`, `FeedForwardNetwork`, `EdgeDegreeEmbedding`, `SO3_LinearV2`
and the norm are drop-ins; the insides are different:

  * edges are sorted by destination once per edge type (ops.EdgeSet, cached) and every per-edge tensor lives in that
    order; nothing of size [E,K,K] or [E,K,112] is ever materialised;
  * between the two rotations the edge tensors stay in m-primary order as plain [E, rows*C] matrices, so each SO(2)
    convolution is one real GEMM (m = 0) and one complex GEMM launch (m = 1, 2: the +-m recombination of EF:721-729 IS a
    complex product, evaluated with three real multiplications on the fc weights themselves, k7c) - no permutation
    einsums, no recombination pass, no block weight;
  * gather + Wigner rotate + radial scaling, S2 activation, segment softmax, alpha-scale + rotate-back + scatter and
    the equivariant norm are the hand-written HIP kernels of libsinga_hip.so (singa_amd.ops).

Registered buffers of the reference that are pure functions of (lmax, mmax) (to_m, expand_index, grid matrices ...)
are not registered here; load reference checkpoints with strict=False for buffers.
"""
import copy
import math
from typing import Dict, Optional, Tuple, Union

import torch
import torch.nn as nn
from torch import Tensor

from .. import ops, so3
from ..nn import Linear


# ----------------------------------------------------------------------------------------------- containers / helpers
class SO3_Embedding:
    """Duck-type of the reference container (EF:273-399): `.embedding [N,K,C]`, lmax/mmax lists, channel count."""

    def __init__(self, length: int, lmax_list: list, num_channels: int, dtype=torch.float32, device: str = "cuda",
                 embedding: Optional[Tensor] = None) -> None:
        self.num_channels = num_channels
        self.device = device
        self.dtype = dtype
        self.num_resolutions = len(lmax_list)
        self.num_coefficients = sum(int((l + 1) ** 2) for l in lmax_list)
        if embedding is None:
            embedding = torch.zeros(length, self.num_coefficients, num_channels, device=device, dtype=dtype)
        self.set_embedding(embedding)
        self.set_lmax_mmax(list(lmax_list), list(lmax_list))

    def clone(self):
        return SO3_Embedding(0, self.lmax_list.copy(), self.num_channels, self.dtype, self.device, self.embedding.clone())

    def set_embedding(self, embedding) -> None:
        self.length = len(embedding)
        self.embedding = embedding

    def set_lmax_mmax(self, lmax_list, mmax_list) -> None:
        self.lmax_list = lmax_list
        self.mmax_list = mmax_list


_edge_cache: Dict[tuple, ops.EdgeSet] = {}
_edge_pinned: Dict[int, ops.EdgeSet] = {}     # static batches (HIP-graph replay): edge_index storage -> its EdgeSet


def edge_set(edge_index: Tensor, n_src: int, n_dst: int) -> ops.EdgeSet:
    """Destination-sorted view of an edge list, cached per (storage, shape, sizes): the four edge types of a batch are
    sorted once and reused by all layers, by backward, and by the edge-degree embedding."""
    pinned = _edge_pinned.get(edge_index.data_ptr())
    if pinned is not None:
        return pinned
    key = (edge_index.data_ptr(), tuple(edge_index.shape), int(n_src), int(n_dst), edge_index._version)
    es = _edge_cache.get(key)
    if es is None:
        if len(_edge_cache) > 64:
            _edge_cache.clear()
        es = ops.EdgeSet(edge_index, n_src, n_dst)
        es._keepalive = edge_index
        _edge_cache[key] = es
    return es


class CoefficientMappingModule(nn.Module):
    """Index tables of EF:1413-1552 (single resolution). Kept for API parity; kernels use compile-time tables."""

    def __init__(self, lmax_list: list, mmax_list: list, device: str = "cuda") -> None:
        super().__init__()
        assert len(lmax_list) == 1, "single resolution only (as the shipped config)"
        self.lmax_list, self.mmax_list, self.device = lmax_list, mmax_list, device
        self.layout = so3.layout(int(lmax_list[0]), int(mmax_list[0]))
        self.m_size = list(self.layout.m_size)

    def coefficient_idx(self, lmax: int, mmax: int):
        return torch.as_tensor(so3.layout(lmax, mmax).reduced, device=self.device)


class SO3_Rotation(nn.Module):
    """Holds the edge frames of the current pass (EF:472-528). `set_wigner` keeps the 3x3 frames; the reduced Wigner
    rows for a destination-sorted EdgeSet are produced on first use by the k2 kernel and cached for the pass
    (they are layer-invariant, EMB:238-239)."""

    def __init__(self, lmax: int, device: str = "cuda"):
        super().__init__()
        self.lmax, self.device = lmax, device
        self._rot, self._rows = None, {}

    def set_wigner(self, rot_mat3x3: Tensor):
        self._rot = rot_mat3x3.detach()
        self._rows = {}

    def rows_for(self, es: ops.EdgeSet, mmax: int) -> Tensor:
        wr = self._rows.get(id(es))
        if wr is None:
            assert self._rot is not None and self._rot.shape[0] == es.E, "set_wigner() was not called for these edges"
            wr = ops.wigner_rows(self._rot.index_select(0, es.order), self.lmax, mmax)
            self._rows[id(es)] = wr
        return wr


class SO3_Grid(nn.Module):
    """Placeholder with the reference's name (EF:531-621): grid matrices are built by singa_amd.so3.s2_grid and cached
    per device inside ops; nothing to register."""

    def __init__(self, lmax: int, mmax: int, normalization: str = "component", resolution=None, device: str = "cuda"):
        super().__init__()
        self.lmax, self.mmax = lmax, mmax


class ModuleListInfo(nn.ModuleList):
    def __init__(self, info_str, modules=None) -> None:
        super().__init__(modules)
        self.info_str = str(info_str)

    def __repr__(self):
        return self.info_str


# ----------------------------------------------------------------------------------------------- small modules
class RadialFunction(nn.Module):
    """Linear-LayerNorm-SiLU x2 + Linear (EF:1634-1657); same Sequential indices (net.0,1,3,4,6)."""

    def __init__(self, channels_list, device: str = "cuda") -> None:
        super().__init__()
        modules, input_channels = [], channels_list[0]
        for i in range(1, len(channels_list)):
            modules.append(Linear(input_channels, channels_list[i], bias=True, device=device))
            input_channels = channels_list[i]
            if i == len(channels_list) - 1:
                break
            modules.append(nn.LayerNorm(channels_list[i], device=device))
            modules.append(nn.SiLU())
        self.net = nn.Sequential(*modules)

    def forward(self, inputs):
        x, mods, i = inputs, list(self.net), 0
        while i < len(mods):
            m = mods[i]
            if (isinstance(m, nn.LayerNorm) and x.shape[-1] == 16 and i + 1 < len(mods)
                    and isinstance(mods[i + 1], nn.SiLU)):
                x = ops.ln_silu(x, m.weight, m.bias, m.eps)              # net.1+net.2, net.4+net.5 as one kernel each
                i += 2
            else:
                x = m(x)
                i += 1
        return x


class SmoothLeakyReLU(nn.Module):
    def __init__(self, negative_slope: float = 0.2) -> None:
        super().__init__()
        self.alpha = negative_slope

    def forward(self, x):
        return ((1 + self.alpha) / 2) * x + ((1 - self.alpha) / 2) * x * (2 * torch.sigmoid(x) - 1)


class GaussianSmearing(nn.Module):
    def __init__(self, start=-5.0, stop=5.0, num_gaussians=50, basis_width_scalar=1.0, device: str = "cuda") -> None:
        super().__init__()
        self.num_output = num_gaussians
        offset = torch.linspace(start, stop, num_gaussians, device=device)
        self.coeff = -0.5 / (basis_width_scalar * (offset[1] - offset[0])).item() ** 2
        self.register_buffer("offset", offset)

    def forward(self, dist) -> Tensor:
        dist = dist.view(-1, 1) - self.offset.view(1, -1)
        return torch.exp(self.coeff * torch.pow(dist, 2))


class SO3_LinearV2(nn.Module):
    """Per-degree linear map with bias on l = 0 (EF:624-674).  Computed as one batched GEMM over the K coefficient
    rows with the weight expanded by degree."""

    def __init__(self, in_features, out_features, lmax, bias: bool = True, device: str = "cuda"):
        super().__init__()
        self.device, self.in_features, self.out_features, self.lmax = device, in_features, out_features, lmax
        self.weight = nn.Parameter(torch.empty(lmax + 1, out_features, in_features, device=device))
        bound = 1 / math.sqrt(in_features)
        nn.init.uniform_(self.weight, -bound, bound)
        self.bias = nn.Parameter(torch.zeros(out_features, device=device))
        self._deg = None

    def apply_tensor(self, x: Tensor, residual: Optional[Tensor] = None) -> Tensor:
        return ops.so3_linear(x, self.weight, self.bias, self.lmax, residual)

    def forward(self, input_embedding: SO3_Embedding) -> SO3_Embedding:
        out = self.apply_tensor(input_embedding.embedding)
        return SO3_Embedding(0, input_embedding.lmax_list.copy(), self.out_features, input_embedding.dtype, self.device, out)


class EquivariantRMSNormArraySphericalHarmonicsV2(nn.Module):
    """EF:2099-2192 as instantiated by get_normalization_layer (Q3): centred, degree-balanced, affine + l=0 bias."""

    def __init__(self, lmax, num_channels, eps: float = 1e-5, affine: bool = True, centering: bool = True,
                 std_balance_degrees: bool = True, normalization: str = "component", device: str = "cuda"):
        super().__init__()
        assert affine and centering and std_balance_degrees, "only the configuration the reference instantiates is built"
        self.lmax, self.num_channels, self.eps = lmax, num_channels, eps
        self.affine_weight = nn.Parameter(torch.ones(lmax + 1, num_channels, device=device))
        self.affine_bias = nn.Parameter(torch.zeros(num_channels, device=device))

    def forward(self, node_input: Tensor) -> Tensor:
        return ops.so3_rmsnorm(node_input, self.affine_weight, self.affine_bias, self.lmax, self.eps)

    def forward_skip(self, node_input: Tensor):
        """-> (norm(x), x) with both uses of x in one autograd node (the residual branch of a TransBlockV2): the backward
        kernel adds the residual's gradient itself."""
        return ops.so3_rmsnorm_skip(node_input, self.affine_weight, self.affine_bias, self.lmax, self.eps)


def get_normalization_layer(norm_type, lmax, num_channels, eps: float = 1e-5, affine: bool = True,
                            normalization: str = "component", device: str = "cuda"):
    assert norm_type == "rms_norm_sh", "the shipped config uses rms_norm_sh (config/train.yml:41)"
    # the reference passes `normalization` into the `centering` slot (EF:2273): truthy -> centred (Q3)
    return EquivariantRMSNormArraySphericalHarmonicsV2(lmax, num_channels, eps, affine, True, device=device)


# ----------------------------------------------------------------------------------------------- SO(2) convolution
_pass_token = [0, False]
_bw_cache: Dict[int, Tensor] = {}          # id(SO2_m_Convolution) -> its block weight, alive for ONE forward pass only


class forward_pass:
    """`with forward_pass():` brackets one EquivariantEmbedding.forward.  Inside it, parameter-derived tensors (the SO(2)
    block weights) are built once and shared by the homogeneous and heterogeneous passes; the cache is emptied when the
    pass ends: the cached tensors carry the autograd history of the pass that built them, and a history kept alive past its
    pass pins that pass's AccumulateGrad nodes (and their stream) - an eager backward followed by a graph capture on
    another stream then crashed inside the capture."""

    def __enter__(self):
        _pass_token[0] += 1
        _pass_token[1] = True
        _bw_cache.clear()

    def __exit__(self, *a):
        _pass_token[1] = False
        _bw_cache.clear()
        return False


class SO2_m_Convolution(nn.Module):
    """Weights of the order-m SO(2) convolution (EF:677-729): fc.weight = [Wr; Wi].  SO2_Convolution hands them to the complex
    GEMM (k7c) as they are.  `block_weight()` returns [[Wr,-Wi],[Wi,Wr]] so that [x_+m | x_-m] @ block^T = [x_+ Wr^T - x_- Wi^T |
    x_+ Wi^T + x_- Wr^T] = (real | imag) in one REAL GEMM - the form used for other mmax than 2 and by the tests' cross-check."""

    def __init__(self, m, sphere_channels, m_output_channels, lmax_list, mmax_list, device: str = "cuda"):
        super().__init__()
        self.m = m
        num_coefficients = lmax_list[0] - m + 1
        num_channels = num_coefficients * sphere_channels
        self.fc = Linear(num_channels, 2 * m_output_channels * num_coefficients, bias=False, device=device)
        self.fc.weight.data.mul_(1 / math.sqrt(2))

    def block_weight(self) -> Tensor:
        """Built once per forward pass of the model (`forward_pass`): the blocks are shared by the homogeneous and the
        two heterogeneous passes, which would otherwise each rebuild (and back-propagate through) the same four cats."""
        hit = _bw_cache.get(id(self)) if _pass_token[1] else None
        if hit is not None and hit[1] == torch.is_grad_enabled():
            return hit[0]
        bw = ops.block_weight(self.fc.weight)                         # one launch (and one for its gradient)
        if _pass_token[1]:
            _bw_cache[id(self)] = (bw, torch.is_grad_enabled())
        return bw


class SO2_Convolution(nn.Module):
    """SO(2) convolution over all orders (EF:732-875) on an m-primary edge matrix X [E, KR*Cin]: a real GEMM for m = 0 and a
    complex (3M) GEMM launch for m = 1, 2.  precision: "f32", or "bf16" - the convolution's GEMMs, real and complex, forward and
    backward, round their operands to bfloat16 inside the kernel (ops.so2_conv3m); set by EquivariantEmbedding(precision=...)."""

    precision = "f32"

    def __init__(self, sphere_channels: int, m_output_channels: int, lmax_list: list, mmax_list: list, mappingReduced,
                 edge_channels_list=None, extra_m0_output_channels=None, internal_weights: bool = True,
                 device: str = "cuda"):
        super().__init__()
        self.sphere_channels, self.m_output_channels = sphere_channels, m_output_channels
        self.lmax_list, self.mmax_list = lmax_list, mmax_list
        self.layout = so3.layout(int(lmax_list[0]), int(mmax_list[0]))
        self.extra_m0_output_channels = extra_m0_output_channels
        n0 = (lmax_list[0] + 1) * sphere_channels
        out0 = m_output_channels * (lmax_list[0] + 1) + (extra_m0_output_channels or 0)
        self.fc_m0 = Linear(n0, out0, device=device)
        num_channels_rad = n0
        self.so2_m_conv = nn.ModuleList()
        for m in range(1, max(mmax_list) + 1):
            self.so2_m_conv.append(SO2_m_Convolution(m, sphere_channels, m_output_channels, lmax_list, mmax_list, device))
            num_channels_rad += self.so2_m_conv[-1].fc.in_features
        self.rad_func = None
        if not internal_weights:
            ecl = copy.deepcopy(edge_channels_list)
            ecl.append(int(num_channels_rad))
            self.rad_func = RadialFunction(ecl, device=device)

    def forward(self, X: Tensor):
        """X: [E, KR*Cin] m-primary (radial weights already applied).  Returns the per-m outputs
        (y0 [E, extra + (L+1)*Cout], y1 [E, 2*L*Cout], y2 [E, 2*(L-1)*Cout]), each m-primary and contiguous."""
        c = self.sphere_channels
        st = self.layout.seg_start
        if len(self.so2_m_conv) == 2:
            # m = 1, 2 as complex products in three real multiplications on the fc weights themselves (k7c)
            return list(ops.so2_conv3m(X, self.fc_m0.weight, self.fc_m0.bias, self.so2_m_conv[0].fc.weight,
                                       self.so2_m_conv[1].fc.weight, st[1] * c, (st[2] - st[1]) * c, self.precision))
        outs = [ops.linear(X[:, : st[1] * c], self.fc_m0.weight, self.fc_m0.bias, self.precision)]
        for i, conv in enumerate(self.so2_m_conv):
            outs.append(ops.linear(X[:, st[i + 1] * c: st[i + 2] * c], conv.block_weight(), precision=self.precision))
        return outs


# ----------------------------------------------------------------------------------------------- edge-degree embedding
class EdgeDegreeEmbedding(nn.Module):
    """EF:23-149: radial MLP -> m=0 coefficients -> rotate back -> sum over incoming edges -> / rescale_factor.
    The zero-padding, l-primary permutation, bmm and index_add_ of the reference are one kernel (k13)."""

    def __init__(self, sphere_channels: int, lmax_list: list, mmax_list: list, SO3_rotation, mappingReduced,
                 max_num_elements: int, edge_channels_list: list, use_atom_edge_embedding: bool, rescale_factor: float,
                 device: str = "cuda") -> None:
        super().__init__()
        assert not use_atom_edge_embedding, "shared atom-edge embedding only (as EMB:154)"
        self.sphere_channels, self.lmax_list, self.mmax_list = sphere_channels, lmax_list, mmax_list
        object.__setattr__(self, "SO3_rotation", SO3_rotation)
        self.m_0_num_coefficients = lmax_list[0] + 1
        ecl = copy.deepcopy(edge_channels_list)
        ecl.append(self.m_0_num_coefficients * sphere_channels)
        self.rad_func = RadialFunction(ecl, device=device)
        self.rescale_factor = rescale_factor
        self.device = device

    def forward(self, atomic_numbers: Union[Tensor, Dict], edge_distance: Tensor, edge_index: Tensor, hetero: bool,
                source_target: Optional[Tuple[str, str]] = None):
        assert hetero is not None, "Please specify args: hetero"
        if hetero:
            n_src, n_dst = atomic_numbers[source_target[0]].shape[0], atomic_numbers[source_target[1]].shape[0]
        else:
            n_src = n_dst = atomic_numbers.shape[0]
        es = edge_set(edge_index, n_src, n_dst)
        L, M = self.lmax_list[0], self.mmax_list[0]
        wr = self.SO3_rotation[0].rows_for(es, M)
        r = self.rad_func(edge_distance.index_select(0, es.order))
        out = ops.edge_degree_scatter(r, wr, es, L, M, 1.0 / self.rescale_factor)
        return SO3_Embedding(0, self.lmax_list.copy(), self.sphere_channels, out.dtype, self.device, out)


# ----------------------------------------------------------------------------------------------- attention
class SO2EquivariantGraphAttention(nn.Module):
    """EF:878-1204 for the configuration the reference instantiates (shared atom-edge embedding, separable S2
    activation, attention re-normalisation, no dropout)."""

    def __init__(self, sphere_channels, hidden_channels, num_heads: int, attn_alpha_channels, attn_value_channels,
                 output_channels, lmax_list: list, mmax_list: list, SO3_rotation, mappingReduced, SO3_grid,
                 max_num_elements, edge_channels_list: list, use_atom_edge_embedding: bool = True,
                 use_m_share_rad: bool = False, activation: str = "scaled_silu", use_s2_act_attn: bool = False,
                 use_attn_renorm: bool = True, use_gate_act: bool = False, use_sep_s2_act: bool = True,
                 alpha_drop: float = 0.0, device: str = "cuda", recompute: bool = False):
        super().__init__()
        assert not use_atom_edge_embedding and not use_m_share_rad and not use_s2_act_attn and use_attn_renorm
        assert not use_gate_act and use_sep_s2_act and alpha_drop == 0.0
        if recompute and max(mmax_list) != 2:
            raise ValueError(f"recompute=True: the attention block rebuilds its activation for mmax = 2 only, got mmax_list {mmax_list}")
        self.recompute = recompute      # the S2 activation between the two SO(2) convolutions is rebuilt in backward, not held
        self.sphere_channels, self.hidden_channels, self.num_heads = sphere_channels, hidden_channels, num_heads
        self.attn_alpha_channels, self.attn_value_channels = attn_alpha_channels, attn_value_channels
        self.output_channels, self.lmax_list, self.mmax_list, self.device = output_channels, lmax_list, mmax_list, device
        object.__setattr__(self, "SO3_rotation", SO3_rotation)
        extra = num_heads * attn_alpha_channels + hidden_channels
        self.so2_conv_1 = SO2_Convolution(2 * sphere_channels, hidden_channels, lmax_list, mmax_list, mappingReduced,
                                          internal_weights=False, edge_channels_list=copy.deepcopy(edge_channels_list),
                                          extra_m0_output_channels=extra, device=device)
        self.alpha_norm = nn.LayerNorm(attn_alpha_channels, device=device)
        self.alpha_act = SmoothLeakyReLU()
        self.alpha_dot = nn.Parameter(torch.empty(num_heads, attn_alpha_channels, device=device))
        std = 1.0 / math.sqrt(attn_alpha_channels)
        nn.init.uniform_(self.alpha_dot, -std, std)
        self.so2_conv_2 = SO2_Convolution(hidden_channels, num_heads * attn_value_channels, lmax_list, mmax_list,
                                          mappingReduced, internal_weights=True, device=device)
        self.proj = SO3_LinearV2(num_heads * attn_value_channels, output_channels, lmax=lmax_list[0], device=device)

    def forward(self, x, atomic_numbers: Union[Tensor, Dict], edge_distance: Tensor, edge_index: Tensor, hetero: bool,
                source_target: Optional[Tuple[str, str]] = None, residual: Optional[Tensor] = None):
        """`residual` (not in the reference's signature): a tensor added to the result inside the output projection's launch
        - TransBlockV2's `output + x_res` (EF:1383-1384)."""
        assert hetero is not None, "Please specify args: hetero"
        if isinstance(x, dict):
            x_src, x_dst = x[source_target[0]].embedding, x[source_target[1]].embedding
        else:
            x_src = x_dst = x.embedding
        L, M = self.lmax_list[0], self.mmax_list[0]
        es = edge_set(edge_index, x_src.shape[0], x_dst.shape[0])
        wr = self.SO3_rotation[0].rows_for(es, M)
        x_edge = edge_distance.index_select(0, es.order)
        H, heads, A = self.hidden_channels, self.num_heads, self.attn_alpha_channels
        # k3-k6: gather both endpoints, rotate into the edge frame, m-primary, times radial weights
        rad = self.so2_conv_1.rad_func(x_edge)
        X = ops.gather_rotate(x_src, x_dst, rad, wr, es, L, M)
        # first SO(2) convolution (three GEMMs); h0 = [alpha inputs | gate | m=0 rows]
        h0, h1, h2 = self.so2_conv_1(X)
        # k9a + k8 in one autograd node: attention logits (LayerNorm -> smooth leaky ReLU -> dot, EF:1175-1178) and the
        # separable S2 activation of the gated message (EF:1156-1160).  The softmax over each destination's edges follows
        # at once (it only needs the logits), so nothing streams between the conv2 GEMMs and the scatter kernel that
        # consumes their output: the per-m value tensors are then still largely resident in the Infinity Cache.
        if self.recompute:
            c2 = self.so2_conv_2
            logits, y0, y1, y2 = ops.edge_head_conv_recompute(
                h0, h1, h2, self.alpha_norm.weight, self.alpha_norm.bias, self.alpha_dot, c2.fc_m0.weight, c2.fc_m0.bias,
                c2.so2_m_conv[0].fc.weight, c2.so2_m_conv[1].fc.weight, heads, A, H, L, M, self.alpha_norm.eps, c2.precision)
            alpha = ops.segment_softmax(logits, es.row_ptr, 1e-16)
        else:
            logits, act = ops.edge_head(h0, h1, h2, self.alpha_norm.weight, self.alpha_norm.bias, self.alpha_dot, heads, A, H,
                                        L, M, self.alpha_norm.eps)
            alpha = ops.segment_softmax(logits, es.row_ptr, 1e-16)
            y0, y1, y2 = self.so2_conv_2(act)
        # k10: alpha * value, rotate back, sum over incoming edges
        agg = ops.rotate_back_scatter(y0, y1, y2, alpha, wr, es, heads, L, M)
        out = self.proj.apply_tensor(agg, residual)
        return SO3_Embedding(0, self.lmax_list.copy(), self.output_channels, out.dtype, self.device, out)


# ----------------------------------------------------------------------------------------------- feed-forward
class FeedForwardNetwork(nn.Module):
    """EF:152-270 with separable S2 activation on the [L][L] grid."""

    def __init__(self, sphere_channels: int, hidden_channels: int, output_channels: int, lmax_list: list,
                 mmax_list: list, SO3_grid, activation: str = "scaled_silu", use_gate_act: bool = False,
                 use_grid_mlp: bool = False, use_sep_s2_act: bool = True, device: str = "cuda",
                 recompute: bool = False) -> None:
        super().__init__()
        assert not use_gate_act and not use_grid_mlp and use_sep_s2_act
        if recompute and not (ops.USE_SKINNY_SO3 and (sphere_channels, hidden_channels, output_channels) == (16, 512, 16)):
            raise ValueError("recompute=True: the feed-forward block is rebuilt by the 16 -> 512 -> 16 kernels only "
                             f"(ops.USE_SKINNY_SO3, sphere_channels 16), got ffn_hidden_channels = {hidden_channels}, "
                             f"sphere_channels = {sphere_channels}, output {output_channels}")
        self.recompute = recompute      # neither [N, K, 512] tensor of the block is held for backward (ops._FFNRecompute)
        self.device, self.lmax_list, self.max_lmax = device, lmax_list, max(lmax_list)
        self.sphere_channels, self.hidden_channels, self.output_channels = sphere_channels, hidden_channels, output_channels
        self.so3_linear_1 = SO3_LinearV2(sphere_channels, hidden_channels, lmax=self.max_lmax, device=device)
        self.gating_linear = Linear(sphere_channels, hidden_channels, device=device)
        self.so3_linear_2 = SO3_LinearV2(hidden_channels, output_channels, lmax=self.max_lmax, device=device)

    def forward(self, input_embedding: SO3_Embedding, residual: Optional[Tensor] = None) -> SO3_Embedding:
        x = input_embedding.embedding
        gate = self.gating_linear(x[:, 0])
        if self.recompute:
            l1, l2 = self.so3_linear_1, self.so3_linear_2
            out = ops.ffn_recompute(x, gate, l1.weight, l1.bias, l2.weight, l2.bias, self.max_lmax, residual)
            return SO3_Embedding(0, input_embedding.lmax_list.copy(), self.output_channels, out.dtype, self.device, out)
        h = self.so3_linear_1.apply_tensor(x)
        if ops.USE_SKINNY_SO3 and self.hidden_channels == 512 and self.output_channels == 16:
            # activation + second linear (+ x_res of EF:1405-1406) as one autograd node: its backward forms the activation's
            # output gradient inside the activation's backward kernel (ops._FFNTail)
            out = ops.ffn_tail(h, gate, self.so3_linear_2.weight, self.so3_linear_2.bias, self.max_lmax, residual)
        else:
            h = ops.s2act_node(h, gate, self.max_lmax)
            out = self.so3_linear_2.apply_tensor(h, residual)         # (+ x_res of EF:1405-1406 in the same launch)
        return SO3_Embedding(0, input_embedding.lmax_list.copy(), self.output_channels, out.dtype, self.device, out)


# ----------------------------------------------------------------------------------------------- transformer block
class TransBlockV2(nn.Module):
    """EF:1207-1410 (drop rates 0, rms_norm_sh).  Hetero calls reproduce the in-place side effect on the shared
    dict (Q4): both stores are replaced by norm_1 of themselves."""

    def __init__(self, sphere_channels: int, attn_hidden_channels: int, attn_alpha_channels: int,
                 attn_value_channels: int, ffn_hidden_channels: int, output_channels: int, edge_channels_list: list,
                 lmax_list: list, mmax_list: list, SO3_rotation, mappingReduced, SO3_grid, num_heads: int,
                 max_num_elements: int, use_atom_edge_embedding: bool = True, use_m_share_rad: bool = False,
                 use_gate_act: bool = False, use_grid_mlp: bool = False, use_sep_s2_act: bool = True,
                 attn_activation: str = "silu", use_s2_act_attn: bool = False, use_attn_renorm: bool = True,
                 ffn_activation: str = "silu", norm_type: str = "rms_norm_sh", alpha_drop: float = 0.0,
                 drop_path_rate: float = 0.0, proj_drop: float = 0.0, device: str = "cuda", recompute: bool = False):
        super().__init__()
        assert drop_path_rate == 0.0 and proj_drop == 0.0 and sphere_channels == output_channels
        self.device = device
        max_lmax = max(lmax_list)
        self.norm_1 = get_normalization_layer(norm_type, lmax=max_lmax, num_channels=sphere_channels, device=device)
        self.norm_2 = get_normalization_layer(norm_type, lmax=max_lmax, num_channels=sphere_channels, device=device)
        self.ga = SO2EquivariantGraphAttention(
            sphere_channels=sphere_channels, hidden_channels=attn_hidden_channels, num_heads=num_heads,
            attn_alpha_channels=attn_alpha_channels, attn_value_channels=attn_value_channels,
            output_channels=sphere_channels, lmax_list=lmax_list, mmax_list=mmax_list, SO3_rotation=SO3_rotation,
            mappingReduced=mappingReduced, SO3_grid=SO3_grid, max_num_elements=max_num_elements,
            edge_channels_list=edge_channels_list, use_atom_edge_embedding=use_atom_edge_embedding,
            use_m_share_rad=use_m_share_rad, activation=attn_activation, use_s2_act_attn=use_s2_act_attn,
            use_attn_renorm=use_attn_renorm, use_gate_act=use_gate_act, use_sep_s2_act=use_sep_s2_act,
            alpha_drop=alpha_drop, device=device, recompute=recompute)
        self.ffn = FeedForwardNetwork(sphere_channels=sphere_channels, hidden_channels=ffn_hidden_channels,
                                      output_channels=output_channels, lmax_list=lmax_list, mmax_list=mmax_list,
                                      SO3_grid=SO3_grid, activation=ffn_activation, use_gate_act=use_gate_act,
                                      use_grid_mlp=use_grid_mlp, use_sep_s2_act=use_sep_s2_act, device=device,
                                      recompute=recompute)

    def renorm_only(self, x: Dict, source_target: Tuple[str, str]) -> None:
        """The only effect of a hetero call whose return value the caller discards (EMB:415-428 keeps just the last
        layer's output): both dict entries are overwritten with norm_1 of themselves (EF:1356-1357)."""
        source, target = source_target
        x[source].embedding = self.norm_1(x[source].embedding)
        x[target].embedding = self.norm_1(x[target].embedding)

    def renorm_with_residual(self, x: Dict, source_target: Tuple[str, str]) -> Tensor:
        """renorm_only for a layer whose output IS used: returns the target's embedding from before the norm (the block's
        residual, EF:1356) tied to the norm in one autograd node."""
        source, target = source_target
        x[source].embedding = self.norm_1(x[source].embedding)
        x[target].embedding, x_res = self.norm_1.forward_skip(x[target].embedding)
        return x_res

    def forward(self, x: Union[SO3_Embedding, Dict], atomic_numbers: Union[Tensor, Dict], edge_distance: Tensor,
                edge_index: Tensor, batch: int, hetero: bool, source_target: Optional[Tuple[str, str]] = None,
                renormed_residual: Optional[Tensor] = None):
        """renormed_residual (hetero only): the caller has applied `renorm_only` already and hands over the target's
        embedding from before it (the block's residual) - the dict is then only read."""
        if isinstance(x, dict):
            assert hetero and source_target is not None
            if renormed_residual is None:
                x_res = self.renorm_with_residual(x, source_target)
            else:
                x_res = renormed_residual
            out = self.ga(x, atomic_numbers, edge_distance, edge_index, hetero, source_target, residual=x_res)
        else:
            x.embedding, x_res = self.norm_1.forward_skip(x.embedding)
            out = self.ga(x, atomic_numbers, edge_distance, edge_index, hetero, residual=x_res)
        # (both residual sums of the block ride in the epilogue of the SO3 linear in front of them, and their gradients in
        # the backward kernel of the norm they bypass: forward_skip)
        out.embedding, x_res = self.norm_2.forward_skip(out.embedding)
        return self.ffn(out, residual=x_res)


_frame_flags: Dict[str, Tensor] = {}      # device -> [min edge length, max |cos(edge, helper)|] seen under graph capture


def _frame_flag_tensor(device) -> Tensor:
    key = str(device)
    if key not in _frame_flags:
        _frame_flags[key] = torch.tensor([float("inf"), 0.0], device=device)
    return _frame_flags[key]


def _judge_frames(dmin: float, dotmax: float) -> None:
    """The reference's two guards: edges shorter than 1e-4 are only reported (EF:2292-2297, a print there - a warning
    here); a helper vector still aligned with the edge after both swaps aborts (EF:2329, an assert there - RuntimeError
    here; `not <` so that the NaN of a zero-length edge fails like it fails the reference's assert)."""
    import warnings
    if dmin < 0.0001:
        warnings.warn("Error edge_vec_0_distance: {}".format(dmin), RuntimeWarning, stacklevel=3)
    if not dotmax < 0.99:
        raise RuntimeError(f"init_edge_rot_mat: helper vector aligned with an edge (max |cos| = {dotmax}); "
                           "zero-length edge or degenerate random draw (reference EF_layers.py:2329)")


def check_edge_frames(device=None, reset: bool = True) -> None:
    """Evaluate the guards for the frames built inside captured HIP graphs (where a host read-back is impossible, the
    statistics are accumulated on the device instead): one read-back, then the same warning / RuntimeError.  Called by
    the training loop whenever it reads the loss back (TrainStep.check)."""
    for key, t in list(_frame_flags.items()):
        if device is not None and key != str(device):
            continue
        dmin, dotmax = t.tolist()
        if reset:
            t.copy_(torch.tensor([float("inf"), 0.0]))
        if dmin != float("inf"):
            _judge_frames(dmin, dotmax)


def init_edge_rot_mat(edge_distance_vec: Tensor, device: str = "cuda", rand: Optional[Tensor] = None) -> Tensor:
    """Edge frames (EF:2286-2351) by the k1 kernel (ops.edge_frames): one launch builds the frames and folds the two
    statistics the reference's guards need.  `rand` is the uniform [0,1) draw the reference takes from torch.rand_like
    (Q6); pass it explicitly for reproducible parity, otherwise it is drawn on the tensor's device.  Both guards of the
    reference are kept (`_judge_frames`): evaluated at once in eager mode (one read-back), accumulated on the device
    under graph capture (`check_edge_frames`)."""
    v = edge_distance_vec
    if v.shape[0] == 0:
        return v.new_zeros(0, 3, 3)
    if rand is None:
        rand = torch.rand_like(v)
    capturing = v.is_cuda and torch.cuda.is_current_stream_capturing()
    stats = _frame_flag_tensor(v.device) if capturing else torch.tensor([float("inf"), 0.0], device=v.device)
    rot = ops.edge_frames(v, rand, stats)
    if not capturing:
        _judge_frames(*stats.tolist())
    return rot
