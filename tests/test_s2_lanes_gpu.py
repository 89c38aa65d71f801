"""-m gpu: the separable S2 activation's forward kernel in its two lane forms.  singa_s2act_sep_fwd runs two channels per thread
(packed f32) where gate, every segment and `out` start 8-byte aligned and every pitch is even, and one channel per thread
otherwise; both come from one kernel body and are held to each other bit for bit here, through the C ABI itself (ops._rows
would copy a misaligned view).  Also: ops.s2act_node / ops.s2act_edge on an empty set."""
import numpy as np
import pytest
import torch

from oracle import singa_oracle as O
from singa_amd import _capi, so3
from tests.helpers import S2_LANE_LAYOUTS, s2_lane_layout

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _forward(name, L, edge, x, gate):
    """singa_s2act_sep_fwd on the values x [E, KIN, C], gate [E, C] in layout `name` -> out [E, KIN, C] (checked: margins intact)"""
    from singa_amd import _lib, ops
    ops._dev(x, gate)
    E, KIN, C = x.shape
    M = 2 if edge else L
    rows = list(so3.layout(L, M).seg_rows) if edge else [KIN]
    tabs = ops._grid_factors(L, M, edge, x.device)

    def alloc(n):
        buf = torch.full((n,), float("nan"), device=DEV, dtype=torch.float32)
        return buf, buf.data_ptr()

    lo = s2_lane_layout(name, rows, C, E, alloc)
    lo["gate"].copy_(gate)
    at = 0
    for v, r in zip(lo["x"], rows):
        v.copy_(x[:, at:at + r].reshape(E, r * C))
        at += r
    seg, n = _capi.segs(lo["items"])
    _capi.check(_lib.lib(), _lib.lib().singa_s2act_sep_fwd(seg, n, lo["gate_ptr"], lo["ldg"], *[ops._p(t) for t in tabs], lo["out_ptr"],
                                                          E, C, L, ops._stream()), f"singa_s2act_sep_fwd ({name})")
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(m).all()) for m in lo["margins"]), name
    return lo["out"].reshape(E, KIN, C).clone()


# edge grid: two workgroups of the two-channel form (5 * 64 threads), the second partial; three of the one-channel form
@pytest.mark.parametrize("L,edge", [(2, True), (4, True), (6, True), (2, False), (4, False)])
def test_one_channel_form_equals_two_channel_form(L, edge):
    """Every layout that misses the pairing rule by one clause gives the bits of the paired layout.
    (This found the L = 6 edge grid's one-channel kernel out of step - 7247 of 18560 elements, up to 5.4e-07 at |y| = 5.4: the
    compiler vectorised its rolled ring loop ahead of the contraction of SiLU's product that every other instantiation gets.
    The kernel now unrolls that loop; see s2act_sep_fwd_kernel.)"""
    g = torch.Generator().manual_seed(900 + L)
    E, C, KIN = (5, 128, 5 * L - 1) if edge else (2, 512, (L + 1) ** 2)
    x, gate = torch.randn(E, KIN, C, generator=g).to(DEV), torch.randn(E, C, generator=g).to(DEV)
    paired = _forward("paired", L, edge, x, gate)
    assert not bool(torch.isnan(paired).any())
    outs = {name: _forward(name, L, edge, x, gate) for name in S2_LANE_LAYOUTS[1:]}
    for name, out in outs.items():
        print(f"L = {L} {'edge' if edge else 'node'}, {name}: {int((out != paired).sum())} of {out.numel()} elements differ, "
              f"max |difference| {float((out - paired).abs().max()):.3e} at max |value| {float(paired.abs().max()):.3f}")
    for name, out in outs.items():
        assert torch.equal(out, paired), name


def test_l6_node_grid_is_one_channel_in_every_layout():
    """(167 registers per channel: the launcher never pairs this grid.)  Against the oracle at test_s2act_edge_and_node's bound."""
    L, N, C = 6, 2, 512
    g = torch.Generator().manual_seed(906)
    x, gate = torch.randn(N, (L + 1) ** 2, C, generator=g), torch.randn(N, C, generator=g)
    ref = O.sep_s2_act(gate, x, L, L).double()
    for name in S2_LANE_LAYOUTS:
        out = _forward(name, L, False, x.to(DEV), gate.to(DEV)).cpu().double()
        assert float((out - ref).norm() / ref.norm()) < 2e-5, name


def test_s2act_on_empty_sets():
    """No rows, no launch: empty results and empty gradients of the right shapes."""
    from singa_amd import ops
    L, C, extra = 2, 128, 32
    lay = so3.layout(L, 2)
    hs = [torch.zeros(0, w, device=DEV, requires_grad=True)
          for w in (extra + C + lay.seg_rows[0] * C, lay.seg_rows[1] * C, lay.seg_rows[2] * C)]
    out = ops.s2act_edge(hs[0], hs[1], hs[2], extra, extra + C, C, L)
    assert out.shape == (0, lay.KR * C)
    out.sum().backward()
    assert all(h.grad is not None and h.grad.shape == h.shape for h in hs)
    x = torch.zeros(0, (L + 1) ** 2, 512, device=DEV, requires_grad=True)
    gate = torch.zeros(0, 512, device=DEV, requires_grad=True)
    out = ops.s2act_node(x, gate, L)
    assert out.shape == x.shape
    out.sum().backward()
    assert x.grad.shape == x.shape and gate.grad.shape == gate.shape
