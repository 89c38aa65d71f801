"""-m gpu: the decoder step kernels (k17: singa_dec_self_attn / singa_dec_cross_attn / singa_dec_ffn through
ops.dec_layer_step) against an independent float64 reference, in the regimes generation runs in: all 256 cache positions
(the four 64-lane passes of the score loop, the last cache slot), encoder lengths on both sides of the 64-lane stride and
at the kernel's limit of 1024, ragged and fully padded proteins, rows = proteins x beams with beams > 1.

Reference: ONE decoder layer evaluated the way the reference model does it - on the whole sequence at once with a causal
mask (oracle.singa_oracle.dense_mha / pos_ffn, plain torch, fed float64 tensors; masked_fill(-1e9) + softmax, so a fully
padded protein gets the uniform average of its value rows).  Device: ops.dec_layer_step position by position with the
weights laid out by BeamSearch.KVDecoder.  Every position's output row and the whole written key / value cache are
compared per row (tests.helpers.rowwise_err) with the 2e-5 bound the project uses for k17 against the library path.
The float32 evaluation of the same layer on the CPU deviates by 4.4e-7 per row from the float64 one; the kernels, measured
on MI355X: outputs 2.8e-7 .. 3.8e-7, key cache 2.4e-7 .. 2.8e-7, value cache 2.2e-7 .. 2.3e-7 over all cases (`__expf` in
the softmax included), the same in each of the four 64-position ranges.  With the score loop reading `lane + 64 * (m & 1)`
instead of `lane + 64 * m`, every comparison with the reference here fails (the graph-replay test compares the kernels with
themselves) while tests/test_beam_gpu.py and tests/test_kernels_gpu.py pass.
"""
import math
from types import SimpleNamespace

import pytest
import torch

from oracle import singa_oracle as O
from tests.helpers import rowwise_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 2e-5
B, BEAMS, P = 3, 5, 256            # rows = 15: r / beams is not the identity, and the row count is not a multiple of 4
R = B * BEAMS


def make_layer(seed):
    """One DecoderLayer of the shipped geometry (hidden 256, 4 heads of 32 / 64 channels, FFN 1024) with random weights
    (randn / sqrt(fan_in); biases and LayerNorm affines away from their initial 0 / 1) and the same weights as the float64
    state dict the oracle functions read (prefix 'l.')."""
    from singa_amd.config import Config
    from singa_amd.model.CProMG import DecoderLayer
    cfg = Config()
    cfg.hidden_channels, cfg.key_channels, cfg.num_heads = 256, 128, 4
    layer = DecoderLayer(cfg, device=DEV)
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, p in layer.state_dict().items():
        if name.endswith("layer_norm.weight"):
            v = 1 + 0.1 * torch.randn(p.shape, generator=g)
        elif p.dim() == 1:
            v = 0.1 * torch.randn(p.shape, generator=g)
        else:
            v = torch.randn(p.shape, generator=g) / math.sqrt(p.shape[1])
        sd[name] = v
    layer.load_state_dict(sd)
    return layer, {"l." + k: v.double() for k, v in sd.items()}


def make_kv(layer, enc, pad):
    """A one-layer KVDecoder: the transposed weights and the projected encoder keys / values exactly as generation has them."""
    from singa_amd.model.BeamSearch import KVDecoder
    dec = SimpleNamespace(layers=[layer], num_props=0)
    with torch.no_grad():
        kv = KVDecoder(dec, None, enc.to(DEV), pad.to(DEV), BEAMS, P, 1, fused=True, search_buffers=False)
    assert kv.fused
    return kv


def reference(sd, x, enc, pad):
    """x [R, P, 256] f64 -> (layer output [R, P, 256], K [R, 4, P, 32], V [R, 4, P, 64]): one causal attention over all
    positions, the encoder rows of protein r // BEAMS."""
    n = x.shape[1]
    causal = torch.triu(torch.ones(n, n, dtype=torch.bool), 1).unsqueeze(0).expand(x.shape[0], n, n)
    enc_r = enc.double().repeat_interleave(BEAMS, 0)
    mask = pad.repeat_interleave(BEAMS, 0).expand(x.shape[0], n, pad.shape[2])
    with torch.no_grad():
        y = O.dense_mha(sd, "l.dec_self_attn", x, x, x, causal)
        y = O.dense_mha(sd, "l.dec_enc_attn", y, enc_r, enc_r, mask)
        out = O.pos_ffn(sd, "l.pos_ffn", y)
        k = O.lin(sd, "l.dec_self_attn.W_K", x).view(x.shape[0], n, 4, 32).transpose(1, 2)
        v = O.lin(sd, "l.dec_self_attn.W_V", x).view(x.shape[0], n, 4, 64).transpose(1, 2)
    return out, k, v


def inputs(S, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, P, 256, generator=g)
    enc = torch.randn(B, S, 256, generator=g)
    pad = torch.zeros(B, 1, S, dtype=torch.bool)
    pad[1, 0, max(1, (2 * S) // 3):] = True               # ragged: protein 1 is shorter than the batch's longest
    pad[2] = True                                         # protein 2: every position is padding
    return x, enc, pad


def decode(kv, x, follow_at=None, src=None):
    """All of x's positions through the step kernels -> outputs [R, n, 256] (CPU)."""
    outs = []
    for pos in range(x.shape[1]):
        if pos == follow_at:
            kv.follow(src.to(DEV))
        outs.append(kv.advance(x[:, pos].to(DEV)).cpu())
    torch.cuda.synchronize()
    return torch.stack(outs, 1)


def check(tag, got, kv, want, wk, wv):
    n = want.shape[1]
    e_out = rowwise_err(got.reshape(-1, 256), want.reshape(-1, 256), f"{tag} outputs (row = decoder row * {n} + position)")
    e_k = rowwise_err(kv.k[0, :, :, :n].cpu().reshape(-1, 32), wk.reshape(-1, 32), f"{tag} key cache")
    e_v = rowwise_err(kv.v[0, :, :, :n].cpu().reshape(-1, 64), wv.reshape(-1, 64), f"{tag} value cache")
    # the four score passes separately: positions 64 m .. 64 m + 63 are the first to read pass m
    for m in range((n + 63) // 64):
        rowwise_err(got[:, 64 * m:64 * m + 64].reshape(-1, 256), want[:, 64 * m:64 * m + 64].reshape(-1, 256),
                    f"{tag} outputs at positions {64 * m}..{min(n, 64 * m + 64) - 1}")
    assert e_out <= TOL and e_k <= TOL and e_v <= TOL, (tag, e_out, e_k, e_v)


@pytest.mark.parametrize("S", [1, 63, 64, 65, 300, 1024])
def test_all_256_positions_against_float64(S):
    """Every cache position 0..255 (score passes m = 0..3, the last cache slot) for 3 proteins x 5 beams, encoder lengths
    around the 64-lane stride of the cross attention and at its limit, ragged and fully padded proteins."""
    layer, sd = make_layer(S)
    x, enc, pad = inputs(S, 1000 + S)
    kv = make_kv(layer, enc, pad)
    assert kv.P == 256 and kv.R == 15 and bool(pad[2].all()) and not bool(pad[0].any())
    with torch.no_grad():
        got = decode(kv, x)
    assert int(kv.pos) == 256                              # the last slot of the cache was written
    want, wk, wv = reference(sd, x.double(), enc, pad)
    check(f"S={S}", got, kv, want, wk, wv)


def test_cache_rows_follow_a_permutation():
    """After 100 positions the cache rows are re-ranked as a beam-search step does (KVDecoder.follow, rows exchanged inside
    a protein), then decoding continues to position 255: row r must reproduce the reference of the row whose prefix it took
    over (inputs of row src[r] up to position 99, its own from 100 on)."""
    S, cut = 300, 100
    layer, sd = make_layer(7)
    x, enc, pad = inputs(S, 77)
    g = torch.Generator().manual_seed(5)
    src = torch.cat([torch.randperm(BEAMS, generator=g) + b * BEAMS for b in range(B)])
    assert not torch.equal(src, torch.arange(R)) and torch.equal(src // BEAMS, torch.arange(R) // BEAMS)
    kv = make_kv(layer, enc, pad)
    with torch.no_grad():
        got = decode(kv, x, follow_at=cut, src=src)
    x_new = torch.cat([x[src, :cut], x[:, cut:]], 1)
    before, _, _ = reference(sd, x[:, :cut].double(), enc, pad)
    after, wk, wv = reference(sd, x_new.double(), enc, pad)
    e0 = rowwise_err(got[:, :cut].reshape(-1, 256), before.reshape(-1, 256), "follow: outputs before the permutation")
    assert e0 <= TOL, e0
    got_new = torch.cat([got[src, :cut], got[:, cut:]], 1)
    check("follow", got_new, kv, after, wk, wv)
    e1 = rowwise_err(got[:, cut:].reshape(-1, 256), after[:, cut:].reshape(-1, 256), "follow: outputs after the permutation")
    assert e1 <= TOL, e1


def test_graph_replay_is_bit_identical():
    """The 256-position run replayed from ONE captured dec_layer_step (the position is a device scalar, incremented on the
    device between replays; the input row buffer has a fixed address) against the eager run: the same bits in every output
    row and in the caches."""
    from singa_amd import ops
    S = 65
    layer, _ = make_layer(11)
    x, enc, pad = inputs(S, 111)
    kv = make_kv(layer, enc, pad)
    with torch.no_grad():
        eager = decode(kv, x)
        k_eager, v_eager = kv.k.clone(), kv.v.clone()
        kv.k.zero_(), kv.v.zero_(), kv.reset()
        x_in = x[:, 0].to(DEV).contiguous()

        def step():
            return ops.dec_layer_step(x_in, kv.w[0], kv.k[0], kv.v[0], kv.pos, kv.cross_k[0], kv.cross_v[0], kv.pad_u8, BEAMS)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()                                     # warm-up at position 0: writes slot 0, which the replay rewrites
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            out = step()
        outs = []
        x_dev = x.to(DEV)
        for pos in range(P):
            x_in.copy_(x_dev[:, pos])
            graph.replay()
            outs.append(out.clone())
            kv.pos += 1
        torch.cuda.synchronize()
    assert int(kv.pos) == 256
    assert torch.equal(torch.stack(outs, 1).cpu(), eager)
    assert torch.equal(kv.k, k_eager) and torch.equal(kv.v, v_eager)
