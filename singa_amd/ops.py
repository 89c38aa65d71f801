"""torch.autograd.Function wrappers around the C ABI of libsinga_hip.so.

Every op takes CUDA (ROCm) fp32 tensors, hands raw device pointers plus the current HIP stream to the library and
returns tensors allocated by PyTorch.  There is NO CPU path: CPU tensors raise.  Rotations are non-differentiable
inputs exactly as in the reference (`.detach()` at EF:490-491, 2351); backward kernels recompute instead of saving
rotated intermediates.
"""
import ctypes
import math
import warnings

import torch

warnings.filterwarnings("ignore", message=".*preferred_blas_library is an experimental feature.*")

from . import _capi, _lib, so3


# Optional exact timing of the scatter-TP forward dispatches (bench.py): while PROFILE_ON, the library attaches a
# start and a stop event to each such dispatch on the stream it is launched on (singa_prof_enable / _collect).
PROFILE_ON = False


def profile_start(in_graph=False):
    """in_graph: a device-timestamp kernel in front of and behind every tagged dispatch instead of events attached to it -
    plain kernel nodes that are captured with the step and re-run by every replay (read with profile_read after a replay)."""
    global PROFILE_ON, _STAMPS
    PROFILE_ON = True
    if in_graph:
        _STAMPS = torch.zeros(2 * 8192 + 2, dtype=torch.int64, device="cuda")
        _chk(_lib.lib().singa_prof_stamps(_p(_STAMPS), _STAMPS.numel()), "singa_prof_stamps")
    else:
        _chk(_lib.lib().singa_prof_enable(1), "singa_prof_enable")


_STAMPS = None


def profile_pause():
    """Stop tagging new dispatches but keep the records and the stamp buffer (graph mode: after the capture, before the
    replays)."""
    global PROFILE_ON
    PROFILE_ON = False
    _chk(_lib.lib().singa_prof_stamps(None, 0), "singa_prof_stamps")
    _chk(_lib.lib().singa_prof_enable(0), "singa_prof_enable")


def profile_read():
    """Graph mode, after a replay + synchronize: [(tag, ms, n_edges, n_nodes)] of the captured dispatches (kept)."""
    cap = 8192
    host = _STAMPS.cpu().numpy()
    ms, tg, ne, nn = (ctypes.c_float * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    n = _lib.lib().singa_prof_read_stamps(host.ctypes.data_as(ctypes.c_void_p), ms, tg, ne, nn, cap)
    return [(PROF_TAGS.get(tg[i], str(tg[i])), ms[i], ne[i], nn[i]) for i in range(n)]


def profile_end():
    """Graph mode: forget the records and release the stamp buffer (the capture that writes into it must be gone)."""
    global _STAMPS
    _chk(_lib.lib().singa_prof_stamps(None, 0), "singa_prof_stamps")
    _chk(_lib.lib().singa_prof_reset(), "singa_prof_reset")
    _STAMPS = None


PROF_TAGS = {1: "k10_fwd", 2: "k10_bwd", 3: "k4_fwd", 4: "k4_bwd_rad", 5: "k4_bwd_dst", 6: "k4_bwd_src",           # include/singa_hip.h
             7: "gemm_nt", 8: "gemm_nn", 9: "gemm_tn", 10: "s2_edge_fwd", 11: "s2_edge_bwd", 12: "s2_node_fwd", 13: "s2_node_bwd",
             14: "cgemm_nt", 15: "cgemm_nn", 16: "cgemm_tn"}


def profile_collect():
    """Call after torch.cuda.synchronize().  Returns [(kernel tag name, ms, n_edges, n_nodes)] for every profiled
    dispatch (tags: SINGA_PROF_* of include/singa_hip.h)."""
    global PROFILE_ON
    PROFILE_ON = False
    lib = _lib.lib()
    _chk(lib.singa_prof_enable(0), "singa_prof_enable")
    cap = 8192
    ms, tg, ne, nn = (ctypes.c_float * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)(), (ctypes.c_int * cap)()
    n = lib.singa_prof_collect_tagged(ms, tg, ne, nn, cap)
    return [(PROF_TAGS.get(tg[i], str(tg[i])), ms[i], ne[i], nn[i]) for i in range(n)]


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_branch_streams = {}


def branch_stream(device=None):
    """THE second stream of the model's forward / backward passes on `device` (one per device, created on first use): the
    ligand encoder beside the protein encoder (CProMG.Transformer), the ligand -> protein pass's live layer beside the protein
    -> ligand pass (EquivariantEmbedding).  One shared stream on purpose: a captured step then never has more than two
    concurrent branches - with a stream per module the embedding's backward branch could run beside the ligand encoder's
    (three branches), and an instrumented capture of such a step crashed inside hipGraphLaunch on this ROCm build."""
    dev = torch.cuda.current_device() if device is None else torch.device(device).index
    dev = torch.cuda.current_device() if dev is None else dev
    cur = torch.cuda.current_stream(dev)
    # torch hands its streams out of a pool of 32 per device, round robin: a stream made later - a graph capture's, a warm-up's -
    # can BE the one kept here, and a pass that forks onto its own stream runs on one stream and captures one branch (seen in a
    # whole-suite process: the capture stream equalled this one).  The stream in use as the current one is replaced.
    while _branch_streams.get(dev) is None or _branch_streams[dev] == cur:
        _branch_streams[dev] = torch.cuda.Stream(device=dev)
    return _branch_streams[dev]


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _chk(code, what):
    _capi.check(_lib.lib(), code, what)


def _dev(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("singa_amd ops run on the GPU only (no CPU fallback); got a CPU tensor")
        if t.dtype not in (torch.float32, torch.int32):
            raise RuntimeError(f"singa_amd ops take float32 / int32 tensors, got {t.dtype}")
    _lib.ensure_init(ts[0].device.index if ts[0].device.index is not None else torch.cuda.current_device())


class EdgeSet:
    """Edges of one edge type sorted by destination (CSR) plus the source-sorted permutation used by backward.

    order: the permutation that was applied to the caller's edge list (edge i here = original edge order[i])."""

    def __init__(self, edge_index, n_src, n_dst):
        ei = edge_index.to(torch.int64)
        dev = ei.device
        self.n_src, self.n_dst, self.E = int(n_src), int(n_dst), int(ei.shape[1])
        order = torch.argsort(ei[1], stable=True)
        self.order = order
        self.src64, self.dst64 = ei[0][order].contiguous(), ei[1][order].contiguous()
        self.src, self.dst = self.src64.to(torch.int32), self.dst64.to(torch.int32)
        # CSR / CSC pointers by binary search in the sorted index lists (no atomics)
        self.row_ptr = torch.searchsorted(self.dst64, torch.arange(self.n_dst + 1, device=dev)).to(torch.int32)
        eperm = torch.argsort(self.src64, stable=True)
        self.eperm = eperm.to(torch.int32)
        self.col_ptr = torch.searchsorted(self.src64[eperm], torch.arange(self.n_src + 1, device=dev)).to(torch.int32)

    def tensors(self):
        return [self.order, self.src64, self.dst64, self.src, self.dst, self.row_ptr, self.eperm, self.col_ptr]


def edge_frames(vec, rand, stats):
    """k1: edge vectors [E,3] + the uniform draws [E,3] of the reference's torch.rand_like (Q6) -> edge frames [E,3,3]
    (no gradient, EF:2286-2351, `.detach()` at EF:2351).  stats: float32 [2] on the same device, updated in place to
    (min(stats[0], shortest edge), max(stats[1], largest |cos(edge, helper)|)) - the reference's two guards."""
    vec, rand = vec.detach().contiguous().float(), rand.detach().contiguous().float()
    _dev(vec, rand, stats)
    E = vec.shape[0]
    assert vec.shape == (E, 3) and rand.shape == (E, 3) and stats.shape == (2,) and stats.is_contiguous()
    rot = torch.empty(E, 3, 3, device=vec.device, dtype=torch.float32)
    _chk(_lib.lib().singa_edge_frames(_p(vec), _p(rand), _p(rot), _p(stats), E, _stream()), "singa_edge_frames")
    return rot


def lap_pe(src, dst, eptr, num, start, n_total, mx, k=8):
    """n2: Laplacian positional encoding of every graph of a batch (reference model/CProMG.py:562-571; no gradient).
    src / dst: int32 LOCAL atom indices of the edges, grouped by graph; eptr [B + 1] the graphs' edge ranges; num [B]
    atoms per graph; start [B] first row of each graph in the result (the graphs tile the n_total rows: a row that belongs to no
    graph is not written); mx >= max(num).  -> fp32 [n_total, k]."""
    for t in (src, dst, eptr):
        if not t.is_cuda or t.dtype != torch.int32:
            raise RuntimeError("lap_pe: CUDA int32 edge arrays (no CPU path)")
    B = num.numel()
    dev = src.device
    _lib.ensure_init(dev.index if dev.index is not None else torch.cuda.current_device())
    lib = _lib.lib()
    src, dst, eptr = src.contiguous(), dst.contiguous(), eptr.contiguous()
    nn, st = num.to(torch.int32).contiguous(), start.to(torch.int32).contiguous()
    scratch = torch.empty(B * mx * mx, device=dev, dtype=torch.float64)           # only the components' diagonal blocks are touched
    work = torch.empty(max(lib.singa_lap_pe_work(B, mx), 1), device=dev, dtype=torch.float64)
    out = torch.empty(n_total, k, device=dev, dtype=torch.float32)   # the kernel writes all k columns of every graph's rows (zeros past n - 1)
    _chk(lib.singa_lap_pe(_p(scratch), _p(src), _p(dst), _p(eptr), _p(nn), _p(st), _p(work), _p(out), B, mx, k, _stream()),
         "singa_lap_pe")
    return out


def wigner_rows(rot, L, M=2):
    """k2: rot [E,3,3] -> reduced Wigner rows [E, WSZ] (no gradient, EF:485-528)."""
    rot = rot.detach().contiguous().float()
    _dev(rot)
    lay = so3.layout(L, M)
    E = rot.shape[0]
    wr = torch.empty(E, lay.WSZ, device=rot.device, dtype=torch.float32)     # WSZ is padded to 16-byte records; the kernel writes the pad floats (0)
    _chk(_lib.lib().singa_wigner_rows(_p(rot), _p(wr), E, L, M, _stream()), "singa_wigner_rows")
    return wr


class _GatherRotate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_src, x_dst, rad, wr, es, L, M):
        x_src, x_dst, rad = x_src.contiguous(), x_dst.contiguous(), rad.contiguous()
        _dev(x_src, x_dst, rad, wr)
        lay = so3.layout(L, M)
        C = x_src.shape[2]
        assert x_src.shape[1] == lay.K and x_dst.shape[1] == lay.K and wr.shape == (es.E, lay.WSZ)
        assert x_src.shape[0] == es.n_src and x_dst.shape[0] == es.n_dst and rad.shape == (es.E, lay.rad_rows * 2 * C)
        out = torch.empty(es.E, lay.KR * 2 * C, device=x_src.device, dtype=torch.float32)
        _chk(_lib.lib().singa_gather_rotate_fwd(_p(x_src), _p(x_dst), _p(es.src), _p(es.dst), _p(wr), _p(rad), _p(out),
                                                es.E, C, L, M, _stream()), "singa_gather_rotate_fwd")
        ctx.save_for_backward(x_src, x_dst, rad, wr)
        ctx.es, ctx.L, ctx.M = es, L, M
        return out

    @staticmethod
    def backward(ctx, g):
        x_src, x_dst, rad, wr = ctx.saved_tensors
        es, L, M = ctx.es, ctx.L, ctx.M
        g = g.contiguous()
        C = x_src.shape[2]
        g_rad = torch.empty_like(rad)
        gx_src, gx_dst = torch.empty_like(x_src), torch.empty_like(x_dst)
        _chk(_lib.lib().singa_gather_rotate_bwd(_p(g), _p(x_src), _p(x_dst), _p(es.src), _p(es.dst), _p(wr), _p(rad),
                                                _p(es.row_ptr), _p(es.col_ptr), _p(es.eperm), _p(g_rad), _p(gx_src),
                                                _p(gx_dst), es.E, es.n_src, es.n_dst, C, L, M, _stream()),
             "singa_gather_rotate_bwd")
        return gx_src, gx_dst, g_rad, None, None, None, None


def gather_rotate(x_src, x_dst, rad, wr, es, L, M=2):
    """k3-k6: [N,K,C] node tensors -> m-primary edge tensor [E, KR*2C], multiplied by rad [E, RAD_ROWS*2C]."""
    return _GatherRotate.apply(x_src, x_dst, rad, wr, es, L, M)


def _segs3(ts, rows, CH):
    return _capi.segs([(t.data_ptr(), t.stride(0), r) for t, r in zip(ts, rows)])


class _RotateBackScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y0, y1, y2, alpha, wr, es, heads, L, M):
        y0, y1, y2, alpha = _rows(y0), _rows(y1), _rows(y2), alpha.contiguous()      # column-block views are taken as they are
        _dev(y0, y1, y2, alpha, wr)
        lay = so3.layout(L, M)
        CH = y0.shape[1] // lay.seg_rows[0]
        assert y1.shape[1] == lay.seg_rows[1] * CH and y2.shape[1] == lay.seg_rows[2] * CH
        assert alpha.shape == (es.E, heads) and wr.shape == (es.E, lay.WSZ)
        ctx.save_for_backward(y0, y1, y2, alpha, wr)
        ctx.es, ctx.heads, ctx.L, ctx.M, ctx.CH = es, heads, L, M, CH
        if es.E == 0:                             # an edge type without edges: empty tensors have no address to hand over
            return torch.zeros(es.n_dst, lay.K, CH, device=y0.device, dtype=torch.float32)
        out = torch.empty(es.n_dst, lay.K, CH, device=y0.device, dtype=torch.float32)
        seg, n = _segs3((y0, y1, y2), lay.seg_rows, CH)
        if PROFILE_ON:
            _lib.lib().singa_prof_hint_edges(es.E)
        _chk(_lib.lib().singa_rotate_back_scatter_fwd(seg, n, _p(alpha), _p(wr), _p(es.row_ptr), _p(out), es.n_dst, CH,
                                                      heads, L, M, 0, 1.0, _stream()), "singa_rotate_back_scatter_fwd")
        return out

    @staticmethod
    def backward(ctx, g):
        y0, y1, y2, alpha, wr = ctx.saved_tensors
        es, heads, L, M, CH = ctx.es, ctx.heads, ctx.L, ctx.M, ctx.CH
        lay = so3.layout(L, M)
        if es.E == 0:
            return torch.zeros_like(y0), torch.zeros_like(y1), torch.zeros_like(y2), torch.zeros_like(alpha), None, None, None, None, None
        g = g.contiguous()
        widths = [y0.shape[1], y1.shape[1], y2.shape[1]]
        gY = torch.empty(es.E, sum(widths), device=g.device, dtype=torch.float32)   # the three gradients as column blocks
        gy = list(gY.split(widths, dim=1))
        gap = torch.empty(es.E, CH, device=g.device, dtype=torch.float32)
        seg, n = _segs3((y0, y1, y2), lay.seg_rows, CH)
        gseg, _ = _segs3(gy, lay.seg_rows, CH)
        if PROFILE_ON:
            _lib.lib().singa_prof_hint_edges(es.E)
        _chk(_lib.lib().singa_rotate_back_scatter_bwd(_p(g), seg, gseg, n, _p(alpha), _p(wr), _p(es.row_ptr), _p(gap),
                                                      es.n_dst, CH, heads, L, M, 0, 1.0, _stream()),
             "singa_rotate_back_scatter_bwd")
        g_alpha = gap.view(es.E, heads, CH // heads).sum(-1)
        return gy[0], gy[1], gy[2], g_alpha, None, None, None, None, None


def rotate_back_scatter(y0, y1, y2, alpha, wr, es, heads, L, M=2):
    """k10: per-m SO(2)-conv outputs (m-primary) * alpha -> rotate back -> sum into destination nodes [Nd,K,CH]."""
    return _RotateBackScatter.apply(y0, y1, y2, alpha, wr, es, heads, L, M)


class _EdgeDegreeScatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r, wr, es, L, M, scale):
        r = r.contiguous()
        _dev(r, wr)
        lay = so3.layout(L, M)
        C = r.shape[1] // lay.m_size[0]
        out = torch.empty(es.n_dst, lay.K, C, device=r.device, dtype=torch.float32)
        seg, n = _capi.segs([(r.data_ptr(), r.stride(0), lay.m_size[0])])
        _chk(_lib.lib().singa_rotate_back_scatter_fwd(seg, n, None, _p(wr), _p(es.row_ptr), _p(out), es.n_dst, C, 1, L, M,
                                                      1, scale, _stream()), "singa_rotate_back_scatter_fwd(m0)")
        ctx.save_for_backward(wr)
        ctx.es, ctx.L, ctx.M, ctx.scale, ctx.shape, ctx.C = es, L, M, scale, r.shape, C
        return out

    @staticmethod
    def backward(ctx, g):
        (wr,) = ctx.saved_tensors
        es, L, M = ctx.es, ctx.L, ctx.M
        lay = so3.layout(L, M)
        g = g.contiguous()
        gr = torch.empty(ctx.shape, device=g.device, dtype=torch.float32)
        gseg, n = _capi.segs([(gr.data_ptr(), gr.stride(0), lay.m_size[0])])
        _chk(_lib.lib().singa_rotate_back_scatter_bwd(_p(g), None, gseg, n, None, _p(wr), _p(es.row_ptr), None, es.n_dst,
                                                      ctx.C, 1, L, M, 1, ctx.scale, _stream()),
             "singa_rotate_back_scatter_bwd(m0)")
        return gr, None, None, None, None, None


def edge_degree_scatter(r, wr, es, L, M=2, scale=1.0):
    """k13: m=0 radial output [E,(L+1)*C] -> rotate back (m=0 Wigner columns only) -> node sum * scale."""
    return _EdgeDegreeScatter.apply(r, wr, es, L, M, scale)


class _SegmentSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, row_ptr, eps):
        x = x.contiguous()
        _dev(x, row_ptr)
        y = torch.empty_like(x)
        N = row_ptr.numel() - 1
        ctx.dense = int(x.shape[1] == 4 and x.shape[0] >= 16 * N)      # >= 16 edges per segment on average: wave per segment
        if x.shape[0] == 0:                       # no edges: nothing to normalise (and an empty tensor has no address)
            ctx.save_for_backward(y, row_ptr)
            return y
        _chk(_lib.lib().singa_segment_softmax_fwd(_p(x), _p(row_ptr), _p(y), N, x.shape[1], eps, ctx.dense, _stream()),
             "singa_segment_softmax_fwd")
        ctx.save_for_backward(y, row_ptr)
        return y

    @staticmethod
    def backward(ctx, gy):
        y, row_ptr = ctx.saved_tensors
        gy = gy.contiguous()
        gx = torch.empty_like(y)
        N = row_ptr.numel() - 1
        if y.shape[0] == 0:
            return gx, None, None
        _chk(_lib.lib().singa_segment_softmax_bwd(_p(y), _p(gy), _p(row_ptr), _p(gx), N, y.shape[1], ctx.dense, _stream()),
             "singa_segment_softmax_bwd")
        return gx, None, None


def segment_softmax(x, row_ptr, eps):
    """k9: softmax of x[E,H] over the edge segments of row_ptr (edges sorted by segment)."""
    return _SegmentSoftmax.apply(x, row_ptr, eps)


class _SegmentWSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, w, v, row_ptr):
        w, v = w.contiguous(), v.contiguous()
        _dev(w, v, row_ptr)
        E, H, F = v.shape
        N = row_ptr.numel() - 1
        ctx.save_for_backward(w, v, row_ptr)
        if E == 0:                                # no edges: every segment sums to zero (and empty tensors have no address)
            return torch.zeros(N, H, F, device=v.device, dtype=torch.float32)
        out = torch.empty(N, H, F, device=v.device, dtype=torch.float32)
        _chk(_lib.lib().singa_segment_wsum_fwd(_p(w), _p(v), _p(row_ptr), _p(out), N, H, F, _stream()),
             "singa_segment_wsum_fwd")
        return out

    @staticmethod
    def backward(ctx, g):
        w, v, row_ptr = ctx.saved_tensors
        g = g.contiguous()
        E, H, F = v.shape
        N = row_ptr.numel() - 1
        gw, gv = torch.empty_like(w), torch.empty_like(v)
        if E == 0:
            return gw, gv, None
        _chk(_lib.lib().singa_segment_wsum_bwd(_p(g), _p(w), _p(v), _p(row_ptr), _p(gw), _p(gv), N, H, F, _stream()),
             "singa_segment_wsum_bwd")
        return gw, gv, None


def segment_sum_rows(v, row_ptr):
    """out[n, :] = sum of the rows v[row_ptr[n] : row_ptr[n+1], :] (no gradient; rows sorted by segment): the segmented
    sum kernel with unit weights, no atomics."""
    v = v.detach()
    _dev(v, row_ptr)
    E, F = v.shape
    N = row_ptr.numel() - 1
    out = torch.empty(N, 1, F, device=v.device, dtype=torch.float32)
    w = torch.ones(max(E, 1), 1, device=v.device, dtype=torch.float32)
    _chk(_lib.lib().singa_segment_wsum_fwd(_p(w), _p(v), _p(row_ptr), _p(out), N, 1, F, _stream()), "singa_segment_wsum_fwd")
    return out.view(N, F)


def knn_edge_attr(ln, seg_ptr, E0, n_real, offset, coeff):
    """n1: the kNN graph's edge features in their final layout (singa_knn_edge_attr): ln [n_real] lengths of the first n_real
    of the E0 row-sorted undirected edges (the rest: inert padding edges, zeros), seg_ptr [N + 1] int32 -> [E0 + N, 64]:
    -smear(len) at row e + i for edge e of node i, the row sums (the degree) at the self loops' rows."""
    ln, offset = ln.detach().contiguous(), offset.detach().contiguous()
    _dev(ln, seg_ptr, offset)
    N = seg_ptr.numel() - 1
    out = torch.empty(E0 + N, offset.numel(), device=ln.device, dtype=torch.float32)
    _chk(_lib.lib().singa_knn_edge_attr(_p(ln), _p(seg_ptr), int(n_real), _p(offset), float(coeff), _p(out), N, offset.numel(),
                                        _stream()), "singa_knn_edge_attr")
    return out


def knn_graph(pos, k, batch, ptr, max_nodes):
    """n1: torch_cluster.knn_graph(pos, k, batch, flow='target_to_source') (CP:293,330) -> [2, N * k] int64, row = centre,
    -1 where a slot does not exist (singa_knn_graph).  batch ids outside [0, len(ptr) - 1) = atoms of no molecule."""
    pos = pos.detach().to(torch.float32).contiguous()
    b32 = batch.to(torch.int32).contiguous()
    _dev(pos, b32)
    p64 = ptr.to(device=pos.device, dtype=torch.int64).contiguous()
    N = pos.shape[0]
    out = torch.empty(2, N * k, dtype=torch.int64, device=pos.device)
    _chk(_lib.lib().singa_knn_graph(_p(pos), _p(b32), _p(p64), p64.numel() - 1, N, int(k), int(max_nodes), _p(out[0]), _p(out[1]),
                                    _stream()), "singa_knn_graph")
    return out


def segment_wsum(w, v, row_ptr):
    """k15: out[n,H,F] = sum over the segment of w[e,H] * v[e,H,F]."""
    return _SegmentWSum.apply(w, v, row_ptr)


_grid_cache = {}


def _grid_factors(L, M, m_primary, device):
    """Separable S2-grid tables (P [RB,KIN], Q [RB,KIN], A [RA,2M+1]) on `device`, cached (so3.s2_grid_factors)."""
    key = (L, M, m_primary, str(device))
    if key not in _grid_cache:
        _grid_cache[key] = tuple(torch.tensor(t, dtype=torch.float32, device=device).contiguous()
                                 for t in so3.s2_grid_factors(L, M, m_primary))
    return _grid_cache[key]


# The k8 launches.  `src`: the leading arguments every one of them takes - segments, gate, tables - from _s2_edge_src (the three
# m-primary SO(2)-conv outputs; h0 = [alpha inputs | gate | m = 0 rows]) or _s2_node_src (one l-primary [N, K, C] record).  No rows,
# no launch: an empty tensor has no address to hand over.
def _s2_edge_src(h0, h1, h2, gate_off, x_off, C, L, M):
    seg, n = _segs3((h0[:, x_off:], h1, h2), so3.layout(L, M).seg_rows, C)
    return (seg, n, _p(h0[:, gate_off:]), h0.stride(0)) + tuple(_p(t) for t in _grid_factors(L, M, True, h0.device))


def _s2_node_src(x, gate, L):
    seg, n = _capi.segs([(x.data_ptr(), x.shape[1] * x.shape[2], x.shape[1])])
    return (seg, n, _p(gate), gate.stride(0)) + tuple(_p(t) for t in _grid_factors(L, L, False, x.device))


def _s2_fwd_edge(h0, h1, h2, gate_off, x_off, C, L, M):
    """-> the activated m-primary tensor [E, KR*C]"""
    E = h0.shape[0]
    out = torch.empty(E, so3.layout(L, M).KR * C, device=h0.device, dtype=torch.float32)
    if E > 0:
        _chk(_lib.lib().singa_s2act_sep_fwd(*_s2_edge_src(h0, h1, h2, gate_off, x_off, C, L, M), _p(out), E, C, L, _stream()),
             "singa_s2act_sep_fwd")
    return out


def _s2_fwd_node(x, gate, L):
    """-> the activated [N, K, C] tensor"""
    out = torch.empty_like(x)
    if x.shape[0] > 0:
        _chk(_lib.lib().singa_s2act_sep_fwd(*_s2_node_src(x, gate, L), _p(out), x.shape[0], x.shape[2], L, _stream()),
             "singa_s2act_sep_fwd(node)")
    return out


def _s2_bwd(src, g, E, KC, C, L, what):
    """-> (the input gradient as one contiguous [E, KC] tensor, the gate's gradient [E, C])"""
    gx = torch.empty(E, KC, device=g.device, dtype=torch.float32)
    gg = torch.empty(E, C, device=g.device, dtype=torch.float32)
    if E > 0:
        _chk(_lib.lib().singa_s2act_sep_bwd(*src, _p(g), _p(gx), _p(gg), E, C, L, _stream()), what)
    return gx, gg


def _s2_bwd_seg(src, g, gseg, g_gate, E, C, L):
    """The input gradient into the segments `gseg`, the gate's gradient into the column block `g_gate` of a wider tensor."""
    if E > 0:
        _chk(_lib.lib().singa_s2act_sep_bwd_seg(*src, _p(g), gseg, _p(g_gate), g_gate.stride(0), E, C, L, _stream()),
             "singa_s2act_sep_bwd_seg")


class _S2ActEdge(torch.autograd.Function):
    """SeparableS2Activation on the attention grid [L][M] applied directly to the three SO(2)-conv GEMM outputs
    (m-primary).  h0 = [alpha inputs | gate | m=0 rows]; returns the activated m-primary tensor [E, KR*C]."""

    @staticmethod
    def forward(ctx, h0, h1, h2, gate_off, x_off, C, L, M):
        h0, h1, h2 = _rows(h0), _rows(h1), _rows(h2)
        _dev(h0, h1, h2)
        ctx.save_for_backward(h0, h1, h2)
        ctx.cfg = (gate_off, x_off, C, L, M)
        return _s2_fwd_edge(h0, h1, h2, gate_off, x_off, C, L, M)

    @staticmethod
    def backward(ctx, g):
        h0, h1, h2 = ctx.saved_tensors
        gate_off, x_off, C, L, M = ctx.cfg
        lay = so3.layout(L, M)
        gx, gg = _s2_bwd(_s2_edge_src(h0, h1, h2, *ctx.cfg), g.contiguous(), h0.shape[0], lay.KR * C, C, L,
                         "singa_s2act_sep_bwd")
        n0, n1 = lay.seg_rows[0] * C, lay.seg_rows[1] * C
        g0 = torch.zeros_like(h0)
        g0[:, gate_off:gate_off + C] = gg
        g0[:, x_off:] = gx[:, :n0]
        return g0, gx[:, n0:n0 + n1], gx[:, n0 + n1:], None, None, None, None, None


def s2act_edge(h0, h1, h2, gate_off, x_off, C, L, M=2):
    return _S2ActEdge.apply(h0, h1, h2, gate_off, x_off, C, L, M)


class _EdgeHead(torch.autograd.Function):
    """Everything that consumes the first SO(2) convolution (EF:1148-1178): attention logits (LayerNorm(A) ->
    SmoothLeakyReLU -> dot with alpha_dot, k9a) from the first heads*A columns of h0, and the separable S2 activation
    (k8) of [gate | m=0 rows] + h1 + h2.  One autograd node, so the gradient of h0 is assembled once (no zero-filled
    full-width buffers, no add of two partial gradients)."""

    @staticmethod
    def forward(ctx, h0, h1, h2, ln_w, ln_b, dot, heads, A, C, L, M, eps):
        ctx.params = (ln_w, ln_b, dot)
        ctx.cfg = (heads, A, C, L, M, eps)
        saved, logits, act = _edge_head_fwd(h0, h1, h2, ln_w, ln_b, dot, ctx.cfg)
        ctx.save_for_backward(*saved)
        return logits, act

    @staticmethod
    def backward(ctx, g_logits, g_act):
        return _edge_head_bwd(ctx.saved_tensors, ctx.cfg, ctx.params, g_logits, g_act) + (None,) * 6


def _edge_act(h0, h1, h2, cfg):
    """The activation launch of the edge head: the separable S2 activation of [gate | m = 0 rows] of h0, h1, h2 -> [E, KR*C]."""
    heads, A, C, L, M, _ = cfg
    return _s2_fwd_edge(h0, h1, h2, heads * A, heads * A + C, C, L, M)


def _edge_head_fwd(h0, h1, h2, ln_w, ln_b, dot, cfg):
    """The forward launches of _EdgeHead -> (the six tensors its backward needs, logits, act)."""
    heads, A, C, L, M, eps = cfg
    h0, h1, h2 = _rows(h0), _rows(h1), _rows(h2)
    ln_w, ln_b, dot = ln_w.contiguous(), ln_b.contiguous(), dot.contiguous()
    _dev(h0, h1, h2, ln_w, ln_b, dot)
    E = h0.shape[0]
    logits = torch.empty(E, heads, device=h0.device, dtype=torch.float32)
    if E > 0:
        _chk(_lib.lib().singa_alpha_logits_fwd(_p(h0), h0.stride(0), _p(ln_w), _p(ln_b), _p(dot), _p(logits), E, heads, A, eps,
                                               _stream()), "singa_alpha_logits_fwd")
    return (h0, h1, h2, ln_w, ln_b, dot), logits, _edge_act(h0, h1, h2, cfg)


def _edge_head_bwd(saved, cfg, params, g_logits, g_act):
    """The backward launches of _EdgeHead -> the gradients of (h0, h1, h2, ln_w, ln_b, dot); params: the three parameters as
    the caller was given them (the targets of direct accumulation, _GradSink)."""
    h0, h1, h2, ln_w, ln_b, dot = saved
    heads, A, C, L, M, eps = cfg
    lay = so3.layout(L, M)
    lib = _lib.lib()
    E = h0.shape[0]
    gate_off, x_off = heads * A, heads * A + C
    g_logits, g_act = g_logits.contiguous(), g_act.contiguous()
    # the gradients of the convolution's three outputs are assembled in place: h0's is [alpha inputs | gate | m = 0 rows],
    # written by two kernels into column blocks of one buffer (the concatenation they replaced cost 0.6 ms per step)
    n0, n1, n2 = (r * C for r in lay.seg_rows)
    g_h0 = torch.empty(E, x_off + n0, device=h0.device, dtype=torch.float32)
    g_h1 = torch.empty(E, n1, device=h0.device, dtype=torch.float32)
    g_h2 = torch.empty(E, n2, device=h0.device, dtype=torch.float32)
    nslots = lib.singa_alpha_logits_nslots(E)
    part = (torch.empty if E > 0 else torch.zeros)(nslots, (2 + heads) * A, device=h0.device, dtype=torch.float32)
    if E > 0:
        _chk(lib.singa_alpha_logits_bwd_ld(_p(h0), h0.stride(0), _p(ln_w), _p(ln_b), _p(dot), _p(g_logits), _p(g_h0),
                                           g_h0.stride(0), _p(part), E, heads, A, eps, _stream()), "singa_alpha_logits_bwd_ld")
    pw, pb, pd = params
    g_lnw, g_lnb, g_dot = param_colsum(part, [(0, A, pw), (A, A, pb), (2 * A, heads * A, pd)])
    if g_dot is not None:
        g_dot = g_dot.view(heads, A)
    gseg, _ = _segs3((g_h0[:, x_off:], g_h1, g_h2), lay.seg_rows, C)
    _s2_bwd_seg(_s2_edge_src(h0, h1, h2, gate_off, x_off, C, L, M), g_act, gseg, g_h0[:, gate_off:], E, C, L)
    return (g_h0, g_h1, g_h2, g_lnw, g_lnb, g_dot)


def edge_head(h0, h1, h2, ln_w, ln_b, alpha_dot, heads, A, C, L, M=2, eps=1e-5):
    """-> (attention logits [E, heads], activated m-primary tensor [E, KR*C])"""
    return _EdgeHead.apply(h0, h1, h2, ln_w, ln_b, alpha_dot, heads, A, C, L, M, eps)


class _S2ActNode(torch.autograd.Function):
    """SeparableS2Activation on the FFN grid [L][L] for an l-primary node tensor [N,K,C] and gate [N,C]."""

    @staticmethod
    def forward(ctx, x, gate, L):
        x, gate = x.contiguous(), gate.contiguous()
        _dev(x, gate)
        ctx.save_for_backward(x, gate)
        ctx.L = L
        return _s2_fwd_node(x, gate, L)

    @staticmethod
    def backward(ctx, g):
        x, gate = ctx.saved_tensors
        N, K, C = x.shape
        gx, gg = _s2_bwd(_s2_node_src(x, gate, ctx.L), g.contiguous(), N, K * C, C, ctx.L, "singa_s2act_sep_bwd(node)")
        return gx.view(N, K, C), gg, None


def s2act_node(x, gate, L):
    return _S2ActNode.apply(x, gate, L)


_deg_cache = {}


def _degree_onehot(L, device):
    """[L+1, K] 0/1 matrix that sums coefficient rows by degree: a small GEMM instead of index_add_ (atomics, ~20 us for
    nine indices)."""
    key = ("onehot", L, str(device))
    if key not in _deg_cache:
        deg = torch.as_tensor(so3.layout(L, L).degree, dtype=torch.int64)
        _deg_cache[key] = torch.nn.functional.one_hot(deg, L + 1).t().to(torch.float32).contiguous().to(device)
    return _deg_cache[key]


def _degree_index(L, device):
    """degree l of every coefficient row, as a device tensor (cached: no host->device copy inside a graph capture)."""
    key = (L, str(device))
    if key not in _deg_cache:
        _deg_cache[key] = torch.as_tensor(so3.layout(L, L).degree, device=device, dtype=torch.int64)
    return _deg_cache[key]


class _SO3RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, L, eps):
        ctx.params = (weight, bias)
        x, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
        _dev(x, weight, bias)
        N, K, C = x.shape
        y = torch.empty_like(x)
        _chk(_lib.lib().singa_so3_rmsnorm_fwd(_p(x), _p(weight), _p(bias), _p(y), N, C, L, eps, _stream()),
             "singa_so3_rmsnorm_fwd")
        ctx.save_for_backward(x, weight)
        ctx.L, ctx.eps = L, eps
        return y

    @staticmethod
    def backward(ctx, gy):
        x, weight = ctx.saved_tensors
        L, eps = ctx.L, ctx.eps
        gy = gy.contiguous()
        N, K, C = x.shape
        nparts = _lib.lib().singa_so3_rmsnorm_nparts(N)
        gx = torch.empty_like(x)
        gwp = torch.empty(nparts, (L + 1) * C, device=x.device, dtype=torch.float32)       # already summed over each degree's rows
        gbp = torch.empty(nparts, C, device=x.device, dtype=torch.float32)
        _chk(_lib.lib().singa_so3_rmsnorm_bwd(_p(x), _p(weight), _p(gy), _p(gx), _p(gwp), _p(gbp), N, C, L, eps,
                                              _stream()), "singa_so3_rmsnorm_bwd")
        gw = param_colsum(gwp, [(0, (L + 1) * C, ctx.params[0])])[0]
        if gw is not None:
            gw = gw.view(L + 1, C)
        return gx, gw, param_colsum(gbp, [(0, C, ctx.params[1])])[0], None, None


def so3_rmsnorm(x, weight, bias, L, eps=1e-5):
    """k12: centred, degree-balanced RMS norm with per-degree affine weight and l=0 bias (EF:2155-2192, Q3)."""
    return _SO3RMSNorm.apply(x, weight, bias, L, eps)


class _SO3RMSNormSkip(torch.autograd.Function):
    """(norm(x), x): the norm together with the residual branch that leaves its input (x + f(norm(x)) of a TransBlockV2,
    EF:1383-1384, 1405-1406).  One autograd node for both uses of x, so that the backward kernel adds the residual's gradient
    to the norm's input gradient itself (singa_so3_rmsnorm_bwd_add) instead of autograd adding two [N, K, C] tensors afterwards."""

    @staticmethod
    def forward(ctx, x, weight, bias, L, eps):
        ctx.params = (weight, bias)
        xc, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
        _dev(xc, weight, bias)
        N, K, C = xc.shape
        y = torch.empty_like(xc)
        _chk(_lib.lib().singa_so3_rmsnorm_fwd(_p(xc), _p(weight), _p(bias), _p(y), N, C, L, eps, _stream()),
             "singa_so3_rmsnorm_fwd")
        ctx.save_for_backward(xc, weight)
        ctx.L, ctx.eps = L, eps
        return y, x.view_as(x)

    @staticmethod
    def backward(ctx, gy, gskip):
        x, weight = ctx.saved_tensors
        L, eps = ctx.L, ctx.eps
        N, K, C = x.shape
        lib = _lib.lib()
        if gy is None:                                  # (the norm's output unused: only the skip carries a gradient)
            return gskip, None, None, None, None
        gy = gy.contiguous()
        nparts = lib.singa_so3_rmsnorm_nparts(N)
        gx = torch.empty_like(x)
        gwp = torch.empty(nparts, (L + 1) * C, device=x.device, dtype=torch.float32)
        gbp = torch.empty(nparts, C, device=x.device, dtype=torch.float32)
        if gskip is not None:
            gskip = gskip.contiguous()
            _chk(lib.singa_so3_rmsnorm_bwd_add(_p(x), _p(weight), _p(gy), _p(gskip), _p(gx), _p(gwp), _p(gbp), N, C, L, eps,
                                               _stream()), "singa_so3_rmsnorm_bwd_add")
        else:
            _chk(lib.singa_so3_rmsnorm_bwd(_p(x), _p(weight), _p(gy), _p(gx), _p(gwp), _p(gbp), N, C, L, eps, _stream()),
                 "singa_so3_rmsnorm_bwd")
        gw = param_colsum(gwp, [(0, (L + 1) * C, ctx.params[0])])[0]
        if gw is not None:
            gw = gw.view(L + 1, C)
        return gx, gw, param_colsum(gbp, [(0, C, ctx.params[1])])[0], None, None


def so3_rmsnorm_skip(x, weight, bias, L, eps=1e-5):
    """-> (norm(x), x) as ONE autograd node: see _SO3RMSNormSkip."""
    return _SO3RMSNormSkip.apply(x, weight, bias, L, eps)


# ----------------------------------------------------------------------------------------------- fused graph attention
class _EdgeLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qp, wk, hk, cterm, edges, scale):
        qp, wk, hk, cterm = qp.contiguous(), wk.contiguous(), hk.contiguous(), cterm.contiguous()
        _dev(qp, wk, hk, cterm)
        N, H, D = qp.shape
        qk = torch.empty(wk.shape[0], H, device=qp.device, dtype=torch.float32)
        ctx.edges, ctx.scale = edges, scale
        if wk.shape[0] == 0:                      # no edges: no logits (and empty tensors have no address to hand over)
            ctx.save_for_backward(qp, wk, hk)
            return qk
        _chk(_lib.lib().singa_edge_logits_fwd(_p(qp), _p(wk), _p(hk), _p(cterm), _p(edges.row_ptr), _p(edges.col32),
                                              _p(qk), N, H, D, scale, _stream()), "singa_edge_logits_fwd")
        ctx.save_for_backward(qp, wk, hk)
        ctx.edges, ctx.scale = edges, scale
        return qk

    @staticmethod
    def backward(ctx, g):
        qp, wk, hk = ctx.saved_tensors
        e, N, H, D = ctx.edges, qp.shape[0], qp.shape[1], qp.shape[2]
        g = g.contiguous()
        g_qp, g_wk, g_hk = torch.empty_like(qp), torch.empty_like(wk), torch.empty_like(hk)
        g_c = torch.empty(N, H, device=g.device, dtype=torch.float32)
        if wk.shape[0] == 0:
            return g_qp.zero_(), g_wk, g_hk.zero_(), g_c.zero_(), None, None
        _chk(_lib.lib().singa_edge_logits_bwd(_p(g), _p(qp), _p(wk), _p(hk), _p(e.row_ptr), _p(e.col32), _p(e.col_ptr),
                                              _p(e.eperm), _p(e.row32), _p(g_qp), _p(g_wk), _p(g_hk), _p(g_c), N, H, D,
                                              ctx.scale, _stream()), "singa_edge_logits_bwd")
        return g_qp, g_wk, g_hk, g_c, None, None


def edge_logits(qp, wk, hk, cterm, edges, scale):
    """qk[e,h] = scale * sum_d qp[row,h,d] wk[e,d] hk[col,h,d] + cterm[row,h]  (CP:61-65 with weight_k_lin hoisted)."""
    return _EdgeLogits.apply(qp, wk, hk, cterm, edges, scale)


class _GatherWSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, alpha, wv, hv, edges):
        alpha, wv, hv = alpha.contiguous(), wv.contiguous(), hv.contiguous()
        _dev(alpha, wv, hv)
        N, H, F = hv.shape
        out = torch.empty(N, H, F, device=hv.device, dtype=torch.float32)
        ctx.edges = edges
        if alpha.shape[0] == 0:                   # no edges: every node sums to zero (and empty tensors have no address)
            ctx.save_for_backward(alpha, wv, hv)
            return out.zero_()
        _chk(_lib.lib().singa_gather_wsum_fwd(_p(alpha), _p(wv), _p(hv), _p(edges.row_ptr), _p(edges.col32), _p(out), N,
                                              H, F, _stream()), "singa_gather_wsum_fwd")
        ctx.save_for_backward(alpha, wv, hv)
        ctx.edges = edges
        return out

    @staticmethod
    def backward(ctx, g):
        alpha, wv, hv = ctx.saved_tensors
        e = ctx.edges
        N, H, F = hv.shape
        g = g.contiguous()
        g_a, g_wv, g_hv = torch.empty_like(alpha), torch.empty_like(wv), torch.empty_like(hv)
        if alpha.shape[0] == 0:
            return g_a, g_wv, g_hv.zero_(), None
        _chk(_lib.lib().singa_gather_wsum_bwd(_p(g), _p(alpha), _p(wv), _p(hv), _p(e.row_ptr), _p(e.col32), _p(e.col_ptr),
                                              _p(e.eperm), _p(e.row32), _p(g_a), _p(g_wv), _p(g_hv), N, H, F, _stream()),
             "singa_gather_wsum_bwd")
        return g_a, g_wv, g_hv, None


def gather_wsum(alpha, wv, hv, edges):
    """out[n,h,f] = sum_e alpha[e,h] wv[e,f] hv[col_e,h,f]  (CP:70-74 with weight_v_lin hoisted)."""
    return _GatherWSum.apply(alpha, wv, hv, edges)


class _LnSilu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        ctx.params = (gamma, beta)
        x, gamma, beta = x.contiguous(), gamma.contiguous(), beta.contiguous()
        _dev(x, gamma, beta)
        C = x.shape[-1]
        M = x.numel() // C
        out = torch.empty_like(x)
        _chk(_lib.lib().singa_ln_silu_fwd(_p(x), _p(gamma), _p(beta), _p(out), M, C, eps, _stream()), "singa_ln_silu_fwd")
        ctx.save_for_backward(x, gamma, beta)
        ctx.eps = eps
        return out

    @staticmethod
    def backward(ctx, g):
        x, gamma, beta = ctx.saved_tensors
        g = g.contiguous()
        C = x.shape[-1]
        M = x.numel() // C
        lib = _lib.lib()
        gx = torch.empty_like(x)
        part = torch.empty(lib.singa_ln_silu_nparts(M), 2 * C, device=x.device, dtype=torch.float32)
        _chk(lib.singa_ln_silu_bwd(_p(x), _p(gamma), _p(beta), _p(g), _p(gx), _p(part), M, C, ctx.eps, _stream()),
             "singa_ln_silu_bwd")
        gg, gb = param_colsum(part, [(0, C, ctx.params[0]), (C, C, ctx.params[1])])
        return gx, gg, gb, None


def ln_silu(x, gamma, beta, eps=1e-5):
    """SiLU(LayerNorm(x)) over the last axis of 16 channels (k6a): one pass forward, one pass backward."""
    return _LnSilu.apply(x, gamma, beta, eps)


def dec_layer_step(x, w, k_cache, v_cache, pos, cross_k, cross_v, pad, beams, per_row=False, tiles=False):
    """One decoder layer for one new position of every beam-search row (k17; inference only, no autograd): three launches.
    `w`: dict of the layer's transposed weights as built by BeamSearch.KVDecoder; k_cache [R,4,P,32], v_cache [R,4,P,64];
    pos: int64 device scalar; cross_k [B,4,32,S], cross_v [B,4,S,64], pad [B,S] uint8.  `pos` of shape [R] (more than one
    dimension-0 entry, or `per_row=True`) is one position per row: the self-attention launch is `singa_dec_self_attn_rows` of
    include/singa_hip_stream.h, the other two launches do not depend on the position.  `tiles=True`: the three launches are the
    row-tiled ones of include/singa_hip_dec_tiles.h (one workgroup per 16 rows of a pocket, any number of encoder positions)."""
    _dev(x, k_cache, v_cache, cross_k, cross_v)
    lib, st = _lib.lib(), _stream()
    R, P, S = x.shape[0], k_cache.shape[2], cross_v.shape[2]
    y, z, out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    a, c, f = w["self"], w["cross"], w["ffn"]
    if per_row:
        _check_views("dec_layer_step", ((pos, torch.int64, (R,)),))
    if tiles:
        _chk(lib.singa_dec_tile_self_attn(_p(x), _p(a["wqkv_t"]), _p(a["bqkv"]), _p(a["wo_t"]), _p(a["bo"]), _p(a["gamma"]),
                                          _p(a["beta"]), _p(k_cache), _p(v_cache), _p(pos), 1 if per_row else 0, R, beams, P, _p(y),
                                          a["eps"], st), "singa_dec_tile_self_attn")
        _chk(lib.singa_dec_tile_cross_attn(_p(y), _p(c["wq_t"]), _p(c["bq"]), _p(cross_k), _p(cross_v), _p(pad), _p(c["wo_t"]),
                                           _p(c["bo"]), _p(c["gamma"]), _p(c["beta"]), R, beams, S, _p(z), c["eps"], st),
             "singa_dec_tile_cross_attn")
        _chk(lib.singa_dec_tile_ffn(_p(z), _p(f["w1_t"]), _p(f["b1"]), _p(f["w2_t"]), _p(f["b2"]), _p(f["gamma"]), _p(f["beta"]), R,
                                    _p(out), f["eps"], st), "singa_dec_tile_ffn")
        return out
    self_attn, name = (lib.singa_dec_self_attn_rows, "singa_dec_self_attn_rows") if per_row else \
        (lib.singa_dec_self_attn, "singa_dec_self_attn")
    _chk(self_attn(_p(x), _p(a["wqkv_t"]), _p(a["bqkv"]), _p(a["wo_t"]), _p(a["bo"]), _p(a["gamma"]), _p(a["beta"]), _p(k_cache),
                   _p(v_cache), _p(pos), R, P, _p(y), a["eps"], st), name)
    _chk(lib.singa_dec_cross_attn(_p(y), _p(c["wq_t"]), _p(c["bq"]), _p(cross_k), _p(cross_v), _p(pad), _p(c["wo_t"]), _p(c["bo"]),
                                  _p(c["gamma"]), _p(c["beta"]), R, beams, S, _p(z), c["eps"], st), "singa_dec_cross_attn")
    _chk(lib.singa_dec_ffn(_p(z), _p(f["w1_t"]), _p(f["b1"]), _p(f["w2_t"]), _p(f["b2"]), _p(f["gamma"]), _p(f["beta"]), R, _p(out),
                           f["eps"], st), "singa_dec_ffn")
    return out


def _check_views(what, items):
    """Every (tensor, dtype, shape) triple of `items` whose tensor is given: a contiguous GPU tensor of that dtype and, unless
    the shape is None, that shape."""
    for t, dt, shape in items:
        if t is None:
            continue
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise RuntimeError(f"{what}: expected a contiguous {dt} GPU tensor of shape {shape}, got {t.dtype} "
                               f"{tuple(t.shape)} on {t.device}")


def _cap_with_cls(what, cls, cap, vstate):
    """The operands of the valence rule: cap and vstate go together, and only with cls."""
    if (cap is None) != (vstate is None) or (cap is not None and cls is None):
        raise RuntimeError(f"{what}: cap and vstate go together, and only with cls")


def _sample_token_views(what, logits, uniforms, pos, state, allowed, cls=None, gstate=None, alp=None, forced=None, rank=None,
                        cap=None, vstate=None):
    """The argument checks of the token-choice ops; gstate, alp / rank / vstate: the state's grammar, allowed_logp / rank /
    valence where `cls` / `forced` / `cap` is given."""
    _dev(logits, uniforms, state["sum_logp"], state["length"], state["live"], state.get("tok_logp"))
    R, V = logits.shape
    tokens, nxt, fin = state["tokens"], state["next"], state["finished"]
    T = tokens.shape[1]
    _check_views(what, ((tokens, torch.int64, (R, T)), (nxt, torch.int64, (R,)), (fin, torch.uint8, (R,)),
                        (state["length"], torch.int32, (R,)), (state["sum_logp"], torch.float32, (R,)),
                        (state["live"], torch.int32, (1,)), (pos, torch.int64, None), (allowed, torch.uint8, (V,)),
                        (state.get("tok_logp"), torch.float32, (R, T)), (forced, torch.int64, (R, T)),
                        (rank, torch.int32, (R, T)), (cls, torch.uint8, (V,)), (gstate, torch.int32, (R,)),
                        (alp, torch.float32, (R, T)), (cap, torch.uint8, (V,)), (vstate, torch.int32, (R, 2))))
    if not (logits.is_contiguous() and uniforms.is_contiguous() and uniforms.dim() == 2 and uniforms.shape[1] == R
            and uniforms.shape[0] >= T - 1):
        raise RuntimeError(f"{what}: logits [R, V] and uniforms [>= T - 1, R] must be contiguous, got "
                           f"{tuple(logits.shape)}, {tuple(uniforms.shape)} for T = {T}")
    return R, V, T


def sample_token(logits, uniforms, pos, pos_offset, state, temperature=1.0, top_k=0, top_p=1.0, eos=0, pad=0, allowed=None,
                 cls=None, forced=None, cap=None, vstate=None):
    """The next token of every row, drawn on the device (`singa_sample_token`, include/singa_hip.h states the rule; inference
    only, no autograd): one launch.  logits [R, V] f32 (raw projection outputs), uniforms [>= T - 1, R] f32 in [0, 1), pos: int64
    device scalar, the step is pos - pos_offset.  `state`: dict of the rows' device state, updated in place - tokens [R, T] int64,
    next [R] int64, finished [R] uint8, length [R] int32, sum_logp [R] f32, live [1] int32 and, optionally, tok_logp [R, T] f32.
    allowed: [V] uint8, 0 = never drawn.  `cls` / `forced`: the op is `sample_token_grammar` / `sample_token_forced`, which
    describe them; this is where all three assemble their arguments.  `cap` ([V] uint8 capacities, `smiles.capacity`; with the
    class bytes of `smiles.classify_orders`) and `vstate` ([R, 2] int32, updated in place; a row whose grammar word is
    `smiles.FRESH` needs no reset of it): the valence rule of include/singa_hip_valence.h (`singa_sample_token_valence`) in
    place of the SMILES rule, with or without `forced`."""
    _cap_with_cls("sample_token", cls, cap, vstate)
    entry = "sample_token_valence" if cap is not None else "sample_token_forced" if forced is not None else \
        "sample_token_grammar" if cls is not None else "sample_token"
    rank = state.get("rank") if forced is not None else None
    gstate, alp = (state["grammar"], state.get("allowed_logp")) if cls is not None else (None, None)
    for t in (rank, gstate, alp, vstate):
        if t is not None:
            _dev(t)
    R, V, T = _sample_token_views(entry, logits, uniforms, pos, state, allowed, cls, gstate, alp, forced, rank, cap, vstate)
    lib, head = _lib.lib(), (_p(logits), _p(uniforms), _p(allowed))
    rest = (_p(pos), pos_offset, R, V, T, temperature, top_k, top_p, eos, pad, _p(state["finished"]), _p(state["length"]),
            _p(state["sum_logp"]), _p(state["tokens"]), _p(state["next"]), _p(state["live"]), _p(state.get("tok_logp")))
    if cap is not None:
        code = lib.singa_sample_token_valence(*head, _p(cls), _p(cap), _p(pos), None, pos_offset, R, 0, *rest[3:], _p(gstate),
                                              _p(vstate), _p(alp), _p(forced), _p(rank), _stream())
    elif forced is not None:
        code = lib.singa_sample_token_forced(*head, _p(cls), *rest, _p(gstate), _p(alp), _p(forced), _p(rank), _stream())
    elif cls is not None:
        code = lib.singa_sample_token_grammar(*head, _p(cls), *rest, _p(gstate), _p(alp), _stream())
    else:
        code = lib.singa_sample_token(*head, *rest, _stream())
    _chk(code, "singa_" + entry)


def sample_token_grammar(logits, uniforms, pos, pos_offset, state, cls, temperature=1.0, top_k=0, top_p=1.0, eos=0, pad=0,
                         allowed=None):
    """`sample_token` under the SMILES rule of include/singa_hip_gen.h (`singa_sample_token_grammar`): the mask is `allowed` AND
    what the rule lets follow the row's state.  cls: [V] uint8 class bytes (`singa_amd.smiles.classify`); `state` as for
    `sample_token`, plus grammar [R] int32 (the rows' packed rule state, `smiles.FRESH` for a fresh row; updated in place) and,
    optionally, allowed_logp [R, T] f32 (log of the model's probability mass on the effective mask)."""
    sample_token(logits, uniforms, pos, pos_offset, state, temperature, top_k, top_p, eos, pad, allowed, cls=cls)


def sample_token_forced(logits, uniforms, pos, pos_offset, state, forced, cls=None, temperature=1.0, top_k=0, top_p=1.0, eos=0,
                        pad=0, allowed=None):
    """`sample_token` (cls=None) or `sample_token_grammar` (cls: [V] uint8 class bytes) with given tokens
    (`singa_sample_token_forced`, include/singa_hip_force.h states the rule): forced [R, T] int64, contiguous, on the GPU - at
    step t a row whose forced[row, t + 1] lies in [0, V) takes that token with the bookkeeping of a drawn one, any other row
    chooses as the unforced op does, bit for bit.  `state` as for those ops (grammar [R] int32 and, optionally, allowed_logp
    under the grammar) and, optionally, rank [R, T] int32: the rank of every emitted token among the row's raw logits."""
    sample_token(logits, uniforms, pos, pos_offset, state, temperature, top_k, top_p, eos, pad, allowed, cls=cls, forced=forced)


def sample_token_stream(logits, uniforms, pos, mol, pos_offset, state, temperature=1.0, top_k=0, top_p=1.0, eos=0, pad=0,
                        allowed=None, cls=None, cap=None, vstate=None, forced=None):
    """`sample_token` (cls=None) or `sample_token_grammar` for rows that hold a molecule each (`singa_sample_token_stream`,
    include/singa_hip_stream.h states the rule; inference only): logits [R, V] f32; pos [R] int64, the rows' own positions (a
    row's step is pos - pos_offset); mol [R] int32, the molecule a row decodes (-1: retired, the row is skipped); uniforms
    [>= T - 1, M] f32, one column per molecule.  `state`: tokens [M, T] int64, length [M] int32, sum_logp [M] f32 and,
    optionally, tok_logp [M, T] f32 - indexed by molecule - and next [R] int64; with `cls` also grammar [R] int32 and, optionally,
    allowed_logp [M, T] f32.  Updated in place, bit for bit as the per-row ops update a row that draws the same logits.
    `cap` [V] uint8 and `vstate` [R, 2] int32 (with `cls`): the valence rule, as in `sample_token`.
    `forced` [M, T] int64, one row per molecule: the op is `singa_sample_token_stream_forced` (include/singa_hip_prefix.h), under
    any of the three rules; a molecule whose forced[j, t + 1] lies in [0, V) takes that token at its step t, as in
    `sample_token_forced`, and `state` may then hold rank [M, T] int32."""
    _cap_with_cls("sample_token_stream", cls, cap, vstate)
    R, V = logits.shape
    M, T = state["tokens"].shape
    gstate, alp = (state["grammar"], state.get("allowed_logp")) if cls is not None else (None, None)
    rank = state.get("rank") if forced is not None else None
    _check_views("sample_token_stream", (
        (forced, torch.int64, (M, T)), (rank, torch.int32, (M, T)),
        (logits, torch.float32, (R, V)), (uniforms, torch.float32, None), (pos, torch.int64, (R,)), (mol, torch.int32, (R,)),
        (state["tokens"], torch.int64, (M, T)), (state["length"], torch.int32, (M,)), (state["sum_logp"], torch.float32, (M,)),
        (state.get("tok_logp"), torch.float32, (M, T)), (state["next"], torch.int64, (R,)), (allowed, torch.uint8, (V,)),
        (cls, torch.uint8, (V,)), (gstate, torch.int32, (R,)), (alp, torch.float32, (M, T)), (cap, torch.uint8, (V,)),
        (vstate, torch.int32, (R, 2))))
    if uniforms.dim() != 2 or uniforms.shape[1] != M or uniforms.shape[0] < T - 1:
        raise RuntimeError(f"sample_token_stream: uniforms [>= T - 1, molecules], got {tuple(uniforms.shape)} for T = {T}, {M} molecules")
    _lib.ensure_init(logits.device.index if logits.device.index is not None else torch.cuda.current_device())
    if forced is not None:
        _chk(_lib.lib().singa_sample_token_stream_forced(_p(logits), _p(uniforms), _p(allowed), _p(cls), _p(cap), _p(pos), _p(mol),
                                                         pos_offset, R, M, V, T, temperature, top_k, top_p, eos, pad,
                                                         _p(state["length"]), _p(state["sum_logp"]), _p(state["tokens"]),
                                                         _p(state["next"]), _p(state.get("tok_logp")), _p(gstate), _p(vstate), _p(alp),
                                                         _p(forced), _p(rank), _stream()), "singa_sample_token_stream_forced")
        return
    if cap is not None:
        _chk(_lib.lib().singa_sample_token_valence(_p(logits), _p(uniforms), _p(allowed), _p(cls), _p(cap), _p(pos), _p(mol), pos_offset,
                                                   R, M, V, T, temperature, top_k, top_p, eos, pad, None, _p(state["length"]),
                                                   _p(state["sum_logp"]), _p(state["tokens"]), _p(state["next"]), None,
                                                   _p(state.get("tok_logp")), _p(gstate), _p(vstate), _p(alp), None, None, _stream()),
             "singa_sample_token_valence")
        return
    _chk(_lib.lib().singa_sample_token_stream(_p(logits), _p(uniforms), _p(allowed), _p(cls), _p(pos), _p(mol), pos_offset, R, M, V,
                                              T, temperature, top_k, top_p, eos, pad, _p(state["length"]), _p(state["sum_logp"]),
                                              _p(state["tokens"]), _p(state["next"]), _p(state.get("tok_logp")), _p(gstate), _p(alp),
                                              _stream()), "singa_sample_token_stream")


def stream_refill(pos, mol, pos_offset, state, rows_per_pocket, num_samples, T, sos=0, eos=0, fresh=0, grammar=False):
    """The hand-over of continuous sampling (`singa_stream_refill`, include/singa_hip_stream.h states the rule): per pocket the
    rows that have ended their molecule take the pocket's next molecules in ascending row order, or retire; every other live
    row moves on by one position.  pos [R] int64, mol [R] int32, `state`: next [R] int64, issued / live [pockets] int32, row_of /
    start_step [pockets * num_samples] int32 and, with `grammar`, grammar [R] int32 (restarted at `fresh`).  One launch, one
    workgroup per pocket."""
    B = state["issued"].shape[0]
    R, M = B * rows_per_pocket, B * num_samples
    gstate = state["grammar"] if grammar else None
    _check_views("stream_refill", ((pos, torch.int64, (R,)), (mol, torch.int32, (R,)), (state["next"], torch.int64, (R,)),
                                   (gstate, torch.int32, (R,)), (state["issued"], torch.int32, (B,)),
                                   (state["live"], torch.int32, (B,)), (state["row_of"], torch.int32, (M,)),
                                   (state["start_step"], torch.int32, (M,))))
    _lib.ensure_init(pos.device.index if pos.device.index is not None else torch.cuda.current_device())
    _chk(_lib.lib().singa_stream_refill(B, rows_per_pocket, num_samples, T, pos_offset, sos, eos, fresh, _p(pos), _p(mol),
                                        _p(state["next"]), _p(gstate), _p(state["issued"]), _p(state["live"]), _p(state["row_of"]),
                                        _p(state["start_step"]), _stream()), "singa_stream_refill")


def _slot_work(what, rows, T, device):
    """The scratch of a slot search's select op: a uint8 tensor of `singa_<what>(rows, T)` bytes."""
    n = int(getattr(_lib.lib(), "singa_" + what)(rows, T))
    if n < 0:
        raise RuntimeError(f"{what}: rows >= 0 and T >= 2, got {rows}, {T}")
    return torch.empty(max(n, 16), dtype=torch.uint8, device=device)


def swor_work(rows, T, device):
    """The scratch `swor_select` needs for `rows` rows of `T` columns: a uint8 tensor of `singa_swor_work` bytes."""
    return _slot_work("swor_work", rows, T, device)


def _slot_views(what, state, R, k, V, T, names, cls=None, cap=None, extra=()):
    """The argument checks of the swor and beam ops (R = pockets x k slots): `names` of `state` - and grammar with `cls`,
    vstate with `cap` - are contiguous GPU tensors of the dtypes / shapes of include/singa_hip_swor.h and singa_hip_beam.h."""
    B, f32, i32, i64 = R // max(k, 1), torch.float32, torch.int32, torch.int64
    spec = {"gumbel": (f32, (R,)), "prop_logp": (f32, (R,)), "sum_logp": (f32, (R,)), "hash": (i64, (R,)),
            "finished": (torch.uint8, (R,)), "tok_logp": (f32, (R, T)), "cand_logp": (f32, (R, V)), "cand_phi": (f32, (R, V)),
            "score": (f32, (R,)), "length": (i32, (R,)), "tokens": (i64, (R, T)), "next": (i64, (R,)), "src": (i64, (R,)),
            "grammar": (i32, (R,)), "vstate": (i32, (R, 2)), "cand": (f32, (R, V)), "hyp_score": (torch.float64, (R,)),
            "hyp_sum": (f32, (R,)), "hyp_len": (i32, (R,)), "hyp_stamp": (i32, (R,)), "hyp_tokens": (i64, (R, T)),
            "n_hyp": (i32, (B,)), "worst": (torch.float64, (B,)), "done": (torch.uint8, (B,)), "live": (i32, (B,))}
    if cap is not None and cls is None:
        raise RuntimeError(f"{what}: cap goes only with cls")
    names = names + (("grammar",) if cls is not None else ()) + (("vstate",) if cap is not None else ())
    items = [(state[n],) + spec[n] for n in names] + [(cls, torch.uint8, (V,)), (cap, torch.uint8, (V,))] + list(extra)
    _check_views(what, items)
    _lib.ensure_init(items[0][0].device.index if items[0][0].device.index is not None else torch.cuda.current_device())


def swor_expand(logits, pos, pos_offset, state, k, streams, temperature=1.0, seed=0, pad=0, allowed=None, cls=None, forced=None):
    """Sub-steps 1 to 3 of stochastic beam search (`singa_swor_expand`, include/singa_hip_swor.h states the rule; inference
    only): the perturbed, parent-conditioned score of every candidate of every row.  logits [R, V] f32, R = pockets * k; pos:
    int64 device scalar (the step is pos - pos_offset); streams [pockets] int32 (read as 32-bit words); `state`: gumbel,
    prop_logp [R] f32, hash [R] int64 (the 64 bits of the prefix hash), finished [R] uint8, tokens [R, T] (for T only), with
    `cls` ([V] uint8 class bytes) also grammar [R] int32 - all read - and cand, cand_logp, cand_phi [R, V] f32, written.
    `forced` [pockets, T] int64, one prefix per pocket: the op is `singa_swor_expand_forced` (include/singa_hip_prefix.h) - where
    forced[p, t + 1] lies in [0, V) that token is the only candidate of pocket p's live rows, with the row's own G and phi."""
    R, V = logits.shape
    T = state["tokens"].shape[1]
    _slot_views("swor_expand", state, R, k, V, T, ("gumbel", "prop_logp", "hash", "finished", "cand", "cand_logp", "cand_phi"), cls,
                None, ((allowed, torch.uint8, (V,)), (logits, torch.float32, (R, V)), (pos, torch.int64, None),
                       (streams, torch.int32, (R // max(k, 1),)), (forced, torch.int64, (R // max(k, 1), T))))
    args = (_p(logits), _p(allowed), _p(cls), _p(pos), pos_offset, R, k, V, T, temperature, int(seed) & (2 ** 64 - 1), _p(streams), pad,
            _p(state["gumbel"]), _p(state["prop_logp"]), _p(state["hash"]), _p(state["finished"]),
            _p(state["grammar"] if cls is not None else None), _p(state["cand"]), _p(state["cand_logp"]), _p(state["cand_phi"]))
    if forced is not None:
        _chk(_lib.lib().singa_swor_expand_forced(*args, _p(forced), _stream()), "singa_swor_expand_forced")
    else:
        _chk(_lib.lib().singa_swor_expand(*args, _stream()), "singa_swor_expand")


def swor_select(pos, pos_offset, state, k, work, eos=0, pad=0, cls=None):
    """Sub-steps 4 and 5 (`singa_swor_select`): per pocket the k best candidates of `state`'s cand in the rule's order become
    the new slots; gumbel, prop_logp, sum_logp, hash, finished, length, (grammar,) tokens and tok_logp follow the parents,
    next [R] int64 (the emitted token), src [R] int64 (the parent row) and live [pockets] int32 are written.  `work`:
    `swor_work(R, T, device)`."""
    R, V = state["cand"].shape
    T = state["tokens"].shape[1]
    names = ("gumbel", "prop_logp", "sum_logp", "hash", "finished", "length", "tokens", "tok_logp", "next", "src", "cand",
             "cand_logp", "cand_phi")
    _slot_views("swor_select", state, R, k, V, T, names, cls, None,
                ((pos, torch.int64, None), (state["live"], torch.int32, (R // max(k, 1),)), (work, torch.uint8, None)))
    need = int(_lib.lib().singa_swor_work(R, T))
    if work.numel() < need:
        raise RuntimeError(f"swor_select: work holds {work.numel()} bytes, singa_swor_work({R}, {T}) = {need}")
    _chk(_lib.lib().singa_swor_select(_p(state["cand"]), _p(state["cand_logp"]), _p(state["cand_phi"]), _p(cls), _p(pos),
                                      pos_offset, R, k, V, T, eos, pad, _p(state["gumbel"]), _p(state["prop_logp"]),
                                      _p(state["sum_logp"]), _p(state["hash"]), _p(state["finished"]), _p(state["length"]),
                                      _p(state["grammar"] if cls is not None else None), _p(state["tokens"]),
                                      _p(state["tok_logp"]), _p(state["next"]), _p(state["src"]), _p(state["live"]), _p(work),
                                      _stream()), "singa_swor_select")


def swor_follow(k_src, v_src, k_dst, v_dst, src, gumbel, finished, pos):
    """The caches follow the surviving prefixes (`singa_swor_follow`): positions [0, pos) of every layer's and head's keys /
    values move from row src[r] of (k_src, v_src) to row r of (k_dst, v_dst), skipping dead (gumbel = -inf) and finished rows;
    one launch, 16-byte accesses.  Caches [layers, R, heads, P, dk] / [.., dv] f32, dense from the heads on (row and layer
    strides are passed on); the two buffers are alike and distinct."""
    n, R, H, P, dk = k_src.shape
    dv = v_src.shape[4]
    for a, b, d in ((k_src, k_dst, dk), (v_src, v_dst, dv)):
        if not (a.is_cuda and b.is_cuda and a.dtype == b.dtype == torch.float32 and tuple(a.shape) == tuple(b.shape) == (n, R, H, P, d)
                and a.stride() == b.stride() and a.stride()[2:] == (P * d, d, 1)):
            raise RuntimeError(f"swor_follow: two alike float32 GPU caches [layers, rows, heads, P, d], dense from the heads on; "
                               f"got {tuple(a.shape)} {a.stride()} and {tuple(b.shape)} {b.stride()}")
    for t, dt in ((src, torch.int64), (gumbel, torch.float32), (finished, torch.uint8)):
        if not t.is_cuda or t.dtype != dt or not t.is_contiguous() or tuple(t.shape) != (R,):
            raise RuntimeError(f"swor_follow: expected a contiguous {dt} GPU tensor of shape {(R,)}, got {t.dtype} {tuple(t.shape)}")
    if not pos.is_cuda or pos.dtype != torch.int64:
        raise RuntimeError("swor_follow: pos is an int64 device scalar")
    _lib.ensure_init(k_src.device.index if k_src.device.index is not None else torch.cuda.current_device())
    _chk(_lib.lib().singa_swor_follow(_p(k_src), _p(v_src), _p(k_dst), _p(v_dst), _p(src), _p(gumbel), _p(finished), _p(pos), n, R,
                                      H, P, dk, dv, k_src.stride(1), k_src.stride(0), v_src.stride(1), v_src.stride(0), _stream()),
         "singa_swor_follow")


def beam_work(rows, T, device):
    """The scratch `beam_select` needs for `rows` rows of `T` columns: a uint8 tensor of `singa_beam_work` bytes."""
    return _slot_work("beam_work", rows, T, device)


def beam_expand(logits, pos, pos_offset, state, k, allowed=None, cls=None, cap=None, forced=None):
    """Sub-step 1 of the device beam search (`singa_beam_expand`, include/singa_hip_beam.h states the rule; inference only):
    the summed log-probability of every candidate of every live row, -inf where `allowed`, the SMILES rule (`cls`: [V] uint8
    class bytes) or the valence rule (`cls` of `smiles.classify_orders` and `cap`: [V] uint8 capacities) refuses the token.
    logits [R, V] f32, R = pockets * k; pos: int64 device scalar (the step is pos - pos_offset); `state`: score [R] f32, tokens
    [R, T] (for T only), done [pockets] uint8, with `cls` grammar [R] int32, with `cap` vstate [R, 2] int32 - all read - and
    cand [R, V] f32, written.  `forced` [pockets, T] int64, one prefix per pocket: the op is `singa_forced_beam_expand`
    (include/singa_hip_prefix.h) - where forced[p, t + 1] lies in [0, V) that token is the only candidate of pocket p's live rows."""
    R, V = logits.shape
    T = state["tokens"].shape[1]
    _slot_views("beam_expand", state, R, k, V, T, ("score", "done", "cand"), cls, cap,
                ((logits, torch.float32, (R, V)), (pos, torch.int64, None), (allowed, torch.uint8, (V,)),
                 (forced, torch.int64, (R // max(k, 1), T))))
    args = (_p(logits), _p(allowed), _p(cls), _p(cap), _p(pos), pos_offset, R, k, V, T, _p(state["score"]),
            _p(state["grammar"] if cls is not None else None), _p(state["vstate"] if cap is not None else None), _p(state["done"]),
            _p(state["cand"]))
    if forced is not None:
        _chk(_lib.lib().singa_forced_beam_expand(*args, _p(forced), _stream()), "singa_forced_beam_expand")
    else:
        _chk(_lib.lib().singa_beam_expand(*args, _stream()), "singa_beam_expand")


def beam_select(pos, pos_offset, state, k, work, len_pow, eos=0, pad=0, cls=None, cap=None):
    """Sub-steps 2 and 3 (`singa_beam_select`): per pocket that is not done the 2k best candidates of `state`'s cand are walked
    with the reference's rules - '$' candidates inside the first k are stored among the pocket's hypotheses (hyp_score f64,
    hyp_sum f32, hyp_len, hyp_stamp int32 [R], hyp_tokens [R, T] int64, n_hyp int32, worst f64, done uint8 [pockets]), the others
    become the new slots (score, length, tokens, next, src, grammar, vstate follow the parents) - and live [pockets] int32 is
    written.  len_pow: [>= T] f64 on the device, n ** length_penalty.  `work`: `beam_work(R, T, device)`."""
    R, V = state["cand"].shape
    T = state["tokens"].shape[1]
    names = ("score", "length", "tokens", "next", "src", "cand", "hyp_score", "hyp_sum", "hyp_len", "hyp_stamp", "hyp_tokens",
             "n_hyp", "worst", "done", "live")
    _slot_views("beam_select", state, R, k, V, T, names, cls, cap,
                ((pos, torch.int64, None), (work, torch.uint8, None), (len_pow, torch.float64, None)))
    need = int(_lib.lib().singa_beam_work(R, T))
    if work.numel() < need or len_pow.numel() < T:
        raise RuntimeError(f"beam_select: work holds {work.numel()} bytes, singa_beam_work({R}, {T}) = {need}; len_pow holds "
                           f"{len_pow.numel()} entries for T = {T}")
    s = state
    _chk(_lib.lib().singa_beam_select(_p(s["cand"]), _p(cls), _p(cap), _p(pos), pos_offset, R, k, V, T, eos, pad, _p(len_pow),
                                      _p(s["score"]), _p(s["length"]), _p(s["tokens"]), _p(s["next"]), _p(s["src"]),
                                      _p(s["grammar"] if cls is not None else None), _p(s["vstate"] if cap is not None else None),
                                      _p(s["hyp_score"]), _p(s["hyp_sum"]), _p(s["hyp_len"]), _p(s["hyp_stamp"]), _p(s["hyp_tokens"]),
                                      _p(s["n_hyp"]), _p(s["worst"]), _p(s["done"]), _p(s["live"]), _p(work), _stream()),
         "singa_beam_select")


class _MaskedSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, mask, scale, heads):
        s = s.contiguous()
        _dev(s)
        assert mask.dtype == torch.bool and mask.dim() == 3 and mask.stride(2) == 1 and mask.is_cuda
        BH, T, S = s.shape
        p = torch.empty_like(s)
        assert mask.shape[0] * heads == BH and mask.shape[2] == S and mask.shape[1] in (1, T)
        ctx.mst = 0 if mask.shape[1] == 1 else mask.stride(1)          # a [B, 1, S] padding mask serves every query row
        _chk(_lib.lib().singa_masked_softmax_fwd(_p(s), _p(mask), mask.stride(0), ctx.mst, _p(p), BH, T, S, heads, scale,
                                                 _stream()), "singa_masked_softmax_fwd")
        ctx.save_for_backward(p, mask)
        ctx.scale, ctx.heads = scale, heads
        return p

    @staticmethod
    def backward(ctx, gp):
        p, mask = ctx.saved_tensors
        gp = gp.contiguous()
        BH, T, S = p.shape
        gs = torch.empty_like(p)
        _chk(_lib.lib().singa_masked_softmax_bwd(_p(p), _p(gp), _p(mask), mask.stride(0), ctx.mst, _p(gs), BH, T, S, ctx.heads,
                                                 ctx.scale, _stream()), "singa_masked_softmax_bwd")
        return gs, None, None, None


def masked_softmax(s, mask, scale, heads):
    """softmax(masked_fill(s * scale, mask, -1e9), -1) for attention scores s[B*heads, T, S] and a boolean mask [B, T, S]
    (k18): one pass instead of divide, masked_fill and softmax, forward and backward."""
    return _MaskedSoftmax.apply(s, mask, scale, heads)


def _tok_view(t, heads, D):
    """A token-major attention operand [B, T, heads, D]: dense, or a column block of a wider [B, T, P] buffer (the fused
    W_Q | W_K | W_V projection output).  Returns (tensor usable as it is, token pitch in floats) - a copy if the view
    cannot be addressed as (base, pitch)."""
    B, T = t.shape[0], t.shape[1]
    st = t.stride()
    ok = (st[3] == 1 and st[2] == D and st[1] % 4 == 0 and st[1] >= heads * D and (T == 1 or st[0] == T * st[1] or B == 1)
          and t.data_ptr() % 16 == 0)
    if B > 1 and T == 1:
        ok = ok and st[0] == st[1]
    if not ok:
        t = t.contiguous()
        return t, heads * D
    return t, st[1]


def _fused_blocks(ts):
    """True when the views ts (same leading shape) are consecutive column blocks of one row-pitched buffer."""
    p0, pitch = ts[0].data_ptr(), ts[0].stride(1)
    off = 0
    for t in ts:
        if t.stride(1) != pitch or t.stride(0) != ts[0].stride(0) or t.data_ptr() != p0 + 4 * off:
            return False
        off += t.shape[2] * t.shape[3]
    return pitch >= off


class _Attention(torch.autograd.Function):
    """softmax(masked_fill(q k^T * scale, mask, -1e9)) v on the MFMA (k19): scores never leave registers; the backward
    recomputes them from q, k and the stored log-sum-exp.  token_major: q / k / v / context are [B, T|S, heads, D] (as the
    projections produce them) instead of [B*heads, T|S, D] - no head transposes; q / k / v may then be column blocks of one
    fused projection output, and their gradients are written as the same column blocks of one buffer, so that the fused
    projection's backward takes them without a copy."""

    @staticmethod
    def forward(ctx, q, k, v, mask, scale, heads, token_major, tile_rows=None, tile_cols=None):
        assert mask.dtype == torch.bool and mask.dim() == 3 and mask.stride(2) == 1 and mask.is_cuda
        if token_major:
            B, T, _, DK = q.shape
            S, DV = v.shape[1], v.shape[3]
            BH = B * heads
            assert q.shape[2] == heads and k.shape == (B, S, heads, DK) and v.shape[:3] == (B, S, heads)
            (q, lq), (k, lk), (v, lv) = _tok_view(q, heads, DK), _tok_view(k, heads, DK), _tok_view(v, heads, DV)
            out = torch.empty(B, T, heads, DV, device=q.device, dtype=torch.float32)
        else:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            lq = lk = lv = 0
            BH, T, DK = q.shape
            S, DV = v.shape[1], v.shape[2]
            out = torch.empty(BH, T, DV, device=q.device, dtype=torch.float32)
        _dev(q, k, v)
        assert mask.shape[0] * heads == BH and mask.shape[2] == S and mask.shape[1] in (1, T)
        ctx.mst = 0 if mask.shape[1] == 1 else mask.stride(1)
        lse = torch.empty(BH, T, 2, device=q.device, dtype=torch.float32)       # (row maximum, 1 / row sum)
        if tile_rows is None:
            _chk(_lib.lib().singa_attn_fwd(_p(q), _p(k), _p(v), _p(mask), mask.stride(0), ctx.mst, _p(out), _p(lse), BH, T, S, heads,
                                           DK, DV, int(token_major), lq, lk, lv, scale, _stream()), "singa_attn_fwd")
            ctx.save_for_backward(q, k, v, mask, out, lse)
        else:
            _check_tiles(tile_rows, tile_cols, mask.shape[0], T, S)
            _chk(_lib.lib().singa_attn_tiled_fwd(_p(q), _p(k), _p(v), _p(mask), mask.stride(0), ctx.mst, _p(out), _p(lse), BH, T, S,
                                                 heads, DK, DV, int(token_major), lq, lk, lv, scale, _p(tile_rows), _stream()),
                 "singa_attn_tiled_fwd")
            ctx.save_for_backward(q, k, v, mask, out, lse, tile_rows, tile_cols)
        ctx.scale, ctx.heads, ctx.tm, ctx.dims, ctx.ld = scale, heads, bool(token_major), (BH, T, S, DK, DV), (lq, lk, lv)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, mask, out, lse, *tiles = ctx.saved_tensors
        g = g.contiguous()
        BH, T, S, DK, DV = ctx.dims
        lq, lk, lv = ctx.ld

        def like(ts):
            """Gradients laid out like the operands: column blocks of ONE buffer where the operands are."""
            if ctx.tm and len(ts) > 1 and _fused_blocks(ts):
                B, rows, pitch = ts[0].shape[0], ts[0].shape[1], ts[0].stride(1)
                buf = torch.empty(B, rows, pitch, device=g.device, dtype=torch.float32)
                outs, off = [], 0
                for t in ts:
                    w = t.shape[2] * t.shape[3]
                    outs.append(buf[:, :, off:off + w].view(B, rows, t.shape[2], t.shape[3]))
                    off += w
                if off < pitch:                       # columns of the buffer no operand covers (none in the model's layouts)
                    buf[:, :, off:].zero_()
                return outs
            return [torch.empty(t.shape, device=g.device, dtype=torch.float32) for t in ts]

        if ctx.tm and T == S and _fused_blocks([q, k, v]):
            gq, gk, gv = like([q, k, v])
        elif ctx.tm and _fused_blocks([k, v]):
            (gq,), (gk, gv) = like([q]), like([k, v])
        else:
            (gq,), (gk,), (gv,) = like([q]), like([k]), like([v])
        if ctx.tm:
            lq, lk, lv = gq.stride(1), gk.stride(1), gv.stride(1)
            # the kernels address the gradients with the operands' pitches: they agree by construction
            assert (lq, lk, lv) == (q.stride(1), k.stride(1), v.stride(1))
        dsum = torch.empty(BH, T, device=q.device, dtype=torch.float32)
        if tiles:
            _chk(_lib.lib().singa_attn_tiled_bwd(_p(q), _p(k), _p(v), _p(mask), mask.stride(0), ctx.mst, _p(out), _p(lse), _p(g),
                                                 _p(gq), _p(gk), _p(gv), _p(dsum), BH, T, S, ctx.heads, DK, DV, int(ctx.tm), lq, lk,
                                                 lv, ctx.scale, _p(tiles[0]), _p(tiles[1]), _stream()), "singa_attn_tiled_bwd")
        else:
            _chk(_lib.lib().singa_attn_bwd(_p(q), _p(k), _p(v), _p(mask), mask.stride(0), ctx.mst, _p(out), _p(lse), _p(g), _p(gq),
                                           _p(gk), _p(gv), _p(dsum), BH, T, S, ctx.heads, DK, DV, int(ctx.tm), lq, lk, lv, ctx.scale,
                                           _stream()), "singa_attn_bwd")
        return gq, gk, gv, None, None, None, None, None, None


def _tile_shapes(B, T, S):
    qt, kt = (T + 31) // 32, (S + 31) // 32
    return (B, qt, (kt + 31) // 32), (B, kt, (qt + 31) // 32)


def _check_tiles(tile_rows, tile_cols, B, T, S):
    for t, shape in zip((tile_rows, tile_cols), _tile_shapes(B, T, S)):
        assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shape, (tuple(t.shape), shape)


def attn_tiles(mask, T, S):
    """The tile map of a boolean attention mask [B, T|1, S] (include/singa_hip_attn_tiles.h): which 32 x 32 tiles of the score
    matrix `attention(..., tiles=...)` has to compute.  It depends on the mask alone: build it once per mask and pass it to
    every attention that uses that mask.  Returns (tile_rows, tile_cols), the two orientations of the bits."""
    assert mask.dtype == torch.bool and mask.dim() == 3 and mask.stride(2) == 1 and mask.is_cuda
    assert mask.shape[2] == S and mask.shape[1] in (1, T)
    B = mask.shape[0]
    rs, cs = _tile_shapes(B, T, S)
    rows = torch.empty(rs, device=mask.device, dtype=torch.int32)
    cols = torch.empty(cs, device=mask.device, dtype=torch.int32)
    mst = 0 if mask.shape[1] == 1 else mask.stride(1)
    _chk(_lib.lib().singa_attn_tiles(_p(mask), mask.stride(0), mst, _p(rows), _p(cols), B, T, S, _stream()), "singa_attn_tiles")
    return rows, cols


def attention(q, k, v, mask, scale, heads, token_major=False, tiles=None):
    """Dense attention core (k19) for q[B*heads,T,32], k[B*heads,S,32], v[B*heads,S,64] - or, token_major, q[B,T,heads,32],
    k[B,S,heads,32], v[B,S,heads,64] (dense, or column blocks of a fused projection output) -> context in the same layout
    - and a boolean mask [B, T|1, S].  tiles: `attn_tiles(mask, T, S)` of the same mask - the kernels then skip the score
    tiles that are masked in every element; the result is the same."""
    if tiles is None:
        return _Attention.apply(q, k, v, mask, scale, heads, token_major)
    return _Attention.apply(q, k, v, mask, scale, heads, token_major, tiles[0], tiles[1])


class _LayerNorm256(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, r, gamma, beta, eps):
        ctx.params = (gamma, beta)
        a = a.contiguous()
        r = r.contiguous() if r is not None else None
        gamma, beta = gamma.contiguous(), beta.contiguous()
        _dev(a, gamma, beta)
        M = a.numel() // 256
        y = torch.empty_like(a)
        _chk(_lib.lib().singa_ln256_fwd(_p(a), _p(r) if r is not None else None, _p(gamma), _p(beta), _p(y), M, 256, eps,
                                        _stream()), "singa_ln256_fwd")
        ctx.save_for_backward(a, r, gamma)
        ctx.eps = eps
        return y

    @staticmethod
    def backward(ctx, g):
        a, r, gamma = ctx.saved_tensors
        g = g.contiguous()
        M = a.numel() // 256
        lib = _lib.lib()
        gs = torch.empty_like(a)
        part = torch.empty(lib.singa_ln256_nparts(M), 512, device=a.device, dtype=torch.float32)
        _chk(lib.singa_ln256_bwd(_p(a), _p(r) if r is not None else None, _p(gamma), _p(g), _p(gs), _p(part), M, 256, ctx.eps,
                                 _stream()), "singa_ln256_bwd")
        gg, gb = param_colsum(part, [(0, 256, ctx.params[0]), (256, 256, ctx.params[1])])
        return gs, (gs if r is not None else None), gg, gb, None


def layer_norm_residual(a, r, ln):
    """ln(a + r) for an nn.LayerNorm `ln` (r may be None).  256-channel rows on the GPU take the fused kernel (k16): the sum
    is never materialised and the backward is one pass + a column sum."""
    if a.shape[-1] == 256 and tuple(ln.normalized_shape) == (256,) and (r is None or r.shape == a.shape):
        return _LayerNorm256.apply(a, r, ln.weight, ln.bias, ln.eps)
    return ln(a if r is None else a + r)


class _BiasSsp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, u, b):
        ctx.param = b
        u, b = u.contiguous(), b.contiguous()
        _dev(u, b)
        n = u.shape[-1]
        y = torch.empty_like(u)
        _chk(_lib.lib().singa_bias_ssp_fwd(_p(u), _p(b), _p(y), u.numel() // n, n, _stream()), "singa_bias_ssp_fwd")
        ctx.save_for_backward(u, b)
        return y

    @staticmethod
    def backward(ctx, g):
        u, b = ctx.saved_tensors
        g = g.contiguous()
        n = u.shape[-1]
        gu = torch.empty_like(u)
        _chk(_lib.lib().singa_bias_ssp_bwd(_p(u), _p(b), _p(g), _p(gu), u.numel() // n, n, _stream()), "singa_bias_ssp_bwd")
        return gu, param_colsum(gu.reshape(-1, n), [(0, n, ctx.param)])[0]


def bias_ssp(u, b):
    """softplus(u + b) - ln 2 (k15d): ShiftedSoftplus with the preceding Linear's bias folded in."""
    return _BiasSsp.apply(u, b)


class _EdgeMLPPair(torch.autograd.Function):
    """(W_k, W_v) = (L2k(ssp(L1k(attr))), L2v(ssp(L1v(attr)))) for all kNN edges (CP:41-48, 58, 68) on the f32 MFMA
    (k15c): one kernel forward for both nets, one kernel per net backward; only the attribute rows are kept for the
    backward pass, which recomputes the hidden units and reduces all four parameter gradients itself."""

    @staticmethod
    def forward(ctx, attr, unit_a, unit_b, w1k, b1k, w2k, b2k, w1v, b1v, w2v, b2v):
        ctx.params = (w1k, b1k, w2k, b2k, w1v, b1v, w2v, b2v)
        attr = attr.contiguous()
        fw = [t.contiguous() for t in (w1k, b1k, w2k, b2k, w1v, b1v, w2v, b2v)]      # nn.Linear's own layouts, no copies
        _dev(attr, *fw)
        E, CIN = attr.shape
        HK, HV = w1k.shape[0], w1v.shape[0]
        wk = torch.empty(E, HK, device=attr.device, dtype=torch.float32)
        wv = torch.empty(E, HV, device=attr.device, dtype=torch.float32)
        ctx.units = unit_a is not None
        if ctx.units:           # once per undirected edge (include/singa_hip_units.h): every row is some unit's a or b
            unit_a, unit_b = unit_a.contiguous(), unit_b.contiguous()
            _dev(unit_a, unit_b)
            assert unit_a.dtype == unit_b.dtype == torch.int32 and unit_a.shape == unit_b.shape == (E,)
            _chk(_lib.lib().singa_edge_mlp_units_fwd(_p(attr), _p(unit_a), _p(unit_b), *[_p(t) for t in fw], _p(wk), _p(wv), E, CIN,
                                                     HK, HV, _stream()), "singa_edge_mlp_units_fwd")
            ctx.save_for_backward(attr, fw[0], fw[1], fw[2], fw[4], fw[5], fw[6], unit_a, unit_b)
            return wk, wv
        _chk(_lib.lib().singa_edge_mlp_fwd(_p(attr), *[_p(t) for t in fw], _p(wk), _p(wv), E, CIN, HK, HV, _stream()),
             "singa_edge_mlp_fwd")
        ctx.save_for_backward(attr, fw[0], fw[1], fw[2], fw[4], fw[5], fw[6])
        return wk, wv

    @staticmethod
    def backward(ctx, gk, gv):
        attr, w1tk, b1k, w2k, w1tv, b1v, w2v = ctx.saved_tensors[:7]
        units = [_p(t) for t in ctx.saved_tensors[7:]]
        E, CIN = attr.shape
        lib = _lib.lib()
        bwd, what = (lib.singa_edge_mlp_units_bwd, "singa_edge_mlp_units_bwd") if ctx.units else \
            (lib.singa_edge_mlp_bwd, "singa_edge_mlp_bwd")
        grads = []
        for g, w1t, b1, w2, params in ((gk, w1tk, b1k, w2k, ctx.params[:4]), (gv, w1tv, b1v, w2v, ctx.params[4:])):
            g = g.contiguous()
            H = w2.shape[0]
            row = H * CIN + H + H * H + H                 # [dW1 | db1 | dW2 | db2] in the parameters' layouts (include/singa_hip.h)
            part = torch.empty(lib.singa_edge_mlp_bwd_nparts(E, H), row, device=attr.device, dtype=torch.float32)
            _chk(bwd(_p(attr), *units, _p(g), _p(w1t), _p(b1), _p(w2), _p(part), E, CIN, H, _stream()), what)
            o1, o2, o3 = H * CIN, H * CIN + H, H * CIN + H + H * H
            gs = param_colsum(part, [(0, o1, params[0]), (o1, H, params[1]), (o2, H * H, params[2]), (o3, H, params[3])])
            grads += [gs[0].view(H, CIN) if gs[0] is not None else None, gs[1], gs[2].view(H, H) if gs[2] is not None else None, gs[3]]
        return (None, None, None, *grads)


# k15c once per undirected edge when the caller names the units (`KnnEdges.unit_a / unit_b`); False: every directed row, as
# without units (A/B runs and the tests' comparison of the two)
USE_EDGE_UNITS = True


def edge_mlp_pair(attr, k_net, v_net, units=None):
    """k_net / v_net: (first Linear, second Linear) of `weight_k_net` / `weight_v_net`.  units: (unit_a, unit_b) int32 [E] of
    include/singa_hip_units.h - every row of attr is named once, and a unit's two rows hold the same attributes."""
    unit_a, unit_b = units if units is not None and USE_EDGE_UNITS else (None, None)
    return _EdgeMLPPair.apply(attr, unit_a, unit_b, k_net[0].weight, k_net[0].bias, k_net[1].weight, k_net[1].bias,
                              v_net[0].weight, v_net[0].bias, v_net[1].weight, v_net[1].bias)


def colsum(t):
    """Column sums of a [M, ...] tensor over dim 0 with the library's two-pass kernel.  torch's own long-column
    reductions (bias gradients of Linear layers, broadcast gradients, `t.sum(0)`) go through a multi-block kernel with
    global semaphores that returned garbage (1e12..1e36) for a few outputs per step under HIP-graph replay on this ROCm
    build; this kernel has no cross-launch state and a fixed summation order."""
    if t.shape[0] == 0:                       # nothing to add up (an empty edge / node set)
        return torch.zeros(t.shape[1:], device=t.device, dtype=torch.float32)
    t2 = t.reshape(t.shape[0], -1)
    _dev(t2)
    if t2.stride(1) != 1:
        t2 = t2.contiguous()
    M, n = t2.shape
    lib = _lib.lib()
    work = torch.empty(lib.singa_colsum_work(M, n), device=t.device, dtype=torch.float32)
    out = torch.empty(n, device=t.device, dtype=torch.float32)
    _chk(lib.singa_colsum(_p(t2), t2.stride(0), M, n, _p(work), _p(out), _stream()), "singa_colsum")
    return out.view(t.shape[1:])


class _GradSink:
    """Direct accumulation of parameter gradients (TrainStep turns it on around its backward pass).  A backward function
    whose output is the gradient of a leaf parameter that already owns a `.grad` buffer does not return it to autograd
    (which would launch one AccumulateGrad add per parameter on top of the reduction that produced it): column-sum
    reductions are queued and run as ONE multi-job launch pair that adds into the `.grad` buffers
    (singa_colsum_multi), GEMM-shaped weight gradients accumulate in the GEMM itself (beta = 1).  `flush()` must run after
    the backward pass and before anything reads the gradients.  Off (the default): every backward returns its gradients."""
    on = False
    found = None       # a dict while the engine records which parameters are produced by sink-aware backward functions
    jobs = []          # (src [M, n] kept alive until the flush, [(col0, flat .grad view)])
    @staticmethod
    def takes(*params):
        """True when every given parameter can receive its gradient directly."""
        if _GradSink.found is not None:
            for p in params:
                if p is not None and p.is_leaf and p.requires_grad:
                    _GradSink.found[id(p)] = p
        if not _GradSink.on:
            return False
        for p in params:
            if p is None or not (p.is_leaf and p.requires_grad) or p.grad is None or not p.grad.is_contiguous():
                return False
        return True

    @staticmethod
    def flush():
        jobs, _GradSink.jobs = _GradSink.jobs, []
        jobs = [j for j in jobs if j[0].shape[0] > 0 and j[0].shape[1] > 0]
        if not jobs:
            return
        # jobs of one call run concurrently, so two jobs that add into the same buffer (a parameter used several times
        # per forward pass) go to different rounds, in queue order: a fixed summation order, no atomics
        seen, rounds = {}, []
        for job in jobs:
            r = max(seen.get(g.data_ptr(), 0) for _, g in job[1])
            for _, g in job[1]:
                seen[g.data_ptr()] = r + 1
            while len(rounds) <= r:
                rounds.append([])
            rounds[r].append(job)
        lib = _lib.lib()
        for jobs in rounds:
            nj = len(jobs)
            ns = sum(len(j[1]) for j in jobs)
            xs, lds, Ms, ns_ = ((ctypes.c_void_p * nj)(), (ctypes.c_longlong * nj)(), (ctypes.c_longlong * nj)(),
                                (ctypes.c_int * nj)())
            seg0, col0, dst = (ctypes.c_int * nj)(), (ctypes.c_int * ns)(), (ctypes.c_void_p * ns)()
            q = total = 0
            for k, (src, segs) in enumerate(jobs):
                xs[k], lds[k], Ms[k], ns_[k], seg0[k] = src.data_ptr(), src.stride(0), src.shape[0], src.shape[1], q
                total += lib.singa_colsum_multi_work(src.shape[0], src.shape[1])
                for c0, g in segs:
                    col0[q], dst[q] = c0, g.data_ptr()
                    q += 1
            work = torch.empty(max(total, 1), device=jobs[0][0].device, dtype=torch.float32)
            _chk(lib.singa_colsum_multi(nj, xs, lds, Ms, ns_, seg0, ns, col0, dst, _p(work), total, _stream()),
                 "singa_colsum_multi")


def param_colsum(src, targets):
    """Column sums of src [M, n] split over parameters: targets = [(col0, ncols, param)] covering 0..n in order.  Returns
    one gradient per target - None where the sum was queued to be added straight into param.grad (_GradSink).  Runs of
    neighbouring targets of the same kind share one job / one immediate reduction."""
    src = src.reshape(src.shape[0], math.prod(src.shape[1:]))
    if src.stride(1) != 1:
        src = src.contiguous()
    direct = [src.shape[0] > 0 and _GradSink.takes(t[2]) for t in targets]
    out = [None] * len(targets)
    i = 0
    while i < len(targets):
        j = i
        while j + 1 < len(targets) and direct[j + 1] == direct[i]:
            j += 1
        c0, c1 = targets[i][0], targets[j][0] + targets[j][1]
        blk = src[:, c0:c1]
        if direct[i]:
            _GradSink.jobs.append((blk, [(t[0] - c0, t[2].grad) for t in targets[i:j + 1]]))
        else:
            tot = colsum(blk)
            for k in range(i, j + 1):
                out[k] = tot[targets[k][0] - c0: targets[k][0] - c0 + targets[k][1]]
        i = j + 1
    return out


class _BiasAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b):
        ctx.param = b
        return x + b

    @staticmethod
    def backward(ctx, g):
        n = g.shape[-1]
        return g, param_colsum(g.reshape(-1, n), [(0, n, ctx.param)])[0]


def bias_add(x, b):
    """x[..., n] + b[n] whose bias gradient is a replay-safe column sum."""
    return _BiasAdd.apply(x, b)


class _rocblas:
    """Inside: torch's GEMMs go to rocBLAS (the `cublas` backend) instead of hipBLASLt.  Only the generic dense-attention
    branch (head sizes other than the shipped 32 / 64) still multiplies through the library, see _BmmSmall."""

    def __enter__(self):
        torch.backends.cuda.preferred_blas_library("cublas")

    def __exit__(self, *a):
        torch.backends.cuda.preferred_blas_library("cublaslt")
        return False


class _BmmSmall(torch.autograd.Function):
    """torch.bmm for batches of small matrices (the dense attention of the decoder: 128 batches of 201 x 230 scores with
    32 / 64 channels), forward and both backward products through rocBLAS: hipBLASLt runs one 256x256 tile per batch
    there (QK^T 32 us vs 13 us, dP 40 vs 20, dV 21 vs 12, dK 18 vs 11: tools/lab/bmm_probe.py).  A plain torch.bmm would
    take whatever library is preferred at the time autograd runs its backward."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        with _rocblas():
            return torch.bmm(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        with _rocblas():
            ga = torch.bmm(g, b.transpose(1, 2)) if ctx.needs_input_grad[0] else None
            gb = torch.bmm(a.transpose(1, 2), g) if ctx.needs_input_grad[1] else None
        return ga, gb


def bmm_small(a, b):
    return _BmmSmall.apply(a, b)


# ---------------------------------------------------------------------------------------- k7 / k11: own f32 MFMA GEMM
# The BLAS-library evaluation of the same contractions lives in tests/lib_gemm.py (the tests' second opinion); the product has
# one path.  USE_SKINNY_SO3: the VALU kernels k11s for the 16 <-> 512 / 112 channel SO3 linears (the tests switch it off to
# reach the MFMA kernel's grouped-row problems on those shapes too).
USE_SKINNY_SO3 = True
_GEMM_SPLIT_ROWS = 2048


def _rows(t):
    """A 2-D operand with unit column stride and 16-byte aligned rows (column-block views qualify); a copy otherwise."""
    if t.stride(-1) != 1 or t.stride(0) % 4 or t.data_ptr() % 16:
        t = t.contiguous()
    return t


def _mat(t, what):
    """(pointer, rows, columns, row pitch, rows per group, group pitch) of a GEMM operand given as a view: [rows, cols], or
    [N, n, cols] = N groups of n rows (the 2l+1 coefficient rows of one degree, x[:, l*l:(l+1)**2]).  Raises where the view
    cannot be addressed that way under the float4 rule of include/singa_hip.h: unit column stride, 16-byte aligned base,
    pitches that are multiples of 4 floats."""
    if t.dim() == 2:
        (rows, cols), ld, grp, gld = t.shape, t.stride(0), 0, 0
    elif t.dim() == 3:
        (n, grp, cols), gld, ld = t.shape, t.stride(0), t.stride(1)
        rows = n * grp
    else:
        raise RuntimeError(f"GEMM operand {what}: a 2-D or 3-D view, got {tuple(t.shape)}")
    ptr = t.data_ptr()
    bad = ("the columns are not contiguous" if t.stride(-1) != 1 else "the base is not 16-byte aligned" if ptr % 16 else
           "the pitches are not multiples of 4 floats" if ld % 4 or gld % 4 else None)
    if bad:
        raise RuntimeError(f"GEMM operand {what}, shape {tuple(t.shape)}, strides {t.stride()}, address {ptr:#x}: {bad}")
    return ptr, rows, cols, ld, grp, gld


def _like_c(t, C, what):
    """Pointer of an epilogue operand that the kernel addresses with C's pitches (the pitch of an axis of length 1 is never used)."""
    pitches = all(st == sc for st, sc, n in zip(t.stride(), C.stride(), C.shape) if n > 1)
    if t.shape != C.shape or not pitches or t.data_ptr() % 16:
        raise RuntimeError(f"GEMM {what}: shape {tuple(t.shape)}, strides {t.stride()} must be those of the result "
                         f"({tuple(C.shape)}, {C.stride()}), 16-byte aligned")
    return t.data_ptr()


def _extents(a_rc, b_rc, a, b, c, unit=""):
    """(I, J, R) of c[I, J] = sum_r A(i, r) B(r, j) from the (rows, columns) of A, B and C in the given operand form
    (a_rc: A is [I][R], else [R][I]; b_rc: B is [J][R], else [R][J]) - raises when the three disagree."""
    (I, Ra), (J, Rb) = (a if a_rc else a[::-1]), (b if b_rc else b[::-1])
    if Ra != Rb or c != (I, J):
        raise RuntimeError(f"GEMM form ({int(a_rc)}, {int(b_rc)}): A {a}, B {b} and C {c} (rows, columns{unit}) disagree on I, J, R")
    return I, J, Ra


def _prob(A, B, C, a_rc, b_rc, bias=None, addend=None, mask=None, relu=False, asum=None):
    """One singa_gemm_t record (the dict _gemm takes) from views of the operands: pointers, pitches and row grouping come
    from the views (_mat), I, J, R from their shapes (_extents).  C of the (0, 0) form may be a [S, I, J] view of a slab
    buffer: the dense partial results of S splits, c_split_stride = its stride(0); asum then a [S, I] view of the rows that
    take the column sums of A.  bias [J]; addend / mask: views laid out like C.  Host checks only, no device work."""
    a, ar, ac, lda, ag, agl = _mat(A, "A")
    b, br, bc, ldb, bg, bgl = _mat(B, "B")
    c, cr, cc, ldc, cg, cgl = _mat(C, "C")
    slabs = C.dim() == 3 and not a_rc
    I, J, R = _extents(a_rc, b_rc, (ar, ac), (br, bc), (cg, cc) if slabs else (cr, cc))
    it = dict(a=a, lda=lda, b=b, ldb=ldb, c=c, ldc=ldc, I=I, J=J, R=R)
    if ag:
        it.update(a_group=ag, a_group_ld=agl)
    if bg:
        it.update(b_group=bg, b_group_ld=bgl)
    if slabs:
        if ldc != J or cgl < I * J:
            raise RuntimeError(f"GEMM slabs {tuple(C.shape)}, strides {C.stride()}: dense [I, J] blocks that do not overlap")
        it.update(c_split_stride=cgl)
    elif cg:
        it.update(c_group=cg, c_group_ld=cgl)
    if bias is not None:
        if bias.shape != (J,) or bias.stride(0) != 1 or bias.data_ptr() % 16:
            raise RuntimeError(f"GEMM bias: a contiguous 16-byte aligned [{J}], got {tuple(bias.shape)}")
        it.update(bias=bias.data_ptr())
    if addend is not None:
        it.update(addend=_like_c(addend, C, "addend"))
    if mask is not None:
        it.update(mask=_like_c(mask, C, "mask"))
    if relu:
        it.update(relu=1)
    if asum is not None:
        if (a_rc or ag or asum.dim() != 2 or asum.shape[1] != I or asum.stride(1) != 1
                or (slabs and asum.shape[0] != C.shape[0])):
            raise RuntimeError(f"GEMM asum {tuple(asum.shape)}: one contiguous row of I = {I} floats per split, (0, 0) form, plain A rows")
        it.update(asum=asum.data_ptr(), asum_stride=asum.stride(0))
    return it


def _cprob(A, B, C, a_rc, b_rc, sigma):
    """One singa_cgemm_t record (the dict _cgemm takes).  A, B, C: (real part, imaginary part) pairs of views - the caller
    names the layout by how it halves the stored matrix: `X.chunk(2, 1)` for [x_+ | x_-] column halves, `w.chunk(2, 0)` for
    [Wr; Wi] row halves.  a_im / b_im / c_im are the distances between the two parts; I, J, R count complex elements.  C of
    the (0, 0) form may be a pair of [S, I, J] slab views as in _prob."""
    parts = []
    for (re, im), what in zip((A, B, C), "ABC"):
        ptr, rows, cols, ld, grp, gld = _mat(re, what)
        off = im.data_ptr() - ptr
        if im.shape != re.shape or im.stride() != re.stride() or off % 16:
            raise RuntimeError(f"complex GEMM operand {what}: the imaginary part {tuple(im.shape)}, strides {im.stride()} must be "
                             f"laid out like the real part {tuple(re.shape)}, {re.stride()}, a multiple of 4 floats away")
        parts.append((ptr, rows, cols, ld, grp, gld, off // 4))
    (a, ar, ac, lda, ag, _, a_im), (b, br, bc, ldb, bg, _, b_im), (c, cr, cc, ldc, cg, cgl, c_im) = parts
    slabs = cg > 0 and not a_rc
    if ag or bg or (cg and not slabs):
        raise RuntimeError("complex GEMM: plain rows only (no grouped operands)")
    I, J, R = _extents(a_rc, b_rc, (ar, ac), (br, bc), (cg, cc) if slabs else (cr, cc), ", complex")
    it = dict(a=a, lda=lda, a_im=a_im, b=b, ldb=ldb, b_im=b_im, c=c, ldc=ldc, c_im=c_im, I=I, J=J, R=R, sigma=sigma)
    if slabs:
        it.update(c_split_stride=cgl)
    return it


# precision -> entry point of the real GEMM.  "bf16" (include/singa_hip_bf16.h): the operands are rounded to bfloat16 inside
# the kernel, products and sums stay f32; tensors in memory are f32 either way.  The autograd functions below that take a
# `precision` keep it on ctx: backward runs on autograd's thread, where a switch set around the forward call is not seen, and
# the input- and weight-gradient launches have to follow the forward's.  No (operand form, tile shape) class is sent back to
# f32 under "bf16": each of the nine classes a config-3 step launches under the flag takes less time per step in the bf16 kernel
# (bf16 / f32 0.27 - 0.94 per class, profiles/bf16/README.md; the 32 x 128 tile is launched by the embedding only).
_GEMM_ENTRY = {"f32": "singa_gemm_f32", "bf16": "singa_gemm_bf16"}


def check_precision(precision):
    if precision not in _GEMM_ENTRY:
        raise ValueError(f"precision must be one of {sorted(_GEMM_ENTRY)}, got {precision!r}")
    return precision


def _gemm(items, a_rc, b_rc, splits=1, precision="f32"):
    """The one place that picks the real GEMM's entry point."""
    name = _GEMM_ENTRY[check_precision(precision)]
    arr, n = _capi.gemm_probs(items)
    _chk(getattr(_lib.lib(), name)(arr, n, int(a_rc), int(b_rc), int(splits), _stream()), name)


# precision -> entry point of the complex GEMM (the m > 0 blocks of an SO(2) convolution).  "bf16" is singa_cgemm_bf16
# (include/singa_hip_bf16.h): rounded operands, four real products, f32 sums.  No operand-form class is sent back to f32: each
# of the three takes less time per config-3 step in the bf16 kernel (bf16 / f32 0.40 / 0.38 / 0.30 for forward / dX / dW, 0.26 - 0.53
# per launch, profiles/bf16_embed/README.md), and so do the convolutions' m = 0 launches in ops._gemm (0.31 - 0.52).
_CGEMM_ENTRY = {"f32": "singa_cgemm3m_f32", "bf16": "singa_cgemm_bf16"}


def _cgemm(items, a_rc, b_rc, splits=1, precision="f32"):
    """The one place that picks the complex GEMM's entry point."""
    name = _CGEMM_ENTRY[check_precision(precision)]
    arr, n = _capi.gemm_probs(items, _capi.CGemm)
    _chk(getattr(_lib.lib(), name)(arr, n, int(a_rc), int(b_rc), int(splits), _stream()), name)


def _splits_for(rows, tiles=None):
    """Split count of a weight-gradient launch over `rows` rows: one split per _GEMM_SPLIT_ROWS rows.  With `tiles` (128 x 128
    output tiles of all problems) given and only 2-8 rounds of workgroups over the 256 CUs, the count is moved (up to 2x,
    at least 512 rows per split) to the one whose last round is fullest: 117 tiles x 9 splits = 4.11 rounds run as 5
    (656 us for the 16.5 k-edge shard of config 4, 566 us with 13 splits = 5.94 rounds; tools/lab/conv_split_probe.py)."""
    base = max(1, min(64, -(-rows // _GEMM_SPLIT_ROWS)))
    if not tiles or not 512 <= tiles * base < 2048:
        return base
    best, best_fill = base, 0.0
    for S in range(base, max(base, min(64, rows // 512, 2 * base)) + 1):
        w = tiles * S
        fill = w / (-(-w // 256) * 256)
        if fill > best_fill + 0.02:
            best, best_fill = S, fill
    return best


def _splits_few(rows, tiles):
    """Split count of a weight-gradient launch with FEW output tiles (an SO(2) convolution's m = 0 block alone, or its two
    complex blocks: 10-50 tiles).  Model: the launch runs in rounds of 512 workgroups (two per CU), a workgroup costs its
    rows / S reduction rows plus ~64 rows' worth of prologue and epilogue; the cheapest S of 1..64 with at least 128 rows per
    split (50 tiles x 11 splits = 1.07 rounds ran as two: 393 us for the 13 k-edge shard's conv2, tools/lab/cgemm_probe.py)."""
    best, best_cost = 1, None
    for S in range(1, max(1, min(64, rows // 128)) + 1):
        cost = -(-tiles * S // 512) * (-(-rows // S) + 64)
        if best_cost is None or cost < best_cost:
            best, best_cost = S, cost
    return best


def _dw_grads(probs, splits, cplx=False, precision="f32"):
    """The weight gradients of ONE split-reduction launch.  probs: [(A, B, weight parameter, bias parameter or None)] - the
    (0, 0)-form products dW = A^T B over the rows of the views A [rows, out] and B [rows, in] (grouped rows allowed), whose
    result is (a part of) the parameter in the parameter's own layout; problems in a row that name the same parameter fill it
    front to back.  A bias parameter takes the column sums of A from the same launch (asum).  cplx: A = [g_r | g_i], B =
    [x_+ | x_-] column halves, the result an fc weight [Wr; Wi] (the complex GEMM, no bias).  precision: of either launch.  The partial slabs of all
    problems, then the asum rows, are the columns of one [splits, row] buffer that param_colsum adds up.
    -> ([gradient per distinct weight parameter, shaped like it], [gradient per bias parameter]): None where the sum was
    queued into .grad (_GradSink), zeros when there are no rows to reduce over."""
    dims = [(A.shape[-1], B.shape[-1] // 2 if cplx else B.shape[-1]) for A, B, _, _ in probs]
    sizes = [i * j for i, j in dims] + [i for (i, _), p in zip(dims, probs) if p[3] is not None]
    targets, off = [], 0                   # (first column, columns, parameter) in the buffer's order
    for sz, (_, _, w, _) in zip(sizes, probs):
        if targets and targets[-1][2] is w:
            targets[-1] = (targets[-1][0], targets[-1][1] + sz, w)
        else:
            targets.append((off, sz, w))
        off += sz
    nw = len(targets)
    for sz, bias in zip(sizes[len(probs):], [p[3] for p in probs if p[3] is not None]):
        targets.append((off, sz, bias))
        off += sz
    A0 = probs[0][0]
    if A0.numel() == 0:
        res = [torch.zeros(n, device=A0.device, dtype=torch.float32) for _, n, _ in targets]
    else:
        part = torch.empty(splits, off, device=A0.device, dtype=torch.float32)
        blocks = part.split(sizes, 1)
        asums = iter(blocks[len(probs):])
        items = []
        for (A, B, _, bias), (i, j), blk in zip(probs, dims, blocks):
            slab = blk.as_strided((splits, i, j), (off, j, 1))      # (unflatten would make up a pitch for a single split)
            if cplx:
                items.append(_cprob(A.chunk(2, 1), B.chunk(2, 1), slab.chunk(2, 1), False, False, -1.0))
            else:
                items.append(_prob(A, B, slab, False, False, asum=next(asums) if bias is not None else None))
        (_cgemm if cplx else _gemm)(items, False, False, splits, precision)
        res = param_colsum(part, targets)
    return [g.view(p.shape) if g is not None else None for g, (_, _, p) in zip(res[:nw], targets)], res[nw:]


def _rows_gemm(x, w, b_rc, precision, bias=None, addend=None, relu=False, out=None):
    """One launch of y = x w^T (b_rc: w is [N, K]) or y = x w (w [K, N]) over the rows of x [..., K], with the epilogue options of
    _prob; addend: shaped like y up to the flattening of its rows; out: the [M, N] tensor to write instead of a fresh one.
    -> (x2, w2, y): x as [M, K] rows and the weight w2, both as the launch read them (copies where _rows had to make one: what
    a backward pass saves), and the result y [M, N]."""
    x2, w2 = _rows(x.reshape(-1, x.shape[-1])), _rows(w)
    _dev(x2, w2, bias)
    M, N = x2.shape[0], w2.shape[0 if b_rc else 1]
    y = torch.empty(M, N, device=x2.device, dtype=torch.float32) if out is None else out
    if addend is not None:
        addend = addend.reshape(M, N).contiguous()
        _dev(addend)
    _gemm([_prob(x2, w2, y, True, b_rc, bias=bias, addend=addend, relu=relu)], True, b_rc, precision=precision)
    return x2, w2, y


def _rows_gemm_dx(g2, w2, b_rc, precision, mask=None):
    """The input gradient of a _rows_gemm as one launch, g2 w2 (w2 [N, K]) or g2 w2^T (b_rc: w2 [K, N]) for the output gradient's
    rows g2 [M, N] and the weight as forward read it; mask [M, K]: the output of the ReLU that produced the forward's x - the
    result is zeroed where it is not positive.  -> [M, K]."""
    gx = torch.empty(g2.shape[0], w2.shape[0 if b_rc else 1], device=g2.device, dtype=torch.float32)
    _gemm([_prob(g2, w2, gx, True, b_rc, mask=mask)], True, b_rc, precision=precision)
    return gx


def gemm_nt(x, w, bias=None, out=None, precision="f32"):
    """y = x w^T (+ bias) on the library's own MFMA kernel; x [M, K] (row-strided views allowed), w [N, K]."""
    return _rows_gemm(x, w, True, precision, bias=bias, out=out)[2]


class _SO2Linear3(torch.autograd.Function):
    """The three contractions of one SO(2) convolution (m = 0 with bias, m = 1, m = 2; EF:807-875 with the +-m
    recombination folded into the block weights) on column blocks of ONE m-primary edge matrix X [E, n0+n1+n2]: one launch
    of the library's f32 MFMA GEMM (k7) forward, one for dX (written straight into the column blocks of one buffer), one
    split-reduction launch + one column sum for the three weight gradients.  The results are column blocks of one
    [E, o0+o1+o2] buffer; their consumers take (pointer, row pitch) pairs."""

    @staticmethod
    def forward(ctx, X, w0, b0, w1, w2, n0, n1):
        ctx.params = (w0, w1, w2, b0)
        X = _rows(X)
        ws = [_rows(w0), _rows(w1), _rows(w2)]
        b0 = b0.contiguous()
        _dev(X, *ws, b0)
        E, nin = X.shape
        ins = (n0, n1, nin - n0 - n1)
        outs = tuple(w.shape[0] for w in ws)
        assert all(w.shape[1] == k for w, k in zip(ws, ins))
        H = torch.empty(E, sum(outs), device=X.device, dtype=torch.float32)
        hs = H.split(outs, 1)
        if E > 0:
            _gemm([_prob(x, w, h, True, True, bias=b) for x, w, h, b in zip(X.split(ins, 1), ws, hs, (b0, None, None))],
                  True, True)
        ctx.save_for_backward(X, *ws)
        ctx.ins = ins
        return hs

    @staticmethod
    def backward(ctx, g0, g1, g2):
        X, *ws = ctx.saved_tensors
        ins, outs = ctx.ins, tuple(w.shape[0] for w in ws)
        E = X.shape[0]
        gs = [_rows(g) for g in (g0, g1, g2)]
        xs = X.split(ins, 1)
        gX = None
        if ctx.needs_input_grad[0]:
            gX = torch.empty_like(X)
            if E > 0:                                       # dX_blk = g_blk @ w_blk: A = g [E, o] (RC), B = w [o, k] ([R][J])
                _gemm([_prob(g, w, gx, True, False) for g, w, gx in zip(gs, ws, gX.split(ins, 1))], True, False)
        # dW_blk = g_blk^T X_blk: reduction over the edges, split over workgroups into dense partial slabs; the m = 0 bias
        # gradient (column sums of g0) is taken inside the same launch
        S = _splits_for(E, sum(-(-o // 128) * -(-k // 128) for o, k in zip(outs, ins)))
        pw0, pw1, pw2, pb0 = ctx.params
        gws, (gb,) = _dw_grads([(gs[0], xs[0], pw0, pb0), (gs[1], xs[1], pw1, None), (gs[2], xs[2], pw2, None)], S)
        return gX, gws[0], gb, gws[1], gws[2], None, None


class _SO2Conv3M(torch.autograd.Function):
    """One SO(2) convolution (EF:807-875) on the m-primary edge matrix X [E, n0 + n1 + n2], the m = 1, 2 blocks as COMPLEX
    products in three real multiplications (k7c, `singa_cgemm3m_f32`) on the modules' own fc weights [2N, K] (Wr = w[:N],
    Wi = w[N:]; no block weight is built), the m = 0 block on the real GEMM (k7): two launches forward, two for dX, two
    split reductions + one column sum for the weight gradients, which arrive in the parameters' own layout.  Under
    precision "bf16" all six launches take the bf16 entry points (singa_gemm_bf16, singa_cgemm_bf16); the m = 0 bias gradient
    still comes from the unrounded column sums."""

    @staticmethod
    def forward(ctx, X, w0, b0, w1, w2, n0, n1, precision):
        ctx.params = (w0, w1, w2, b0)
        ctx.precision = check_precision(precision)
        X, ws, ctx.ins, hs = _so2_conv3m_fwd(X, w0, b0, w1, w2, n0, n1, precision)
        ctx.save_for_backward(X, *ws)
        return hs

    @staticmethod
    def backward(ctx, g0, g1, g2):
        X, *ws = ctx.saved_tensors
        gX, gw0, gb, gw1, gw2 = _so2_conv3m_bwd(X, ws, ctx.ins, ctx.params, (g0, g1, g2), ctx.needs_input_grad[0], ctx.precision)
        return gX, gw0, gb, gw1, gw2, None, None, None


def _so2_conv3m_fwd(X, w0, b0, w1, w2, n0, n1, precision):
    """The forward launches of _SO2Conv3M -> (X and the three weights as the launches read them, the input widths, the outputs)."""
    X = _rows(X)
    ws = [_rows(w0), w1.contiguous(), w2.contiguous()]
    b0 = b0.contiguous()
    _dev(X, *ws, b0)
    E, nin = X.shape
    ins = (n0, n1, nin - n0 - n1)
    outs = tuple(w.shape[0] for w in ws)
    assert ws[0].shape[1] == n0 and all(2 * w.shape[1] == k and w.shape[0] % 2 == 0 for w, k in zip(ws[1:], ins[1:]))
    H = torch.empty(E, sum(outs), device=X.device, dtype=torch.float32)
    xs, hs = X.split(ins, 1), H.split(outs, 1)
    if E > 0:
        _gemm([_prob(xs[0], ws[0], hs[0], True, True, bias=b0)], True, True, precision=precision)
        # A = [x_+ | x_-], B = fc.weight [Wr; Wi], C = [out_r | out_i]
        _cgemm([_cprob(x.chunk(2, 1), w.chunk(2, 0), h.chunk(2, 1), True, True, 1.0)
                for x, w, h in zip(xs[1:], ws[1:], hs[1:])], True, True, precision=precision)
    return X, ws, ins, hs


def _so2_conv3m_bwd(X, ws, ins, params, gs, need_gx, precision):
    """The backward launches of _SO2Conv3M -> the gradients of (X, w0, b0, w1, w2); params = (w0, w1, w2, b0) as the caller was
    given them (the targets of direct accumulation, _GradSink)."""
    outs = tuple(w.shape[0] for w in ws)
    E = X.shape[0]
    gs = [_rows(g) for g in gs]
    xs = X.split(ins, 1)
    # weight gradients: reductions over the edges, split over workgroups into dense partial slabs (the fc weights' layouts).
    # The two launches have few tiles each (conv1: 16 and 14): each gets the split count that fills the CUs.  They are
    # issued in front of the input-gradient launches: nothing in the backward pass waits for them
    S0 = _splits_few(E, -(-outs[0] // 128) * -(-ins[0] // 128))
    Sc = _splits_few(E, sum(-(-(o // 2) // 128) * -(-(k // 2) // 64) for o, k in zip(outs[1:], ins[1:])))
    pw0, pw1, pw2, pb0 = params
    (gw0,), (gb,) = _dw_grads([(gs[0], xs[0], pw0, pb0)], S0, precision=precision)
    (gw1, gw2), _ = _dw_grads([(gs[1], xs[1], pw1, None), (gs[2], xs[2], pw2, None)], Sc, cplx=True, precision=precision)
    gX = None
    if need_gx:
        gX = torch.empty_like(X)
        if E > 0:
            gxs = gX.split(ins, 1)
            _gemm([_prob(gs[0], ws[0], gxs[0], True, False)], True, False, precision=precision)
            # A = [g_r | g_i], B = fc.weight [Wr; Wi] as [r = n][j = k], C = [dx_+ | dx_-]
            _cgemm([_cprob(g.chunk(2, 1), w.chunk(2, 0), gx.chunk(2, 1), True, False, -1.0)
                    for g, w, gx in zip(gs[1:], ws[1:], gxs[1:])], True, False, precision=precision)
    return gX, gw0, gb, gw1, gw2


def so2_conv3m(X, w0, b0, w1, w2, n0, n1, precision="f32"):
    """The SO(2) convolution on the fc weights themselves (w1, w2: [2N, K] = [Wr; Wi]) - see _SO2Conv3M."""
    return _SO2Conv3M.apply(X, w0, b0, w1, w2, n0, n1, check_precision(precision))


def so2_linear3(X, w0, b0, w1, w2, n0, n1):
    """(X[:, :n0] w0^T + b0, X[:, n0:n0+n1] w1^T, X[:, n0+n1:] w2^T) - see _SO2Linear3."""
    return _SO2Linear3.apply(X, w0, b0, w1, w2, n0, n1)


def _degrees(t, L):
    """The row sets of the degrees 0..L of [N, K, C] coefficient rows: L + 1 views [N, 2l + 1, C] (one split call)."""
    return t.split([2 * l + 1 for l in range(L + 1)], 1)


def _so3_linear_probs(x, weight, out, L, b_rc, bias=None, addend=None):
    """The launch of an SO3_LinearV2 on [N, K, C] rows: one problem per degree l, A = the degree's rows of x (a grouped row
    set), B = weight[l], C = the same rows of out, so that the result is written in place.  b_rc: out = x weight[l]^T (the
    forward product; bias on the l = 0 row, addend a tensor like out), else out = x weight[l] (the input gradient)."""
    if weight.shape[0] != L + 1:
        raise RuntimeError(f"SO3 linear: {weight.shape[0]} weight matrices for the degrees 0..{L}")
    ads = _degrees(addend, L) if addend is not None else [None] * (L + 1)
    return [_prob(a, w, c, True, b_rc, bias=bias if l == 0 else None, addend=ad)
            for l, (a, w, c, ad) in enumerate(zip(_degrees(x, L), weight.unbind(0), _degrees(out, L), ads))]


class _SO3Linear(torch.autograd.Function):
    """SO3_LinearV2 (EF:624-674) on [N, K, C] coefficient rows with the library's f32 MFMA GEMM (k11): one launch with one
    problem per degree l (its 2l+1 rows of every node form a grouped row set, so the [N, K, out] result is written in
    place, bias on the l = 0 row), one launch for dX, one split-reduction launch + column sum for the per-degree weight
    gradients.  No expanded [K, out, in] weight, no transposed copies."""

    @staticmethod
    def forward(ctx, x, weight, bias, L, addend=None):
        ctx.params = (weight, bias)
        x, weight, bias = x.contiguous(), weight.contiguous(), bias.contiguous()
        _dev(x, weight, bias)
        N, K, cin = x.shape
        cout = weight.shape[1]
        out = torch.empty(N, K, cout, device=x.device, dtype=torch.float32)
        ctx.has_addend = addend is not None
        if addend is not None:                    # a residual [N, K, cout] added in the GEMM's epilogue (MFMA path only)
            addend = addend.contiguous()
            _dev(addend)
            assert addend.shape == out.shape and not (USE_SKINNY_SO3 and cin == 16 and cout == 512)
        if USE_SKINNY_SO3 and cin == 16 and cout == 512:
            # k11s: a 16-long contraction - VALU kernel, thread = output channel, whole 2 KB rows per store
            if N > 0:                             # (an empty node set has no address to hand over)
                _chk(_lib.lib().singa_so3_skinny_expand(_p(x), _p(weight), cout * cin, cin, 1, _p(bias), _p(out), N, cout, L,
                                                        _stream()), "singa_so3_skinny_expand")
        elif N > 0:
            _gemm(_so3_linear_probs(x, weight, out, L, True, bias, addend), True, True)
        ctx.save_for_backward(x, weight)
        ctx.L = L
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        gx, gw, gb = _so3_linear_bwd(x, weight, ctx.L, ctx.params, g, ctx.needs_input_grad[0])
        return gx, gw, gb, None, (g if ctx.has_addend else None)


def _so3_linear_bwd(x, weight, L, params, g, need_gx):
    """The backward launches of _SO3Linear for the (contiguous) output gradient g -> the gradients of (x, weight, bias); params =
    (weight, bias) as the caller was given them (the targets of direct accumulation, _GradSink)."""
    N, K, cin = x.shape
    cout = weight.shape[1]
    lib = _lib.lib()
    # (wide, 16) pairs the VALU kernels are built for: the feed-forward block's 512 and the output projection's 112
    skinny = USE_SKINNY_SO3 and N > 0 and ((cin == 16 and cout == 512) or (cin in (512, 112) and cout == 16))
    wide = max(cin, cout)
    gx = None
    if need_gx:
        gx = torch.empty_like(x)
        if skinny and cout == 16:
            # k11s: d x = g expanded through weight[l][u][c] - again a 16-long contraction
            _chk(lib.singa_so3_skinny_expand(_p(g), _p(weight), cout * cin, 1, cin, None, _p(gx), N, wide, L, _stream()),
                 "singa_so3_skinny_expand(dx)")
        elif N > 0:
            _gemm(_so3_linear_probs(g, weight, gx, L, False), True, False)
    if skinny:
        # k11s: the weight gradient as a VALU reduction over whole 2 KB rows of the 512-channel tensor (16 -> 512:
        # small = x, big = g, rows [l][c][u] + the bias gradient; 512 -> 16: small = g, big = x, rows [l][u][c])
        wide_out = cout == wide
        wsz = (L + 1) * 16 * wide
        part = torch.empty(lib.singa_so3_skinny_nparts(N, L, wide), wsz + (wide if wide_out else 0), device=x.device,
                           dtype=torch.float32)
        small, big = (x, g) if wide_out else (g, x)
        _chk(lib.singa_so3_skinny_reduce(_p(small), _p(big), _p(part), N, wide, L, int(wide_out), int(wide_out), _stream()),
             "singa_so3_skinny_reduce")
        if wide_out:
            gw, gb = param_colsum(part, [(0, wsz, params[0]), (wsz, wide, params[1])])
        else:
            gw = param_colsum(part, [(0, wsz, params[0])])[0]
            gb = param_colsum(g[:, 0, :], [(0, cout, params[1])])[0]
        return gx, (gw.view(L + 1, cout, cin) if gw is not None else None), gb
    # dW_l = sum over the (node, row) pairs of degree l of g_row^T x_row
    (gw,), _ = _dw_grads([(gl, xl, params[0], None) for gl, xl in zip(_degrees(g, L), _degrees(x, L))],
                         _splits_for(N * (2 * L + 1)))
    return gx, gw, param_colsum(g[:, 0, :], [(0, cout, params[1])])[0]


def so3_linear(x, weight, bias, L, addend=None):
    """SO3_LinearV2 (EF:624-674); `addend` [N, K, out]: a residual added in the same launch (EF:1383-1384, 1405-1406)."""
    return _SO3Linear.apply(x, weight, bias, L, addend)


class _FFNTail(torch.autograd.Function):
    """The back half of the feed-forward block, a = SeparableS2Activation(h, gate) -> SO3_LinearV2(512 -> 16)(a) (+ residual)
    (EF:256-262, 1405-1406), as ONE autograd node, so that the backward pass touches the [N, K, 512] tensors once less: the
    gradient of `a` (the linear's input gradient, a 16-long contraction per row) is formed inside the activation's backward kernel
    (singa_s2act_ffn_bwd) instead of being written by an expand launch and read back.  Forward: the two existing launches."""

    @staticmethod
    def forward(ctx, h, gate, weight, bias, L, addend=None):
        ctx.params = (weight, bias)
        h, gate, weight, bias = h.contiguous(), gate.contiguous(), weight.contiguous(), bias.contiguous()
        _dev(h, gate, weight, bias)
        N, K, cin = h.shape
        cout = weight.shape[1]
        assert cin == 512 and cout == 16 and weight.shape[2] == cin
        a = _s2_fwd_node(h, gate, L)
        out = torch.empty(N, K, cout, device=h.device, dtype=torch.float32)
        ctx.has_addend = addend is not None
        if addend is not None:
            addend = addend.contiguous()
            _dev(addend)
            assert addend.shape == out.shape
        if N > 0:
            _gemm(_so3_linear_probs(a, weight, out, L, True, bias, addend), True, True)
        ctx.save_for_backward(h, gate, a, weight)
        ctx.L = L
        return out

    @staticmethod
    def backward(ctx, g):
        h, gate, a, weight = ctx.saved_tensors
        g = g.contiguous()
        gh, gg, gw, gb = _ffn_tail_bwd(h, gate, a, weight, ctx.L, ctx.params, g)
        return gh, gg, gw, gb, None, (g if ctx.has_addend else None)


def _ffn_tail_bwd(h, gate, a, weight, L, params, g):
    """The backward launches of _FFNTail for the (contiguous) output gradient g -> the gradients of (h, gate, weight, bias);
    params = (weight, bias) as the caller was given them (the targets of direct accumulation, _GradSink)."""
    N, K, cin = h.shape
    cout = weight.shape[1]
    lib = _lib.lib()
    P, Q, _ = _grid_factors(L, L, False, h.device)
    gh, gg = torch.empty_like(h), torch.empty_like(gate)
    if N > 0:
        _chk(lib.singa_s2act_ffn_bwd(_p(h), _p(gate), gate.stride(0), _p(P), _p(Q), _p(g), _p(weight), _p(gh), _p(gg), N, cin, L,
                                     _stream()), "singa_s2act_ffn_bwd")
    # the linear's weight gradient: rows [l][u][c] summed over the nodes (k11s reduce: small = g, big = a)
    wsz = (L + 1) * 16 * cin
    gw = None
    if N > 0:
        part = torch.empty(lib.singa_so3_skinny_nparts(N, L, cin), wsz, device=h.device, dtype=torch.float32)
        _chk(lib.singa_so3_skinny_reduce(_p(g), _p(a), _p(part), N, cin, L, 0, 0, _stream()), "singa_so3_skinny_reduce")
        gw = param_colsum(part, [(0, wsz, params[0])])[0]
    else:
        gw = torch.zeros(wsz, device=h.device, dtype=torch.float32)
    gb = param_colsum(g[:, 0, :], [(0, cout, params[1])])[0]
    return gh, gg, (gw.view(L + 1, cout, cin) if gw is not None else None), gb


def ffn_tail(h, gate, weight, bias, L, addend=None):
    """SO3_LinearV2(512 -> 16)(SeparableS2Activation(h, gate)) (+ addend) - see _FFNTail."""
    return _FFNTail.apply(h, gate, weight, bias, L, addend)


# ---------------------------------------------------------------------------------------------- activation recomputation
# `SINGA(..., recompute=True)`: the two places of the embedding where a step holds large activations for its backward pass that
# are cheap functions of tensors it holds anyway.  Both nodes run the launches of the nodes they stand for, in their order, on
# the same inputs (so their results are bit-identical to the default path's); what they do not save they rebuild at the start
# of their backward pass.
def _ffn_front(x, w1, b1, gate, L):
    """(h, a) of the feed-forward block's front, h = SO3_LinearV2(16 -> 512)(x), a = SeparableS2Activation(h, gate): the k11s
    expand launch of _SO3Linear.forward and the activation launch of _FFNTail.forward, into fresh tensors.  (One fused launch
    that never writes h was built and measured for this place and lost to these two: profiles/recompute/README.md.)"""
    N, K, cin = x.shape
    C = w1.shape[1]
    h = torch.empty(N, K, C, device=x.device, dtype=torch.float32)
    if N > 0:
        _chk(_lib.lib().singa_so3_skinny_expand(_p(x), _p(w1), C * cin, cin, 1, _p(b1), _p(h), N, C, L, _stream()),
             "singa_so3_skinny_expand")
    return h, _s2_fwd_node(h, gate, L)


class _FFNRecompute(torch.autograd.Function):
    """The feed-forward block SO3_LinearV2(16 -> 512) -> SeparableS2Activation -> SO3_LinearV2(512 -> 16) (+ residual) as one
    autograd node that holds neither of its [N, K, 512] tensors: forward = the launches of _SO3Linear.forward and
    _FFNTail.forward (h and a are dropped on return); backward = the first two of them again (_ffn_front), then the launches of
    _FFNTail.backward and of _SO3Linear.backward.  The same kernels on the same inputs in the same order as so3_linear ->
    ffn_tail: bit-identical results."""

    @staticmethod
    def forward(ctx, x, gate, w1, b1, w2, b2, L, addend=None):
        ctx.params = (w1, b1, w2, b2)
        x, gate, w1, b1, w2, b2 = (t.contiguous() for t in (x, gate, w1, b1, w2, b2))
        _dev(x, gate, w1, b1, w2, b2)
        if not USE_SKINNY_SO3 or tuple(w1.shape[1:]) != (512, 16) or tuple(w2.shape[1:]) != (16, 512) or x.shape[2] != 16:
            raise RuntimeError("ffn_recompute: built for the skinny 16 -> 512 -> 16 feed-forward block (ffn_hidden_channels = 512)")
        h, a = _ffn_front(x, w1, b1, gate, L)
        del h
        out = torch.empty(x.shape[0], x.shape[1], 16, device=x.device, dtype=torch.float32)
        ctx.has_addend = addend is not None
        if addend is not None:
            addend = addend.contiguous()
            _dev(addend)
            assert addend.shape == out.shape
        if x.shape[0] > 0:
            _gemm(_so3_linear_probs(a, w2, out, L, True, b2, addend), True, True)
        ctx.save_for_backward(x, gate, w1, b1, w2)
        ctx.L = L
        return out

    @staticmethod
    def backward(ctx, g):
        x, gate, w1, b1, w2 = ctx.saved_tensors
        pw1, pb1, pw2, pb2 = ctx.params
        g = g.contiguous()
        h, a = _ffn_front(x, w1, b1, gate, ctx.L)
        gh, gg, gw2, gb2 = _ffn_tail_bwd(h, gate, a, w2, ctx.L, (pw2, pb2), g)
        del h, a
        gx, gw1, gb1 = _so3_linear_bwd(x, w1, ctx.L, (pw1, pb1), gh, ctx.needs_input_grad[0])
        return gx, gg, gw1, gb1, gw2, gb2, None, (g if ctx.has_addend else None)


def ffn_recompute(x, gate, w1, b1, w2, b2, L, addend=None):
    """so3_linear(x, w1, b1) -> ffn_tail(., gate, w2, b2, addend) without saved [N, K, 512] tensors - see _FFNRecompute."""
    return _FFNRecompute.apply(x, gate, w1, b1, w2, b2, L, addend)


class _EdgeHeadConvRecompute(torch.autograd.Function):
    """edge_head followed by the second SO(2) convolution (so2_conv3m) as one autograd node that does not hold the activated
    tensor `act` [E, KR*C] between them: its backward pass rebuilds it from h0, h1, h2 (held anyway) with the activation's
    forward launch, then runs the launches of _SO2Conv3M.backward and of _EdgeHead.backward.  -> (logits, y0, y1, y2)."""

    @staticmethod
    def forward(ctx, h0, h1, h2, ln_w, ln_b, dot, w0, b0, w1, w2, heads, A, C, L, M, eps, precision):
        ctx.head_params, ctx.conv_params = (ln_w, ln_b, dot), (w0, w1, w2, b0)
        ctx.cfg = (heads, A, C, L, M, eps)
        ctx.precision = check_precision(precision)          # of the convolution's launches, forward and backward
        saved, logits, act = _edge_head_fwd(h0, h1, h2, ln_w, ln_b, dot, ctx.cfg)
        st = so3.layout(L, M).seg_start
        _, ws, ctx.ins, hs = _so2_conv3m_fwd(act, w0, b0, w1, w2, st[1] * C, (st[2] - st[1]) * C, precision)
        ctx.save_for_backward(*saved, *ws)
        return (logits,) + tuple(hs)

    @staticmethod
    def backward(ctx, g_logits, g0, g1, g2):
        *head, w0, w1, w2 = ctx.saved_tensors
        h0, h1, h2 = head[:3]
        act = _edge_act(h0, h1, h2, ctx.cfg)
        g_act, gw0, gb0, gw1, gw2 = _so2_conv3m_bwd(act, [w0, w1, w2], ctx.ins, ctx.conv_params, (g0, g1, g2), True,
                                                    ctx.precision)
        del act
        return _edge_head_bwd(head, ctx.cfg, ctx.head_params, g_logits, g_act) + (gw0, gb0, gw1, gw2) + (None,) * 7


def edge_head_conv_recompute(h0, h1, h2, ln_w, ln_b, alpha_dot, w0, b0, w1, w2, heads, A, C, L, M=2, eps=1e-5, precision="f32"):
    """edge_head(...) -> so2_conv3m(act, w0, b0, w1, w2, ..., precision) without a saved `act` - see _EdgeHeadConvRecompute."""
    return _EdgeHeadConvRecompute.apply(h0, h1, h2, ln_w, ln_b, alpha_dot, w0, b0, w1, w2, heads, A, C, L, M, eps,
                                        check_precision(precision))


class _GroupedLinear3(torch.autograd.Function):
    """The three grouped 1x1 Conv1d layers of the graph attention (k_lin, q_lin, v_lin: CP:27-29, 55-57) on the SAME node
    rows h [N, heads * ig] as ONE launch of the own MFMA GEMM (k7) with one problem per (layer, head) - h's column block
    of the head times that head's [og, ig] weight block into the head's column block of the layer's output - instead of
    three batched library GEMMs; backward: the three input-gradient contributions as three chained launches (each adds the
    previous one's result in its epilogue: no separate additions) and one split-reduction launch for all weight gradients."""

    @staticmethod
    def forward(ctx, h, wk, wq, wv, heads, precision):
        ctx.params = (wk, wq, wv)
        ctx.precision = check_precision(precision)
        h = _rows(h)
        ws = [_rows(w.view(w.shape[0], w.shape[1])) for w in (wk, wq, wv)]       # [heads * og, ig] (the Conv1d weight as it is)
        _dev(h, *ws)
        N, ig = h.shape[0], ws[0].shape[1]
        ogs = [w.shape[0] // heads for w in ws]
        outs = [torch.empty(N, heads, og, device=h.device, dtype=torch.float32) for og in ogs]
        if N > 0:
            hs = h.split(ig, 1)                                      # the heads' column blocks of h, row blocks of a weight
            _gemm([_prob(hh, wh, oh, True, True) for w, o, og in zip(ws, outs, ogs)
                   for hh, wh, oh in zip(hs, w.split(og, 0), o.unbind(1))], True, True, precision=precision)
        ctx.save_for_backward(h, *ws)
        ctx.heads, ctx.ogs = heads, ogs
        return tuple(outs)

    @staticmethod
    def backward(ctx, gk, gq, gv):
        h, *ws = ctx.saved_tensors
        heads, ogs = ctx.heads, ctx.ogs
        N, ig = h.shape[0], ws[0].shape[1]
        gs = [_rows(g.reshape(N, heads * og)) for g, og in zip((gk, gq, gv), ogs)]
        gh = None
        if ctx.needs_input_grad[0] and N > 0:
            prev = [None] * heads
            for g, w, og in zip(gs, ws, ogs):                        # dh += g_layer W_layer, head by head; chained through `addend`
                gh = torch.empty(N, heads * ig, device=h.device, dtype=torch.float32)
                cur = gh.split(ig, 1)
                _gemm([_prob(gg, wh, c, True, False, addend=ad)
                       for gg, wh, c, ad in zip(g.split(og, 1), w.split(og, 0), cur, prev)], True, False,
                      precision=ctx.precision)
                prev = cur
        elif ctx.needs_input_grad[0]:
            gh = torch.zeros_like(h)
        hs = h.split(ig, 1)                                          # dW[layer][head] [og, ig] = g_head^T h_head
        gws, _ = _dw_grads([(gg, hh, p, None) for g, og, p in zip(gs, ogs, ctx.params) for gg, hh in zip(g.split(og, 1), hs)],
                           _tn_splits(N, max(ogs), ig), precision=ctx.precision)
        return gh, gws[0], gws[1], gws[2], None, None


def grouped_linear3(h, wk, wq, wv, heads, precision="f32"):
    """(k_lin(h), q_lin(h), v_lin(h)) for grouped 1x1 Conv1d weights [heads * og, ig, 1] -> three [N, heads, og] tensors."""
    ig = wk.shape[1]
    ok = (h.is_cuda and ig % 4 == 0 and all((w.shape[0] // heads) % 4 == 0 and w.shape[1] == ig for w in (wk, wq, wv))
          and 3 * heads <= 12)
    if not ok:
        raise ValueError("grouped_linear3: channel counts per head must be multiples of 4 and heads <= 4 (the own GEMM's "
                         "float4 accesses, 12 problems per launch)")
    return _GroupedLinear3.apply(h, wk, wq, wv, heads, precision)


def _tn_splits(rows, out, cin):
    """Split count of a weight-gradient GEMM dW[out, cin] = g^T x over `rows` rows (tools/lab/tn_split_probe.py): at most
    4,096 rows per split; else enough workgroups to fill the chip (~512 tiles in all) but no more than 64 splits for outputs
    of 128 x 128 and up - every split writes a partial slab - and proportionally more for smaller ones; at least 256 rows
    per split.  (A flat cap of 64 used to sit on top: the gradient of a 20 -> 64 Linear over the 2.9 M kNN edges ran as 64
    workgroups of 45 k rows, 1.6 ms instead of 0.3; a 32 -> 128 one over 186 k rows 101 us instead of 34.)"""
    tiles = -(-out // 128) * -(-cin // 128)
    fill = min(-(-512 // tiles), 64 * max(1, 16384 // max(1, out * cin)))
    return max(1, min(1024, max(-(-rows // 4096), fill), rows // 256))


def _own_linear_ok(x, w):
    K = x.shape[-1]
    N = w.shape[0]
    return x.is_cuda and x.dtype == torch.float32 and K % 4 == 0 and N % 4 == 0 and x.numel() > 0


class _LinearOwn(torch.autograd.Function):
    """nn.Linear / 1x1 Conv1d on rows (CP:55-61, 96-117, 161-191) on the library's own f32 MFMA GEMM (k7): y = x W^T + b
    (+ addend, a tensor shaped like y: the sum of two Linears' outputs costs no extra pass) in ONE launch, dX one launch,
    dW one split-reduction launch whose partial slabs - like the bias gradient - are added up by the step's shared
    column-sum launch (ops._GradSink)."""

    @staticmethod
    def forward(ctx, x, w, b, addend, precision):
        ctx.params = (w, b)
        ctx.precision = check_precision(precision)
        K, N = x.shape[-1], w.shape[0]
        x2, w2, y = _rows_gemm(x, w.view(N, K), True, precision, bias=b, addend=addend)
        ctx.save_for_backward(x2, w2)
        ctx.xshape, ctx.has_bias, ctx.ashape = x.shape, b is not None, (addend.shape if addend is not None else None)
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, g):
        x2, w2 = ctx.saved_tensors
        M, N = x2.shape[0], w2.shape[0]
        g2 = _rows(g.reshape(-1, N))
        wp, bp = ctx.params
        gx = gw = gb = None
        # the weight gradient first: nothing in the backward pass waits for it, the input gradient's launch follows it
        if ctx.needs_input_grad[1] and ctx.has_bias and ctx.needs_input_grad[2] and M > 0:
            gw, gb = _tn_grad(g2, x2, wp, bp, ctx.precision)          # the bias gradient rides in the weight gradient's launch
        else:
            if ctx.needs_input_grad[1]:
                gw = _tn_grad(g2, x2, wp, precision=ctx.precision)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb = param_colsum(g2, [(0, N, bp)])[0]
        if ctx.needs_input_grad[0]:
            gx = _rows_gemm_dx(g2, w2, False, ctx.precision).view(ctx.xshape)
        ga = g.reshape(ctx.ashape) if ctx.ashape is not None and ctx.needs_input_grad[3] else None
        return gx, gw, gb, ga, None


class _LinearNN(torch.autograd.Function):
    """y = x W for a parameter W [K, N] used untransposed (the hoisted `weight_k_lin` of the graph attention: (q W), CP:61
    with W(w*k) moved to the query side) - the (1, 0) form of the own GEMM, no transposed copy of W."""

    @staticmethod
    def forward(ctx, x, w, precision):
        ctx.param = w
        ctx.precision = check_precision(precision)
        x2, w2, y = _rows_gemm(x, w, False, precision)
        ctx.save_for_backward(x2, w2)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], w.shape[1])

    @staticmethod
    def backward(ctx, g):
        x2, w2 = ctx.saved_tensors
        g2 = _rows(g.reshape(-1, w2.shape[1]))
        gx = gw = None
        if ctx.needs_input_grad[0]:                  # dx = g W^T: W [K, N] is the [J][R] operand of the (1, 1) form
            gx = _rows_gemm_dx(g2, w2, True, ctx.precision).view(ctx.xshape)
        if ctx.needs_input_grad[1]:                  # dW [K, N] = x^T g
            gw = _tn_grad(x2, g2, ctx.param, precision=ctx.precision)
        return gx, gw, None


def linear_nn(x, w, precision="f32"):
    if x.is_cuda and w.shape[0] % 4 == 0 and w.shape[1] % 4 == 0 and x.numel() > 0:
        return _LinearNN.apply(x, w, precision)
    return linear(x, w.t(), precision=precision)


def _tn_grad(g2, x2, param, bias=None, precision="f32"):
    """dW[N, K] = g2^T x2 (reduction over the rows, split over workgroups): the one-problem case of _dw_grads.  Returns the
    gradient shaped like `param`, or None when it was queued into param.grad - and, with `bias`, the bias gradient (the
    per-split column sums of g ride behind the slab) as a second result.  (Tried and dropped in round 3: queueing the
    products themselves and launching them 12 at a time - one split count and one tile shape for a mixed batch cost 12 ms
    per step at config 3 and gained nothing on the 17-graph shard, tools/lab/ab_bench.py.)"""
    (gw,), gb = _dw_grads([(g2, x2, param, bias)], _tn_splits(g2.shape[0], g2.shape[1], x2.shape[1]), precision=precision)
    return (gw, gb[0]) if bias is not None else gw


def _pad4(x, w):
    """Zero-pad the reduction axis of (x [.., K], w [N, K]) to a multiple of 4 floats - the own GEMM reads float4s (the
    3-column property embedding prop_nn, CP:379, is the one such Linear of the model).  Plain differentiable torch ops."""
    K = x.shape[-1]
    if w.dim() == 3:
        w = w.view(w.shape[0], w.shape[1])
    pad = -K % 4
    if pad:
        x = torch.nn.functional.pad(x, (0, pad))
        w = torch.nn.functional.pad(w, (0, pad))
    return x, w


def linear(x, w, b=None, precision="f32"):
    """y = x W^T + b (w: [out, in] or a 1x1 Conv1d weight [out, in, 1]) on the own MFMA GEMM (k7).  A reduction that is not a
    multiple of 4 floats is zero-padded, an output width that is not is computed 4-aligned and cut; there is no
    BLAS-library path."""
    if not x.is_cuda:
        raise RuntimeError("singa_amd ops run on the GPU only (no CPU fallback); got a CPU tensor")
    N = w.shape[0]
    if x.numel() == 0:                              # nothing to multiply: zeros that still hang in the autograd graph
        return x.new_zeros(*x.shape[:-1], N) + 0.0 * w.sum() + (0.0 * b.sum() if b is not None else 0.0)
    if _own_linear_ok(x, w):
        return _LinearOwn.apply(x, w, b, None, precision)
    x, w = _pad4(x, w)
    padn = -N % 4
    if padn:
        w = torch.nn.functional.pad(w, (0, 0, 0, padn))
        b = torch.nn.functional.pad(b, (0, padn)) if b is not None else None
    y = _LinearOwn.apply(x.contiguous(), w.contiguous(), b, None, precision)
    return y[..., :N] if padn else y


class _LinearMulti(torch.autograd.Function):
    """Several nn.Linear layers applied to the SAME input (W_Q | W_K | W_V of a self-attention, W_K | W_V of a cross
    attention; CP:96-101, 140-143): one launch forward - one problem per layer, each writing its column block of ONE
    [M, sum N] buffer - one launch for dX (a single product over the concatenated output columns: no per-layer input
    gradients to add up) and one split-reduction launch for all weight gradients.  The outputs are views of the fused
    buffer; the attention kernels read them in place and hand back their gradients in the same arrangement."""

    @staticmethod
    def forward(ctx, x, precision, *wb):
        ws, bs = wb[0::2], wb[1::2]
        ctx.params = (ws, bs)
        ctx.precision = check_precision(precision)
        K = x.shape[-1]
        x2 = _rows(x.reshape(-1, K))
        w2 = [_rows(w.view(w.shape[0], K)) for w in ws]
        _dev(x2, *w2, *bs)
        M = x2.shape[0]
        ns = [w.shape[0] for w in w2]
        tot = sum(ns)
        y = torch.empty(M, tot, device=x.device, dtype=torch.float32)
        ys = y.split(ns, 1)
        _gemm([_prob(x2, w, yb, True, True, bias=b) for w, b, yb in zip(w2, bs, ys)], True, True, precision=precision)
        ctx.save_for_backward(x2, *w2)
        ctx.xshape, ctx.ns = x.shape, ns
        return tuple(yb.view(*x.shape[:-1], n) for yb, n in zip(ys, ns))

    @staticmethod
    def backward(ctx, *gs):
        x2, *w2 = ctx.saved_tensors
        ns = ctx.ns
        tot = sum(ns)
        M, K = x2.shape
        ws, bs = ctx.params
        g2 = [g.reshape(M, n) for g, n in zip(gs, ns)]
        # the gradients normally arrive as the column blocks of one [M, tot] buffer (ops._Attention writes them so)
        fused = all(g.stride(1) == 1 and g.stride(0) == g2[0].stride(0) for g in g2) and g2[0].stride(0) >= tot
        off = 0
        for g, n in zip(g2, ns):
            fused = fused and g.data_ptr() - g2[0].data_ptr() == 4 * off
            off += n
        if fused and g2[0].data_ptr() % 16 == 0 and g2[0].stride(0) % 4 == 0:
            G = g2[0].as_strided((M, tot), (g2[0].stride(0), 1))     # the buffer's first `tot` columns: all blocks side by side
        else:
            G = torch.cat(g2, 1)
        gx = None
        if ctx.needs_input_grad[0]:
            wcat = torch.cat(w2, 0)                                  # [tot, K]: the reduction runs over all output columns
            gx = _rows_gemm_dx(G, wcat, False, ctx.precision).view(ctx.xshape)
        # weight-gradient slabs + the bias gradients (column sums of G, same launch)
        gws, gbs = _dw_grads([(g, x2, w, b) for g, w, b in zip(G.split(ns, 1), ws, bs)], _tn_splits(M, max(ns), K),
                             precision=ctx.precision)
        gbs = iter(gbs)
        out = [gx, None]
        for gw, b in zip(gws, bs):
            out += [gw, next(gbs) if b is not None else None]
        return tuple(out)


def linear_multi(x, layers, precision="f32"):
    """[(weight, bias), ...] applied to the same x -> tuple of outputs (views of one fused buffer).  Falls back to
    separate ops.linear calls for shapes the own GEMM cannot take."""
    if all(_own_linear_ok(x, w) and b is not None for w, b in layers) and len(layers) <= 8:
        flat = []
        for w, b in layers:
            flat += [w, b]
        return _LinearMulti.apply(x, precision, *flat)
    return tuple(linear(x, w, b, precision) for w, b in layers)


def linear_add(x, w, b, addend, precision="f32"):
    """x W^T + b + addend (addend shaped like the result) in one launch."""
    if _own_linear_ok(x, w):
        return _LinearOwn.apply(x, w, b, addend, precision)
    return linear(x, w, b, precision) + addend


class _PosFFN(torch.autograd.Function):
    """PoswiseFeedForward(De)Net up to its residual LayerNorm (CP:161-191): Linear(256 -> 1024) + ReLU + Linear(1024 -> 256)
    as two launches forward (ReLU in the first GEMM's epilogue) and four backward: dh = (g W2) masked by h > 0 in the
    epilogue of its own GEMM, dx = dh W1, and the two split-reduction weight gradients; bias gradients ride in the step's
    shared column-sum launch.  `precision` is that of all six GEMMs; forward keeps it on ctx for backward, like the other
    functions.  forward allocates h and y before its first launch (the order a captured step's memory pool has seen so far),
    so it spells its two products out where two _rows_gemm calls would allocate y between them."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, precision):
        ctx.params = (w1, b1, w2, b2)
        ctx.precision = check_precision(precision)
        K, H = x.shape[-1], w1.shape[0]
        x2 = _rows(x.reshape(-1, K))
        a1, a2 = _rows(w1.view(H, K)), _rows(w2.view(w2.shape[0], H))
        _dev(x2, a1, a2, b1, b2)
        M, N = x2.shape[0], a2.shape[0]
        h = torch.empty(M, H, device=x.device, dtype=torch.float32)
        y = torch.empty(M, N, device=x.device, dtype=torch.float32)
        _gemm([_prob(x2, a1, h, True, True, bias=b1, relu=True)], True, True, precision=precision)
        _gemm([_prob(h, a2, y, True, True, bias=b2)], True, True, precision=precision)
        ctx.save_for_backward(x2, a1, a2, h)
        ctx.xshape = x.shape
        return y.view(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, g):
        x2, a1, a2, h = ctx.saved_tensors
        g2 = _rows(g.reshape(-1, a2.shape[0]))
        w1, b1, w2, b2 = ctx.params
        prec = ctx.precision
        gw2, gb2 = _tn_grad(g2, h, w2, b2, prec)           # (each weight gradient in front of the input gradient it goes with)
        dh = _rows_gemm_dx(g2, a2, False, prec, mask=h)
        gw1, gb1 = _tn_grad(dh, x2, w1, b1, prec)
        gx = _rows_gemm_dx(dh, a1, False, prec).view(ctx.xshape) if ctx.needs_input_grad[0] else None
        return gx, gw1, gb1, gw2, gb2, None


def pos_ffn(x, w1, b1, w2, b2, precision="f32"):
    """relu(x W1^T + b1) W2^T + b2 (the position-wise feed-forward of CP:161-191 before its residual LayerNorm)."""
    return _PosFFN.apply(x, w1, b1, w2, b2, check_precision(precision))


class _SmallVocabEmbedding(torch.autograd.Function):
    """weight[idx] for small tables (atomic numbers, SMILES tokens).  The backward of nn.Embedding on this ROCm build goes
    through thrust::unique_by_key with its own hipMalloc'ed scratch and a host read-back of the segment count - neither
    survives HIP-graph replay (dangling scratch pointers -> memory-aperture faults).  Here the weight gradient is a
    one-hot GEMM: deterministic, allocation-free apart from PyTorch's own pool, capturable."""

    @staticmethod
    def forward(ctx, weight, idx, padding_idx):
        ctx.save_for_backward(idx)
        ctx.V, ctx.padding_idx = weight.shape[0], padding_idx
        return weight.index_select(0, idx.reshape(-1)).view(*idx.shape, weight.shape[1])

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        onehot = torch.nn.functional.one_hot(idx.reshape(-1), ctx.V).to(g.dtype)
        gw = onehot.t() @ g.reshape(-1, g.shape[-1])
        if ctx.padding_idx is not None:                     # nn.Embedding(padding_idx=i): row i receives no gradient
            gw[ctx.padding_idx] = 0
        return gw, None, None


def embedding(weight, idx, padding_idx=None):
    return _SmallVocabEmbedding.apply(weight, idx, padding_idx)


class _RowDotBias(torch.autograd.Function):
    """scale * (x[..., d] * b[d]).sum(-1) (the hoisted bias term of the graph attention's logits, CP:61-65) as one launch
    each way for 32-channel rows (k15e); the bias gradient's per-workgroup partials ride in the step's shared column-sum
    launch.  Other widths: plain torch ops with the same replay-safe bias gradient."""

    @staticmethod
    def forward(ctx, x, b, scale):
        ctx.param, ctx.scale = b, scale
        D = x.shape[-1]
        ctx.own = bool(x.is_cuda and D == 32 and x.numel() > 0)
        if ctx.own:
            x2, b2 = x.reshape(-1, D).contiguous(), b.contiguous()
            _dev(x2, b2)
            out = torch.empty(x2.shape[0], device=x.device, dtype=torch.float32)
            _chk(_lib.lib().singa_rowdot_fwd(_p(x2), _p(b2), _p(out), x2.shape[0], D, scale, _stream()), "singa_rowdot_fwd")
            ctx.save_for_backward(x2, b2)
            ctx.xshape = x.shape
            return out.view(x.shape[:-1])
        ctx.save_for_backward(x, b)
        return (x * (b * scale)).sum(-1)

    @staticmethod
    def backward(ctx, g):
        x, b = ctx.saved_tensors
        if ctx.own:
            M, D = x.shape
            g = g.reshape(-1).contiguous()
            lib = _lib.lib()
            gx = torch.empty_like(x)
            part = torch.empty(lib.singa_rowdot_nparts(M), D, device=x.device, dtype=torch.float32)
            _chk(lib.singa_rowdot_bwd(_p(g), _p(x), _p(b), _p(gx), _p(part), M, D, ctx.scale, _stream()), "singa_rowdot_bwd")
            return gx.view(ctx.xshape), param_colsum(part, [(0, D, ctx.param)])[0], None
        ge = g.unsqueeze(-1) * ctx.scale
        return ge * b, param_colsum((ge * x).reshape(-1, x.shape[-1]), [(0, x.shape[-1], ctx.param)])[0], None


def rowdot_bias(x, b, scale=1.0):
    return _RowDotBias.apply(x, b, scale)


class _BlockWeight(torch.autograd.Function):
    """[[Wr, -Wi], [Wi, Wr]] of an SO2_m_Convolution's Linear weight w = [Wr; Wi] (EF:677-729 with the recombination of
    EF:721-729 folded in): one launch instead of two slices, a negation and three concatenations, and one launch for its
    gradient - added straight into w.grad when the step engine's gradient sink is on."""

    @staticmethod
    def forward(ctx, w):
        ctx.param = w
        w2 = w.contiguous()
        _dev(w2)
        h, k = w2.shape[0] // 2, w2.shape[1]
        out = torch.empty(2 * h, 2 * k, device=w.device, dtype=torch.float32)
        _chk(_lib.lib().singa_block_weight_fwd(_p(w2), _p(out), h, k, _stream()), "singa_block_weight_fwd")
        ctx.hk = (h, k)
        return out

    @staticmethod
    def backward(ctx, G):
        h, k = ctx.hk
        G = G.contiguous()
        wp = ctx.param
        if _GradSink.takes(wp):
            _chk(_lib.lib().singa_block_weight_bwd(_p(G), _p(wp.grad), h, k, 1, _stream()), "singa_block_weight_bwd")
            return None
        gw = torch.empty(2 * h, k, device=G.device, dtype=torch.float32)
        _chk(_lib.lib().singa_block_weight_bwd(_p(G), _p(gw), h, k, 0, _stream()), "singa_block_weight_bwd")
        return gw


def block_weight(w):
    return _BlockWeight.apply(w)
