"""Protein-ligand hetero-graph containers for the hot path, with the PyG `HeteroData` access pattern the reference
uses (`g['protein_atoms']['x']`, `g[('protein_atoms','linked_to','protein_atoms')]['edge_index']`,
`g['atomicnum'][...]`, `g['ligand_data'][...]`; reference model/Embedding.py:227-230, model/GAN.py:26-49) but without
torch_geometric.  Also: PyG-style collate, the synthetic CrossDocked-like generator of SURVEY.md §8d,
a deterministic per-graph Laplacian positional encoding, and a loader for the golden graph fixtures.
"""
import numpy as np
import torch

PA, LA = "protein_atoms", "ligand_atoms"
E_PP, E_LL = (PA, "linked_to", PA), (LA, "linked_to", LA)
E_LP, E_PL = (LA, "interact_with", PA), (PA, "interact_with", LA)
PAD_TOKEN, START_TOKEN, END_TOKEN = 110, 2, 1


class _Store(dict):
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


def _map(v, fn):
    if torch.is_tensor(v):
        return fn(v)
    if isinstance(v, dict):
        return type(v)((k, _map(x, fn)) for k, x in v.items())
    return v


class HeteroGraph:
    """One graph or a collated batch.  Node stores: x [N,59], pos [N,3] (+ ptr, batch, lap_pe after collate);
    edge stores: edge_index [2,E] int64; globals: atomicnum {type: [N] int64}, ligand_data {...}.
    Optional inputs pinned for parity: `rot_rand[(etype)]` = the uniform draws of init_edge_rot_mat (Q6) or
    `edge_rot_mat[...]`, and `knn[node_type]` = the raw kNN edge lists of the CProMG encoders (tie order)."""

    def __init__(self):
        self.nodes = {PA: _Store(), LA: _Store()}
        self.edges = {E_PP: _Store(), E_LL: _Store(), E_LP: _Store(), E_PL: _Store()}
        self.globals = _Store(atomicnum={}, ligand_data={})
        self.extras = _Store()
        self.num_graphs = 1

    def __getitem__(self, key):
        if isinstance(key, tuple):
            return self.edges[key]
        if key in self.nodes:
            return self.nodes[key]
        return self.globals[key]

    def to(self, device):
        fn = lambda t: t.to(device, non_blocking=True)
        self.nodes = {k: _map(v, fn) for k, v in self.nodes.items()}
        self.edges = {k: _map(v, fn) for k, v in self.edges.items()}
        self.globals = _map(self.globals, fn)
        self.extras = _map(self.extras, fn)
        return self


def collate(graphs):
    """PyG collate of HeteroData: concat node tensors, offset edge_index by the cumulative node counts
    of (source type, destination type), `ptr`/`batch` per node type, ligand_data floats -> 1-D tensors."""
    out = HeteroGraph()
    out.num_graphs = len(graphs)
    ptr = {}
    for nt in (PA, LA):
        sizes = [g[nt]["x"].shape[0] for g in graphs]
        ptr[nt] = torch.tensor([0] + sizes).cumsum(0)
        for k in graphs[0][nt]:
            out.nodes[nt][k] = torch.cat([g[nt][k] for g in graphs], 0)
        out.nodes[nt]["ptr"] = ptr[nt]
        out.nodes[nt]["batch"] = torch.repeat_interleave(torch.arange(len(graphs)), torch.tensor(sizes))
        out.globals["atomicnum"][nt] = torch.cat([g["atomicnum"][nt] for g in graphs], 0)
    for et in (E_PP, E_LL, E_LP, E_PL):
        off = [torch.stack([ptr[et[0]][i], ptr[et[2]][i]]).view(2, 1) for i in range(len(graphs))]
        out.edges[et]["edge_index"] = torch.cat([g[et]["edge_index"] + off[i] for i, g in enumerate(graphs)], 1)
    ld0 = graphs[0]["ligand_data"]
    for k in ld0:
        vals = [g["ligand_data"][k] for g in graphs]
        # Python floats -> torch.tensor(list) = float32, as PyG's collate hands them to the reference (the thresholds of
        # GAN:38-40 are therefore taken on float32 values)
        out.globals["ligand_data"][k] = torch.cat(vals, 0) if torch.is_tensor(vals[0]) else torch.tensor(
            vals, dtype=torch.float32)
    for name in ("rot_rand", "edge_rot_mat"):
        if name in graphs[0].extras:
            out.extras[name] = {k: torch.cat([g.extras[name][k] for g in graphs], 0) for k in graphs[0].extras[name]}
    return out


def laplacian_pe(edge_index, n, k=8):
    """Deterministic Laplacian positional encoding of ONE graph: the k eigenvectors after the smallest of
    I - D^-1/2 A D^-1/2 (in-degree clipped at 1), symmetric eigensolver, sign fixed by making the entry of largest
    magnitude positive.  (dgl.lap_pe, reference model/CProMG.py:562-571, uses random signs on the whole batched
    graph - not reproducible, so at our boundary the encoding is an input)

    A bonded pocket graph has dozens of connected components, i.e. a many-fold zero eigenvalue (and further exact
    repeats from isomorphic fragments), and LAPACK's basis of a repeated eigenvalue's subspace depends on its blocking -
    on the BLAS thread count of the process (round 3's "8-graph discrepancy": bench.py's GPU process and its CPU-oracle
    child computed different, equally valid encodings of the same graphs).  So every cluster of repeated eigenvalues gets
    a canonical basis first: Gram-Schmidt over the columns of the cluster's projector V V^T - which does not depend on
    the basis - in atom order."""
    a = np.zeros((n, n))
    ei = np.asarray(edge_index)
    a[ei[0], ei[1]] = 1.0
    dinv = np.clip(a.sum(0), 1, None) ** -0.5
    lap = np.eye(n) - dinv[:, None] * a * dinv[None, :]
    w, v = np.linalg.eigh(0.5 * (lap + lap.T))
    v = _canonical_eigenbasis(w, v, k + 1)
    v = v[:, 1:k + 1]
    if v.shape[1] < k:
        v = np.concatenate([v, np.zeros((n, k - v.shape[1]))], 1)
    idx = np.argmax(np.abs(v), axis=0)
    sign = np.where(v[idx, np.arange(v.shape[1])] < 0, -1.0, 1.0)
    return torch.tensor(v * sign, dtype=torch.float32)


def _canonical_eigenbasis(w, v, upto, tol=1e-9):
    """Replace the eigenvectors of every cluster of (numerically) repeated eigenvalues that reaches into the first `upto`
    columns by a basis that only depends on the cluster's SUBSPACE: the projector P = V V^T is the same for any basis, and
    Gram-Schmidt over its columns P e_0, P e_1, ... (atom order, columns that add less than 1e-6 of new direction are
    skipped) is a function of P alone."""
    v = v.copy()
    n = w.shape[0]
    lo = 0
    while lo < min(upto, n):
        hi = lo + 1
        while hi < n and w[hi] - w[hi - 1] <= tol:
            hi += 1
        m = hi - lo
        if m > 1:
            vc = v[:, lo:hi]
            basis = np.zeros((n, m))
            found = 0
            for j in range(n):
                r = vc @ vc[j]                                     # P e_j
                if found:
                    b = basis[:, :found]
                    r = r - b @ (b.T @ r)
                    r = r - b @ (b.T @ r)                          # twice: orthogonal to rounding
                nr = np.linalg.norm(r)
                if nr > 1e-6:
                    basis[:, found] = r / nr
                    found += 1
                    if found == m:
                        break
            if found == m:
                v[:, lo:hi] = basis
        lo = hi
    return v


def from_arrays(d, with_lap=True):
    """Build a HeteroGraph from the arrays of a tests/golden/graph_*.npz fixture (or the synthetic generator)."""
    g = HeteroGraph()
    t = lambda a, dt=None: torch.as_tensor(np.asarray(a), dtype=dt)
    for nt, s in ((PA, "p"), (LA, "l")):
        g.nodes[nt]["x"] = t(d[f"x_{s}"], torch.float32)
        g.nodes[nt]["pos"] = t(d[f"pos_{s}"], torch.float32)
        g.globals["atomicnum"][nt] = t(d[f"z_{s}"], torch.int64)
    for et, s in ((E_PP, "pp"), (E_LL, "ll"), (E_LP, "lp"), (E_PL, "pl")):
        g.edges[et]["edge_index"] = t(d[f"ei_{s}"], torch.int64)
    vina, qed, sas = (float(v) for v in np.asarray(d["props"]))
    g.globals["ligand_data"] = dict(vina_score=vina, qed=qed, sas=sas, logP=0.0, weight=0.0, tpsa=0.0,
                                    smiIndices_input=t(d["tok_in"], torch.int64).view(1, -1),
                                    smiIndices_tgt=t(d["tok_tgt"], torch.int64).view(1, -1))
    if with_lap:
        g.nodes[PA]["lap_pe"] = laplacian_pe(g.edges[E_PP]["edge_index"].numpy(), g.nodes[PA]["x"].shape[0])
        g.nodes[LA]["lap_pe"] = laplacian_pe(g.edges[E_LL]["edge_index"].numpy(), g.nodes[LA]["x"].shape[0])
    return g


def load_npz(path, with_lap=True):
    z = np.load(path)
    return from_arrays({k: z[k] for k in z.files}, with_lap)


EXAMPLE_NAMES = ("3wi2_4tpp", "4agq_5a7b", "5cp5_4nue")


def example_graph(i, with_lap=True):
    """The i-th (mod 3) of the three protein-ligand graphs the reference bundles (example/*.pt), shipped as plain arrays
    under singa_amd/data/examples (what `train.py --data golden` trains on)."""
    import os
    here = os.path.dirname(os.path.abspath(__file__))
    return load_npz(os.path.join(here, "data", "examples", f"graph_{EXAMPLE_NAMES[i % 3]}.npz"), with_lap)


# ----------------------------------------------------------------------------------------------- synthetic graphs
def _closest_pairs(pa, pb, count, same):
    d = np.linalg.norm(pa[:, None, :] - pb[None, :, :], axis=-1)
    if same:
        iu = np.triu_indices(pa.shape[0], 1)
        order = np.argsort(d[iu], kind="stable")[:count]
        return iu[0][order], iu[1][order]
    flat = np.argsort(d.reshape(-1), kind="stable")[:count]
    return flat // pb.shape[0], flat % pb.shape[0]


def synthetic_graph(graph_id, n_protein=200, n_ligand=30, e_pp=1700, e_ll=64, e_x=118, tgt_len=200, with_lap=True):
    """One random protein-ligand hetero-graph with the bundled files' schema (SURVEY.md §8d 'Synthetic generator'):
    rng = default_rng(1000 + graph_id); protein atoms uniform in a cube of density 0.05 A^-3 with min pair distance
    1.0 A; ligand atoms inside a 6 A sphere at the centre; linked_to = the e/2 closest pairs in both directions;
    interact_with = the e_x closest ligand-protein pairs, PL = LP mirrored in the same order (Q5).  with_lap=False leaves
    the Laplacian encodings out (numpy's dense eigensolver is 90 % of the generation time; batches whose encodings are
    computed inside the step - SINGA.prepare / TrainStep._stage - do not need them)."""
    rng = np.random.default_rng(1000 + graph_id)
    side = (n_protein / 0.05) ** (1.0 / 3.0)

    def place(n, draw, others):
        # accepted points live in one preallocated array (same draws, same acceptance test as a list rebuilt per draw,
        # without the per-draw list -> array conversion that made a 470-atom graph cost 0.1 s)
        ref = np.empty((n + len(others), 3), np.float64)
        m = len(others)
        if m:
            ref[:m] = np.asarray(others)
        k = 0
        while k < n:
            cand = draw()
            if m + k == 0 or np.min(np.linalg.norm(ref[:m + k] - cand, axis=1)) >= 1.0:
                ref[m + k] = cand
                k += 1
        return [ref[m + i].copy() for i in range(n)]

    def lig_draw():
        while True:
            c = rng.uniform(-6, 6, 3)
            if np.linalg.norm(c) <= 6.0:
                return c + side / 2
    lig = place(n_ligand, lig_draw, [])
    pro = place(n_protein, lambda: rng.uniform(0, side, 3), lig)
    pos_p, pos_l = np.asarray(pro, np.float32), np.asarray(lig, np.float32)

    def feats(n):
        x = np.zeros((n, 59), np.float32)
        z = rng.choice([6, 7, 8, 16], size=n, p=[0.65, 0.15, 0.17, 0.03])
        x[np.arange(n), rng.integers(0, 44, n)] = 1.0
        x[:, -15:] = (rng.random((n, 15)) < 0.2).astype(np.float32)
        x[:, 51] = rng.uniform(-0.3, 0.3, n)
        return x, z.astype(np.int64)
    x_p, z_p = feats(n_protein)
    x_l, z_l = feats(n_ligand)
    a, b = _closest_pairs(pos_p, pos_p, e_pp // 2, True)
    ei_pp = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    a, b = _closest_pairs(pos_l, pos_l, e_ll // 2, True)
    ei_ll = np.stack([np.concatenate([a, b]), np.concatenate([b, a])])
    li, pj = _closest_pairs(pos_l, pos_p, e_x, False)
    ei_lp = np.stack([li, pj])
    ei_pl = np.stack([pj, li])
    n_tok = int(rng.integers(20, 61))
    body = rng.integers(3, 116, n_tok)
    tok_in = np.full(tgt_len, PAD_TOKEN, np.int64)
    tok_tgt = np.full(tgt_len, PAD_TOKEN, np.int64)
    tok_in[0], tok_in[1:1 + n_tok] = START_TOKEN, body
    tok_tgt[:n_tok], tok_tgt[n_tok] = body, END_TOKEN
    props = np.array([rng.uniform(-10, -5), rng.uniform(0.3, 0.9), rng.uniform(2, 6)])
    g = from_arrays(dict(x_p=x_p, pos_p=pos_p, z_p=z_p, x_l=x_l, pos_l=pos_l, z_l=z_l, ei_pp=ei_pp, ei_ll=ei_ll,
                         ei_lp=ei_lp, ei_pl=ei_pl, props=props, tok_in=tok_in, tok_tgt=tok_tgt), with_lap)
    g.extras["rot_rand"] = {k: torch.tensor(rng.random((n, 3)), dtype=torch.float32)
                            for k, n in (("pp", ei_pp.shape[1]), ("ll", ei_ll.shape[1]), ("lp", ei_lp.shape[1]))}
    return g


def ragged_sizes(graph_id, n_protein=(230, 470), n_ligand=(25, 35), e_pp_per_node=2.0, e_ll_per_node=2.2, e_x=80):
    """Sizes of synthetic graph `graph_id` of a CrossDocked-shaped (ragged) workload, SURVEY.md §8d config 3: Np ~ U[230,470],
    Nl ~ U[25,35] (integers, inclusive), Epp = 2 Np, Ell ~ 2.2 Nl (even: both directions of each bond), Ex = 80 - the
    statistics of the bundled example graphs.  Drawn from their own stream so that the graph's content stream
    (default_rng(1000 + graph_id)) is the same as for a fixed-size graph."""
    rng = np.random.default_rng(77_000_000 + graph_id)
    n_p = int(rng.integers(n_protein[0], n_protein[1] + 1))
    n_l = int(rng.integers(n_ligand[0], n_ligand[1] + 1))
    e_ll = 2 * int(round(e_ll_per_node * n_l / 2))
    return dict(n_protein=n_p, n_ligand=n_l, e_pp=2 * int(round(e_pp_per_node * n_p / 2)), e_ll=e_ll, e_x=int(e_x))


WORKLOADS = {
    # SURVEY.md §8d configs 2, 3 (ragged, as the survey defines it; config 4 = the same batch sharded over the ranks), 5
    "cfg2_b32_l2": dict(n_graphs=32, lmax=2, n_protein=200, n_ligand=30, e_pp=1700, e_ll=64, e_x=118),
    "cfg3_b128_l4": dict(n_graphs=128, lmax=4, ragged=dict(n_protein=(230, 470), n_ligand=(25, 35), e_pp_per_node=2.0,
                                                            e_ll_per_node=2.2, e_x=80)),
    "cfg3_fixed_b128_l4": dict(n_graphs=128, lmax=4, n_protein=350, n_ligand=30, e_pp=700, e_ll=66, e_x=80),
    "cfg5_l6": dict(n_graphs=64, lmax=6, n_protein=800, n_ligand=40, e_pp=7600, e_ll=88, e_x=156),
    "cfg5_l6_b8": dict(n_graphs=8, lmax=6, n_protein=800, n_ligand=40, e_pp=7600, e_ll=88, e_x=156),
    # BASELINE.json configs[3] seen from ONE rank: the cost-balanced shard rank 0 of 8 owns of the
    # config-3 batch (dp.shard_ranges_by_cost over graphs 0..127) - what a one-GPU box can time of the 8-GPU strong split
    "cfg4_shard_r0of8": dict(parent="cfg3_b128_l4", shard=(0, 8)),
}


def resolve_workload(name):
    """-> (lmax, generator kwargs, graph ids of one batch, graphs of the parent batch).  A `shard` workload names the
    graphs one rank of a strong split of its parent owns."""
    wl = dict(WORKLOADS[name])
    if "parent" in wl:
        from .dp import shard_ranges_by_cost
        rank, world = wl["shard"]
        L, kw, ids, n = resolve_workload(wl["parent"])
        lo, hi = shard_ranges_by_cost([graph_cost(graph_sizes(i, **kw)) for i in ids], world)[rank]
        return L, kw, list(ids[lo:hi]), n
    n, L = wl.pop("n_graphs"), wl.pop("lmax")
    return L, wl, list(range(n)), n


def graph_sizes(graph_id, ragged=None, **kw):
    """Generator arguments of synthetic graph `graph_id` of a workload (fixed sizes, or drawn per graph when `ragged`)."""
    return ragged_sizes(graph_id, **ragged) if ragged else dict(kw)


def graph_cost(sizes):
    """Edge count E_pp + E_ll + 2 E_x of a graph: the cost driver by which shards are balanced."""
    return sizes["e_pp"] + sizes["e_ll"] + 2 * sizes["e_x"]


def synthetic_batch(n_graphs, first_id=0, ragged=None, ids=None, with_lap=True, **kw):
    ids = range(first_id, first_id + n_graphs) if ids is None else ids
    return collate([synthetic_graph(i, with_lap=with_lap, **graph_sizes(i, ragged, **kw)) for i in ids])


# ----------------------------------------------------------------------------------------------- padding to capacities
def batch_sizes(batch):
    """(protein atoms, ligand atoms, E_pp, E_ll, E_x) of a collated batch - from tensor shapes, no device read-back."""
    return (batch[PA]["x"].shape[0], batch[LA]["x"].shape[0], batch[E_PP]["edge_index"].shape[1],
            batch[E_LL]["edge_index"].shape[1], batch[E_LP]["edge_index"].shape[1])


def pad_batch(batch, n_p, n_l, e_pp, e_ll, e_x):
    """The batch grown to fixed capacities with INERT padding, so that batches of different sizes share one captured HIP
    graph (real CrossDocked batches are ragged: reference utils/Data.py:230, train.py:113-133).  Padding atoms belong to
    no graph (batch id = num_graphs): they sit far away from everything, get no kNN neighbours, never reach the
    transformer's dense layout and therefore receive a zero gradient; padding edges only connect padding atoms (spread
    evenly over them, never a self loop, so every edge frame is well defined).  Logits, loss and every parameter gradient
    of the padded batch equal the unpadded ones (tests/test_padding_gpu.py).  Needs `lap_pe` on the node stores."""
    r_p, r_l, r_pp, r_ll, r_x = batch_sizes(batch)
    d_p, d_l = n_p - r_p, n_l - r_l
    assert d_p >= 2 and d_l >= 2 and e_pp >= r_pp and e_ll >= r_ll and e_x >= r_x, "capacities must exceed the batch"
    dev = batch[PA]["x"].device
    B = batch.num_graphs
    out = HeteroGraph()
    out.num_graphs = B
    for nt, real, extra, yoff in ((PA, r_p, d_p, 1.0e3), (LA, r_l, d_l, 2.0e3)):
        st, o = batch.nodes[nt], out.nodes[nt]
        assert "lap_pe" in st, "pad_batch: compute the Laplacian encodings before padding"
        far = torch.zeros(extra, 3, device=dev)
        far[:, 0] = 1.0e3 + 4.0 * torch.arange(extra, device=dev)
        far[:, 1] = yoff
        far[:, 2] = 1.0e3
        o["x"] = torch.cat([st["x"], st["x"].new_zeros(extra, st["x"].shape[1])])
        o["pos"] = torch.cat([st["pos"], far.to(st["pos"].dtype)])
        o["batch"] = torch.cat([st["batch"], st["batch"].new_full((extra,), B)])
        o["lap_pe"] = torch.cat([st["lap_pe"], st["lap_pe"].new_zeros(extra, st["lap_pe"].shape[1])])
        o["ptr"] = st["ptr"]
        z = batch.globals["atomicnum"][nt]
        out.globals["atomicnum"][nt] = torch.cat([z, z.new_full((extra,), 6)])
    out.globals["ligand_data"] = batch.globals["ligand_data"]

    def ring(count, base_s, n_s, base_d, n_d, same):
        """`count` padding edges: source i % n_s, destination shifted so that (same node set) it never equals the source."""
        i = torch.arange(count, device=dev)
        s = i % n_s
        if same:
            d = (s + 1 + (i // n_s) % (n_s - 1)) % n_s
        else:
            d = (i + i // n_s) % n_d
        return torch.stack([base_s + s, base_d + d])

    pads = {E_PP: ring(e_pp - r_pp, r_p, d_p, r_p, d_p, True), E_LL: ring(e_ll - r_ll, r_l, d_l, r_l, d_l, True),
            E_LP: ring(e_x - r_x, r_l, d_l, r_p, d_p, False)}
    pads[E_PL] = pads[E_LP].flip(0)                                   # mirrored in the same order (Q5)
    for et in (E_PP, E_LL, E_LP, E_PL):
        out.edges[et]["edge_index"] = torch.cat([batch.edges[et]["edge_index"], pads[et].to(batch.edges[et]["edge_index"].dtype)], 1)
    for k, v in batch.extras.items():
        if k == "rot_rand":
            fill = torch.tensor([0.1, 0.5, 0.9], device=dev)
            want = {"pp": e_pp, "ll": e_ll, "lp": e_x}
            out.extras[k] = {kk: torch.cat([t, fill.to(t.dtype).expand(want[kk] - t.shape[0], 3)]) for kk, t in v.items()}
        elif k in ("edge_rot_mat", "knn"):
            raise ValueError(f"pad_batch: pinned '{k}' inputs (parity fixtures) cannot be padded")
        elif k not in ("prepared", "prefetched", "prepared_by_prefetch", "pad"):
            out.extras[k] = v
    out.extras["pad"] = {"n_real": {PA: r_p, LA: r_l}}
    return out


# ----------------------------------------------------------------------------------------------- reference .pt graphs
def load_reference_pt(path, with_lap=True):
    """Read a pickled PyG `HeteroData` graph of the reference (example/*.pt, dataset/crossdocked_graph10_v3/*.pt) without
    torch_geometric: stub classes with the pickled class paths receive the state dicts, and the
    fields the hot path reads are copied into a HeteroGraph.  Older files keep the Vina score in `y[0]`
    (reference utils/Featuriser.py:155 vs :164)."""
    import sys
    import types

    created = []

    def stub(mod, *names):
        if mod not in sys.modules:
            sys.modules[mod] = types.ModuleType(mod)
            created.append(mod)
        for n in names:
            if not hasattr(sys.modules[mod], n):
                setattr(sys.modules[mod], n, type(n, (), {}))

    try:
        import torch_geometric  # noqa: F401  (if the real package is present, use it)
    except ImportError:
        stub("torch_geometric")
        stub("torch_geometric.data")
        stub("torch_geometric.data.hetero_data", "HeteroData")
        stub("torch_geometric.data.storage", "BaseStorage", "NodeStorage", "EdgeStorage")
        stub("torch_geometric.data.graph_store", "EdgeAttr")
        stub("torch_geometric.data.feature_store", "TensorAttr")
    try:
        obj = torch.load(path, map_location="cpu", weights_only=False)
    finally:
        for m in created:
            sys.modules.pop(m, None)
    st = obj.__dict__

    def mapping(store):
        return store.__dict__["_mapping"]
    glob = mapping(st["_global_store"])
    g = HeteroGraph()
    for nt in (PA, LA):
        m = mapping(st["_node_store_dict"][nt])
        g.nodes[nt]["x"] = m["x"].float()
        g.nodes[nt]["pos"] = m["pos"].float()
        g.globals["atomicnum"][nt] = glob["atomicnum"][nt].long()
    for et in (E_PP, E_LL, E_LP, E_PL):
        g.edges[et]["edge_index"] = mapping(st["_edge_store_dict"][et])["edge_index"].long()
    ld = glob["ligand_data"]
    vina = float(ld["vina_score"]) if "vina_score" in ld else float(glob["y"][0])
    g.globals["ligand_data"] = dict(vina_score=vina, qed=float(ld["qed"]), sas=float(ld["sas"]), logP=float(ld["logP"]),
                                    weight=float(ld["weight"]), tpsa=float(ld["tpsa"]),
                                    smiIndices_input=ld["smiIndices_input"].long().view(1, -1),
                                    smiIndices_tgt=ld["smiIndices_tgt"].long().view(1, -1))
    if with_lap:
        g.nodes[PA]["lap_pe"] = laplacian_pe(g.edges[E_PP]["edge_index"].numpy(), g.nodes[PA]["x"].shape[0])
        g.nodes[LA]["lap_pe"] = laplacian_pe(g.edges[E_LL]["edge_index"].numpy(), g.nodes[LA]["x"].shape[0])
    return g


def laplacian_pe_batched(edge_index, batch, num_graphs, k=8):
    """laplacian_pe for every graph of a collated batch on the tensors' own device (reference
    model/CProMG.py:562-571, called inside forward at GAN.py:71,77).  On the GPU: the library's own batched eigensolver
    (ops.lap_pe -> singa_lap_pe: one workgroup per graph builds the normalised Laplacian from the graph's edges and
    diagonalises it per connected component - Householder tridiagonalisation + Sturm multi-section + inverse iteration,
    fp64), same sign convention as `laplacian_pe`.  Eigenvectors of a repeated eigenvalue (a bonded pocket graph has dozens
    of connected components, i.e. a many-fold zero eigenvalue) are ANY orthonormal basis of that invariant subspace, as in
    the reference (dgl adds random signs on top).

    The route is chosen PER GRAPH (k <= 8 on the GPU): graphs of up to 896 atoms go to ops.lap_pe - a batch of such graphs
    alone is one launch, as ever, and a small graph's rows do not depend on what else the batch holds; graphs of 897 .. 2,048
    atoms go to ops.lap_pe_large in one launch over just those graphs (no dense matrix: sparse rows, the zero eigenvalue's
    vectors written per connected component, filtered subspace iteration for the rest); only a graph that kernel gives up on
    (its status entry: an atom with more than 32 neighbours, no convergence, ...) takes the dense route below, in a sub-batch
    of its own.  Graphs of 2,049 .. 32,768 atoms go to ops.lap_pe_xl in one call over just those graphs (many workgroups per
    graph, the same sparse rows and null vectors, a filter whose degree follows the Ritz values, so that a single long chain
    converges); a graph that route gives up on, or one above 32,768 atoms, takes the dense route too.  A batch with a large
    graph costs two read-backs more than one without: the sizes of the launches, and "did any graph give up"; one with a graph
    above 2,048 atoms also the read-backs of ops.lap_pe_xl.  CPU tensors / k > 8: dense Laplacians and one batched
    torch.linalg.eigh (padding rows get a unit diagonal above every real eigenvalue (<= 2), so they sort last)."""
    dev = edge_index.device
    n = batch.numel()
    num = torch.zeros(num_graphs, dtype=torch.long, device=dev).index_add_(0, batch, torch.ones_like(batch))
    mx = int(num.max())
    start = num.cumsum(0) - num
    gb = batch[edge_index[0]]
    if not (edge_index.is_cuda and k <= 8):
        return _laplacian_pe_dense(edge_index, batch, num, mx, start, gb, k)
    from . import ops
    # edges grouped by graph (a collated batch already has them so; the stable sort makes no assumption)
    order = torch.argsort(gb, stable=True)
    gs = gb[order]
    src = (edge_index[0][order] - start[gs]).to(torch.int32)
    dst = (edge_index[1][order] - start[gs]).to(torch.int32)
    eptr = torch.searchsorted(gs, torch.arange(num_graphs + 1, device=dev)).to(torch.int32)
    if mx <= 896:
        return ops.lap_pe(src, dst, eptr, num, start, n, mx, k)
    small = num <= 896
    large = ~small & (num <= 2048)
    stats = [(num * small).max(), (num * large).max(), large.sum(), large[gs].sum()]
    xl = None
    if mx >= ops.LAP_XL_MIN_ATOMS:                       # (a batch without such a graph runs what it always ran)
        xl = (num >= ops.LAP_XL_MIN_ATOMS) & (num <= ops.LAP_XL_MAX_ATOMS)
        stats += [(num * xl).max(), xl.sum(), xl[gs].sum()]
    mx_s, mx_l, n_l, e_l, mx_x, n_x, e_x = (torch.stack(stats).tolist() + [0, 0, 0])[:7]
    # the small graphs: the same launch with the other graphs' sizes set to 0 (a workgroup without atoms returns at once)
    out = ops.lap_pe(src, dst, eptr, num * small, start, n, mx_s, k) if mx_s else torch.empty(n, k, device=dev, dtype=torch.float32)
    bad = num > ops.LAP_XL_MAX_ATOMS
    for op, which, mx_w, n_w, e_w in ((ops.lap_pe_large, large, mx_l, n_l, e_l), (ops.lap_pe_xl, xl, mx_x, n_x, e_x)):
        if n_w:
            sel = torch.argsort(~which, stable=True)[:n_w]                         # this route's graphs, in batch order
            esel = torch.argsort(~which[gs], stable=True)[:e_w]                    # their edges, still grouped by graph
            ecount = (eptr[1:] - eptr[:-1])[sel]
            eptr_w = torch.cat([ecount.new_zeros(1), ecount.cumsum(0)]).to(torch.int32)
            _, status = op(src[esel], dst[esel], eptr_w, num[sel], start[sel], n, mx_w, k, out=out)
            bad[sel] = status != 0
    if bool(bad.any()):
        # the graphs left over, as a batch of their own through the dense route
        rows = torch.nonzero(bad[batch]).squeeze(1)
        new_row = torch.zeros(n, dtype=torch.long, device=dev)
        new_row[rows] = torch.arange(rows.numel(), device=dev)
        new_graph = bad.long().cumsum(0) - 1
        sub_batch = new_graph[batch[rows]]
        sub_num = num[bad]
        sub_ei = new_row[edge_index[:, bad[gb]]]
        out[rows] = _laplacian_pe_dense(sub_ei, sub_batch, sub_num, int(sub_num.max()), sub_num.cumsum(0) - sub_num,
                                        sub_batch[sub_ei[0]], k)
    return out


def _laplacian_pe_dense(edge_index, batch, num, mx, start, gb, k):
    """laplacian_pe_batched's dense route: [B, mx, mx] fp64 Laplacians, one batched torch.linalg.eigh."""
    dev = edge_index.device
    n = batch.numel()
    num_graphs = num.numel()
    local = torch.arange(n, device=dev) - start[batch]
    a = torch.zeros(num_graphs, mx, mx, dtype=torch.float64, device=dev)
    a[gb, local[edge_index[0]], local[edge_index[1]]] = 1.0
    dinv = a.sum(1).clamp(min=1).pow(-0.5)
    lap = torch.eye(mx, dtype=torch.float64, device=dev).unsqueeze(0) - dinv.unsqueeze(2) * a * dinv.unsqueeze(1)
    lap = 0.5 * (lap + lap.transpose(1, 2))
    pad = torch.arange(mx, device=dev).unsqueeze(0) >= num.unsqueeze(1)          # [B, mx]
    lap = lap.masked_fill(pad.unsqueeze(1) | pad.unsqueeze(2), 0.0) + torch.diag_embed(pad.double() * 3.0)
    _, v = torch.linalg.eigh(lap)
    v = v[:, :, 1:k + 1]
    if v.shape[2] < k:
        v = torch.cat([v, v.new_zeros(num_graphs, mx, k - v.shape[2])], 2)
    idx = v.abs().argmax(dim=1, keepdim=True)
    sign = torch.where(torch.gather(v, 1, idx) < 0, -1.0, 1.0)
    v = (v * sign)
    return v[batch, local].to(torch.float32)
