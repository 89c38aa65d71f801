"""A packed dataset of featurised protein-ligand graphs: G graphs as flat arrays plus per-graph counts, on disk as one
memory-mappable `.npy` per array, on the host as numpy arrays, and - after `.to(device)` - resident on the GPU, where
`batch(ids)` assembles a collated batch with the collate kernel of include/singa_hip_data.h (one host call, two
launches, no per-graph host work and no host -> device copy of graph data).

    pack = PackedDataset.from_reference_dir(root, split_file)      # or .from_graphs(...), or .load(dir)
    pack.save(out_dir)
    store = PackedDataset.load(out_dir).to("cuda")
    batch = store.batch(batch_ids(store.splits["train"], it, batch_size, seed))

`batch(ids)` returns what `graph.collate([graph_i for i in ids])` returns: same keys, shapes, dtypes and values
(`lap_pe` is not stored: `SINGA.prepare` / `TrainStep._stage` compute it for batches that do not carry one).

Featurisation (RDKit / ODDT / OpenBabel, reference utils/Featuriser.py) stays out of scope: a pack is made from graphs
that are already featurised - the reference's `.pt` files through `graph.load_reference_pt`, or the synthetic generator.
"""
import json
import os

import numpy as np
import torch

from . import graph as G
from .graph import E_LL, E_LP, E_PL, E_PP, LA, PA

VERSION = 1
FEAT = 59                                  # atom feature width of the reference's featuriser
MAX_ATOMS = 2048                           # per graph and node type: the limit of singa_knn_graph
AXES = ("n_p", "n_l", "e_pp", "e_ll", "e_lp", "e_pl")
PROPS = ("vina_score", "qed", "sas", "logP", "weight", "tpsa")
_NODE = ((PA, "p", 0), (LA, "l", 1))                                   # node type, suffix, axis
_EDGE = ((E_PP, "pp", 2), (E_LL, "ll", 3), (E_LP, "lp", 4), (E_PL, "pl", 5))   # edge type, suffix, axis
_ROT = (("pp", 2), ("ll", 3), ("lp", 4))                               # rot_rand key, axis (its rows are that type's edges)
_NODE_AXIS = {PA: 0, LA: 1}
GRAPH_AXIS = 6                                                         # one row per graph (tokens, properties)
# field kinds of the collate kernel (include/singa_hip_data.h)
KIND_COPY32, KIND_WIDEN, KIND_WIDEN_BASE, KIND_SLOT = 0, 1, 2, 3
_INT32_MAX = 2 ** 31 - 1


class PackError(ValueError):
    """A graph that cannot be packed; the message names it."""


def _fits_int32(name, what, t):
    if t.numel() and (int(t.min()) < -_INT32_MAX - 1 or int(t.max()) > _INT32_MAX):
        raise PackError(f"graph '{name}': {what} holds a value that does not fit 32-bit storage")
    return t.to(torch.int32).numpy()


def _check_graph(name, g, T):
    """The arrays of one graph, validated (every refusal names the graph) -> dict of numpy arrays."""
    out = {}
    n = {}
    for nt, s, _ in _NODE:
        x, pos, z = g[nt]["x"], g[nt]["pos"], g["atomicnum"][nt]
        if x.dim() != 2 or x.shape[1] != FEAT:
            raise PackError(f"graph '{name}': {nt} feature width {tuple(x.shape)[1:]} is not {FEAT}")
        n[nt] = x.shape[0]
        if n[nt] > MAX_ATOMS:
            raise PackError(f"graph '{name}': {n[nt]} {nt} exceed the {MAX_ATOMS} atoms of one type a graph may have")
        if tuple(pos.shape) != (n[nt], 3) or tuple(z.shape) != (n[nt],):
            raise PackError(f"graph '{name}': {nt} pos / atomicnum do not match its {n[nt]} atoms")
        out[f"x_{s}"] = x.to(torch.float32).numpy()
        out[f"pos_{s}"] = pos.to(torch.float32).numpy()
        out[f"z_{s}"] = _fits_int32(name, f"{nt} atomicnum", z)
    for et, s, _ in _EDGE:
        ei = g[et]["edge_index"]
        if ei.dim() != 2 or ei.shape[0] != 2:
            raise PackError(f"graph '{name}': edge_index of {et} is not [2, E]")
        if ei.shape[1]:
            for row, nt in ((0, et[0]), (1, et[2])):
                lo, hi = int(ei[row].min()), int(ei[row].max())
                if lo < 0 or hi >= n[nt]:
                    raise PackError(f"graph '{name}': edge_index of {et} row {row} leaves its graph's range "
                                    f"[0, {n[nt]}) ({lo}..{hi})")
        out[f"ei_{s}"] = ei.to(torch.int32).numpy()
    ld = g["ligand_data"]
    for k, key in (("tok_in", "smiIndices_input"), ("tok_tgt", "smiIndices_tgt")):
        t = ld[key]
        if t.numel() != T or t.dim() > 2 or (t.dim() == 2 and t.shape[0] != 1):
            raise PackError(f"graph '{name}': token row {key} has shape {tuple(t.shape)}, not [1, {T}]")
        out[k] = _fits_int32(name, key, t.reshape(-1))
    # Python floats -> float32 exactly as collate's torch.tensor(vals, dtype=float32) rounds them
    out["props"] = torch.tensor([float(ld[k]) for k in PROPS], dtype=torch.float32).numpy()
    rot = g.extras.get("rot_rand")
    if rot is not None:
        for k, _ in _ROT:
            r = rot[k]
            if tuple(r.shape) != (out[f"ei_{k}"].shape[1], 3):
                raise PackError(f"graph '{name}': rot_rand['{k}'] has shape {tuple(r.shape)}, not one row of 3 per edge")
            out[f"rot_{k}"] = r.to(torch.float32).numpy()
    return out


class PackedDataset:
    """G graphs as flat arrays.

    counts   int32 [G, 6]   n_p, n_l, e_pp, e_ll, e_lp, e_pl; the exclusive prefix sums of its columns are the offsets
    x_p, pos_p, z_p, x_l, pos_l, z_l     node fields concatenated over the graphs ([sum N, 59] f32, [sum N, 3] f32, [sum N] i32)
    ei_pp, ei_ll, ei_lp, ei_pl           int32 [2, sum E], graph-LOCAL indices
    tok_in, tok_tgt                      int32 [G, T]
    props    float32 [G, 6] vina_score, qed, sas, logP, weight, tpsa
    rot_pp, rot_ll, rot_lp               optional f32 [sum E, 3]: the pinned edge-frame draws (`extras['rot_rand']`), kept
                                         only when every graph carries them
    splits   {'train' | 'val' | 'test': int64 ids into the pack}

    Integers are stored in 32 bits (atomic numbers, tokens, local edge indices); packing refuses a value that does not fit.
    """

    def __init__(self, arrays, names, splits=None, skipped=0):
        self.arrays = arrays
        self.names = list(names)
        self.splits = {k: np.asarray(v, np.int64) for k, v in (splits or {}).items()}
        self.skipped = skipped                      # graphs dropped by skip_invalid=True
        self.counts = np.ascontiguousarray(arrays["counts"], np.int32)
        self.G = self.counts.shape[0]
        self.T = int(arrays["tok_in"].shape[1])
        self.has_rot = "rot_pp" in arrays
        # offsets[a] int64 [G + 1] for the six ragged axes, and the identity for the per-graph axis
        off = np.zeros((7, self.G + 1), np.int64)
        off[:6, 1:] = np.cumsum(self.counts.astype(np.int64), 0).T
        off[6] = np.arange(self.G + 1)
        self.offsets = off
        self.device = None
        self._dev = None

    # ------------------------------------------------------------------------------------------------ constructors
    @classmethod
    def from_graphs(cls, graphs, names=None, skip_invalid=False, splits=None):
        """Pack an iterable of HeteroGraph.  `names` (default: '0', '1', ...) appear in every refusal.  Refused: a feature
        width other than 59, a token row whose length is not T (the first graph's), an edge index outside its graph's
        range, more than 2048 atoms of one type (singa_knn_graph refuses those later anyway), an integer that does not
        fit 32 bits.  skip_invalid=True drops such graphs and counts them in `.skipped` instead (ids in `splits`, which
        index the INPUT sequence, are renumbered and the dropped ones removed)."""
        per, kept_names, kept = [], [], []
        T = None
        skipped = 0
        names = None if names is None else list(names)
        for i, g in enumerate(graphs):
            name = str(i) if names is None else str(names[i])
            try:
                if T is None:
                    T = int(g["ligand_data"]["smiIndices_input"].numel())
                per.append(_check_graph(name, g, T))
            except PackError:
                if not skip_invalid:
                    raise
                skipped += 1
                continue
            kept_names.append(name)
            kept.append(i)
        if not per:
            raise PackError("no graph to pack")
        has_rot = all("rot_pp" in d for d in per)
        arrays = {"counts": np.array([[d["x_p"].shape[0], d["x_l"].shape[0], d["ei_pp"].shape[1], d["ei_ll"].shape[1],
                                       d["ei_lp"].shape[1], d["ei_pl"].shape[1]] for d in per], np.int32)}
        for _, s, _a in _NODE:
            for f in ("x", "pos", "z"):
                arrays[f"{f}_{s}"] = np.concatenate([d[f"{f}_{s}"] for d in per], 0)
        for _, s, _a in _EDGE:
            arrays[f"ei_{s}"] = np.ascontiguousarray(np.concatenate([d[f"ei_{s}"] for d in per], 1))
        for k in ("tok_in", "tok_tgt", "props"):
            arrays[k] = np.stack([d[k] for d in per], 0)
        if has_rot:
            for k, _a in _ROT:
                arrays[f"rot_{k}"] = np.concatenate([d[f"rot_{k}"] for d in per], 0)
        if splits:
            new_id = {old: new for new, old in enumerate(kept)}
            splits = {k: [new_id[int(i)] for i in v if int(i) in new_id] for k, v in splits.items()}
        return cls(arrays, kept_names, splits, skipped)

    @classmethod
    def from_reference_dir(cls, root, split_file=None, skip_invalid=False):
        """Pack the reference's featurised `.pt` graphs under `root` (read with load_reference_pt(path, with_lap=False)).

        The split rule follows the reference's data module (utils/Data.py:206-228): names are
        `split_idx['train' | 'test'][i][0]` with the extension replaced by `.pt`; missing files are skipped; the first
        90 % (int(n * 0.9)) of the surviving train list is `train`, the rest `val`; the test list is `test`.  The
        reference then trains on `lt_train[5000:5512]` only - a debugging leftover that is NOT reproduced here: `train`
        is the whole 90 %.  Without a split file every `.pt` file (sorted by name) is in the train list.  With
        skip_invalid=True a graph that cannot be packed counts as missing."""
        if split_file is None:
            lists = {"train": sorted(f for f in os.listdir(root) if f.endswith(".pt")), "test": []}
        else:
            idx = torch.load(split_file, map_location="cpu", weights_only=False)
            lists = {k: [str(e[0]).split(".")[0] + ".pt" for e in idx[k]] for k in ("train", "test")}
        order, seen = [], {}
        for k in ("train", "test"):
            lists[k] = [f for f in lists[k] if os.path.isfile(os.path.join(root, f))]
            for f in lists[k]:
                if f not in seen:
                    seen[f] = len(order)
                    order.append(f)
        graphs = (G.load_reference_pt(os.path.join(root, f), with_lap=False) for f in order)
        by_list = {k: [seen[f] for f in v] for k, v in lists.items()}
        pack = cls.from_graphs(graphs, names=[f[:-3] for f in order], skip_invalid=skip_invalid, splits=by_list)
        tr = pack.splits["train"]
        cut = int(len(tr) * 0.9)
        pack.splits = {"train": tr[:cut], "val": tr[cut:], "test": pack.splits["test"]}
        return pack

    # ------------------------------------------------------------------------------------------------ disk
    @property
    def nbytes(self):
        return int(sum(a.nbytes for a in self.arrays.values()))

    def save(self, out_dir):
        """One `.npy` per array (memory-mappable) + the split lists + meta.json."""
        os.makedirs(out_dir, exist_ok=True)
        for k, a in self.arrays.items():
            np.save(os.path.join(out_dir, f"{k}.npy"), np.ascontiguousarray(a))
        for k, v in self.splits.items():
            np.save(os.path.join(out_dir, f"split_{k}.npy"), np.asarray(v, np.int64))
        meta = dict(version=VERSION, feat=FEAT, T=self.T, n_graphs=self.G, axes=list(AXES), props=list(PROPS),
                    arrays=sorted(self.arrays), splits=sorted(self.splits), has_rot=self.has_rot, names=self.names,
                    counts=self.counts.tolist(), nbytes=self.nbytes, skipped=self.skipped)
        with open(os.path.join(out_dir, "meta.json"), "w") as f:
            json.dump(meta, f)

    @classmethod
    def load(cls, in_dir, mmap=True):
        with open(os.path.join(in_dir, "meta.json")) as f:
            meta = json.load(f)
        if meta["version"] != VERSION or meta["feat"] != FEAT:
            raise PackError(f"{in_dir}: pack version {meta['version']} / feature width {meta['feat']} is not "
                            f"{VERSION} / {FEAT}")
        mode = "r" if mmap else None
        arrays = {k: np.load(os.path.join(in_dir, f"{k}.npy"), mmap_mode=mode) for k in meta["arrays"]}
        splits = {k: np.load(os.path.join(in_dir, f"split_{k}.npy")) for k in meta["splits"]}
        pack = cls(arrays, meta["names"], splits, meta.get("skipped", 0))
        if pack.counts.tolist() != meta["counts"] or pack.T != meta["T"]:
            raise PackError(f"{in_dir}: meta.json does not describe the arrays next to it")
        return pack

    # ------------------------------------------------------------------------------------------------ host batch
    def _check_ids(self, ids):
        ids = np.asarray(ids, np.int64).reshape(-1)
        if ids.size < 1:
            raise IndexError("batch(ids): at least one graph id")
        if ids.min() < 0 or ids.max() >= self.G:
            raise IndexError(f"batch(ids): id outside [0, {self.G})")
        return ids

    def host_batch(self, ids):
        """`graph.collate([graph_i for i in ids])` by plain gathers from the (possibly memory-mapped) arrays: the reference
        of the collate kernel, and the path of a pack that does not fit on the device."""
        ids = self._check_ids(ids)
        B = ids.size
        cnt = self.counts[ids].astype(np.int64)                             # [B, 6]
        base = np.zeros((6, B + 1), np.int64)
        base[:, 1:] = np.cumsum(cnt, 0).T

        def rows(a):                                                        # source rows of axis a, in batch order
            return np.repeat(self.offsets[a][ids] - base[a][:-1], cnt[:, a]) + np.arange(base[a][-1])

        t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(dt) if dt else torch.from_numpy(np.ascontiguousarray(a))
        out = G.HeteroGraph()
        out.num_graphs = B
        slot = {}
        for nt, s, a in _NODE:
            r = rows(a)
            out.nodes[nt]["x"] = t(self.arrays[f"x_{s}"][r])
            out.nodes[nt]["pos"] = t(self.arrays[f"pos_{s}"][r])
            out.nodes[nt]["ptr"] = t(base[a])
            slot[a] = np.repeat(np.arange(B), cnt[:, a])
            out.nodes[nt]["batch"] = t(slot[a])
            out.globals["atomicnum"][nt] = t(self.arrays[f"z_{s}"][r], torch.int64)
        for et, s, a in _EDGE:
            ei = np.asarray(self.arrays[f"ei_{s}"][:, rows(a)], np.int64)
            e_slot = np.repeat(np.arange(B), cnt[:, a])
            ei[0] += base[_NODE_AXIS[et[0]]][e_slot]
            ei[1] += base[_NODE_AXIS[et[2]]][e_slot]
            out.edges[et]["edge_index"] = t(ei)
        ld = out.globals["ligand_data"]
        props = np.asarray(self.arrays["props"][ids], np.float32)
        for k, name in enumerate(PROPS):
            ld[name] = t(props[:, k])
        ld["smiIndices_input"] = t(self.arrays["tok_in"][ids], torch.int64)
        ld["smiIndices_tgt"] = t(self.arrays["tok_tgt"][ids], torch.int64)
        if self.has_rot:
            out.extras["rot_rand"] = {k: t(self.arrays[f"rot_{k}"][rows(a)]) for k, a in _ROT}
        return out

    # ------------------------------------------------------------------------------------------------ device store
    def to(self, device, device_resident=True, reserve_bytes=2 << 30):
        """Upload the arrays and the offset tables once.  The pack plus `reserve_bytes` (what the training step itself
        needs at least: 2 GiB by default) must fit in the device's free memory; otherwise this raises, naming both sizes -
        device_resident=False keeps the pack on the host: `batch(ids)` is then `host_batch(ids).to(device)`."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("PackedDataset.to: the device store is GPU only (host batches: host_batch)")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self._dev = None
        if not device_resident:
            return self
        need = self.nbytes + self.offsets.nbytes
        free, _ = torch.cuda.mem_get_info(device)
        if need + reserve_bytes > free:
            raise RuntimeError(f"PackedDataset.to: the pack needs {need} bytes on the device plus a reserve of "
                               f"{reserve_bytes} bytes, but {free} bytes are free; pass device_resident=False to keep "
                               "the pack on the host (host batches, copied per step)")
        from . import _lib
        _lib.lib()                                            # a missing library is an error here, not at the first batch
        # (np.array: a writable host copy of one array at a time - a memory-mapped array is read-only)
        dev = {k: torch.from_numpy(np.array(a)).to(device) for k, a in self.arrays.items() if k != "props"}
        dev["props_t"] = torch.from_numpy(np.array(np.asarray(self.arrays["props"]).T, order="C")).to(device)   # [6, G]
        dev["offsets"] = torch.from_numpy(self.offsets).to(device)
        self._dev = dev
        return self

    def batch(self, ids, host_ids=None, alloc=None):
        """The collated batch of graphs `ids`: a host sequence, or - device store only - a contiguous device int32 tensor
        (for instance a slice of an epoch's permutation uploaded once) together with `host_ids`, the same ids on the host:
        output sizes come from the host copy of `counts`, never from a read-back.  Host store: `host_batch`.  Device store:
        outputs are allocated, then the plan and the copy kernel run on the current stream.  Host ids out of range raise;
        device ids out of range are clamped and flagged in `last_status` (a device int32 the caller may read).
        `alloc(shape, dtype)` (device store) supplies the output tensors instead of torch.empty - contiguous, on the store's
        device."""
        if self.device is None:
            return self.host_batch(ids)
        if self._dev is None:
            return self.host_batch(host_ids if host_ids is not None else ids).to(self.device)
        return self._device_batch(ids, host_ids, alloc)

    def _device_batch(self, ids, host_ids, alloc):
        import ctypes

        from . import _capi, _lib
        dev, d = self.device, self._dev
        if torch.is_tensor(ids) and ids.is_cuda:
            if ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous() or ids.device != dev:
                raise ValueError("batch(ids): device ids are a contiguous 1-D int32 tensor on the store's device")
            if host_ids is None or len(host_ids) != ids.numel():
                raise ValueError("batch(ids): device ids need host_ids, their host copy (output sizes come from the host)")
            ids_dev = ids
            host = np.asarray(host_ids, np.int64).reshape(-1)
        else:
            host = self._check_ids(ids.numpy() if torch.is_tensor(ids) else ids)
            ids_dev = torch.from_numpy(host.astype(np.int32)).to(dev, non_blocking=True)
        B = int(host.size)
        if B < 1:
            raise IndexError("batch(ids): at least one graph id")
        cl = np.clip(host, 0, self.G - 1)                   # what the kernel does with a device id out of range
        tot = [int(v) for v in self.counts[cl].astype(np.int64).sum(0)] + [B]          # B additions per axis, no read-back
        if max(tot) > _INT32_MAX:
            raise ValueError("batch(ids): more than 2^31 rows on one axis")
        e = lambda *shape, dt=torch.float32: (alloc(shape, dt) if alloc else torch.empty(shape, dtype=dt, device=dev))
        i64 = torch.int64
        bases = e(7, B + 1, dt=i64)                        # the scans of counts[ids]; rows 0 and 1 are the two `ptr`
        status = e(1, dt=torch.int32)
        out = G.HeteroGraph()
        out.num_graphs = B
        fields = []

        def field(src, dst, axis, width, kind, base_axis=0):
            if tot[axis] > 0:                              # an axis without rows in this batch: nothing to copy
                fields.append((src.data_ptr() if src is not None else 0, dst.data_ptr(), axis, width, kind, base_axis))
            return dst

        for nt, s, a in _NODE:
            st = out.nodes[nt]
            st["x"] = field(d[f"x_{s}"], e(tot[a], FEAT), a, FEAT, KIND_COPY32)
            st["pos"] = field(d[f"pos_{s}"], e(tot[a], 3), a, 3, KIND_COPY32)
            st["ptr"] = bases[a]
            st["batch"] = field(None, e(tot[a], dt=i64), a, 1, KIND_SLOT)
            out.globals["atomicnum"][nt] = field(d[f"z_{s}"], e(tot[a], dt=i64), a, 1, KIND_WIDEN)
        for et, s, a in _EDGE:
            ei = e(2, tot[a], dt=i64)
            src = d[f"ei_{s}"]
            field(src[0], ei[0], a, 1, KIND_WIDEN_BASE, _NODE_AXIS[et[0]])
            field(src[1], ei[1], a, 1, KIND_WIDEN_BASE, _NODE_AXIS[et[2]])
            out.edges[et]["edge_index"] = ei
        ld = out.globals["ligand_data"]
        props = e(6, B)
        for k, name in enumerate(PROPS):
            ld[name] = field(d["props_t"][k], props[k], GRAPH_AXIS, 1, KIND_COPY32)
        ld["smiIndices_input"] = field(d["tok_in"], e(B, self.T, dt=i64), GRAPH_AXIS, self.T, KIND_WIDEN)
        ld["smiIndices_tgt"] = field(d["tok_tgt"], e(B, self.T, dt=i64), GRAPH_AXIS, self.T, KIND_WIDEN)
        if self.has_rot:
            out.extras["rot_rand"] = {k: field(d[f"rot_{k}"], e(tot[a], 3), a, 3, KIND_COPY32) for k, a in _ROT}
        arr = (_capi.CollateField * len(fields))()
        for f, (src, dst, axis, width, kind, base_axis) in zip(arr, fields):
            f.src, f.dst, f.axis, f.width, f.kind, f.base_axis = src, dst, axis, width, kind, base_axis
        totals = (ctypes.c_int64 * 7)(*tot)
        lib = _lib.lib()
        code = lib.singa_collate_batch(ids_dev.data_ptr(), B, self.G, d["offsets"].data_ptr(), bases.data_ptr(),
                                       status.data_ptr(), arr, len(fields), totals,
                                       torch.cuda.current_stream(dev).cuda_stream)
        _capi.check(lib, code, "singa_collate_batch")
        self.last_status = status
        self.last_launches = 2                              # the plan kernel and the copy kernel
        per_word = {KIND_COPY32: 8, KIND_WIDEN: 12, KIND_WIDEN_BASE: 12, KIND_SLOT: 8}      # bytes read + written
        self.last_bytes = sum(per_word[k] * w * tot[a] for _, _, a, w, k, _ in fields) + 7 * 8 * (B + 1)
        return out


# ---------------------------------------------------------------------------------------------------- sampler
def n_batches(split, batch_size, train=True):
    """Batches of one pass over `split`: floor(n / B) when training (the remainder is dropped), ceil(n / B) otherwise."""
    n = len(split)
    return n // batch_size if train else -(-n // batch_size)


def batch_ids(split, it, batch_size, seed, shuffle=True, rank=0, world=1, train=True):
    """The graph ids of iteration `it` (1-based): a pure function, so resuming at `it` reproduces the ids.

    Training: an epoch is floor(n / batch_size) full batches; the remainder of an epoch's permutation is dropped, so that
    every batch has `batch_size` graphs and shapes stay within the engine's size classes (a stated deviation from PyG's
    loader, which yields the short last batch).  The permutation of epoch e comes from numpy.random.default_rng((seed, e)):
    torch's global generator is never touched.  shuffle=False: rows (it-1)*B .. it*B-1 of the split, modulo n.
    train=False (evaluation): the split in order, batch `it` = rows (it-1)*B .. min(it*B, n)-1, a short last batch included.
    Several ranks: each takes dp.shard_range(len(batch), rank, world) of the batch's ids (every rank holds the whole store)."""
    from .dp import shard_range
    split = np.asarray(split, np.int64)
    n, B = len(split), int(batch_size)
    if it < 1 or B < 1:
        raise ValueError("batch_ids: it >= 1 and batch_size >= 1")
    if not train:
        ids = split[(it - 1) * B: min(it * B, n)]
        if ids.size == 0:
            raise IndexError(f"batch_ids: evaluation batch {it} is past the split's {n} graphs")
    elif not shuffle:
        if n < 1:
            raise ValueError("batch_ids: empty split")
        ids = split[np.arange((it - 1) * B, it * B) % n]
    else:
        per = n // B
        if per < 1:
            raise ValueError(f"batch_ids: the split's {n} graphs do not fill one batch of {B}")
        e, k = divmod(it - 1, per)
        perm = np.random.default_rng((int(seed), int(e))).permutation(n)
        ids = split[perm[k * B:(k + 1) * B]]
    lo, hi = shard_range(len(ids), rank, world)
    return ids[lo:hi]
