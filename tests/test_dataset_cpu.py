"""The packed dataset on the host (singa_amd/dataset.py): pack -> save -> memory-mapped load -> batch(ids) equals
graph.collate of the same graphs key for key; the reference's `.pt` files and split rule; the refusals at pack time; the
stateless sampler; the argument errors of the collate entry point through the built library.  No GPU."""
import ctypes
import os
import shutil

import numpy as np
import pytest
import torch

from singa_amd import dataset as D
from singa_amd import graph as G
from tests.test_capi_exports import declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
NAMES = ("3wi2_4tpp", "4agq_5a7b", "5cp5_4nue")
# twelve small ragged graphs: one above 256 protein atoms, one with a single ligand atom's worth of edges
SIZES = [(40, 9), (23, 5), (300, 12), (64, 7), (17, 4), (90, 11), (33, 6), (128, 8), (51, 10), (29, 5), (75, 9), (45, 13)]
ID_LISTS = ([0], [11, 0, 5, 5, 3], list(range(11, -1, -1)))


def small_graphs():
    """Twelve ragged synthetic graphs (module cache; never modified); graph 4 has no ligand-protein edges."""
    if not hasattr(small_graphs, "gs"):
        gs = []
        for i, (n_p, n_l) in enumerate(SIZES):
            g = G.synthetic_graph(i, n_protein=n_p, n_ligand=n_l, e_pp=2 * n_p, e_ll=2 * (n_l - 1), e_x=5 + i, tgt_len=64,
                                  with_lap=False)
            if i == 4:
                g.edges[G.E_LP]["edge_index"] = torch.zeros(2, 0, dtype=torch.int64)
                g.edges[G.E_PL]["edge_index"] = torch.zeros(2, 0, dtype=torch.int64)
                g.extras["rot_rand"]["lp"] = torch.zeros(0, 3)
            gs.append(g)
        small_graphs.gs = gs
    return small_graphs.gs


def without_rot(gs):
    out = []
    for g in gs:
        h = G.HeteroGraph()
        h.nodes, h.edges, h.globals = g.nodes, g.edges, g.globals
        out.append(h)
    return out


def flat(g):
    """Every tensor of a HeteroGraph under a path key."""
    out = {}

    def walk(prefix, v):
        if torch.is_tensor(v):
            out[prefix] = v
        elif isinstance(v, dict):
            for k, x in v.items():
                walk(f"{prefix}/{k}", x)
        else:
            out[prefix] = v
    walk("nodes", g.nodes)
    walk("edges", g.edges)
    walk("globals", dict(g.globals))
    walk("extras", dict(g.extras))
    return out


def assert_same_graph(got, want):
    a, b = flat(got), flat(want)
    assert list(a) == list(b), (list(a), list(b))
    assert got.num_graphs == want.num_graphs
    for k in a:
        if torch.is_tensor(b[k]):
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (k, a[k].dtype, b[k].dtype, a[k].shape, b[k].shape)
            assert torch.equal(a[k].cpu(), b[k].cpu()), k
        else:
            assert a[k] == b[k], k


@pytest.mark.parametrize("rot", [True, False])
def test_round_trip_equals_collate(tmp_path, rot):
    gs = small_graphs() if rot else without_rot(small_graphs())
    assert max(g[G.PA]["x"].shape[0] for g in gs) > 256
    pack = D.PackedDataset.from_graphs(gs)
    assert pack.has_rot == rot and pack.G == 12 and pack.T == 64
    pack.save(str(tmp_path))
    assert os.path.exists(tmp_path / "meta.json") and os.path.exists(tmp_path / "x_p.npy")
    loaded = D.PackedDataset.load(str(tmp_path), mmap=True)
    assert isinstance(loaded.arrays["x_p"], np.memmap)
    assert loaded.nbytes == pack.nbytes and loaded.names == [str(i) for i in range(12)]
    for ids in ID_LISTS:
        assert_same_graph(loaded.batch(ids), G.collate([gs[i] for i in ids]))
    with pytest.raises(IndexError):
        loaded.batch([12])
    with pytest.raises(IndexError):
        loaded.batch([])


def test_reference_files_equal_golden_arrays():
    pts = [G.load_reference_pt(os.path.join(GOLD, f"example_{n}.pt"), with_lap=False) for n in NAMES]
    pack = D.PackedDataset.from_graphs(pts, names=NAMES)
    assert not pack.has_rot and pack.T == 200
    want = G.collate([G.load_npz(os.path.join(GOLD, f"graph_{n}.npz"), with_lap=False) for n in NAMES])
    got = pack.batch([0, 1, 2])
    a, b = flat(got), flat(want)
    assert list(a) == list(b)
    for k in a:
        if k.endswith(("logP", "weight", "tpsa")):            # the .npz fixtures carry three of the six properties
            continue
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    assert_same_graph(got, G.collate(pts))


def test_from_reference_dir_split_rule(tmp_path):
    root = tmp_path / "graphs"
    root.mkdir()
    # 11 train entries that exist (copies of the three fixtures under new names) + one missing; 2 test entries + one missing
    train = [f"t{i:02d}" for i in range(11)]
    for i, n in enumerate(train):
        shutil.copy(os.path.join(GOLD, f"example_{NAMES[i % 3]}.pt"), root / f"{n}.pt")
    for n in ("u0", "u1"):
        shutil.copy(os.path.join(GOLD, f"example_{NAMES[0]}.pt"), root / f"{n}.pt")
    split = {"train": [(f"{n}.sdf", "ligand") for n in train[:4]] + [("gone.sdf", "x")] + [(f"{n}.pdb", "y") for n in train[4:]],
             "test": [("u0.sdf", 0), ("absent.sdf", 0), ("u1.sdf", 0)]}
    torch.save(split, str(tmp_path / "split.pt"))
    pack = D.PackedDataset.from_reference_dir(str(root), str(tmp_path / "split.pt"))
    assert pack.G == 13 and "gone" not in pack.names and "absent" not in pack.names
    names = lambda k: [pack.names[i] for i in pack.splits[k]]
    assert names("train") == train[:9]                         # int(11 * 0.9) = 9: the first 90 % of the surviving list
    assert names("val") == train[9:]
    assert names("test") == ["u0", "u1"]
    pack.save(str(tmp_path / "pack"))
    again = D.PackedDataset.load(str(tmp_path / "pack"))
    assert {k: v.tolist() for k, v in again.splits.items()} == {k: v.tolist() for k, v in pack.splits.items()}
    want = G.collate([G.load_reference_pt(os.path.join(GOLD, f"example_{NAMES[i % 3]}.pt"), with_lap=False) for i in (10, 1)])
    assert_same_graph(again.batch([pack.names.index("t10"), pack.names.index("t01")]), want)
    # without a split file: every file, sorted, is in the train list
    allp = D.PackedDataset.from_reference_dir(str(root))
    assert allp.G == 13 and len(allp.splits["train"]) == 11 and len(allp.splits["val"]) == 2 and len(allp.splits["test"]) == 0


def _broken(kind):
    g = G.synthetic_graph(100, n_protein=20, n_ligand=5, e_pp=30, e_ll=8, e_x=6, tgt_len=64, with_lap=False)
    if kind == "width":
        g.nodes[G.LA]["x"] = g.nodes[G.LA]["x"][:, :58]
    elif kind == "tokens":
        g.globals["ligand_data"]["smiIndices_tgt"] = g.globals["ligand_data"]["smiIndices_tgt"][:, :63]
    elif kind == "edge":
        g.edges[G.E_LP]["edge_index"] = g.edges[G.E_LP]["edge_index"].clone()
        g.edges[G.E_LP]["edge_index"][1, 2] = 20               # protein index 20 of 20 atoms
    elif kind == "atoms":
        n = 2049
        g.nodes[G.PA]["x"] = torch.zeros(n, 59)
        g.nodes[G.PA]["pos"] = torch.zeros(n, 3)
        g.globals["atomicnum"][G.PA] = torch.full((n,), 6)
    elif kind == "int32":
        g.globals["atomicnum"][G.LA] = g.globals["atomicnum"][G.LA].clone()
        g.globals["atomicnum"][G.LA][0] = 2 ** 31
    return g


@pytest.mark.parametrize("kind,word", [("width", "feature width"), ("tokens", "token row"), ("edge", "edge_index"),
                                       ("atoms", "2048"), ("int32", "32-bit")])
def test_refusals_name_the_graph(kind, word):
    good = small_graphs()[:2]
    with pytest.raises(D.PackError, match="culprit") as e:
        D.PackedDataset.from_graphs(good + [_broken(kind)], names=["a", "b", "culprit"])
    assert word in str(e.value)
    pack = D.PackedDataset.from_graphs([good[0], _broken(kind), good[1]], names=["a", "culprit", "b"], skip_invalid=True,
                                       splits={"train": [0, 1, 2]})
    assert pack.skipped == 1 and pack.names == ["a", "b"] and pack.splits["train"].tolist() == [0, 1]
    assert_same_graph(pack.batch([1, 0]), G.collate([good[1], good[0]]))


def test_sampler_is_stateless_and_covers_epochs():
    split = np.arange(100, 123)                                 # 23 graphs, B = 5: 4 batches per epoch, 3 dropped
    B, seed = 5, 7
    state = torch.random.get_rng_state()
    epochs = []
    for e in range(3):
        ids = np.concatenate([D.batch_ids(split, 4 * e + k + 1, B, seed) for k in range(4)])
        assert len(ids) == 20 and len(set(ids.tolist())) == 20 and set(ids.tolist()) <= set(split.tolist())
        epochs.append(ids)
    assert torch.equal(torch.random.get_rng_state(), state)     # torch's global generator is never touched
    assert not np.array_equal(epochs[0], epochs[1]) and not np.array_equal(epochs[1], epochs[2])
    assert np.array_equal(D.batch_ids(split, 7, B, seed), epochs[1][10:15])          # resuming at `it` reproduces the ids
    assert not np.array_equal(D.batch_ids(split, 7, B, seed + 1), epochs[1][10:15])
    # rank shards are disjoint and their concatenation is the batch
    full = D.batch_ids(split, 3, B, seed)
    parts = [D.batch_ids(split, 3, B, seed, rank=r, world=2) for r in range(2)]
    assert np.array_equal(np.concatenate(parts), full) and [len(p) for p in parts] == [3, 2]
    # shuffle=False: rows (it-1)*B .. it*B-1 modulo n
    for it in (1, 5, 6):
        assert np.array_equal(D.batch_ids(split, it, B, seed, shuffle=False), split[np.arange((it - 1) * B, it * B) % 23])
    # evaluation: in order, the short last batch included
    ev = [D.batch_ids(split, k, B, seed, train=False) for k in range(1, D.n_batches(split, B, train=False) + 1)]
    assert [len(v) for v in ev] == [5, 5, 5, 5, 3] and np.array_equal(np.concatenate(ev), split)
    assert D.n_batches(split, B) == 4
    with pytest.raises(ValueError):
        D.batch_ids(split[:3], 1, B, seed)


def test_data_binding_table_matches_header():
    from singa_amd import _capi
    assert sorted(_capi.DATA_EXPORTS) == declared_symbols("singa_hip_data.h")
    others = set(_capi.EXPORTS) | set(_capi.LAB_EXPORTS) | set(_capi.GEN_EXPORTS) | set(_capi.FORCE_EXPORTS) | \
        set(_capi.SWOR_EXPORTS) | set(_capi.STREAM_EXPORTS) | set(_capi.VALENCE_EXPORTS) | set(_capi.BEAM_EXPORTS) | \
        set(_capi.UNITS_EXPORTS) | set(_capi.PREFIX_EXPORTS)
    assert not set(_capi.DATA_EXPORTS) & others


def test_collate_argument_errors_without_gpu():
    """Argument validation happens before any HIP call, so it is checked on the CPU through the built library (host
    buffers stand in for device pointers: nothing is launched)."""
    import __graft_entry__
    from singa_amd import _capi
    __graft_entry__.build()
    lib = _capi.bind(__graft_entry__.LIB)
    B, Gn = 3, 5
    ids = np.zeros(B, np.int32)
    off = np.zeros((7, Gn + 1), np.int64)
    bases = np.zeros((7, B + 1), np.int64)
    status = np.zeros(1, np.int32)
    src, dst = np.zeros(64, np.int32), np.zeros(64, np.int64)
    p = lambda a: a.ctypes.data

    def call(ids_=ids, B_=B, G_=Gn, off_=off, bases_=bases, status_=status, fld=(), tot=(4, 4, 4, 4, 4, 4, B), n=None):
        arr = (_capi.CollateField * max(1, len(fld)))()
        for f, (s, d, axis, width, kind, base_axis) in zip(arr, fld):
            f.src, f.dst, f.axis, f.width, f.kind, f.base_axis = s, d, axis, width, kind, base_axis
        totals = (ctypes.c_int64 * 7)(*tot) if tot is not None else None
        g = lambda a: p(a) if a is not None else None
        return lib.singa_collate_batch(g(ids_), B_, G_, g(off_), g(bases_), g(status_), arr if fld is not None else None,
                                       len(fld) if n is None else n, totals, None)

    ok = (p(src), p(dst), 0, 1, D.KIND_WIDEN, 0)
    assert call(ids_=None, fld=[ok]) == -1                                            # SINGA_E_NULL
    assert call(off_=None, fld=[ok]) == -1 and call(bases_=None, fld=[ok]) == -1 and call(status_=None, fld=[ok]) == -1
    assert call(tot=None, fld=[ok]) == -1
    assert call(fld=[(0, p(dst), 0, 1, D.KIND_WIDEN, 0)]) == -1 and call(fld=[(p(src), 0, 0, 1, D.KIND_COPY32, 0)]) == -1
    assert b"collate_batch" in lib.singa_last_error_string()
    assert call(B_=0, fld=[ok]) == -3 and call(B_=2049, fld=[ok]) == -3               # SINGA_E_SHAPE
    assert call(G_=0, fld=[ok]) == -3
    assert call(fld=[ok], n=33) == -3 and call(fld=[ok], n=-1) == -3
    assert call(fld=[ok], tot=(4, 4, 4, 4, 4, 4, B + 1)) == -3                        # totals[6] != B
    assert b"width mismatch" in lib.singa_last_error_string()
    assert call(fld=[ok], tot=(-1, 4, 4, 4, 4, 4, B)) == -3
    assert call(fld=[(p(src), p(dst), 7, 1, D.KIND_WIDEN, 0)]) == -3                  # axis
    assert call(fld=[(p(src), p(dst), 0, 0, D.KIND_WIDEN, 0)]) == -3                  # width
    assert b"width" in lib.singa_last_error_string()
    assert call(fld=[(p(src), p(dst), 0, 1, 4, 0)]) == -3                             # kind
    assert call(fld=[(p(src), p(dst), 2, 1, D.KIND_WIDEN_BASE, 2)]) == -3             # base_axis
    assert call(fld=[(p(src) + 2, p(dst), 0, 1, D.KIND_WIDEN, 0)]) == -3              # misaligned source
    assert call(fld=[(p(src), p(dst) + 4, 0, 1, D.KIND_WIDEN, 0)]) == -3              # i64 destination on 4 bytes
    assert call(fld=[(p(src), p(dst), 0, 1 << 30, D.KIND_WIDEN, 0)]) == -3            # 2^31 or more items
