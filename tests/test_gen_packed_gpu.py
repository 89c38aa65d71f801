"""-m gpu: generation over a packed dataset (singa_amd/generate.py, `gen.py --data packed`).  Every pass of `generate_split`
against the decoder called directly on `graph.collate` of the same graphs, as gen.py called it before there were passes: ids,
order, names, uniforms, streams and prompts are right exactly when the two agree bit for bit.  lmax 2, random weights, a pack of
synthetic_graph(3..11) with train = ids 0-4 and test = ids 5-8, 4 rows per pocket, 16 columns."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from singa_amd import dataset as D
from singa_amd import graph as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
T, PER, SEED = 16, 4, 1
TEST_IDS = [5, 6, 7, 8]
NAMES = [f"synthetic_{i}" for i in range(3, 12)]


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same(a, b):
    a, b = torch.as_tensor(a).cpu(), torch.as_tensor(b).cpu()
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """(model, cfg, voc, the graphs, the pack's directory, a device-resident store)"""
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA
    cfg = load_config(lmax=2)
    torch.manual_seed(7)
    model = SINGA(cfg, device=DEV).eval()
    graphs = [G.synthetic_graph(i, with_lap=False) for i in range(3, 12)]
    pack = D.PackedDataset.from_graphs(graphs, names=NAMES, splits={"train": range(5), "val": [], "test": TEST_IDS})
    out = str(tmp_path_factory.mktemp("pack") / "pack")
    pack.save(out)
    return model, cfg, list(cfg.model.decoder.smiVoc), graphs, out, D.PackedDataset.load(out).to(DEV)


def direct_example(world, ids):
    """The pockets `ids` as gen.py prepared its pockets before this module existed: collate on the host, prepare, the protein
    pass of the embedding, the encoder's kNN list -> (example, the batch)"""
    from singa_amd.config import Config
    from singa_amd.model.CProMG import DenseMap, knn_graph
    model, cfg, _, graphs, _, _ = world
    B = len(ids)
    batch = G.collate([graphs[i] for i in ids]).to(DEV)
    model.prepare(batch)
    with torch.no_grad():
        feat = model.embedding(batch, gen_mode=True)[G.PA].embedding.reshape(batch[G.PA]["x"].shape[0], -1)
    ex = Config()
    at = batch[G.PA]["batch"]
    ex.protein_element_batch, ex.protein_atom_feature, ex.protein_pos = at, feat, batch[G.PA]["pos"]
    ex.protein_atom_laplacian = batch[G.PA]["lap_pe"]
    knn = knn_graph(batch[G.PA]["pos"], cfg.model.encoder.knn, at, B, DenseMap(at, B))
    ex.protein_knn = knn[:, knn[0] >= 0]
    return ex, batch


def ones(rows):
    return torch.ones(rows, 3, dtype=torch.float32, device=DEV)


@pytest.fixture(scope="module")
def direct_sample(world):
    """`sample` called directly on the passes [5, 6, 7] and [8]: computed once, left unchanged."""
    from singa_amd.generate import pocket_uniforms
    from singa_amd.model.Sampling import sample
    model, _, voc = world[:3]
    out = []
    for ids in ([5, 6, 7], [8]):
        ex, _ = direct_example(world, ids)
        tr = {}
        tokens = sample(model, voc, PER, len(ids), T, ex, ones(len(ids) * PER), device=DEV, suppress=("&", "^"),
                        uniforms=pocket_uniforms(SEED, ids, PER, T, DEV), trace=tr, grammar="smiles")
        out.append((tokens.cpu(), tr["lengths"].cpu(), tr["sum_logp"].cpu()))
    return out


def test_sample_passes_equal_direct_calls(world, direct_sample):
    from singa_amd.generate import format_lines, generate_split
    model, cfg, voc, _, _, store = world
    recs = list(generate_split(model, cfg, voc, store, "test", "sample", PER, 3, max_length=T, seed=SEED, grammar="smiles"))
    assert [r["ids"].tolist() for r in recs] == [[5, 6, 7], [8]]
    assert [r["names"] for r in recs] == [NAMES[5:8], NAMES[8:9]]
    assert sum(r["tokens"].shape[0] for r in recs) == 16
    eos = voc.index("$")
    for rec, (tokens, lengths, logp) in zip(recs, direct_sample):
        assert same(rec["tokens"], tokens) and same(rec["lengths"], lengths) and same(rec["sum_logp"], logp)
        assert rec["pocket_of"] == [r // PER for r in range(tokens.shape[0])]
        assert all(eos in row for row in rec["tokens"].tolist())              # the grammar ended every row
    lines = [ln.split("\t") for rec in recs for ln in format_lines(rec, voc)]
    assert [ln[0] for ln in lines] == [n for n in NAMES[5:9] for _ in range(PER)] and all(len(ln) == 4 for ln in lines)
    # the two passes did not get each other's numbers: pocket 8 alone is not pocket 5
    assert not torch.equal(recs[1]["tokens"], recs[0]["tokens"][:PER])


def test_host_resident_store_gives_the_same_bits(world, direct_sample):
    from singa_amd.generate import generate_split
    model, cfg, voc, _, out, _ = world
    host = D.PackedDataset.load(out).to(DEV, device_resident=False)
    rec = next(generate_split(model, cfg, voc, host, "test", "sample", PER, 3, max_length=T, seed=SEED, grammar="smiles"))
    tokens, lengths, logp = direct_sample[0]
    assert rec["names"] == NAMES[5:8]
    assert same(rec["tokens"], tokens) and same(rec["lengths"], lengths) and same(rec["sum_logp"], logp)


def test_distinct_pass_equals_direct_call(world):
    from singa_amd.generate import generate_split
    from singa_amd.model.Sampling import sample_distinct
    model, cfg, voc, _, _, store = world
    rec = next(generate_split(model, cfg, voc, store, "test", "distinct", PER, 2, max_length=T, seed=SEED, grammar="smiles"))
    ids = [5, 6]
    assert rec["ids"].tolist() == ids and rec["names"] == NAMES[5:7]
    ex, _ = direct_example(world, ids)
    tr = {}
    tokens = sample_distinct(model, voc, PER, 2, T, ex, ones(2 * PER), device=DEV, suppress=("&", "^"), grammar="smiles", seed=SEED,
                             streams=np.array(ids), trace=tr)                 # the graph ids, not the places in the pass
    assert same(rec["tokens"], tokens) and same(rec["lengths"], tr["lengths"]) and same(rec["sum_logp"], tr["sum_logp"])
    assert same(rec["valid"], tr["valid"]) and int(rec["valid"].sum()) > 0


def test_device_beam_pass_equals_direct_call(world):
    from singa_amd.generate import generate_split
    from singa_amd.model.BeamSearch import beam_search_device
    model, cfg, voc, _, _, store = world
    rec = next(generate_split(model, cfg, voc, store, "test", "beam", PER, 2, max_length=T, grammar="valence"))
    ids = [5, 6]
    assert rec["ids"].tolist() == ids and rec["names"] == NAMES[5:7] and rec["per"] == 1 and rec["on_device"]
    ex, _ = direct_example(world, ids)
    tr = {}
    tokens = beam_search_device(model, voc, PER, 2, T, 1, ex, ones(2 * PER), device=DEV, trace=tr, grammar="valence")
    best = [max(h.beams, key=lambda x: x[0]) for h in tr["hyps"]]
    assert same(rec["tokens"], tokens) and rec["tokens"].shape[0] == 2
    assert rec["lengths"].tolist() == [len(h) for _, h in best]
    assert rec["sum_logp"].tolist() == [s * len(h) ** 0.7 for s, h in best]
    assert rec["steps"] == tr["steps"]


def test_stream_pass_equals_direct_call(world):
    from singa_amd.generate import generate_split, pocket_uniforms
    from singa_amd.model.Sampling import sample_stream
    model, cfg, voc, _, _, store = world
    rec = next(generate_split(model, cfg, voc, store, "test", "sample", PER, 4, max_length=T, seed=SEED, rows_per_pocket=2))
    assert rec["ids"].tolist() == TEST_IDS and rec["tokens"].shape == (16, T)
    ex, _ = direct_example(world, TEST_IDS)
    tr = {}
    tokens = sample_stream(model, voc, PER, 4, T, ex, ones(4), 2, device=DEV, suppress=("&", "^"),
                           uniforms=pocket_uniforms(SEED, TEST_IDS, PER, T, DEV), trace=tr)
    assert same(rec["tokens"], tokens) and same(rec["lengths"], tr["lengths"]) and same(rec["sum_logp"], tr["sum_logp"])


def test_own_ligands_scored_under_the_training_prompt(world):
    """`molecules="dataset", prop="dataset"`: the numbers are `score`'s for the decoded `tok_tgt` string under `dataset_props`, and
    `dataset_props` is what the training forward of the same batch feeds `prop_nn`."""
    from singa_amd.generate import dataset_props, generate_split, ligand_strings
    from singa_amd.model.Sampling import score
    model, cfg, voc, graphs, _, store = world
    recs = list(generate_split(model, cfg, voc, store, "test", "score", 1, 3, first=3, molecules="dataset", prop="dataset"))
    assert len(recs) == 1
    rec, ids = recs[0], [5, 6, 7]
    eos = voc.index("$")
    texts = []
    for i in ids:                                                              # tok_tgt spelled with the vocabulary up to '$'
        row = graphs[i]["ligand_data"]["smiIndices_tgt"].reshape(-1).tolist()
        texts.append("".join(voc[t] for t in row[:row.index(eos)]))
    assert rec["molecules"] == texts == ligand_strings(store, ids, voc) and rec["names"] == NAMES[5:8]
    ex, batch = direct_example(world, ids)
    props = dataset_props(model, batch)
    res = score(model, voc, [[t] for t in texts], 3, ex, props, device=DEV)
    print("sum_logp", rec["sum_logp"].tolist(), "direct", res["sum_logp"])
    for b in range(3):
        assert float(rec["sum_logp"][b]) == res["sum_logp"][b][0] and int(rec["lengths"][b]) == res["length"][b][0]
        assert int(rec["lengths"][b]) == graphs[ids[b]]["ligand_data"]["smiIndices_tgt"].reshape(-1).tolist().index(eos) + 1

    seen = []
    hook = model.model.decoder.prop_nn.register_forward_hook(lambda mod, args, out: seen.append(args[0].detach().clone()))
    try:
        with torch.no_grad():
            model(batch)                                                       # the training forward, on the prepared batch
    finally:
        hook.remove()
    assert len(seen) == 1 and tuple(props.shape) == (3, cfg.train.num_props) and props.dtype == torch.float32
    assert same(seen[0].reshape(3, -1), props)
    want = [[float(graphs[i]["ligand_data"]["vina_score"] < -7.5), float(graphs[i]["ligand_data"]["qed"] > 0.6),
             float(graphs[i]["ligand_data"]["sas"] < 4.0)] for i in ids]
    assert props.cpu().tolist() == want
    # ... and the pack's own batch gives the same prompt
    assert same(dataset_props(model, store.batch(ids)), props)


def test_a_pass_that_cannot_fit_is_refused_before_any_launch(world, monkeypatch):
    from singa_amd.generate import generate_split
    model, cfg, voc, _, _, store = world
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    total = torch.cuda.mem_get_info()[1]
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, total))

    def no_batch(*a, **k):
        raise AssertionError("a batch was assembled before the refusal")
    monkeypatch.setattr(store, "batch", no_batch)
    before = torch.cuda.memory_allocated()
    for mode, kw in (("sample", {}), ("distinct", {}), ("beam", dict(beam_select="device")), ("sample", dict(rows_per_pocket=1024))):
        with pytest.raises(ValueError, match="pockets_per_pass"):              # 4 x 1024 rows x 201 positions: 7.6 GB of caches
            next(generate_split(model, cfg, voc, store, "test", mode, 1024, 4, max_length=201, **kw))
    assert torch.cuda.memory_allocated() == before


def test_gen_entry_point_on_a_pack(world):
    cmd = [sys.executable, os.path.join(ROOT, "gen.py"), "--data", "packed", "--dataset", world[4], "--split", "test", "--mode", "sample",
           "--num-samples", "4", "--max-length", "16", "--pockets-per-pass", "3", "--grammar", "smiles", "--lmax", "2", "--seed", "1"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout.decode()[-2000:], r.stderr.decode()[-2000:])
    out = r.stdout.decode().splitlines()
    data = [ln.split("\t") for ln in out if not ln.startswith("#")]
    assert len(data) == 16 and all(len(ln) == 4 for ln in data)
    assert [ln[0] for ln in data] == [n for n in NAMES[5:9] for _ in range(4)]
    for _, text, length, logp in data:
        assert 0 < int(length) <= 15 and float(logp) <= 0.0 and not set(text) & set("&$^")
    passes = [ln for ln in out if ln.startswith("# pass ")]
    assert len(passes) == 2 and "3 pockets" in passes[0] and "1 pockets" in passes[1] and all("steps" in ln for ln in passes)
