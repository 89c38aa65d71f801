"""Generation over the pockets of a packed dataset, pass by pass: the layer between `dataset.PackedDataset` and the decoders
of model/Sampling.py and model/BeamSearch.py.

    store = PackedDataset.load(dir).to("cuda")
    for rec in generate_split(model, cfg, voc, store, "test", "sample", 100, 20, grammar="smiles", seed=1):
        for line in format_lines(rec, voc):
            print(line)

A pass is `pockets_per_pass` consecutive graphs of a split: `store.batch(ids)` (the collate kernel), `pocket_example`
(`SINGA.prepare`, the protein pass of the embedding, the kNN list the encoder takes) and one call of `sample`, `sample_stream`,
`sample_distinct`, `beam_search_device`, `beam_search` or `score` (`decode`: the calls gen.py makes, written once for every data
source).  No kernel is launched here that those calls do not launch.

What a pocket receives does not depend on the pass it falls into: its uniforms are drawn from a generator seeded with a mix of
(seed, graph id) (`pocket_uniforms`), `sample_distinct` takes `streams = graph ids mod 2^32`, the prompt is the pocket's own
(`dataset_props`) or one for all.  Whether the encoder rounds a pocket alike in every batch composition is not established for
every launch, so equal molecules across different `pockets_per_pass` are measured (profiles/gen_packed/), not promised.  A pack
whose graphs carry no edge-frame draws (`rot_rand`) has them drawn per pass from torch's global generator.

Out of scope: pockets without a ligand in the pack (the packer refuses such graphs), overlapping the next pass's encoding with
the current pass's decoding, and graphs above the existing atom limits.
"""
import time

import numpy as np
import torch

from . import graph as G
from . import smiles
from .config import Config

MODES = ("sample", "distinct", "beam", "score")
_M64 = (1 << 64) - 1


# ---------------------------------------------------------------------------------------------------- one batch of pockets
def pocket_example(model, cfg, batch, prepared=None):
    """(example, B) of a collated batch on the device: `model.prepare`, the protein pass of the embedding alone (reference
    gen.py:157-160), and the attribute bag the decoders read - protein_element_batch, protein_atom_feature, protein_pos,
    protein_atom_laplacian and protein_knn, the encoder's kNN list without its empty (-1) slots.  `prepared()`, if given, is
    called once `model.prepare` has returned (a clock's lap)."""
    from .model.CProMG import DenseMap, knn_graph
    B = batch.num_graphs
    model.prepare(batch)
    if prepared is not None:
        prepared()
    with torch.no_grad():
        feat = model.embedding(batch, gen_mode=True)[G.PA].embedding.reshape(batch[G.PA]["x"].shape[0], -1)
    ex = Config()
    ids = batch[G.PA]["batch"]
    ex.protein_element_batch, ex.protein_atom_feature, ex.protein_pos = ids, feat, batch[G.PA]["pos"]
    ex.protein_atom_laplacian = batch[G.PA]["lap_pe"]
    knn = knn_graph(batch[G.PA]["pos"], cfg.model.encoder.knn, ids, B, DenseMap(ids, B))
    ex.protein_knn = knn[:, knn[0] >= 0]
    return ex, B


def dataset_props(model, batch):
    """[B, num_props] f32: the property prompt training gives each graph of `batch` (`GAN.property_prompt`, the function
    the training forward calls); None for a model without a prompt."""
    from .model.GAN import property_prompt
    tr = model.config.train
    return property_prompt(batch["ligand_data"], tr.prop) if tr.num_props else None


# ---------------------------------------------------------------------------------------------------- ids, passes, uniforms
def split_ids(store, split, first=None):
    """The int64 ids of `store.splits[split]` in stored order, the first `first` of them if given.  ValueError, naming the
    splits the pack has, for a split that is absent or empty."""
    ids = store.splits.get(split)
    if ids is None or len(ids) == 0:
        have = {k: len(v) for k, v in store.splits.items() if len(v)}
        raise ValueError(f"split_ids: the pack has no graphs in a split '{split}'; its splits are {have or 'none'}")
    if first is not None:
        if first < 1:
            raise ValueError(f"split_ids: first >= 1 (got {first})")
        ids = ids[:first]
    return np.asarray(ids, np.int64)


def passes(ids, pockets_per_pass):
    """Consecutive chunks of `ids`, `pockets_per_pass` each, the last one possibly shorter: every id once, in order."""
    P = int(pockets_per_pass)
    if P < 1:
        raise ValueError(f"passes: pockets_per_pass >= 1 (got {pockets_per_pass})")
    return [ids[i:i + P] for i in range(0, len(ids), P)]


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def pocket_seed(seed, graph_id):
    """The 64-bit mix of (seed, graph id) that seeds a pocket's generator: splitmix64(splitmix64(seed mod 2^64) xor (graph id
    mod 2^64)), splitmix64 being Steele, Lea and Flood's finaliser with the increment 0x9E3779B97F4A7C15 added first; the
    lowest 63 bits are used."""
    return _splitmix64(_splitmix64(int(seed) & _M64) ^ (int(graph_id) & _M64)) & ((1 << 63) - 1)


def pocket_uniforms(seed, graph_ids, per, max_length, device):
    """f32 [max_length, len(graph_ids) * per] in [0, 1) on `device`: what `sample` and `sample_stream` take as `uniforms=`.
    Pocket-major: columns p * per .. (p + 1) * per - 1 belong to graph_ids[p] and are torch.rand((max_length, per)) of a CPU
    torch.Generator seeded with `pocket_seed(seed, graph_ids[p])` - a function of (seed, graph id, per, max_length) alone, not
    of the pass, the pocket's place in it or its neighbours."""
    cols = []
    for g in np.asarray(graph_ids, np.int64).reshape(-1):
        gen = torch.Generator().manual_seed(pocket_seed(seed, int(g)))
        cols.append(torch.rand((int(max_length), int(per)), generator=gen, dtype=torch.float32))
    return torch.cat(cols, 1).to(device)


# ---------------------------------------------------------------------------------------------------- one decoder call
def decode(model, voc, example, B, mode, per, prop, max_length, *, device, temperature=1.0, top_k=0, top_p=1.0, grammar=None,
           prefix=None, rows_per_pocket=None, tiles=False, beam_select="host", seed=0, generator=None, uniforms=None, streams=None,
           molecules=None):
    """One decoder call for the `B` pockets of `example`, as gen.py makes it, and its result as a record of host tensors.

    mode "sample": `sample`, or `sample_stream` with `rows_per_pocket`; `per` molecules per pocket from `uniforms`, else
    `generator`.  "distinct": `sample_distinct` with `seed` and `streams`.  "beam": `beam_search`, or `beam_search_device` with
    beam_select="device" or under a `grammar`; `per` beams, the best hypothesis of each pocket.  "score": `score` of
    `molecules[b]`, the strings of pocket b.  `prop`: [B, num_props], one prompt per pocket, or None.  `prefix`: a SMILES
    fragment every sequence starts with.  `max_length` may be None in score mode only (the longest molecule + 2).

    The record: `mode`, `per` (rows per pocket: 1 in beam mode, the longest list in score mode), `pocket_of` (the pocket of every
    row), `tokens` int64 [rows, L], `lengths`, `sum_logp`, `steps`, `path` where the call reports one, `valid` (uint8, distinct
    mode: 0 for a slot a small tree left empty) and `molecules` (score mode: the string of every row).  In score mode the rows
    are the molecules given, pocket-major, and `tokens` spells them; in host-selected beam mode `steps` is the length the live
    beams reached."""
    from .model.BeamSearch import beam_search, beam_search_device
    from .model.Sampling import sample, sample_distinct, sample_stream, score
    if mode not in MODES:
        raise ValueError(f"decode: mode is one of {MODES} (got {mode!r})")
    dev, tr = device, {}
    if mode == "score":
        res = score(model, voc, molecules, B, example, prop, device=dev, max_length=max_length, grammar=grammar,
                    rows_per_pocket=rows_per_pocket, tiles=tiles)
        flat = [m for ms in molecules for m in ms]
        L = max_length or max(len(smiles.tokenize(m, voc)) for m in flat) + 2
        tokens = torch.from_numpy(smiles.encode(flat, voc, L, end=True))
        tokens[tokens < 0] = list(voc).index("^")
        return dict(mode=mode, per=max(len(ms) for ms in molecules), pocket_of=[b for b, ms in enumerate(molecules) for _ in ms],
                    tokens=tokens, lengths=torch.tensor([n for ns in res["length"] for n in ns], dtype=torch.int32),
                    sum_logp=torch.tensor([s for ss in res["sum_logp"] for s in ss], dtype=torch.float32), steps=None,
                    molecules=flat, result=res)
    rows_prop = None if prop is None else prop.to(dev).float().repeat_interleave(per, 0)
    forced = None if prefix is None else smiles.encode([prefix] * B, voc, max_length)
    rec = dict(mode=mode, per=per)
    if mode == "sample":
        common = dict(device=dev, temperature=temperature, top_k=top_k, top_p=top_p, suppress=("&", "^"), generator=generator,
                      uniforms=uniforms, trace=tr, grammar=grammar, forced=forced, tiles=tiles)
        if rows_per_pocket is not None:
            tokens = sample_stream(model, voc, per, B, max_length, example, None if prop is None else prop.to(dev).float(),
                                   rows_per_pocket, **common)
        else:
            tokens = sample(model, voc, per, B, max_length, example, rows_prop, **common)
        rec.update(tokens=tokens.cpu(), lengths=tr["lengths"].cpu(), sum_logp=tr["sum_logp"].cpu(), steps=tr["steps"], path=tr["path"])
    elif mode == "distinct":
        tokens = sample_distinct(model, voc, per, B, max_length, example, rows_prop, device=dev, temperature=temperature,
                                 suppress=("&", "^"), grammar=grammar, seed=seed, streams=streams, trace=tr, forced=forced, tiles=tiles)
        rec.update(tokens=tokens.cpu(), lengths=tr["lengths"].cpu(), sum_logp=tr["sum_logp"].cpu(), valid=tr["valid"].cpu(),
                   steps=tr["steps"])
    else:
        on_device = beam_select == "device" or grammar is not None
        if on_device:
            tokens = beam_search_device(model, voc, per, B, max_length, 1, example, rows_prop, device=dev, trace=tr, grammar=grammar,
                                        forced=forced, tiles=tiles)
        else:
            tokens = beam_search(model, voc, per, B, max_length, 1, example, rows_prop, device=dev, trace=tr, tiles=tiles)
        best = [max(h.beams, key=lambda x: x[0]) for h in tr["hyps"]]         # score = summed log-probability / len ** 0.7
        rec.update(per=1, tokens=tokens.cpu(), lengths=torch.tensor([len(h) for _, h in best], dtype=torch.int64),
                   sum_logp=torch.tensor([s * len(h) ** 0.7 for s, h in best], dtype=torch.float64),
                   steps=tr["steps"] if on_device else tr["last_beams"].shape[1] - 1, path=tr["path"], on_device=on_device)
    rec["pocket_of"] = [r // rec["per"] for r in range(rec["tokens"].shape[0])]
    return rec


def format_lines(rec, voc, names=None):
    """The four tab-separated columns gen.py writes, one line per row of a record (a distinct run's empty slots left out):
    pocket name (`names`, default the record's), the text between '&' and '$', the tokens decoded, the summed log-probability."""
    names = rec["names"] if names is None else names
    voc = list(voc)
    eos, pad = voc.index("$"), voc.index("^")
    lengths, logps = rec["lengths"].tolist(), rec["sum_logp"].tolist()
    keep = rec["valid"].bool().tolist() if "valid" in rec else None
    lines = []
    for r, row in enumerate(rec["tokens"].tolist()):
        if keep is not None and not keep[r]:
            continue
        if rec["mode"] == "score":
            text = rec["molecules"][r]
        else:
            body = []
            for t in (row[1:1 + lengths[r]] if rec["mode"] != "beam" else row[1:]):   # a sampled row is `lengths[r]` tokens long
                if t == eos or (t == pad and rec["mode"] == "beam"):
                    break
                body.append(voc[t])
            text = "".join(body)
        lines.append(f"{names[rec['pocket_of'][r]]}\t{text}\t{lengths[r]}\t{logps[r]:.6f}")
    return lines


# ---------------------------------------------------------------------------------------------------- a split, pass by pass
def ligand_strings(store, ids, voc):
    """The ligand of every graph `ids` of the pack as text: its `tok_tgt` row spelled with `voc` up to '$'."""
    voc = [str(v) for v in voc]
    eos = voc.index("$")
    out = []
    for row in np.asarray(store.arrays["tok_tgt"][np.asarray(ids, np.int64)]):
        row = row.tolist()
        out.append("".join(voc[t] for t in row[:row.index(eos) if eos in row else len(row)]))
    return out


def pass_bytes(model, store, ids, mode, rows_per_pocket, positions, two_buffers):
    """The bytes the decoder call of one pass holds at least: the key / value caches of its rows (`Sampling.cache_bytes`, both
    buffers where the rows exchange prefixes) and the encoder's outputs with their per-layer key / value projections, padded
    to the pass's largest pocket.  From the host copy of the pack's counts: nothing is launched."""
    from .model.Sampling import cache_bytes
    dec = model.model.decoder
    a = dec.layers[0].dec_self_attn
    B, atoms = len(ids), int(store.counts[np.asarray(ids, np.int64), 0].max())
    encoder = B * atoms * 4 * (a.hidden_channels + len(dec.layers) * (a.key_channels + a.hidden_channels))
    return (2 if two_buffers else 1) * cache_bytes(dec, B * rows_per_pocket, positions) + encoder


def generate_split(model, cfg, voc, store, split, mode, per, pockets_per_pass, *, first=None, prop=None, molecules=None,
                   max_length=None, seed=0, timings=False, **decoder):
    """A generator over the passes of `store.splits[split]` (its first `first` graphs): one record per pass, in split order.

    `store`: a `PackedDataset` after `.to(device)`, device resident or not.  `mode`, `per` and the keyword arguments `decoder`
    (temperature, top_k, top_p, grammar, prefix, rows_per_pocket, tiles, beam_select) as in `decode`.  `prop`: None (every
    property wanted: 1.0 each, gen.py's default), a sequence of num_props numbers (one prompt for every pocket) or "dataset"
    (`dataset_props`: each graph's own).  `molecules`: "dataset" in score mode, and only there - every graph's own ligand
    (`ligand_strings`) is scored for its pocket; `per` is not consulted.  `max_length`: default the decoder's tgt_len + 1, in
    score mode the pass's longest ligand + 2.  `seed`: of `pocket_uniforms` (sample) and of `sample_distinct`, whose `streams`
    are the graph ids mod 2^32.

    A record is `decode`'s plus `ids` (int64, the pass's graph ids) and `names` (`store.names[id]`); with `timings=True` also
    `seconds`: the wall time of `batch` (collate + prepare), `embed` (the protein pass of the embedding and the kNN list) and
    `decode` (the encoder and the decoder call), each ended by a device synchronisation.

    ValueError before any launch of a pass whose caches and encoder outputs (`pass_bytes`) exceed the device's free memory
    (torch.cuda.mem_get_info plus what torch's allocator holds unused): it names `pockets_per_pass`."""
    if mode not in MODES:
        raise ValueError(f"generate_split: mode is one of {MODES} (got {mode!r})")
    if molecules not in (None, "dataset") or (mode == "score") != (molecules == "dataset"):
        raise ValueError("generate_split: molecules='dataset' in score mode and only there (a file of molecules is gen.py's)")
    if store.device is None:
        raise ValueError("generate_split: the store is not on a device yet: PackedDataset.to(device) first")
    dev = store.device
    ids = split_ids(store, split, first)
    chunks = passes(ids, pockets_per_pass)
    tr = cfg.train
    num = 1 if tr.num_props else 0
    fixed = None
    if num and not (isinstance(prop, str) and prop == "dataset"):
        fixed = torch.tensor([[1.0] * tr.num_props if prop is None else [float(v) for v in prop]], dtype=torch.float32)
        if fixed.shape[1] != tr.num_props:
            raise ValueError(f"generate_split: prop holds {fixed.shape[1]} numbers, the model's prompt has {tr.num_props}")
    if mode != "score":
        max_length = max_length or cfg.model.decoder.tgt_len + 1
        if per < 1:
            raise ValueError(f"generate_split: per >= 1 (got {per})")
    R = decoder.get("rows_per_pocket")
    on_device = mode == "beam" and (decoder.get("beam_select", "host") == "device" or decoder.get("grammar") is not None)
    for chunk in chunks:
        B = len(chunk)
        mols, T = None, max_length
        if mode == "score":
            mols = [[m] for m in ligand_strings(store, chunk, voc)]
            T = max_length or max(len(smiles.tokenize(m[0], voc)) for m in mols) + 2
        rows = R if R is not None else 1 if mode == "score" else per
        positions = T + num if mode == "beam" and not on_device else T - 1 + num
        need = pass_bytes(model, store, chunk, mode, rows, positions, mode == "distinct" or on_device)
        free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
        if need > free:
            raise ValueError(f"generate_split: a pass of {B} pockets x {rows} rows x {positions} positions needs {need} bytes for its "
                             f"key / value caches and encoder outputs, {free} bytes are free on {dev}: lower pockets_per_pass "
                             f"(now {pockets_per_pass})")
        clock = _Clock(timings)
        batch = store.batch(chunk)
        ex, _ = pocket_example(model, cfg, batch, prepared=lambda: clock.lap("batch"))
        clock.lap("embed")
        p = fixed.repeat(B, 1) if fixed is not None else dataset_props(model, batch) if num else None
        rec = decode(model, voc, ex, B, mode, 1 if mode == "score" else per, p, max_length, device=dev, seed=seed,
                     uniforms=pocket_uniforms(seed, chunk, per, T, dev) if mode == "sample" else None,
                     streams=chunk % (1 << 32) if mode == "distinct" else None, molecules=mols, **decoder)
        clock.lap("decode")
        rec.update(ids=chunk, names=[store.names[int(i)] for i in chunk])
        if timings:
            rec["seconds"] = clock.laps
        yield rec


class _Clock:
    """Wall time between device synchronisations; does nothing when off."""

    def __init__(self, on):
        self.on, self.laps = on, {}
        if on:
            torch.cuda.synchronize()
            self.t = time.perf_counter()

    def lap(self, name):
        if self.on:
            torch.cuda.synchronize()
            now = time.perf_counter()
            self.laps[name], self.t = now - self.t, now
