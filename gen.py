#!/usr/bin/env python
"""Generation entrypoint, the counterpart of train.py for the reference's gen.py:156-196: embed the pockets with the
equivariant embedding in `gen_mode`, then decode SMILES token sequences conditioned on them - with the reference's beam
search (`--mode beam`, one sequence per pocket) or by sampling (`--mode sample`, `--num-samples` sequences per pocket with
temperature / top-k / top-p; singa_amd/model/Sampling.py).  `--mode distinct` samples WITHOUT replacement: `--num-samples`
pairwise distinct sequences per pocket (stochastic beam search; `--temperature`, `--grammar` and `--seed` apply, top-k / top-p
do not), best perturbed score first.

The reference's PDB / docking front end is out of scope, so pockets come from `--data golden` (the three
example graphs the reference bundles) or `--data synthetic`.  No chemistry toolkit is required: the sequences are written as
they were decoded, without a validity filter.  `--grammar smiles` (sample, distinct and beam mode) removes the syntactic rejects
where the token is chosen: every sequence then ends with '$' before `--max-length` and has balanced branches, paired
ring-closure digits and no dangling bond symbol (include/singa_hip_gen.h states the rule).  Under `--grammar smiles` chemical
validity - valence, aromaticity, duplicate ring bonds - is still not checked.  `--grammar valence` (sample and beam mode) adds a
bonding-capacity rule: no atom of a sequence carries more bond order than its token can (include/singa_hip_valence.h; a necessary
condition for validity - aromaticity and duplicate ring bonds stay unchecked).  Beam search selects on the host, as the
reference does, unless `--beam-select device` or a `--grammar` is given: then the selection runs on the device
(`beam_search_device`; include/singa_hip_beam.h states the rule), which is what lets a grammar constrain it; without a grammar
the two select the same hypotheses up to the order of exactly tied candidates.  `--prefix TEXT` starts every sequence with
that fragment - a scaffold to continue - in sample mode (with or without `--rows-per-pocket`), in distinct mode and in beam
mode with the selection on the device (include/singa_hip_prefix.h states the rule; host-selected beam search refuses it); under
a `--grammar` a fragment the rule refuses is an error before anything runs.
`--mode score --molecules FILE` draws nothing: FILE holds lines of `pocket name<TAB>SMILES`, and every molecule's
log-likelihood under the model for its pocket is written, in the same four columns and in the order of the input;
`--rows-per-pocket R` scores them on R rows per pocket (same numbers, the caches of R rows whatever the length of FILE).

    python gen.py --config ./config/train.yml --ckpt logs/.../checkpoints/100.pt --data golden --mode sample \\
                  --num-samples 100 --temperature 0.9 --top-p 0.95 --seed 1

    python gen.py --data golden --mode sample --num-samples 100 --grammar smiles --prefix "c1ccc("
    python gen.py --data golden --mode score --molecules library.tsv
    python gen.py --data golden --mode distinct --num-samples 100 --grammar smiles --seed 3
    python gen.py --data golden --mode distinct --num-samples 100 --grammar smiles --prefix "c1ccc("
    python gen.py --data golden --mode score --molecules library.tsv --rows-per-pocket 256
    python gen.py --data golden --mode beam --num-beams 20 --grammar valence

One line per sequence on stdout (or in `--out`), tab-separated: pocket name, the SMILES string between '&' and '$', the
number of tokens decoded ('$' included), the summed log-probability of the sequence under the model.  Everything else that
is printed starts with '#'.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    """The command line, parsed and checked: everything that can be refused before a device is touched."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default=os.path.join(ROOT, "config", "train.yml"))
    ap.add_argument("--ckpt", type=str, default=None, help="a train.py checkpoint; without it the weights are random")
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--data", choices=["golden", "synthetic"], default="golden")
    ap.add_argument("--pockets", type=int, default=3, help="number of pockets (synthetic data)")
    ap.add_argument("--lmax", type=int, default=None, help="override embedding.lmax_list (2, 3, 4 or 6)")
    ap.add_argument("--mode", choices=["beam", "sample", "score", "distinct"], default="sample")
    ap.add_argument("--num-samples", type=int, default=100, help="sequences per pocket (sample, distinct)")
    ap.add_argument("--num-beams", type=int, default=20, help="beams per pocket (beam); the best hypothesis is written")
    ap.add_argument("--max-length", type=int, default=None, help="default: model.decoder.tgt_len + 1")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--grammar", choices=["none", "smiles", "valence"], default="none",
                    help="sample, distinct, beam: choose only tokens that keep the sequence a completable SMILES string")
    ap.add_argument("--beam-select", choices=["host", "device"], default="host",
                    help="beam: where the candidates are selected; a --grammar selects on the device whatever this says")
    ap.add_argument("--rows-per-pocket", type=int, default=None, metavar="R",
                    help="sample, score: decode on R rows per pocket; a row that ends its sequence starts the pocket's next one "
                         "(sample_stream: same sequences and scores for the same uniforms, whatever R)")
    ap.add_argument("--decoder-tiles", action="store_true",
                    help="every mode: the row-tiled decoder step kernels (16 rows per workgroup, weights read once per tile, a "
                         "pocket of any size) instead of the one-row-per-workgroup ones")
    ap.add_argument("--prefix", type=str, default=None,
                    help="sample, distinct, beam (selected on the device): every sequence starts with this SMILES fragment")
    ap.add_argument("--molecules", type=str, default=None,
                    help="score: a file of lines `pocket name<TAB>SMILES` (further columns are ignored)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--prop", type=float, nargs=3, default=[1.0, 1.0, 1.0], metavar=("V", "Q", "S"),
                    help="the property prompt: vina score below -7.5, QED above 0.6, SAS below 4 (1 = wanted)")
    ap.add_argument("--out", type=str, default=None, help="write the sequences here instead of stdout")
    args = ap.parse_args(argv)
    assert args.device.startswith("cuda"), "the hot path is the HIP path: there is no CPU fallback"
    assert args.grammar == "none" or args.mode in ("sample", "distinct", "beam"), "--grammar constrains what is generated, not --mode score"
    assert args.grammar != "valence" or args.mode in ("sample", "beam"), \
        "--grammar valence: sample and beam mode only (distinct gathers one state word)"
    assert args.beam_select == "host" or args.mode == "beam", "--beam-select is about beam search: beam mode only"
    assert args.mode != "distinct" or (args.top_k == 0 and args.top_p == 1.0), "--mode distinct takes no --top-k / --top-p"
    if args.prefix is not None and args.mode == "score":
        ap.error("--prefix gives generated sequences their start: sample, distinct and beam mode, not --mode score")
    if args.prefix is not None and args.mode == "beam" and args.beam_select == "host" and args.grammar == "none":
        ap.error("--prefix in beam mode needs the selection on the device: add --beam-select device (or a --grammar); the "
                 "host-selected beam search takes no forced tokens")
    if args.rows_per_pocket is not None and args.mode not in ("sample", "score"):
        ap.error("--rows-per-pocket is continuous sampling: sample and score mode only")
    assert (args.mode == "score") == (args.molecules is not None), "--mode score reads its molecules from --molecules FILE"
    return args


def main():
    args = parse_args()
    dev = torch.device(args.device if ":" in args.device else "cuda:0")
    torch.cuda.set_device(dev)

    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import graph as G
    from singa_amd.config import Config, load_config
    from singa_amd.model.BeamSearch import beam_search, beam_search_device
    from singa_amd.model.CProMG import DenseMap, knn_graph
    from singa_amd.model.GAN import SINGA
    from singa_amd import smiles
    from singa_amd.model.Sampling import sample, sample_distinct, sample_stream, score

    cfg = load_config(args.config, lmax=args.lmax)
    torch.manual_seed(args.seed)
    model = SINGA(cfg, device=dev)
    if args.ckpt:
        model.load_state_dict(torch.load(args.ckpt, map_location=dev)["model"], strict=False)
        print(f"# weights from {args.ckpt}")
    else:
        print("# no --ckpt: random initial weights")
    model.eval()
    voc = list(cfg.model.decoder.smiVoc)
    eos, pad = voc.index("$"), voc.index("^")
    max_length = args.max_length or cfg.model.decoder.tgt_len + 1

    if args.data == "golden":
        names, graphs = list(G.EXAMPLE_NAMES), [G.example_graph(i) for i in range(len(G.EXAMPLE_NAMES))]
    else:
        names, graphs = [f"synthetic_{i}" for i in range(args.pockets)], [G.synthetic_graph(i) for i in range(args.pockets)]
    B = len(graphs)
    batch = G.collate(graphs).to(dev)
    model.prepare(batch)
    with torch.no_grad():                                                     # gen.py:157-160: the protein pass alone
        feat = model.embedding(batch, gen_mode=True)[G.PA].embedding.reshape(batch[G.PA]["x"].shape[0], -1)
    ex = Config()
    ids = batch[G.PA]["batch"]
    ex.protein_element_batch, ex.protein_atom_feature, ex.protein_pos = ids, feat, batch[G.PA]["pos"]
    ex.protein_atom_laplacian = batch[G.PA]["lap_pe"]
    knn = knn_graph(batch[G.PA]["pos"], cfg.model.encoder.knn, ids, B, DenseMap(ids, B))
    ex.protein_knn = knn[:, knn[0] >= 0]

    if args.mode == "score":
        wanted = [ln.rstrip("\n").split("\t")[:2] for ln in open(args.molecules) if ln.strip() and not ln.startswith("#")]
        assert wanted and all(len(w) == 2 and w[0] in names for w in wanted), \
            f"--molecules: every line is `pocket name<TAB>SMILES`, the pockets are {names}"
        mols = [[smi for name, smi in wanted if name == n] for n in names]
        grammar = None if args.grammar == "none" else args.grammar
        res = score(model, voc, mols, B, ex, torch.tensor([args.prop], dtype=torch.float32) if cfg.train.num_props else None,
                    device=dev, max_length=args.max_length, grammar=grammar, rows_per_pocket=args.rows_per_pocket, tiles=args.decoder_tiles)
        print(f"# scored {len(wanted)} molecules for {B} pockets")
        seen = {n: 0 for n in names}
        lines = []
        for name, smi in wanted:
            b, i = names.index(name), seen[name]
            seen[name] += 1
            lines.append(f"{name}\t{smi}\t{res['length'][b][i]}\t{res['sum_logp'][b][i]:.6f}")
        emit(args, lines)
        return

    per = args.num_samples if args.mode in ("sample", "distinct") else args.num_beams
    prop = torch.tensor([args.prop] * (B * per), dtype=torch.float32, device=dev) if cfg.train.num_props else None
    tr = {}
    forced = None if args.prefix is None else smiles.encode([args.prefix] * B, voc, max_length)
    if args.mode == "sample":
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        if args.rows_per_pocket is not None:
            tokens = sample_stream(model, voc, per, B, max_length, ex, None if prop is None else prop[:B], args.rows_per_pocket,
                                   device=dev, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
                                   suppress=("&", "^"), generator=gen, trace=tr,
                                   grammar=None if args.grammar == "none" else args.grammar, forced=forced,
                                   tiles=args.decoder_tiles).cpu()
        else:
            tokens = sample(model, voc, per, B, max_length, ex, prop, device=dev, temperature=args.temperature, top_k=args.top_k,
                            top_p=args.top_p, suppress=("&", "^"), generator=gen, trace=tr,
                            grammar=None if args.grammar == "none" else args.grammar, forced=forced, tiles=args.decoder_tiles).cpu()
        lengths, logps = tr["lengths"].cpu().tolist(), tr["sum_logp"].cpu().tolist()
        print(f"# sampled {per} sequences for each of {B} pockets: {tr['steps']} steps on the {tr['path']} path")
    elif args.mode == "distinct":
        tokens = sample_distinct(model, voc, per, B, max_length, ex, prop, device=dev, temperature=args.temperature,
                                 suppress=("&", "^"), grammar=None if args.grammar == "none" else args.grammar, seed=args.seed,
                                 trace=tr, forced=forced, tiles=args.decoder_tiles).cpu()
        keep = tr["valid"].cpu().bool()                                       # a small tree leaves trailing slots empty
        print(f"# {int(keep.sum())} distinct sequences for {B} pockets ({per} asked for each): {tr['steps']} steps")
        rows = [r for r in range(B * per) if keep[r]]
        tokens, names_of = tokens[keep], [names[r // per] for r in rows]
        lengths, logps = tr["lengths"].cpu()[keep].tolist(), tr["sum_logp"].cpu()[keep].tolist()
    else:
        if args.beam_select == "device" or args.grammar != "none":
            tokens = beam_search_device(model, voc, per, B, max_length, 1, ex, prop, device=dev, trace=tr,
                                        grammar=None if args.grammar == "none" else args.grammar, forced=forced,
                                        tiles=args.decoder_tiles).cpu()
            print(f"# beam search selected on the device: {tr['steps']} steps")
        else:
            tokens = beam_search(model, voc, per, B, max_length, 1, ex, prop, device=dev, trace=tr, tiles=args.decoder_tiles).cpu()
        best = [max(h.beams, key=lambda x: x[0]) for h in tr["hyps"]]         # score = summed log-probability / len ** 0.7
        lengths, logps = [len(h) for _, h in best], [s * len(h) ** 0.7 for s, h in best]
        per = 1

    if args.mode != "distinct":
        names_of = [names[r // per] for r in range(tokens.shape[0])]
    lines = []
    for r, row in enumerate(tokens.tolist()):
        body = []
        for t in (row[1:1 + lengths[r]] if args.mode != "beam" else row[1:]):     # a sampled row is `lengths[r]` tokens long
            if t == eos or (t == pad and args.mode == "beam"):
                break
            body.append(voc[t])
        lines.append(f"{names_of[r]}\t{''.join(body)}\t{lengths[r]}\t{logps[r]:.6f}")
    emit(args, lines)


def emit(args, lines):
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print(f"# {len(lines)} sequences written to {args.out}")
    else:
        print("\n".join(lines))


if __name__ == "__main__":
    main()
