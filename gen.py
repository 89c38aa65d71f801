#!/usr/bin/env python
"""Generation entrypoint, the counterpart of train.py for the reference's gen.py:156-196: embed the pockets with the
equivariant embedding in `gen_mode`, then decode SMILES token sequences conditioned on them - with the reference's beam
search (`--mode beam`, one sequence per pocket) or by sampling (`--mode sample`, `--num-samples` sequences per pocket with
temperature / top-k / top-p; singa_amd/model/Sampling.py).  `--mode distinct` samples WITHOUT replacement: `--num-samples`
pairwise distinct sequences per pocket (stochastic beam search; `--temperature`, `--grammar` and `--seed` apply, top-k / top-p
do not), best perturbed score first.

The reference's PDB / docking front end is out of scope, so pockets are graphs that are featurised already:
`--data golden` (the three example graphs the reference bundles), `--data synthetic`, or `--data packed --dataset DIR`, the
packed dataset train.py trains on (singa_amd/dataset.py, made by tools/pack_dataset.py).  A pack is run over split by split
(`--split`, default test; `--first N` pockets of it) in passes of `--pockets-per-pass` pockets, each pass one collate, one
encoding and one decoder call (singa_amd/generate.py); lines are written pass by pass in split order, named as the pack names
its graphs; `--prop-from-dataset` prompts every pocket with its own graph's property bits, and `--mode score --molecules
dataset` scores every graph's own ligand.  A pocket's random numbers are a function of `--seed` and its graph id, not of the
pass it falls into.  No chemistry toolkit is required: the sequences are written as
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
    python gen.py --ckpt 100.pt --data packed --dataset packs/crossdocked --split test --mode sample --num-samples 100 \\
                  --grammar smiles --prop-from-dataset --out test_samples.tsv
    python gen.py --ckpt 100.pt --data packed --dataset packs/crossdocked --mode score --molecules dataset

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
    ap.add_argument("--data", choices=["golden", "synthetic", "packed"], default="golden")
    ap.add_argument("--pockets", type=int, default=None, help="number of pockets (synthetic data; default 3)")
    ap.add_argument("--dataset", type=str, default=None, help="--data packed: directory of a packed dataset (tools/pack_dataset.py)")
    ap.add_argument("--split", choices=["train", "val", "test"], default=None, help="--data packed: the split to run over (default test)")
    ap.add_argument("--first", type=int, default=None, metavar="N", help="--data packed: only the first N pockets of the split")
    ap.add_argument("--pockets-per-pass", type=int, default=None, metavar="P",
                    help="--data packed: pockets encoded and decoded together; default: the largest P with P x rows per pocket "
                         "<= 2048 (rows per pocket: --rows-per-pocket, else --num-samples or --num-beams, 1 in score mode)")
    ap.add_argument("--prop-from-dataset", action="store_true",
                    help="--data packed: every pocket's property prompt is the one training gives its graph, instead of --prop")
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
                    help="score: a file of lines `pocket name<TAB>SMILES` (further columns are ignored); with --data packed the "
                         "word `dataset`: every graph's own ligand is scored for its pocket")
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
    if args.data == "packed":
        if args.dataset is None:
            ap.error("--data packed reads its pockets from a pack: add --dataset DIR")
        if args.pockets is not None:
            ap.error("--pockets counts synthetic pockets; with --data packed use --split and --first")
        if args.first is not None and args.first < 1:
            ap.error("--first N: at least 1")
        if args.pockets_per_pass is not None and args.pockets_per_pass < 1:
            ap.error("--pockets-per-pass P: at least 1")
        if args.mode == "score" and args.molecules != "dataset":
            ap.error("--data packed scores every graph's own ligand: --molecules dataset (a file names the bundled pockets only)")
        args.split = args.split or "test"
        if args.pockets_per_pass is None:
            rows = args.rows_per_pocket or (1 if args.mode == "score" else args.num_beams if args.mode == "beam" else args.num_samples)
            args.pockets_per_pass = max(1, 2048 // max(1, rows))
    else:
        given = [flag for flag, on in (("--dataset", args.dataset is not None), ("--split", args.split is not None),
                                       ("--first", args.first is not None), ("--pockets-per-pass", args.pockets_per_pass is not None),
                                       ("--prop-from-dataset", args.prop_from_dataset),
                                       ("--molecules dataset", args.molecules == "dataset")) if on]
        if given:
            ap.error(f"{', '.join(given)}: only with --data packed")
        args.pockets = 3 if args.pockets is None else args.pockets
    return args


def main():
    args = parse_args()
    dev = torch.device(args.device if ":" in args.device else "cuda:0")
    torch.cuda.set_device(dev)

    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import generate as GEN
    from singa_amd import graph as G
    from singa_amd.config import load_config
    from singa_amd.model.GAN import SINGA

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
    max_length = args.max_length or cfg.model.decoder.tgt_len + 1
    per = args.num_samples if args.mode in ("sample", "distinct") else args.num_beams
    decoder = dict(temperature=args.temperature, top_k=args.top_k, top_p=args.top_p, grammar=None if args.grammar == "none" else args.grammar,
                   prefix=args.prefix, rows_per_pocket=args.rows_per_pocket, tiles=args.decoder_tiles, beam_select=args.beam_select)
    out = Output(args.out)

    if args.data == "packed":
        from singa_amd.dataset import PackedDataset
        store = PackedDataset.load(args.dataset).to(dev)
        print(f"# packed dataset {args.dataset}: {store.G} graphs, split {args.split}")
        for k, rec in enumerate(GEN.generate_split(model, cfg, voc, store, args.split, args.mode, per, args.pockets_per_pass,
                                                   first=args.first, prop="dataset" if args.prop_from_dataset else args.prop,
                                                   molecules=args.molecules, max_length=args.max_length, seed=args.seed, **decoder)):
            print(f"# pass {k}: {len(rec['names'])} pockets ({rec['names'][0]} .. {rec['names'][-1]}), {args.mode} mode, "
                  + (f"{rec['steps']} steps" if rec["steps"] is not None else f"{len(rec['molecules'])} molecules scored"))
            out.write(GEN.format_lines(rec, voc))
        out.close()
        return

    if args.data == "golden":
        names, graphs = list(G.EXAMPLE_NAMES), [G.example_graph(i) for i in range(len(G.EXAMPLE_NAMES))]
    else:
        names, graphs = [f"synthetic_{i}" for i in range(args.pockets)], [G.synthetic_graph(i) for i in range(args.pockets)]
    ex, B = GEN.pocket_example(model, cfg, G.collate(graphs).to(dev))
    prop = torch.tensor([args.prop] * B, dtype=torch.float32, device=dev) if cfg.train.num_props else None

    if args.mode == "score":
        wanted = [ln.rstrip("\n").split("\t")[:2] for ln in open(args.molecules) if ln.strip() and not ln.startswith("#")]
        assert wanted and all(len(w) == 2 and w[0] in names for w in wanted), \
            f"--molecules: every line is `pocket name<TAB>SMILES`, the pockets are {names}"
        mols = [[smi for name, smi in wanted if name == n] for n in names]
        rec = GEN.decode(model, voc, ex, B, "score", 1, prop, args.max_length, device=dev, molecules=mols, **decoder)
        print(f"# scored {len(wanted)} molecules for {B} pockets")
        by_row = GEN.format_lines(rec, voc, names)                            # pocket-major; written in the order of the input
        first_row, seen = [sum(len(m) for m in mols[:b]) for b in range(B)], {n: 0 for n in names}
        lines = []
        for name, _ in wanted:
            lines.append(by_row[first_row[names.index(name)] + seen[name]])
            seen[name] += 1
        out.write(lines)
        out.close()
        return

    rec = GEN.decode(model, voc, ex, B, args.mode, per, prop, max_length, device=dev, seed=args.seed,
                     generator=torch.Generator(device=dev).manual_seed(args.seed) if args.mode == "sample" else None, **decoder)
    if args.mode == "sample":
        print(f"# sampled {per} sequences for each of {B} pockets: {rec['steps']} steps on the {rec['path']} path")
    elif args.mode == "distinct":
        print(f"# {int(rec['valid'].sum())} distinct sequences for {B} pockets ({per} asked for each): {rec['steps']} steps")
    elif rec["on_device"]:
        print(f"# beam search selected on the device: {rec['steps']} steps")
    out.write(GEN.format_lines(rec, voc, names))
    out.close()


class Output:
    """The sequence lines: on stdout, or in `path`, opened once and written pass by pass."""

    def __init__(self, path):
        self.path, self.n = path, 0
        self.f = open(path, "w") if path else None

    def write(self, lines):
        self.n += len(lines)
        if lines:
            print("\n".join(lines), file=self.f or sys.stdout)

    def close(self):
        if self.f:
            self.f.close()
            print(f"# {self.n} sequences written to {self.path}")


if __name__ == "__main__":
    main()
