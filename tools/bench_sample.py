#!/usr/bin/env python
"""Throughput of sampled generation (singa_amd/model/Sampling.py) in gen.py's configuration - one protein pocket of 200
atoms, property prompt, max_length = tgt_len + 1 = 201 - on a synthetic pocket with random-init weights, next to the beam
step of `tools/bench_beam.py` measured in the same process on the same pocket.

    python tools/bench_sample.py [--rows 128] [--max-length 201] [--reps 5] [--fused auto|k17|library] [--table] [--grammar] [--forced]
                                  [--distinct] [--rows-per-pocket R] [--valence] [--score-stream] [--tiles]

Prints one JSON line: rows, steps, ms per step, new tokens / s, sequences / s and the decoder path of the sampled run; the
20-row comparison (`at_20_rows`: medians of `--reps` full generations each, sampled and beam runs interleaved, both in ms
per step, and their ratio); with `--table` also both decoder paths at rows = 20, 128, 512, 2048 (the table `fused=None`
picks from, profiles/sampling/README.md); with `--grammar` also the k17 step under `grammar="smiles"` next to the plain one at
rows = 20, 128, 2048, both timed in this process, runs interleaved (`grammar_table`; '$' is then not suppressed - the grammar
needs it - but its logit keeps rows from ending before the budget forces them to: `steps` is reported); with `--forced` also
the k17 step with a forced prefix of 5 tokens next to the plain one at rows = 20, 2048, interleaved (`forced_table`), and
`score` on 2,048 molecules of 40 tokens for the pocket, timed as a whole call (`score_2048`: molecules / s).  A generation is timed
as a whole - encoder, cache set-up, graph capture and
every step - and divided by its steps, as bench_beam.py does.  With `--distinct` also `sample_distinct` (sampling without
replacement: expand, select and the cache move inside the step, two captured graphs) next to the plain k17 step at rows = 128,
512, 2048 for the one pocket, interleaved (`distinct_table`).  With `--rows-per-pocket R` nothing but continuous sampling
(`sample_stream`) is measured: `stream_table` - the streaming step (per-row positions, choice by molecule, hand-over) next to
the plain k17 step at rows = 128, 512, 2048 on the synthetic pocket, one molecule per row so that both run max_length - 1 steps,
interleaved - and `throughput` - on the `beam_b2_k6_eos` golden model (tests/golden; its rows end all over a 41-column
window), 4,096 molecules per pocket through `sample_stream(rows_per_pocket=R)` against `sample` called 16 times with 256 rows
per pocket, whole calls timed, with the length distribution of the run and the ratio it predicts: (steps until the longest
of 256 rows has ended, as the polling loop sees it) / (mean length).  With `--valence` nothing but the k17 step under
`grammar="valence"` next to the one under `grammar="smiles"` at rows = 128, 512, 2048, interleaved (`valence_table`).
With `--score-stream` nothing but forced tokens outside the lockstep sampler (include/singa_hip_prefix.h): `score_stream` - 2,048
molecules per pocket of ragged length, drawn once by `sample` from the `beam_b2_k6_eos` golden model, scored by `score` in chunks
of 256 molecules per pocket against `score(rows_per_pocket=256)`, whole calls timed, alternately, twice each, with the ratio of
step counts that predicts the gain - and `prefix_table`: `sample_distinct` and `beam_search_device` on the synthetic pocket with
a forced prefix of 5 tokens next to the same run without one, ms per step of whole generations, interleaved.
With `--tiles` nothing but the row-tiled decoder step (include/singa_hip_dec_tiles.h) next to k17: `tiles_table` - `sample` on
both paths at rows = 20, 128, 512, 2048 (5 / 5 / 3 / 3 whole generations each, as `--table` takes them), interleaved - and
`tiles_distinct` - `sample_distinct` at 2,048 rows on both paths, 3 generations each, interleaved.  Every run is listed.  With
`--tiles-only ROWS` nothing but two `sample(tiles=True)` generations of ROWS rows: the run to take a kernel trace of.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=128, help="samples drawn for the pocket in one call")
    ap.add_argument("--max-length", type=int, default=201)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--fused", choices=["auto", "k17", "library"], default="auto")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--table", action="store_true")
    ap.add_argument("--grammar", action="store_true", help="also time the grammar-constrained step (grammar_table)")
    ap.add_argument("--forced", action="store_true", help="also time the step with a forced prefix, and score() (forced_table)")
    ap.add_argument("--distinct", action="store_true", help="also time sample_distinct next to the plain step (distinct_table)")
    ap.add_argument("--distinct-only", type=int, default=0, metavar="ROWS",
                    help="nothing but two sample_distinct generations of ROWS slots: the run to take a kernel trace of")
    ap.add_argument("--valence", action="store_true",
                    help="nothing but the k17 step under grammar='valence' next to grammar='smiles' at rows = 128, 512, 2048 (valence_table)")
    ap.add_argument("--rows-per-pocket", type=int, default=0, metavar="R",
                    help="nothing but sample_stream: the streaming step next to the plain one, and molecules / s at R rows per pocket")
    ap.add_argument("--tiles", action="store_true",
                    help="nothing but the row-tiled decoder step next to k17: sample at rows = 20, 128, 512, 2048 and sample_distinct at "
                         "2048 (tiles_table, tiles_distinct)")
    ap.add_argument("--tiles-only", type=int, default=0, metavar="ROWS",
                    help="nothing but two sample(tiles=True) generations of ROWS rows: the run to take a kernel trace of")
    ap.add_argument("--score-stream", action="store_true",
                    help="nothing but score on a row budget against score in chunks, and the forced step of the two slot searches")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import graph as G
    from singa_amd.config import Config, load_config
    from singa_amd.model.BeamSearch import beam_search
    from singa_amd.model.CProMG import DenseMap, knn_graph
    from singa_amd.model.GAN import SINGA
    from singa_amd import smiles
    from singa_amd.model.Sampling import LIVE_POLL, sample, sample_distinct, sample_stream, score
    dev = torch.device("cuda", 0)
    cfg = load_config(lmax=2)
    torch.manual_seed(cfg.train.seed)
    model = SINGA(cfg, device=dev).eval()
    voc = list(cfg.model.decoder.smiVoc)
    with torch.no_grad():
        # as bench_beam.py: keep '$' from ending a run early, so that every run decodes max_length tokens
        model.model.decoder.layers[-1].pos_ffn.layer_norm.bias[0] = 10.0
        model.model.projection.weight[voc.index("$")] = 0.0
        model.model.projection.weight[voc.index("$"), 0] = -3.0
    b = G.collate([G.synthetic_graph(500)]).to(dev)
    model.prepare(b)
    with torch.no_grad():
        feat = model.embedding(b, gen_mode=True)[G.PA].embedding.reshape(b[G.PA]["x"].shape[0], -1)
    ex = Config()
    batch = b[G.PA]["batch"]
    ex.protein_element_batch, ex.protein_atom_feature, ex.protein_pos = batch, feat, b[G.PA]["pos"]
    ex.protein_atom_laplacian = b[G.PA]["lap_pe"]
    knn = knn_graph(b[G.PA]["pos"], cfg.model.encoder.knn, batch, 1, DenseMap(batch, 1))
    ex.protein_knn = knn[:, knn[0] >= 0]
    T = args.max_length
    gen = torch.Generator(device=dev).manual_seed(0)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        steps = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    def run_sample(rows, fused, grammar=None, forced=None, tiles=False):
        tr = {}
        prop = torch.ones(rows, 3, device=dev)
        sample(model, voc, rows, 1, T, ex, prop, device=dev, temperature=args.temperature, top_k=args.top_k, top_p=args.top_p,
               suppress=() if grammar else ("$",), generator=gen, fused=fused, trace=tr, grammar=grammar, forced=forced, tiles=tiles)
        run_sample.path = tr["path"]
        return tr["steps"]

    def run_beam():
        return beam_search(model, voc, 20, 1, T, 1, ex, torch.ones(20, 3, device=dev), device=dev).shape[1] - 1

    def entry(rows, ms):
        return {"rows": rows, "ms_per_step": round(ms, 4), "new_tokens_per_s": round(rows / ms * 1e3, 1),
                "sequences_per_s": round(rows / (ms * (T - 1)) * 1e3, 2)}

    if args.tiles_only:
        ms = [timed(lambda: run_sample(args.tiles_only, True, tiles=True)) for _ in range(2)]
        print(json.dumps({"tiles_only_rows": args.tiles_only, "path": run_sample.path, "ms_per_step": [round(x, 4) for x in ms]}))
        return
    if args.tiles:
        def both(fn, reps):
            """fn(tiles) -> steps: one warm-up each, then `reps` whole generations each, interleaved -> (k17 runs, tile runs) in ms per step"""
            fn(False), fn(True)
            k17, til = [], []
            for _ in range(reps):
                k17.append(timed(lambda: fn(False)))
                til.append(timed(lambda: fn(True)))
            return k17, til

        def row(rows, k17, til):
            return {"rows": rows, "k17_ms_per_step": round(statistics.median(k17), 4), "tiles_ms_per_step": round(statistics.median(til), 4),
                    "k17_runs_ms": [round(x, 4) for x in k17], "tiles_runs_ms": [round(x, 4) for x in til],
                    "tiles_faster": max(til) < min(k17), "k17_faster": max(k17) < min(til)}       # faster = the runs do not overlap

        def run_distinct(rows, tiles):
            tr = {}
            sample_distinct(model, voc, rows, 1, T, ex, torch.ones(rows, 3, device=dev), device=dev, temperature=args.temperature,
                            suppress=("$",), seed=rows, trace=tr, tiles=tiles)
            return tr["steps"]
        ttable = [row(rows, *both(lambda t: run_sample(rows, True, tiles=t), 3 if rows >= 512 else args.reps)) for rows in (20, 128, 512, 2048)]
        print(json.dumps({"max_length": T, "tiles_table": ttable,
                          "tiles_distinct": [row(2048, *both(lambda t: run_distinct(2048, t), 3))]}))
        return
    if args.score_stream:
        import numpy as np
        from singa_amd.model.BeamSearch import beam_search_device
        from tests.helpers import golden, smi_voc
        from tests.test_beam_gpu import build_model
        from tests.test_sampling_gpu import example_of
        z = golden("beam_b2_k6_eos.npz")
        gmodel, gex, gvoc, B, Tg = build_model(z)[0], example_of(z), smi_voc(), len(z["names"]), 41
        n, chunk, eos = 2048, 256, smi_voc().index("$")
        prop1 = torch.as_tensor(z["prop"][:1]).float()
        library = [[] for _ in range(B)]
        for c in range(n // chunk):                                            # the library: what the model itself draws
            tr = {}
            u = torch.rand(Tg, B * chunk, generator=torch.Generator().manual_seed(c))
            tok = sample(gmodel, gvoc, chunk, B, Tg, gex, prop1.repeat(B * chunk, 1).to(dev), device=dev, uniforms=u, fused=True,
                         trace=tr).cpu().numpy()
            ln = tr["lengths"].cpu().numpy()
            for r in range(B * chunk):
                body = tok[r, 1:1 + ln[r]]
                library[r // chunk].append([int(t) for t in body[body != eos]])
        tokens = np.array([len(m) + 1 for ms in library for m in ms]).reshape(B, n)       # scored columns, the '$' included
        got = {}

        def chunks():
            out = []
            for c in range(n // chunk):
                out.append(score(gmodel, gvoc, [ms[c * chunk:(c + 1) * chunk] for ms in library], B, gex, prop1, device=dev,
                                 max_length=Tg + 1, fused=True)["sum_logp"])
            got["chunks"] = [sum((o[b] for o in out), []) for b in range(B)]
            return 1

        def streamed():
            got["stream"] = score(gmodel, gvoc, library, B, gex, prop1, device=dev, max_length=Tg + 1, rows_per_pocket=chunk)["sum_logp"]
            return 1
        chunks(), streamed()
        assert got["chunks"] == got["stream"]                                  # the same floats, whatever the row budget
        t_chunks, t_stream = [], []
        for _ in range(2):
            t_chunks.append(timed(chunks) / 1e3)
            t_stream.append(timed(streamed) / 1e3)
        per_chunk = [int(-(-tokens[:, c * chunk:(c + 1) * chunk].max() // LIVE_POLL) * LIVE_POLL) for c in range(n // chunk)]
        sc, ss = statistics.median(t_chunks), statistics.median(t_stream)
        res = {"metric": "score_stream_molecules_per_s", "unit": "molecules/s", "value": round(B * n / ss, 1),
               "score_stream": {"model": "beam_b2_k6_eos", "pockets": B, "molecules_per_pocket": n, "max_length": Tg + 1,
                                "rows_per_pocket": chunk, "stream_seconds": [round(x, 4) for x in t_stream],
                                "score_8x256_seconds": [round(x, 4) for x in t_chunks],
                                "stream_molecules_per_s": round(B * n / ss, 1), "score_molecules_per_s": round(B * n / sc, 1),
                                "observed_ratio": round(sc / ss, 3),
                                "tokens": {"mean": round(float(tokens.mean()), 2), "min": int(tokens.min()), "max": int(tokens.max())},
                                "steps_per_256_row_call": per_chunk,
                                "predicted_ratio": round(statistics.mean(per_chunk) / float(tokens.mean()), 3)}}
        prefix = smiles.encode(["CCOCN"], voc, T)                               # 5 forced columns, then the free search

        def run_distinct(rows, forced):
            tr = {}
            sample_distinct(model, voc, rows, 1, T, ex, torch.ones(rows, 3, device=dev), device=dev, temperature=args.temperature,
                            suppress=("$",), seed=rows, trace=tr, forced=forced)
            return tr["steps"]

        def run_beam_device(rows, forced):
            tr = {}
            beam_search_device(model, voc, rows, 1, T, 1, ex, torch.ones(rows, 3, device=dev), device=dev, suppress=("$",), trace=tr,
                               forced=forced)
            return tr["steps"]
        ptable = []
        for name, fn, sizes in (("sample_distinct", run_distinct, (128, 2048)), ("beam_search_device", run_beam_device, (128, 1024))):
            for rows in sizes:
                fn(rows, None), fn(rows, prefix)
                plain, forc = [], []
                for _ in range(3):
                    plain.append(timed(lambda: fn(rows, None)))
                    forc.append(timed(lambda: fn(rows, prefix)))
                ptable.append({"mode": name, "rows": rows, "plain_ms_per_step": round(statistics.median(plain), 4),
                               "prefix_ms_per_step": round(statistics.median(forc), 4),
                               "plain_runs_ms": [round(x, 4) for x in plain], "prefix_runs_ms": [round(x, 4) for x in forc]})
        res["prefix_table"] = ptable
        print(json.dumps(res))
        return
    if args.distinct_only:
        rows = args.distinct_only
        ms = []
        for _ in range(2):
            tr = {}
            ms.append(timed(lambda: sample_distinct(model, voc, rows, 1, T, ex, torch.ones(rows, 3, device=dev), device=dev,
                                                    temperature=args.temperature, suppress=("$",), seed=rows, trace=tr) is None
                            or tr["steps"]))
        print(json.dumps({"distinct_only_rows": rows, "ms_per_step": [round(x, 4) for x in ms]}))
        return
    if args.valence:
        vtable = []
        for rows in (128, 512, 2048):
            run_sample(rows, True, "smiles"), run_sample(rows, True, "valence")
            gram, val, steps = [], [], {"smiles": [], "valence": []}
            for _ in range(3 if rows >= 512 else args.reps):
                for g, ms in (("smiles", gram), ("valence", val)):
                    ms.append(timed(lambda: steps[g].append(run_sample(rows, True, g)) or steps[g][-1]))
            vtable.append({"rows": rows, "path": "k17", "smiles_ms_per_step": round(statistics.median(gram), 4),
                           "valence_ms_per_step": round(statistics.median(val), 4), "steps": steps,
                           "smiles_runs_ms": [round(x, 4) for x in gram], "valence_runs_ms": [round(x, 4) for x in val]})
        print(json.dumps({"max_length": T, "valence_table": vtable}))
        return

    if args.rows_per_pocket:
        def run_stream(rows):
            tr = {}
            sample_stream(model, voc, rows, 1, T, ex, torch.ones(1, 3, device=dev), rows, device=dev, temperature=args.temperature,
                          top_k=args.top_k, top_p=args.top_p, suppress=("$",), generator=gen, trace=tr)
            return tr["steps"]
        stable = []
        for rows in (128, 512, 2048):
            run_sample(rows, True), run_stream(rows)
            plain, strm = [], []
            for _ in range(3 if rows >= 512 else args.reps):
                plain.append(timed(lambda: run_sample(rows, True)))
                strm.append(timed(lambda: run_stream(rows)))
            stable.append({"rows": rows, "path": "k17", "plain_ms_per_step": round(statistics.median(plain), 4),
                           "stream_ms_per_step": round(statistics.median(strm), 4),
                           "plain_runs_ms": [round(x, 4) for x in plain], "stream_runs_ms": [round(x, 4) for x in strm]})
        # molecules / s on the golden model whose rows end early
        import numpy as np
        from tests.helpers import golden, smi_voc
        from tests.test_beam_gpu import build_model
        from tests.test_sampling_gpu import example_of
        z = golden("beam_b2_k6_eos.npz")
        gmodel, gex, gvoc, B, Tg, R = build_model(z)[0], example_of(z), smi_voc(), len(z["names"]), 41, args.rows_per_pocket
        n, chunk = 4096, 256
        u = torch.rand(Tg, B * n, generator=torch.Generator().manual_seed(1))
        prop1 = torch.as_tensor(z["prop"][:1]).float()
        lengths = []

        def chunks():
            lengths.clear()
            for c in range(n // chunk):
                cols = torch.cat([torch.arange(b * n + c * chunk, b * n + (c + 1) * chunk) for b in range(B)])
                tr = {}
                sample(gmodel, gvoc, chunk, B, Tg, gex, prop1.repeat(B * chunk, 1).to(dev), device=dev, uniforms=u[:, cols], fused=True,
                       trace=tr)
                lengths.append(tr["lengths"].cpu().numpy())
            return 1

        def streamed():
            tr = {}
            sample_stream(gmodel, gvoc, n, B, Tg, gex, prop1.repeat(B, 1).to(dev), R, device=dev, uniforms=u, trace=tr)
            streamed.steps = tr["steps"]
            return 1
        chunks(), streamed()
        t_chunks, t_stream = [], []
        for _ in range(3):
            t_chunks.append(timed(chunks) / 1e3)
            t_stream.append(timed(streamed) / 1e3)
        per_chunk = [int(-(-l.max() // LIVE_POLL) * LIVE_POLL) for l in lengths]
        flat = np.concatenate(lengths)
        mean = float(flat.mean())
        sc, ss = statistics.median(t_chunks), statistics.median(t_stream)
        res = {"metric": "stream_molecules_per_s", "unit": "molecules/s", "value": round(B * n / ss, 1), "stream_table": stable,
               "throughput": {"model": "beam_b2_k6_eos", "pockets": B, "molecules_per_pocket": n, "max_length": Tg,
                              "rows_per_pocket": R, "stream_seconds": [round(x, 4) for x in t_stream], "stream_steps": streamed.steps,
                              "sample_16x256_seconds": [round(x, 4) for x in t_chunks],
                              "stream_molecules_per_s": round(B * n / ss, 1), "sample_molecules_per_s": round(B * n / sc, 1),
                              "observed_ratio": round(sc / ss, 3),
                              "lengths": {"mean": round(mean, 2), "min": int(flat.min()), "max": int(flat.max()),
                                          "deciles": [int(x) for x in np.percentile(flat, range(10, 100, 10))]},
                              "steps_per_256_row_call": per_chunk,
                              "predicted_ratio": round(statistics.mean(per_chunk) / mean, 3)}}
        print(json.dumps(res))
        return
    fused = {"auto": None, "k17": True, "library": False}[args.fused]
    run_beam(), run_sample(20, None), run_sample(args.rows, fused)           # warm-up: library initialisation, code objects
    beam_ms, samp_ms = [], []
    for _ in range(max(args.reps, 5)):                                        # interleaved: both see the same machine state
        beam_ms.append(timed(run_beam))
        samp_ms.append(timed(lambda: run_sample(20, None)))
    path20 = run_sample.path
    bm, sm = statistics.median(beam_ms), statistics.median(samp_ms)
    main_ms = statistics.median(timed(lambda: run_sample(args.rows, fused)) for _ in range(args.reps))
    res = {"metric": "sample_new_tokens_per_s", "unit": "tokens/s", "steps": T - 1, "path": run_sample.path}
    res.update(entry(args.rows, main_ms))
    res["value"] = res["new_tokens_per_s"]
    res["at_20_rows"] = {"sample_ms_per_step": round(sm, 4), "beam_ms_per_step": round(bm, 4), "sample_over_beam": round(sm / bm, 4),
                         "sample_path": path20, "generations_each": len(beam_ms),
                         "sample_runs_ms": [round(x, 4) for x in samp_ms], "beam_runs_ms": [round(x, 4) for x in beam_ms]}
    res["config"] = {"workload": "gen.py: 1 pocket (200 atoms), property prompt", "max_length": T, "temperature": args.temperature,
                     "top_k": args.top_k, "top_p": args.top_p, "launch": "hipGraph replay per step",
                     "fused_none_picks": "k17 at every row count"}
    if args.table:
        table = []
        for rows in (20, 128, 512, 2048):
            for name, f in (("k17", True), ("library", False)):
                run_sample(rows, f)
                ms = statistics.median(timed(lambda: run_sample(rows, f)) for _ in range(3 if rows >= 512 else args.reps))
                table.append(dict(entry(rows, ms), path=name))
        res["table"] = table
    if args.grammar:
        gtable = []
        for rows in (20, 128, 2048):
            run_sample(rows, True), run_sample(rows, True, "smiles")
            plain, gram, steps = [], [], []
            for _ in range(3 if rows >= 512 else args.reps):
                plain.append(timed(lambda: run_sample(rows, True)))
                gram.append(timed(lambda: steps.append(run_sample(rows, True, "smiles")) or steps[-1]))
            gtable.append({"rows": rows, "path": "k17", "plain_ms_per_step": round(statistics.median(plain), 4),
                           "grammar_ms_per_step": round(statistics.median(gram), 4), "grammar_steps": steps,
                           "plain_runs_ms": [round(x, 4) for x in plain], "grammar_runs_ms": [round(x, 4) for x in gram]})
        res["grammar_table"] = gtable
    if args.forced:
        ftable = []
        prefix = smiles.encode(["CCOCN"], voc, T)                               # 5 forced columns, then the free draw
        for rows in (20, 2048):
            run_sample(rows, True), run_sample(rows, True, forced=prefix)
            plain, forc = [], []
            for _ in range(3 if rows >= 512 else args.reps):
                plain.append(timed(lambda: run_sample(rows, True)))
                forc.append(timed(lambda: run_sample(rows, True, forced=prefix)))
            ftable.append({"rows": rows, "path": "k17", "plain_ms_per_step": round(statistics.median(plain), 4),
                           "forced_ms_per_step": round(statistics.median(forc), 4),
                           "plain_runs_ms": [round(x, 4) for x in plain], "forced_runs_ms": [round(x, 4) for x in forc]})
        res["forced_table"] = ftable
        mols = [["CCOCN" * 8] * 2048]                                            # 40 tokens each, '$' the 41st
        do_score = lambda: score(model, voc, mols, 1, ex, torch.ones(1, 3), device=dev, fused=True) and 1
        do_score()
        secs = [timed(do_score) / 1e3 for _ in range(3)]
        res["score_2048"] = {"molecules": 2048, "tokens_each": 40, "seconds": [round(x, 4) for x in secs],
                             "molecules_per_s": round(2048 / statistics.median(secs), 1)}
    if args.distinct:
        def run_distinct(rows):
            tr = {}
            sample_distinct(model, voc, rows, 1, T, ex, torch.ones(rows, 3, device=dev), device=dev, temperature=args.temperature,
                            suppress=("$",), seed=rows, trace=tr)
            return tr["steps"]
        dtable = []
        for rows in (128, 512, 2048):
            run_sample(rows, True), run_distinct(rows)
            plain, dist = [], []
            for _ in range(3 if rows >= 512 else args.reps):
                plain.append(timed(lambda: run_sample(rows, True)))
                dist.append(timed(lambda: run_distinct(rows)))
            dtable.append({"rows": rows, "path": "k17", "plain_ms_per_step": round(statistics.median(plain), 4),
                           "distinct_ms_per_step": round(statistics.median(dist), 4),
                           "plain_runs_ms": [round(x, 4) for x in plain], "distinct_runs_ms": [round(x, 4) for x in dist]})
        res["distinct_table"] = dtable
    print(json.dumps(res))


if __name__ == "__main__":
    main()
