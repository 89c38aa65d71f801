#!/usr/bin/env python
"""The cost ladder over the degree: one replayed training step of the same ragged config-3-shaped batch at every degree built.

    python tools/bench_lmax.py [--graphs 128] [--degrees 2 3 4 6] [--runs 3] [--steps 10] [--warmup 3]
                               [--recompute] [--lib PATH] [--label NAME] [--out FILE.jsonl]

The batch is the first `--graphs` graphs of the cfg3_b128_l4 workload's generator (singa_amd.graph: ragged protein and ligand
sizes), the same graphs at every degree; only `embedding.lmax_list` changes.  Per run and degree: a fresh model (seeded), the
step captured after `--warmup` calls (TrainStep, one capture, the same resident batch), then `--steps` replays timed with
device events.  The runs are alternated - degree after degree, then the next run - so that a drift of the machine falls on
all degrees alike.  One JSON line per (run, degree): median / min ms per step and the peak allocated memory of that build;
then one summary line per degree.  --lib: another build of libsinga_hip.so (the parent commit's, a tuning variant) under the
same Python, for comparisons kernel against kernel."""
import argparse
import gc
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def median(xs):
    xs = sorted(xs)
    return 0.5 * (xs[(len(xs) - 1) // 2] + xs[len(xs) // 2])


def one(L, batch, args, dev):
    import torch
    from singa_amd.config import load_config
    from singa_amd.engine import TrainStep
    from singa_amd.model import EF_layers
    from singa_amd.model.GAN import SINGA
    from singa_amd.optim import Adam
    cfg = load_config(lmax=L)
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    torch.manual_seed(cfg.train.seed)
    model = SINGA(cfg, device=dev, recompute=args.recompute).train()
    opt = Adam(model.parameters(), lr=cfg.train.optimizer.lr, betas=(cfg.train.optimizer.beta1, cfg.train.optimizer.beta2))
    eng = TrainStep(model, opt, None, use_graph=True, max_grad_norm=float(cfg.train.max_grad_norm))
    try:
        for _ in range(max(2, args.warmup)):
            eng.step(batch)
        torch.cuda.synchronize()
        captures = eng.captures
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        marks[0].record()
        for i in range(args.steps):
            loss = eng.step(batch)
            marks[i + 1].record()
        torch.cuda.synchronize()
        assert eng.captures == captures, "the timed steps re-captured"
        per = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
        res = {"lmax": L, "ms_per_step": round(median(per), 3), "ms_min": round(min(per), 3), "ms_max": round(max(per), 3),
               "peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2),
               "peak_reserved_gb": round(torch.cuda.max_memory_reserved(dev) / 1e9, 2), "loss": round(float(loss.detach()), 6)}
    finally:
        eng.release()
        EF_layers._edge_cache.clear()
        EF_layers._edge_pinned.clear()
        del eng, opt, model
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--graphs", type=int, default=128)
    ap.add_argument("--degrees", type=int, nargs="+", default=[2, 3, 4, 6])
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--recompute", action="store_true")
    ap.add_argument("--lib", default=None, help="another build of libsinga_hip.so to load instead of the tree's own")
    ap.add_argument("--label", default="this")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file as well")
    args = ap.parse_args()

    import torch
    from singa_amd import _lib, graph as G
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    else:
        import __graft_entry__
        __graft_entry__.build()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _, kw, ids, _ = G.resolve_workload("cfg3_b128_l4")
    assert args.graphs <= len(ids)
    batch = G.synthetic_batch(args.graphs, ids=ids[:args.graphs], with_lap=False, **kw).to(dev)
    sizes = dict(zip(("protein_atoms", "ligand_atoms", "e_pp", "e_ll", "e_x"), G.batch_sizes(batch)))
    head = {"label": args.label, "graphs": args.graphs, "recompute": bool(args.recompute), "steps": args.steps,
            "lib": args.lib or "singa_amd/lib/libsinga_hip.so", "device": torch.cuda.get_device_name(dev), **sizes}

    def emit(d):
        line = json.dumps(d)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    emit({"kind": "setup", **head})
    rows = {L: [] for L in args.degrees}
    for run in range(args.runs):
        for L in args.degrees:
            r = one(L, batch, args, dev)
            rows[L].append(r)
            emit({"kind": "run", "label": args.label, "run": run, **r})
    for L in args.degrees:
        ms = [r["ms_per_step"] for r in rows[L]]
        emit({"kind": "summary", "label": args.label, "lmax": L, "graphs": args.graphs, "ms_per_step": round(median(ms), 3),
              "ms_runs": ms, "spread_pct": round(100.0 * (max(ms) - min(ms)) / median(ms), 2),
              "peak_allocated_gb": max(r["peak_allocated_gb"] for r in rows[L])})


if __name__ == "__main__":
    main()
