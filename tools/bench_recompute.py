#!/usr/bin/env python
"""What `SINGA(..., recompute=True)` costs and saves, on the GPU only, for BASELINE configs[2] (cfg3_b128_l4) and the 64-graph
share of configs[4] (cfg5_l6), both built as bench.py builds them (bucketed HIP-graph replay over `--distinct-batches` resident
batches whose Laplacian encodings are recomputed inside the step).

  steps    per workload, the flag off and on ALTERNATED (off, on, off, on, ... `--rounds` times, a fresh model / engine each
           time, released before the next): median replayed step time of `--steps` steps (device events, bench.timed_region)
           and the peak allocated / reserved memory of that engine's life.  One JSON line per (workload, round, mode) and a
           summary line per workload: medians over the rounds, the spread (min .. max of the round medians) and the
           on / off differences.
  kernels  per workload's node count N (protein + ligand atoms of one batch) and L, per launch (a device-event pair around
           every launch, warm, `--launches` of them, median): singa_so3_skinny_expand (the default matrix-core form) and
           singa_s2act_sep_fwd on its result - the two launches a recomputing feed-forward block repeats in its backward pass.
           (profiles/recompute/kernels_fused_candidate.jsonl holds the same figures beside those of a fused kernel that was
           measured for this place and not kept.)

    python tools/bench_recompute.py [--part steps|kernels|all] [--workloads cfg3_b128_l4,cfg5_l6] [--out FILE.jsonl]

Prints JSON lines (and appends them to --out).
"""
import argparse
import gc
import hashlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as f:
            f.write(line + "\n")


def make_batches(workload, count, dev):
    """bench.run_workload's batches of one GPU: `count` different batches of the workload's graphs, resident on the device,
    their Laplacian encodings left to the step."""
    from singa_amd import graph as G
    L, kw, ids, n_parent = G.resolve_workload(workload)
    out = [G.synthetic_batch(len(ids), ids=[i + k * n_parent for i in ids], with_lap=False, **kw).to(dev) for k in range(count)]
    for b in out:
        b.extras["lap_pe_in_step"] = True
    return L, out


def run_steps(workload, recompute, batches, L, args, dev):
    import bench
    from singa_amd.config import load_config
    from singa_amd.engine import TrainStep
    from singa_amd.model.GAN import SINGA
    from singa_amd.optim import Adam
    cfg = load_config(lmax=L)
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.manual_seed(cfg.train.seed)
    model = SINGA(cfg, device=dev, recompute=recompute)
    model.train()
    opt = Adam(model.parameters(), lr=cfg.train.optimizer.lr, betas=(cfg.train.optimizer.beta1, cfg.train.optimizer.beta2))
    engine = TrainStep(model, opt, None, use_graph=True, max_grad_norm=float(cfg.train.max_grad_norm), bucket=True,
                       growth=args.growth, max_cached=6)
    t0 = time.perf_counter()
    for i in range(max(args.warmup, len(batches))):               # every batch once: all captures exist before the timed region
        engine.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    warm_s = time.perf_counter() - t0
    captures = engine.captures
    elapsed, per_step, loss, _ = bench.timed_region(engine, batches, args.steps, False, dev, True)
    rec = {"kind": "steps", "workload": workload, "recompute": bool(recompute), "steps": args.steps,
           "ms_per_step_median": round(bench.median(per_step), 3), "ms_per_step_mean": round(1e3 * elapsed / args.steps, 3),
           "ms_per_step_min": round(min(per_step), 3), "ms_per_step_max": round(max(per_step), 3),
           "peak_allocated_gb": round(torch.cuda.max_memory_allocated(dev) / 1e9, 2),
           "peak_reserved_gb": round(torch.cuda.max_memory_reserved(dev) / 1e9, 2),
           "resident_before_gb": round(base / 1e9, 2), "final_loss": round(float(loss.detach()), 6),
           "captures": engine.captures, "captures_in_timed_region": engine.captures - captures, "warmup_s": round(warm_s, 1)}
    engine.release()
    del engine, opt, model, loss
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def steps_part(args, dev):
    for workload in args.workloads:
        t0 = time.perf_counter()
        L, batches = make_batches(workload, args.distinct_batches, dev)
        torch.cuda.synchronize()
        from singa_amd import graph as G
        atoms = int(batches[0][G.PA]["x"].shape[0] + batches[0][G.LA]["x"].shape[0])
        runs = {False: [], True: []}
        for rnd in range(args.rounds):
            for mode in (False, True):
                rec = run_steps(workload, mode, batches, L, args, dev)
                rec.update(round=rnd, lmax=L, atoms=atoms)
                runs[mode].append(rec)
                emit(rec, args.out)
        med = lambda mode, key: statistics.median(r[key] for r in runs[mode])
        spread = lambda mode: [min(r["ms_per_step_median"] for r in runs[mode]), max(r["ms_per_step_median"] for r in runs[mode])]
        off, on = med(False, "ms_per_step_median"), med(True, "ms_per_step_median")
        emit({"kind": "steps_summary", "workload": workload, "lmax": L, "atoms": atoms, "rounds": args.rounds,
              "off_ms": off, "on_ms": on, "off_spread_ms": spread(False), "on_spread_ms": spread(True),
              "cost_ms": round(on - off, 3), "cost_pct": round(100.0 * (on - off) / off, 2),
              "off_peak_allocated_gb": med(False, "peak_allocated_gb"), "on_peak_allocated_gb": med(True, "peak_allocated_gb"),
              "off_peak_reserved_gb": med(False, "peak_reserved_gb"), "on_peak_reserved_gb": med(True, "peak_reserved_gb"),
              "saved_allocated_gb": round(med(False, "peak_allocated_gb") - med(True, "peak_allocated_gb"), 2),
              "saved_reserved_gb": round(med(False, "peak_reserved_gb") - med(True, "peak_reserved_gb"), 2),
              "same_loss": all(r["final_loss"] == runs[False][0]["final_loss"] for r in runs[False] + runs[True]),
              "wall_s": round(time.perf_counter() - t0, 1)}, args.out)
        del batches
        gc.collect()
        torch.cuda.empty_cache()


def per_launch_ms(fn, launches, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    pairs = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        pairs.append((a, b))
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in pairs)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(ts[0], 4), "p90_ms": round(ts[int(0.9 * (len(ts) - 1))], 4)}


def kernels_part(args, dev):
    from singa_amd import _capi, _lib, graph as G, ops
    lib = _lib.lib()
    for workload in args.workloads:
        L, kw, ids, _ = G.resolve_workload(workload)
        N = sum(s["n_protein"] + s["n_ligand"] for s in (G.graph_sizes(i, **kw) for i in ids))
        K, C = (L + 1) ** 2, 512
        g = torch.Generator(device="cpu").manual_seed(L)
        x = torch.randn(N, K, 16, generator=g).to(dev)
        w1 = (torch.randn(L + 1, C, 16, generator=g) * 0.25).to(dev)
        b1 = torch.randn(C, generator=g).to(dev)
        gate = torch.randn(N, C, generator=g).to(dev)
        ops._dev(x)
        P, Q, A = ops._grid_factors(L, L, False, x.device)
        h, a = torch.empty(N, K, C, device=dev), torch.empty(N, K, C, device=dev)
        st = ops._stream()
        p = ops._p
        seg, n = _capi.segs([(h.data_ptr(), K * C, K)])

        def chk(code):
            assert code == 0, lib.singa_last_error_string()
        expand = lambda: chk(lib.singa_so3_skinny_expand(p(x), p(w1), C * 16, 16, 1, p(b1), p(h), N, C, L, st))
        s2act = lambda: chk(lib.singa_s2act_sep_fwd(seg, n, p(gate), C, p(P), p(Q), p(A), p(a), N, C, L, st))
        rec = {"kind": "kernels", "workload": workload, "N": N, "lmax": L, "launches": args.launches,
               "tensor_gb": round(N * K * C * 4 / 1e9, 3)}
        for name, fn in (("expand", expand), ("s2act_fwd", s2act)):
            rec[name] = per_launch_ms(fn, args.launches)
        rec.update(two_launches_ms=round(rec["expand"]["median_ms"] + rec["s2act_fwd"]["median_ms"], 4))
        emit(rec, args.out)
        del x, w1, b1, gate, h, a
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["steps", "kernels", "all"], default="all")
    ap.add_argument("--workloads", default="cfg3_b128_l4,cfg5_l6")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--distinct-batches", type=int, default=3)
    ap.add_argument("--growth", type=float, default=1.04)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.workloads = [w for w in args.workloads.split(",") if w]
    assert args.launches >= 50, "per-launch medians over at least 50 launches"
    import __graft_entry__
    __graft_entry__.build()
    assert torch.cuda.is_available(), "bench_recompute needs a GPU"
    dev = torch.device("cuda", 0)
    with open(__graft_entry__.LIB, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:16]
    emit({"kind": "run", "device": torch.cuda.get_device_name(0), "lib_sha256": sha, "part": args.part,
          "distinct_batches": args.distinct_batches, "growth": args.growth}, args.out)
    if args.part in ("kernels", "all"):
        kernels_part(args, dev)
    if args.part in ("steps", "all"):
        steps_part(args, dev)


if __name__ == "__main__":
    main()
