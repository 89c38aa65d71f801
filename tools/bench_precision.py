#!/usr/bin/env python
"""What `SINGA(..., precision="bf16")` and `SINGA(..., embedding_precision="bf16")` change in time, on the GPU only.

  steps    BASELINE configs[2] (cfg3_b128_l4) built as bench.py builds it (bucketed HIP-graph replay over `--distinct-batches`
           resident batches), the flag off and on ALTERNATED (off, on, off, on, ... `--rounds` times, a fresh model / engine
           each time): median replayed step time of `--steps` steps.  One JSON line per (round, mode) and a summary line: the
           medians over the rounds, their spread (min .. max of the round medians) and the difference.
  kernels  every real GEMM launch one step of the workload makes under the flag, recorded from the model itself (ops._gemm
           wrapped for one eager step) and timed where it is made, on its own operands: singa_gemm_f32 against singa_gemm_bf16
           per launch (a device-event pair around every launch, warm, `--launches` of them, median).  One line per distinct
           launch with its count per step, one per shape class - operand form x tile shape - with the class's time per step
           in both kernels.  This is the figure a routing table in ops._gemm would be built from.  The complex launches
           (ops._cgemm: the m > 0 blocks of the SO(2) convolutions under --embedding-precision bf16) are recorded and timed the
           same way through singa_cgemm3m_f32 and singa_cgemm_bf16; their tile is 128 rows x 64 complex columns.

  --embedding-precision bf16 switches the embedding's SO(2) convolutions as well (both parts); --settings P/E,P/E,... alternates
  the steps part over (precision, embedding precision) pairs instead of over --precisions.

    python tools/bench_precision.py [--part steps|kernels|all] [--workload cfg3_b128_l4] [--embedding-precision bf16] [--out FILE.jsonl]
"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_recompute import emit, make_batches, per_launch_ms  # noqa: E402


def run_steps(workload, precision, batches, L, args, dev, embedding_precision="f32"):
    import gc
    import bench
    from singa_amd.config import load_config
    from singa_amd.engine import TrainStep
    from singa_amd.model.GAN import SINGA
    from singa_amd.optim import Adam
    cfg = load_config(lmax=L)
    gc.collect()
    torch.cuda.empty_cache()
    torch.manual_seed(cfg.train.seed)
    model = SINGA(cfg, device=dev, precision=precision, embedding_precision=embedding_precision)
    model.train()
    opt = Adam(model.parameters(), lr=cfg.train.optimizer.lr, betas=(cfg.train.optimizer.beta1, cfg.train.optimizer.beta2))
    engine = TrainStep(model, opt, None, use_graph=True, max_grad_norm=float(cfg.train.max_grad_norm), bucket=True,
                       growth=args.growth, max_cached=6)
    for i in range(max(args.warmup, len(batches))):               # every batch once: all captures exist before the timed region
        engine.step(batches[i % len(batches)])
    torch.cuda.synchronize()
    elapsed, per_step, loss, _ = bench.timed_region(engine, batches, args.steps, False, dev, True)
    rec = {"kind": "steps", "workload": workload, "precision": precision, "embedding_precision": embedding_precision, "steps": args.steps,
           "ms_per_step_median": round(bench.median(per_step), 3), "ms_per_step_min": round(min(per_step), 3),
           "ms_per_step_max": round(max(per_step), 3), "final_loss": round(float(loss.detach()), 6)}
    engine.release()
    del engine, opt, model, loss
    gc.collect()
    torch.cuda.empty_cache()
    return rec


def steps_part(args, dev):
    L, batches = make_batches(args.workload, args.distinct_batches, dev)
    t0 = time.perf_counter()
    if args.settings:                         # (precision, embedding precision) pairs, alternated
        runs = {s: [] for s in args.settings}
        for rnd in range(args.rounds):
            for s in args.settings:
                rec = run_steps(args.workload, s[0], batches, L, args, dev, s[1])
                rec.update(round=rnd)
                runs[s].append(rec)
                emit(rec, args.out)
        base = statistics.median(r["ms_per_step_median"] for r in runs[args.settings[0]])
        for s in args.settings:
            meds = [r["ms_per_step_median"] for r in runs[s]]
            emit({"kind": "settings_summary", "workload": args.workload, "rounds": args.rounds, "precision": s[0],
                  "embedding_precision": s[1], "ms": statistics.median(meds), "spread_ms": [min(meds), max(meds)],
                  "diff_ms_against_first": round(statistics.median(meds) - base, 3),
                  "diff_pct_against_first": round(100.0 * (statistics.median(meds) - base) / base, 2),
                  "wall_s": round(time.perf_counter() - t0, 1)}, args.out)
        return
    runs = {p: [] for p in args.precisions}
    for rnd in range(args.rounds):
        for precision in args.precisions:
            rec = run_steps(args.workload, precision, batches, L, args, dev, args.embedding_precision)
            rec.update(round=rnd)
            runs[precision].append(rec)
            emit(rec, args.out)
    if len(runs) < 2:                         # one mode alone (a profiler's run): no comparison
        return
    med = {p: statistics.median(r["ms_per_step_median"] for r in runs[p]) for p in runs}
    spread = {p: [min(r["ms_per_step_median"] for r in runs[p]), max(r["ms_per_step_median"] for r in runs[p])] for p in runs}
    emit({"kind": "steps_summary", "workload": args.workload, "rounds": args.rounds, "f32_ms": med["f32"], "bf16_ms": med["bf16"],
          "f32_spread_ms": spread["f32"], "bf16_spread_ms": spread["bf16"], "diff_ms": round(med["bf16"] - med["f32"], 3),
          "diff_pct": round(100.0 * (med["bf16"] - med["f32"]) / med["f32"], 2), "wall_s": round(time.perf_counter() - t0, 1)}, args.out)


TILES = {0: "128x128", 1: "128x32", 2: "32x128", 3: "64x64"}
FORMS = {(True, True): "forward (1,1)", (True, False): "dX (1,0)", (False, False): "dW (0,0)"}


def tile_shape(items, splits):
    """singa_gemm_f32's selection rule (gemm_launch in singa_amd/csrc/singa_hip.hip)."""
    imax, jmax = max(it["I"] for it in items), max(it["J"] for it in items)
    if jmax <= 32:
        return 1
    if imax <= 32:
        return 2
    t128 = sum(-(-it["I"] // 128) * -(-it["J"] // 128) for it in items)
    return 3 if t128 * splits < 384 or (imax <= 64 and jmax <= 64) else 0


def kernels_part(args, dev):
    """Every real GEMM launch that one training step of the workload makes under precision="bf16", timed where it is made:
    ops._gemm is wrapped for one eager step (the second of an eager engine: gradients accumulate in place as in the replayed
    step; the batch is the workload's first, not padded to a size class), and the first launch of every distinct
    (form, splits, extents and operand options of its problems) is repeated on its own operands through singa_gemm_f32 and
    through singa_gemm_bf16.  One line per distinct launch with its count per step, then one line per (form, tile) class."""
    from singa_amd import ops
    from singa_amd.config import load_config
    from singa_amd.engine import TrainStep
    from singa_amd.model.GAN import SINGA
    from singa_amd.optim import Adam
    L, batches = make_batches(args.workload, 1, dev)
    cfg = load_config(lmax=L)
    torch.manual_seed(cfg.train.seed)
    model = SINGA(cfg, device=dev, precision="bf16", embedding_precision=args.embedding_precision)
    model.train()
    opt = Adam(model.parameters(), lr=cfg.train.optimizer.lr, betas=(cfg.train.optimizer.beta1, cfg.train.optimizer.beta2))
    engine = TrainStep(model, opt, None, use_graph=False, max_grad_norm=float(cfg.train.max_grad_norm))
    engine.step(batches[0])
    torch.cuda.synchronize()
    inner, inner_c, seen, other = ops._gemm, ops._cgemm, {}, [0]
    opts = ("a_group", "b_group", "c_group", "c_split_stride", "bias", "addend", "mask", "relu", "asum")

    def recorded(items, a_rc, b_rc, splits=1, precision="f32"):
        if precision != "bf16" or not items:
            other[0] += 1
            return inner(items, a_rc, b_rc, splits, precision)
        key = (bool(a_rc), bool(b_rc), int(splits), tuple((it["I"], it["J"], it["R"], tuple(o for o in opts if it.get(o))) for it in items))
        if key in seen:
            seen[key]["per_step"] += 1
            return inner(items, a_rc, b_rc, splits, precision)
        rec = {"kind": "kernels", "launch": FORMS[key[0], key[1]], "tile": TILES[tile_shape(items, splits)], "splits": int(splits),
               "problems": len(items), "I": items[0]["I"], "J": items[0]["J"], "R": items[0]["R"],
               "options": list(key[3][0][3]), "equal_problems": len(set(key[3])) == 1,
               "gflop": round(2e-9 * sum(it["I"] * it["J"] * it["R"] for it in items), 3), "per_step": 1}
        for p in ("f32", "bf16"):
            rec[p] = per_launch_ms(lambda: inner(items, a_rc, b_rc, splits, p), args.launches)
        rec["bf16_over_f32"] = round(rec["bf16"]["median_ms"] / rec["f32"]["median_ms"], 3)
        seen[key] = rec
        return inner(items, a_rc, b_rc, splits, precision)

    def recorded_c(items, a_rc, b_rc, splits=1, precision="f32"):
        """The same for the complex launches (extents in complex units; 8 real flops per complex multiply-add)."""
        if precision != "bf16" or not items:
            other[0] += 1
            return inner_c(items, a_rc, b_rc, splits, precision)
        key = ("complex", bool(a_rc), bool(b_rc), int(splits), tuple((it["I"], it["J"], it["R"]) for it in items))
        if key in seen:
            seen[key]["per_step"] += 1
            return inner_c(items, a_rc, b_rc, splits, precision)
        rec = {"kind": "kernels", "launch": "complex " + FORMS[key[1], key[2]], "tile": "128x64c", "splits": int(splits),
               "problems": len(items), "I": items[0]["I"], "J": items[0]["J"], "R": items[0]["R"], "options": [],
               "equal_problems": len(set(key[4])) == 1, "all_problems": [list(k) for k in key[4]],
               "gflop": round(8e-9 * sum(it["I"] * it["J"] * it["R"] for it in items), 3), "per_step": 1}
        for p in ("f32", "bf16"):
            rec[p] = per_launch_ms(lambda: inner_c(items, a_rc, b_rc, splits, p), args.launches)
        rec["bf16_over_f32"] = round(rec["bf16"]["median_ms"] / rec["f32"]["median_ms"], 3)
        seen[key] = rec
        return inner_c(items, a_rc, b_rc, splits, precision)

    ops._gemm, ops._cgemm = recorded, recorded_c
    try:
        engine.step(batches[0])
        torch.cuda.synchronize()
    finally:
        ops._gemm, ops._cgemm = inner, inner_c
    classes = {}
    for rec in seen.values():
        emit(rec, args.out)
        c = classes.setdefault((rec["launch"], rec["tile"]), {"distinct": 0, "per_step": 0, "f32_ms": 0.0, "bf16_ms": 0.0, "ratios": []})
        c["distinct"] += 1
        c["per_step"] += rec["per_step"]
        c["f32_ms"] += rec["per_step"] * rec["f32"]["median_ms"]
        c["bf16_ms"] += rec["per_step"] * rec["bf16"]["median_ms"]
        c["ratios"].append(rec["bf16_over_f32"])
    for (launch, tile), c in sorted(classes.items()):
        emit({"kind": "class", "launch": launch, "tile": tile, "distinct_launches": c["distinct"], "launches_per_step": c["per_step"],
              "f32_ms_per_step": round(c["f32_ms"], 4), "bf16_ms_per_step": round(c["bf16_ms"], 4),
              "bf16_over_f32": round(c["bf16_ms"] / c["f32_ms"], 3), "ratio_min": min(c["ratios"]), "ratio_max": max(c["ratios"])}, args.out)
    emit({"kind": "kernels_summary", "bf16_launches_per_step": sum(c["per_step"] for c in classes.values()),
          "f32_gemm_launches_per_step": other[0], "f32_ms_per_step": round(sum(c["f32_ms"] for c in classes.values()), 3),
          "bf16_ms_per_step": round(sum(c["bf16_ms"] for c in classes.values()), 3)}, args.out)
    engine.release()


def ops_precision(p):
    if p not in ("f32", "bf16"):
        raise argparse.ArgumentTypeError(p)
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["steps", "kernels", "all"], default="all")
    ap.add_argument("--workload", default="cfg3_b128_l4")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--distinct-batches", type=int, default=3)
    ap.add_argument("--growth", type=float, default=1.04)
    ap.add_argument("--precisions", type=lambda v: [ops_precision(p) for p in v.split(",")], default=["f32", "bf16"],
                    help="steps part: the modes to alternate; one mode alone for a run under a kernel trace")
    ap.add_argument("--embedding-precision", type=ops_precision, default="f32",
                    help="the embedding's SO(2) convolutions (SINGA(..., embedding_precision=...)), in both parts")
    ap.add_argument("--settings", type=lambda v: [tuple(ops_precision(p) for p in s.split("/")) for s in v.split(",")], default=None,
                    help="steps part: precision/embedding-precision pairs to alternate, e.g. f32/f32,bf16/f32,f32/bf16,bf16/bf16; "
                         "differences are reported against the first")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert not args.settings or all(len(s) == 2 for s in args.settings), "--settings takes precision/embedding-precision pairs"
    assert args.launches >= 50, "per-launch medians over at least 50 launches"
    import __graft_entry__
    __graft_entry__.build()
    assert torch.cuda.is_available(), "bench_precision needs a GPU"
    dev = torch.device("cuda", 0)
    with open(__graft_entry__.LIB, "rb") as f:
        sha = hashlib.sha256(f.read()).hexdigest()[:16]
    emit({"kind": "run", "device": torch.cuda.get_device_name(0), "lib_sha256": sha, "part": args.part, "workload": args.workload,
          "distinct_batches": args.distinct_batches, "growth": args.growth}, args.out)
    if args.part in ("kernels", "all"):
        kernels_part(args, dev)
    if args.part in ("steps", "all"):
        steps_part(args, dev)


if __name__ == "__main__":
    main()
