#!/usr/bin/env python
"""What a batch costs before the step can start, three ways, on `--graphs` (1,024) ragged graphs of the default bench
workload and batches of `--batch` (128) ids drawn by the sampler (dataset.batch_ids, shuffled epochs):

  (a) collate_to   graph.collate of B host graphs + .to(device)            - what train.py offered before the packed dataset
  (b) host_batch   PackedDataset.host_batch(ids) + .to(device)             - the packed store on the host
  (c) device_batch PackedDataset.to(device).batch(ids)                     - the packed store on the device, collate kernel

Per path: the median over `--iters` (50) batches after `--warmup` of the host wall time of the call (the host is free again)
and of the device time (events around the call; for (a) and (b) this is dominated by the copies).  For (c) also the bytes the
kernels read and write and the launches per batch.  `load_reference_pt_ms`: time per graph of reading the three .pt fixtures
under tests/golden over and over - what one-file-per-graph loading costs before any collation.

    python tools/bench_loader.py [--out profiles/dataloader/loader.jsonl]

Prints one JSON line (and appends it to --out).
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="cfg3_b128_l4")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import dataset as D
    from singa_amd import graph as G
    assert torch.cuda.is_available(), "bench_loader needs a GPU"
    dev = torch.device("cuda", 0)
    _, kw, _, _ = G.resolve_workload(args.workload)
    t0 = time.perf_counter()
    graphs = [G.synthetic_graph(i, with_lap=False, **G.graph_sizes(i, **kw)) for i in range(args.graphs)]
    gen_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    pack = D.PackedDataset.from_graphs(graphs)
    pack_s = time.perf_counter() - t0
    split = np.arange(pack.G)
    ids_of = lambda it: D.batch_ids(split, it, args.batch, seed=0)

    def timed(fn):
        host, devt = [], []
        for it in range(1, args.warmup + args.iters + 1):
            ids = ids_of(it)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            t = time.perf_counter()
            out = fn(ids)
            dt = time.perf_counter() - t
            b.record()
            torch.cuda.synchronize()
            if it > args.warmup:
                host.append(dt * 1e3)
                devt.append(a.elapsed_time(b))
            del out
        return {"host_ms": round(statistics.median(host), 4), "device_ms": round(statistics.median(devt), 4)}

    res = {"graphs": pack.G, "batch": args.batch, "iters": args.iters, "workload": args.workload,
           "pack_bytes": pack.nbytes, "bytes_per_graph": round(pack.nbytes / pack.G), "generate_s": round(gen_s, 2),
           "pack_s": round(pack_s, 2)}
    res["collate_to"] = timed(lambda ids: G.collate([graphs[i] for i in ids]).to(dev))
    res["host_batch"] = timed(lambda ids: pack.host_batch(ids).to(dev))
    store = pack.to(dev)
    res["device_batch"] = timed(lambda ids: store.batch(ids))
    res["device_batch"].update(bytes_moved=int(store.last_bytes), launches=int(store.last_launches),
                               status=int(store.last_status.item()))
    # device ids: the epoch's permutation uploaded once and sliced (no per-batch copy at all)
    perm = {}

    def sliced(ids):
        key = ids.tobytes()
        if key not in perm:
            perm[key] = torch.from_numpy(ids.astype(np.int32)).to(dev)
        return store.batch(perm[key], host_ids=ids)
    for it in range(1, args.warmup + args.iters + 1):
        sliced(ids_of(it))                                   # upload outside the timed calls
    res["device_batch_resident_ids"] = timed(sliced)
    res["ratio_a_over_c_host"] = round(res["collate_to"]["host_ms"] / res["device_batch"]["host_ms"], 1)
    # one file per graph: the three fixtures, read again and again
    names = ("3wi2_4tpp", "4agq_5a7b", "5cp5_4nue")
    paths = [os.path.join(ROOT, "tests", "golden", f"example_{n}.pt") for n in names]
    for p in paths:
        G.load_reference_pt(p, with_lap=False)
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        for p in paths:
            G.load_reference_pt(p, with_lap=False)
    res["load_reference_pt_ms"] = round((time.perf_counter() - t0) * 1e3 / (reps * len(paths)), 3)
    with open(__graft_entry__.LIB, "rb") as f:
        res["lib_sha256"] = hashlib.sha256(f.read()).hexdigest()[:16]
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
