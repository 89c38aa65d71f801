#!/usr/bin/env python
"""Training entrypoint with the reference's shape (reference train.py:32-260): `--config --device --logdir`, YAML config,
seeded model build, Adam(lr 1e-4, betas (0.99, 0.999)), CrossEntropy, clip_grad_norm_(max_grad_norm), plateau scheduler,
validation every `val_freq` iterations with early stopping, checkpoints {'config','model','optimizer','scheduler',
'iteration'}.  The step itself runs through singa_amd.engine.TrainStep (HIP kernels + HIP-graph replay).

The CrossDocked dataset and the RDKit/ODDT featurisation of the reference are out of scope, so graphs
come from `--data golden` (the three example graphs the reference bundles, shipped under singa_amd/data/examples), `--data synthetic`
(singa_amd.graph.synthetic_graph) or `--data packed --dataset DIR`: a packed dataset of already featurised graphs
(singa_amd.dataset, made by tools/pack_dataset.py), held on the device, whose batches a kernel assembles.  Under
`torch.distributed.run` every rank trains on its own shard of each batch and gradients are averaged with RCCL (singa_amd.dp).

    python train.py --config ./config/train.yml --device cuda --logdir ./logs --data synthetic --max-iters 20
"""
import argparse
import logging
import os
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class EarlyStopping:
    """utils/Stopping.py:3-42 of the reference: stop after `patience` validations without a `delta` improvement."""

    def __init__(self, mode="min", patience=20, delta=0.00005):
        self.best, self.bad, self.patience, self.delta = None, 0, patience, delta

    def step(self, value):
        if self.best is None or value < self.best - self.delta:
            self.best, self.bad = value, 0
        else:
            self.bad += 1
        return self.bad >= self.patience


def get_logger(name, log_dir):
    logger = logging.getLogger(name)
    logger.setLevel(logging.DEBUG)
    fmt = logging.Formatter("[%(asctime)s::%(name)s::%(levelname)s] %(message)s")
    for h in (logging.StreamHandler(), logging.FileHandler(os.path.join(log_dir, "log.txt"))):
        h.setFormatter(fmt)
        logger.addHandler(h)
    return logger


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default=os.path.join(ROOT, "config", "train.yml"))
    ap.add_argument("--device", type=str, default="cuda")
    ap.add_argument("--logdir", type=str, default="./logs")
    ap.add_argument("--data", choices=["synthetic", "golden", "packed"], default="synthetic")
    ap.add_argument("--dataset", type=str, default=None, help="--data packed: directory of a packed dataset (tools/pack_dataset.py)")
    ap.add_argument("--no-shuffle", action="store_true",
                    help="--data packed: iteration `it` takes rows (it-1)*B .. it*B-1 of the train split instead of a shuffled epoch")
    ap.add_argument("--val-batches", type=int, default=None,
                    help="--data packed: validate on the first N batches of the val split (default: all of them)")
    ap.add_argument("--host-dataset", action="store_true",
                    help="--data packed: keep the pack on the host (batches gathered on the host and copied per step) - for a "
                         "pack that does not fit on the device")
    ap.add_argument("--lmax", type=int, default=None, help="override embedding.lmax_list (2, 3, 4 or 6)")
    ap.add_argument("--max-iters", type=int, default=None)
    ap.add_argument("--batch-size", type=int, default=None, help="graphs per step over all ranks")
    ap.add_argument("--graph", action="store_true",
                    help="capture the step into HIP graphs and replay it; batches of different sizes are padded to size "
                         "classes, one capture per class")
    ap.add_argument("--allreduce-overlap", action="store_true",
                    help="several ranks: two-phase backward, the transformer's gradient buckets are all-reduced while the "
                         "embedding's backward pass computes (dp.GradAllReducer(phases=True)); default: one all-reduce after "
                         "the backward pass")
    ap.add_argument("--resume", type=str, default=None, help="checkpoint to load (model, optimizer, scheduler, iteration)")
    ap.add_argument("--no-dropout", action="store_true",
                    help="switch the decoder's positional-encoding dropout (reference CProMG.py:198, p = 0.1: the only stochastic "
                         "op of the step besides the edge-frame draws) off - reproducible runs for parity checks")
    ap.add_argument("--recompute", action="store_true",
                    help="rebuild the embedding's largest saved activations in the backward pass instead of holding them (both "
                         "[N, K, 512] tensors of every feed-forward block, the S2 activation of every attention block): less memory, "
                         "slightly longer steps, the same checkpoints")
    ap.add_argument("--precision", choices=["f32", "bf16"], default="f32",
                    help="bf16: the CProMG transformer's real GEMMs (Linears, feed-forward, grouped projections; forward, input and "
                         "weight gradients) round their operands to bfloat16 inside the kernel and accumulate in f32 "
                         "(include/singa_hip_bf16.h).  Tensors, master weights, gradients, Adam and checkpoints stay f32; the "
                         "equivariant embedding and generation stay f32")
    ap.add_argument("--embedding-precision", choices=["f32", "bf16"], default="f32",
                    help="bf16: the same for the GEMMs of the equivariant embedding's SO(2) convolutions, real (m = 0) and complex "
                         "(m > 0), and for nothing else in the embedding; independent of --precision")
    args = ap.parse_args()
    assert args.device.startswith("cuda"), "the hot path is the HIP path: there is no CPU fallback"

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world > 1:
        dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    import __graft_entry__
    if rank == 0:
        __graft_entry__.build()
    if world > 1:
        dist.barrier()
    from singa_amd import dp, graph as G
    from singa_amd.config import load_config
    from singa_amd.engine import TrainStep
    from singa_amd.model.GAN import SINGA

    cfg = load_config(args.config, lmax=args.lmax)
    torch.manual_seed(cfg.train.seed)
    log_dir = os.path.join(args.logdir, time.strftime("train_%Y_%m_%d__%H_%M_%S"))
    ckpt_dir = os.path.join(log_dir, "checkpoints")
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
        logger = get_logger("training_log", log_dir)
        logger.info(f"args {vars(args)}; world {world}")
    log = (lambda m: logger.info(m)) if rank == 0 else (lambda m: None)

    batch_size = args.batch_size or cfg.train.batch_size
    lo, hi = dp.shard_range(batch_size, rank, world)     # equal-sized shards when world divides batch_size

    store = None
    if args.data == "packed":
        from singa_amd import dataset as D
        assert args.dataset, "--data packed needs --dataset DIR"
        store = D.PackedDataset.load(args.dataset).to(dev, device_resident=not args.host_dataset)
        log(f"packed dataset {args.dataset}: {store.G} graphs, {store.nbytes} bytes, "
            f"{'host' if args.host_dataset else 'device'} resident; splits " +
            ", ".join(f"{k} {len(v)}" for k, v in store.splits.items()))

    def make_batch(split, it):
        """One batch of `batch_size` graphs; this rank materialises only its shard [lo, hi).  `it` counts from 1 for the
        packed dataset (dataset.batch_ids) and is the generator's batch number otherwise."""
        if store is not None:
            ids = D.batch_ids(store.splits[split], it, batch_size, cfg.train.seed, shuffle=not args.no_shuffle, rank=rank,
                              world=world, train=split == "train")
            return store.batch(ids)
        if args.data == "golden":
            # the three example graphs the reference bundles (example/*.pt), shipped with the package as plain arrays
            gs = [G.example_graph(i) for i in range(lo, hi)]
        else:
            base = {"train": 0, "val": 10_000_000, "test": 20_000_000}[split] + it * batch_size
            gs = [G.synthetic_graph(base + i) for i in range(lo, hi)]
        return G.collate(gs).to(dev)

    model = SINGA(cfg, device=dev, recompute=args.recompute, precision=args.precision, embedding_precision=args.embedding_precision)
    log(f"precision {args.precision}: the transformer's real GEMMs take " +
        ("bf16 operands with f32 accumulation" if args.precision == "bf16" else "f32 operands"))
    if args.embedding_precision != "f32":
        log(f"embedding precision {args.embedding_precision}: the SO(2) convolutions' real and complex GEMMs take bf16 operands "
            "with f32 accumulation")
    if args.no_dropout:
        model.model.decoder.pos_emb.dropout.p = 0.0
    o = cfg.train.optimizer
    from singa_amd.optim import Adam
    assert o.type == "adam" and o.weight_decay == 0
    opt = Adam(model.parameters(), lr=o.lr, betas=(o.beta1, o.beta2))
    s = cfg.train.scheduler
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, factor=s.factor, patience=s.patience, min_lr=s.min_lr)
    start_it = 1
    if args.resume:
        ck = torch.load(args.resume, map_location=dev)
        model.load_state_dict(ck["model"], strict=False)        # reference checkpoints: derived buffers are recomputed
        opt.load_state_dict(ck["optimizer"])
        sched.load_state_dict(ck["scheduler"])
        start_it = ck["iteration"] + 1
    reducer = dp.GradAllReducer(model, phases=bool(args.allreduce_overlap)) if world > 1 else None
    if reducer:
        reducer.check_same_init()
        reducer.set_shard_weight(hi - lo, batch_size)        # token-weighted combination: exact for unequal shards too
    # --graph: ragged batches are padded to size classes and replay a few captured HIP graphs (TrainStep bucket mode)
    engine = TrainStep(model, opt, reducer, use_graph=args.graph, max_grad_norm=float(cfg.train.max_grad_norm),
                       bucket=args.graph)
    early = EarlyStopping(patience=20, delta=0.00005)

    def evaluate(split, n_batches=2):
        first = 0
        if store is not None:
            # the packed split in order: all of its batches (a last batch too short to give every rank a graph is left
            # out), or --val-batches of them; a pack without this split has nothing to evaluate
            n_graphs = len(store.splits.get(split, ()))
            n_batches = D.n_batches(range(n_graphs), batch_size, train=False)
            if n_batches and n_graphs - (n_batches - 1) * batch_size < world:
                n_batches -= 1
            if args.val_batches is not None:
                n_batches = min(n_batches, args.val_batches)
            if n_batches < 1:
                return None
            first = 1
        model.eval()
        tot = 0.0
        with torch.no_grad():
            for b in range(first, first + n_batches):
                batch = make_batch(split, b)
                model.prepare(batch)
                logits = model(batch)
                loss = torch.nn.functional.cross_entropy(logits, batch["ligand_data"]["smiIndices_tgt"].reshape(-1))
                t = loss.detach().clone()
                if world > 1:
                    dist.all_reduce(t)
                    t /= world
                tot += float(t)
        return tot / n_batches

    max_iters = args.max_iters or cfg.train.max_iters
    log(f"model built: {sum(p.numel() for p in model.parameters())} parameters; training for {max_iters} iterations")
    # the next batch is generated, copied and prepared (edge sorting, kNN graphs) on a second stream while the current
    # step computes: TrainStep.prefetch
    nxt = engine.prefetch(lambda: make_batch("train", start_it)) if start_it <= max_iters else None
    for it in range(start_it, max_iters + 1):
        model.train()
        t0 = time.perf_counter()
        loss = engine.step(nxt)
        if it < max_iters:
            nxt = engine.prefetch(lambda: make_batch("train", it + 1))
        loss_v = float(loss.detach())
        engine.check()                      # the reference's edge-frame guards for frames built inside replayed graphs
        log(f"[Train] Iter {it} | Loss {loss_v:.6f} | Grad {float(engine.grad_norm):.4f} | "
            f"LR {opt.param_groups[0]['lr']:.2e} | {time.perf_counter() - t0:.3f} s")
        if it % cfg.train.val_freq == 0 or it == max_iters:
            val = evaluate("val")
            if val is None:
                log(f"[Validate] Iter {it} | the dataset has no val split: scheduler and early stopping see the training loss")
                val = loss_v
            sched.step(val)
            log(f"[Validate] Iter {it} | Loss {val:.6f}")
            if rank == 0:
                torch.save({"config": cfg.to_dict(), "model": model.state_dict(), "optimizer": opt.state_dict(),
                            "scheduler": sched.state_dict(), "iteration": it}, os.path.join(ckpt_dir, f"{it}.pt"))
            if early.step(val):
                log("Early stopping")
                break
    test = evaluate("test")
    log(f"[Test] Loss {test:.6f}" if test is not None else "[Test] the dataset has no test split")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
