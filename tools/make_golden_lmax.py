#!/usr/bin/env python
"""Goldens of lmax 3 from the reference's own modules:

    python tools/make_golden_lmax.py [L ...]        # default: 3; writes tests/golden/
    python oracle/make_relu_ties.py 3               # then the pinned ReLU gates of the full step (reads the whole step file)
    python tools/make_golden_lmax.py --split [L ...]   # last: the gradient samples move into a file of their own

oracle/make_golden.py fixes its degrees and its node-stride table at (2, 4, 6).  This tool imports it as a module (which sets up
the shim path) and reuses load_graph, config_for, overwrite_params, Recorder and run_singa unchanged; the embedding run is the
same recipe with the node stride as an argument.  Like make_golden.py it is run once, in the build container, and it is the
only place that reads the reference; only tensors and parameter names are written:

  embed_L<L>_<name>.npz        as make_golden.py writes it (block-0 intermediates for 4agq_5a7b only)
  param_spec_embed_L<L>.npz    through overwrite_params
  singa_L<L>_B3.npz, param_spec_singa_L<L>.npz    through run_singa
  singa_L<L>_B3_grad_samples.npz                  --split: the `grad_samples` array of singa_L<L>_B3.npz, which keeps the rest
                                                  (0.85 MB of incompressible floats: together the file is above 1 MiB);
                                                  tests/golden_lmax.py reads the pair as one
"""
import importlib.util
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# node stride of the recorded protein-side tensors: every file stays below 1 MiB
NODE_STRIDE = {3: 3}


def load_make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(ROOT, "oracle", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run_embedding(MG, L, stride, rec):
    import numpy as np
    import torch
    from model.Embedding import EquivariantEmbedding
    PA, LA = MG.PA, MG.LA
    cfg = MG.config_for(L)
    torch.manual_seed(2022)
    emb = EquivariantEmbedding(cfg.embedding, device="cpu")
    MG.overwrite_params(emb, f"embed_L{L}")
    for name in MG.NAMES:
        g = MG.load_graph(name)
        rec.clear()
        torch.manual_seed(2022)
        inter = {}

        def save(key):
            def fn(mod, inp, out):
                if key not in inter:      # first call only = protein pass
                    t = out.embedding if hasattr(out, "embedding") else out
                    inter[key] = t.detach().clone().numpy()
            return fn

        b0 = emb.blocks[0]
        hooks = [emb.edge_degree_embedding.register_forward_hook(save("edge_degree_pp")),
                 b0.norm_1.register_forward_hook(save("b0_norm1_pp")),
                 b0.ga.so2_conv_1.rad_func.register_forward_hook(save("b0_rad_pp")),
                 b0.ga.register_forward_hook(save("b0_ga_pp")),
                 b0.ffn.register_forward_hook(save("b0_ffn_pp")),
                 b0.register_forward_hook(save("b0_out_pp"))]
        emb.zero_grad()
        out = emb(g)
        for h in hooks:
            h.remove()
        assert len(rec.rot) == 3
        loss = (out[PA].embedding ** 2).sum() + (out[LA].embedding ** 2).sum()
        loss.backward()
        params = dict(emb.named_parameters())
        gn = {n: (float(p.grad.norm()) if p.grad is not None else -1.0) for n, p in params.items()}
        d = {f"rot_{k}": rec.rot[i].numpy() for i, k in enumerate(["pp", "ll", "lp"])}
        d["node_stride"] = np.array(stride)
        if name == MG.NAMES[1]:
            for k, v in inter.items():
                d[k] = v[::stride]
        d["out_p"] = out[PA].embedding.detach().numpy()[::stride]
        d["out_l"] = out[LA].embedding.detach().numpy()
        d["out_lp"] = out["lp_edge"].embedding.detach().numpy()[::stride]
        d["out_pl"] = out["pl_edge"].embedding.detach().numpy()
        d["loss"] = np.array(float(loss))
        d["grad_names"] = np.array(list(gn.keys()))
        d["grad_norms"] = np.array(list(gn.values()))
        for n in ["blocks.0.ga.alpha_dot", "blocks.2.norm_1.affine_weight",
                  "edge_degree_embedding.rad_func.net.0.weight", "blocks.1.ga.proj.bias"]:
            d["grad:" + n] = params[n].grad.numpy()
        path = os.path.join(MG.OUT, f"embed_L{L}_{name}.npz")
        np.savez_compressed(path, **d)
        print(f"embed L={L} {name}: loss {float(loss):.6e}, {os.path.getsize(path) / 1e6:.2f} MB")


def main(degrees):
    MG = load_make_golden()
    rec = MG.Recorder().install()
    for L in degrees:
        run_embedding(MG, L, NODE_STRIDE[L], rec)
    for L in degrees:
        MG.run_singa(L, rec)


def split(degrees):
    import numpy as np
    out = os.path.join(ROOT, "tests", "golden")
    for L in degrees:
        path = os.path.join(out, f"singa_L{L}_B3.npz")
        z = dict(np.load(path))
        np.savez_compressed(os.path.join(out, f"singa_L{L}_B3_grad_samples.npz"), grad_samples=z.pop("grad_samples"))
        np.savez_compressed(path, **z)
        print(f"singa L={L}: " + ", ".join(f"{f} {os.path.getsize(os.path.join(out, f)) / 1e6:.2f} MB"
                                           for f in (f"singa_L{L}_B3.npz", f"singa_L{L}_B3_grad_samples.npz")))


if __name__ == "__main__":
    args = sys.argv[1:]
    if args[:1] == ["--split"]:
        split([int(a) for a in args[1:]] or [3])
    else:
        main([int(a) for a in args] or [3])
