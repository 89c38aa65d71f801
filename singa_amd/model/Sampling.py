"""Sampled generation for MI355X: many molecules per pocket, one HIP graph replay per token.

The reference generates with beam search only (model/BeamSearch.py, one sequence per pocket in gen.py); whoever evaluates a
pocket-conditioned generator draws a SET of molecules per pocket.  `sample` is ancestral sampling with temperature, top-k
and top-p (greedy decoding as the limit temperature = 0) on the pieces `beam_search` already has - the KV-cached decoder
(`BeamSearch.KVDecoder`: encoder keys / values projected once per pocket, the samples of a pocket as its query rows) - and
differs from it where beam search is coupled:

  * rows never exchange prefixes, so the caches are never re-ranked (`KVDecoder.follow` is not called);
  * the token choice is a per-row function of the row's logits and ONE uniform number, so it runs on the device inside the
    captured step (`ops.sample_token`, kernel `singa_sample_token`; include/singa_hip.h states the rule), together with the
    rows' bookkeeping: finished flag, length, summed log-probability, the output matrix, the next input token;
  * nothing comes back to the host per token: the loop reads one 4-byte counter of live rows every 16 tokens and stops when
    it is zero.

The captured step is: embed the previous token, the decoder layers (the k17 step kernels, or library GEMMs for many rows),
the vocabulary projection, `singa_sample_token`.  All randomness is a `[max_length, rows]` tensor of uniforms drawn once per
call (or handed in: `uniforms=`), which the kernel indexes with the device-resident position - a run is reproduced exactly
by its uniforms, on any device and at any row count.

A live row that draws '^' or '&' carries on: to the KV-cached decoder they are tokens like any other (as in beam search, the
caches have no padding mask).  `suppress=("&", "^")` keeps them from being drawn.

`grammar="smiles"` constrains the draw to syntactically complete SMILES: the token choice then runs as
`ops.sample_token_grammar` (kernel `singa_sample_token_grammar`; include/singa_hip_gen.h states the rule), which keeps one
more word of state per row on the device and masks, per row, what cannot follow the row's prefix or could not be finished in
the columns left.  Every row then ends in '$' before `max_length` and the text in front of it has balanced branches, paired
ring-closure digits and no dangling bond symbol.  Syntax only: valence, aromaticity, duplicate ring bonds (C1C1), %nn
closures and beam search are outside the rule (singa_amd/smiles.py).  The step stays one captured graph.
"""
import torch

from .. import ops, smiles
from .BeamSearch import KVDecoder

# Row count above which `fused=None` takes the library path (GEMMs that read a layer's weights once per step) instead of the
# k17 step kernels (one workgroup per row, the weights re-read per workgroup).  Measured at 20 / 128 / 512 / 2,048 rows
# (profiles/sampling/README.md): k17 is faster at every one of them (2.40 against 3.36 ms per step at 2,048 rows, and both
# grow by about 1.1 us per row from 512 on), so there is no crossover to switch at: None = k17 wherever its limits allow.
FUSED_MAX_ROWS = None
LIVE_POLL = 16          # tokens between two reads of the live-row counter


def cache_bytes(decoder, rows, positions):
    a = decoder.layers[0].dec_self_attn
    return len(decoder.layers) * rows * positions * (a.key_channels + a.hidden_channels) * 4


@torch.no_grad()
def sample(model, smiVoc, num_samples, batch_size, max_length, example, prop=None, device="cuda", temperature=1.0, top_k=0,
           top_p=1.0, suppress=(), generator=None, uniforms=None, graph=True, fused=None, trace=None, grammar=None):
    """`num_samples` sequences for each of the `batch_size` pockets of `example`, drawn token by token from the model's own
    distribution reshaped by `temperature` (0 = greedy), `top_k` (0 = off) and `top_p` (1 = off).

    `model`, `smiVoc`, `example`, `prop` ([batch_size * num_samples, num_props]; position 0 is the property prompt) and `device`
    as in `beam_search`.  `suppress`: tokens never to be drawn.  `generator`: torch.Generator for the uniforms (CPU or device);
    `uniforms` [max_length, rows] f32 in [0, 1) replaces the draw (row t is read by the step that writes column t + 1).
    `graph=False` launches the step's kernels one by one (same tokens).  `fused`: True = k17 step kernels, False = library
    GEMMs, None = the faster one for the row count (`FUSED_MAX_ROWS`: k17 wherever the k17 kernels' limits allow).

    Returns the int64 token matrix [batch_size * num_samples, max_length], pocket-major: a row starts with '&', ends with
    '$' if the model ended it before `max_length`, and is padded with '^'.  `trace`, if a dict, receives `lengths` (int32:
    tokens drawn per row, the '$' included, '&' not), `sum_logp` (f32: the model's own log-likelihood of the drawn tokens,
    temperature 1 and nothing filtered), `token_logp` [rows, max_length] (per drawn token), `uniforms`, `path`
    ('k17' / 'library') and `steps` (tokens decoded before every row had ended).

    `grammar="smiles"`: only tokens that keep the row a prefix of a syntactically complete SMILES string which still fits
    into `max_length` (>= 3) are drawn, so every row ends with '$'.  `token_logp` / `sum_logp` stay the unconstrained model's;
    `trace` also receives `allowed_logp` [rows, max_length]: log of the model's probability mass on the tokens the rule (and
    `suppress`) allowed at that step, so that token_logp - allowed_logp is the log-probability under the constrained proposal.
    ValueError for an unknown grammar, max_length < 3, or a `suppress` that removes every atom, '$', or ')' but not '('."""
    dev = torch.device(device)
    if dev.type != "cuda" or not example.protein_atom_feature.is_cuda:
        raise RuntimeError("sample runs on the GPU only (no CPU fallback): device and the example's tensors must be cuda")
    if num_samples < 1 or batch_size < 1 or max_length < 2:
        raise ValueError(f"sample: num_samples >= 1, batch_size >= 1, max_length >= 2 (got {num_samples}, {batch_size}, {max_length})")
    if temperature < 0 or top_k < 0 or not 0 < top_p <= 1:
        raise ValueError(f"sample: temperature >= 0, top_k >= 0, 0 < top_p <= 1 (got {temperature}, {top_k}, {top_p})")
    cls = smiles.check_arguments(grammar, smiVoc, max_length, suppress)
    tf = model.model
    voc = list(smiVoc)
    V = len(voc)
    sos, eos, pad = voc.index("&"), voc.index("$"), voc.index("^")
    rows = batch_size * num_samples
    num = 1 if tf.decoder.num_props else 0
    positions = max_length - 1 + num
    need = cache_bytes(tf.decoder, rows, positions)
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if need + (64 << 10) * rows > free:                  # + the step's activations: a few [rows, 1024] f32 operands
        raise ValueError(f"sample: the key / value caches of {rows} rows x {positions} positions take {need} bytes, "
                         f"{free} bytes are free on {dev}: draw fewer samples per call and call again with the next "
                         f"generator state")
    if uniforms is None:
        gdev = generator.device if generator is not None else dev
        uniforms = torch.rand((max_length, rows), generator=generator, device=gdev, dtype=torch.float32)
    if tuple(uniforms.shape) != (max_length, rows) or uniforms.dtype != torch.float32:
        raise ValueError(f"sample: uniforms must be float32 [max_length, rows] = [{max_length}, {rows}], got "
                         f"{uniforms.dtype} {tuple(uniforms.shape)}")
    uniforms = uniforms.to(dev).contiguous()

    enc_outputs, enc_pad_mask, _ = tf.encoder(example.protein_atom_feature.float(), example.protein_pos,
                                              example.protein_element_batch, example.protein_atom_laplacian, batch_size,
                                              getattr(example, "protein_knn", None))
    want_fused = (FUSED_MAX_ROWS is None or rows <= FUSED_MAX_ROWS) if fused is None else bool(fused)
    kv = KVDecoder(tf.decoder, tf.projection, enc_outputs, enc_pad_mask, num_samples, positions, V, want_fused,
                   search_buffers=False)
    if fused and not kv.fused:
        raise ValueError("sample: fused=True needs the shipped decoder geometry, at most 256 positions and 1024 pocket atoms")
    allowed = None
    if suppress:
        allowed = torch.ones(V, dtype=torch.uint8)
        allowed[[voc.index(s) for s in suppress]] = 0
        allowed = allowed.to(dev)
    state = {"tokens": torch.empty(rows, max_length, dtype=torch.int64, device=dev),
             "next": torch.empty(rows, dtype=torch.int64, device=dev),
             "finished": torch.empty(rows, dtype=torch.uint8, device=dev),
             "length": torch.empty(rows, dtype=torch.int32, device=dev),
             "sum_logp": torch.empty(rows, dtype=torch.float32, device=dev),
             "live": torch.empty(1, dtype=torch.int32, device=dev),
             "tok_logp": torch.empty(rows, max_length, dtype=torch.float32, device=dev)}
    if grammar is not None:
        cls = torch.as_tensor(cls).to(dev)
        state["grammar"] = torch.empty(rows, dtype=torch.int32, device=dev)
        state["allowed_logp"] = torch.empty(rows, max_length, dtype=torch.float32, device=dev)

    def start():
        state["tokens"].fill_(pad)
        state["tokens"][:, 0] = sos
        state["next"].fill_(sos)
        state["finished"].zero_(), state["length"].zero_(), state["sum_logp"].zero_(), state["tok_logp"].zero_()
        state["live"].fill_(rows)
        if grammar is not None:
            state["grammar"].fill_(smiles.FRESH), state["allowed_logp"].zero_()
        kv.reset()

    def step():
        out = kv.advance(kv.token_input(state["next"]))
        if grammar is None:
            ops.sample_token(tf.projection(out).contiguous(), uniforms, kv.pos, num + 1, state, float(temperature), int(top_k),
                             float(top_p), eos, pad, allowed)
        else:
            ops.sample_token_grammar(tf.projection(out).contiguous(), uniforms, kv.pos, num + 1, state, cls, float(temperature),
                                     int(top_k), float(top_p), eos, pad, allowed)

    replay = step
    if graph:
        # as KVDecoder.capture: two warm-up steps on a side stream, then the capture; both write cache slots and row state,
        # which `start` resets, and slots >= pos are never read
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                start()
                kv.pos += num
                step()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        start()
        kv.pos += num
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            step()
        replay = g.replay
    start()
    if num:
        kv.advance(kv.prop_input(prop.to(dev).float()))                # position 0 is the property prompt, CP:404-412
    steps = 0
    while steps < max_length - 1:
        replay()
        steps += 1
        if steps % LIVE_POLL == 0 and int(state["live"].item()) == 0:  # one 4-byte copy: every row has drawn its '$'
            break
    if trace is not None:
        trace.update(lengths=state["length"], sum_logp=state["sum_logp"], token_logp=state["tok_logp"], uniforms=uniforms,
                     path="k17" if kv.fused else "library", steps=steps)
        if grammar is not None:
            trace.update(allowed_logp=state["allowed_logp"])
    return state["tokens"]
