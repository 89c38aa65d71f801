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

`grammar="smiles"` constrains the draw to syntactically complete SMILES: `ops.sample_token`, given the class bytes, then
runs `singa_sample_token_grammar` (include/singa_hip_gen.h states the rule), which keeps one
more word of state per row on the device and masks, per row, what cannot follow the row's prefix or could not be finished in
the columns left.  Every row then ends in '$' before `max_length` and the text in front of it has balanced branches, paired
ring-closure digits and no dangling bond symbol.  This grammar is syntax only: valence, aromaticity, duplicate ring bonds
(C1C1) and %nn closures are outside its rule (singa_amd/smiles.py); beam search takes it through `beam_search_device`.  The step
stays one captured graph.

`grammar="valence"` adds a bonding-capacity rule to that syntax (include/singa_hip_valence.h states it): `ops.sample_token`,
given the capacity bytes as well, runs `singa_sample_token_valence`, which keeps two more words of state per row and also
masks what would give an atom more bond order than its token can carry - `F(C)C`, `C1CF1`, `C(=O)(=O)(=O)C` are not drawn.
A necessary condition for validity, not a sufficient one: aromaticity, kekulisation and duplicate ring bonds stay outside.
`sample`, `score` and `sample_stream` take it; `sample_distinct` does not (its selection gathers one state word per row).

`sample_stream`, `sample_distinct` and `BeamSearch.beam_search_device` take `forced=` as well (include/singa_hip_prefix.h
states the rule: a forced column's effective mask is the single given token, and everything behind the choice is the code a
chosen token runs), and `score(..., rows_per_pocket=R)` scores a library on a fixed budget of rows through `sample_stream`.

`forced=` gives tokens instead of drawing them: `ops.sample_token`, given the forced matrix, then runs
`singa_sample_token_forced` (include/singa_hip_force.h states the rule), which reads one more 8-byte word per row from a
fixed device matrix indexed by the device-resident position - like the uniforms, so the step stays one captured graph - and,
where that word is a token, takes it with the bookkeeping of a drawn one.  Forcing the first columns of a row continues a
scaffold; forcing every column up to '$' scores a given molecule (`score`): the log-likelihood then comes from the same
kernels, in the same order, as the `sum_logp` of a drawn row, so the two are comparable bit for bit.  The host validates what
it forces (`smiles.check_forced`, through the library's own rule) before any device work; the kernel does not.

`sample_distinct` draws WITHOUT replacement: `num_samples` pairwise distinct sequences per pocket by stochastic beam search
(Kool, van Hoof, Welling 2019; include/singa_hip_swor.h states the rule), an exact sample without replacement from the
proposal in one pass of `num_samples` rows.  Here the rows of a pocket ARE coupled, and the coupled part runs on the device
inside the captured step: `ops.swor_expand` (the perturbed score of every candidate), `ops.swor_select` (the best k per
pocket, the row state gathered from the parents) and `ops.swor_follow` (one launch moves the surviving prefixes' key / value
cache rows from one cache buffer to the other; the step is captured twice, for even and odd tokens, and the two graphs are
replayed in turn).  `swor_weights` turns the run's `gumbel` / `prop_logp` into the importance weights of the paper's estimator.

`sample_stream` makes the number of ROWS a fixed budget and the number of molecules free: `rows_per_pocket` rows per pocket
decode `num_samples` molecules per pocket, and a row that has ended its molecule starts the pocket's next one in the following
step (include/singa_hip_stream.h states the rule).  Every row is at a position of its own, so the step is: the per-row token
input, the decoder layers with `singa_dec_self_attn_rows`, the projection, `ops.sample_token_stream` (the choice of `sample`,
with the uniform and the bookkeeping indexed by the row's molecule) and `ops.stream_refill` (the hand-over, which is also
where positions move) - one captured graph.  A molecule is a function of its pocket, the pocket's property prompt, the
settings and its own column of the uniforms, so the result is `sample`'s, bit for bit, whatever the row budget.

What the loops share is written once: `_prologue` (the checks and figures both start from), `BeamSearch.encode_pockets`,
`BeamSearch.capture_steps` (warm-up on a side stream, one HIP graph per step body) and `_decode` (replay, count, poll).
"""
import numpy as np
import torch

from .. import ops, smiles
from .BeamSearch import KVDecoder, capture_steps, encode_pockets

LIVE_POLL = 16          # tokens between two reads of the live-row counter


def cache_bytes(decoder, rows, positions):
    a = decoder.layers[0].dec_self_attn
    return len(decoder.layers) * rows * positions * (a.key_channels + a.hidden_channels) * 4


def check_tiles(fn, decoder, positions, fused):
    """`tiles=True` of `fn` before any device work: the row-tiled step kernels are a form of the fused step and are built for the
    shipped decoder geometry and at most 256 positions (`KVDecoder` checks the same, but only once the encoder has run)."""
    a0, f0 = decoder.layers[0].dec_self_attn, decoder.layers[0].pos_ffn
    if fused is not None and not fused:
        raise ValueError(f"{fn}: tiles=True is a form of the fused step, fused=False contradicts it")
    if not (a0.hidden_channels == 256 and a0.key_channels == 128 and a0.num_heads == 4 and f0.conv1.out_channels == 1024
            and positions <= 256):
        raise ValueError(f"{fn}: tiles=True needs the shipped decoder geometry and at most 256 positions")


def _prologue(fn, model, smiVoc, num_samples, batch_size, max_length, example, device, grammar, suppress):
    """What `sample` and `sample_distinct` (`fn`: the caller's name, for the messages) check and work out alike before they
    differ -> (device, transformer, vocabulary, (sos, eos, pad), rows, 1 with a property prompt else 0, cache positions, free
    bytes on the device, the grammar's class bytes or None, the [V] uint8 mask of `suppress` on the device or None)."""
    dev = torch.device(device)
    if dev.type != "cuda" or not example.protein_atom_feature.is_cuda:
        raise RuntimeError(f"{fn} runs on the GPU only (no CPU fallback): device and the example's tensors must be cuda")
    if num_samples < 1 or batch_size < 1 or max_length < 2:
        raise ValueError(f"{fn}: num_samples >= 1, batch_size >= 1, max_length >= 2 (got {num_samples}, {batch_size}, {max_length})")
    cls = smiles.check_arguments(grammar, smiVoc, max_length, suppress)
    tf = model.model
    voc = list(smiVoc)
    marks = voc.index("&"), voc.index("$"), voc.index("^")
    rows = batch_size * num_samples
    num = 1 if tf.decoder.num_props else 0
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    allowed = None
    if suppress:
        allowed = torch.ones(len(voc), dtype=torch.uint8)
        allowed[[voc.index(s) for s in suppress]] = 0
        allowed = allowed.to(dev)
    return dev, tf, voc, marks, rows, num, max_length - 1 + num, free, cls, allowed


def _valence_operands(grammar, smiVoc, rows, dev):
    """-> (the [V] uint8 capacities, the rows' [rows, 2] int32 valence words) on the device under grammar="valence", else
    (None, None).  The words are zeroed once and never reset: a row whose rule state is fresh reads them as 0."""
    if grammar != "valence":
        return None, None
    return torch.as_tensor(smiles.capacity(smiVoc)).to(dev), torch.zeros(rows, 2, dtype=torch.int32, device=dev)


def _decode(replays, max_steps, live, each=None):
    """Replay the step - `replays` in turn - up to `max_steps` times; `each()`, if given, after every step; every `LIVE_POLL`
    steps `live()` reads the device's count of live rows, and zero ends the loop.  Returns the steps taken."""
    steps = 0
    while steps < max_steps:
        replays[steps % len(replays)]()
        steps += 1
        if each is not None:
            each()
        if steps % LIVE_POLL == 0 and live() == 0:
            break
    return steps


@torch.no_grad()
def sample(model, smiVoc, num_samples, batch_size, max_length, example, prop=None, device="cuda", temperature=1.0, top_k=0,
           top_p=1.0, suppress=(), generator=None, uniforms=None, graph=True, fused=None, trace=None, grammar=None, forced=None,
           tiles=False):
    """`num_samples` sequences for each of the `batch_size` pockets of `example`, drawn token by token from the model's own
    distribution reshaped by `temperature` (0 = greedy), `top_k` (0 = off) and `top_p` (1 = off).

    `model`, `smiVoc`, `example`, `prop` ([batch_size * num_samples, num_props]; position 0 is the property prompt) and `device`
    as in `beam_search`.  `suppress`: tokens never to be drawn.  `generator`: torch.Generator for the uniforms (CPU or device);
    `uniforms` [max_length, rows] f32 in [0, 1) replaces the draw (row t is read by the step that writes column t + 1).
    `graph=False` launches the step's kernels one by one (same tokens).  `fused`: True = k17 step kernels, False = library
    GEMMs, None = k17 wherever the k17 kernels' limits allow (it is the faster one at every row count measured).  `tiles=True`:
    the row-tiled step kernels (include/singa_hip_dec_tiles.h) instead of k17 - no limit on the pocket's atoms; a ValueError with
    `fused=False` or another decoder geometry.

    Returns the int64 token matrix [batch_size * num_samples, max_length], pocket-major: a row starts with '&', ends with
    '$' if the model ended it before `max_length`, and is padded with '^'.  `trace`, if a dict, receives `lengths` (int32:
    tokens drawn per row, the '$' included, '&' not), `sum_logp` (f32: the model's own log-likelihood of the drawn tokens,
    temperature 1 and nothing filtered), `token_logp` [rows, max_length] (per drawn token), `uniforms`, `path`
    ('k17' / 'tiles' / 'library') and `steps` (tokens decoded before every row had ended).

    `grammar="smiles"`: only tokens that keep the row a prefix of a syntactically complete SMILES string which still fits
    into `max_length` (>= 3) are drawn, so every row ends with '$'.  `token_logp` / `sum_logp` stay the unconstrained model's;
    `trace` also receives `allowed_logp` [rows, max_length]: log of the model's probability mass on the tokens the rule (and
    `suppress`) allowed at that step, so that token_logp - allowed_logp is the log-probability under the constrained proposal.
    ValueError for an unknown grammar, max_length < 3, or a `suppress` that removes every atom, '$', or ')' but not '('.
    `grammar="valence"`: the same, and no atom of a row carries more bond order than `smiles.capacity` gives its token;
    `allowed_logp` is then the mass on that stricter mask.  ValueError also for a `suppress` that leaves no atom of capacity >= 4.

    `forced`: int64 tensor or array [rows, max_length] or [batch_size, max_length] (one prefix per pocket, repeated for its
    `num_samples` rows), `smiles.encode` builds it: a value inside the vocabulary in column c is the token of column c, given
    instead of drawn - with the same bookkeeping, so `token_logp` / `sum_logp` hold the model's log-probability of it - and any
    other value (-1) leaves the column to the draw.  A row's forced columns are one run from column 1: a scaffold to continue,
    or, with its '$', a whole molecule to score (`score`).  `smiles.check_forced` refuses anything else, and under `grammar` a
    prefix the rule does not allow or that cannot be finished in `max_length`, with a ValueError before any device work.
    `trace` also receives `rank` [rows, max_length] int32: the rank of every emitted token among the row's raw logits (0 = the
    arg-max; 0 behind a row's end).  Free columns are drawn exactly as without `forced`, from the same uniforms."""
    dev, tf, voc, (sos, eos, pad), rows, num, positions, free, cls, allowed = _prologue(
        "sample", model, smiVoc, num_samples, batch_size, max_length, example, device, grammar, suppress)
    if temperature < 0 or top_k < 0 or not 0 < top_p <= 1:
        raise ValueError(f"sample: temperature >= 0, top_k >= 0, 0 < top_p <= 1 (got {temperature}, {top_k}, {top_p})")
    if forced is not None:
        forced = forced.cpu().numpy() if torch.is_tensor(forced) else forced
        forced = smiles.check_forced(forced, smiVoc, max_length, grammar)
        if forced.shape[0] == batch_size and num_samples > 1:
            forced = forced.repeat(num_samples, 0)
        if forced.shape[0] != batch_size * num_samples:
            raise ValueError(f"sample: forced has {forced.shape[0]} rows, expected {batch_size * num_samples} (or one per pocket: "
                             f"{batch_size})")
    if tiles:
        check_tiles("sample", tf.decoder, positions, fused)
    need = cache_bytes(tf.decoder, rows, positions)
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

    kv = KVDecoder(tf.decoder, tf.projection, *encode_pockets(tf, example, batch_size), num_samples, positions, len(voc),
                   fused is None or bool(fused), search_buffers=False, tiles=tiles)
    if fused and not kv.fused:
        raise ValueError("sample: fused=True needs the shipped decoder geometry, at most 256 positions and 1024 pocket atoms")
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
    cap, vstate = _valence_operands(grammar, smiVoc, rows, dev)
    if forced is not None:
        forced = torch.as_tensor(forced).to(dev).contiguous()          # uploaded once; the step indexes it with the device's position
        state["rank"] = torch.empty(rows, max_length, dtype=torch.int32, device=dev)

    def start():
        state["tokens"].fill_(pad)
        state["tokens"][:, 0] = sos
        state["next"].fill_(sos)
        state["finished"].zero_(), state["length"].zero_(), state["sum_logp"].zero_(), state["tok_logp"].zero_()
        state["live"].fill_(rows)
        if grammar is not None:
            state["grammar"].fill_(smiles.FRESH), state["allowed_logp"].zero_()
        if forced is not None:
            state["rank"].zero_()
        kv.reset()

    def prime():
        start()
        kv.pos += num

    def step():
        out = kv.advance(kv.token_input(state["next"]))
        ops.sample_token(tf.projection(out).contiguous(), uniforms, kv.pos, num + 1, state, float(temperature), int(top_k),
                         float(top_p), eos, pad, allowed, cls=cls, forced=forced, cap=cap, vstate=vstate)

    replays = capture_steps(prime, [step], 2) if graph else [step]     # two warm-up steps, as KVDecoder.capture
    start()
    if num:
        kv.advance(kv.prop_input(prop.to(dev).float()))                # position 0 is the property prompt, CP:404-412
    # one 4-byte copy per poll: zero when every row has drawn its '$'
    steps = _decode(replays, max_length - 1, lambda: int(state["live"].item()))
    if trace is not None:
        trace.update(lengths=state["length"], sum_logp=state["sum_logp"], token_logp=state["tok_logp"], uniforms=uniforms,
                     path="tiles" if kv.tiles else "k17" if kv.fused else "library", steps=steps)
        if grammar is not None:
            trace.update(allowed_logp=state["allowed_logp"])
        if forced is not None:
            trace.update(rank=state["rank"])
    return state["tokens"]


def score(model, smiVoc, molecules, batch_size, example, prop=None, device="cuda", max_length=None, grammar=None, fused=None,
          rows_per_pocket=None, tiles=False):
    """The model's own log-likelihood of given molecules: `molecules[b]` is the list of SMILES strings (or token lists, as
    `smiles.encode` takes them) to score for pocket b of `example`; the lists may differ in length.  Every molecule is one row
    of `sample` with all its columns forced up to and including '$', so a score comes from the same kernels, in the same
    order, as the `sum_logp` that `sample` reports for a drawn row.  Shorter lists are padded with empty rows (forced to '$'
    in column 1), which are dropped from the result.  `max_length`: default the longest molecule + 2 ('&' and '$').  `prop`:
    [num_props] or [batch_size, num_props] (one prompt per pocket) or one row per molecule slot
    [batch_size * longest list, num_props].

    Returns a dict of per-pocket lists, one entry per molecule in the order given: `sum_logp` (float), `length` (tokens, the
    '$' included), `token_logp` and `rank` (arrays of `length` entries: per token, '$' last; rank 0 = the model's arg-max,
    so the mean of rank == 0 is the top-1 accuracy) and, under `grammar`, `allowed_logp`.  ValueError before any launch for a
    molecule the vocabulary cannot spell, one that does not fit `max_length`, or, under `grammar`, one the rule refuses.

    `rows_per_pocket`: the molecules go through `sample_stream` on that many rows per pocket instead - the caches are those of
    the rows, not of the library, and a row that has ended a short molecule starts the pocket's next one.  The same dict comes
    back, bit for bit.  `prop` is then one prompt per pocket ([num_props] or [batch_size, num_props]); a prompt per molecule is
    a ValueError (a row keeps its cache position 0 across molecules), and `fused` is not consulted (the k17 step kernels are
    that mode's only path).  `tiles`: handed to `sample` / `sample_stream`; with it the returned dict also holds `path`: "tiles"."""
    dev = torch.device(device)
    if dev.type != "cuda" or not example.protein_atom_feature.is_cuda:
        raise RuntimeError("score runs on the GPU only (no CPU fallback): device and the example's tensors must be cuda")
    if len(molecules) != batch_size:
        raise ValueError(f"score: one list of molecules per pocket: got {len(molecules)} lists for {batch_size} pockets")
    voc = [str(v) for v in smiVoc]
    per = max((len(m) for m in molecules), default=0)
    if per < 1:
        raise ValueError("score: no molecule to score")
    items = []
    for m in molecules:
        items += [smiles.tokenize(x, voc) if isinstance(x, str) else list(x) for x in m] + [[]] * (per - len(m))
    if max_length is None:
        max_length = max(len(x) for x in items) + 2
    forced = smiles.encode(items, voc, max_length, end=True)
    if prop is not None:
        prop = torch.as_tensor(prop).float().reshape(-1, torch.as_tensor(prop).shape[-1])
        if rows_per_pocket is not None:
            if prop.shape[0] not in (1, batch_size):
                raise ValueError(f"score: with rows_per_pocket, prop is one prompt per pocket ([num_props] or [{batch_size}, num_props]); "
                                 f"a prompt per molecule is unsupported there (got {prop.shape[0]} rows)")
            prop = prop.repeat(batch_size, 1) if prop.shape[0] == 1 and batch_size > 1 else prop
        elif prop.shape[0] == 1:
            prop = prop.repeat(batch_size * per, 1)
        elif prop.shape[0] == batch_size and per > 1:
            prop = prop.repeat_interleave(per, 0)
    tr = {}
    uniforms = torch.zeros(max_length, batch_size * per)
    if rows_per_pocket is not None:
        sample_stream(model, smiVoc, per, batch_size, max_length, example, prop, rows_per_pocket, device=device, uniforms=uniforms,
                      trace=tr, grammar=grammar, forced=forced, tiles=tiles)
    else:
        sample(model, smiVoc, per, batch_size, max_length, example, prop, device=device, uniforms=uniforms, fused=fused, trace=tr,
               grammar=grammar, forced=forced, tiles=tiles)
    keys = {"token_logp": "token_logp", "rank": "rank"}
    if grammar is not None:
        keys["allowed_logp"] = "allowed_logp"
    host = {k: tr[v].cpu().numpy() for k, v in keys.items()}
    lengths, sums = tr["lengths"].cpu().numpy(), tr["sum_logp"].cpu().numpy()
    out = {k: [] for k in ("sum_logp", "length", *keys)}
    for b, m in enumerate(molecules):
        rows = range(b * per, b * per + len(m))
        out["sum_logp"].append([float(sums[r]) for r in rows])
        out["length"].append([int(lengths[r]) for r in rows])
        for k in keys:
            out[k].append([host[k][r, 1:1 + lengths[r]].copy() for r in rows])
    if tiles:
        out["path"] = tr["path"]
    return out


STREAM_MAX_ROWS = 2048  # rows per pocket singa_stream_refill is built for


@torch.no_grad()
def sample_stream(model, smiVoc, num_samples, batch_size, max_length, example, prop=None, rows_per_pocket=64, device="cuda",
                  temperature=1.0, top_k=0, top_p=1.0, suppress=(), generator=None, uniforms=None, graph=True, trace=None,
                  grammar=None, forced=None, tiles=False):
    """`sample` on a fixed budget of rows: `num_samples` molecules for each of the `batch_size` pockets of `example`, decoded on
    batch_size * `rows_per_pocket` rows; a row that has ended its molecule ('$', or the last column) starts the pocket's next
    one in the following step, until the pocket has none left (include/singa_hip_stream.h states the rule).  Rows that have
    ended cost nothing but the tail of the run, and the key / value caches are those of the rows, not of the molecules.

    `model`, `smiVoc`, `example`, `device`, `temperature`, `top_k`, `top_p`, `suppress`, `graph` and `grammar` as in `sample`.
    `prop`: [batch_size, num_props], ONE property prompt per pocket (a row keeps cache position 0 across its molecules).
    `uniforms`: [max_length, batch_size * num_samples] f32, column j belongs to MOLECULE j (row t is read by the step that
    writes the molecule's column t + 1); drawn once per call from `generator` if not given.

    Returns the int64 token matrix [batch_size * num_samples, max_length], pocket-major, with `sample`'s conventions.  Molecule
    j is a function of its pocket, the pocket's prompt, the settings and uniforms[:, j] alone: the result does not depend on
    `rows_per_pocket` and equals, bit for bit, what `sample` returns for `num_samples` rows per pocket given the same uniforms
    and `prop` repeated per row - tokens and everything `trace` receives: `lengths`, `sum_logp`, `token_logp`, `uniforms`,
    `path`, `steps` (steps of the run) and, under `grammar`, `allowed_logp`, all indexed by molecule, plus `row_of` (int32: the
    row that decoded the molecule) and `start_step` (int32: the step of the run, from 0, that chose its first token).

    `forced`: as in `sample`, int64 [batch_size * num_samples, max_length], one row per MOLECULE, or [batch_size, max_length]
    (one prefix per pocket, repeated for its molecules); `smiles.check_forced` validates it (a matrix that is not of an integer
    type is a TypeError here).  `ops.sample_token_stream`, given
    the matrix, runs `singa_sample_token_stream_forced` (include/singa_hip_prefix.h states the rule): the row that decodes
    molecule j reads row j of the matrix at its own position.  `trace` then also receives `rank`, per molecule, and the result
    still equals `sample(forced=...)`'s bit for bit.

    ValueError before any device work for a `prop` of another shape, `rows_per_pocket` outside 1..2048, a decoder geometry,
    length or pocket size the k17 step kernels are not built for (they are the only path), and a run whose caches and
    per-molecule buffers (`forced` and `rank` included) do not fit the free memory.

    `tiles=True`: the row-tiled step kernels (include/singa_hip_dec_tiles.h) instead of k17; the limit on the pocket's atoms does
    not apply to them, and `trace["path"]` says "tiles"."""
    dev, tf, voc, (sos, eos, pad), mols, num, positions, free, cls, allowed = _prologue(
        "sample_stream", model, smiVoc, num_samples, batch_size, max_length, example, device, grammar, suppress)
    R, V = int(rows_per_pocket), len(voc)
    if temperature < 0 or top_k < 0 or not 0 < top_p <= 1:
        raise ValueError(f"sample_stream: temperature >= 0, top_k >= 0, 0 < top_p <= 1 (got {temperature}, {top_k}, {top_p})")
    if not 1 <= R <= STREAM_MAX_ROWS:
        raise ValueError(f"sample_stream: rows_per_pocket of 1..{STREAM_MAX_ROWS} is supported (got {rows_per_pocket})")
    if num and (prop is None or tuple(prop.shape) != (batch_size, tf.decoder.num_props)):
        raise ValueError(f"sample_stream: prop must be [batch_size, num_props] = [{batch_size}, {tf.decoder.num_props}], one prompt "
                         f"per pocket; a prompt per row is unsupported (got {None if prop is None else tuple(prop.shape)})")
    a0, f0 = tf.decoder.layers[0].dec_self_attn, tf.decoder.layers[0].pos_ffn
    atoms = int(torch.bincount(example.protein_element_batch.cpu().long()).max())
    if not (a0.hidden_channels == 256 and a0.key_channels == 128 and a0.num_heads == 4 and f0.conv1.out_channels == 1024
            and positions <= 256 and (tiles or atoms <= 1024) and V <= 1024):
        raise ValueError("sample_stream: unsupported decoder geometry - the k17 step kernels are the only path: the shipped "
                         "decoder geometry, at most 256 positions, 1024 pocket atoms and 1024 tokens")
    if forced is not None:
        forced = forced.cpu().numpy() if torch.is_tensor(forced) else np.asarray(forced)
        if forced.dtype.kind not in "iu":
            raise TypeError(f"sample_stream: forced holds token ids, an integer matrix is expected (got {forced.dtype})")
        forced = smiles.check_forced(forced, smiVoc, max_length, grammar)
        if forced.shape[0] == batch_size and num_samples > 1:
            forced = forced.repeat(num_samples, 0)
        if forced.shape[0] != mols:
            raise ValueError(f"sample_stream: forced has {forced.shape[0]} rows, expected one per molecule: {mols} (or one per "
                             f"pocket: {batch_size})")
    rows = batch_size * R
    need = cache_bytes(tf.decoder, rows, positions) + mols * max_length * (8 + 4 + 4 + 4 + (8 + 4 if forced is not None else 0))
    if need + (64 << 10) * rows > free:                  # + the step's activations, as in `sample`
        raise ValueError(f"sample_stream: the key / value caches of {rows} rows x {positions} positions and the outputs and "
                         f"uniforms of {mols} molecules take {need} bytes, {free} bytes are free on {dev}: unsupported - use "
                         f"fewer rows per pocket or draw fewer molecules per call")
    if uniforms is None:
        gdev = generator.device if generator is not None else dev
        uniforms = torch.rand((max_length, mols), generator=generator, device=gdev, dtype=torch.float32)
    if tuple(uniforms.shape) != (max_length, mols) or uniforms.dtype != torch.float32:
        raise ValueError(f"sample_stream: uniforms must be float32 [max_length, molecules] = [{max_length}, {mols}], got "
                         f"{uniforms.dtype} {tuple(uniforms.shape)}")
    uniforms = uniforms.to(dev).contiguous()

    kv = KVDecoder(tf.decoder, tf.projection, *encode_pockets(tf, example, batch_size), R, positions, V, True, search_buffers=False,
                   tiles=tiles)
    if not kv.fused:
        raise ValueError("sample_stream: unsupported decoder geometry for the k17 step kernels")
    i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
    state = {"tokens": torch.empty(mols, max_length, dtype=torch.int64, device=dev), "tok_logp": torch.empty(mols, max_length, **f32),
             "length": torch.empty(mols, **i32), "sum_logp": torch.empty(mols, **f32), "row_of": torch.empty(mols, **i32),
             "start_step": torch.empty(mols, **i32), "next": torch.empty(rows, dtype=torch.int64, device=dev),
             "pos": torch.empty(rows, dtype=torch.int64, device=dev), "mol": torch.empty(rows, **i32),
             "issued": torch.empty(batch_size, **i32), "live": torch.empty(batch_size, **i32)}
    if grammar is not None:
        cls = torch.as_tensor(cls).to(dev)
        state["grammar"] = torch.empty(rows, **i32)
        state["allowed_logp"] = torch.empty(mols, max_length, **f32)
    cap, vstate = _valence_operands(grammar, smiVoc, rows, dev)
    if forced is not None:
        forced = torch.as_tensor(forced).to(dev).contiguous()          # uploaded once, indexed by molecule and position
        state["rank"] = torch.empty(mols, max_length, **i32)
    # the start of a run: the first min(R, num_samples) rows of pocket b hold its first molecules, the others are retired
    first = min(R, num_samples)
    mol0 = np.full((batch_size, R), -1, np.int32)
    mol0[:, :first] = np.arange(batch_size)[:, None] * num_samples + np.arange(first)[None]
    row0 = np.zeros((batch_size, num_samples), np.int32)
    row0[:, :first] = np.arange(batch_size)[:, None] * R + np.arange(first)[None]
    mol0, row0 = torch.as_tensor(mol0.reshape(-1)).to(dev), torch.as_tensor(row0.reshape(-1)).to(dev)

    def start():
        state["tokens"].fill_(pad)
        state["tokens"][:, 0] = sos
        state["next"].fill_(sos)
        state["length"].zero_(), state["sum_logp"].zero_(), state["tok_logp"].zero_(), state["start_step"].zero_()
        state["mol"].copy_(mol0), state["row_of"].copy_(row0)
        state["pos"].fill_(num)
        state["issued"].fill_(first), state["live"].fill_(first)
        if grammar is not None:
            state["grammar"].fill_(smiles.FRESH), state["allowed_logp"].zero_()
        if forced is not None:
            state["rank"].zero_()
        kv.reset()

    def step():
        out = kv.advance(kv.token_input(state["next"], state["pos"]), row_pos=state["pos"])
        ops.sample_token_stream(tf.projection(out).contiguous(), uniforms, state["pos"], state["mol"], num, state, float(temperature),
                                int(top_k), float(top_p), eos, pad, allowed, cls=cls, cap=cap, vstate=vstate, forced=forced)
        ops.stream_refill(state["pos"], state["mol"], num, state, R, num_samples, max_length, sos, eos, smiles.FRESH,
                          grammar is not None)

    replays = capture_steps(start, [step], 2) if graph else [step]
    start()
    if num:                                                            # position 0 of every row is its pocket's property prompt
        kv.advance(kv.prop_input(prop.to(dev).float().repeat_interleave(R, 0)))
    live = lambda: int(state["live"].sum().item())
    steps = _decode(replays, (-(-num_samples // R) + 1) * (max_length - 1), live)
    if live() != 0:
        raise RuntimeError(f"sample_stream: {live()} rows still hold a molecule after {steps} steps")
    if trace is not None:
        trace.update(lengths=state["length"], sum_logp=state["sum_logp"], token_logp=state["tok_logp"], uniforms=uniforms,
                     path="tiles" if kv.tiles else "k17", steps=steps, row_of=state["row_of"], start_step=state["start_step"])
        if grammar is not None:
            trace.update(allowed_logp=state["allowed_logp"])
        if forced is not None:
            trace.update(rank=state["rank"])
    return state["tokens"]


SWOR_MAX_K = 2048       # slots per pocket singa_swor_select is built for


@torch.no_grad()
def sample_distinct(model, smiVoc, num_samples, batch_size, max_length, example, prop=None, device="cuda", temperature=1.0,
                    suppress=(), grammar=None, seed=0, streams=None, graph=True, trace=None, forced=None, tiles=False):
    """Up to `num_samples` pairwise DISTINCT sequences for each of the `batch_size` pockets of `example`: a sample without
    replacement from the model's distribution reshaped by `temperature` (> 0), `suppress` and `grammar` ("smiles", as in `sample`;
    "valence" is a ValueError here), by
    stochastic beam search on the device (include/singa_hip_swor.h states the rule).  `model`, `smiVoc`, `example`, `prop`
    and `device` as in `sample`; the rows of a pocket exchange prefixes, so they are expected to carry one property prompt.

    All randomness is a function of (`seed`, the pocket's entry of `streams`, the prefix): `seed` is a 64-bit integer,
    `streams` [batch_size] 32-bit integers (default 0, 1, ...), so a pocket's result does not depend on its neighbours in the
    batch, and the k best of a run with more slots are the run with k slots.  `graph=False` launches the step's kernels one
    by one (same result).  Only the k17 step kernels serve this mode.

    Returns the int64 token matrix [batch_size * num_samples, max_length], pocket-major, a pocket's rows in descending order
    of their perturbed log-probability G.  A pocket whose tree has fewer than `num_samples` leaves leaves trailing slots dead.
    `trace`, if a dict, receives `gumbel` (G, -inf for dead slots), `prop_logp` (log-probability under the proposal),
    `sum_logp` / `token_logp` (the unmodified model's, as `sample` and `score` report them), `lengths`, `valid` (uint8: 0 for
    dead slots) and `steps`.  A list handed in as `trace["gumbel_history"]` receives a copy of G [rows] after every step:
    G[k - 1] - G[k] of a run with one slot more bounds the margin by which the k-slot run's selections were decided.

    `forced`: int64 [batch_size, max_length], ONE prefix per pocket (`smiles.encode` builds it, `smiles.check_prefix` validates
    it: one run of tokens from column 1 without '$', at least one free column, under `grammar` a prefix the rule accepts and
    can finish): every sequence of the pocket starts with it - distinct completions of a scaffold.  `ops.swor_expand`, given
    the matrix, runs `singa_swor_expand_forced` (include/singa_hip_prefix.h states the rule): through the prefix a pocket
    keeps one slot with G = 0.  `sum_logp` / `token_logp` include the prefix and stay `score`'s bit for bit; `prop_logp` is the
    log-probability under the proposal CONDITIONAL on the prefix, so `swor_weights` of such a run estimates expectations over
    the completions of the prefix, not over all sequences.  A matrix without a forced column gives the bits of `forced=None`.

    ValueError before any launch for temperature <= 0, num_samples > 2048, a decoder geometry,
    length or pocket size the k17 kernels are not built for, and caches (two buffers) that do not fit the free memory.

    `tiles=True`: the row-tiled step kernels (include/singa_hip_dec_tiles.h) instead of k17; the limit on the pocket's atoms does
    not apply to them, and `trace` also receives `path`: "tiles"."""
    if grammar == "valence":
        raise ValueError("sample_distinct: grammar='valence' is unsupported (the selection gathers one state word per row); use "
                         "grammar='smiles' here, or `sample` / `sample_stream` for the valence rule")
    dev, tf, voc, (sos, eos, pad), rows, num, positions, free, cls, allowed = _prologue(
        "sample_distinct", model, smiVoc, num_samples, batch_size, max_length, example, device, grammar, suppress)
    k, V = num_samples, len(voc)
    if not temperature > 0:
        raise ValueError(f"sample_distinct: temperature > 0 (got {temperature}): the perturbation needs a proper distribution")
    if num_samples > SWOR_MAX_K:
        raise ValueError(f"sample_distinct: at most {SWOR_MAX_K} samples per pocket (got {num_samples})")
    a0, f0 = tf.decoder.layers[0].dec_self_attn, tf.decoder.layers[0].pos_ffn
    atoms = int(torch.bincount(example.protein_element_batch.cpu().long()).max())
    if not (a0.hidden_channels == 256 and a0.key_channels == 128 and a0.num_heads == 4 and f0.conv1.out_channels == 1024
            and positions <= 256 and (tiles or atoms <= 1024) and V <= 1024):
        raise ValueError("sample_distinct: the k17 step kernels are the only path: the shipped decoder geometry, at most 256 "
                         "positions, 1024 pocket atoms and 1024 tokens")
    if streams is None:
        streams = np.arange(batch_size)
    streams = np.asarray(streams.cpu() if torch.is_tensor(streams) else streams).astype(np.int64)
    if streams.shape != (batch_size,) or (streams < 0).any() or (streams >= 2 ** 32).any():
        raise ValueError(f"sample_distinct: streams holds one 32-bit integer per pocket, got shape {streams.shape}")
    need = 2 * cache_bytes(tf.decoder, rows, positions) + 3 * rows * V * 4 + 2 * rows * max_length * 12
    if need + (64 << 10) * rows > free:                  # + the step's activations, as in `sample`
        raise ValueError(f"sample_distinct: the two key / value cache buffers of {rows} rows x {positions} positions and the "
                         f"candidates take {need} bytes, {free} bytes are free on {dev}: draw fewer samples per call")
    streams = torch.as_tensor(streams.astype(np.uint32).view(np.int32)).to(dev)
    if forced is not None:
        forced = forced.cpu().numpy() if torch.is_tensor(forced) else forced
        forced = torch.as_tensor(smiles.check_prefix(forced, smiVoc, batch_size, max_length, grammar)).to(dev).contiguous()

    kv = KVDecoder(tf.decoder, tf.projection, *encode_pockets(tf, example, batch_size), k, positions, V, True, search_buffers=False,
                   tiles=tiles)
    bufs = ((kv.k, kv.v), (torch.zeros_like(kv.k), torch.zeros_like(kv.v)))
    f32 = dict(dtype=torch.float32, device=dev)
    state = {"gumbel": torch.empty(rows, **f32), "prop_logp": torch.empty(rows, **f32), "sum_logp": torch.empty(rows, **f32),
             "hash": torch.empty(rows, dtype=torch.int64, device=dev), "finished": torch.empty(rows, dtype=torch.uint8, device=dev),
             "length": torch.empty(rows, dtype=torch.int32, device=dev),
             "tokens": torch.empty(rows, max_length, dtype=torch.int64, device=dev), "tok_logp": torch.empty(rows, max_length, **f32),
             "next": torch.empty(rows, dtype=torch.int64, device=dev), "src": torch.empty(rows, dtype=torch.int64, device=dev),
             "live": torch.empty(batch_size, dtype=torch.int32, device=dev), "cand": torch.empty(rows, V, **f32),
             "cand_logp": torch.empty(rows, V, **f32), "cand_phi": torch.empty(rows, V, **f32)}
    if grammar is not None:
        cls = torch.as_tensor(cls).to(dev)
        state["grammar"] = torch.empty(rows, dtype=torch.int32, device=dev)
    work = ops.swor_work(rows, max_length, dev)

    def start():
        state["tokens"].fill_(pad)
        state["tokens"][:, 0] = sos
        state["next"].fill_(sos)
        state["gumbel"].fill_(float("-inf")), state["prop_logp"].fill_(float("-inf"))
        state["gumbel"].view(batch_size, k)[:, 0] = 0                  # slot 0 of every pocket is the root
        state["prop_logp"].view(batch_size, k)[:, 0] = 0
        state["sum_logp"].zero_(), state["hash"].zero_(), state["finished"].zero_(), state["length"].zero_()
        state["tok_logp"].zero_(), state["src"].zero_()
        state["live"].fill_(1)
        if grammar is not None:
            state["grammar"].fill_(smiles.FRESH)
        kv.reset()

    def step(parity):
        (ck, cv), (ok, ov) = bufs[parity], bufs[1 - parity]
        out = kv.advance(kv.token_input(state["next"]), ck, cv)
        ops.swor_expand(tf.projection(out).contiguous(), kv.pos, num + 1, state, k, streams, float(temperature), int(seed), pad,
                        allowed, cls, forced=forced)
        ops.swor_select(kv.pos, num + 1, state, k, work, eos, pad, cls)
        ops.swor_follow(ck, cv, ok, ov, state["src"], state["gumbel"], state["finished"], kv.pos)

    def prime():
        start()
        kv.pos += num

    replays = [lambda: step(0), lambda: step(1)]                       # the step on each pair of cache buffers, taken in turn
    if graph:
        replays = capture_steps(prime, replays, 1)
    start()
    if num:
        kv.advance(kv.prop_input(prop.to(dev).float()))                # position 0 is the property prompt, in the first buffer
    history = trace.get("gumbel_history") if trace is not None else None
    steps = _decode(replays, max_length - 1, lambda: int(state["live"].sum().item()),
                    (lambda: history.append(state["gumbel"].clone())) if history is not None else None)
    if trace is not None:
        trace.update(gumbel=state["gumbel"], prop_logp=state["prop_logp"], sum_logp=state["sum_logp"], token_logp=state["tok_logp"],
                     lengths=state["length"], valid=(state["gumbel"] > float("-inf")).to(torch.uint8), steps=steps)
        if tiles:
            trace.update(path="tiles")
    return state["tokens"]


def swor_weights(prop_logp, gumbel, valid):
    """The importance weights of a `sample_distinct` run (Kool et al. 2019, section 4.2): per pocket (one row of the 2-D
    arguments), kappa is the smallest G among the valid slots; the slot at kappa gets weight 0 and every other valid slot
    1 / q with q = 1 - exp(-exp(phi - kappa)), the probability that its perturbed score exceeds kappa.  sum_i w_i f(s_i) is
    then an unbiased estimate of E[f] under the proposal.  float64 arrays [pockets, k] in, float64 weights out (0 for dead
    slots)."""
    phi, g = np.asarray(prop_logp, np.float64), np.asarray(gumbel, np.float64)
    ok = np.asarray(valid).astype(bool)
    if phi.ndim != 2 or phi.shape != g.shape or ok.shape != g.shape:
        raise ValueError(f"swor_weights: three arrays [pockets, k], got {phi.shape}, {g.shape}, {ok.shape}")
    w = np.zeros_like(phi)
    for b in range(phi.shape[0]):
        idx = np.flatnonzero(ok[b])
        if len(idx) == 0:
            continue
        at = idx[np.argmin(g[b, idx])]
        rest = idx[idx != at]
        w[b, rest] = 1.0 / -np.expm1(-np.exp(phi[b, rest] - g[b, at]))
    return w
