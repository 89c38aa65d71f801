"""Beam-search generation for MI355X (reference model/BeamSearch.py = "BS", driven by gen.py:156-196).

Same entry point and arguments as the reference - `beam_search(model, smiVoc, num_beams, batch_size, max_length, topk,
example, prop, device)` returning the decoded token matrix - and the same selection rules, so the same hypotheses
survive (see `_select` for the rules that are easy to get subtly different).  What is different is where the time goes:

  * the reference re-runs the whole decoder on the growing prefix for every new token (BS:82, O(T^2) positions);
    here each decoder layer keeps its self-attention keys / values per live beam (`KVDecoder`), so a step evaluates ONE
    position per beam, and the caches follow the beams when they are re-ranked;
  * the reference copies the encoder output once per beam (BS:78-79, 135-136) and recomputes its key / value
    projections in every layer at every step; here they are projected once per protein, and the beams of a protein
    form the query rows of one batched matmul against them - nothing is replicated or re-gathered;
  * one device->host transfer per step (the 2*num_beams ranked candidates of every protein) instead of an `.item()`
    per candidate (BS:107-122).

The device work of a step is GEMMs (library calls through ops.linear), softmax / layer norm / top-k (library ops) on
[rows, 256] operands; hypothesis bookkeeping stays on the host, as in the reference.

`beam_search_device` is a second search beside it: the same selection rules as kernels inside the captured step
(`ops.beam_expand`, `ops.beam_select`; include/singa_hip_beam.h states the rule), the hypotheses kept on the device, nothing
copied per token - and therefore able to take the SMILES and the valence rule of the samplers (`grammar=`).  `beam_search`,
its defaults and its host path are the ones pinned to the reference's goldens and stay as they are.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from .. import ops


class BeamHypotheses(object):
    """The `num_beams` best finished sequences of one protein (BS:7-35)."""

    def __init__(self, num_beams, max_length, length_penalty):
        self.max_length = max_length - 1
        self.length_penalty = length_penalty
        self.num_beams = num_beams
        self.beams = []
        self.worst_score = 1e9

    def __len__(self):
        return len(self.beams)

    def add(self, hyp, sum_logprobs):
        score = sum_logprobs / len(hyp) ** self.length_penalty
        if len(self) >= self.num_beams and score <= self.worst_score:
            return
        self.beams.append((score, hyp))
        if len(self) > self.num_beams:
            order = sorted((s, i) for i, (s, _) in enumerate(self.beams))
            del self.beams[order[0][1]]
            self.worst_score = order[1][0]
        else:
            self.worst_score = min(score, self.worst_score)

    def is_done(self, best_sum_logprobs, cur_len):
        if len(self) < self.num_beams:
            return False
        return self.worst_score >= best_sum_logprobs / cur_len ** self.length_penalty


class KVDecoder:
    """Incremental evaluation of `Decoder` (CP:385-423): one new position per row and call, self-attention keys / values
    cached per layer, encoder keys / values projected once per protein.

    rows = proteins x beams, protein-major (row r belongs to protein r // beams, as BS:105).  Causality makes the result
    for the newest position identical to the reference's full re-run on the prefix; the padding mask of the self-
    attention (CP:414) never fires for a live beam because a live prefix contains no '^'.

    Every tensor has a fixed shape: the caches span `max_positions`, the current position is a device scalar, and
    attention masks the positions that are not written yet.  A whole search step (`step`: re-rank the caches, embed
    the chosen tokens, all decoder layers, vocabulary projection, log-softmax, candidate top-k) is therefore one HIP
    graph, captured once per search and replayed per token."""

    def __init__(self, decoder, projection, enc_outputs, enc_pad_mask, beams, max_positions, vocab_size, fused=True,
                 search_buffers=True, tiles=False):
        """search_buffers=False leaves out the beam step's own input / output buffers (`step_in`, `step_out`, `logp`): the
        sampling loop (model/Sampling.py) only uses `token_input` / `prop_input` / `advance`.  `tiles=True`: the fused step is the
        row-tiled one (include/singa_hip_dec_tiles.h), which has no limit on the pocket's size; ValueError, before any launch,
        with `fused=False` or a decoder the step kernels are not built for."""
        self.dec, self.proj, self.beams, self.V = decoder, projection, beams, vocab_size
        a0, f0 = decoder.layers[0].dec_self_attn, decoder.layers[0].pos_ffn
        # the step kernels are built for the shipped decoder geometry; anything else takes the library path
        geometry = bool(a0.hidden_channels == 256 and a0.key_channels == 128 and a0.num_heads == 4
                        and f0.conv1.out_channels == 1024 and max_positions <= 256)
        self.tiles = bool(tiles)
        if self.tiles and not (fused and geometry):
            raise ValueError("KVDecoder: tiles=True is a form of the fused step: fused=True, the shipped decoder geometry and at most "
                             "256 positions")
        self.fused = bool(fused and geometry and (self.tiles or enc_outputs.shape[1] <= 1024))
        B, S, _ = enc_outputs.shape
        a0 = decoder.layers[0].dec_self_attn
        self.heads = a0.num_heads
        self.dk, self.dv = a0.key_channels // self.heads, a0.hidden_channels // self.heads
        self.B, self.R, self.P = B, B * beams, max_positions
        self.num = 1 if decoder.num_props else 0
        dev = self.dev = enc_outputs.device
        self.cross_k, self.cross_v = [], []
        for layer in decoder.layers:
            c = layer.dec_enc_attn
            self.cross_k.append(c.W_K(enc_outputs).view(B, S, self.heads, self.dk).permute(0, 2, 3, 1).contiguous())
            self.cross_v.append(c.W_V(enc_outputs).view(B, S, self.heads, self.dv).transpose(1, 2).contiguous())
        self.cross_mask = enc_pad_mask.view(B, 1, 1, S)
        self.pad_u8 = enc_pad_mask.reshape(B, S).to(torch.uint8).contiguous()
        # the layers' weights as the fused step kernels (k17) read them: transposed, q/k/v concatenated
        tr = lambda w: w.detach().t().contiguous()
        self.w = []
        for layer in decoder.layers:
            a, c, f = layer.dec_self_attn, layer.dec_enc_attn, layer.pos_ffn
            self.w.append({
                "self": dict(wqkv_t=tr(torch.cat([a.W_Q.weight, a.W_K.weight, a.W_V.weight], 0)),
                             bqkv=torch.cat([a.W_Q.bias, a.W_K.bias, a.W_V.bias]).detach().contiguous(),
                             wo_t=tr(a.linear.weight), bo=a.linear.bias.detach(), gamma=a.layer_norm.weight.detach(),
                             beta=a.layer_norm.bias.detach(), eps=a.layer_norm.eps),
                "cross": dict(wq_t=tr(c.W_Q.weight), bq=c.W_Q.bias.detach(), wo_t=tr(c.linear.weight), bo=c.linear.bias.detach(),
                              gamma=c.layer_norm.weight.detach(), beta=c.layer_norm.bias.detach(), eps=c.layer_norm.eps),
                "ffn": dict(w1_t=tr(f.conv1.weight[:, :, 0]), b1=f.conv1.bias.detach(), w2_t=tr(f.conv2.weight[:, :, 0]),
                            b2=f.conv2.bias.detach(), gamma=f.layer_norm.weight.detach(), beta=f.layer_norm.bias.detach(),
                            eps=f.layer_norm.eps)})
        n = len(decoder.layers)
        self.k = torch.zeros(n, self.R, self.heads, max_positions, self.dk, device=dev)
        self.v = torch.zeros(n, self.R, self.heads, max_positions, self.dv, device=dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=dev)            # next position to be written
        self.slots = torch.arange(max_positions, device=dev)
        self.replay = None                                                 # the captured step's replay, once `capture` has run
        if not search_buffers:
            return
        # the step's inputs (scores, tokens, source rows - one row each, as doubles: exact for fp32 and for indices) and
        # outputs (2*beams ranked candidate scores and flat beam*vocab indices per protein), fixed addresses
        self.step_in = torch.zeros(3, self.R, dtype=torch.float64, device=dev)
        self.step_out = torch.zeros(2, B, 2 * beams, dtype=torch.float64, device=dev)
        self.logp = torch.zeros(self.R, vocab_size, device=dev)

    def reset(self):
        self.pos.zero_()

    def follow(self, src_rows):
        """Row r continues the prefix that row src_rows[r] held (BS:134-136)."""
        self.k.copy_(self.k.index_select(1, src_rows))
        self.v.copy_(self.v.index_select(1, src_rows))

    def token_input(self, tokens, row_pos=None):
        """`row_pos` [rows] int64: one position per row instead of the decoder's own `pos` (`Sampling.sample_stream`)."""
        d = self.dec
        x = d.mol_emb.weight.index_select(0, tokens) + d.pos_emb.pe[:, 0].index_select(0, (self.pos if row_pos is None else row_pos) - self.num)
        return x + d.type_emb.weight[1] if d.num_props else x

    def prop_input(self, prop):
        d = self.dec
        return d.prop_nn(prop) + d.type_emb.weight[0]

    def advance(self, x, k=None, v=None, row_pos=None):
        """x [rows, hidden]: decoder input at position `pos` -> decoder output at that position; pos += 1.  `k`, `v`: the
        caches to append to and attend over instead of the decoder's own (same shapes; `sample_distinct` alternates between
        two pairs of buffers).  `row_pos` [rows] int64: row r is at position row_pos[r] instead, and nothing is advanced - the
        positions are the caller's to move (`Sampling.sample_stream`; the k17 step kernels only)."""
        k, v = self.k if k is None else k, self.v if v is None else v
        if row_pos is not None:
            if not self.fused:
                raise ValueError("KVDecoder.advance: one position per row needs the k17 step kernels (fused)")
            for l in range(len(self.dec.layers)):
                x = ops.dec_layer_step(x.contiguous(), self.w[l], k[l], v[l], row_pos, self.cross_k[l], self.cross_v[l],
                                       self.pad_u8, self.beams, per_row=True, tiles=self.tiles)
            return x
        if self.fused:
            # three hand-written launches per layer (singa_dec_*): q/k/v + cache append + attention + projection + LayerNorm,
            # encoder-decoder attention, feed-forward - instead of ~33 library / elementwise launches on 20-row operands
            for l in range(len(self.dec.layers)):
                x = ops.dec_layer_step(x.contiguous(), self.w[l], k[l], v[l], self.pos, self.cross_k[l],
                                       self.cross_v[l], self.pad_u8, self.beams, tiles=self.tiles)
            self.pos += 1
            return x
        R, B, H = self.R, self.B, self.heads
        unwritten = (self.slots > self.pos).view(1, 1, 1, self.P)
        for l, layer in enumerate(self.dec.layers):
            a = layer.dec_self_attn
            k[l].index_copy_(2, self.pos, a.W_K(x).view(R, H, 1, self.dk))
            v[l].index_copy_(2, self.pos, a.W_V(x).view(R, H, 1, self.dv))
            q = a.W_Q(x).view(R, H, 1, self.dk)
            s = (torch.matmul(q, k[l].transpose(-1, -2)) / math.sqrt(self.dk)).masked_fill(unwritten, float("-inf"))
            ctx = torch.matmul(torch.softmax(s, dim=-1), v[l]).reshape(R, H * self.dv)
            y = a.layer_norm(a.linear(ctx) + x)
            c = layer.dec_enc_attn
            q = c.W_Q(y).view(B, self.beams, H, self.dk).transpose(1, 2)                   # beams = query rows
            s = (torch.matmul(q, self.cross_k[l]) / math.sqrt(self.dk)).masked_fill(self.cross_mask, -1e9)
            ctx = torch.matmul(torch.softmax(s, dim=-1), self.cross_v[l]).transpose(1, 2).reshape(R, H * self.dv)
            x = layer.pos_ffn(c.layer_norm(c.linear(ctx) + y))
        self.pos += 1
        return x

    def _step_body(self):
        scores, tokens, src_rows = self.step_in[0].float(), self.step_in[1].long(), self.step_in[2].long()
        self.follow(src_rows)
        out = self.advance(self.token_input(tokens))
        self.logp.copy_(F.log_softmax(self.proj(out), dim=-1))                               # BS:83-85
        cand = (self.logp + scores[:, None]).view(self.B, self.beams * self.V)               # BS:86-89
        cand_score, cand_flat = torch.topk(cand, 2 * self.beams, dim=1, largest=True, sorted=True)
        self.step_out[0].copy_(cand_score)
        self.step_out[1].copy_(cand_flat)

    def capture(self):
        """Capture `_step_body` into a HIP graph.  The warm-up and the capture itself write cache slots and advance `pos`;
        the caller resets `pos` afterwards, and slots >= pos are never read."""
        self.step_in.zero_()
        self.step_in[2] = torch.arange(self.R, device=self.dev)

        def prime():
            self.reset()
            self.pos += self.num

        self.replay, = capture_steps(prime, [self._step_body], 2)
        self.reset()

    def step(self, scores, tokens, src_rows):
        """One search step for host arrays (scores f32, tokens, source rows) -> (candidate scores f32 [B, 2*beams],
        flat candidate indices int64 [B, 2*beams]) on the host.  One H2D copy, one graph replay, one D2H copy."""
        host = np.stack([scores.astype(np.float64), tokens.astype(np.float64), src_rows.astype(np.float64)])
        self.step_in.copy_(torch.from_numpy(host))
        (self.replay or self._step_body)()
        out = self.step_out.cpu().numpy()
        return out[0].astype(np.float32), out[1].astype(np.int64)


def capture_steps(prime, bodies, warmups):
    """The one place where decode steps become HIP graphs (`KVDecoder.capture`, `Sampling.sample`, `sample_distinct`).
    `prime()` resets the caller's row state and advances `pos` past the property prompt; `bodies` are the steps, each captured
    into a graph of its own.  `warmups` times on a side stream: prime, then every body in order; back on the current stream
    and synchronised, per body: prime, capture.  Returns the graphs' replay callables, one per body.  Warm-up and capture write
    cache slots and row state, which the caller resets afterwards; slots >= pos are never read."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(warmups):
            prime()
            for body in bodies:
                body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    replays = []
    for body in bodies:
        prime()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, capture_error_mode="thread_local"):
            body()
        replays.append(g.replay)                                       # the bound method keeps its graph alive
    return replays


def encode_pockets(tf, example, batch_size):
    """The encoder's (outputs, padding mask) for the `batch_size` pockets of `example` (its optional `protein_knn`: a
    precomputed [2, E] kNN list; otherwise drawn on the GPU)."""
    enc_outputs, enc_pad_mask, _ = tf.encoder(example.protein_atom_feature.float(), example.protein_pos,
                                              example.protein_element_batch, example.protein_atom_laplacian, batch_size,
                                              getattr(example, "protein_knn", None))
    return enc_outputs, enc_pad_mask


def _select(cand_score, cand_flat, prefixes, hyps, done, num_beams, vocab_size, eos, pad, cur_len):
    """Host side of one step (BS:92-125) for all proteins: from the 2*num_beams ranked candidates of each protein pick the
    next live beams and store finished sequences.  Returns (scores, tokens, source rows), one entry per row.

    Rules kept exactly: '$' candidates are stored only when ranked inside the first num_beams, without the '$' and
    scored by the candidate's summed log-probability; `done` is re-evaluated after every candidate except the one that
    fills the beam (the reference's `break` comes first); a finished protein emits (0, '^', row 0)."""
    scores, tokens, rows = [], [], []
    for b in range(len(done)):
        if done[b]:
            scores += [0.0] * num_beams
            tokens += [pad] * num_beams
            rows += [0] * num_beams
            continue
        kept = 0
        best = float(cand_score[b].max())
        for rank in range(2 * num_beams):
            flat = int(cand_flat[b, rank])
            row, tok = b * num_beams + flat // vocab_size, flat % vocab_size
            if tok == eos:
                if rank >= num_beams:
                    continue
                hyps[b].add(prefixes[row].copy(), float(cand_score[b, rank]))
            else:
                scores.append(cand_score[b, rank])
                tokens.append(tok)
                rows.append(row)
                kept += 1
            if kept == num_beams:
                break
            done[b] = done[b] or hyps[b].is_done(best, cur_len)
        assert kept == num_beams, "fewer than num_beams live continuations among 2*num_beams candidates"
    return np.asarray(scores, dtype=np.float32), np.asarray(tokens, dtype=np.int64), np.asarray(rows, dtype=np.int64)


@torch.no_grad()
def beam_search(model, smiVoc, num_beams, batch_size, max_length, topk, example, prop=None, device="cuda", trace=None,
                graph=True, fused=True, tiles=False):
    """BS:38-175.  `model`: SINGA (uses model.model.encoder / decoder / projection); `example`: attribute bag with
    protein_element_batch, protein_atom_feature, protein_pos, protein_atom_laplacian (gen.py:176-181) and, optionally,
    protein_knn (a precomputed [2,E] kNN list; otherwise drawn on the GPU); `prop` [batch_size*num_beams, num_props].
    `graph=False` launches the step's kernels one by one instead of replaying the captured HIP graph (same numbers);
    `fused=False` evaluates the decoder layers with library GEMMs / elementwise ops instead of the k17 step kernels;
    `tiles=True` evaluates them with the row-tiled step kernels (`KVDecoder`), and `trace["path"]` says which path ran.
    Returns the decoded int64 token matrix [batch_size*topk, T] on `device`."""
    tf = model.model
    vocab_size = len(smiVoc)
    voc = list(smiVoc)
    sos, eos, pad = voc.index("&"), voc.index("$"), voc.index("^")
    dev = torch.device(device)
    num = 1 if tf.decoder.num_props else 0
    if tiles:
        from .Sampling import check_tiles
        check_tiles("beam_search", tf.decoder, max_length + num, fused)
    enc_outputs, enc_pad_mask = encode_pockets(tf, example, batch_size)
    rows = batch_size * num_beams
    kv = KVDecoder(tf.decoder, tf.projection, enc_outputs, enc_pad_mask, num_beams, max_length + num, vocab_size, fused, tiles=tiles)
    if graph:
        kv.capture()
    if num:
        kv.advance(kv.prop_input(prop.to(dev).float()))                # position 0 is the property prompt, CP:404-412

    beam_scores = np.zeros((batch_size, num_beams), dtype=np.float32)
    beam_scores[:, 1:] = -1e9                                          # all beams start equal: only beam 0 counts at step 1
    beam_scores = beam_scores.reshape(-1)
    prefixes = np.full((rows, 1), sos, dtype=np.int64)                 # input_ids live on the host: bookkeeping only
    tokens, src = prefixes[:, 0].copy(), np.arange(rows, dtype=np.int64)
    done = [False] * batch_size
    hyps = [BeamHypotheses(num_beams, max_length, length_penalty=0.7) for _ in range(batch_size)]
    cur_len = 1
    while cur_len < max_length:
        cand_score, cand_flat = kv.step(beam_scores, tokens, src)
        if trace is not None and "first_logp" not in trace:
            trace["first_logp"] = kv.logp.clone()
        beam_scores_next, tokens_next, src_next = _select(cand_score, cand_flat, prefixes, hyps, done, num_beams,
                                                          vocab_size, eos, pad, cur_len)
        if all(done):
            break
        beam_scores, tokens, src = beam_scores_next, tokens_next, src_next
        prefixes = np.concatenate([prefixes[src], tokens[:, None]], axis=1)
        cur_len += 1
    if trace is not None:
        trace["last_beams"], trace["hyps"] = prefixes.copy(), hyps
        trace["path"] = "tiles" if kv.tiles else "k17" if kv.fused else "library"

    final = beam_scores
    for b in range(batch_size):
        if not done[b]:                                                # BS:141-149
            for k in range(num_beams):
                r = b * num_beams + k
                hyps[b].add(prefixes[r], float(final[r]))
    best = []
    for h in hyps:
        ranked = sorted(h.beams, key=lambda x: x[0])
        best += [ranked.pop()[1] for _ in range(topk)]
    lens = [len(x) for x in best]
    if min(lens) == max(lens):                                         # BS:164-173
        decoded = np.stack(best)
    else:
        decoded = np.full((len(best), min(max(lens) + 1, max_length)), pad, dtype=np.int64)
        for i, x in enumerate(best):
            decoded[i, :lens[i]] = x
            if lens[i] < max_length:
                decoded[i, lens[i]] = eos
    return torch.from_numpy(decoded).to(dev)


BEAM_MAX_K = 1024       # slots per pocket singa_beam_select is built for


@torch.no_grad()
def beam_search_device(model, smiVoc, num_beams, batch_size, max_length, topk, example, prop=None, device="cuda", grammar=None,
                       suppress=(), length_penalty=0.7, graph=True, trace=None, forced=None, tiles=False):
    """`beam_search` with the selection on the device (include/singa_hip_beam.h states the rule: `_select` and `BeamHypotheses`
    as kernels, ties ranked by slot, then token), which can therefore be constrained: `grammar` None, "smiles" or "valence"
    and `suppress` as in `Sampling.sample`.  Under a grammar every stored hypothesis is a string the rule accepts, ended by its
    own '$'.  The scores are the unmodified model's: the mask removes candidates, it does not renormalise.

    `model`, `smiVoc`, `num_beams`, `batch_size`, `max_length`, `topk`, `example`, `prop` and `device` as in `beam_search`, and the
    same return value: the int64 token matrix [batch_size * topk, T'] on `device`, padded and '$'-terminated as BS:164-173
    does - except that under a grammar, where every hypothesis was ended by its own '$', the '$' is written back also when all
    returned rows are equally long (BS:164-166 returns such rows bare).  `length_penalty`: the exponent of
    `BeamHypotheses`.  `graph=False` launches the step's kernels one by one (same result).  The loop is `sample_distinct`'s:
    two cache buffers taken in turn, the step captured once per parity, one read of the pockets' live counters every
    `Sampling.LIVE_POLL` tokens and nothing else per token.  Only the fused step kernels serve this mode: k17, or with
    `tiles=True` the row-tiled ones, which take a pocket of any size (`trace["path"]` says "k17" or "tiles").  The end of the search
    stays on the host: a pocket that is not done adds its live beams as hypotheses (BS:141-149), the `topk` best are returned.

    `forced`: int64 [batch_size, max_length], ONE prefix per pocket (`smiles.encode` builds it, `smiles.check_prefix` validates
    it before any device work): every hypothesis of the pocket starts with it.  `ops.beam_expand`, given the matrix, runs
    `singa_forced_beam_expand` (include/singa_hip_prefix.h states the rule): through the prefix a pocket keeps one live slot,
    and the sums include the prefix.  The host-selected `beam_search` has no such argument.

    `trace`, if a dict, receives `hyps` (one `BeamHypotheses` per pocket, as `beam_search` leaves them), `hyp_sum_logp` and
    `hyp_tokens` (per pocket, one entry per stored hypothesis in the order of `hyps[b].beams`: the f32 summed log-probability,
    '$' included where the search ended the string, and the tokens without '$'), `steps` and `valid` (uint8 per returned row: 0
    where the pocket stored fewer than `topk` hypotheses - such rows are all '^').  ValueError before any launch unless
    1 <= topk <= num_beams <= 1024, for what `smiles.check_arguments` refuses, for a decoder geometry, length or pocket size
    the k17 kernels are not built for, and for caches (two buffers) that do not fit the free memory."""
    from . import Sampling as S
    from .. import smiles
    if not 1 <= topk <= num_beams <= BEAM_MAX_K:
        raise ValueError(f"beam_search_device: 1 <= topk <= num_beams <= {BEAM_MAX_K} (got topk {topk}, num_beams {num_beams})")
    dev, tf, voc, (sos, eos, pad), rows, num, positions, free, cls, allowed = S._prologue(
        "beam_search_device", model, smiVoc, num_beams, batch_size, max_length, example, device, grammar, suppress)
    k, V, T = num_beams, len(voc), max_length
    a0, f0 = tf.decoder.layers[0].dec_self_attn, tf.decoder.layers[0].pos_ffn
    atoms = int(torch.bincount(example.protein_element_batch.cpu().long()).max())
    if not (a0.hidden_channels == 256 and a0.key_channels == 128 and a0.num_heads == 4 and f0.conv1.out_channels == 1024
            and positions <= 256 and (tiles or atoms <= 1024) and V <= 1024):
        raise ValueError("beam_search_device: the k17 step kernels are the only path: the shipped decoder geometry, at most 256 "
                         "positions, 1024 pocket atoms and 1024 tokens")
    need = 2 * S.cache_bytes(tf.decoder, rows, positions) + rows * V * 4 + 3 * rows * T * 8
    if need + (64 << 10) * rows > free:                  # + the step's activations, as in `sample`
        raise ValueError(f"beam_search_device: the two key / value cache buffers of {rows} rows x {positions} positions and the "
                         f"candidates take {need} bytes, {free} bytes are free on {dev}: use fewer beams or pockets per call")

    if forced is not None:
        forced = forced.cpu().numpy() if torch.is_tensor(forced) else forced
        forced = torch.as_tensor(smiles.check_prefix(forced, smiVoc, batch_size, max_length, grammar)).to(dev).contiguous()

    kv = KVDecoder(tf.decoder, tf.projection, *encode_pockets(tf, example, batch_size), k, positions, V, True, search_buffers=False,
                   tiles=tiles)
    bufs = ((kv.k, kv.v), (torch.zeros_like(kv.k), torch.zeros_like(kv.v)))
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)
    state = {"score": new(rows, torch.float32), "length": new(rows, torch.int32), "tokens": new((rows, T), torch.int64),
             "next": new(rows, torch.int64), "src": new(rows, torch.int64), "cand": new((rows, V), torch.float32),
             "hyp_score": new(rows, torch.float64), "hyp_sum": new(rows, torch.float32), "hyp_len": new(rows, torch.int32),
             "hyp_stamp": new(rows, torch.int32), "hyp_tokens": new((rows, T), torch.int64), "n_hyp": new(batch_size, torch.int32),
             "worst": new(batch_size, torch.float64), "done": new(batch_size, torch.uint8), "live": new(batch_size, torch.int32)}
    never = torch.zeros(rows, dtype=torch.uint8, device=dev)           # `finished` of the cache mover: a beam slot is live or dead
    if grammar is not None:
        cls = torch.as_tensor(cls).to(dev)
        state["grammar"] = new(rows, torch.int32)
    cap, vstate = S._valence_operands(grammar, smiVoc, rows, dev)
    if vstate is not None:
        state["vstate"] = vstate
    # n ** length_penalty by Python's own `**`, as BeamHypotheses.add evaluates it (entry 0 is never read)
    len_pow = torch.tensor([1.0] + [float(n ** length_penalty) for n in range(1, T)], dtype=torch.float64).to(dev)
    work = ops.beam_work(rows, T, dev)

    def start():
        state["tokens"].fill_(pad)
        state["tokens"][:, 0] = sos
        state["next"].fill_(sos)
        state["score"].fill_(float("-inf"))
        state["score"].view(batch_size, k)[:, 0] = 0                   # slot 0 of every pocket is the root
        state["length"].zero_(), state["src"].zero_(), state["cand"].fill_(float("-inf"))
        state["hyp_score"].zero_(), state["hyp_sum"].zero_(), state["hyp_len"].zero_(), state["hyp_stamp"].zero_()
        state["hyp_tokens"].fill_(pad)
        state["n_hyp"].zero_(), state["worst"].fill_(1e9), state["done"].zero_(), state["live"].fill_(1)
        if grammar is not None:
            state["grammar"].fill_(smiles.FRESH)
        kv.reset()

    def step(parity):
        (ck, cv), (ok, ov) = bufs[parity], bufs[1 - parity]
        out = kv.advance(kv.token_input(state["next"]), ck, cv)
        ops.beam_expand(tf.projection(out).contiguous(), kv.pos, num + 1, state, k, allowed, cls, cap, forced=forced)
        ops.beam_select(kv.pos, num + 1, state, k, work, len_pow, eos, pad, cls, cap)
        ops.swor_follow(ck, cv, ok, ov, state["src"], state["score"], never, kv.pos)

    def prime():
        start()
        kv.pos += num

    replays = [lambda: step(0), lambda: step(1)]                       # the step on each pair of cache buffers, taken in turn
    if graph:
        replays = capture_steps(prime, replays, 1)
    start()
    if num:
        kv.advance(kv.prop_input(prop.to(dev).float()))                # position 0 is the property prompt, in the first buffer
    steps = S._decode(replays, T - 1, lambda: int(state["live"].sum().item()))

    # the end of the search on the host: a few hundred numbers, once
    host = {n: state[n].cpu().numpy() for n in ("score", "length", "tokens", "hyp_score", "hyp_sum", "hyp_len", "hyp_stamp",
                                                "hyp_tokens", "n_hyp", "worst", "done")}
    per = lambda name: host[name].reshape(batch_size, k, *host[name].shape[1:])
    hyps, sums = [], {}
    for b in range(batch_size):
        h = BeamHypotheses(k, T, length_penalty)
        n = int(host["n_hyp"][b])
        for i in np.argsort(per("hyp_stamp")[b, :n], kind="stable"):   # ascending stamps: the order `add` would have left
            hyp = per("hyp_tokens")[b, i, :per("hyp_len")[b, i]].copy()
            h.beams.append((float(per("hyp_score")[b, i]), hyp))
            sums[id(hyp)] = per("hyp_sum")[b, i]
        h.worst_score = float(host["worst"][b])
        if not host["done"][b]:                                        # BS:141-149
            for j in range(k):
                if per("score")[b, j] > float("-inf"):
                    hyp = per("tokens")[b, j, :per("length")[b, j] + 1].copy()
                    sums[id(hyp)] = per("score")[b, j]
                    h.add(hyp, float(per("score")[b, j]))
        hyps.append(h)
    best = []
    for h in hyps:
        ranked = sorted(h.beams, key=lambda x: x[0])
        best += [ranked.pop()[1] if ranked else None for _ in range(topk)]
    valid = np.array([x is not None for x in best], dtype=np.uint8)
    lens = [len(x) for x in best if x is not None]
    if grammar is None and valid.all() and min(lens) == max(lens):     # BS:164-173; under a grammar every row gets its '$' back
        decoded = np.stack(best)
    else:
        decoded = np.full((len(best), min(max(lens, default=0) + 1, T)), pad, dtype=np.int64)
        for i, x in enumerate(best):
            if x is not None:
                decoded[i, :len(x)] = x
                if len(x) < T:
                    decoded[i, len(x)] = eos
    if trace is not None:
        trace.update(hyps=hyps, hyp_sum_logp=[[sums[id(x)] for _, x in h.beams] for h in hyps],
                     hyp_tokens=[[x for _, x in h.beams] for h in hyps], steps=steps, valid=torch.from_numpy(valid),
                     path="tiles" if kv.tiles else "k17")
    return torch.from_numpy(decoded).to(dev)
