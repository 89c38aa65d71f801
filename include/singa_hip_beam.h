/* Beam search selected on the device, optionally constrained by the SMILES or the valence rule: the reference's selection rule
 * (model/BeamSearch.py = "BS" of the reference, kept by `_select` and `BeamHypotheses` of singa_amd/model/BeamSearch.py) as
 * kernels.  NOT part of the drop-in training ABI (include/singa_hip.h) and none of the other generation-time headers: these
 * entry points exist for `beam_search_device` of singa_amd/model/BeamSearch.py.  Conventions as in singa_hip.h (device
 * pointers, `stream`, SINGA_E_* return codes).
 *
 * THE RULE.  Rows are pocket-major, k = num_beams slots per pocket (rows = pockets * k).  Per slot the device holds
 *   score    f32   the summed log-probability of the slot's prefix under the unmodified model; -inf marks a DEAD slot
 *   length   i32   tokens chosen so far ('&' not counted)
 *   tokens[T] i64, next i64 (the token the decoder reads next), src i64 (the row whose caches the slot continues)
 *   gstate   i32   with a grammar: the packed state of singa_hip_gen.h;  vstate[2] i32: the two words of singa_hip_valence.h
 * and per pocket up to k stored hypotheses, slot h of them being
 *   hyp_score f64 (sum / len ** length_penalty), hyp_sum f32, hyp_len i32 (tokens, '&' included, '$' not), hyp_tokens[T] i64,
 *   hyp_stamp i32 (t * 2k + rank of the candidate that stored it: ascending stamps are the order of BeamHypotheses.beams)
 * with n_hyp i32, worst f64 (1e9 at the start), done u8 and live i32.  A run starts with slot 0 of every pocket at score 0 and
 * every other slot dead (the host path's -1e9 exists only to make them lose), prefix '&', length 0, gstate FRESH, n_hyp = 0,
 * done = 0, live = 1, hyp_tokens all `pad`.  The step index is t = *pos - pos_offset, read on the device, so that a captured
 * launch replays; a step outside 0 <= t < T - 1 writes nothing.  Step t is singa_beam_expand, then singa_beam_select.
 *
 * 1. Expand (per live slot r of a pocket that is not done).  cand[r][v] = score[r] + (z_v - lse) in f32 with
 *    lse = zmax + logf(sum expf(z - zmax)) over all V tokens: the expressions of singa_sample_token, so that the sum carries
 *    the bits `score(...)` reports for the string.  cand = -inf where allowed[v] == 0 or where the rule in force - with cls:
 *    smiles_allows(gstate, cls[v], rem), with cap as well: valence_allows((gstate, vstate), cls[v], cap[v], rem),
 *    rem = T - 2 - t - refuses v.  The mask removes candidates; it does not renormalise.  A dead slot's candidates are all
 *    -inf; a done pocket's are not written.
 * 2. Select (per pocket that is not done).  The 2k largest finite candidates of the pocket's k V are ranked in descending
 *    order; ties go to the lower slot, then to the lower token (torch.topk leaves ties open: a refinement of the host rule).
 *    There may be fewer than 2k.  They are walked in rank order:
 *      - an `eos` candidate of rank < k is stored as a hypothesis: the parent's prefix (t + 1 tokens, without '$'), sum = cand,
 *        score = (double)sum / len_pow[t + 1], where len_pow[n] = n ** length_penalty is a table the host fills;
 *      - an `eos` candidate of rank >= k is skipped, and so is the re-evaluation of `done` behind it;
 *      - any other candidate becomes the next new slot, until k are kept: the candidate that fills the beam ends the walk;
 *      - behind every other candidate, done |= n_hyp >= k and worst >= best / len_pow[t + 1], best = the rank-0 candidate.
 *    Storing is BeamHypotheses.add: refused when n_hyp >= k and score <= worst; below k the hypothesis is appended and
 *    worst = min(worst, score); at k the stored hypothesis of the lowest score (the lowest stamp among equals) is replaced and
 *    worst = the lowest score then stored.  A hypothesis slot replaced twice in one step belongs to its last owner.
 *    Fewer than k kept leaves the trailing slots dead (the host path asserts here; it happens only under a mask).
 *    live[pocket] = the slots kept, or 0 once done is set.  The step that sets done is still committed; from the next step on
 *    nothing of a done pocket is written - slots, hypotheses, next, src, live and cand stay as they are.
 * 3. Commit.  New slot j from (parent i, token v): score = cand[i][v], length_i + 1, columns 0 .. t of tokens are the parent's,
 *    column t + 1 = v, next = v, src = the parent's row, gstate and both vstate words are the state after v.  A dead slot:
 *    score = -inf, next = pad, src = its own row; its tokens, length and state words are kept.
 *
 * WHAT THE RULE GUARANTEES.  With cls (and cap) the budget term of the rule leaves a live slot nothing but '$' at the last
 * step t = T - 2.  Every stored hypothesis therefore was ended by its own '$'; no live slot is left behind the last step for
 * the host to add unfinished; and every pocket stores at least one hypothesis (the rank-0 candidate is always kept or stored,
 * and a kept slot can always be continued).  With cap no atom of a hypothesis exceeds its token's capacity.
 *
 * Limits: 1 <= k <= 1024, 1 <= V <= 1024, T >= 2 (3 with cls), rows a multiple of k; anything else is SINGA_E_SHAPE.  cls and
 * gstate go together, cap and vstate go together and need cls (SINGA_E_NULL otherwise).  Nothing is allocated: `work` is
 * caller-provided scratch of singa_beam_work(rows, T) bytes, 16-byte aligned, which holds the new slots until every parent is
 * read.  One workgroup serves one pocket in select (radix select and sort of sample_distinct's selection, then a serial walk
 * of at most 2k decisions by one thread, then the token rows of the stored hypotheses copied by all); the parents' columns
 * are gathered and the slots committed by two row-parallel launches behind it.  The caches follow through singa_swor_follow
 * with `score` in the place of `gumbel`. */
#ifndef SINGA_HIP_BEAM_H
#define SINGA_HIP_BEAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* bytes of scratch singa_beam_select needs; -1 for rows < 0 or T < 2 */
long long singa_beam_work(int rows, int T);

/* sub-step 1: cand [rows][V] from logits [rows][V]; allowed, cls, cap [V] (each may be null), done [pockets] */
int singa_beam_expand(const float* logits, const unsigned char* allowed, const unsigned char* cls, const unsigned char* cap,
                      const long long* pos, int pos_offset, int rows, int k, int V, int T, const float* score,
                      const int32_t* gstate, const int32_t* vstate, const unsigned char* done, float* cand, void* stream);

/* sub-steps 2 and 3; len_pow holds T doubles; the hyp_* arrays are [rows] / [rows][T], n_hyp, worst, done, live [pockets] */
int singa_beam_select(const float* cand, const unsigned char* cls, const unsigned char* cap, const long long* pos, int pos_offset,
                      int rows, int k, int V, int T, int eos, int pad, const double* len_pow, float* score, int32_t* length,
                      long long* tokens, long long* next, long long* src, int32_t* gstate, int32_t* vstate, double* hyp_score,
                      float* hyp_sum, int32_t* hyp_len, int32_t* hyp_stamp, long long* hyp_tokens, int32_t* n_hyp, double* worst,
                      unsigned char* done, int32_t* live, void* work, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_BEAM_H */
