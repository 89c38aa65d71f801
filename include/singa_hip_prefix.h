/* Forced tokens in the modes that followed the lockstep sampler: continuous sampling (`sample_stream`), sampling without
 * replacement (`sample_distinct`) and beam search selected on the device (`beam_search_device`).  NOT part of the drop-in
 * training ABI (include/singa_hip.h) and none of the other generation-time headers: these entry points exist for the `forced=`
 * argument of those three functions and for `score(..., rows_per_pocket=...)` of singa_amd/model/Sampling.py.  Conventions as
 * in singa_hip.h.
 *
 * THE RULE.  Each entry point is its unforced sibling - same arguments, same state arrays, same kernels in the same order -
 * with one more input: a token that is GIVEN instead of chosen.  A forced column's effective mask is the single given token;
 * `allowed` and the grammar take no part; everything behind the choice is the code a chosen token runs.  A value f of `forced`
 * outside [0, V) leaves the column FREE: every output then receives the very bits the sibling writes.  `forced` is read once
 * per row and step (8 bytes, wave-uniform) and never written.  Validating what is forced is the host's job
 * (singa_amd.smiles.check_forced / check_prefix walk it through the rule's host twins before anything is launched).
 *
 * singa_sample_token_stream_forced = singa_sample_token_stream (include/singa_hip_stream.h; with cap and vstate, both null or
 * both given and only with cls / gstate: the valence form of include/singa_hip_valence.h) + the forced token of
 * singa_sample_token_forced (include/singa_hip_force.h).  forced[molecules][T] (required, int64) and rank[molecules][T]
 * (optional, int32) are indexed by MOLECULE, as every other per-molecule output is: the row that decodes molecule j reads
 * forced[j][t + 1] at its own step t and writes rank[j][t + 1].  Everything include/singa_hip_force.h says about a forced
 * token's bookkeeping (tok_logp, sum_logp, length, the grammar state after f whether or not the rule allows f, allowed_logp,
 * rank) holds per molecule; next[row] = f, so a forced '$' ends the molecule in the hand-over that follows.
 *
 * singa_swor_expand_forced = singa_swor_expand (include/singa_hip_swor.h) + forced[pockets][T] (required, int64): ONE prefix
 * per pocket.  A live, unfinished row of pocket p = row / k reads f = forced[p][t + 1].  With f inside [0, V):
 *     cand[row][f] = gumbel[row]      cand_phi[row][f] = prop_logp[row]      cand_logp[row][f] = z_f - lse
 * and every other token of the row is -inf in all three.  This is what the unforced expansion gives under a one-hot mask: the
 * proposal's log-probability of the only token is logf(1) = 0, so the child's phi is the parent's; its perturbed score is the
 * row's maximum, whose conditioning term log1p(-exp(0)) vanishes, so the child's G is the parent's.  No noise is drawn.  lse is
 * the unmodified model's, as everywhere (z_f - lse carries the bits `score` reports).  Dead and finished rows behave as in
 * singa_swor_expand whatever `forced` holds.  singa_swor_select is used unchanged behind it: it advances the prefix hash with
 * the child hash and the grammar state with the transition for f, as it does for a chosen token.  Through a prefix that
 * starts at column 1 a pocket therefore keeps one live slot with G = phi = 0, and prop_logp at the end of a run is the
 * log-probability under the proposal CONDITIONAL on the prefix, while sum_logp and tok_logp include the prefix.
 *
 * singa_forced_beam_expand = singa_beam_expand (include/singa_hip_beam.h) + forced[pockets][T] (required, int64).  A live row
 * of a pocket that is not done reads f = forced[row / k][t + 1]; with f inside [0, V) cand[row][f] = score[row] + (z_f - lse)
 * and every other candidate of the row is -inf.  Done pockets and dead rows behave as in singa_beam_expand.
 * singa_beam_select is used unchanged behind it.  (The name does not begin like its sibling's: the singa_beam_* names are
 * those of include/singa_hip_beam.h alone, which tests/test_beam_device_cpu.py holds every other header to.)
 *
 * Errors: the sibling's, checked before any HIP call, and SINGA_E_NULL also for a null `forced`.  rows = 0 succeeds.  The
 * SINGA_EMUL build answers as for the siblings. */
#ifndef SINGA_HIP_PREFIX_H
#define SINGA_HIP_PREFIX_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_sample_token_stream_forced(const float* logits, const float* uniforms, const unsigned char* allowed,
                                     const unsigned char* cls, const unsigned char* cap, const long long* pos, const int32_t* mol,
                                     int pos_offset, int rows, int molecules, int V, int T, float tau, int top_k, float top_p,
                                     int eos, int pad, int32_t* length, float* sum_logp, long long* tokens, long long* next,
                                     float* tok_logp, int32_t* gstate, int32_t* vstate, float* allowed_logp,
                                     const long long* forced, int32_t* rank, void* stream);

int singa_swor_expand_forced(const float* logits, const unsigned char* allowed, const unsigned char* cls, const long long* pos,
                             int pos_offset, int rows, int k, int V, int T, float tau, unsigned long long seed,
                             const uint32_t* streams, int pad, const float* gumbel, const float* prop_logp,
                             const unsigned long long* hash, const unsigned char* finished, const int32_t* gstate, float* cand,
                             float* cand_logp, float* cand_phi, const long long* forced, void* stream);

int singa_forced_beam_expand(const float* logits, const unsigned char* allowed, const unsigned char* cls, const unsigned char* cap,
                             const long long* pos, int pos_offset, int rows, int k, int V, int T, const float* score,
                             const int32_t* gstate, const int32_t* vstate, const unsigned char* done, float* cand,
                             const long long* forced, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_PREFIX_H */
