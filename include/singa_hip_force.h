/* Forced tokens in sampled generation.  NOT part of the drop-in training ABI (include/singa_hip.h) and not one of the
 * generation-time extensions of include/singa_hip_gen.h either: this entry point exists for `sample(..., forced=...)` and
 * `score` of singa_amd/model/Sampling.py.  Conventions as in singa_hip.h.
 *
 * THE RULE.  singa_sample_token_forced is singa_sample_token / singa_sample_token_grammar (same arguments, same state arrays,
 * same kernels in the same order) with one more input per row and column: a token that is GIVEN instead of drawn.
 *
 * Grammar switch.  cls, gstate and allowed_logp all null: no grammar, the step is singa_sample_token's.  cls and gstate both
 * non-null: the step is singa_sample_token_grammar's (allowed_logp stays optional).  Anything else - exactly one of cls and
 * gstate, or allowed_logp without them - is SINGA_E_NULL.
 *
 * forced[rows][T] (required, int64).  At step t an unfinished row reads f = forced[row][t + 1], once (wave-uniform).
 *   f outside [0, V)   the column is FREE: the token is chosen exactly as the unforced entry point chooses it, from the same
 *                      inputs, and every state array receives the very same bits.
 *   f inside [0, V)    the token is f.  uniforms, tau, top_k, top_p, allowed and the grammar's mask take no part in the choice.
 * The bookkeeping is that of a drawn token: tokens[row][t + 1] = next[row] = f, length += 1, tok_logp[row][t + 1] = the
 * log-softmax of the unmodified logits at f, sum_logp += the same; finished = 1 and live -= 1 if f == eos.  Under the grammar
 * gstate[row] becomes the state after f - the transition of singa_hip_gen.h for f's class - WHETHER OR NOT THE RULE WOULD HAVE
 * ALLOWED f: validating a forced prefix is the host's job (singa_amd.smiles.check_forced walks it through
 * singa_smiles_rule_host before anything is launched).  allowed_logp[row][t + 1] still receives the log of the model's mass
 * on the effective mask (`allowed` AND the rule) of that step, so tok_logp - allowed_logp is the log-probability under the
 * constrained proposal ONLY for a forced token that lies inside the mask; for one outside it the difference means nothing.
 * A finished row emits `pad` whatever forced holds.  forced itself is never written.
 *
 * rank[rows][T] (optional, may be null, int32).  Column t + 1 receives the number of tokens j with z_j > z_tok, or
 * z_j == z_tok and j < tok: the rank of the emitted token among all V raw logits (no mask, no temperature), for drawn and
 * forced tokens alike; 0 is the arg-max.  Finished rows write 0; a free row whose effective mask is empty (it emits `pad` as
 * singa_sample_token does) writes -1.
 *
 * Errors: those of singa_sample_token_grammar, with SINGA_E_NULL also for null forced and for the grammar switch above, and
 * T >= 3 demanded only when the grammar is on (T >= 2 without it). */
#ifndef SINGA_HIP_FORCE_H
#define SINGA_HIP_FORCE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_sample_token_forced(const float* logits, const float* uniforms, const unsigned char* allowed,
                              const unsigned char* cls, const long long* pos, int pos_offset, int rows, int V,
                              int T, float tau, int top_k, float top_p, int eos, int pad,
                              unsigned char* finished, int32_t* length, float* sum_logp, long long* tokens,
                              long long* next, int32_t* live, float* tok_logp, int32_t* gstate,
                              float* allowed_logp, const long long* forced, int32_t* rank, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_FORCE_H */
