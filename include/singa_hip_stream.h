/* Continuous sampling: the number of ROWS is a fixed budget, the number of MOLECULES is not - a row that has ended its
 * molecule starts the pocket's next one in the following step.  NOT part of the drop-in training ABI (include/singa_hip.h) and
 * none of the other generation-time headers: these entry points exist for `sample_stream` of singa_amd/model/Sampling.py.
 * Conventions as in singa_hip.h (device pointers, `stream`, SINGA_E_* return codes).
 *
 * THE RULE.  Rows are pocket-major, R per pocket (rows = pockets * R); molecules are pocket-major, num_samples per pocket
 * (molecules = pockets * num_samples).  Per row the device holds
 *   pos    i64  the row's own next key / value cache position
 *   mol    i32  the molecule the row decodes, -1 for a RETIRED row
 *   next   i64  the token the next step embeds
 *   gstate i32  (grammar on) the rule state of singa_sample_token_grammar
 * per pocket
 *   issued i32  molecule indices of the pocket handed out so far
 *   live   i32  rows of the pocket that are not retired
 * and per molecule what singa_sample_token keeps per row - tokens[T] i64, tok_logp[T] f32, allowed_logp[T] f32 (grammar on),
 * sum_logp f32, length i32 - and row_of i32 (the row that decoded it), start_step i32 (the step of the run, counted from 0,
 * in which its first token was chosen).
 *
 * Start of a run (the caller's): rows b*R + i with i < min(R, num_samples) hold molecule b*num_samples + i at pos =
 * pos_offset with next = sos and gstate FRESH, row_of / start_step of those molecules are the row / 0, every other row of
 * the pocket is retired (its pos any valid cache position), issued[b] = live[b] = min(R, num_samples); the per-molecule
 * outputs are prefilled: tokens sos in column 0 and pad behind it, tok_logp / allowed_logp / sum_logp / length 0.
 *
 * A step is the decoder on every row at ITS position (singa_dec_self_attn_rows appends the row's keys / values at pos[row]
 * and attends over positions 0 .. pos[row]; positions behind it, left by an earlier molecule, are never read), then
 *
 * 1. Choice (singa_sample_token_stream; per row with mol[row] = j >= 0).  t = pos[row] - pos_offset; a row with t outside
 *    0 <= t < T - 1 or j >= molecules writes nothing.  The token is chosen exactly as singa_sample_token - with cls and gstate,
 *    singa_sample_token_grammar - chooses it, by the same expressions in the same order, from the row's logits and
 *    u = uniforms[t][j] (uniforms is [>= T - 1][molecules]: a column belongs to a molecule, not to a row).  The bookkeeping
 *    goes to molecule j: tokens[j][t + 1], tok_logp[j][t + 1], allowed_logp[j][t + 1], sum_logp[j] +=, length[j] += 1;
 *    next[row] and gstate[row] are the row's.  Retired rows return at once.
 * 2. Hand-over (singa_stream_refill; per pocket, after all choices).  A row with mol >= 0 is DONE if next[row] == eos or
 *    pos[row] - pos_offset >= T - 2.  The done rows of a pocket, in ascending row order, take molecule indices issued[b],
 *    issued[b] + 1, ... while those are < num_samples.  A row that receives index i holds molecule j' = b*num_samples + i from
 *    then on: start_step[j'] = start_step[j] + (pos[row] - pos_offset) + 1 with j the molecule it has ended (a molecule's
 *    steps follow each other without a gap, so this is the run's step count), row_of[j'] = row, pos[row] = pos_offset,
 *    next[row] = sos, gstate[row] = fresh.  A done row that receives nothing is retired: mol[row] = -1, and only that.  A row
 *    that is not done advances pos[row] by one.  issued[b] and live[b] are stored where they change.  A retired row is not
 *    touched, so its pos keeps naming the cache position it had: positions move HERE and not in an elementwise operation over
 *    all rows, which would walk a retired row out of its cache.  A pocket without a live row writes nothing at all.
 *
 * Columns of a molecule behind its end keep the prefill (pad / 0), as singa_sample_token leaves them.
 *
 * Limits: 1 <= R <= 2048, 1 <= V <= 1024, T >= 2 (3 with the grammar), num_samples >= 1, molecules >= 1, eos / pad / sos inside
 * the vocabulary; anything else is SINGA_E_SHAPE, a missing pointer SINGA_E_NULL (cls and gstate go together, allowed_logp only
 * with them; allowed, tok_logp and, in refill, gstate are optional).  One workgroup serves one pocket in the hand-over: the
 * order within a pocket is an LDS scan over wave-level prefix counts of the done rows; pockets share nothing, and no atomic
 * operation is used. */
#ifndef SINGA_HIP_STREAM_H
#define SINGA_HIP_STREAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* singa_dec_self_attn of singa_hip.h with one position per row: pos is [R] and row r appends at and attends up to pos[r].
 * A row whose pos[r] lies outside [0, P) is left alone (neither its caches nor its row of y are written). */
int singa_dec_self_attn_rows(const float* x, const float* wqkv_t, const float* bqkv, const float* wo_t, const float* bo,
                             const float* gamma, const float* beta, float* k_cache, float* v_cache, const long long* pos, int R,
                             int P, float* y, float eps, void* stream);

/* Step 1.  logits [rows][V]; uniforms [>= T - 1][molecules]; pos [rows]; mol [rows]; tokens / tok_logp / allowed_logp
 * [molecules][T]; length / sum_logp [molecules]; next / gstate [rows]. */
int singa_sample_token_stream(const float* logits, const float* uniforms, const unsigned char* allowed,
                              const unsigned char* cls, const long long* pos, const int32_t* mol, int pos_offset, int rows,
                              int molecules, int V, int T, float tau, int top_k, float top_p, int eos, int pad,
                              int32_t* length, float* sum_logp, long long* tokens, long long* next, float* tok_logp,
                              int32_t* gstate, float* allowed_logp, void* stream);

/* Step 2.  pos / mol / next / gstate [pockets * R]; issued / live [pockets]; row_of / start_step [pockets * num_samples]. */
int singa_stream_refill(int pockets, int R, int num_samples, int T, int pos_offset, int sos, int eos, int fresh, long long* pos,
                        int32_t* mol, long long* next, int32_t* gstate, int32_t* issued, int32_t* live, int32_t* row_of,
                        int32_t* start_step, void* stream);

/* Step 2 on the CPU, host pointers (one source with the kernel: the rule can be checked without a GPU). */
int singa_stream_refill_host(int pockets, int R, int num_samples, int T, int pos_offset, int sos, int eos, int fresh,
                             long long* pos, int32_t* mol, long long* next, int32_t* gstate, int32_t* issued, int32_t* live,
                             int32_t* row_of, int32_t* start_step);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_STREAM_H */
