/* Generation-time extensions of libsinga_hip.so.  NOT part of the drop-in training ABI (include/singa_hip.h): these entry
 * points exist for singa_amd/model/Sampling.py and have no call site in the reference.  Conventions as in singa_hip.h.
 *
 * Grammar-constrained token choice: singa_sample_token with a per-row mask that depends on what the row has drawn so far,
 * so that every sampled row ends in `eos` before its columns run out and the text in front of it is a syntactically
 * complete SMILES string.  THE RULE (kernel, singa_amd/smiles.py and tests/grammar_rule.py restate this text):
 *
 * Token classes.  cls[V] bytes, derived by the caller from the vocabulary's strings: low nibble = class, high nibble =
 * ring digit index 0..8 (token '1' .. '9'; 0 for every other class).
 *   0 NONE   never drawn: '&', '^', anything unrecognised ('%', ...)
 *   1 ATOM   B C N O P S F I Br Cl b c n o p s, and any [...]
 *   2 BOND   - = # / \ :
 *   3 OPEN   (
 *   4 CLOSE  )
 *   5 RING   1 .. 9
 *   6 DOT    .
 *   7 EOS    $
 *
 * Row state.  One int32 per row, gstate[rows]:
 *   bits 0-3    prev    class of the last token: 1 ATOM, 2 BOND (a bond symbol right after an atom or a ring digit), 3 OPEN,
 *                       4 CLOSE, 5 RING, 6 DOT, 7 START (fresh row), 8 BONDX (a bond symbol right after '(' or ')')
 *   bits 4-9    depth   open branches, at most 63
 *   bits 10-18  ring    digits currently open (bit d = digit index d)
 *   bits 19-27  here    digits opened on the current atom
 * A fresh row is prev = START, everything else 0 (the value 7).
 *
 * Which token may follow.  With A = prev in {ATOM, RING, CLOSE}:
 *   ATOM                 always
 *   BOND                 A or prev = OPEN
 *   OPEN                 A and depth < 63
 *   CLOSE                A and depth > 0
 *   DOT                  A
 *   RING d, d open       prev in {ATOM, RING} and d not in here              (this closes d)
 *   RING d, d not open   prev in {ATOM, RING, BOND}                          (this opens d)
 *   EOS                  A, depth = 0 and ring = 0
 *   NONE                 never
 *
 * Transition (fields not named stay):
 *   ATOM    prev = ATOM, here = 0
 *   BOND    prev = BOND if the old prev in {ATOM, RING}, else BONDX
 *   OPEN    prev = OPEN, depth + 1
 *   CLOSE   prev = CLOSE, depth - 1
 *   RING d  prev = RING, bit d of ring toggles; an opening digit also sets bit d of here
 *   DOT     prev = DOT
 *   EOS     nothing (the row is finished)
 *
 * Budget.  Step t writes column t + 1 of T; rem = T - 2 - t columns are left after it.  A non-EOS token is allowed only if
 * rem >= need(state'), state' the state after the token, where
 *   need = a + popcount(ring) + depth + 1,
 *   a = 1 if prev in {START, DOT, BOND, BONDX, OPEN}, or if ring != 0 and (prev = CLOSE or ring & here != 0); else a = 0.
 * need counts the shortest completion: [one atom], the closing digits, ')' x depth, '$'.  That completion is allowed from any
 * state with rem >= need and keeps rem >= need, so every row has drawn `eos` by column T - 1 (T >= 3).
 *
 * Out of scope of THIS rule: chemical validity (aromaticity, duplicate ring bonds such as C1C1 or C12CC12; valence is what the
 * rule of singa_hip_valence.h adds to this one), %nn closures, a bond symbol in front of a CLOSING ring digit (never drawn).
 * (Beam search takes this rule through singa_hip_beam.h.)
 *
 * singa_sample_token_grammar: singa_sample_token (same arguments, same state arrays, same rule 1-5) on the effective mask
 * allowed[i] (null: all) AND the grammar evaluated on gstate[row], cls[i] and rem.  The log-probability stays log-softmax of
 * the unmodified logits.  gstate[row] becomes the state after the drawn token.  A finished row emits `pad` and keeps its state;
 * a row whose effective mask is empty (an unreachable state, or a contradictory `allowed`) emits `pad` as singa_sample_token
 * does, stays unfinished unless pad == eos, and keeps its state.
 *   allowed_logp[rows][T] (optional, may be null): column t + 1 receives log of the model's own probability mass (tau = 1,
 *   nothing filtered) on the tokens of the effective mask: tok_logp - allowed_logp is the log-probability of the token under
 *   the model restricted to what the grammar allows.  0 for finished rows, -inf for an empty mask.
 * Errors: those of singa_sample_token; SINGA_E_NULL also for null cls / gstate; SINGA_E_SHAPE also for T < 3. */
#ifndef SINGA_HIP_GEN_H
#define SINGA_HIP_GEN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_sample_token_grammar(const float* logits, const float* uniforms, const unsigned char* allowed,
                               const unsigned char* cls, const long long* pos, int pos_offset, int rows, int V,
                               int T, float tau, int top_k, float top_p, int eos, int pad,
                               unsigned char* finished, int32_t* length, float* sum_logp, long long* tokens,
                               long long* next, int32_t* live, float* tok_logp, int32_t* gstate,
                               float* allowed_logp, void* stream);

/* The same rule on the HOST (all pointers are host pointers, nothing is enqueued): for i < n, ok[i] = 1 if the token of class
 * byte cls[i] may follow state[i] with rem[i] columns left, else 0; next_state[i] = the state after that token if it may,
 * state[i] otherwise.  Part of every build of the library: the kernel and this function share one source. */
int singa_smiles_rule_host(const unsigned char* cls, const int32_t* state, const int32_t* rem, int n, unsigned char* ok,
                           int32_t* next_state);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_GEN_H */
