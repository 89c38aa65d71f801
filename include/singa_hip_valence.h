/* Valence-aware token choice.  NOT part of the drop-in training ABI (include/singa_hip.h) and none of the other
 * generation-time headers: these entry points exist for `grammar="valence"` of singa_amd/model/Sampling.py.  Conventions as in
 * singa_hip.h (device pointers, `stream`, SINGA_E_* return codes).
 *
 * THE RULE (kernel, singa_amd/smiles.py and tests/valence_rule.py restate this text).  The SMILES rule of singa_hip_gen.h plus
 * a bonding-capacity rule: every drawn row still ends with `eos` before its columns run out and still parses, and in the
 * molecule it spells no atom carries more bond order than the capacity of its token.  A NECESSARY condition for chemical
 * validity, not a sufficient one: aromaticity, kekulisation, duplicate ring bonds (C12CC12) and %nn closures stay out of
 * scope.  (Beam search takes this rule through singa_hip_beam.h.)
 *
 * Capacity of a token.  cap[V] bytes, derived by the caller from the vocabulary's strings (singa_amd.smiles.capacity): 0..7
 * for an ATOM token, 0 for every other token.  UPPER bounds, so that no valid string is excluded:
 *     B 3    C, Si 4    N 3    O 2    P, As 5    S, Se 6    F, Cl, Br, I 1
 * A lower-case (aromatic) symbol takes its element's value.  A bracket atom is read as
 * [isotope? element chirality? H-count? charge?]; its capacity is table[element] + the charge term - the H count, clamped to
 * 0..7.  The charge term is + charge for the N, O and halogen groups ([N+] 4, [O-] 1, [Cl-] 0), - charge for B ([B-] 4) and
 * - |charge| for C and Si.  An element outside the table, or a bracket that does not read this way, gets 7 (no constraint).
 *
 * Bond order: 2 for '=', 3 for '#', 1 for every other bond symbol and for no symbol.  cls[V] are the class bytes of
 * singa_hip_gen.h, and the high nibble of a BOND token holds its order - 1 (0, 1 or 2; singa_amd.smiles.classify_orders).
 *
 * Row state.  gstate[rows] is the word of singa_hip_gen.h, unchanged but for one limit: depth is at most 10.  vstate[rows][2],
 * int32:
 *   word 0   bits 0-2    att    remaining capacity of the atom the next bond attaches to
 *            bits 3-4    pend   order of a pending bond symbol, 0 = none
 *            bit  5      first  the next atom is the first of a branch: its bond is also charged to the top of the stack
 *            bits 6-14   rord   bit d set: open ring d has order 2 (the bit of a ring that is not open means nothing)
 *   word 1   bits 3l .. 3l+2, l = 0 .. 9: stack[l], `att` of the branch point of open level l; the top is level depth - 1; the
 *            entries of levels >= depth are 0
 * A row whose prev is START reads both words as 0, whatever they hold: a fresh row and a streamed restart
 * (singa_stream_refill resets gstate alone) need no reset of vstate.
 *
 * Which token may follow.  A = prev in {ATOM, RING, CLOSE}; E = the maximum over the live stack entries (levels < depth), and
 * over att as well when A holds.  A token may follow if the rule of singa_hip_gen.h allows it - with depth < 10 in place of
 * depth < 63 for OPEN and without that rule's budget term - AND:
 *   ATOM y           o = 0 after START or DOT, else pend or 1.  If o > 0: att >= o and cap[y] >= o.
 *                    Then: if first, the stack top loses o; att = cap[y] - o, first = pend = 0 (here = 0).
 *                    Refused if a ring is open and E < 1 afterwards.
 *   BOND of order o  att >= o.  Then pend = o.
 *   OPEN             att >= 1 (and depth < 10).  Then att is pushed - it stays the attach capacity - and first = 1.
 *                    (So `F(` is allowed - F(C) spells fluoromethane; what the rule refuses is the second bond: the last C of
 *                    `F(C)C`, the '=' of `F(=`.)
 *   CLOSE            if a ring is open: some live stack entry >= 1.  Then att = the popped entry.
 *   RING d, opening  o = pend or 1.  o <= 2 and att >= o.  Then att -= o, rord[d] = (o == 2), pend = 0.
 *                    Refused if E < 1 afterwards.
 *   RING d, closing  o = the order of d (2 if rord[d], else 1).  att >= o.  Then att -= o.
 *                    Refused if a ring remains open and E < 1 afterwards.
 *   DOT              as in the SMILES rule; att = 0.
 *   EOS              as in the SMILES rule.
 * The state word itself moves as singa_hip_gen.h says.
 *
 * Budget.  rem as in singa_hip_gen.h.  A non-EOS token needs rem >= need(state'), state' the state after the token, where
 *   need = depth + 1 + a + 2 k - b,
 *   k = the number of open rings,
 *   a = 1 if prev in {START, DOT, BOND, BONDX, OPEN},
 *   b = 1 if k > 0, prev in {ATOM, RING} and some closing digit passes the rule above in that state.
 * need is at most 30.  Why no row dead-ends: while a ring is open an attach point of capacity >= 1 exists (E >= 1); from there
 * a chain of capacity-4 atoms closes any set of order-1 and order-2 rings, one ring per atom - 2 k - b counts exactly that -
 * so from every state some allowed token lowers need by at least one.  THE CALLER therefore has to offer an ATOM token of
 * capacity >= 4 (singa_amd.smiles.check_arguments refuses a vocabulary or a `suppress` without one).
 *
 * singa_sample_token_valence: the token choice of singa_sample_token_grammar on the effective mask allowed[i] (null: all) AND
 * this rule evaluated on gstate[row], vstate[row], cls[i], cap[i] and rem; gstate[row] and vstate[row] become the state after
 * the emitted token.  The arguments are the union of singa_sample_token_forced's and singa_sample_token_stream's:
 *   forced, rank   null, or as in singa_hip_force.h (rank only with forced): a forced token takes the transition WHETHER OR NOT
 *                  THE RULE WOULD HAVE ALLOWED IT - validating a prefix is the host's job (singa_amd.smiles.check_forced walks
 *                  it through singa_valence_rule_host);
 *   mol            null: rows as in singa_sample_token_grammar (`molecules` is ignored).  Non-null: the stream form of
 *                  singa_hip_stream.h - pos is [rows], the outputs and the uniforms are indexed by molecule, finished and live
 *                  are not read (they may be null), next, gstate and vstate stay the row's.  forced and mol exclude each other.
 * A finished row, a retired row and a row whose effective mask is empty keep all three state words.  allowed_logp as in
 * singa_hip_gen.h, against this stricter mask.
 * Errors: those of singa_sample_token_grammar; SINGA_E_NULL also for null cap / vstate and for rank without forced;
 * SINGA_E_SHAPE also for forced together with mol and for mol with molecules < 1. */
#ifndef SINGA_HIP_VALENCE_H
#define SINGA_HIP_VALENCE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_sample_token_valence(const float* logits, const float* uniforms, const unsigned char* allowed,
                               const unsigned char* cls, const unsigned char* cap, const long long* pos, const int32_t* mol,
                               int pos_offset, int rows, int molecules, int V, int T, float tau, int top_k, float top_p, int eos,
                               int pad, unsigned char* finished, int32_t* length, float* sum_logp, long long* tokens,
                               long long* next, int32_t* live, float* tok_logp, int32_t* gstate, int32_t* vstate,
                               float* allowed_logp, const long long* forced, int32_t* rank, void* stream);

/* The same rule on the HOST (all pointers are host pointers, nothing is enqueued): for i < n, ok[i] = 1 if the token of class
 * byte cls[i] and capacity cap[i] may follow (state[i], vstate[i][0..1]) with rem[i] columns left, else 0; next_state[i] and
 * next_vstate[i][0..1] = the state after that token if it may, the given words otherwise.  Part of every build of the
 * library: the kernel and this function share one source. */
int singa_valence_rule_host(const unsigned char* cls, const unsigned char* cap, const int32_t* state, const int32_t* vstate,
                            const int32_t* rem, int n, unsigned char* ok, int32_t* next_state, int32_t* next_vstate);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_VALENCE_H */
