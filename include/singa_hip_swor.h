/* Sampling WithOut Replacement: k distinct sequences per pocket by stochastic beam search (Kool, van Hoof, Welling 2019,
 * "Stochastic Beams and Where to Find Them": Gumbel-top-k over the sequence tree).  NOT part of the drop-in training ABI
 * (include/singa_hip.h) and none of the other generation-time headers: these entry points exist for `sample_distinct` of
 * singa_amd/model/Sampling.py.  Conventions as in singa_hip.h (device pointers, `stream`, SINGA_E_* return codes).
 *
 * THE RULE.  Rows are pocket-major, k slots per pocket (rows = pockets * k).  Per slot the device holds
 *   gumbel    f32   G, the perturbed log-probability of the slot's prefix; -inf marks a DEAD slot
 *   prop_logp f32   phi, the log-probability of the prefix under the proposal (temperature, `allowed`, grammar)
 *   sum_logp  f32   the log-probability under the unmodified model, accumulated as singa_sample_token accumulates it
 *   hash      u64   prefix hash
 *   finished  u8, length i32, gstate i32 (grammar on), tokens[T] i64, tok_logp[T] f32: as in singa_sample_token(_grammar)
 * A run starts with slot 0 of every pocket as the root (G = 0, phi = 0, sum_logp = 0, hash = 0, prefix '&', gstate FRESH) and
 * every other slot dead.  The step index is t = *pos - pos_offset, read on the device, so that a captured launch replays;
 * a step outside 0 <= t < T - 1 writes nothing.  Step t is singa_swor_expand, then singa_swor_select.
 *
 * 1. Proposal (expand; per live - not dead, not finished - parent slot i).  The mask is `allowed` AND, with cls / gstate
 *    given, smiles_allows(gstate[i], cls[v], T - 2 - t) of singa_hip_gen.h.  q = log-softmax of z / tau over the masked
 *    tokens.  The model's own log-probability of token v is z_v - lse with lse = zmax + logf(sum expf(z - zmax)) over all V
 *    tokens: the expressions of singa_sample_token, so that it carries the same bits.
 * 2. Noise.  x = the first output word of Philox4x32-10 with key (seed & 0xffffffff, seed >> 32) and counter
 *    (hash_i & 0xffffffff, hash_i >> 32, v, streams[pocket]);  u = ((float)(x >> 8) + 0.5f) * 2^-24 in f32 arithmetic, and a u
 *    that rounds to 1 is replaced by 1 - 2^-24.  g_v = phi_i + q_v - log(-log u).  The noise is keyed by the parent's prefix
 *    hash, not by slot or step; the child's hash is splitmix64's finaliser of h + (v + 1) * 0x9E3779B97F4A7C15:
 *        z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31.
 *    The perturbed tree is therefore a function of (seed, stream, prefix) alone.
 * 3. Conditioning on the parent's G.  Z = max_v g_v over the mask;  d = g_v - Z;  a = G_i - g_v + log1p(-exp(d));
 *    g~_v = G_i - max(a, 0) - log1p(exp(-|a|)).  The arg-max child receives exactly G_i.  Masked tokens are no candidates.
 *    Sub-steps 2 and 3 are evaluated in double precision from the f32 q, phi and G (log1p(-exp(d)) magnifies the rounding
 *    of a g close to Z by 1 / |d|), and g~ is rounded to f32 once.
 *    expand writes, for every row and all V tokens, cand = g~_v, cand_logp = z_v - lse and cand_phi = phi_i + q_v, each -inf
 *    where the token is no candidate.
 * 4. A finished parent is one candidate of its own: token `pad`, cand = G_i, cand_logp = 0, cand_phi = phi_i.  A dead parent
 *    has no candidate.
 * 5. Selection (select; per pocket).  The new slots are the k candidates with the largest g~ in descending order; ties go to
 *    the lower parent slot, then to the lower token.  Fewer than k candidates leave the trailing slots dead.  New slot j with
 *    candidate (parent i, token v):  gumbel = g~,  prop_logp = cand_phi,  sum_logp = sum_logp_i + cand_logp,  hash = child
 *    hash,  length_i + 1,  finished = (v == eos),  gstate = the state after v;  columns 0 .. t of tokens / tok_logp are the
 *    parent's, column t + 1 receives v / cand_logp;  next = v.  A finished parent's candidate copies the parent (column t + 1:
 *    pad / 0, next = pad).  A dead slot: gumbel = prop_logp = -inf, sum_logp = 0, hash = 0, length = 0, finished = 0, gstate
 *    kept, column 0 kept, columns 1 .. t + 1 pad / 0, next = pad.  src[row] = the parent's row (a dead slot: its own row),
 *    live[pocket] = the number of new slots that are neither dead nor finished, written in full every step.
 *
 * Limits: 1 <= k <= 2048, 1 <= V <= 1024, T >= 2 (3 with the grammar); anything else is SINGA_E_SHAPE.  cls and gstate go
 * together (SINGA_E_NULL for one without the other).  tau > 0.  Nothing is allocated: `work` is caller-provided scratch of
 * singa_swor_work(rows, T) bytes, 16-byte aligned, which select uses to hold the new row state until every parent is read.
 * One workgroup serves one pocket in select (radix select of the k-th largest of k * V ordered float keys, then a sort of the
 * k survivors in LDS); the parents' columns are gathered and the state committed by two row-parallel launches behind it. */
#ifndef SINGA_HIP_SWOR_H
#define SINGA_HIP_SWOR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The noise of the rule on the CPU (one source with the kernel): for i < n, x[i] = the Philox word, u[i] = the uniform,
 * child[i] = the child hash of (hash[i], v[i]).  Any output may be null. */
int singa_swor_noise_host(unsigned long long seed, const unsigned long long* hash, const int32_t* v, const uint32_t* streams,
                          int n, uint32_t* x, float* u, unsigned long long* child);

/* bytes of scratch singa_swor_select needs; -1 for rows < 0 or T < 2 */
long long singa_swor_work(int rows, int T);

int singa_swor_expand(const float* logits, const unsigned char* allowed, const unsigned char* cls, const long long* pos,
                      int pos_offset, int rows, int k, int V, int T, float tau, unsigned long long seed,
                      const uint32_t* streams, int pad, const float* gumbel, const float* prop_logp,
                      const unsigned long long* hash, const unsigned char* finished, const int32_t* gstate, float* cand,
                      float* cand_logp, float* cand_phi, void* stream);

int singa_swor_select(const float* cand, const float* cand_logp, const float* cand_phi, const unsigned char* cls,
                      const long long* pos, int pos_offset, int rows, int k, int V, int T, int eos, int pad, float* gumbel,
                      float* prop_logp, float* sum_logp, unsigned long long* hash, unsigned char* finished, int32_t* length,
                      int32_t* gstate, long long* tokens, float* tok_logp, long long* next, long long* src, int32_t* live,
                      void* work, void* stream);

/* One launch: for every layer, head and row r that is neither dead (gumbel[r] == -inf) nor finished, positions [0, *pos) of
 * the key / value cache rows src[r] of (k_src, v_src) are copied to row r of (k_dst, v_dst), as 16-byte accesses.  The caches
 * are [layers][rows][heads][P][dk] and [..][dv] f32 with the row and layer pitches given in floats (both buffers alike);
 * dk, dv and the pitches are multiples of 4 and the bases 16-byte aligned (SINGA_E_SHAPE otherwise).  *pos is clamped to P;
 * a src[r] outside [0, rows) skips the row.  Nothing else is written, and the source buffers are only read. */
int singa_swor_follow(const float* k_src, const float* v_src, float* k_dst, float* v_dst, const long long* src,
                      const float* gumbel, const unsigned char* finished, const long long* pos, int layers, int rows,
                      int heads, int P, int dk, int dv, long long k_row_ld, long long k_layer_ld, long long v_row_ld,
                      long long v_layer_ld, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_SWOR_H */
