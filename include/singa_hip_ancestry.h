/* Ancestry-indexed key / value caches: the rows of a pocket exchange prefixes without moving a cache entry.  NOT part of the
 * drop-in training ABI (include/singa_hip.h) and none of the other generation-time headers: these entry points exist for
 * `cache="ancestry"` of `sample_distinct` (singa_amd/model/Sampling.py) and `beam_search_device` (singa_amd/model/BeamSearch.py),
 * through `ops.dec_layer_step(..., anc=...)`, `ops.anc_follow` and `KVDecoder(..., ancestry=True)`.  Conventions as in singa_hip.h
 * (device pointers, `stream`, SINGA_E_* return codes).
 *
 * THE RULE.  Rows are pocket-major, k slots per pocket (R = pockets * k).  A key / value entry at (slot, position) of
 * k_cache [R][4][P][32] / v_cache [R][4][P][64] is written once, by the row that stands in that slot when the position is
 * appended, and never changed afterwards.  A row's past is therefore one small integer per position:
 *   anc   int32 [P][R], position-major;  anc[p][r] = the absolute row (slot) whose caches hold position p of row r's prefix.
 * A slot only ever names slots of its own pocket.  The identity (anc[p][r] = r) is the state after a reset: every row owns its
 * past, which is what the plain entry points assume.
 *
 * 1. Self-attention through the table (singa_dec_self_attn_anc, singa_dec_tile_self_attn_anc: singa_dec_self_attn of
 *    singa_hip.h and singa_dec_tile_self_attn of singa_hip_dec_tiles.h with one more operand).  q | k | v of the new position are
 *    appended at (row r, pos), as there.  For every cached position tt < pos the key and the value of head h are read from slot
 *    anc[tt][r] instead of r; the new position's key and value come from on-chip memory.  Everything else - the order of the
 *    score loop, the sums, the order in which the partial context sums meet, output projection, residual, LayerNorm - is the
 *    plain kernel's code: given equal cache contents a row's result equals the plain entry point's bit for bit.  Only rows
 *    tt < pos of the table are read.  A table entry outside the valid slots (the R rows; for the tiled form the row's pocket) is
 *    clamped into them, so that a damaged table yields wrong numbers, never a read outside the caches.
 *    One position for all rows only: pos is [1]; singa_dec_tile_self_attn_anc refuses per_row != 0 with SINGA_E_SHAPE.
 *
 * 2. The table follows a re-ranking (singa_anc_follow).  `src` [R] int64 names every row's parent row, as singa_swor_select /
 *    singa_beam_select write it.  The launch stands where singa_swor_follow stands: BEHIND the step's increment of the
 *    position, so n = *pos, read on the device (a captured launch replays), counts the positions written so far and t = n - 1 is
 *    the one this step's self-attention appended.  For every row r whose src[r] lies in r's pocket:
 *      anc[p][r] = anc_before[p][src[r]]   for every p < t
 *      anc[t][r] = src[r]                  (the parent wrote position t into its own slot)
 *    Positions > t are untouched, and so is a row whose src[r] lies outside its pocket.  n <= 0 or n > P writes nothing.
 *    The update is in place: a slot may be the parent of a slot before it and may have many children.  One workgroup per
 *    (pocket, position) loads the pocket's k entries of that position into LDS (8 KB), meets at a barrier and writes the gathered
 *    column back; workgroups of positions beyond t leave at once.  No second table, no scratch, no atomic operation.
 *
 * Limits: the shipped decoder geometry (hidden 256, 4 heads of 32 key / 64 value channels) is built in; 1 <= P <= 256; for the
 * tiled form and the update R is a multiple of beams / k, beams >= 1, 1 <= k <= 2048; anything else is SINGA_E_SHAPE, a missing
 * pointer SINGA_E_NULL, both before any device call.  R = 0 is a successful no-op. */
#ifndef SINGA_HIP_ANCESTRY_H
#define SINGA_HIP_ANCESTRY_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_dec_self_attn_anc(const float* x, const float* wqkv_t, const float* bqkv, const float* wo_t, const float* bo,
                            const float* gamma, const float* beta, float* k_cache, float* v_cache, const long long* pos, int R,
                            int P, float* y, float eps, const int32_t* anc, void* stream);

int singa_dec_tile_self_attn_anc(const float* x, const float* wqkv_t, const float* bqkv, const float* wo_t, const float* bo,
                                 const float* gamma, const float* beta, float* k_cache, float* v_cache, const long long* pos,
                                 int per_row, int R, int beams, int P, float* y, float eps, const int32_t* anc, void* stream);

int singa_anc_follow(int32_t* anc, const long long* src, const long long* pos, int rows, int k, int P, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_ANCESTRY_H */
