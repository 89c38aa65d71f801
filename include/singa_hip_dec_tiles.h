/* The decoder step of generation with a TILE OF ROWS as the unit of work.  NOT part of the drop-in training ABI
 * (include/singa_hip.h) and none of the other generation-time headers: these entry points exist for `tiles=True` of
 * `ops.dec_layer_step` / `KVDecoder` (singa_amd/model/BeamSearch.py).  Conventions as in singa_hip.h (device pointers, `stream`,
 * SINGA_E_* return codes).
 *
 * singa_dec_self_attn / singa_dec_self_attn_rows, singa_dec_cross_attn and singa_dec_ffn give one workgroup to one row and let it
 * read the layer's weights itself: built for a few dozen rows.  Here a workgroup serves 16 consecutive rows: the weights are read
 * once per tile and meet the tile's rows on the f32 matrix cores (v_mfma_f32_16x16x4_f32).  Operands, layouts and semantics are
 * those of the per-row entry points, to the letter:
 *   wqkv_t [256][512] (q | k | v), wo_t [256][256], wq_t [256][128], w1_t [256][1024], w2_t [1024][256], biases, LayerNorm affine
 *   k_cache [R][4][P][32], v_cache [R][4][P][64]; ck [B][4][32][S], cv [B][4][S][64], pad [B][S] (non-zero = padding)
 *   rows are pocket-major: row r belongs to pocket r / beams, R = B * beams.
 * Self-attention: q | k | v of the new position with bias, k and v appended at pos, attention of each head over positions
 * 0 .. pos (the new position's own key and value come from on-chip memory), scale 1/sqrt(32), output projection + bias + residual
 * + LayerNorm.  per_row = 0: pos is [1], one position for all rows; per_row != 0: pos is [R], row r appends at and attends up to
 * pos[r], positions behind it are masked like unwritten ones.  A row whose position lies outside [0, P) is left alone: neither its
 * caches nor its row of y are written.  Encoder-decoder attention: padded positions score -1e9f, not -inf, so a fully padded
 * pocket yields the plain average of its value rows; the keys are walked in chunks of 64 positions with a running maximum and
 * sum, in ascending order, so S has no upper limit.  Feed-forward: 256 -> 1024 (ReLU) -> 256, residual, LayerNorm.
 *
 * Tiles.  The two attention entry points cut every pocket's rows into tiles of 16 (grid = B * ceil(beams / 16)): no tile holds
 * rows of two pockets, the last tile of a pocket is partial, and the rows it lacks are neither read nor written.  The
 * feed-forward cuts the R rows as they come.  Every output element is a sum over its own row's data in an order that depends on
 * nothing else: a row's results do not depend, to the bit, on which rows share its tile or on where in the batch it stands.  No
 * atomic operation, nothing shared between workgroups.
 *
 * Limits: the shipped decoder geometry (hidden 256, 4 heads of 32 key / 64 value channels, feed-forward 1024) is built in;
 * 1 <= P <= 256, S >= 1, beams >= 1, R a multiple of beams; anything else is SINGA_E_SHAPE, a missing pointer SINGA_E_NULL, both
 * before any device call.  R = 0 is a successful no-op. */
#ifndef SINGA_HIP_DEC_TILES_H
#define SINGA_HIP_DEC_TILES_H
#ifdef __cplusplus
extern "C" {
#endif
int singa_dec_tile_self_attn(const float* x, const float* wqkv_t, const float* bqkv, const float* wo_t, const float* bo,
                             const float* gamma, const float* beta, float* k_cache, float* v_cache, const long long* pos,
                             int per_row, int R, int beams, int P, float* y, float eps, void* stream);

int singa_dec_tile_cross_attn(const float* y, const float* wq_t, const float* bq, const float* ck, const float* cv,
                              const unsigned char* pad, const float* wo_t, const float* bo, const float* gamma, const float* beta,
                              int R, int beams, int S, float* z, float eps, void* stream);

int singa_dec_tile_ffn(const float* z, const float* w1_t, const float* b1, const float* w2_t, const float* b2, const float* gamma,
                       const float* beta, int R, float* out, float eps, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_DEC_TILES_H */
