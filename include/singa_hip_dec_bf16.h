/* The row-tiled decoder step of generation with its weight products on the bf16 matrix cores (k20b).  NOT part of the drop-in
 * training ABI (include/singa_hip.h) and none of the other generation-time headers: these entry points exist for
 * `ops.dec_layer_step(..., tiles=True, precision="bf16")` / `KVDecoder(..., precision="bf16")` (singa_amd/model/BeamSearch.py).
 * Conventions as in singa_hip.h (device pointers, `stream`, SINGA_E_* return codes).
 *
 * The three step entry points keep the contract of singa_dec_tile_self_attn (and its _anc form), singa_dec_tile_cross_attn and
 * singa_dec_tile_ffn of include/singa_hip_dec_tiles.h / include/singa_hip_ancestry.h to the letter - operands, layouts, cache
 * appends, per_row positions, rows outside [0, P) left alone, padded positions at -1e9f, the walk over the pocket in chunks of 64
 * positions (no limit on S), tiles of 16 rows that never span two pockets, partial tiles that neither read nor write the rows they
 * lack, no atomics, nothing shared between workgroups, a row's bits independent of its tile and of its place in the batch - with
 * two differences:
 *   - every weight MATRIX argument (wqkv, wo, wq, w1, w2) is the packed bf16 image singa_dec_bf16_pack made of the transposed f32
 *     matrix the f32 entry point takes, 16-byte aligned; biases and the LayerNorm affine stay f32;
 *   - `anc` is an argument of the one self-attention entry point: null = the caches are read in place, otherwise the int32
 *     [P][R] ancestry table of include/singa_hip_ancestry.h, which goes with per_row = 0 only.
 *
 * singa_dec_bf16_pack(w_t [K][N] f32, K, N, packed): K * N bf16 values (2 K N bytes), each the f32 value rounded to the nearest
 * bfloat16, ties to even, in the order the step kernels read them: fragment ((n / 16) * (K / 32) + k / 32) * 64 + 16 g + i holds
 * w_t[32 (k / 32) + 8 g + j][16 (n / 16) + i], j = 0 .. 7.  K a multiple of 32, N a multiple of 16.  Called once per matrix.
 *
 * Numerics contract, with ^ = bf16(): round to nearest, ties to even.
 *   q | k | v = x^ Wqkv^ + b        ctx (f32 attention over the f32 caches, as the f32 kernels)     y = LN(ctx^ Wo^ + bo + x)
 *   q = y^ Wq^ + bq                 ctx (f32 attention over the f32 encoder keys / values)          z = LN(ctx^ Wo^ + bo + y)
 *   h = relu(z^ W1^ + b1)           out = LN(h^ W2^ + b2 + z)
 *   Each left operand is rounded once, from the f32 value the step computed, on the way into the matrix-core operand
 *   (v_mfma_f32_16x16x32_bf16).  What stays f32: all accumulators, biases, residuals (the unrounded x, y, z), the LayerNorms, the
 *   appended key and value rows and everything read from the caches and the encoder rows, scores, softmax, every output.
 *
 * Limits and errors as in singa_hip_dec_tiles.h: SINGA_E_NULL for a null pointer other than `anc`; SINGA_E_SHAPE unless
 * 1 <= P <= 256, S >= 1, beams >= 1, R >= 0 a multiple of beams, per_row = 0 with a table, packed weights 16-byte aligned; both
 * before any device call.  R = 0 is a successful no-op.  Enqueue-only on `stream`. */
#ifndef SINGA_HIP_DEC_BF16_H
#define SINGA_HIP_DEC_BF16_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_dec_bf16_pack(const float* w_t, int K, int N, unsigned short* packed, void* stream);

int singa_dec_bf16_tile_self_attn(const float* x, const unsigned short* wqkv_pk, const float* bqkv, const unsigned short* wo_pk,
                                  const float* bo, const float* gamma, const float* beta, float* k_cache, float* v_cache,
                                  const long long* pos, int per_row, int R, int beams, int P, float* y, float eps, const int32_t* anc,
                                  void* stream);

int singa_dec_bf16_tile_cross_attn(const float* y, const unsigned short* wq_pk, const float* bq, const float* ck, const float* cv,
                                   const unsigned char* pad, const unsigned short* wo_pk, const float* bo, const float* gamma,
                                   const float* beta, int R, int beams, int S, float* z, float eps, void* stream);

int singa_dec_bf16_tile_ffn(const float* z, const unsigned short* w1_pk, const float* b1, const unsigned short* w2_pk, const float* b2,
                            const float* gamma, const float* beta, int R, float* out, float eps, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_DEC_BF16_H */
