/* The dense attention core with bf16 operands on the matrix cores (k19b).  NOT part of the drop-in training ABI
 * (include/singa_hip.h): these entry points exist for `ops.attention(..., precision="bf16")` of singa_amd/ops.py.  Conventions as
 * in singa_hip.h (device pointers, `stream`, SINGA_E_* return codes).
 *
 * Arguments, layouts (head-major, or token-major with the pitches ld_q / ld_k / ld_v), DK = 32 and DV = 64, the byte mask and its
 * strides, the `lse` pair (row maximum, 1 / row sum) per query, the `dsum` output and the checks are those of the f32 core
 * (singa_attn_fwd / singa_attn_bwd of singa_hip.h) and of its forms over a tile map (include/singa_hip_attn_tiles.h:
 * singa_attn_tiled_fwd, singa_attn_tiled_bwd), whose tile arguments these take: tile_rows / tile_cols are null - every tile is
 * visited - or the two orientations of the map that singa_attn_tiles made from the same mask, T and S, and then the cleared pairs
 * are skipped under the rule stated there, with the same result up to the sign of a zero.  Every tensor in memory is f32.
 *
 * Numerics contract, with ^ = bf16(): the f32 value rounded to the nearest bfloat16 (8 significant bits), ties to even.
 *   Operands.  Every operand of every matrix product is rounded once, in registers, on the way from the load registers or from an
 *   accumulator into the MFMA operand (v_mfma_f32_32x32x16_bf16): q, k, v, dO, the unnormalised probabilities p~ = exp(s - m) of
 *   the forward, the probabilities P = p~ / l of the backward, and dS.
 *     forward    s = q^ k^^T,  x = mask ? -1e9 : s * scale,  m = running max x,  p~ = exp(x - m),  l = sum p~,
 *                ctx = (sum over keys of p~^ v^) / l
 *     backward   s recomputed by the forward's instructions on the forward's q^ and k^, so P = exp(x - m) / l agrees with `lse`;
 *                D = rowsum(dO * ctx),  dP = dO^ v^^T,  dS = mask ? 0 : P (dP - D) scale,
 *                dq = dS^ k^,  dk = dS^^T q^,  dv = P^^T dO^
 *   What stays f32: all accumulators; the scale, the mask value -1e9, the running maximum and the exp; the row sum l, which adds
 *   the UNROUNDED p~; the rescale of the context accumulators; D, from the unrounded dO and ctx as the f32 core computes it; dS
 *   until it becomes an operand; every output (ctx, lse, dq, dk, dv, dsum).
 *
 * SINGA_E_NULL for a null pointer other than the tile maps; SINGA_E_SHAPE - before any HIP call - unless DK == 32, DV == 64,
 * heads > 0 divides BH and the pitches / alignments are those the f32 core accepts.  BH, T or S <= 0 does nothing.
 * Enqueue-only on `stream`. */
#ifndef SINGA_HIP_ATTN_BF16_H
#define SINGA_HIP_ATTN_BF16_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_attn_bf16_fwd(const float* q, const float* k, const float* v, const unsigned char* mask, long long mask_stride_b,
                        long long mask_stride_t, float* ctx, float* lse, int BH, int T, int S, int heads, int DK, int DV,
                        int token_major, long long ld_q, long long ld_k, long long ld_v, float scale, const uint32_t* tile_rows,
                        void* stream);

int singa_attn_bf16_bwd(const float* q, const float* k, const float* v, const unsigned char* mask, long long mask_stride_b,
                        long long mask_stride_t, const float* ctx, const float* lse, const float* g_ctx, float* g_q, float* g_k,
                        float* g_v, float* dsum, int BH, int T, int S, int heads, int DK, int DV, int token_major, long long ld_q,
                        long long ld_k, long long ld_v, float scale, const uint32_t* tile_rows, const uint32_t* tile_cols,
                        void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_ATTN_BF16_H */
