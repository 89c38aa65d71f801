/* Dense attention (k19) over the score tiles the mask leaves standing.  NOT part of the drop-in training ABI
 * (include/singa_hip.h): these entry points exist for `ops.attn_tiles` / `ops.attention(..., tiles=...)` of singa_amd/ops.py.
 * Conventions as in singa_hip.h (device pointers, `stream`, SINGA_E_* return codes).
 *
 * The k19 kernels work on 32 x 32 tiles of the [T, S] score matrix: query tile qt holds the queries [32 qt, 32 qt + 32), key
 * tile kt the keys [32 kt, 32 kt + 32); qtiles = ceil(T / 32), ktiles = ceil(S / 32).  The TILE MAP holds one bit per pair
 * (qt, kt) of every batch entry, "compute", in both orientations:
 *   tile_rows  u32 [B][qtiles][ceil(ktiles / 32)]   bit kt % 32 of word kt / 32: pair (qt, kt); read by the forward and dQ
 *   tile_cols  u32 [B][ktiles][ceil(qtiles / 32)]   bit qt % 32 of word qt / 32: the same pair; read by the dK / dV pass
 * Bits past the last tile of a row are 0.  The kernels find the next computed tile with a find-first-set on these words.
 *
 * singa_attn_tiles writes the map of a byte mask (nonzero = masked) with the batch and row strides singa_attn_fwd takes (row
 * stride 0: one mask row for all queries).  The bit of (qt, kt) is CLEARED exactly when
 *   every element (q, k) of the pair with q < T is masked - a key k >= S counts as masked - AND
 *   no query row q < T of tile qt is masked over all of [0, S).
 * Under that rule a skipped pair contributes exact zeros: a masked score is -1e9, so beside one unmasked key of the same row
 * its weight exp(-1e9 - max) is 0 in f32.  A row masked in all keys spreads its weight evenly over them, so its query tile keeps
 * every bit (with row stride 0: the whole batch entry does).  A key tile may have no computed pair at all; its dK / dV rows
 * are zeros.
 *
 * singa_attn_tiled_fwd / singa_attn_tiled_bwd are singa_attn_fwd / singa_attn_bwd with the map of their mask: the same
 * arguments, checks and outputs; the results are the ones the untiled entry points give, bit for bit up to the sign of a zero.
 * A null tile_rows (tile_cols) makes the passes that read it visit every tile, as the untiled entry points do.  The map has to
 * be the one singa_attn_tiles made from the same mask, T and S: a map that clears other bits gives other results (but never
 * an access outside the operands). */
#ifndef SINGA_HIP_ATTN_TILES_H
#define SINGA_HIP_ATTN_TILES_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_attn_tiles(const unsigned char* mask, long long mask_stride_b, long long mask_stride_t, uint32_t* tile_rows,
                     uint32_t* tile_cols, int B, int T, int S, void* stream);

int singa_attn_tiled_fwd(const float* q, const float* k, const float* v, const unsigned char* mask, long long mask_stride_b,
                         long long mask_stride_t, float* ctx, float* lse, int BH, int T, int S, int heads, int DK, int DV,
                         int token_major, long long ld_q, long long ld_k, long long ld_v, float scale, const uint32_t* tile_rows,
                         void* stream);

int singa_attn_tiled_bwd(const float* q, const float* k, const float* v, const unsigned char* mask, long long mask_stride_b,
                         long long mask_stride_t, const float* ctx, const float* lse, const float* g_ctx, float* g_q, float* g_k,
                         float* g_v, float* dsum, int BH, int T, int S, int heads, int DK, int DV, int token_major, long long ld_q,
                         long long ld_k, long long ld_v, float scale, const uint32_t* tile_rows, const uint32_t* tile_cols,
                         void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_ATTN_TILES_H */
