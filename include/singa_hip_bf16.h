/* The real GEMM (k7) with bf16 operands on the matrix cores.  NOT part of the drop-in training ABI (include/singa_hip.h): this
 * entry point exists for `precision="bf16"` of singa_amd/ops.py (the CProMG transformer's Linears).  Conventions as in
 * singa_hip.h (device pointers, `stream`, SINGA_E_* return codes).
 *
 * singa_gemm_bf16 is singa_gemm_f32 with rounded operands: the same singa_gemm_t records, operand forms (1, 1) / (1, 0) / (0, 0),
 * tile shapes and their selection rule, grouped rows, `splits` / c_split_stride, epilogue options and alignment rules; it accepts
 * what singa_gemm_f32 accepts and refuses the rest with the same codes.  What it computes:
 *     c[i, j] = epilogue( sum_r bf16(A(i, r)) * bf16(B(r, j)) )
 *   bf16(x): the f32 value x rounded to the nearest bf16 (8 significant bits), ties to even - 1 + 2^-8 gives 1, 1 + 3 * 2^-8 gives
 *     1 + 2^-6; infinities stay, a NaN stays a NaN.  The rounding happens inside the kernel, on the way from the f32 global
 *     loads to LDS: nothing in memory is bf16, no copy of an operand is kept.
 *   Products and sums are f32 (v_mfma_f32_32x32x16_bf16); a product of two bf16 values is exact in f32.
 *   The epilogue - bias, addend, ReLU, mask - works on the f32 sums exactly as singa_gemm_f32's.
 *   asum (the (0, 0) form's column sums of A) is taken from the UNROUNDED f32 values: bit for bit what singa_gemm_f32 returns for
 *     the same operands and splits.
 *
 * singa_cgemm_bf16 is the complex product of singa_cgemm3m_f32 with rounded operands, for `embedding_precision="bf16"` (the SO(2)
 * convolutions of the equivariant embedding): the same singa_cgemm_t records, operand forms, part offsets a_im / b_im / c_im,
 * sigma = +1 or -1, `splits` / c_split_stride, up to SINGA_CGEMM_MAX problems per launch and alignment rules; it accepts what
 * singa_cgemm3m_f32 accepts and refuses the rest with the same codes.  With A = a + i b, B = c + i sigma d and ^ = bf16():
 *     re[i, j] = sum_r a^(i, r) c^(r, j)  -  sigma * sum_r b^(i, r) d^(r, j)
 *     im[i, j] = sum_r b^(i, r) c^(r, j)  +  sigma * sum_r a^(i, r) d^(r, j)
 *   Four real products, not 3M's three: every operand value is rounded once, no sum of operand parts is rounded a second time.
 *   Products and sums are f32 (v_mfma_f32_32x32x16_bf16), the order of the f32 additions is the kernel's own; the rounding
 *   happens inside the kernel as for singa_gemm_bf16.
 * Enqueue-only on `stream`. */
#ifndef SINGA_HIP_BF16_H
#define SINGA_HIP_BF16_H
#include "singa_hip.h"
#ifdef __cplusplus
extern "C" {
#endif
int singa_gemm_bf16(const singa_gemm_t* probs, int n, int a_r_contig, int b_r_contig, int splits, void* stream);
int singa_cgemm_bf16(const singa_cgemm_t* probs, int n, int a_r_contig, int b_r_contig, int splits, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_BF16_H */
