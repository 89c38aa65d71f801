/* The kNN edge MLPs once per undirected edge (include/singa_hip_units.h) with bf16 operands on the matrix cores (k15e).  NOT part
 * of the drop-in training ABI (include/singa_hip.h): these entry points exist for `ops.edge_mlp_pair(..., units=...,
 * precision="bf16")` of singa_amd/ops.py.  Conventions as in singa_hip.h (device pointers, `stream`, SINGA_E_* return codes,
 * nn.Linear's own parameter layouts).
 *
 * Arguments, the units contract and the error codes are those of singa_edge_mlp_units_fwd / _bwd: unit_a / unit_b name the units,
 * rows that no unit names are not written, no access leaves the arrays whatever the lists hold, `part` has the layout and the
 * singa_edge_mlp_bwd_nparts(E, H) rows of singa_edge_mlp_bwd and every row is written, E == 0 does nothing.  There is no
 * directed-row form.
 *
 * What is computed, with ^ = bf16(): the f32 value rounded to the nearest bf16 (8 significant bits), ties to even:
 *   forward    h = ssp(W1^ attr^ + b1),  out = W2^ h^ + b2                       for both nets, written f32 at rows a and b
 *   backward   g = g_out[a] + g_out[b] (b != a), added in f32;  pre = W1^ attr^ + b1,  h = ssp(pre)
 *              gh = W2^T^ g^,  g_pre = gh * sigmoid(pre)                          (gh is no operand of a product: it stays f32)
 *              dW2 = sum over units of g^ h^T,   dW1 = sum over units of g_pre^ attr^T
 *              db2 = sum of g, db1 = sum of g_pre: the UNROUNDED f32 values
 *   Every operand of every matrix product is rounded once; products and sums are f32 (v_mfma_f32_32x32x16_bf16); biases, the
 *   softplus and its derivative are f32.  The rounding happens in registers and on the way to LDS: nothing in memory is bf16.
 *
 * SINGA_E_NULL for a null pointer; SINGA_E_SHAPE unless CIN == 64, (HK, HV) == (32, 64) / H in {32, 64}, E >= 0 and attr, wk,
 * wv, g_out are 16-byte aligned.  Enqueue-only on `stream`. */
#ifndef SINGA_HIP_EMLP_BF16_H
#define SINGA_HIP_EMLP_BF16_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_edge_mlp_bf16_units_fwd(const float* attr, const int32_t* unit_a, const int32_t* unit_b, const float* w1tk, const float* b1k,
                                  const float* w2tk, const float* b2k, const float* w1tv, const float* b1v, const float* w2tv,
                                  const float* b2v, float* wk, float* wv, int E, int CIN, int HK, int HV, void* stream);

int singa_edge_mlp_bf16_units_bwd(const float* attr, const int32_t* unit_a, const int32_t* unit_b, const float* g_out, const float* w1t,
                                  const float* b1, const float* w2, float* part, int E, int CIN, int H, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_EMLP_BF16_H */
