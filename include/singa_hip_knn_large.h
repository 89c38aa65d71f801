/* n1 for molecules of any size: a kNN graph kernel that streams its candidates.  Beside the drop-in training ABI
 * (include/singa_hip.h), whose singa_knn_graph keeps its signature and its limit of 2,048 atoms per molecule: this entry point
 * exists for `ops.knn_graph(..., route=...)`, which takes it above that limit.  Conventions as in singa_hip.h (device pointers,
 * `stream`, SINGA_E_* return codes).
 *
 * singa_knn_graph's contract, word for word: pos [N, 3] fp32, batch [N] int32 (the molecule of every atom; ids outside [0, B) =
 * atoms of no molecule), ptr [B + 1] int64 (molecule g owns the atoms ptr[g] .. ptr[g+1] - 1) -> row, col [N * k] int64: for
 * every atom its k nearest other atoms of the same molecule, row = centre, col = neighbour, k consecutive slots per atom in
 * increasing order of the 64-bit key  float_bits(d2) << 32 | atom index  with d2 = (dx*dx + dy*dy) + dz*dz from exact fp32
 * differences and no contraction: exact ties go to the lower index, and the order is total, so the output is the integers
 * singa_knn_graph writes.  -1 in the slots that do not exist (molecules of fewer than k + 1 atoms, atoms of no molecule).
 *
 * 1 <= k <= 64.  SINGA_E_NULL for a null pointer; SINGA_E_SHAPE for any other k, a negative size, or 3 * N or N * k beyond an
 * int32 count; all of it before any HIP call.  N == 0 does nothing, with any B; with B == 0 every atom is one of no molecule. */
#ifndef SINGA_HIP_KNN_LARGE_H
#define SINGA_HIP_KNN_LARGE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_knn_graph_large(const float* pos, const int32_t* batch, const long long* ptr, int B, int N, int k, long long* row,
                          long long* col, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_KNN_LARGE_H */
