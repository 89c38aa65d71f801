/* n2 - the Laplacian positional encoding for graphs of 1 .. 2,048 atoms.  Beside the drop-in training ABI (include/singa_hip.h),
 * whose singa_lap_pe keeps its signature and its limit of 896 atoms: these entry points exist for `ops.lap_pe_large` and the
 * per-graph routing of `graph.laplacian_pe_batched`.  Conventions as in singa_hip.h (device pointers, `stream`, SINGA_E_* return
 * codes).
 *
 * singa_lap_pe's encoding, word for word: the normalised Laplacian I - D^-1/2 A D^-1/2 from LOCAL edge lists grouped by graph
 * (graph b owns eptr[b] .. eptr[b+1] - 1; A[src, dst] = 1 for every edge, repeats count once; D = in-degree clipped at 1;
 * symmetrised), the kout (<= 8) eigenvectors after the smallest, entry of largest magnitude made positive, fp32 rows
 * out[first[b] + i, 0..kout-1], zero columns for graphs of fewer than kout + 1 atoms, rows of `out` that belong to no graph not
 * touched.  The kernel keeps nothing of size O(n) in LDS and needs no [ld, ld] matrix: work = singa_lap_pe_large_work(B, ld)
 * doubles (104 per atom of ld, not initialised by the caller; 0 = B * ld beyond an int32 count), ld >= max nnodes, <= 2,048.
 * One workgroup per graph: sparse (ELL, <= 32 neighbours) rows from the edge list, the zero eigenvalue's vectors written as the
 * D^1/2-weighted indicators of the connected components, the non-zero pairs - when fewer than kout + 1 components carry a zero -
 * by Chebyshev-filtered subspace iteration (block of 16, degree 24, CholQR2, residual 2e-10, <= 40 iterations) with its blocks in
 * `work`; graphs of <= 32 atoms by dense Jacobi sweeps in LDS.
 *
 * status [B] int32 is written for every graph: 0 = its rows of `out` are written; otherwise NONE of them is, and the value says
 * why - 1 an atom with more than 32 distinct neighbours (or more than 64 edge ends, repeats included), 2 a vanishing Cholesky
 * pivot, 3 no convergence, 4 an edge list that is not symmetric, 5 an edge index outside the graph, 6 nnodes[b] > ld.
 *
 * SINGA_E_NULL for a null pointer; SINGA_E_SHAPE unless 1 <= kout <= 8, 1 <= ld <= 2,048 and the work size fits.  B <= 0 does
 * nothing. */
#ifndef SINGA_HIP_LAP_LARGE_H
#define SINGA_HIP_LAP_LARGE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_lap_pe_large_work(int B, int ld);
int singa_lap_pe_large(const int32_t* esrc, const int32_t* edst, const int32_t* eptr, const int32_t* nnodes, const int32_t* first,
                       double* work, float* out, int32_t* status, int B, int ld, int kout, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_LAP_LARGE_H */
