/* n2 - the Laplacian positional encoding for graphs of 2,049 .. 32,768 atoms, MANY workgroups per graph.  Beside
 * include/singa_hip_lap_large.h, whose one-workgroup-per-graph kernel keeps its range (1 .. 2,048 atoms) and its bits: these entry
 * points exist for `ops.lap_pe_xl` and the per-graph routing of `graph.laplacian_pe_batched`.  Conventions as in singa_hip.h
 * (device pointers, `stream`, SINGA_E_* return codes).
 *
 * The encoding is singa_lap_pe_large's, word for word: the normalised Laplacian I - D^-1/2 A D^-1/2 from LOCAL edge lists grouped
 * by graph (graph b owns eptr[b] .. eptr[b+1] - 1; A[src, dst] = 1 for every edge, repeats count once; D = in-degree clipped at
 * 1; symmetrised), the kout (<= 8) eigenvectors after the smallest, entry of largest magnitude made positive, fp32 rows
 * out[first[b] + i, 0..kout-1], rows of `out` that belong to no graph not touched.
 *
 * status [B] int32 is written for every graph: 0 = its rows of `out` are written; otherwise NONE of them is, and the value says
 * why - 1 an atom with more than 32 distinct neighbours (or more than 64 edge ends, repeats included), 2 a vanishing Cholesky
 * pivot, 3 no convergence (of the component labels within 64 rounds, or of the iteration within 40 outer iterations), 4 an edge
 * list that is not symmetric, 5 an edge index outside the graph, 6 a size this route does not take: nnodes[b] > ld, or 1 .. 2,048
 * atoms (singa_lap_pe_large's range).  nnodes[b] <= 0: status 0, nothing written.
 *
 * work: singa_lap_pe_xl_work(B, ld) doubles, not initialised by the caller, ld >= max nnodes, 2,049 <= ld <= 32,768.  The count
 * is 64-bit: 128 + B * (104 ld + 256 ceil(ld / 32) + 5,632) - per atom three [16] fp64 block rows, an ELL row of 32 values and
 * indices and the per-atom words; per 32-row slab one 16 x 16 partial sum; per graph the filter's coefficient table and the
 * 16 x 16 matrices.  0 if B * ceil(ld / 32), the number of workgroups of a launch, is beyond 2^22 (that bounds it below 2^39).
 *
 * The function enqueues a sequence of launches on `stream` (every dependency between phases is a launch boundary: no grid-wide
 * wait inside a kernel) and READS BACK a pair of words at most once per round of the component labelling ("did a label change")
 * and once per outer iteration ("graphs still running", "largest next filter degree"): it synchronises `stream` that often and
 * returns with all work enqueued but not necessarily finished.  It must not be called while `stream` is being captured.  The
 * graphs of one call are processed together: the slabs of all graphs form one grid, and a graph that is done makes its
 * workgroups return at once.
 *
 * SINGA_E_NULL for a null pointer; SINGA_E_SHAPE unless 1 <= kout <= 8, 2,049 <= ld <= 32,768 and the work size fits.  B <= 0
 * does nothing.  Not part of the emulation build. */
#ifndef SINGA_HIP_LAP_XL_H
#define SINGA_HIP_LAP_XL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
long long singa_lap_pe_xl_work(int B, int ld);
int singa_lap_pe_xl(const int32_t* esrc, const int32_t* edst, const int32_t* eptr, const int32_t* nnodes, const int32_t* first,
                    double* work, float* out, int32_t* status, int B, int ld, int kout, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_LAP_XL_H */
