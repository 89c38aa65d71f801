/* The kNN edge MLPs (k15c) once per UNDIRECTED edge.  NOT part of the drop-in training ABI (include/singa_hip.h): these entry
 * points exist for `ops.edge_mlp_pair(..., units=...)` of singa_amd/ops.py.  Conventions as in singa_hip.h (device pointers,
 * `stream`, SINGA_E_* return codes, nn.Linear's own parameter layouts).
 *
 * `KnnEdges` (singa_amd/model/CProMG.py) symmetrises the kNN list: a real edge (i -> j) has its mate (j -> i), and the two
 * carry the same attribute row bit for bit, so singa_edge_mlp_fwd computes every such row twice.  A UNIT is one undirected
 * edge: a row a of attr [E][64] and its mate b.  b == a is a row without a mate (a self loop, an inert padding edge).
 *   unit_a, unit_b  i32 [E]   the units come first, in any order; behind them a < 0 marks "no unit" down to the end of the
 *                             list.  Every row of [0, E) that is to be computed is named by exactly one unit, as its a or
 *                             as its b.  An entry that is no row of [0, E) is taken as "no unit" (a) or "no mate" (b): no
 *                             access leaves the arrays, whatever the list holds.
 * Forward: (wk [E][32], wv [E][64]) rows a and b of every unit = both nets on attr[a]; the two rows get the same registers, so
 * they are the bits singa_edge_mlp_fwd writes for row a.  Rows that no unit names are not written.
 * Backward, per net as singa_edge_mlp_bwd: the gradient row of a unit is g_out[a] + g_out[b] (b != a; added in f32), its
 * attribute row attr[a]; the four parameter gradients are summed over the units.  `part` has the layout and the
 * singa_edge_mlp_bwd_nparts(E, H) rows of singa_edge_mlp_bwd, and every row is written (zeros where a workgroup had no unit).
 * The kernels stop at the first 32-unit tile that holds no unit; nothing is read back.
 *
 * SINGA_E_NULL for a null pointer; SINGA_E_SHAPE unless CIN == 64, (HK, HV) == (32, 64) / H in {32, 64}, E >= 0 and attr, wk,
 * wv, g_out are 16-byte aligned.  E == 0 does nothing. */
#ifndef SINGA_HIP_UNITS_H
#define SINGA_HIP_UNITS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int singa_edge_mlp_units_fwd(const float* attr, const int32_t* unit_a, const int32_t* unit_b, const float* w1tk, const float* b1k,
                             const float* w2tk, const float* b2k, const float* w1tv, const float* b1v, const float* w2tv,
                             const float* b2v, float* wk, float* wv, int E, int CIN, int HK, int HV, void* stream);

int singa_edge_mlp_units_bwd(const float* attr, const int32_t* unit_a, const int32_t* unit_b, const float* g_out, const float* w1t,
                             const float* b1, const float* w2, float* part, int E, int CIN, int H, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_UNITS_H */
