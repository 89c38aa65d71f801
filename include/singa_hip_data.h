/* Batches from a packed dataset that is resident on the device (singa_amd/dataset.py: PackedDataset.to(device).batch(ids)).
 * NOT part of the drop-in training ABI (include/singa_hip.h): this entry point exists for the data path.  Conventions as in
 * singa_hip.h (device pointers unless stated, `stream`, SINGA_E_* return codes).
 *
 * THE STORE.  G graphs as flat arrays.  A ragged field is the concatenation over the graphs of its per-graph rows; the rows
 * a graph owns on an AXIS are given by that axis' offset table.  Seven axes:
 *     0 protein atoms   1 ligand atoms   2 pp edges   3 ll edges   4 lp edges   5 pl edges   6 the graph itself (one row)
 *   offsets  i64 [7][G + 1]   exclusive prefix sums of the per-graph counts; row 6 is 0, 1, ..., G
 *
 * THE CALL.  singa_collate_batch builds the PyG-style collation of graphs ids[0 .. B) (duplicates and any order allowed)
 * with two launches on `stream` and nothing else: no atomics, no host synchronisation, no allocation, a deterministic result.
 *   1. the plan kernel (one workgroup) writes  bases i64 [7][B + 1]: bases[a][b] = sum of the counts of axis a over slots
 *      < b.  Rows 0 and 1 are the `ptr` tensors of the two node types.  It writes status[0] = the number of ids outside
 *      [0, G) (0 = all fine); such an id is CLAMPED into the range wherever it is used, so no access leaves the store.
 *   2. the copy kernel moves every field.  A field's destination is the concatenation of its rows in slot order, so its
 *      destination is one flat run of `rows x width` items; each workgroup takes a chunk of that run and finds the slot of
 *      its first row by a search in the scanned bases it holds in LDS.  Only 4-byte alignment of sources, destinations and
 *      segments is assumed (a row of 59 floats is 236 bytes).
 *
 * A FIELD (singa_collate_field_t, a HOST array of n_fields <= SINGA_COLLATE_MAX_FIELDS):
 *   src, dst    device pointers, 4-byte aligned (dst of the widening kinds: 8-byte aligned); src is unused by kind 3
 *   axis        the axis whose rows it holds
 *   width       4-byte source words per row (>= 1)
 *   kind        0  SINGA_COLLATE_COPY32      dst[w] = src[w]                          32-bit words
 *               1  SINGA_COLLATE_WIDEN       dst[w] = (i64) src[w]                    i32 -> i64
 *               2  SINGA_COLLATE_WIDEN_BASE  dst[w] = (i64) src[w] + bases[base_axis][slot]   (edge_index rows: the node base
 *                                            of the source / destination node type of the slot the row belongs to)
 *               3  SINGA_COLLATE_SLOT        dst[w] = (i64) slot                      (the `batch` vector of a node type)
 *   base_axis   kind 2 only: 0 or 1
 *
 * totals (HOST, i64 [7]): the rows of every axis in this batch as the caller computed them from its host copy of the counts
 * (totals[6] = B); the destinations hold exactly totals[axis] x width items.  The kernels never write past them: should the
 * device's own scan disagree (an id that was clamped), rows beyond the device's total are left unwritten and rows beyond the
 * host's total are not written.  A field whose axis has no rows in this batch is skipped (its pointers may be null).
 *
 * Errors, all detected before any HIP call: SINGA_E_NULL for a null ids / offsets / bases / status / fields / totals or a null
 * src / dst of a field with rows; SINGA_E_SHAPE for B < 1, B > SINGA_COLLATE_MAX_B, G < 1, n_fields outside
 * [0, SINGA_COLLATE_MAX_FIELDS], an axis outside [0, 7), a width < 1, a kind outside [0, 4), a base_axis outside {0, 1}, a
 * misaligned pointer, totals[6] != B, a negative total, or a field of 2^31 or more items. */
#ifndef SINGA_HIP_DATA_H
#define SINGA_HIP_DATA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define SINGA_COLLATE_AXES 7
#define SINGA_COLLATE_MAX_FIELDS 32
#define SINGA_COLLATE_MAX_B 2048
#define SINGA_COLLATE_COPY32 0
#define SINGA_COLLATE_WIDEN 1
#define SINGA_COLLATE_WIDEN_BASE 2
#define SINGA_COLLATE_SLOT 3

typedef struct {
    const void* src;
    void* dst;
    int32_t axis, width, kind, base_axis;
} singa_collate_field_t;

int singa_collate_batch(const int32_t* ids, int B, int G, const int64_t* offsets, int64_t* bases, int32_t* status,
                        const singa_collate_field_t* fields, int n_fields, const int64_t* totals, void* stream);
#ifdef __cplusplus
}
#endif
#endif /* SINGA_HIP_DATA_H */
