// n2 for graphs of 2,049 .. 32,768 atoms (include/singa_hip_lap_xl.h): singa_lap_pe_large's encoding with MANY workgroups per
// graph.  A translation unit of its own, linked into libsinga_hip.so; it reports errors through the two hooks singa_hip.hip
// exports (hidden: not part of any ABI).
//
// Work split.  A graph of n atoms is cut into slabs of XL_SLAB = 32 consecutive atoms; a workgroup of 256 threads owns one slab,
// and the slabs of all graphs of a call form one grid (ceil(ld / 32) workgroups per graph: a workgroup past its graph's last
// atom, or of a graph that is done, returns at once).  Every dependency between phases is a LAUNCH BOUNDARY - there is no
// grid-wide wait inside any kernel - so the host function enqueues a sequence of small launches and reads two words back per
// round of the component labelling and per outer iteration.  All per-atom state lives in `work`, indexed by atom; LDS holds a
// slab's two [32][16] tiles and 16 x 16 matrices, whatever n is.  What one workgroup per graph decides (the Cholesky factor, the
// rotations, convergence, the next filter) is a kernel on a grid of B small workgroups, and it leaves its answer in the graph's
// record in `work`, where the slab kernels of the next launch read it: no step of the iteration needs a value from the host.
//
// Phases (xl_*_kernel, in launch order):
//   init, edges, merge, values   ELL rows (<= 32 off-diagonal neighbours, sorted by atom, + the diagonal) from the edge list, as
//                                in lap_pe_large_kernel: a thread per edge drops tagged entries into both end points' raw rows
//                                (one integer counter per atom is the only atomic), a thread per atom merges them.
//   cc (one launch per round)    component labels: every atom takes the minimum label around it, hooks its old parent to it
//                                and jumps up to 8 pointers; rounds until one changes nothing (<= XL_CC_CAP).
//   null_check, null_rank, null_fill   the zero eigenvalue's vectors, written per component and checked against their rows;
//                                c >= m = kout + 1 of them end the graph here.
//   zdot, coef, gram<0>, chol, solve   X <- X R^-1 (twice: CholQR2), the block first projected against the c null vectors.
//   gram<1>, rr, rotate, decide  Rayleigh-Ritz: W = L X, H = sym(X^T W), Jacobi, X <- X Q, W <- W Q, residual norms; converged,
//                                given up, or the next filter's interval, degree and three-term coefficients.
//   filter (one launch per Chebyshev degree)   the hot kernel: N = f1 (L X - c X) - f2 Y on the three blocks.
//   emit_part, emit_sign, emit_write   sign convention and the fp32 rows of `out`, behind the last status check.
//
// The filter.  Sixteen consecutive lanes own the 16 columns of one row, a wavefront four rows: a neighbour's row of X is one
// contiguous 128-byte read, and the ELL index and value of a step are one broadcast read per row.  The indices are NOT staged in
// LDS: a launch is one filter step, LDS does not outlive it, and within a step every index is read exactly once - staging would
// only add a copy.  They come from L2 (an 8,192-atom graph's ELL rows are 3 MB, its three blocks 3 MB).
//
// Sums over atoms are per-slab partials in a fixed order, one per workgroup in `work`, finished by one workgroup in a fixed
// order: no floating-point atomics, the same bits run to run.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/singa_hip.h"
#include "../../include/singa_hip_lap_xl.h"

int singa_detail_fail(int code, const char* msg);
int singa_detail_check_launch(const char* what);

#ifndef SINGA_EMUL      // (many launches with device-side state: not part of the sequential CPU emulation build of tests/emul)
namespace {

constexpr int XL_MINN = 2049, XL_MAXN = 32768;   // atoms per graph this route takes
constexpr int XL_PB = 16, XL_W = 32, XL_RAW = 64, XL_SLAB = 32, XL_THREADS = 256;
constexpr int XL_CC_CAP = 64;                    // rounds of component labelling (a shuffled 32,768-atom path takes 10)
// The filter of an outer iteration: interval [theta_16, 2], the largest degree that amplifies the lowest Ritz value by at most
// XL_AMPLIFY against the interval, log(2 XL_AMPLIFY) / acosh(t(theta_1)), clamped to XL_DEG_MIN .. XL_DEG_MAX.  The cap on the
// amplification keeps CholQR2 inside fp64: pure paths of 2,049 / 8,192 atoms in fp64 numpy converge in 7 outer iterations and
// 1,377 / 4,120 products with Gram condition numbers up to 9e7; an amplification of 1e6 takes them to 4e11.
constexpr double XL_AMPLIFY = 1e4;
constexpr int XL_DEG_MIN = 24, XL_DEG_MAX = 2048;
constexpr int XL_MAXIT = 40;                     // outer iterations
constexpr double XL_RESIDUAL = 2e-10;
// doubles of `work`: per atom of ld (ints count half), per slab, per graph (coefficient table + record), in front of all graphs
constexpr int XL_PER_LD = 3 * XL_PB + XL_W + 4 + (XL_W + 8) / 2;
constexpr int XL_PER_SLAB = 256;
constexpr int XL_TAB = 2 * XL_DEG_MAX, XL_REC = 1536, XL_PER_GRAPH = XL_TAB + XL_REC;
constexpr int XL_HOST = 128;                     // 256 ints: [round] a label changed; [64 + 2 it] graphs running, [65 + 2 it] degree
static_assert(XL_PER_LD == 104 && XL_PER_GRAPH == 5632, "singa_lap_pe_xl_work and the header state these");
static_assert(XL_CC_CAP <= 64 && 64 + 2 * XL_MAXIT <= 2 * XL_HOST, "the host record's slots");
// a graph's state word: 0 running, 1 .. 6 the status it ends with, 7 its answer stands in the current block, 8 no atoms
constexpr int XL_DONE = 7, XL_EMPTY = 8;
// record, in doubles: H | Q (Cholesky factor / rotations) | Q sorted | coef [8][16] | theta | resn | sign | misc | ints
constexpr int XL_R_H = 0, XL_R_Q = 256, XL_R_QS = 512, XL_R_COEF = 768, XL_R_THETA = 896, XL_R_RESN = 912, XL_R_SIGN = 928,
              XL_R_MISC = 936, XL_R_CTRL = 1024;
// ints of the record: state, last round that changed a label, null vectors, current block, filter degree, current block at the
// filter's start
constexpr int XL_C_STATE = 0, XL_C_ROUND = 1, XL_C_NULL = 2, XL_C_ROT = 3, XL_C_DEG = 4, XL_C_ROTF = 5;

struct XlGraph {
    double* blk0;        // three [ld][16] blocks of the recurrence, rotated by index
    long long bstride;
    __device__ __forceinline__ double* blk(int i) const { return blk0 + i * bstride; }     // (arithmetic, not a table: no scratch)
    double *ell_v, *diag, *dinv, *zn, *part, *tab, *rec;
    int *ell_i, *ell_n, *cnt, *label, *zr, *degsum, *dclip, *selfl, *raw, *ctrl;
};

__device__ __forceinline__ XlGraph xl_graph(double* work, int g, int ld, int spg) {
    XlGraph G;
    double* base = work + XL_HOST + (long long)g * ((long long)XL_PER_LD * ld + (long long)XL_PER_SLAB * spg + XL_PER_GRAPH);
    G.blk0 = base, G.bstride = (long long)XL_PB * ld;
    G.ell_v = base + (long long)3 * XL_PB * ld;
    G.diag = G.ell_v + (long long)XL_W * ld;
    G.dinv = G.diag + ld;
    G.zn = G.dinv + ld;
    G.ell_i = reinterpret_cast<int*>(G.zn + 2 * (long long)ld);
    G.ell_n = G.ell_i + (long long)XL_W * ld;
    G.cnt = G.ell_n + ld;
    G.label = G.cnt + ld;
    G.zr = G.label + ld;
    G.degsum = G.zr + ld;
    G.dclip = G.degsum + ld;
    G.selfl = G.dclip + ld;
    G.part = base + (long long)XL_PER_LD * ld;
    G.tab = G.part + (long long)XL_PER_SLAB * spg;
    G.rec = G.tab + XL_TAB;
    G.ctrl = reinterpret_cast<int*>(G.rec + XL_R_CTRL);
    G.raw = reinterpret_cast<int*>(G.blk(1));            // [n][RAW] atom | direction << 16, over blocks 1 and 2 (dead before they are used)
    return G;
}

// what atomics wrote (labels, degree sums) is read back at device scope, past the vector cache
__device__ __forceinline__ int xl_aload(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// entry k of the answer at atom i: null vector k while k < c, then the Ritz vectors in ascending order
__device__ __forceinline__ double xl_answer(const XlGraph& G, const double* X, int c, int i, int k) {
    return k < c ? (G.zr[i] == k ? G.zn[i] : 0.0) : X[(long long)i * XL_PB + k - c];
}

// sum over the slabs' partials, entry tid of each, four interleaved chains added in a fixed order
__device__ __forceinline__ double xl_sum_parts(const double* part, int nslab, int tid) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int w = 0;
    for (; w + 3 < nslab; w += 4) {
        a0 += part[(long long)w * XL_PER_SLAB + tid];
        a1 += part[(long long)(w + 1) * XL_PER_SLAB + tid];
        a2 += part[(long long)(w + 2) * XL_PER_SLAB + tid];
        a3 += part[(long long)(w + 3) * XL_PER_SLAB + tid];
    }
    for (; w < nslab; ++w) a0 += part[(long long)w * XL_PER_SLAB + tid];
    return (a0 + a1) + (a2 + a3);
}

#define XL_SLAB_HEAD                                                                      \
    const int g = blockIdx.x / spg, row0 = (blockIdx.x % spg) * XL_SLAB, tid = threadIdx.x; \
    const int n = nnodes[g];                                                              \
    if (n < XL_MINN || n > ld || n > XL_MAXN || row0 >= n) return;                        \
    const XlGraph G = xl_graph(work, g, ld, spg);

// ---- ELL rows
__global__ void __launch_bounds__(XL_THREADS) xl_init_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    const int g = blockIdx.x / spg, row0 = (blockIdx.x % spg) * XL_SLAB, tid = threadIdx.x;
    if (blockIdx.x == 0) reinterpret_cast<int*>(work)[tid] = 0;          // the host record (2 XL_HOST == XL_THREADS ints)
    const int n = nnodes[g];
    const bool valid = n >= XL_MINN && n <= ld && n <= XL_MAXN;
    const XlGraph G = xl_graph(work, g, ld, spg);
    if (row0 == 0 && tid < 16) G.ctrl[tid] = tid == XL_C_STATE ? (n <= 0 ? XL_EMPTY : valid ? 0 : 6) : 0;
    if (row0 == 0 && tid == 16) G.rec[XL_R_MISC] = 0.0;
    if (!valid) return;
    const int i = row0 + tid;
    if (tid < XL_SLAB && i < n) G.cnt[i] = 0, G.label[i] = i, G.degsum[i] = 0;
}

__global__ void __launch_bounds__(XL_THREADS) xl_edges_kernel(const int* __restrict__ esrc, const int* __restrict__ edst,
                                                              const int* __restrict__ eptr, const int* __restrict__ nnodes,
                                                              double* work, int B, int ld, int spg) {
    const long long e0 = eptr[0], e1 = eptr[B];
    for (long long e = e0 + (long long)blockIdx.x * XL_THREADS + threadIdx.x; e < e1; e += (long long)gridDim.x * XL_THREADS) {
        int lo = 0, hi = B;                              // the graph that owns edge e: the last one with eptr[g] <= e
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (eptr[mid] <= e) lo = mid; else hi = mid;
        }
        const int n = nnodes[lo];
        if (n < XL_MINN || n > ld || n > XL_MAXN) continue;
        const XlGraph G = xl_graph(work, lo, ld, spg);
        const int a = esrc[e], b = edst[e];
        if ((unsigned)a >= (unsigned)n || (unsigned)b >= (unsigned)n) { atomicMax(&G.ctrl[XL_C_STATE], 5); continue; }
        const int sa = atomicAdd(&G.cnt[a], 1);
        if (sa < XL_RAW) G.raw[(long long)a * XL_RAW + sa] = b | (1 << 16);          // a -> b seen from a
        const int sb = atomicAdd(&G.cnt[b], 1);
        if (sb < XL_RAW) G.raw[(long long)b * XL_RAW + sb] = a | (2 << 16);          // a -> b seen from b: counts into b's in-degree
    }
}

__global__ void __launch_bounds__(XL_THREADS) xl_merge_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0) return;
    const int i = row0 + tid;
    if (tid >= XL_SLAB || i >= n) return;
    int* row = G.ell_i + (long long)i * XL_W;
    const int c = G.cnt[i];
    int nn = 0, self = 0, over = c > XL_RAW;
    for (int s = 0; s < c && s < XL_RAW; ++s) {
        const int ent = G.raw[(long long)i * XL_RAW + s], j = ent & 0xFFFF, f = ent >> 16;
        if (j == i) { self |= f; continue; }
        int p = 0;
        while (p < nn && (row[p] & 0xFFFF) < j) ++p;
        if (p < nn && (row[p] & 0xFFFF) == j) row[p] |= f << 16;
        else if (nn < XL_W) {
            for (int q = nn; q > p; --q) row[q] = row[q - 1];
            row[p] = ent;
            ++nn;
        } else over = 1;
    }
    int indeg = (self >> 1) & 1;
    for (int p = 0; p < nn; ++p) indeg += (row[p] >> 17) & 1;
    const int d = indeg < 1 ? 1 : indeg;
    G.ell_n[i] = nn, G.selfl[i] = self != 0, G.dclip[i] = d;
    G.dinv[i] = 1.0 / sqrt((double)d);
    if (over) atomicMax(&G.ctrl[XL_C_STATE], 1);
}

__global__ void __launch_bounds__(XL_THREADS) xl_values_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0) return;
    const int i = row0 + (tid >> 3), sub = tid & 7;      // eight lanes per atom
    if (i >= n) return;
    int* row = G.ell_i + (long long)i * XL_W;
    const double di = G.dinv[i];
    const int nn = G.ell_n[i];
    for (int p = sub; p < nn; p += 8) {
        const int ent = row[p], j = ent & 0xFFFF;
        G.ell_v[(long long)i * XL_W + p] = -0.5 * di * G.dinv[j] * (double)(((ent >> 16) & 1) + ((ent >> 17) & 1));
        row[p] = j;
    }
    if (sub == 0) G.diag[i] = 1.0 - (G.selfl[i] ? di * di : 0.0);
}

// ---- connected components: one round.  Labels are atoms of the same component and only ever decrease, so a round in which no
// thread lowers one leaves every component on its smallest atom.
__global__ void __launch_bounds__(XL_THREADS) xl_cc_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg, int round) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0) return;
    const int i = row0 + tid;
    if (tid >= XL_SLAB || i >= n) return;
    const int l0 = xl_aload(&G.label[i]), nn = G.ell_n[i];
    int l = l0;
    for (int p = 0; p < nn; ++p) {
        const int lj = xl_aload(&G.label[G.ell_i[(long long)i * XL_W + p]]);
        l = lj < l ? lj : l;
    }
    if (l < l0) atomicMin(&G.label[l0], l);              // hook the old parent
    for (int h = 0; h < 8; ++h) {                        // pointer jumping
        const int l2 = xl_aload(&G.label[l]);
        if (l2 >= l) break;
        l = l2;
    }
    if (l < l0) {
        atomicMin(&G.label[i], l);
        G.ctrl[XL_C_ROUND] = round + 1;
        reinterpret_cast<int*>(work)[round] = 1;
    }
}

// ---- the null vectors: sqrt(d_i) / sqrt(sum d) per component with an edge, each checked against its own rows
__global__ void __launch_bounds__(XL_THREADS) xl_null_check_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0) return;
    const int i = row0 + tid;
    if (tid >= XL_SLAB || i >= n) return;
    const int nn = G.ell_n[i];
    double r = G.diag[i] * sqrt((double)G.dclip[i]);
    for (int p = 0; p < nn; ++p) r += G.ell_v[(long long)i * XL_W + p] * sqrt((double)G.dclip[G.ell_i[(long long)i * XL_W + p]]);
    if (nn == 0 && !G.selfl[i]) return;                  // an atom without any edge: eigenvalue 1, no null vector
    if (!(fabs(r) <= 1e-12)) atomicMax(&G.ctrl[XL_C_STATE], 4);
    atomicAdd(&G.degsum[G.label[i]], G.dclip[i]);
}

// one wavefront per graph: rank of every null-carrying component, in order of its smallest atom; c >= m of them are the answer
__global__ void __launch_bounds__(64) xl_null_rank_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg, int kout) {
    const int g = blockIdx.x, lane = threadIdx.x;
    const int n = nnodes[g];
    if (n < XL_MINN || n > ld || n > XL_MAXN) return;
    const XlGraph G = xl_graph(work, g, ld, spg);
    if (G.ctrl[XL_C_STATE] != 0) return;
    if (G.ctrl[XL_C_ROUND] >= XL_CC_CAP) {               // the last round allowed still changed a label
        if (lane == 0) G.ctrl[XL_C_STATE] = 3;
        return;
    }
    int seen = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const bool root = i < n && G.label[i] == i && G.degsum[i] > 0;
        const unsigned long long mask = __ballot(root);
        if (i < n) G.zr[i] = root ? seen + __popcll(mask & ((1ull << lane) - 1ull)) : -1;
        seen += __popcll(mask);
    }
    if (lane == 0) {
        G.ctrl[XL_C_NULL] = seen;
        if (seen >= kout + 1) G.ctrl[XL_C_STATE] = XL_DONE;
    }
}

// per atom: its entry of its component's null vector and the component's rank; the start block (deterministic pseudo-random)
__global__ void __launch_bounds__(XL_THREADS) xl_null_fill_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    const int state = G.ctrl[XL_C_STATE];
    if (state != 0 && state != XL_DONE) return;
    const int i = row0 + tid;
    if (tid < XL_SLAB && i < n) {
        const int l = G.label[i], s = G.degsum[l];
        G.zn[i] = s > 0 ? sqrt((double)G.dclip[i] / (double)s) : 0.0;
        if (l != i) G.zr[i] = G.zr[l];                   // (roots hold their own rank: no atom reads a slot another one writes)
    }
    if (state != 0) return;
    for (int e = tid; e < XL_SLAB * XL_PB; e += XL_THREADS) {
        const int r = row0 + (e >> 4), j = e & 15;
        if (r >= n) break;
        unsigned h = (unsigned)(r * 2654435761u) ^ (unsigned)((j + 11) * 40503u * 2246822519u);
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
        G.blk(0)[(long long)r * XL_PB + j] = (double)(h & 0xFFFFFF) / 8388608.0 - 1.0;
    }
}

// ---- X <- X R^-1.  zdot: the slab's part of Z^T X over the c null vectors (supports are disjoint, so they are orthonormal as
// they stand); coef: the sum; gram<0>: X <- X - Z coef, then the slab's part of X^T X
__global__ void __launch_bounds__(XL_THREADS) xl_zdot_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0 || G.ctrl[XL_C_NULL] == 0) return;
    __shared__ double red[XL_THREADS];
    const double* X = G.blk(G.ctrl[XL_C_ROT]);
    const int j = tid & 15, a = (tid >> 4) & 7, half = tid >> 7;
    double acc = 0.0;
    for (int rr = 0; rr < 16; ++rr) {
        const int r = row0 + half * 16 + rr;
        if (r < n && G.zr[r] == a) acc += G.zn[r] * X[(long long)r * XL_PB + j];
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < 128) G.part[(long long)(blockIdx.x % spg) * XL_PER_SLAB + tid] = red[tid] + red[128 + tid];
}

__global__ void __launch_bounds__(128) xl_coef_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n = nnodes[g];
    if (n < XL_MINN || n > ld || n > XL_MAXN) return;
    const XlGraph G = xl_graph(work, g, ld, spg);
    if (G.ctrl[XL_C_STATE] != 0 || G.ctrl[XL_C_NULL] == 0) return;
    G.rec[XL_R_COEF + tid] = xl_sum_parts(G.part, (n + XL_SLAB - 1) / XL_SLAB, tid);
}

// MODE 0: project, A = B = X.  MODE 1: W = L X into the next block, A = X, B = W.  part[slab] = A^T B over the slab's rows
template <int MODE>
__global__ void __launch_bounds__(XL_THREADS) xl_gram_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0) return;
    __shared__ double As[XL_SLAB][XL_PB], Bs[XL_SLAB][XL_PB];
    const int rot = G.ctrl[XL_C_ROT], c = G.ctrl[XL_C_NULL];
    double* X = G.blk(rot);
    double* Wg = G.blk((rot + 1) % 3);
    const int j = tid & 15;
    for (int pass = 0; pass < 2; ++pass) {
        const int rl = pass * 16 + (tid >> 4), r = row0 + rl;
        double x = 0.0, w = 0.0;
        if (r < n) {
            x = X[(long long)r * XL_PB + j];
            if (MODE == 0) {
                const int a = G.zr[r];
                if (c > 0 && a >= 0) {
                    x -= G.zn[r] * G.rec[XL_R_COEF + a * 16 + j];
                    X[(long long)r * XL_PB + j] = x;
                }
                w = x;
            } else {
                const int nn = G.ell_n[r];
                const double* ev = G.ell_v + (long long)r * XL_W;
                const int* ei = G.ell_i + (long long)r * XL_W;
                w = G.diag[r] * x;
                for (int p = 0; p < nn; ++p) w += ev[p] * X[(long long)ei[p] * XL_PB + j];
                Wg[(long long)r * XL_PB + j] = w;
            }
        }
        As[rl][j] = x, Bs[rl][j] = w;
    }
    __syncthreads();
    const int a = tid >> 4;
    double acc = 0.0;
#pragma unroll 8
    for (int r = 0; r < XL_SLAB; ++r) acc += As[r][a] * Bs[r][j];
    G.part[(long long)(blockIdx.x % spg) * XL_PER_SLAB + tid] = acc;
}

#define XL_GRAPH_HEAD                                                       \
    const int g = blockIdx.x, tid = threadIdx.x;                            \
    const int n = nnodes[g];                                                \
    if (n < XL_MINN || n > ld || n > XL_MAXN) return;                       \
    const XlGraph G = xl_graph(work, g, ld, spg);                           \
    if (G.ctrl[XL_C_STATE] != 0) return;                                    \
    const int nslab = (n + XL_SLAB - 1) / XL_SLAB;

// H = sym(sum of the partials), in LDS
__device__ __forceinline__ void xl_sym_sum(const XlGraph& G, int nslab, int tid, double* H, double* T) {
    T[tid] = xl_sum_parts(G.part, nslab, tid);
    __syncthreads();
    H[tid] = 0.5 * (T[tid] + T[(tid & 15) * 16 + (tid >> 4)]);
    __syncthreads();
}

// the Cholesky factor R of the Gram matrix (G = R^T R), lap_fsi_iterate's pivot rule; a vanishing pivot ends the graph
__global__ void __launch_bounds__(XL_THREADS) xl_chol_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_GRAPH_HEAD
    __shared__ double H[256], Q[256];
    xl_sym_sum(G, nslab, tid, H, Q);
    if (tid == 0) {
        int bad = 0;
        double tr = 0.0;
        for (int j = 0; j < XL_PB; ++j) tr += H[j * 16 + j];
        for (int j = 0; j < XL_PB; ++j) {
            double d = H[j * 16 + j];
            for (int k = 0; k < j; ++k) d -= Q[k * 16 + j] * Q[k * 16 + j];
            if (!(d > 1e-26 * tr)) { bad = 1; d = 1.0; }
            const double rj = sqrt(d);
            Q[j * 16 + j] = rj;
            for (int i = j + 1; i < XL_PB; ++i) {
                double v = H[j * 16 + i];
                for (int k = 0; k < j; ++k) v -= Q[k * 16 + j] * Q[k * 16 + i];
                Q[j * 16 + i] = v / rj;
            }
            for (int i = 0; i < j; ++i) Q[j * 16 + i] = 0.0;
        }
        if (bad) G.ctrl[XL_C_STATE] = 2;
    }
    __syncthreads();
    G.rec[XL_R_Q + tid] = Q[tid];
}

// a row of X solved in place (y R = x) by its sixteen lanes
__global__ void __launch_bounds__(XL_THREADS) xl_solve_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0) return;
    __shared__ double R[256];
    R[tid] = G.rec[XL_R_Q + tid];
    __syncthreads();
    double* X = G.blk(G.ctrl[XL_C_ROT]);
    const int j = tid & 15;
    for (int pass = 0; pass < 2; ++pass) {
        const int r = row0 + pass * 16 + (tid >> 4);
        double x = r < n ? X[(long long)r * XL_PB + j] : 0.0;
#pragma unroll
        for (int i = 0; i < XL_PB; ++i) {
            const double yi = __shfl(x, i, 16) / R[i * 16 + i];
            if (j == i) x = yi;
            else if (j > i) x -= yi * R[i * 16 + j];
        }
        if (r < n) X[(long long)r * XL_PB + j] = x;
    }
}

__device__ __forceinline__ void xl_rotation(double hpp, double hqq, double hpq, double& c, double& sn) {
    c = 1.0, sn = 0.0;
    if (fabs(hpq) > 1e-300) {
        const double tau = (hqq - hpp) / (2.0 * hpq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        c = 1.0 / sqrt(1.0 + t * t);
        sn = t * c;
    }
}

// ---- Rayleigh-Ritz on the projected matrix: cyclic Jacobi (round-robin ordering: 8 disjoint pairs per step, 8 lanes per pair),
// Ritz values ascending (stable), the rotations' columns in that order
__global__ void __launch_bounds__(XL_THREADS) xl_rr_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_GRAPH_HEAD
    __shared__ double H[256], Q[256], so[16], sd[16];
    __shared__ int ord[16];
    xl_sym_sum(G, nslab, tid, H, Q);
    Q[tid] = (tid >> 4) == (tid & 15) ? 1.0 : 0.0;
    __syncthreads();
    for (int sweep = 0; sweep < 10; ++sweep) {
        if (tid < 16) {
            double o = 0.0;
            for (int b = 0; b < 16; ++b)
                if (b != tid) o += H[tid * 16 + b] * H[tid * 16 + b];
            so[tid] = o, sd[tid] = H[tid * 17] * H[tid * 17];
        }
        __syncthreads();
        double off2 = 0.0, dg2 = 0.0;
        for (int b = 0; b < 16; ++b) off2 += so[b], dg2 += sd[b];
        __syncthreads();
        if (off2 <= 1e-30 * (dg2 + 1e-300)) break;
        for (int st = 0; st < 15; ++st) {
            const int pr = tid >> 3, sub = tid & 7;
            const int p = pr == 0 ? 15 : (st + pr) % 15, q = pr == 0 ? st : (st + 15 - pr) % 15;
            double c = 1.0, sn = 0.0;
            if (tid < 64) xl_rotation(H[p * 16 + p], H[q * 16 + q], H[p * 16 + q], c, sn);
            __syncthreads();
            if (tid < 64) {
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const int i = sub + 8 * h2;
                    const double aip = H[i * 16 + p], aiq = H[i * 16 + q];
                    H[i * 16 + p] = c * aip - sn * aiq;
                    H[i * 16 + q] = sn * aip + c * aiq;
                    const double qip = Q[i * 16 + p], qiq = Q[i * 16 + q];
                    Q[i * 16 + p] = c * qip - sn * qiq;
                    Q[i * 16 + q] = sn * qip + c * qiq;
                }
            }
            __syncthreads();
            if (tid < 64) {
#pragma unroll
                for (int h2 = 0; h2 < 2; ++h2) {
                    const int i = sub + 8 * h2;
                    const double api = H[p * 16 + i], aqi = H[q * 16 + i];
                    H[p * 16 + i] = c * api - sn * aqi;
                    H[q * 16 + i] = sn * api + c * aqi;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        for (int a = 0; a < XL_PB; ++a) {
            int b = a;
            while (b > 0 && H[ord[b - 1] * 17] > H[a * 17]) { ord[b] = ord[b - 1]; --b; }
            ord[b] = a;
        }
    }
    __syncthreads();
    if (tid < XL_PB) G.rec[XL_R_THETA + tid] = H[ord[tid] * 17];
    G.rec[XL_R_QS + tid] = Q[(tid >> 4) * 16 + ord[tid & 15]];
}

// X <- X Q, W <- W Q by a row's sixteen lanes; the slab's part of the squared residual norms |W - X theta| per column
__global__ void __launch_bounds__(XL_THREADS) xl_rotate_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0) return;
    __shared__ double Qs[256], red[XL_SLAB][XL_PB];
    Qs[tid] = G.rec[XL_R_QS + tid];
    __syncthreads();
    const int rot = G.ctrl[XL_C_ROT], j = tid & 15;
    double* X = G.blk(rot);
    double* Wg = G.blk((rot + 1) % 3);
    const double th = G.rec[XL_R_THETA + j];
    for (int pass = 0; pass < 2; ++pass) {
        const int rl = pass * 16 + (tid >> 4), r = row0 + rl;
        const double x = r < n ? X[(long long)r * XL_PB + j] : 0.0, w = r < n ? Wg[(long long)r * XL_PB + j] : 0.0;
        double xs = 0.0, ws = 0.0;
#pragma unroll
        for (int i = 0; i < XL_PB; ++i) {
            const double q = Qs[i * 16 + j];
            xs += __shfl(x, i, 16) * q;
            ws += __shfl(w, i, 16) * q;
        }
        if (r < n) X[(long long)r * XL_PB + j] = xs, Wg[(long long)r * XL_PB + j] = ws;
        const double d = ws - th * xs;
        red[rl][j] = d * d;
    }
    __syncthreads();
    if (tid < XL_PB) {
        double s = 0.0;
        for (int r = 0; r < XL_SLAB; ++r) s += red[r][tid];
        G.part[(long long)(blockIdx.x % spg) * XL_PER_SLAB + tid] = s;
    }
}

// residual norms of the lowest m - c pairs; converged, given up, or the next filter: interval, degree, Zhou & Saad's scaled
// three-term coefficients for every step, and the block the filter starts from
__global__ void __launch_bounds__(64) xl_decide_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg, int kout, int it) {
    XL_GRAPH_HEAD
    __shared__ double resn[XL_PB];
    if (tid < XL_PB) {
        double s = 0.0;
        for (int w = 0; w < nslab; ++w) s += G.part[(long long)w * XL_PER_SLAB + tid];
        resn[tid] = sqrt(s);
        G.rec[XL_R_RESN + tid] = resn[tid];
    }
    __syncthreads();
    if (tid != 0) return;
    const int want = kout + 1 - G.ctrl[XL_C_NULL];
    double worst = 0.0;
    for (int j = 0; j < want; ++j) worst = fmax(worst, resn[j]);
    if (worst <= XL_RESIDUAL) { G.ctrl[XL_C_STATE] = XL_DONE; return; }
    const double prev = G.rec[XL_R_MISC];
    // no iteration left, or a residual that falls too slowly to get there in the iterations left
    if (it >= XL_MAXIT - 1 || (it >= 3 && (worst >= prev || log(XL_RESIDUAL / worst) / log(worst / prev) > (double)(XL_MAXIT - 1 - it)))) {
        G.ctrl[XL_C_STATE] = 3;
        return;
    }
    G.rec[XL_R_MISC] = worst;
    const double a0 = G.rec[XL_R_THETA], a = G.rec[XL_R_THETA + XL_PB - 1], b = 2.0 + 1e-9;
    if (!(a > a0) || !(a < b - 1e-3)) { G.ctrl[XL_C_STATE] = 3; return; }
    const double e = 0.5 * (b - a), c = 0.5 * (b + a);
    const double dg = ceil(log(2.0 * XL_AMPLIFY) / acosh((c - a0) / e));
    const int deg = !(dg > XL_DEG_MIN) ? XL_DEG_MIN : dg > XL_DEG_MAX ? XL_DEG_MAX : (int)dg;
    double sigma = e / (a0 - c);
    const double sigma1 = sigma;
    G.tab[0] = sigma1 / e, G.tab[1] = 0.0;
    for (int i = 2; i <= deg; ++i) {
        const double sigma2 = 1.0 / (2.0 / sigma1 - sigma);
        G.tab[2 * (i - 1)] = 2.0 * sigma2 / e, G.tab[2 * (i - 1) + 1] = sigma * sigma2;
        sigma = sigma2;
    }
    G.rec[XL_R_MISC + 1] = c;
    const int rot = G.ctrl[XL_C_ROT];
    G.ctrl[XL_C_DEG] = deg, G.ctrl[XL_C_ROTF] = rot, G.ctrl[XL_C_ROT] = (rot + deg) % 3;
    int* host = reinterpret_cast<int*>(work);
    atomicAdd(&host[64 + 2 * it], 1);
    atomicMax(&host[65 + 2 * it], deg);
}

// ---- the filter, step `step` (1-based) of the graph's degree: N = f1 (L X - c X) - f2 Y
__global__ void __launch_bounds__(XL_THREADS) xl_filter_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg, int step) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != 0 || step > G.ctrl[XL_C_DEG]) return;
    const int rf = G.ctrl[XL_C_ROTF];
    const double* __restrict__ X = G.blk((rf + step - 1) % 3);
    const double* __restrict__ Y = G.blk((rf + step + 1) % 3);
    double* __restrict__ N = G.blk((rf + step) % 3);
    const double f1 = G.tab[2 * (step - 1)], f2 = G.tab[2 * (step - 1) + 1], c = G.rec[XL_R_MISC + 1];
    const int j = tid & 15;
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
        const int r = row0 + pass * 16 + (tid >> 4);
        if (r >= n) break;
        const int nn = G.ell_n[r];
        const double* __restrict__ ev = G.ell_v + (long long)r * XL_W;
        const int* __restrict__ ei = G.ell_i + (long long)r * XL_W;
        double acc = (G.diag[r] - c) * X[(long long)r * XL_PB + j];
        for (int p = 0; p < nn; ++p) acc += ev[p] * X[(long long)ei[p] * XL_PB + j];
        acc *= f1;
        if (step > 1) acc -= f2 * Y[(long long)r * XL_PB + j];     // (step 1 has no previous block: Y is not read)
        N[(long long)r * XL_PB + j] = acc;
    }
}

// ---- the finish: per column the entry of largest magnitude (lowest atom on ties) made positive
__global__ void __launch_bounds__(XL_THREADS) xl_emit_part_kernel(const int* __restrict__ nnodes, double* work, int ld, int spg, int kout) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != XL_DONE || tid >= kout) return;
    const double* X = G.blk(G.ctrl[XL_C_ROT]);
    const int c = G.ctrl[XL_C_NULL];
    double best = -1.0;
    int bi = 0;
    for (int i = row0; i < n && i < row0 + XL_SLAB; ++i) {
        const double v = fabs(xl_answer(G, X, c, i, tid + 1));
        if (v > best) best = v, bi = i;
    }
    double* p = G.part + (long long)(blockIdx.x % spg) * XL_PER_SLAB;
    p[tid] = best, p[8 + tid] = (double)bi;
}

// one small workgroup per graph: the columns' signs, and the graph's status - the last check in front of `out`
__global__ void __launch_bounds__(64) xl_emit_sign_kernel(const int* __restrict__ nnodes, double* work, int* status, int ld, int spg, int kout) {
    const int g = blockIdx.x, tid = threadIdx.x;
    const int n = nnodes[g];
    const XlGraph G = xl_graph(work, g, ld, spg);
    const int state = G.ctrl[XL_C_STATE];
    if (tid == 0) status[g] = state == XL_DONE || state == XL_EMPTY ? 0 : state == 0 ? 3 : state;
    if (state != XL_DONE || tid >= kout) return;
    const int nslab = (n + XL_SLAB - 1) / XL_SLAB;
    double best = -1.0;
    int bi = 0;
    for (int w = 0; w < nslab; ++w) {
        const double* p = G.part + (long long)w * XL_PER_SLAB;
        if (p[tid] > best) best = p[tid], bi = (int)p[8 + tid];
    }
    G.rec[XL_R_SIGN + tid] = xl_answer(G, G.blk(G.ctrl[XL_C_ROT]), G.ctrl[XL_C_NULL], bi, tid + 1) < 0.0 ? -1.0 : 1.0;
}

__global__ void __launch_bounds__(XL_THREADS) xl_emit_write_kernel(const int* __restrict__ nnodes, const int* __restrict__ first,
                                                                   double* work, float* out, int ld, int spg, int kout) {
    XL_SLAB_HEAD
    if (G.ctrl[XL_C_STATE] != XL_DONE) return;
    const int i = row0 + (tid >> 3), col = tid & 7;
    if (i >= n || col >= kout) return;
    const double v = xl_answer(G, G.blk(G.ctrl[XL_C_ROT]), G.ctrl[XL_C_NULL], i, col + 1);
    out[((long long)first[g] + i) * kout + col] = (float)(G.rec[XL_R_SIGN + col] * v);
}

}  // namespace
#endif  // SINGA_EMUL

extern "C" long long singa_lap_pe_xl_work(int B, int ld) {
    if (B <= 0) return 0;
    if (ld < 2049 || ld > 32768) return 0;
    const long long spg = (ld + 31) / 32;
    if ((long long)B * spg > (1ll << 22)) return 0;
    return 128 + (long long)B * (104ll * ld + 256 * spg + 5632);
}

extern "C" int singa_lap_pe_xl(const int32_t* esrc, const int32_t* edst, const int32_t* eptr, const int32_t* nnodes, const int32_t* first,
                               double* work, float* out, int32_t* status, int B, int ld, int kout, void* stream) {
    if (!esrc || !edst || !eptr || !nnodes || !first || !work || !out || !status) return singa_detail_fail(SINGA_E_NULL, "lap_pe_xl: null pointer");
    if (kout < 1 || kout > 8) return singa_detail_fail(SINGA_E_SHAPE, "lap_pe_xl: 1..8 eigenvectors");
    if (ld < 2049 || ld > 32768) return singa_detail_fail(SINGA_E_SHAPE, "lap_pe_xl: graphs of 2,049 up to 32,768 atoms");
    if (B <= 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "lap_pe_xl: not part of the emulation build");
#else
    if (singa_lap_pe_xl_work(B, ld) <= 0) return singa_detail_fail(SINGA_E_SHAPE, "lap_pe_xl: B * ceil(ld / 32) beyond 2^22 workgroups");
    hipStream_t st = (hipStream_t)stream;
    const int spg = (ld + XL_SLAB - 1) / XL_SLAB;
    const dim3 slabs((unsigned)(B * spg)), graphs((unsigned)B), wg(XL_THREADS);
    int host[2];
    // two words of the host record, once the stream has run what was enqueued
    auto read_back = [&](int slot) -> hipError_t {
        hipError_t e = hipMemcpyAsync(host, reinterpret_cast<const int*>(work) + slot, sizeof host, hipMemcpyDeviceToHost, st);
        return e != hipSuccess ? e : hipStreamSynchronize(st);
    };
    hipLaunchKernelGGL(xl_init_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
    hipLaunchKernelGGL(xl_edges_kernel, slabs, wg, 0, st, esrc, edst, eptr, nnodes, work, B, ld, spg);
    hipLaunchKernelGGL(xl_merge_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
    hipLaunchKernelGGL(xl_values_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
    for (int round = 0; round < XL_CC_CAP; ++round) {
        hipLaunchKernelGGL(xl_cc_kernel, slabs, wg, 0, st, nnodes, work, ld, spg, round);
        if (read_back(round) != hipSuccess) return singa_detail_check_launch("lap_pe_xl (component labels)");
        if (!host[0]) break;
    }
    hipLaunchKernelGGL(xl_null_check_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
    hipLaunchKernelGGL(xl_null_rank_kernel, graphs, dim3(64), 0, st, nnodes, work, ld, spg, kout);
    hipLaunchKernelGGL(xl_null_fill_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
    auto orthonormalise = [&]() {
        for (int pass = 0; pass < 2; ++pass) {
            hipLaunchKernelGGL(xl_zdot_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
            hipLaunchKernelGGL(xl_coef_kernel, graphs, dim3(128), 0, st, nnodes, work, ld, spg);
            hipLaunchKernelGGL(xl_gram_kernel<0>, slabs, wg, 0, st, nnodes, work, ld, spg);
            hipLaunchKernelGGL(xl_chol_kernel, graphs, wg, 0, st, nnodes, work, ld, spg);
            hipLaunchKernelGGL(xl_solve_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
        }
    };
    orthonormalise();
    for (int it = 0; it < XL_MAXIT; ++it) {
        hipLaunchKernelGGL(xl_gram_kernel<1>, slabs, wg, 0, st, nnodes, work, ld, spg);
        hipLaunchKernelGGL(xl_rr_kernel, graphs, wg, 0, st, nnodes, work, ld, spg);
        hipLaunchKernelGGL(xl_rotate_kernel, slabs, wg, 0, st, nnodes, work, ld, spg);
        hipLaunchKernelGGL(xl_decide_kernel, graphs, dim3(64), 0, st, nnodes, work, ld, spg, kout, it);
        if (read_back(64 + 2 * it) != hipSuccess) return singa_detail_check_launch("lap_pe_xl (outer iteration)");
        if (!host[0]) break;                             // every graph has converged or given up
        for (int step = 1; step <= host[1]; ++step) hipLaunchKernelGGL(xl_filter_kernel, slabs, wg, 0, st, nnodes, work, ld, spg, step);
        orthonormalise();
    }
    hipLaunchKernelGGL(xl_emit_part_kernel, slabs, wg, 0, st, nnodes, work, ld, spg, kout);
    hipLaunchKernelGGL(xl_emit_sign_kernel, graphs, dim3(64), 0, st, nnodes, work, status, ld, spg, kout);
    hipLaunchKernelGGL(xl_emit_write_kernel, slabs, wg, 0, st, nnodes, first, work, out, ld, spg, kout);
    return singa_detail_check_launch("lap_pe_xl");
#endif
}
