// n1 for molecules of any size (include/singa_hip_knn_large.h): singa_knn_graph's contract with the candidates streamed instead
// of held in registers.  A translation unit of its own, linked into libsinga_hip.so; it reports errors through the two hooks
// singa_hip.hip exports to it (hidden: not part of any ABI).
//
// Work split.  A workgroup of 256 threads = 4 wavefronts owns 4 C consecutive centre atoms, C per wavefront against the same
// tile: C = 1 for launches of up to 8,192 atoms, where the workgroups would otherwise not fill the device, C = 2 above (measured:
// profiles/knn_large/README.md; C = 4 was slower at every size).  It walks the atom
// range [LO, HI) that its centres' molecules cover (one molecule for all but the workgroups at a molecule boundary) in tiles of
// 1,024 atoms: a tile's coordinates come from L2 once per workgroup, as one contiguous read, and are laid out in LDS as three
// planes, so that lane l of a batch reads word 64 b + l of each plane - no bank conflict (the plane stride 1,024 + 22 also
// spreads the transposing writes over the banks).  The tiles are visited from the one that holds the first centre outwards,
// alternating sides: atoms of a chain are numbered along it, so the near tiles tighten the threshold first.  The result does
// not depend on the order.
//
// Selection.  Per centre the k <= 64 best keys so far are ONE 64-bit key per lane, sorted ascending across the wavefront, all
// ones where empty; the admission threshold is lane k - 1's key, wave-uniform.  A batch is 64 candidates, one per lane: three
// LDS reads, then per centre a distance, a key, a compare against the threshold and a ballot.  Nothing admitted - the common
// case once the list has tightened - costs nothing more.  Otherwise the admitted keys enter the list: up to KL_INSERT of them
// one by one (rank by ballot + popcount, shift the tail up a lane), more through a bitonic network - the batch sorted descending
// (21 compare-exchanges), the lane-wise minimum against the list (= the lower half of a 128-key bitonic merge), six more
// compare-exchanges.  Keys are unique (the atom index is part of them), so no stage needs a tie rule; the all-ones fillers are
// equal to each other, and exchanging equals changes nothing.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/singa_hip.h"
#include "../../include/singa_hip_knn_large.h"

int singa_detail_fail(int code, const char* msg);
int singa_detail_check_launch(const char* what);

#ifndef SINGA_EMUL      // (cross-lane / workgroup-cooperative: not part of the sequential CPU emulation build of tests/emul)
namespace {

typedef unsigned long long u64;

constexpr int KL_SPLIT = 8192;                   // atoms per launch up to which a wavefront carries one centre, two above
constexpr int KL_TILE = 1024;                    // candidate atoms per LDS tile (a multiple of 64)
constexpr int KL_PLANE = KL_TILE + 22;           // words between the x, y and z planes
#ifndef SINGA_KNN_LARGE_INSERT
#define SINGA_KNN_LARGE_INSERT 8
#endif
constexpr int KL_INSERT = SINGA_KNN_LARGE_INSERT;   // admitted keys per batch up to which they are inserted one by one
constexpr u64 KL_NONE = ~0ull;

__device__ __forceinline__ u64 kl_lane(u64 v, int src) {          // lane `src`'s value (src wave-uniform) in every lane
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 kl_xor(u64 v, int mask) {
    const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, mask, 64);
    const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(v >> 32), mask, 64);
    return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 kl_up1(u64 v) {                     // lane l - 1's value; lane 0 keeps its own
    const unsigned lo = (unsigned)__shfl_up((int)(unsigned)v, 1, 64);
    const unsigned hi = (unsigned)__shfl_up((int)(unsigned)(v >> 32), 1, 64);
    return ((u64)hi << 32) | lo;
}

// one compare-exchange with lane ^ stride: this lane keeps the smaller of the pair where flip == 0, the larger where flip is all
// ones (min(a ^ f, b ^ f) ^ f is the maximum).  The direction is lane arithmetic in a vector register, not a lane predicate:
// 27 predicates hoisted out of the batch loop would take more scalar registers than there are.
__device__ __forceinline__ u64 kl_cex(u64 v, int stride, unsigned flip) {
    const u64 o = kl_xor(v, stride), f = ((u64)flip << 32) | flip;
    return ((o ^ f) < (v ^ f)) ? o : v;
}

// `list` ascending across the lanes + one key -> the 64 smallest of the 65, ascending
__device__ __forceinline__ u64 kl_insert(u64 list, u64 key, int lane) {
    const int p = __popcll(__ballot(list < key));
    const u64 prev = kl_up1(list);
    return lane < p ? list : (lane == p ? key : prev);
}

// `list` ascending + 64 keys `v` in any order -> the 64 smallest of the 128, ascending
__device__ __forceinline__ u64 kl_merge(u64 list, u64 v, int lane) {
#pragma unroll
    for (int lsize = 1; lsize <= 6; ++lsize) {                     // sort descending: the blocks a plain sort runs up run down
#pragma unroll
        for (int ls = lsize - 1; ls >= 0; --ls) v = kl_cex(v, 1 << ls, ((((unsigned)lane >> ls) ^ ((unsigned)lane >> lsize)) & 1u) - 1u);
    }
    v = v < list ? v : list;                                       // ascending against descending: bitonic, and the lower half
#pragma unroll
    for (int ls = 5; ls >= 0; --ls) v = kl_cex(v, 1 << ls, 0u - (((unsigned)lane >> ls) & 1u));
    return v;
}

// The squared distance, every operation rounded on its own.  Plain operators under `fp contract(off)`, not __fmul_rn / __fadd_rn:
// those are inline functions of the HIP headers, compiled under the default that lets a * b + c fuse, and the fused form came
// out of them here (v_fmac_f32) - an exact tie of (dx*dx + dy*dy) + dz*dz then stops being one.
__device__ __forceinline__ float kl_d2(float px, float py, float pz, float x, float y, float z) {
#pragma clang fp contract(off)
    const float dx = px - x, dy = py - y, dz = pz - z;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ int kl_clamp(long long v, int n) { return v < 0 ? 0 : (v > n ? n : (int)v); }

template <int KL_C>                               // centres per wavefront
__global__ __launch_bounds__(256) void knn_graph_large_kernel(const float* __restrict__ pos, const int* __restrict__ batch,
                                                              const long long* __restrict__ ptr, int B, int N, int k,
                                                              long long* __restrict__ row, long long* __restrict__ col) {
    constexpr int KL_CENTRES = 4 * KL_C;          // per workgroup
    __shared__ float tile[3 * KL_PLANE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i0 = blockIdx.x * KL_CENTRES;

    // the atom range the workgroup's centres can draw candidates from (ptr clamped to [0, N]: no read leaves pos)
    int LO = N, HI = 0;
    for (int j = 0; j < KL_CENTRES; ++j) {
        const int g = i0 + j < N ? batch[i0 + j] : -1;
        if (g < 0 || g >= B) continue;
        const int lo = kl_clamp(ptr[g], N), hi = kl_clamp(ptr[g + 1], N);
        if (lo >= hi) continue;
        LO = lo < LO ? lo : LO;
        HI = hi > HI ? hi : HI;
    }

    // this wavefront's centres; one of no molecule (or past N) has the empty range and keeps an empty list
    int ci[KL_C], clo[KL_C], chi[KL_C];
    float px[KL_C], py[KL_C], pz[KL_C];
    u64 list[KL_C], thr[KL_C];
#pragma unroll
    for (int c = 0; c < KL_C; ++c) {
        const int i = i0 + wave * KL_C + c;
        const int g = i < N ? batch[i] : -1;
        const bool in = g >= 0 && g < B;
        ci[c] = i;
        clo[c] = in ? kl_clamp(ptr[g], N) : 0;
        chi[c] = in ? kl_clamp(ptr[g + 1], N) : 0;
        px[c] = in ? pos[3ll * i] : 0.f;
        py[c] = in ? pos[3ll * i + 1] : 0.f;
        pz[c] = in ? pos[3ll * i + 2] : 0.f;
        list[c] = thr[c] = KL_NONE;
    }

    const int T = LO < HI ? (HI - LO + KL_TILE - 1) / KL_TILE : 0;
    int up = T ? ((i0 < LO ? LO : (i0 >= HI ? HI - 1 : i0)) - LO) / KL_TILE : 0, down = up - 1;
    for (int s = 0; s < T; ++s) {
        const bool take_up = (s & 1) == 0 ? up < T : down < 0;     // alternate; the side that has run out yields
        const int t = take_up ? up++ : down--;
        const int base = LO + t * KL_TILE;
        const int cnt = HI - base < KL_TILE ? HI - base : KL_TILE;
        __syncthreads();                                           // the previous tile has been read by every wavefront
        for (int e = threadIdx.x; e < 3 * cnt; e += 256) {
            const int a = e / 3;
            tile[(e - 3 * a) * KL_PLANE + a] = pos[3ll * base + e];
        }
        __syncthreads();
        for (int b0 = 0; b0 < cnt; b0 += 64) {
            const int j = b0 + lane;                               // < KL_TILE; past cnt: stale words, masked below
            const int cand = base + j;
            const float x = tile[j], y = tile[KL_PLANE + j], z = tile[2 * KL_PLANE + j];
#pragma unroll
            for (int c = 0; c < KL_C; ++c) {
                const float d2 = kl_d2(px[c], py[c], pz[c], x, y, z);
                const bool ok = j < cnt && cand >= clo[c] && cand < chi[c] && cand != ci[c];
                const u64 key = ok ? ((u64)__float_as_uint(d2) << 32) | (unsigned)cand : KL_NONE;
                const bool adm = key < thr[c];
                u64 mask = __ballot(adm);
                if (mask == 0) continue;
                if (__popcll(mask) <= KL_INSERT) {
                    do {
                        list[c] = kl_insert(list[c], kl_lane(key, __ffsll((long long)mask) - 1), lane);
                        mask &= mask - 1;
                    } while (mask);
                } else {
                    list[c] = kl_merge(list[c], adm ? key : KL_NONE, lane);
                }
                thr[c] = kl_lane(list[c], k - 1);
            }
        }
    }

#pragma unroll
    for (int c = 0; c < KL_C; ++c) {
        if (ci[c] >= N || lane >= k) continue;
        const bool have = list[c] != KL_NONE;
        const long long o = (long long)ci[c] * k + lane;
        row[o] = have ? (long long)ci[c] : -1;
        col[o] = have ? (long long)(unsigned)list[c] : -1;
    }
}

}  // namespace
#endif  // SINGA_EMUL

extern "C" int singa_knn_graph_large(const float* pos, const int32_t* batch, const long long* ptr, int B, int N, int k,
                                     long long* row, long long* col, void* stream) {
    if (!pos || !batch || !ptr || !row || !col) return singa_detail_fail(SINGA_E_NULL, "knn_graph_large: null pointer");
    if (k < 1 || k > 64) return singa_detail_fail(SINGA_E_SHAPE, "knn_graph_large: k must be 1 .. 64");
    if (B < 0 || N < 0) return singa_detail_fail(SINGA_E_SHAPE, "knn_graph_large: negative size");
    if (3ll * N > INT_MAX || (long long)N * k > INT_MAX)
        return singa_detail_fail(SINGA_E_SHAPE, "knn_graph_large: 3 * N and N * k must fit an int32 count");
    if (N == 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "knn_graph_large: not part of the emulation build");
#else
    const dim3 block(256);
    hipStream_t st = (hipStream_t)stream;
    if (N <= KL_SPLIT) hipLaunchKernelGGL(knn_graph_large_kernel<1>, dim3((unsigned)((N + 3) / 4)), block, 0, st, pos, batch, ptr, B, N, k, row, col);
    else hipLaunchKernelGGL(knn_graph_large_kernel<2>, dim3((unsigned)((N + 7) / 8)), block, 0, st, pos, batch, ptr, B, N, k, row, col);
    return singa_detail_check_launch("knn_graph_large");
#endif
}
