// k15e: the kNN edge MLPs once per undirected edge with bf16 operands on the matrix cores (include/singa_hip_emlp_bf16.h).  A
// translation unit of its own, linked into libsinga_hip.so; it reports errors through the two hooks singa_hip.hip exports
// (hidden: not part of any ABI).  The units contract, the grids, the end test and the partial rows are those of the f32 unit
// kernels (k15c, singa_hip.hip); what differs is the arithmetic of the products and how the operands travel.
//
// v_mfma_f32_32x32x16_bf16: lane l gives row / column l % 32 and the 8 reduction indices 8 h .. 8 h + 7 (h = l / 32) of the
// instruction's 16, for both operands; the accumulator has the map of 32x32x2f32 (register s of half h: row 8 (s/4) + 4 h + s%4,
// column l % 32).
//
// Chaining.  GEMM 1 is computed transposed as in k15c, pre^T[hidden x edge] = W1 . attr^T: the edge is on the lane.  Registers
// 8 n .. 8 n + 7 of the activated accumulator, rounded and packed pairwise (v_cvt_pk_bf16_f32), ARE the B fragment of MFMA n of
// GEMM 2 - its reduction index j of half h is then hidden unit 16 n + 8 (j/4) + 4 h + j%4 of the 32-unit tile - and the W2 image
// in LDS holds its columns in that order (column 16 n' + 8 q + 4 h + j at position 16 n' + 8 h + 4 q + j, permuted once at
// staging), so the A fragment is one contiguous ds_read_b128.  Two MFMAs per hidden tile; h never leaves registers.  The
// backward's two chains (pre^T, and gh^T = W2^T g^T) feed only register-wise code, so they need no permutation.
//
// attr.  A lane keeps the f32 half row k15c gives it (32 channels 32 h .. 32 h + 31 of its edge: one contiguous 128-byte read,
// prefetched one tile ahead, unit numbers two tiles ahead) and packs it in registers: MFMA m of GEMM 1 takes channels
// 32 h + 8 m + j, four MFMAs for the 64-channel reduction, and the W1 image is read at the same place.  The forward packs once
// for both nets.
//
// Weight images.  bf16, rounded once at staging, [row][cols + 8]: 144 bytes a row for 64 columns, 80 for 32, i.e. 9 or 5 16-byte
// slots.  A ds_read_b128 is served per 16-lane group, each group lies in one lane half and holds 16 rows of all residues mod 16
// (k7b's note); times an odd slot pitch these are 16 different slots of the 256-byte bank row: conflict-free.  Derived from
// the bank rules; no LDS bank-conflict counter was read.
//
// Weight gradients (reduction over the edge).  dW2 += g^T h and dW1 += g_pre^T attr take all four operands from wave-private
// bf16 images [edge][column] written from registers as rows (ds_write_b128 / b64: a lane's packed registers are consecutive
// columns of its edge) and read TRANSPOSED with ds_read_b64_tr_b16, exactly as k7b reads its output-contiguous images: 16 lanes
// fetch 4 edges x 16 columns, lane 4 q + p gives the address of (edge q, columns 4 p ..), two reads make a lane's 8 edges.
// Row pitches 192 bytes (64 columns) and 64 bytes (32 columns), 48 and 16 dwords mod 64: the four edges of a 32-lane half's
// read lie in four different 16-bank quarters.  Transposed stores instead would be 16 ds_write_b16 per lane and image.  A
// wavefront's region is 8 KB ([32][32] for g_pre then h, [32][64] for attr then g; LDS operations of one wavefront complete in
// order), 42 KB a workgroup where k15c has 70 KB.  Three workgroups would fit a CU, but the grid is fixed by the partial rows
// of singa_edge_mlp_bwd_nparts at two per CU, so there is no third to place; the forward kernel (26 KB, grid of up to 768) runs
// three per CU.
//
// Bias gradients are column sums of the UNROUNDED f32 g and g_pre: every lane adds its own edge's values into registers tile after
// tile, and the 32 lanes of a half are summed once, behind the tile loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/singa_hip.h"
#include "../../include/singa_hip_emlp_bf16.h"

int singa_detail_fail(int code, const char* msg);
int singa_detail_check_launch(const char* what);

#ifndef SINGA_EMUL      // (bf16 matrix cores and the transposing LDS read: no stand-in in the CPU emulation build of tests/emul)
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bfx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bfx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bfx8 __attribute__((ext_vector_type(8)));

constexpr int EB_P64 = 72, EB_P32 = 40;             // bf16 per row of a weight image of 64 / 32 columns
constexpr int eb_wpitch(int cols) { return cols == 64 ? EB_P64 : EB_P32; }
constexpr int EB_T64 = 192, EB_T32 = 64;            // bytes per row of a transposed-read image of 64 / 32 columns
constexpr int eb_tpitch(int cols) { return cols == 64 ? EB_T64 : EB_T32; }
constexpr int EB_REG = 32 * EB_T32 + 32 * EB_T64;   // a wavefront's region of the backward kernel, bytes

__device__ __forceinline__ unsigned eb_pack2(float x, float y) {       // bf16(x) | bf16(y) << 16, round to nearest even
    const f32x2 v = {x, y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bfx2));
}
__device__ __forceinline__ bfx8 eb_frag(unsigned a, unsigned b, unsigned c, unsigned d) {
    return __builtin_bit_cast(bfx8, make_uint4(a, b, c, d));
}
__device__ __forceinline__ bfx8 eb_read128(const char* p) { return __builtin_bit_cast(bfx8, *reinterpret_cast<const uint4*>(p)); }
__device__ __forceinline__ f32x16 eb_mfma(const bfx8& a, const bfx8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// the fragment of MFMA m (edges 16 m .. 16 m + 15) of the 32 columns from `col0` of an [edge][column] image: lane l receives
// column col0 + l % 32 of edges 16 m + 8 h .. + 7.  Every address is a multiple of 8 bytes; EXEC is full where this runs.
__device__ __forceinline__ bfx8 eb_frag_tr(const char* img, int pitch, int col0, int m, int lane) {
    const int half = lane >> 5, q = (lane >> 2) & 3, p = lane & 3, c0 = col0 + (lane & 16);
    const char* a = img + (16 * m + 8 * half + q) * pitch + 2 * (c0 + 4 * p);
    typedef __attribute__((address_space(3))) bfx4* lds4;
    const bfx4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)a);
    const bfx4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds4)(a + 4 * pitch));
    return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
__device__ __forceinline__ void eb_lds_order() { asm volatile("" ::: "memory"); }      // the compiler keeps LDS accesses on their side

// stage w[ROWS][COLS] (f32, as stored; element (r, c) at w[r * ld_r + c * ld_c]) as a bf16 image.  PERM: the column order of a
// GEMM 2 operand (head of the file).  Two phases, so that a workgroup's loads are all in flight together (k15c's note).
template <int ROWS, int COLS>
__device__ __forceinline__ void eb_stage_load(float (&v)[ROWS * COLS / 256], const float* __restrict__ w, int ld_r, int ld_c) {
#pragma unroll
    for (int k = 0; k < ROWS * COLS / 256; ++k) {
        const int t = threadIdx.x + 256 * k;
        v[k] = w[(t / COLS) * ld_r + (t % COLS) * ld_c];
    }
}
template <int ROWS, int COLS, bool PERM>
__device__ __forceinline__ void eb_stage_store(unsigned short* __restrict__ img, const float (&v)[ROWS * COLS / 256]) {
#pragma unroll
    for (int k = 0; k < ROWS * COLS / 256; ++k) {
        const int t = threadIdx.x + 256 * k, c = t % COLS;
        const int pos = PERM ? (c & ~15) | (((c >> 2) & 1) << 3) | (((c >> 3) & 1) << 2) | (c & 3) : c;
        img[(t / COLS) * eb_wpitch(COLS) + pos] = (unsigned short)(eb_pack2(v[k], 0.f) & 0xffffu);
    }
}

__device__ __forceinline__ float eb_ssp(float x) { return fmaxf(x, 0.f) + __logf(1.f + __expf(-fabsf(x))) - 0.69314718055994530942f; }

// acc[k] += v[2 k + b] of this lane + v[2 k + b] of lane ^ 16, b = bit 4 of the lane: one exchange halves the registers that a
// running column sum over the lanes costs (the sums are f32, the order of their additions is free)
template <int N>
__device__ __forceinline__ void eb_fold(float (&acc)[N / 2], const float (&v)[N], bool hi) {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) acc[k] += (hi ? v[2 * k + 1] : v[2 * k]) + __shfl_xor(hi ? v[2 * k] : v[2 * k + 1], 16, 64);
}

// the unit of lane i of tile tl; anything that is no row of [0, E) counts as "no unit" / "no mate": no address leaves the arrays
__device__ __forceinline__ void eb_unit_of(const int32_t* __restrict__ unit_a, const int32_t* __restrict__ unit_b, long long tl, int i,
                                           int E, int& a, int& b) {
    const long long u = tl * 32 + i, uc = u < E ? u : (long long)E - 1;
    const int ra = unit_a[uc], rb = unit_b[uc];
    a = u < E && ra >= 0 && ra < E ? ra : -1;
    b = rb >= 0 && rb < E ? rb : a;
}

// one net on one 32-unit tile: pa = the lane's packed half row of attr (pa[k]: channels 32 h + 2 k, + 1).  w1 [H][64] and w2 [H][H]
// (permuted columns) are the bf16 images, b1 / b2 f32.  T = H / 32 hidden and output tiles.
template <int H>
__device__ __forceinline__ void eb_tile(const unsigned (&pa)[16], const unsigned short* __restrict__ w1, const float* __restrict__ b1,
                                        const unsigned short* __restrict__ w2, const float* __restrict__ b2, int lane,
                                        f32x16 (&out)[H / 32]) {
    constexpr int T = H / 32, P2 = eb_wpitch(H);
    const int i = lane & 31, half = lane >> 5;
    f32x16 hacc[T];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) hacc[t][r] = b1[32 * t + 8 * (r >> 2) + 4 * half + (r & 3)];
    const char* a1 = reinterpret_cast<const char*>(w1) + i * (2 * EB_P64) + 64 * half;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const bfx8 b = eb_frag(pa[4 * m], pa[4 * m + 1], pa[4 * m + 2], pa[4 * m + 3]);
#pragma unroll
        for (int t = 0; t < T; ++t) hacc[t] = eb_mfma(eb_read128(a1 + 32 * t * (2 * EB_P64) + 16 * m), b, hacc[t]);
    }
#pragma unroll
    for (int u = 0; u < T; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) out[u][r] = b2[32 * u + 8 * (r >> 2) + 4 * half + (r & 3)];
    const char* a2 = reinterpret_cast<const char*>(w2) + i * (2 * P2) + 16 * half;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            unsigned hb[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) hb[k] = eb_pack2(eb_ssp(hacc[t][8 * n + 2 * k]), eb_ssp(hacc[t][8 * n + 2 * k + 1]));
            const bfx8 b = eb_frag(hb[0], hb[1], hb[2], hb[3]);
#pragma unroll
            for (int u = 0; u < T; ++u) out[u] = eb_mfma(eb_read128(a2 + 32 * u * (2 * P2) + 2 * (32 * t + 16 * n)), b, out[u]);
        }
}

__global__ void __launch_bounds__(256, 3) emlp_bf16_fwd_kernel(const float* __restrict__ attr, const float* __restrict__ w1k,
                                                               const float* __restrict__ b1k, const float* __restrict__ w2k,
                                                               const float* __restrict__ b2k, const float* __restrict__ w1v,
                                                               const float* __restrict__ b1v, const float* __restrict__ w2v,
                                                               const float* __restrict__ b2v, float* __restrict__ wk,
                                                               float* __restrict__ wv, int E, const int32_t* __restrict__ unit_a,
                                                               const int32_t* __restrict__ unit_b) {
    __shared__ __attribute__((aligned(16))) unsigned short lw1k[32 * EB_P64], lw2k[32 * EB_P32], lw1v[64 * EB_P64], lw2v[64 * EB_P64];
    __shared__ float lb[32 + 32 + 64 + 64];
    {                                                      // the parameters arrive in nn.Linear's own [out][in] layout
        float s1k[8], s2k[4], s1v[16], s2v[16];
        eb_stage_load<32, 64>(s1k, w1k, 64, 1);
        eb_stage_load<32, 32>(s2k, w2k, 32, 1);
        eb_stage_load<64, 64>(s1v, w1v, 64, 1);
        eb_stage_load<64, 64>(s2v, w2v, 64, 1);
        const int tb = threadIdx.x & 63;
        const float bias = threadIdx.x < 64 ? (tb < 32 ? b1k[tb] : b2k[tb - 32]) : threadIdx.x < 128 ? b1v[tb] : threadIdx.x < 192 ? b2v[tb] : 0.f;
        eb_stage_store<32, 64, false>(lw1k, s1k);
        eb_stage_store<32, 32, true>(lw2k, s2k);
        eb_stage_store<64, 64, false>(lw1v, s1v);
        eb_stage_store<64, 64, true>(lw2v, s2v);
        if (threadIdx.x < 192) lb[threadIdx.x] = bias;     // [b1k | b2k | b1v | b2v]
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, i = lane & 31, half = lane >> 5;
    const long long tiles = ((long long)E + 31) / 32, stride = (long long)gridDim.x * 4;
    long long tile = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    float4 nxt[8];
    int ca = -1, cb = -1, na = -1, nb = -1;     // the rows of the tile whose attr rows `nxt` holds, of the tile behind it
    auto fetch = [&]() __attribute__((always_inline)) {                  // this lane's half row of the unit (na, nb)
        const float* row = attr + (long long)(na > 0 ? na : 0) * 64 + 32 * half;
#pragma unroll
        for (int m = 0; m < 8; ++m) nxt[m] = *reinterpret_cast<const float4*>(row + 4 * m);
    };
    auto advance = [&](long long tl) __attribute__((always_inline)) {    // fetched (na, nb); now the unit of tile tl
        ca = na, cb = nb, na = nb = -1;
        if (tl < tiles) eb_unit_of(unit_a, unit_b, tl, i, E, na, nb);
    };
    if (tile < tiles) {
        eb_unit_of(unit_a, unit_b, tile, i, E, na, nb);
        fetch();
        advance(tile + stride);
    }
    for (; tile < tiles; tile += stride) {
        const long long e0 = ca, e1 = cb;
        const bool ok = ca >= 0;
        if (__ballot(ok) == 0ull) break;                   // the units come first: nothing but the null tail from here on
        const int rows = !ok ? 0 : e1 != e0 ? 2 : 1;       // the rows this lane's registers go to
        unsigned pa[16];
#pragma unroll
        for (int m = 0; m < 8; ++m) pa[2 * m] = eb_pack2(nxt[m].x, nxt[m].y), pa[2 * m + 1] = eb_pack2(nxt[m].z, nxt[m].w);
        if (tile + stride < tiles) fetch();                // the next tile's rows travel while this tile is computed and stored
        advance(tile + 2 * stride);
        {
            f32x16 out[1];
            eb_tile<32>(pa, lw1k, lb, lw2k, lb + 32, lane, out);
            for (int d = 0; d < rows; ++d) {
                const long long e = d ? e1 : e0;
#pragma unroll
                for (int blk = 0; blk < 4; ++blk)
                    *reinterpret_cast<float4*>(wk + e * 32 + 8 * blk + 4 * half) =
                        make_float4(out[0][4 * blk], out[0][4 * blk + 1], out[0][4 * blk + 2], out[0][4 * blk + 3]);
            }
        }
        {
            f32x16 out[2];
            eb_tile<64>(pa, lw1v, lb + 64, lw2v, lb + 128, lane, out);
            for (int d = 0; d < rows; ++d) {
                const long long e = d ? e1 : e0;
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int blk = 0; blk < 4; ++blk)
                        *reinterpret_cast<float4*>(wv + e * 64 + 32 * u + 8 * blk + 4 * half) =
                            make_float4(out[u][4 * blk], out[u][4 * blk + 1], out[u][4 * blk + 2], out[u][4 * blk + 3]);
            }
        }
    }
}

// Backward of one net, one slice of 32 hidden units per workgroup (blockIdx.y), as k15c: pre^T and gh^T on the lane's packed
// registers, h and g_pre register-wise in f32, then the two weight-gradient products from the wave's images.  The partial row
// and its reduction through LDS are k15c's.
template <int H>
__global__ void __launch_bounds__(256, 2) emlp_bf16_bwd_kernel(const float* __restrict__ attr, const float* __restrict__ g_out,
                                                               const float* __restrict__ w1, const float* __restrict__ b1,
                                                               const float* __restrict__ w2, float* __restrict__ part, int E,
                                                               const int32_t* __restrict__ unit_a, const int32_t* __restrict__ unit_b) {
    constexpr int TO = H / 32, HH = H / 2, P2 = eb_wpitch(H), GP = eb_tpitch(H);
    constexpr int PSZ = 32 * 64 + 32 + H * 32 + H;
    __shared__ __attribute__((aligned(16))) unsigned short lw1[32 * EB_P64], lw2[32 * P2];
    __shared__ __attribute__((aligned(16))) char tiles[4 * EB_REG];
    __shared__ float lb1[32];
    static_assert(4 * EB_REG >= 4 * PSZ, "the tile images double as the reduction buffer");
    const int ht = blockIdx.y;                          // hidden units [32 ht, 32 ht + 32)
    {
        float s1[8], s2[H / 8];
        eb_stage_load<32, 64>(s1, w1 + (long long)32 * ht * 64, 64, 1);       // rows 32 ht .. of W1 [H][64]
        eb_stage_load<32, H>(s2, w2 + 32 * ht, 1, H);                         // columns 32 ht .. of W2 [H][H], as rows of W2^T
        const float bias = b1[32 * ht + (threadIdx.x & 31)];
        eb_stage_store<32, 64, false>(lw1, s1);
        eb_stage_store<32, H, false>(lw2, s2);
        if (threadIdx.x < 32) lb1[threadIdx.x] = bias;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 31, half = lane >> 5;
    char* timg = tiles + wave * EB_REG;                 // [32 edges][32 hidden] bf16: g_pre, then h
    char* rimg = timg + 32 * EB_T32;                    // [32 edges][64] attr, then [32 edges][H] g
    f32x16 dw2[TO], dw1[2];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int a = 0; a < TO; ++a) dw2[a][r] = 0.f;
        dw1[0][r] = 0.f, dw1[1][r] = 0.f;
    }
    // sums of g (output unit HH half + 2 k + hi) and of g_pre (accumulator register 2 k + hi) over the edges of lanes l and l ^ 16
    const bool hi = (lane & 16) != 0;
    float gsum[HH / 2], psum[8];
#pragma unroll
    for (int s = 0; s < HH / 2; ++s) gsum[s] = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) psum[r] = 0.f;
    const long long tilesN = ((long long)E + 31) / 32, stride = (long long)gridDim.x * 4;
    long long tile = (long long)blockIdx.x * 4 + wave;
    float4 nasel4[8], ngrow4[HH / 4], nmate4[HH / 4];
    int ca = -1, cb = -1, na = -1, nb = -1;             // the rows of the tile that is fetched, of the tile behind it
    auto fetch = [&]() __attribute__((always_inline)) {                  // this lane's half row of attr of the unit (na, nb)
        const long long er = na > 0 ? na : 0;
#pragma unroll
        for (int m = 0; m < 8; ++m) nasel4[m] = *reinterpret_cast<const float4*>(attr + er * 64 + 32 * half + 4 * m);
    };
    auto advance = [&](long long tl) __attribute__((always_inline)) {    // fetched (na, nb); now the unit of tile tl
        ca = na, cb = nb;
        eb_unit_of(unit_a, unit_b, tl, i, E, na, nb);                    // (a tile behind the last one: no unit)
    };
    auto fetch_g = [&]() __attribute__((always_inline)) {                // the gradient half rows of the unit (ca, cb)
        const long long er = ca > 0 ? ca : 0, em = ca >= 0 ? cb : 0;     // (a row without a mate: its own row, read and not added)
#pragma unroll
        for (int m = 0; m < HH / 4; ++m) ngrow4[m] = *reinterpret_cast<const float4*>(g_out + er * H + HH * half + 4 * m);
#pragma unroll
        for (int m = 0; m < HH / 4; ++m) nmate4[m] = *reinterpret_cast<const float4*>(g_out + em * H + HH * half + 4 * m);
    };
    if (tile < tilesN) {
        eb_unit_of(unit_a, unit_b, tile, i, E, na, nb);
        fetch();
        advance(tile + stride), fetch_g();
    }
    for (; tile < tilesN; tile += stride) {
        const bool ok = ca >= 0;                            // false: a lane without a unit - it computes on zero rows
        if (__ballot(ok) == 0ull) break;                    // the units come first: nothing but the null tail from here on
        const bool mated = ok && cb != ca;
        unsigned pa[16], pg[HH / 2];
        float gf[HH], gpf[16];
        // the unit's gradient row, g[a] + g[b] in f32: summed into the bias gradient as it is, rounded once for the products
#pragma unroll
        for (int m = 0; m < HH / 4; ++m) {
            const float4 ga = ngrow4[m], gb = nmate4[m];
            const float x = (ok ? ga.x : 0.f) + (mated ? gb.x : 0.f), y = (ok ? ga.y : 0.f) + (mated ? gb.y : 0.f);
            const float z = (ok ? ga.z : 0.f) + (mated ? gb.z : 0.f), w = (ok ? ga.w : 0.f) + (mated ? gb.w : 0.f);
            gf[4 * m] = x, gf[4 * m + 1] = y, gf[4 * m + 2] = z, gf[4 * m + 3] = w;
            pg[2 * m] = eb_pack2(x, y), pg[2 * m + 1] = eb_pack2(z, w);
        }
        eb_fold<HH>(gsum, gf, hi);
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const float4 v = nasel4[m];
            pa[2 * m] = eb_pack2(ok ? v.x : 0.f, ok ? v.y : 0.f), pa[2 * m + 1] = eb_pack2(ok ? v.z : 0.f, ok ? v.w : 0.f);
        }
        eb_lds_order();                                     // (the previous tile's dW2 reads of the region lie before these writes)
#pragma unroll
        for (int k = 0; k < 4; ++k)                         // region = {g_pre (after the activation), attr rows (now)}
            *reinterpret_cast<uint4*>(rimg + i * EB_T64 + 64 * half + 16 * k) = make_uint4(pa[4 * k], pa[4 * k + 1], pa[4 * k + 2], pa[4 * k + 3]);
        f32x16 pacc, gacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pacc[r] = lb1[8 * (r >> 2) + 4 * half + (r & 3)];
            gacc[r] = 0.f;
        }
        {
            const char* a1 = reinterpret_cast<const char*>(lw1) + i * (2 * EB_P64) + 64 * half;
#pragma unroll
            for (int m = 0; m < 4; ++m)
                pacc = eb_mfma(eb_read128(a1 + 16 * m), eb_frag(pa[4 * m], pa[4 * m + 1], pa[4 * m + 2], pa[4 * m + 3]), pacc);
        }
        fetch();                                            // (a tile behind the last one has no units and fetches row 0)
        advance(tile + 2 * stride);
        {
            const char* a2 = reinterpret_cast<const char*>(lw2) + i * (2 * P2) + 2 * HH * half;   // reduction index: output unit HH half + 8 m + j
#pragma unroll
            for (int m = 0; m < HH / 8; ++m)
                gacc = eb_mfma(eb_read128(a2 + 16 * m), eb_frag(pg[4 * m], pg[4 * m + 1], pg[4 * m + 2], pg[4 * m + 3]), gacc);
        }
        // ---- dW1: g_pre joins the attr rows; h stays in registers, packed
        unsigned ph[8];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            float gp[4], hh[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // h = ssp(p) = max(p, 0) + log(1 + t) - ln 2 and sigmoid(p) = (p >= 0 ? 1 : t) / (1 + t) share t = exp(-|p|)
                const float p = pacc[4 * blk + j];
                const float tq = __expf(-fabsf(p)), u = 1.f + tq;
                gp[j] = gacc[4 * blk + j] * ((p >= 0.f ? 1.f : tq) * __builtin_amdgcn_rcpf(u));
                hh[j] = fmaxf(p, 0.f) + __logf(u) - 0.69314718055994530942f;
                gpf[4 * blk + j] = gp[j];
            }
            ph[2 * blk] = eb_pack2(hh[0], hh[1]), ph[2 * blk + 1] = eb_pack2(hh[2], hh[3]);
            *reinterpret_cast<uint2*>(timg + i * EB_T32 + 2 * (8 * blk + 4 * half)) = make_uint2(eb_pack2(gp[0], gp[1]), eb_pack2(gp[2], gp[3]));
        }
        eb_fold<16>(psum, gpf, hi);
        eb_lds_order();
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const bfx8 a = eb_frag_tr(timg, EB_T32, 0, m, lane);
            dw1[0] = eb_mfma(a, eb_frag_tr(rimg, EB_T64, 0, m, lane), dw1[0]);
            dw1[1] = eb_mfma(a, eb_frag_tr(rimg, EB_T64, 32, m, lane), dw1[1]);
        }
        eb_lds_order();
        // ---- dW2: region = {h, g rows (zero rows for lanes without a unit)}
#pragma unroll
        for (int blk = 0; blk < 4; ++blk)
            *reinterpret_cast<uint2*>(timg + i * EB_T32 + 2 * (8 * blk + 4 * half)) = make_uint2(ph[2 * blk], ph[2 * blk + 1]);
#pragma unroll
        for (int k = 0; k < HH / 8; ++k)
            *reinterpret_cast<uint4*>(rimg + i * GP + 2 * HH * half + 16 * k) = make_uint4(pg[4 * k], pg[4 * k + 1], pg[4 * k + 2], pg[4 * k + 3]);
        fetch_g();                                          // the gradient registers are free: the two rows of the next tile, (ca, cb)
        eb_lds_order();
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            const bfx8 b = eb_frag_tr(timg, EB_T32, 0, m, lane);
#pragma unroll
            for (int a = 0; a < TO; ++a) dw2[a] = eb_mfma(eb_frag_tr(rimg, GP, 32 * a, m, lane), b, dw2[a]);
        }
    }
    // the bias gradients: the 16 lanes of a quarter hold the edges of one set of columns
#pragma unroll
    for (int msk = 1; msk < 16; msk <<= 1) {
#pragma unroll
        for (int s = 0; s < HH / 2; ++s) gsum[s] += __shfl_xor(gsum[s], msk, 64);
#pragma unroll
        for (int r = 0; r < 8; ++r) psum[r] += __shfl_xor(psum[r], msk, 64);
    }
    // workgroup reduction through LDS (the tile images are free now), then one partial row per workgroup and slice
    __syncthreads();
    float* red = reinterpret_cast<float*>(tiles);
    constexpr int O_B1 = 32 * 64, O_W2 = O_B1 + 32, O_B2 = O_W2 + H * 32;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = 8 * (r >> 2) + 4 * half + (r & 3);
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    float* q = red + row * 64 + 32 * b + i;                  // dW1[hidden row of the slice][input channel]
                    *q = w == 0 ? dw1[b][r] : *q + dw1[b][r];
                }
#pragma unroll
                for (int a = 0; a < TO; ++a) {
                    float* q = red + O_W2 + (32 * a + row) * 32 + i;         // dW2[output unit][hidden unit of the slice]
                    *q = w == 0 ? dw2[a][r] : *q + dw2[a][r];
                }
            }
            if ((lane & 15) == 0) {                                          // one lane per quarter: columns 2 k + hi
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int r = 2 * k + (hi ? 1 : 0);
                    float* q = red + O_B1 + 8 * (r >> 2) + 4 * half + (r & 3);
                    *q = w == 0 ? psum[k] : *q + psum[k];
                }
#pragma unroll
                for (int k = 0; k < HH / 2; ++k) {
                    float* q = red + O_B2 + HH * half + 2 * k + (hi ? 1 : 0);
                    *q = w == 0 ? gsum[k] : *q + gsum[k];
                }
            }
        }
        __syncthreads();
    }
    // One partial row per workgroup COLUMN (blockIdx.x), the slices' pieces placed where the parameters' rows are:
    // [dW1 [H][64] | db1 [H] | dW2 [H][H] | db2 [H]] (db2 is the same in every slice: slice 0 writes it).
    constexpr int SL = H / 32, ROW = H * 64 + H + H * H + H;
    float* dst = part + (long long)blockIdx.x * ROW;
    for (int t = threadIdx.x; t < PSZ; t += 256) {
        int off;
        if (t < O_B1) off = ht * 32 * 64 + t;
        else if (t < O_W2) off = SL * 32 * 64 + ht * 32 + (t - O_B1);
        else if (t < O_B2) off = SL * 32 * 64 + SL * 32 + ((t - O_W2) >> 5) * H + ht * 32 + ((t - O_W2) & 31);
        else off = ht == 0 ? SL * 32 * 64 + SL * 32 + H * H + (t - O_B2) : -1;
        if (off >= 0) dst[off] = red[t];
    }
}

}  // namespace
#endif  // SINGA_EMUL

extern "C" int singa_edge_mlp_bf16_units_fwd(const float* attr, const int32_t* unit_a, const int32_t* unit_b, const float* w1tk,
                                             const float* b1k, const float* w2tk, const float* b2k, const float* w1tv, const float* b1v,
                                             const float* w2tv, const float* b2v, float* wk, float* wv, int E, int CIN, int HK, int HV,
                                             void* stream) {
    if (!attr || !unit_a || !unit_b || !w1tk || !b1k || !w2tk || !b2k || !w1tv || !b1v || !w2tv || !b2v || !wk || !wv)
        return singa_detail_fail(SINGA_E_NULL, "edge_mlp_bf16_units_fwd: null pointer");
    if (CIN != 64 || HK != 32 || HV != 64)
        return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_fwd: built for 64 edge channels, 32 key / 64 value channels per head");
    if (E < 0) return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_fwd: E >= 0 rows");
    if ((uintptr_t)attr % 16 || (uintptr_t)wk % 16 || (uintptr_t)wv % 16)
        return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_fwd: attr, wk and wv must be 16-byte aligned");
    if (E == 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_fwd: not part of the emulation build");
#else
    const long long blocks = (((long long)E + 31) / 32 + 3) / 4;
    hipLaunchKernelGGL(emlp_bf16_fwd_kernel, dim3((unsigned)(blocks < 768 ? blocks : 768)), dim3(256), 0, (hipStream_t)stream, attr,
                       w1tk, b1k, w2tk, b2k, w1tv, b1v, w2tv, b2v, wk, wv, E, unit_a, unit_b);
    return singa_detail_check_launch("edge_mlp_bf16_units_fwd");
#endif
}

extern "C" int singa_edge_mlp_bf16_units_bwd(const float* attr, const int32_t* unit_a, const int32_t* unit_b, const float* g_out,
                                             const float* w1t, const float* b1, const float* w2, float* part, int E, int CIN, int H,
                                             void* stream) {
    if (!attr || !unit_a || !unit_b || !g_out || !w1t || !b1 || !w2 || !part)
        return singa_detail_fail(SINGA_E_NULL, "edge_mlp_bf16_units_bwd: null pointer");
    if (CIN != 64 || (H != 32 && H != 64))
        return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_bwd: built for 64 edge channels, 32 key / 64 value channels per head");
    if (E < 0) return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_bwd: E >= 0 rows");
    if ((uintptr_t)attr % 16 || (uintptr_t)g_out % 16)
        return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_bwd: attr and g_out must be 16-byte aligned");
    if (E == 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "edge_mlp_bf16_units_bwd: not part of the emulation build");
#else
    const int blocks = singa_edge_mlp_bwd_nparts(E, H);
    if (H == 32)
        hipLaunchKernelGGL(emlp_bf16_bwd_kernel<32>, dim3(blocks, 1), dim3(256), 0, (hipStream_t)stream, attr, g_out, w1t, b1, w2, part, E,
                           unit_a, unit_b);
    else
        hipLaunchKernelGGL(emlp_bf16_bwd_kernel<64>, dim3(blocks, 2), dim3(256), 0, (hipStream_t)stream, attr, g_out, w1t, b1, w2, part, E,
                           unit_a, unit_b);
    return singa_detail_check_launch("edge_mlp_bf16_units_bwd");
#endif
}
