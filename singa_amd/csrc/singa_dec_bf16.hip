// k20b: the row-tiled decoder step of generation (singa_hip.hip, include/singa_hip_dec_tiles.h) with the five products against a
// weight matrix on the bf16 matrix cores (include/singa_hip_dec_bf16.h).  A translation unit of its own, linked into
// libsinga_hip.so; it reports errors through the two hooks singa_hip.hip exports (hidden: not part of any ABI).  Grids, tiles,
// cache appends, masks, the attention over the caches and over the encoder rows, the LayerNorm and every output are those of the
// f32 tile kernels; what differs is how a product with a weight matrix is made and where the tile's rows wait for it.
//
// v_mfma_f32_16x16x32_bf16: lane l = 16 g + i gives row (A) / column (B) i and the 8 reduction indices 8 g .. 8 g + 7 of the
// instruction's 32; accumulator register r of lane l is row 4 g + r, column i.
//
// Every product is made TRANSPOSED, out^T = W^T x^T: the A operand is a 16 x 32 block of W^T (16 output columns), the B operand
// the tile's 16 rows, so that column i of every MFMA - one lane index - is one row of the tile from the first product to the
// LayerNorm, and a lane's four accumulator registers are four CONSECUTIVE output columns 16 tile + 4 g + r of its row: bias,
// cache append, ReLU and the LDS writes are float4 / packed 8-byte accesses, never a transpose.  Column i of an MFMA depends on
// column i of B alone, so a row's bits depend on nothing else in its tile.
//
// Weights.  singa_dec_bf16_pack rounds a transposed weight matrix [K][N] once (ties to even) and writes it in the order the
// products read it: fragment (column tile, k block, lane) = the 8 values w[32 kb + 8 g + j][16 tile + i], 16 contiguous bytes.
// A wavefront's A operand is one 1 KB run from L2 per MFMA, a lane's part one 16-byte load; the weights have no LDS image, and
// the fragments of the next k blocks are in flight while the matrix cores work on the present ones (db_gemm).
//
// Activations.  The tile's rows are rounded once (v_cvt_pk_bf16_f32) when they are put into LDS as a bf16 image [16][K + 8]
// (pitch = 4 banks mod 64: the 16-byte B reads of a lane group fall on all 64 banks): x, y and z on the way in, the attention
// contexts as they are normalised, the ReLU output as it leaves its accumulators.  Every wavefront re-reads the image, one
// ds_read_b128 per MFMA step shared by its column tiles.  q, the new key and the new value stay f32 in LDS: the attention reads
// them as the f32 kernels do.  The residual is read again from global memory (f32) where the sum for the LayerNorm is formed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/singa_hip.h"
#include "../../include/singa_hip_dec_bf16.h"

int singa_detail_fail(int code, const char* msg);
int singa_detail_check_launch(const char* what);

#ifndef SINGA_EMUL      // (bf16 matrix cores: no stand-in in the CPU emulation build of tests/emul)
namespace {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bfx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bfx8 __attribute__((ext_vector_type(8)));

constexpr int DB_ROWS = 16;                                            // rows of a tile = columns of an MFMA tile
constexpr int DB_LD = 260, DB_QLD = 516, DB_SLD = 132, DB_PLD = 68;    // f32 pitches of [16][256], [16][512], [16][128], [16][64]
constexpr int DB_BLD = 264, DB_HLD = 1032;                             // bf16 pitches of the images [16][256] and [16][1024]
constexpr int DB_CHUNK = 64;                                           // encoder positions per step of the running softmax
constexpr float DB_SCALE = 0.17677669529663687f;                       // 1 / sqrt(32)

__device__ __forceinline__ unsigned db_pack2(float x, float y) {       // bf16(x) | bf16(y) << 16, round to nearest even
    const f32x2 v = {x, y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bfx2));
}
__device__ __forceinline__ uint2 db_pack4(float a, float b, float c, float d) { return make_uint2(db_pack2(a, b), db_pack2(c, d)); }

__device__ __forceinline__ float db_wave_sum64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float db_wave_max64(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// acc[t] (register r: tile row i, output column 16 (tile0 + t) + 4 g + r) += sum over the K = 32 KB reduction indices of
// img[i][k] * w[k][column], `img` a bf16 image in LDS with pitch ldb, `wpk` the packed matrix (KB k blocks per column tile).
// U k blocks = 8 fragments of 16 bytes per lane are requested together, one batch ahead of the MFMAs that use them.
template <int NT, int KB>
__device__ __forceinline__ void db_gemm(const unsigned short* img, int ldb, const uint4* __restrict__ wpk, int tile0,
                                        floatx4 (&acc)[NT]) {
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const unsigned short* bp = img + i * ldb + 8 * g;
    const uint4* wp = wpk + (long long)tile0 * KB * 64 + lane;
    constexpr int U = 8 / NT;
    static_assert(NT * U == 8 && KB % U == 0, "db_gemm: 2 or 4 column tiles per wavefront");
    uint4 cur[U][NT], nxt[U][NT];
    auto load = [&](uint4 (&f)[U][NT], int kb0) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) f[u][t] = wp[(t * KB + kb0 + u) * 64];
    };
    load(nxt, 0);
    for (int kb0 = 0; kb0 < KB; kb0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int t = 0; t < NT; ++t) cur[u][t] = nxt[u][t];
        if (kb0 + U < KB) load(nxt, kb0 + U);
        __builtin_amdgcn_sched_barrier(0);                             // (keep the requests ahead of the MFMAs, as dt_gemm does)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bfx8 b = __builtin_bit_cast(bfx8, *reinterpret_cast<const uint4*>(bp + 32 * (kb0 + u)));
#pragma unroll
            for (int t = 0; t < NT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bfx8, cur[u][t]), b, acc[t], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the tile's 16 input rows, rounded, -> the bf16 image [16][DB_BLD]; rows with live[row] < 0 as zeros, never read
template <int THREADS>
__device__ __forceinline__ void db_rows_in(const float* __restrict__ src, long long row0, const int* live, unsigned short* img) {
    for (int e = threadIdx.x; e < DB_ROWS * 64; e += THREADS) {
        const int row = e >> 6, c4 = (e & 63) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live[row] >= 0) v = *reinterpret_cast<const float4*>(src + (row0 + row) * 256 + c4);
        *reinterpret_cast<uint2*>(img + row * DB_BLD + c4) = db_pack4(v.x, v.y, v.z, v.w);
    }
}

// projection result + bias + residual -> LayerNorm(256) -> out, live rows only.  The residual is the f32 row of `res` in global
// memory; `rs` (LDS [16][DB_LD]) receives (bias + residual) + accumulator - the f32 tile kernels' order -, every wavefront then
// normalises its rows, four channels per lane, as dt_ln_store does.
template <int NW, int NT>
__device__ __forceinline__ void db_ln_store(const floatx4 (&acc)[NT], int tile0, const float* __restrict__ bias,
                                            const float* __restrict__ res, float* rs, const float* __restrict__ gamma,
                                            const float* __restrict__ beta, float eps, float* __restrict__ out, long long row0,
                                            const int* live) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, i = lane & 15, g = lane >> 4;
    const bool on = live[i] >= 0;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const int col = 16 * (tile0 + t) + 4 * g;
        const float4 b = *reinterpret_cast<const float4*>(bias + col);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on) x = *reinterpret_cast<const float4*>(res + (row0 + i) * 256 + col);
        *reinterpret_cast<float4*>(rs + i * DB_LD + col) =
            make_float4((b.x + x.x) + acc[t][0], (b.y + x.y) + acc[t][1], (b.z + x.z) + acc[t][2], (b.w + x.w) + acc[t][3]);
    }
    __syncthreads();
    const float4 gm = *reinterpret_cast<const float4*>(gamma + lane * 4), bt = *reinterpret_cast<const float4*>(beta + lane * 4);
    for (int row = wave; row < DB_ROWS; row += NW) {
        const float4 o = *reinterpret_cast<const float4*>(rs + row * DB_LD + lane * 4);
        const float mean = db_wave_sum64((o.x + o.y) + (o.z + o.w)) * (1.f / 256);
        const float d0 = o.x - mean, d1 = o.y - mean, d2 = o.z - mean, d3 = o.w - mean;
        const float var = db_wave_sum64((d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3)) * (1.f / 256);
        const float rstd = 1.f / sqrtf(var + eps);
        if (live[row] >= 0)
            *reinterpret_cast<float4*>(out + (row0 + row) * 256 + lane * 4) =
                make_float4(d0 * rstd * gm.x + bt.x, d1 * rstd * gm.y + bt.y, d2 * rstd * gm.z + bt.z, d3 * rstd * gm.w + bt.w);
    }
}

// one-time: w_t [K][N] f32 -> the fragments of db_gemm.  One thread per fragment (column tile, k block, lane).
__global__ void __launch_bounds__(256) dec_bf16_pack_kernel(const float* __restrict__ w, int K, int N, uint4* __restrict__ out) {
    const long long f = (long long)blockIdx.x * 256 + threadIdx.x;
    const int KB = K / 32;
    if (f >= (long long)(N / 16) * KB * 64) return;
    const int lane = (int)(f & 63), i = lane & 15, g = lane >> 4, kb = (int)((f >> 6) % KB), tile = (int)((f >> 6) / KB);
    const float* p = w + (long long)(32 * kb + 8 * g) * N + 16 * tile + i;
    out[f] = make_uint4(db_pack2(p[0], p[N]), db_pack2(p[2LL * N], p[3LL * N]), db_pack2(p[4LL * N], p[5LL * N]),
                        db_pack2(p[6LL * N], p[7LL * N]));
}

// self-attention sub-block.  512 threads: q | k | v = 8 wavefronts x 4 column tiles; the attention per row is
// dec_tile_self_attn_kernel's, f32 on f32 caches (wavefront w rows 2 w and 2 w + 1, the new position's key and value from LDS,
// ANC as there); a row's context is rounded into the image that held x and is the B operand of the output projection, whose
// LayerNorm sum lies where q | k | v lay.
template <bool ANC>
__global__ void __launch_bounds__(512) dec_bf16_self_attn_kernel(const float* __restrict__ x, const uint4* __restrict__ wqkv_pk,
                                                                 const float* __restrict__ bqkv, const uint4* __restrict__ wo_pk,
                                                                 const float* __restrict__ bo, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float* __restrict__ kc,
                                                                 float* __restrict__ vc, const long long* __restrict__ pos_ptr,
                                                                 int per_row, int beams, int tiles, int P, float* __restrict__ y,
                                                                 float eps, const int32_t* __restrict__ anc, int R) {
    __shared__ __attribute__((aligned(16))) unsigned short xb[DB_ROWS * DB_BLD];
    __shared__ __attribute__((aligned(16))) float qkv[DB_ROWS * DB_QLD];
    __shared__ float ps[8][256];
    __shared__ int spos[DB_ROWS];
    __shared__ int sslot[ANC ? 8 : 1][64];                             // [wavefront]: one chunk of 64 positions' slots
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * DB_ROWS;
    const long long row0 = (long long)b * beams + j0;
    if (t < DB_ROWS) {
        int p = -1;
        if (j0 + t < beams) {
            const long long pp = pos_ptr[per_row ? row0 + t : 0];
            if (pp >= 0 && pp < P) p = (int)pp;
        }
        spos[t] = p;
    }
    __syncthreads();
    db_rows_in<512>(x, row0, spos, xb);
    __syncthreads();
    {
        floatx4 acc[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] = floatx4{0.f, 0.f, 0.f, 0.f};
        db_gemm<4, 8>(xb, DB_BLD, wqkv_pk, 4 * wave, acc);
        const int p = spos[i];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int col = 16 * (4 * wave + q) + 4 * g;               // [0,128): q   [128,256): k   [256,512): v
            const float4 bias = *reinterpret_cast<const float4*>(bqkv + col);
            const float4 v = make_float4(acc[q][0] + bias.x, acc[q][1] + bias.y, acc[q][2] + bias.z, acc[q][3] + bias.w);
            *reinterpret_cast<float4*>(qkv + i * DB_QLD + col) = v;
            if (p >= 0) {
                if (col >= 256)
                    *reinterpret_cast<float4*>(vc + (((row0 + i) * 4 + (col - 256) / 64) * P + p) * 64 + (col - 256) % 64) = v;
                else if (col >= 128)
                    *reinterpret_cast<float4*>(kc + (((row0 + i) * 4 + (col - 128) / 32) * P + p) * 32 + (col - 128) % 32) = v;
            }
        }
    }
    __syncthreads();
    // attention: wavefront w serves rows 2 w and 2 w + 1, the four heads of a row together (their loads are independent)
    float* pw = ps[wave];                                              // [head][64]: one chunk of 64 positions' probabilities
    for (int rr = 0; rr < 2; ++rr) {
        const int row = 2 * wave + rr, pos = spos[row];
        if (pos < 0) continue;                                         // (uniform over the wavefront; no workgroup barrier in this loop)
        const float* qrow = qkv + row * DB_QLD;
        const float* krow = kc + (row0 + row) * 4 * P * 32;
        const float* vrow = vc + (row0 + row) * 4 * P * 64 + 4 * i;
        float sc[4][4];                                                // [head][m]: position lane + 64 m
        int sl[ANC ? 4 : 1];                                           // ANC: the slot that holds position lane + 64 m
        if constexpr (ANC) {
            const int lo = b * beams, hi = lo + beams - 1;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int tt = lane + 64 * m;
                int s = tt < pos ? anc[(long long)tt * R + row0 + row] : lo;
                sl[m] = s < lo ? lo : (s > hi ? hi : s);
            }
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int tt = lane + 64 * m;
#pragma unroll
            for (int h = 0; h < 4; ++h) sc[h][m] = -INFINITY;
            if (tt < pos) {
                if constexpr (ANC) krow = kc + (long long)sl[m] * 4 * P * 32;
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const float4* kr = reinterpret_cast<const float4*>(krow + ((long long)h * P + tt) * 32);
                    const float* q = qrow + h * 32;
                    float acc = 0.f;
#pragma unroll
                    for (int d = 0; d < 8; ++d) {
                        const float4 kv = kr[d];
                        acc = fmaf(q[4 * d], kv.x, acc), acc = fmaf(q[4 * d + 1], kv.y, acc);
                        acc = fmaf(q[4 * d + 2], kv.z, acc), acc = fmaf(q[4 * d + 3], kv.w, acc);
                    }
                    sc[h][m] = acc * DB_SCALE;
                }
            } else if (tt == pos) {                                    // the new position: its key is in LDS
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const float* q = qrow + h * 32;
                    float acc = 0.f;
#pragma unroll
                    for (int d = 0; d < 32; ++d) acc = fmaf(q[d], q[128 + d], acc);
                    sc[h][m] = acc * DB_SCALE;
                }
            }
        }
        float ppos[4];                                                 // the new position's probability, per head
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const float mx = db_wave_max64(fmaxf(fmaxf(sc[h][0], sc[h][1]), fmaxf(sc[h][2], sc[h][3])));
            float sum = 0.f;
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                sc[h][m] = lane + 64 * m <= pos ? __expf(sc[h][m] - mx) : 0.f;
                sum += sc[h][m];
            }
            sum = 1.f / db_wave_sum64(sum);
#pragma unroll
            for (int m = 0; m < 4; ++m) sc[h][m] *= sum;
            const int mp = pos >> 6;
            const float sel = mp == 0 ? sc[h][0] : (mp == 1 ? sc[h][1] : (mp == 2 ? sc[h][2] : sc[h][3]));
            ppos[h] = __shfl(sel, pos & 63, 64);
        }
        // context: lane (g, i) = cached positions g, g + 4, ... of a chunk, value channels 4 i .. 4 i + 3 of every head; the four
        // partial sums of the lane groups meet in a fixed order, the new position (value in LDS) joins group 0 last
        float4 ca[4];
#pragma unroll
        for (int h = 0; h < 4; ++h) ca[h] = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int cnt = pos - 64 * m < 64 ? pos - 64 * m : 64;     // cached positions 64 m .. 64 m + cnt - 1 (uniform)
            if (cnt > 0) {
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int h = 0; h < 4; ++h) pw[h * 64 + lane] = sc[h][m];
                if constexpr (ANC) sslot[wave][lane] = sl[m];
                __builtin_amdgcn_wave_barrier();
#pragma unroll 2
                for (int j = g; j < cnt; j += 4) {
                    if constexpr (ANC) vrow = vc + (long long)sslot[wave][j] * 4 * P * 64 + 4 * i;
#pragma unroll
                    for (int h = 0; h < 4; ++h) {
                        const float4 v = *reinterpret_cast<const float4*>(vrow + ((long long)h * P + 64 * m + j) * 64);
                        const float p = pw[h * 64 + j];
                        ca[h].x = fmaf(p, v.x, ca[h].x), ca[h].y = fmaf(p, v.y, ca[h].y);
                        ca[h].z = fmaf(p, v.z, ca[h].z), ca[h].w = fmaf(p, v.w, ca[h].w);
                    }
                }
            }
        }
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            float c[4] = {ca[h].x, ca[h].y, ca[h].z, ca[h].w};
            if (g == 0) {
                const float4 v = *reinterpret_cast<const float4*>(qkv + row * DB_QLD + 256 + h * 64 + 4 * i);
                c[0] = fmaf(ppos[h], v.x, c[0]), c[1] = fmaf(ppos[h], v.y, c[1]);
                c[2] = fmaf(ppos[h], v.z, c[2]), c[3] = fmaf(ppos[h], v.w, c[3]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {                              // (g0 + g1) + (g2 + g3)
                c[e] += __shfl_xor(c[e], 16, 64);
                c[e] += __shfl_xor(c[e], 32, 64);
            }
            // the context, rounded once, into the operand image of the output projection (x's image is no longer read)
            if (g == 0) *reinterpret_cast<uint2*>(xb + row * DB_BLD + h * 64 + 4 * i) = db_pack4(c[0], c[1], c[2], c[3]);
        }
    }
    __syncthreads();
    floatx4 oa[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
    db_gemm<2, 8>(xb, DB_BLD, wo_pk, 2 * wave, oa);
    db_ln_store<8, 2>(oa, 2 * wave, bo, x, qkv, gamma, beta, eps, y, row0, spos);
}

// encoder-decoder attention sub-block.  256 threads, wavefront = head: its two column tiles of the q product are its head's 32
// query channels.  The walk over the pocket's keys and values is dec_tile_cross_attn_kernel's (f32 matrix cores on f32 encoder
// rows, chunks of 64 positions, running maximum and sum); the normalised context is rounded into a bf16 image.
__global__ void __launch_bounds__(256) dec_bf16_cross_attn_kernel(const float* __restrict__ y, const uint4* __restrict__ wq_pk,
                                                                  const float* __restrict__ bq, const float* __restrict__ ck,
                                                                  const float* __restrict__ cv, const unsigned char* __restrict__ pad,
                                                                  const uint4* __restrict__ wo_pk, const float* __restrict__ bo,
                                                                  const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                  int beams, int tiles, int S, float* __restrict__ z, float eps) {
    __shared__ __attribute__((aligned(16))) unsigned short yb[DB_ROWS * DB_BLD], cb[DB_ROWS * DB_BLD];
    __shared__ __attribute__((aligned(16))) float qs[DB_ROWS * DB_SLD], rs[DB_ROWS * DB_LD];
    __shared__ float pb[4][DB_ROWS * DB_PLD];
    __shared__ int live[DB_ROWS];
    const int t = threadIdx.x, h = t >> 6, lane = t & 63, i = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / tiles, j0 = (blockIdx.x % tiles) * DB_ROWS;
    const long long row0 = (long long)b * beams + j0;
    if (t < DB_ROWS) live[t] = j0 + t < beams ? 0 : -1;
    __syncthreads();
    db_rows_in<256>(y, row0, live, yb);
    __syncthreads();
    {
        floatx4 qa[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
        db_gemm<2, 8>(yb, DB_BLD, wq_pk, 2 * h, qa);
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int col = 16 * (2 * h + u) + 4 * g;
            const float4 bias = *reinterpret_cast<const float4*>(bq + col);
            *reinterpret_cast<float4*>(qs + i * DB_SLD + col) =
                make_float4(qa[u][0] + bias.x, qa[u][1] + bias.y, qa[u][2] + bias.z, qa[u][3] + bias.w);
        }
    }
    __syncthreads();
    const float* kh = ck + ((long long)b * 4 + h) * 32 * (long long)S;
    const float* vh = cv + ((long long)b * 4 + h) * (long long)S * 64 + 4 * i;
    const unsigned char* padb = pad + (long long)b * S;
    float qf[8];
#pragma unroll
    for (int kk = 0; kk < 8; ++kk) qf[kk] = qs[i * DB_SLD + h * 32 + 4 * kk + g];
    float m[4], l[4];
    floatx4 ca[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) m[r] = -INFINITY, l[r] = 0.f, ca[r] = floatx4{0.f, 0.f, 0.f, 0.f};
    float* pw = pb[h];
    for (int s0 = 0; s0 < S; s0 += DB_CHUNK) {
        // the chunk's keys and values are requested together: one memory latency per chunk, not one per product
        float kf[8][4];
        float4 vf[DB_CHUNK / 4];
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int s = s0 + 16 * u + i;
                kf[kk][u] = kh[(long long)(4 * kk + g) * S + (s < S ? s : S - 1)];
            }
#pragma unroll
        for (int kk = 0; kk < DB_CHUNK / 4; ++kk) {
            const int s = s0 + 4 * kk + g;
            vf[kk] = *reinterpret_cast<const float4*>(vh + (long long)(s < S ? s : S - 1) * 64);
        }
        __builtin_amdgcn_sched_barrier(0);
        floatx4 sa[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) sa[u] = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 8; ++kk)
#pragma unroll
            for (int u = 0; u < 4; ++u) sa[u] = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[kk], kf[kk][u], sa[u], 0, 0, 0);
        // sa[u][r]: row 4 g + r, position s0 + 16 u + i
        float cm[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = s0 + 16 * u + i;
            const bool in = s < S;
            const bool pd = in && padb[s] != 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = in ? (pd ? -1e9f : sa[u][r] * DB_SCALE) : -INFINITY;
                sa[u][r] = v;
                cm[r] = fmaxf(cm[r], v);
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float c = cm[r];
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) c = fmaxf(c, __shfl_xor(c, o, 64));       // over the 16 lanes of the row's group
            const float mn = fmaxf(m[r], c), alpha = __expf(m[r] - mn);
            float sum = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float p = __expf(sa[u][r] - mn);
                pw[(4 * g + r) * DB_PLD + 16 * u + i] = p;
                sum += p;
            }
#pragma unroll
            for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
            l[r] = fmaf(l[r], alpha, sum);
            m[r] = mn;
#pragma unroll
            for (int u = 0; u < 4; ++u) ca[u][r] *= alpha;
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int kk = 0; kk < DB_CHUNK / 4; ++kk) {
            const float4 v = vf[kk];
            const float p = pw[i * DB_PLD + 4 * kk + g];
            ca[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, v.x, ca[0], 0, 0, 0);
            ca[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, v.y, ca[1], 0, 0, 0);
            ca[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, v.z, ca[2], 0, 0, 0);
            ca[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(p, v.w, ca[3], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                                      // ca[u][r]: row 4 g + r, channel h * 64 + 4 i + u
        const float inv = 1.f / l[r];
        *reinterpret_cast<uint2*>(cb + (4 * g + r) * DB_BLD + h * 64 + 4 * i) =
            db_pack4(ca[0][r] * inv, ca[1][r] * inv, ca[2][r] * inv, ca[3][r] * inv);
    }
    __syncthreads();
    floatx4 oa[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) oa[u] = floatx4{0.f, 0.f, 0.f, 0.f};
    db_gemm<4, 8>(cb, DB_BLD, wo_pk, 4 * h, oa);
    db_ln_store<4, 4>(oa, 4 * h, bo, y, rs, gamma, beta, eps, z, row0, live);
}

// feed-forward sub-block.  512 threads, tiles of 16 consecutive rows of the whole batch.  A wavefront makes 128 hidden channels
// (two passes of four column tiles), ReLU, rounds them into the image [16][1024]; the second product walks all 1024 of them with
// one accumulator per output: a sum over k in the instruction's order, k blocks ascending.
__global__ void __launch_bounds__(512) dec_bf16_ffn_kernel(const float* __restrict__ z, const uint4* __restrict__ w1_pk,
                                                           const float* __restrict__ b1, const uint4* __restrict__ w2_pk,
                                                           const float* __restrict__ b2, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int R, float* __restrict__ out, float eps) {
    __shared__ __attribute__((aligned(16))) unsigned short zb[DB_ROWS * DB_BLD], hb[DB_ROWS * DB_HLD];
    __shared__ __attribute__((aligned(16))) float rs[DB_ROWS * DB_LD];
    __shared__ int live[DB_ROWS];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, i = lane & 15, g = lane >> 4;
    const long long row0 = (long long)blockIdx.x * DB_ROWS;
    if (t < DB_ROWS) live[t] = row0 + t < R ? 0 : -1;
    __syncthreads();
    db_rows_in<512>(z, row0, live, zb);
    __syncthreads();
    for (int pass = 0; pass < 2; ++pass) {
        floatx4 ha[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) ha[u] = floatx4{0.f, 0.f, 0.f, 0.f};
        const int tile0 = 8 * wave + 4 * pass;
        db_gemm<4, 8>(zb, DB_BLD, w1_pk, tile0, ha);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int col = 16 * (tile0 + u) + 4 * g;
            const float4 bias = *reinterpret_cast<const float4*>(b1 + col);
            *reinterpret_cast<uint2*>(hb + i * DB_HLD + col) =
                db_pack4(fmaxf(ha[u][0] + bias.x, 0.f), fmaxf(ha[u][1] + bias.y, 0.f), fmaxf(ha[u][2] + bias.z, 0.f),
                         fmaxf(ha[u][3] + bias.w, 0.f));
        }
    }
    __syncthreads();
    floatx4 oa[2] = {floatx4{0.f, 0.f, 0.f, 0.f}, floatx4{0.f, 0.f, 0.f, 0.f}};
    db_gemm<2, 32>(hb, DB_HLD, w2_pk, 2 * wave, oa);
    db_ln_store<8, 2>(oa, 2 * wave, b2, z, rs, gamma, beta, eps, out, row0, live);
}

}  // namespace
#endif  // SINGA_EMUL

extern "C" int singa_dec_bf16_pack(const float* w_t, int K, int N, unsigned short* packed, void* stream) {
    if (!w_t || !packed) return singa_detail_fail(SINGA_E_NULL, "dec_bf16_pack: null pointer");
    if (K <= 0 || N <= 0 || K % 32 || N % 16 || ((uintptr_t)packed & 15))
        return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_pack: K a multiple of 32, N a multiple of 16, a 16-byte aligned output");
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_pack: not part of the emulation build");
#else
    const long long frags = (long long)(N / 16) * (K / 32) * 64;
    hipLaunchKernelGGL(dec_bf16_pack_kernel, dim3((unsigned)((frags + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_t, K, N,
                       reinterpret_cast<uint4*>(packed));
    return singa_detail_check_launch("dec_bf16_pack");
#endif
}

extern "C" int singa_dec_bf16_tile_self_attn(const float* x, const unsigned short* wqkv_pk, const float* bqkv,
                                             const unsigned short* wo_pk, const float* bo, const float* gamma, const float* beta,
                                             float* k_cache, float* v_cache, const long long* pos, int per_row, int R, int beams, int P,
                                             float* y, float eps, const int32_t* anc, void* stream) {
    if (!x || !wqkv_pk || !bqkv || !wo_pk || !bo || !gamma || !beta || !k_cache || !v_cache || !pos || !y)
        return singa_detail_fail(SINGA_E_NULL, "dec_bf16_tile_self_attn: null pointer");
    if (P <= 0 || P > 256) return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_self_attn: built for at most 256 cached positions");
    if (R < 0 || beams <= 0 || R % beams) return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_self_attn: rows must be proteins x beams");
    if (anc && per_row)
        return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_self_attn: an ancestry table goes with one position for all rows (per_row = 0)");
    if (((uintptr_t)wqkv_pk & 15) || ((uintptr_t)wo_pk & 15))
        return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_self_attn: packed weights must be 16-byte aligned");
    if (R == 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_self_attn: not part of the emulation build");
#else
    const int tiles = (beams + DB_ROWS - 1) / DB_ROWS;
    const dim3 grid((unsigned)(R / beams * tiles));
    const uint4 *wa = reinterpret_cast<const uint4*>(wqkv_pk), *wb = reinterpret_cast<const uint4*>(wo_pk);
    if (anc)
        hipLaunchKernelGGL(dec_bf16_self_attn_kernel<true>, grid, dim3(512), 0, (hipStream_t)stream, x, wa, bqkv, wb, bo, gamma, beta,
                           k_cache, v_cache, pos, 0, beams, tiles, P, y, eps, anc, R);
    else
        hipLaunchKernelGGL(dec_bf16_self_attn_kernel<false>, grid, dim3(512), 0, (hipStream_t)stream, x, wa, bqkv, wb, bo, gamma, beta,
                           k_cache, v_cache, pos, per_row, beams, tiles, P, y, eps, nullptr, R);
    return singa_detail_check_launch("dec_bf16_tile_self_attn");
#endif
}

extern "C" int singa_dec_bf16_tile_cross_attn(const float* y, const unsigned short* wq_pk, const float* bq, const float* ck,
                                              const float* cv, const unsigned char* pad, const unsigned short* wo_pk, const float* bo,
                                              const float* gamma, const float* beta, int R, int beams, int S, float* z, float eps,
                                              void* stream) {
    if (!y || !wq_pk || !bq || !ck || !cv || !pad || !wo_pk || !bo || !gamma || !beta || !z)
        return singa_detail_fail(SINGA_E_NULL, "dec_bf16_tile_cross_attn: null pointer");
    if (S <= 0) return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_cross_attn: at least one encoder position");
    if (R < 0 || beams <= 0 || R % beams) return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_cross_attn: rows must be proteins x beams");
    if (((uintptr_t)wq_pk & 15) || ((uintptr_t)wo_pk & 15))
        return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_cross_attn: packed weights must be 16-byte aligned");
    if (R == 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_cross_attn: not part of the emulation build");
#else
    const int tiles = (beams + DB_ROWS - 1) / DB_ROWS;
    hipLaunchKernelGGL(dec_bf16_cross_attn_kernel, dim3((unsigned)(R / beams * tiles)), dim3(256), 0, (hipStream_t)stream, y,
                       reinterpret_cast<const uint4*>(wq_pk), bq, ck, cv, pad, reinterpret_cast<const uint4*>(wo_pk), bo, gamma, beta,
                       beams, tiles, S, z, eps);
    return singa_detail_check_launch("dec_bf16_tile_cross_attn");
#endif
}

extern "C" int singa_dec_bf16_tile_ffn(const float* z, const unsigned short* w1_pk, const float* b1, const unsigned short* w2_pk,
                                       const float* b2, const float* gamma, const float* beta, int R, float* out, float eps,
                                       void* stream) {
    if (!z || !w1_pk || !b1 || !w2_pk || !b2 || !gamma || !beta || !out)
        return singa_detail_fail(SINGA_E_NULL, "dec_bf16_tile_ffn: null pointer");
    if (R < 0) return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_ffn: rows must not be negative");
    if (((uintptr_t)w1_pk & 15) || ((uintptr_t)w2_pk & 15))
        return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_ffn: packed weights must be 16-byte aligned");
    if (R == 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "dec_bf16_tile_ffn: not part of the emulation build");
#else
    hipLaunchKernelGGL(dec_bf16_ffn_kernel, dim3((unsigned)((R + DB_ROWS - 1) / DB_ROWS)), dim3(512), 0, (hipStream_t)stream, z,
                       reinterpret_cast<const uint4*>(w1_pk), b1, reinterpret_cast<const uint4*>(w2_pk), b2, gamma, beta, R, out, eps);
    return singa_detail_check_launch("dec_bf16_tile_ffn");
#endif
}
