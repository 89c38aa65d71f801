// k19b: the dense attention core (k19, singa_hip.hip) with bf16 operands on the matrix cores (include/singa_hip_attn_bf16.h).  A
// translation unit of its own, linked into libsinga_hip.so; it reports errors through the two hooks singa_hip.hip exports
// (hidden: not part of any ABI).  Split, layouts, masks, tile maps, grids and outputs are k19's; what differs is the arithmetic
// of the five kinds of product and how their operands are put together.
//
// v_mfma_f32_32x32x16_bf16: lane l gives row / column l % 32 and the 8 reduction indices 8 h .. 8 h + 7 (h = l / 32) of the
// instruction's 16, for both operands; the accumulator has the map of 32x32x2f32 (register r of half h: row 8 (r/4) + 4 h + r%4,
// column l % 32).
//
// Score products (s^T = K Q^T, and s = Q K^T of the dK / dV pass).  A lane holds the 16 features 16 h .. 16 h + 15 of its q or k
// row, one contiguous 64-byte read as in k19, and packs them pairwise (v_cvt_pk_bf16_f32) into two operands: reduction index j
// of half h of MFMA `step` is feature 16 h + 8 step + j, for both operands alike.  Two MFMAs for DK = 32.  The three kernels
// issue the same two instructions on the same rounded values in the same order, so the backward's scores are the forward's.
// dP = V dO^T over 64 channels: the same with channel 32 h + 8 step + j, four MFMAs.
//
// Chaining (k15e's head describes the same thing for the edge MLPs).  Registers 8 step .. 8 step + 7 of a score-shaped
// accumulator hold, in half h, the keys (queries in the dK / dV pass) 16 step + 8 (j/4) + 4 h + j%4 of the tile, j = 0 .. 7.
// Rounded and packed they ARE the B operand of MFMA `step` of the product that follows (ctx^T += V^T P^T, dQ^T += K^T dS^T,
// dV^T += dO^T P, dK^T += Q^T dS), which fixes the meaning of its reduction index; the A operand of lane i is then column i
// (and i + 32 for the 64 value channels) of the 8 rows in that order - the strided read k19 makes, 32 lanes a 128-byte run -
// packed eight to an operand.  Two MFMAs per 32 output channels.  No LDS anywhere: the dK / dV pass, which in k19 stages the
// query rows in LDS to read them in two layouts, reads them twice from global memory (row form one tile ahead, column form at the
// head of the tile) and takes the per-query statistics from the lane that loaded them with a lane permute.
//
// f32: accumulators, scale, mask value, maximum, exp, the row sum (of the UNROUNDED exp), the rescale, D = rowsum(dO ctx) (of
// the unrounded values), dS before it becomes an operand, every output.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/singa_hip.h"
#include "../../include/singa_hip_attn_bf16.h"

int singa_detail_fail(int code, const char* msg);
int singa_detail_check_launch(const char* what);

#ifndef SINGA_EMUL      // (bf16 matrix cores, lane permutes: no stand-in in the CPU emulation build of tests/emul)
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bfx2 __attribute__((ext_vector_type(2)));
typedef __bf16 bfx8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ unsigned ab_pack2(float x, float y) {       // bf16(x) | bf16(y) << 16, round to nearest even
    const f32x2 v = {x, y};
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bfx2));
}
__device__ __forceinline__ bfx8 ab_frag(float a, float b, float c, float d, float e, float f, float g, float h) {
    return __builtin_bit_cast(bfx8, make_uint4(ab_pack2(a, b), ab_pack2(c, d), ab_pack2(e, f), ab_pack2(g, h)));
}
__device__ __forceinline__ bfx8 ab_frag(const float4& a, const float4& b) { return ab_frag(a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w); }
// registers 8 step .. 8 step + 7 of an accumulator as the B operand of MFMA `step` of the product it is chained into
__device__ __forceinline__ bfx8 ab_frag(const f32x16& c, int step) {
    return ab_frag(c[8 * step], c[8 * step + 1], c[8 * step + 2], c[8 * step + 3], c[8 * step + 4], c[8 * step + 5], c[8 * step + 6],
                   c[8 * step + 7]);
}
// elements first + st * (8 step + j), j = 0 .. 7, of the column reads made in the accumulator's row order
template <int N>
__device__ __forceinline__ bfx8 ab_frag(const float (&v)[N], int step, int st, int first) {
    const int o = first + 8 * st * step;
    return ab_frag(v[o], v[o + st], v[o + 2 * st], v[o + 3 * st], v[o + 4 * st], v[o + 5 * st], v[o + 6 * st], v[o + 7 * st]);
}
__device__ __forceinline__ f32x16 ab_mfma(const bfx8& a, const bfx8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ f32x16 ab_zero() {
    f32x16 c;
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
    return c;
}
__device__ __forceinline__ void ab_store16(float* dst, const f32x16& c, float f) {     // channels 8 blk + 4 half + 0 .. 3 at dst + 8 blk
#pragma unroll
    for (int blk = 0; blk < 4; ++blk)
        *reinterpret_cast<float4*>(dst + 8 * blk) = make_float4(c[4 * blk] * f, c[4 * blk + 1] * f, c[4 * blk + 2] * f, c[4 * blk + 3] * f);
}

// ---- k19's small helpers, restated (singa_hip.hip keeps its own inside its unnamed namespace): where the rows of one (batch,
// head) sit, the 16 mask bytes of a lane and tile as four clamped 4-byte loads, the scalar walk over a row of the tile map, and
// the XCD-contiguous order of the workgroups.  See there for the reasons.
struct AbLay {
    long long qb, kb, vb, ob;      // float offset of row 0 in q / k / v / ctx-like tensors
    int qs, ks, vs, os;            // floats between consecutive rows
};
struct AbPitch {
    int q, k, v;
};
__device__ __forceinline__ AbLay ab_lay(int bh, int heads, int T, int S, int tm, AbPitch ld) {
    AbLay a;
    if (tm) {
        const int b = bh / heads, h = bh - b * heads;
        a.qb = (long long)b * T * ld.q + h * 32; a.kb = (long long)b * S * ld.k + h * 32;
        a.vb = (long long)b * S * ld.v + h * 64; a.ob = ((long long)b * T * heads + h) * 64;
        a.qs = ld.q; a.ks = ld.k; a.vs = ld.v; a.os = heads * 64;
    } else {
        a.qb = (long long)bh * T * 32; a.kb = (long long)bh * S * 32; a.vb = (long long)bh * S * 64; a.ob = (long long)bh * T * 64;
        a.qs = 32; a.ks = 32; a.vs = 64; a.os = 64;
    }
    return a;
}
__device__ __forceinline__ void ab_mask_fetch(const unsigned char* __restrict__ mrow, int k0, int half, int S, unsigned (&w)[4]) {
    if (S >= 4) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int kr = k0 + 8 * g + 4 * half, ks = kr < S - 4 ? kr : S - 4;
            __builtin_memcpy(&w[g], mrow + ks, 4);
        }
    } else {
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
            unsigned v = 0;
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int kr = k0 + 8 * g + 4 * half + j;
                v |= (unsigned)mrow[kr < S ? kr : S - 1] << (8 * j);
            }
            w[g] = v;
        }
    }
}
__device__ __forceinline__ bool ab_mask_bit(const unsigned (&w)[4], int k0, int half, int S, int r) {
    const int kr = k0 + 8 * (r >> 2) + 4 * half;
    const int sh = 8 * ((S >= 4 && kr > S - 4 ? kr - (S - 4) : 0) + (r & 3));
    return (sh < 32) & (((w[r >> 2] >> (sh & 31)) & 0xffu) != 0u);
}
struct AbWalk {
    const unsigned* w;
    int nt, base;
    unsigned cur;
    __device__ __forceinline__ unsigned word(int b0) const {
        const unsigned x = (unsigned)__builtin_amdgcn_readfirstlane((int)w[b0 >> 5]);
        return nt - b0 < 32 ? x & ((1u << (nt - b0)) - 1u) : x;
    }
    __device__ __forceinline__ void start(const unsigned* words, int ntiles) { w = words, nt = ntiles, base = 0, cur = word(0); }
    __device__ __forceinline__ int next() {
        while (cur == 0u && base + 32 < nt) base += 32, cur = word(base);
        if (cur == 0u) return nt;
        const int t = base + __builtin_ctz(cur);
        cur &= cur - 1u;
        return t;
    }
};
__device__ __forceinline__ int ab_xcd_range_id(int vb, int n8) { return (vb & 7) * (n8 >> 3) + (vb >> 3); }

// ---- forward: a wavefront = 32 queries of one (batch, head), lane = query.  2 + 4 MFMAs per tile.
template <bool TILED>
__global__ void __launch_bounds__(256) attn_bf16_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                            const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                            long long msb, long long mst, float* __restrict__ ctx, float* __restrict__ lse,
                                                            int BH, int T, int S, int heads, int tm, float scale, AbPitch ld,
                                                            const unsigned* __restrict__ tiles) {
    const int lane = threadIdx.x & 63, i = lane & 31, half = lane >> 5;
    const int qtiles = (T + 31) / 32;
    const long long w = (long long)ab_xcd_range_id((int)blockIdx.x, (int)gridDim.x) * 4 + (threadIdx.x >> 6);
    if (w >= (long long)BH * qtiles) return;
    const int bh = (int)(w / qtiles), qt = (int)(w - (long long)bh * qtiles);
    const int tq = qt * 32 + i, tqc = tq < T ? tq : T - 1;
    const AbLay A = ab_lay(bh, heads, T, S, tm, ld);
    bfx8 qf[2];
    {
        const float4* qr = reinterpret_cast<const float4*>(q + A.qb + (long long)tqc * A.qs + 16 * half);
        qf[0] = ab_frag(qr[0], qr[1]), qf[1] = ab_frag(qr[2], qr[3]);
    }
    const unsigned char* mrow = mask + (long long)(bh / heads) * msb + (long long)tqc * mst;
    const float* kb = k + A.kb;
    const float* vb = v + A.vb;
    f32x16 o0 = ab_zero(), o1 = ab_zero();
    float mrun = -INFINITY, lrun = 0.f;
    float4 knext[4];
    unsigned mnext[4];
    auto fetch_k = [&](int k0) __attribute__((always_inline)) {      // the next tile's key rows (f32: packing would wait for them) and mask words
        const int ka = k0 + i < S ? k0 + i : S - 1;
#pragma unroll
        for (int m4 = 0; m4 < 4; ++m4) knext[m4] = *reinterpret_cast<const float4*>(kb + (long long)ka * A.ks + 16 * half + 4 * m4);
        ab_mask_fetch(mrow, k0, half, S, mnext);
    };
    auto tile = [&](int k0, int knx) __attribute__((always_inline)) {
        float vreg[32];
        unsigned mb[4];
        const bfx8 kf0 = ab_frag(knext[0], knext[1]), kf1 = ab_frag(knext[2], knext[3]);
#pragma unroll
        for (int g = 0; g < 4; ++g) mb[g] = mnext[g];
#pragma unroll
        for (int s = 0; s < 16; ++s) {                 // v[key of accumulator register s][i], [i + 32]
            const int ks = k0 + 8 * (s >> 2) + 4 * half + (s & 3);
            const float* vr = vb + (long long)(ks < S ? ks : S - 1) * A.vs + i;
            vreg[2 * s] = vr[0], vreg[2 * s + 1] = vr[32];
        }
        fetch_k(knx);                                  // unconditional: the last tile re-reads itself (k19's note)
        f32x16 sc = ab_mfma(kf0, qf[0], ab_zero());
        sc = ab_mfma(kf1, qf[1], sc);
        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = k0 + 8 * (r >> 2) + 4 * half + (r & 3);
            const float vin = ab_mask_bit(mb, k0, half, S, r) ? -1e9f : sc[r] * scale;
            const float val = kr < S ? vin : -INFINITY;
            sc[r] = val;
            mx = fmaxf(mx, val);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(mrun, mx);
        const float alpha = __expf(mrun - mnew);
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            sc[r] = __expf(sc[r] - mnew);
            psum += sc[r];                             // the row sum takes the unrounded value
        }
        lrun = lrun * alpha + psum;
        mrun = mnew;
#pragma unroll
        for (int r = 0; r < 16; ++r) o0[r] *= alpha, o1[r] *= alpha;
#pragma unroll
        for (int step = 0; step < 2; ++step) {
            const bfx8 pf = ab_frag(sc, step);
            o0 = ab_mfma(ab_frag(vreg, step, 2, 0), pf, o0);
            o1 = ab_mfma(ab_frag(vreg, step, 2, 1), pf, o1);
        }
    };
    if constexpr (TILED) {                             // a skipped tile adds exact zeros (include/singa_hip_attn_tiles.h)
        const int ktiles = (S + 31) / 32;
        AbWalk walk;
        walk.start(tiles + ((long long)(bh / heads) * qtiles + qt) * ((ktiles + 31) / 32), ktiles);
        int kt = walk.next();
        fetch_k(32 * (kt < ktiles ? kt : 0));
        while (kt < ktiles) {
            const int nx = walk.next();
            tile(32 * kt, 32 * (nx < ktiles ? nx : kt));
            kt = nx;
        }
    } else {
        fetch_k(0);
        for (int k0 = 0; k0 < S; k0 += 32) tile(k0, k0 + 32 < S ? k0 + 32 : k0);
    }
    lrun += __shfl_xor(lrun, 32, 64);
    if (tq < T) {
        const float inv = 1.f / lrun;
        float* dst = ctx + A.ob + (long long)tq * A.os + 4 * half;
        ab_store16(dst, o0, inv);
        ab_store16(dst + 32, o1, inv);
        if (half == 0) {
            lse[((long long)bh * T + tq) * 2] = mrun;
            lse[((long long)bh * T + tq) * 2 + 1] = inv;
        }
    }
}

// ---- dQ pass: the forward's split.  2 (S) + 4 (dP^T = V dO^T) + 2 (dQ^T += K^T dS^T) MFMAs per tile; writes D for the dK / dV pass.
template <bool TILED>
__global__ void __launch_bounds__(256) attn_bf16_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                               const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                               long long msb, long long mst, const float* __restrict__ ctx,
                                                               const float* __restrict__ lse, const float* __restrict__ go,
                                                               float* __restrict__ gq, float* __restrict__ dsum, int BH, int T, int S,
                                                               int heads, int tm, float scale, AbPitch ld,
                                                               const unsigned* __restrict__ tiles) {
    const int lane = threadIdx.x & 63, i = lane & 31, half = lane >> 5;
    const int qtiles = (T + 31) / 32;
    const long long w = (long long)ab_xcd_range_id((int)blockIdx.x, (int)gridDim.x) * 4 + (threadIdx.x >> 6);
    if (w >= (long long)BH * qtiles) return;
    const int bh = (int)(w / qtiles), qt = (int)(w - (long long)bh * qtiles);
    const int tq = qt * 32 + i, tqc = tq < T ? tq : T - 1;
    const long long qrow = (long long)bh * T + tqc;
    const AbLay A = ab_lay(bh, heads, T, S, tm, ld);
    bfx8 qf[2], gof[4];
    {
        const float4* qr = reinterpret_cast<const float4*>(q + A.qb + (long long)tqc * A.qs + 16 * half);
        qf[0] = ab_frag(qr[0], qr[1]), qf[1] = ab_frag(qr[2], qr[3]);
    }
    float dpart = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const float4* gr = reinterpret_cast<const float4*>(go + A.ob + (long long)tqc * A.os + 32 * half + 8 * s);
        const float4* cr = reinterpret_cast<const float4*>(ctx + A.ob + (long long)tqc * A.os + 32 * half + 8 * s);
        const float4 g0 = gr[0], g1 = gr[1], c0 = cr[0], c1 = cr[1];
        gof[s] = ab_frag(g0, g1);
        dpart += (g0.x * c0.x + g0.y * c0.y) + (g0.z * c0.z + g0.w * c0.w);          // D: the unrounded values, k19's order
        dpart += (g1.x * c1.x + g1.y * c1.y) + (g1.z * c1.z + g1.w * c1.w);
    }
    const float dq_i = dpart + __shfl_xor(dpart, 32, 64);
    const float m_i = lse[qrow * 2], linv_i = lse[qrow * 2 + 1];
    if (half == 0 && tq < T) dsum[qrow] = dq_i;
    const unsigned char* mrow = mask + (long long)(bh / heads) * msb + (long long)tqc * mst;
    const float* kb = k + A.kb;
    const float* vb = v + A.vb;
    f32x16 dq = ab_zero();
    float4 kn[4], vn[8];
    unsigned mnext[4];
    auto fetch = [&](int k0) __attribute__((always_inline)) {
        const int ka = k0 + i < S ? k0 + i : S - 1;
#pragma unroll
        for (int m4 = 0; m4 < 4; ++m4) kn[m4] = *reinterpret_cast<const float4*>(kb + (long long)ka * A.ks + 16 * half + 4 * m4);
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4) vn[m4] = *reinterpret_cast<const float4*>(vb + (long long)ka * A.vs + 32 * half + 4 * m4);
        ab_mask_fetch(mrow, k0, half, S, mnext);
    };
    auto tile = [&](int k0, int knx) __attribute__((always_inline)) {
        float kd[16];
        unsigned mb[4];
        bfx8 vf[4];
        const bfx8 kf0 = ab_frag(kn[0], kn[1]), kf1 = ab_frag(kn[2], kn[3]);
#pragma unroll
        for (int s = 0; s < 4; ++s) vf[s] = ab_frag(vn[2 * s], vn[2 * s + 1]);
#pragma unroll
        for (int g = 0; g < 4; ++g) mb[g] = mnext[g];
#pragma unroll
        for (int s = 0; s < 16; ++s) {                 // k[key of accumulator register s][i]: the A operands of the dQ product
            const int ks = k0 + 8 * (s >> 2) + 4 * half + (s & 3);
            kd[s] = kb[(long long)(ks < S ? ks : S - 1) * A.ks + i];
        }
        fetch(knx);
        f32x16 sc = ab_mfma(kf0, qf[0], ab_zero());    // the forward's two instructions on the forward's operands
        sc = ab_mfma(kf1, qf[1], sc);
        f32x16 dp = ab_zero();
#pragma unroll
        for (int s = 0; s < 4; ++s) dp = ab_mfma(vf[s], gof[s], dp);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = k0 + 8 * (r >> 2) + 4 * half + (r & 3);
            const bool in = kr < S;
            const bool msk = in & ab_mask_bit(mb, k0, half, S, r);
            const float val = msk ? -1e9f : sc[r] * scale;
            const float pr = __expf((in ? val : -INFINITY) - m_i) * linv_i;
            sc[r] = msk ? 0.f : pr * (dp[r] - dq_i) * scale;        // dS^T, f32 until it is packed
        }
#pragma unroll
        for (int step = 0; step < 2; ++step) dq = ab_mfma(ab_frag(kd, step, 1, 0), ab_frag(sc, step), dq);
    };
    if constexpr (TILED) {
        const int ktiles = (S + 31) / 32;
        AbWalk walk;
        walk.start(tiles + ((long long)(bh / heads) * qtiles + qt) * ((ktiles + 31) / 32), ktiles);
        int kt = walk.next();
        fetch(32 * (kt < ktiles ? kt : 0));
        while (kt < ktiles) {
            const int nx = walk.next();
            tile(32 * kt, 32 * (nx < ktiles ? nx : kt));
            kt = nx;
        }
    } else {
        fetch(0);
        for (int k0 = 0; k0 < S; k0 += 32) tile(k0, k0 + 32 < S ? k0 + 32 : k0);
    }
    if (tq < T) ab_store16(gq + A.qb + (long long)tq * A.qs + 4 * half, dq, 1.f);
}

// ---- dK / dV pass: a wavefront = 32 keys, lane = key.  2 (S) + 4 (dP) + 4 (dV^T += dO^T P) + 2 (dK^T += Q^T dS) MFMAs per tile.
// WPB wavefronts per workgroup, one in the tiled form (k19's note: wavefronts of unequal length share nothing).
template <bool TILED, int WPB>
__global__ void __launch_bounds__(64 * WPB) attn_bf16_bwd_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const float* __restrict__ v, const unsigned char* __restrict__ mask,
                                                                     long long msb, long long mst, const float* __restrict__ lse,
                                                                     const float* __restrict__ dsum, const float* __restrict__ go,
                                                                     float* __restrict__ gk, float* __restrict__ gv, int BH, int T, int S,
                                                                     int heads, int tm, float scale, AbPitch ld,
                                                                     const unsigned* __restrict__ tiles) {
    const int lane = threadIdx.x & 63, i = lane & 31, half = lane >> 5;
    const int ktiles = (S + 31) / 32;
    const long long w = (long long)ab_xcd_range_id((int)blockIdx.x, (int)gridDim.x) * WPB + (threadIdx.x >> 6);
    if (w >= (long long)BH * ktiles) return;
    const int bh = (int)(w / ktiles), kt = (int)(w - (long long)bh * ktiles);
    const int key = kt * 32 + i, keyc = key < S ? key : S - 1;
    const bool kin = key < S;
    const AbLay A = ab_lay(bh, heads, T, S, tm, ld);
    bfx8 kf[2], vf[4];
    {
        const float4* kr = reinterpret_cast<const float4*>(k + A.kb + (long long)keyc * A.ks + 16 * half);
        const float4* vr = reinterpret_cast<const float4*>(v + A.vb + (long long)keyc * A.vs + 32 * half);
        kf[0] = ab_frag(kr[0], kr[1]), kf[1] = ab_frag(kr[2], kr[3]);
#pragma unroll
        for (int s = 0; s < 4; ++s) vf[s] = ab_frag(vr[2 * s], vr[2 * s + 1]);
    }
    const unsigned char* mb = mask + (long long)(bh / heads) * msb + keyc;
    const float* qb = q + A.qb;
    const float* gob = go + A.ob;
    f32x16 dk = ab_zero(), dv0 = ab_zero(), dv1 = ab_zero();
    // one tile ahead: the row form of the tile's queries (lane = query: 16 features of q, 32 channels of dO), that query's
    // (row maximum, 1 / row sum, D), and the 16 mask bytes of this lane's key
    float4 qn[4], gn[8];
    float sn0 = 0.f, sn1 = 0.f, sn2 = 0.f;
    unsigned char mraw[16];
    auto fetch = [&](int t0) __attribute__((always_inline)) {
        const int ta = t0 + i < T ? t0 + i : T - 1;
        const float4* qr = reinterpret_cast<const float4*>(qb + (long long)ta * A.qs + 16 * half);
        const float4* gr = reinterpret_cast<const float4*>(gob + (long long)ta * A.os + 32 * half);
#pragma unroll
        for (int m4 = 0; m4 < 4; ++m4) qn[m4] = qr[m4];
#pragma unroll
        for (int m4 = 0; m4 < 8; ++m4) gn[m4] = gr[m4];
        const float2 st = *reinterpret_cast<const float2*>(lse + ((long long)bh * T + ta) * 2);
        sn0 = st.x, sn1 = st.y, sn2 = dsum[(long long)bh * T + ta];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tr = t0 + 8 * (r >> 2) + 4 * half + (r & 3);
            mraw[r] = mb[(long long)(tr < T ? tr : T - 1) * mst];
        }
    };
    auto tile = [&](int t0, int tnext) __attribute__((always_inline)) {
        float qc[16], gc[32];
        bfx8 gf[4];
        const bfx8 qf0 = ab_frag(qn[0], qn[1]), qf1 = ab_frag(qn[2], qn[3]);
#pragma unroll
        for (int s = 0; s < 4; ++s) gf[s] = ab_frag(gn[2 * s], gn[2 * s + 1]);
        const float s0 = sn0, s1 = sn1, s2 = sn2;
        unsigned mbits = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) mbits |= (mraw[r] != 0 ? 1u : 0u) << r;
#pragma unroll
        for (int s = 0; s < 16; ++s) {                 // the column form: q[query of accumulator register s][i], dO[..][i], [i + 32]
            const int tr = t0 + 8 * (s >> 2) + 4 * half + (s & 3), tc = tr < T ? tr : T - 1;
            qc[s] = qb[(long long)tc * A.qs + i];
            const float* gr = gob + (long long)tc * A.os + i;
            gc[2 * s] = gr[0], gc[2 * s + 1] = gr[32];
        }
        fetch(tnext);                                  // unconditional: the last tile re-reads its own rows
        f32x16 sc = ab_mfma(qf0, kf[0], ab_zero());    // s[query x key]: the forward's products, operands exchanged
        sc = ab_mfma(qf1, kf[1], sc);
        f32x16 dp = ab_zero();
#pragma unroll
        for (int s = 0; s < 4; ++s) dp = ab_mfma(gf[s], vf[s], dp);
        f32x16 pr;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int tl = 8 * (r >> 2) + 4 * half + (r & 3);          // query of register r inside the tile: its statistics are lane tl's
            const float m_t = __shfl(s0, tl, 64), linv_t = __shfl(s1, tl, 64), d_t = __shfl(s2, tl, 64);
            const bool in = t0 + tl < T && kin;
            const bool msk = in && ((mbits >> r) & 1u);
            const float val = msk ? -1e9f : sc[r] * scale;
            const float p = in ? __expf(val - m_t) * linv_t : 0.f;
            pr[r] = p;
            sc[r] = msk ? 0.f : p * (dp[r] - d_t) * scale;              // dS, f32 until it is packed
        }
#pragma unroll
        for (int step = 0; step < 2; ++step) {
            const bfx8 pf = ab_frag(pr, step);
            dv0 = ab_mfma(ab_frag(gc, step, 2, 0), pf, dv0);
            dv1 = ab_mfma(ab_frag(gc, step, 2, 1), pf, dv1);
            dk = ab_mfma(ab_frag(qc, step, 1, 0), ab_frag(sc, step), dk);
        }
    };
    if constexpr (TILED) {                             // a key tile without a computed pair stores the zeros it starts from
        const int qtiles = (T + 31) / 32;
        AbWalk walk;
        walk.start(tiles + ((long long)(bh / heads) * ktiles + kt) * ((qtiles + 31) / 32), qtiles);
        int qt = walk.next();
        if (qt < qtiles) fetch(32 * qt);
        while (qt < qtiles) {
            const int nx = walk.next();
            tile(32 * qt, 32 * (nx < qtiles ? nx : qt));
            qt = nx;
        }
    } else {
        fetch(0);
        for (int t0 = 0; t0 < T; t0 += 32) tile(t0, t0 + 32 < T ? t0 + 32 : t0);
    }
    if (kin) {
        ab_store16(gk + A.kb + (long long)key * A.ks + 4 * half, dk, 1.f);
        float* dvd = gv + A.vb + (long long)key * A.vs + 4 * half;
        ab_store16(dvd, dv0, 1.f);
        ab_store16(dvd + 32, dv1, 1.f);
    }
}

bool ab_pitch(int token_major, int heads, long long lq, long long lk, long long lv, const float* q, const float* k, const float* v,
              AbPitch* out) {
    out->q = (int)(lq > 0 ? lq : heads * 32);
    out->k = (int)(lk > 0 ? lk : heads * 32);
    out->v = (int)(lv > 0 ? lv : heads * 64);
    if (!token_major) return lq <= 0 && lk <= 0 && lv <= 0;
    if (lq > (1 << 30) || lk > (1 << 30) || lv > (1 << 30)) return false;
    if (out->q % 4 || out->k % 4 || out->v % 4 || out->q < heads * 32 || out->k < heads * 32 || out->v < heads * 64) return false;
    return !(((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)v & 15));
}

}  // namespace
#endif  // SINGA_EMUL

extern "C" int singa_attn_bf16_fwd(const float* q, const float* k, const float* v, const unsigned char* mask, long long mask_stride_b,
                                   long long mask_stride_t, float* ctx, float* lse, int BH, int T, int S, int heads, int DK, int DV,
                                   int token_major, long long ld_q, long long ld_k, long long ld_v, float scale,
                                   const uint32_t* tile_rows, void* stream) {
    if (!q || !k || !v || !mask || !ctx || !lse) return singa_detail_fail(SINGA_E_NULL, "attn_bf16_fwd: null pointer");
    if (DK != 32 || DV != 64) return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_fwd: built for 32 key / 64 value channels per head");
    if (heads <= 0 || BH % heads) return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_fwd: BH must be batch x heads");
    if (BH <= 0 || T <= 0 || S <= 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_fwd: not part of the emulation build");
#else
    AbPitch ld;
    if (!ab_pitch(token_major, heads, ld_q, ld_k, ld_v, q, k, v, &ld))
        return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_fwd: token pitches must be multiples of 4 floats, at least heads * D, 16-byte aligned bases");
    const long long waves = (long long)BH * ((T + 31) / 32);
    const dim3 grid((unsigned)(((waves + 3) / 4 + 7) / 8 * 8));
    const int tm = token_major ? 1 : 0;
    if (tile_rows)
        hipLaunchKernelGGL(attn_bf16_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, q, k, v, mask, mask_stride_b,
                           mask_stride_t, ctx, lse, BH, T, S, heads, tm, scale, ld, tile_rows);
    else
        hipLaunchKernelGGL(attn_bf16_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, q, k, v, mask, mask_stride_b,
                           mask_stride_t, ctx, lse, BH, T, S, heads, tm, scale, ld, nullptr);
    return singa_detail_check_launch("attn_bf16_fwd");
#endif
}

extern "C" int singa_attn_bf16_bwd(const float* q, const float* k, const float* v, const unsigned char* mask, long long mask_stride_b,
                                   long long mask_stride_t, const float* ctx, const float* lse, const float* g_ctx, float* g_q,
                                   float* g_k, float* g_v, float* dsum, int BH, int T, int S, int heads, int DK, int DV,
                                   int token_major, long long ld_q, long long ld_k, long long ld_v, float scale,
                                   const uint32_t* tile_rows, const uint32_t* tile_cols, void* stream) {
    if (!q || !k || !v || !mask || !ctx || !lse || !g_ctx || !g_q || !g_k || !g_v || !dsum)
        return singa_detail_fail(SINGA_E_NULL, "attn_bf16_bwd: null pointer");
    if (DK != 32 || DV != 64) return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_bwd: built for 32 key / 64 value channels per head");
    if (heads <= 0 || BH % heads) return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_bwd: BH must be batch x heads");
    if (BH <= 0 || T <= 0 || S <= 0) return SINGA_OK;
#ifdef SINGA_EMUL
    return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_bwd: not part of the emulation build");
#else
    AbPitch ld;
    if (!ab_pitch(token_major, heads, ld_q, ld_k, ld_v, q, k, v, &ld) || ((uintptr_t)g_q & 15) || ((uintptr_t)g_k & 15) || ((uintptr_t)g_v & 15))
        return singa_detail_fail(SINGA_E_SHAPE, "attn_bf16_bwd: token pitches must be multiples of 4 floats, at least heads * D, 16-byte aligned bases");
    const long long wq = (long long)BH * ((T + 31) / 32), wk = (long long)BH * ((S + 31) / 32);
    const dim3 gq((unsigned)(((wq + 3) / 4 + 7) / 8 * 8)), gk((unsigned)(((wk + 3) / 4 + 7) / 8 * 8));
    const int tm = token_major ? 1 : 0;
    if (tile_rows)
        hipLaunchKernelGGL(attn_bf16_bwd_dq_kernel<true>, gq, dim3(256), 0, (hipStream_t)stream, q, k, v, mask, mask_stride_b,
                           mask_stride_t, ctx, lse, g_ctx, g_q, dsum, BH, T, S, heads, tm, scale, ld, tile_rows);
    else
        hipLaunchKernelGGL(attn_bf16_bwd_dq_kernel<false>, gq, dim3(256), 0, (hipStream_t)stream, q, k, v, mask, mask_stride_b,
                           mask_stride_t, ctx, lse, g_ctx, g_q, dsum, BH, T, S, heads, tm, scale, ld, nullptr);
    if (tile_cols)
        hipLaunchKernelGGL((attn_bf16_bwd_dkv_kernel<true, 1>), dim3((unsigned)((wk + 7) / 8 * 8)), dim3(64), 0, (hipStream_t)stream, q,
                           k, v, mask, mask_stride_b, mask_stride_t, lse, dsum, g_ctx, g_k, g_v, BH, T, S, heads, tm, scale, ld, tile_cols);
    else
        hipLaunchKernelGGL((attn_bf16_bwd_dkv_kernel<false, 4>), gk, dim3(256), 0, (hipStream_t)stream, q, k, v, mask, mask_stride_b,
                           mask_stride_t, lse, dsum, g_ctx, g_k, g_v, BH, T, S, heads, tm, scale, ld, nullptr);
    return singa_detail_check_launch("attn_bf16_bwd");
#endif
}
