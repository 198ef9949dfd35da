// fd_train_common.h -- what the training kernels (fd_*_train.hip, fd_*_bwd.hip) share: the host-side size helpers, the sigmoid, the
// four-element load / store, the workgroup sum, the fixed-order partial sum and the split-K tap correlation behind both convolution weight gradients.  Everything sits in an
// anonymous namespace: each file that includes this header gets its own copy of the kernels it launches, and of no other.
#pragma once
#include <type_traits>
#include "fd_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * x)); }

int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// n <= 4 floats at p: one 16-byte access when VEC (then n == 4), scalar otherwise; missing elements read as 0
template <bool VEC>
__device__ __forceinline__ void load4(const float *p, int n, float v[4]) {
    if (VEC) {
        const f32x4 q = *(const f32x4 *)p;
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = e < n ? p[e] : 0.f;
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float *p, int n, const float v[4]) {
    if (VEC) {
        *(f32x4 *)p = f32x4{v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (e < n) p[e] = v[e];
    }
}

// the sum of v over the 256 lanes, in a fixed tree order; every lane gets it.  red: 256 floats of LDS, the caller's; a second sum
// in one kernel takes a second array (the first one's red[0] may still be read when the next sum writes it)
__device__ __forceinline__ float block_sum256(float v, float *red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// ---- the fixed-order partial sum -----------------------------------------------------------------------------------------------
// out[b][j][q] = sum of p[b][m][q] over m in [j G, min((j + 1) G, M)) in order; p rows ldp floats apart, out rows ldo.  (This kernel,
// its launcher and tapcorr_reduce_kernel below are templates only so that a file that never calls them gets no copy of the kernel.)
template <int = 0>
__global__ __launch_bounds__(256) void partial_sum_kernel(const float *__restrict__ p, int64_t ldp, int64_t p_bstride, int M, int Q,
                                                          int G, float *__restrict__ out, int64_t ldo, int64_t o_bstride) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int j = blockIdx.y, b = blockIdx.z;
    const int m1 = min(M, (j + 1) * G);
    const float *pp = p + (int64_t)b * p_bstride + q;
    float v = 0.f;
    for (int m = j * G; m < m1; ++m) v += pp[(int64_t)m * ldp];
    out[(int64_t)b * o_bstride + (int64_t)j * ldo + q] = v;
}

template <int = 0>
void launch_sum(const float *p, int64_t ldp, int64_t p_bstride, int M, int Q, int G, float *out, int64_t ldo, int64_t o_bstride,
                int nb, hipStream_t st) {
    hipLaunchKernelGGL(partial_sum_kernel<>, dim3((unsigned)((Q + 255) / 256), (unsigned)((M + G - 1) / G), (unsigned)nb), dim3(256), 0,
                       st, p, ldp, p_bstride, M, Q, G, out, ldo, o_bstride);
}

// ---- the tap correlation -------------------------------------------------------------------------------------------------------
// g[p][t][u][q] = sum_{b,i,j} a[b, i, j, p] f[b, STRIDE i + t - 1, STRIDE j + u - 1, q], t, u in [0, KT): a (B, H, W, P) dense, f
// channels [off, off + Q) of (B, STRIDE H, STRIDE W, ld), zero outside; P a multiple of 4, Q of 16.  A GEMM with M = P,
// N = KT KT Q, K = B H W pixels of a on v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain).  Both operands are K-major as stored (a
// pixel's channels are contiguous), so the LDS images are [pixel][channel] and a fragment is one ds_read_b32 per lane.
//   KT, STRIDE : taps per axis and the step of f per pixel of a
//   TY, TX     : the K step, a tile of TY x TX pixels of a (TX a power of two, TY TX a multiple of 16) and its halo of f,
//                STRIDE (TX - 1) + KT wide and STRIDE (TY - 1) + KT high, which serves all KT KT taps
//   LDB        : the halo's LDS row stride in floats, chosen so that the four pixels of one MFMA K step, STRIDE LDB floats apart,
//                fall into different banks (a's row stride is 80)
//   workgroup  = 4 waves, output tile 64 p x KT KT taps x 32 q; wave w owns p in [16 w, +16): 2 KT KT accumulator tiles.  The next
//                tile's global loads are issued before the MFMAs of the current one.
//   split K    : the B tiles_y tiles_x pixel tiles are cut into S contiguous ranges, S = min(tiles, ceil(1024 / output tiles), 256,
//                the caller's cap); split s writes its partial [P][KT KT Q] to the workspace and a second launch adds the S partials
//                in order.  S = 1 (one pixel tile) writes g directly.
constexpr int TC_PB = 64, TC_QB = 32, TC_LDA = 80;

struct TapPlan {
    int tiles_x, tiles_y, pblk, qblk, tps, S;
    int64_t ntiles, out;
};

// cap: the most splits the caller's workspace budget allows (256: none)
TapPlan tap_plan(int KT, int TY, int TX, int B, int H, int W, int P, int Q, int64_t cap = 256) {
    TapPlan p;
    p.tiles_x = (W + TX - 1) / TX;
    p.tiles_y = (H + TY - 1) / TY;
    p.ntiles = (int64_t)B * p.tiles_y * p.tiles_x;
    p.pblk = (P + TC_PB - 1) / TC_PB;
    p.qblk = (Q + TC_QB - 1) / TC_QB;
    p.out = (int64_t)P * KT * KT * Q;
    int64_t want = (1024 + p.pblk * p.qblk - 1) / (p.pblk * p.qblk);
    if (want > 256) want = 256;
    if (want > cap) want = cap;
    if (want < 1) want = 1;
    if (want > p.ntiles) want = p.ntiles;
    p.tps = (int)((p.ntiles + want - 1) / want);
    p.S = (int)((p.ntiles + p.tps - 1) / p.tps);
    return p;
}

int64_t tap_ws_floats(const TapPlan &p) { return p.S > 1 ? round4((int64_t)p.S * p.out) : 4; }

// grid (split, p block x q block); out = the workspace [S][P][KT KT Q], or g itself when S = 1
template <int KT, int STRIDE, int TY, int TX, int LDB>
__global__ __launch_bounds__(256) void tapcorr_kernel(const float *__restrict__ a, const float *__restrict__ f, int ld, int off,
                                                     float *__restrict__ out, int H, int W, int P, int Q, int tiles_x, int tiles_y,
                                                     int64_t ntiles, int tps, int qblk) {
    constexpr int PIX = TY * TX, HX = STRIDE * (TX - 1) + KT, HY = STRIDE * (TY - 1) + KT, HPIX = HX * HY;
    constexpr int AV = PIX * (TC_PB / 4) / 256;                          // 16-byte vectors of a per thread and tile
    constexpr int BV = (HPIX * (TC_QB / 4) + 255) / 256;                 // of the halo of f (the last one partly)
    constexpr int TXS = __builtin_ctz(TX);                               // pixel k of the tile is (k >> TXS, k & (TX - 1))
    static_assert((TX & (TX - 1)) == 0 && PIX % 16 == 0, "tapcorr_kernel: TX a power of two, TY TX a multiple of 16");
    __shared__ __attribute__((aligned(16))) float sA[PIX * TC_LDA];
    __shared__ __attribute__((aligned(16))) float sB[HPIX * LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int pb = blockIdx.y / qblk, qb = blockIdx.y - pb * qblk;
    const int p_base = pb * TC_PB, q_base = qb * TC_QB;
    const bool wave_on = p_base + 16 * wave < P;
    const int64_t t0 = (int64_t)blockIdx.x * tps;
    const int64_t t1 = min(ntiles, t0 + tps);
    // halo coordinates: 64-bit where STRIDE scales them; with STRIDE = 1 they stay below H + KT and int keeps the 3x3 weight
    // gradient at its register count
    using HC = std::conditional_t<STRIDE == 1, int, int64_t>;
    const HC FH = STRIDE * (HC)H, FW = STRIDE * (HC)W;
    f32x4 acc[KT * KT][2];
#pragma unroll
    for (int t = 0; t < KT * KT; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra[AV], rb[BV];
    const int qc = q_base + 4 * (tid & 7);                               // this thread's channels of f, the same in every vector
    auto gload = [&](int64_t t) {
        const int tx = (int)(t % tiles_x);
        const int64_t tq = t / tiles_x;
        const int ty = (int)(tq % tiles_y);
        const int64_t b = tq / tiles_y;
        const int y0 = ty * TY, x0 = tx * TX;
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int idx = tid + 256 * i;
            const int v = idx & 15, px = idx >> 4;
            const int yy = y0 + (px >> TXS), xx = x0 + (px & (TX - 1)), pc = p_base + 4 * v;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (yy < H && xx < W && pc < P) val = *(const f32x4 *)(a + ((b * H + yy) * W + xx) * P + pc);
            ra[i] = val;
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = tid + 256 * i;
            const int px = idx >> 3;
            const int hy = px / HX, hx = px - hy * HX;
            const HC yy = STRIDE * (HC)y0 + hy - 1, xx = STRIDE * (HC)x0 + hx - 1;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (px < HPIX && yy >= 0 && yy < FH && xx >= 0 && xx < FW && qc < Q)
                val = *(const f32x4 *)(f + ((b * FH + yy) * FW + xx) * ld + (off + qc));
            rb[i] = val;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < AV; ++i) {
            const int idx = tid + 256 * i;
            *(f32x4 *)(sA + (idx >> 4) * TC_LDA + 4 * (idx & 15)) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < BV; ++i) {
            const int idx = tid + 256 * i;
            if ((idx >> 3) < HPIX) *(f32x4 *)(sB + (idx >> 3) * LDB + 4 * (idx & 7)) = rb[i];
        }
    };
    if (t0 < t1) gload(t0);
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();                       // the previous tile's fragment reads are done
        lstore();
        __syncthreads();
        if (t + 1 < t1) gload(t + 1);
        if (wave_on) {
            // lane (g, r): A[p = 16 wave + r][k = k0 + g], B[k = k0 + g][q = 16 j + r]; pixel k = (ky, kx) of the tile, whose tap
            // (kh, kw) is pixel (STRIDE ky + kh, STRIDE kx + kw) of the halo
            const float *ap = sA + g * TC_LDA + 16 * wave + r;
            const float *bp = sB + STRIDE * g * LDB + r;
#pragma unroll 2
            for (int k0 = 0; k0 < PIX; k0 += 4) {
                const float av = ap[k0 * TC_LDA];
                const float *bq = bp + (STRIDE * (k0 >> TXS) * HX + STRIDE * (k0 & (TX - 1))) * LDB;
#pragma unroll
                for (int kh = 0; kh < KT; ++kh)
#pragma unroll
                    for (int kw = 0; kw < KT; ++kw) {
                        const float *bt = bq + (kh * HX + kw) * LDB;
                        acc[kh * KT + kw][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bt[0], acc[kh * KT + kw][0], 0, 0, 0);
                        acc[kh * KT + kw][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bt[16], acc[kh * KT + kw][1], 0, 0, 0);
                    }
            }
        }
    }
    if (!wave_on) return;
    // D: lane (g, r) holds rows p = 4 g + i, column q = r of each 16 x 16 tile.  Q is a multiple of 16, so the second 16 columns of
    // a workgroup are all inside or all outside
    float *op = out + (int64_t)blockIdx.x * P * (KT * KT) * Q;
    const int nj = q_base + 16 < Q ? 2 : 1;
#pragma unroll
    for (int t = 0; t < KT * KT; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (j >= nj) continue;
            const int q = q_base + 16 * j + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = p_base + 16 * wave + 4 * g + i;
                op[((int64_t)p * (KT * KT) + t) * Q + q] = acc[t][j][i];
            }
        }
}

// g[i] = the S partials in order
template <int = 0>
__global__ __launch_bounds__(256) void tapcorr_reduce_kernel(const float *__restrict__ ws, int S, int64_t n, float *__restrict__ g) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) v += *(const f32x4 *)(ws + (int64_t)s * n + i);
    *(f32x4 *)(g + i) = v;
}

template <int KT, int STRIDE, int TY, int TX, int LDB>
void tapcorr_launch(const TapPlan &p, const float *a, const float *f, int ld, int off, float *g, float *ws, int H, int W, int P,
                    int Q, hipStream_t st) {
    hipLaunchKernelGGL((tapcorr_kernel<KT, STRIDE, TY, TX, LDB>), dim3((unsigned)p.S, (unsigned)(p.pblk * p.qblk)), dim3(256), 0, st,
                       a, f, ld, off, p.S > 1 ? ws : g, H, W, P, Q, p.tiles_x, p.tiles_y, p.ntiles, p.tps, p.qblk);
    if (p.S > 1)
        hipLaunchKernelGGL(tapcorr_reduce_kernel<>, dim3((unsigned)((p.out / 4 + 255) / 256)), dim3(256), 0, st, ws, p.S, p.out, g);
}

}  // namespace
