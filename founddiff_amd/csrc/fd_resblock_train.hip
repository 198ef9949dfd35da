// fd_resblock_train.hip -- the two backward pieces of the reference's ResnetBlock (src/DADiff.py:139-154, 213-229, 397-430) that
// had no kernel, for training, fp32, NHWC.  The block is out = SiLU(GroupNorm(conv3x3(x, w) + bias)) (+ res); its forward is
// fd_conv2d(FD_F32) with stats_partial -> fd_gn_finalize -> fd_gn_silu_apply, and the input gradient is fd_conv2d on the mirrored,
// transposed weights.
//
//   fd_gn_silu_bwd_f32     dout, h -> dh (the gradient of the raw convolution output), dgamma, dbeta, dbias
//   fd_conv3x3_wgrad_f32   x, dh -> dweight [Cout][9 Cin], K order (kh, kw, c) as fd_conv2d takes the weight
//
// No float atomics: every sum is per-workgroup partials in the workspace, added in a fixed order.  Chunk sizes, tile sizes, the
// split count and every order of summation depend on the shape only.
//
// 1. GroupNorm + SiLU backward.  With hn = (h - mean_g) rstd_g, z = gamma hn + beta, s = sigmoid(z), dz = dout s (1 + z (1 - s)):
//      dgamma_c = sum_{b,p} dz hn,  dbeta_c = sum_{b,p} dz,
//      per (b, g), m = hw C/G:  S1 = sum gamma_c dz / m,  S2 = sum gamma_c dz hn / m,
//      dh = rstd_g (gamma_c dz - S1 - hn S2),  dbias_c = sum_{b,p} dh.
//    Two streaming passes over (dout, h), lane = 4 consecutive channels, 16-byte accesses; z is recomputed in both.
//      pass 1: per (b, chunk of pixels) the channel sums of dz, dz hn and hn -> one partial row [3][C] per workgroup, summed by two
//              launches of a fixed-order kernel; S1 and S2 from the channel sums in double; dgamma, dbeta over the batch in order;
//              dbias in closed form, sum_b rstd (gamma A1 - hw S1 - S2 A3) with A1 = sum_p dz, A3 = sum_p hn, in double.
//      pass 2: dh.
//    Traffic: 2 A + (2 A + A) = 5 A for an activation of A bytes (algorithmic: 3 A).
// 2. 3x3 weight gradient: dw[n][kh][kw][c] = sum_{b,y,x} dh[b,y,x,n] x[b,y+kh-1,x+kw-1,c], a GEMM with M = Cout, N = 9 Cin,
//    K = B H W on v_mfma_f32_16x16x4_f32 (exact fp32: an fmaf chain).  Both operands are K-major as stored (a pixel's channels are
//    contiguous), so the LDS images are [pixel][channel] and a fragment is one ds_read_b32 per lane.
//      workgroup = 4 waves, output tile 64 n x 9 taps x 32 c; wave w owns n in [16 w, +16): 18 accumulator tiles (72 VGPRs).
//      K step   = a tile of 8 x 16 pixels: dh [128][64] and the (8+2) x (16+2) halo of x [180][32] in LDS (row strides 80 and 48
//                 floats: the four pixels of one MFMA K step fall into different banks); the halo serves all nine taps.  The next
//                 tile's global loads are issued before the 32 x 18 MFMAs of the current one.
//      split K  : the B tiles_y tiles_x pixel tiles are cut into S contiguous ranges, S = min(tiles, ceil(1024 / output tiles),
//                 256); split s writes its partial [Cout][9 Cin] to the workspace and a second launch adds the S partials in
//                 order: 256 splits at down0 (2 output tiles, 4 096 pixel tiles), 6 at ups0 (192 output tiles, 64 pixel tiles).
//                 S = 1 (one pixel tile) writes dweight directly.
#include "fd_common.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-LOG2E * x)); }

int64_t round4(int64_t n) { return (n + 3) & ~(int64_t)3; }

bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// out[b][j][q] = sum of p[b][m][q] over m in [j G, min((j + 1) G, M)) in order; rows Q floats apart
__global__ __launch_bounds__(256) void rb_sum_kernel(const float *__restrict__ p, int M, int Q, int G, float *__restrict__ out,
                                                    int Mo) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    const int j = blockIdx.y;
    const int64_t b = blockIdx.z;
    const int m1 = min(M, (j + 1) * G);
    const float *pp = p + b * M * Q + q;
    float v = 0.f;
    for (int m = j * G; m < m1; ++m) v += pp[(int64_t)m * Q];
    out[(b * Mo + j) * Q + q] = v;
}

// ---- 1. GroupNorm + SiLU backward ----------------------------------------------------------------------------------------------
constexpr int GSB_G = 16;

struct GsbPlan {
    int lpr, rpb, nthr, ch, nchunk, M1;
    int64_t part, stage, fin, coef, total;
};

bool gsb_shape_ok(int B, int64_t hw, int C, int groups) {
    return B > 0 && B < 65536 && hw > 0 && hw < (1ll << 31) && C > 0 && C % 32 == 0 && C <= 512 && groups > 0 && C % groups == 0 &&
           (C / groups) % 4 == 0;
}

GsbPlan gsb_plan(int B, int64_t hw, int C, int groups) {
    GsbPlan p;
    p.lpr = C / 4;                                  // lanes per pixel row
    p.rpb = 256 / p.lpr;                            // rows per step of a workgroup (C <= 512: at least 2)
    p.nthr = p.rpb * p.lpr;
    // rows per workgroup: ~512 workgroups from one slice, 16 .. 512 rows each (a function of hw alone)
    int64_t ch = ((hw + 511) / 512 + 15) / 16 * 16;
    p.ch = (int)(ch < 16 ? 16 : (ch > 512 ? 512 : ch));
    p.nchunk = (int)((hw + p.ch - 1) / p.ch);
    p.M1 = (p.nchunk + GSB_G - 1) / GSB_G;
    p.part = round4((int64_t)B * p.nchunk * 3 * C);
    p.stage = round4((int64_t)B * p.M1 * 3 * C);
    p.fin = round4((int64_t)B * 3 * C);
    p.coef = round4((int64_t)B * groups * 2);
    p.total = p.part + p.stage + p.fin + p.coef;
    return p;
}

// one lane's 4 channels of one pixel: hn and dz
__device__ __forceinline__ void gsb_point(const f32x4 hv, const f32x4 g, float mean, float rstd, const f32x4 gm, const f32x4 bt,
                                          f32x4 &hn, f32x4 &dz) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        hn[e] = (hv[e] - mean) * rstd;
        const float z = gm[e] * hn[e] + bt[e];
        const float s = sigmoid_f(z);
        dz[e] = g[e] * (s * (1.0f + z * (1.0f - s)));
    }
}

// grid (chunk, b), rpb lpr threads: rows [chunk ch, +ch) of slice b; part[b][chunk][sum dz | sum dz hn | sum hn][C]
__global__ __launch_bounds__(256) void gsb_sums_kernel(const float *__restrict__ dout, const float *__restrict__ h,
                                                      const float *__restrict__ mean_rstd, const float *__restrict__ gamma,
                                                      const float *__restrict__ beta, float *__restrict__ part, int64_t hw, int C,
                                                      int groups, int lpr, int rpb, int ch) {
    __shared__ __attribute__((aligned(16))) float red[3 * 1024];      // [row slot][3][C], rpb C <= 1024
    const int tid = threadIdx.x, cq = tid % lpr, slot = tid / lpr;
    const int c = 4 * cq;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * ch;
    const int g = c / (C / groups);
    const float mean = mean_rstd[(b * groups + g) * 2], rstd = mean_rstd[(b * groups + g) * 2 + 1];
    const f32x4 gm = *(const f32x4 *)(gamma + c), bt = *(const f32x4 *)(beta + c);
    f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
    const int64_t r1 = min(hw, r0 + ch);
    for (int64_t r = r0 + slot; r < r1; r += rpb) {
        const int64_t o = (b * hw + r) * C + c;
        f32x4 hn, dz;
        gsb_point(*(const f32x4 *)(h + o), *(const f32x4 *)(dout + o), mean, rstd, gm, bt, hn, dz);
        a1 += dz;
        a2 += dz * hn;
        a3 += hn;
    }
    // the row slots' sums, in slot order
    *(f32x4 *)(red + (slot * 3 + 0) * C + c) = a1;
    *(f32x4 *)(red + (slot * 3 + 1) * C + c) = a2;
    *(f32x4 *)(red + (slot * 3 + 2) * C + c) = a3;
    __syncthreads();
    float *pp = part + (b * gridDim.x + blockIdx.x) * 3 * C;
    for (int idx = tid; idx < 3 * C; idx += blockDim.x) {
        float v = 0.f;
        for (int sl = 0; sl < rpb; ++sl) v += red[sl * 3 * C + idx];
        pp[idx] = v;
    }
}

// fin [B][A1 | A2 | A3][C] -> coef [B][G][S1, S2]: one thread per (b, g), double as gn_finalize_kernel
__global__ __launch_bounds__(256) void gsb_coef_kernel(const float *__restrict__ fin, const float *__restrict__ gamma, int B, int C,
                                                      int groups, double inv_m, float *__restrict__ coef) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * groups) return;
    const int b = i / groups, g = i - b * groups, cpg = C / groups;
    const float *f = fin + (int64_t)b * 3 * C;
    double s1 = 0.0, s2 = 0.0;
    for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        s1 += (double)gamma[c] * (double)f[c];
        s2 += (double)gamma[c] * (double)f[C + c];
    }
    coef[2 * i] = (float)(s1 * inv_m);
    coef[2 * i + 1] = (float)(s2 * inv_m);
}

// one thread per channel: the sums over the batch in order
__global__ __launch_bounds__(256) void gsb_param_kernel(const float *__restrict__ fin, const float *__restrict__ coef,
                                                       const float *__restrict__ mean_rstd, const float *__restrict__ gamma, int B,
                                                       int C, int groups, double hw, float *__restrict__ dgamma,
                                                       float *__restrict__ dbeta, float *__restrict__ dbias) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const int g = c / (C / groups);
    float dg = 0.f, db = 0.f;
    double dbs = 0.0;
    for (int b = 0; b < B; ++b) {
        const float *f = fin + (int64_t)b * 3 * C;
        dg += f[C + c];
        db += f[c];
        const int i = b * groups + g;
        dbs += (double)mean_rstd[2 * i + 1] *
               ((double)gamma[c] * (double)f[c] - hw * (double)coef[2 * i] - (double)coef[2 * i + 1] * (double)f[2 * C + c]);
    }
    dgamma[c] = dg;
    dbeta[c] = db;
    if (dbias) dbias[c] = (float)dbs;
}

__global__ __launch_bounds__(256) void gsb_dh_kernel(const float *__restrict__ dout, const float *__restrict__ h,
                                                    const float *__restrict__ mean_rstd, const float *__restrict__ gamma,
                                                    const float *__restrict__ beta, const float *__restrict__ coef,
                                                    float *__restrict__ dh, int64_t hw, int C, int groups, int lpr, int rpb, int ch) {
    const int tid = threadIdx.x, cq = tid % lpr, slot = tid / lpr;
    const int c = 4 * cq;
    const int64_t b = blockIdx.y;
    const int64_t r0 = (int64_t)blockIdx.x * ch;
    const int g = c / (C / groups);
    const float mean = mean_rstd[(b * groups + g) * 2], rstd = mean_rstd[(b * groups + g) * 2 + 1];
    const float s1 = coef[(b * groups + g) * 2], s2 = coef[(b * groups + g) * 2 + 1];
    const f32x4 gm = *(const f32x4 *)(gamma + c), bt = *(const f32x4 *)(beta + c);
    const int64_t r1 = min(hw, r0 + ch);
    for (int64_t r = r0 + slot; r < r1; r += rpb) {
        const int64_t o = (b * hw + r) * C + c;
        f32x4 hn, dz, d;
        gsb_point(*(const f32x4 *)(h + o), *(const f32x4 *)(dout + o), mean, rstd, gm, bt, hn, dz);
#pragma unroll
        for (int e = 0; e < 4; ++e) d[e] = rstd * (gm[e] * dz[e] - s1 - hn[e] * s2);
        *(f32x4 *)(dh + o) = d;
    }
}

// ---- 2. 3x3 weight gradient --------------------------------------------------------------------------------------------------
constexpr int WG_TY = 8, WG_TX = 16, WG_PIX = WG_TY * WG_TX, WG_HX = WG_TX + 2, WG_HY = WG_TY + 2, WG_HPIX = WG_HX * WG_HY;
constexpr int WG_NB = 64, WG_CB = 32, WG_LDA = 80, WG_LDB = 48;
constexpr int WG_AV = WG_PIX * (WG_NB / 4) / 256;                        // 16-byte vectors of dh per thread and tile: 8
constexpr int WG_BV = (WG_HPIX * (WG_CB / 4) + 255) / 256;               // of the halo of x: 6 (the last one partly)

struct WgPlan {
    int tiles_x, tiles_y, nblk, cblk, tps, S;
    int64_t ntiles, out;
};

bool wg_shape_ok(int B, int H, int W, int Cin, int Cout) {
    return B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 16 == 0 && Cin <= 1024 && Cout > 0 && Cout % 32 == 0 && Cout <= 512 &&
           (int64_t)B * ((H + WG_TY - 1) / WG_TY) * ((W + WG_TX - 1) / WG_TX) < (1ll << 31);
}

WgPlan wg_plan(int B, int H, int W, int Cin, int Cout) {
    WgPlan p;
    p.tiles_x = (W + WG_TX - 1) / WG_TX;
    p.tiles_y = (H + WG_TY - 1) / WG_TY;
    p.ntiles = (int64_t)B * p.tiles_y * p.tiles_x;
    p.nblk = (Cout + WG_NB - 1) / WG_NB;
    p.cblk = (Cin + WG_CB - 1) / WG_CB;
    int64_t want = (1024 + p.nblk * p.cblk - 1) / (p.nblk * p.cblk);
    if (want > 256) want = 256;
    if (want > p.ntiles) want = p.ntiles;
    p.tps = (int)((p.ntiles + want - 1) / want);
    p.S = (int)((p.ntiles + p.tps - 1) / p.tps);
    p.out = (int64_t)Cout * 9 * Cin;
    return p;
}

// grid (split, n block x c block); out = the workspace [S][Cout][9 Cin], or dweight itself when S = 1
__global__ __launch_bounds__(256) void wgrad_kernel(const float *__restrict__ x, int ld_x, int off_x, const float *__restrict__ dh,
                                                   float *__restrict__ out, int H, int W, int Cin, int Cout, int tiles_x,
                                                   int tiles_y, int64_t ntiles, int tps, int cblk) {
    __shared__ __attribute__((aligned(16))) float sA[WG_PIX * WG_LDA];
    __shared__ __attribute__((aligned(16))) float sB[WG_HPIX * WG_LDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, r = lane & 15;
    const int nb = blockIdx.y / cblk, cb = blockIdx.y - nb * cblk;
    const int n_base = nb * WG_NB, c_base = cb * WG_CB;
    const bool wave_on = n_base + 16 * wave < Cout;
    const int64_t t0 = (int64_t)blockIdx.x * tps;
    const int64_t t1 = min(ntiles, t0 + tps);
    f32x4 acc[9][2];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 ra[WG_AV], rb[WG_BV];
    auto gload = [&](int64_t t) {
        const int tx = (int)(t % tiles_x);
        const int64_t q = t / tiles_x;
        const int ty = (int)(q % tiles_y);
        const int64_t b = q / tiles_y;
        const int y0 = ty * WG_TY, x0 = tx * WG_TX;
#pragma unroll
        for (int i = 0; i < WG_AV; ++i) {
            const int idx = tid + 256 * i;
            const int v = idx & 15, p = idx >> 4;
            const int yy = y0 + (p >> 4), xx = x0 + (p & 15), n = n_base + 4 * v;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (yy < H && xx < W && n < Cout) val = *(const f32x4 *)(dh + ((b * H + yy) * W + xx) * Cout + n);
            ra[i] = val;
        }
#pragma unroll
        for (int i = 0; i < WG_BV; ++i) {
            const int idx = tid + 256 * i;
            const int v = idx & 7, p = idx >> 3;
            const int hy = p / WG_HX, hx = p - hy * WG_HX;
            const int yy = y0 + hy - 1, xx = x0 + hx - 1, c = c_base + 4 * v;
            f32x4 val = {0.f, 0.f, 0.f, 0.f};
            if (p < WG_HPIX && yy >= 0 && yy < H && xx >= 0 && xx < W && c < Cin)
                val = *(const f32x4 *)(x + ((b * H + yy) * W + xx) * ld_x + off_x + c);
            rb[i] = val;
        }
    };
    auto lstore = [&]() {
#pragma unroll
        for (int i = 0; i < WG_AV; ++i) {
            const int idx = tid + 256 * i;
            *(f32x4 *)(sA + (idx >> 4) * WG_LDA + 4 * (idx & 15)) = ra[i];
        }
#pragma unroll
        for (int i = 0; i < WG_BV; ++i) {
            const int idx = tid + 256 * i;
            if ((idx >> 3) < WG_HPIX) *(f32x4 *)(sB + (idx >> 3) * WG_LDB + 4 * (idx & 7)) = rb[i];
        }
    };
    if (t0 < t1) gload(t0);
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();                       // the previous tile's fragment reads are done
        lstore();
        __syncthreads();
        if (t + 1 < t1) gload(t + 1);
        if (wave_on) {
            // lane (g, r): A[n = 16 wave + r][k = k0 + g], B[k = k0 + g][c = 16 j + r]; pixel k = (k >> 4, k & 15) of the tile
            const float *ap = sA + g * WG_LDA + 16 * wave + r;
            const float *bp = sB + g * WG_LDB + r;
#pragma unroll 2
            for (int k0 = 0; k0 < WG_PIX; k0 += 4) {
                const float a = ap[k0 * WG_LDA];
                const float *bq = bp + ((k0 >> 4) * WG_HX + (k0 & 15)) * WG_LDB;
#pragma unroll
                for (int kh = 0; kh < 3; ++kh)
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const float *bt = bq + (kh * WG_HX + kw) * WG_LDB;
                        acc[kh * 3 + kw][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bt[0], acc[kh * 3 + kw][0], 0, 0, 0);
                        acc[kh * 3 + kw][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bt[16], acc[kh * 3 + kw][1], 0, 0, 0);
                    }
            }
        }
    }
    if (!wave_on) return;
    // D: lane (g, r) holds rows n = 4 g + i, column c = r of each 16 x 16 tile
    float *op = out + (int64_t)blockIdx.x * Cout * 9 * Cin;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int c = c_base + 16 * j + r;
            if (c >= Cin) continue;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int n = n_base + 16 * wave + 4 * g + i;
                op[((int64_t)n * 9 + t) * Cin + c] = acc[t][j][i];
            }
        }
}

// dw[i] = the S partials in order
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ ws, int S, int64_t n, float *__restrict__ dw) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) v += *(const f32x4 *)(ws + (int64_t)s * n + i);
    *(f32x4 *)(dw + i) = v;
}

}  // namespace

extern "C" int64_t fd_gn_silu_bwd_ws_floats(int B, int64_t hw, int C, int groups) {
    if (!gsb_shape_ok(B, hw, C, groups)) return 0;
    return gsb_plan(B, hw, C, groups).total;
}

extern "C" int fd_gn_silu_bwd_f32(const float *dout, const float *h, const float *mean_rstd, const float *gamma, const float *beta,
                                  float *dh, float *dgamma, float *dbeta, float *dbias, float *ws, int B, int64_t hw, int C,
                                  int groups, void *stream) {
    FD_REQUIRE(dout && h && mean_rstd && gamma && beta && dh && dgamma && dbeta && ws, "fd_gn_silu_bwd_f32: null pointer");
    FD_REQUIRE(gsb_shape_ok(B, hw, C, groups),
               "fd_gn_silu_bwd_f32: unsupported shape B=%d hw=%lld C=%d groups=%d (C %% 32 == 0, C <= 512, (C / groups) %% 4 == 0)", B,
               (long long)hw, C, groups);
    FD_REQUIRE(al16(dout) && al16(h) && al16(gamma) && al16(beta) && al16(dh) && al16(ws),
               "fd_gn_silu_bwd_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const GsbPlan p = gsb_plan(B, hw, C, groups);
    float *part = ws, *stage = part + p.part, *fin = stage + p.stage, *coef = fin + p.fin;
    const int Q = 3 * C;
    hipLaunchKernelGGL(gsb_sums_kernel, dim3((unsigned)p.nchunk, (unsigned)B), dim3((unsigned)p.nthr), 0, st, dout, h, mean_rstd, gamma,
                       beta, part, hw, C, groups, p.lpr, p.rpb, p.ch);
    hipLaunchKernelGGL(rb_sum_kernel, dim3((unsigned)((Q + 255) / 256), (unsigned)p.M1, (unsigned)B), dim3(256), 0, st, part, p.nchunk, Q,
                       GSB_G, stage, p.M1);
    hipLaunchKernelGGL(rb_sum_kernel, dim3((unsigned)((Q + 255) / 256), 1, (unsigned)B), dim3(256), 0, st, stage, p.M1, Q, p.M1, fin, 1);
    hipLaunchKernelGGL(gsb_coef_kernel, dim3((unsigned)((B * groups + 255) / 256)), dim3(256), 0, st, fin, gamma, B, C, groups,
                       1.0 / ((double)hw * (C / groups)), coef);
    hipLaunchKernelGGL(gsb_param_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, fin, coef, mean_rstd, gamma, B, C, groups,
                       (double)hw, dgamma, dbeta, dbias);
    hipLaunchKernelGGL(gsb_dh_kernel, dim3((unsigned)p.nchunk, (unsigned)B), dim3((unsigned)p.nthr), 0, st, dout, h, mean_rstd, gamma,
                       beta, coef, dh, hw, C, groups, p.lpr, p.rpb, p.ch);
    FD_LAUNCH_OK("fd_gn_silu_bwd_f32");
    return FD_OK;
}

extern "C" int64_t fd_conv3x3_wgrad_ws_floats(int B, int H, int W, int Cin, int Cout) {
    if (!wg_shape_ok(B, H, W, Cin, Cout)) return 0;
    const WgPlan p = wg_plan(B, H, W, Cin, Cout);
    return p.S > 1 ? round4((int64_t)p.S * p.out) : 4;
}

extern "C" int fd_conv3x3_wgrad_f32(const float *x, int ld_x, int off_x, const float *dh, float *dw, float *ws, int B, int H, int W,
                                    int Cin, int Cout, void *stream) {
    FD_REQUIRE(x && dh && dw && ws, "fd_conv3x3_wgrad_f32: null pointer");
    FD_REQUIRE(wg_shape_ok(B, H, W, Cin, Cout),
               "fd_conv3x3_wgrad_f32: unsupported shape B=%d H=%d W=%d Cin=%d Cout=%d (Cin %% 16 == 0, Cin <= 1024, Cout %% 32 == 0, "
               "Cout <= 512)", B, H, W, Cin, Cout);
    FD_REQUIRE(off_x >= 0 && ld_x >= off_x + Cin && ld_x % 4 == 0 && off_x % 4 == 0,
               "fd_conv3x3_wgrad_f32: stride / offset must be multiples of 4 with off + Cin <= ld (ld_x=%d off_x=%d)", ld_x, off_x);
    FD_REQUIRE(al16(x) && al16(dh) && al16(dw) && al16(ws), "fd_conv3x3_wgrad_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const WgPlan p = wg_plan(B, H, W, Cin, Cout);
    hipLaunchKernelGGL(wgrad_kernel, dim3((unsigned)p.S, (unsigned)(p.nblk * p.cblk)), dim3(256), 0, st, x, ld_x, off_x, dh,
                       p.S > 1 ? ws : dw, H, W, Cin, Cout, p.tiles_x, p.tiles_y, p.ntiles, p.tps, p.cblk);
    if (p.S > 1)
        hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((p.out / 4 + 255) / 256)), dim3(256), 0, st, ws, p.S, p.out, dw);
    FD_LAUNCH_OK("fd_conv3x3_wgrad_f32");
    return FD_OK;
}
