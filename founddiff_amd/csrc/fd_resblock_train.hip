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
//              launches of partial_sum_kernel; S1 and S2 from the channel sums in double; dgamma, dbeta over the batch in order;
//              dbias in closed form, sum_b rstd (gamma A1 - hw S1 - S2 A3) with A1 = sum_p dz, A3 = sum_p hn, in double.
//      pass 2: dh.
//    Traffic: 2 A + (2 A + A) = 5 A for an activation of A bytes (algorithmic: 3 A).
// 2. 3x3 weight gradient: dw[n][kh][kw][c] = sum_{b,y,x} dh[b,y,x,n] x[b,y+kh-1,x+kw-1,c], a GEMM with M = Cout, N = 9 Cin,
//    K = B H W: the tap correlation of fd_train_common.h with a = dh and f = x, tapcorr_kernel<KT = 3 taps per axis, STRIDE = 1,
//    TY x TX = 8 x 16 pixels per K step, LDB = 48 floats per halo row in LDS>.
//      workgroup = 4 waves, output tile 64 n x 9 taps x 32 c; wave w owns n in [16 w, +16): 18 accumulator tiles (72 AGPRs).
//      K step   = dh [128][64] and the (8+2) x (16+2) halo of x [180][32] in LDS; the halo serves all nine taps.  The next tile's
//                 global loads are issued before the 32 x 18 MFMAs of the current one.
//      split K  : S = min(tiles, ceil(1024 / output tiles), 256) contiguous ranges of the B tiles_y tiles_x pixel tiles, added in
//                 order by tapcorr_reduce_kernel: 256 splits at down0 (2 output tiles, 4 096 pixel tiles), 6 at ups0 (192 output
//                 tiles, 64 pixel tiles).  S = 1 (one pixel tile) writes dweight directly.
#include "fd_train_common.h"

namespace {

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
constexpr int WG_TY = 8, WG_TX = 16;
constexpr auto wg_launch = tapcorr_launch<3, 1, WG_TY, WG_TX, 48>;

bool wg_shape_ok(int B, int H, int W, int Cin, int Cout) {
    return B > 0 && H > 0 && W > 0 && Cin > 0 && Cin % 16 == 0 && Cin <= 1024 && Cout > 0 && Cout % 32 == 0 && Cout <= 512 &&
           (int64_t)B * ((H + WG_TY - 1) / WG_TY) * ((W + WG_TX - 1) / WG_TX) < (1ll << 31);
}

TapPlan wg_plan(int B, int H, int W, int Cin, int Cout) { return tap_plan(3, WG_TY, WG_TX, B, H, W, Cout, Cin); }

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
    launch_sum(part, Q, (int64_t)p.nchunk * Q, p.nchunk, Q, GSB_G, stage, Q, (int64_t)p.M1 * Q, B, st);
    launch_sum(stage, Q, (int64_t)p.M1 * Q, p.M1, Q, p.M1, fin, Q, Q, B, st);
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
    return tap_ws_floats(wg_plan(B, H, W, Cin, Cout));
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
    wg_launch(wg_plan(B, H, W, Cin, Cout), dh, x, ld_x, off_x, dw, ws, H, W, Cout, Cin, (hipStream_t)stream);
    FD_LAUNCH_OK("fd_conv3x3_wgrad_f32");
    return FD_OK;
}
