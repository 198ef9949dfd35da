// fd_cross_scan_bwd.hip -- the reference's cross_selective_scan (src/emamba2.py:295-367) up to out_norm, forward and backward,
// on the fused dataflow of the sampling engine: xc (NHWC) and the x_proj rows xdbl are the only activations either pass reads.
//
// Forward (fd_cross_scan_fwd_f32): NCHW -> NHWC into xc, the x_proj gather as ONE fd_conv2d launch with ndir = 4 (exact fp32),
// fd_selective_scan in FD_F32.  No EfficientScan / EfficientMerge copies, no delta tensor (dt_proj + bias + softplus are
// recomputed per step), y written at the merged pixels.
//
// Backward (fd_cross_scan_bwd_f32), direction k, channel d, row k D + d, position l, pixel p(k, l) (scan_pos of fd_scan.hip):
//     u = xc[b, p, d] (0 at padded positions),  delta = dtw[k, d, :] . xdbl[k, b, l, :R] + dtb[k, d],  dt = softplus(delta)
//     the scan's gradients as fd_scan_bwd.hip states them -> du, ddelta = ddt sigmoid(delta), dA, dD, dB, dC
//     dxdbl[k, b, l] = [ sum_d ddelta dtw[k, d, :] | sum_d dB | sum_d dC ]           (sums over the direction's d_inner channels)
//     ddtw[k, d, r] = sum_{b,l} ddelta xdbl[r]     ddtb[k, d] = sum_{b,l} ddelta
//     dx_proj_w[k, c, d] = sum_{b,l} dxdbl[c] u    dx[b, d, p] = du + sum_c x_proj_w[k, c, d] dxdbl[c]     (inside pixels)
// The padded positions of odd-sized images take part in the recurrence with u = 0, a zero x_dbl row and dy = 0, as in the
// reference's autograd through EfficientScan / EfficientMerge: their ddelta counts in ddtb and dA, their dx is dropped.
//
// Launches (the scheme of fd_scan_bwd_core.h -- h and dL/dh recomputed from tile carries -- on the NHWC operands):
//   1. carry: per (batch, direction, tile, channel split) a workgroup stages the tile's x_dbl rows and, 16 channels at a time,
//             its u / dy pixels in LDS (coalesced 64-byte loads per pixel, stored transposed: [channel][position]); each wave
//             walks 4 channels of a slab, lane = E consecutive positions, and leaves per (row, tile, state) the composites
//             (the core's fold and lane-0 composition);
//   2. chain: the core's chain kernel;
//   3. main:  the same staging; per channel the core's carry-in and replay of h and g, du straight into dx (NCHW), ddelta, the dxdbl row partial
//             kept in registers (R + 2N values per position, summed over the channels in-lane), per (row, tile) partials of
//             dA / ddtw / dD / ddtb; the four waves' rows are summed through LDS in wave order;
//   4. (channel splits only) the split partials of dxdbl summed in split order;
//   5. x_proj: per (batch, direction, 256 sub-grid rows, 64 channels) dx += W^T dxdbl (lane = pixel) and the dx_proj_w
//             partial (lane = channel, sum over the rows in order);
//   6. the dx_proj_w partials and 7. the parameter partials summed over (batch, block) in a fixed order.
// Tile length, channel split and every reduction order are functions of (H, W, D, N, R) only, never of the batch: a slice's
// y and dx are the same bits alone or in a batch.  No float atomics.  fp32 throughout; the same code in both library builds.
// fd_cross_scan_fwd_nhwc_f32 / fd_cross_scan_bwd_nhwc_f32 (founddiff_amd.ss2d_train) are the same launches with NHWC on both
// sides: the forward without the layout move, the backward with the kernels' NHWC template parameter set (a second instantiation: the NCHW one
// is the code it was, register for register) -- launch 3 sends du back through the slab
// buffer and stores it as the slab was loaded, launch 5 adds W^T dxdbl in its lane = channel loop.
#include "fd_scan_bwd_core.h"

namespace {

constexpr int CS_T = 256, CS_W = CS_T / 64, CS_SLAB = 16;

struct CsGeom {
    int B, H, W, D, N, R, CD, H2, W2, L, ntiles, S, nxb;
};

// E consecutive positions per lane: 4 where the dxdbl row fits the registers 4 times (R + 2N <= 24), else 1
__host__ __device__ constexpr int cs_e(int CD) { return CD <= 24 ? 4 : 1; }

// position l of direction k -> NHWC pixel index inside the image (-1: padding); lrow = the x_dbl row (h2 * W2 + w2)
__device__ __forceinline__ int cs_pix(const CsGeom &g, int k, int l, int &lrow) {
    int h2, w2;
    if (k & 1) { w2 = l / g.H2; h2 = l - w2 * g.H2; }
    else { h2 = l / g.W2; w2 = l - h2 * g.W2; }
    lrow = h2 * g.W2 + w2;
    const int hh = 2 * h2 + (k & 1), ww = 2 * w2 + (k >> 1);
    return hh < g.H && ww < g.W ? hh * g.W + ww : -1;
}

// ---- 1. / 3. carry and main ---------------------------------------------------------------------------------------------
// ws_pa / ws_h / ws_g: [tile][row][n], row = b 4D + k D + d.  dxp: [split][4][B][L][CD].  part: [b ntiles + tile][4D][N + R + 2]
// (dA n | ddtw r | dD | ddtb).  NHWC (MAIN only): dx is [B,H,W,D] (fd_cross_scan_bwd_nhwc_f32) instead of [B,D,H,W].
template <int N, int R, bool MAIN, bool NHWC = false>
__global__ __launch_bounds__(CS_T) void cs_scan_kernel(const float *__restrict__ xc, const float *__restrict__ xdbl,
                                                      const float *__restrict__ dy, const float *__restrict__ dtw,
                                                      const float *__restrict__ dtb, const float *__restrict__ A,
                                                      const float *__restrict__ Ds, float *__restrict__ ws_pa,
                                                      float *__restrict__ ws_h, float *__restrict__ ws_g, float *__restrict__ dx,
                                                      float *__restrict__ dxp, float *__restrict__ part, const CsGeom g) {
    constexpr int CD = R + 2 * N, E = cs_e(CD), TILE = 64 * E, TP = TILE + 4, J = N + R + 2;
    __shared__ __attribute__((aligned(16))) float sT[CD * TP];            // x_dbl rows of the tile, [e][position]
    __shared__ __attribute__((aligned(16))) float sU[CS_SLAB * TP], sY[CS_SLAB * TP];   // u / dy of a slab, [channel][position]
    __shared__ int sPix[TILE];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = blockIdx.x / g.S, s = blockIdx.x - tile * g.S;
    const int bk = blockIdx.y, b = bk >> 2, k = bk & 3;
    const int Dg = g.D / g.S, cbeg = s * Dg;
    const int l0 = tile * TILE;
    const int64_t rows = (int64_t)g.B * 4 * g.D, HW = (int64_t)g.H * g.W;
    const float *xb = xdbl + ((int64_t)k * g.B + b) * g.L * CD;
    for (int lt = threadIdx.x; lt < TILE; lt += CS_T) {
        int lrow;
        sPix[lt] = l0 + lt < g.L ? cs_pix(g, k, l0 + lt, lrow) : -1;
    }
    for (int idx = threadIdx.x; idx < TILE * CD; idx += CS_T) {
        const int lt = idx / CD, e = idx - lt * CD;
        float v = 0.f;
        if (l0 + lt < g.L) {
            int lrow;
            cs_pix(g, k, l0 + lt, lrow);
            v = xb[(int64_t)lrow * CD + e];
        }
        sT[e * TP + lt] = v;
    }
    const int p0 = lane * E;                 // this lane's first position inside the tile
    float acc[CD][E];
#pragma unroll
    for (int e = 0; e < CD; ++e)
#pragma unroll
        for (int i = 0; i < E; ++i) acc[e][i] = 0.f;
    for (int cs = cbeg; cs < cbeg + Dg; cs += CS_SLAB) {
        __syncthreads();
        for (int idx = threadIdx.x; idx < TILE * (CS_SLAB / 4); idx += CS_T) {
            const int lt = idx >> 2, q = idx & 3;
            const int pix = sPix[lt];
            f32x4 uv = {0.f, 0.f, 0.f, 0.f}, yv = {0.f, 0.f, 0.f, 0.f};
            if (pix >= 0) {
                const int64_t o = ((int64_t)b * HW + pix) * g.D + cs + 4 * q;
                uv = *(const f32x4 *)(xc + o);
                yv = *(const f32x4 *)(dy + o);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                sU[(4 * q + j) * TP + lt] = uv[j];
                sY[(4 * q + j) * TP + lt] = yv[j];
            }
        }
        __syncthreads();
        for (int cl = wave * (CS_SLAB / CS_W); cl < (wave + 1) * (CS_SLAB / CS_W); ++cl) {
            const int d = cs + cl, kd = k * g.D + d;
            const int64_t row = (int64_t)b * 4 * g.D + kd;
            float uu[E], yy[E], dt[E], fac[E];
            float dl[E];
#pragma unroll
            for (int i = 0; i < E; ++i) {
                uu[i] = sU[cl * TP + p0 + i];
                yy[i] = sY[cl * TP + p0 + i];
                dl[i] = dtb[kd];
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const float w = dtw[(int64_t)kd * R + r];
#pragma unroll
                for (int i = 0; i < E; ++i) dl[i] += w * sT[r * TP + p0 + i];
            }
#pragma unroll
            for (int i = 0; i < E; ++i) {
                const float v = dl[i];
                dt[i] = l0 + p0 + i < g.L ? fd_softplus(v) : 0.f;     // past the end: the identity map a = 1, b = 0
                fac[i] = sbc_softplus_grad(v);
            }
            float gu[E], gt[E], pA[N];
            if constexpr (MAIN) {
                const float Dd = Ds[kd];
#pragma unroll
                for (int i = 0; i < E; ++i) gu[i] = Dd * yy[i], gt[i] = 0.f;
            }
#pragma unroll
            for (int n = 0; n < N; ++n) {
                const float An = A[(int64_t)kd * N + n];
                float Bv[E], Cv[E], a[E], hv[E], Pa, Pb, Qb;
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    Bv[i] = sT[(R + n) * TP + p0 + i];
                    Cv[i] = sT[(R + N + n) * TP + p0 + i];
                }
                sbc_fold(dt, An, Bv, Cv, uu, yy, a, hv, Pa, Pb, Qb);
                const int64_t kk = ((int64_t)tile * rows + row) * N + n;
                if constexpr (!MAIN) {
                    sbc_compose0(Pa, Pb, Qb);
                    if (lane == 0) {
                        ws_pa[kk] = Pa;
                        ws_h[kk] = Pb;
                        ws_g[kk] = Qb;
                    }
                } else {
                    float h, X;
                    sbc_carry_in(lane, Pa, Pb, Qb, ws_h[kk], ws_g[kk], h, X);
                    pA[n] = 0.f;
                    sbc_replay(dt, An, Bv, Cv, uu, yy, a, hv, h, X, acc[R + n], acc[R + N + n], gu, gt, pA[n]);
                }
            }
            if constexpr (MAIN) {
                if constexpr (NHWC) {
                    // NHWC dx: du, complete here, goes back over this channel's u in the slab buffer (read by this lane alone,
                    // above) and the slab leaves as it came, 16 bytes per (pixel, 4 channels), after the channel loop
#pragma unroll
                    for (int i = 0; i < E; ++i) sU[cl * TP + p0 + i] = gu[i];
                }
                float pD = 0.f, pBias = 0.f, pR[R];
#pragma unroll
                for (int i = 0; i < E; ++i) {
                    gt[i] = l0 + p0 + i < g.L ? gt[i] * fac[i] : 0.f;
                    pD += yy[i] * uu[i];
                    pBias += gt[i];
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float w = dtw[(int64_t)kd * R + r];
                    pR[r] = 0.f;
#pragma unroll
                    for (int i = 0; i < E; ++i) {
                        acc[r][i] += gt[i] * w;
                        pR[r] += gt[i] * sT[r * TP + p0 + i];
                    }
                }
                if constexpr (!NHWC) {
                    float *dxd = dx + ((int64_t)b * g.D + d) * HW;
#pragma unroll
                    for (int i = 0; i < E; ++i) {
                        const int pix = sPix[p0 + i];
                        if (pix >= 0) dxd[pix] = gu[i];
                    }
                }
                float *pp = part + ((int64_t)b * g.ntiles + tile) * (4 * (int64_t)g.D * J) + (int64_t)kd * J;
#pragma unroll
                for (int n = 0; n < N; ++n) {
                    const float v = wave_sum(pA[n]);
                    if (lane == 0) pp[n] = v;
                }
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float v = wave_sum(pR[r]);
                    if (lane == 0) pp[N + r] = v;
                }
                const float vD = wave_sum(pD), vB = wave_sum(pBias);
                if (lane == 0) {
                    pp[N + R] = vD;
                    pp[N + R + 1] = vB;
                }
            }
        }
        if constexpr (MAIN && NHWC) {
            __syncthreads();
            for (int idx = threadIdx.x; idx < TILE * (CS_SLAB / 4); idx += CS_T) {
                const int lt = idx >> 2, q = idx & 3;
                const int pix = sPix[lt];
                if (pix < 0) continue;
                const f32x4 v = {sU[(4 * q) * TP + lt], sU[(4 * q + 1) * TP + lt], sU[(4 * q + 2) * TP + lt],
                                 sU[(4 * q + 3) * TP + lt]};
                *(f32x4 *)(dx + ((int64_t)b * HW + pix) * g.D + cs + 4 * q) = v;
            }
        }
    }
    if constexpr (MAIN) {
        // the dxdbl rows of the tile: wave 0 + wave 1 + wave 2 + wave 3, through the (no longer needed) row buffer
        for (int w = 1; w < CS_W; ++w) {
            __syncthreads();
            if (wave == w)
#pragma unroll
                for (int e = 0; e < CD; ++e)
#pragma unroll
                    for (int i = 0; i < E; ++i) sT[e * TP + p0 + i] = acc[e][i];
            __syncthreads();
            if (wave == 0)
#pragma unroll
                for (int e = 0; e < CD; ++e)
#pragma unroll
                    for (int i = 0; i < E; ++i) acc[e][i] += sT[e * TP + p0 + i];
        }
        if (wave == 0) {
            float *ob = dxp + (((int64_t)s * 4 + k) * g.B + b) * g.L * CD;
#pragma unroll
            for (int i = 0; i < E; ++i) {
                if (l0 + p0 + i >= g.L) continue;
                int lrow;
                cs_pix(g, k, l0 + p0 + i, lrow);
#pragma unroll
                for (int e = 0; e < CD; ++e) ob[(int64_t)lrow * CD + e] = acc[e][i];
            }
        }
    }
}

// ---- 4. / 6. out[q] = sum_m p[m Q + q], m in order --------------------------------------------------------------------------
__global__ __launch_bounds__(CS_T) void cs_sum_kernel(const float *__restrict__ p, int M, int64_t Q, float *__restrict__ out) {
    const int64_t q = (int64_t)blockIdx.x * CS_T + threadIdx.x;
    if (q >= Q) return;
    float v = 0.f;
    for (int m = 0; m < M; ++m) v += p[(int64_t)m * Q + q];
    out[q] = v;
}

// ---- 7. the parameter partials: [m][4D][J] -> dA [4D][N], ddtw [4D][R], dDs [4D], ddtb [4D] ----------------------------
__global__ __launch_bounds__(CS_T) void cs_param_kernel(const float *__restrict__ p, int M, int KD, int N, int R,
                                                       float *__restrict__ dA, float *__restrict__ ddtw,
                                                       float *__restrict__ dDs, float *__restrict__ ddtb) {
    const int J = N + R + 2;
    const int64_t Q = (int64_t)KD * J;
    const int64_t q = (int64_t)blockIdx.x * CS_T + threadIdx.x;
    if (q >= Q) return;
    float v = 0.f;
    for (int m = 0; m < M; ++m) v += p[(int64_t)m * Q + q];
    const int kd = (int)(q / J), j = (int)(q - (int64_t)kd * J);
    if (j < N) dA[(int64_t)kd * N + j] = v;
    else if (j < N + R) ddtw[(int64_t)kd * R + (j - N)] = v;
    else if (j == N + R) dDs[kd] = v;
    else ddtb[kd] = v;
}

// ---- 5. the x_proj einsum's backward -------------------------------------------------------------------------------------
// One wave per (256 sub-grid rows, batch x direction, 64 channels), in blocks of 64 rows: dx[b, d, p] += sum_c W[k, c, d] dxdbl[c]
// with lane = row (W's 64 x CD slab in LDS, read as broadcasts), then lane = channel: wpart[b nxb + blk][k][c][d] +=
// dxdbl[c] u over the rows in order (u from xc: 256 coalesced bytes per pixel).  NHWC dx: the dx += moves into the second loop
// (lane = channel, 256 coalesced bytes per pixel there too), the sum over c in the same order.
constexpr int XB = 64, XBL = 4;
template <int N, int R, bool NHWC = false>
__global__ __launch_bounds__(64) void cs_xproj_kernel(const float *__restrict__ xc, const float *__restrict__ dxdbl,
                                                     const float *__restrict__ xw, float *__restrict__ dx,
                                                     float *__restrict__ wpart, const CsGeom g) {
    constexpr int CD = R + 2 * N, CS = CD + 1;
    __shared__ float sX[XB * CS], sW[CD * 64];
    __shared__ int sP[XB];
    const int lane = threadIdx.x;
    const int blk = blockIdx.x, bk = blockIdx.y, b = bk >> 2, k = bk & 3;
    const int d0 = blockIdx.z * 64;
    const int64_t HW = (int64_t)g.H * g.W;
    const float *xr = dxdbl + ((int64_t)k * g.B + b) * g.L * CD;
#pragma unroll
    for (int c = 0; c < CD; ++c) sW[c * 64 + lane] = xw[((int64_t)k * CD + c) * g.D + d0 + lane];
    float acc[CD];
#pragma unroll
    for (int c = 0; c < CD; ++c) acc[c] = 0.f;
    for (int sb = 0; sb < XBL; ++sb) {
        const int r0 = (blk * XBL + sb) * XB;
        if (r0 >= g.L) break;
        __syncthreads();
        {
            const int lr = r0 + lane;
            int pix = -1;
            if (lr < g.L) {
                const int h2 = lr / g.W2, w2 = lr - h2 * g.W2;
                const int hh = 2 * h2 + (k & 1), ww = 2 * w2 + (k >> 1);
                if (hh < g.H && ww < g.W) pix = hh * g.W + ww;
            }
            sP[lane] = pix;
        }
        for (int idx = lane; idx < XB * CD; idx += 64) {
            const int r = idx / CD, c = idx - r * CD;
            sX[r * CS + c] = r0 + r < g.L ? xr[(int64_t)r0 * CD + idx] : 0.f;
        }
        __syncthreads();
        // dx += W^T dxdbl: lane = row
        {
            float v[CD];
#pragma unroll
            for (int c = 0; c < CD; ++c) v[c] = sX[lane * CS + c];
            const int pix = sP[lane];
            if (!NHWC && pix >= 0) {
                float *dxp = dx + ((int64_t)b * g.D + d0) * HW + pix;
                for (int j = 0; j < 64; ++j) {
                    float t = 0.f;
#pragma unroll
                    for (int c = 0; c < CD; ++c) t += sW[c * 64 + j] * v[c];
                    dxp[(int64_t)j * HW] += t;
                }
            }
        }
        // dx_proj_w partial: lane = channel
        for (int r = 0; r < XB; ++r) {
            const int pix = sP[r];
            if (pix < 0) continue;
            const int64_t o = ((int64_t)b * HW + pix) * g.D + d0 + lane;
            const float u = xc[o];
#pragma unroll
            for (int c = 0; c < CD; ++c) acc[c] += sX[r * CS + c] * u;
            if constexpr (NHWC) {
                float t = 0.f;
#pragma unroll
                for (int c = 0; c < CD; ++c) t += sW[c * 64 + lane] * sX[r * CS + c];
                dx[o] += t;
            }
        }
    }
    float *wp = wpart + (((int64_t)b * g.nxb + blk) * 4 + k) * CD * g.D + d0 + lane;
#pragma unroll
    for (int c = 0; c < CD; ++c) wp[(int64_t)c * g.D] = acc[c];
}

// ---- the forward's layout move: NCHW -> NHWC through a 64 x 64 LDS tile ------------------------------------------------
__global__ __launch_bounds__(CS_T) void cs_nchw_nhwc_kernel(const float *__restrict__ x, float *__restrict__ out, int D,
                                                           int64_t HW) {
    __shared__ float t[64][65];
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int c0 = blockIdx.y * 64, b = blockIdx.z;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int c = ty; c < 64; c += CS_W)
        t[c][tx] = p0 + tx < HW ? x[((int64_t)b * D + c0 + c) * HW + p0 + tx] : 0.f;
    __syncthreads();
    for (int p = ty; p < 64; p += CS_W)
        if (p0 + p < HW) out[((int64_t)b * HW + p0 + p) * D + c0 + tx] = t[tx][p];
}

struct CsLayout {
    CsGeom g;
    int tile;                                     // positions per tile of the scan kernels: 64 cs_e(CD)
    int64_t comp, part, dxd, dxp, wpart, total;   // floats: each composite array, parameter partials, dxdbl, its split partials,
};                                                // the dx_proj_w partials

// static LDS of cs_scan_kernel<N, R> (sT, sU, sY, sPix) and of cs_xproj_kernel<N, R> (sX, sW, sP), as declared there: host-side
// restatements for fd_cross_scan_bwd_geom, held to the compiler's own figures by tests/test_scan_bwd_cases_cpu.py
constexpr int cs_scan_lds(int CD) { return ((CD + 2 * CS_SLAB) * (64 * cs_e(CD) + 4) + 64 * cs_e(CD)) * 4; }
constexpr int cs_xproj_lds(int CD) { return (XB * (CD + 1) + CD * 64 + XB) * 4; }

CsLayout cs_layout(int B, int H, int W, int D, int N, int R) {
    CsLayout w;
    CsGeom &g = w.g;
    g.B = B; g.H = H; g.W = W; g.D = D; g.N = N; g.R = R; g.CD = R + 2 * N;
    g.H2 = (H + 1) / 2; g.W2 = (W + 1) / 2; g.L = g.H2 * g.W2;
    const int tile = w.tile = 64 * cs_e(g.CD);
    g.ntiles = (g.L + tile - 1) / tile;
    // channel splits: enough workgroups for the chip from ONE slice (4 directions x tiles x splits >= 512), at least 64 channels
    // per split -- a function of the shape, never of the batch
    g.S = 1;
    while (4 * g.ntiles * g.S < 512 && D % (2 * g.S * 64) == 0) g.S *= 2;
    g.nxb = (g.L + XB * XBL - 1) / (XB * XBL);
    const int64_t rows = (int64_t)B * 4 * D;
    w.comp = round4((int64_t)g.ntiles * rows * N);
    w.part = round4((int64_t)B * g.ntiles * 4 * D * (N + R + 2));
    w.dxd = round4((int64_t)4 * B * g.L * g.CD);
    w.dxp = g.S > 1 ? round4((int64_t)g.S * 4 * B * g.L * g.CD) : 0;
    w.wpart = round4((int64_t)B * g.nxb * 4 * g.CD * D);
    w.total = 3 * w.comp + w.part + w.dxd + w.dxp + w.wpart;
    return w;
}

bool cs_shape_ok(int B, int H, int W, int D, int N, int R) {
    // (B <= 16383: the scan and x_proj launches carry batch x direction in grid.y, 4 B <= 65535)
    return B > 0 && B <= 16383 && H > 0 && W > 0 && D > 0 && D % 64 == 0 && (N == 4 || N == 8 || N == 16 || N == 32) &&
           (R == 2 || R == 4 || R == 8 || R == 16 || R == 32) && (int64_t)H * W * D * 4 < (1ll << 31);
}

// the shape check of every entry, with the entry's name in the error
int cs_shape(const char *name, int B, int H, int W, int D, int N, int R) {
    FD_REQUIRE(cs_shape_ok(B, H, W, D, N, R),
               "%s: unsupported shape B=%d H=%d W=%d d_inner=%d d_state=%d dt_rank=%d (d_inner %% 64 == 0, "
               "N in {4,8,16,32}, R in {2,4,8,16,32}, B <= 16383)", name, B, H, W, D, N, R);
    return FD_OK;
}

template <int N, int R, bool NHWC>
void cs_launch(const CsLayout &w, const float *xc, const float *xdbl, const float *xw, const float *dtw, const float *dtb,
               const float *A, const float *Ds, const float *dy, float *dx, float *dxw, float *ddtw, float *ddtb, float *dA,
               float *dDs, float *ws, hipStream_t st) {
    const CsGeom &g = w.g;
    float *pa = ws, *hh = ws + w.comp, *gg = ws + 2 * w.comp, *part = ws + 3 * w.comp;
    float *dxd = part + w.part, *dxp = dxd + w.dxd, *wpart = dxp + w.dxp;
    const dim3 grid((unsigned)(g.ntiles * g.S), (unsigned)(g.B * 4));
    hipLaunchKernelGGL((cs_scan_kernel<N, R, false>), grid, dim3(CS_T), 0, st, xc, xdbl, dy, dtw, dtb, A, Ds, pa, hh, gg,
                       dx, nullptr, nullptr, g);
    const int64_t RN = (int64_t)g.B * 4 * g.D * N;
    scan_bwd_chain_launch(pa, hh, gg, RN, g.ntiles, st);
    hipLaunchKernelGGL((cs_scan_kernel<N, R, true, NHWC>), grid, dim3(CS_T), 0, st, xc, xdbl, dy, dtw, dtb, A, Ds, pa, hh, gg, dx,
                       g.S > 1 ? dxp : dxd, part, g);
    if (g.S > 1) {
        const int64_t tot = (int64_t)4 * g.B * g.L * g.CD;
        hipLaunchKernelGGL(cs_sum_kernel, dim3((unsigned)((tot + CS_T - 1) / CS_T)), dim3(CS_T), 0, st, dxp, g.S, tot, dxd);
    }
    hipLaunchKernelGGL((cs_xproj_kernel<N, R, NHWC>), dim3((unsigned)g.nxb, (unsigned)(g.B * 4), (unsigned)(g.D / 64)), dim3(64), 0,
                       st, xc, dxd, xw, dx, wpart, g);
    const int64_t Qw = (int64_t)4 * g.CD * g.D;
    hipLaunchKernelGGL(cs_sum_kernel, dim3((unsigned)((Qw + CS_T - 1) / CS_T)), dim3(CS_T), 0, st, wpart, g.B * g.nxb, Qw, dxw);
    const int64_t Qp = (int64_t)4 * g.D * (N + R + 2);
    hipLaunchKernelGGL(cs_param_kernel, dim3((unsigned)((Qp + CS_T - 1) / CS_T)), dim3(CS_T), 0, st, part, g.B * g.ntiles,
                       4 * g.D, N, R, dA, ddtw, dDs, ddtb);
}

}  // namespace

extern "C" int64_t fd_cross_scan_bwd_ws_floats(int B, int H, int W, int D, int N, int R) {
    if (!cs_shape_ok(B, H, W, D, N, R)) return 0;
    return cs_layout(B, H, W, D, N, R).total;
}

// What fd_cross_scan_bwd_f32 / _nhwc_f32 launch for this shape: cs_layout's own values, host only (tests/scan_bwd_cases.py).
extern "C" int fd_cross_scan_bwd_geom(int B, int H, int W, int D, int N, int R, int32_t out[8]) {
    FD_REQUIRE(out, "fd_cross_scan_bwd_geom: null pointer");
    for (int i = 0; i < 8; ++i) out[i] = 0;
    if (int rc = cs_shape("fd_cross_scan_bwd_geom", B, H, W, D, N, R)) return rc;
    const CsLayout w = cs_layout(B, H, W, D, N, R);
    const CsGeom &g = w.g;
    out[0] = cs_e(g.CD);
    out[1] = w.tile;
    out[2] = g.L;
    out[3] = g.ntiles;
    out[4] = g.L - (g.ntiles - 1) * w.tile;
    out[5] = g.S;
    out[6] = g.nxb;
    out[7] = cs_scan_lds(g.CD) > cs_xproj_lds(g.CD) ? cs_scan_lds(g.CD) : cs_xproj_lds(g.CD);
    return FD_OK;
}

namespace {

// the x_proj gather (src/emamba2.py:335) as the engine's fp32 parity mode runs it -- 4 stride-2 sub-grids, exact fp32, out-of-image
// pixels of odd sizes zero-filled -- and the scan, from xc [B,H,W,D]
int cs_fwd_from_xc(const float *xc, const float *x_proj_w, const float *dtw, const float *dtb, const float *A, const float *Ds,
                   float *xdbl, float *y, float *ws, int B, int H, int W, int D, int N, int R, void *stream) {
    const int H2 = (H + 1) / 2, W2 = (W + 1) / 2, CD = R + 2 * N;
    fd_conv_params p = {};
    p.dtype = FD_F32;
    p.out_f32 = 1;
    p.in0 = xc;
    p.c0 = D; p.ld0 = D; p.off0 = 0;
    p.B = B; p.H = H; p.W = W;
    p.KH = 1; p.KW = 1; p.stride = 2; p.pad_h = 0; p.pad_w = 0;
    p.OH = H2; p.OW = W2;
    p.ndir = 4;
    p.weight = x_proj_w;
    p.w_dir_stride = (int64_t)CD * D;
    p.Cout = CD;
    p.out = xdbl; p.ldo = CD; p.offo = 0;
    p.out_dir_stride = (int64_t)B * H2 * W2 * CD;
    p.gn_groups = 8;
    p.ln_eps = 1e-5f;
    int rc = fd_conv2d(&p, stream);
    if (rc != FD_OK) return rc;
    return fd_selective_scan(FD_F32, xc, xdbl, dtw, dtb, A, Ds, y, ws, B, H, W, D, N, R, stream);
}

int cs_bwd(const char *name, int nhwc, const float *xc, const float *xdbl, const float *x_proj_w, const float *dtw,
           const float *dtb, const float *A, const float *Ds, const float *dy, float *dx, float *dx_proj_w, float *ddtw,
           float *ddtb, float *dA, float *dDs, float *ws, int B, int H, int W, int D, int N, int R, void *stream) {
    FD_REQUIRE(xc && xdbl && x_proj_w && dtw && dtb && A && Ds && dy && dx && dx_proj_w && ddtw && ddtb && dA && dDs && ws,
               "%s: null pointer", name);
    if (int rc = cs_shape(name, B, H, W, D, N, R)) return rc;
    FD_REQUIRE((((uintptr_t)xc | (uintptr_t)dy | (uintptr_t)ws | (nhwc ? (uintptr_t)dx : 0)) & 15) == 0,
               "%s: tensors must be 16-byte aligned", name);
    const CsLayout w = cs_layout(B, H, W, D, N, R);
    const hipStream_t st = (hipStream_t)stream;
#define FD_CS_R(NN, RR) \
    case RR:                                                                                                            \
        if (nhwc) cs_launch<NN, RR, true>(w, xc, xdbl, x_proj_w, dtw, dtb, A, Ds, dy, dx, dx_proj_w, ddtw, ddtb, dA, dDs, ws, st); \
        else cs_launch<NN, RR, false>(w, xc, xdbl, x_proj_w, dtw, dtb, A, Ds, dy, dx, dx_proj_w, ddtw, ddtb, dA, dDs, ws, st);    \
        break;
#define FD_CS_N(NN)                                                                          \
    case NN:                                                                                 \
        switch (R) { FD_CS_R(NN, 2) FD_CS_R(NN, 4) FD_CS_R(NN, 8) FD_CS_R(NN, 16) FD_CS_R(NN, 32) } \
        break;
    switch (N) { FD_CS_N(4) FD_CS_N(8) FD_CS_N(16) FD_CS_N(32) }
#undef FD_CS_N
#undef FD_CS_R
    FD_LAUNCH_OK(name);
    return FD_OK;
}

}  // namespace

extern "C" int fd_cross_scan_fwd_f32(const float *x, const float *x_proj_w, const float *dtw, const float *dtb, const float *A,
                                     const float *Ds, float *xc, float *xdbl, float *y, float *ws, int B, int H, int W, int D,
                                     int N, int R, void *stream) {
    FD_REQUIRE(x && x_proj_w && dtw && dtb && A && Ds && xc && xdbl && y && ws, "fd_cross_scan_fwd_f32: null pointer");
    if (int rc = cs_shape("fd_cross_scan_fwd_f32", B, H, W, D, N, R)) return rc;
    FD_REQUIRE((((uintptr_t)x | (uintptr_t)xc | (uintptr_t)xdbl | (uintptr_t)y | (uintptr_t)x_proj_w) & 15) == 0,
               "fd_cross_scan_fwd_f32: tensors must be 16-byte aligned");
    const hipStream_t st = (hipStream_t)stream;
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(cs_nchw_nhwc_kernel, dim3((unsigned)((HW + 63) / 64), (unsigned)(D / 64), (unsigned)B), dim3(CS_T), 0,
                       st, x, xc, D, HW);
    FD_LAUNCH_OK("fd_cross_scan_fwd_f32 (layout)");
    return cs_fwd_from_xc(xc, x_proj_w, dtw, dtb, A, Ds, xdbl, y, ws, B, H, W, D, N, R, stream);
}

extern "C" int fd_cross_scan_fwd_nhwc_f32(const float *xc, const float *x_proj_w, const float *dtw, const float *dtb,
                                          const float *A, const float *Ds, float *xdbl, float *y, float *ws, int B, int H, int W,
                                          int D, int N, int R, void *stream) {
    FD_REQUIRE(xc && x_proj_w && dtw && dtb && A && Ds && xdbl && y && ws, "fd_cross_scan_fwd_nhwc_f32: null pointer");
    if (int rc = cs_shape("fd_cross_scan_fwd_nhwc_f32", B, H, W, D, N, R)) return rc;
    FD_REQUIRE((((uintptr_t)xc | (uintptr_t)xdbl | (uintptr_t)y | (uintptr_t)x_proj_w) & 15) == 0,
               "fd_cross_scan_fwd_nhwc_f32: tensors must be 16-byte aligned");
    return cs_fwd_from_xc(xc, x_proj_w, dtw, dtb, A, Ds, xdbl, y, ws, B, H, W, D, N, R, stream);
}

extern "C" int fd_cross_scan_bwd_f32(const float *xc, const float *xdbl, const float *x_proj_w, const float *dtw,
                                     const float *dtb, const float *A, const float *Ds, const float *dy, float *dx, float *dx_proj_w,
                                     float *ddtw, float *ddtb, float *dA, float *dDs, float *ws, int B, int H, int W, int D, int N,
                                     int R, void *stream) {
    return cs_bwd("fd_cross_scan_bwd_f32", 0, xc, xdbl, x_proj_w, dtw, dtb, A, Ds, dy, dx, dx_proj_w, ddtw, ddtb, dA, dDs, ws, B,
                  H, W, D, N, R, stream);
}

extern "C" int fd_cross_scan_bwd_nhwc_f32(const float *xc, const float *xdbl, const float *x_proj_w, const float *dtw,
                                          const float *dtb, const float *A, const float *Ds, const float *dy, float *dxc,
                                          float *dx_proj_w, float *ddtw, float *ddtb, float *dA, float *dDs, float *ws, int B, int H,
                                          int W, int D, int N, int R, void *stream) {
    return cs_bwd("fd_cross_scan_bwd_nhwc_f32", 1, xc, xdbl, x_proj_w, dtw, dtb, A, Ds, dy, dxc, dx_proj_w, ddtw, ddtb, dA, dDs, ws,
                  B, H, W, D, N, R, stream);
}
