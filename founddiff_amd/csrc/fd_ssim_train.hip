// fd_ssim_train.hip -- the structural term of the training loss: 1 - SSIM of the one-step estimate against x_start, with its
// gradient, and the image pair validation measures SSIM on.  fp32, the same in both builds of the library.
//
//   fd_ssim_loss_f32     loss += scale (1 - mean_b mean_i S), dout += its gradient; items[b] = the slice's mean S
//   fd_onestep_u01_f32   u(clamp(x_input - clamp(pred))) and u(x_start): the pair fd_metrics reads in Trainer.validate
//
// S is fd_metrics.hip's SSIM map -- the 11-tap Gaussian, sigma 1.5, normalised, separable, reflect padding of 5, C1 = 0.01^2,
// C2 = 0.03^2 on [0, 1] images -- WITHOUT its clamp to [0, 1]: S goes below 0 exactly where the gradient is needed.  The images
// are formed on the load: y = (x_start + 1) / 2, p = (x_input - out + 1) / 2 for a residual output, (out + 1) / 2 for an x0
// output; nothing is clamped.
//
// Pass 1, one workgroup per 16 x 16 tile: the halo of p and y in LDS, the five filtered moments by the direct 121-tap sum, S, and
// the three coefficient maps of the backward (A, dS/dv, dS/dc; include/founddiff_hip.h has the formulas) to the workspace; one
// partial sum of S per workgroup.  The moments are taken about two per-tile constants (p and y at the tile's first pixel): the
// variances and the covariance do not depend on them, the means are shifted back.  That takes the cancellation out of
// E[x^2] - mu^2, whose fp32 error (1e-8 for values near 0.3) is otherwise 1e-5 of C2; constant images become exact.
// Pass 2, the same grid: the adjoint of the reflect-padded filter applied to the three maps, gathered per output pixel.  Per
// axis of length n, the filter's tap d at position i reads x[r(i + d)], r the reflection; so output j collects source i with
// the weight g[j - i] + g[-j - i] (where i + d = -j < 0, so 1 <= j) + g[2(n - 1) - j - i] (where i + d = 2(n - 1) - j >= n, so
// j <= n - 2), each present where its tap index lies in [-5, 5].  Every source of j lies within 5 of it, so the tile's halo of
// the maps (zero outside the image) serves it, and the 2-D weight is the product of the axes'.  For n in 6 .. 10 both folds can
// land on one j: they are two terms of one weight.  Then 2p . and y . , the factor -+scale / (2 N), one rounding to fp32 and
// one plain fp32 add onto dout: the sum is bitwise the sum of the separate gradients.  Each pixel is owned by one lane.
// Finalise: a slice's partials in index order in double (as metrics_finalize_kernel) -> items[b]; the term is
// (float)(scale (1 - mean_b (double)items[b])), added onto the loss with one fp32 add.
//
// No atomics.  A slice's items[b] and maps do not depend on the rest of its batch.
#include "fd_train_common.h"

namespace {

constexpr int ST = 16;           // output tile
constexpr int SR = 5;            // window radius (11 taps)
constexpr int SH = ST + 2 * SR;  // halo tile

__device__ __forceinline__ int ssim_reflect(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    // halo positions of tiles that hang over a small image (n < 11) can reflect twice: they only feed masked-out outputs, but
    // the load must stay inside the buffer
    return min(max(i, 0), n - 1);
}

// the 11 normalised weights, rounded once from double
__device__ __forceinline__ void ssim_window(float *g, int tid) {
    if (tid < 11) {
        double s = 0.0;
        for (int i = 0; i < 11; ++i) s += exp(-(double)((i - 5) * (i - 5)) / 4.5);
        g[tid] = (float)(exp(-(double)((tid - 5) * (tid - 5)) / 4.5) / s);
    }
}

// p and y in [0, 1] units at one pixel; every rounding is spelled out, so that both passes form the same bits
template <bool RES>
__device__ __forceinline__ float ssim_pred(const float *__restrict__ out, const float *__restrict__ xin, int64_t i) {
    const float v = RES ? __fsub_rn(xin[i], out[i]) : out[i];
    return __fmul_rn(__fadd_rn(v, 1.f), 0.5f);
}
__device__ __forceinline__ float ssim_tgt(const float *__restrict__ x0, int64_t i) { return __fmul_rn(__fadd_rn(x0[i], 1.f), 0.5f); }

// grid (tile x, tile y, b).  coef: [b][3][H][W] or null (no backward follows); part: [b][tiles]
template <bool RES>
__global__ __launch_bounds__(256) void ssim_fwd_kernel(const float *__restrict__ out, const float *__restrict__ xin,
                                                      int64_t xin_bstride, const float *__restrict__ x0, int H, int W,
                                                      float *__restrict__ coef, float *__restrict__ part) {
    __shared__ float sp[SH][SH + 1], sy[SH][SH + 1];
    __shared__ float g[11];
    __shared__ float red[4];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int b = blockIdx.z, bx0 = blockIdx.x * ST, by0 = blockIdx.y * ST;
    const int64_t npix = (int64_t)H * W;
    const float *o = out + (int64_t)b * npix, *t = x0 + (int64_t)b * npix;
    const float *xi = RES ? xin + (int64_t)b * xin_bstride : nullptr;
    ssim_window(g, tid);
    const int64_t first = (int64_t)by0 * W + bx0;                     // the tile's first pixel: always inside the image
    const float shp = ssim_pred<RES>(o, xi, first), shy = ssim_tgt(t, first);
    for (int i = tid; i < SH * SH; i += 256) {
        const int hy = i / SH, hx = i - hy * SH;
        const int64_t at = (int64_t)ssim_reflect(by0 + hy - SR, H) * W + ssim_reflect(bx0 + hx - SR, W);
        sp[hy][hx] = __fsub_rn(ssim_pred<RES>(o, xi, at), shp);
        sy[hy][hx] = __fsub_rn(ssim_tgt(t, at), shy);
    }
    __syncthreads();
    float ss = 0.f;
    const int x = bx0 + tx, y = by0 + ty;
    if (x < W && y < H) {
        float m1 = 0.f, m2 = 0.f, s11 = 0.f, s22 = 0.f, s12 = 0.f;
        for (int dy = 0; dy < 11; ++dy)
#pragma unroll
            for (int dx = 0; dx < 11; ++dx) {
                const float w = g[dy] * g[dx];
                const float a = sp[ty + dy][tx + dx], c = sy[ty + dy][tx + dx];
                const float wa = w * a, wc = w * c;
                m1 += wa; m2 += wc;
                s11 = fmaf(wa, a, s11); s22 = fmaf(wc, c, s22); s12 = fmaf(wa, c, s12);
            }
        const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
        const float vp = s11 - m1 * m1, vy = s22 - m2 * m2, cv = s12 - m1 * m2;
        const float mp = m1 + shp, my = m2 + shy;
        const float a1 = 2.f * mp * my + C1, a2 = 2.f * cv + C2, b1 = mp * mp + my * my + C1, b2 = vp + vy + C2;
        const float r1 = 1.f / b1, r2 = 1.f / b2;
        const float S = (a1 * a2) * (r1 * r2);
        ss = S;
        if (coef) {
            const float dmu = 2.f * my * a2 * (r1 * r2) - S * 2.f * mp * r1;
            const float dv = -S * r2, dc = 2.f * a1 * (r1 * r2);
            float *cf = coef + (int64_t)b * 3 * npix + (int64_t)y * W + x;
            cf[0] = dmu - 2.f * mp * dv - my * dc;
            cf[npix] = dv;
            cf[2 * npix] = dc;
        }
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) red[tid >> 6] = ss;
    __syncthreads();
    if (tid == 0)
        part[((int64_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// the adjoint's weight of source i = j + k - 5 (k = 0 .. 10) at output j, one axis of length n
__device__ __forceinline__ float ssim_adjoint_weight(const float *g, int j, int k, int n) {
    const int i = j + k - SR;
    if (j >= n || i < 0 || i >= n) return 0.f;
    float w = g[SR + j - i];                                          // i + d = j
    const int d2 = -j - i, d3 = 2 * (n - 1) - j - i;
    if (j >= 1 && d2 >= -SR) w += g[SR + d2];                          // i + d = -j, reflected at 0
    if (j <= n - 2 && d3 <= SR) w += g[SR + d3];                       // i + d = 2 (n - 1) - j, reflected at n - 1
    return w;
}

// grid (tile x, tile y, b).  dout (+)= cf (W^T A + 2 p W^T dS/dv + y W^T dS/dc), cf = -+scale / (2 N) rounded to fp32 by the host
template <bool RES>
__global__ __launch_bounds__(256) void ssim_bwd_kernel(const float *__restrict__ out, const float *__restrict__ xin,
                                                      int64_t xin_bstride, const float *__restrict__ x0, int H, int W,
                                                      const float *__restrict__ coef, float cf, int accumulate,
                                                      float *__restrict__ dout) {
    __shared__ float sc[3][SH][SH + 1];
    __shared__ float g[11];
    __shared__ float wy[ST][12], wx[ST][12];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int b = blockIdx.z, bx0 = blockIdx.x * ST, by0 = blockIdx.y * ST;
    const int64_t npix = (int64_t)H * W;
    const float *cb = coef + (int64_t)b * 3 * npix;
    ssim_window(g, tid);
    for (int i = tid; i < SH * SH; i += 256) {
        const int hy = i / SH, hx = i - hy * SH;
        const int yy = by0 + hy - SR, xx = bx0 + hx - SR;
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int64_t at = in ? (int64_t)yy * W + xx : 0;
        sc[0][hy][hx] = in ? cb[at] : 0.f;
        sc[1][hy][hx] = in ? cb[npix + at] : 0.f;
        sc[2][hy][hx] = in ? cb[2 * npix + at] : 0.f;
    }
    __syncthreads();                                                  // g is written
    if (tid < ST * 11) {
        const int j = tid / 11, k = tid - j * 11;
        wy[j][k] = ssim_adjoint_weight(g, by0 + j, k, H);
        wx[j][k] = ssim_adjoint_weight(g, bx0 + j, k, W);
    }
    __syncthreads();
    const int x = bx0 + tx, y = by0 + ty;
    if (x >= W || y >= H) return;
    float ta = 0.f, tv = 0.f, tc = 0.f;
    for (int dy = 0; dy < 11; ++dy)
#pragma unroll
        for (int dx = 0; dx < 11; ++dx) {
            const float w = wy[ty][dy] * wx[tx][dx];
            ta = fmaf(w, sc[0][ty + dy][tx + dx], ta);
            tv = fmaf(w, sc[1][ty + dy][tx + dx], tv);
            tc = fmaf(w, sc[2][ty + dy][tx + dx], tc);
        }
    const int64_t at = (int64_t)y * W + x, gi = (int64_t)b * npix + at;
    const float p = ssim_pred<RES>(out + (int64_t)b * npix, RES ? xin + (int64_t)b * xin_bstride : nullptr, at);
    const float yv = ssim_tgt(x0 + (int64_t)b * npix, at);
    const float gp = ta + 2.f * p * tv + yv * tc;
    const float r = __fmul_rn(gp, cf);                                 // rounded to fp32 here: no fma with the add below
    dout[gi] = accumulate ? __fadd_rn(dout[gi], r) : r;
}

// grid (b): items[b] = the slice's partials in index order, in double, over the slice's pixels
__global__ __launch_bounds__(256) void ssim_items_kernel(const float *__restrict__ part, int nblk, double inv_n,
                                                        float *__restrict__ items) {
    __shared__ double sh[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < nblk; i += 256) s += (double)part[(int64_t)b * nblk + i];
    sh[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) items[b] = (float)(sh[0] * inv_n);
}

// one workgroup: loss (+)= (float)(scale (1 - mean_b items[b])), the mean in double in a fixed order
__global__ __launch_bounds__(256) void ssim_term_kernel(const float *__restrict__ items, int B, double scale, int accumulate,
                                                       float *__restrict__ loss) {
    __shared__ double sh[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < B; i += 256) s += (double)items[i];
    sh[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) sh[tid] += sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const float term = (float)(scale * (1.0 - sh[0] / (double)B));
        loss[0] = accumulate ? __fadd_rn(loss[0], term) : term;
    }
}

__device__ __forceinline__ float clamp_pm1(float v) { return fminf(fmaxf(v, -1.f), 1.f); }
__device__ __forceinline__ float unit01(float v) { return fminf(fmaxf(__fmul_rn(__fadd_rn(v, 1.f), 0.5f), 0.f), 1.f); }

template <bool VEC>
__global__ __launch_bounds__(256) void onestep_u01_kernel(const float *__restrict__ pred, const float *__restrict__ xin,
                                                         int64_t xin_bstride, const float *__restrict__ x0, int64_t npix,
                                                         float *__restrict__ est, float *__restrict__ tgt) {
    const int64_t i0 = 4 * ((int64_t)blockIdx.x * 256 + threadIdx.x);
    if (i0 >= npix) return;
    const int b = blockIdx.y;
    const int n = (int)min((int64_t)4, npix - i0);
    float p[4], xi[4], xs[4], e[4], t[4];
    load4<VEC>(pred + b * npix + i0, n, p);
    load4<VEC>(xin + b * xin_bstride + i0, n, xi);
    load4<VEC>(x0 + b * npix + i0, n, xs);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        e[k] = unit01(clamp_pm1(__fsub_rn(xi[k], clamp_pm1(p[k]))));
        t[k] = unit01(xs[k]);
    }
    store4<VEC>(est + b * npix + i0, n, e);
    store4<VEC>(tgt + b * npix + i0, n, t);
}

int ssim_nblk(int H, int W) { return cdiv(H, ST) * cdiv(W, ST); }

bool ssim_shape_ok(int B, int H, int W) { return B > 0 && B <= 65535 && H > SR && W > SR && H <= 32768 && W <= 32768; }

}  // namespace

extern "C" int64_t fd_ssim_loss_ws_floats(int B, int H, int W) {
    if (!ssim_shape_ok(B, H, W)) return 0;
    return round4(3 * (int64_t)B * H * W) + round4((int64_t)B * ssim_nblk(H, W)) + round4(B);
}

extern "C" int fd_ssim_loss_f32(const float *out, const float *x_input, int64_t x_input_bstride, const float *x_start, int residual,
                                double scale, float *loss, float *items, float *dout, int accumulate, float *ws, int B, int H,
                                int W, void *stream) {
    FD_REQUIRE(out && x_start && ws, "fd_ssim_loss_f32: null pointer");
    FD_REQUIRE(!residual || x_input, "fd_ssim_loss_f32: a residual output needs x_input");
    FD_REQUIRE(B > 0 && B <= 65535, "fd_ssim_loss_f32: unsupported shape B=%d (at most 65535 slices)", B);
    FD_REQUIRE(H > SR && W > SR, "fd_ssim_loss_f32: unsupported shape H=%d W=%d (reflect padding of 5 needs H, W >= 6)", H, W);
    FD_REQUIRE(ssim_shape_ok(B, H, W), "fd_ssim_loss_f32: unsupported shape B=%d H=%d W=%d (H, W <= 32768)", B, H, W);
    FD_REQUIRE(!residual || x_input_bstride >= (int64_t)H * W, "fd_ssim_loss_f32: x_input_bstride %lld is below H W",
               (long long)x_input_bstride);
    const hipStream_t st = (hipStream_t)stream;
    const int nblk = ssim_nblk(H, W);
    float *coef = ws, *part = coef + round4(3 * (int64_t)B * H * W), *it = items ? items : part + round4((int64_t)B * nblk);
    const dim3 grid((unsigned)cdiv(W, ST), (unsigned)cdiv(H, ST), (unsigned)B);
    float *cw = dout ? coef : nullptr;
    if (residual) hipLaunchKernelGGL(ssim_fwd_kernel<true>, grid, dim3(256), 0, st, out, x_input, x_input_bstride, x_start, H, W, cw, part);
    else hipLaunchKernelGGL(ssim_fwd_kernel<false>, grid, dim3(256), 0, st, out, x_input, x_input_bstride, x_start, H, W, cw, part);
    if (dout) {
        // d term / d out = -+1/2 d term / d p, d term / d p = -scale (...) / N: + for a residual output, - for an x0 output
        const float cf = (float)((residual ? 0.5 : -0.5) * scale / ((double)B * H * W));
        if (residual)
            hipLaunchKernelGGL(ssim_bwd_kernel<true>, grid, dim3(256), 0, st, out, x_input, x_input_bstride, x_start, H, W, coef, cf,
                               accumulate, dout);
        else
            hipLaunchKernelGGL(ssim_bwd_kernel<false>, grid, dim3(256), 0, st, out, x_input, x_input_bstride, x_start, H, W, coef, cf,
                               accumulate, dout);
    }
    hipLaunchKernelGGL(ssim_items_kernel, dim3((unsigned)B), dim3(256), 0, st, part, nblk, 1.0 / ((double)H * W), it);
    if (loss) hipLaunchKernelGGL(ssim_term_kernel, dim3(1), dim3(256), 0, st, it, B, scale, accumulate, loss);
    FD_LAUNCH_OK("fd_ssim_loss_f32");
    return FD_OK;
}

extern "C" int fd_onestep_u01_f32(const float *pred, const float *x_input, int64_t x_input_bstride, const float *x_start, float *est,
                                  float *tgt, int B, int64_t npix, void *stream) {
    FD_REQUIRE(pred && x_input && x_start && est && tgt, "fd_onestep_u01_f32: null pointer");
    FD_REQUIRE(B > 0 && B <= 65535 && npix > 0 && npix < (1ll << 33) && x_input_bstride >= npix,
               "fd_onestep_u01_f32: unsupported shape B=%d npix=%lld x_input_bstride=%lld (B <= 65535, npix < 2^33, stride >= npix)",
               B, (long long)npix, (long long)x_input_bstride);
    const bool vec = npix % 4 == 0 && x_input_bstride % 4 == 0 && al16(pred) && al16(x_input) && al16(x_start) && al16(est) && al16(tgt);
    const dim3 grid((unsigned)(((npix + 3) / 4 + 255) / 256), (unsigned)B);
    if (vec) hipLaunchKernelGGL(onestep_u01_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, pred, x_input, x_input_bstride, x_start, npix, est, tgt);
    else hipLaunchKernelGGL(onestep_u01_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, pred, x_input, x_input_bstride, x_start, npix, est, tgt);
    FD_LAUNCH_OK("fd_onestep_u01_f32");
    return FD_OK;
}
