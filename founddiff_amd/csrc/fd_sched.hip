// fd_sched.hip -- the ancestral sampler's per-step scheduler work without a host in the loop, and its step noise
// as a counter-based stream keyed per SLICE (src/DADiff.py:1222-1273: p_sample_loop / p_sample / q_posterior).
//
// The reference draws `torch.randn_like(x)` from the device generator at every step (1228): the noise a slice
// receives depends on its position in the batch and on everything drawn before it, so a volume sharded over ranks
// (BASELINE configs[3]: 64 slices over 8 GPUs) would depend on the world size.  Here the noise of (slice, step,
// pixel) is a pure function of (seed of the slice, t, pixel index): Philox4x32-10 keyed by the slice's 64-bit seed,
// counter = (pixel / 4, t, domain tag, 0), Box-Muller on the four 32-bit outputs.  Nothing is stored, nothing is
// drawn on the host, and the same slice gets the same stream on any rank, in any batch, on either HIP stream.
// oracle/keyed_noise.py restates the generator in numpy (tests/).
//
// fd_ancestral_begin / fd_res_posterior_step_keyed read the timestep from a device counter and the posterior
// coefficients from a device table, so a chunk of steps can be captured in one HIP graph and replayed.
#include "fd_common.h"
#include "fd_keyed_noise.h"
#include "fd_obj_pixel.h"

namespace {

__device__ __forceinline__ float clamp1s(float v) { return fd_clamp1(v); }

__global__ void keyed_normal_kernel(const int64_t *__restrict__ seeds, int t, float *__restrict__ out, int64_t npix) {
    const int b = blockIdx.y;
    const uint64_t seed = (uint64_t)seeds[b];
    const int64_t ng = (npix + 3) / 4;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
        float z[4];
        keyed_normal4(seed, (uint32_t)t, (uint32_t)g, z);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (4 * g + e < npix) out[(int64_t)b * npix + 4 * g + e] = z[e];
    }
}

// start of an ancestral step: t <- t - 1, time[b] <- times[t] (the UNet's time input alphas_cumsum[t] * T)
__global__ void ancestral_begin_kernel(int *t_dev, const float *__restrict__ times, float *__restrict__ time_buf, int B) {
    const int t = max(*t_dev - 1, 0);          // a caller that runs more steps than the table has rows repeats t = 0
    __syncthreads();
    if (threadIdx.x == 0) *t_dev = t;
    for (int b = threadIdx.x; b < B; b += blockDim.x) time_buf[b] = times[t];
}

// xt / out may be the same buffer (in-place update): no __restrict__ on them; a thread reads its pixels before it
// writes them
__global__ void res_posterior_keyed_kernel(const float *__restrict__ mo, const float *xt, const float *__restrict__ xin,
                                           const float *__restrict__ coef_table, const int *__restrict__ t_dev,
                                           const int64_t *__restrict__ seeds, float *out, float *__restrict__ xs_out,
                                           int64_t npix) {
    const int b = blockIdx.y;
    const int t = max(*t_dev, 0);
    const float c1 = coef_table[t * 4], c2 = coef_table[t * 4 + 1], c3 = coef_table[t * 4 + 2];
    const float sd = t > 0 ? expf(0.5f * coef_table[t * 4 + 3]) : 0.f;       // no noise at t = 0 (src/DADiff.py:1228)
    const uint64_t seed = (uint64_t)seeds[b];
    const int64_t ng = (npix + 3) / 4;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) keyed_normal4(seed, (uint32_t)t, (uint32_t)g, z);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = 4 * g + e;
            if (i < npix) {
                const int64_t j = (int64_t)b * npix + i;
                const float pr = clamp1s(mo[j]);
                const float xs = clamp1s(xin[j] - pr);
                out[j] = c1 * xt[j] + c2 * pr + c3 * xs + sd * z[e];
                if (xs_out) xs_out[j] = xs;
            }
        }
    }
}

// The objective-general twins (src/DADiff.py:1168-1207 + 1142-1151, 1226-1229): every objective of model_predictions and the
// two-U-Net model, one or two U-Net time inputs per step, the eight step parameters from ONE device table row.

// start of a step: t <- max(t - 1, 0) (held below T), time0[b] <- times0[t], time1[b] <- times1[t]; a NULL output is not written
__global__ void obj_begin_kernel(int *t_dev, const float *__restrict__ times0, const float *__restrict__ times1,
                                 float *__restrict__ time0, float *__restrict__ time1, int B, int T) {
    const int t = min(max(*t_dev - 1, 0), T - 1);
    __syncthreads();
    if (threadIdx.x == 0) *t_dev = t;
    if (time0) {
        const float v = times0[t];
        for (int b = threadIdx.x; b < B; b += blockDim.x) time0[b] = v;
    }
    if (time1) {
        const float v = times1[t];
        for (int b = threadIdx.x; b < B; b += blockDim.x) time1[b] = v;
    }
}

// one pixel: obj_pixel<MODE> of fd_obj_pixel.h, the predictions of res_step_obj_kernel's `mode`, then its step == 2 update; the
// 16-byte and the one-pixel form of the kernel round alike, so a slice's bits do not depend on the alignment of its buffers.
//
// xt / out may be the same buffer: no __restrict__ on them; a thread reads its four pixels before it writes them.  A mode reads
// only the streams its formulas name (modes 0, 3: no o1 -- the update takes no predicted noise --, mode 1: no o0, mode 2: no
// x_in).  VEC: npix % 4 == 0 and every pointer 16-byte aligned -- one 16-byte access per stream and group; otherwise the same
// pixels per lane, one at a time, ragged last group.
template <int MODE, bool VEC>
__global__ void res_step_obj_keyed_kernel(const float *__restrict__ o0, const float *__restrict__ o1, const float *xt,
                                          const float *__restrict__ xin, const float *__restrict__ par_table,
                                          const int *__restrict__ t_dev, const int64_t *__restrict__ seeds, float *out,
                                          int64_t npix, int T) {
    constexpr bool R0 = MODE != 1, R1 = MODE == 1 || MODE == 2, RI = MODE != 2;
    const int b = blockIdx.y;
    const int t = min(max(*t_dev, 0), T - 1);
    const float *p = par_table + (int64_t)t * 8;
    obj_row r;
    r.a = p[0]; r.bb = p[1]; r.oma = p[2]; r.c1 = p[3]; r.c2 = p[4]; r.c3 = p[5];
    r.sd = t > 0 ? expf(0.5f * p[6]) : 0.f;                                  // no noise at t = 0 (src/DADiff.py:1228)
    const uint64_t seed = (uint64_t)seeds[b];
    const int64_t ng = (npix + 3) / 4, base = (int64_t)b * npix;
    for (int64_t g = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; g < ng; g += (int64_t)gridDim.x * blockDim.x) {
        float z[4] = {0.f, 0.f, 0.f, 0.f};
        if (t > 0) keyed_normal4(seed, (uint32_t)t, (uint32_t)g, z);
        const int64_t j = base + 4 * g;
        if (VEC) {
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 v0 = R0 ? *reinterpret_cast<const float4 *>(o0 + j) : zero;
            const float4 v1 = R1 ? *reinterpret_cast<const float4 *>(o1 + j) : zero;
            const float4 vx = *reinterpret_cast<const float4 *>(xt + j);
            const float4 vi = RI ? *reinterpret_cast<const float4 *>(xin + j) : zero;
            float4 w;
            w.x = obj_pixel<MODE>(r, v0.x, v1.x, vx.x, vi.x, z[0]);
            w.y = obj_pixel<MODE>(r, v0.y, v1.y, vx.y, vi.y, z[1]);
            w.z = obj_pixel<MODE>(r, v0.z, v1.z, vx.z, vi.z, z[2]);
            w.w = obj_pixel<MODE>(r, v0.w, v1.w, vx.w, vi.w, z[3]);
            *reinterpret_cast<float4 *>(out + j) = w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * g + e < npix)
                    out[j + e] = obj_pixel<MODE>(r, R0 ? o0[j + e] : 0.f, R1 ? o1[j + e] : 0.f, xt[j + e], RI ? xin[j + e] : 0.f, z[e]);
        }
    }
}

inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

inline int g4(int64_t npix) { int64_t b = ((npix + 3) / 4 + 255) / 256; return (int)(b > 2048 ? 2048 : (b < 1 ? 1 : b)); }

}  // namespace

extern "C" int fd_keyed_normal(const int64_t *seeds, int t, float *out, int B, int64_t npix, void *stream) {
    FD_REQUIRE(seeds && out && B > 0 && npix > 0 && npix < (1ll << 33), "fd_keyed_normal: bad args");
    hipLaunchKernelGGL(keyed_normal_kernel, dim3(g4(npix), B), dim3(256), 0, (hipStream_t)stream, seeds, t, out, npix);
    FD_LAUNCH_OK("fd_keyed_normal");
    return FD_OK;
}

extern "C" int fd_ancestral_begin(int *t_dev, const float *times, float *time_buf, int B, void *stream) {
    FD_REQUIRE(t_dev && times && time_buf && B > 0, "fd_ancestral_begin: bad args");
    hipLaunchKernelGGL(ancestral_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t_dev, times, time_buf, B);
    FD_LAUNCH_OK("fd_ancestral_begin");
    return FD_OK;
}

extern "C" int fd_res_posterior_step_keyed(const float *model_out, const float *x_t, const float *x_in,
                                           const float *coef_table, const int *t_dev, const int64_t *seeds,
                                           float *img_out, float *x_start_out, int B, int64_t npix, void *stream) {
    FD_REQUIRE(model_out && x_t && x_in && coef_table && t_dev && seeds && img_out, "fd_res_posterior_step_keyed: null pointer");
    FD_REQUIRE(npix < (1ll << 33), "fd_res_posterior_step_keyed: image too large for the 32-bit pixel-group counter");
    hipLaunchKernelGGL(res_posterior_keyed_kernel, dim3(g4(npix), B), dim3(256), 0, (hipStream_t)stream, model_out, x_t,
                       x_in, coef_table, t_dev, seeds, img_out, x_start_out, npix);
    FD_LAUNCH_OK("fd_res_posterior_step_keyed");
    return FD_OK;
}

extern "C" int fd_obj_begin(int *t_dev, const float *times0, const float *times1, float *time0, float *time1, int B, int T,
                            void *stream) {
    FD_REQUIRE(t_dev && B > 0 && T > 0, "fd_obj_begin: bad args");
    FD_REQUIRE((!time0 || times0) && (!time1 || times1), "fd_obj_begin: a time output without its table");
    hipLaunchKernelGGL(obj_begin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t_dev, times0, times1, time0, time1, B, T);
    FD_LAUNCH_OK("fd_obj_begin");
    return FD_OK;
}

namespace {
template <int MODE>
void launch_obj_keyed(const float *o0, const float *o1, const float *x_t, const float *x_in, const float *par_table,
                      const int *t_dev, const int64_t *seeds, float *img_out, int B, int64_t npix, int T, hipStream_t s) {
    const bool vec = npix % 4 == 0 && al16(x_t) && al16(img_out) && (MODE == 1 || al16(o0)) && ((MODE != 1 && MODE != 2) || al16(o1)) &&
                     (MODE == 2 || al16(x_in));
    if (vec)
        hipLaunchKernelGGL((res_step_obj_keyed_kernel<MODE, true>), dim3(g4(npix), B), dim3(256), 0, s, o0, o1, x_t, x_in,
                           par_table, t_dev, seeds, img_out, npix, T);
    else
        hipLaunchKernelGGL((res_step_obj_keyed_kernel<MODE, false>), dim3(g4(npix), B), dim3(256), 0, s, o0, o1, x_t, x_in,
                           par_table, t_dev, seeds, img_out, npix, T);
}
}  // namespace

extern "C" int fd_res_step_obj_keyed(int mode, const float *o0, const float *o1, const float *x_t, const float *x_in,
                                     const float *par_table, const int *t_dev, const int64_t *seeds, float *img_out, int B,
                                     int64_t npix, int T, void *stream) {
    FD_REQUIRE(mode >= 0 && mode <= 3, "fd_res_step_obj_keyed: bad mode %d", mode);
    FD_REQUIRE(x_t && par_table && t_dev && seeds && img_out, "fd_res_step_obj_keyed: null pointer");
    FD_REQUIRE((mode == 1 || o0) && ((mode != 1 && mode != 2) || o1) && (mode == 2 || x_in), "fd_res_step_obj_keyed: mode %d needs o0=%p o1=%p x_in=%p",
               mode, (const void *)o0, (const void *)o1, (const void *)x_in);
    FD_REQUIRE(B > 0 && B <= 65535 && T > 0 && npix > 0, "fd_res_step_obj_keyed: bad sizes B=%d T=%d", B, T);
    FD_REQUIRE(npix < (1ll << 33), "fd_res_step_obj_keyed: image too large for the 32-bit pixel-group counter");
    hipStream_t s = (hipStream_t)stream;
    if (mode == 0) launch_obj_keyed<0>(o0, o1, x_t, x_in, par_table, t_dev, seeds, img_out, B, npix, T, s);
    else if (mode == 1) launch_obj_keyed<1>(o0, o1, x_t, x_in, par_table, t_dev, seeds, img_out, B, npix, T, s);
    else if (mode == 2) launch_obj_keyed<2>(o0, o1, x_t, x_in, par_table, t_dev, seeds, img_out, B, npix, T, s);
    else launch_obj_keyed<3>(o0, o1, x_t, x_in, par_table, t_dev, seeds, img_out, B, npix, T, s);
    FD_LAUNCH_OK("fd_res_step_obj_keyed");
    return FD_OK;
}
